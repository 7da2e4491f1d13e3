"""GPU (-m gpu): the signing kernel (csrc/plume_sign.hip) against tests/plume_reference.py, exactly and on every output.  The kernel puts two
lanes on a voter and one wavefront in a workgroup: 32 voters fill both, so the counts are 0, 1, 31, 32, 33 and 65 (a third workgroup with one
voter).  The voters are the shared ones of tests/plume_cases.py, whose (sk, r) pairs are re-drawn from its generator; the pipeline test takes
65 voters signed on the device through the verifier, the members tree and the nullifier tree."""
import functools

import numpy as np
import pytest
import torch

import plume_cases as PC
import plume_reference as R
from zksnap_circuits_halo2_amd import plume as PL, poseidon

pytestmark = pytest.mark.gpu

N = R.N
POOL = 65
EDGES = [1, 2, N - 1, 1 << 255]
BAD = [0, N, PC.FULL]
ZEROS = ((0, 0), (0, 0), 0, 0)


@functools.lru_cache(maxsize=None)
def secrets(count, msg=PC.MSG, tag="voters"):
    """the (sk, r) pairs behind PC.voters(count, msg, tag): the same draws from the same generator"""
    rng = PC.rng(f"{tag}-{msg.hex()}")
    return tuple((rng.randrange(1, N), rng.randrange(1, N)) for _ in range(count))


@functools.lru_cache(maxsize=None)
def hashes(count, msg=PC.MSG, tag="voters"):
    return tuple(R.hash_to_curve(msg, v[0]) for v in PC.voters(count, msg, tag))


def _sign(msg, pairs, stream=None):
    return PL.sign_many_device(msg, PL.encode_scalars([p[0] for p in pairs]), PL.encode_scalars([p[1] for p in pairs]), stream=stream)


def _signed(sig):
    return list(zip(PL.decode_points(sig.pk), PL.decode_points(sig.nullifier), PL.decode_scalars(sig.s), PL.decode_scalars(sig.c)))


def _well_formed(pair):
    return 1 <= pair[0] < N and 1 <= pair[1] < N


def test_the_re_drawn_secrets_are_those_of_the_shared_voters():
    sk, r = secrets(POOL)[0]
    assert R.gen(sk, PC.MSG, r) == PC.voters(POOL)[0]


@pytest.mark.parametrize("count", [0, 1, 31, 32, 33, POOL])
def test_every_output_is_exact_at_the_wavefront_and_workgroup_counts(lib, count):
    sig = _sign(PC.MSG, secrets(POOL)[:count])
    assert [tuple(t.shape) for t in (sig.pk, sig.nullifier, sig.s, sig.c, sig.status, sig.h)] == [(count, 8), (count, 8), (count, 4), (count, 4), (count,), (count, 8)]
    assert sig.status.dtype == torch.int32 and sig.status.tolist() == [0] * count
    assert _signed(sig) == list(PC.voters(POOL)[:count])
    assert PL.decode_points(sig.h) == list(hashes(POOL)[:count])
    found = PL.verify_many_device(PC.MSG, sig.pk, sig.nullifier, sig.s, sig.c)
    assert found.failures == 0 and found.first is None and found.status.tolist() == [0] * count
    assert torch.equal(found.h, sig.h)


def test_edge_scalars_mixed_into_a_batch(lib):
    base = list(secrets(POOL)[:40])
    pairs = list(base)
    at = 0
    for sk in EDGES:
        for r in EDGES:
            pairs[at] = (sk, r)
            at += 2                                            # every other voter: each edge pair between two ordinary ones, across the first wavefront's end
    assert at == 32
    pairs[33], pairs[39] = (N - 1, secrets(POOL)[33][1]), (secrets(POOL)[39][0], N - 1)
    sig = _sign(PC.MSG, pairs)
    want = [PC.voters(POOL)[i] if pairs[i] == base[i] else R.gen(pairs[i][0], PC.MSG, pairs[i][1]) for i in range(40)]
    assert sig.status.tolist() == [0] * 40 and _signed(sig) == want
    assert PL.verify_many_device(PC.MSG, sig.pk, sig.nullifier, sig.s, sig.c).failures == 0


def test_malformed_secrets_get_status_2_and_zeros_and_leave_their_neighbours_exact(lib):
    """at the first and the last voter of a wavefront and at the next wavefront's first; sk, r and both, each bad value in turn"""
    base = secrets(POOL)
    for k, bad in enumerate(BAD):
        pairs = list(base)
        places = {}
        for j, at in enumerate((0, 31, 32)):                   # the roles turn with k, so every place sees a bad sk, a bad r and both
            role = (j + k) % 3
            places[at] = pairs[at] = (bad if role != 1 else base[at][0], bad if role != 0 else base[at][1])
        assert [i for i, p in enumerate(pairs) if not _well_formed(p)] == [0, 31, 32]
        sig = _sign(PC.MSG, pairs)
        assert sig.status.tolist() == [2 if i in places else 0 for i in range(POOL)]
        assert _signed(sig) == [ZEROS if i in places else PC.voters(POOL)[i] for i in range(POOL)]
        assert PL.decode_points(sig.h) == [(0, 0) if i in places else hashes(POOL)[i] for i in range(POOL)]


@pytest.mark.parametrize("length", [0, 34, 64])
def test_message_lengths_either_side_of_the_block_counts(lib, length):
    msg = bytes(range(1, length + 1))
    sig = _sign(msg, secrets(3, msg))
    assert sig.status.tolist() == [0] * 3 and _signed(sig) == list(PC.voters(3, msg))
    assert PL.decode_points(sig.h) == list(hashes(3, msg))


def test_two_streams_with_two_messages_do_not_disturb_each_other(lib):
    other = bytes(range(34))
    a, b = secrets(POOL), secrets(33, other, "second")
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    fa = _sign(PC.MSG, a, stream=sa.cuda_stream)
    fb = _sign(other, b, stream=sb.cuda_stream)
    sa.synchronize()
    sb.synchronize()
    assert _signed(fa) == list(PC.voters(POOL)) and _signed(fb) == list(PC.voters(33, other, "second"))
    assert fa.status.tolist() == [0] * POOL and fb.status.tolist() == [0] * 33


def test_wrong_tensors_are_refused(lib):
    sk = PL.encode_scalars([1, 2])
    with pytest.raises(ValueError):
        PL.sign_many_device(PC.MSG, sk, PL.encode_scalars([1]))
    with pytest.raises(ValueError):
        PL.sign_many_device(PC.MSG, sk.cpu(), sk.cpu())
    with pytest.raises(ValueError):
        PL.sign_many_device(bytes(65), sk, sk)


def test_a_population_signed_on_the_device_goes_through_verify_and_both_trees(lib):
    """65 voters never leave HBM between the signer, the verifier and the packers; the roots are those built from the host-generated voters.
    The members tree takes a power of two of leaves: both sides pad the 65 with zero leaves to 128."""
    voters = PC.voters(POOL)
    sig = _sign(PC.MSG, secrets(POOL))
    assert PL.verify_many_device(PC.MSG, sig.pk, sig.nullifier, sig.s, sig.c).failures == 0

    def padded(leaves):
        return torch.cat([leaves, torch.zeros((128 - POOL, 4), dtype=torch.int64, device=leaves.device)])

    from_device, from_host = poseidon.member_leaves(sig.pk), poseidon.member_leaves([v[0] for v in voters])
    assert torch.equal(from_device, from_host)
    assert poseidon.MerkleTree(padded(from_device)).get_root() == poseidon.MerkleTree(padded(from_host)).get_root()

    values, host_values = poseidon.nullifier_values(sig.nullifier), poseidon.nullifier_values([v[1] for v in voters])
    assert torch.equal(values, host_values)
    roots = []
    for batch in (values, host_values):
        with poseidon.IndexedMerkleTree(8) as tree:
            tree.insert_batch(np.ascontiguousarray(batch.cpu().numpy()).view(np.uint64), witness=False)
            roots.append(tree.get_root())
            assert tree.used == POOL + 1
    assert roots[0] == roots[1]
