"""GPU (-m gpu): the PLUME kernels (csrc/plume.hip over csrc/secp256k1.hpp, sha256.hpp, secp256k1_h2c.hpp) against tests/plume_reference.py,
exactly and on every element.  The verify kernel puts two lanes on a voter and one wavefront in a workgroup: 32 voters fill both, so the counts
are 0, 1, 31, 32, 33 and 65 (a third workgroup with one voter); the other two kernels put one lane on an element, 64 to a workgroup: 63, 64,
65.  The grid has one row.  The voters are generated once (tests/plume_cases.py) and shared."""
import pytest
import torch

import plume_cases as PC
import plume_reference as R
from zksnap_circuits_halo2_amd import plume as PL, poseidon

pytestmark = pytest.mark.gpu

P, N, G = R.P, R.N, R.G
POOL = 65


def _verify(msg, voters, stream=None):
    pk, nul, s, c = ([v[i] for v in voters] for i in range(4))
    return PL.verify_many_device(msg, PL.encode_points(pk), PL.encode_points(nul), PL.encode_scalars(s), PL.encode_scalars(c), stream=stream)


def _want(msg, voters):
    return [R.verdict(msg, nul, pk, s, c) for pk, nul, s, c in voters]


def _h(msg, voters):
    return [R.hash_to_curve(msg, v[0]) if R.on_curve(v[0]) else (0, 0) for v in voters]


def _check(found, verdicts):
    assert found.status.dtype == torch.int32 and found.status.tolist() == verdicts
    bad = [i for i, v in enumerate(verdicts) if v]
    assert found.failures == len(bad) and found.first == (bad[0] if bad else None)


@pytest.mark.parametrize("count", [0, 1, 31, 32, 33, POOL])
def test_valid_voters_are_accepted_at_the_wavefront_and_workgroup_counts(lib, count):
    voters = list(PC.voters(POOL)[:count])
    found = _verify(PC.MSG, voters)
    _check(found, [0] * count)
    assert tuple(found.h.shape) == (count, 8) and PL.decode_points(found.h) == _h(PC.MSG, voters)
    assert [int(v) & (2**64 - 1) for v in found.report.cpu().tolist()] == [0, 2**64 - 1], "the report of a clean batch is (0, none)"


def test_one_wrong_voter_at_a_time_is_refused_at_its_own_index(lib):
    """N, pk, s, c wrong in turn, in the first wavefront, at its last voter, at the next wavefront's first and in the last"""
    base = list(PC.voters(POOL))
    other = PC.voters(2, tag="strangers")
    for at in (0, 31, 32, POOL - 1):
        pk, nul, s, c = base[at]
        for wrong in [(pk, other[0][1], s, c), (other[1][0], nul, s, c), (pk, nul, (s + 1) % N, c), (pk, nul, s, (c + 1) % N), (pk, R.neg(nul), s, c)]:
            voters = base[:at] + [wrong] + base[at + 1:]
            found = _verify(PC.MSG, voters)
            assert R.verdict(PC.MSG, wrong[1], wrong[0], wrong[2], wrong[3]) == 1
            _check(found, [1 if i == at else 0 for i in range(POOL)])
    # the message: every voter of the batch signed another one
    found = _verify(bytes([2, 0]), base[:33])
    _check(found, [1] * 33)
    assert PL.decode_points(found.h) == _h(bytes([2, 0]), base[:33])


def test_failures_in_the_first_and_the_last_wavefront_are_counted_and_the_lowest_is_first(lib):
    voters = list(PC.voters(POOL))
    for at in (3, 30, POOL - 1):
        pk, nul, s, c = voters[at]
        voters[at] = (pk, nul, s, (c + 5) % N)
    voters[40] = (voters[40][0], (0, 0), voters[40][2], voters[40][3])
    found = _verify(PC.MSG, voters)
    want = _want(PC.MSG, voters)
    assert [i for i, v in enumerate(want) if v] == [3, 30, 40, POOL - 1] and want[40] == 2
    _check(found, want)
    assert found.failures == 4 and found.first == 3


def test_zero_scalars_and_the_ladders_doubling_and_cancelling_cases(lib):
    """s = 0 and c = 0 are well-formed; N = H makes B = (s - c) H -- both table entries are the same point up to sign -- and pk = G does it to A;
    s = c then cancels: A or B is the identity, compressed as 02 00..00.  The verdict is whatever the reference says."""
    base = list(PC.voters(8))
    voters = []
    for k, (pk, nul, s, c) in enumerate(base):
        h = R.hash_to_curve(PC.MSG, pk)
        voters += [[(pk, nul, 0, c), (pk, nul, s, 0), (pk, nul, 0, 0), (pk, h, s, c), (pk, h, c, c), (G, nul, s, c), (G, R.hash_to_curve(PC.MSG, G), s, s),
                    (pk, R.neg(h), s, c)][k]]
    voters += [base[0], (G, R.mul(5, R.hash_to_curve(PC.MSG, G)), 7, 9)]
    found = _verify(PC.MSG, voters)
    want = _want(PC.MSG, voters)
    assert want[8] == 0 and 2 not in want
    _check(found, want)
    assert PL.decode_points(found.h) == _h(PC.MSG, voters)


def test_malformed_voters_get_verdict_2_and_leave_their_neighbours_exact(lib):
    base = list(PC.voters(POOL))
    voters = list(base)
    bad_points = PC.off_curve_points()
    at = 1
    for bad in bad_points:                                     # a bad pk, then a bad N, two voters apart
        voters[at] = (bad, *base[at][1:])
        voters[at + 2] = (base[at + 2][0], bad, *base[at + 2][2:])
        at += 4
    for k, (s, c) in enumerate([(N, None), (None, N), (PC.FULL, None), (None, PC.FULL), (N + 1, N + 1)]):
        pk, nul, s0, c0 = base[at + k]
        voters[at + k] = (pk, nul, s0 if s is None else s, c0 if c is None else c)
    assert at + 5 <= POOL
    found = _verify(PC.MSG, voters)
    want = _want(PC.MSG, voters)
    assert want.count(2) == 2 * len(bad_points) + 5 and want.count(1) == 0
    _check(found, want)
    assert PL.decode_points(found.h) == _h(PC.MSG, voters), "H is (0, 0) where pk is malformed and exact everywhere else"


def test_two_streams_with_two_messages_do_not_disturb_each_other(lib):
    a, b = list(PC.voters(POOL)), list(PC.voters(40, msg=bytes(range(34)), tag="second"))
    b[7] = (b[7][0], b[7][1], b[7][2], (b[7][3] + 1) % N)
    alone = (_verify(PC.MSG, a).status.tolist(), _verify(bytes(range(34)), b).status.tolist())
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    fa = _verify(PC.MSG, a, stream=sa.cuda_stream)
    fb = _verify(bytes(range(34)), b, stream=sb.cuda_stream)
    sa.synchronize()
    sb.synchronize()
    assert (fa.status.tolist(), fb.status.tolist()) == alone == ([0] * POOL, [1 if i == 7 else 0 for i in range(40)])
    assert (fa.failures, fa.first, fb.failures, fb.first) == (0, None, 1, 7)


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65])
def test_lincomb_edges_mixed_into_random_cases(lib, count):
    rng = PC.rng(f"gpu-lincomb-{count}")
    pts = PC.points(8, "gpu-lincomb")
    edges, bad = PC.lincomb_edges(), PC.off_curve_points()
    cases = []
    for i in range(count):
        k = rng.randrange(4)
        if k == 0:
            cases.append(edges[rng.randrange(len(edges))])
        else:
            cases.append((rng.getrandbits(256) if k == 1 else rng.randrange(N), pts[rng.randrange(8)], rng.getrandbits(256), pts[rng.randrange(8)]))
    if count >= 63:                                            # every edge once, and every malformed point on either side with exact neighbours
        cases[:len(edges)] = edges
        for j, pt in enumerate(bad):
            a, p, b, q = cases[len(edges) + 2 * j]
            cases[len(edges) + 2 * j] = (a, pt, b, q) if j % 2 else (a, p, b, pt)
        assert len(edges) + 2 * len(bad) <= 63
    out, status = PL.lincomb_device(PL.encode_scalars([c[0] for c in cases]), PL.encode_points([c[1] for c in cases]), PL.encode_scalars([c[2] for c in cases]),
                                    PL.encode_points([c[3] for c in cases]))
    ok = [R.on_curve(c[1]) and R.on_curve(c[3]) for c in cases]
    assert status.dtype == torch.int32 and status.tolist() == [0 if good else 2 for good in ok]
    assert PL.decode_points(out) == [R.lincomb(*c) if good else (0, 0) for c, good in zip(cases, ok)]
    if count >= 63:
        assert ok.count(False) == len(bad)


@pytest.mark.parametrize("length", [0, 2, 33, 34, 64])
def test_hash_to_curve_at_the_padding_switch_of_the_first_hash(lib, length):
    """the first hash of expand_message_xmd is over 150 + len bytes: 33 and 34 sit either side of SHA-256's padding switch.  The RFC's own
    messages carry no key, so its vectors cannot pass through this call; the reference stands in."""
    rng = PC.rng(f"gpu-h2c-{length}")
    msg = bytes(rng.getrandbits(8) for _ in range(length))
    keys = list(PC.points(60, "gpu-h2c")) + [G, R.neg(G), PC.small_x_point()] + PC.off_curve_points()[:2]
    for count in (len(keys), 1):
        out, status = PL.hash_to_curve_many_device(msg, PL.encode_points(keys[:count]))
        assert status.tolist() == [0 if R.on_curve(k) else 2 for k in keys[:count]]
        assert PL.decode_points(out) == [R.hash_to_curve(msg, k) if R.on_curve(k) else (0, 0) for k in keys[:count]]
    out, status = PL.hash_to_curve_many_device(msg, PL.encode_points([]))
    assert tuple(out.shape) == (0, 8) and tuple(status.shape) == (0,)


def test_member_leaves_hashes_the_six_packed_values(lib):
    keys = list(PC.points(5, "members")) + [(PC.FULL, PC.FULL), (0, 0)]
    leaves = poseidon.member_leaves(keys)
    from zksnap_circuits_halo2_amd.fields import fr_decode
    got = fr_decode(leaves.cpu().numpy().view("uint64"))
    assert got == [poseidon.hash(poseidon.pack_member(k)) for k in keys]
