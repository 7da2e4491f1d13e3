"""GPU (-m gpu): secp256k1 points packed and hashed on the device (csrc/poseidon.hip, k_poseidon_hash_points) against the host packers
(`poseidon.compress_nullifier`, `poseidon.pack_member`) and the library's host hash.  The kernel puts one lane on a point, 128 to a workgroup:
the counts are 0, 1, 127, 128 and 129.  The coordinates are not curve points -- the packers take any 256 bits: 0, 2^256 - 1 and the single bits
87, 88, 175, 176 and 255 either side of the chunk seams (bytes 11 and 22), with odd and even y, then seeded 256-bit values.  The host hashes are
computed once and shared."""
import functools

import pytest
import torch

import plume_cases as PC
from zksnap_circuits_halo2_amd import plume as PL, poseidon
from zksnap_circuits_halo2_amd.tensors import fr_ints as _ints

pytestmark = pytest.mark.gpu

BLOCK = 128                                                    # PH_BLOCK of csrc/poseidon.hip
SEAMS = [0, PC.FULL] + [1 << b for b in (87, 88, 175, 176, 255)] + [(1 << 88) - 1, (1 << 176) - 1, PC.FULL ^ (1 << 88), 1, 0xFF << 80, 0xFFFF << 168]
PACKERS = {poseidon.LAYOUT_NULLIFIER: poseidon.compress_nullifier, poseidon.LAYOUT_MEMBER: poseidon.pack_member}


@functools.lru_cache(maxsize=None)
def points():
    """BLOCK + 1 points: every seam value as x beside an even and an odd y, every seam value as y, then seeded values"""
    rng = PC.rng("poseidon-points")
    pts = [(x, y) for x in SEAMS for y in (2, 3)] + [(rng.getrandbits(256), y) for y in SEAMS] + [(PC.FULL, PC.FULL), (0, 0), (0, 1)]
    pts += [(rng.getrandbits(256), rng.getrandbits(256)) for _ in range(BLOCK + 1 - len(pts))]
    assert len(pts) == BLOCK + 1 and {p[1] & 1 for p in pts} == {0, 1}
    return tuple(pts)


@functools.lru_cache(maxsize=None)
def host_hashes(layout):
    return tuple(poseidon.hash(PACKERS[layout](p)) for p in points())


def test_the_packers_cut_at_bytes_11_and_22():
    x = sum(b << (8 * i) for i, b in enumerate(range(1, 33)))
    assert poseidon.pack_member((x, 0))[:3] == [x & ((1 << 88) - 1), (x >> 88) & ((1 << 88) - 1), x >> 176]
    assert poseidon.compress_nullifier((x, 5)) == [3] + poseidon.pack_member((x, 0))[:3]


@pytest.mark.parametrize("layout", sorted(PACKERS))
@pytest.mark.parametrize("count", [0, 1, BLOCK - 1, BLOCK, BLOCK + 1])
def test_the_device_packs_and_hashes_what_the_host_packers_build(lib, layout, count):
    pts = list(points()[:count])
    out = poseidon.hash_points_device(PL.encode_points(pts), layout)
    assert tuple(out.shape) == (count, 4) and out.dtype == torch.int64
    assert _ints(out) == list(host_hashes(layout)[:count])


@pytest.mark.parametrize("layout", sorted(PACKERS))
def test_the_last_points_of_a_batch_are_the_seams_too(lib, layout):
    """the same points in reverse: the seam values sit in the second workgroup's only lane and the first one's last lanes"""
    pts = list(reversed(points()))
    assert _ints(poseidon.hash_points_device(PL.encode_points(pts), layout)) == list(reversed(host_hashes(layout)))


def test_the_pairs_path_and_the_tensor_path_agree(lib):
    pts = list(points()[:BLOCK + 1])
    dev = PL.encode_points(pts)
    leaves_pairs, leaves_tensor = poseidon.member_leaves(pts), poseidon.member_leaves(dev)
    assert torch.equal(leaves_pairs, leaves_tensor) and _ints(leaves_tensor) == list(host_hashes(poseidon.LAYOUT_MEMBER))
    values_pairs, values_tensor = poseidon.nullifier_values(pts), poseidon.nullifier_values(dev)
    assert torch.equal(values_pairs, values_tensor) and _ints(values_tensor) == list(host_hashes(poseidon.LAYOUT_NULLIFIER))


def test_the_tensor_path_equals_hash_many_over_the_host_packed_message(lib):
    import numpy as np

    from zksnap_circuits_halo2_amd.fields import fr_encode

    pts = list(points()[:33])
    for layout, width in ((poseidon.LAYOUT_NULLIFIER, 4), (poseidon.LAYOUT_MEMBER, 6)):
        packed = fr_encode([v for p in pts for v in PACKERS[layout](p)]).reshape(len(pts), width, 4)
        want = poseidon.hash_many_device(torch.from_numpy(packed.view(np.int64)).cuda())
        assert torch.equal(poseidon.hash_points_device(PL.encode_points(pts), layout), want)


def test_wrong_tensors_and_layouts_are_refused(lib):
    from zksnap_circuits_halo2_amd._lib import ZkhipError

    dev = PL.encode_points(list(points()[:2]))
    with pytest.raises(ValueError):
        poseidon.hash_points_device(dev.cpu(), 0)
    with pytest.raises(ValueError):
        poseidon.hash_points_device(dev.reshape(4, 4), 0)
    with pytest.raises(ZkhipError):
        poseidon.hash_points_device(dev, 2)
