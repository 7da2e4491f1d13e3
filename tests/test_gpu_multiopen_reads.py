"""GPU (-m gpu; a transcript decodes and normalises its points on the device): each multi-open's verifier class reads its own part of a proof.
The part is written with a Blake2bWrite, with the squeezes between the writes as the prover makes them (GWC: three small multiples of the
generator; SHPLONK: two), and read back twice: through `read_proof` with host points, and through the sequence spelled out here.  Points and
challenges agree, SHPLONK's come back as [H', H], `read_proof` with device points returns the same limbs, and with the bytes cut in the middle
of the last point transcript.decoded reports a part that does not decode and leaves the reader where the failing read left it."""
import numpy as np
import pytest

from oracle import bn254 as O
from zksnap_circuits_halo2_amd import _lib, fields as F, multiopen as MO
from zksnap_circuits_halo2_amd.transcript import Blake2bRead, Blake2bWrite, decoded

pytestmark = pytest.mark.gpu


def write_part(scheme, xyz):
    with Blake2bWrite() as w:
        w.common_scalar(7)
        if scheme == "gwc":
            challenges = [w.squeeze_challenge()]
            w.write_points(np.stack(xyz))
            challenges.append(w.squeeze_challenge())
        else:
            challenges = [w.squeeze_challenge(), w.squeeze_challenge()]
            w.write_points(xyz[0].reshape(1, 12))
            challenges.append(w.squeeze_challenge())
            w.write_points(xyz[1].reshape(1, 12))
        return w.finalize(), tuple(challenges)


def read_part_by_hand(scheme, r):
    if scheme == "gwc":
        v = r.squeeze_challenge()
        W = r.read_points(3, device=False)
        return list(W), (v, r.squeeze_challenge())
    y, v = r.squeeze_challenge(), r.squeeze_challenge()
    H = r.read_points(1, device=False)[0]
    u = r.squeeze_challenge()
    return [r.read_points(1, device=False)[0], H], (y, v, u)


@pytest.mark.parametrize("scheme, multiples", [("gwc", (2, 3, 5)), ("shplonk", (2, 3))])
def test_a_verifier_class_reads_its_part_of_a_proof_in_its_provers_order(scheme, multiples):
    written = [F.g1_encode([O.scalar_mul(m, O.G1_GEN)])[0] for m in multiples]
    proof, written_challenges = write_part(scheme, [MO._affine_to_xyz(p) for p in written])
    assert len(proof) == 32 * len(multiples)
    verifier = MO.multiopen_classes(scheme)[1](None)
    limbs = lambda points: [np.asarray(p.cpu() if hasattr(p, "cpu") else p).view(np.uint64).tolist() for p in points]
    with Blake2bRead(proof) as r, Blake2bRead(proof) as twin, Blake2bRead(proof) as on_device:
        for t in (r, twin, on_device):
            t.common_scalar(7)
        points, challenges = verifier.read_proof(r, len(multiples))
        want_points, want_challenges = read_part_by_hand(scheme, twin)
        assert challenges == want_challenges == written_challenges and len(set(challenges)) == (2 if scheme == "gwc" else 3)
        assert limbs(points) == limbs(want_points) == limbs(written if scheme == "gwc" else written[::-1])        # SHPLONK: [H', H]
        d_points, d_challenges = verifier.read_proof(on_device, len(multiples), device=True)
        assert all(p.is_cuda for p in d_points) and limbs(d_points) == limbs(points) and d_challenges == challenges
        assert r.squeeze_challenge() == twin.squeeze_challenge() == on_device.squeeze_challenge()                # all stand behind the part
    with Blake2bRead(proof[:-16]) as r, Blake2bRead(proof[:-16]) as twin:           # cut in the middle of the last point
        r.common_scalar(7), twin.common_scalar(7)
        assert decoded(verifier.read_proof, r, len(multiples)) is None              # "does not decode"
        with pytest.raises(_lib.ZkhipError) as refused:
            read_part_by_hand(scheme, twin)
        assert refused.value.code == -1
        assert r.squeeze_challenge() == twin.squeeze_challenge()                    # left where the failing read left it
