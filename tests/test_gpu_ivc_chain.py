"""GPU: the reference's IVC chain in miniature, without the in-circuit verifier.  One key with one instance column of 13 values -- the 12 limbs
of the accumulator a proof carries, and the round.  Round 0 carries the default accumulator; round t carries
accumulate(succinct_verify(proof_(t-1), accumulator_indices=[(0, 0)])): the new accumulator of the last proof folded with the one it carried.
The final check is verify_transcript_proofs(..., accumulator_indices=[(0, 0)]): the last proof's identity and openings, and the decider on the
accumulator it carries -- which, by the chain, vouches for every earlier round's openings."""
import random

import numpy as np
import pytest
import torch

import zksnap_circuits_halo2_amd as Z
from zksnap_circuits_halo2_amd import accumulator as A, fields as F, keygen as KG, prover as P, verifier as V

pytestmark = pytest.mark.gpu
K, GATE_COLS, LOOKUPS = 7, 3, 2
INDICES = [(0, 0)]


def limbs_of(acc):
    """the 12 integers an accumulator (2, 8) is carried as"""
    return F.fr_decode(A.to_limbs(acc.contiguous()).cpu().numpy().view(np.uint64).reshape(12, 4))


class Chain:
    def __init__(self, multiopen="gwc"):
        self.multiopen = multiopen
        self.params = Z.ParamsKZG.setup(K, P.SeededChallenges(1).s)
        self.dpk, self.proofs, self.public = None, [], []
        self.shape = None

    def prove(self, public, seed):
        torch.manual_seed(1)
        blinding = P.DeviceBlinding(random.Random(seed).randbytes(32))
        w = P.halo2_lib_witness(K, GATE_COLS, LOOKUPS, blinding, instances=1, instance_len=13, public_inputs=[public])
        if self.dpk is None:
            self.dpk = KG.keygen_device(self.params, w.cs, [f.cpu().numpy().view(np.uint64).reshape(-1, 4) for f in w.fixed], w.assembly)
            self.shape = {"advice": GATE_COLS + LOOKUPS, "lookups": LOOKUPS, "permutation_sets": self.dpk.vk.cs.num_permutation_sets, "random_poly": True}
        pv = P.create_proof(self.params, self.dpk, w, P.TranscriptChallenges(self.dpk.vk, "poseidon"), blinding, lap=None, multiopen=self.multiopen)
        self.plan = pv.plan
        return pv.proof, [list(col) for col in w.instance_values]

    def verify(self, proofs, public, **kw):
        return V.verify_transcript_proofs(self.params, self.dpk.vk, K, proofs, self.shape, self.plan, "poseidon", self.multiopen, instances=public, **kw)

    def succinct(self, proof, public):
        return A.succinct_verify_proofs(self.params, self.dpk.vk, K, [proof], self.shape, self.plan, "poseidon", self.multiopen, instances=[public], accumulator_indices=INDICES)

    def close(self):
        if self.dpk is not None:
            self.dpk.free()
        self.params.close()


@pytest.fixture(scope="module", params=["gwc", "shplonk"])
def chain(request):
    c = Chain(request.param)
    carried = A.default_accumulator(c.params)
    for t in range(3):
        proof, public = c.prove(limbs_of(carried) + [t], seed=t + 1)
        c.proofs.append(proof)
        c.public.append(public)
        got = c.succinct(proof, public)
        assert got.status.tolist() == [0] and torch.equal(got.accumulators[0, 1], carried)      # the carried accumulator comes back from the public inputs
        carried, as_proof, _ = A.accumulate(got.accumulators[0].contiguous())                     # new, then old
        assert as_proof == b""
    c.next = carried
    yield c
    c.close()


def test_the_chain_is_accepted(chain):
    assert chain.verify(chain.proofs[-1:], chain.public[-1:], accumulator_indices=INDICES) == [True]
    assert chain.verify(chain.proofs, chain.public, accumulator_indices=INDICES) == [True] * 3
    assert chain.verify(chain.proofs, chain.public, accumulator_indices=INDICES, fold=True) == [True] * 3
    assert chain.verify(chain.proofs, chain.public) == [True] * 3
    assert A.decide(chain.params, chain.next) is True                                            # what round 3 would carry
    assert chain.public[2][0][:12] != chain.public[1][0][:12] != chain.public[0][0][:12] and [p[0][12] for p in chain.public] == [0, 1, 2]


def test_a_proof_that_carries_a_false_accumulator_is_refused_only_with_the_indices(chain):
    g = torch.from_numpy(np.stack([np.asarray(chain.params.g[0], dtype=np.uint64).reshape(8)] * 2).view(np.int64)).to(V.DEV)      # (G, G): e(G, g2) != e(G, [s]g2)
    assert A.decide(chain.params, g) is False
    proof, public = chain.prove(limbs_of(g) + [7], seed=11)
    assert chain.verify([proof], [public]) == [True]                                             # nothing reads the carried accumulator
    assert chain.verify([proof], [public], fold=True) == [True]
    assert chain.verify([proof], [public], accumulator_indices=INDICES) == [False]
    assert chain.verify([proof], [public], accumulator_indices=INDICES, fold=True) == [False]
    got = chain.succinct(proof, public)
    assert got.status.tolist() == [0] and torch.equal(got.accumulators[0, 1], g)                 # well formed: deciding it is the decider's part
    assert A.decide(chain.params, got.accumulators[0, 0].contiguous()) is True
    # among honest proofs it is refused alone
    proofs, publics = [chain.proofs[0], proof, chain.proofs[2]], [chain.public[0], public, chain.public[2]]
    assert chain.verify(proofs, publics, accumulator_indices=INDICES) == [True, False, True]
    assert chain.verify(proofs, publics, accumulator_indices=INDICES, fold=True) == [True, False, True]


def test_a_proof_that_carries_a_limb_of_2_to_the_88_is_refused_only_with_the_indices(chain):
    limbs = limbs_of(A.default_accumulator(chain.params))
    limbs[4] = 1 << 88
    proof, public = chain.prove(limbs + [9], seed=12)
    assert chain.verify([proof], [public]) == [True] == chain.verify([proof], [public], fold=True)
    assert chain.verify([proof], [public], accumulator_indices=INDICES) == [False]
    assert chain.verify([proof], [public], accumulator_indices=INDICES, fold=True) == [False]
    got = chain.succinct(proof, public)
    assert got.status.tolist() == [3] and not got.accumulators[0, 1].any()
    assert A.decide(chain.params, got.accumulators[0, 0].contiguous()) is True
    with pytest.raises(ValueError, match="accumulator_indices"):
        chain.verify([proof], [public], accumulator_indices=[(0, 2)])                            # no 12 values from 2 in a column of 13
