"""The closed forms of tests/ntt_cases.py, pinned on the CPU before a GPU sees them: every family with every constant equals a direct
O(N^2) sum in Python integers where that is affordable, and the oracle's best_fft (the C restatement of the reference algorithm) at every
size of the list."""
import numpy as np
import pytest

import ntt_cases as NC


def test_constants_are_the_words_the_issue_names():
    c, r = NC.CONSTANTS, NC.R
    inv = pow(1 << 256, -1, r)
    assert [c[k] * inv % r for k in ("enc0", "enc1", "enc_r_minus_1")] == [0, 1, r - 1]
    assert c["raw_r_minus_1"] == r - 1 and c["raw1"] == 1
    top = c["raw_low_limbs_full"]
    assert top < r and top + 1 == (r >> 232) << 232
    assert [(top >> (29 * i)) & (2**29 - 1) for i in range(8)] == [2**29 - 1] * 8
    assert len(set(c.values())) == 7 and 1 < c["seeded"] < r - 1
    assert list(NC.SIZES) == [0, 1, 2, 3, 4, 5, 9, 10, 11, 18, 19]


def test_case_lists_hold_every_family_member():
    for L in NC.SIZES:
        N = 1 << L
        cs = NC.cases(L)
        assert len(set(cs)) == len(cs) and len({NC.case_id(c) for c in cs}) == len(cs)
        fam = {f: [c for c in cs if c.family == f] for f in ("zero", "constant", "alternating", "half", "geometric", "delta")}
        assert len(fam["zero"]) == 1 and len(fam["constant"]) == 7
        assert len(fam["alternating"]) == len(fam["half"]) == (7 if L >= 1 else 0)
        ks, js = {c.param for c in fam["geometric"]}, {c.param for c in fam["delta"]}
        assert ks == {k for k in [1, N - 1] + ([1023, 1024] if N > 1024 else []) if k < N}
        assert js == {j for j in [0, 1, N // 2, N - 1] if j < N}
        assert len(fam["geometric"]) == 7 * len(ks) and len(fam["delta"]) == 7 * len(js)


@pytest.mark.parametrize("L", NC.DFT_SIZES)
def test_closed_forms_equal_the_direct_sum(L):
    N, w = 1 << L, NC.omega(L)
    pw = [pow(w, i, NC.R) for i in range(N)]
    for c in NC.cases(L):
        a, e = NC.vector(L, c)
        ai = NC.ints(a)
        assert all(x < NC.R for x in ai), NC.case_id(c)                     # canonical words only: the ABI's input format
        direct = [sum(ai[j] * pw[i * j % N] for j in range(N)) % NC.R for i in range(N)]
        assert NC.ints(e) == direct, NC.case_id(c)
        if c.family in ("zero", "constant", "alternating", "half", "geometric"):
            assert sum(1 for x in direct if x) <= 1, NC.case_id(c)          # N - 1 (or N) exact zeros
        if c.family == "half" and c.mname != "enc0":
            assert ai[1] == NC.R - ai[0]


@pytest.mark.parametrize("L", list(NC.SIZES))
def test_closed_forms_equal_best_fft(cref, L):
    cs = NC.cases(L)
    om = NC.word(NC.enc(NC.omega(L)))

    def mismatch(i):                                                        # vectors made on demand: 78 pairs of 2^19 words would be 2.6 GB
        a, e = NC.vector(L, cs[i])
        cref.best_fft(a, om, L, 1)
        return None if np.array_equal(a, e) else NC.case_id(cs[i])

    assert [b for b in NC.for_each(mismatch, len(cs), L) if b] == []
