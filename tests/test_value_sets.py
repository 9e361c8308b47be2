"""The condition that keeps tests/test_gpu_value_codes.py honest: every value array it uploads holds EXACTLY the number of
distinct bit patterns its case claims -- matrix-wide, per 64-row slice, per 3 x 3 block, of 1 / diagonal -- counted here with
np.unique on the uint64 view, independently of the generator's own checks; the solve cases are symmetric and strictly diagonally
dominant.  Patterns and assembled values come from the oracle (zo.pattern, zo.assemble_matrix) on the same zzz.Part.  No GPU."""
import numpy as np
import pytest

import zzz_oracle as zo
import _value_sets as vs


@pytest.fixture(scope="module", autouse=True)
def _threads():
    zo.set_num_threads(4)


def _blocks_of(v, rp, cl):
    """the matrix's 3 x 3 blocks as rows of nine patterns, straight from the CSR arrays (not through Gen.block_positions)"""
    b = vs.bits(v)
    out = []
    for a in range(3):
        seg = [b[rp[r]:rp[r + 1]].reshape(-1, 3) for r in range(a, rp.size - 1, 3)]
        out.append(np.concatenate(seg))
    return np.concatenate(out, axis=1)  # [block][3 a + b]


@pytest.mark.parametrize("name", sorted(vs.CASES))
def test_case_holds_what_it_claims(name):
    pname, _, claim = vs.CASES[name]
    P, rp, cl, base, g = vs.problem(pname)
    v = vs.values(name)
    assert v.dtype == np.float64 and v.shape == (cl.size,)
    pats = vs.nonzero_patterns(v)
    if "matrix" in claim:
        assert pats.size == (cl.size if claim["matrix"] == "nnz" else claim["matrix"])
    if "slices" in claim:
        got = [vs.nonzero_patterns(v[rp[s]:rp[min(s + 64, rp.size - 1)]]).size for s in range(0, rp.size - 1, 64)]
        assert got == list(claim["slices"])
        assert pats.size == sum(got) > 2046  # (pairwise disjoint; the matrix-wide dictionary steps aside)
    if "slice_max" in claim:
        assert pats.size > 2046 and max(vs.slice_counts(v, rp)) <= claim["slice_max"]
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    dg = v[rows == cl]
    assert dg.size == rp.size - 1
    if "dinv" in claim:
        assert np.unique(vs.bits(1.0 / dg)).size == claim["dinv"]
    if "diag_pattern" in claim:
        assert (vs.bits(dg) == np.uint64(claim["diag_pattern"])).sum() == 1
        with np.errstate(all="ignore"):
            assert np.unique(vs.bits(1.0 / np.where(dg == 0.0, 1.0, dg))).size <= 2048
    if "blocks" in claim:
        blk = _blocks_of(v, rp, cl)
        zero = ((blk << np.uint64(1)) == 0).all(axis=1)
        kept = np.unique(blk[~zero], axis=0)
        u = np.unique(kept)
        assert (kept.shape[0], int(u[u != 0].size)) == claim["blocks"]
        # the special relatives: one entry apart, a permutation of another, +0.0 against -0.0 in one entry; whole blocks of +-0.0
        have = set(map(bytes, kept))
        signed = one_apart = False
        for row in kept[(kept == vs.NEG_ZERO).any(axis=1)]:
            for i in np.nonzero(row == vs.NEG_ZERO)[0]:
                t = row.copy()
                t[i] = 0
                signed |= bytes(t) in have
        srt = np.sort(kept, axis=1)
        assert np.unique(srt, axis=0).shape[0] < kept.shape[0]  # two blocks with the same nine values in another order
        for i in range(9):
            rest = np.delete(kept, i, axis=1)
            one_apart |= np.unique(rest, axis=0).shape[0] < kept.shape[0]
        assert signed and one_apart
        if not claim.get("spd"):
            assert (blk[zero] == 0).all(axis=1).any() and (blk[zero] == vs.NEG_ZERO).all(axis=1).any()
    if claim.get("spd"):
        assert vs.is_symmetric_dominant(rp, cl, v)
    if "hostile" in claim:
        lvl = claim["hostile"]
        want = vs.hostile_patterns(lvl >= 1, lvl >= 2)
        assert np.isin(want, pats).all()
        assert (vs.ALL_ONES in pats) == (lvl >= 2) and (vs.QUIET_NAN in pats) == (lvl >= 1)
        assert any((vs.bits(v[rp[r]:rp[r + 1]]) == vs.NEG_ZERO).all() for r in range(rp.size - 1))
        if P.bs == 3:
            blk = _blocks_of(v, rp, cl)
            assert (blk == vs.NEG_ZERO).all(axis=1).any()
        if claim.get("every_slice"):
            assert all((vs.bits(v[rp[s]:rp[min(s + 64, rp.size - 1)]]) == vs.ALL_ONES).any() for s in range(0, rp.size - 1, 64))
    if "hostile" in claim or "clustered" in claim:
        # capacity is not what these cases are about: the counts stay inside every set they meet
        if pname == "p3_555":
            assert pats.size <= 8191 and max(vs.slice_counts(v, rp)) <= 1023
        elif pname == "el_20":
            nb, nv = vs.block_counts(v, g.block_positions()[0])
            assert nv <= 2046 and (2200 <= nb <= 65535 if name.endswith("form2") or "clustered" in claim else nb <= 2199)
        else:
            assert pats.size <= 2046
    if "clustered" in claim:
        assert np.isfinite(v).all()


def test_clustered_values_are_distinct_finite_and_at_the_table_end():
    rng = np.random.default_rng(3)
    for nbits in (18, 14, 13, 11):
        c = vs.clustered(nbits, 300, rng)
        assert c.size == 300 and np.isfinite(c).all() and np.unique(vs.bits(c)).size == 300


def test_generators_refuse_what_they_cannot_deliver():
    _, rp, cl, base, g = vs.problem("p1_17")
    with pytest.raises(AssertionError):
        g.matrix_wide(cl.size + 1)  # more patterns than entries
    with pytest.raises(AssertionError):
        g.per_slice([1] * 3)  # not one count per slice
