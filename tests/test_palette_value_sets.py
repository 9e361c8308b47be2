"""CPU proof of the value arrays of tests/_palette_sets.py: each holds exactly the per-(slice, slot) counts of distinct values
its case claims (16: packed, 17: that slice alone not, 64: nothing packed), so every edge case of
tests/test_gpu_palette_codes.py is on the side it says before a kernel sees it; and the assembled values of the small lattices
have slices of at most 16 per slot and slices of more, so "0 < packed slices < all" there is derived, not hoped for (which
slices, depends on the rounding of the oracle's assembly, i.e. on its thread count: only that both kinds exist is claimed).

The slot rule is restated here in numpy on dense [slice][lane][slot] arrays; it shares no code with the library or with
_palette_sets.slots().  Rule: exact zeros are dropped; the kept entries of a row, in column order, take slots 0, 1, ... -- unless
every row of the slice fits the column offsets of the slice's first longest row (column - lane = that row's column - its lane,
offsets >= 0 and offset + 63 < rows), then an entry takes the slot of its offset.  Holes, slots beyond the width and lanes without
a row are +0.0 and count as that value."""
import numpy as np
import pytest

import _palette_sets as ps


def _dense(rp, cl, v):
    """bits[slice][lane][slot] (uint64) of what the product multiplies, have[slice][lane][slot]"""
    n = rp.size - 1
    nsl = (n + 63) // 64
    row = np.repeat(np.arange(n), np.diff(rp))
    keep = v != 0.0  # (NaN is kept, -0.0 is not)
    kr, kc, kb = row[keep], cl[keep].astype(np.int64), v.view(np.uint64)[keep]
    first = np.searchsorted(kr, np.arange(n))  # CSR order: rows ascending, columns ascending in a row
    rank = np.arange(kr.size) - first[kr]
    cnt = np.bincount(kr, minlength=n)
    assert cnt.max() <= 8
    bits = np.zeros((nsl, 64, 8), np.uint64)
    have = np.zeros((nsl, 64, 8), bool)
    off = kc - (kr % 64)
    for s in range(nsl):
        m = kr // 64 == s
        c = cnt[64 * s:64 * s + 64]
        ref = 64 * s + int(np.argmax(c == c.max()))
        d = off[kr == ref]
        slot = rank[m]
        if d.min() >= 0 and d.max() + 63 < n and np.isin(off[m], d).all():
            slot = np.searchsorted(d, off[m])
        bits[s, kr[m] % 64, slot] = kb[m]
        have[s, kr[m] % 64, slot] = True
    return bits, have


def _counts(rp, cl, v):
    """distinct values per (slice, slot), [slices][8]"""
    bits, _ = _dense(rp, cl, v)
    return np.array([[np.unique(bits[s, :, e]).size for e in range(8)] for s in range(bits.shape[0])])


@pytest.mark.parametrize("case", sorted(ps.CASES))
def test_case_holds_the_counts_it_claims(case):
    name, _, claim = ps.CASES[case]
    _, rp, cl, base = ps.problem(name)
    v = ps.values(case)
    assert v.shape == base.shape
    assert not np.any((base == 0.0) & (v.view(np.uint64) != 0))  # (an exact zero where the assembled matrix has one: rows stay one chunk)
    cnt = _counts(rp, cl, v)
    worst = cnt.max(axis=1)
    print(case, "slices", worst.size, "largest", worst.max(), "slices over 16:", np.nonzero(worst > 16)[0].tolist())
    if "largest" in claim:
        assert worst.max() == claim["largest"]
    if "unpacked" in claim:
        assert np.nonzero(worst > 16)[0].tolist() == claim["unpacked"]
    if "at" in claim:
        s, e, c = claim["at"]
        assert cnt[s, e] == c and np.delete(cnt[s], e).max() <= 16
    if claim.get("some_packed"):
        assert (worst <= 16).sum() > 0
    if claim.get("some_unpacked"):
        assert (worst > 16).sum() > 0
    if claim.get("all_unpacked"):
        assert (worst > 16).all() and np.unique(v).size < 2047
    if claim.get("hostile"):
        bits, _ = _dense(rp, cl, v)
        for s in (ps.SLICE - 1, ps.SLICE):
            assert np.isin(ps.HOSTILE[1:], bits[s]).all() and not np.isin(ps.HOSTILE[0], bits[s])
            assert worst[s] <= 16


def test_the_counted_slice_has_packed_neighbours_and_a_partner():
    """17 values: the slice's partner in its pair and the slices either side stay at 16 or fewer -- a mixed pair"""
    _, rp, cl, _ = ps.problem("p1_17")
    worst = _counts(rp, cl, ps.values("seventeen")).max(axis=1)
    assert ps.SLICE % 2 == 1 and worst[ps.SLICE] == 17 and worst[ps.SLICE - 1] <= 16 and worst[ps.SLICE + 1] <= 16


def test_the_generators_slots_agree_with_the_restatement():
    """the generator's placement and the restatement's, written apart, put every kept entry in the same slot"""
    for name, case in (("p1_17", "assembled_p1_17"), ("p1_10_9_11", "assembled_p1_10_9_11"), ("p1_17", "hostile")):
        _, rp, cl, _ = ps.problem(name)
        v = ps.values(case)
        sl = ps.slots(rp, cl, v)
        bits, have = _dense(rp, cl, v)
        row = np.repeat(np.arange(rp.size - 1), np.diff(rp))
        k = np.nonzero(sl >= 0)[0]
        assert have.sum() == k.size
        np.testing.assert_array_equal(bits[row[k] // 64, row[k] % 64, sl[k]], v.view(np.uint64)[k])
