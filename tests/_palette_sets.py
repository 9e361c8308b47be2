"""Value arrays for tests/test_gpu_palette_codes.py: the packed form of the one-chunk product's value codes (4-bit indices into
per-(slice, slot) palettes of 16 codes; csrc/zzz_sellp_dict.hip, k_sp_pal_build).  tests/test_palette_value_sets.py proves on the
CPU, with a restatement of its own, that every array holds the per-(slice, slot) counts its case claims.

The arrays live on the assembled pattern of a small P1 lattice and keep an exact zero wherever the assembled matrix has one:
the packer drops exact zeros, so every row keeps at most eight entries and every slice stays one chunk.

slots(): where the packer puts a kept entry (csrc/zzz_sellp_pack.hip, emit_chunk).  Entries by rank in their row; but where
every row of a slice fits "column = delta[slot] + lane" on the deltas of the slice's first longest row, by column (short
boundary rows then leave holes).  A hole, a slot beyond the slice's width and a lane without a row read as +0.0."""
import numpy as np

import _value_sets as vs

# the cube of tests/_value_sets.py (5 832 rows = 92 slices, the last one of 8 rows) and a lattice that is no cube:
# 11 x 10 x 12 vertices = 1 320 rows = 21 slices (an odd count: the last slice has no partner), the last one of 40 rows
PROBLEMS = {"p1_17": None, "p1_10_9_11": ("poisson", 1, (10, 9, 11))}
_problems = {}


def problem(name):
    """(Part, rowptr, cols, assembled values) of the lattice: pattern and values from the oracle"""
    if name not in _problems:
        if PROBLEMS[name] is None:
            _problems[name] = vs.problem(name)[:4]
        else:
            import zzz
            import zzz_oracle as zo

            kind, order, dims = PROBLEMS[name]
            P = zzz.Part(kind, order, *dims)
            rp, cl = zo.pattern(P.n_owned, P.cell_dofs, P.bs)
            _problems[name] = (P, rp, cl, zo.assemble_matrix(P.form, order, P.x, P.cells, P.cell_dofs, P.bc_marker(), rp, cl))
    return _problems[name]


def slots(rp, cl, v):
    """slot of every CSR entry in its slice's chunk (-1: an exact zero, dropped); every slice must stay one chunk"""
    n = rp.size - 1
    slot = np.full(cl.size, -1, np.int64)
    for s in range((n + 63) // 64):
        rows = range(64 * s, min(n, 64 * s + 64))
        kept = [[k for k in range(rp[r], rp[r + 1]) if v[k] != 0.0] for r in rows]
        w = max(len(ks) for ks in kept)
        assert 1 <= w <= 8, (s, w)
        ref = next(i for i, ks in enumerate(kept) if len(ks) == w)
        delta = [int(cl[k]) - ref for k in kept[ref]]
        by_column = all(d >= 0 and d + 63 < n for d in delta)
        trial = {}
        for lane, ks in enumerate(kept):
            for k in ks:
                t = int(cl[k]) - lane
                if t in delta:
                    trial[k] = delta.index(t)
                else:
                    by_column = False
        for ks in kept:
            for q, k in enumerate(ks):
                slot[k] = trial[k] if by_column else q
    return slot


def _pool(n, seed):
    """n distinct finite doubles in (1, 2), none of them a lattice's stencil entry"""
    rng = np.random.default_rng(seed)
    p = np.unique(1.0 + rng.integers(1, 1 << 40, size=2 * n + 8).astype(np.float64) * 2.0 ** -41)
    assert p.size >= n
    return rng.permutation(p)[:n]


def tame(name):
    """few values in every slot of every slice: the diagonal 2, every other kept entry one of five by its distance to the
    diagonal"""
    _, rp, cl, base = problem(name)
    row = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    v = np.where(cl == row, 2.0, -0.25 - 0.001 * ((cl - row) % 5))
    return np.where(base != 0.0, v, 0.0)


SLICE, SLOT = 41, 3  # where the counted cases put their values: an interior slice of the cube, the second of its pair


def counted(name, count):
    """tame(), but slot SLOT of slice SLICE holds exactly `count` distinct values (a hole's +0.0 among them, if it has holes)"""
    _, rp, cl, _ = problem(name)
    v = tame(name)
    sl = slots(rp, cl, v)
    row = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    at = np.nonzero((sl == SLOT) & (row // 64 == SLICE))[0]
    fresh = count - (1 if at.size < 64 else 0)
    assert at.size >= fresh
    v[at] = _pool(fresh, 1000 + count)[np.arange(at.size) % fresh]
    return v


def every_entry_its_own(name):
    """every kept entry of a slice has a value of its own (512 values in all, far fewer than the LDS dictionary holds): a slot
    holds as many distinct values as it has entries"""
    _, rp, cl, base = problem(name)
    pool = _pool(512, 7)
    v = np.zeros(cl.size)
    for r in range(rp.size - 1):
        ks = [k for k in range(rp[r], rp[r + 1]) if base[k] != 0.0]
        for q, k in enumerate(ks):
            v[k] = pool[(r % 64) + 64 * q]
    return v


HOSTILE = np.array([0x8000000000000000, 0x0000000000000001, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000,
                    0x7FEFFFFFFFFFFFFF, 0x0010000000000000], np.uint64)  # -0.0, a subnormal, +-inf, NaN, DBL_MAX, DBL_MIN


def hostile(name):
    """tame(), with the hostile patterns on off-diagonal entries of interior rows of slices SLICE - 1 and SLICE (-0.0 is an
    exact zero to the packer: it leaves a hole)"""
    _, rp, cl, _ = problem(name)
    v = tame(name)
    for s in (SLICE - 1, SLICE):
        inner = [r for r in range(64 * s, 64 * s + 64) if np.count_nonzero(v[rp[r]:rp[r + 1]]) == 7]  # (no boundary row)
        for i, pat in enumerate(HOSTILE):
            r = inner[2 * i]
            ks = [k for k in range(rp[r], rp[r + 1]) if v[k] != 0.0 and cl[k] != r]
            v.view(np.uint64)[ks[i % len(ks)]] = pat
    return v


# name -> (lattice, maker, claim); claims: largest = the largest per-(slice, slot) count in the matrix, unpacked = the slices
# with a slot of more than 16
CASES = {
    "assembled_p1_17": ("p1_17", lambda: problem("p1_17")[3].copy(), dict(some_packed=True, some_unpacked=True)),
    "assembled_p1_10_9_11": ("p1_10_9_11", lambda: problem("p1_10_9_11")[3].copy(), dict(some_packed=True, some_unpacked=True)),
    "tame": ("p1_17", lambda: tame("p1_17"), dict(unpacked=[])),
    "sixteen": ("p1_17", lambda: counted("p1_17", 16), dict(largest=16, unpacked=[], at=(SLICE, SLOT, 16))),
    "seventeen": ("p1_17", lambda: counted("p1_17", 17), dict(largest=17, unpacked=[SLICE], at=(SLICE, SLOT, 17))),
    "none_packed": ("p1_10_9_11", lambda: every_entry_its_own("p1_10_9_11"), dict(all_unpacked=True, largest=64)),
    "hostile": ("p1_17", lambda: hostile("p1_17"), dict(unpacked=[], hostile=True)),
}
_values = {}


def values(case):
    if case not in _values:
        _values[case] = CASES[case][1]()
    return _values[case]
