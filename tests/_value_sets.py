"""Hostile value arrays for the value dictionaries (csrc/zzz_valset.h and its five users): given a CSR pattern in the library's
internal order, arrays with EXACTLY a requested number of distinct nonzero bit patterns matrix-wide, per 64-row slice, on the
diagonal (as inverses) or per 3 x 3 block, plus the bit patterns a dictionary could mistake for something else.  CPU, numpy only.
Every generator checks its own claim before it returns; tests/test_value_sets.py checks them again, independently, for every
case tests/test_gpu_value_codes.py uses.

"Distinct" always means distinct as 64-bit patterns (-0.0 is a value of its own, +0.0 is no value: code 0 stands for it)."""
import numpy as np

NEG_ZERO = np.uint64(0x8000000000000000)
QUIET_NAN = np.uint64(0x7FF8000000000000)
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
_M52 = (1 << 52) - 1


def bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.uint64)


def nonzero_patterns(v):
    """the distinct bit patterns of v other than +0.0"""
    u = np.unique(bits(v))
    return u[u != 0]


def set_hash(b, nbits):
    """valset_hash of csrc/zzz_valset.h restated: used only to AIM inputs at a table's end, never asserted on"""
    b = np.asarray(b, np.uint64).copy()
    b ^= b >> np.uint64(29)
    b *= np.uint64(0x9E3779B97F4A7C15)
    return (b >> np.uint64(64 - nbits)).astype(np.int64)


def pool(n, rng, avoid=None):
    """n distinct finite doubles of magnitude [0.5, 2), either sign, none of them in `avoid`"""
    out = np.zeros(0, np.uint64)
    while out.size < n:
        m = rng.integers(0, _M52, size=n + 64, dtype=np.uint64, endpoint=True)
        e = rng.integers(1022, 1024, size=n + 64).astype(np.uint64)  # 2^-1, 2^0
        s = rng.integers(0, 2, size=n + 64).astype(np.uint64)
        out = np.unique(np.concatenate([out, (s << np.uint64(63)) | (e << np.uint64(52)) | m]))
        if avoid is not None:
            out = np.setdiff1d(out, np.asarray(avoid, np.uint64))
    out = out[rng.permutation(out.size)[:n]]
    return out.view(np.float64)


def clustered(nbits, n, rng, transform=None, lo=0.5, hi=2.0):
    """n distinct finite doubles in [lo, hi) whose home slot (of transform(value), if given: the inverse diagonal holds 1 / d)
    lies in the last four slots of a table of 2^nbits: probe chains of hundreds that wrap round the table's end"""
    got = np.zeros(0)
    while got.size < n:
        d = rng.uniform(lo, hi, size=1 << 22)
        t = d if transform is None else transform(d)
        d = d[set_hash(bits(t), nbits) >= (1 << nbits) - 4]
        got = np.concatenate([got, d])
        t = got if transform is None else transform(got)
        got = got[np.unique(bits(t), return_index=True)[1]]
    return got[:n]


def hostile_patterns(infinite=False, all_ones=False):
    """the small pool of hostile() as bit patterns"""
    p = [0x8000000000000000, 1, 0x000FFFFFFFFFFFFF, 0x0010000000000000, 0x7FEFFFFFFFFFFFFF,  # -0.0, least / largest subnormal, DBL_MIN, DBL_MAX
         0x3FF0000000000000, 0x3FF0000000000001, 0xBFE0000000000000, 0xBFE0000000000001,  # pairs one ulp apart
         0x3FF123456789ABCD, 0x3FF12345FEDCBA98, 0x4001234589ABCDEF, 0x3FE9876589ABCDEF]  # pairs equal in the upper / lower half
    if infinite:
        p += [0x7FF0000000000000, 0xFFF0000000000000, int(QUIET_NAN)]
    if all_ones:
        p += [int(ALL_ONES)]
    return np.array(p, np.uint64)


class Gen:
    def __init__(self, rowptr, cols, bs=1, seed=0):
        self.rp = np.asarray(rowptr, np.int64)
        self.cl = np.asarray(cols, np.int64)
        self.bs = bs
        self.n = self.rp.size - 1
        self.nnz = int(self.rp[-1])
        self.seed = seed
        self.rows = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.rp))
        self.diag_at = np.nonzero(self.rows == self.cl)[0]
        assert self.diag_at.size == self.n, "every row holds its diagonal"

    def _rng(self, *key):
        return np.random.default_rng([self.seed, *key])

    # ---- assignment of a pool to entries: every value used, runs of repeats as assembled rows have them ----------------------
    @staticmethod
    def _spread(m, n, rng):
        """m indices into a pool of n, every one of 0..n-1 present, a third of them repeating their predecessor"""
        assert m >= n, (m, n)
        idx = rng.integers(0, n, size=m)
        keep = rng.random(m) >= 0.33
        keep[0] = True
        idx = idx[np.maximum.accumulate(np.where(keep, np.arange(m), 0))]
        idx[rng.permutation(m)[:n]] = np.arange(n)
        return idx

    def _pairs(self):
        """entry -> index of its unordered (row, column) pair, and the pairs' (lo, hi)"""
        lo, hi = np.minimum(self.rows, self.cl), np.maximum(self.rows, self.cl)
        ncol = int(max(self.n, self.cl.max() + 1))
        key, inv = np.unique(lo * ncol + hi, return_inverse=True)
        return inv, key // ncol, key % ncol

    def _dominant_shift(self, v):
        off = np.abs(v).copy()
        off[self.diag_at] = 0.0
        rs = np.add.reduceat(off, self.rp[:-1])
        return float(2.0 ** np.ceil(np.log2(rs.max() + 1.0)))

    def matrix_wide(self, n, spd=False, zero_frac=0.02, include=None, diag_values=8):
        """exactly n distinct nonzero patterns over all entries, every one used; some entries +0.0.  include: patterns that must
        be among the n.  spd: symmetric, the diagonal = shift + k 2^-12 (diag_values of them), strictly diagonally dominant"""
        rng = self._rng(1, n)
        inc = np.zeros(0, np.uint64) if include is None else np.unique(np.asarray(include, np.uint64))
        inc = inc[inc != 0]
        v = np.zeros(self.nnz)
        if not spd:
            p = np.concatenate([inc.view(np.float64), pool(n - inc.size, rng, avoid=inc)])
            nz = np.nonzero(rng.random(self.nnz) >= zero_frac)[0]
            v[nz] = p[self._spread(nz.size, n, rng)]
        else:
            assert inc.size == 0
            nd = min(diag_values, n - 1, self.n)
            inv, lo, hi = self._pairs()
            offp = np.nonzero(lo != hi)[0]
            p = pool(n - nd, rng)
            pv = np.zeros(lo.size)
            live = offp[rng.random(offp.size) >= zero_frac]
            pv[live] = p[self._spread(live.size, n - nd, rng)]
            v = pv[inv]
            shift = self._dominant_shift(v)
            v[self.diag_at] = shift + self._spread(self.n, nd, rng) * 2.0 ** -12
        assert nonzero_patterns(v).size == n
        return v

    def per_slice(self, counts):
        """slice s (rows 64 s .. 64 s + 63) holds exactly counts[s] distinct nonzero patterns, the slices' sets pairwise disjoint"""
        counts = np.asarray(counts, np.int64)
        assert counts.size == (self.n + 63) // 64
        rng = self._rng(2, int(counts.sum()))
        p = pool(int(counts.sum()), rng)
        v = np.zeros(self.nnz)
        at = 0
        for s, c in enumerate(counts):
            a, b = self.rp[64 * s], self.rp[min(64 * s + 64, self.n)]
            v[a:b] = p[at + self._spread(int(b - a), int(c), rng)]
            at += int(c)
        return v

    def diagonal(self, d, base, extra=None):
        """the off-diagonal entries of `base` kept (its upper triangle, mirrored), the diagonal replaced by shift + t[i], t from d values (steps of 2^-12; the d
        values of `extra`, offsets in [0, d 2^-12), replace the first of them) such that the INVERSE diagonal holds exactly d
        patterns; shift above the largest absolute row sum"""
        rng = self._rng(3, d)
        inv, lo, _ = self._pairs()
        pv = np.zeros(lo.size)
        pv[inv[self.rows <= self.cl]] = np.asarray(base, np.float64)[self.rows <= self.cl]
        v = pv[inv]  # (assembled (i, j) and (j, i) differ in the last bit here and there: the upper triangle serves both)
        shift = self._dominant_shift(v)
        t = np.arange(d) * 2.0 ** -12
        if extra is not None:
            t[:len(extra)] = np.asarray(extra) - shift
        v[self.diag_at] = shift + t[self._spread(self.n, d, rng)]
        dg = v[self.diag_at]
        assert np.unique(bits(1.0 / dg)).size == d and np.unique(bits(dg)).size == d
        return v

    # ---- block size 3 ---------------------------------------------------------------------------------------------------------
    def block_positions(self):
        """pos[q, a, b] = entry of block q's (a, b); brow[q], bcol[q] its block row / column"""
        assert self.bs == 3 and self.n % 3 == 0
        r0 = self.rp[0:-1:3]
        nb = (self.rp[1::3] - r0) // 3
        assert np.array_equal(self.rp[1::3] - r0, self.rp[2::3] - self.rp[1::3]) and np.all(nb * 3 == self.rp[1::3] - r0)
        brow = np.repeat(np.arange(self.n // 3), nb)
        k = np.arange(brow.size) - np.repeat(np.cumsum(nb) - nb, nb)
        ln = np.repeat(nb * 3, nb)
        pos = (np.repeat(r0, nb) + 3 * k)[:, None, None] + (np.arange(3)[:, None] * ln[:, None, None]) + np.arange(3)[None, None, :]
        return pos, brow, self.cl[pos[:, 0, 0]] // 3

    @staticmethod
    def _sym9(t6):
        return t6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]]

    def blocks(self, nblocks, nvalues, spd=False, zero_blocks=40):
        """exactly nblocks distinct nonzero 3 x 3 blocks (9-tuples of patterns) from exactly nvalues distinct nonzero values (-0.0
        one of them); among them blocks that differ in one entry, permutations of each other, and pairs that differ only by
        +0.0 / -0.0 in one entry; zero_blocks whole blocks of +0.0 and as many of -0.0 (not counted: the forms drop them).
        spd: every block symmetric, mirrored over the diagonal; the diagonal blocks carry `shift` (one of the values) on their
        diagonal: symmetric and strictly diagonally dominant"""
        rng = self._rng(4, nblocks, nvalues)
        V, B = nvalues, nblocks
        pos, brow, bcol = self.block_positions()
        vals = np.concatenate([[0.0], pool(V, rng)])  # index 0 = +0.0, 1 = -0.0, 2.. ordinary; spd: V = the shift
        vals[1] = -0.0
        nord = V - 1 if spd else V  # indices 1 .. nord may go anywhere
        # index tuples: coverage first (every value used), then the special relatives of block 0, then random ones
        w = 6 if spd else 9
        ncov = -(-nord // w)
        cov = (np.arange(ncov * w) % nord + 1).reshape(ncov, w)
        b0 = cov[0].copy()
        sp = [b0.copy() for _ in range(4)]
        sp[0][w // 2] = b0[w // 2] % nord + 1  # one entry differs
        sp[1] = b0[[5, 4, 2, 3, 1, 0]] if spd else b0[::-1].copy()  # a permutation (rows and columns reversed)
        sp[2][w - 1] = 1  # -0.0 in one entry ...
        sp[3][w - 1] = 0  # ... +0.0 in the same
        ndiag = 0
        tup = np.concatenate([cov, np.array(sp), rng.integers(0, nord + 1, size=(2 * B + 64, w))])
        if spd:
            tup = self._sym9(tup)
            ndiag = min(16, B // 4)
            dg = self._sym9(rng.integers(2, nord + 1, size=(4 * ndiag + 8, 6)))
            dg[:, [0, 4, 8]] = V
            dg = dg[np.sort(np.unique(dg, axis=0, return_index=True)[1])][:ndiag]
            assert dg.shape[0] == ndiag
        tup = tup[np.sort(np.unique(tup, axis=0, return_index=True)[1])]
        tup = tup[(tup > 1).any(axis=1)][:B - ndiag]  # (a block of nothing but +-0.0 is a zero block)
        assert tup.shape[0] == B - ndiag and ncov + 4 <= B - ndiag, (tup.shape, B, ncov)
        v = np.zeros(self.nnz)
        if not spd:
            live = rng.permutation(brow.size)
            zb = live[:2 * zero_blocks]
            live = np.sort(live[2 * zero_blocks:])
            which = self._spread(live.size, B, rng)
            v[pos[live].reshape(-1)] = vals[tup[which]].reshape(-1)
            v[pos[zb[zero_blocks:]].reshape(-1)] = -0.0
        else:
            ncol = int(bcol.max()) + 1
            lo, hi = np.minimum(brow, bcol), np.maximum(brow, bcol)
            key, inv = np.unique(lo * ncol + hi, return_inverse=True)
            isd = (key // ncol) == (key % ncol)
            offp, dgp = np.nonzero(~isd)[0], np.nonzero(isd)[0]
            pick = np.zeros((key.size, 9), np.int64)
            pick[offp] = tup[self._spread(offp.size, B - ndiag, rng)]
            pick[dgp] = dg[self._spread(dgp.size, ndiag, rng)]
            shift = 2.0 ** np.ceil(np.log2(6.0 * (np.bincount(brow).max() + 1)))  # > 3 entries of magnitude < 2 per block of the row
            vals[V] = shift
            v[pos.reshape(-1)] = vals[pick[inv]].reshape(-1)
        nb, nv = block_counts(v, pos)
        assert (nb, nv) == (B, V), (nb, nv, B, V)
        return v

    # ---- hostile bit patterns mixed into ordinary values ------------------------------------------------------------------------
    def hostile(self, base, infinite=False, all_ones=False, every_slice=False):
        """`base` with the hostile pool written over a few entries spread through the matrix: each pattern as single entries
        (twice; all_ones with every_slice: once in every 64-row slice), -0.0 also as a whole row and, block size 3, as a whole
        3 x 3 block and as one entry inside a kept block"""
        v = np.array(base, np.float64)
        b = v.view(np.uint64)
        p = hostile_patterns(infinite, all_ones)
        at = (np.arange(1, 2 * p.size + 1) * self.nnz) // (2 * p.size + 2) + 1
        b[at] = np.concatenate([p, p])
        r = self.n // 3
        b[self.rp[r]:self.rp[r + 1]] = NEG_ZERO
        if self.bs == 3:
            pos, _, _ = self.block_positions()
            b[pos[pos.shape[0] // 5].reshape(-1)] = NEG_ZERO
            b[pos[pos.shape[0] // 7][1, 2]] = NEG_ZERO
        if all_ones and every_slice:
            b[self.rp[0:self.n:64] + 1] = ALL_ONES
        return v


def block_counts(v, pos):
    """(distinct nonzero 3 x 3 blocks, distinct nonzero values inside them): a block of nothing but +-0.0 is no block"""
    blk = bits(v)[pos.reshape(-1, 9)]
    kept = blk[((blk << np.uint64(1)) != 0).any(axis=1)]
    u = np.unique(kept)
    return np.unique(kept, axis=0).shape[0], int(u[u != 0].size)


def slice_counts(v, rowptr):
    n = rowptr.size - 1
    return np.array([nonzero_patterns(v[rowptr[s]:rowptr[min(s + 64, n)]]).size for s in range(0, n, 64)])


def is_symmetric_dominant(rowptr, cols, v):
    import scipy.sparse as sp

    n = rowptr.size - 1
    A = sp.csr_matrix((v, cols, rowptr), shape=(n, n))
    d = A.diagonal()
    off = abs(A).sum(axis=1).A1 - np.abs(d)
    return (abs(A - A.T)).max() == 0.0 and bool(np.all(d > off))


# ---- the cases of tests/test_gpu_value_codes.py, proved on the CPU by tests/test_value_sets.py -------------------------------
PROBLEMS = {"p1_17": ("poisson", 1, (17, 17, 17)), "p1_80": ("poisson", 1, (80, 80, 80)), "p3_555": ("poisson", 3, (5, 5, 5)),
            "p3_546": ("poisson", 3, (5, 4, 6)), "p3_666": ("poisson", 3, (6, 6, 6)), "el_20": ("elasticity", 1, (20, 20, 20)),
            "p1_diag": ("poisson", 1, (24, 22, 23))}
_problems = {}


def problem(name):
    """(Part, rowptr, cols, assembled values, Gen) of PROBLEMS[name]: pattern and values from the oracle"""
    if name not in _problems:
        import zzz
        import zzz_oracle as zo

        kind, order, dims = PROBLEMS[name]
        P = zzz.Part(kind, order, *dims)
        rp, cl = zo.pattern(P.n_owned, P.cell_dofs, P.bs)
        base = zo.assemble_matrix(P.form, order, P.x, P.cells, P.cell_dofs, P.bc_marker(), rp, cl)
        _problems[name] = (P, rp, cl, base, Gen(rp, cl, P.bs, seed=len(name) + order))
    return _problems[name]


def _ordinary(g, name, form2=False):
    """values the form under test holds with room to spare (what the hostile patterns are mixed into)"""
    if name == "el_20" and form2:
        return g.blocks(3000, 150)  # (more blocks than the table in LDS holds: rows of offsets into a value dictionary)
    if name == "p3_555":
        return g.per_slice([120] * ((g.n + 63) // 64))  # (7 680 matrix-wide: the slice dictionaries' turn, every block window's too)
    if name == "el_20":
        return g.blocks(600, 150)
    return g.matrix_wide(700)


def _hostile(name, level, every_slice=False, clustered_bits=0, form2=False):
    def make(g, base):
        v = _ordinary(g, name, form2)
        if clustered_bits:
            c = clustered(clustered_bits, 300, g._rng(5, clustered_bits))
            at = (np.arange(1, 601) * g.nnz) // 602 + 3
            v[at] = np.concatenate([c, c])
            return v
        return g.hostile(v, infinite=level >= 1, all_ones=level >= 2, every_slice=every_slice)
    return make


def _diag_special(pattern):
    def make(g, base):
        v = g.diagonal(64, base)
        v.view(np.uint64)[g.diag_at[g.n // 2]] = np.uint64(pattern)
        return v
    return make


def _diag_clustered(g, base):
    shift = g._dominant_shift(np.asarray(base))
    c = clustered(14, 300, g._rng(6), transform=lambda d: 1.0 / d, lo=shift, hi=2.0 * shift)
    return g.diagonal(1000, base, extra=c)


# name -> (problem, maker(gen, assembled values), claim).  Claims: matrix = distinct nonzero patterns matrix-wide; slices =
# per 64-row slice (disjoint); dinv = distinct patterns of 1 / diagonal; blocks = (distinct nonzero blocks, values in them);
# spd = symmetric and strictly diagonally dominant with a positive diagonal
CASES = {}
for _n in (2047, 2048, 65534, 65535):
    CASES[f"stream_forced_{_n}"] = ("p1_17", lambda g, b, n=_n: g.matrix_wide(n), dict(matrix=_n))
for _n in (2046, 2047):
    CASES[f"stream_default_{_n}"] = ("p1_80", lambda g, b, n=_n: g.matrix_wide(n), dict(matrix=_n))
CASES["stream_spd_1500"] = ("p1_17", lambda g, b: g.matrix_wide(1500, spd=True), dict(matrix=1500, spd=True))
CASES["stream_spd_2047"] = ("p1_17", lambda g, b: g.matrix_wide(2047, spd=True), dict(matrix=2047, spd=True))
CASES["stream_spd_2048"] = ("p1_17", lambda g, b: g.matrix_wide(2048, spd=True), dict(matrix=2048, spd=True))
CASES["stream_spd_30000"] = ("p1_17", lambda g, b: g.matrix_wide(30000, spd=True), dict(matrix=30000, spd=True))
CASES["slices_all_1023"] = ("p3_555", lambda g, b: g.per_slice([1023] * 64), dict(slices=[1023] * 64))
CASES["slices_one_1024"] = ("p3_555", lambda g, b: g.per_slice([1023] * 17 + [1024] + [1023] * 46), dict(slices=[1023] * 17 + [1024] + [1023] * 46))
CASES["slices_odd_1024"] = ("p3_555", lambda g, b: g.per_slice([1023, 1024] * 32), dict(slices=[1023, 1024] * 32))
for _d in (2048, 2049, 13800):
    CASES[f"dinv_{_d}"] = ("p1_diag", lambda g, b, d=_d: g.diagonal(d, b), dict(dinv=_d, spd=True))
CASES["dinv_clustered"] = ("p1_diag", _diag_clustered, dict(dinv=1000, spd=True))
for _k, _p in (("zero", 0), ("subnormal", 0x0000000000000400), ("inf", 0x7FF0000000000000), ("negative", 0xC000000000000000),
               ("nan", int(QUIET_NAN)), ("all_ones", int(ALL_ONES))):
    CASES[f"dinv_end_{_k}"] = ("p1_diag", _diag_special(_p), dict(diag_pattern=_p))
for _b, _v in ((2199, 400), (2200, 400), (5000, 2046), (5000, 2047), (65535, 40), (65536, 40)):
    CASES[f"blocks_{_b}_{_v}"] = ("el_20", lambda g, b, B=_b, V=_v: g.blocks(B, V), dict(blocks=(_b, _v)))
for _b, _v in ((2199, 400), (2200, 400), (2200, 2046), (2200, 2047)):
    CASES[f"blocks_spd_{_b}_{_v}"] = ("el_20", lambda g, b, B=_b, V=_v: g.blocks(B, V, spd=True), dict(blocks=(_b, _v), spd=True))
for _w in (4095, 4096, 8191, 8192):
    CASES[f"windows_{_w}"] = ("p3_555", lambda g, b, n=_w: g.matrix_wide(n), dict(matrix=_w))
for _w in (3000, 4095, 4096, 8191):
    CASES[f"windows_spd_{_w}"] = ("p3_555", lambda g, b, n=_w: g.matrix_wide(n, spd=True), dict(matrix=_w, spd=True))
CASES["p3_555_spd_1500"] = ("p3_555", lambda g, b: g.matrix_wide(1500, spd=True), dict(matrix=1500, spd=True))
# (off-diagonal entries from a pool of 500, every row a diagonal value of its own: 4 596 matrix-wide, at most 564 in a slice)
CASES["p3_555_spd_sliced"] = ("p3_555", lambda g, b: g.matrix_wide(4596, spd=True, diag_values=4096), dict(matrix=4596, spd=True, slice_max=1023))
CASES["p3_555_all"] = ("p3_555", lambda g, b: g.matrix_wide(g.nnz, zero_frac=0.0), dict(matrix="nnz"))
for _p in ("p3_546", "p3_666"):
    CASES[f"windows_{_p}_8191"] = (_p, lambda g, b: g.matrix_wide(8191), dict(matrix=8191))
    CASES[f"windows_{_p}_all"] = (_p, lambda g, b: g.matrix_wide(g.nnz, zero_frac=0.0), dict(matrix="nnz"))
for _p in ("p1_17", "p3_555", "el_20"):
    for _l in (0, 1, 2):
        CASES[f"hostile_{_p}_{_l}"] = (_p, _hostile(_p, _l), dict(hostile=_l))
CASES["hostile_p3_555_2_every_slice"] = ("p3_555", _hostile("p3_555", 2, every_slice=True), dict(hostile=2, every_slice=True))
for _l in (0, 1, 2):
    CASES[f"hostile_el_20_{_l}_form2"] = ("el_20", _hostile("el_20", _l, form2=True), dict(hostile=_l))
for _p, _bits in (("p1_17", 18), ("p3_555", 14), ("p3_555", 11), ("el_20", 13)):
    CASES[f"clustered_{_p}_{_bits}"] = (_p, _hostile(_p, 0, clustered_bits=_bits, form2=True), dict(clustered=_bits))
_values = {}


def values(name):
    """the value array of CASES[name] (cached: the CPU proof and the GPU test see the same array)"""
    if name not in _values:
        _, _, _, base, g = problem(CASES[name][0])
        _values[name] = CASES[name][1](g, base)
    return _values[name]
