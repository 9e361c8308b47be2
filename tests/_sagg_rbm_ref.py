"""numpy / scipy restatement of the smoothed-aggregation multigrid with rigid-body modes (ZZZ_PC_SAGG_RBM, include/zzz_abi.h).
It shares no code with the library: the aggregation is tests/_agg_ref.py's restatement of ZZZ_PC_AGG's rule, the smoother, the
V-cycle and the dense coarsest solve are tests/_mg_ref.py's, the term-by-term products are tests/_sagg_ref.py's, and the
orthogonalisation, the tentative prolongator and the dropped coarse dofs are written out below from the rule.

The rule, per level.  Scope, options, level rule, smoother, cycle, spectrum bound and omega = 4 / (3 hi) are ZZZ_PC_SAGG's.  Every
sum is a chain of plain double additions of individually rounded products, with no fused multiply-add.
  node size   3 on level 0, 6 on every coarse level.
  B           level 0: the library's six vectors as zzz_near_nullspace_build left them, in the caller's numbering, entries of
              constrained scalar dofs taken as 0.  Level l + 1: the B_c below, 6 columns by 6 rows per aggregate.
  aggregates  ZZZ_PC_AGG's rule on the node graph of the level's matrix: nodes are blocks of 3 scalar dofs on level 0 and
              blocks of 6 below.
  P_t, B_c    per aggregate J, its m member nodes in ascending index (the caller's numbering on level 0): take the rows of B of
              its member dofs, node-major then component ascending; modified Gram-Schmidt over the six columns in column order
              q = 0..5: for j < q, R(j, q) = <Q_j, b_q>, then b_q -= R(j, q) Q_j; then R(q, q) = |b_q| and Q_q = b_q / R(q, q).
              A column is DROPPED when |b_q| after the projections is at most 2^-30 of its norm before them, or when it is
              zero: then Q_q = 0 and row q of R is 0.  P_t(row, (J, q)) = Q_q(row); rows of constrained dofs and dropped
              columns carry no entries.  B_c's rows (J, 0..5) are R.
  one sum     every inner product and norm: partial sum l (l = 0..63) adds the products of the rows l, l + 64, ... front to
              back, then the 64 partial sums meet in the tree s[i] += s[i + o] for i < o, o = 32, 16, 8, 4, 2, 1; the result
              is s[0].  A norm is the square root of that sum of squares.
  P           P_t - omega D^-1 (A P_t): P(i, (J, q)) = P_t(i, (J, q)) - (omega s) / a_ii, s = sum_k a_ik P_t(k, (J, q)) over
              the unconstrained k in ascending k.  Pattern: (i, (J, q)) wherever row i is unconstrained and has a structural
              a_ik with k unconstrained, k in aggregate J and column q kept.  Rows of constrained dofs are empty.
  R, T, A_c   R = P^T, T = A P and A_c = P^T T exactly as ZZZ_PC_SAGG forms them: ascending summation index.
  dropped     a dropped coarse dof (J, q) has no entry in P; its row of A_c is the single entry 1 on the diagonal.  On the
              next level it is an ordinary dof with a zero row in B.
`descending` adds the same terms of every sum back to front (the 64 partial sums from their last row to their first, the tree
from neighbouring pairs upwards): what rounding alone changes."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp

import _agg_ref as AR
import _sagg_ref as SR
from _agg_ref import CASES, CASE_IDS, LIMIT, MAX_LEVELS, aggregate, bound, case_part, case_system, pcg  # noqa: F401
from _sagg_ref import row_bars  # noqa: F401

ELASTICITY = [c for c in CASE_IDS if "elasticity" in c]
NCOL = 6
DROP = 2.0 ** -30

# The spread of the restatement's PCG iteration count under rounding alone, measured by tests/test_sagg_rbm_ref.py on the
# twelve (case, norm type) pairs -- the three elasticity cases and the island case -- at rtol 1e-8: the plain restatement
# against the restatement with every level's numbering reversed and KSPCG's sums in reversed chunks of 64: 0 in all twelve
# (13 14 13, 28 31 29, 12 12 12 and 11 12 12 in both, against ZZZ_PC_SAGG's 22 24 23, 42 47 45, 18 19 19 and 16 17 17).  The GPU
# bar on the count is this spread + 2, the + 2 being the standing allowance of the other CG forms' tests.
MEASURED_SPREAD = 0
IT_BAR = MEASURED_SPREAD + 2


def wave_sum(v, descending=False):
    """the rule's one sum of the terms v"""
    pad = (-v.size) % 64
    rows = np.concatenate([v, np.zeros(pad)]).reshape(-1, 64)
    s = np.zeros(64)
    for r in (rows[::-1] if descending else rows):
        s = s + r
    if descending:
        n = 64
        while n > 1:
            s = s[0:n:2] + s[1:n:2]
            n //= 2
        return float(s[0])
    for o in (32, 16, 8, 4, 2, 1):
        s[:o] = s[:o] + s[o:2 * o]
    return float(s[0])


def orthogonalise(X, descending=False):
    """X: 6 columns as rows [6][M].  Returns (Q [6][M], R [6][6], keep [6], ratios [6]: |b_q| after / before the projections)"""
    Q = np.array(X, float)
    R = np.zeros((NCOL, NCOL))
    keep = np.zeros(NCOL, bool)
    ratios = np.zeros(NCOL)
    for q in range(NCOL):
        before = np.sqrt(wave_sum(Q[q] * Q[q], descending))
        for j in range(q):
            if keep[j]:
                R[j, q] = wave_sum(Q[j] * Q[q], descending)
                Q[q] = Q[q] - R[j, q] * Q[j]
        after = np.sqrt(wave_sum(Q[q] * Q[q], descending))
        ratios[q] = after / before if before > 0.0 else 0.0
        if after == 0.0 or after <= DROP * before:
            Q[q] = 0.0
        else:
            keep[q] = True
            R[q, q] = after
            Q[q] = Q[q] / after
    return Q, R, keep, ratios


def tentative(B, agg, bc, ns, nagg, descending=False):
    """(P_t as CSR with its structural zeros, B_c [6][6 nagg], keep [6 nagg], ratios [6 nagg])"""
    bc = np.asarray(bc)
    nf = agg.size * ns
    Bz = np.where(bc[None, :] != 0, 0.0, B)
    order = np.argsort(agg, kind="stable")  # members of an aggregate in ascending node index
    order = order[agg[order] >= 0]
    starts = np.searchsorted(agg[order], np.arange(nagg + 1))
    Bc, keep, ratios = np.zeros((NCOL, NCOL * nagg)), np.zeros(NCOL * nagg, bool), np.zeros(NCOL * nagg)
    Qrow = np.zeros((NCOL, nf))
    for J in range(nagg):
        nodes = order[starts[J]:starts[J + 1]]
        rows = (nodes[:, None] * ns + np.arange(ns)[None, :]).ravel()
        Q, R, k, rt = orthogonalise(Bz[:, rows], descending)
        Qrow[:, rows] = Q
        Bc[:, NCOL * J:NCOL * J + NCOL] = R.T  # row (J, q) of B_c is row q of R
        keep[NCOL * J:NCOL * J + NCOL] = k
        ratios[NCOL * J:NCOL * J + NCOL] = rt
    # the rows of P_t: the kept columns of the row's aggregate, none in a constrained row
    d = np.arange(nf)
    a = agg[d // ns]
    has = (a >= 0) & (bc == 0)
    kept = keep.reshape(nagg, NCOL)
    cnt = np.where(has, kept.sum(axis=1)[np.maximum(a, 0)], 0)
    indptr = np.zeros(nf + 1, np.int64)
    np.cumsum(cnt, out=indptr[1:])
    ri = np.repeat(d, cnt)
    qs = np.concatenate([np.flatnonzero(kept[a[i]]) for i in d[has]]) if has.any() else np.zeros(0, np.int64)
    Pt = sp.csr_matrix((Qrow[qs, ri], (a[ri] * NCOL + qs).astype(np.int32), indptr), shape=(nf, NCOL * nagg))
    return Pt, Bc, keep, ratios


def smoothed(A, Pt, bc, omega, descending=False):
    """P = P_t - omega D^-1 (A P_t) on the structural pattern of A P_t"""
    S = SR.product_ap(A, Pt, bc, descending)
    si = SR._rows_of(S)
    own = np.zeros(S.nnz)
    key = si.astype(np.int64) * S.shape[1] + S.indices
    pk = SR._rows_of(Pt).astype(np.int64) * Pt.shape[1] + Pt.indices
    pos = np.searchsorted(key, pk)  # (P_t's entries are entries of S: a_ii is structural)
    assert np.array_equal(key[pos], pk)
    own[pos] = Pt.data
    S.data = own - (omega * S.data) / A.diagonal()[si]
    return S


def with_unit_rows(Ac, dropped):
    """A_c with the single entry 1 on the diagonal of every dropped coarse dof (whose row and column are empty)"""
    d = np.flatnonzero(dropped)
    assert np.all(np.diff(Ac.indptr)[d] == 0)
    rows = np.concatenate([SR._rows_of(Ac), d])
    cols = np.concatenate([Ac.indices.astype(np.int64), d])
    return SR._sum_terms(rows, cols, np.concatenate([Ac.data, np.ones(d.size)]), Ac.shape, False)


class RbmHierarchy(AR.AggHierarchy):
    """the levels of ZZZ_PC_SAGG_RBM for the matrix A with Dirichlet bytes bc and the near-nullspace B [6][dofs]; smooth(),
    vcycle(), reversed() and vcycle_reversed() are the base classes'.  like: take the aggregates and bounds of that hierarchy
    and add every sum back to front."""

    def __init__(self, A, bc, B, his=None, degree=2, ratio=10.0, limit=1000, max_levels=0, est_its=10, like=None):
        cap = min(max_levels, MAX_LEVELS) if max_levels > 0 else MAX_LEVELS
        A = sp.csr_matrix(A)
        A.sort_indices()
        desc = like is not None
        if desc:
            his = like.hi
        bc = np.asarray(bc, np.uint8)
        self.bs = 3
        self.A, self.bc, self.B = [A], [bc], [np.where(bc[None, :] != 0, 0.0, np.asarray(B, float))]
        self.agg, self.roots, self.rounds, self.hi, self.Pt, self.P, self.T, self.keep, self.ratios = [], [], [], [], [], [], [], [], []
        while self.A[-1].shape[0] > limit and len(self.A) < cap:
            Al, bcl, l = self.A[-1], self.bc[-1], len(self.A) - 1
            ns = 3 if l == 0 else NCOL
            if desc:
                if l >= len(like.agg):
                    break
                agg, roots, nagg, rounds = like.agg[l], like.roots[l], like.A[l + 1].shape[0] // NCOL, like.rounds[l]
            else:
                agg, roots, nagg, rounds = aggregate(Al, bcl, ns)
            if nagg == 0 or 2 * nagg * NCOL > Al.shape[0]:
                break
            hi = his[l] if his is not None and l < len(his) else bound(Al, est_its)
            Pt, Bc, keep, ratios = tentative(self.B[l], agg, bcl, ns, nagg, desc)
            P = smoothed(Al, Pt, bcl, 4.0 / (3.0 * hi), desc)
            T = SR.product_ap(Al, P, bcl, desc)
            self.agg.append(agg)
            self.roots.append(roots)
            self.rounds.append(rounds)
            self.hi.append(hi)
            self.Pt.append(Pt)
            self.P.append(P)
            self.T.append(T)
            self.keep.append(keep)
            self.ratios.append(ratios)
            self.A.append(with_unit_rows(SR.product_ptt(P, T, desc), ~keep))
            self.B.append(Bc)
            self.bc.append(np.zeros(nagg * NCOL, np.uint8))
        self.dinv = [1.0 / a.diagonal() for a in self.A]
        self.degree, self.ratio = degree, ratio
        self.coarse = scipy.linalg.cho_factor(self.A[-1].toarray())

    def dropped(self):
        """per level: how many of its dofs are dropped coarse dofs (level 0: none)"""
        return [0] + [int((~k).sum()) for k in self.keep]

    def descending(self):
        if not hasattr(self, "_desc"):
            self._desc = RbmHierarchy(self.A[0], self.bc[0], self.B[0], degree=self.degree, ratio=self.ratio, limit=-1,
                                      max_levels=len(self.A), like=self)
        return self._desc


def rigid_body_modes(x, n_owned):
    """six orthonormal rigid-body modes [6][3 n_owned] at the dof coordinates x, turned about their centre (for the CPU tests:
    the GPU tests take the library's)"""
    x = np.asarray(x, float)[:n_owned]
    c = x - x.mean(axis=0)
    B = np.zeros((6, n_owned, 3))
    for a in range(3):
        B[a, :, a] = 1.0
    B[3, :, 0], B[3, :, 1] = -c[:, 1], c[:, 0]
    B[4, :, 0], B[4, :, 2] = c[:, 2], -c[:, 0]
    B[5, :, 2], B[5, :, 1] = c[:, 1], -c[:, 2]
    B = B.reshape(6, -1)
    for i in range(6):
        for k in range(i):
            B[i] -= (B[i] @ B[k]) * B[k]
        B[i] /= np.linalg.norm(B[i])
    return B


def island_bc(P):
    """the island case on the elasticity P1 6 x 6 x 6 Part: every node of x-index >= 4 constrained (beside the Part's own set)
    except the nodes (5, 3, 3), (5, 1, 1) and (5, 1, 2): (bc bytes, the constrained scalar dofs)"""
    x = np.asarray(P.dof_x)[:P.n_owned]
    lo, hi = x.min(axis=0), x.max(axis=0)
    idx = np.rint((x - lo) / (hi - lo) * np.array(P.dims)).astype(int)
    bc = P.bc_marker().copy().reshape(-1, 3)
    free = np.zeros(P.n_owned, bool)
    for t in ((5, 3, 3), (5, 1, 1), (5, 1, 2)):
        free |= (idx == np.array(t)).all(axis=1)
    assert free.sum() == 3
    bc[(idx[:, 0] >= 4) & ~free] = 1
    bc[free] = 0
    bc = bc.reshape(-1)
    return bc, np.flatnonzero(bc).astype(np.int32)
