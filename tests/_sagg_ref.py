"""numpy / scipy restatement of the smoothed-aggregation multigrid preconditioner (ZZZ_PC_SAGG, include/zzz_abi.h).  It shares
no code with the library: the aggregation is tests/_agg_ref.py's restatement of ZZZ_PC_AGG's rule, the smoother, the V-cycle and
the dense coarsest solve are tests/_mg_ref.py's, and the smoothed prolongator and the two products are written out below, term
by term, from the rule.

The rule, per level.  Every sum is a chain of plain double additions of individually rounded products, in ascending index:
  aggregates  _agg_ref.aggregate on the graph of the level's matrix.
  P_t         _agg_ref.prolongator: 1 from each unconstrained scalar dof (i, c) to (aggregate(i), c).
  omega       4 / (3 hi), hi the bound of D^-1 A of the level's smoother (_agg_ref.bound, or PASSED IN).
  P           (I - omega D^-1 A) P_t.  Pattern: (i, J) wherever row i is unconstrained and has a structural entry a_ik, zero or
              not, with k unconstrained and mapped to J by P_t.  s = sum_k a_ik over those k;  P(i, J) = delta - (omega s) / a_ii,
              delta = 1 when P_t(i, J) = 1, else 0.  Rows of constrained dofs are empty.
  T           A P:  T(i, J) = sum_k a_ik P(k, J)  (rows of constrained dofs left out: P^T never reads them).
  A_c         P^T T:  A_c(I, J) = sum_i P(i, I) T(i, J); its pattern is every (I, J) that receives a structural term.
  levels      _agg_ref's rule.
np.add.at adds in the order it is given: ascending, or -- `descending` -- the same terms back to front, which is the hierarchy
with every level's numbering reversed, written in the forward numbering."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp

import _agg_ref as R
from _agg_ref import CASES, CASE_IDS, LIMIT, MAX_LEVELS, aggregate, bound, case_part, case_system, pcg  # noqa: F401

# The spread of the restatement's PCG iteration count under rounding alone, measured by tests/test_sagg_ref.py on the
# twenty-one (case, norm type) pairs at rtol 1e-8: the plain restatement with plain sums against the restatement with every
# level's numbering reversed and KSPCG's sums in reversed chunks of 64: 0 in all twenty-one (9 10 9, 17 19 18, 33 36 35,
# 22 24 23, 42 47 45, 7 6 6, 18 19 19 in both, against plain aggregation's 15 16 15, 21 23 22, 36 38 37, 27 29 27, 48 52 50,
# 7 7 7, 19 20 19 and Jacobi's 71, 88, 152, 126, 237, 18, 63).  The GPU bar on the count is this spread + 2, the + 2 being the
# standing allowance of the other CG forms' tests.
MEASURED_SPREAD = 0
IT_BAR = MEASURED_SPREAD + 2


def _sum_terms(rows, cols, vals, shape, descending):
    """the CSR matrix whose entry (r, c) is the sum of the terms with that (r, c), added in the order given (or backwards)"""
    key = rows.astype(np.int64) * shape[1] + cols.astype(np.int64)
    uk, inv = np.unique(key, return_inverse=True)
    inv = inv.ravel()
    out = np.zeros(uk.size)
    if descending:
        np.add.at(out, inv[::-1], vals[::-1])
    else:
        np.add.at(out, inv, vals)
    indptr = np.zeros(shape[0] + 1, np.int64)
    np.cumsum(np.bincount(uk // shape[1], minlength=shape[0]), out=indptr[1:])
    return sp.csr_matrix((out, (uk % shape[1]).astype(np.int32), indptr), shape=shape)


def _rows_of(M):
    return np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))


def smoothed_prolongator(A, agg, bc, bs, nagg, omega, descending=False):
    assert A.has_sorted_indices
    bc = np.asarray(bc)
    rows, cols = _rows_of(A), A.indices.astype(np.int64)
    ok = (bc[rows] == 0) & (bc[cols] == 0) & (agg[cols // bs] >= 0)
    i, k = rows[ok], cols[ok]
    S = _sum_terms(i, agg[k // bs] * bs + k % bs, A.data[ok], (A.shape[0], nagg * bs), descending)
    si = _rows_of(S)
    delta = (S.indices == agg[si // bs] * bs + si % bs).astype(float)
    S.data = delta - (omega * S.data) / A.diagonal()[si]
    return S


def _paired_rows(L, Rm, which):
    """for every entry e of L in CSR order and every entry f of row which[e] of Rm in CSR order: (e, f)"""
    assert L.has_sorted_indices and Rm.has_sorted_indices
    cnt = np.diff(Rm.indptr)[which]
    el = np.repeat(np.arange(L.nnz), cnt)
    er = np.repeat(Rm.indptr[which], cnt) + np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return el, er


def product_ap(A, P, bc, descending=False):
    """T(i, J) = sum_k a_ik P(k, J), k ascending"""
    ea, ep = _paired_rows(A, P, A.indices)  # entry (i, k) of A with the entries (k, J) of P's row k
    i = _rows_of(A)[ea]
    keep = np.asarray(bc)[i] == 0
    ea, ep, i = ea[keep], ep[keep], i[keep]
    return _sum_terms(i, P.indices[ep], A.data[ea] * P.data[ep], (A.shape[0], P.shape[1]), descending)


def product_ptt(P, T, descending=False):
    """A_c(I, J) = sum_i P(i, I) T(i, J), i ascending"""
    et, ep = _paired_rows(T, P, _rows_of(T))  # entry (i, J) of T with the entries (i, I) of P's row i
    return _sum_terms(P.indices[ep], T.indices[et], P.data[ep] * T.data[et], (P.shape[1], T.shape[1]), descending)


class SaggHierarchy(R.AggHierarchy):
    """the levels of ZZZ_PC_SAGG for the matrix A with Dirichlet bytes bc; smooth(), vcycle(), reversed() and vcycle_reversed()
    are the base classes'.  like: take the aggregates and bounds of that hierarchy and add every sum back to front."""

    def __init__(self, A, bc, bs, his=None, degree=2, ratio=10.0, limit=1000, max_levels=0, est_its=10, like=None):
        cap = min(max_levels, MAX_LEVELS) if max_levels > 0 else MAX_LEVELS
        A = sp.csr_matrix(A)
        A.sort_indices()
        desc = like is not None
        if desc:
            his = like.hi
        self.bs = bs
        self.A, self.bc, self.agg, self.roots, self.P, self.T, self.rounds, self.hi = [A], [np.asarray(bc, np.uint8)], [], [], [], [], [], []
        while self.A[-1].shape[0] > limit and len(self.A) < cap:
            Al, bcl, l = self.A[-1], self.bc[-1], len(self.A) - 1
            if desc:
                if l >= len(like.agg):
                    break
                agg, roots, nagg, rounds = like.agg[l], like.roots[l], like.A[l + 1].shape[0] // bs, like.rounds[l]
            else:
                agg, roots, nagg, rounds = aggregate(Al, bcl, bs)
            if nagg == 0 or 2 * nagg * bs > Al.shape[0]:
                break
            hi = his[l] if his is not None and l < len(his) else bound(Al, est_its)
            omega = 4.0 / (3.0 * hi)
            P = smoothed_prolongator(Al, agg, bcl, bs, nagg, omega, desc)
            T = product_ap(Al, P, bcl, desc)
            self.agg.append(agg)
            self.roots.append(roots)
            self.rounds.append(rounds)
            self.hi.append(hi)
            self.P.append(P)
            self.T.append(T)
            self.A.append(product_ptt(P, T, desc))
            self.bc.append(np.zeros(nagg * bs, np.uint8))
        self.dinv = [1.0 / a.diagonal() for a in self.A]
        self.degree, self.ratio = degree, ratio
        self.coarse = scipy.linalg.cho_factor(self.A[-1].toarray())

    def descending(self):
        """the same aggregates, bounds and patterns with every sum added back to front: what rounding alone changes"""
        if not hasattr(self, "_desc"):
            self._desc = SaggHierarchy(self.A[0], self.bc[0], self.bs, degree=self.degree, ratio=self.ratio, limit=-1,
                                       max_levels=len(self.A), like=self)
        return self._desc


def row_bars(M, Md, floor=1e-12):
    """per entry of M: 8 x the largest difference between M and Md (the same pattern) in that entry's row, and not below `floor`
    of the row's largest entry"""
    assert np.array_equal(M.indptr, Md.indptr) and np.array_equal(M.indices, Md.indices)
    n = np.diff(M.indptr)
    full = n > 0
    diff, big = np.zeros(M.shape[0]), np.zeros(M.shape[0])
    diff[full] = np.maximum.reduceat(np.abs(M.data - Md.data), M.indptr[:-1][full])
    big[full] = np.maximum.reduceat(np.abs(M.data), M.indptr[:-1][full])
    return np.repeat(np.maximum(8.0 * diff, floor * big), n)
