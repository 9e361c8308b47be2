"""numpy / scipy restatement of the plain-aggregation multigrid preconditioner (ZZZ_PC_AGG, include/zzz_abi.h) and of KSPCG
around it.  It shares no code with the library: the fine matrices come from the oracle (or from the test), the aggregation,
P and P^T A P are written out from the rule below, the smoother and the V-cycle are tests/_mg_ref.py's (Chebyshev-Jacobi with
the bounds PASSED IN, a dense coarsest solve).

The rule, per level (bs scalar dofs per block dof):
  graph     nodes: the block dofs with at least one unconstrained component; i ~ j (i != j) when any scalar entry of their
            coupling is nonzero.  Block dofs whose components are all constrained stay out.
  priority  of node i, in 64-bit unsigned arithmetic:  x = i + 0x9E3779B97F4A7C15;  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;
            x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31;  priority = ((x >> 33) << 32) | i.
  roots     synchronous rounds until nobody is undecided: an undecided node whose priority exceeds that of every undecided
            node within distance 2 becomes a root; then every undecided node within distance 2 of a root goes out.
  numbers   aggregates by ascending root index.
  joins     two synchronous rounds: an unaggregated node joins the aggregate of its adjacent aggregated neighbour with the
            largest aggregate number.
  the rest  singletons in index order, numbered behind the roots' aggregates.
  P         1 from each unconstrained scalar dof (i, c) to (aggregate(i), c); zero rows elsewhere.
  A_c       P^T A P, every entry summed in ascending fine (row, column) order; its pattern holds (I, J) whenever a fine
            entry (structural, zero or not) has both ends in P's range.
  levels    level l + 1 is added while level l has more than `limit` scalar dofs, fewer than max_levels (12 at most) levels
            exist, and the aggregation of level l leaves at most half its dofs (and at least one)."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp

import zzz
import zzz_oracle as zo
from _mg_ref import Hierarchy

MAX_LEVELS = 12
LIMIT = 50  # pc_mg_coarse_eq_limit of the tests: every case below then has at least three levels

# (name, problem, order, shape); shape None: Part.spoke(problem, order, 3).  Poisson P2 is 7 x 6 x 8, not the 6 x 5 x 7 of the
# other CG tests, Poisson P3 6 x 5 x 7, not 4 x 3 x 5, and elasticity P2 4 x 4 x 5, not 3 x 3 x 4: the smaller shapes reach two
# levels only at limit 50 (their first aggregation already leaves fewer than 50 dofs: 35 at Poisson P2).
CASES = [("poisson_p1", "poisson", 1, (12, 10, 14)), ("poisson_p2", "poisson", 2, (7, 6, 8)), ("poisson_p3", "poisson", 3, (6, 5, 7)),
         ("elasticity_p1", "elasticity", 1, (6, 6, 6)), ("elasticity_p2", "elasticity", 2, (4, 4, 5)),
         ("spoke_poisson", "poisson", 1, None), ("spoke_elasticity", "elasticity", 1, None)]
CASE_IDS = [c[0] for c in CASES]

# The spread of the restatement's PCG iteration count under rounding alone, measured by tests/test_agg_ref.py on the
# twenty-one (case, norm type) pairs at rtol 1e-8: the sums of KSPCG plain against in reversed chunks of 64
# (tests/_pipecg_ref.py's dot product): 0 in all twenty-one (15 16 15, 21 23 22, 36 38 37, 27 29 27, 48 52 50, 7 7 7, 19 20 19
# in both orders, against Jacobi's 71, 88, 152, 126, 237, 18, 63).  The GPU bar on the count is this spread + 2, the + 2 being
# the standing allowance of the other CG forms' tests.
MEASURED_SPREAD = 0
IT_BAR = MEASURED_SPREAD + 2

_M64 = (1 << 64) - 1


def priority(i):
    x = (int(i) + 0x9E3779B97F4A7C15) & _M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M64
    x ^= x >> 31
    return ((x >> 33) << 32) | int(i)


def node_edges(A, bc, bs):
    """(free, ei, ej): the graph's nodes and its directed edges, both ends free, i != j, one per nonzero scalar entry"""
    n = A.shape[0] // bs
    free = (np.asarray(bc).reshape(n, bs) == 0).any(axis=1)
    coo = A.tocoo()
    nz = coo.data != 0.0
    ei, ej = coo.row[nz] // bs, coo.col[nz] // bs
    keep = (ei != ej) & free[ei] & free[ej]
    return free, ei[keep], ej[keep]


def aggregate(A, bc, bs):
    """returns (agg, roots, naggregates, rounds): agg[i] = aggregate of block dof i, -1 for a node out of the graph;
    roots[a] = the root of aggregate a < roots.size (the aggregates behind them are singletons)"""
    n = A.shape[0] // bs
    free, ei, ej = node_edges(A, bc, bs)
    key = np.array([priority(i) for i in range(n)], np.int64)
    state = np.where(free, 0, 3)  # 0 undecided, 1 root, 2 out, 3 not in the graph
    rounds = 0
    while (state == 0).any():
        own = np.where(state == 0, key, -1)
        m1 = own.copy()
        np.maximum.at(m1, ei, own[ej])
        m1[~free] = -1
        m2 = m1.copy()
        np.maximum.at(m2, ei, m1[ej])
        state[(state == 0) & (m2 == key)] = 1
        root = state == 1
        near1 = root.copy()
        np.logical_or.at(near1, ei, root[ej])
        near1 &= free
        near2 = near1.copy()
        np.logical_or.at(near2, ei, near1[ej])
        state[(state == 0) & near2] = 2
        rounds += 1
        assert rounds < 4096
    agg = np.full(n, -1, np.int64)
    roots = np.flatnonzero(state == 1)
    agg[roots] = np.arange(roots.size)
    for _ in range(2):
        best = np.full(n, -1, np.int64)
        np.maximum.at(best, ei, agg[ej])
        agg = np.where(free & (agg < 0), best, agg)
    rest = np.flatnonzero(free & (agg < 0))
    agg[rest] = roots.size + np.arange(rest.size)
    return agg, roots, roots.size + rest.size, rounds


def prolongator(agg, bc, bs, nagg):
    n = agg.size
    d = np.arange(n * bs)
    ok = (agg[d // bs] >= 0) & (np.asarray(bc) == 0)
    return sp.csr_matrix((np.ones(ok.sum()), (d[ok], agg[d[ok] // bs] * bs + d[ok] % bs)), shape=(n * bs, nagg * bs))


def galerkin(A, agg, bc, bs, nagg):
    """P^T A P entry by entry: np.add.at adds in the order given, which is ascending fine (row, column)"""
    A = A.tocsr()
    assert A.has_sorted_indices
    N, nc = A.shape[0], nagg * bs
    rows = np.repeat(np.arange(N), np.diff(A.indptr))
    cols = A.indices.astype(np.int64)
    bc = np.asarray(bc)
    ok = (agg[rows // bs] >= 0) & (agg[cols // bs] >= 0) & (bc[rows] == 0) & (bc[cols] == 0)
    R = agg[rows[ok] // bs] * bs + rows[ok] % bs
    C = agg[cols[ok] // bs] * bs + cols[ok] % bs
    uk, inv = np.unique(R * nc + C, return_inverse=True)
    vals = np.zeros(uk.size)
    np.add.at(vals, inv.ravel(), A.data[ok])
    indptr = np.zeros(nc + 1, np.int64)
    np.cumsum(np.bincount(uk // nc, minlength=nc), out=indptr[1:])
    return sp.csr_matrix((vals, (uk % nc).astype(np.int32), indptr), shape=(nc, nc))


def bound(A, est_its=10):
    """min(Gershgorin's bound of D^-1 A, 1.1 x the Lanczos estimate): ZZZ_PC_CHEBYSHEV_JACOBI's, restated by the oracle"""
    A = A.tocsr()
    gersh = float((abs(A).sum(axis=1).A1 / np.abs(A.diagonal())).max())
    ritz = zo.esteig(A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data, est_its)
    return min(gersh, 1.1 * ritz) if ritz > 0.0 else gersh


class AggHierarchy(Hierarchy):
    """the levels of ZZZ_PC_AGG for the matrix A with Dirichlet bytes bc; smooth() and vcycle() are _mg_ref.Hierarchy's"""

    def __init__(self, A, bc, bs, his=None, degree=2, ratio=10.0, limit=1000, max_levels=0, est_its=10):
        cap = min(max_levels, MAX_LEVELS) if max_levels > 0 else MAX_LEVELS
        A = sp.csr_matrix(A)
        A.sort_indices()
        self.bs = bs
        self.A, self.bc, self.agg, self.roots, self.P, self.rounds = [A], [np.asarray(bc, np.uint8)], [], [], [], []
        while self.A[-1].shape[0] > limit and len(self.A) < cap:
            Al, bcl = self.A[-1], self.bc[-1]
            agg, roots, nagg, rounds = aggregate(Al, bcl, bs)
            if nagg == 0 or 2 * nagg * bs > Al.shape[0]:
                break
            self.agg.append(agg)
            self.roots.append(roots)
            self.rounds.append(rounds)
            self.P.append(prolongator(agg, bcl, bs, nagg))
            self.A.append(galerkin(Al, agg, bcl, bs, nagg))
            self.bc.append(np.zeros(nagg * bs, np.uint8))
        self.dinv = [1.0 / a.diagonal() for a in self.A]
        nl = len(self.A)
        if his is None:
            his = [bound(self.A[l], est_its) for l in range(nl - 1)]
        self.hi = list(his)[:nl - 1]
        self.degree, self.ratio = degree, ratio
        self.coarse = scipy.linalg.cho_factor(self.A[-1].toarray())

    def complexity(self):
        return sum(a.nnz for a in self.A) / self.A[0].nnz

    def reversed(self):
        """the same hierarchy with every level's numbering reversed: the same operator, every sum in the opposite order"""
        H = object.__new__(AggHierarchy)
        H.bs = self.bs
        H.A = [sp.csr_matrix(a[::-1, ::-1]) for a in self.A]
        for a in H.A:
            a.sort_indices()
        H.P = [sp.csr_matrix(p[::-1, ::-1]) for p in self.P]
        H.dinv = [d[::-1].copy() for d in self.dinv]
        H.hi, H.degree, H.ratio = self.hi, self.degree, self.ratio
        H.coarse = scipy.linalg.cho_factor(H.A[-1].toarray())
        return H

    def vcycle_reversed(self, b):
        if not hasattr(self, "_rev"):
            self._rev = self.reversed()
        return self._rev.vcycle(b[::-1].copy())[::-1].copy()


def pcg(A, b, M, norm_type=0, rtol=1e-8, atol=1e-50, max_it=10000, dot=np.dot):
    """KSPCG, zero initial guess, KSPConvergedDefault; norm_type 0 preconditioned, 1 unpreconditioned, 2 natural; `dot`
    replaces the summation order of its sums.  Returns (iterations, x)"""
    x = np.zeros_like(b)
    r = b.copy()
    z = M(r)
    rz = float(dot(r, z))

    def norm():
        if norm_type == 0:
            return float(np.sqrt(dot(z, z)))
        if norm_type == 1:
            return float(np.sqrt(dot(r, r)))
        return float(np.sqrt(abs(rz)))
    dp = norm()
    ttol = max(rtol * dp, atol)
    if dp <= ttol:
        return 0, x
    p = z.copy()
    it = 0
    while it < max_it:
        w = A @ p
        alpha = rz / float(dot(p, w))
        x += alpha * p
        r -= alpha * w
        z = M(r)
        rz_old, rz = rz, float(dot(r, z))
        it += 1
        if norm() <= ttol:
            break
        p = z + (rz / rz_old) * p
    return it, x


_parts, _systems = {}, {}


def case_part(name):
    if name not in _parts:
        _, problem, order, shape = CASES[CASE_IDS.index(name)]
        _parts[name] = zzz.Part.spoke(problem, order, 3) if shape is None else zzz.Part(problem, order, *shape)
    return _parts[name]


def case_system(name):
    """(A, bc, b, bs) of the case from the oracle, in the numbering of its Part"""
    if name not in _systems:
        P = case_part(name)
        zo.set_num_threads(4)
        bc = P.bc_marker()
        rp, cl = zo.pattern(P.n_owned, P.cell_dofs, P.bs)
        v = zo.assemble_matrix(P.form, P.order, P.x, P.cells, P.cell_dofs, bc, rp, cl)
        b = zo.assemble_vector(P.form, P.order, P.x, P.cells, P.cell_dofs, P.f, P.g, P.facets, bc)
        A = sp.csr_matrix((v, cl, rp), shape=(rp.size - 1, rp.size - 1))
        _systems[name] = (A, bc, b, P.bs)
    return _systems[name]
