"""numpy / scipy restatement of the p-multigrid preconditioner (ZZZ_PC_PMG, include/zzz_abi.h) for the P2 and P3 cube
problems.  It shares no code with the library.

Fine problem: the host feed zzz.Part(kind, order, nx, ny, nz) -- the same numbering as the generated cube -- assembled by the
oracle (zo.pattern, zo.assemble_matrix, zo.assemble_vector).

Transfer: P from its definition, "the P1 basis of the same mesh evaluated at the Pk dof points", cell by cell: the Pk nodes of
the reference tetrahedron are zo.ref_nodes(order), the P1 basis there is (1 - x - y - z, x, y, z) on the cell's four vertices,
and the vertices of the feed are the P1 dofs (lexicographic).  No lattice formula is used.  P~ = F_k P F_1 with F zeroing the
constrained dofs; block size 3 per component.

Cycle: Pk Chebyshev-Jacobi smoothing from zero, the P1 V-cycle of tests/_mg_ref.py on the same cube through P~, Pk smoothing
from the corrected iterate; the bounds are PASSED IN (level 0's first, then the P1 hierarchy's)."""
import numpy as np
import scipy.sparse as sp
import zzz
import zzz_oracle as zo
from _mg_ref import Hierarchy, level_dims

_parts = {}


def part(kind, order, n):
    key = (kind, order, tuple(n))
    if key not in _parts:
        _parts[key] = zzz.Part(kind, order, *n)
    return _parts[key]


def prolongation(kind, order, n):
    """P (no Dirichlet handling, scalar): Pk dofs x lattice points.  Returns (P, the largest disagreement between two cells that
    share a dof)"""
    F, C = part(kind, order, n), part(kind, 1, n)
    assert np.array_equal(F.cells, C.cells) and np.array_equal(F.x, C.x)
    # the feed's vertices are the P1 dofs
    assert np.array_equal(C.cell_dofs, C.cells)
    X = zo.ref_nodes(order)
    lam = np.stack([1.0 - X.sum(axis=1), X[:, 0], X[:, 1], X[:, 2]], 1)  # nd x 4
    nc, nd = F.cell_dofs.shape
    rows = np.repeat(F.cell_dofs.astype(np.int64), 4, axis=1).reshape(-1)
    cols = np.tile(F.cells.astype(np.int64), (1, nd)).reshape(-1)
    vals = np.tile(lam.reshape(-1), nc)
    keep = np.abs(vals) > 1e-14  # (a node on an edge or a face has exact zeros on the vertices off it)
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    key = rows * C.n_owned + cols
    order_ = np.argsort(key, kind="stable")
    key, vals = key[order_], vals[order_]
    first = np.ones(key.shape[0], bool)
    first[1:] = key[1:] != key[:-1]
    start = np.nonzero(first)[0]
    spread = float((np.maximum.reduceat(vals, start) - np.minimum.reduceat(vals, start)).max())
    P = sp.csr_matrix((vals[first], (key[first] // C.n_owned, key[first] % C.n_owned)), shape=(F.n_owned, C.n_owned))
    return P, spread


def fine_problem(kind, order, n):
    """(A as scipy CSR, b, bc bytes, rowptr int64, cols, vals) of the Pk problem, by the oracle on the host feed"""
    P = part(kind, order, n)
    zo.set_num_threads(4)
    rp, cl = zo.pattern(P.n_owned, P.cell_dofs, P.bs)
    bc = P.bc_marker()
    v = zo.assemble_matrix(P.form, order, P.x, P.cells, P.cell_dofs, bc, rp, cl)
    poisson = P.form == zzz.FORM_POISSON
    b = zo.assemble_vector(P.form, order, P.x, P.cells, P.cell_dofs, P.f, P.g if poisson else None, P.facets if poisson else None, bc)
    N = P.n_owned * P.bs
    return sp.csr_matrix((v, cl, rp), shape=(N, N)), b, bc, rp.astype(np.int64), cl, v


def pmg_level_dims(n, bs, limit=1000, max_levels=0):
    """all levels: the Pk level, then the P1 levels from the same cube on; max_levels counts all of them"""
    assert max_levels != 1
    return [tuple(n)] + level_dims(n, bs, limit, max_levels - 1 if max_levels > 0 else 0)


class PHierarchy:
    def __init__(self, kind, order, n, his=None, degree=2, ratio=10.0, limit=1000, max_levels=0, est_its=10):
        """his: the bounds of every smoothing level, level 0 (Pk) first; None: the oracle's own"""
        self.kind, self.order, self.n = kind, order, tuple(n)
        self.bs = 3 if kind == "elasticity" else 1
        self.A, self.b, self.bc, self.rowptr, self.cols, self.vals = fine_problem(kind, order, n)
        if his is None:
            gersh = float((abs(self.A).sum(axis=1).A1 / np.abs(self.A.diagonal())).max())
            ritz = zo.esteig(self.rowptr, self.cols, self.vals, est_its)
            hi0, his1 = (min(gersh, 1.1 * ritz) if ritz > 0.0 else gersh), None
        else:
            hi0, his1 = his[0], list(his[1:])
        self.H1 = Hierarchy(kind, self.n, his=his1, degree=degree, ratio=ratio, limit=limit,
                            max_levels=max_levels - 1 if max_levels > 0 else 0, est_its=est_its)
        self.dims = [self.n] + list(self.H1.dims)
        self.hi = [hi0] + list(self.H1.hi)
        P, self.spread = prolongation(kind, order, n)
        if self.bs > 1:
            P = sp.kron(P, sp.identity(self.bs), format="csr")
        self.Praw = P.tocsr()
        free_f = sp.diags(1.0 - self.bc.astype(float))
        self.P = (free_f @ self.Praw @ self.H1.free[0]).tocsr()
        self.dinv = 1.0 / self.A.diagonal()
        self.degree, self.ratio = degree, ratio

    def smooth(self, x, b):
        A, dinv, hi = self.A, self.dinv, self.hi[0]
        lo = hi / self.ratio
        theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
        sigma = theta / delta
        rho = 1.0 / sigma
        g = dinv * b if x is None else dinv * (b - A @ x)
        d = g / theta
        x = d.copy() if x is None else x + d
        for _ in range(1, self.degree):
            g = g - dinv * (A @ d)
            rhon = 1.0 / (2.0 * sigma - rho)
            d = (rhon * rho) * d + (2.0 * rhon / delta) * g
            rho = rhon
            x = x + d
        return x

    def vcycle(self, b):
        x = self.smooth(None, b)
        r = b - self.A @ x
        x = x + self.P @ self.H1.vcycle(self.P.T @ r)
        return self.smooth(x, b)
