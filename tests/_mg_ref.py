"""numpy / scipy restatement of the geometric multigrid preconditioner (ZZZ_PC_MG, include/zzz_abi.h) and of KSPCG around it.
It shares no code with the library: the level matrices come from the oracle (zo.Problem(kind, 1, nx, ny, nz).assemble() per
level), the transfer is built from its definition as a scipy matrix, the Chebyshev recurrences are written out with the
bounds PASSED IN, the coarsest level is a dense solve.

Level rule: level l+1 has max(2, (n+1)//2) cells per axis; the coarsest level is the first with at most `limit` scalar dofs,
or with 2 x 2 x 2 cells, or level `max_levels` (12 at most).

Transfer, for fine vertex (i_x, i_y, i_z) and axis a: c_a = min(i_a nc_a // nf_a, nc_a - 1);
f_a = float(i_a nc_a - c_a nf_a) / float(nf_a); axes sorted by descending f, ties to the lower axis: (a1, a2, a3); weights
1 - f_a1, f_a1 - f_a2, f_a2 - f_a3, f_a3 on the coarse vertices c, c + e_a1, c + e_a1 + e_a2, c + e_a1 + e_a2 + e_a3.
P~ = F_f P F_c with F zeroing the constrained dofs; block size 3 per component."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp
import zzz_oracle as zo

MAX_LEVELS = 12


def level_dims(n, bs, limit=1000, max_levels=0):
    cap = min(max_levels, MAX_LEVELS) if max_levels > 0 else MAX_LEVELS
    dims = [tuple(int(v) for v in n)]
    while True:
        d = dims[-1]
        dofs = (d[0] + 1) * (d[1] + 1) * (d[2] + 1) * bs
        if dofs <= limit or max(d) <= 2 or len(dims) >= cap:
            return dims
        dims.append(tuple(max(2, (v + 1) // 2) for v in d))


def prolongation(nf, nc, bs=1):
    """P (no Dirichlet handling) from the definition, one fine vertex at a time in integers"""
    pf = [v + 1 for v in nf]
    pc = [v + 1 for v in nc]
    rows, cols, vals = [], [], []
    for iz in range(pf[2]):
        for iy in range(pf[1]):
            for ix in range(pf[0]):
                i = (ix, iy, iz)
                c = [min(i[a] * nc[a] // nf[a], nc[a] - 1) for a in range(3)]
                f = [float(i[a] * nc[a] - c[a] * nf[a]) / float(nf[a]) for a in range(3)]
                order = sorted(range(3), key=lambda a: (-f[a], a))
                fs = [f[a] for a in order]
                w = (1.0 - fs[0], fs[0] - fs[1], fs[1] - fs[2], fs[2])
                row = (iz * pf[1] + iy) * pf[0] + ix
                pos = list(c)
                for k in range(4):
                    if k > 0:
                        pos[order[k - 1]] += 1
                    rows.append(row)
                    cols.append((pos[2] * pc[1] + pos[1]) * pc[0] + pos[0])
                    vals.append(w[k])
    P = sp.csr_matrix((vals, (rows, cols)), shape=(pf[0] * pf[1] * pf[2], pc[0] * pc[1] * pc[2]))
    if bs > 1:
        P = sp.kron(P, sp.identity(bs), format="csr")
    return P.tocsr()


def csr(p):
    return sp.csr_matrix((p.vals, p.cols, p.rowptr), shape=(p.n, p.n))


_problems = {}


def oracle_problem(kind, dims):
    key = (kind, tuple(dims))
    if key not in _problems:
        zo.set_num_threads(1)
        _problems[key] = zo.Problem(kind, 1, *dims).assemble()
    return _problems[key]


def oracle_bound(p, est_its=10):
    """min(Gershgorin's bound of D^-1 A, 1.1 x the Lanczos estimate): what ZZZ_PC_CHEBYSHEV_JACOBI takes, restated by the
    oracle (zo.esteig)"""
    A = csr(p)
    gersh = float((abs(A).sum(axis=1).A1 / np.abs(A.diagonal())).max())
    ritz = zo.esteig(p.rowptr.astype(np.int64), p.cols, p.vals, est_its)
    return min(gersh, 1.1 * ritz) if ritz > 0.0 else gersh


class Hierarchy:
    def __init__(self, kind, n, his=None, degree=2, ratio=10.0, limit=1000, max_levels=0, est_its=10):
        self.kind = kind
        self.bs = 3 if kind == "elasticity" else 1
        self.dims = level_dims(n, self.bs, limit, max_levels)
        self.probs = [oracle_problem(kind, d) for d in self.dims]
        self.A = [csr(p) for p in self.probs]
        self.free = [sp.diags(1.0 - p.bc.astype(float)) for p in self.probs]
        self.P = [(self.free[l] @ prolongation(self.dims[l], self.dims[l + 1], self.bs) @ self.free[l + 1]).tocsr()
                  for l in range(len(self.dims) - 1)]
        self.dinv = [1.0 / a.diagonal() for a in self.A]
        nl = len(self.dims)
        if his is None:
            his = [oracle_bound(self.probs[l], est_its) for l in range(nl - 1)]
        self.hi = list(his)[:nl - 1]
        self.degree, self.ratio = degree, ratio
        self.coarse = scipy.linalg.cho_factor(self.A[-1].toarray())

    def smooth(self, l, x, b):
        """Chebyshev-Jacobi of `degree` terms on [hi / ratio, hi]; x is None: the start from zero"""
        A, dinv = self.A[l], self.dinv[l]
        hi = self.hi[l]
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

    def vcycle(self, b, l=0):
        if l == len(self.A) - 1:
            return scipy.linalg.cho_solve(self.coarse, b)
        x = self.smooth(l, None, b)
        r = b - self.A[l] @ x
        x = x + self.P[l] @ self.vcycle(self.P[l].T @ r, l + 1)
        return self.smooth(l, x, b)


def pcg(A, b, M, norm_type=0, rtol=1e-8, atol=1e-50, max_it=10000):
    """KSPCG, zero initial guess, KSPConvergedDefault; norm_type 0 preconditioned, 1 unpreconditioned, 2 natural.
    Returns (iterations, x, history)"""
    x = np.zeros_like(b)
    r = b.copy()
    z = M(r)
    rz = float(r @ z)

    def norm():
        if norm_type == 0:
            return float(np.sqrt(z @ z))
        if norm_type == 1:
            return float(np.sqrt(r @ r))
        return float(np.sqrt(abs(rz)))
    dp = norm()
    hist = [dp]
    ttol = max(rtol * dp, atol)
    if dp <= ttol:
        return 0, x, np.array(hist)
    p = z.copy()
    it = 0
    while it < max_it:
        w = A @ p
        alpha = rz / float(p @ w)
        x += alpha * p
        r -= alpha * w
        z = M(r)
        rzn = float(r @ z)
        it += 1
        rz_old, rz = rz, rzn
        dp = norm()
        hist.append(dp)
        if dp <= ttol:
            break
        p = z + (rz / rz_old) * p
    return it, x, np.array(hist)
