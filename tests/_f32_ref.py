"""numpy float32 restatement of the single-precision cgpoisson path (zzz_action_f32, zzz_cg_solve_f32; the reference with
T = float at src/cgpoisson_problem.cpp:28 and U = float in src/cg.h:18-86).  It shares no code with the library.

Action.  y_e = float32(A_e) . float32(u_e) in float32, A_e from the oracle's `tabulate` in double; the element vectors are
scattered in double and the constrained rows zeroed.  For P1 there is a second form, `action32_p1_geometry`, that builds
the element geometry in float32 as a float kernel must: the vertex coordinates are first taken relative to an origin of
their chunk of cells (subtracted in double) and rounded; Jacobian, cofactors, determinant and the element vector are then
float32 arithmetic.  `absolute=True` rounds the absolute coordinates instead -- what the library must NOT do.

CG.  src/cg.h:38-86 on vectors of `dtype`; the sums behind <p,y> and <r,r> are accumulated in double and rounded to `dtype`
once (the library's stated difference from the reference, which accumulates in U); alpha and beta are `dtype`.

Measured with this restatement (u = noise for the action; the oracle's right-hand side, x0 = 0, 100 iterations at rtol 1e-6
for cg.h):
  case          action error max|y32 - y64| / max|y64|                            |x32 - x64| / |x64|   <r,r>/<r0,r0> f64 / f32
  P1 24x22x23   5.0e-8  (float geometry: 1.3e-7 on 12x10x14, 5.5e-7 on 40x38x42)   2.4e-7                2.4756e-11 / 2.4758e-11
  P2 12x11x13   6.0e-8                                                           1.6e-6                6.8106e-11 / 6.8110e-11
  P3  8x7x9     7.8e-8                                                           6.7e-6                2.0831e-6  / 2.1792e-6
  P3 14x13x15   8.3e-8
(An earlier float32 restatement on the assembled matrices recorded larger solution differences, 1.7e-5 / 8.2e-6 / 6.4e-6;
the figures pinned below are this module's own, which is what the GPU tests are told to scale.)
"""
import functools

import numpy as np
import zzz_oracle as zo

# |x32 - x64| / |x64| of this restatement after cg.h's 100 iterations at rtol 1e-6, as recorded above: what the GPU tests
# scale their bound from (tests/test_f32_ref.py keeps them honest)
SOLUTION_DIFF = {(1, (24, 22, 23)): 2.4e-7, (2, (12, 11, 13)): 1.6e-6, (3, (8, 7, 9)): 6.7e-6}


def noise(n):
    L = zo.lib()
    return np.array([L.zo_noise(i) for i in range(n)])


def element_matrices(order, x, cells):
    """A_e [ncells, nd, nd] in double from the oracle's tabulate.  Cells that are translates of each other (a lattice has six
    shapes) share one call: the form is translation invariant and the cache key is the shape to 1e-12."""
    cd = x[cells]  # [nc, 4, 3]
    rel = np.round((cd - cd[:, :1, :]).reshape(len(cells), 12), 12)
    shapes, first, inv = np.unique(rel, axis=0, return_index=True, return_inverse=True)
    A = np.array([zo.tabulate("poisson_a", order, cd[i]) for i in first])
    return A[np.asarray(inv).reshape(-1)]


def scatter(cell_dofs, ye, bc, n):
    y = np.zeros(n)
    np.add.at(y, cell_dofs.reshape(-1), ye.astype(np.float64).reshape(-1))
    y[bc.astype(bool)] = 0.0
    return y


def action(Ae, cell_dofs, bc, u, dtype):
    """y = action(u): element products in `dtype`, scattered in double"""
    ue = u.astype(dtype)[cell_dofs]
    ye = np.einsum("cij,cj->ci", Ae.astype(dtype), ue).astype(dtype)
    return scatter(cell_dofs, ye, bc, u.shape[0])


def action32_p1_geometry(x, cells, cell_dofs, bc, u, chunk=2048, absolute=False):
    """P1 with the geometry formed in float32 from chunk-relative coordinates"""
    f = np.float32
    nc = len(cells)
    origin = x[cells[(np.arange(nc) // chunk) * chunk, 0]]  # first vertex of the chunk's first cell
    p = (x[cells].astype(f) if absolute else (x[cells] - origin[:, None, :]).astype(f))  # [nc, 4, 3]
    J = (p[:, 1:, :] - p[:, :1, :]).transpose(0, 2, 1)  # J[a][al] = p_(al+1)[a] - p_0[a]
    C = np.empty_like(J)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            C[:, j, i] = J[:, i1, j1] * J[:, i2, j2] - J[:, i1, j2] * J[:, i2, j1]  # C = adj(J): K = C / det
    det = J[:, 0, 0] * C[:, 0, 0] + J[:, 0, 1] * C[:, 1, 0] + J[:, 0, 2] * C[:, 2, 0]
    assert det.dtype == f
    # grad phi_(al+1) = C[al][:] / det, grad phi_0 = -(their sum); A_ij = grad phi_i . grad phi_j |det| / 6
    Gr = np.concatenate([-(C.sum(axis=1, keepdims=True)), C], axis=1)  # [nc, 4, 3], times det
    ue = u.astype(f)[cell_dofs]
    t = np.einsum("cja,cj->ca", Gr, ue).astype(f) / (f(6.0) * np.abs(det))[:, None]
    ye = np.einsum("cia,ca->ci", Gr, t).astype(f)
    return scatter(cell_dofs, ye, bc, u.shape[0])


def cg_h(apply, b, dtype, kmax=100, rtol=1e-6):
    """src/cg.h:38-86 with U = dtype and x0 = 0; apply(p) returns y as doubles (rounded to dtype here).  Returns
    (k, x as double, history of <r,r> with history[0] = <r0,r0>)"""
    T = dtype
    dot = lambda a, c: T(np.dot(a.astype(np.float64), c.astype(np.float64)))
    x = np.zeros(b.shape[0], T)
    y = apply(x.astype(np.float64)).astype(T)
    r = b.astype(T) - y
    p = r.copy()
    rnorm0 = dot(r, r)
    rnorm = rnorm0
    hist = [float(rnorm0)]
    k = 0
    while k < kmax:
        k += 1
        y = apply(p.astype(np.float64)).astype(T)
        alpha = T(rnorm / dot(p, y))
        x = alpha * p + x
        r = -alpha * y + r
        rnorm_new = dot(r, r)
        beta = T(rnorm_new / rnorm)
        rnorm = rnorm_new
        hist.append(float(rnorm))
        if float(rnorm) / float(rnorm0) < rtol * rtol:
            break
        p = beta * p + r
    return k, x.astype(np.float64), np.array(hist)


@functools.lru_cache(maxsize=None)
def cube(order, dims):
    """the oracle's Poisson problem on a cube with its element matrices and right-hand side (computed once, shared)"""
    P = zo.Problem("poisson", order, *dims)
    b = zo.assemble_vector(0, order, P.x, P.cells, P.cell_dofs, P.f, P.g, P.facets, P.bc)
    return P, element_matrices(order, P.x, P.cells), b


@functools.lru_cache(maxsize=None)
def cg_pair(order, dims, kmax=100, rtol=1e-6):
    """cg.h in double and in float on one cube: ((k64, x64, hist64), (k32, x32, hist32))"""
    P, Ae, b = cube(order, dims)
    return tuple(cg_h(lambda v, T=T: action(Ae, P.cell_dofs, P.bc, v, T), b, T, kmax, rtol) for T in (np.float64, np.float32))


# the converging case of the GPU tests: P1 on the first cube of the family n x (n - 1) x (n + 1), n = 4, 6, 8, ... whose cg.h
# solve ends before 100 iterations in float and within +-2 of the double count (29 and 30 iterations here;
# tests/test_f32_ref.py checks it)
CONVERGING = (1, (4, 3, 5))
