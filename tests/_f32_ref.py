"""numpy float32 restatement of the single-precision cgpoisson path (zzz_action_f32, zzz_cg_solve_f32; the reference with
T = float at src/cgpoisson_problem.cpp:28 and U = float in src/cg.h:18-86).  It shares no code with the library.

Action.  y_e = float32(A_e) . float32(u_e) in float32, A_e from the oracle's `tabulate` in double; the element vectors are
scattered in double and the constrained rows zeroed.  For P1 there is a second form, `action32_p1_geometry`, that builds
the element geometry in float32 as a float kernel must: the vertex coordinates are first taken relative to an origin of
their chunk of cells (subtracted in double) and rounded; Jacobian, cofactors, determinant and the element vector are then
float32 arithmetic.  `absolute=True` rounds the absolute coordinates instead -- what the library must NOT do.  The chunks and
their origins can be given (`block`, `origin`), and the library's rule for the origin -- check every cell's float Jacobian
against the double one, take the better of it and a second origin past a bar, refuse the block past another -- is restated next to it (p1_block_origins).

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


def action32_p1_geometry(x, cells, cell_dofs, bc, u, chunk=2048, absolute=False, block=None, origin=None):
    """P1 with the geometry formed in float32 from block-relative coordinates.  block[c] = the block of cell c and
    origin[b] = the origin of block b; without them: chunks of `chunk` consecutive cells, each relative to the first vertex
    of its first cell.  A cell whose float determinant is 0 gives non-finite entries, as it does in a kernel."""
    f = np.float32
    nc = len(cells)
    if block is None:
        first = (np.arange(nc) // chunk) * chunk
        o = x[cells[first, 0]]  # first vertex of the chunk's first cell
    else:
        o = np.asarray(origin, np.float64)[np.asarray(block)]
    p = (x[cells].astype(f) if absolute else (x[cells] - o[:, None, :]).astype(f))  # [nc, 4, 3]
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
    with np.errstate(all="ignore"):
        t = np.einsum("cja,cj->ca", Gr, ue).astype(f) / (f(6.0) * np.abs(det))[:, None]
        ye = np.einsum("cia,ca->ci", Gr, t).astype(f)
    return scatter(cell_dofs, ye, bc, u.shape[0])


U32 = 2.0 ** -24


def figure32(y, y_ref, t_ref):
    """the per-entry figure of tests/_hp_ref.py (metric: max |y - y_ref| / scale, exact where the scale is 0) in units of
    2^-24; inf when an entry is not finite"""
    y, y_ref, t_ref = np.asarray(y, np.float64), np.asarray(y_ref), np.asarray(t_ref)
    if not np.isfinite(y).all():
        return float("inf")
    z = t_ref == 0
    assert np.array_equal(y[z], y_ref[z]), "an entry of scale 0 is not exact"
    return float((np.abs(y[~z] - y_ref[~z]) / t_ref[~z]).max() / U32) if not z.all() else 0.0


# ---- the rule that picks a block's origin, or refuses the block (csrc/zzz_mf_elem.h: mf_f32_cell_ok, MfF32Thin), restated --
JKEEP, JTOL, DET_MARGIN, DET_MIN, DET_MAX = 2.0 ** -16, 2.0 ** -12, 2.0 ** -18, 2.0 ** -100, 2.0 ** 100


def p1_cells(xc, o):
    """xc [n, 4, 3] vertex coordinates, o [3] origin -> (ok [n], jerr [n], ratio [n]).  jerr: the largest |J_float - J_double|
    over the entries of the Jacobian (float: differences of the rounded relative coordinates), each against the cell's extent
    along that axis.  ok: the float determinant DET_MARGIN of its terms' magnitudes away from zero, of the double one's sign
    and inside [DET_MIN, DET_MAX].  ratio: largest distance from the origin / extent over the axes."""
    f = np.float32
    o = np.broadcast_to(np.asarray(o, np.float64), (len(xc), 3))
    ext = xc.max(1) - xc.min(1)  # [n, 3]
    r = (xc - o[:, None, :]).astype(f)
    Jf = (r[:, 1:, :] - r[:, :1, :]).astype(np.float64)  # [n, al, a]
    Jd = xc[:, 1:, :] - xc[:, :1, :]
    with np.errstate(all="ignore"):
        jerr = np.where(ext > 0, np.abs(Jf - Jd).max(1) / ext, np.inf).max(1)
        ok = (ext > 0).all(1)
        ratio = np.where(ext > 0, np.abs(xc - o[:, None, :]).max(1) / ext, np.inf).max(1)

    def terms(J):  # J[n, al, a]: the three terms of det and of its magnitude
        d, m = 0.0, 0.0
        for al in range(3):
            b, c = (al + 1) % 3, (al + 2) % 3
            d = d + J[:, al, 0] * (J[:, b, 1] * J[:, c, 2] - J[:, c, 1] * J[:, b, 2])
            m = m + np.abs(J[:, al, 0]) * (np.abs(J[:, b, 1] * J[:, c, 2]) + np.abs(J[:, c, 1] * J[:, b, 2]))
        return d, m

    det, mag = terms(Jf)
    detd, _ = terms(Jd)
    ok &= (np.abs(det) >= DET_MARGIN * mag) & (np.abs(det) >= DET_MIN) & (np.abs(det) <= DET_MAX) & ((det > 0) == (detd > 0))
    return ok, jerr, ratio


def p1_second_origin(xc):
    """the second origin of a block with cells xc [n, 4, 3]: along every axis the lowest coordinate among the cells whose
    extent along that axis is within a factor 2 of the block's least"""
    lo, ext = xc.min(1), xc.max(1) - xc.min(1)
    return np.array([lo[ext[:, a] <= 2.0 * ext[:, a].min(), a].min() for a in range(3)])


def p1_block_origins(x, cells, block, first):
    """(origin [nb, 3], status [nb], jerr [nb]) of the rule.  first[b] stays the origin of block b while every cell is ok and
    within JKEEP; past it the better of first[b] and the second origin is taken (status 1: the second); status 2 -- neither
    is ok and within JTOL: the float action is refused.  jerr: the chosen origin's largest Jacobian error"""
    xc = x[cells]
    nb = int(block.max()) + 1
    origin, status, jerr = np.array(first, np.float64).copy(), np.zeros(nb, np.int64), np.zeros(nb)
    for b in range(nb):
        xb = xc[block == b]
        ok0, j0, _ = p1_cells(xb, origin[b])
        ok0, j0 = ok0.all(), j0.max()
        jerr[b] = j0
        if ok0 and j0 <= JKEEP:
            continue
        o1 = p1_second_origin(xb)
        ok1, j1, _ = p1_cells(xb, o1)
        ok1, j1 = ok1.all(), j1.max()
        c0, c1 = ok0 and j0 <= JTOL, ok1 and j1 <= JTOL
        if c1 and (not c0 or j1 < j0):
            origin[b], status[b], jerr[b] = o1, 1, j1
        elif not c0:
            status[b], jerr[b] = 2, min(j0, j1)
    return origin, status, jerr


def first_listed_dof(cell_dofs, block, rank=None):
    """the dof a block lists first (csrc/zzz_matfree.hip: dofs interior to the block, then those shared with other blocks,
    each ascending in the library's internal numbering): [nb] caller dof ids.  rank[d] = internal number of caller dof d
    (identity when the library kept the caller's order)"""
    nb = int(block.max()) + 1
    n = int(cell_dofs.max()) + 1
    rank = np.arange(n) if rank is None else np.asarray(rank)
    touch = np.zeros((nb, n), bool)
    touch[np.repeat(block, cell_dofs.shape[1]), cell_dofs.reshape(-1)] = True
    shared = touch.sum(0) > 1
    out = np.empty(nb, np.int64)
    for b in range(nb):
        d = np.nonzero(touch[b])[0]
        key = shared[d].astype(np.int64) * n + rank[d]
        out[b] = d[np.argmin(key)]
    return out


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
