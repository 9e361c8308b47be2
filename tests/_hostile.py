"""Hostile geometries for the parity tests: TEST INFRASTRUCTURE ONLY.

The base is the oracle's cube (zo.Problem): mesh, dofmap, Dirichlet set, coefficients, exterior facets.  Vertices, dofs
and cells are shuffled with a fixed seed, so that the library's internal orders have something to undo; a case then maps
the vertex coordinates and leaves everything else alone (Dirichlet set, facets and coefficients are inputs).  Every case
is a valid mesh: the maps are injective and no cell degenerates.

reference(case) is the one mp pass per (case, order, problem) that the matrix, vector, action, diagonal and lifting tests
share (tests/_hp_ref.py), with the oracle's values on the same input next to it.
"""
import numpy as np

import _hp_ref as hp
import zzz_oracle as zo

BASE = {1: (6, 5, 5), 2: (4, 4, 5), 3: (3, 3, 4)}
# elasticity costs nine times the mp work per pair of nodes: smaller P2 / P3 bases (88 911 and 164 574 nonzeros -- still dozens
# of assembly tiles, a padded window block, interior vertices and both constrained faces)
ELASTICITY_BASE = {1: (6, 5, 5), 2: (3, 3, 4), 3: (2, 2, 3)}
SEED = 20240611


def _rotation():
    """a fixed generic rotation: angle 0.7 about (1, 2, 3) (Rodrigues)"""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(0.7) * Kx + (1 - np.cos(0.7)) * Kx @ Kx


def _shear50(x, xi):
    y = x.copy()
    y[:, 0] += 50.0 * x[:, 1]
    return y


def _mirror(x, xi):
    y = x.copy()
    y[:, 0] = 1.0 - x[:, 0]
    return y


# name -> (map(x, xi) -> x', dims of the P1 base when they are not BASE[1])
MAPS = {
    "identity": (lambda x, xi: x.copy(), None),
    "offset": (lambda x, xi: x + np.array([1024.0, -4096.0, 65536.0]), None),
    "aniso": (lambda x, xi: x * np.array([2.0 ** 20, 1.0, 2.0 ** -20]), None),
    "needle": (lambda x, xi: x * np.array([1.0, 2.0 ** -12, 2.0 ** -12]), None),
    "needle_line": (lambda x, xi: x * np.array([1.0, 2.0 ** -12, 2.0 ** -12]), (30, 1, 1)),
    "graded": (lambda x, xi: x ** 3, None),
    "graded_corner": (lambda x, xi: x ** 6, (12, 10, 10)),
    "graded_corner_16": (lambda x, xi: x ** 8, (16, 14, 14)),  # the one whose default plan has to halve its blocks
    "mirror": (_mirror, None),
    "mirror_axes": (lambda x, xi: np.ascontiguousarray(_mirror(x, xi)[:, [2, 0, 1]]), None),
    "noise13": (lambda x, xi: x * (1.0 + 1e-13 * xi), None),
    "noise10": (lambda x, xi: x + 3e-10 * xi, None),
    "noise7": (lambda x, xi: x + 1e-7 * xi, None),
    "rotated": (lambda x, xi: x @ _rotation().T, None),
    "shear50_a": (_shear50, None),          # ny = 5: (nx+1)(ny+1) x (ny+1) x (nz+1) lines <= 8 nv -- passes for a lattice
    "shear50_b": (_shear50, (6, 9, 5)),     # ny = 9: ny + 1 > 8 -- a point cloud
}
P1_CASES = list(MAPS)
# P1 cases of the float action alone (tests/test_gpu_f32_hostile.py): small meshes graded so steeply that float coordinates
# relative to a badly placed block origin collapse cells to det J == 0 -- x^12 towards the low corner, 1 - (1 - x)^8 towards
# the far one (where no min-corner origin helps).  Not in MAPS: the parametrisations of the double tests stay as they are.
F32_P1_EXTRA = ["graded12", "graded_far8"]


def _both_ends12(x, xi):
    t = 2.0 * x - 1.0
    return 0.5 * (1.0 + np.sign(t) * (1.0 - (1.0 - np.abs(t)) ** 12))


F32_MAPS = {
    "graded12": (lambda x, xi: x ** 12, (6, 5, 5)),
    "graded_far8": (lambda x, xi: 1.0 - (1.0 - x) ** 8, (8, 6, 6)),
    # graded towards BOTH ends of every axis: one block of the default plan holds cells of 1e-6 at 0 and at 1 and no single
    # origin resolves both -- the float action must refuse it (blocks of 128 cells hold one corner each and are served)
    "graded_ends12": (_both_ends12, (6, 5, 5)),
}
F32_P1_REFUSED = "graded_ends12"
P2_CASES = ["aniso", "graded", "mirror", "shear50_a", "noise10"]
P3_CASES = ["offset", "graded", "mirror", "shear50_a"]
POISSON_CASES = [(n, 1) for n in P1_CASES] + [(n, 2) for n in P2_CASES] + [(n, 3) for n in P3_CASES]
ELASTICITY_P1_ORACLE_CASES = ["offset", "aniso", "mirror", "shear50_a", "noise10"]  # (judged against the oracle alone)
# elasticity against the 50-digit reference, per order (tests/test_gpu_hostile_elasticity.py)
ELASTICITY_CASES = {1: ["identity", "offset", "aniso", "needle", "graded", "mirror", "noise10", "noise7", "rotated", "shear50_a",
                        "shear50_b"],
                    2: ["aniso", "graded", "mirror", "rotated", "shear50_a", "noise10"],
                    3: ["offset", "graded", "rotated", "shear50_a"]}
ELASTICITY_SOLVE_CASES = ("identity", "offset", "graded", "mirror", "noise10", "noise7", "rotated")
# the lifting pass (Dirichlet values): (name, order) per problem
LIFTING_CASES = {"poisson": [("offset", 1), ("aniso", 1), ("graded", 1), ("rotated", 1), ("shear50_a", 1), ("graded", 2), ("offset", 3)],
                 "elasticity": [("aniso", 1), ("rotated", 1), ("shear50_a", 1), ("aniso", 2), ("graded", 3)]}
SOLVE_CASES = ("identity", "offset", "graded", "mirror", "mirror_axes", "noise13", "noise10", "noise7", "rotated")
# the kind of internal order the code fixes for a case (1: lattice, 0: the caller's, or 2 when the bins are asked for)
KIND_LATTICE = ("identity", "offset", "aniso", "needle", "needle_line", "graded", "graded_corner", "graded_corner_16", "noise13")
KIND_CLOUD = ("noise7", "rotated")


class Case:
    pass


_CASES = {}


def case(name, order, problem="poisson", dims=None):
    """dims: a base of the caller's own instead of the map's or the table's (it enters the keys of _CASES and of the mp pass)"""
    key = (name, order, problem) if dims is None else (name, order, problem, tuple(dims))
    if key in _CASES:
        return _CASES[key]
    fmap, own = MAPS[name] if name in MAPS else F32_MAPS[name]
    if dims is not None:
        dims = tuple(dims)
    else:
        dims = own if (own is not None and order == 1) else (ELASTICITY_BASE if problem == "elasticity" else BASE)[order]
    zo.set_num_threads(1)
    O = zo.Problem(problem, order, *dims)
    rng = np.random.default_rng(SEED + 97 * order)
    nv, nb, nc = O.x.shape[0], O.nblock, O.cells.shape[0]
    pv, pd, pc = rng.permutation(nv), rng.permutation(nb), rng.permutation(nc)
    xi = rng.standard_normal(O.x.shape)
    C = Case()
    C.name, C.order, C.problem, C.dims, C.bs, C.form, C.nblock = name, order, problem, dims, O.bs, O.form, nb
    C.n = nb * O.bs
    C.key = key
    x0 = np.zeros_like(O.x)
    x0[pv] = O.x  # vertex v is now called pv[v]
    C.x_base = x0
    C.x = np.ascontiguousarray(fmap(x0, xi), dtype=np.float64)
    C.cells = np.ascontiguousarray(pv[O.cells][pc].astype(np.int32))
    C.cell_dofs = np.ascontiguousarray(pd[O.cell_dofs][pc].astype(np.int32))
    sd = (pd[:, None] * O.bs + np.arange(O.bs)).reshape(-1)  # scalar dof d is now called sd[d]
    C.bc = np.zeros_like(O.bc)
    C.bc[sd] = O.bc
    C.f = np.zeros_like(O.f)
    C.f[sd] = O.f
    if problem == "poisson":
        C.g = np.zeros_like(O.g)
        C.g[sd] = O.g
        C.facets = zo.exterior_facets(C.cells)
    else:
        C.g, C.facets = None, None
    dof_x = np.zeros_like(O.dof_x)
    dof_x[pd] = O.dof_x
    C.dof_x_base = dof_x
    C.rowptr, C.cols = zo.pattern(nb, C.cell_dofs, O.bs)
    _CASES[key] = C
    return C


def oracle(C):
    """the oracle's A and b on the case's input (one thread: the serial sums)"""
    if not hasattr(C, "ov"):
        zo.set_num_threads(1)
        C.ov = zo.assemble_matrix(C.form, C.order, C.x, C.cells, C.cell_dofs, C.bc, C.rowptr, C.cols)
        C.ob = zo.assemble_vector(C.form, C.order, C.x, C.cells, C.cell_dofs, C.f, C.g, C.facets, C.bc)
    return C.ov, C.ob


def reference(C):
    """dict of the mp pass of a case: R, S (unconstrained), Rc, Sc (Dirichlet rows and columns applied), r, s (b,
    constrained entries exactly zero), r_unc, s_unc (b with nothing constrained), the oracle's unconstrained matrix ou and
    vector ob_unc, and the oracle's figures against the reference"""
    key = getattr(C, "key", (C.name, C.order, C.problem))  # ((name, order, problem), and the dims where the caller chose them)
    if key in hp.CACHE:
        return hp.CACHE[key]
    if C.problem == "poisson":
        R, S = hp.matrix(C.order, C.x, C.cells, C.cell_dofs, C.rowptr, C.cols)
        r, s = hp.vector(C.order, C.x, C.cells, C.cell_dofs, C.f, C.g, C.facets, C.n)
    else:
        R, S = hp.elasticity_matrix(C.order, C.x, C.cells, C.cell_dofs, C.rowptr, C.cols)
        r, s = hp.elasticity_vector(C.order, C.x, C.cells, C.cell_dofs, C.f, C.n)
    r_unc, s_unc = r.copy(), s.copy()
    bcb = C.bc.astype(bool)
    r[bcb] = 0.0
    s[bcb] = 0.0
    Rc, Sc = hp.dirichlet(R, S, C.rowptr, C.cols, C.bc)
    zo.set_num_threads(1)
    ou = zo.assemble_matrix(C.form, C.order, C.x, C.cells, C.cell_dofs, np.zeros_like(C.bc), C.rowptr, C.cols)
    ob_unc = zo.assemble_vector(C.form, C.order, C.x, C.cells, C.cell_dofs, C.f, C.g, C.facets, np.zeros_like(C.bc))
    ov, ob = oracle(C)
    ref = dict(R=R, S=S, Rc=Rc, Sc=Sc, r=r, s=s, r_unc=r_unc, s_unc=s_unc, ou=ou, ob_unc=ob_unc,
               oracle_A_free=hp.metric(ou, R, S) / hp.U, oracle_A=hp.metric(ov, Rc, Sc) / hp.U,
               oracle_b=hp.metric(ob, r, s) / hp.U, oracle_b_free=hp.metric(ob_unc, r_unc, s_unc) / hp.U)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    hp.CACHE[key] = ref
    return ref


def lifted_reference(C, g):
    """(r, s, the oracle's figure) of the vector with the Dirichlet values g lifted (g is read on the Dirichlet set alone):
        free rows          r_i = r_unc_i - sum_(j in bc) R_ij g_j   (products and sums in long double, rounded once)
                           s_i = s_unc_i + sum_(j in bc) S_ij |g_j|
        constrained rows   r_i = g_i exactly, s_i = 0
    and the oracle's unconstrained A and b lifted the same way in doubles"""
    ref = reference(C)
    bcb = C.bc.astype(bool)
    gm = np.where(bcb, g, 0.0)  # (g may hold NaN off the Dirichlet set: never multiplied)
    rows = C.rowptr[:-1]
    assert np.all(np.diff(C.rowptr) > 0)
    lift = np.add.reduceat(ref["R"].astype(np.longdouble) * gm[C.cols].astype(np.longdouble), rows)
    r = (ref["r_unc"].astype(np.longdouble) - lift).astype(np.float64)
    s = ref["s_unc"] + np.add.reduceat(ref["S"] * np.abs(gm[C.cols]), rows)
    r[bcb] = g[bcb]
    s[bcb] = 0.0
    ro = ref["ob_unc"] - np.add.reduceat(ref["ou"] * gm[C.cols], rows)
    ro[bcb] = g[bcb]
    return r, s, hp.metric(ro, r, s) / hp.U


def dof_coords(C):
    """The coordinates of the block dofs of a mapped case: the affine image of the reference nodes in each MAPPED cell (what
    a Pk space on the mapped mesh has), not the map applied to the base dof coordinates -- on a graded mesh the two differ"""
    X = zo.ref_nodes(C.order)
    xs = C.x[C.cells]  # [cell][vertex][a]
    e = xs[:, 1:, :] - xs[:, :1, :]
    pts = xs[:, :1, :] + np.einsum("ia,cab->cib", X, e)
    out = np.zeros((C.nblock, 3))
    out[C.cell_dofs] = pts
    return out


def action_reference(C, u):
    """(y, t, the oracle's figure) of y = A_unconstrained u, y[bc] = 0 (the matrix-free operator of cgpoisson)"""
    ref = reference(C)
    y, t = hp.apply(ref["R"], ref["S"], C.rowptr, C.cols, u)
    bcb = C.bc.astype(bool)
    y[bcb] = 0.0
    t[bcb] = 0.0
    oy = zo.action_poisson(C.order, C.x, C.cells, C.cell_dofs, C.bc, u)
    return y, t, hp.metric(oy, y, t) / hp.U


def diagonal_reference(C):
    """(d, scale, the oracle's figure): the diagonal of the constrained matrix, 1.0 exactly on constrained rows"""
    ref = reference(C)
    d, sd = hp.diagonal(ref["Rc"], ref["Sc"], C.rowptr, C.cols)
    od, _ = hp.diagonal(oracle(C)[0], ref["Sc"], C.rowptr, C.cols)
    return d, sd, hp.metric(od, d, sd) / hp.U


def plan_cell_order(C):
    """The order in which the matrix-free plan (csrc/zzz_matfree.hip, plan_attempt) cuts the cells into blocks, restated:
    centroids in 1024 bins of ONE resolution taken from the longest extent, bit-interleaved (x lowest), stable sort of the
    cells in the caller's order.  Exact when the library keeps the caller's cell order."""
    def spread(q):
        r = np.zeros_like(q)
        for b in range(10):
            r |= ((q >> b) & 1) << (3 * b)
        return r
    lo, hi = C.x.min(0), C.x.max(0)
    sc = (1024.0 / (hi - lo)).min()
    xs = C.x[C.cells]
    m = 0.25 * (xs[:, 0] + xs[:, 1] + xs[:, 2] + xs[:, 3])
    q = np.clip(((m - lo) * sc).astype(np.int64), 0, 1023)
    key = spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
    return np.argsort(key, kind="stable")


def plan_cell_blocks(C, nc):
    """The block of every cell: consecutive runs of nc cells of plan_cell_order"""
    o = plan_cell_order(C)
    blk = np.empty(len(o), np.int64)
    blk[o] = np.arange(len(o)) // nc
    return blk


def plan_blocks(C, nc):
    """The dofs that each block of nc cells of the matrix-free plan touches"""
    blk = plan_cell_blocks(C, nc)
    return [len(np.unique(C.cell_dofs[blk == b])) for b in range(int(blk.max()) + 1)]
