"""Connectivities that sit ON the capacity limits of the pattern build (csrc/zzz_pattern.hip, build_adjT in
csrc/zzz_assemble.hip) and one unit past them, each with a `claim`: the quantities the build branches on, restated in
numpy, and the path through the build that follows from them.  CPU only; tests/test_pattern_sets.py proves every claim by
an independent count, tests/test_gpu_pattern_edges.py requires the library to report the claimed path (zzz_pattern_info).

The limits as the code has them (test_pattern_sets.py reads them out of the sources and compares):

  ADJ_MAX_RUNS   512  (monotone block, local index) pairs the sort-free adjacency takes; beyond: radix sort from the start
  ADJ_BREAK_CAP 4096  break records adjacency_find_runs collects before it gives up
  ADJ_CAP       7168  incidences a window of ADJ_W = 256 dofs holds in LDS; beyond: flag, filler, second build with the sort
  ROW_T_CAP    16, 32 unique block columns of a row in k_row_pattern_thread4 (P1); beyond 32: a wavefront per row
  ROW_T_ADJ     4096  adjacency entries of a block of ROW_T_BLOCK = 128 rows in that kernel; beyond: a wavefront per row
  64 .. 512           candidates (cells x nd) of a row sorted in registers by k_row_pattern: P = 64, 128, 256, 512
  PAT_CAP       1024  candidates sorted in LDS; beyond: ZZZ_ERR_LIMIT inside, the host builder outside
  tiles               the longest scalar row must fit twice into SPMV_TILE_NNZ - 2 = 2046 and the bs rows of a block twice
                      into the assembly tile: scalar P1 min(1023, 1920 / 2) = 960 columns, elasticity P1
                      min(2046 / 6, 8704 / 18) = 341 block columns
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "performance-test_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import zzz  # noqa: E402
import zzz_oracle as zo  # noqa: E402

ADJ_W, ADJ_CAP, ADJ_MAX_RUNS, ADJ_BREAK_CAP = 256, 7168, 512, 4096
ROW_T_BLOCK, ROW_T_ADJ, ROW_T_CAPS = 128, 4096, (16, 32)
REG_CAPS, PAT_CAP = (64, 128, 256, 512), 1024
SPMV_TILE_NNZ = 2048
ASM_TILE_NNZ = {(1, 1): 1920, (1, 3): 8704}  # (order, bs): asm_tile_nnz of the P1 kernels
THETA = 0.5  # the fan's angle between neighbouring ring vertices
FAN_SHAPE_BOUND = 0.4  # smallest |det J| over the largest, every k: radii in [1, 1.5), so >= 1 / 1.5^2 = 0.444


def tile_limit(order, bs):
    """most unique block columns of a row that build_tiles_device accepts: Ws = SPMV_TILE_NNZ - maxrow - 2 >= maxrow and
    Wa = asm_tile_nnz - maxblock >= maxblock with maxrow = bs c, maxblock = bs^2 c"""
    return min((SPMV_TILE_NNZ - 2) // (2 * bs), ASM_TILE_NNZ[(order, bs)] // (2 * bs * bs))


# ---- the quantities the build branches on, in numpy ---------------------------------------------------------------------
def measure(cell_dofs, n_owned):
    cd = np.asarray(cell_dofs, np.int64)
    nc, nd = cd.shape
    # k_run_breaks: a record per (cell, local index) whose dof does not grow; adjacency_find_runs cuts at every such cell
    brk = cd[1:] <= cd[:-1]
    records = int(brk.sum())
    blocks = int(brk.any(axis=1).sum()) + 1
    runs = blocks * nd
    nwin = (n_owned + ADJ_W - 1) // ADJ_W
    # a window's incidences are counted between the bounds of ITS keys: the last one's also hold the ghost keys below nwin * 256
    win = np.bincount(cd.ravel() // ADJ_W, minlength=nwin)[:nwin]
    owned = cd.ravel()[cd.ravel() < n_owned]
    val = np.bincount(owned, minlength=n_owned)
    blk = np.add.reduceat(val, np.arange(0, n_owned, ROW_T_BLOCK))
    rows = np.repeat(cd, nd, axis=1).ravel()
    cols = np.tile(cd, (1, nd)).ravel()
    keep = rows < n_owned
    ncol = int(cd.max()) + 1
    uniq = np.unique(rows[keep] * ncol + cols[keep])
    ucols = np.bincount(uniq // ncol, minlength=n_owned)
    return dict(nd=nd, blocks=blocks, break_records=records, runs=runs, window_max=int(win.max()), block_adj_max=int(blk.max()),
                cand_max=int(val.max()) * nd, cols_max=int(ucols.max()))


def predict(m, order, bs):
    """the path that follows from the measured quantities (what zzz_pattern_info must report with ZZZ_RENUMBER=0)"""
    nd = m["nd"]
    by_runs = m["break_records"] <= ADJ_BREAK_CAP and m["runs"] <= ADJ_MAX_RUNS
    adjacency = (1 if m["window_max"] <= ADJ_CAP else 3) if by_runs else 2
    row_kernel = 0
    if nd == 4 and m["block_adj_max"] <= ROW_T_ADJ:
        row_kernel = 16 if m["cols_max"] <= 16 else (32 if m["cols_max"] <= 32 else 0)
    host = m["cand_max"] > PAT_CAP
    p = dict(adjacency=0 if host else adjacency, runs=m["runs"] if adjacency == 1 and not host else 0,
             row_kernel=-1 if host else row_kernel, builder=1 if host else 0, max_cols=m["cols_max"],
             adj_source=1 if row_kernel and not host else 0,
             have_asm_pos=1 if nd > 4 and not host and m["cand_max"] <= REG_CAPS[-1] else 0)
    # the second build of the same dofmap: an overflow is remembered
    p["adjacency_again"] = 2 if p["adjacency"] == 3 else p["adjacency"]
    p["refused"] = order == 1 and m["cols_max"] > tile_limit(order, bs)
    # which sort of k_row_pattern the longest row takes (0: none runs, the thread kernel served every row)
    p["sort"] = 0 if (row_kernel or host) else next((c for c in REG_CAPS + (PAT_CAP,) if m["cand_max"] <= c))
    return p


# ---- generators -----------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, problem, order, x, cells, cell_dofs, n_owned, n_ghost, bc_dofs, facets, f, g, limit=None, synthetic=True):
        self.name, self.problem, self.order = name, problem, order
        self.bs = 3 if problem == "elasticity" else 1
        self.form = zzz.FORM_ELASTICITY if self.bs == 3 else zzz.FORM_POISSON
        self.x = np.ascontiguousarray(x, np.float64)
        self.cells = np.ascontiguousarray(cells, np.int32)
        self.cell_dofs = np.ascontiguousarray(cell_dofs, np.int32)
        self.n_owned, self.n_ghost = int(n_owned), int(n_ghost)
        self.bc_dofs = np.ascontiguousarray(bc_dofs, np.int32)
        self.facets = np.ascontiguousarray(facets, np.int32).reshape(-1, 2)
        self.f, self.g = f, g
        self.limit = limit  # (quantity, value the case must have as its maximum) or None
        self.synthetic = synthetic  # a fan or repeated cells: the bar for A and b is measured against the 50-digit reference
        self.claim = measure(self.cell_dofs, self.n_owned)
        self.path = predict(self.claim, order, self.bs)

    def bc_marker(self):
        m = np.zeros((self.n_owned + self.n_ghost) * self.bs, np.uint8)
        m[self.bc_dofs] = 1
        return m


def _coeffs(dof_x, bs):
    X = np.asarray(dof_x)
    f = 1.0 + 0.5 * np.sin(3.0 * X[:, 0]) + 0.25 * X[:, 1] * X[:, 2]
    if bs == 3:
        return np.ascontiguousarray(np.column_stack([f, 0.5 - 0.25 * X[:, 0], np.cos(2.0 * X[:, 1])]).reshape(-1)), None
    return f, np.cos(2.0 * X[:, 0]) - 0.5 * X[:, 2]


def fan_mesh(k):
    """k tetrahedra around the edge v0 = (0, 0, 0), v1 = (0, 0, 1): ring vertex i at angle i THETA, its radius in [1, 1.5) and
    its height in [0.25, 0.75) by two irrational rotations of i -- all vertices distinct (i THETA mod 2 pi never repeats)
    and |det J| = r_i r_(i+1) sin THETA whatever k is.  Vertices: v0, v1, ring 0 .. k; cell i = (v0, v1, ring i, ring i + 1)"""
    i = np.arange(k + 1)
    r = 1.0 + 0.5 * np.mod(i * 0.6180339887498949, 1.0)
    z = 0.25 + 0.5 * np.mod(i * 0.7548776662466927, 1.0)
    ring = np.column_stack([r * np.cos(i * THETA), r * np.sin(i * THETA), z])
    x = np.vstack([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], ring])
    c = np.arange(k)
    cells = np.column_stack([np.zeros(k, np.int64), np.ones(k, np.int64), 2 + c, 3 + c]).astype(np.int32)
    return x, cells


def fan_shape(k):
    x, cells = fan_mesh(k)
    p = x[cells]
    det = np.abs(np.linalg.det(p[:, 1:] - p[:, :1]))
    return float(det.min() / det.max())


def fan(name, problem, k, limit=None):
    """P1 on the fan: the rows of v0 and v1 have k + 3 unique columns and 4 k candidates.  Three ring vertices are
    constrained (they and the axis are not coplanar: A is SPD for Poisson and for elasticity)"""
    x, cells = fan_mesh(k)
    bs = 3 if problem == "elasticity" else 1
    n = k + 3
    nodes = np.array(sorted({2, 2 + k // 2, 2 + k}))
    bc = (nodes[:, None] * bs + np.arange(bs)).reshape(-1)
    f, g = _coeffs(x, bs)
    return Case(name, problem, 1, x, cells, cells, n, 0, bc, zo.exterior_facets(cells), f, g, limit)


def _from_part(name, P, cells=None, cell_dofs=None, limit=None, synthetic=False):
    return Case(name, P.problem, P.order, P.x, P.cells if cells is None else cells, P.cell_dofs if cell_dofs is None else cell_dofs,
                P.n_owned, P.n_ghost, P.bc_dofs, P.facets, P.f, P.g, limit, synthetic)


def lattice(name, problem, order, dims, nparts=1, part=0):
    return _from_part(name, zzz.Part(problem, order, *dims, nparts, part))


def _repeat(weights, target, whole):
    """cells to append so that sum(weights) reaches `target` exactly: rounds in ascending cell order (each one more
    monotone block where the lattice's own order is one), first of the cells with weight `whole` while they fit, then one
    of any cell whose weight still fits"""
    w = np.asarray(weights, np.int64)
    total, extra = int(w.sum()), []
    assert total <= target
    full = np.nonzero(w == whole)[0]
    while target - total >= whole and full.size:
        take = full[: (target - total) // whole]
        extra.extend(take.tolist())
        total += whole * len(take)
    for c in np.nonzero(w > 0)[0]:
        if 0 < w[c] <= target - total:
            extra.append(int(c))
            total += int(w[c])
    assert total == target, (total, target)
    return np.array(extra, np.int64)


def lattice_repeats(name, problem, order, dims, quantity, target, limit):
    """a lattice with chosen cells appended again until a row (quantity 'cand': candidates of the dof of highest valence and
    lowest number), window 0 ('window') or block 0 of 128 rows ('block_adj') reaches `target`; no column is added"""
    P = zzz.Part(problem, order, *dims)
    cd = P.cell_dofs.astype(np.int64)
    if quantity == "cand":
        val = np.bincount(cd.ravel(), minlength=P.n_owned)
        r = int(np.argmax(val))
        assert target % P.nd == 0
        extra = _repeat((cd == r).any(axis=1), target // P.nd, 1)
    elif quantity == "window":
        extra = _repeat((cd < ADJ_W).sum(axis=1), target, P.nd)
    else:
        extra = _repeat((cd < ROW_T_BLOCK).sum(axis=1), target, P.nd)
    idx = np.concatenate([np.arange(P.ncells), extra])
    return _from_part(name, P, P.cells[idx], P.cell_dofs[idx], limit, synthetic=True)


def tet_repeats(name, order, m, limit):
    """ONE tetrahedron listed m times (the smallest mesh there is: 20 m candidates per row at P3)"""
    x = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.1], [0.1, 0.2, 1.1]])
    cells1 = np.array([[0, 1, 2, 3]], np.int32)
    n, cd1, dof_x, _ = zo.build_dofmap(order, x, cells1)
    idx = np.zeros(m, np.int64)
    f, g = _coeffs(dof_x, 1)
    return Case(name, "poisson", order, x, cells1[idx], cd1[idx], n, 0, np.array([0, 1, 2], np.int32), zo.exterior_facets(cells1), f, g, limit)


def lattice_reversed(name, problem, order, dims, nblocks, limit):
    """the lattice's cells cut into pieces that are listed in reverse: exactly `nblocks` monotone blocks.  The cuts the
    lattice's own order has (one per simplex type) stay and the others are spread evenly over the cells between them;
    a junction of the reversed list can happen to ascend (the first piece of one simplex type is followed by the last piece
    of the type before it), so cuts are added until the count, measured, is the one asked for"""
    P = zzz.Part(problem, order, *dims)
    cd = P.cell_dofs.astype(np.int64)
    own = np.nonzero((cd[1:] <= cd[:-1]).any(axis=1))[0] + 1
    free = np.setdiff1d(np.arange(1, P.ncells), own)
    for need in range(max(nblocks - 1 - own.size, 0), free.size + 1):
        cuts = np.unique(np.concatenate([own, free[np.linspace(0, free.size - 1, need).round().astype(np.int64)]]))
        idx = np.concatenate(np.split(np.arange(P.ncells), cuts)[::-1])
        if measure(P.cell_dofs[idx], P.n_owned)["blocks"] == nblocks:
            break
    else:
        raise AssertionError((name, nblocks))
    inv = np.argsort(idx)
    C = _from_part(name, P, P.cells[idx], P.cell_dofs[idx], limit)
    C.facets = np.ascontiguousarray(np.column_stack([inv[P.facets[:, 0]], P.facets[:, 1]]).astype(np.int32))
    return C


def lattice_plus_cone(name, dims):
    """a P1 lattice and one more tetrahedron on its first exterior facet, with a new vertex: one dof more than a lattice has"""
    P = zzz.Part("poisson", 1, *dims)
    c, lf = (int(v) for v in P.facets[0])
    face = [v for j, v in enumerate(P.cells[c]) if j != lf]
    apex = P.x[face].mean(axis=0) + (P.x[face].mean(axis=0) - P.x[P.cells[c][lf]])
    x = np.vstack([P.x, apex])
    cells = np.vstack([P.cells, [face + [P.nverts]]]).astype(np.int32)
    f, g = _coeffs(x, 1)
    f[: P.nverts], g[: P.nverts] = P.f, P.g
    facets = zo.exterior_facets(cells)
    return Case(name, "poisson", 1, x, cells, cells, P.n_owned + 1, 0, P.bc_dofs, facets, f, g, None, synthetic=False)


# ---- the table: name -> builder, from the smallest upward --------------------------------------------------------------
def _nd_floor(v, nd):
    return v // nd * nd


def _table():
    T = {}

    def add(name, fn, *a, **kw):
        T[name] = functools.partial(fn, name, *a, **kw)

    # P3 60 | 80 candidates: one tetrahedron three and four times
    add("p3_tet_cand_60", tet_repeats, 3, 3, ("cand_max", 60))
    add("p3_tet_cand_80", tet_repeats, 3, 4, ("cand_max", 80))
    # P1 fans: unique columns 16 | 17 and 32 | 33 (the thread kernel's caps), candidates either side of every sort size
    for k, lim in ((13, ("cols_max", 16)), (14, ("cols_max", 17)), (16, ("cand_max", 64)), (17, ("cand_max", 68)),
                   (29, ("cols_max", 32)), (30, ("cols_max", 33)), (32, ("cand_max", 128)), (33, ("cand_max", 132)),
                   (64, ("cand_max", 256)), (65, ("cand_max", 260)), (128, ("cand_max", 512)), (129, ("cand_max", 516)),
                   (256, ("cand_max", 1024)), (257, ("cand_max", 1028))):
        add(f"fan_{k}", fan, "poisson", k, lim)
    for k, lim in ((13, ("cols_max", 16)), (14, ("cols_max", 17)), (29, ("cols_max", 32)), (30, ("cols_max", 33))):
        add(f"fan3_{k}", fan, "elasticity", k, lim)
    # P2 / P3 candidates by repeats on the 1 x 1 x 1 lattice (six cells around the main diagonal: 60 / 120 candidates as it is)
    for cap in REG_CAPS + (PAT_CAP,):
        v = _nd_floor(cap, 10)
        add(f"p2_cand_{v}", lattice_repeats, "poisson", 2, (1, 1, 1), "cand", v, ("cand_max", v))
        add(f"p2_cand_{v + 10}", lattice_repeats, "poisson", 2, (1, 1, 1), "cand", v + 10, ("cand_max", v + 10))
    for cap in REG_CAPS[1:] + (PAT_CAP,):
        v = _nd_floor(cap, 20)
        add(f"p3_cand_{v}", lattice_repeats, "poisson", 3, (1, 1, 1), "cand", v, ("cand_max", v))
        add(f"p3_cand_{v + 20}", lattice_repeats, "poisson", 3, (1, 1, 1), "cand", v + 20, ("cand_max", v + 20))
    # n_owned either side of the window of 256 dofs, and on it with and without ghost keys behind
    add("lattice_255", lattice, "poisson", 1, (2, 4, 16))
    add("lattice_256", lattice, "poisson", 1, (7, 7, 3))
    add("lattice_257", lattice_plus_cone, (7, 7, 3))
    add("lattice_512", lattice, "poisson", 1, (7, 7, 7))
    add("part_256_and_ghosts", lattice, "poisson", 1, (7, 7, 7), 2, 0)
    add("part_ghosts_in_last_window", lattice, "poisson", 1, (5, 6, 9), 2, 0)
    # runs: 512 | more
    add("p1_blocks_128", lattice_reversed, "poisson", 1, (5, 4, 4), 128, ("runs", 512))
    add("p1_blocks_129", lattice_reversed, "poisson", 1, (5, 4, 4), 129, ("runs", 516))
    add("p2_blocks_51", lattice_reversed, "poisson", 2, (3, 3, 3), 51, ("runs", 510))
    add("p2_blocks_52", lattice_reversed, "poisson", 2, (3, 3, 3), 52, ("runs", 520))
    # the tile limits, scalar and elasticity: the longest row the tiles take, and one column more (refused)
    add("fan3_338", fan, "elasticity", tile_limit(1, 3) - 3, ("cols_max", tile_limit(1, 3)))
    add("fan3_339", fan, "elasticity", tile_limit(1, 3) - 2, ("cols_max", tile_limit(1, 3) + 1))
    add("fan_957", fan, "poisson", tile_limit(1, 1) - 3, ("cols_max", tile_limit(1, 1)))
    add("fan_958", fan, "poisson", tile_limit(1, 1) - 2, ("cols_max", tile_limit(1, 1) + 1))
    # a block of 128 rows at 4096 | 4097 adjacency entries (rows of at most 15 columns), a window at 7168 | 7169 incidences
    add("block_adj_4096", lattice_repeats, "poisson", 1, (7, 7, 7), "block_adj", ROW_T_ADJ, ("block_adj_max", ROW_T_ADJ))
    add("block_adj_4097", lattice_repeats, "poisson", 1, (7, 7, 7), "block_adj", ROW_T_ADJ + 1, ("block_adj_max", ROW_T_ADJ + 1))
    add("window_7168", lattice_repeats, "poisson", 1, (7, 7, 7), "window", ADJ_CAP, ("window_max", ADJ_CAP))
    add("window_7169", lattice_repeats, "poisson", 1, (7, 7, 7), "window", ADJ_CAP + 1, ("window_max", ADJ_CAP + 1))
    # the same at P2, where the overflow is met behind the wavefront kernel; and once more on a lattice whose repeats also
    # pass PAT_CAP: the window overflows, the sorted build refuses the row, the host builds
    add("p2_window_7168", lattice_repeats, "poisson", 2, (1, 2, 12), "window", ADJ_CAP, ("window_max", ADJ_CAP))
    add("p2_window_7169", lattice_repeats, "poisson", 2, (1, 2, 12), "window", ADJ_CAP + 1, ("window_max", ADJ_CAP + 1))
    add("p2_window_7169_then_host", lattice_repeats, "poisson", 2, (2, 2, 8), "window", ADJ_CAP + 1, ("window_max", ADJ_CAP + 1))
    return T


TABLE = _table()
NAMES = list(TABLE)


@functools.lru_cache(maxsize=None)
def case(name):
    return TABLE[name]()


# (limit case, its twin one unit past, quantity, unit): what test_pattern_sets.py proves pair by pair
PAIRS = [("p3_tet_cand_60", "p3_tet_cand_80", "cand_max", 20),
         ("fan_13", "fan_14", "cols_max", 1), ("fan_29", "fan_30", "cols_max", 1),
         ("fan3_13", "fan3_14", "cols_max", 1), ("fan3_29", "fan3_30", "cols_max", 1),
         ("fan_16", "fan_17", "cand_max", 4), ("fan_32", "fan_33", "cand_max", 4), ("fan_64", "fan_65", "cand_max", 4),
         ("fan_128", "fan_129", "cand_max", 4), ("fan_256", "fan_257", "cand_max", 4),
         ("p2_cand_60", "p2_cand_70", "cand_max", 10), ("p2_cand_120", "p2_cand_130", "cand_max", 10),
         ("p2_cand_250", "p2_cand_260", "cand_max", 10), ("p2_cand_510", "p2_cand_520", "cand_max", 10),
         ("p2_cand_1020", "p2_cand_1030", "cand_max", 10),
         ("p3_cand_120", "p3_cand_140", "cand_max", 20), ("p3_cand_240", "p3_cand_260", "cand_max", 20),
         ("p3_cand_500", "p3_cand_520", "cand_max", 20), ("p3_cand_1020", "p3_cand_1040", "cand_max", 20),
         ("p1_blocks_128", "p1_blocks_129", "runs", 4), ("p2_blocks_51", "p2_blocks_52", "runs", 10),
         ("fan3_338", "fan3_339", "cols_max", 1), ("fan_957", "fan_958", "cols_max", 1),
         ("block_adj_4096", "block_adj_4097", "block_adj_max", 1), ("window_7168", "window_7169", "window_max", 1),
         ("p2_window_7168", "p2_window_7169", "window_max", 1)]
# the capacity each pair straddles: the limit case's maximum is the largest multiple of the unit that does not exceed it
CAPACITY = {"cols_max": (16, 32, tile_limit(1, 3), tile_limit(1, 1)), "cand_max": REG_CAPS + (PAT_CAP,),
            "runs": (ADJ_MAX_RUNS,), "block_adj_max": (ROW_T_ADJ,), "window_max": (ADJ_CAP,)}


def covered_paths(names=None):
    """the values of the adjacency, row-kernel and builder fields that the table's claims reach"""
    ps = [case(n).path for n in (names or NAMES) if not case(n).path["refused"]]
    return ({p["adjacency"] for p in ps}, {p["row_kernel"] for p in ps}, {p["builder"] for p in ps}, {p["sort"] for p in ps})
