"""What single precision costs the cgpoisson path, measured on the CPU with the numpy float32 restatement of tests/_f32_ref.py
on the oracle's element matrices: the figures the GPU tests of the float32 path (tests/test_gpu_f32.py) scale their bounds
from.  No GPU and no library code is involved.

Bounds.  Action: 1e-6 of max|y64| -- a loose cap; a float32 element product of nd <= 20 terms and a scatter of at most a few
dozen of them carry a few eps32 = 6e-8 each, the recorded values are 5e-8 to 5e-7.  CG: cg.h's 100 iterations at rtol 1e-6 in
both precisions on the three small cubes, residual ratios within 10 % of each other; the float-against-double solution
difference within a factor 2 of the recorded one (the order in which numpy sums an element product is not pinned)."""
import numpy as np
import pytest

import _f32_ref as fr
import _hostile as H

SMALL = [(1, (24, 22, 23)), (2, (12, 11, 13)), (3, (8, 7, 9))]


@pytest.mark.parametrize("order,dims", SMALL + [(3, (14, 13, 15))])
def test_float32_element_products_stay_within_the_cap(order, dims):
    P, Ae, _ = fr.cube(order, dims)
    u = fr.noise(P.n)
    y64 = fr.action(Ae, P.cell_dofs, P.bc, u, np.float64)
    y32 = fr.action(Ae, P.cell_dofs, P.bc, u, np.float32)
    err = np.abs(y32 - y64).max() / np.abs(y64).max()
    print(f"P{order} {dims}: action error {err:.2e}")
    assert 0 < err <= 1e-6
    assert np.all(y32[P.bc.astype(bool)] == 0)


@pytest.mark.parametrize("dims", [(12, 10, 14), (40, 38, 42)])
def test_float32_p1_geometry_from_block_relative_coordinates(dims):
    """The P1 kernel forms its geometry in float: from coordinates relative to an origin of the cell block the action stays
    within the cap on a mesh of any size; from rounded ABSOLUTE coordinates the Jacobian's error is eps32 / h and the larger
    mesh is the worse one."""
    P, Ae, _ = fr.cube(1, dims)
    u = fr.noise(P.n)
    y64 = fr.action(Ae, P.cell_dofs, P.bc, u, np.float64)
    rel = np.abs(fr.action32_p1_geometry(P.x, P.cells, P.cell_dofs, P.bc, u) - y64).max() / np.abs(y64).max()
    ab = np.abs(fr.action32_p1_geometry(P.x, P.cells, P.cell_dofs, P.bc, u, absolute=True) - y64).max() / np.abs(y64).max()
    print(f"P1 {dims}: float geometry, block-relative {rel:.2e}, absolute {ab:.2e}")
    assert 0 < rel <= 1e-6
    assert ab > rel


@pytest.mark.parametrize("order,dims", SMALL)
def test_float32_cg_runs_the_same_100_iterations(order, dims):
    (k64, x64, h64), (k32, x32, h32) = fr.cg_pair(order, dims)
    r64, r32 = h64[-1] / h64[0], h32[-1] / h32[0]
    diff = np.linalg.norm(x32 - x64) / np.linalg.norm(x64)
    print(f"P{order} {dims}: iterations {k64} / {k32}, residual ratio {r64:.4e} / {r32:.4e}, solution difference {diff:.2e}")
    assert k64 == 100 and k32 == 100
    assert abs(r32 - r64) <= 0.1 * r64
    pinned = fr.SOLUTION_DIFF[(order, dims)]
    assert pinned / 2 <= diff <= 2 * pinned


def test_a_converging_case_takes_the_same_iterations_in_both_precisions():
    """the first cube of the family n x (n - 1) x (n + 1), n = 4, 6, ... on which cg.h converges before 100 iterations in
    float and within +-2 of the double count: the GPU test's converging case"""
    (k64, _, _), (k32, _, _) = fr.cg_pair(*fr.CONVERGING)
    print(f"converging case {fr.CONVERGING}: {k64} / {k32} iterations")
    assert k32 < 100 and abs(k32 - k64) <= 2


# ---- the P1 float geometry on hostile meshes: figures per entry against the 50-digit reference, in units of 2^-24 -------------
# Measured with this restatement (blocks: Morton runs of nc cells, H.plan_cell_blocks; origins: the first vertex of the
# block's first cell / the library's rule, p1_block_origins, started from the dof the block lists first / none -- absolute):
#   case            first vertex, nc 128 / 2048   the rule, nc 128 / 2048 (blocks on the second origin)   absolute
#   offset              0.28 /     0.28               0.20 /  0.19  (0 of 8 / 0 of 1)                      25 431
#   shear50_b           2.7  /    35                  3.27 / 16.34  (0 of 13 / 0 of 1)                       35
#   graded              7.2  /     0.26               3.72 /  0.61  (0 of 8 / 0 of 1)                         0.26
#   graded_corner  38 063    / 129 297                0.67 /  0.67  (53 of 57 / 4 of 4)                       0.67
#   graded12          inf    /  (finite)              1.00 /  1.00  (7 of 8 / 1 of 1)                         1.00
#   graded_far8    (127 of 441 entries > 32)          0.69 /  0.70  (11 of 14 / 1 of 1)                   5 507
#   graded_ends12  refused: 6 of 8 blocks / the one block (no origin serves cells of 1e-6 at both ends of a block)
# the other served cases: 0.14 .. 5.8 at nc 128, 0.18 .. 13.8 at nc 2048, every block on its first origin.
SERVED = ["identity", "offset", "aniso", "needle", "needle_line", "mirror", "mirror_axes", "noise13", "noise10", "noise7",
          "rotated", "shear50_a", "shear50_b", "graded", "graded_corner"] + H.F32_P1_EXTRA


def _p1(name):
    C = H.case(name, 1)
    u = np.random.default_rng(1).standard_normal(C.n).astype(np.float32).astype(np.float64)  # float-representable
    y_ref, t_ref, _ = H.action_reference(C, u)
    return C, u, y_ref, t_ref


def _first_vertex(C, nc):
    """(block of every cell, first vertex of every block's first cell)"""
    o = H.plan_cell_order(C)
    blk = H.plan_cell_blocks(C, nc)
    return blk, C.x[C.cells[o[::nc], 0]]


def _figure(C, u, y_ref, t_ref, **kw):
    return fr.figure32(fr.action32_p1_geometry(C.x, C.cells, C.cell_dofs, C.bc, u, **kw), y_ref, t_ref)


def test_block_relative_coordinates_beat_absolute_ones_far_from_the_origin():
    C, u, y_ref, t_ref = _p1("offset")
    blk, first = _first_vertex(C, 128)
    rel, ab = _figure(C, u, y_ref, t_ref, block=blk, origin=first), _figure(C, u, y_ref, t_ref, absolute=True)
    print(f"offset: relative {rel:.2f}, absolute {ab:.2f} units of 2^-24")
    assert rel <= 1.0 and ab >= 1000.0 * rel


@pytest.mark.parametrize("nc", [128, 2048])
def test_a_fixed_block_origin_loses_to_absolute_coordinates_on_a_mesh_graded_to_a_corner(nc):
    """x -> x^6: the cells at the corner are 10^5 times smaller than a block; relative to a vertex elsewhere in the block
    their coordinates round at the block's scale -- worse than rounding them where they stand, next to 0"""
    C, u, y_ref, t_ref = _p1("graded_corner")
    blk, first = _first_vertex(C, nc)
    rel, ab = _figure(C, u, y_ref, t_ref, block=blk, origin=first), _figure(C, u, y_ref, t_ref, absolute=True)
    print(f"graded_corner nc {nc}: relative {rel:.0f}, absolute {ab:.2f} units of 2^-24")
    assert ab <= 1.0 and rel >= 1000.0


def test_a_fixed_block_origin_collapses_cells_of_x12_to_a_zero_determinant():
    C, u, y_ref, t_ref = _p1("graded12")
    blk, first = _first_vertex(C, 128)
    y = fr.action32_p1_geometry(C.x, C.cells, C.cell_dofs, C.bc, u, block=blk, origin=first)
    print(f"graded12 nc 128: {np.count_nonzero(~np.isfinite(y))} of {C.n} entries are not finite")
    assert not np.isfinite(y).all() and fr.figure32(y, y_ref, t_ref) == float("inf")
    # ... and the rule's verdict on exactly those origins: not served
    ok, jerr = zip(*[[v.min() if i == 0 else v.max() for i, v in enumerate(fr.p1_cells(C.x[C.cells][blk == b], first[b])[:2])]
                     for b in range(len(first))])
    assert not all(ok) and max(jerr) > fr.JTOL


@pytest.mark.parametrize("nc", [128, 2048])
@pytest.mark.parametrize("name", SERVED)
def test_the_origin_rule_serves_the_hostile_meshes_within_the_bar(name, nc):
    """The library's rule restated (fr.p1_block_origins), started from the dof each block lists first: no block is refused,
    the action is finite and every entry within 32 units of 2^-24 of the 50-digit reference at its own scale -- the floor of
    the bar of tests/test_gpu_hostile_geometry.py in float units.  (The rule keeps a first origin up to 256 units in an entry
    of the worst cell's Jacobian; on these meshes the blocks it keeps are at 64 units or less and the largest figure is 16.3,
    shear50_b in one block.)  A block past the first bar would be past this one without the second origin: both figures are
    printed."""
    C, u, y_ref, t_ref = _p1(name)
    blk = H.plan_cell_blocks(C, nc)
    dof_x = np.zeros((C.n, 3))
    dof_x[C.cell_dofs] = C.x[C.cells]
    first = dof_x[fr.first_listed_dof(C.cell_dofs, blk)]
    origin, status, jerr = fr.p1_block_origins(C.x, C.cells, blk, first)
    f_first, f_rule = _figure(C, u, y_ref, t_ref, block=blk, origin=first), _figure(C, u, y_ref, t_ref, block=blk, origin=origin)
    print(f"{name} nc {nc}: {len(status)} blocks, {np.count_nonzero(status == 1)} on the second origin; figure {f_rule:.2f} "
          f"(first origins alone {f_first:.2f})")
    assert np.all(status < 2)
    assert f_rule <= 32.0
    if name in ("graded_corner", "graded12", "graded_far8"):
        assert np.any(status == 1) and f_first > 32.0  # the retry is what serves them
    if not np.any(status == 1):
        assert f_rule == f_first


@pytest.mark.parametrize("nc", [128, 2048])
def test_the_origin_rule_refuses_a_mesh_graded_to_both_ends(nc):
    C, u, y_ref, t_ref = _p1(H.F32_P1_REFUSED)
    blk = H.plan_cell_blocks(C, nc)
    dof_x = np.zeros((C.n, 3))
    dof_x[C.cell_dofs] = C.x[C.cells]
    origin, status, jerr = fr.p1_block_origins(C.x, C.cells, blk, dof_x[fr.first_listed_dof(C.cell_dofs, blk)])
    f = _figure(C, u, y_ref, t_ref, block=blk, origin=origin)
    worst = max(fr.p1_cells(C.x[C.cells][blk == b], origin[b])[2].max() for b in np.nonzero(status == 2)[0])
    print(f"{H.F32_P1_REFUSED} nc {nc}: {np.count_nonzero(status == 2)} of {len(status)} blocks refused, figure if served "
          f"anyway {f:.0f}, largest distance / extent {worst:.3g}")
    assert np.any(status == 2) and f > 32.0 and worst > 4096.0  # (2^-24 x distance / extent > JTOL, or the block were served)
