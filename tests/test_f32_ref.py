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
