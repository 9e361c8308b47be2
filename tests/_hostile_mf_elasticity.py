"""The 50-digit reference of the matrix-free ELASTICITY action and diagonal on the hostile meshes: TEST INFRASTRUCTURE ONLY.

tests/_hostile.py's action_reference is the Poisson one (its oracle figure comes from zo.action_poisson); this is the same
rule for block size 3: y = R u with products and sums in long double on the mp pass's unconstrained matrix, t its per-row
scale sum_j S_ij |u_j|, constrained rows y = 0 exactly with scale 0; the oracle's figure is that of its own unconstrained
matrix applied through zo.spmv with the constrained rows zeroed.

The P3 cases run on a base of their own, 3 x 3 x 3 (162 cells, 3000 scalar dofs): at 128 cells per block that is two blocks
(of about 850 and 300 nodes, by the cell order), where H.ELASTICITY_BASE[3] -- which the assembled tests keep -- is one."""
import numpy as np

import _hostile as H
import _hp_ref as hp
import zzz_oracle as zo

CASES = [(n, o) for o in (1, 2, 3) for n in ("offset", "aniso", "graded", "rotated") if n in H.ELASTICITY_CASES[o]]
DIMS = {3: (3, 3, 3)}  # (orders not listed: H.ELASTICITY_BASE)


def case(name, order):
    return H.case(name, order, "elasticity", dims=DIMS.get(order))


def action_reference(C, u):
    """(y, t, the oracle's figure in units of 2^-53)"""
    ref = H.reference(C)
    y, t = hp.apply(ref["R"], ref["S"], C.rowptr, C.cols, u)
    y, t = np.array(y, np.float64), np.array(t, np.float64)
    bcb = C.bc.astype(bool)
    y[bcb] = 0.0
    t[bcb] = 0.0
    oy = zo.spmv(np.ascontiguousarray(C.rowptr, np.int64), C.cols, ref["ou"], u)
    oy[bcb] = 0.0
    return y, t, hp.metric(oy, y, t) / hp.U


# oracle_constants() below, rounded up to two places: how far the ORACLE is from the 50-digit reference on the undistorted cube
#   PYTHONPATH=oracle:tests:performance-test_amd python -c "import _hostile_mf_elasticity as HE; print(HE.oracle_constants())"
#   {1: (0.3771, 1.1629), 2: (0.3780, 1.7737), 3: (0.3256, 1.7230)}
O_ACTION = {1: 0.38, 2: 0.38, 3: 0.33}
O_DIAGONAL = {1: 1.17, 2: 1.78, 3: 1.73}


def oracle_system(order, x, cells, cell_dofs, nblock):
    """(rowptr, cols, Au, its diagonal): the oracle's UNCONSTRAINED elasticity matrix (a zero marker) of a mesh"""
    zo.set_num_threads(1)
    rp, cl = zo.pattern(nblock, cell_dofs, 3)
    Au = zo.assemble_matrix(1, order, x, cells, cell_dofs, np.zeros(3 * nblock, np.uint8), rp, cl)
    rows = np.repeat(np.arange(3 * nblock), np.diff(rp))
    diag = np.zeros(3 * nblock)
    diag[rows[cl == rows]] = Au[cl == rows]
    return rp, cl, Au, diag


def oracle_figures(rp, cl, Au, diag, bc, v, y, d=None):
    """(action figure, diagonal figure) of y = action(v) and d = matfree_diagonal() against the oracle's matrix, per row and in
    units of 2^-53:
      action    oy = where(bc, 0, Au v) judged against t_i = sum_j |Au_ij| |v_j|, t[bc] = 0
      diagonal  od = where(bc, 1, diag Au) judged against od itself on free rows (every cell's contribution to a diagonal entry
                is positive) and against 0 on constrained ones
    a scale of 0 makes hp.metric ask for the reference's bits: 0.0 and 1.0 on the constrained rows."""
    bcb = np.asarray(bc).astype(bool)
    oy = np.where(bcb, 0.0, zo.spmv(rp, cl, Au, v))
    t = zo.spmv(rp, cl, np.abs(Au), np.abs(v))
    t[bcb] = 0.0
    assert np.all(t[~bcb] > 0) and np.all(diag[~bcb] > 0)
    fy = hp.metric(y, oy, t) / hp.U
    fd = None if d is None else hp.metric(d, np.where(bcb, 1.0, diag), np.where(bcb, 0.0, diag)) / hp.U
    return fy, fd


def oracle_constants(orders=(1, 2, 3)):
    """{order: (action figure, diagonal figure)} of the ORACLE against the 50-digit reference on the undistorted cube
    H.case("identity", order, "elasticity"), u = default_rng(40 + order): the constants O_ACTION / O_DIAGONAL of
    tests/test_gpu_mf_elasticity_plans.py (CPU only)"""
    out = {}
    for order in orders:
        C = H.case("identity", order, "elasticity")
        u = np.random.default_rng(40 + order).standard_normal(C.n)
        out[order] = (action_reference(C, u)[2], diagonal_reference(C)[2])
    return out


def diagonal_reference(C):
    """(d, scale, the oracle's figure in units of 2^-53): the diagonal of the mp pass's CONSTRAINED matrix -- 1.0 exactly, scale
    0, on constrained rows -- and the diagonal of the oracle's constrained matrix against it"""
    ref = H.reference(C)
    d, sd = hp.diagonal(ref["Rc"], ref["Sc"], C.rowptr, C.cols)
    od, _ = hp.diagonal(H.oracle(C)[0], ref["Sc"], C.rowptr, C.cols)
    return np.array(d, np.float64), np.array(sd, np.float64), hp.metric(od, d, sd) / hp.U
