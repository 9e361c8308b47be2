"""GPU parity tests on hostile geometries against a 50-digit reference.

The other parity tests compare a kernel with the oracle -- the same formulae in the same doubles -- at 1e-12 of the largest
value, nearly always on the unit cube.  Here the meshes are those of tests/_hostile.py (far from the origin, anisotropic by
2^40, needles, graded, mirrored, noisy below / inside / above the lattice tolerance of csrc/zzz_renumber.hip, rotated,
sheared by 50), the reference is tests/_hp_ref.py (mpmath, 50 digits) and every entry is judged against its own scale:

    figure = max |value - reference| / scale          in units of 2^-53

for the assembled A and b, the matrix-free action and the matrix-free diagonal.  The oracle's figure on the same input is
one realisation of the rounding of this computation; another summation order, fused multiply-adds and the factorised
P2/P3 tables make a few times more operations, so a kernel must stay within

    figure(gpu) <= max(8 x figure(oracle), 32)

Constrained rows and columns of A, constrained entries of b, of the action and of the diagonal are exact (scale 0).
Pattern and product are bit-exact as everywhere else; the internal order's kind is asserted where the code fixes it.

FIGURES measured on an MI355X (units of 2^-53; ZZZ_RENUMBER unset and = 2 give the same figures; matrix-free figures with
ZZZ_MF_T = ZZZ_MF_NC = 128; 'cells' says whether the library moved the cells into its lattice order):

    case              P  kind (default/bins)  cells  |  A gpu oracle |  b gpu oracle |  action gpu oracle |  diagonal gpu oracle
    identity          1  1 / 1                moved  |   1.04   1.04 |   3.88   3.88 |   0.30   0.30      |   0.78   1.04
    offset            1  1 / 1                moved  |   1.04   1.56 |   3.13   4.12 |   0.50   0.50      |   1.04   1.56
    aniso             1  1 / 1                moved  |   1.80   1.80 |   3.88   3.88 |   0.60   0.60      |   1.80   1.80
    needle            1  1 / 1                moved  |   0.92   1.04 |   3.88   3.88 |   0.33   0.51      |   1.38   1.04
    needle_line       1  1 / 1                moved  |   0.87   0.87 |   2.31   2.61 |   0.41   0.41      |   0.87   0.87
    graded            1  1 / 1                moved  |   1.22   1.20 |   4.07   4.49 |   0.37   0.43      |   0.66   0.99
    graded_corner     1  1 / 1                moved  |   2.59   3.28 |   5.97   5.82 |   0.82   1.22      |   2.69   3.28
    graded_corner_16  1  1 / 1                kept   |   4.71   3.14 |   5.68   5.48 |   1.58   2.18      |   3.14   3.14
    mirror            1  1 / 1                moved  |   1.04   1.56 |   3.88   4.41 |   0.39   0.53      |   1.17   1.56
    mirror_axes       1  1 / 1                moved  |   1.04   1.04 |   3.71   4.41 |   0.30   0.53      |   1.04   1.04
    noise13           1  1 / 1                moved  |   0.78   1.04 |   3.39   3.60 |   0.35   0.35      |   0.52   1.04
    noise10           1  1 / 1                moved  |   1.04   1.15 |   3.88   3.69 |   0.25   0.23      |   0.52   1.04
    noise7            1  0 / 2                kept   |   1.53   1.15 |   3.88   3.88 |   0.30   0.25      |   0.78   0.52
    rotated           1  0 / 2                kept   |   1.04   1.17 |   3.88   4.12 |   0.19   0.26      |   0.52   1.17
    shear50_a         1  1 / 1                kept   |  23.61  23.61 |  28.64  29.84 |   4.85   4.24      |  11.55  11.17
    shear50_b         1  0 / 2                kept   |  22.56  22.56 |  18.02  18.87 |   1.80   2.65      |   4.28   7.72
    aniso             2  1 / 1                moved  |   1.00   2.25 |   2.15   6.27 |   0.36   0.51      |   0.50   1.60
    graded            2  1 / 1                moved  |   1.86   4.15 |   2.99   4.48 |   0.41   0.44      |   0.83   0.79
    mirror            2  1 / 1                moved  |   1.04   1.15 |   2.15   6.27 |   0.18   0.24      |   1.02   0.70
    shear50_a         2  0 / 1                kept   |  24.44  26.32 |  36.36  37.59 |   3.25   3.50      |  13.29  14.39
    noise10           2  1 / 1                moved  |   1.04   1.91 |   2.93   4.36 |   0.21   0.25      |   1.02   1.53
    offset            3  1 / 1                moved  |   0.62   2.02 |   3.62   5.96 |   0.23   0.31      |   0.60   0.75
    graded            3  1 / 1                moved  |   2.01   5.93 |   4.82   9.69 |   0.33   0.29      |   0.71   1.31
    mirror            3  0 / 1                moved  |   0.93   2.30 |   3.34   7.45 |   0.21   0.25      |   0.60   0.60
    shear50_a         3  0 / 1                kept   |  25.43  24.87 |  47.50  47.50 |   3.69   3.83      |  10.56  11.19
    worst of each column                       |  25.43  26.32 |  47.50  47.50 |   4.85   4.24      |  13.29  14.39
    graded_corner P1 default plan, ZZZ_RENUMBER None: blocks 4 x 2048, nloc_max 765 (host: 2048 cells, 765 dofs) | y 1.22 1.22 | d 2.61 3.28
    graded_corner P1 default plan, ZZZ_RENUMBER 0: blocks 4 x 2048, nloc_max 765 (host: 2048 cells, 765 dofs) | y 1.20 1.22 | d 3.14 3.28
    graded_corner_16 P1 default plan, ZZZ_RENUMBER None: blocks 19 x 1024, nloc_max 783 (host: 1024 cells, 783 dofs) | y 1.63 2.18 | d 3.14 3.14
    graded_corner_16 P1 default plan, ZZZ_RENUMBER 0: blocks 19 x 1024, nloc_max 783 (host: 1024 cells, 783 dofs) | y 1.63 2.18 | d 3.14 3.14

Kinds seen where the code does not fix them: mirror P1/P2 1, P3 0 / 1 (face dofs of a mirrored cube share keys: the
caller's order stays); noise10 1 (every line merges); shear50_a P1 1, P2/P3 0 / 1 (cells straddle cubes, kept); shear50_b
0 / 2 (a point cloud).  No case needed a bar of its own.

Elasticity is held to the oracle alone here, at 1e-12 of the largest value (test_elasticity_p1_block_rows).  The same
50-digit bar per entry for elasticity P1-P3, for the lifting pass of both problems and for the P2 / P3 near-nullspace is
tests/test_gpu_hostile_elasticity.py.
"""
from _gpu_helpers import *  # noqa: F401,F403 -- helpers, np / os / zzz / zo / pytest
import _hostile as H
import _hp_ref as hp
from _hostile_gpu import MF_SMALL, _assembled, _bar, _check_kind, _env, _upload

pytestmark = pytest.mark.gpu  # noqa: F405

_IDS = [f"{n}-P{o}" for n, o in H.POISSON_CASES]


@pytest.mark.parametrize("renumber", [None, "2"], ids=["default", "bins"])
@pytest.mark.parametrize("name,order", H.POISSON_CASES, ids=_IDS)
def test_operators_against_the_50_digit_reference(name, order, renumber):
    C = H.case(name, order)
    ref = H.reference(C)
    bcb = C.bc.astype(bool)
    u = np.random.default_rng(order).standard_normal(C.n)
    y_ref, t_ref, y_oracle = H.action_reference(C, u)
    d_ref, ds_ref, d_oracle = H.diagonal_reference(C)
    with zzz.Context(0) as c:
        _upload(c, C, renumber)
        kind = _check_kind(c, C, renumber)
        moved = c.cells_renumbered()
        rp, cl, v, b = _assembled(c, C)
        with _env(**MF_SMALL):
            c.matfree_setup()
            info = c.matfree_info()
            y = c.action(u)
            d = c.matfree_diagonal()
            np.testing.assert_array_equal(c.action(u), y)
            np.testing.assert_array_equal(c.matfree_diagonal(), d)
    fig = dict(A=hp.metric(v, ref["Rc"], ref["Sc"]) / hp.U, b=hp.metric(b, ref["r"], ref["s"]) / hp.U,
               y=hp.metric(y, y_ref, t_ref) / hp.U, d=hp.metric(d, d_ref, ds_ref) / hp.U)
    ofig = dict(A=ref["oracle_A"], b=ref["oracle_b"], y=y_oracle, d=d_oracle)
    print(f"\nHOSTILE {name:14s} P{order} {'bins   ' if renumber else 'default'} kind {kind} cells {'moved' if moved else 'kept '}"
          + "".join(f" | {k} {fig[k]:8.2f} {ofig[k]:7.2f}" for k in "Abyd")
          + f" | blocks {info['blocks']} x {info['cells_per_block']}")
    assert info["valid"] == 1 and info["blocks"] >= 2 and info["shared_dofs"] > 0 and info["threads"] == 128
    assert info["cells_per_block"] == 128
    # exact where a Dirichlet dof is involved (metric() has already asked the rows and columns of A and b for their bits)
    assert np.all(y[bcb] == 0.0) and np.all(d[bcb] == 1.0) and np.all(b[bcb] == 0.0)
    for k in "Abyd":
        assert fig[k] <= _bar(ofig[k]), (k, fig[k], ofig[k])


@pytest.mark.parametrize("name,order", H.POISSON_CASES, ids=_IDS)
def test_product_is_the_serial_loop_on_the_internal_system(name, order):
    """ctx.spmv against zo.spmv on P A P^T, bit for bit, under every form of the value dictionaries and both orders"""
    C = H.case(name, order)
    xv = np.random.default_rng(7).standard_normal(C.n)
    for renumber in (None, "2"):
        for knob in ("0", "2", "3"):
            with _env(ZZZ_SELLP_DICT=knob), zzz.Context(0) as c:
                _upload(c, C, renumber)
                perm = c.internal_order()[0]
                rp, cl, v, _ = _assembled(c, C)
                y = c.spmv(xv)
                np.testing.assert_array_equal(c.spmv(xv), y)
            irp, icl, iv, sperm = _internal_system(rp.astype(np.int64), cl, v, perm, C.bs)
            np.testing.assert_array_equal(y[sperm], zo.spmv(irp, icl, iv, xv[sperm]), err_msg=f"{renumber} {knob}")


@pytest.mark.parametrize("name,order", [(n, o) for n, o in H.POISSON_CASES if n in H.SOLVE_CASES],
                         ids=[i for i, (n, o) in zip(_IDS, H.POISSON_CASES) if n in H.SOLVE_CASES])
def test_jacobi_pcg_assembled_and_matrix_free(name, order):
    """The cases whose conditioning leaves a solve something to say: the oracle's Jacobi PCG on the oracle's system, +-2
    iterations and 1e-6 in the solution, for the assembled and for the matrix-free operator"""
    C = H.case(name, order)
    ov, ob = H.oracle(C)
    oit, ou, _, _ = zo.pcg(C.rowptr, C.cols, ov, ob, rtol=1e-8)
    for renumber in (None, "2"):
        with zzz.Context(0) as c:
            _upload(c, C, renumber)
            _assembled(c, C)
            it, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
            ua = c.vec_download(zzz.VEC_U)
            with _env(**MF_SMALL):
                itm, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, op=zzz.OP_MATFREE, rtol=1e-8)
            um = c.vec_download(zzz.VEC_U)
        print(f"\nHOSTILE solve {name} P{order}: oracle {oit}, assembled {it}, matrix-free {itm}")
        assert abs(it - oit) <= 2 and abs(itm - oit) <= 2
        assert np.linalg.norm(ua - ou) <= 1e-6 * np.linalg.norm(ou)
        assert np.linalg.norm(um - ou) <= 1e-6 * np.linalg.norm(ou)


P1_NC_DEFAULT, P1_NLOC_LIMIT = 2048, 1024  # mf_plan_build: cells per block and dofs a block's LDS holds, P1


@pytest.mark.parametrize("name", ["graded_corner", "graded_corner_16"])
def test_graded_corner_and_the_plan_retry(name):
    """x -> x^6 or x^8 crowds the centroids into few cells of the plan's Morton grid (one resolution, from the longest
    extent) and leaves the rest in long strings, so a block of the default size touches many dofs; beyond what LDS holds
    the plan halves its blocks and tries again (mf_plan_build).  With the caller's cell order kept (ZZZ_RENUMBER=0) the
    blocks are restated on the host (H.plan_blocks): the plan must hold exactly those dofs per block and stop at the first
    size that fits.  The 12 x 10 x 10 mesh with x^6 does NOT reach the retry: its largest default block touches 765 dofs
    of the 1024 that fit, so the plan rightly stays at 2048 cells; the 16 x 14 x 14 mesh with x^8 does (1201 dofs; 783 at
    1024 cells).  The action and the diagonal of those plans against the reference."""
    C = H.case(name, 1)
    u = np.random.default_rng(1).standard_normal(C.n)
    y_ref, t_ref, y_oracle = H.action_reference(C, u)
    d_ref, ds_ref, d_oracle = H.diagonal_reference(C)
    want_nc = P1_NC_DEFAULT
    while max(H.plan_blocks(C, want_nc)) > P1_NLOC_LIMIT:
        want_nc //= 2
    for renumber in (None, "0"):
        with _env(ZZZ_MF_T=None, ZZZ_MF_NC=None), zzz.Context(0) as c:
            _upload(c, C, renumber)
            c.matfree_setup()
            info = c.matfree_info()
            y = c.action(u)
            d = c.matfree_diagonal()
            np.testing.assert_array_equal(c.action(u), y)
        fy, fd = hp.metric(y, y_ref, t_ref) / hp.U, hp.metric(d, d_ref, ds_ref) / hp.U
        print(f"\nHOSTILE {name} P1 default plan, ZZZ_RENUMBER {renumber}: blocks {info['blocks']} x {info['cells_per_block']}, "
              f"nloc_max {info['nloc_max']} (host: {want_nc} cells, {max(H.plan_blocks(C, want_nc))} dofs)"
              f" | y {fy:.2f} {y_oracle:.2f} | d {fd:.2f} {d_oracle:.2f}")
        assert info["valid"] == 1 and info["blocks"] >= 2 and info["shared_dofs"] > 0 and info["threads"] == 256
        assert info["nloc_max"] <= P1_NLOC_LIMIT
        if renumber == "0":
            assert info["cells_per_block"] == want_nc and info["nloc_max"] == max(H.plan_blocks(C, want_nc))
        if name == "graded_corner_16":
            assert info["cells_per_block"] < P1_NC_DEFAULT  # the retry ran
        assert fy <= _bar(y_oracle) and fd <= _bar(d_oracle)


@pytest.mark.parametrize("name", H.ELASTICITY_P1_ORACLE_CASES)
def test_elasticity_p1_block_rows(name):
    """Elasticity P1 (block rows, by-node assembly) against the oracle at the bar of the other parity tests, the product
    against the serial loop"""
    C = H.case(name, 1, "elasticity")
    ov, ob = H.oracle(C)
    xv = np.random.default_rng(5).standard_normal(C.n)
    for renumber in (None, "2"):
        with zzz.Context(0) as c:
            _upload(c, C, renumber)
            perm, kind = c.internal_order()
            assert kind in (0, 1, 2)
            rp, cl, v, b = _assembled(c, C)
            y = c.spmv(xv)
        print(f"\nHOSTILE elasticity {name} {'bins' if renumber else 'default'} kind {kind}: A {np.abs(v - ov).max() / np.abs(ov).max():.2e}"
              f" b {np.abs(b - ob).max() / np.abs(ob).max():.2e}")
        assert np.abs(v - ov).max() <= 1e-12 * np.abs(ov).max()
        assert np.abs(b - ob).max() <= 1e-12 * np.abs(ob).max()
        irp, icl, iv, sperm = _internal_system(rp.astype(np.int64), cl, v, perm, C.bs)
        np.testing.assert_array_equal(y[sperm], zo.spmv(irp, icl, iv, xv[sperm]))


@pytest.mark.parametrize("name", H.ELASTICITY_P1_ORACLE_CASES)
def test_elasticity_p1_near_nullspace(name):
    """The six orthonormalised rigid-body modes against the oracle's at the bar of test_near_nullspace_against_oracle.

    `offset` is the case that made the library and the oracle take the rotations about the centre of the dofs.  With the
    reference's (-y, x, 0), ... of the coordinates as given, both missed this bar (MI355X: deviation from orthonormality
    3.05e-11 in the library, 3.62e-11 in the oracle, |B - OB| = 3.37e-11 max|OB|; the other four cases 4e-16 .. 4e-15):
    65 536 away from the origin a rotation is a translation up to 1.5e-5 of its size, and what the projection leaves
    carries 2^-53 x 65 536 ~ 1e-11.  Rotations about the centre span the same space and orthonormalise to the same basis."""
    C = H.case(name, 1, "elasticity")
    dof_x = np.zeros((C.nblock, 3))
    dof_x[C.cell_dofs] = C.x[C.cells]  # P1: a dof sits on its vertex
    OB, odev = zo.near_nullspace(dof_x)
    with zzz.Context(0) as c:
        _upload(c, C, None)
        B, dev = c.near_nullspace()
    print(f"\nHOSTILE nullspace {name}: |B - OB| {np.abs(B - OB).max() / np.abs(OB).max():.2e} deviation {dev:.2e} (oracle {odev:.2e})")
    assert dev <= 1e-12 and odev <= 1e-12
    assert np.abs(B - OB).max() <= 1e-12 * np.abs(OB).max()
    assert np.abs(B @ B.T - np.eye(6)).max() <= 1e-12
