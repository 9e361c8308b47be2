"""GPU parity tests on hostile geometries against a 50-digit reference: elasticity P1-P3, the lifting pass of both problems,
the near-nullspace at P2 and P3.

tests/test_gpu_hostile_geometry.py judges every Poisson entry against its own scale; elasticity it compares with the oracle
alone, at 1e-12 of the largest value, and only at P1.  On `aniso` (x 2^20, y 1, z 2^-20) the nine entries of one 3 x 3 block
span 2^80 (gradients go with 1 / length: z-z is the largest, x-x the smallest) and the smallest scale is 8.8e-20 of max|A|
(1.0e-20 at P2): at that bar every x-x, x-y, x-z and y-y coupling could be wrong by a factor of two.  Here the reference
is tests/_hp_ref.py's elasticity (mpmath, 50 digits, component-aware scale), the meshes are H.ELASTICITY_CASES (P2 on
3 x 3 x 4, P3 on 2 x 2 x 3 cubes: one mp pass of 2-6 s per case, shared) and the bar is the one of the Poisson file,

    figure = max |value - reference| / scale  in units of 2^-53,        figure(gpu) <= max(8 x figure(oracle), 32)

with entries of scale 0 (Dirichlet rows and columns, constrained entries of b) exact.

(a) A and b under both internal orders (ZZZ_RENUMBER unset, = 2) and both matrix kernels of the order (P1: by node /
    ZZZ_ASM_NODE3=0 by scalar row; P2, P3: stored positions / ZZZ_ASM_SEARCH=1); pattern, second assembly and second
    download bit for bit.
(b) The product == the serial loop on the internal system, bit for bit, with the special forms asked for (block rows; at
    P2, P3 block windows where those decline) and on the generic stream, under ZZZ_SELLP_DICT 0, 2 and 3; the form that
    served is asserted (SPECIAL_FORM).
(c) Jacobi PCG against the oracle's on the oracle's system (iterations +-2, solution 1e-6) where the conditioning leaves a
    solve something to say.
(d) The lifting pass (zzz_bc_values_upload; k_lift has its own gather and its own Dirichlet logic): b with noise for u0
    against the lifted reference of H.lifted_reference, for Poisson and elasticity; the oracle's figure is that of its
    unconstrained A and b lifted the same way.
(e) The near-nullspace at P2 and P3 against the oracle's of H.dof_coords.  The library takes the dof coordinates from
    k_nn_dof_coords (csrc/zzz_nullspace.hip): sum_k w_k x_k with the barycentric weights of the node, in the dof's first
    cell.  (k_dof_coords of csrc/zzz_assemble.hip is P1-only and copies vertices.)

FIGURES measured on an MI355X (units of 2^-53; both matrix kernels of an order and both internal orders gave the same figures
to the digits shown; 'old bar' is max |A - oracle| / max|A|, the comparison of test_elasticity_p1_block_rows, next to the
figures it cannot see; 'special form' is what served under ZZZ_SELLP_BLK = ZZZ_SELLP_BWIN = 2; PCG iterations where (c) runs):

    case        P  kind (default/bins)  cells  |  A gpu oracle |  b gpu oracle |  old bar   | special form   | PCG oracle gpu
    identity    1  1 / 1                moved  |   1.25   1.55 |   3.93   4.52 |  6.4e-16   | block rows    |  115 115
    offset      1  1 / 1                moved  |   1.30   1.74 |   3.99   4.80 |  3.9e-16   | block rows    |  115 115
    aniso       1  1 / 1                moved  |   1.50   2.34 |   3.93   4.52 |  3.9e-16   | block rows    |    -
    needle      1  1 / 1                moved  |   1.17   2.00 |   3.93   4.52 |  4.0e-16   | block rows    |    -
    graded      1  1 / 1                moved  |   1.57   2.34 |   5.14   4.85 |  5.7e-16   | block rows    |  348 348
    mirror      1  1 / 1                moved  |   1.25   1.55 |   3.60   4.77 |  5.2e-16   | block rows    |  117 117
    noise10     1  1 / 1                moved  |   2.17   2.17 |   3.76   4.57 |  3.9e-16   | declined      |  115 115
    noise7      1  0 / 2                kept   |   2.20   2.93 |   4.07   4.69 |  3.9e-16   | declined      |  115 115
    rotated     1  0 / 2                kept   |   1.88   2.33 |   3.96   3.96 |  3.9e-16   | declined      |  118 118
    shear50_a   1  1 / 1                kept   |  26.15  26.15 |  38.71  38.71 |  4.4e-16   | block rows    |    -
    shear50_b   1  0 / 2                kept   |  22.64  22.83 |  30.95  30.06 |  5.2e-16   | declined      |    -
    aniso       2  1 / 1                moved  |   1.75   3.61 |   2.17   3.79 |  4.9e-16   | block rows    |    -
    graded      2  1 / 1                moved  |   1.63   2.90 |   2.98   4.75 |  1.6e-16   | block windows |  525 526
    mirror      2  1 / 1                moved  |   1.51   3.25 |   2.17   3.65 |  6.0e-16   | block rows    |  190 190
    rotated     2  0 / 2                kept   |   2.29   3.46 |   2.48   3.24 |  4.2e-16   | declined      |  197 197
    shear50_a   2  0 / 1                kept   |  26.10  25.91 |  34.98  34.98 |  3.5e-16   | block windows |    -
    noise10     2  1 / 1                moved  |   1.99   3.80 |   2.27   4.15 |  5.0e-16   | declined      |  187 187
    offset      3  1 / 1                moved  |   1.38   5.46 |   2.68   9.52 |  3.2e-16   | block windows |  257 256
    graded      3  1 / 1                moved  |   1.88   6.37 |   4.65   7.74 |  2.3e-16   | declined      |  621 622
    rotated     3  0 / 2                kept   |   2.13   5.48 |   3.68  11.66 |  4.7e-16   | declined      |  270 268
    shear50_a   3  0 / 1                kept   |  32.76  33.70 |  59.68  65.45 |  5.4e-16   | declined      |    -
    worst of each column                       |  32.76  33.70 |  59.68  65.45 |

    lifting (default and bins alike)          |  b gpu oracle |  without values gpu oracle
    poisson    offset     P1                  |   3.13   3.71 |   3.13   4.12
    poisson    aniso      P1                  |   3.88   3.88 |   3.88   3.88
    poisson    graded     P1                  |   3.38   4.49 |   4.07   4.49
    poisson    rotated    P1                  |   3.88   3.88 |   3.88   4.12
    poisson    shear50_a  P1                  |  28.64  29.84 |  28.64  29.84
    poisson    graded     P2                  |   1.87   4.27 |   2.99   4.48
    poisson    offset     P3                  |   3.00   5.96 |   3.62   5.96
    elasticity aniso      P1                  |   3.93   3.76 |   3.93   4.52
    elasticity rotated    P1                  |   3.96   3.96 |   3.96   3.96
    elasticity shear50_a  P1                  |  38.71  38.71 |  38.71  38.71
    elasticity aniso      P2                  |   2.17   3.57 |   2.17   3.79
    elasticity graded     P3                  |   3.55   5.56 |   4.65   7.74

    nullspace offset P2: |B - OB| 1.62e-15 max|OB|, deviation 2.22e-16 (oracle 8.22e-15)
    nullspace aniso  P2: |B - OB| 2.14e-15 max|OB|, deviation 2.22e-16 (oracle 7.55e-15)
    nullspace graded P3: |B - OB| 3.03e-15 max|OB|, deviation 2.22e-16 (oracle 1.11e-14)
    nullspace offset P3: |B - OB| 2.67e-11 max|OB|, deviation 2.22e-16 (bar 4.7e-10: _nullspace_bar)

No kernel missed the bar and no case of A, b, the product, the solves or the lifting needed one of its own.  The product was
the serial loop's in every form (the generic stream under ZZZ_SELLP_DICT=2 held 260 .. 44 675 distinct values; on `aniso`
they span 2^80).  The whole file took 33 s there, the shared mp passes included; its slowest test 3.1 s.
"""
from _gpu_helpers import *  # noqa: F401,F403 -- helpers, np / os / zzz / zo / pytest
import _hostile as H
import _hp_ref as hp
from _hostile_gpu import _assembled, _bar, _check_kind, _env, _upload

pytestmark = pytest.mark.gpu  # noqa: F405

_EL = [(n, o) for o in (1, 2, 3) for n in H.ELASTICITY_CASES[o]]
_EL_IDS = [f"{n}-P{o}" for n, o in _EL]
# the second matrix kernel of an order: (knob, value)
SECOND_KERNEL = {1: ("ZZZ_ASM_NODE3", "0"), 2: ("ZZZ_ASM_SEARCH", "1"), 3: ("ZZZ_ASM_SEARCH", "1")}
# the special form of the product asked for at an order, and the knobs that keep every special form away
SPECIAL = {1: dict(ZZZ_SELLP_BLK="2", ZZZ_SELLP="2"), 2: dict(ZZZ_SELLP_BLK="2", ZZZ_SELLP_BWIN="2", ZZZ_SELLP="2"),
           3: dict(ZZZ_SELLP_BLK="2", ZZZ_SELLP_BWIN="2", ZZZ_SELLP="2")}
GENERIC = {1: dict(ZZZ_SELLP_BLK="0", ZZZ_SELLP="2"), 2: dict(ZZZ_SELLP_BLK="0", ZZZ_SELLP_BWIN="0", ZZZ_SELLP="2"),
           3: dict(ZZZ_SELLP_BLK="0", ZZZ_SELLP_BWIN="0", ZZZ_SELLP="2")}
# The form that serves under SPECIAL, seen on the MI355X and the same under every ZZZ_SELLP_DICT.  The block rows hold a table
# of distinct 3 x 3 blocks and a dictionary of their values in LDS, the block windows a table of distinct blocks of rows: a
# lattice feeds them few (also stretched, graded, mirrored or sheared along a lattice direction), a point cloud (noise, a
# rotation, ny + 1 > 8 sheared lines) more than they hold, and they decline -- the generic stream then serves, with
# 3 382 .. 44 675 distinct values in its dictionary under ZZZ_SELLP_DICT=2.
BLOCK_ROWS, BLOCK_WINDOWS, DECLINED = "block rows", "block windows", ""
SPECIAL_FORM = {("identity", 1): BLOCK_ROWS, ("offset", 1): BLOCK_ROWS, ("aniso", 1): BLOCK_ROWS, ("needle", 1): BLOCK_ROWS,
                ("graded", 1): BLOCK_ROWS, ("mirror", 1): BLOCK_ROWS, ("noise10", 1): DECLINED, ("noise7", 1): DECLINED,
                ("rotated", 1): DECLINED, ("shear50_a", 1): BLOCK_ROWS, ("shear50_b", 1): DECLINED,
                ("aniso", 2): BLOCK_ROWS, ("graded", 2): BLOCK_WINDOWS, ("mirror", 2): BLOCK_ROWS, ("rotated", 2): DECLINED,
                ("shear50_a", 2): BLOCK_WINDOWS, ("noise10", 2): DECLINED,
                ("offset", 3): BLOCK_WINDOWS, ("graded", 3): DECLINED, ("rotated", 3): DECLINED, ("shear50_a", 3): DECLINED}


@pytest.mark.parametrize("name,order", _EL, ids=_EL_IDS)
def test_matrix_and_vector_against_the_50_digit_reference(name, order):
    """(a)"""
    C = H.case(name, order, "elasticity")
    ref = H.reference(C)
    bcb = C.bc.astype(bool)
    assert np.all(ref["S"] > 0) and ref["oracle_A_free"] <= 100 and ref["oracle_b_free"] <= 100
    knob, second = SECOND_KERNEL[order]
    for renumber in (None, "2"):
        for kv in (None, second):
            with _env(**{knob: kv}), zzz.Context(0) as c:
                _upload(c, C, renumber)
                kind = _check_kind(c, C, renumber)
                moved = c.cells_renumbered()
                rp, cl, v, b = _assembled(c, C)  # (pattern == C.rowptr, C.cols; a second download gives the same bits)
                c.assemble_matrix(C.form)
                c.assemble_vector(C.form)
                np.testing.assert_array_equal(c.csr_download()[2], v)
                np.testing.assert_array_equal(c.vec_download(zzz.VEC_B), b)
            # metric() asks the entries of scale 0 -- constrained rows and columns of A, constrained entries of b -- for the bits
            fig = dict(A=hp.metric(v, ref["Rc"], ref["Sc"]) / hp.U, b=hp.metric(b, ref["r"], ref["s"]) / hp.U)
            ofig = dict(A=ref["oracle_A"], b=ref["oracle_b"])
            old = np.abs(v - H.oracle(C)[0]).max() / np.abs(H.oracle(C)[0]).max()
            print(f"\nHOSTILE elasticity {name:10s} P{order} {'bins   ' if renumber else 'default'} {knob[8:]}={kv or '-'} kind {kind} cells "
                  f"{'moved' if moved else 'kept '}" + "".join(f" | {k} {fig[k]:8.2f} {ofig[k]:7.2f}" for k in "Ab")
                  + f" | against the oracle / max|A| {old:.1e}")
            assert np.all(b[bcb] == 0.0)
            for k in "Ab":
                assert fig[k] <= _bar(ofig[k]), (k, fig[k], ofig[k], renumber, kv)


@pytest.mark.parametrize("name,order", _EL, ids=_EL_IDS)
def test_product_is_the_serial_loop_on_the_internal_system(name, order):
    """(b) ctx.spmv against zo.spmv on P A P^T, bit for bit.  `aniso` is the interesting one: its value dictionary spans
    2^80."""
    C = H.case(name, order, "elasticity")
    xv = np.random.default_rng(7).standard_normal(C.n)
    wrong = []
    for label, knobs in (("special", SPECIAL[order]), ("generic", GENERIC[order])):
        for knob in ("0", "2", "3"):
            with _env(ZZZ_SELLP_DICT=knob, **knobs), zzz.Context(0) as c:
                _upload(c, C, None)
                perm = c.internal_order()[0]
                rp, cl, v, _ = _assembled(c, C)
                y = c.spmv(xv)
                np.testing.assert_array_equal(c.spmv(xv), y)
                vi = c.spmv_values_info()
            irp, icl, iv, sperm = _internal_system(rp.astype(np.int64), cl, v, perm, C.bs)
            np.testing.assert_array_equal(y[sperm], zo.spmv(irp, icl, iv, xv[sperm]), err_msg=f"{label} {knob}")
            print(f"\nHOSTILE elasticity product {name:10s} P{order} {label} DICT={knob}: '{vi['special_form']}' block form "
                  f"{vi['block_form']}, values as {vi['form']} ({vi['distinct_values']} distinct)")
            want = DECLINED if label == "generic" else SPECIAL_FORM[(name, order)]
            if vi["special_form"] != want:
                wrong.append((label, knob, vi["special_form"], want))
            if vi["special_form"] == DECLINED:  # the generic stream: its values as doubles, or through a dictionary
                if (knob == "0" and vi["form"] != "doubles") or (knob == "2" and not vi["form"].startswith("dictionary")):
                    wrong.append((label, knob, vi["form"]))
    assert not wrong, wrong


_SOLVE = [(n, o) for n, o in _EL if n in H.ELASTICITY_SOLVE_CASES]


@pytest.mark.parametrize("name,order", _SOLVE, ids=[f"{n}-P{o}" for n, o in _SOLVE])
def test_jacobi_pcg(name, order):
    """(c) the oracle's Jacobi PCG on the oracle's system: +-2 iterations, 1e-6 in the solution"""
    C = H.case(name, order, "elasticity")
    ov, ob = H.oracle(C)
    oit, ou, _, _ = zo.pcg(C.rowptr, C.cols, ov, ob, rtol=1e-8)
    for renumber in (None, "2"):
        with zzz.Context(0) as c:
            _upload(c, C, renumber)
            _assembled(c, C)
            it, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
            u = c.vec_download(zzz.VEC_U)
        print(f"\nHOSTILE elasticity solve {name} P{order} {'bins' if renumber else 'default'}: oracle {oit}, gpu {it}, "
              f"|u - ou| / |ou| {np.linalg.norm(u - ou) / np.linalg.norm(ou):.1e}")
        assert abs(it - oit) <= 2
        assert np.linalg.norm(u - ou) <= 1e-6 * np.linalg.norm(ou)


_LIFT = [(p, n, o) for p in ("poisson", "elasticity") for n, o in H.LIFTING_CASES[p]]


@pytest.mark.parametrize("problem,name,order", _LIFT, ids=[f"{p}-{n}-P{o}" for p, n, o in _LIFT])
def test_lifted_vector_against_the_50_digit_reference(problem, name, order):
    """(d) u0 is seeded noise at every dof with NaN at a few unconstrained entries (they must never be read).  b with the
    values against the lifted reference at the bar of (a), b[bc] == u0[bc] exactly, the same bits from a second assembly, and
    once the values are cleared the vector has the bits it had before them."""
    C = H.case(name, order, problem)
    ref = H.reference(C)
    bcb = C.bc.astype(bool)
    rng = np.random.default_rng(11 * order + C.bs)
    g = rng.standard_normal(C.n)
    g[rng.choice(np.nonzero(~bcb)[0], size=7, replace=False)] = np.nan
    r, s, fo = H.lifted_reference(C, g)
    assert np.all(s[~bcb] > 0) and np.all(s[bcb] == 0) and np.isfinite(r).all() and fo <= 100
    for renumber in (None, "2"):
        with zzz.Context(0) as c:
            _upload(c, C, renumber)
            c.pattern_build()
            c.assemble_vector(C.form)
            b0 = c.vec_download(zzz.VEC_B)
            c.upload_bc_values(g)
            c.assemble_vector(C.form)
            b = c.vec_download(zzz.VEC_B)
            c.assemble_vector(C.form)
            b2 = c.vec_download(zzz.VEC_B)
            c.upload_bc_values(None)
            c.assemble_vector(C.form)
            b1 = c.vec_download(zzz.VEC_B)
        assert np.isfinite(b).all()
        fig, fig0 = hp.metric(b, r, s) / hp.U, hp.metric(b0, ref["r"], ref["s"]) / hp.U
        print(f"\nHOSTILE lifting {problem:10s} {name:10s} P{order} {'bins   ' if renumber else 'default'} | b {fig:8.2f} {fo:7.2f}"
              f" | without values {fig0:8.2f} {ref['oracle_b']:7.2f}")
        assert np.array_equal(b[bcb], g[bcb])
        assert np.array_equal(b2, b)
        assert np.array_equal(b1, b0)
        # the lifting did something (how much is the figure's business: on the Kuhn lattice of `aniso` a Poisson row couples
        # to the constrained faces through G_xx ~ 2^-40 alone and the lift is 1e-25 of the row's scale)
        assert not np.array_equal(b[~bcb], b0[~bcb]) and not np.array_equal(r[~bcb], ref["r"][~bcb])
        assert fig <= _bar(fo), (fig, fo)
        assert fig0 <= _bar(ref["oracle_b"]), (fig0, ref["oracle_b"])


def _nullspace_bar(C, X):
    """The bar of |B - OB| / max|OB|: 1e-12, the bar of test_elasticity_p1_near_nullspace, wherever the input allows it.

    At P2 it does: the nodes are mid-points of dyadic vertices, exact doubles whoever tabulates them.  A P3 edge or face node
    is no double, and two correct tabulations of it differ.  With ulp = the spacing of the doubles at max|x|:
      - H.dof_coords takes x_0 + sum X_al (x_al - x_0): the differences are exact or small, one rounding at the size of x
        is left -- 0.5 ulp;
      - the library (k_nn_dof_coords) and the oracle's own zo_build_dofmap take sum_k w_k x_k: up to three products rounded
        at the size of x (1.5 ulp), the rounding of the weights (sum |w_k x_k| 2^-53 = 0.5 ulp), two sums (1 ulp) -- 3 ulp;
    so a coordinate may differ by delta = 4 ulp (rounded up), the centre of the dofs by as much, a coordinate relative to
    the centre -- an entry of a rotation before it is orthonormalised -- by 2 delta.  An orthonormalised rotation is that
    vector less its projections on the modes before it, over its norm; projections and norm move by no more, relative to
    the vector, than its entries do: a factor 2.  Its largest entry is r_max = max |x - centre| over the same norm, and
    max|OB| is at least that, so

        |B - OB| / max|OB| <= 2 x 2 delta / r_max = 16 ulp / r_max.

    `graded` P3 (|x| <= 1): 5e-15, the bar stays 1e-12.  `offset` P3 (ulp of 65 536 = 1.46e-11, r_max = 0.5): 4.7e-10.
    Measured there: 2.67e-11 on the MI355X -- and the ORACLE against ITSELF, fed the nodes in the two forms above (they
    differ by one ulp), 2.67e-11 as well: at 1e-12 that case would judge the rounding of the reference's input."""
    if C.order < 3:
        return 1e-12
    return max(1e-12, 16.0 * np.spacing(np.abs(X).max()) / np.abs(X - X.mean(axis=0)).max())


@pytest.mark.parametrize("name,order", [("offset", 2), ("aniso", 2), ("offset", 3), ("graded", 3)])
def test_near_nullspace_at_p2_and_p3(name, order):
    """(e) the six orthonormalised rigid-body modes of the P2 / P3 dof coordinates of the MAPPED mesh against the oracle's, at
    the bars of test_elasticity_p1_near_nullspace: deviation from orthonormality and |B B^T - I| within 1e-12 in every case
    (they do not depend on how the reference's input is rounded; `offset` is the mesh on which the rotations about the
    origin missed them), |B - OB| within _nullspace_bar.  `graded` is there because its dofs do not sit where the map sends
    the base's (H.dof_coords)."""
    C = H.case(name, order, "elasticity")
    X = H.dof_coords(C)
    OB, odev = zo.near_nullspace(X)
    bar = _nullspace_bar(C, X)
    for renumber in (None, "2"):
        with zzz.Context(0) as c:
            _upload(c, C, renumber)
            B, dev = c.near_nullspace()
        print(f"\nHOSTILE nullspace {name} P{order} {'bins' if renumber else 'default'}: |B - OB| {np.abs(B - OB).max() / np.abs(OB).max():.2e}"
              f" (bar {bar:.1e}) deviation {dev:.2e} (oracle {odev:.2e}) |B B^T - I| {np.abs(B @ B.T - np.eye(6)).max():.2e}")
        assert dev <= 1e-12 and odev <= 1e-12
        assert np.abs(B @ B.T - np.eye(6)).max() <= 1e-12
        assert np.abs(B - OB).max() <= bar * np.abs(OB).max()
