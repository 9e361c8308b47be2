"""GPU tests of the single-precision cgpoisson path: zzz_action_f32 and zzz_cg_solve_f32 (T = float of
src/cgpoisson_problem.cpp:28, U = float of src/cg.h:18-86) and the driver's --scalar_type float32.

Bounds, all scaled from the numpy float32 restatement of tests/_f32_ref.py (which shares no code with the library):
  action   max|y32 - y64| / max|y64| against the oracle's double action <= 4 x the restatement's figure on the same input (the
           float-geometry form for P1, float32(A_e) . float32(u_e) otherwise).  The margin covers another summation order,
           the factorised tables and fused multiply-adds -- not a wrong digit.
  cg.h     100 iterations as the oracle; final <r,r>/<r0,r0> within a factor 1.5 of the double solve's;
           |u32 - u64| / |u64| <= 10 x the restatement's own float-against-double difference on that case (CG amplifies
           rounding, hence the wider margin).
Every test prints its figures before it asserts; what is known of them: DESIGN.md 4e."""
import subprocess

from _gpu_helpers import *  # noqa: F401,F403 -- helpers, fixtures (ctx), np / os / zzz / zo

import _f32_ref as fr

pytestmark = pytest.mark.gpu  # noqa: F405

CGH = dict(variant=zzz.CG_CGH, pc=zzz.PC_NONE, op=zzz.OP_MATFREE, rtol=1e-6, max_it=100)  # noqa: F405


class _Env:
    """ZZZ_MF_NC for the plans built inside the block"""

    def __init__(self, nc):
        self.nc = nc

    def __enter__(self):
        self.old = os.environ.get("ZZZ_MF_NC")
        os.environ.pop("ZZZ_MF_NC", None)
        if self.nc:
            os.environ["ZZZ_MF_NC"] = str(self.nc)

    def __exit__(self, *a):
        os.environ.pop("ZZZ_MF_NC", None)
        if self.old is not None:
            os.environ["ZZZ_MF_NC"] = self.old


def _part(kind, order, dims):
    return zzz.Part.spoke("poisson", order, dims) if kind == "spoke" else zzz.Part("poisson", order, *dims)


@pytest.mark.parametrize("kind,order,dims", [("cube", 1, (12, 10, 14)), ("cube", 1, (40, 38, 42)), ("cube", 2, (12, 11, 13)),
                                             ("cube", 3, (8, 7, 9)), ("spoke", 1, 3), ("spoke", 2, 3)])
def test_float_action_against_the_double_oracle(ctx, kind, order, dims):
    zo.set_num_threads(8)
    P = _part(kind, order, dims)
    bc = P.bc_marker()
    u = fr.noise(P.n_owned)
    oy = zo.action_poisson(order, P.x, P.cells, P.cell_dofs, bc, u)
    if order == 1:
        ry = fr.action32_p1_geometry(P.x, P.cells, P.cell_dofs, bc, u)
    else:
        ry = fr.action(fr.element_matrices(order, P.x, P.cells), P.cell_dofs, bc, u, np.float32)
    ref_err = np.abs(ry - oy).max() / np.abs(oy).max()
    with _Env(256):
        ctx.upload_part(P)
        ctx.matfree_setup()
        info = ctx.matfree_info()
        # at least three blocks, dofs shared between them, a partial last block
        assert info["valid"] == 1 and info["blocks"] >= 3 and info["shared_dofs"] > 0
        assert P.ncells % info["cells_per_block"] != 0
        assert ctx.matfree_info_f32()["built"] == 0
        y64 = ctx.action(u)
        y32 = ctx.action_f32(u.astype(np.float32))
        f = ctx.matfree_info_f32()
        assert f["built"] == 1 and 0 < f["bytes_per_action"] < info["bytes_per_action"]
        assert f["lds_bytes"] == {1: 20, 2: 8, 3: 4}[order] * info["nloc_max"] and f["workgroups_per_cu"] >= 1
        assert y32.dtype == np.float32
        err = np.abs(y32 - oy).max() / np.abs(oy).max()
        print(f"{kind} P{order} {dims}: float action error {err:.3e}, restatement {ref_err:.3e}, blocks {info['blocks']}")
        assert err <= 4 * ref_err
        assert np.all(y32[bc.astype(bool)] == 0)
        np.testing.assert_array_equal(ctx.action_f32(u.astype(np.float32)), y32)  # the same bits every time
        np.testing.assert_array_equal(ctx.action(u), y64)  # the double action before and after: the same bits


@pytest.mark.parametrize("order,dims", [(1, (24, 22, 23)), (2, (12, 11, 13)), (3, (8, 7, 9))])
def test_float_cg_against_the_double_oracle(ctx, order, dims):
    zo.set_num_threads(8)
    P = zzz.Part("poisson", order, *dims)
    bc = P.bc_marker()
    ob = zo.assemble_vector(0, order, P.x, P.cells, P.cell_dofs, P.f, P.g, P.facets, bc)
    ok, ou = zo.cg_matfree_poisson(order, P.x, P.cells, P.cell_dofs, bc, ob, kmax=100, rtol=1e-6)
    (k64, _, h64), _ = fr.cg_pair(order, dims)  # cg.h in double on the oracle's element matrices: the residual history
    assert ok == 100 and k64 == 100
    with _Env(0):
        ctx.upload_part(P)
        ctx.vec_upload(zzz.VEC_B, ob)
        ctx.vec_upload(zzz.VEC_U, np.zeros(P.n_owned))
        k, rr, rr0 = ctx.cg_solve_f32(**CGH)
        u32 = ctx.vec_download(zzz.VEC_U)
        hist = ctx.cg_history(k + 1)
        assert k == ok and ctx.cg_reason() == -3
        assert hist[0] == rr0 and hist[-1] == rr
        ratio, oratio = rr / rr0, h64[-1] / h64[0]
        diff = np.linalg.norm(u32 - ou) / np.linalg.norm(ou)
        print(f"P{order} {dims}: residual ratio {ratio:.4e} (double {oratio:.4e}), |u32 - u64| / |u64| = {diff:.3e} "
              f"(restatement {fr.SOLUTION_DIFF[(order, dims)]:.1e})")
        assert oratio / 1.5 <= ratio <= oratio * 1.5
        assert diff <= 10 * fr.SOLUTION_DIFF[(order, dims)]
        down = np.diff(h64) < 0  # monotone where the oracle's is
        assert np.all(np.diff(hist)[down] < 0)
        # a second identical solve: identical bits
        ctx.vec_upload(zzz.VEC_U, np.zeros(P.n_owned))
        k2, rr2, _ = ctx.cg_solve_f32(**CGH)
        assert k2 == k and rr2 == rr
        np.testing.assert_array_equal(ctx.vec_download(zzz.VEC_U), u32)
        np.testing.assert_array_equal(ctx.cg_history(k + 1), hist)


def test_float_cg_converges_with_the_double_count(ctx):
    order, dims = fr.CONVERGING
    P = zzz.Part("poisson", order, *dims)
    bc = P.bc_marker()
    ob = zo.assemble_vector(0, order, P.x, P.cells, P.cell_dofs, P.f, P.g, P.facets, bc)
    ok, ou = zo.cg_matfree_poisson(order, P.x, P.cells, P.cell_dofs, bc, ob, kmax=100, rtol=1e-6)
    ctx.upload_part(P)
    ctx.vec_upload(zzz.VEC_B, ob)
    ctx.vec_upload(zzz.VEC_U, np.zeros(P.n_owned))
    k, rr, rr0 = ctx.cg_solve_f32(**CGH)
    print(f"converging case P{order} {dims}: {k} iterations in float, {ok} in double")
    assert ok < 100 and abs(k - ok) <= 2 and ctx.cg_reason() == 2
    assert rr / rr0 < 1e-12 and len(ctx.cg_history(k + 1)) == k + 1
    assert np.linalg.norm(ctx.vec_download(zzz.VEC_U) - ou) <= 1e-4 * np.linalg.norm(ou)


def test_the_double_path_is_untouched_by_a_float_solve():
    P = zzz.Part("poisson", 2, 7, 6, 8)
    with zzz.Context(0) as c:
        c.upload_part(P)
        c.pattern_build()  # the right-hand side's assembly walks the dof -> cell adjacency
        c.assemble_vector(zzz.FORM_POISSON)

        def double_solve(**kw):
            c.vec_upload(zzz.VEC_U, np.zeros(P.n_owned))
            k, rr, rr0 = c.cg_solve(**kw)
            return k, rr, rr0, c.cg_history(k + 1), c.vec_download(zzz.VEC_U)

        before = double_solve(**CGH)
        jac_before = double_solve(pc=zzz.PC_JACOBI, op=zzz.OP_MATFREE, rtol=1e-8)
        assert c.matfree_info_f32()["built"] == 0
        c.vec_upload(zzz.VEC_U, np.zeros(P.n_owned))
        k32, _, _ = c.cg_solve_f32(**CGH)
        assert k32 > 0 and c.matfree_info_f32()["built"] == 1
        for a, b in zip(before, double_solve(**CGH)):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(jac_before, double_solve(pc=zzz.PC_JACOBI, op=zzz.OP_MATFREE, rtol=1e-8)):
            np.testing.assert_array_equal(a, b)


def test_float_solve_declines_what_it_does_not_serve():
    P = zzz.Part("poisson", 1, 6, 5, 7)
    with zzz.Context(0) as c:
        c.upload_part(P)
        c.pattern_build()
        c.assemble_matrix(zzz.FORM_POISSON)
        c.assemble_vector(zzz.FORM_POISSON)

        def declined(word, **kw):
            with pytest.raises(zzz.ZzzError) as e:
                c.cg_solve_f32(**kw)
            assert e.value.code == 1 and word in str(e.value), str(e.value)

        declined("operator", op=zzz.OP_CSR)
        declined("variant", variant=zzz.CG_PETSC)
        declined("preconditioner", pc=zzz.PC_JACOBI)
        declined("single_reduction", single_reduction=True)
        c.upload_bc_values(np.full(P.n_owned, 0.25))
        declined("Dirichlet values")
        c.upload_bc(P.bc_dofs)  # (a new Dirichlet set: the values are gone)
        c.assemble_vector(zzz.FORM_POISSON)
        # ... and the context solves in double as usual, and in float
        c.vec_upload(zzz.VEC_U, np.zeros(P.n_owned))
        k64, _, _ = c.cg_solve(**CGH)
        u64 = c.vec_download(zzz.VEC_U)
        c.vec_upload(zzz.VEC_U, np.zeros(P.n_owned))
        k32, _, _ = c.cg_solve_f32(**CGH)
        assert 0 < k64 < 100 and abs(k32 - k64) <= 2
        assert np.linalg.norm(c.vec_download(zzz.VEC_U) - u64) <= 1e-4 * np.linalg.norm(u64)
    # an elasticity context
    E = zzz.Part("elasticity", 1, 4, 3, 5)
    with zzz.Context(0) as c:
        c.upload_part(E)
        c.pattern_build()
        c.assemble_vector(zzz.FORM_ELASTICITY)
        with pytest.raises(zzz.ZzzError) as e:
            c.cg_solve_f32(**CGH)
        assert e.value.code == 1 and "block size 3" in str(e.value)
        with pytest.raises(zzz.ZzzError) as e:
            c.action_f32(np.zeros(E.n_owned * 3, np.float32))
        assert e.value.code == 1 and "block size 3" in str(e.value)
        c.assemble_matrix(zzz.FORM_ELASTICITY)
        it, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
        assert it > 0
    # a one-rank communicator attached (as tests/test_gpu_cg.py::test_rccl_path_single_rank attaches it)
    with zzz.Context(0) as c:
        c.comm_init(1, 0, zzz.comm_unique_id())
        c.upload_part(P)
        c.upload_halo(P)
        c.pattern_build()
        c.assemble_vector(zzz.FORM_POISSON)
        with pytest.raises(zzz.ZzzError) as e:
            c.cg_solve_f32(**CGH)
        assert e.value.code == 1 and "communicator" in str(e.value)
        c.vec_upload(zzz.VEC_U, np.zeros(P.n_owned))
        k, _, _ = c.cg_solve(**CGH)
        assert 0 < k < 100


def test_driver_scalar_type():
    exe = os.path.join(zzz.PKG, "dolfinx-scaling-test")
    base = [exe, "--problem_type", "cgpoisson", "--ndofs", "50000", "--order", "2"]

    def run(extra, cmd=base):
        return subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300)

    d = run([])
    f = run(["--scalar_type", "float32"])
    assert d.returncode == 0 and f.returncode == 0, (d.stderr, f.stderr)
    assert "  Scalar type:     float32\n" in f.stdout and "Scalar type" not in d.stdout
    its = lambda s: int(s.split("*** Number of Krylov iterations: ")[1].split()[0])
    nrm = lambda s: float(s.split("*** Solution norm:  ")[1].split()[0])
    print("driver: iterations", its(d.stdout), its(f.stdout), "norms", nrm(d.stdout), nrm(f.stdout))
    assert its(f.stdout) == 100 and its(d.stdout) == 100
    assert abs(nrm(f.stdout) - nrm(d.stdout)) <= 1e-4 * nrm(d.stdout)
    assert "CG matrix-free action processed: " in f.stdout
    # the explicit default is the default
    assert run(["--scalar_type", "float64"]).stdout.count("Scalar type") == 0
    for extra, cmd, word in ((["--scalar_type", "float32"], [exe, "--problem_type", "poisson", "--ndofs", "20000"], "cgpoisson"),
                             (["--scalar_type", "float32", "--ngpus", "2", "--comm", "local"], base, "ngpus"),
                             (["--scalar_type", "half"], base, "float64 or float32")):
        bad = run(extra, cmd)
        assert bad.returncode != 0 and word in bad.stderr, (extra, bad.stderr)
