"""GPU parity tests of -pc_type pmg (ZZZ_PC_PMG: csrc/zzz_pmg.hip in front of csrc/zzz_mg.hip) through the C-ABI against its
numpy / scipy restatement (tests/_pmg_ref.py, pinned on the CPU by tests/test_pmg_ref.py), against the oracle's tight Jacobi
solve and against the library's own Jacobi solve.

Cases: all axes unequal, so a swapped axis or a PX / nx slip shows; (3, 2, 4) at P3 is the smallest cube on which every entity
type has interior and cut-off instances.

Bars, those of tests/test_gpu_mg.py for the same reasons (none comes from what the code under test gives):
  transfer    1e-13 of max |out|: a sum of at most 65 terms, which rounding cannot reach; adjointness 1e-13 on noise; the
              restriction bit-identical between two calls; exactly 0.0 on constrained dofs.
  V-cycle     relative l2 difference to the restated cycle, fed with the library's own bounds, at most 1e-9; symmetry defect at
              most 1e-12 on noise, <M a, a> > 0; bit-identical on repeat.
  solves      iterations within +-1 of the restatement's, the solution within 1e-6 relative of zo.pcg at rtol 1e-12, fewer than
              a tenth of the library's own Jacobi iterations, reason 2, history iterations + 1 long.
  full size   the cube of bench.py's c5_rank record (Poisson P3, 61^3 cells, 6.2 M dofs) in at most 26 iterations: twice the
              restatement's 13, the rule of test_gpu_mg.py's full-size caps (the restatement's count did not grow from 910 to
              438 k dofs); within 1e-6 of Jacobi's solution; the count at this size is unmeasured.

The observed differences are printed before they are asserted; none is recorded yet: this file has not run on an MI355X
(DESIGN.md section 5c)."""
import os
import subprocess

import numpy as np
import pytest

import zzz
import zzz_oracle as zo
from _mg_ref import level_dims, pcg
from _pmg_ref import PHierarchy

pytestmark = pytest.mark.gpu

SOLVE_CASES = [("poisson", 2, (12, 10, 14)), ("poisson", 3, (8, 7, 9)), ("elasticity", 2, (10, 9, 8)), ("elasticity", 3, (6, 5, 7))]
TRANSFER_CASES = SOLVE_CASES + [("poisson", 3, (3, 2, 4))]


def _generated(c, kind, order, n, rhs=True):
    form = zzz.FORM_ELASTICITY if kind == "elasticity" else zzz.FORM_POISSON
    c.cube_generate(kind, order, *n)
    c.pattern_build()
    c.assemble_matrix(form)
    if rhs:
        c.assemble_vector(form)
    return form


_ref = {}


def _hierarchy(c, kind, order, n):
    """the restatement with the library's own bounds"""
    nl = c.mg_info()["levels"]
    his = tuple(c.mg_info(l)["hi"] for l in range(nl - 1))
    key = (kind, order, n, his)
    if key not in _ref:
        _ref[key] = PHierarchy(kind, order, n, his=his)
    return _ref[key]


@pytest.mark.parametrize("kind,order,n", TRANSFER_CASES)
def test_info_transfer_cycle_and_symmetry(kind, order, n):
    zo.set_num_threads(4)
    rng = np.random.default_rng(13)
    bs = 3 if kind == "elasticity" else 1
    with zzz.Context(0) as c:
        _generated(c, kind, order, n, rhs=False)
        c.mg_setup(pc=zzz.PC_PMG)
        info = c.mg_info()
        assert info["levels"] == 1 + len(level_dims(n, bs)) and info["high_order_levels"] == 1 and info["setups"] == 1
        assert info["products_per_cycle"] == 4
        H = _hierarchy(c, kind, order, n)
        assert H.spread <= 1e-15
        l0, l1 = c.mg_info(0), c.mg_info(1)
        assert l0["dofs"] == H.A.shape[0] == c.n_owned * bs and l0["nnz"] == H.cols.size
        assert l0["cells"] == n and l1["cells"] == n and l1["dofs"] == H.H1.A[0].shape[0]
        assert (l0["degree"], l0["lo"] > 0) == (2, True)
        for l, d in enumerate(H.dims):
            assert c.mg_info(l)["cells"] == d
        # 1. the transfer between the Pk and the P1 level, then the P1 levels' own
        bcf, bcc = H.bc.astype(bool), H.H1.probs[0].bc.astype(bool)
        for l, P in enumerate([H.P] + list(H.H1.P)):
            e, r = rng.standard_normal(P.shape[1]), rng.standard_normal(P.shape[0])
            pe, ptr = c.mg_transfer(l, 0, e), c.mg_transfer(l, 1, r)
            d0 = np.abs(pe - P @ e).max() / np.abs(pe).max()
            d1 = np.abs(ptr - P.T @ r).max() / np.abs(ptr).max()
            adj = abs(pe @ r - e @ ptr) / (np.linalg.norm(pe) * np.linalg.norm(r))
            print(f"pmg transfer {kind} P{order} {n} level {l}: prolongation {d0:.2e}, restriction {d1:.2e}, adjointness {adj:.2e}")
            assert d0 <= 1e-13 and d1 <= 1e-13 and adj <= 1e-13
            assert np.array_equal(ptr, c.mg_transfer(l, 1, r))
            if l == 0:
                assert bcf.any() and bcc.any() and np.all(pe[bcf] == 0.0) and np.all(ptr[bcc] == 0.0)
        # 2. one V-cycle against the restated one
        a, b = rng.standard_normal(H.A.shape[0]), rng.standard_normal(H.A.shape[0])
        Ma, Mb = c.mg_apply(a), c.mg_apply(b)
        ref = H.vcycle(a)
        dv = np.linalg.norm(Ma - ref) / np.linalg.norm(ref)
        print(f"pmg V-cycle {kind} P{order} {n}: relative l2 difference to the restatement {dv:.2e}")
        assert dv <= 1e-9
        # 3. symmetric and positive on the device, the same bits on repeat
        sym = abs(Ma @ b - a @ Mb) / (np.linalg.norm(Ma) * np.linalg.norm(b))
        print(f"pmg V-cycle {kind} P{order} {n}: symmetry defect {sym:.2e}")
        assert sym <= 1e-12 and Ma @ a > 0.0 and Mb @ b > 0.0
        assert np.array_equal(Ma, c.mg_apply(a))


@pytest.mark.parametrize("kind,order,n", SOLVE_CASES)
def test_solves_with_every_norm_type(kind, order, n):
    zo.set_num_threads(4)
    with zzz.Context(0) as c:
        _generated(c, kind, order, n)
        rp, cl, v = c.csr_download()
        b = c.vec_download(zzz.VEC_B)
        _, xt, _, _ = zo.pcg(rp.astype(np.int64), cl, v, b, rtol=1e-12)
        itj, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
        H = None
        for norm in (zzz.NORM_PRECONDITIONED, zzz.NORM_UNPRECONDITIONED, zzz.NORM_NATURAL):
            it, rn, r0 = c.cg_solve(pc=zzz.PC_PMG, norm=norm, rtol=1e-8)
            u = c.vec_download(zzz.VEC_U)
            longer = c.cg_history(it + 5)  # (the library copies min(n, iterations + 1) entries)
            assert np.all(longer[it + 1:] == 0.0) and longer[it] > 0.0
            hist = longer[:it + 1]
            H = H or _hierarchy(c, kind, order, n)
            ito, xo, histo = pcg(H.A, b, H.vcycle, norm_type=norm, rtol=1e-8)
            err = np.linalg.norm(u - xt) / np.linalg.norm(xt)
            print(f"pmg solve {kind} P{order} {n} norm {norm}: gpu {it}, restatement {ito}, jacobi {itj}; |u-xt|/|xt| {err:.2e}")
            assert abs(it - ito) <= 1
            assert err <= 1e-6
            assert 10 * it < itj
            assert c.cg_info()["reason"] == 2
            assert hist.shape[0] == it + 1 and hist[0] == r0 and hist[-1] == rn and rn <= 1e-8 * r0
            assert abs(r0 - histo[0]) <= 1e-9 * histo[0]


def test_order_one_is_pc_mg_bit_for_bit():
    kind, n = "poisson", (12, 10, 14)
    got = []
    for pc in (zzz.PC_MG, zzz.PC_PMG):
        with zzz.Context(0) as c:
            _generated(c, kind, 1, n)
            it, rn, r0 = c.cg_solve(pc=pc, rtol=1e-8)
            info = c.mg_info()
            assert info["high_order_levels"] == 0 and info["levels"] == len(level_dims(n, 1))
            got.append((it, rn, r0, c.cg_history(it + 1), c.vec_download(zzz.VEC_U), [c.mg_info(l) for l in range(info["levels"])]))
    (it0, rn0, r00, h0, u0, lv0), (it1, rn1, r01, h1, u1, lv1) = got
    assert (it0, rn0, r00) == (it1, rn1, r01) and np.array_equal(h0, h1) and np.array_equal(u0, u1) and lv0 == lv1


def test_hierarchy_is_kept_refreshed_and_not_leaked():
    kind, order, n = "poisson", 2, (12, 10, 14)
    with zzz.Context(0) as c:
        form = _generated(c, kind, order, n)
        it1, _, _ = c.cg_solve(pc=zzz.PC_PMG)
        h1, u1 = c.cg_history(it1 + 1), c.vec_download(zzz.VEC_U)
        free1 = zzz.device_memory(0)[0]
        it2, _, _ = c.cg_solve(pc=zzz.PC_PMG)
        assert it2 == it1 and np.array_equal(h1, c.cg_history(it2 + 1)) and np.array_equal(u1, c.vec_download(zzz.VEC_U))
        assert c.mg_info()["setups"] == 1
        # a second assembly: the values are refreshed, the levels stay
        c.assemble_matrix(form)
        it3, _, _ = c.cg_solve(pc=zzz.PC_PMG)
        assert it3 == it1 and np.linalg.norm(c.vec_download(zzz.VEC_U) - u1) <= 1e-12 * np.linalg.norm(u1)
        assert c.mg_info()["setups"] == 2 and c.mg_info()["levels"] == 1 + len(level_dims(n, 1))
        for _ in range(8):
            c.cg_solve(pc=zzz.PC_PMG)
        used1 = zzz.device_memory(0)[1] - free1
        used10 = zzz.device_memory(0)[1] - zzz.device_memory(0)[0]
        print(f"pmg device memory in use after the first solve {used1}, after ten solves and a refresh {used10}")
        assert abs(used10 - used1) <= 0.01 * used1
        # a new feed of another order: the hierarchy is rebuilt for it
        n3 = (8, 7, 9)
        _generated(c, kind, 3, n3)
        it4, _, _ = c.cg_solve(pc=zzz.PC_PMG)
        info = c.mg_info()
        assert c.mg_info(0)["cells"] == n3 and c.mg_info(0)["dofs"] == c.n_owned and info["setups"] == 1 and it4 <= 19
        assert info["levels"] == 1 + len(level_dims(n3, 1)) and info["high_order_levels"] == 1
        # ... and an order-1 feed gets ZZZ_PC_MG's
        _generated(c, kind, 1, n)
        assert c.cg_solve(pc=zzz.PC_PMG)[0] <= 12 and c.mg_info()["high_order_levels"] == 0


def test_level_options():
    kind, order, n = "elasticity", 2, (6, 5, 7)
    with zzz.Context(0) as c:
        _generated(c, kind, order, n)
        rp, cl, v = c.csr_download()
        b = c.vec_download(zzz.VEC_B)
        _, xt, _, _ = zo.pcg(rp.astype(np.int64), cl, v, b, rtol=1e-12)
        for kw in (dict(), dict(pc_mg_levels=2), dict(pc_mg_levels=3, pc_mg_coarse_eq_limit=200), dict(pc_mg_coarse_eq_limit=200),
                   dict(pc_degree=3, pc_ratio=20.0)):
            it, _, _ = c.cg_solve(pc=zzz.PC_PMG, **kw)
            lv, limit = kw.get("pc_mg_levels", 0), kw.get("pc_mg_coarse_eq_limit", 0) or 1000
            dims = [n] + level_dims(n, 3, limit=limit, max_levels=lv - 1 if lv else 0)
            info = c.mg_info()
            assert info["levels"] == len(dims) and [c.mg_info(l)["cells"] for l in range(len(dims))] == dims, (kw, info, dims)
            assert c.mg_info(0)["degree"] == (kw.get("pc_degree") or 2)
            # the restatement under the same options and the library's bounds
            H = PHierarchy(kind, order, n, his=[c.mg_info(l)["hi"] for l in range(len(dims) - 1)], degree=kw.get("pc_degree") or 2,
                           ratio=kw.get("pc_ratio") or 10.0, limit=limit, max_levels=lv)
            ito, _, _ = pcg(H.A, b, H.vcycle, rtol=1e-8)
            print(f"pmg options {kw}: levels {dims}, gpu {it}, restatement {ito}")
            assert H.dims == dims and abs(it - ito) <= 1 and c.cg_info()["reason"] == 2
            u = c.vec_download(zzz.VEC_U)
            assert np.linalg.norm(u - xt) <= 1e-6 * np.linalg.norm(xt)


def test_declined_combinations_leave_the_context_usable():
    zo.set_num_threads(4)

    def declined(c, **kw):
        with pytest.raises(zzz.ZzzError) as e:
            c.cg_solve(**dict(dict(pc=zzz.PC_PMG), **kw))
        assert e.value.code == 1 and len(str(e.value)) > len("libzzz_hip error 1: "), str(e.value)
        return str(e.value)

    def jacobi_as_usual(c):
        rp, cl, v = c.csr_download()
        oit, ou, _, _ = zo.pcg(rp.astype(np.int64), cl, v, c.vec_download(zzz.VEC_B), rtol=1e-8)
        it, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
        assert abs(it - oit) <= 2 and np.linalg.norm(c.vec_download(zzz.VEC_U) - ou) <= 1e-6 * np.linalg.norm(ou)

    with zzz.Context(0) as c:
        _generated(c, "poisson", 2, (12, 10, 14))
        assert "MATFREE" in declined(c, op=zzz.OP_MATFREE)
        assert "single_reduction" in declined(c, single_reduction=True)
        assert "pipecg" in declined(c, variant=zzz.CG_PIPE)
        declined(c, variant=zzz.CG_CGH)
        assert "pc_mg_levels" in declined(c, pc_mg_levels=1)
        # -pc_type mg keeps declining the order, and says where to go
        with pytest.raises(zzz.ZzzError) as e:
            c.cg_solve(pc=zzz.PC_MG)
        assert e.value.code == 1 and "P1 only" in str(e.value) and "pmg" in str(e.value)
        jacobi_as_usual(c)
        assert c.cg_solve(pc=zzz.PC_PMG)[0] <= 12
    # an uploaded feed (the same cube built on the host)
    P = zzz.Part("poisson", 2, 4, 3, 5)
    with zzz.Context(0) as c:
        c.upload_part(P)
        c.pattern_build()
        c.assemble_matrix(P.form)
        c.assemble_vector(P.form)
        assert "zzz_cube_generate" in declined(c)
        jacobi_as_usual(c)
    # a communicator attached (one rank, as tests/test_gpu_cg.py::test_rccl_path_single_rank attaches it)
    with zzz.Context(0) as c:
        c.comm_init(1, 0, zzz.comm_unique_id())
        _generated(c, "poisson", 2, (12, 10, 14))
        assert "communicator" in declined(c)
        jacobi_as_usual(c)


def test_full_size():
    kind, order = "poisson", 3
    n = tuple(zzz.mesh_size(6250000, True, 1, 1, 3)[:3])  # bench.py's c5_rank record
    assert n == (61, 61, 61)
    with zzz.Context(0) as c:
        _generated(c, kind, order, n)
        itj, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
        uj = c.vec_download(zzz.VEC_U)
        it, rn, r0 = c.cg_solve(pc=zzz.PC_PMG, rtol=1e-8)
        u = c.vec_download(zzz.VEC_U)
        err = np.linalg.norm(u - uj) / np.linalg.norm(uj)
        info = c.mg_info()
        print(f"pmg full size {kind} P{order} {n}: {c.n_owned} dofs, {info['levels']} levels, coarsest {info['coarse_dofs']} dofs, "
              f"pmg {it} iterations, jacobi {itj}; |u-uj|/|uj| {err:.2e}")
        assert it <= 26 and c.cg_info()["reason"] == 2
        assert err <= 1e-6
        assert info["levels"] == 1 + len(level_dims(n, 1)) and info["high_order_levels"] == 1


def test_driver():
    exe = os.path.join(zzz.PKG, "dolfinx-scaling-test")

    def run(args, ok=True):
        o = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert (o.returncode == 0) == ok, (args, o.stderr[-1000:])
        if not ok:
            return None
        return (int(o.stdout.split("*** Number of Krylov iterations: ")[1].split()[0]),
                float(o.stdout.split("*** Solution norm:  ")[1].split()[0]), o.stdout)

    for problem in ("poisson", "elasticity"):
        for order in (2, 3):
            base = ["--problem_type", problem, "--scaling_type", "weak", "--ndofs", "50000", "--order", str(order), "-ksp_type", "cg",
                    "-ksp_rtol", "1.0e-8"]
            itj, nj, _ = run(base + ["-pc_type", "jacobi"])
            itm, nm, out = run(base + ["-pc_type", "pmg", "-ksp_view"])
            print(f"driver {problem} P{order}: jacobi {itj} iterations, pmg {itm}; norms {nj} {nm}")
            assert abs(nm - nj) <= 1e-6 * nj and 10 * itm < itj
            assert "PC Object: type: pmg" in out and "dense direct solve" in out and "ZZZ Solve" in out
            assert f", order {order}, dofs" in out.split("  level 0: cells ")[1].split("\n")[0]
            assert ", order 1, dofs" in out.split("  level 1: cells ")[1].split("\n")[0]
    # order 1 through the same selector, and the level options
    base = ["--problem_type", "poisson", "--scaling_type", "weak", "--ndofs", "50000", "-ksp_rtol", "1.0e-8"]
    it1, n1, out1 = run(base + ["-pc_type", "pmg", "-ksp_view"])
    itg, ng, _ = run(base + ["-pc_type", "mg"])
    assert (it1, n1) == (itg, ng) and ", order 1, dofs" in out1.split("  level 0: cells ")[1].split("\n")[0]
    it2, n2, out2 = run(base + ["--order", "2", "-pc_type", "pmg", "-pc_mg_levels", "3", "-pc_mg_coarse_eq_limit", "4000",
                                "-mg_levels_ksp_max_it", "3", "-mg_levels_ksp_chebyshev_ratio", "20", "-ksp_view"])
    assert "degree 3" in out2 and "  level 3" not in out2 and "  level 2" in out2
    base = ["--problem_type", "poisson", "--ndofs", "50000", "--order", "2", "-pc_type", "pmg"]
    for bad in (["--mesh_type", "unstructured"], ["--ngpus", "2", "--comm", "local"], ["--operator", "matfree"],
                ["-ksp_type", "pipecg"], ["-ksp_cg_single_reduction"], ["-pc_mg_levels", "1"]):
        run(base + bad, ok=False)
    run(["--problem_type", "cgpoisson", "--ndofs", "50000", "--order", "2", "-pc_type", "pmg"], ok=False)
    o = subprocess.run([exe, "--ndofs", "50000", "-pc_type", "gamg"], capture_output=True, text=True, timeout=60)
    assert o.returncode != 0 and "-pc_type mg" in o.stderr and "pmg" in o.stderr
