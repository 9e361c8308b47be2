"""GPU parity tests of -pc_type mg (ZZZ_PC_MG, csrc/zzz_mg.hip) through the C-ABI against its numpy / scipy restatement
(tests/_mg_ref.py, pinned on the CPU by tests/test_mg_ref.py), against the oracle's tight Jacobi solve and against the
library's own Jacobi solve.

Bars (none comes from what the code under test gives):
  transfer    1e-13 of max |out|: a sum of at most about 30 terms, which rounding cannot reach; adjointness 1e-13 on noise;
              the restriction bit-identical between two calls.
  V-cycle     relative l2 difference to the restated cycle, fed with the library's own bounds, at most 1e-9: a few hundred
              backward-stable operations at 2^-53, amplified by at most the condition number of the coarsest solve (at most
              1e4 under the 1000-dof limit) stays under 1e-10; an algorithmic slip shows at 1e-2.
  symmetry    <M a, b> = <a, M b> to 1e-12 relative on noise, <M a, a> > 0.
  solves      iterations within +-1 of the restatement's, the solution within 1e-6 relative of zo.pcg at rtol 1e-12 (the
              project's solution bar), fewer than a tenth of the library's own Jacobi iterations, reason 2, history
              iterations + 1 long.
  full size   C2's cube at most 16 iterations (twice what the restatement needs at 40^3, 45x43x41 and 79^3: 8 each, and the
              count does not grow with the mesh), C4's 109^3 elasticity cube at most 24; both within 1e-6 of Jacobi's."""
import os
import subprocess

import numpy as np
import pytest

import zzz
import zzz_oracle as zo
from _mg_ref import Hierarchy, level_dims, pcg

pytestmark = pytest.mark.gpu

CASES = [("poisson", (45, 43, 41)), ("poisson", (40, 40, 40)), ("elasticity", (35, 33, 31))]


def _generated(c, kind, n, rhs=True):
    form = zzz.FORM_ELASTICITY if kind == "elasticity" else zzz.FORM_POISSON
    c.cube_generate(kind, 1, *n)
    c.pattern_build()
    c.assemble_matrix(form)
    if rhs:
        c.assemble_vector(form)
    return form


def _library_bounds(c):
    nl = c.mg_info()["levels"]
    return [c.mg_info(l)["hi"] for l in range(nl - 1)]


_ref = {}


def _hierarchy(c, kind, n, **kw):
    """the restatement with the library's own bounds"""
    his = _library_bounds(c)
    key = (kind, n, tuple(his), tuple(sorted(kw.items())))
    if key not in _ref:
        _ref[key] = Hierarchy(kind, n, his=his, **kw)
    return _ref[key]


@pytest.mark.parametrize("kind,n", CASES)
def test_transfer_cycle_and_symmetry(kind, n):
    zo.set_num_threads(4)
    rng = np.random.default_rng(11)
    with zzz.Context(0) as c:
        _generated(c, kind, n, rhs=False)
        c.mg_setup()
        H = _hierarchy(c, kind, n)
        info = c.mg_info()
        assert info["levels"] == len(H.dims) and info["setups"] == 1 and info["products_per_cycle"] == 4
        for l, d in enumerate(H.dims):
            li = c.mg_info(l)
            assert li["cells"] == d and li["dofs"] == H.A[l].shape[0] and li["nnz"] == H.probs[l].cols.size
            assert (li["degree"], li["lo"] > 0) == ((2, True) if l + 1 < len(H.dims) else (0, False))
        # 1. the transfer, both directions, every level
        for l, P in enumerate(H.P):
            e, r = rng.standard_normal(P.shape[1]), rng.standard_normal(P.shape[0])
            pe, ptr = c.mg_transfer(l, 0, e), c.mg_transfer(l, 1, r)
            d0 = np.abs(pe - P @ e).max() / np.abs(pe).max()
            d1 = np.abs(ptr - P.T @ r).max() / np.abs(ptr).max()
            adj = abs(pe @ r - e @ ptr) / (np.linalg.norm(pe) * np.linalg.norm(r))
            print(f"mg transfer {kind} {n} level {l}: prolongation {d0:.2e}, restriction {d1:.2e}, adjointness {adj:.2e}")
            assert d0 <= 1e-13 and d1 <= 1e-13 and adj <= 1e-13
            assert np.array_equal(ptr, c.mg_transfer(l, 1, r))
        # 2. one V-cycle against the restated one (the observed difference is printed; none is recorded yet: this file has not
        #    run on an MI355X)
        a, b = rng.standard_normal(H.A[0].shape[0]), rng.standard_normal(H.A[0].shape[0])
        Ma, Mb = c.mg_apply(a), c.mg_apply(b)
        ref = H.vcycle(a)
        dv = np.linalg.norm(Ma - ref) / np.linalg.norm(ref)
        print(f"mg V-cycle {kind} {n}: relative l2 difference to the restatement {dv:.2e}")
        assert dv <= 1e-9
        # 3. symmetric and positive on the device
        sym = abs(Ma @ b - a @ Mb) / (np.linalg.norm(Ma) * np.linalg.norm(b))
        print(f"mg V-cycle {kind} {n}: symmetry defect {sym:.2e}")
        assert sym <= 1e-12 and Ma @ a > 0.0 and Mb @ b > 0.0
        assert np.array_equal(Ma, c.mg_apply(a))


@pytest.mark.parametrize("kind,n", CASES)
def test_solves_with_every_norm_type(kind, n):
    zo.set_num_threads(4)
    with zzz.Context(0) as c:
        _generated(c, kind, n)
        rp, cl, v = c.csr_download()
        b = c.vec_download(zzz.VEC_B)
        _, xt, _, _ = zo.pcg(rp.astype(np.int64), cl, v, b, rtol=1e-12)
        itj, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
        H = None
        for norm in (zzz.NORM_PRECONDITIONED, zzz.NORM_UNPRECONDITIONED, zzz.NORM_NATURAL):
            it, rn, r0 = c.cg_solve(pc=zzz.PC_MG, norm=norm, rtol=1e-8)
            u = c.vec_download(zzz.VEC_U)
            longer = c.cg_history(it + 5)  # (the library copies min(n, iterations + 1) entries)
            assert np.all(longer[it + 1:] == 0.0) and longer[it] > 0.0
            hist = longer[:it + 1]
            H = H or _hierarchy(c, kind, n)
            ito, xo, histo = pcg(H.A[0], b, H.vcycle, norm_type=norm, rtol=1e-8)
            err = np.linalg.norm(u - xt) / np.linalg.norm(xt)
            print(f"mg solve {kind} {n} norm {norm}: gpu {it}, restatement {ito}, jacobi {itj}; |u-xt|/|xt| {err:.2e}")
            assert abs(it - ito) <= 1
            assert err <= 1e-6
            assert 10 * it < itj
            assert c.cg_info()["reason"] == 2
            assert hist.shape[0] == it + 1 and hist[0] == r0 and hist[-1] == rn and rn <= 1e-8 * r0
            assert abs(r0 - histo[0]) <= 1e-9 * histo[0]


def test_hierarchy_is_kept_refreshed_and_not_leaked():
    kind, n = "poisson", (40, 40, 40)
    with zzz.Context(0) as c:
        form = _generated(c, kind, n)
        it1, _, _ = c.cg_solve(pc=zzz.PC_MG)
        h1, u1 = c.cg_history(it1 + 1), c.vec_download(zzz.VEC_U)
        free1 = zzz.device_memory(0)[0]
        it2, _, _ = c.cg_solve(pc=zzz.PC_MG)
        assert it2 == it1 and np.array_equal(h1, c.cg_history(it2 + 1)) and np.array_equal(u1, c.vec_download(zzz.VEC_U))
        assert c.mg_info()["setups"] == 1
        # a second assembly: the values are refreshed, the levels stay
        c.assemble_matrix(form)
        it3, _, _ = c.cg_solve(pc=zzz.PC_MG)
        assert it3 == it1 and np.linalg.norm(c.vec_download(zzz.VEC_U) - u1) <= 1e-12 * np.linalg.norm(u1)
        assert c.mg_info()["setups"] == 2 and c.mg_info()["levels"] == len(level_dims(n, 1))
        for _ in range(8):
            c.cg_solve(pc=zzz.PC_MG)
        used1 = zzz.device_memory(0)[1] - free1
        used10 = zzz.device_memory(0)[1] - zzz.device_memory(0)[0]
        print(f"mg device memory in use after the first solve {used1}, after ten solves and a refresh {used10}")
        assert abs(used10 - used1) <= 0.01 * used1
        # Jacobi on the same context is what it was
        itj, _, _ = c.cg_solve(pc=zzz.PC_JACOBI)
        # a new feed: the hierarchy is rebuilt for it
        _generated(c, kind, (12, 10, 14))
        it4, _, _ = c.cg_solve(pc=zzz.PC_MG)
        assert c.mg_info(0)["cells"] == (12, 10, 14) and c.mg_info()["setups"] == 1 and it4 <= 12 and itj > 10 * it1


def test_level_options_and_a_problem_under_the_limit():
    kind, n = "poisson", (12, 10, 14)
    with zzz.Context(0) as c:
        _generated(c, kind, n)
        rp, cl, v = c.csr_download()
        b = c.vec_download(zzz.VEC_B)
        _, xt, _, _ = zo.pcg(rp.astype(np.int64), cl, v, b, rtol=1e-12)
        for kw in (dict(), dict(pc_mg_levels=2), dict(pc_mg_coarse_eq_limit=200), dict(pc_degree=3, pc_ratio=20.0)):
            it, _, _ = c.cg_solve(pc=zzz.PC_MG, **kw)
            dims = level_dims(n, 1, limit=kw.get("pc_mg_coarse_eq_limit", 0) or 1000, max_levels=kw.get("pc_mg_levels", 0))
            info = c.mg_info()
            assert info["levels"] == len(dims) and c.mg_info(len(dims) - 1)["cells"] == dims[-1], (kw, info, dims)
            assert c.mg_info(0)["degree"] == (kw.get("pc_degree") or 2)
            assert it <= 12 and c.cg_info()["reason"] == 2
            u = c.vec_download(zzz.VEC_U)
            assert np.linalg.norm(u - xt) <= 1e-6 * np.linalg.norm(xt)
        # two levels of a large cube would need a dense solve of thousands of dofs: declined, and said why
        _generated(c, kind, (45, 43, 41))
        with pytest.raises(zzz.ZzzError) as e:
            c.cg_solve(pc=zzz.PC_MG, pc_mg_levels=2)
        assert e.value.code == 1 and "dense" in str(e.value)
        assert c.cg_solve(pc=zzz.PC_MG)[0] <= 12
        # a fine problem under the limit: one level, the preconditioner is the dense solve
        _generated(c, kind, (4, 4, 4))
        it, _, _ = c.cg_solve(pc=zzz.PC_MG)
        assert c.mg_info()["levels"] == 1 and it <= 2 and c.cg_info()["reason"] == 2


def test_declined_combinations_leave_the_context_usable():
    zo.set_num_threads(4)

    def declined(c, **kw):
        with pytest.raises(zzz.ZzzError) as e:
            c.cg_solve(**dict(dict(pc=zzz.PC_MG), **kw))
        assert e.value.code == 1 and len(str(e.value)) > len("libzzz_hip error 1: "), str(e.value)
        return str(e.value)

    def jacobi_as_usual(c):
        rp, cl, v = c.csr_download()
        oit, ou, _, _ = zo.pcg(rp.astype(np.int64), cl, v, c.vec_download(zzz.VEC_B), rtol=1e-8)
        it, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
        assert abs(it - oit) <= 2 and np.linalg.norm(c.vec_download(zzz.VEC_U) - ou) <= 1e-6 * np.linalg.norm(ou)

    with zzz.Context(0) as c:
        _generated(c, "poisson", (12, 10, 14))
        assert "MATFREE" in declined(c, op=zzz.OP_MATFREE)
        assert "single_reduction" in declined(c, single_reduction=True)
        assert "pipecg" in declined(c, variant=zzz.CG_PIPE)
        declined(c, variant=zzz.CG_CGH)
        jacobi_as_usual(c)
        assert c.cg_solve(pc=zzz.PC_MG)[0] <= 12
    for order in (2, 3):
        with zzz.Context(0) as c:
            form = zzz.FORM_POISSON
            c.cube_generate("poisson", order, 4, 3, 5)
            c.pattern_build()
            c.assemble_matrix(form)
            c.assemble_vector(form)
            assert "P1 only" in declined(c)
            jacobi_as_usual(c)
    # an uploaded feed (the same cube built on the host) and an unstructured one
    for P in (zzz.Part("poisson", 1, 12, 10, 14), zzz.Part.spoke("poisson", 1, 3)):
        with zzz.Context(0) as c:
            c.upload_part(P)
            c.pattern_build()
            c.assemble_matrix(P.form)
            c.assemble_vector(P.form)
            assert "zzz_cube_generate" in declined(c)
            jacobi_as_usual(c)
    # a generated cube whose Dirichlet set was then uploaded is no longer the generated problem
    with zzz.Context(0) as c:
        _generated(c, "poisson", (6, 5, 4))
        c.upload_bc(np.array([0, 1], np.int32))
        declined(c)
    # a communicator attached (one rank, as tests/test_gpu_cg.py::test_rccl_path_single_rank attaches it)
    with zzz.Context(0) as c:
        c.comm_init(1, 0, zzz.comm_unique_id())
        _generated(c, "poisson", (12, 10, 14))
        assert "communicator" in declined(c)
        jacobi_as_usual(c)


@pytest.mark.parametrize("kind,n,cap", [("poisson", (216, 206, 222), 16), ("elasticity", (109, 109, 109), 24)])
def test_full_size(kind, n, cap):
    with zzz.Context(0) as c:
        _generated(c, kind, n)
        itj, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
        uj = c.vec_download(zzz.VEC_U)
        it, rn, r0 = c.cg_solve(pc=zzz.PC_MG, rtol=1e-8)
        u = c.vec_download(zzz.VEC_U)
        err = np.linalg.norm(u - uj) / np.linalg.norm(uj)
        info = c.mg_info()
        print(f"mg full size {kind} {n}: {info['levels']} levels, coarsest {info['coarse_dofs']} dofs, mg {it} iterations, "
              f"jacobi {itj}; |u-uj|/|uj| {err:.2e}")
        assert it <= cap and c.cg_info()["reason"] == 2
        assert err <= 1e-6
        assert info["levels"] == len(level_dims(n, 3 if kind == "elasticity" else 1))


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
        base = ["--problem_type", problem, "--scaling_type", "weak", "--ndofs", "50000", "-ksp_type", "cg", "-ksp_rtol", "1.0e-8"]
        itj, nj, _ = run(base + ["-pc_type", "jacobi"])
        itm, nm, out = run(base + ["-pc_type", "mg", "-ksp_view"])
        print(f"driver {problem}: jacobi {itj} iterations, mg {itm}; norms {nj} {nm}")
        assert abs(nm - nj) <= 1e-6 * nj and 10 * itm < itj
        assert "PC Object: type: mg" in out and "  level 0: cells " in out and "dense direct solve" in out and "ZZZ Solve" in out
        it2, n2, out2 = run(base + ["-pc_type", "mg", "-pc_mg_levels", "3", "-pc_mg_coarse_eq_limit", "4000", "-mg_levels_ksp_max_it", "3",
                                    "-mg_levels_ksp_chebyshev_ratio", "20", "-ksp_view"])
        assert abs(n2 - nj) <= 1e-6 * nj and "degree 3" in out2 and "  level 3" not in out2
    base = ["--problem_type", "poisson", "--ndofs", "50000", "-pc_type", "mg"]
    for bad in (["--order", "2"], ["--mesh_type", "unstructured"], ["--ngpus", "2", "--comm", "local"], ["--operator", "matfree"],
                ["-ksp_type", "pipecg"], ["-ksp_cg_single_reduction"]):
        run(base + bad, ok=False)
    run(["--problem_type", "cgpoisson", "--ndofs", "50000", "-pc_type", "mg"], ok=False)
    for other in ("gamg", "hypre"):
        o = subprocess.run([exe, "--ndofs", "50000", "-pc_type", other], capture_output=True, text=True, timeout=60)
        assert o.returncode != 0 and "-pc_type mg" in o.stderr
