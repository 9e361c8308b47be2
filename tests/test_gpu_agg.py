"""GPU parity tests of -pc_type agg (ZZZ_PC_AGG, csrc/zzz_agg.hip under csrc/zzz_mg.hip) through the C-ABI against its numpy /
scipy restatement (tests/_agg_ref.py, pinned on the CPU by tests/test_agg_ref.py).  The restatement is fed the matrix the
library holds (zzz_csr_download) and the library's own spectrum bounds; pc_mg_coarse_eq_limit is 50 so that every case has
at least three levels.

Bars (none comes from what the code under test gives):
  aggregates  exact: the prolongation of (1, 2, 3, ...) names every scalar dof's coarse dof.
  coarse CSR  indices exact, values within 1e-12 of the row's largest entry; two set-ups give the same bits.
  transfer    1e-14 of max |out| in both directions (P has one unit entry per row; P^T sums the members in the same
              ascending order as scipy's transposed CSR); the restriction bit-identical between two calls.
  V-cycle     8 x the restatement's own difference between its two summation orders on the same vector, and not below
              1e-12 of max |z|.
  solves      iterations within MEASURED_SPREAD + 2 of the restatement's and below Jacobi's, reason 2, the solution within
              1e-6 of the Jacobi solve's (taken at rtol 1e-10)."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import zzz
import _agg_ref as R

pytestmark = pytest.mark.gpu

LIMIT = R.LIMIT
AGG = dict(pc=zzz.PC_AGG, pc_mg_coarse_eq_limit=LIMIT)


def _feed(c, P):
    c.upload_part(P)
    c.pattern_build()
    c.assemble_matrix(P.form)
    c.assemble_vector(P.form)


def _matrix(c):
    rp, cl, v = c.csr_download()
    return sp.csr_matrix((v, cl, rp), shape=(rp.size - 1, rp.size - 1))


def _bounds(c):
    return [c.mg_info(l)["hi"] for l in range(c.mg_info()["levels"] - 1)]


def _restated(c, bc, bs, **kw):
    """the restatement of the hierarchy the context holds: its matrix, its bounds"""
    return R.AggHierarchy(_matrix(c), bc, bs, his=_bounds(c), limit=kw.pop("limit", LIMIT), **kw)


def _aggregate_map(c, l):
    """coarse scalar dof + 1 of every scalar dof of level l (0: none), read through the prolongation"""
    nc = c.mg_info(l + 1)["dofs"]
    return c.mg_transfer(l, 0, np.arange(1.0, nc + 1.0))


def _expected_map(H, l):
    return H.P[l] @ np.arange(1.0, H.P[l].shape[1] + 1.0)


def _level_csrs(c):
    return [c.mg_level_csr(l) for l in range(1, c.mg_info()["levels"])]


_cache = {}


def _case(name):
    """one context per case for the whole file: fed, set up, with its restatement"""
    if name not in _cache:
        P = R.case_part(name)
        c = zzz.Context(0)
        _feed(c, P)
        c.mg_setup(**AGG)
        _cache[name] = (c, P, _restated(c, P.bc_marker(), P.bs))
    return _cache[name]


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_aggregates_coarse_matrices_and_transfer(name):
    c, P, H = _case(name)
    rng = np.random.default_rng(3)
    info = c.mg_info()
    assert info["levels"] == len(H.A) >= 3 and info["products_per_cycle"] == 4
    for l, A in enumerate(H.A):
        li = c.mg_info(l)
        assert li["cells"] == (0, 0, 0) and li["dofs"] == A.shape[0] and li["nnz"] == A.nnz
        assert (li["degree"], li["lo"] > 0) == ((2, True) if l + 1 < len(H.A) else (0, False))
    first = _level_csrs(c)
    for l in range(len(H.A) - 1):
        assert np.array_equal(_aggregate_map(c, l), _expected_map(H, l)), f"aggregates of level {l}"
        rp, cl, v = first[l]
        Ac = H.A[l + 1]
        assert np.array_equal(rp, Ac.indptr) and np.array_equal(cl, Ac.indices)
        rowmax = np.maximum.reduceat(np.abs(Ac.data), Ac.indptr[:-1])
        dv = (np.abs(v - Ac.data) / np.repeat(rowmax, np.diff(Ac.indptr))).max()
        print(f"agg {name} level {l + 1}: {Ac.shape[0]} dofs, {Ac.nnz} nonzeros, values differ by {dv:.2e} of the row's largest")
        assert dv <= 1e-12
        # the transfer, both directions
        Pm = H.P[l]
        e, r = rng.standard_normal(Pm.shape[1]), rng.standard_normal(Pm.shape[0])
        pe, ptr = c.mg_transfer(l, 0, e), c.mg_transfer(l, 1, r)
        d0 = np.abs(pe - Pm @ e).max() / np.abs(pe).max()
        d1 = np.abs(ptr - Pm.T @ r).max() / np.abs(ptr).max()
        print(f"agg {name} level {l}: prolongation {d0:.2e}, restriction {d1:.2e}")
        assert d0 <= 1e-14 and d1 <= 1e-14
        assert np.array_equal(ptr, c.mg_transfer(l, 1, r))
    # a second set-up from scratch (another level limit, then this one again): the same bits
    c.mg_setup(pc=zzz.PC_AGG, pc_mg_coarse_eq_limit=LIMIT, pc_mg_levels=2)
    assert c.mg_info()["levels"] == 2 and c.mg_info()["setups"] == 1
    c.mg_setup(**AGG)
    assert c.mg_info()["setups"] == 1
    for (rp, cl, v), (rp2, cl2, v2) in zip(first, _level_csrs(c)):
        assert np.array_equal(rp, rp2) and np.array_equal(cl, cl2) and np.array_equal(v, v2)


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_cycle_against_the_restatement(name):
    c, P, H = _case(name)
    c.mg_setup(**AGG)
    rng = np.random.default_rng(11)
    n = H.A[0].shape[0]
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    Ma, Mb = c.mg_apply(a), c.mg_apply(b)
    ref = H.vcycle(a)
    own = np.abs(H.vcycle_reversed(a) - ref).max()
    bar = max(8.0 * own, 1e-12 * np.abs(ref).max())
    dv = np.abs(Ma - ref).max()
    print(f"agg V-cycle {name}: |gpu - restatement| {dv:.2e}, the restatement's two orders {own:.2e}, bar {bar:.2e}, "
          f"max |z| {np.abs(ref).max():.2e}")
    assert dv <= bar
    sym = abs(Ma @ b - a @ Mb) / (np.linalg.norm(Ma) * np.linalg.norm(b))
    assert sym <= 1e-12 and Ma @ a > 0.0 and Mb @ b > 0.0
    assert np.array_equal(Ma, c.mg_apply(a))


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_solves_with_every_norm_type(name):
    c, P, H = _case(name)
    b = c.vec_download(zzz.VEC_B)
    c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-10)
    uj = c.vec_download(zzz.VEC_U)
    itj, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
    for norm in (zzz.NORM_PRECONDITIONED, zzz.NORM_UNPRECONDITIONED, zzz.NORM_NATURAL):
        it, rn, r0 = c.cg_solve(norm=norm, rtol=1e-8, **AGG)
        u = c.vec_download(zzz.VEC_U)
        ito, _ = R.pcg(H.A[0], b, H.vcycle, norm_type=norm, rtol=1e-8)
        err = np.linalg.norm(u - uj) / np.linalg.norm(uj)
        print(f"agg solve {name} norm {norm}: gpu {it}, restatement {ito}, jacobi {itj}; |u-uj|/|uj| {err:.2e}")
        assert abs(it - ito) <= R.IT_BAR
        assert it < itj
        assert c.cg_info()["reason"] == 2 and rn <= 1e-8 * r0
        assert err <= 1e-6
        assert c.cg_history(it + 1)[0] == r0


@pytest.mark.parametrize("problem,shape", [("poisson", (12, 10, 14)), ("elasticity", (6, 6, 6))])
def test_a_feed_in_another_numbering(problem, shape):
    """the cube as a caller with a random numbering feeds it: the library keeps an internal dof order, the rule speaks of the
    caller's -- aggregates, coarse matrices, cycle and counts must be the restatement's in the caller's numbering"""
    P = zzz.Part(problem, 1, *shape).renumbered("random", seed=3)
    with zzz.Context(0) as c:
        _feed(c, P)
        perm, kind = c.internal_order()
        assert kind == 1 and not np.array_equal(perm, np.arange(perm.size))
        c.mg_setup(**AGG)
        H = _restated(c, P.bc_marker(), P.bs)
        assert c.mg_info()["levels"] == len(H.A) >= 3
        for l in range(len(H.A) - 1):
            assert np.array_equal(_aggregate_map(c, l), _expected_map(H, l)), f"aggregates of level {l}"
            rp, cl, v = c.mg_level_csr(l + 1)
            Ac = H.A[l + 1]
            assert np.array_equal(rp, Ac.indptr) and np.array_equal(cl, Ac.indices)
            rowmax = np.maximum.reduceat(np.abs(Ac.data), Ac.indptr[:-1])
            assert (np.abs(v - Ac.data) / np.repeat(rowmax, np.diff(Ac.indptr))).max() <= 1e-12
            r = np.random.default_rng(l).standard_normal(H.P[l].shape[0])
            ptr = c.mg_transfer(l, 1, r)
            assert np.abs(ptr - H.P[l].T @ r).max() <= 1e-14 * np.abs(ptr).max()
        a = np.random.default_rng(11).standard_normal(H.A[0].shape[0])
        ref = H.vcycle(a)
        bar = max(8.0 * np.abs(H.vcycle_reversed(a) - ref).max(), 1e-12 * np.abs(ref).max())
        assert np.abs(c.mg_apply(a) - ref).max() <= bar
        b = c.vec_download(zzz.VEC_B)
        itj = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)[0]
        it = c.cg_solve(rtol=1e-8, **AGG)[0]
        ito, _ = R.pcg(H.A[0], b, H.vcycle, rtol=1e-8)
        print(f"agg renumbered {problem}: gpu {it}, restatement {ito}, jacobi {itj}")
        assert abs(it - ito) <= R.IT_BAR and it < itj and c.cg_info()["reason"] == 2


def _declined(c, **kw):
    with pytest.raises(zzz.ZzzError) as e:
        c.cg_solve(**kw)
    assert e.value.code == 1 and len(str(e.value)) > len("libzzz_hip error 1: "), str(e.value)
    return str(e.value)


def _scaled(A, seed):
    """D A D with a random positive diagonal: symmetric positive definite on the same pattern"""
    d = np.random.default_rng(seed).uniform(0.5, 2.0, A.shape[0])
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    # (entry by entry, so that the values keep the order of the context's pattern)
    return sp.csr_matrix((d[rows] * A.data * d[A.indices], A.indices, A.indptr), shape=A.shape), d


def test_accepted_feeds_that_mg_declines():
    feeds = []
    c = zzz.Context(0)
    _feed(c, zzz.Part("poisson", 1, 12, 10, 14))  # the cube built on the host and uploaded
    feeds.append(c)
    c = zzz.Context(0)
    _feed(c, zzz.Part.spoke("poisson", 1, 3))
    feeds.append(c)
    c = zzz.Context(0)  # a generated cube whose Dirichlet set was uploaded afterwards
    c.cube_generate("poisson", 1, 6, 5, 4)
    c.upload_bc(zzz.Part("poisson", 1, 6, 5, 4).bc_dofs)
    c.pattern_build()
    c.assemble_matrix(zzz.FORM_POISSON)
    c.assemble_vector(zzz.FORM_POISSON)
    feeds.append(c)
    for c in feeds:
        with c:
            assert "zzz_cube_generate" in _declined(c, pc=zzz.PC_MG)
            c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-10)
            uj = c.vec_download(zzz.VEC_U)
            itj = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)[0]
            it = c.cg_solve(rtol=1e-8, **AGG)[0]
            u = c.vec_download(zzz.VEC_U)
            assert c.cg_info()["reason"] == 2 and it < itj
            assert np.linalg.norm(u - uj) <= 1e-6 * np.linalg.norm(uj)


def test_uploaded_values_refresh_and_a_new_pattern_rebuilds():
    P = R.case_part("poisson_p1")
    with zzz.Context(0) as c:
        _feed(c, P)
        bc = P.bc_marker()
        c.mg_setup(**AGG)
        H1 = _restated(c, bc, P.bs)
        maps = [_aggregate_map(c, l) for l in range(len(H1.A) - 1)]
        before = _level_csrs(c)
        # new values on the same pattern: D A D
        A2, d = _scaled(_matrix(c), 7)
        c.csr_upload_values(A2.data)
        b = c.vec_download(zzz.VEC_B)
        c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-10)
        uj = c.vec_download(zzz.VEC_U)
        itj = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)[0]
        it = c.cg_solve(rtol=1e-8, **AGG)[0]
        u = c.vec_download(zzz.VEC_U)
        assert c.mg_info()["setups"] == 2 and c.cg_info()["reason"] == 2 and it < itj
        assert np.linalg.norm(u - uj) <= 1e-6 * np.linalg.norm(uj)
        # the same aggregates, the new coarse values (the scaling changes no zero: a fresh restatement has the same aggregates)
        H2 = _restated(c, bc, P.bs)
        assert len(H2.A) == len(H1.A)
        for l in range(len(H2.A) - 1):
            assert np.array_equal(_aggregate_map(c, l), maps[l]) and np.array_equal(maps[l], _expected_map(H2, l))
            rp, cl, v = c.mg_level_csr(l + 1)
            Ac = H2.A[l + 1]
            assert np.array_equal(rp, before[l][0]) and np.array_equal(cl, before[l][1]) and not np.array_equal(v, before[l][2])
            rowmax = np.maximum.reduceat(np.abs(Ac.data), Ac.indptr[:-1])
            assert (np.abs(v - Ac.data) / np.repeat(rowmax, np.diff(Ac.indptr))).max() <= 1e-12
        ito, _ = R.pcg(H2.A[0], b, H2.vcycle, rtol=1e-8)
        assert abs(it - ito) <= R.IT_BAR
        # a new pattern: rebuilt for it
        Q = zzz.Part("poisson", 1, 9, 8, 7)
        _feed(c, Q)
        it = c.cg_solve(rtol=1e-8, **AGG)[0]
        H3 = _restated(c, Q.bc_marker(), Q.bs)
        assert c.mg_info()["setups"] == 1 and c.mg_info()["levels"] == len(H3.A) and c.mg_info(0)["dofs"] == Q.n_owned
        assert np.array_equal(_aggregate_map(c, 0), _expected_map(H3, 0))
        assert c.cg_info()["reason"] == 2


def test_alternating_with_mg_leaves_device_memory_where_it_was():
    with zzz.Context(0) as c:
        c.cube_generate("poisson", 1, 40, 40, 40)
        c.pattern_build()
        c.assemble_matrix(zzz.FORM_POISSON)
        c.assemble_vector(zzz.FORM_POISSON)
        free0 = zzz.device_memory(0)[0]
        itm = c.cg_solve(pc=zzz.PC_MG)[0]
        ita = c.cg_solve(pc=zzz.PC_AGG)[0]
        assert c.mg_info(0)["cells"] == (0, 0, 0)
        used1 = zzz.device_memory(0)[1] - zzz.device_memory(0)[0]
        for _ in range(3):
            assert c.cg_solve(pc=zzz.PC_MG)[0] == itm and c.mg_info(0)["cells"] == (40, 40, 40) and c.mg_info()["setups"] == 1
            assert c.cg_solve(pc=zzz.PC_AGG)[0] == ita and c.mg_info(0)["cells"] == (0, 0, 0) and c.mg_info()["setups"] == 1
        used4 = zzz.device_memory(0)[1] - zzz.device_memory(0)[0]
        print(f"agg device memory in use after the first mg / agg pair {used1}, after four pairs {used4} (free before: {free0})")
        assert abs(used4 - used1) <= 0.01 * used1
        itj = c.cg_solve(pc=zzz.PC_JACOBI)[0]
        assert ita < itj and c.cg_info()["reason"] == 2
        # two levels of this cube would end above the dense limit: declined, and said why
        assert "dense" in _declined(c, pc=zzz.PC_AGG, pc_mg_levels=2)
        assert c.cg_solve(pc=zzz.PC_AGG)[0] == ita


def test_declined_combinations_leave_the_context_usable():
    P = R.case_part("poisson_p1")
    with zzz.Context(0) as c:
        _feed(c, P)
        itj = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)[0]
        uj = c.vec_download(zzz.VEC_U)
        assert "MATFREE" in _declined(c, op=zzz.OP_MATFREE, **AGG)
        assert "single_reduction" in _declined(c, single_reduction=True, **AGG)
        assert "pipecg" in _declined(c, variant=zzz.CG_PIPE, **AGG)
        _declined(c, variant=zzz.CG_CGH, **AGG)
        assert c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)[0] == itj and np.array_equal(c.vec_download(zzz.VEC_U), uj)
        assert c.cg_solve(rtol=1e-8, **AGG)[0] < itj
    with zzz.Context(0) as c:
        c.comm_init(1, 0, zzz.comm_unique_id())
        _feed(c, P)
        assert "communicator" in _declined(c, **AGG)
        assert c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)[0] == itj


def test_all_constrained_and_an_isolated_node():
    with zzz.Context(0) as c:
        c.cube_generate("poisson", 1, 4, 4, 4)
        c.upload_bc(np.arange(125, dtype=np.int32))
        c.pattern_build()
        c.assemble_matrix(zzz.FORM_POISSON)
        c.assemble_vector(zzz.FORM_POISSON)
        it = c.cg_solve(rtol=1e-8, **AGG)[0]
        assert c.mg_info()["levels"] == 1 and it <= 1 and c.cg_info()["reason"] in (2, 3)
    P = R.case_part("poisson_p1")
    with zzz.Context(0) as c:
        _feed(c, P)
        A = _matrix(c)
        bc = P.bc_marker()
        node = int(np.flatnonzero(bc == 0)[300])
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        off = (rows == node) ^ (A.indices == node)  # its row and its column without the diagonal
        assert off.sum() >= 6
        A.data[off] = 0.0  # (explicit zeros: the pattern stays the context's)
        c.csr_upload_values(A.data)
        c.mg_setup(**AGG)
        H = _restated(c, bc, 1)
        m = _aggregate_map(c, 0)
        assert np.array_equal(m, _expected_map(H, 0))
        assert m[node] > 0 and np.sum(m == m[node]) == 1
        assert c.cg_solve(rtol=1e-8, **AGG)[0] < c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)[0]


def test_driver():
    exe = os.path.join(zzz.PKG, "dolfinx-scaling-test")

    def run(args):
        return subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)

    base = ["--scaling_type", "weak", "--ndofs", "20000", "-ksp_type", "cg", "-ksp_rtol", "1.0e-8", "-ksp_view"]
    for extra in (["--problem_type", "poisson", "--mesh_type", "unstructured"], ["--problem_type", "elasticity", "--order", "2"]):
        oj = run(base + extra + ["-pc_type", "jacobi"])
        oa = run(base + extra + ["-pc_type", "agg"])
        assert oj.returncode == 0 and oa.returncode == 0, (extra, oa.stderr[-1000:])
        its = [int(o.stdout.split("*** Number of Krylov iterations: ")[1].split()[0]) for o in (oj, oa)]
        norms = [float(o.stdout.split("*** Solution norm:  ")[1].split()[0]) for o in (oj, oa)]
        print(f"driver {extra}: jacobi {its[0]} iterations, agg {its[1]}; norms {norms}")
        assert its[1] < its[0] and abs(norms[1] - norms[0]) <= 1e-6 * norms[0]
        assert "PC Object: type: agg" in oa.stdout and "  level 0: the assembled matrix, dofs " in oa.stdout
        assert "  level 1: aggregates of the level above, dofs " in oa.stdout and "dense direct solve" in oa.stdout
    for bad in (["--ngpus", "2", "--comm", "local"], ["--operator", "matfree"], ["-ksp_type", "pipecg"], ["-ksp_cg_single_reduction"]):
        assert run(["--ndofs", "20000", "-pc_type", "agg"] + bad).returncode != 0
    o = run(["--ndofs", "20000", "-pc_type", "gamg"])
    assert o.returncode != 0 and "-pc_type mg" in o.stderr
