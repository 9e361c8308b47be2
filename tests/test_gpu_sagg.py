"""GPU parity tests of -pc_type sagg (ZZZ_PC_SAGG, csrc/zzz_sagg.hip under csrc/zzz_mg.hip) through the C-ABI against its numpy /
scipy restatement (tests/_sagg_ref.py, pinned on the CPU by tests/test_sagg_ref.py).  The restatement is fed the matrix the
library holds (zzz_csr_download) and the library's own spectrum bounds (omega is their function); pc_mg_coarse_eq_limit is 50 so
that every case has at least three levels, coarse levels of block size 3 without Dirichlet rows, singleton aggregates and rows of
P from 0 to 21 entries.

Bars (none comes from what the code under test gives):
  hierarchy   level sizes and aggregate counts equal; the indices of P (zzz_mg_level_p) and of every coarse matrix
              (zzz_mg_level_csr) exact; each value within 8 x the largest difference in its row between the restatement's sums
              front to back and back to front, and not below 1e-12 of the row's largest entry; two set-ups on fresh contexts give
              the same bits.
  transfer    8 x the difference between scipy's product in the level's numbering and in the reversed one, and not below 1e-14
              of max |out|, in both directions; two calls give the same bits.
  V-cycle     8 x the restatement's own difference between its two summation orders on the same vector, and not below 1e-12 of
              max |z| (tests/test_gpu_agg.py's bar); symmetry 1e-12; positive.
  solves      iterations within MEASURED_SPREAD + 2 of the restatement's, reason 2, the solution within 1e-6 of the Jacobi
              solve's (taken at rtol 1e-10); on poisson_p1 fewer iterations than ZZZ_PC_AGG on the same context."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import zzz
import _agg_ref as AR
import _sagg_ref as R
from _hostile_gpu import _env

pytestmark = pytest.mark.gpu

LIMIT = R.LIMIT
SAGG = dict(pc=zzz.PC_SAGG, pc_mg_coarse_eq_limit=LIMIT)
AGG = dict(pc=zzz.PC_AGG, pc_mg_coarse_eq_limit=LIMIT)
NORMS = (zzz.NORM_PRECONDITIONED, zzz.NORM_UNPRECONDITIONED, zzz.NORM_NATURAL)


def _feed(c, P, bc_dofs=None):
    c.upload_part(P)
    if bc_dofs is not None:
        c.upload_bc(bc_dofs)
    c.pattern_build()
    c.assemble_matrix(P.form)
    c.assemble_vector(P.form)


def _matrix(c):
    rp, cl, v = c.csr_download()
    return sp.csr_matrix((v, cl, rp), shape=(rp.size - 1, rp.size - 1))


def _bounds(c):
    return [c.mg_info(l)["hi"] for l in range(c.mg_info()["levels"] - 1)]


def _restated(c, bc, bs):
    """the restatement of the hierarchy the context holds: its matrix, its bounds"""
    return R.SaggHierarchy(_matrix(c), bc, bs, his=_bounds(c), limit=LIMIT)


def _stored(c):
    """[(P of level l, A of level l + 1)] as the library holds them"""
    return [(c.mg_level_p(l), c.mg_level_csr(l + 1)) for l in range(c.mg_info()["levels"] - 1)]


def _same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for pa, pb in zip(a, b) for ma, mb in zip(pa, pb) for x, y in zip(ma, mb))


def _check_hierarchy(c, H, tag):
    """item 1 of the module's bars, per level; returns what the library stores"""
    D = H.descending()
    info = c.mg_info()
    assert info["levels"] == len(H.A) and info["products_per_cycle"] == (4 if len(H.A) > 1 else 0)
    for l, A in enumerate(H.A):
        li = c.mg_info(l)
        assert li["cells"] == (0, 0, 0) and li["dofs"] == A.shape[0] and li["nnz"] == A.nnz, (tag, l, li, A.shape, A.nnz)
    stored = _stored(c)
    for l, ((prp, pcl, pv), (rp, cl, v)) in enumerate(stored):
        Pm, Ac = H.P[l], H.A[l + 1]
        assert np.array_equal(prp, Pm.indptr) and np.array_equal(pcl, Pm.indices), f"{tag}: pattern of P, level {l}"
        assert np.array_equal(rp, Ac.indptr) and np.array_equal(cl, Ac.indices), f"{tag}: pattern of A, level {l + 1}"
        bp, ba = R.row_bars(Pm, D.P[l]), R.row_bars(Ac, D.A[l + 1])
        dp, da = np.abs(pv - Pm.data), np.abs(v - Ac.data)
        print(f"sagg {tag} level {l}: P {Pm.shape[0]} x {Pm.shape[1]}, {Pm.nnz} entries, rows up to {int(np.diff(Pm.indptr).max())}, "
              f"worst |gpu - restatement| / bar {np.max(dp / bp):.2e}; A_c {Ac.nnz} nonzeros, worst {np.max(da / ba):.2e}")
        assert np.all(dp <= bp), f"{tag}: values of P, level {l}"
        assert np.all(da <= ba), f"{tag}: values of A, level {l + 1}"
    return stored


_cache = {}


def _case(name):
    """one context per case for the whole file: fed, set up, with its restatement"""
    if name not in _cache:
        P = R.case_part(name)
        c = zzz.Context(0)
        _feed(c, P)
        c.mg_setup(**SAGG)
        _cache[name] = (c, P, _restated(c, P.bc_marker(), P.bs))
    return _cache[name]


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_hierarchy_against_the_restatement(name):
    c, P, H = _case(name)
    c.mg_setup(**SAGG)
    assert len(H.A) >= 3
    first = _check_hierarchy(c, H, name)
    assert np.array_equal(H.agg[0], AR.aggregate(H.A[0], H.bc[0], H.bs)[0])
    assert min(int(np.diff(p.indptr).min()) for p in H.P) == 0
    with zzz.Context(0) as c2:
        _feed(c2, P)
        c2.mg_setup(**SAGG)
        assert _same_bits(first, _stored(c2)), "two set-ups on fresh contexts differ"


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_transfers(name):
    c, P, H = _case(name)
    c.mg_setup(**SAGG)
    rng = np.random.default_rng(3)
    for l, Pm in enumerate(H.P):
        e, r = rng.standard_normal(Pm.shape[1]), rng.standard_normal(Pm.shape[0])
        Prev = sp.csr_matrix(Pm[::-1, ::-1])
        Prev.sort_indices()
        for d, M, Mrev, x in ((0, Pm, Prev, e), (1, sp.csr_matrix(Pm.T), sp.csr_matrix(Prev.T), r)):
            ref = M @ x
            own = np.abs((Mrev @ x[::-1])[::-1] - ref).max()
            bar = max(8.0 * own, 1e-14 * np.abs(ref).max())
            out = c.mg_transfer(l, d, x)
            dv = np.abs(out - ref).max()
            print(f"sagg {name} level {l} direction {d}: |gpu - P e| {dv:.2e}, scipy's two orders {own:.2e}, bar {bar:.2e}")
            assert dv <= bar
            assert np.array_equal(out, c.mg_transfer(l, d, x))


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_cycle_against_the_restatement(name):
    c, P, H = _case(name)
    c.mg_setup(**SAGG)
    rng = np.random.default_rng(11)
    n = H.A[0].shape[0]
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    Ma, Mb = c.mg_apply(a), c.mg_apply(b)
    ref = H.vcycle(a)
    own = np.abs(H.vcycle_reversed(a) - ref).max()
    bar = max(8.0 * own, 1e-12 * np.abs(ref).max())
    dv = np.abs(Ma - ref).max()
    print(f"sagg V-cycle {name}: |gpu - restatement| {dv:.2e}, the restatement's two orders {own:.2e}, bar {bar:.2e}, "
          f"max |z| {np.abs(ref).max():.2e}")
    assert dv <= bar
    sym = abs(Ma @ b - a @ Mb) / (np.linalg.norm(Ma) * np.linalg.norm(b))
    assert sym <= 1e-12 and Ma @ a > 0.0 and Mb @ b > 0.0
    assert np.array_equal(Ma, c.mg_apply(a))


def _check_solves(c, H, tag):
    b = c.vec_download(zzz.VEC_B)
    c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-10)
    uj = c.vec_download(zzz.VEC_U)
    its = []
    for norm in NORMS:
        it, rn, r0 = c.cg_solve(norm=norm, rtol=1e-8, **SAGG)
        u = c.vec_download(zzz.VEC_U)
        ito, _ = R.pcg(H.A[0], b, H.vcycle, norm_type=norm, rtol=1e-8)
        err = np.linalg.norm(u - uj) / np.linalg.norm(uj)
        print(f"sagg solve {tag} norm {norm}: gpu {it}, restatement {ito}; |u-uj|/|uj| {err:.2e}")
        assert abs(it - ito) <= R.IT_BAR
        assert c.cg_info()["reason"] == 2 and rn <= 1e-8 * r0
        assert err <= 1e-6
        its.append(it)
    return its


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_solves_with_every_norm_type(name):
    c, P, H = _case(name)
    its = _check_solves(c, H, name)
    if name == "poisson_p1":
        ita = [c.cg_solve(norm=norm, rtol=1e-8, **AGG)[0] for norm in NORMS]
        print(f"sagg solve {name}: sagg {its}, agg {ita} on the same context")
        assert all(s < a for s, a in zip(its, ita))
        assert c.cg_solve(rtol=1e-8, **SAGG)[0] == its[0]


@pytest.mark.parametrize("renumber", [None, "0"], ids=["internal-order", "callers-order-kept"])
@pytest.mark.parametrize("problem,shape", [("poisson", (12, 10, 14)), ("elasticity", (6, 6, 6))])
def test_a_feed_in_another_numbering(problem, shape, renumber):
    """the cube as a caller with a random numbering feeds it: with the library's internal dof order and without, the rule
    speaks of the caller's -- P, the coarse matrices and the counts must be the restatement's in the caller's numbering"""
    P = zzz.Part(problem, 1, *shape).renumbered("random", seed=3)
    with _env(ZZZ_RENUMBER=renumber), zzz.Context(0) as c:
        _feed(c, P)
        perm, kind = c.internal_order()
        assert (kind == 1 and not np.array_equal(perm, np.arange(perm.size))) if renumber is None else kind == 0
        c.mg_setup(**SAGG)
        H = _restated(c, P.bc_marker(), P.bs)
        assert len(H.A) >= 3
        _check_hierarchy(c, H, f"{problem} renumber={renumber}")
        for l, Pm in enumerate(H.P):
            r = np.random.default_rng(l).standard_normal(Pm.shape[0])
            ref = Pm.T @ r
            assert np.abs(c.mg_transfer(l, 1, r) - ref).max() <= 1e-12 * np.abs(ref).max()
        _check_solves(c, H, f"{problem} renumber={renumber}")


def test_partly_constrained_nodes():
    """an uploaded elasticity feed whose Dirichlet set holds ONE component of three interior nodes: those rows of P are empty,
    the other two components of the node keep theirs, and the rest is the restatement's"""
    P = R.case_part("elasticity_p1")
    free = np.flatnonzero((P.bc_marker().reshape(-1, 3) == 0).all(axis=1))
    nodes = free[[20, free.size // 2, free.size - 21]]
    extra = nodes * 3 + np.array([1, 0, 2])
    bc = P.bc_marker().copy()
    bc[extra] = 1
    with zzz.Context(0) as c:
        _feed(c, P, np.flatnonzero(bc).astype(np.int32))
        c.mg_setup(**SAGG)
        H = _restated(c, bc, 3)
        assert len(H.A) >= 3
        stored = _check_hierarchy(c, H, "partly constrained")
        prp = stored[0][0][0]
        rows = np.diff(prp)
        assert np.all(rows[extra] == 0) and np.all(rows[bc == 0] > 0)
        for n, d in zip(nodes, extra):
            assert sorted(rows[3 * n:3 * n + 3] > 0) == [False, True, True]
        _check_solves(c, H, "partly constrained")


def _scaled(A, seed):
    """D A D with a random positive diagonal: symmetric positive definite on the same pattern"""
    d = np.random.default_rng(seed).uniform(0.5, 2.0, A.shape[0])
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return sp.csr_matrix((d[rows] * A.data * d[A.indices], A.indices, A.indptr), shape=A.shape)


@pytest.mark.parametrize("name", ["poisson_p1", "elasticity_p1"])
def test_uploaded_values_refresh_to_the_bits_of_a_fresh_context_and_a_new_pattern_rebuilds(name):
    P = R.case_part(name)
    with zzz.Context(0) as c, zzz.Context(0) as c2:
        _feed(c, P)
        c.mg_setup(**SAGG)
        before = _stored(c)
        assert c.mg_info()["setups"] == 1
        A2 = _scaled(_matrix(c), 7)
        c.csr_upload_values(A2.data)
        c.mg_setup(**SAGG)
        assert c.mg_info()["setups"] == 2, "a refresh, not a rebuild"
        after = _stored(c)
        H2 = _restated(c, P.bc_marker(), P.bs)
        _check_hierarchy(c, H2, f"{name} refreshed")
        for (p0, a0), (p1, a1) in zip(before, after):
            assert np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1], p1[1]) and not np.array_equal(p0[2], p1[2])
            assert np.array_equal(a0[0], a1[0]) and np.array_equal(a0[1], a1[1]) and not np.array_equal(a0[2], a1[2])
        _feed(c2, P)
        c2.csr_upload_values(A2.data)
        c2.mg_setup(**SAGG)
        assert c2.mg_info()["setups"] == 1 and _bounds(c2) == _bounds(c)
        assert _same_bits(after, _stored(c2)), "a refresh differs from a fresh set-up with the same values"
        _check_solves(c, H2, f"{name} refreshed")
        # another estimate changes the bounds, omega with them, and so P: a refresh as well
        c.mg_setup(pc_esteig_its=4, **SAGG)
        assert c.mg_info()["setups"] == 3
        _check_hierarchy(c, R.SaggHierarchy(A2, P.bc_marker(), P.bs, his=_bounds(c), limit=LIMIT), f"{name} esteig 4")
        # a new pattern: rebuilt for it
        Q = zzz.Part("poisson" if P.bs == 1 else "elasticity", 1, 9, 8, 7)
        _feed(c, Q)
        it = c.cg_solve(rtol=1e-8, **SAGG)[0]
        H3 = _restated(c, Q.bc_marker(), Q.bs)
        assert c.mg_info()["setups"] == 1 and c.mg_info(0)["dofs"] == Q.n_owned * Q.bs
        _check_hierarchy(c, H3, f"{name} new pattern")
        assert c.cg_info()["reason"] == 2 and abs(it - R.pcg(H3.A[0], c.vec_download(zzz.VEC_B), H3.vcycle, rtol=1e-8)[0]) <= R.IT_BAR


def test_alternating_with_agg_and_mg_leaves_device_memory_where_it_was():
    with zzz.Context(0) as c:
        c.cube_generate("poisson", 1, 40, 40, 40)
        c.pattern_build()
        c.assemble_matrix(zzz.FORM_POISSON)
        c.assemble_vector(zzz.FORM_POISSON)
        free0 = zzz.device_memory(0)[0]
        itm = c.cg_solve(pc=zzz.PC_MG)[0]
        ita = c.cg_solve(pc=zzz.PC_AGG)[0]
        its = c.cg_solve(pc=zzz.PC_SAGG)[0]
        assert c.mg_info(0)["cells"] == (0, 0, 0) and c.mg_level_p(0)[1].size > 0
        used1 = zzz.device_memory(0)[1] - zzz.device_memory(0)[0]
        for _ in range(3):
            assert c.cg_solve(pc=zzz.PC_MG)[0] == itm and c.mg_info(0)["cells"] == (40, 40, 40) and c.mg_info()["setups"] == 1
            assert c.cg_solve(pc=zzz.PC_AGG)[0] == ita and c.mg_info(0)["cells"] == (0, 0, 0) and c.mg_info()["setups"] == 1
            assert c.cg_solve(pc=zzz.PC_SAGG)[0] == its and c.mg_info(0)["cells"] == (0, 0, 0) and c.mg_info()["setups"] == 1
        used4 = zzz.device_memory(0)[1] - zzz.device_memory(0)[0]
        print(f"sagg device memory in use after the first mg / agg / sagg round {used1}, after four {used4} (free before: {free0}); "
              f"iterations mg {itm}, agg {ita}, sagg {its}")
        assert abs(used4 - used1) <= 0.01 * used1
        itj = c.cg_solve(pc=zzz.PC_JACOBI)[0]
        assert its < ita < itj and c.cg_info()["reason"] == 2
        assert "dense" in _declined(c, pc=zzz.PC_SAGG, pc_mg_levels=2)
        assert c.cg_solve(pc=zzz.PC_SAGG)[0] == its


def _declined(c, code=1, **kw):
    with pytest.raises(zzz.ZzzError) as e:
        c.cg_solve(**kw)
    assert e.value.code == code and len(str(e.value)) > len("libzzz_hip error 1: "), str(e.value)
    return str(e.value)


def test_declined_combinations_leave_the_context_usable():
    P = R.case_part("poisson_p1")
    with zzz.Context(0) as c:
        _feed(c, P)
        itj = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)[0]
        uj = c.vec_download(zzz.VEC_U)
        assert "MATFREE" in _declined(c, op=zzz.OP_MATFREE, **SAGG)
        assert "single_reduction" in _declined(c, single_reduction=True, **SAGG)
        assert "pipecg" in _declined(c, variant=zzz.CG_PIPE, **SAGG)
        _declined(c, variant=zzz.CG_CGH, **SAGG)
        assert c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)[0] == itj and np.array_equal(c.vec_download(zzz.VEC_U), uj)
        # the stored prolongator belongs to this kind of hierarchy alone
        for other in (zzz.PC_AGG, zzz.PC_MG):
            if other == zzz.PC_MG:
                c.cube_generate("poisson", 1, 12, 10, 14)
                c.pattern_build()
                c.assemble_matrix(zzz.FORM_POISSON)
                c.assemble_vector(zzz.FORM_POISSON)
            c.mg_setup(pc=other, pc_mg_coarse_eq_limit=LIMIT)
            with pytest.raises(zzz.ZzzError) as e:
                c.mg_level_p(0)
            assert e.value.code == 1 and "ZZZ_PC_SAGG" in str(e.value)
        _feed(c, P)
        # more terms on a level than the positions take: ZZZ_ERR_LIMIT with the level and the count (the limit lowered to a size
        # these cases reach), the context usable, and the set-up served again without the knob
        with _env(ZZZ_SAGG_MAX_TERMS="1000"):
            msg = _declined(c, code=5, rtol=1e-8, **SAGG)
        assert "level 0" in msg and "terms of A P" in msg and "1000" in msg
        assert c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)[0] == itj and np.array_equal(c.vec_download(zzz.VEC_U), uj)
        assert c.cg_solve(rtol=1e-8, **SAGG)[0] < itj
    with zzz.Context(0) as c:
        c.comm_init(1, 0, zzz.comm_unique_id())
        _feed(c, P)
        assert "communicator" in _declined(c, **SAGG)
        assert c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)[0] == itj


def test_driver():
    exe = os.path.join(zzz.PKG, "dolfinx-scaling-test")

    def run(args):
        return subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)

    base = ["--scaling_type", "weak", "--ndofs", "20000", "-ksp_type", "cg", "-ksp_rtol", "1.0e-8", "-ksp_view"]
    for extra in (["--problem_type", "poisson"], ["--problem_type", "elasticity"]):
        oj = run(base + extra + ["-pc_type", "jacobi"])
        os_ = run(base + extra + ["-pc_type", "sagg"])
        assert oj.returncode == 0 and os_.returncode == 0, (extra, os_.stderr[-1000:])
        its = [int(o.stdout.split("*** Number of Krylov iterations: ")[1].split()[0]) for o in (oj, os_)]
        norms = [float(o.stdout.split("*** Solution norm:  ")[1].split()[0]) for o in (oj, os_)]
        print(f"driver {extra}: jacobi {its[0]} iterations, sagg {its[1]}; norms {norms}")
        assert its[1] < its[0] and abs(norms[1] - norms[0]) <= 1e-6 * norms[0]
        assert "PC Object: type: sagg" in os_.stdout and "  level 0: the assembled matrix, dofs " in os_.stdout
        assert "  level 1: aggregates of the level above, dofs " in os_.stdout and "dense direct solve" in os_.stdout
        assert ", prolongator entries " in os_.stdout and ", omega " in os_.stdout
    for bad in (["--problem_type", "cgpoisson"], ["--ngpus", "2", "--comm", "local"]):
        o = run(["--ndofs", "20000", "-pc_type", "sagg"] + bad)
        assert o.returncode != 0 and len(o.stderr.strip()) > 0
