"""-pc_type mg (ZZZ_PC_MG, csrc/zzz_mg.hip) on several ranks: level 0 on the z-slabs of the generated cube, every coarser level
whole on every rank.  The ranks are threads of this process on one GPU with the host-mediated communicator (zzz.LocalGroup), as
tests/test_gpu_partitions.py::test_chebyshev_jacobi_partitioned_on_one_gpu runs them; a rank that fails breaks the group, so
no peer waits for it.  Every check is against a one-rank context on the same cube and against the numpy / scipy restatement
(tests/_mg_ref.py) fed with the library's own bounds.

Shapes: (10, 9, 12) nested in z (levels of 1430, 252, 64 dofs under the limit 200) on 2, 3 and 4 ranks; (7, 6, 9) not nested;
(6, 5, 3) on 3 ranks, slabs of one vertex plane and the capped top coarse index; elasticity (5, 5, 8), block size 3.

Bars (none comes from what the code under test gives):
  prolongation  the ranks' pieces, concatenated, are the one-rank result bit for bit (the same walk on the same numbers).
  restriction   equal on all ranks, bit-identical between two calls, within 1e-13 of max |out| of the one-rank result
                (test_gpu_mg's transfer bar: a sum of at most about 30 terms, here split in at most three places).
  V-cycle       1e-9 relative l2 to the restated cycle, symmetry defect 1e-12, positive: test_gpu_mg's bars and reasons.
  solves        the same count on all ranks, within +-1 of the one-rank library solve, under half the partitioned Jacobi count
                (the restatement: 8 against 67, 50, 32 and 13 against 138 on these cubes), the solution within 1e-6 of zo.pcg at
                rtol 1e-12 (the project's solution bar), rn <= 1e-8 r0."""
import threading

import numpy as np
import pytest

import zzz
import zzz_oracle as zo
from _mg_ref import Hierarchy

pytestmark = pytest.mark.gpu

CASES = [("poisson", (10, 9, 12), 2, 200), ("poisson", (10, 9, 12), 3, 200), ("poisson", (10, 9, 12), 4, 200),
         ("poisson", (7, 6, 9), 3, 100), ("poisson", (6, 5, 3), 3, 50), ("elasticity", (5, 5, 8), 2, 200),
         ("elasticity", (5, 5, 8), 4, 200)]
NORMS = (zzz.NORM_PRECONDITIONED, zzz.NORM_UNPRECONDITIONED, zzz.NORM_NATURAL)


def _form(kind):
    return zzz.FORM_ELASTICITY if kind == "elasticity" else zzz.FORM_POISSON


def _on_ranks(nparts, body):
    """body(rank, ctx, barrier) on nparts threads, each with a context of the local group; returns the ranks' results"""
    grp = zzz.LocalGroup(nparts)
    out, err = [None] * nparts, []
    bar = threading.Barrier(nparts)

    def run(rank):
        try:
            with zzz.Context(0) as c:
                c.comm_init_local(grp.h, rank)
                out[rank] = body(rank, c, bar)
        except Exception as e:  # noqa: BLE001
            err.append((rank, repr(e)))
            grp.abort()  # (the peers leave their collectives with an error instead of waiting)
            bar.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(nparts)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    alive = [t.is_alive() for t in th]
    if not any(alive):
        grp.close()
    assert not any(alive), "a rank did not come back"
    assert not err, err
    return out


def _generate(c, kind, n, nparts=1, rank=0, order=1):
    c.cube_generate(kind, order, *n, nparts, rank)
    c.pattern_build()
    c.assemble_matrix(_form(kind))
    c.assemble_vector(_form(kind))


def _table(c):
    nl = c.mg_info()["levels"]
    return [c.mg_info(l) for l in range(nl)]


def _vectors(kind, n):
    """coarse and fine noise, and a right-hand side that is zero at the constrained dofs"""
    G = zzz.Part(kind, 1, *n)
    rng = np.random.default_rng(31)
    nf = G.n_owned * G.bs
    free = 1.0 - G.bc_marker()[:nf]
    return dict(r=rng.standard_normal(nf), a=rng.standard_normal(nf), b=rng.standard_normal(nf), rhs=rng.standard_normal(nf) * free)


_one, _many = {}, {}


def _one_rank(kind, n, limit):
    key = (kind, n, limit)
    if key not in _one:
        zo.set_num_threads(4)
        V = _vectors(kind, n)
        with zzz.Context(0) as c:
            _generate(c, kind, n)
            c.mg_setup(pc_mg_coarse_eq_limit=limit)
            tab = _table(c)
            e = np.random.default_rng(32).standard_normal(tab[1]["dofs"])
            res = dict(V, e=e, table=tab, pe=c.mg_transfer(0, 0, e), rt=c.mg_transfer(0, 1, V["r"]), Ma=c.mg_apply(V["a"]))
            c.vec_upload(zzz.VEC_B, V["rhs"])
            rp, cl, v = c.csr_download()
            res["xt"] = zo.pcg(rp.astype(np.int64), cl, v, V["rhs"], rtol=1e-12)[1]
            res["its"] = [c.cg_solve(pc=zzz.PC_MG, norm=norm, rtol=1e-8, pc_mg_coarse_eq_limit=limit)[0] for norm in NORMS]
        _one[key] = res
    return _one[key]


def _ranks(kind, n, nparts, limit):
    key = (kind, n, nparts, limit)
    if key not in _many:
        R = _one_rank(kind, n, limit)

        def body(rank, c, bar):
            _generate(c, kind, n, nparts, rank)
            P = zzz.Part(kind, 1, *n, nparts, rank)
            lo, hi = P.own_offset * P.bs, (P.own_offset + P.n_owned) * P.bs
            c.mg_setup(pc_mg_coarse_eq_limit=limit)
            o = dict(lo=lo, hi=hi, table=_table(c), summary=c.mg_info())
            o["pe"] = c.mg_transfer(0, 0, R["e"])
            o["rt"] = c.mg_transfer(0, 1, R["r"][lo:hi])
            o["rt2"] = c.mg_transfer(0, 1, R["r"][lo:hi])
            o["Ma"], o["Mb"] = c.mg_apply(R["a"][lo:hi]), c.mg_apply(R["b"][lo:hi])
            c.vec_upload(zzz.VEC_B, R["rhs"][lo:hi])
            o["jacobi"] = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)[0]
            o["solves"] = []
            for norm in NORMS:
                it, rn, r0 = c.cg_solve(pc=zzz.PC_MG, norm=norm, rtol=1e-8, pc_mg_coarse_eq_limit=limit)
                o["solves"].append((it, rn, r0, c.vec_download(zzz.VEC_U), c.cg_info()["reason"]))
            o["setups"] = c.mg_info()["setups"]
            return o

        _many[key] = _on_ranks(nparts, body)
    return _one_rank(kind, n, limit), _many[key]


@pytest.mark.parametrize("kind,n,nparts,limit", CASES)
def test_level_table_and_transfer(kind, n, nparts, limit):
    R, out = _ranks(kind, n, nparts, limit)
    assert len(R["table"]) >= 2
    if n == (10, 9, 12):
        assert [t["dofs"] for t in R["table"]] == [1430, 252, 64]
    for o in out:
        # the whole cube's cells, dofs and nonzeros on every rank; levels 1.. are the one-rank run's to the bit, level 0's bound is
        # the partitioned estimate's (the ranks' common one: 1e-5, as the partitioned Chebyshev-Jacobi test takes it)
        assert len(o["table"]) == len(R["table"]) and o["summary"]["levels"] == len(R["table"])
        for l, (a, b) in enumerate(zip(o["table"], R["table"])):
            assert (a["cells"], a["dofs"], a["nnz"], a["degree"]) == (b["cells"], b["dofs"], b["nnz"], b["degree"]), (l, a, b)
            assert a["hi"] == b["hi"] if l else abs(a["hi"] - b["hi"]) <= 1e-5 * b["hi"], (l, a, b)
        assert o["table"] == out[0]["table"]
        assert o["setups"] == 1  # (the three solves found the hierarchy of mg_setup)
    assert [o["lo"] for o in out] == sorted(o["lo"] for o in out) and out[-1]["hi"] == R["pe"].size
    assert np.array_equal(np.concatenate([o["pe"] for o in out]), R["pe"])
    top = np.abs(R["rt"]).max()
    for o in out:
        assert np.array_equal(o["rt"], out[0]["rt"]) and np.array_equal(o["rt"], o["rt2"])
    d = np.abs(out[0]["rt"] - R["rt"]).max() / top
    print(f"mg on {nparts} ranks, {kind} {n}: restriction off the one-rank result by {d:.2e} of max |out|")
    assert d <= 1e-13


@pytest.mark.parametrize("kind,n,nparts,limit", CASES)
def test_vcycle_is_the_one_rank_operator(kind, n, nparts, limit):
    R, out = _ranks(kind, n, nparts, limit)
    his = [t["hi"] for t in out[0]["table"][:-1]]
    H = Hierarchy(kind, n, his=his, limit=limit)
    assert [tuple(t["cells"]) for t in out[0]["table"]] == list(H.dims)
    Ma, Mb = np.concatenate([o["Ma"] for o in out]), np.concatenate([o["Mb"] for o in out])
    ref = H.vcycle(R["a"])
    dv = np.linalg.norm(Ma - ref) / np.linalg.norm(ref)
    d1 = np.linalg.norm(Ma - R["Ma"]) / np.linalg.norm(R["Ma"])
    sym = abs(Ma @ R["b"] - R["a"] @ Mb) / (np.linalg.norm(Ma) * np.linalg.norm(R["b"]))
    print(f"mg on {nparts} ranks, {kind} {n}: V-cycle off the restatement by {dv:.2e}, off the one-rank library by {d1:.2e}, symmetry "
          f"defect {sym:.2e}")
    assert dv <= 1e-9
    assert sym <= 1e-12 and Ma @ R["a"] > 0.0 and Mb @ R["b"] > 0.0


@pytest.mark.parametrize("kind,n,nparts,limit", CASES)
def test_solves_with_every_norm_type(kind, n, nparts, limit):
    R, out = _ranks(kind, n, nparts, limit)
    itj = {o["jacobi"] for o in out}
    assert len(itj) == 1
    itj = itj.pop()
    for k, norm in enumerate(NORMS):
        its = {o["solves"][k][0] for o in out}
        assert len(its) == 1
        it = its.pop()
        u = np.concatenate([o["solves"][k][3] for o in out])
        err = np.linalg.norm(u - R["xt"]) / np.linalg.norm(R["xt"])
        print(f"mg on {nparts} ranks, {kind} {n}, norm {norm}: {it} iterations, one rank {R['its'][k]}, partitioned jacobi {itj}; "
              f"|u-xt|/|xt| {err:.2e}")
        assert abs(it - R["its"][k]) <= 1
        assert 2 * it < itj
        assert err <= 1e-6
        for o in out:
            _, rn, r0, _, reason = o["solves"][k]
            assert rn <= 1e-8 * r0 and reason == 2
            assert (rn, r0) == out[0]["solves"][k][1:3]  # (the scalars are all-reduced: every rank sees the same)


def test_refresh_equals_a_fresh_setup():
    """new matrix values on the live contexts (zzz_csr_upload_values): the kept levels with refreshed values give what contexts
    that never saw the old values give, to the bit"""
    kind, n, nparts, limit = "poisson", (10, 9, 12), 2, 200
    a = _vectors(kind, n)["a"]

    def body(refresh):
        def run(rank, c, bar):
            _generate(c, kind, n, nparts, rank)
            P = zzz.Part(kind, 1, *n, nparts, rank)
            lo, hi = P.own_offset * P.bs, (P.own_offset + P.n_owned) * P.bs
            v = c.csr_download()[2]
            if refresh:
                c.mg_setup(pc_mg_coarse_eq_limit=limit)
                before = c.mg_apply(a[lo:hi])
            c.csr_upload_values(1.5 * v)
            c.mg_setup(pc_mg_coarse_eq_limit=limit)
            z = c.mg_apply(a[lo:hi])
            if refresh:
                assert c.mg_info()["setups"] == 2 and not np.array_equal(z, before)
            return z, [t["hi"] for t in _table(c)]
        return run

    refreshed, fresh = _on_ranks(nparts, body(True)), _on_ranks(nparts, body(False))
    for (z1, h1), (z2, h2) in zip(refreshed, fresh):
        assert h1 == h2 and np.array_equal(z1, z2)


def test_alternating_with_jacobi_does_not_grow():
    kind, n, nparts, limit = "elasticity", (5, 5, 8), 2, 200

    def body(rank, c, bar):
        _generate(c, kind, n, nparts, rank)
        first = (c.cg_solve(pc=zzz.PC_MG, pc_mg_coarse_eq_limit=limit)[0], c.cg_solve(pc=zzz.PC_JACOBI)[0])
        u1 = c.vec_download(zzz.VEC_U)
        bar.wait()
        used1 = zzz.device_memory(0)[1] - zzz.device_memory(0)[0]
        bar.wait()
        for _ in range(4):
            again = (c.cg_solve(pc=zzz.PC_MG, pc_mg_coarse_eq_limit=limit)[0], c.cg_solve(pc=zzz.PC_JACOBI)[0])
            assert again == first and np.array_equal(u1, c.vec_download(zzz.VEC_U))
        assert c.mg_info()["setups"] == 1
        bar.wait()
        used5 = zzz.device_memory(0)[1] - zzz.device_memory(0)[0]
        bar.wait()
        return used1, used5

    for used1, used5 in _on_ranks(nparts, body):
        print(f"mg on {nparts} ranks: device memory in use after the first pair of solves {used1}, after five {used5}")
        assert abs(used5 - used1) <= 0.01 * used1


def _declined(c, **kw):
    with pytest.raises(zzz.ZzzError) as e:
        c.cg_solve(**dict(dict(pc=zzz.PC_MG), **kw))
    assert e.value.code == 1 and len(str(e.value)) > len("libzzz_hip error 1: "), str(e.value)
    return str(e.value)


def test_refusals_leave_every_rank_usable():
    kind, n = "poisson", (6, 5, 8)
    with zzz.Context(0) as c0:
        _generate(c0, kind, n)
        it0 = c0.cg_solve(pc=zzz.PC_JACOBI)[0]
        u0 = c0.vec_download(zzz.VEC_U)

    def jacobi_as_usual(c):
        it = c.cg_solve(pc=zzz.PC_JACOBI)[0]
        return it, c.vec_download(zzz.VEC_U)

    # a communicator of one rank: today's refusal, today's words
    def one(rank, c, bar):
        _generate(c, kind, n)
        msg = _declined(c)
        assert "a communicator is attached; multi-rank multigrid is not built" in msg
        return jacobi_as_usual(c)

    (it, u), = _on_ranks(1, one)
    assert abs(it - it0) <= 1 and np.linalg.norm(u - u0) <= 1e-6 * np.linalg.norm(u0)

    # the other multigrid kinds keep declining any communicator; order 2; nz < nparts (the generator refuses, on every rank)
    def two(rank, c, bar):
        _generate(c, kind, n, 2, rank)
        for pc in (zzz.PC_PMG, zzz.PC_AGG, zzz.PC_SAGG):
            assert "communicator" in _declined(c, pc=pc)
        assert "pipecg" in _declined(c, variant=zzz.CG_PIPE)
        assert "single_reduction" in _declined(c, single_reduction=True)
        assert c.cg_solve(pc=zzz.PC_MG, pc_mg_coarse_eq_limit=100)[0] <= 12
        # a hierarchy of one level would be a dense solve of a matrix that no rank holds
        assert "one level" in _declined(c, pc_mg_coarse_eq_limit=100000)
        with pytest.raises(zzz.ZzzError) as e:
            c.cube_generate(kind, 1, 4, 4, 1, 2, rank)
        assert "nz >= number of parts" in str(e.value)
        _generate(c, kind, (4, 3, 5), 2, rank, order=2)
        assert "P1 only" in _declined(c)
        jacobi_as_usual(c)
        _generate(c, kind, n, 2, rank)
        return jacobi_as_usual(c)

    out = _on_ranks(2, two)
    assert {o[0] for o in out} <= {it0 - 1, it0, it0 + 1} and len({o[0] for o in out}) == 1
    u = np.concatenate([o[1] for o in out])
    assert np.linalg.norm(u - u0) <= 1e-6 * np.linalg.norm(u0)

    # a native partition completed by zzz_ghost_layer_build is an uploaded feed: the library does not know the cube
    def native(rank, c, bar):
        P = zzz.Part(kind, 1, *n, 2, rank, native=True)
        c.upload_part(P)
        c.upload_halo(P)
        c.upload_global_ids(P.global_dofs, P.global_verts)
        c.ghost_layer_build()
        c.pattern_build()
        c.assemble_matrix(P.form)
        c.assemble_vector(P.form)
        assert "zzz_cube_generate" in _declined(c)
        return jacobi_as_usual(c)

    out = _on_ranks(2, native)
    assert {o[0] for o in out} <= {it0 - 1, it0, it0 + 1} and len({o[0] for o in out}) == 1
    u = np.concatenate([o[1] for o in out])
    assert np.linalg.norm(u - u0) <= 1e-6 * np.linalg.norm(u0)
