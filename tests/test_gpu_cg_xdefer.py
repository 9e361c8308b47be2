"""GPU parity tests: the classical CG loop with its solution update deferred (ZZZ_CG_XDEFER: a ring of K direction vectors,
x read and written once per K iterations -- k_update_p_light / k_update_p_flush / k_x_apply_pending of csrc/zzz_cg.hip)
against the in-place loop (ZZZ_CG_XDEFER=0) on a fresh context.  Every entry of x receives the same multiplies and adds in
the same order, only later, so everything is compared BIT FOR BIT: solution, iteration count, both norms, the residual
history and the reason -- at every way a solve can end with updates still pending."""
import contextlib
import threading

from _gpu_helpers import *  # noqa: F401,F403 -- np / os / pytest / zzz / zo

pytestmark = pytest.mark.gpu  # noqa: F405

KS = (2, 4, 8)
NORMS = (zzz.NORM_PRECONDITIONED, zzz.NORM_UNPRECONDITIONED, zzz.NORM_NATURAL)


@contextlib.contextmanager
def _env(**knobs):
    """the knobs are read when a context is created: set for the block, restored afterwards (None: unset)"""
    saved = {k: os.environ.get(k) for k in knobs}
    try:
        for k, v in knobs.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _setup(c, P, matrix=True):
    c.upload_part(P)
    c.pattern_build()
    if matrix:
        c.assemble_matrix(P.form)
    c.assemble_vector(P.form)


def _solve(c, **kw):
    """one solve and everything that is compared"""
    it, rn, r0 = c.cg_solve(**kw)
    return dict(it=it, rn=rn, r0=r0, u=c.vec_download(zzz.VEC_U), hist=c.cg_history(it + 1), reason=c.cg_reason(),
                k=c.cg_info()["xdefer_k"])


def _same(a, b, what=""):
    assert a["it"] == b["it"], (what, a["it"], b["it"])
    assert a["reason"] == b["reason"], (what, a["reason"], b["reason"])
    # (norms of a breakdown are NaN on both sides: compared as arrays, where NaN equals NaN)
    np.testing.assert_array_equal(np.array([a["rn"], a["r0"]]), np.array([b["rn"], b["r0"]]), err_msg=str(what))
    np.testing.assert_array_equal(a["hist"], b["hist"], err_msg=str(what))
    np.testing.assert_array_equal(a["u"], b["u"], err_msg=str(what))


def _run(P, knobs, solves, prepare=None, matrix=True):
    """fresh context under `knobs`, the system of P, then the list of solves (keyword sets of cg_solve); prepare(c, i):
    called before solve i (without one, linalg::cg starts from zero and not from the previous solve's solution)"""
    with _env(**knobs):
        with zzz.Context(0) as c:
            _setup(c, P, matrix)
            out = []
            for i, kw in enumerate(solves):
                if prepare:
                    prepare(c, i)
                elif kw.get("variant") == zzz.CG_CGH:
                    c.vec_upload(zzz.VEC_U, np.zeros(c.n_owned * c.bs))
                out.append(_solve(c, **kw))
            return out


def _pairs(P, K, solves, prepare=None, matrix=True, extra=None):
    extra = extra or {}
    ref = _run(P, dict(ZZZ_CG_XDEFER=0, ZZZ_CG_XDEFER_K=None, **extra), solves, prepare, matrix)
    new = _run(P, dict(ZZZ_CG_XDEFER=2, ZZZ_CG_XDEFER_K=K, **extra), solves, prepare, matrix)
    assert all(r["k"] == 1 for r in ref)
    return ref, new


# (an odd number of rows -- the last entry has a path of its own -- and even ones)
_SYSTEMS = [("poisson", 1, (20, 18, 18)), ("poisson", 2, (6, 5, 7)), ("elasticity", 1, (8, 7, 9))]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("problem,order,dims", _SYSTEMS, ids=[f"{p}-P{o}" for p, o, _ in _SYSTEMS])
def test_deferred_update_keeps_every_bit(problem, order, dims, K):
    """K in {2, 4, 8} x Poisson P1 / P2, elasticity P1 x the three norm types x PCJACOBI (inverse diagonal as codes and as
    doubles) / PCNONE, and linalg::cg (ZZZ_CG_CGH)."""
    P = zzz.Part(problem, order, *dims)
    solves = [dict(pc=zzz.PC_JACOBI, norm=nm, rtol=1e-9) for nm in NORMS] + [dict(pc=zzz.PC_NONE, norm=nm, rtol=1e-9) for nm in NORMS]
    solves.append(dict(variant=zzz.CG_CGH, pc=zzz.PC_NONE, rtol=1e-7, max_it=2000))
    for codes in (0, 2):
        ref, new = _pairs(P, K, solves, extra=dict(ZZZ_CG_DINV_CODES=codes))
        for kw, a, b in zip(solves, ref, new):
            assert b["k"] == K and a["it"] > 2 * K and a["reason"] > 0, (kw, a["it"], b["k"])
            _same(a, b, (problem, order, K, codes, kw))


@pytest.mark.parametrize("K", KS)
def test_stopping_at_every_residue(K):
    """Where a solve stops decides what is still pending: max_it = 0 .. 2 K + 1 with a tolerance that is never met (both CG forms),
    and a sweep of rtol whose converged iteration counts cover every value of c mod K."""
    P = zzz.Part("poisson", 1, 12, 10, 13)
    solves = [dict(pc=zzz.PC_JACOBI, rtol=1e-30, max_it=m) for m in range(2 * K + 2)]
    solves += [dict(variant=zzz.CG_CGH, pc=zzz.PC_NONE, rtol=1e-30, max_it=m) for m in range(2 * K + 2)]
    rtols = [10.0 ** (-0.125 * e) for e in range(1, 89)]
    solves += [dict(pc=zzz.PC_JACOBI, rtol=r) for r in rtols]
    solves += [dict(variant=zzz.CG_CGH, pc=zzz.PC_NONE, rtol=r, max_it=5000) for r in rtols[:48]]
    ref, new = _pairs(P, K, solves)
    for kw, a, b in zip(solves, ref, new):
        assert b["k"] == K
        _same(a, b, (K, kw))
    n_cap = 2 * (2 * K + 2)
    assert [a["it"] for a in ref[:n_cap]] == 2 * list(range(2 * K + 2)) and all(a["reason"] == -3 for a in ref[:n_cap])
    conv = ref[n_cap:n_cap + len(rtols)]
    assert all(a["reason"] == 2 for a in conv)
    assert {a["it"] % K for a in conv} == set(range(K)), sorted({a["it"] for a in conv})
    assert {a["it"] % K for a in ref[n_cap + len(rtols):]} == set(range(K))


@pytest.mark.parametrize("K", KS)
def test_initial_guess_and_matrix_free_operator(K):
    """linalg::cg starts from what VEC_U holds (x0 != 0: the deferred updates land on it); the operator never assembled
    (op = OP_MATFREE), KSPCG + PCJACOBI / PCNONE and linalg::cg."""
    P = zzz.Part("poisson", 2, 5, 4, 6)
    x0 = np.random.default_rng(7).standard_normal(P.n_owned)
    solves = [dict(variant=zzz.CG_CGH, pc=zzz.PC_NONE, rtol=1e-7, max_it=1000),
              dict(variant=zzz.CG_CGH, pc=zzz.PC_NONE, rtol=1e-30, max_it=K + 1),
              dict(variant=zzz.CG_CGH, pc=zzz.PC_NONE, op=zzz.OP_MATFREE, rtol=1e-6, max_it=1000),
              dict(pc=zzz.PC_JACOBI, op=zzz.OP_MATFREE, rtol=1e-8),
              dict(pc=zzz.PC_NONE, op=zzz.OP_MATFREE, rtol=1e-8, norm=zzz.NORM_UNPRECONDITIONED)]

    def prepare(c, i):
        if i < 3:
            c.vec_upload(zzz.VEC_U, x0)

    ref, new = _pairs(P, K, solves, prepare)
    for kw, a, b in zip(solves, ref, new):
        assert b["k"] == K and a["it"] > 0
        _same(a, b, (K, kw))
    assert ref[1]["it"] == K + 1 and np.any(ref[1]["u"] != x0)
    # ... and with nothing but the mesh uploaded: no pattern, no matrix
    ref, new = _pairs(P, K, solves[3:], matrix=False)
    for kw, a, b in zip(solves[3:], ref, new):
        assert b["k"] == K and a["it"] > K
        _same(a, b, (K, "no matrix", kw))


@pytest.mark.parametrize("K", KS)
def test_breakdown_divergence_and_zero_right_hand_side(K):
    """A right-hand side of zeros (KSPCG stops at iteration 0; linalg::cg has no guard, runs to max_it and leaves NaN), a
    right-hand side that is not finite (KSP_DIVERGED_NANORINF), and a divergence tolerance that trips (KSP_DIVERGED_DTOL)."""
    P = zzz.Part("poisson", 1, 9, 8, 10)
    solves = [dict(pc=zzz.PC_JACOBI, rtol=1e-8), dict(pc=zzz.PC_NONE, rtol=1e-8, norm=zzz.NORM_NATURAL),
              dict(variant=zzz.CG_CGH, pc=zzz.PC_NONE, rtol=1e-6, max_it=2 * K + 1),
              dict(pc=zzz.PC_JACOBI, rtol=1e-8),
              dict(pc=zzz.PC_JACOBI, rtol=1e-8, dtol=0.5)]
    # (a limit above one trips where the norm first rises that far above its initial value, if it does: whatever happens,
    # it happens in both loops)
    solves += [dict(pc=pc, rtol=1e-8, dtol=d, norm=nm) for d in (1.0 + 1e-9, 1.01, 1.05, 1.2, 1.5, 2.0)
               for pc, nm in ((zzz.PC_JACOBI, zzz.NORM_PRECONDITIONED), (zzz.PC_NONE, zzz.NORM_NATURAL))]
    solves.append(dict(pc=zzz.PC_JACOBI, rtol=1e-8))
    keep = {}

    def prepare(c, i):
        if i == 0:
            keep["b"] = c.vec_download(zzz.VEC_B)
            c.vec_upload(zzz.VEC_B, np.zeros_like(keep["b"]))
        if i == 2:
            c.vec_upload(zzz.VEC_U, np.zeros_like(keep["b"]))
        if i == 3:
            bad = keep["b"].copy()
            bad[bad.size // 2] = np.inf
            c.vec_upload(zzz.VEC_B, bad)
        if i == 4:
            c.vec_upload(zzz.VEC_B, keep["b"])

    ref, new = _pairs(P, K, solves, prepare)
    for kw, a, b in zip(solves, ref, new):
        assert b["k"] == K
        _same(a, b, (K, kw))
    assert ref[0]["it"] == 0 and ref[1]["it"] == 0 and np.all(new[0]["u"] == 0)
    assert ref[2]["it"] == 2 * K + 1 and np.all(np.isnan(new[2]["u"]))
    assert ref[3]["reason"] == -9
    assert ref[4]["reason"] == -4 and all(a["reason"] in (-4, 2) for a in ref[5:]) and ref[-1]["reason"] == 2
    print("divergence test:", [(a["reason"], a["it"]) for a in ref[4:]])


@pytest.mark.parametrize("K", KS)
def test_solves_in_a_row_and_a_resized_ring(K):
    """Two right-hand sides one after the other on one context (nothing pending or stale carried over), then another mesh
    on the same context -- larger, then smaller again: the ring follows the vectors' size."""
    parts = [zzz.Part("poisson", 1, 10, 9, 11), zzz.Part("poisson", 1, 17, 15, 16), zzz.Part("elasticity", 1, 5, 4, 6)]
    res = {}
    for knob in (0, 2):
        with _env(ZZZ_CG_XDEFER=knob, ZZZ_CG_XDEFER_K=K):
            with zzz.Context(0) as c:
                out = []
                for P in parts:
                    _setup(c, P)
                    b = c.vec_download(zzz.VEC_B)
                    out.append(_solve(c, pc=zzz.PC_JACOBI, rtol=1e-9))
                    c.vec_upload(zzz.VEC_B, np.random.default_rng(K).standard_normal(b.size))
                    out.append(_solve(c, pc=zzz.PC_JACOBI, rtol=1e-9, max_it=3 * K + 1))
                    out.append(_solve(c, pc=zzz.PC_NONE, rtol=1e-7))
                    c.vec_upload(zzz.VEC_B, b)
                    out.append(_solve(c, pc=zzz.PC_JACOBI, rtol=1e-9))
                res[knob] = out
    for i, (a, b) in enumerate(zip(res[0], res[2])):
        assert a["k"] == 1 and b["k"] == K
        _same(a, b, (K, i))
    for j in range(len(parts)):  # the first right-hand side again: the same solve as the first time
        _same(res[2][4 * j], res[2][4 * j + 3], (K, "repeat", j))


@pytest.mark.parametrize("problem,order,dims,nparts", [("poisson", 1, (10, 9, 12), 2), ("poisson", 1, (8, 8, 13), 4),
                                                       ("elasticity", 1, (5, 5, 8), 2)])
@pytest.mark.parametrize("K", KS)
def test_partitioned_solve_with_the_update_deferred(problem, order, dims, nparts, K):
    """2 and 4 ranks on one GPU through the host-mediated local communicator (set up as test_partitioned_solve_on_one_gpu):
    the halo exchange and the overlapped product take each slot of the ring in turn; against the same partition in place."""

    def partitioned(knob, op):
        grp = zzz.LocalGroup(nparts)
        out, err = [None] * nparts, []

        def run(rank):
            try:
                P = zzz.Part(problem, order, *dims, nparts, rank)
                with zzz.Context(0) as c:
                    c.comm_init_local(grp.h, rank)
                    c.upload_part(P)
                    c.upload_halo(P)
                    c.pattern_build()
                    c.assemble_matrix(P.form)
                    c.assemble_vector(P.form)
                    res = [_solve(c, pc=zzz.PC_JACOBI, rtol=1e-8), _solve(c, pc=zzz.PC_JACOBI, rtol=1e-30, max_it=K + 1)]
                    if op:
                        res.append(_solve(c, pc=zzz.PC_JACOBI, op=zzz.OP_MATFREE, rtol=1e-8))
                    out[rank] = res
            except Exception as e:  # noqa: BLE001
                err.append((rank, repr(e)))

        with _env(ZZZ_CG_XDEFER=knob, ZZZ_CG_XDEFER_K=K):
            th = [threading.Thread(target=run, args=(r,)) for r in range(nparts)]
            for t in th:
                t.start()
            for t in th:
                t.join(timeout=300)
        grp.close()
        assert not err, err
        assert all(o is not None for o in out)
        return out

    matfree = problem == "poisson"
    ref, new = partitioned(0, matfree), partitioned(2, matfree)
    for rank in range(nparts):
        for i, (a, b) in enumerate(zip(ref[rank], new[rank])):
            assert a["k"] == 1 and b["k"] == K
            _same(a, b, (K, rank, i))
    assert len({o[0]["it"] for o in new}) == 1 and new[0][0]["it"] > 2 * K


def test_cg_info_says_which_solves_defer():
    """K > 1 for the classical loop under ZZZ_CG_XDEFER=2; K = 1 for the single-reduction, Chebyshev-Jacobi and pipelined
    solves, which keep their kernels, for a default-knob solve below the size rule, and for a K that is not 2, 4 or 8."""
    P = zzz.Part("poisson", 1, 12, 10, 14)
    solves = [dict(pc=zzz.PC_JACOBI, rtol=1e-8), dict(variant=zzz.CG_CGH, pc=zzz.PC_NONE, rtol=1e-6, max_it=500),
              dict(pc=zzz.PC_JACOBI, rtol=1e-8, single_reduction=True), dict(pc=zzz.PC_CHEBYSHEV_JACOBI, rtol=1e-8),
              dict(pc=zzz.PC_CHEBYSHEV_JACOBI, rtol=1e-8, single_reduction=True), dict(variant=zzz.CG_PIPE, pc=zzz.PC_JACOBI, rtol=1e-8),
              dict(pc=zzz.PC_NONE, rtol=1e-8)]
    for K in KS:
        new = _run(P, dict(ZZZ_CG_XDEFER=2, ZZZ_CG_XDEFER_K=K), solves)
        assert [r["k"] for r in new] == [K, K, 1, 1, 1, 1, K]
        assert all(r["reason"] > 0 for r in new)
    ref = _run(P, dict(ZZZ_CG_XDEFER=0, ZZZ_CG_XDEFER_K=None), solves)
    for a, b in zip(ref, new):
        _same(a, b)  # (the Chebyshev loop launches the in-place k_update_p: it must keep working beside the ring)
    assert [r["k"] for r in _run(P, dict(ZZZ_CG_XDEFER=None, ZZZ_CG_XDEFER_K=None), solves)] == [1] * len(solves)
    dflt = _run(P, dict(ZZZ_CG_XDEFER=2, ZZZ_CG_XDEFER_K=None), solves[:1])[0]["k"]
    assert dflt in KS
    assert _run(P, dict(ZZZ_CG_XDEFER=2, ZZZ_CG_XDEFER_K=3), solves[:1])[0]["k"] == dflt


def _cube_case(n, knobs, **kw):
    with _env(**knobs):
        with zzz.Context(0) as c:
            c.cube_generate("poisson", 1, n, n - 1, n + 1, 1, 0)
            c.pattern_build()
            c.assemble_matrix(zzz.FORM_POISSON)
            c.assemble_vector(zzz.FORM_POISSON)
            r = _solve(c, pc=zzz.PC_JACOBI, **kw)
            r["dinv"] = c.cg_info()["dinv_codes"] > 0
            return r


def test_size_rule_with_the_default_knob():
    """By default the update is deferred where an iteration's bytes exceed the Infinity Cache -- the rule of the non-temporal
    loads and of the coded inverse diagonal (200 MB per iteration): Poisson P1 cubes of the size sweep of
    tests/test_gpu_product.py either side of it (1.9 M rows: ~130 MB; 3.4 M rows: ~220 MB)."""
    dflt = dict(ZZZ_CG_XDEFER=None, ZZZ_CG_XDEFER_K=None, ZZZ_CG_DINV_CODES=None)
    small, large = _cube_case(124, dflt, rtol=1e-30, max_it=21), _cube_case(150, dflt, rtol=1e-30, max_it=21)
    assert small["k"] == 1 and not small["dinv"]
    assert large["k"] in KS and large["dinv"]
    for n, r in ((124, small), (150, large)):
        _same(_cube_case(n, dict(dflt, ZZZ_CG_XDEFER=0), rtol=1e-30, max_it=21), r, n)


def test_headline_system_takes_the_deferred_path_by_default():
    """The 10 016 937-dof Poisson P1 system of the headline with no knob set: K > 1, 975 +- 2 iterations, and bit for bit the
    in-place loop's solve."""
    nx, ny, nz, r = zzz.mesh_size(10000000, True, 1, 1, 1)
    dims = (nx << r, ny << r, nz << r)
    res = {}
    for knob in (None, 0):
        with _env(ZZZ_CG_XDEFER=knob, ZZZ_CG_XDEFER_K=None, ZZZ_CG_DINV_CODES=None):
            with zzz.Context(0) as c:
                c.cube_generate("poisson", 1, *dims, 1, 0)
                c.pattern_build()
                c.assemble_matrix(zzz.FORM_POISSON)
                c.assemble_vector(zzz.FORM_POISSON)
                res[knob] = _solve(c, pc=zzz.PC_JACOBI, rtol=1e-8)
    assert res[None]["k"] in KS and res[0]["k"] == 1
    assert abs(res[None]["it"] - 975) <= 2 and res[None]["reason"] == 2
    _same(res[0], res[None], "headline")
