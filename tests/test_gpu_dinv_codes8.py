"""GPU parity tests: Jacobi's inverse diagonal as 8-bit codes (at most 256 distinct values: one byte per row, the DZ = 2
instantiations of the vector kernels of csrc/zzz_cg.hip and csrc/zzz_cg_pipe.hip) against the same solve on 16-bit codes (ZZZ_CG_DINV_CODES=3) and on the
doubles (=0), each on a fresh context.  A code selects the same double from the table whatever its width, and the kernels
multiply the same doubles in the same order, so everything is compared BIT FOR BIT: solution, iteration count, both norms,
the residual history and the reason.

The matrices are a small P1 lattice's assembled values with rows and columns scaled symmetrically, v'[i, j] = (s_i s_j) v[i, j],
so that the inverse diagonal holds exactly the number of distinct values a case asks for; the count is proved in numpy before
a kernel sees the array.  Values go in through csr_upload_values."""
import contextlib

from _gpu_helpers import *  # noqa: F401,F403 -- np / os / pytest / zzz / zo
from _pipecg_ref import IT_BAR, pipecg_ref

pytestmark = pytest.mark.gpu  # noqa: F405

K = 4
NORMS = (zzz.NORM_PRECONDITIONED, zzz.NORM_UNPRECONDITIONED, zzz.NORM_NATURAL)
# 11 x 10 x 12 = 1 320 rows (even) and 11 x 9 x 13 = 1 287 rows (odd: the last entry has a path of its own in every kernel)
LATTICES = {"even": ("poisson", 1, (10, 9, 11)), "odd": ("poisson", 1, (10, 8, 12))}
_KNOBS = ("ZZZ_CG_DINV_CODES", "ZZZ_CG_XDEFER", "ZZZ_CG_XDEFER_K")


@contextlib.contextmanager
def _env(**knobs):
    """the knobs are read when a context is created: set for the block, every other one of this file unset, restored afterwards"""
    kw = {k: None for k in _KNOBS}
    kw.update(knobs)
    saved = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
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


_systems = {}


def _system(name):
    """(Part, rowptr, cols, assembled values, right-hand side) of a lattice, in the library's own CSR layout"""
    if name not in _systems:
        kind, order, dims = LATTICES[name]
        P = zzz.Part(kind, order, *dims)
        with _env():
            with zzz.Context(0) as c:
                c.upload_part(P)
                c.pattern_build()
                c.assemble_matrix(P.form)
                c.assemble_vector(P.form)
                rp, cl, v = c.csr_download()
                b = c.vec_download(zzz.VEC_B)
        _systems[name] = (P, rp.astype(np.int64), cl, v, b)
    return _systems[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _inverse_count(rp, cl, v):
    """distinct bit patterns of PCJACOBI's inverse diagonal: 1 / d, a zero entry replaced by one"""
    row = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    d = v[row == cl].copy()
    assert d.size == rp.size - 1
    d[d == 0.0] = 1.0
    return np.unique(_bits(1.0 / d)).size


_scaled = {}


def _scaled_values(name, count):
    """the lattice's values with rows and columns scaled by s (symmetrically; s = 1 but for one row per added value, each of
    them a row of the most frequent diagonal value) such that the inverse diagonal holds exactly `count` distinct patterns"""
    if (name, count) not in _scaled:
        _, rp, cl, v, _ = _system(name)
        n = rp.size - 1
        row = np.repeat(np.arange(n), np.diff(rp))
        d0 = v[row == cl]
        vals, freq = np.unique(d0, return_counts=True)
        rows = np.nonzero(d0 == vals[np.argmax(freq)])[0]
        s = np.ones(n)
        have = np.unique(_bits(1.0 / d0)).size
        assert have <= count <= have + rows.size - 1, (have, count, rows.size)
        j = 0
        for r in rows[1:]:
            if have == count:
                break
            j += 1
            s[r] = 1.0 + j * 2.0 ** -10
            now = np.unique(_bits(1.0 / ((s * s) * d0))).size
            assert now in (have, have + 1)
            if now == have:
                s[r] = 1.0
            have = now
        out = (s[row] * s[cl]) * v
        assert _inverse_count(rp, cl, out) == count
        _scaled[(name, count)] = out
    return _scaled[(name, count)]


def _solve(c, **kw):
    it, rn, r0 = c.cg_solve(**kw)
    info = c.cg_info()
    return dict(it=it, rn=rn, r0=r0, u=c.vec_download(zzz.VEC_U), hist=c.cg_history(it + 1), reason=c.cg_reason(),
                codes=info["dinv_codes"], bits=info["dinv_code_bits"], k=info["xdefer_k"])


def _same(a, b, what=""):
    assert a["it"] == b["it"], (what, a["it"], b["it"])
    assert a["reason"] == b["reason"], (what, a["reason"], b["reason"])
    np.testing.assert_array_equal(np.array([a["rn"], a["r0"]]), np.array([b["rn"], b["r0"]]), err_msg=str(what))
    np.testing.assert_array_equal(a["hist"], b["hist"], err_msg=str(what))
    np.testing.assert_array_equal(a["u"], b["u"], err_msg=str(what))


def _run(name, values, knob, solves, xdefer, k=K):
    """fresh context under ZZZ_CG_DINV_CODES=knob; the classical loop in place (xdefer False) or over a ring of k directions"""
    P = _system(name)[0]
    xd = dict(ZZZ_CG_XDEFER=2, ZZZ_CG_XDEFER_K=k) if xdefer else dict(ZZZ_CG_XDEFER=0)
    with _env(ZZZ_CG_DINV_CODES=knob, **xd):
        with zzz.Context(0) as c:
            c.upload_part(P)
            c.pattern_build()
            c.assemble_matrix(P.form)
            c.assemble_vector(P.form)
            c.csr_upload_values(values)
            return [_solve(c, **kw) for kw in solves]


def _three_ways(name, values, solves, xdefer, codes, bits, k=K):
    """knob 2 (the width the count allows) against 3 (16 bits) and 0 (doubles); the forms each run must report"""
    new, wide, dbl = (_run(name, values, knob, solves, xdefer, k) for knob in (2, 3, 0))
    for kw, a, w, d in zip(solves, new, wide, dbl):
        classical = not kw.get("single_reduction") and kw.get("variant") != zzz.CG_PIPE
        assert (a["codes"], a["bits"]) == (codes, bits), (kw, a["codes"], a["bits"])
        assert (w["codes"], w["bits"]) == (codes, 16), (kw, w["codes"], w["bits"])
        assert (d["codes"], d["bits"]) == (0, 0), (kw, d["codes"], d["bits"])
        assert a["k"] == w["k"] == d["k"] == (k if xdefer and classical else 1), (kw, a["k"], w["k"], d["k"])
        _same(w, a, (name, "against 16-bit codes", kw))
        _same(d, a, (name, "against doubles", kw))
    return new


_FORMS = [dict(pc=zzz.PC_JACOBI, norm=nm, rtol=1e-9) for nm in NORMS] + [
    dict(pc=zzz.PC_JACOBI, rtol=1e-9, single_reduction=True), dict(variant=zzz.CG_PIPE, pc=zzz.PC_JACOBI, rtol=1e-9)]


@pytest.mark.parametrize("xdefer", [False, True], ids=["K1", "K4"])
@pytest.mark.parametrize("name,count,bits", [("even", 256, 8), ("even", 257, 16), ("odd", 256, 8)])
def test_width_follows_the_count_and_every_bit_is_kept(name, count, bits, xdefer):
    """Exactly 256 distinct inverses: 8-bit codes; 257: 16-bit codes as before; an odd row count.  The classical form (three
    norm types; in place and with the solution update deferred over K = 4), the single-reduction form and pipecg."""
    v = _scaled_values(name, count)
    new = _three_ways(name, v, _FORMS, xdefer, count, bits)
    assert all(r["reason"] == 2 and r["it"] > 2 * K for r in new), [(r["reason"], r["it"]) for r in new]
    if not xdefer:  # ... and the oracle's solves within the project's bars
        _, rp, cl, _, b = _system(name)
        oit, ou, _, _ = zo.pcg(rp, cl, v, b, rtol=1e-9)
        sit, su, _, _ = zo.pcg_single_reduction(rp, cl, v, b, rtol=1e-9)
        pit, pu, _, _, _ = pipecg_ref(rp, cl, v, b, zzz.PC_JACOBI, zzz.NORM_PRECONDITIONED, 1e-9)
        assert abs(new[0]["it"] - oit) <= 2 and np.linalg.norm(new[0]["u"] - ou) <= 1e-6 * np.linalg.norm(ou)
        assert abs(new[3]["it"] - sit) <= 2 and np.linalg.norm(new[3]["u"] - su) <= 1e-6 * np.linalg.norm(su)
        assert abs(new[4]["it"] - pit) <= IT_BAR and np.linalg.norm(new[4]["u"] - pu) <= 1e-7 * np.linalg.norm(pu)


@pytest.mark.parametrize("name", ["even", "odd"])
def test_every_way_a_deferred_solve_can_end(name):
    """The iteration counts of tests/test_gpu_cg_xdefer.py with K = 4: max_it = 0 .. 2 K + 1 under a tolerance that is never
    met, and a sweep of rtol whose converged counts cover every value of c mod K -- the flush form, the light form and the pass
    over what is pending each read the 8-bit codes."""
    v = _scaled_values(name, 256)
    solves = [dict(pc=zzz.PC_JACOBI, rtol=1e-30, max_it=m) for m in range(2 * K + 2)]
    solves += [dict(pc=zzz.PC_JACOBI, rtol=10.0 ** (-0.125 * e)) for e in range(1, 89)]
    new = _three_ways(name, v, solves, True, 256, 8)
    ncap = 2 * K + 2
    assert [r["it"] for r in new[:ncap]] == list(range(ncap)) and all(r["reason"] == -3 for r in new[:ncap])
    assert all(r["reason"] == 2 for r in new[ncap:])
    assert {r["it"] % K for r in new[ncap:]} == set(range(K)), sorted({r["it"] for r in new[ncap:]})


@pytest.mark.parametrize("k", [2, 8], ids=["K2", "K8"])
@pytest.mark.parametrize("name", ["even", "odd"])
def test_ring_lengths_2_and_8_read_the_8bit_codes(name, k):
    """The ring lengths the other tests leave out: the flush form is compiled per ring length and chosen per form of the
    diagonal, so a mis-wired choice shows only here.  The classical form, max_it = 2 k + 1 under a tolerance never met: the
    light form, two flushes and one pending update, three ways bit for bit."""
    v = _scaled_values(name, 256)
    new = _three_ways(name, v, [dict(pc=zzz.PC_JACOBI, rtol=1e-30, max_it=2 * k + 1)], True, 256, 8, k)
    assert new[0]["bits"] == 8 and new[0]["k"] == k, (new[0]["bits"], new[0]["k"])
    assert new[0]["it"] == 2 * k + 1 and new[0]["reason"] == -3, (new[0]["it"], new[0]["reason"])


@pytest.mark.parametrize("xdefer", [False, True], ids=["K1", "K4"])
def test_zero_diagonal_entry(xdefer):
    """One diagonal entry 0.0: PCJACOBI's 1.0 is a table entry like any other.  Whatever the solve makes of the matrix in 50
    iterations, the 8-bit run makes the same."""
    _, rp, cl, _, _ = _system("even")
    v = _scaled_values("even", 200).copy()
    row = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    v[np.nonzero(row == cl)[0][(rp.size - 1) // 2]] = 0.0
    count = _inverse_count(rp, cl, v)  # (the row's own value may leave the set, and 1.0 may be in it already)
    assert 199 <= count <= 201
    _three_ways("even", v, [dict(max_it=50, **kw) for kw in _FORMS], xdefer, count, 8)


def test_default_knob_takes_8_bits_past_the_size_rule():
    """No knob set: a loop too large for the Infinity Cache (the 3.4 M-row cube of the size sweep) runs on codes, and its few
    distinct inverses make them 8 bits wide; 21 iterations against ZZZ_CG_DINV_CODES=3."""
    res = {}
    for knob in (None, 3):
        with _env(ZZZ_CG_DINV_CODES=knob):
            with zzz.Context(0) as c:
                c.cube_generate("poisson", 1, 150, 149, 151, 1, 0)
                c.pattern_build()
                c.assemble_matrix(zzz.FORM_POISSON)
                c.assemble_vector(zzz.FORM_POISSON)
                res[knob] = _solve(c, pc=zzz.PC_JACOBI, rtol=1e-30, max_it=21)
    assert 0 < res[None]["codes"] <= 256 and res[None]["bits"] == 8 and res[None]["k"] > 1, res[None]
    assert res[3]["codes"] == res[None]["codes"] and res[3]["bits"] == 16
    _same(res[3], res[None], "default against 16-bit codes")
