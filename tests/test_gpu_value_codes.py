"""GPU tests of the five value dictionaries at their capacity edges and on hostile bit patterns: the stream dictionary and the
per-slice dictionaries (csrc/zzz_sellp_dict.hip), Jacobi's inverse diagonal as codes (csrc/zzz_cg.hip), the block-row form's
block table and value dictionary (csrc/zzz_sellp_blk.hip), the block windows' dictionaries (csrc/zzz_sellp_win.hip); the shared
set: csrc/zzz_valset.h.

Values go in through csr_upload_values on a pattern assembled once; they come from tests/_value_sets.py, and
tests/test_value_sets.py proves on the CPU that every array holds exactly the number of distinct bit patterns its case claims --
every boundary case is on the side it says before a kernel sees it.

Bars: the product against the oracle's serial CSR loop (zo.spmv) as BIT PATTERNS, NaN exactly where the reference is NaN (x
finite); solves against zo.pcg / zo.pcg_single_reduction / zo.pcg_chebyshev with the project's bars (iterations +-2, solution
1e-6), the pipelined solve against its restatement with its own (tests/_pipecg_ref.py); a coded against an uncoded run of the
library on the same values (ZZZ_CG_DINV_CODES=2 against 0; ZZZ_SELLP_BLK=2 against 0) as the existing tests do: every bit /
iterations +-2 and 1e-9.  Every case asserts the form it expects through spmv_values_info() / cg_info().

Two things the forms answer differently from "the whole form steps aside", asserted as the code documents them: a slice
whose values the slice dictionary cannot hold (1 024 of them, or the all-ones pattern) stays doubles ALONE -- the form is still
"slice dictionaries", bytes_per_product grows; only when no slice is coded does the stream report "doubles".  And form 1 of the
block rows keeps its table's rows as raw bits found by fingerprints (0 marks an empty slot there), so the all-ones pattern is
an ordinary NaN to it and is served; form 2, whose VALUES go through the shared set, declines it."""
import contextlib
import os

import numpy as np
import pytest

import zzz
import zzz_oracle as zo
import _value_sets as vs
from _pipecg_ref import IT_BAR, pipecg_ref

pytestmark = pytest.mark.gpu

_KNOBS = ("ZZZ_SELLP", "ZZZ_SELLP_DICT", "ZZZ_SELLP_BLK", "ZZZ_SELLP_BWIN", "ZZZ_SELLP_EARLY", "ZZZ_CG_DINV_CODES", "ZZZ_RENUMBER")
STREAM = dict(ZZZ_SELLP_DICT=2, ZZZ_SELLP=2)
SLICES = dict(ZZZ_SELLP_DICT=3, ZZZ_SELLP_BWIN=0, ZZZ_SELLP=2)
BLOCKS = dict(ZZZ_SELLP_BLK=2, ZZZ_SELLP=2)
WINDOWS = dict(ZZZ_SELLP_BWIN=2, ZZZ_SELLP=2)
DEFAULT = dict()


class _Env:
    """the knobs of this file set as given and every other one of them unset, restored on the way out"""

    def __init__(self, **kw):
        self.kw = {k: None for k in _KNOBS}
        self.kw.update({k: str(v) for k, v in kw.items()})

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def _context(pname, **env):
    """a context on PROBLEMS[pname], pattern built and matrix and vector assembled once; the library's pattern and order are the
    oracle's (the value arrays are laid out on them)"""
    zo.set_num_threads(8)
    P, rp, cl, _, _ = vs.problem(pname)
    with _Env(**env):
        with zzz.Context(0) as c:
            c.upload_part(P)
            c.pattern_build()
            c.assemble_matrix(P.form)
            c.assemble_vector(P.form)
            crp, ccl, _ = c.csr_download(values=False)
            np.testing.assert_array_equal(crp, rp)
            np.testing.assert_array_equal(ccl, cl)
            perm, _ = c.internal_order()
            np.testing.assert_array_equal(perm, np.arange(P.n_owned))
            yield c


def _x(pname):
    _, rp, _, _, _ = vs.problem(pname)
    return np.random.default_rng(41).standard_normal(rp.size - 1)


def _same_bits(y, ref, what=""):
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(y), nan, err_msg=f"{what}: NaN where the serial loop has none, or none where it has")
    np.testing.assert_array_equal(y[~nan].view(np.uint64), ref[~nan].view(np.uint64), err_msg=f"{what}: product bits")


def _product(c, pname, case):
    """upload the case's values, one product against the serial CSR loop; returns spmv_values_info()"""
    _, rp, cl, _, _ = vs.problem(pname)
    assert vs.CASES[case][0] == pname
    v = vs.values(case)
    x = _x(pname)
    c.csr_upload_values(v)
    y = c.spmv(x)
    vi = c.spmv_values_info()
    print(f"{case}: form {vi['form']!r} special {vi['special_form']!r} block_form {vi['block_form']} distinct {vi['distinct_values']} "
          f"table {vi['block_table_entries']} bytes {vi['bytes_per_product']} as doubles {vi['bytes_per_product_as_doubles']}")
    with np.errstate(all="ignore"):
        _same_bits(y, zo.spmv(rp, cl, v, x), case)
    return vi


def _solves(c, pname, case, cheb=True):
    """Jacobi-PCG (classical, single reduction) and Chebyshev-Jacobi on the values just uploaded against the oracle's"""
    _, rp, cl, _, _ = vs.problem(pname)
    v = vs.values(case)
    b = c.vec_download(zzz.VEC_B)
    oit, ou, _, _ = zo.pcg(rp, cl, v, b, rtol=1e-8)
    it, rn, r0 = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
    u = c.vec_download(zzz.VEC_U)
    assert c.cg_reason() == 2 and rn <= 1e-8 * r0
    assert abs(it - oit) <= 2 and np.linalg.norm(u - ou) <= 1e-6 * np.linalg.norm(ou), (case, it, oit)
    sit, su, _, _ = zo.pcg_single_reduction(rp, cl, v, b, rtol=1e-8)
    its, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8, single_reduction=True)
    us = c.vec_download(zzz.VEC_U)
    assert abs(its - sit) <= 2 and np.linalg.norm(us - su) <= 1e-6 * np.linalg.norm(su), (case, its, sit)
    if cheb:
        cit, cu, _, _, est = zo.pcg_chebyshev(rp, cl, v, b, degree=2, ratio=10.0, rtol=1e-8, est_its=10)
        itc, _, _ = c.cg_solve(pc=zzz.PC_CHEBYSHEV_JACOBI, rtol=1e-8, pc_degree=2, pc_ratio=10.0, pc_esteig_its=0)
        uc = c.vec_download(zzz.VEC_U)
        assert c.cg_reason() == 2
        assert abs(c.cg_info()["pc_spectrum_bound"] - est) <= 2e-6 * est, (case, c.cg_info(), est)  # (not the previous values' bound)
        assert abs(itc - cit) <= 2 and np.linalg.norm(uc - cu) <= 1e-6 * np.linalg.norm(cu), (case, itc, cit)
    return it, u, its, us


# ---- 1. the stream dictionary ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,form,entries", [(2047, "dictionary in LDS", 2048), (2048, "dictionary in memory", 2049),
                                            (65534, "dictionary in memory", 65535), (65535, "doubles", 0)])
def test_stream_dictionary_forced_at_its_edges(n, form, entries):
    """ZZZ_SELLP_DICT=2: 2 047 values + (+0.0) fill the LDS copy's 2 048 entries; one more and the table is gathered from memory;
    65 534 values fill the 16-bit codes (entries 0 .. 65 534); one more and the stream stays doubles."""
    with _context("p1_17", **STREAM) as c:
        vi = _product(c, "p1_17", f"stream_forced_{n}")
    assert (vi["form"], vi["distinct_values"], vi["special_form"]) == (form, entries, ""), vi
    if form == "dictionary in LDS":
        assert vi["bytes_per_product"] < vi["bytes_per_product_as_doubles"]  # (a table of 65 535 costs this small matrix more than it saves)


def test_stream_dictionary_by_the_default_rule_at_its_edge():
    """No knob: a stream of 48 MiB or more gets the dictionary only if the LDS copy holds it -- 2 046 values yes, 2 047 no."""
    with _context("p1_80", **DEFAULT) as c:
        _, rp, _, _, _ = vs.problem("p1_80")
        a = _product(c, "p1_80", "stream_default_2046")
        assert a["bytes_per_product_as_doubles"] - 8 * ((rp.size - 1 + 63) // 64) >= 48 << 20, a  # (else: enlarge the problem)
        assert (a["form"], a["distinct_values"], a["special_form"]) == ("dictionary in LDS", 2047, ""), a
        b = _product(c, "p1_80", "stream_default_2047")
        assert (b["form"], b["distinct_values"], b["special_form"]) == ("doubles", 0, ""), b
        a2 = _product(c, "p1_80", "stream_default_2046")
        assert (a2["form"], a2["distinct_values"], a2["bytes_per_product"]) == ("dictionary in LDS", 2047, a["bytes_per_product"])


# ---- 2. the per-slice dictionaries --------------------------------------------------------------------------------------------
def test_slice_dictionaries_at_their_edge():
    """1 023 values per slice: every slice coded.  One slice, then every second slice, with 1 024: those slices stay doubles, the
    others coded, in one launch -- the form is kept, the bytes grow.  No slice that can be coded: the stream says doubles."""
    with _context("p3_555", **SLICES) as c:
        a = _product(c, "p3_555", "slices_all_1023")
        b = _product(c, "p3_555", "slices_one_1024")
        d = _product(c, "p3_555", "slices_odd_1024")
        e = _product(c, "p3_555", "p3_555_all")
        a2 = _product(c, "p3_555", "slices_all_1023")
    for vi in (a, b, d, a2):
        assert (vi["form"], vi["special_form"]) == ("slice dictionaries", ""), vi
    assert a["bytes_per_product"] < b["bytes_per_product"] < d["bytes_per_product"] < d["bytes_per_product_as_doubles"]
    assert a2["bytes_per_product"] == a["bytes_per_product"]
    assert (e["form"], e["special_form"]) == ("doubles", ""), e


# ---- 3. Jacobi's inverse diagonal as codes --------------------------------------------------------------------------------------
def _dinv_runs(case, max_it=10000, variants=("classical", "single_reduction", "pipelined")):
    out = {}
    for knob in (0, 2):
        with _context("p1_diag", ZZZ_CG_DINV_CODES=knob) as c:
            c.csr_upload_values(vs.values(case))
            res = []
            for var in variants:
                kw = dict(variant=zzz.CG_PIPE) if var == "pipelined" else dict(single_reduction=var == "single_reduction")
                it, rn, r0 = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-9, max_it=max_it, **kw)
                res.append(dict(var=var, it=it, rn=rn, r0=r0, u=c.vec_download(zzz.VEC_U), codes=c.cg_info()["dinv_codes"],
                                reason=c.cg_reason(), hist=c.cg_history(it + 1)))
            out[knob] = res
            b = c.vec_download(zzz.VEC_B)
    return out, b


def _coded_equals_uncoded(out, case):
    for p, q in zip(out[0], out[2]):
        print(f"{case} {p['var']}: uncoded it {p['it']} reason {p['reason']}, coded it {q['it']} reason {q['reason']} codes {q['codes']}")
        assert p["codes"] == 0
        assert (p["it"], p["reason"]) == (q["it"], q["reason"]), (case, p["var"])
        np.testing.assert_array_equal(p["hist"], q["hist"])  # (NaN where NaN)
        np.testing.assert_array_equal(np.array([p["rn"], p["r0"]]), np.array([q["rn"], q["r0"]]))
        np.testing.assert_array_equal(p["u"], q["u"])


@pytest.mark.parametrize("d,codes", [(2048, 2048), (2049, 0), (13800, 0)])
def test_inverse_diagonal_codes_at_their_edge(d, codes):
    """2 048 distinct inverses fill the table; 2 049 -- and every row its own value, where the set must decline while thousands of
    wavefronts insert -- leave z = D^-1 r to the doubles.  Classical, single-reduction and pipelined solves: the coded run equals
    the uncoded one bit for bit, and the oracle's within the bars."""
    case = f"dinv_{d}"
    out, b = _dinv_runs(case)
    _coded_equals_uncoded(out, case)
    assert [q["codes"] for q in out[2]] == [codes] * 3
    _, rp, cl, _, _ = vs.problem("p1_diag")
    v = vs.values(case)
    oit, ou, _, _ = zo.pcg(rp, cl, v, b, rtol=1e-9)
    sit, su, _, _ = zo.pcg_single_reduction(rp, cl, v, b, rtol=1e-9)
    pit, pu, _, _, _ = pipecg_ref(rp, cl, v, b, zzz.PC_JACOBI, zzz.NORM_PRECONDITIONED, 1e-9)
    q = out[2]
    assert all(r["reason"] == 2 for r in q)
    assert abs(q[0]["it"] - oit) <= 2 and np.linalg.norm(q[0]["u"] - ou) <= 1e-6 * np.linalg.norm(ou)
    assert abs(q[1]["it"] - sit) <= 2 and np.linalg.norm(q[1]["u"] - su) <= 1e-6 * np.linalg.norm(su)
    assert abs(q[2]["it"] - pit) <= IT_BAR and np.linalg.norm(q[2]["u"] - pu) <= 1e-7 * np.linalg.norm(pu)


@pytest.mark.parametrize("kind", ["zero", "subnormal", "inf", "negative"])
def test_inverse_diagonal_codes_on_a_diagonal_that_ends_the_solve(kind):
    """One diagonal entry 0.0 (PCJACOBI's 1.0), subnormal (inverse Inf), Inf (inverse +0.0) or negative: whatever the solve makes of
    it in 50 iterations, the coded run makes the same -- reason, count, history (NaN where NaN)."""
    case = f"dinv_end_{kind}"
    out, _ = _dinv_runs(case, max_it=50)
    _coded_equals_uncoded(out, case)
    assert all(64 <= q["codes"] <= 65 for q in out[2]), [q["codes"] for q in out[2]]  # (64 values and the one written over one row)


@pytest.mark.parametrize("kind", ["nan", "all_ones"])
def test_inverse_diagonal_codes_on_a_nan_diagonal(kind):
    """A diagonal entry holding the quiet NaN / the all-ones pattern (the set's empty marker).  Whether 1.0 / NaN keeps the payload is
    the hardware's business: only that the coded and the uncoded solve end alike."""
    case = f"dinv_end_{kind}"
    out, _ = _dinv_runs(case, max_it=50)
    _coded_equals_uncoded(out, case)


def test_inverse_diagonal_codes_across_uploads_on_one_context():
    """One context: 2 048 inverses (coded), 2 049 (declined), 2 048 again, then 1 000 of which 300 hash to the last four slots of
    the set's 2^14 (probe chains that wrap): after each upload the expected count and solves within the bars."""
    with _context("p1_diag", ZZZ_CG_DINV_CODES=2) as c:
        for case, codes in (("dinv_2048", 2048), ("dinv_2049", 0), ("dinv_2048", 2048), ("dinv_clustered", 1000), ("dinv_13800", 0)):
            c.csr_upload_values(vs.values(case))
            _solves(c, "p1_diag", case)
            c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
            assert c.cg_info()["dinv_codes"] == codes, (case, c.cg_info())
            c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8, single_reduction=True)
            assert c.cg_info()["dinv_codes"] == codes, (case, c.cg_info())
    out, _ = _dinv_runs("dinv_clustered")
    _coded_equals_uncoded(out, "dinv_clustered")
    assert [q["codes"] for q in out[2]] == [1000] * 3


# ---- 4. block rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,nv,served,form,entries", [(2199, 400, True, 1, 2200), (2200, 400, True, 2, 2201), (5000, 2046, True, 2, 5001),
                                                       (5000, 2047, False, 0, 0), (65535, 40, True, 2, 65536), (65536, 40, False, 0, 0)])
def test_block_rows_at_their_edges(nb, nv, served, form, entries):
    """2 199 blocks + the zero block fill the table in LDS (form 1); one more: rows of offsets into a value dictionary (form 2), which
    holds 2 046 values, not 2 047; 65 535 blocks fill the 16-bit block codes, 65 536 do not.  Blocks one entry apart, permutations
    of each other, apart by the sign of a zero, whole blocks of -0.0 in every one.  Declined: the generic stream's product."""
    with _context("el_20", **BLOCKS) as c:
        vi = _product(c, "el_20", f"blocks_{nb}_{nv}")
    assert vi["block_rows"] == served and vi["special_form"] == ("block rows" if served else ""), vi
    if served:
        assert (vi["block_form"], vi["block_table_entries"]) == (form, entries) and vi["block_chunks"] >= 1, vi


@pytest.mark.parametrize("nb,nv,form", [(2199, 400, 1), (2200, 400, 2), (2200, 2046, 2)])
def test_block_rows_solve_at_their_edges(nb, nv, form):
    """Symmetric, diagonally dominant values at the same edges: classical and single-reduction solves of the block-row form against
    the generic stream's (ZZZ_SELLP_BLK=0; iterations +-2, solution 1e-9) and the oracle's (+-2, 1e-6)."""
    case = f"blocks_spd_{nb}_{nv}"
    res = {}
    for blk in (2, 0):
        with _context("el_20", ZZZ_SELLP_BLK=blk, ZZZ_SELLP=2) as c:
            vi = _product(c, "el_20", case)
            assert vi["block_rows"] == (blk == 2) and (blk == 0 or vi["block_form"] == form), vi
            res[blk] = _solves(c, "el_20", case, cheb=False)
    a, b = res[2], res[0]
    assert abs(a[0] - b[0]) <= 2 and abs(a[2] - b[2]) <= 2
    assert np.linalg.norm(a[1] - b[1]) <= 1e-9 * np.linalg.norm(b[1]) and np.linalg.norm(a[3] - b[3]) <= 1e-9 * np.linalg.norm(b[3])


# ---- 5. block windows ---------------------------------------------------------------------------------------------------------------
def test_block_windows_at_their_edges():
    """One block of 4 096 rows: 4 095 values fill the 12-bit codes (the largest, 0xFFF, in use), 4 096 take the 16-bit plane (more
    bytes), 8 191 fill the block's table; 8 192 and the generic stream serves."""
    with _context("p3_555", **WINDOWS) as c:
        vi = {w: _product(c, "p3_555", f"windows_{w}") for w in (4095, 4096, 8191, 8192, 4095)}
    for w in (4095, 4096, 8191):
        assert (vi[w]["special_form"], vi[w]["block_form"]) == ("block windows", 1) and vi[w]["block_table_entries"] >= 4096, (w, vi[w])
    assert vi[4095]["bytes_per_product"] < vi[4096]["bytes_per_product"] < vi[8191]["bytes_per_product"]
    assert vi[4096]["bytes_per_product"] - vi[4095]["bytes_per_product"] > 8  # (more than the one table entry: the plane of codes)
    assert (vi[8192]["special_form"], vi[8192]["block_form"]) == ("", 0), vi[8192]


@pytest.mark.parametrize("pname,nblk", [("p3_546", 1), ("p3_666", 2)])
def test_block_windows_on_a_padded_block_and_on_two_blocks(pname, nblk):
    """3 952 rows (one block, padding rows) and 6 859 (two blocks): 8 191 values matrix-wide are served whichever block they fall
    into; every entry its own value is declined."""
    with _context(pname, **WINDOWS) as c:
        a = _product(c, pname, f"windows_{pname}_8191")
        b = _product(c, pname, f"windows_{pname}_all")
        a2 = _product(c, pname, f"windows_{pname}_8191")
    assert (a["special_form"], a["block_form"]) == ("block windows", nblk), a
    assert (a2["special_form"], a2["bytes_per_product"]) == ("block windows", a["bytes_per_product"]), a2
    assert (b["special_form"], b["form"]) == ("", "doubles"), b


# ---- 6. hostile bits through every form -----------------------------------------------------------------------------------------------
def _served(vi, special="", form=None, block_form=None):
    ok = vi["special_form"] == special and (form is None or vi["form"] == form) and (block_form is None or vi["block_form"] == block_form)
    assert ok, vi


def test_hostile_bits_through_the_stream_dictionary():
    """-0.0 (entries, a whole row), subnormals, DBL_MIN / DBL_MAX, values one ulp apart and equal in one 32-bit half; then +-Inf and
    the quiet NaN; then the all-ones pattern (the set's empty marker: the stream stays doubles); then 300 values whose probe chains
    wrap round the end of the set's 2^18 slots."""
    with _context("p1_17", **STREAM) as c:
        _served(_product(c, "p1_17", "hostile_p1_17_0"), form="dictionary in LDS")
        _served(_product(c, "p1_17", "hostile_p1_17_1"), form="dictionary in LDS")
        _served(_product(c, "p1_17", "hostile_p1_17_2"), form="doubles")
        _served(_product(c, "p1_17", "clustered_p1_17_18"), form="dictionary in LDS")


def test_hostile_bits_through_the_slice_dictionaries():
    """As above; the all-ones pattern in two slices: those stay doubles (more bytes than the same values without it would take, the
    form kept); in every slice: the stream says doubles.  Chains that wrap round the LDS set's 2^11 slots."""
    with _context("p3_555", **SLICES) as c:
        a = _product(c, "p3_555", "hostile_p3_555_0")
        b = _product(c, "p3_555", "hostile_p3_555_1")
        d = _product(c, "p3_555", "hostile_p3_555_2")
        e = _product(c, "p3_555", "hostile_p3_555_2_every_slice")
        f = _product(c, "p3_555", "clustered_p3_555_11")
    for vi in (a, b, d, f):
        _served(vi, form="slice dictionaries")
    assert d["bytes_per_product"] > b["bytes_per_product"] + 16384 and d["bytes_per_product"] > a["bytes_per_product"] + 16384
    _served(e, form="doubles")


def test_hostile_bits_through_the_block_rows():
    """As above, plus -0.0 as a whole 3 x 3 block (dropped like a zero block) and as one entry inside a kept block (a value).  Form 1
    (raw rows, found by fingerprints) serves the all-ones pattern like any NaN; form 2 (values through the shared set) declines."""
    with _context("el_20", **BLOCKS) as c:
        _served(_product(c, "el_20", "hostile_el_20_0"), "block rows", block_form=1)
        _served(_product(c, "el_20", "hostile_el_20_1"), "block rows", block_form=1)
        _served(_product(c, "el_20", "hostile_el_20_2"), "block rows", block_form=1)
        _served(_product(c, "el_20", "hostile_el_20_0_form2"), "block rows", block_form=2)
        _served(_product(c, "el_20", "hostile_el_20_1_form2"), "block rows", block_form=2)
        _served(_product(c, "el_20", "hostile_el_20_2_form2"), "")
        _served(_product(c, "el_20", "clustered_el_20_13"), "block rows", block_form=2)


def test_hostile_bits_through_the_block_windows():
    """As above; the all-ones pattern: the form declines and the generic stream serves; chains that wrap round the LDS set's 2^14."""
    with _context("p3_555", **WINDOWS) as c:
        _served(_product(c, "p3_555", "hostile_p3_555_0"), "block windows")
        _served(_product(c, "p3_555", "hostile_p3_555_1"), "block windows")
        _served(_product(c, "p3_555", "hostile_p3_555_2"), "", form="doubles")
        _served(_product(c, "p3_555", "clustered_p3_555_14"), "block windows")


@pytest.mark.parametrize("pname", ["p1_17", "p3_555", "el_20"])
def test_hostile_bits_with_no_knob_set(pname):
    """The default configuration at these sizes codes nothing (the rules want larger matrices): the same inputs, the same bits."""
    with _context(pname, **DEFAULT) as c:
        for lvl in (0, 1, 2):
            _served(_product(c, pname, f"hostile_{pname}_{lvl}"), "", form="doubles")


# ---- 7. one context across forms ----------------------------------------------------------------------------------------------------
def _walk(pname, env, steps):
    """steps: (case, check(values info), solve?) uploaded in turn on one context"""
    seen = []
    with _context(pname, **env) as c:
        for case, check, solve in steps:
            vi = _product(c, pname, case)
            check(vi)
            if solve:
                _solves(c, pname, case)
            seen.append(vi)
    return seen


def test_one_context_across_the_stream_dictionary_forms():
    lds = lambda vi: _served(vi, form="dictionary in LDS")
    mem = lambda vi: _served(vi, form="dictionary in memory")
    dbl = lambda vi: _served(vi, form="doubles")
    _walk("p1_17", STREAM, [("stream_spd_1500", lds, True), ("stream_forced_65535", dbl, False), ("stream_spd_2047", lds, True),
                            ("stream_spd_2048", mem, True), ("stream_spd_30000", mem, True), ("stream_spd_1500", lds, True)])


def test_one_context_across_the_slice_dictionary_forms():
    lds = lambda vi: _served(vi, form="dictionary in LDS")
    sd = lambda vi: _served(vi, form="slice dictionaries")
    dbl = lambda vi: _served(vi, form="doubles")
    _walk("p3_555", SLICES, [("p3_555_spd_1500", lds, True), ("slices_all_1023", sd, False), ("p3_555_all", dbl, False),
                             ("p3_555_spd_sliced", sd, True), ("slices_odd_1024", sd, False), ("p3_555_spd_1500", lds, True)])


@pytest.mark.parametrize("env", [dict(ZZZ_SELLP_BLK=2), BLOCKS], ids=["early", "at_first_product"])
def test_one_context_across_the_block_row_forms(env):
    """(No ZZZ_SELLP: the special form is built when the values arrive and the generic stream is not packed -- until values come that
    the form cannot hold.)"""
    f1 = lambda vi: _served(vi, "block rows", block_form=1)
    f2 = lambda vi: _served(vi, "block rows", block_form=2)
    gen = lambda vi: _served(vi, "")
    _walk("el_20", env, [("blocks_spd_2199_400", f1, True), ("blocks_65536_40", gen, False), ("blocks_spd_2200_400", f2, True),
                         ("blocks_spd_2200_2047", gen, True), ("blocks_spd_2199_400", f1, True)])


@pytest.mark.parametrize("env", [dict(ZZZ_SELLP_BWIN=2), WINDOWS], ids=["early", "at_first_product"])
def test_one_context_across_the_block_window_forms(env):
    win = lambda vi: _served(vi, "block windows")
    gen = lambda vi: _served(vi, "", form="doubles")
    seen = _walk("p3_555", env, [("windows_spd_3000", win, True), ("windows_8192", gen, False), ("windows_spd_4095", win, True),
                                 ("windows_spd_4096", win, True), ("p3_555_all", gen, False), ("windows_spd_8191", win, True),
                                 ("windows_spd_3000", win, True)])
    assert seen[0]["bytes_per_product"] == seen[6]["bytes_per_product"] < seen[2]["bytes_per_product"] < seen[3]["bytes_per_product"]
    assert seen[3]["bytes_per_product"] - seen[2]["bytes_per_product"] > 8  # (12-bit codes gave way to 16: not just one more table entry)
