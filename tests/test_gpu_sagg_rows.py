"""GPU tests of the row-by-row products of -pc_type sagg and -pc_type sagg_rbm (ZZZ_MG_PRODUCTS_ROWS, csrc/zzz_sagg_rows.hip;
zzz_mg_products, zzz_mg_products_info).  The mode changes how the sums of P, T = A P and A_c = P^T T are organised,
not what they are, so the bar of every comparison with the lists mode is np.array_equal: P, every coarse matrix, the coarse
near-nullspaces, the counts, a V-cycle, the transfers, iteration counts, residual histories and solutions.  The rows-mode
hierarchy is also held against the restatements (tests/_sagg_ref.py, tests/_sagg_rbm_ref.py) with the bars of
tests/test_gpu_sagg.py and tests/test_gpu_sagg_rbm.py (patterns exact, values within R.row_bars), so that both modes drifting
together would still be caught.  Cases, limit (50: three levels at least) and feeds are those two files'; the lists-mode
context and the restatement of a case are the ones those files cache, built once per session.

Counts that come from the restatement, not from the code under test: the longest row of A_c has 20 007 candidates on
elasticity_p2 and 12 634 on poisson_p3 (both above the budget of 4 096 the chunk tests set, so each forms a chunk alone), the
longest rows of spoke_poisson have 108 and 107 (budget 128: chunks of one to four rows)."""
import os
import subprocess

import numpy as np
import pytest

import zzz
import _sagg_ref as R
import _sagg_rbm_ref as RR
import test_gpu_sagg as TS
import test_gpu_sagg_rbm as TR
from _hostile_gpu import _env

pytestmark = pytest.mark.gpu

LISTS, ROWS = zzz.MG_PRODUCTS_LISTS, zzz.MG_PRODUCTS_ROWS
NORMS = TS.NORMS
CASES = [("sagg", n) for n in R.CASE_IDS] + [("sagg_rbm", n) for n in RR.ELASTICITY]
IDS = [f"{k}-{n}" for k, n in CASES]


def _mod(kind):
    return TR if kind == "sagg_rbm" else TS


def _opts(kind):
    return TR.RBM if kind == "sagg_rbm" else TS.SAGG


def _stored(c, kind):
    """what the hierarchy holds: per level the counts and bounds, P, the coarse matrix, and for sagg_rbm the near-nullspaces"""
    info = c.mg_info()
    out = [np.array([info["levels"], info["coarse_dofs"], info["products_per_cycle"]])]
    for l in range(info["levels"]):
        li = c.mg_info(l)
        out.append(np.array([li["dofs"], li["nnz"], li["dropped"], li["degree"], li["hi"], li["lo"]]))
    for l in range(info["levels"] - 1):
        out.extend(c.mg_level_p(l))
        out.extend(c.mg_level_csr(l + 1))
    if kind == "sagg_rbm":
        out.extend(c.mg_level_nns(l) for l in range(info["levels"]))
    return out


def _applied(c, kind):
    """... and what it does: a V-cycle of two random vectors, every transfer both ways, the solves with the three norm types"""
    rng = np.random.default_rng(5)
    info = c.mg_info()
    n = c.mg_info(0)["dofs"]
    out = [c.mg_apply(rng.standard_normal(n)), c.mg_apply(rng.standard_normal(n))]
    for l in range(info["levels"] - 1):
        out.append(c.mg_transfer(l, 0, rng.standard_normal(c.mg_info(l + 1)["dofs"])))
        out.append(c.mg_transfer(l, 1, rng.standard_normal(c.mg_info(l)["dofs"])))
    for norm in NORMS:
        it, rn, r0 = c.cg_solve(norm=norm, rtol=1e-8, **_opts(kind))
        out.extend([np.array([it, c.cg_info()["reason"]]), np.array([rn, r0]), c.cg_history(it + 1), c.vec_download(zzz.VEC_U)])
    return out


def _equal(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), f"{what}: item {i} differs"


def _fresh(kind, P, mode, bc_dofs=None, setup=True):
    c = zzz.Context(0)
    _mod(kind)._feed(c, P, bc_dofs)
    c.mg_products(mode)
    if setup:
        c.mg_setup(**_opts(kind))
    return c


_rows = {}


def _rows_case(kind, name):
    """the rows-mode context of a case at the default budget, one per session, with what it stores"""
    if (kind, name) not in _rows:
        c = _fresh(kind, _mod(kind)._case(name)[1], ROWS)
        _rows[kind, name] = (c, _stored(c, kind))
    return _rows[kind, name]


@pytest.mark.parametrize("kind,name", CASES, ids=IDS)
def test_rows_give_the_bits_of_lists_and_the_restatement_holds(kind, name):
    cl, P, H = _mod(kind)._case(name)
    cl.mg_products(LISTS)
    cl.mg_setup(**_opts(kind))
    cr, stored = _rows_case(kind, name)
    assert len(H.A) >= 3
    li, ri = cl.mg_products_info(), cr.mg_products_info()
    print(f"{kind} {name}: lists keep {li['kept_bytes']} B, rows {ri['kept_bytes']} B; rows: {ri}")
    assert li["mode"] == LISTS and ri["mode"] == ROWS and li["chunks"] == 0 and ri["chunks"] >= 3 * (len(H.A) - 1)
    assert ri["kept_bytes"] < li["kept_bytes"] and ri["lone_rows"] == 0 and ri["budget"] > ri["max_row_candidates"] > 0
    _equal(_stored(cl, kind), stored, f"{kind} {name}: the stored hierarchy")
    _equal(_applied(cl, kind), _applied(cr, kind), f"{kind} {name}: cycle, transfers, solves")
    _mod(kind)._check_hierarchy(cr, H, f"{name} rows")


@pytest.mark.parametrize("kind,name", CASES, ids=IDS)
def test_chunks_of_a_small_budget_give_the_same_hierarchy(kind, name):
    stored = _rows_case(kind, name)[1]
    P = _mod(kind)._case(name)[1]
    chunks = 0
    for budget in (4096, 128) if name == "spoke_poisson" else (4096,):
        with _env(ZZZ_SAGG_ROWS_BUDGET=str(budget)), _fresh(kind, P, ROWS) as c:
            info = c.mg_products_info()
            print(f"{kind} {name} budget {budget}: {info}")
            assert info["mode"] == ROWS and info["budget"] == budget and info["chunks"] >= 3 and info["chunks"] > chunks
            chunks = info["chunks"]
            if kind == "sagg" and name in ("elasticity_p2", "poisson_p3"):
                assert info["lone_rows"] >= 1 and info["max_row_candidates"] >= (20007 if name == "elasticity_p2" else 12634)
            _equal(_stored(c, kind), stored, f"{kind} {name}: budget {budget} against the default budget")
            if budget == 128 or name == "elasticity_p2":
                _equal(_applied(c, kind), _applied(_rows_case(kind, name)[0], kind), f"{kind} {name}: budget {budget}, applied")


@pytest.mark.parametrize("kind,name", [("sagg", "poisson_p2"), ("sagg_rbm", "elasticity_p1")])
def test_rows_too_long_for_lds_accumulate_in_memory_to_the_same_bits(kind, name):
    """ZZZ_SAGG_ROWS_LDS lowers the row length that accumulates in LDS to 8: nearly every row of T and A_c takes the other path"""
    stored = _rows_case(kind, name)[1]
    with _env(ZZZ_SAGG_ROWS_LDS="8"), _fresh(kind, _mod(kind)._case(name)[1], ROWS) as c:
        assert max(int(np.diff(c.mg_level_csr(l)[0]).max()) for l in range(1, c.mg_info()["levels"])) > 8
        _equal(_stored(c, kind), stored, f"{kind} {name}: accumulators in memory")


@pytest.mark.parametrize("renumber", [None, "0"], ids=["internal-order", "callers-order-kept"])
def test_a_feed_in_another_numbering(renumber):
    P = zzz.Part("poisson", 1, 12, 10, 14).renumbered("random", seed=3)
    with _env(ZZZ_RENUMBER=renumber), _fresh("sagg", P, LISTS) as cl, _fresh("sagg", P, ROWS) as cr:
        perm, kind = cr.internal_order()
        assert (kind == 1 and not np.array_equal(perm, np.arange(perm.size))) if renumber is None else kind == 0
        assert cr.mg_info()["levels"] >= 3
        _equal(_stored(cl, "sagg"), _stored(cr, "sagg"), f"renumber={renumber}: the stored hierarchy, caller's numbering")
        _equal(_applied(cl, "sagg"), _applied(cr, "sagg"), f"renumber={renumber}: cycle, transfers, solves")
        TS._check_hierarchy(cr, TS._restated(cr, P.bc_marker(), P.bs), f"rows renumber={renumber}")


@pytest.mark.parametrize("kind", ["sagg", "sagg_rbm"])
def test_partly_constrained_nodes_and_empty_rows_of_p(kind):
    P = R.case_part("elasticity_p1")
    free = np.flatnonzero((P.bc_marker().reshape(-1, 3) == 0).all(axis=1))
    nodes = free[[20, free.size // 2, free.size - 21]]
    extra = nodes * 3 + np.array([1, 0, 2])
    bc = P.bc_marker().copy()
    bc[extra] = 1
    dofs = np.flatnonzero(bc).astype(np.int32)
    with _fresh(kind, P, LISTS, dofs) as cl, _fresh(kind, P, ROWS, dofs) as cr:
        rows = np.diff(cr.mg_level_p(0)[0])
        assert np.all(rows[extra] == 0) and np.all(rows[bc == 0] > 0) and np.all(rows[bc == 1] == 0)
        for n in nodes:
            assert sorted(rows[3 * n:3 * n + 3] > 0) == [False, True, True]
        _equal(_stored(cl, kind), _stored(cr, kind), f"{kind} partly constrained: the stored hierarchy")
        _equal(_applied(cl, kind), _applied(cr, kind), f"{kind} partly constrained: cycle, transfers, solves")


def test_the_island_case_dropped_coarse_dofs_and_their_unit_diagonals():
    """aggregates whose six modes are dependent (tests/test_gpu_sagg_rbm.py's island case: dropped per level 0, 4, 4): the unit
    diagonal of a dropped coarse dof is one more candidate (d, d) of A_c and one term 1.0 x 1.0 of its row.  Rows against lists
    bit for bit, the restatement's bars with its unit-diagonal rows, the same under a budget of 4 096, and a refresh."""
    P = RR.case_part("elasticity_p1")
    bc, bc_dofs = RR.island_bc(P)
    with _fresh("sagg_rbm", P, LISTS, bc_dofs) as cl, zzz.Context(0) as cr:
        B = TR._feed(cr, P, bc_dofs)
        cr.mg_products(ROWS)
        cr.mg_setup(**TR.RBM)
        H = TR._restated(cr, bc, B)
        assert [a.shape[0] for a in H.A] == [1029, 78, 18] and H.dropped() == [0, 4, 4]
        stored = _stored(cr, "sagg_rbm")
        _equal(_stored(cl, "sagg_rbm"), stored, "island: the stored hierarchy")
        TR._check_hierarchy(cr, H, "island rows")
        for l in (1, 2):  # the dropped dofs' rows, read directly: the single entry 1 on the diagonal
            rp, cols, v = cr.mg_level_csr(l)
            d = np.flatnonzero(~H.keep[l - 1])
            assert d.size == 4 and np.all(np.diff(rp)[d] == 1) and np.all(cols[rp[d]] == d) and np.all(v[rp[d]] == 1.0)
        _equal(_applied(cl, "sagg_rbm"), _applied(cr, "sagg_rbm"), "island: cycle, transfers, solves")
        with _env(ZZZ_SAGG_ROWS_BUDGET="4096"), _fresh("sagg_rbm", P, ROWS, bc_dofs) as c4:
            assert c4.mg_products_info()["chunks"] > cr.mg_products_info()["chunks"]
            _equal(_stored(c4, "sagg_rbm"), stored, "island: budget 4096 against the default budget")
        A2 = TS._scaled(TS._matrix(cr), 7)
        for c in (cr, cl):
            c.csr_upload_values(A2.data)
            c.mg_setup(**TR.RBM)
            assert c.mg_info()["setups"] == 2
        after = _stored(cr, "sagg_rbm")
        _equal(_stored(cl, "sagg_rbm"), after, "island: the rows refresh against the lists refresh")
        with _fresh("sagg_rbm", P, ROWS, bc_dofs, setup=False) as c2:
            c2.csr_upload_values(A2.data)
            c2.mg_setup(**TR.RBM)
            _equal(_stored(c2, "sagg_rbm"), after, "island: a refresh against a fresh rows-mode set-up")
        TR._check_hierarchy(cr, TR._restated(cr, bc, B), "island rows refreshed")


def _used():
    free, total = zzz.device_memory(0)
    return total - free


@pytest.mark.parametrize("kind,name", [("sagg", "poisson_p1"), ("sagg_rbm", "elasticity_p1")])
def test_a_refresh_gives_the_bits_of_a_fresh_set_up_and_of_lists_and_allocates_nothing(kind, name):
    P = _mod(kind)._case(name)[1]
    with _fresh(kind, P, ROWS) as c, _fresh(kind, P, LISTS) as cl:
        A2 = TS._scaled(TS._matrix(c), 7)
        before = _stored(c, kind)
        assert c.mg_info()["setups"] == 1
        c.csr_upload_values(A2.data)
        used0 = _used()
        c.mg_setup(**_opts(kind))
        used1 = _used()
        assert c.mg_info()["setups"] == 2, "a refresh, not a rebuild"
        after = _stored(c, kind)
        print(f"{kind} {name}: device memory in use before the refresh {used0}, after {used1}")
        assert used1 == used0
        assert len(before) == len(after) and not all(np.array_equal(x, y) for x, y in zip(before, after)), "the values follow the matrix"
        with _fresh(kind, P, ROWS, setup=False) as c2:
            c2.csr_upload_values(A2.data)
            c2.mg_setup(**_opts(kind))
            assert c2.mg_info()["setups"] == 1
            _equal(_stored(c2, kind), after, f"{kind} {name}: a refresh against a fresh rows-mode set-up")
        cl.csr_upload_values(A2.data)
        cl.mg_setup(**_opts(kind))
        assert cl.mg_info()["setups"] == 2
        _equal(_stored(cl, kind), after, f"{kind} {name}: the rows refresh against the lists refresh")
        _equal(_applied(cl, kind), _applied(c, kind), f"{kind} {name}: refreshed, applied")


@pytest.mark.parametrize("kind,name", [("sagg", "poisson_p1"), ("sagg_rbm", "elasticity_p1")])
def test_the_term_limit_that_declines_lists_does_not_stop_rows(kind, name):
    cl, P, H = _mod(kind)._case(name)
    cl.mg_products(LISTS)
    its = cl.cg_solve(rtol=1e-8, **_opts(kind))[0]
    with _fresh(kind, P, LISTS, setup=False) as c, _env(ZZZ_SAGG_MAX_TERMS="1000"):
        with pytest.raises(zzz.ZzzError) as e:
            c.cg_solve(rtol=1e-8, **_opts(kind))
        assert e.value.code == 5 and "1000" in str(e.value) and "terms of" in str(e.value)
        c.mg_products(ROWS)
        assert c.cg_solve(rtol=1e-8, **_opts(kind))[0] == its and c.cg_info()["reason"] == 2
        assert c.mg_products_info()["mode"] == ROWS


@pytest.mark.parametrize("kind,name", [("sagg", "elasticity_p2"), ("sagg_rbm", "elasticity_p1")])
def test_switching_the_mode_rebuilds_to_the_first_build_and_leaks_nothing(kind, name):
    P = _mod(kind)._case(name)[1]
    AGG = dict(pc=zzz.PC_AGG, pc_mg_coarse_eq_limit=R.LIMIT)
    with _fresh(kind, P, LISTS, setup=False) as c:
        first = {}
        for mode in (LISTS, ROWS, LISTS, ROWS):
            c.mg_products(mode)
            c.mg_setup(**_opts(kind))
            assert c.mg_info()["setups"] == 1, "a switch rebuilds"
            got = (_stored(c, kind), _used(), c.mg_info()["coarse_bytes"], c.mg_products_info())
            assert got[3]["mode"] == mode
            if mode not in first:
                first[mode] = got
                continue
            _equal(got[0], first[mode][0], f"{kind} {name}: mode {mode} again")
            print(f"{kind} {name} mode {mode}: in use {got[1]} (first {first[mode][1]}), coarse_bytes {got[2]}, kept {got[3]['kept_bytes']}")
            assert got[1] == first[mode][1] and got[3]["kept_bytes"] == first[mode][3]["kept_bytes"]
            ms = c.mg_info()["setup_ms"]
            c.mg_products(mode)
            c.mg_setup(**_opts(kind))
            assert c.mg_info()["setups"] == 1 and c.mg_info()["setup_ms"] == ms, "the current mode's hierarchy is kept: no set-up ran"
        _equal(first[LISTS][0], first[ROWS][0], f"{kind} {name}: rows against lists")
        assert first[ROWS][2] < first[LISTS][2] and first[ROWS][3]["kept_bytes"] < first[LISTS][3]["kept_bytes"]
        # plain aggregation neither reads the mode nor rebuilds on it
        c.mg_setup(**AGG)
        agg = [c.mg_level_csr(l) for l in range(1, c.mg_info()["levels"])]
        ms = c.mg_info()["setup_ms"]
        c.mg_products(LISTS)
        c.mg_setup(**AGG)
        assert c.mg_info()["setups"] == 1 and c.mg_info()["setup_ms"] == ms, "no set-up ran: a rebuild would have timed a new one"
        for a, b in zip(agg, [c.mg_level_csr(l) for l in range(1, c.mg_info()["levels"])]):
            _equal(a, b, "agg across a mode change")


def test_refusals_leave_the_context_usable():
    P = R.case_part("poisson_p1")
    with _fresh("sagg", P, LISTS, setup=False) as c:
        itj = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)[0]
        for call, word in ((lambda: c.mg_products(2), "mode 2"), (lambda: c.mg_products(-1), "mode -1"),
                           (c.mg_products_info, "no hierarchy")):
            with pytest.raises(zzz.ZzzError) as e:
                call()
            assert e.value.code == 1 and word in str(e.value)
        c.mg_products(ROWS)
        c.mg_setup(pc=zzz.PC_AGG, pc_mg_coarse_eq_limit=R.LIMIT)
        with pytest.raises(zzz.ZzzError) as e:
            c.mg_products_info()
        assert e.value.code == 1 and "ZZZ_PC_SAGG" in str(e.value)
        assert c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)[0] == itj
        its = c.cg_solve(rtol=1e-8, **TS.SAGG)[0]
        assert its < itj and c.mg_products_info()["mode"] == ROWS
        with pytest.raises(zzz.ZzzError):
            c.mg_products(2)
        assert c.cg_solve(rtol=1e-8, **TS.SAGG)[0] == its and c.mg_info()["setups"] == 1 and c.mg_products_info()["mode"] == ROWS


def test_driver():
    exe = os.path.join(zzz.PKG, "dolfinx-scaling-test")

    def run(args):
        return subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)

    base = ["--scaling_type", "weak", "--ndofs", "20000", "-ksp_type", "cg", "-ksp_rtol", "1.0e-8", "-ksp_view"]
    for extra in (["-pc_type", "sagg"], ["-pc_type", "sagg_rbm", "--problem_type", "elasticity"]):
        ol, orr = run(base + extra), run(base + extra + ["-pc_sagg_products", "rows"])
        assert ol.returncode == 0 and orr.returncode == 0, (extra, orr.stderr[-1000:])
        its = [int(o.stdout.split("*** Number of Krylov iterations: ")[1].split()[0]) for o in (ol, orr)]
        norms = [o.stdout.split("*** Solution norm:  ")[1].split()[0] for o in (ol, orr)]
        print(f"driver {extra}: lists {its[0]} iterations, rows {its[1]}; norms {norms}")
        assert its[0] == its[1] and norms[0] == norms[1]
        assert "  products: lists, " in ol.stdout and "  products: rows, " in orr.stdout and " chunks of at most " in orr.stdout
        assert "  products: lists, " in run(base + extra + ["-pc_sagg_products", "lists"]).stdout
    assert "-pc_sagg_products" in run(["--help"]).stdout
    for bad, word in ((["-pc_type", "jacobi", "-pc_sagg_products", "rows"], "-pc_type jacobi"),
                      (["-pc_type", "sagg", "-pc_sagg_products", "heap"], "lists or rows")):
        o = run(["--ndofs", "20000"] + bad)
        assert o.returncode != 0 and "-pc_sagg_products" in o.stderr and word in o.stderr, o.stderr
