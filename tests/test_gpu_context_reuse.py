"""One context, several problems in a row: after every re-upload sequence the ABI allows, a live context must compute byte
for byte what a fresh context computes for the same final inputs (tests/_reuse.py has the states and the observation).

zzz_ctx carries several dozen caches, each with its own validity flag or version counter; a stale one gives wrong numbers
and no error.  The control (two fresh contexts agree, and meet the oracle) is the condition for everything else here."""
import itertools

import numpy as np
import pytest
import zzz
import zzz_oracle as zo

import _reuse as R

pytestmark = pytest.mark.gpu

# Observables that differ between two FRESH contexts, per state: findings of their own, taken out of the byte comparison by
# name (two at most in all).  None was found.
NOT_REPRODUCIBLE = {}


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    assert zzz.device_count() >= 1, "no GPU visible: these tests must not pass on a fallback"
    zo.set_num_threads(1)
    for k, v in R.KNOBS.items():
        monkeypatch.setenv(k, v)


_fresh = {}


def fresh(S, matrix="assembled", after_feed=None):
    """the observation of state S on a context that has seen nothing else (once per module and state name)"""
    if S.name not in _fresh:
        with zzz.Context(0) as c:
            S.feed(c) if after_feed is None else after_feed(c)
            _fresh[S.name] = R.observe(c, S, matrix)
    return _fresh[S.name]


def same(got, S, **kw):
    bad = R.differing(got, fresh(S, **kw), NOT_REPRODUCIBLE.get(S.name, ()))
    assert not bad, f"{S.name}: differs from a fresh context in {bad}"


# ---- 1. control ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.NAMES)
def test_two_fresh_contexts_agree_and_meet_the_oracle(name):
    S = R.state(name)
    first = fresh(S)
    with zzz.Context(0) as c:
        S.feed(c)
        second = R.observe(c, S)
        if name == "U1r":
            assert first["kind"] & 3 == 1 and c.cells_renumbered()
    bad = R.differing(second, first)
    assert sorted(bad) == sorted(NOT_REPRODUCIBLE.get(name, ())), f"{name}: two fresh contexts differ in {bad}"
    P = S.P
    bc = S.bc_marker()
    orp, ocl = zo.pattern(P.n_owned, P.cell_dofs, P.bs)
    np.testing.assert_array_equal(first["rowptr"], orp)
    np.testing.assert_array_equal(first["cols"], ocl)
    ov = zo.assemble_matrix(P.form, P.order, P.x, P.cells, P.cell_dofs, bc, orp, ocl)
    ob = zo.assemble_vector(P.form, P.order, P.x, P.cells, P.cell_dofs, P.f, P.g, P.facets if P.bs == 1 else None, bc)
    assert np.abs(first["vals"] - ov).max() <= 1e-12 * np.abs(ov).max()
    assert np.abs(first["b"] - ob).max() <= 1e-12 * np.abs(ob).max()
    assert first["b.again"].tobytes() == first["b"].tobytes()


# ---- 2. full re-feed: every ordered pair (none dropped) ------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [pytest.param(a, b, id=f"{a}-then-{b}") for a, b in itertools.permutations(R.NAMES, 2)])
def test_full_refeed(a, b):
    A, B = R.state(a), R.state(b)
    with zzz.Context(0) as c:
        A.feed(c)
        same(R.observe(c, A), A)
        B.feed(c)
        same(R.observe(c, B), B)


# ---- 3. partial re-uploads -----------------------------------------------------------------------------------------------
def _p2_random():
    return R.State("P2r-5x4x6", "uploaded", zzz.Part("poisson", 2, 5, 4, 6).renumbered("random"))


def test_second_dofmap_on_the_same_mesh_p1_then_p2():
    """renumber_cells permutes cell_verts in place: the second dofmap must meet the mesh in the caller's cell order again"""
    S2 = _p2_random()
    S1 = R.p1_on_mesh_of(S2, "P1-on-mesh-of-P2r")
    with zzz.Context(0) as c:
        S1.feed(c)
        got = R.observe(c, S1)
        assert got["kind"] & 3 == 1 and got["cells_renumbered"] == 1  # (else the sequence tests nothing)
        same(got, S1)
        c.matfree_setup()
        S2.feed_behind_mesh(c)
        c.matfree_setup()
        same(R.observe(c, S2), S2)


def test_the_same_dofmap_twice():
    S = R.state("U1r")
    with zzz.Context(0) as c:
        S.feed(c)
        same(R.observe(c, S), S)
        c.matfree_setup()
        S.feed_behind_mesh(c)
        c.matfree_setup()
        same(R.observe(c, S), S)


def test_second_dofmap_block_size_1_then_3():
    S3 = R.state("E1r")
    S1 = R.scalar_on_dofmap_of(S3, "scalar-on-E1r")
    with zzz.Context(0) as c:
        S1.feed(c)
        same(R.observe(c, S1), S1)
        c.matfree_setup()
        S3.feed_behind_mesh(c)
        c.matfree_setup()
        same(R.observe(c, S3), S3)


def test_dofmaps_behind_a_generated_mesh():
    """zzz_cube_generate keeps no host copy of cell_verts: a dofmap uploaded behind it, at block size 1 and then 3"""
    G = R.state("GE1")
    U3 = R.State("GE1-mesh-dofmap-bs3", "uploaded", G.P)
    U1 = R.scalar_on_dofmap_of(U3, "GE1-mesh-dofmap-bs1")

    def behind_generated(S):
        def feed(c):
            G.feed(c)
            S.feed_behind_mesh(c)
        return feed

    with zzz.Context(0) as c:
        G.feed(c)
        same(R.observe(c, G), G)
        c.matfree_setup()
        U1.feed_behind_mesh(c)
        c.matfree_setup()
        same(R.observe(c, U1), U1, after_feed=behind_generated(U1))
        U3.feed_behind_mesh(c)
        c.matfree_setup()
        same(R.observe(c, U3), U3, after_feed=behind_generated(U3))


def _partial(name, change, upload):
    """observed state `name`, then ONE upload and the assemblies on the KEPT pattern (no zzz_csr_pattern_build, which would
    drop by itself what the upload has to invalidate); the fresh context is given the changed state from the start"""
    S = R.state(name)
    T = change(S)
    with zzz.Context(0) as c:
        S.feed(c)
        same(R.observe(c, S), S)
        c.matfree_setup()
        upload(c, T)
        c.matfree_setup()
        same(R.observe(c, T, matrix="reassembled"), T)
        same(R.observe(c, T), T)  # ... and with a pattern build in between


@pytest.mark.parametrize("name", ["U1r", "E1r"])
def test_another_dirichlet_set_alone(name):
    """lifting rows, the matrix-free plan's markers, the agg hierarchy and the Jacobi codes all hang on the Dirichlet set"""
    def change(S):
        free = np.setdiff1d(np.arange(S.n, dtype=np.int32), S.P.bc_dofs)
        return S.but(name + "-other-bc", bc_dofs=np.sort(np.concatenate([S.P.bc_dofs[::2], free[5::7]])).astype(np.int32))

    _partial(name, change, lambda c, T: c.upload_bc(T.P.bc_dofs))


def test_other_facets_alone():
    """U1r's cells are kept in an internal order: the mask is translated at the boundary"""
    _partial("U1r", lambda S: S.but("U1r-other-facets", facets=np.ascontiguousarray(S.P.facets[::2])),
             lambda c, T: c.upload_facets(T.P.facets))


@pytest.mark.parametrize("name", ["U1r", "E1r"])
def test_other_coefficients_alone(name):
    def change(S):
        return S.but(name + "-other-coeff", f=2.0 * S.P.f + 1.0, g=None if S.P.g is None else np.cos(3.0 * S.P.g))

    def upload(c, T):
        c.upload_coeff(zzz.COEFF_F, T.P.f)
        if T.P.g is not None:
            c.upload_coeff(zzz.COEFF_G, T.P.g)

    _partial(name, change, upload)


@pytest.mark.parametrize("name", ["U1r", "E1r"])
def test_uploaded_values_and_the_assembly_after_them(name):
    """zzz_csr_upload_values of D A D (a fixed diagonal D): the product's forms, the Jacobi codes, the Chebyshev bound and the
    agg hierarchy's values follow; the next assembly brings the first observation back"""
    S = R.state(name)
    T = S.but(name + "-DAD")
    first = fresh(S)
    d = 0.5 + np.random.default_rng(9).random(S.n)
    rp, cl = first["rowptr"], first["cols"]
    scaled = d[np.repeat(np.arange(S.n), np.diff(rp))] * first["vals"] * d[cl]

    def fed_and_scaled(c):
        S.feed(c)
        c.pattern_build()
        c.assemble_matrix(S.form)
        c.csr_upload_values(scaled)

    with zzz.Context(0) as c:
        S.feed(c)
        same(R.observe(c, S), S)
        c.matfree_setup()
        c.csr_upload_values(scaled)
        c.matfree_setup()
        got = R.observe(c, T, matrix="kept")
        assert got["vals"].tobytes() == scaled.tobytes()
        same(got, T, matrix="kept", after_feed=fed_and_scaled)
        same(R.observe(c, S, matrix="reassembled"), S)  # zzz_assemble_matrix alone, on the kept pattern


@pytest.mark.parametrize("name", ["U1r", "G2", "E1r", "U3"])
def test_pattern_build_a_second_time(name):
    """zzz_csr_pattern_build forgets the whole pattern tier and the values behind it: also the block-row form's split (E1r) and
    the block-window form's structure (U3), which the first build's assembly has left"""
    S = R.state(name)
    with zzz.Context(0) as c:
        S.feed(c)
        c.matfree_setup()
        same(R.observe(c, S), S)
        c.pattern_build()
        c.matfree_setup()
        same(R.observe(c, S, matrix="reassembled"), S)  # (the second build is the one above)
        same(R.observe(c, S), S)                        # a third


# With KNOBS alone the stream's values stay doubles at these sizes: no value dictionary, no packed palettes, and what is never
# built cannot be stale.  ZZZ_SELLP_DICT=2 on top builds them for the P1 states (P2 / P3 and block size 3 run on the special
# forms, which have their own tables).  The stream's x windows and per-slice dictionaries are not reached by any state here.
DICT_STATES = ["U1", "U1r", "U1big", "J", "G1"]


def _with_dictionary(monkeypatch, name):
    for k, v in R.DICT_KNOB.items():
        monkeypatch.setenv(k, v)
    S = R.state(name)
    return S.but(name + "+dictionary")


@pytest.mark.parametrize("a,b", [pytest.param(a, b, id=f"{a}-then-{b}") for a, b in itertools.permutations(DICT_STATES, 2)])
def test_full_refeed_with_the_value_dictionary(monkeypatch, a, b):
    A, B = _with_dictionary(monkeypatch, a), _with_dictionary(monkeypatch, b)
    with zzz.Context(0) as c:
        A.feed(c)
        same(R.observe(c, A), A)
        B.feed(c)
        same(R.observe(c, B), B)


@pytest.mark.parametrize("name", ["U1r", "J"])
def test_the_value_dictionary_follows_the_values(monkeypatch, name):
    """D A D uploaded (every value distinct: another dictionary, other palettes), then the assembly on the kept pattern"""
    S = _with_dictionary(monkeypatch, name)
    T = S.but(S.name + "-DAD")
    first = fresh(S)
    d = 0.5 + np.random.default_rng(9).random(S.n)
    scaled = d[np.repeat(np.arange(S.n), np.diff(first["rowptr"]))] * first["vals"] * d[first["cols"]]

    def fed_and_scaled(c):
        S.feed(c)
        c.pattern_build()
        c.assemble_matrix(S.form)
        c.csr_upload_values(scaled)

    with zzz.Context(0) as c:
        S.feed(c)
        same(R.observe(c, S), S)
        c.csr_upload_values(scaled)
        got = R.observe(c, T, matrix="kept")
        assert got["spmv_values_info"][0] != 0 and got["spmv_values_info"][1] > 1  # read through a dictionary ...
        if name == "U1r":  # ... of more distinct values than the lattice's assembled matrix has
            assert got["spmv_values_info"][1] > first["spmv_values_info"][1]
        same(got, T, matrix="kept", after_feed=fed_and_scaled)
        same(R.observe(c, S, matrix="reassembled"), S)


@pytest.mark.parametrize("then", ["U1r", "U1big"], ids=["same-cell-count", "another-cell-count"])
def test_a_new_mesh_forgets_the_dofmap(then):
    """zzz_mesh_upload on a live context: until the next zzz_dofmap_upload everything that needs a dofmap is refused on the
    host (with another cell count the old cell_dofs would be walked past its end: nothing may be launched)"""
    S, T = R.state("U1r"), R.state(then)
    with zzz.Context(0) as c:
        S.feed(c)
        same(R.observe(c, S), S)
        c.upload_mesh(T.P.x, T.P.cells)
        for call in (c.pattern_build, lambda: c.action(np.ones(S.n)), c.matfree_setup, lambda: c.assemble_vector(S.form),
                     lambda: c.cg_solve(pc=zzz.PC_JACOBI), lambda: c.cg_solve(pc=zzz.PC_NONE, op=zzz.OP_MATFREE),
                     lambda: c.upload_bc(S.P.bc_dofs), lambda: c.matfree_assemble_vector(S.form), c.matfree_diagonal,
                     lambda: c.action_f32(np.ones(S.n, np.float32)), lambda: c.assemble_matrix(S.form), c.internal_order,
                     # (the agg hierarchy of the observation above belongs to the problem that is gone)
                     c.mg_info, lambda: c.mg_apply(np.ones(S.n)), lambda: c.mg_level_csr(1), lambda: c.mg_transfer(0, 1, np.ones(S.n))):
            with pytest.raises(zzz.ZzzError) as e:
                call()
            assert e.value.code == 1, str(e.value)
        T.feed(c)
        same(R.observe(c, T), T)


def test_a_generated_cube_forgets_the_hierarchy():
    """zzz_cube_generate replaces the mesh as zzz_mesh_upload does: the agg hierarchy of the problem before it is declined, as
    on a fresh context, until a set-up builds this problem's"""
    S, T = R.state("U1r"), R.state("G1")
    with zzz.Context(0) as c:
        S.feed(c)
        same(R.observe(c, S), S)
        T.feed(c)
        for call in (c.mg_info, lambda: c.mg_apply(np.ones(T.n)), lambda: c.mg_level_csr(1), lambda: c.mg_transfer(0, 1, np.ones(T.n))):
            with pytest.raises(zzz.ZzzError) as e:
                call()
            assert e.value.code == 1, str(e.value)
        same(R.observe(c, T), T)


# ---- 4. refusals change nothing ------------------------------------------------------------------------------------------
def _order_4(c, S):
    c.upload_dofmap(4, S.bs, S.P.cell_dofs, S.P.n_owned)


def _block_size_2(c, S):
    c.upload_dofmap(S.order, 2, S.P.cell_dofs, S.P.n_owned)


def _bad_facet(c, S):
    c.upload_facets(np.array([[0, 1], [S.P.cells.shape[0], 0]], np.int32))


def _bad_mesh(c, S):
    cells = S.P.cells.copy()
    cells[-1, 3] = S.P.x.shape[0]
    c.upload_mesh(S.P.x, cells)


def _bad_coefficient(c, S):
    c.upload_coeff(2, S.P.f)


def _unknown_form(c, S):
    for call in (c.assemble_matrix, c.assemble_vector, c.matfree_assemble_vector):
        with pytest.raises(zzz.ZzzError):
            call(7)
    c.assemble_matrix(7)


def _form_of_the_other_block_size(c, S):
    c.assemble_matrix(zzz.FORM_ELASTICITY if S.bs == 1 else zzz.FORM_POISSON)


def _mg_on_an_uploaded_feed(c, S):
    c.cg_solve(pc=zzz.PC_MG)


def _float_solve_at_block_size_3(c, S):
    c.cg_solve_f32()


REFUSED = [("U1r", _order_4), ("E1r", _order_4), ("U1r", _block_size_2), ("E1r", _block_size_2), ("U1r", _bad_facet), ("E1r", _bad_facet),
           ("U1r", _bad_coefficient), ("E1r", _bad_coefficient), ("U1r", _unknown_form), ("E1r", _unknown_form),
           ("U1r", _form_of_the_other_block_size), ("E1r", _form_of_the_other_block_size),
           ("U1r", _mg_on_an_uploaded_feed), ("E1r", _mg_on_an_uploaded_feed), ("E1r", _float_solve_at_block_size_3),
           # a generated cube stays one (ZZZ_PC_MG keeps serving it) after an upload that was refused
           ("U1r", _bad_mesh), ("G1", _bad_mesh), ("G1", _order_4), ("G1", _bad_facet)]


@pytest.mark.parametrize("name,call", [pytest.param(n, f, id=f"{n}-{f.__name__.strip('_')}") for n, f in REFUSED])
def test_a_refused_call_changes_nothing(name, call):
    S = R.state(name)
    with zzz.Context(0) as c:
        S.feed(c)
        same(R.observe(c, S), S)
        with pytest.raises(zzz.ZzzError) as e:
            call(c, S)
        assert e.value.code == 1, str(e.value)
        same(R.observe(c, S), S)


@pytest.mark.parametrize("name", ["U1r", "E1r", "G1"])
def test_a_refused_dirichlet_set_clears_the_values_and_nothing_else(name):
    """the one documented side effect of a refusal (zzz_bc_upload in include/zzz_abi.h): u0 == 0 again"""
    S = R.state(name)
    want = fresh(S)
    u0 = R.vectors(S.n)[1]
    with zzz.Context(0) as c:
        S.feed(c)
        same(R.observe(c, S), S)
        c.upload_bc_values(u0)
        c.assemble_vector(S.form)
        assert c.vec_download(zzz.VEC_B).tobytes() == want["b.lifted"].tobytes()
        with pytest.raises(zzz.ZzzError) as e:
            c.upload_bc(np.array([0, S.n], np.int32))
        assert e.value.code == 1 and "out of range" in str(e.value)
        c.assemble_vector(S.form)
        assert c.vec_download(zzz.VEC_B).tobytes() == want["b"].tobytes()  # the values are gone, the Dirichlet set is not
        same(R.observe(c, S), S)
