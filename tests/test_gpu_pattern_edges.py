"""The pattern build (zzz_csr_pattern_build: csrc/zzz_pattern.hip, build_adjT in csrc/zzz_assemble.hip) at every capacity
edge and fallback: the connectivities of tests/_pattern_sets.py, whose counts tests/test_pattern_sets.py proves on the CPU,
each ON a limit or one unit past it.  With ZZZ_RENUMBER=0 the feed reaches the build as built, and for every case

  * zzz_pattern_info reports the path the case's counts predict (adjacency sort-free / sorted / sorted after an overflow,
    the runs, the P1 row kernel, the builder, the longest block row, where adj_li came from, have_asm_pos);
  * rowptr and cols are the oracle's, exactly; a second build on the same context gives the same arrays (and after a window
    overflow reports "sorted from the start": the dofmap remembers); A and b to 1e-12 of the oracle's largest entry;
  * the product is zo.spmv's bit for bit (zo.spmv_chunked at spmv_lanes_per_row()); Jacobi-CG within 2 iterations and 1e-6
    of zo.pcg; on the scalar fans the matrix-free action to 1e-12 of zo.action_poisson's largest entry (from 255 cells
    around one dof the cell-block plan refuses the mesh and the two-pass form, which needs adj_li, serves it);
  * P2 / P3: ZZZ_ASM_SEARCH=1 gives the same bits as the positions do;
  * ZZZ_PATTERN=host gives the device build's arrays and values bit for bit; with ZZZ_RENUMBER unset the results hold.

The two parts with ghost dofs are one rank's share of a matrix: pattern, A and b are checked, products and solves need the
other rank (tests/test_gpu_partitions.py).

pos_missed (row_unique_regs / k_row_pattern), which withdraws have_asm_pos, has two causes.  A row of 513 .. 1024 candidates
is reached by small inputs: p2_cand_520, p2_cand_1020, p3_cand_520, p3_cand_1020 (52 / 26 cells around one dof) report
have_asm_pos = 0 and their assembly searches.  A row whose columns lie 2^23 or more apart needs a part of more than 8.3 M
local dofs (columns are local indices below n_owned + n_ghost): no small input reaches it, and none is here.

The bar for A and b.  Fans and repeated cells are unlike the meshes the 1e-12 bar was set on, so the oracle's own A and b
were first measured on the CPU against the 50-digit reference (tests/_hp_ref.py; max |oracle - reference| over the largest
|reference|, Dirichlet rows as the library leaves them); every figure is below 1e-13, so the bar stays 1e-12.  Largest
figures per family, oracle against the reference | this library against the oracle on an MI355X:

  family                                  oracle A   oracle b | library A  library b
  scalar fans, k = 13 .. 958              9.0e-16    6.7e-16  | 2.5e-16    1.8e-15
  elasticity fans, k = 13 .. 339          6.0e-16    3.4e-16  | 1.2e-16    3.6e-16
  P2 repeats on the unit cube, 6 .. 103   1.2e-15    1.2e-15  | 2.7e-15    4.6e-16
  P3 repeats (one tet, the unit cube)     5.7e-16    5.3e-16  | 9.1e-16    5.3e-16
  P1 lattice + repeats (block, window)    5.3e-16    5.6e-16  | 1.3e-16    6.2e-16
  P2 lattice + repeats (window)           1.0e-15    8.2e-16  | 1.0e-15    4.1e-16

The matrix-free action on the scalar fans: at most 8.6e-16 of zo.action_poisson's largest entry.
"""
import contextlib
import functools

from _gpu_helpers import *  # noqa: F401,F403 -- np / os / pytest / zzz / zo
import _pattern_sets as ps

pytestmark = pytest.mark.gpu  # noqa: F405

FIELDS = ("adjacency", "runs", "row_kernel", "builder", "max_cols", "adj_source", "have_asm_pos")
REFUSAL = "matrix rows too long for the kernel tiles"


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _upload(ctx, c):
    ctx.upload_mesh(c.x, c.cells)
    ctx.upload_dofmap(c.order, c.bs, c.cell_dofs, c.n_owned, c.n_ghost)
    ctx.upload_bc(c.bc_dofs)
    if c.bs == 1:
        ctx.upload_facets(c.facets)
        ctx.upload_coeff(zzz.COEFF_G, c.g)
    ctx.upload_coeff(zzz.COEFF_F, c.f)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(rowptr, cols, A, b) of the oracle, once per case and left alone"""
    zo.set_num_threads(1)
    c = ps.case(name)
    rp, cl = zo.pattern(c.n_owned, c.cell_dofs, c.bs)
    bc = c.bc_marker()
    v = zo.assemble_matrix(c.form, c.order, c.x, c.cells, c.cell_dofs, bc, rp, cl)
    b = zo.assemble_vector(c.form, c.order, c.x, c.cells, c.cell_dofs, c.f, c.g, c.facets if c.bs == 1 else None, bc)
    for a in (rp, cl, v, b):
        a.setflags(write=False)
    return rp, cl, v, b[: c.n_owned * c.bs]


@functools.lru_cache(maxsize=None)
def _oracle_solve(name):
    rp, cl, v, b = _oracle(name)
    it, u, _, _ = zo.pcg(rp, cl, v, np.array(b), rtol=1e-8)
    return it, u


def _build_and_assemble(ctx, c):
    ctx.pattern_build()
    ctx.assemble_matrix(c.form)
    ctx.assemble_vector(c.form)
    rp, cl, v = ctx.csr_download()
    return rp, cl, v, ctx.vec_download(zzz.VEC_B)


@functools.lru_cache(maxsize=None)
def _device(name):
    """what the device build leaves with the feed as built (ZZZ_RENUMBER=0), on a fresh context; None when it refuses"""
    c = ps.case(name)
    with _env(ZZZ_RENUMBER="0", ZZZ_PATTERN=None, ZZZ_ASM_SEARCH=None), zzz.Context(0) as ctx:
        _upload(ctx, c)
        try:
            return _build_and_assemble(ctx, c)
        except zzz.ZzzError as e:
            assert e.code == 5 and REFUSAL in str(e)
            return None


def _check_values(name, v, b, what=""):
    orp, ocl, ov, ob = _oracle(name)
    ea, eb = np.abs(v - ov).max() / np.abs(ov).max(), np.abs(b - ob).max() / np.abs(ob).max()
    print(f"{name}{what}: |A - oracle| / max|A| = {ea:.2e}   |b - oracle| / max|b| = {eb:.2e}")
    assert ea <= 1e-12, name
    assert eb <= 1e-12, name


def _check_lattice_444(ctx):
    P = zzz.Part("poisson", 1, 4, 4, 4)
    ctx.upload_part(P)
    ctx.pattern_build()
    ctx.assemble_matrix(P.form)
    ctx.assemble_vector(P.form)
    rp, cl, v = ctx.csr_download()
    orp, ocl = zo.pattern(P.n_owned, P.cell_dofs, 1)
    np.testing.assert_array_equal(rp, orp)
    np.testing.assert_array_equal(cl, ocl)
    ov = zo.assemble_matrix(0, 1, P.x, P.cells, P.cell_dofs, P.bc_marker(), orp, ocl)
    ob = zo.assemble_vector(0, 1, P.x, P.cells, P.cell_dofs, P.f, P.g, P.facets, P.bc_marker())
    assert np.abs(v - ov).max() <= 1e-12 * np.abs(ov).max()
    assert np.abs(ctx.vec_download(zzz.VEC_B) - ob).max() <= 1e-12 * np.abs(ob).max()
    assert ctx.pattern_info()["adjacency"] == 1


@pytest.mark.parametrize("name", ps.NAMES)
def test_path_and_results(name):
    c = ps.case(name)
    want = c.path
    with _env(ZZZ_RENUMBER="0", ZZZ_PATTERN=None, ZZZ_ASM_SEARCH=None), zzz.Context(0) as ctx:
        with pytest.raises(zzz.ZzzError) as e:
            ctx.pattern_info()  # no pattern yet
        assert e.value.code == 1
        _upload(ctx, c)
        assert ctx.internal_order()[1] == 0
        if want["refused"]:
            # one column past what the kernel tiles hold: an error, not a crash, and the context goes on
            for _ in range(2):
                with pytest.raises(zzz.ZzzError) as e:
                    ctx.pattern_build()
                assert e.value.code == 5 and REFUSAL in str(e.value)
                with pytest.raises(zzz.ZzzError) as e:
                    ctx.pattern_info()
                assert e.value.code == 1
            _check_lattice_444(ctx)
            return
        orp, ocl, ov, ob = _oracle(name)
        rp, cl, v, b = _build_and_assemble(ctx, c)
        info = ctx.pattern_info()
        print(name, info)
        assert {k: info[k] for k in FIELDS} == {k: want[k] for k in FIELDS}
        np.testing.assert_array_equal(rp, orp)
        np.testing.assert_array_equal(cl, ocl)
        _check_values(name, v, b)
        # the second build on the same context: the same arrays, and an overflow is remembered
        rp2, cl2, v2, b2 = _build_and_assemble(ctx, c)
        info2 = ctx.pattern_info()
        assert info2["adjacency"] == want["adjacency_again"]
        assert {k: info2[k] for k in FIELDS[2:]} == {k: want[k] for k in FIELDS[2:]}
        for x, y in ((rp, rp2), (cl, cl2), (v, v2), (b, b2)):
            np.testing.assert_array_equal(x, y)
        if c.n_ghost:
            return
        xv = np.random.default_rng(len(name)).standard_normal(c.n_owned * c.bs)
        lanes = ctx.spmv_lanes_per_row()
        want_y = zo.spmv(orp, ocl, v, xv) if lanes == 1 else zo.spmv_chunked(orp, ocl, v, xv, lanes)
        np.testing.assert_array_equal(ctx.spmv(xv), want_y)
        it, rn, r0 = ctx.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
        oit, ou = _oracle_solve(name)
        u = ctx.vec_download(zzz.VEC_U)
        print(f"{name}: iterations {it} (oracle {oit}), |u - oracle| / |oracle| = {np.linalg.norm(u - ou) / np.linalg.norm(ou):.2e}")
        assert abs(it - oit) <= 2
        assert np.linalg.norm(u - ou) <= 1e-6 * np.linalg.norm(ou)
        if name.startswith("fan_"):
            oy = zo.action_poisson(1, c.x, c.cells, c.cell_dofs, c.bc_marker(), xv)
            ya = ctx.action(xv)
            print(f"{name}: |action - oracle| / max|oracle| = {np.abs(ya - oy).max() / np.abs(oy).max():.2e}")
            assert np.abs(ya - oy).max() <= 1e-12 * np.abs(oy).max()


@pytest.mark.parametrize("name", [n for n in ps.NAMES if ps.case(n).order > 1])
def test_search_gives_the_bits_of_the_positions(name):
    c = ps.case(name)
    dev = _device(name)
    with _env(ZZZ_RENUMBER="0", ZZZ_PATTERN=None, ZZZ_ASM_SEARCH="1"), zzz.Context(0) as ctx:
        _upload(ctx, c)
        got = _build_and_assemble(ctx, c)
        assert ctx.pattern_info()["have_asm_pos"] == 0
    for x, y in zip(dev, got):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", ps.NAMES)
def test_host_builder_gives_the_device_arrays(name):
    c = ps.case(name)
    dev = _device(name)
    with _env(ZZZ_RENUMBER="0", ZZZ_PATTERN="host", ZZZ_ASM_SEARCH=None), zzz.Context(0) as ctx:
        _upload(ctx, c)
        if c.path["refused"]:
            assert dev is None
            with pytest.raises(zzz.ZzzError) as e:
                ctx.pattern_build()
            assert e.value.code == 5 and REFUSAL in str(e.value)
            return
        got = _build_and_assemble(ctx, c)
        info = ctx.pattern_info()
    assert (info["builder"], info["adjacency"], info["row_kernel"], info["adj_source"], info["have_asm_pos"]) == (2, 0, -1, 0, 0)
    assert info["max_cols"] == c.path["max_cols"]
    for x, y in zip(dev, got):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", ps.NAMES)
def test_results_in_the_library_own_order(name):
    """ZZZ_RENUMBER unset: the library may put dofs and cells into its own order first; whatever path the build then takes,
    the ABI shows the oracle's pattern in the caller's numbering, A, b and the solve"""
    c = ps.case(name)
    with _env(ZZZ_RENUMBER=None, ZZZ_PATTERN=None, ZZZ_ASM_SEARCH=None), zzz.Context(0) as ctx:
        _upload(ctx, c)
        if c.path["refused"]:
            with pytest.raises(zzz.ZzzError) as e:
                ctx.pattern_build()
            assert e.value.code == 5 and REFUSAL in str(e.value)
            return
        orp, ocl, ov, ob = _oracle(name)
        rp, cl, v, b = _build_and_assemble(ctx, c)
        np.testing.assert_array_equal(rp, orp)
        np.testing.assert_array_equal(cl, ocl)
        _check_values(name, v, b, " (own order)")
        assert ctx.pattern_info()["max_cols"] == c.path["max_cols"]
        if c.n_ghost:
            return
        it, rn, r0 = ctx.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
        oit, ou = _oracle_solve(name)
        assert abs(it - oit) <= 2
        assert np.linalg.norm(ctx.vec_download(zzz.VEC_U) - ou) <= 1e-6 * np.linalg.norm(ou)


def test_nothing_leaks_from_one_build_to_the_next():
    """one context: a window overflow, a plain lattice, more than 512 runs, the plain lattice again, a refusal by the device
    (host builder), the plain lattice a third time.  The lattice takes the sort-free path every time and leaves what a fresh
    context leaves, byte for byte"""
    plain = "lattice_512"
    fresh = _device(plain)
    with _env(ZZZ_RENUMBER="0", ZZZ_PATTERN=None, ZZZ_ASM_SEARCH=None), zzz.Context(0) as ctx:
        for name, adjacency in (("window_7169", 3), (plain, 1), ("p1_blocks_129", 2), (plain, 1), ("p2_cand_1030", 0), (plain, 1)):
            c = ps.case(name)
            _upload(ctx, c)
            got = _build_and_assemble(ctx, c)
            info = ctx.pattern_info()
            assert info["adjacency"] == adjacency, (name, info)
            assert {k: info[k] for k in FIELDS} == {k: c.path[k] for k in FIELDS}, name
            for x, y in zip(_device(name), got):
                np.testing.assert_array_equal(x, y, err_msg=name)
            if name == plain:
                for x, y in zip(fresh, got):
                    np.testing.assert_array_equal(x, y)
