"""GPU parity tests, part 7: inhomogeneous Dirichlet values (zzz_bc_values_upload) -- the lifting pass behind the vector
kernels (apply_lifting with scale 1 and x0 empty, then bc->set(b): src/poisson_problem.cpp:152-155,
src/elasticity_problem.cpp:226-229), the matrix-free solve with values, call order, clearing, the driver's --bc_value.

The reference needs no oracle change: with an all-zero marker the oracle assembles the UNCONSTRAINED A and L, and
    b_ref = b_unc - A_unc[:, bc] g[bc],   b_ref[bc] = g[bc]
is DOLFINx's vector.  Bars: 1e-12 of the maximum for assembled values against the oracle, 1e-13 between two feeds of the
same problem, 1e-9 for solutions against a closed form or another partition (tests/test_gpu_assembly.py,
tests/test_gpu_partitions.py)."""
import functools

from _gpu_helpers import *  # noqa: F401,F403 -- helpers, fixtures (ctx), np / os / zzz / zo

pytestmark = pytest.mark.gpu  # noqa: F405

# the smallest cubes that reach every entity type (vertex, edge, face, interior dofs) and both constrained faces
CASES6 = [("poisson", 1, (4, 3, 5)), ("poisson", 2, (3, 2, 3)), ("poisson", 3, (2, 3, 2)),
          ("elasticity", 1, (4, 3, 5)), ("elasticity", 2, (3, 2, 3)), ("elasticity", 3, (2, 3, 2))]
RIGID_A, RIGID_W = np.array([0.3, -0.2, 0.1]), np.array([0.05, -0.07, 0.11])


@functools.lru_cache(maxsize=None)
def _part(problem, order, dims):
    return zzz.Part(problem, order, *dims)


@functools.lru_cache(maxsize=None)
def _unconstrained(problem, order, dims):
    """(rowptr, cols, A_unc, b_unc) of the oracle with nothing constrained, computed once per case"""
    zo.set_num_threads(1)
    P = _part(problem, order, dims)
    none = np.zeros(P.nloc * P.bs, np.uint8)
    rp, cl = zo.pattern(P.n_owned, P.cell_dofs, P.bs)
    A = zo.assemble_matrix(P.form, order, P.x, P.cells, P.cell_dofs, none, rp, cl)
    b = zo.assemble_vector(P.form, order, P.x, P.cells, P.cell_dofs, P.f, P.g, P.facets if P.form == 0 else None, none)
    for a in (rp, cl, A, b):
        a.setflags(write=False)
    return rp, cl, A, b


def _lifted_reference(problem, order, dims, g):
    P = _part(problem, order, dims)
    rp, cl, A, b_unc = _unconstrained(problem, order, dims)
    bc = P.bc_marker().astype(bool)
    gm = np.where(bc, g, 0.0)  # (g may hold NaN off the Dirichlet set: never multiplied)
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    b = b_unc - np.bincount(rows, weights=A * gm[cl], minlength=rp.size - 1)
    b[bc] = g[bc]
    return b


def _noise_values(P, seed):
    """seeded noise at every dof, NaN at a handful of unconstrained entries (they must never be read)"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(P.nloc * P.bs)
    free = np.nonzero(P.bc_marker() == 0)[0]
    g[rng.choice(free, size=min(7, free.size), replace=False)] = np.nan
    return g


def _closed_form(P, spoke=False):
    """the global function of the patch tests at P's dofs: Poisson 1 + 2 x (spoke mesh: 1 + 2 x + 3 y - z), elasticity the
    rigid motion a + w x X"""
    X = P.dof_x
    if P.bs == 1:
        return 1.0 + 2.0 * X[:, 0] + ((3.0 * X[:, 1] - X[:, 2]) if spoke else 0.0)
    return (RIGID_A + np.cross(RIGID_W, X)).reshape(-1)


def _feed(c, P, feed):
    if feed == "cube_generate":
        c.cube_generate(P.problem, P.order, *P.dims, P.nparts, P.part)
    else:
        c.upload_part(P)
        if P.nparts > 1:
            c.upload_halo(P)


@pytest.mark.parametrize("feed", ["upload_part", "cube_generate"])
@pytest.mark.parametrize("problem,order,dims", CASES6)
def test_lifted_vector_matches_the_unconstrained_oracle(problem, order, dims, feed):
    """1. Right-hand side parity with the reference's own coefficients f, g and noise for u0: b within 1e-12 of the
    maximum, b[bc] == g[bc] exactly, NaN at unconstrained entries of the upload reaches nothing, and a second assembly
    gives the same bits."""
    P = _part(problem, order, dims)
    g = _noise_values(P, 11 * order + P.bs)
    b_ref = _lifted_reference(problem, order, dims, g)
    bc = P.bc_marker().astype(bool)
    with zzz.Context(0) as c:
        _feed(c, P, feed)
        c.upload_bc_values(g)
        c.pattern_build()
        c.assemble_vector(P.form)
        b = c.vec_download(zzz.VEC_B)
        c.assemble_vector(P.form)
        b2 = c.vec_download(zzz.VEC_B)
    err = np.abs(b - b_ref).max() / np.abs(b_ref).max()
    print(f"{problem} P{order} {dims} {feed}: |b - b_ref| / |b_ref| = {err:.3e}")
    assert np.isfinite(b).all()
    assert err <= 1e-12
    assert np.array_equal(b[bc], g[bc])
    assert np.array_equal(b, b2)
    # the lifting did something: the u0 == 0 vector is another one
    b0 = np.where(bc, 0.0, _unconstrained(problem, order, dims)[3])
    assert np.abs(b - b0).max() > 1e-3 * np.abs(b_ref).max()


def _patch_solve(c, P, g, **kw):
    c.upload_coeff(zzz.COEFF_F, np.zeros(P.nloc * P.bs))
    if P.g is not None:
        c.upload_coeff(zzz.COEFF_G, np.zeros(P.nloc))
    c.upload_bc_values(g)
    c.pattern_build()
    if kw.get("op", zzz.OP_CSR) == zzz.OP_CSR:
        c.assemble_matrix(P.form)
    c.assemble_vector(P.form)
    it, rn, r0 = c.cg_solve(**kw)
    return it, c.vec_download(zzz.VEC_U)


@pytest.mark.parametrize("feed", ["upload_part", "cube_generate"])
@pytest.mark.parametrize("problem,order,dims", CASES6)
def test_patch_solutions_on_the_cube(problem, order, dims, feed):
    """2. Mathematics, not restatement: with the reference's Dirichlet sets and zero coefficients, u = 1 + 2 x (in every
    Pk space, zero flux on the free faces y, z in {0, 1}) solves Poisson, and the rigid motion a + w x X (zero stress:
    every face but y = 0 is traction-free) solves elasticity.  A missing cell or a sign slip shows at 1e-2."""
    P = _part(problem, order, dims)
    ue = _closed_form(P)
    bc = P.bc_marker().astype(bool)[:P.n_owned * P.bs]
    with zzz.Context(0) as c:
        _feed(c, P, feed)
        it, u = _patch_solve(c, P, ue, pc=zzz.PC_JACOBI, rtol=1e-12)
    uo = ue[:P.n_owned * P.bs]
    err = np.linalg.norm(u - uo) / np.linalg.norm(uo)
    print(f"{problem} P{order} {dims} {feed}: {it} iterations, relative l2 error {err:.3e}")
    assert err <= 1e-9
    assert np.abs(u[bc] - uo[bc]).max() <= 1e-12 * np.abs(uo[bc]).max()


@pytest.mark.parametrize("order,m", [(1, 3), (2, 2)])
def test_patch_solution_on_the_unstructured_mesh(order, m):
    """2. (continued) the ring-with-spurs mesh with its whole boundary constrained: u = 1 + 2 x + 3 y - z."""
    P = zzz.Part.spoke("poisson", order, m)
    ue = _closed_form(P, spoke=True)
    bc = P.bc_marker().astype(bool)
    with zzz.Context(0) as c:
        c.upload_part(P)
        it, u = _patch_solve(c, P, ue, pc=zzz.PC_JACOBI, rtol=1e-12)
    err = np.linalg.norm(u - ue) / np.linalg.norm(ue)
    print(f"spoke P{order} m={m}: {it} iterations, relative l2 error {err:.3e}")
    assert err <= 1e-9
    assert np.abs(u[bc] - ue[bc]).max() <= 1e-12 * np.abs(ue[bc]).max()


@pytest.mark.parametrize("problem,order,dims", [("poisson", 2, (3, 2, 3)), ("elasticity", 1, (4, 3, 5))])
def test_nothing_changes_without_values(problem, order, dims):
    """3. No upload, an upload of zeros and an upload cleared by None give the same b; the Jacobi solves take the same
    iterations, and the first and the last -- the same kernels on the same bits -- the same solution."""
    P = _part(problem, order, dims)
    with zzz.Context(0) as c:
        c.upload_part(P)
        c.pattern_build()
        c.assemble_matrix(P.form)
        out = []
        for values in ("none", np.zeros(P.nloc * P.bs), None):
            if not isinstance(values, str):
                c.upload_bc_values(values)
            c.assemble_vector(P.form)
            b = c.vec_download(zzz.VEC_B)
            it, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
            out.append((b, it, c.vec_download(zzz.VEC_U)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][0], out[2][0])
    assert out[0][1] == out[1][1] == out[2][1]
    assert np.array_equal(out[0][2], out[2][2])


@pytest.mark.parametrize("problem,order,dims", [("poisson", 2, (3, 2, 3)), ("elasticity", 1, (4, 3, 5))])
def test_values_in_the_callers_numbering(problem, order, dims):
    """4. The same problem fed with dofs, vertices and cells in random order: the values are translated on the way in like
    the coefficients, and b is the native feed's after the permutation."""
    P = _part(problem, order, dims)
    Q = P.renumbered("random", seed=4)
    bs = P.bs
    g = _noise_values(P, 3)
    full = np.concatenate([Q.dof_new_of_old, np.arange(P.n_owned, P.nloc)])
    gq = np.empty_like(g)
    gq.reshape(P.nloc, bs)[full] = g.reshape(P.nloc, bs)
    res = []
    for part, vals in ((P, g), (Q, gq)):
        with zzz.Context(0) as c:
            c.upload_part(part)
            c.upload_bc_values(vals)
            c.pattern_build()
            c.assemble_vector(part.form)
            res.append(c.vec_download(zzz.VEC_B))
    s_new = (Q.dof_new_of_old[:, None] * bs + np.arange(bs)).reshape(-1)
    err = np.abs(res[1][s_new] - res[0]).max() / np.abs(res[0]).max()
    print(f"{problem} P{order}: renumbered against native {err:.3e}")
    assert err <= 1e-13
    bc = P.bc_marker().astype(bool)[:P.n_owned * bs]
    assert np.array_equal(res[1][s_new][bc], g[:P.n_owned * bs][bc])


@pytest.mark.parametrize("problem,order,dims,nparts", [("poisson", 1, (10, 9, 12), 2), ("poisson", 2, (5, 4, 9), 3),
                                                       ("elasticity", 1, (5, 5, 8), 2)])
def test_lifting_partitioned_on_one_gpu(problem, order, dims, nparts):
    """5. Partitions (one context per rank on this GPU, host-mediated communicator, host and device feeds mixed): every
    rank uploads the global function of the patch tests at ITS dofs, ghosts included -- lifting needs no communication --
    and the concatenated b, the iteration count and the solution are the one-rank run's."""
    import threading

    G = zzz.Part(problem, order, *dims)
    with zzz.Context(0) as c0:
        c0.upload_part(G)
        c0.upload_bc_values(_closed_form(G))
        c0.pattern_build()
        c0.assemble_matrix(G.form)
        c0.assemble_vector(G.form)
        b0 = c0.vec_download(zzz.VEC_B)
        it0, _, _ = c0.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
        u0 = c0.vec_download(zzz.VEC_U)
    grp = zzz.LocalGroup(nparts)
    out, err = [None] * nparts, []

    def run(rank):
        try:
            P = zzz.Part(problem, order, *dims, nparts, rank)
            with zzz.Context(0) as c:
                c.comm_init_local(grp.h, rank)
                _feed(c, P, "upload_part" if rank % 2 == 0 else "cube_generate")
                c.upload_bc_values(_closed_form(P))
                c.pattern_build()
                c.assemble_matrix(P.form)
                c.assemble_vector(P.form)
                b = c.vec_download(zzz.VEC_B)
                it, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
                out[rank] = (P.own_offset, b, it, c.vec_download(zzz.VEC_U))
        except Exception as e:  # noqa: BLE001
            err.append((rank, repr(e)))
            grp.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(nparts)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    grp.close()
    assert not err, err
    assert [o[0] for o in out] == sorted(o[0] for o in out)
    b = np.concatenate([o[1] for o in out])
    u = np.concatenate([o[3] for o in out])
    eb, eu = np.abs(b - b0).max() / np.abs(b0).max(), np.linalg.norm(u - u0) / np.linalg.norm(u0)
    print(f"{problem} P{order} {dims} on {nparts} ranks: b {eb:.3e}, u {eu:.3e}, iterations {[o[2] for o in out]} / {it0}")
    assert eb <= 1e-13
    assert len({o[2] for o in out}) == 1 and abs(out[0][2] - it0) <= 1
    assert eu <= 1e-9


def test_matrix_free_solves_with_values():
    """6. The matrix-free operator zeroes the constrained rows of its action, so with values the solve runs on b with its
    constrained entries taken as zero, in a copy: KSPCG reaches the closed form and ends with u[bc] = g, the cg.h form
    reaches the same interior values and leaves u[bc] at the (zero) initial guess, and the caller's b is untouched."""
    P = _part("poisson", 2, (3, 2, 3))
    ue = _closed_form(P)
    bc = P.bc_marker().astype(bool)
    with zzz.Context(0) as c:
        c.upload_part(P)
        it, u = _patch_solve(c, P, ue, pc=zzz.PC_JACOBI, op=zzz.OP_MATFREE, rtol=1e-12)
        b = c.vec_download(zzz.VEC_B)
        assert np.array_equal(b[bc], ue[bc]) and np.abs(ue[bc]).min() > 0.5
        c.vec_upload(zzz.VEC_U, np.zeros(P.n_owned))
        it2, _, _ = c.cg_solve(variant=zzz.CG_CGH, pc=zzz.PC_NONE, op=zzz.OP_MATFREE, rtol=1e-10, max_it=1000)
        u2 = c.vec_download(zzz.VEC_U)
        b2 = c.vec_download(zzz.VEC_B)
    e1 = np.linalg.norm(u - ue) / np.linalg.norm(ue)
    e2 = np.linalg.norm((u2 - ue)[~bc]) / np.linalg.norm(ue[~bc])
    print(f"matrix-free: KSPCG {it} iterations, error {e1:.3e}; cg.h {it2} iterations, interior error {e2:.3e}")
    assert e1 <= 1e-9
    assert np.array_equal(u[bc], ue[bc])
    assert e2 <= 1e-7 and it2 < 1000
    assert np.array_equal(u2[bc], np.zeros(int(bc.sum())))
    assert np.array_equal(b, b2)


def test_call_order_and_clearing():
    """7. Values need a dof layout and a Dirichlet set; whatever changes either clears them; a refusal leaves the context
    usable."""
    P = _part("poisson", 1, (4, 3, 5))
    g = _noise_values(P, 5)
    other = P.bc_dofs[::2].copy()  # another Dirichlet set
    with zzz.Context(0) as c:
        with pytest.raises(zzz.ZzzError) as e:
            c.upload_bc_values(g)
        assert e.value.code == 1 and "zzz_dofmap_upload" in str(e.value)
        c.upload_mesh(P.x, P.cells)
        c.upload_dofmap(P.order, P.bs, P.cell_dofs, P.n_owned, P.n_ghost)
        with pytest.raises(zzz.ZzzError) as e:
            c.upload_bc_values(g)
        assert e.value.code == 1 and "Dirichlet set" in str(e.value)
        with pytest.raises(ValueError):
            c.upload_bc_values(g[:-1])
        c.upload_bc(P.bc_dofs)
        c.upload_facets(P.facets)
        c.upload_coeff(zzz.COEFF_F, P.f)
        c.upload_coeff(zzz.COEFF_G, P.g)
        c.upload_bc_values(g)
        c.pattern_build()
        c.assemble_vector(P.form)
        b = c.vec_download(zzz.VEC_B)
        assert np.abs(b - _lifted_reference("poisson", 1, (4, 3, 5), g)).max() <= 1e-12 * np.abs(b).max()
        c.upload_bc(other)  # clears the values: the next b is the u0 == 0 vector of that set
        c.assemble_vector(P.form)
        b1 = c.vec_download(zzz.VEC_B)
    with zzz.Context(0) as c:
        c.upload_part(P)
        c.upload_bc(other)
        c.pattern_build()
        c.assemble_vector(P.form)
        assert np.array_equal(b1, c.vec_download(zzz.VEC_B))
        assert np.all(b1[other] == 0.0)


def test_values_after_ghost_layer_build():
    """7. (continued) zzz_ghost_layer_build changes the dof layout, so it clears the values; an upload sized for the new
    zzz_local_sizes -- the new ghosts included, found through their global numbers -- is accepted and gives the ghost-layer
    feed's vector."""
    import threading

    problem, order, dims, nparts = "poisson", 1, (6, 5, 8), 2
    G = zzz.Part(problem, order, *dims)
    ug = _closed_form(G)
    grp = zzz.LocalGroup(nparts)
    out, err = [None] * nparts, []

    def run(rank):
        try:
            Pn = zzz.Part(problem, order, *dims, nparts, rank, native=True)
            Pg = zzz.Part(problem, order, *dims, nparts, rank)
            with zzz.Context(0) as c, zzz.Context(0) as cg:
                c.comm_init_local(grp.h, rank)
                c.upload_part(Pn)
                c.upload_halo(Pn)
                c.upload_global_ids(Pn.global_dofs, Pn.global_verts)
                c.upload_bc_values(_closed_form(Pn))
                sizes = c.ghost_layer_build()
                c.pattern_build()
                c.assemble_vector(Pn.form)
                cleared = c.vec_download(zzz.VEC_B)
                gid = c.global_ids()
                grew = gid.size > Pn.nloc  # (the rank that owns the interface dofs gains ghosts; the other had them already)
                assert gid.size == sizes[2] + sizes[3]
                if grew:
                    with pytest.raises(ValueError):
                        c.upload_bc_values(_closed_form(Pn))  # the old size
                c.upload_bc_values(ug[gid])
                c.assemble_vector(Pn.form)
                b = c.vec_download(zzz.VEC_B)
                cg.upload_part(Pg)
                cg.pattern_build()
                cg.assemble_vector(Pg.form)
                b_zero = cg.vec_download(zzz.VEC_B)
                cg.upload_bc_values(_closed_form(Pg))
                cg.assemble_vector(Pg.form)
                # rows by their GLOBAL number (the two feeds of a rank may number their local rows differently)
                inv = np.empty(G.n_owned, np.int64)
                inv[Pg.global_dofs[:Pg.n_owned]] = np.arange(Pg.n_owned)
                rows = inv[gid[:Pn.n_owned]]
                out[rank] = (cleared, b_zero[rows], b, cg.vec_download(zzz.VEC_B)[rows], grew)
        except BaseException as e:  # noqa: BLE001 -- (pytest's own failures are no Exception)
            err.append((rank, repr(e)))
            grp.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(nparts)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    grp.close()
    assert not err, err
    assert any(o[4] for o in out)
    for cleared, b_zero, b, b_ghost_feed, _ in out:
        scale = np.abs(b_ghost_feed).max()
        assert np.abs(cleared - b_zero).max() <= 1e-13 * scale
        assert np.abs(b - b_ghost_feed).max() <= 1e-13 * scale
        assert np.abs(b - b_zero).max() > 1e-3 * scale


def _driver(args):
    import subprocess

    exe = os.path.join(zzz.PKG, "dolfinx-scaling-test")
    o = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert o.returncode == 0, o.stderr[-1000:]
    s = o.stdout
    return (int(s.split("*** Number of Krylov iterations: ")[1].split()[0]), float(s.split("*** Solution norm:  ")[1].split()[0]), s)


def _mirror_norm(problem, order, dims, value, rtol):
    with zzz.Context(0) as c:
        c.cube_generate(problem, order, *dims)
        c.upload_bc_values(np.full((c.n_owned + c.n_ghost) * c.bs, value))
        c.pattern_build()
        form = zzz.FORM_ELASTICITY if problem == "elasticity" else zzz.FORM_POISSON
        c.assemble_matrix(form)
        c.assemble_vector(form)
        it, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=rtol)
        return it, c.vec_norm(zzz.VEC_U)


@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
def test_driver_bc_value(problem):
    """8. --bc_value c: u0 == c at every constrained dof, uploaded behind the feed on every rank; the printed solution norm
    is the Python mirror's for the same cube, on one rank and on two; without the flag (or with 0, the reference's u0)
    stdout's iteration count and norm are what they were."""
    import re

    base = ["--problem_type", problem, "--scaling_type", "strong", "--ndofs", "50000", "-ksp_type", "cg", "-pc_type", "jacobi",
            "-ksp_rtol", "1.0e-10"]
    it_ref, nrm_ref, s_ref = _driver(base)
    it_0, nrm_0, s_0 = _driver(base + ["--bc_value", "0"])
    assert (it_0, nrm_0) == (it_ref, nrm_ref)
    assert [ln for ln in s_0.splitlines() if ln.startswith("  ") and "ZZZ" not in ln] == \
           [ln for ln in s_ref.splitlines() if ln.startswith("  ") and "ZZZ" not in ln]
    it_v, nrm_v, s_v = _driver(base + ["--bc_value", "0.25"])
    nx, ny, nz, r = (int(v) for v in re.search(r"UnitCube \((\d+)x(\d+)x(\d+)\) to be refined (\d+) times", s_v).groups())
    assert r == 0
    it_m, nrm_m = _mirror_norm(problem, 1, (nx, ny, nz), 0.25, 1e-10)
    print(f"{problem}: driver {it_v} iterations |u| = {nrm_v}, mirror {it_m} iterations |u| = {nrm_m}; u0 == 0: |u| = {nrm_ref}")
    assert abs(nrm_v - nrm_m) <= 1e-6 * nrm_m and abs(it_v - it_m) <= 2
    assert abs(nrm_v - nrm_ref) > 1e-3 * nrm_ref
    it_2, nrm_2, s_2 = _driver(base + ["--bc_value", "0.25", "--ngpus", "2", "--comm", "local"])
    assert "  Num processes:   2" in s_2
    dims2 = tuple(int(v) for v in re.search(r"UnitCube \((\d+)x(\d+)x(\d+)\) to be refined 0 times", s_2).groups())
    if dims2 != (nx, ny, nz):  # (the mesh-size search may answer two processes with another cube)
        it_m, nrm_m = _mirror_norm(problem, 1, dims2, 0.25, 1e-10)
    assert abs(nrm_2 - nrm_m) <= 1e-6 * nrm_m and abs(it_2 - it_m) <= 2


def test_driver_bc_value_surface():
    """8. (continued) --help names the option; it works with --mesh_type unstructured (the host feed's upload path)."""
    import subprocess

    exe = os.path.join(zzz.PKG, "dolfinx-scaling-test")
    h = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and "--bc_value arg (=0)" in h.stdout
    base = ["--problem_type", "poisson", "--mesh_type", "unstructured", "--scaling_type", "strong", "--ndofs", "20000", "-pc_type",
            "jacobi", "-ksp_rtol", "1.0e-10"]
    it, nrm, s = _driver(base + ["--bc_value", "0.25"])
    m = zzz.host().zzzh_spoke_size(20000, 1)
    P = zzz.Part.spoke("poisson", 1, m)
    with zzz.Context(0) as c:
        c.upload_part(P)
        c.upload_bc_values(np.full(P.nloc, 0.25))
        c.pattern_build()
        c.assemble_matrix(P.form)
        c.assemble_vector(P.form)
        c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-10)
        nrm_m = c.vec_norm(zzz.VEC_U)
    # the driver prints six significant digits: half a unit of the last one on top of the 1e-6 of the cube cases
    bar = 1e-6 * nrm_m + 0.5 * 10.0 ** (np.floor(np.log10(nrm_m)) - 5)
    print(f"unstructured: driver |u| = {nrm}, mirror |u| = {nrm_m}, bar {bar:.2e}")
    assert abs(nrm - nrm_m) <= bar
    it3, nrm3, _ = _driver(base + ["--bc_value", "0.25", "--ngpus", "3", "--comm", "local"])
    assert abs(nrm3 - nrm_m) <= bar
