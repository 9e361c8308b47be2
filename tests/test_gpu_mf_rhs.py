"""The right-hand side on the cell-block plan (zzz_matfree_assemble_vector; csrc/zzz_matfree.hip: k_mf_rhs and the lifting
through the plan's own action): what zzz_assemble_vector fills, on a context that never builds a sparsity pattern.

  1. the oracle's vector within 1e-12 max|b| on one block and on several (MF_SMALL), exact zeros on the Dirichlet set, the
     same bits from a second call and from a rebuilt plan, no pattern afterwards, and both assemblies on one context;
  2. every instantiation: ZZZ_MF_T in 128 / 256 / 512 (1024 at block size 1), with several steps per block;
  3. the hostile meshes of tests/_hostile.py at the per-entry bar of the row-gather vector (50-digit reference);
  4. lifting against H.lifted_reference, NaN off the Dirichlet set;
  5. a per-component Dirichlet set at block size 3;
  6. three ranks, no communicator: every rank's owned rows are complete;
  7. the refusal (ZZZ_ERR_LIMIT naming zzz_csr_pattern_build) and the argument errors;
  8. solves on a context that never had a pattern;
  9. the driver's --vector_assembly cellblock.

No test calls pattern_build before the new entry point unless it says so."""
import subprocess

from _gpu_helpers import *  # noqa: F401,F403 -- helpers, np / os / zzz / zo / pytest
import _hostile as H
import _hp_ref as hp
from _hostile_gpu import MF_SMALL, _bar, _env, _upload

pytestmark = pytest.mark.gpu  # noqa: F405

PARITY = [("poisson", 1, (6, 5, 5)), ("poisson", 2, (4, 4, 5)), ("poisson", 3, (3, 3, 4)),
          ("elasticity", 1, (6, 5, 5)), ("elasticity", 2, (3, 3, 4)), ("elasticity", 3, (3, 3, 4))]
PARITY_IDS = [f"{p}-P{o}" for p, o, _ in PARITY]
_ORACLE = {}


def _cube(problem, order, dims):
    """(Part, the oracle's b): computed once, shared, read-only"""
    key = (problem, order, tuple(dims))
    if key not in _ORACLE:
        zo.set_num_threads(1)
        P = zzz.Part(problem, order, *dims)
        ob = zo.assemble_vector(P.form, order, P.x, P.cells, P.cell_dofs, P.f, P.g, P.facets if P.g is not None else None, P.bc_marker())
        ob.setflags(write=False)
        _ORACLE[key] = (P, ob)
    return _ORACLE[key]


def _no_pattern(c):
    with pytest.raises(zzz.ZzzError) as e:
        c.csr_sizes()
    assert "no sparsity pattern" in str(e.value)


@pytest.mark.parametrize("small", [False, True], ids=["default-plan", "MF_SMALL"])
@pytest.mark.parametrize("problem,order,dims", PARITY, ids=PARITY_IDS)
def test_oracle_parity_bits_and_coexistence(problem, order, dims, small):
    """1."""
    P, ob = _cube(problem, order, dims)
    bcb = P.bc_marker().astype(bool)
    tol = 1e-12 * np.abs(ob).max()
    knobs = MF_SMALL if small else dict(ZZZ_MF_T=None, ZZZ_MF_NC=None)
    with _env(**knobs), zzz.Context(0) as c:
        c.upload_part(P)
        c.matfree_assemble_vector(P.form)
        b = c.vec_download(zzz.VEC_B)
        info = c.matfree_info()
        err = np.abs(b - ob).max()
        print(f"\nMFRHS {problem} P{order} {dims} {'small' if small else 'default'}: {info['blocks']} x {info['cells_per_block']} cells, "
              f"{info['shared_dofs']} shared | |b - oracle| / max|b| {err / np.abs(ob).max():.2e}")
        if small:
            assert info["blocks"] >= 2 and info["shared_dofs"] > 0 and P.ncells % info["cells_per_block"] != 0
        else:
            assert info["blocks"] == 1
        assert err <= tol
        assert np.array_equal(b[bcb].view(np.uint64), np.zeros(int(bcb.sum()), np.uint64))
        c.matfree_assemble_vector(P.form)
        np.testing.assert_array_equal(c.vec_download(zzz.VEC_B).view(np.uint64), b.view(np.uint64))
        c.matfree_setup()  # a rebuilt plan
        c.matfree_assemble_vector(P.form)
        np.testing.assert_array_equal(c.vec_download(zzz.VEC_B).view(np.uint64), b.view(np.uint64))
        _no_pattern(c)
        # the row-gather assembly on the same context, then the cell-block one again
        c.pattern_build()
        c.assemble_vector(P.form)
        br = c.vec_download(zzz.VEC_B)
        assert np.abs(br - b).max() <= tol and np.abs(br - ob).max() <= tol
        c.matfree_assemble_vector(P.form)
        np.testing.assert_array_equal(c.vec_download(zzz.VEC_B).view(np.uint64), b.view(np.uint64))


# 2. the smallest cube on which the SECOND step of a block of 2 T cells holds real cells (more than T cells) and a block of 2 T
# cells fits LDS.  Elasticity P3 with 512 threads has none: 2730 nodes fit a block and any 513 cells of a P3 mesh touch more, so
# its second step runs on the block's tail alone (index words 0, rank bytes 0xff), as in tests/test_gpu_mf_elasticity_plans.py.
INST_DIMS = {("poisson", 1): [(6, 5, 5), (6, 6, 6)], ("poisson", 2): [(4, 4, 5), (6, 6, 6)], ("poisson", 3): [(3, 3, 4), (6, 6, 6)],
             ("elasticity", 1): [(6, 5, 5)], ("elasticity", 2): [(3, 3, 4), (5, 5, 5)], ("elasticity", 3): [(3, 3, 4), (4, 4, 5)]}


def _inst_dims(problem, order, T):
    for d in INST_DIMS[(problem, order)]:
        if 6 * d[0] * d[1] * d[2] > T:
            return d
    assert (problem, order, T) == ("elasticity", 3, 512)
    return INST_DIMS[(problem, order)][-1]


INST = [(p, o, _inst_dims(p, o, T), T) for p, o, _ in PARITY for T in ((128, 256, 512, 1024) if p == "poisson" else (128, 256, 512))]


@pytest.mark.parametrize("problem,order,dims,T", INST, ids=[f"{p}-P{o}-T{T}" for p, o, _, T in INST])
def test_every_instantiation(problem, order, dims, T):
    """2. k_mf_rhs<ND, T, BS> for every T offered, two steps per block (ZZZ_MF_NC = 2 T: the `for s` loop, its `if (s == 0)`
    barrier and the per-step rmax words), both of them holding cells"""
    P, ob = _cube(problem, order, dims)
    with _env(ZZZ_MF_T=T, ZZZ_MF_NC=2 * T), zzz.Context(0) as c:
        c.upload_part(P)
        c.matfree_assemble_vector(P.form)
        b = c.vec_download(zzz.VEC_B)
        info = c.matfree_info()
    err = np.abs(b - ob).max() / np.abs(ob).max()
    print(f"\nMFRHS instantiation {problem} P{order} {dims} T={T}: {P.ncells} cells, plan {info['blocks']} x {info['cells_per_block']}, "
          f"threads {info['threads']} | {err:.2e}")
    assert info["threads"] == T and info["cells_per_block"] == 2 * T
    assert P.ncells > T or (problem, order, T) == ("elasticity", 3, 512)
    assert err <= 1e-12
    assert np.all(b[P.bc_marker().astype(bool)] == 0.0)


_HOSTILE = [("poisson", n, o) for n, o in H.POISSON_CASES] + [("elasticity", n, o) for o in (1, 2, 3) for n in H.ELASTICITY_CASES[o]]


@pytest.mark.parametrize("problem,name,order", _HOSTILE, ids=[f"{p}-{n}-P{o}" for p, n, o in _HOSTILE])
def test_hostile_meshes_against_the_50_digit_reference(problem, name, order):
    """3. the bar the row-gather vector is held to in tests/test_gpu_hostile_geometry.py and test_gpu_hostile_elasticity.py"""
    C = H.case(name, order, problem)
    ref = H.reference(C)
    bcb = C.bc.astype(bool)
    for renumber in (None, "2"):
        with _env(**MF_SMALL), zzz.Context(0) as c:
            _upload(c, C, renumber)
            c.matfree_assemble_vector(C.form)
            b = c.vec_download(zzz.VEC_B)
            info = c.matfree_info()
        fig = hp.metric(b, ref["r"], ref["s"]) / hp.U
        print(f"\nMFRHS hostile {problem:10s} {name:10s} P{order} {'bins   ' if renumber else 'default'} {info['blocks']} blocks | b {fig:8.2f} "
              f"oracle {ref['oracle_b']:7.2f}")
        assert np.all(b[bcb] == 0.0)
        assert fig <= _bar(ref["oracle_b"]), (fig, ref["oracle_b"], renumber)


_LIFT = [(p, n, o) for p in ("poisson", "elasticity") for n, o in H.LIFTING_CASES[p]]


@pytest.mark.parametrize("problem,name,order", _LIFT, ids=[f"{p}-{n}-P{o}" for p, n, o in _LIFT])
def test_lifting_against_the_50_digit_reference(problem, name, order):
    """4. u0 is seeded noise with NaN at a few unconstrained entries, as in test_lifted_vector_against_the_50_digit_reference"""
    C = H.case(name, order, problem)
    bcb = C.bc.astype(bool)
    rng = np.random.default_rng(11 * order + C.bs)
    g = rng.standard_normal(C.n)
    g[rng.choice(np.nonzero(~bcb)[0], size=7, replace=False)] = np.nan
    r, s, fo = H.lifted_reference(C, g)
    for renumber in (None, "2"):
        with _env(**MF_SMALL), zzz.Context(0) as c:
            _upload(c, C, renumber)
            c.matfree_assemble_vector(C.form)
            b0 = c.vec_download(zzz.VEC_B)
            c.upload_bc_values(g)
            c.matfree_assemble_vector(C.form)
            b = c.vec_download(zzz.VEC_B)
            c.matfree_assemble_vector(C.form)
            b2 = c.vec_download(zzz.VEC_B)
            _no_pattern(c)
        fig = hp.metric(b, r, s) / hp.U
        print(f"\nMFRHS lifting {problem:10s} {name:10s} P{order} {'bins   ' if renumber else 'default'} | b {fig:8.2f} oracle {fo:7.2f}")
        assert not np.isnan(b).any() and np.isfinite(b).all()
        assert np.array_equal(b[bcb].view(np.uint64), g[bcb].view(np.uint64))
        np.testing.assert_array_equal(b2.view(np.uint64), b.view(np.uint64))
        assert not np.array_equal(b[~bcb], b0[~bcb])  # the lifting did something
        assert fig <= _bar(fo), (fig, fo)


@pytest.mark.parametrize("order", [1, 2, 3])
def test_dirichlet_set_per_component(order):
    """5. component 1 alone of the nodes on x = 0, all three components on x = 1 (as test_dirichlet_set_per_component of
    tests/test_gpu_mf_elasticity.py): the rows of the constrained scalar dofs are 0.0, the other two components of a
    half-constrained node are the oracle's -- also where such a node is shared between blocks (P3 keeps the caller's cell order,
    so that the host restates the blocks)."""
    dims = {1: (6, 5, 5), 2: (3, 3, 4), 3: (3, 3, 4)}[order]
    P, _ = _cube("elasticity", order, dims)
    x = P.dof_x[:P.n_owned, 0]
    m = np.zeros(3 * P.n_owned, np.uint8)
    m[3 * np.nonzero(x == 0.0)[0] + 1] = 1
    for k in range(3):
        m[3 * np.nonzero(x == 1.0)[0] + k] = 1
    half = m.reshape(-1, 3).sum(axis=1) == 1
    assert half.any() and np.any(m.reshape(-1, 3).sum(axis=1) == 3)
    if order == 3:
        blk = H.plan_cell_blocks(P, int(MF_SMALL["ZZZ_MF_NC"]))
        in_blocks = np.zeros((P.n_owned, int(blk.max()) + 1), bool)
        in_blocks[P.cell_dofs.reshape(-1), np.repeat(blk, P.cell_dofs.shape[1])] = True
        assert (half & (in_blocks.sum(axis=1) > 1)).sum() >= 4
    zo.set_num_threads(1)
    ob = zo.assemble_vector(P.form, order, P.x, P.cells, P.cell_dofs, P.f, None, None, m)
    with _env(**MF_SMALL), zzz.Context(0) as c:
        with _env(ZZZ_RENUMBER="0" if order == 3 else None):
            c.upload_part(P)
        c.upload_bc(np.nonzero(m)[0].astype(np.int32))
        c.matfree_assemble_vector(P.form)
        b = c.vec_download(zzz.VEC_B)
        assert c.matfree_info()["blocks"] >= 2
    mb = m.astype(bool)
    assert np.array_equal(b[mb].view(np.uint64), np.zeros(int(mb.sum()), np.uint64))
    assert np.abs(b - ob).max() <= 1e-12 * np.abs(ob).max()
    free_of_half = np.repeat(half, 3) & ~mb
    assert free_of_half.sum() == 2 * half.sum() and np.all(b[free_of_half] != 0.0)
    assert np.abs(b[free_of_half] - ob[free_of_half]).max() <= 1e-12 * np.abs(ob).max()


@pytest.mark.parametrize("problem", ["poisson", "elasticity"])
def test_three_ranks_without_a_communicator(problem):
    """6. three z-slabs of the 3 x 3 x 6 cube at P2, each on a context of its own with no communicator: the owned rows of every
    rank, through the part's global ids, are the whole mesh's oracle vector"""
    order, dims = 2, (3, 3, 6)
    G, ob = _cube(problem, order, dims)
    bs = G.bs
    seen = np.zeros(G.n_owned, bool)
    for rank in range(3):
        P = zzz.Part(problem, order, *dims, 3, rank)
        assert P.n_ghost > 0
        with _env(**MF_SMALL), zzz.Context(0) as c:
            c.upload_part(P)
            c.matfree_assemble_vector(P.form)
            b = c.vec_download(zzz.VEC_B)
            _no_pattern(c)
        gid = P.global_dofs[:P.n_owned]
        rows = (gid[:, None] * bs + np.arange(bs)).reshape(-1)
        err = np.abs(b - ob[rows]).max() / np.abs(ob).max()
        print(f"\nMFRHS {problem} P2 rank {rank}: {P.n_owned} owned, {P.n_ghost} ghost | {err:.2e}")
        assert err <= 1e-12
        assert not seen[gid].any()
        seen[gid] = True
    assert seen.all()


def test_refusal_and_argument_errors():
    """7. P3 elasticity 5 x 5 x 5 with ZZZ_MF_T=512 (the refusal of tests/test_gpu_mf_elasticity_plans.py): ZZZ_ERR_LIMIT naming
    zzz_csr_pattern_build, b untouched, the row-gather way out works; ZZZ_ERR_ARG for a missing coefficient and an unknown form"""
    P, ob = _cube("elasticity", 3, (5, 5, 5))
    mark = np.random.default_rng(70).standard_normal(3 * P.n_owned)
    with zzz.Context(0) as c:
        c.upload_part(P)
        c.vec_upload(zzz.VEC_B, mark)
        with _env(ZZZ_MF_T=512, ZZZ_MF_NC=None):
            with pytest.raises(zzz.ZzzError) as e:
                c.matfree_assemble_vector(P.form)
        print(f"\nMFRHS refusal: {e.value}")
        assert e.value.code == 5 and "zzz_csr_pattern_build" in str(e.value) and "zzz_assemble_vector" in str(e.value)
        np.testing.assert_array_equal(c.vec_download(zzz.VEC_B), mark)
        c.pattern_build()
        c.assemble_vector(P.form)
        assert np.abs(c.vec_download(zzz.VEC_B) - ob).max() <= 1e-12 * np.abs(ob).max()
        with pytest.raises(zzz.ZzzError) as e:
            c.matfree_assemble_vector(7)
        assert e.value.code == 1 and "unknown form 7" in str(e.value)
    Q, _ = _cube("poisson", 1, (6, 5, 5))
    with zzz.Context(0) as c:
        c.upload_mesh(Q.x, Q.cells)
        c.upload_dofmap(Q.order, Q.bs, Q.cell_dofs, Q.n_owned, Q.n_ghost)
        c.upload_bc(Q.bc_dofs)
        c.upload_facets(Q.facets)
        for have_f in (False, True):  # nothing, then f without g
            if have_f:
                c.upload_coeff(zzz.COEFF_F, Q.f)
            with pytest.raises(zzz.ZzzError) as e:
                c.matfree_assemble_vector(Q.form)
            assert e.value.code == 1 and "coefficient(s) of L not uploaded" in str(e.value)


@pytest.mark.parametrize("problem,dims,cgh_dims", [("poisson", (4, 4, 5), (12, 12, 12)), ("elasticity", (3, 3, 4), (3, 3, 4))])
def test_solves_without_a_pattern(problem, dims, cgh_dims):
    """8. Jacobi-CG on the matrix-free operator from this b: iterations within +-2 of the oracle's PCG on the oracle's system,
    solution within 1e-6; linalg::cg(u, b, action, 100, 1e-6) runs its 100 iterations (Poisson: on 12 x 12 x 12, 15 625 dofs --
    on 4 x 4 x 5 it is done after 57, the oracle's count too); at block size 1 the float32 solve runs from this b"""
    P, ob = _cube(problem, 2, dims)
    zo.set_num_threads(1)
    rp, cl = zo.pattern(P.n_owned, P.cell_dofs, P.bs)
    ov = zo.assemble_matrix(P.form, 2, P.x, P.cells, P.cell_dofs, P.bc_marker(), rp, cl)
    oit, ou, _, _ = zo.pcg(rp, cl, ov, ob, rtol=1e-8)
    with zzz.Context(0) as c:
        c.upload_part(P)
        c.matfree_assemble_vector(P.form)
        it, _, _ = c.cg_solve(op=zzz.OP_MATFREE, pc=zzz.PC_JACOBI, rtol=1e-8)
        u = c.vec_download(zzz.VEC_U)
        _no_pattern(c)
    assert abs(it - oit) <= 2 and np.linalg.norm(u - ou) <= 1e-6 * np.linalg.norm(ou)
    Q, qb = _cube(problem, 2, cgh_dims)
    if problem == "poisson":
        ok, _ = zo.cg_matfree_poisson(2, Q.x, Q.cells, Q.cell_dofs, Q.bc_marker(), np.array(qb), kmax=100, rtol=1e-6)
    else:
        ok, _, _ = zo.cg(rp, cl, ov, np.array(qb), kmax=100, rtol=1e-6)
    with zzz.Context(0) as c:
        c.upload_part(Q)
        c.matfree_assemble_vector(Q.form)
        c.vec_upload(zzz.VEC_U, np.zeros(Q.n_owned * Q.bs))
        ith, _, _ = c.cg_solve(variant=zzz.CG_CGH, pc=zzz.PC_NONE, op=zzz.OP_MATFREE, rtol=1e-6, max_it=100)
        it32 = None
        if problem == "poisson":
            c.vec_upload(zzz.VEC_U, np.zeros(Q.n_owned))
            it32 = c.cg_solve_f32()[0]
        _no_pattern(c)
    print(f"\nMFRHS solve {problem} P2: Jacobi-CG {it} (oracle {oit}), linalg::cg {ith} (oracle {ok}), float32 {it32}")
    assert ith == 100 and ok == 100  # (the iterate after 100 unconverged steps is not compared: rounding differences grow along the way)
    assert it32 is None or it32 == 100


LINE = "  Vector assembly: cellblock (no sparsity pattern)"
DRIVER = [(["--problem_type", "cgpoisson", "--order", "2", "--ndofs", "20000"], "linalg"),
          (["--problem_type", "cgelasticity", "--ndofs", "20000"], "linalg"),
          (["--problem_type", "cgelasticity", "--ndofs", "20000", "--cg_solver", "ksp", "-pc_type", "jacobi", "-ksp_rtol", "1e-8"], "ksp"),
          (["--problem_type", "poisson", "--operator", "matfree", "--ndofs", "30000", "-pc_type", "jacobi", "-ksp_rtol", "1e-8"], "ksp"),
          (["--problem_type", "cgpoisson", "--ndofs", "30000", "--bc_value", "0.25"], "linalg"),
          (["--problem_type", "cgpoisson", "--ndofs", "30000", "--ngpus", "3", "--comm", "local"], "linalg"),
          (["--problem_type", "cgpoisson", "--ndofs", "30000", "--mesh_type", "unstructured"], "linalg")]


def _its_norm(stdout):
    return (int(stdout.split("*** Number of Krylov iterations: ")[1].split()[0]), float(stdout.split("*** Solution norm:  ")[1].split()[0]))


@pytest.mark.parametrize("args,solver", DRIVER, ids=["cgpoisson-P2", "cgelasticity-linalg", "cgelasticity-ksp", "poisson-matfree", "bc_value",
                                                     "three-ranks", "unstructured"])
def test_driver_cellblock(args, solver):
    """9. the same command with and without --vector_assembly cellblock"""
    exe = os.path.join(zzz.PKG, "dolfinx-scaling-test")
    base = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    cell = subprocess.run([exe] + args + ["--vector_assembly", "cellblock"], capture_output=True, text=True, timeout=300)
    assert base.returncode == 0, base.stderr[-1000:]
    assert cell.returncode == 0, cell.stderr[-1000:]
    assert LINE in cell.stdout.splitlines() and "Vector assembly" not in base.stdout
    assert "ZZZ Assemble vector" in cell.stdout
    (it0, n0), (it1, n1) = _its_norm(base.stdout), _its_norm(cell.stdout)
    print(f"\nMFRHS driver {' '.join(args)}: rowgather {it0} {n0:.10g} | cellblock {it1} {n1:.10g}")
    assert (it0 == it1) if solver == "linalg" else abs(it0 - it1) <= 2
    assert abs(n0 - n1) <= 1e-6 * abs(n0)


@pytest.mark.parametrize("args", [["--problem_type", "poisson", "--vector_assembly", "cellblock"],
                                  ["--problem_type", "elasticity", "--vector_assembly", "cellblock"],
                                  ["--problem_type", "cgpoisson", "--vector_assembly", "foo"]], ids=["poisson", "elasticity", "foo"])
def test_driver_rejects(args):
    """9. (continued) the assembled problem types and an unknown value end non-zero, naming the option"""
    exe = os.path.join(zzz.PKG, "dolfinx-scaling-test")
    out = subprocess.run([exe] + args + ["--ndofs", "5000"], capture_output=True, text=True, timeout=60)
    assert out.returncode != 0 and "--vector_assembly" in (out.stderr + out.stdout)
