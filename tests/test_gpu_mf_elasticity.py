"""The matrix-free elasticity operator (block size 3: form a of src/Elasticity.py in csrc/zzz_matfree.hip, k_mf_action3) on the GPU.

Nothing is assembled by the code under test: action, diagonal and the solves on ZZZ_OP_MATFREE are compared with the oracle's
ASSEMBLED matrix (unconstrained, bc = 0, rows of constrained scalar dofs zeroed), with the library's own assembled solve, and
on the hostile meshes with the 50-digit reference.  "many blocks" = ZZZ_MF_NC = ZZZ_MF_T = 128 (_hostile_gpu.MF_SMALL): 8, 2
and 2 cell blocks at the dims below, so nodes are shared between blocks and k_mf_finish3 runs.  The other thread counts, several
steps per block, the LDS retry and the refusal: tests/test_gpu_mf_elasticity_plans.py.

  1. action and diagonal per ROW, in units of 2^-53 of the row's own scale (HE.oracle_figures), within max(8 o, 32) + o of the
     oracle's matrix, o = HE.O_ACTION / HE.O_DIAGONAL being the oracle's own distance from the 50-digit reference.
  5. linalg::cg: the numpy restatement of src/cg.h (tests/_cgh_ref.py) on the P1 cube 4 x 3 x 3 (240 scalar dofs, 60 of them
     constrained) meets the strict test rnorm / rnorm0 < 1e-12 after 90 of its 100 iterations (counted on a CPU, numpy).
  8. hostile meshes: figures in units of 2^-53 of the per-row scale, printed by the test.
"""
import threading

from _gpu_helpers import *  # noqa: F401,F403 -- helpers, np / os / zzz / zo / pytest
import _cgh_ref as cr
import _hostile as H
import _hostile_mf_elasticity as HE
import _hp_ref as hp
from _hostile_gpu import MF_SMALL, _bar, _env, _upload

pytestmark = pytest.mark.gpu  # noqa: F405

DIMS = {1: (6, 5, 5), 2: (3, 3, 4), 3: (3, 3, 4)}
_SYS = {}


def _system(order, dims, bc=None):
    """(P, bc marker, rowptr, cols, A unconstrained, its diagonal) -- and A constrained, b for the part's own Dirichlet set"""
    key = (order, dims, None if bc is None else bc.tobytes())
    if key not in _SYS:
        zo.set_num_threads(1)
        P = zzz.Part("elasticity", order, *dims)
        m = P.bc_marker() if bc is None else bc
        rp, cl = zo.pattern(P.n_owned, P.cell_dofs, 3)
        Au = zo.assemble_matrix(1, order, P.x, P.cells, P.cell_dofs, np.zeros_like(m), rp, cl)
        rows = np.repeat(np.arange(3 * P.n_owned), np.diff(rp))
        diag = np.zeros(3 * P.n_owned)
        diag[rows[cl == rows]] = Au[cl == rows]
        S = dict(P=P, bc=m, rp=rp, cl=cl, Au=Au, diag=diag)
        if bc is None:
            S["Ac"] = zo.assemble_matrix(1, order, P.x, P.cells, P.cell_dofs, m, rp, cl)
            S["b"] = zo.assemble_vector(1, order, P.x, P.cells, P.cell_dofs, P.f, None, P.facets, m)
        _SYS[key] = S
    return _SYS[key]


def _check_action_and_diagonal(c, S, seed, many):
    P, bcb = S["P"], S["bc"].astype(bool)
    v = np.random.default_rng(seed).standard_normal(3 * P.n_owned)
    c.matfree_setup()
    info = c.matfree_info()
    assert info["valid"] == 1
    if many:
        assert info["blocks"] > 1 and info["shared_dofs"] > 0, info
    y = c.action(v)
    d = c.matfree_diagonal()
    # per row, against the row's own scale (HE.oracle_figures; a constrained row must hold the bits 0.0 / 1.0): the bar is what
    # a kernel is granted against the truth plus what the oracle is away from it (HE.O_ACTION, HE.O_DIAGONAL)
    ey, ed = HE.oracle_figures(S["rp"], S["cl"], S["Au"], S["diag"], S["bc"], v, y, d)
    print(f"\nMF elasticity P{P.order} {P.dims}: {info['blocks']} blocks of {info['cells_per_block']} cells, {info['shared_dofs']} shared "
          f"nodes, {info['bytes_per_action']} B per action; action {ey:.2f}, diagonal {ed:.2f} units of 2^-53 of the row's scale")
    assert ey <= _bar(HE.O_ACTION[P.order]) + HE.O_ACTION[P.order]
    assert np.all(y[bcb] == 0.0)
    for _ in range(4):
        np.testing.assert_array_equal(c.action(v), y)
    c.matfree_setup()  # a rebuilt plan is the same plan
    np.testing.assert_array_equal(c.action(v), y)
    assert ed <= _bar(HE.O_DIAGONAL[P.order]) + HE.O_DIAGONAL[P.order]
    assert np.all(d[bcb] == 1.0)
    np.testing.assert_array_equal(c.matfree_diagonal(), d)
    return y


@pytest.mark.parametrize("order,many", [(1, True), (2, True), (3, True), (1, False)])
def test_action_and_diagonal_against_the_oracle(order, many):
    """1."""
    S = _system(order, DIMS[order])
    with _env(**(MF_SMALL if many else {})), zzz.Context(0) as c:
        c.upload_part(S["P"])
        _check_action_and_diagonal(c, S, 10 + order, many)


@pytest.mark.parametrize("order", [1, 2, 3])
def test_dirichlet_set_per_component(order):
    """2. component 1 alone of the nodes on x = 0, all three components on x = 1: a per-node flag gets the first face wrong.
    P3 (u gathered through gid, the dot product read from A.u) keeps the caller's cell order (ZZZ_RENUMBER=0), so that the host
    restates the blocks (H.plan_cell_blocks): half-constrained nodes lie in cells of BOTH blocks, i.e. their component bits are
    read from sh_flag in k_mf_finish3 and not from dof_flag alone."""
    P = _system(order, DIMS[order])["P"]
    x = P.dof_x[:P.n_owned, 0]
    m = np.zeros(3 * P.n_owned, np.uint8)
    m[3 * np.nonzero(x == 0.0)[0] + 1] = 1
    for k in range(3):
        m[3 * np.nonzero(x == 1.0)[0] + k] = 1
    assert 0 < m.sum() and np.any(m.reshape(-1, 3).sum(axis=1) == 1) and np.any(m.reshape(-1, 3).sum(axis=1) == 3)
    if order == 3:
        blk = H.plan_cell_blocks(P, int(MF_SMALL["ZZZ_MF_NC"]))
        in_blocks = np.zeros((P.n_owned, int(blk.max()) + 1), bool)
        in_blocks[P.cell_dofs.reshape(-1), np.repeat(blk, P.cell_dofs.shape[1])] = True
        half_shared = (m.reshape(-1, 3).sum(axis=1) == 1) & (in_blocks.sum(axis=1) > 1)
        print(f"\nMF elasticity P3 {P.dims}: {int(half_shared.sum())} half-constrained nodes shared between blocks")
        assert half_shared.sum() >= 4
    S = _system(order, DIMS[order], m)
    with _env(**MF_SMALL), zzz.Context(0) as c:
        with _env(ZZZ_RENUMBER="0" if order == 3 else None):
            c.upload_part(P)
        c.upload_bc(np.nonzero(m)[0].astype(np.int32))
        y = _check_action_and_diagonal(c, S, 20 + order, True)
    free_on_face = np.zeros_like(m, bool)
    free_on_face[3 * np.nonzero(x == 0.0)[0]] = True
    assert np.all(y[free_on_face] != 0.0)  # the unconstrained components of the half-constrained nodes are served


@pytest.mark.parametrize("order", [1, 2, 3])
def test_symmetry_and_rigid_body_modes(order):
    """3. empty Dirichlet set"""
    P = _system(order, DIMS[order])["P"]
    rng = np.random.default_rng(30 + order)
    v, w = rng.standard_normal(3 * P.n_owned), rng.standard_normal(3 * P.n_owned)
    with _env(**MF_SMALL), zzz.Context(0) as c:
        c.upload_part(P)
        c.upload_bc(np.zeros(0, np.int32))
        Av, Aw = c.action(v), c.action(w)
        B, _ = c.near_nullspace()
        worst = max(np.abs(c.action(B[k])).max() for k in range(6))
    print(f"\nMF elasticity P{order}: |w.Av - v.Aw| / |w.Av| {abs(w @ Av - v @ Aw) / abs(w @ Av):.2e}, "
          f"largest |A mode| / max|A v| {worst / np.abs(Av).max():.2e}")
    assert abs(w @ Av - v @ Aw) <= 1e-10 * abs(w @ Av)
    assert worst <= 1e-9 * np.abs(Av).max()


@pytest.mark.parametrize("order", [1, 2, 3])
def test_jacobi_pcg_and_pc_none_on_the_matrix_free_operator(order):
    """4. the bars of test_jacobi_pcg_on_the_matrix_free_operator"""
    S = _system(order, DIMS[order])
    P, ob = S["P"], S["b"]
    oit, ou, _, or0 = zo.pcg(S["rp"], S["cl"], S["Ac"], ob, rtol=1e-8)
    oitn, oun, _, _ = zo.pcg(S["rp"], S["cl"], S["Ac"], ob, pc=zo.PC_NONE, rtol=1e-8)
    with _env(**MF_SMALL), zzz.Context(0) as c:
        c.upload_part(P)  # nothing but mesh, dofmap, Dirichlet set and the right-hand side: no pattern, no matrix
        c.vec_upload(zzz.VEC_B, ob)
        it, rn, r0 = c.cg_solve(pc=zzz.PC_JACOBI, op=zzz.OP_MATFREE, rtol=1e-8)
        u = c.vec_download(zzz.VEC_U)
        itn, _, _ = c.cg_solve(pc=zzz.PC_NONE, op=zzz.OP_MATFREE, rtol=1e-8)
        un = c.vec_download(zzz.VEC_U)
        its_norm = [c.cg_solve(pc=zzz.PC_JACOBI, op=zzz.OP_MATFREE, norm=nm, rtol=1e-8)[0]
                    for nm in (zzz.NORM_UNPRECONDITIONED, zzz.NORM_NATURAL)]
        # ... and the library's own assembled solves on the same context
        c.pattern_build()
        c.assemble_matrix(zzz.FORM_ELASTICITY)
        c.assemble_vector(zzz.FORM_ELASTICITY)
        ita, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
        ua = c.vec_download(zzz.VEC_U)
        itna, _, _ = c.cg_solve(pc=zzz.PC_NONE, rtol=1e-8)
        una = c.vec_download(zzz.VEC_U)
        its_norm_a = [c.cg_solve(pc=zzz.PC_JACOBI, norm=nm, rtol=1e-8)[0] for nm in (zzz.NORM_UNPRECONDITIONED, zzz.NORM_NATURAL)]
    res = np.linalg.norm(ob - zo.spmv(S["rp"], S["cl"], S["Ac"], u)) / np.linalg.norm(ob)
    print(f"\nMF elasticity P{order}: Jacobi {it} (oracle {oit}, assembled {ita}), none {itn} (oracle {oitn}, assembled {itna}), "
          f"other norms {its_norm} (assembled {its_norm_a}); |u - ou| / |ou| {np.linalg.norm(u - ou) / np.linalg.norm(ou):.1e}, "
          f"true residual {res:.1e}")
    assert abs(it - oit) <= 2
    assert np.linalg.norm(u - ou) <= 1e-6 * np.linalg.norm(ou)
    assert abs(r0 - or0) <= 1e-11 * or0
    assert res <= 1e-7
    assert abs(it - ita) <= 2 and np.linalg.norm(u - ua) <= 1e-7 * np.linalg.norm(ua)
    assert abs(itn - oitn) <= 2 and np.linalg.norm(un - oun) <= 1e-6 * np.linalg.norm(oun)
    assert abs(itn - itna) <= 2 and np.linalg.norm(un - una) <= 1e-7 * np.linalg.norm(una)
    assert all(abs(a - b) <= 2 for a, b in zip(its_norm, its_norm_a))


def test_linalg_cg_against_the_restatement():
    """5. linalg::cg(u, b, action, 100, 1e-6) on the P1 cube 4 x 3 x 3: the restatement converges after 90 iterations"""
    S = _system(1, (4, 3, 3))
    P, b = S["P"], S["b"]
    ok, ou, _ = cr.cg(cr.operator(S["rp"], S["cl"], S["Au"], S["bc"]), np.array(b), kmax=100, rtol=1e-6)
    assert ok < 100
    with zzz.Context(0) as c:
        c.upload_part(P)
        c.vec_upload(zzz.VEC_B, b)
        c.vec_upload(zzz.VEC_U, np.zeros_like(b))
        k, rr, rr0 = c.cg_solve(variant=zzz.CG_CGH, pc=zzz.PC_NONE, op=zzz.OP_MATFREE, rtol=1e-6, max_it=100)
        u = c.vec_download(zzz.VEC_U)
    print(f"\nMF elasticity linalg::cg: {k} iterations (restatement {ok}), |u - ou| / |ou| {np.linalg.norm(u - ou) / np.linalg.norm(ou):.1e}")
    assert abs(k - ok) <= 2 and k < 100
    assert np.linalg.norm(u - ou) <= 1e-6 * np.linalg.norm(ou)


def test_jacobi_pcg_partitioned():
    """6. three z-slabs on one GPU (host-mailbox communicator): comm_halo_forward moves three values per node unchanged"""
    order, dims, nparts = 2, (3, 3, 6), 3
    G = zzz.Part("elasticity", order, *dims)
    with _env(**MF_SMALL), zzz.Context(0) as c0:
        c0.upload_part(G)
        c0.pattern_build()
        c0.assemble_vector(G.form)
        it0, _, _ = c0.cg_solve(pc=zzz.PC_JACOBI, op=zzz.OP_MATFREE, rtol=1e-8)
        u0 = c0.vec_download(zzz.VEC_U)
        d0 = c0.matfree_diagonal()
    grp = zzz.LocalGroup(nparts)
    out = [None] * nparts
    err = []

    def run(rank):
        try:
            P = zzz.Part("elasticity", order, *dims, nparts, rank)
            with zzz.Context(0) as c:
                c.comm_init_local(grp.h, rank)
                c.upload_part(P)
                c.upload_halo(P)
                c.pattern_build()
                c.assemble_vector(P.form)
                c.matfree_setup()
                ready.wait(timeout=120)  # every plan is built before a rank polls for the others (the build frees scratch buffers)
                it, rn, r0 = c.cg_solve(pc=zzz.PC_JACOBI, op=zzz.OP_MATFREE, rtol=1e-8)
                out[rank] = (it, P.own_offset, c.vec_download(zzz.VEC_U), c.matfree_diagonal())
        except Exception as e:  # noqa: BLE001
            err.append((rank, repr(e)))
            ready.abort()

    ready = threading.Barrier(nparts)
    with _env(**MF_SMALL):
        th = [threading.Thread(target=run, args=(r,)) for r in range(nparts)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
    grp.close()
    assert not err, err
    u = np.concatenate([o[2] for o in out])
    d = np.concatenate([o[3] for o in out])
    print(f"\nMF elasticity P{order} {dims} on {nparts} ranks: iterations {[o[0] for o in out]} / {it0}, "
          f"|u - u0| / |u0| {np.linalg.norm(u - u0) / np.linalg.norm(u0):.1e}")
    assert len({o[0] for o in out}) == 1 and abs(out[0][0] - it0) <= 2
    assert np.linalg.norm(u - u0) <= 1e-6 * np.linalg.norm(u0)
    assert np.abs(d - d0).max() <= 1e-12 * np.abs(d0).max()


def test_dirichlet_values():
    """7. u0 = g in closed form on the Dirichlet set: KSPCG + Jacobi on the matrix-free operator iterates on the lifted b with its
    constrained entries taken as zero and ends with u[bc] = g; the assembled solve of the lifted system is the reference"""
    S = _system(2, DIMS[2])
    P, bcb = S["P"], S["bc"].astype(bool)
    X = P.dof_x[:P.n_owned]
    g = (1e-3 * np.stack([1.0 + X[:, 0] + 2.0 * X[:, 1], 0.5 + X[:, 2] - 0.25 * X[:, 0] * X[:, 1], 0.25 + X[:, 1] * X[:, 2]], axis=1)).reshape(-1)
    with _env(**MF_SMALL), zzz.Context(0) as c:
        c.upload_part(P)
        c.pattern_build()
        c.upload_bc_values(g)
        c.assemble_vector(zzz.FORM_ELASTICITY)
        b = c.vec_download(zzz.VEC_B)
        it, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, op=zzz.OP_MATFREE, rtol=1e-10)
        u = c.vec_download(zzz.VEC_U)
        c.assemble_matrix(zzz.FORM_ELASTICITY)
        ita, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-10)
        ua = c.vec_download(zzz.VEC_U)
        np.testing.assert_array_equal(c.vec_download(zzz.VEC_B), b)  # the caller's b is untouched
    print(f"\nMF elasticity with values: {it} iterations (assembled {ita}), |u - ua| / |ua| {np.linalg.norm(u - ua) / np.linalg.norm(ua):.1e}")
    assert np.array_equal(b[bcb], g[bcb]) and np.abs(g[bcb]).min() > 0
    assert np.array_equal(u[bcb], g[bcb])
    assert np.linalg.norm(u - ua) <= 1e-6 * np.linalg.norm(ua)


@pytest.mark.parametrize("name,order", HE.CASES, ids=[f"{n}-P{o}" for n, o in HE.CASES])
def test_hostile_geometry_against_the_50_digit_reference(name, order):
    """8. many blocks (P3 on HE.DIMS: two); the bar of the other hostile tests, for the action and for the diagonal that Jacobi
    divides by entry by entry: figure(gpu) <= max(8 x figure(oracle), 32) units of 2^-53"""
    C = HE.case(name, order)
    u = np.random.default_rng(40 + order).standard_normal(C.n)
    y_ref, t_ref, ofig = HE.action_reference(C, u)
    d_ref, ds_ref, odfig = HE.diagonal_reference(C)
    bcb = C.bc.astype(bool)
    assert np.all(t_ref[~bcb] > 0) and np.all(ds_ref[~bcb] > 0)
    with _env(**MF_SMALL), zzz.Context(0) as c:
        _upload(c, C, None)
        c.matfree_setup()
        info = c.matfree_info()
        y = c.action(u)
        d = c.matfree_diagonal()
        np.testing.assert_array_equal(c.action(u), y)
        np.testing.assert_array_equal(c.matfree_diagonal(), d)
    fig = hp.metric(y, y_ref, t_ref) / hp.U  # (asks the constrained rows, scale 0, for the bits: 0.0)
    dfig = hp.metric(d, d_ref, ds_ref) / hp.U  # (... and for 1.0)
    print(f"\nHOSTILE MF elasticity {name:8s} P{order}: {info['blocks']} blocks, action gpu {fig:7.2f} oracle {ofig:7.2f}, "
          f"diagonal gpu {dfig:7.2f} oracle {odfig:7.2f}")
    assert info["blocks"] == -(-len(C.cells) // 128) and info["blocks"] >= 2 and info["shared_dofs"] > 0
    assert np.all(y[bcb] == 0.0) and np.all(d[bcb] == 1.0)
    assert fig <= _bar(ofig), (fig, ofig)
    assert dfig <= _bar(odfig), (dfig, odfig)


def test_what_stays_declined():
    """9. on a block-size-3 context with op = OP_MATFREE"""
    S = _system(1, DIMS[1])
    P = S["P"]
    with zzz.Context(0) as c:
        c.upload_part(P)
        c.pattern_build()
        c.assemble_matrix(zzz.FORM_ELASTICITY)
        c.assemble_vector(zzz.FORM_ELASTICITY)
        for bad in (dict(pc=zzz.PC_CHEBYSHEV_JACOBI), dict(single_reduction=True), dict(variant=zzz.CG_PIPE), dict(pc=zzz.PC_MG),
                    dict(pc=zzz.PC_PMG)):
            with pytest.raises(zzz.ZzzError) as e:
                c.cg_solve(op=zzz.OP_MATFREE, rtol=1e-8, **bad)
            assert e.value.code == 1, (bad, str(e.value))
        with pytest.raises(zzz.ZzzError, match="block size 3"):
            c.action_f32(np.zeros(3 * P.n_owned, np.float32))
        it, rn, r0 = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)  # the context is still usable
        oit, _, _, _ = zo.pcg(S["rp"], S["cl"], S["Ac"], S["b"], rtol=1e-8)
        assert abs(it - oit) <= 2 and rn <= 1e-8 * r0
