"""The matrix-free elasticity operator (block size 3, csrc/zzz_matfree.hip: k_mf_action3, k_mf_finish3) under every plan shape
and in every instantiation: ND in {4, 10, 20} x T in {128, 256, 512} x {action, diagonal}, one and several steps per block
(nsb = cells_per_block / threads), the LDS retry of mf_plan_build and its refusal, dynamic LDS beyond 48 KiB, non-finite
input, the action on three ranks.  tests/test_gpu_mf_elasticity.py runs all but one of its cases at T = NC = 128.

REFERENCE AND BAR.  On the cubes the reference is the oracle's UNCONSTRAINED matrix Au (HE.oracle_system), judged per row
(HE.oracle_figures), in units of 2^-53:

    action    |y_i - (Au v)_i| / sum_j |Au_ij| |v_j|      constrained rows: the bits 0.0
    diagonal  |d_i - Au_ii| / Au_ii                       constrained rows: the bits 1.0

    bar = max(8 o, 32) + o

max(8 o, 32) is what the project grants a kernel against the TRUTH (_hostile_gpu._bar) and o is how far the oracle itself is
from the truth: its own figure against the 50-digit reference on the undistorted cube H.case("identity", order, "elasticity"),
measured once on a CPU with

    PYTHONPATH=oracle:tests:performance-test_amd python -c "import _hostile_mf_elasticity as HE; print(HE.oracle_constants())"
    {1: (0.3771, 1.1629), 2: (0.3780, 1.7737), 3: (0.3256, 1.7230)}            (order: (action, diagonal))

and kept, rounded up, as HE.O_ACTION = 0.38 / 0.38 / 0.33 and HE.O_DIAGONAL = 1.17 / 1.78 / 1.73: bars of 32.4 and 33.2 .. 33.8
units.  A wrong instantiation -- a missed barrier, a flag read for the wrong component, a node of another block -- is off by
O(1) of the row's scale, 1e15 units.  (A cell-by-cell sum in doubles in a random cell order, on a CPU, is 3.7 .. 5.9 units from
the oracle's matrix on these meshes for the action and 3.1 .. 4.9 for the diagonal.)  Largest figures seen on an MI355X over all
cases below: action 5.33 / 4.53 / 5.96 at P1 / P2 / P3, diagonal 7.44 / 6.20 / 9.98 (the three-rank P3 case).

All plans here are built with the caller's cell order kept (ZZZ_RENUMBER=0), so that H.plan_blocks restates the blocks
exactly: the node counts asserted below are computed on the host, none is written down.  LDS per node at block size 3: 72 B
(P1), 48 B (P2), 24 B (P3), i.e. 910 / 1365 / 2730 nodes in the 64 KiB a block may take.
"""
import threading

from _gpu_helpers import *  # noqa: F401,F403 -- helpers, np / os / zzz / zo / pytest
import _hostile as H
import _hostile_mf_elasticity as HE
from _hostile_gpu import MF_SMALL, _bar, _env, _upload

pytestmark = pytest.mark.gpu  # noqa: F405

LDS_PER_NODE = {1: 72, 2: 48, 3: 24}  # lds_per_dof(nd, 3)
NC_DEFAULT = {1: 1024, 2: 512, 3: 256}  # mf_plan_build, block size 3
_CUBES = {}


def _nloc_limit(order):
    return 65536 // LDS_PER_NODE[order]


def _cube(order, dims):
    """zo.Problem("elasticity", order, *dims) as a H.Case (mesh, dofmap and Dirichlet set as the oracle numbers them), with the
    oracle's unconstrained matrix next to it"""
    key = (order, tuple(dims))
    if key not in _CUBES:
        zo.set_num_threads(1)
        O = zo.Problem("elasticity", order, *dims)
        C = H.Case()
        C.name, C.order, C.problem, C.dims, C.bs, C.form, C.nblock, C.n = "cube", order, "elasticity", tuple(dims), 3, O.form, O.nblock, O.n
        C.x, C.cells, C.cell_dofs, C.bc, C.f, C.g, C.facets = O.x, O.cells, O.cell_dofs, O.bc, O.f, None, None
        C.rowptr, C.cols, C.Au, C.diag = HE.oracle_system(order, C.x, C.cells, C.cell_dofs, C.nblock)
        for a in (C.x, C.cells, C.cell_dofs, C.bc, C.Au, C.diag):
            a.setflags(write=False)
        _CUBES[key] = C
    return _CUBES[key]


def _expected_nc(C, nc, T):
    """mf_plan_build's retry restated: halve while the largest block touches more nodes than LDS holds (None: refused)"""
    while max(H.plan_blocks(C, nc)) > _nloc_limit(C.order):
        if nc // 2 < T or (nc // 2) % T:
            return None
        nc //= 2
    return nc


def _bars(order):
    return _bar(HE.O_ACTION[order]) + HE.O_ACTION[order], _bar(HE.O_DIAGONAL[order]) + HE.O_DIAGONAL[order]


def _action_and_diagonal(c, C, v, tag):
    """the plan in place: action and diagonal against the bar, exact constrained rows, a second pass with the same bits"""
    info = c.matfree_info()
    bcb = C.bc.astype(bool)
    y = c.action(v)
    d = c.matfree_diagonal()
    fy, fd = HE.oracle_figures(C.rowptr, C.cols, C.Au, C.diag, C.bc, v, y, d)  # (asks the constrained rows for 0.0 and 1.0)
    by, bd = _bars(C.order)
    print(f"\nMF3 {tag} P{C.order} {C.dims}: {info['blocks']} x {info['cells_per_block']} cells, {info['threads']} threads, nloc_max "
          f"{info['nloc_max']} ({LDS_PER_NODE[C.order] * info['nloc_max']} B), {info['shared_dofs']} shared | action {fy:.2f} "
          f"(bar {by:.2f}) diagonal {fd:.2f} (bar {bd:.2f})")
    assert fy <= by and fd <= bd, (fy, by, fd, bd)
    assert np.all(y[bcb] == 0.0) and np.all(d[bcb] == 1.0)
    np.testing.assert_array_equal(c.action(v), y)
    np.testing.assert_array_equal(c.matfree_diagonal(), d)
    return y, d, info


def _check_plan(info, C, T, nc):
    nodes = H.plan_blocks(C, nc)
    assert info["valid"] == 1 and info["threads"] == T and info["cells_per_block"] == nc, info
    assert info["blocks"] == len(nodes) == -(-len(C.cells) // nc), (info, len(nodes))
    assert info["nloc_max"] == max(nodes) <= _nloc_limit(C.order), (info, max(nodes))
    assert info["blocks"] == 1 or info["shared_dofs"] > 0, info


# (order, dims, threads, ZZZ_MF_NC): none of these plans needs the retry
SWEEP = ([(1, (8, 8, 8), T, k * T) for T in (128, 256, 512) for k in (1, 4)]  # 3072 cells: 24 .. 2 blocks, nsb 1 and 4
         + [(2, (5, 5, 5), T, k * T) for T in (128, 256, 512) for k in (1, 2)]  # 750 cells: 6 .. 1 blocks, nsb 1 and 2
         + [(2, (5, 5, 5), 256, 1024),  # ONE block of all 1331 nodes (1365 fit), nsb 4, 63 888 B: hipFuncSetAttribute
            (3, (3, 3, 5), 128, 128), (3, (3, 3, 5), 128, 256),  # 270 cells: three and two blocks, nsb 1 and 2
            (3, (5, 5, 5), 256, 256),  # the shipped default: three blocks
            (3, (4, 4, 5), 512, 512)])  # ONE partial block (480 cells) of all 2704 nodes (2730 fit): 64 896 B + the tables' 9.7 KB


@pytest.mark.parametrize("order,dims,T,nc", SWEEP, ids=[f"P{o}-{'x'.join(map(str, d))}-T{T}-NC{nc}" for o, d, T, nc in SWEEP])
def test_every_instantiation_one_and_several_steps_per_block(order, dims, T, nc):
    """1. k_mf_action3<ND, T, DIAG> for every ND and T, with nsb = nc / T = 1 and > 1 (the `for s` loop, its `if (s == 0)`
    barrier and the per-step rmax words), on several blocks (k_mf_finish3) and on one, with dynamic LDS below and above 48 KiB"""
    C = _cube(order, dims)
    assert _expected_nc(C, nc, T) == nc  # no retry
    v = np.random.default_rng(100 + order).standard_normal(C.n)
    with _env(ZZZ_MF_T=T, ZZZ_MF_NC=nc), zzz.Context(0) as c:
        _upload(c, C, "0")
        c.matfree_setup()
        _, _, info = _action_and_diagonal(c, C, v, "sweep")
    _check_plan(info, C, T, nc)


def test_1024_threads_fall_back_to_256():
    """1. block size 3 has no instantiation for 1024 threads: ZZZ_MF_T=1024 is not taken and the plan runs on the default"""
    C = _cube(2, (5, 5, 5))
    v = np.random.default_rng(102).standard_normal(C.n)
    with _env(ZZZ_MF_T=1024, ZZZ_MF_NC=None), zzz.Context(0) as c:
        _upload(c, C, "0")
        c.matfree_setup()
        _, _, info = _action_and_diagonal(c, C, v, "T=1024")
    _check_plan(info, C, 256, NC_DEFAULT[2])


@pytest.mark.parametrize("order,dims,nc,halvings", [(1, (10, 10, 10), 8192, 2), (2, (6, 6, 6), 1024, 1), (3, (5, 5, 5), 512, 1)],
                         ids=["P1-10x10x10-NC8192", "P2-6x6x6-NC1024", "P3-5x5x5-NC512"])
def test_plan_retry_at_block_size_3(order, dims, nc, halvings):
    """2. a block of ZZZ_MF_NC cells touches more nodes than 64 KiB hold at 72 / 48 / 24 B each: the plan halves its blocks
    until they fit and stops at the FIRST size that does (restated on the host), T = 256"""
    C = _cube(order, dims)
    want = _expected_nc(C, nc, 256)
    assert want == nc >> halvings, (want, [max(H.plan_blocks(C, nc >> k)) for k in range(halvings + 1)])
    v = np.random.default_rng(110 + order).standard_normal(C.n)
    with _env(ZZZ_MF_T=256, ZZZ_MF_NC=nc), zzz.Context(0) as c:
        _upload(c, C, "0")
        c.matfree_setup()
        _, _, info = _action_and_diagonal(c, C, v, f"retry from {nc}")
    _check_plan(info, C, 256, want)


def test_refusal_at_block_size_3_leaves_the_context_usable():
    """2. P3 5 x 5 x 5 with ZZZ_MF_T=512: a 512-cell block touches 3066 nodes, 2730 fit, and a block cannot be smaller than the
    workgroup: include/zzz_abi.h promises ZZZ_ERR_LIMIT (5) from every entry that needs the plan -- decided on the host, before
    any kernel of the action runs -- and a context that goes on working: the same calls succeed once the knob is gone, and the
    assembled solve never minded."""
    C = _cube(3, (5, 5, 5))
    assert _expected_nc(C, 512, 512) is None and max(H.plan_blocks(C, 512)) > _nloc_limit(3)
    zo.set_num_threads(1)
    Ac = zo.assemble_matrix(C.form, 3, C.x, C.cells, C.cell_dofs, C.bc, C.rowptr, C.cols)
    b = zo.assemble_vector(C.form, 3, C.x, C.cells, C.cell_dofs, C.f, None, None, C.bc)
    oit, ou, _, _ = zo.pcg(C.rowptr, C.cols, Ac, b, rtol=1e-8)
    rng = np.random.default_rng(120)
    v, mark = rng.standard_normal(C.n), rng.standard_normal(C.n)
    with zzz.Context(0) as c:
        _upload(c, C, "0")
        c.vec_upload(zzz.VEC_B, b)
        with _env(ZZZ_MF_T=512, ZZZ_MF_NC=None):
            refused = [("matfree_setup", c.matfree_setup), ("action", lambda: c.action(v)), ("matfree_diagonal", c.matfree_diagonal),
                       ("cg_solve jacobi", lambda: c.cg_solve(pc=zzz.PC_JACOBI, op=zzz.OP_MATFREE, rtol=1e-8)),
                       ("cg_solve none", lambda: c.cg_solve(pc=zzz.PC_NONE, op=zzz.OP_MATFREE, rtol=1e-8))]
            for what, call in refused:
                c.vec_upload(zzz.VEC_U, mark)
                with pytest.raises(zzz.ZzzError) as e:
                    call()
                print(f"\nMF3 refusal, {what}: {e.value}")
                assert e.value.code == 5 and "24 B per dof" in str(e.value), (what, str(e.value))
                assert c.matfree_info()["valid"] == 0
                np.testing.assert_array_equal(c.vec_download(zzz.VEC_U), mark, err_msg=what)  # u is untouched
        with _env(ZZZ_MF_T=None, ZZZ_MF_NC=None):
            c.matfree_setup()
            _, _, info = _action_and_diagonal(c, C, v, "after the refusal")
            _check_plan(info, C, 256, NC_DEFAULT[3])
            itm, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, op=zzz.OP_MATFREE, rtol=1e-8)
            um = c.vec_download(zzz.VEC_U)
        c.pattern_build()
        c.assemble_matrix(C.form)
        c.assemble_vector(C.form)
        it, _, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)
        ua = c.vec_download(zzz.VEC_U)
    print(f"\nMF3 refusal: afterwards Jacobi-CG assembled {it}, matrix-free {itm}, oracle {oit} iterations")
    assert abs(it - oit) <= 2 and np.linalg.norm(ua - ou) <= 1e-6 * np.linalg.norm(ou)
    assert abs(itm - oit) <= 2 and np.linalg.norm(um - ou) <= 1e-6 * np.linalg.norm(ou)


@pytest.mark.parametrize("poison", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("name,order", [("identity", 1), ("graded", 2), ("offset", 3)])
def test_a_non_finite_input_stays_with_its_cells(name, order, poison):
    """3. include/zzz_abi.h (zzz_action) at block size 3: a non-finite x[3 n + c] at an unconstrained node n makes y[3 n + c]
    non-finite, reaches no scalar dof of a node that shares no cell with n -- those keep the bits of the clean action -- and no
    constrained row (0.0); the next clean action gives the clean bits again.

    P1: EVERY unconstrained scalar dof of every node that shares a cell with n is non-finite.  mf_el_element_p1 forms the
    displacement gradient H[c][.] = sum_k u_k[c] grad phi_k[.] of the cell, which is non-finite in row c; the trace
    H[0][0] + H[1][1] + H[2][2] contains H[c][c] and lambda tr(eps) is added to the whole diagonal of sigma, so sigma[a][a] is
    non-finite for a = 0, 1, 2; and ye[k][a] = |det J| sum_b sigma[a][b] grad phi_k[b] contains sigma[a][a] grad phi_k[a], which
    is non-finite whatever the finite factor (0 x inf is NaN).  A sum with a non-finite term is non-finite.

    P3 runs on HE.DIMS (two blocks): u is then gathered from memory through gid."""
    C = HE.case(name, order)
    bcb = C.bc.astype(bool)
    nbc = bcb.reshape(-1, 3).any(axis=1)  # (the cube's Dirichlet set holds whole nodes)
    assert np.array_equal(np.repeat(nbc, 3), bcb)
    u = np.random.default_rng(130 + order).standard_normal(C.n)
    # an interior node next to the boundary: of the unconstrained nodes that share a cell with a constrained one, the one that
    # meets most cells (lowest number among equals)
    beside = np.zeros(C.nblock, bool)
    beside[C.cell_dofs[nbc[C.cell_dofs].any(1)].reshape(-1)] = True
    meets = np.bincount(C.cell_dofs.reshape(-1), minlength=C.nblock) * (beside & ~nbc)
    n = int(np.argmax(meets))
    near = np.zeros(C.nblock, bool)
    near[C.cell_dofs[(C.cell_dofs == n).any(1)].reshape(-1)] = True
    assert near.sum() > 4 and (~near).sum() > 4 and (near & nbc).any() and not nbc[n]
    near3 = np.repeat(near, 3)
    with _env(**MF_SMALL), zzz.Context(0) as c:
        _upload(c, C, None)
        clean = c.action(u)
        assert c.matfree_info()["blocks"] >= 2
        assert np.all(np.isfinite(clean)) and np.all(clean[bcb] == 0.0)
        for comp in range(3):
            up = u.copy()
            up[3 * n + comp] = poison
            dirty = c.action(up)
            print(f"\nMF3 {poison} at node {n} component {comp} of {name} P{order}: {np.count_nonzero(~np.isfinite(dirty))} entries not "
                  f"finite, {int(near.sum())} nodes share a cell with it ({int((near & ~nbc).sum())} unconstrained)")
            assert not np.isfinite(dirty[3 * n + comp])
            np.testing.assert_array_equal(dirty[~near3], clean[~near3])
            assert np.all(dirty[bcb] == 0.0)
            if order == 1:
                assert not np.isfinite(dirty[near3 & ~bcb]).any()
            np.testing.assert_array_equal(c.action(u), clean)  # nothing lingers in the context


@pytest.mark.parametrize("order", [1, 2, 3])
def test_action_partitioned(order):
    """4. three z-slabs of the 3 x 3 x 6 cube on one GPU (host-mailbox communicator): every rank applies the operator to its
    owned part of one vector; ghost nodes get their three values from the exchange (P3: read through gid straight from the
    exchanged vector).  The ranks' results side by side against the oracle's matrix of the WHOLE cube, per row; two collective
    actions give the same bits.  Every rank builds its plan before any rank enters a collective (the build frees scratch buffers)."""
    dims, nparts = (3, 3, 6), 3
    G = zzz.Part("elasticity", order, *dims)
    rp, cl, Au, diag = HE.oracle_system(order, G.x, G.cells, G.cell_dofs, G.n_owned)
    bc = G.bc_marker()
    v = np.random.default_rng(140 + order).standard_normal(3 * G.n_owned)
    grp = zzz.LocalGroup(nparts)
    out = [None] * nparts
    err = []

    def run(rank):
        try:
            P = zzz.Part("elasticity", order, *dims, nparts, rank)
            assert np.array_equal(P.global_dofs[:P.n_owned], P.own_offset + np.arange(P.n_owned))
            mine = v[3 * P.own_offset:3 * (P.own_offset + P.n_owned)]
            with zzz.Context(0) as c:
                c.comm_init_local(grp.h, rank)
                c.upload_part(P)
                c.upload_halo(P)
                c.matfree_setup()
                ready.wait(timeout=120)
                y = c.action(mine)
                d = c.matfree_diagonal()
                y2 = c.action(mine)
                out[rank] = (P.own_offset, P.n_ghost, c.matfree_info(), y, d, y2, c.matfree_diagonal())
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
    assert [o[0] for o in out] == sorted(o[0] for o in out) and all(o[1] > 0 for o in out)  # rank order; every rank has ghosts
    y, d = np.concatenate([o[3] for o in out]), np.concatenate([o[4] for o in out])
    assert y.shape == v.shape
    fy, fd = HE.oracle_figures(rp, cl, Au, diag, bc, v, y, d)
    by, bd = _bars(order)
    print(f"\nMF3 P{order} {dims} on {nparts} ranks: blocks {[o[2]['blocks'] for o in out]}, ghosts {[o[1] for o in out]} | action {fy:.2f} "
          f"(bar {by:.2f}) diagonal {fd:.2f} (bar {bd:.2f})")
    assert fy <= by and fd <= bd
    bcb = bc.astype(bool)
    assert np.all(y[bcb] == 0.0) and np.all(d[bcb] == 1.0)
    for o in out:
        np.testing.assert_array_equal(o[5], o[3])
        np.testing.assert_array_equal(o[6], o[4])
