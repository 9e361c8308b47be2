"""GPU parity tests of -ksp_type pipecg (ZZZ_CG_PIPE, csrc/zzz_cg_pipe.hip): PETSc's KSPPIPECG through the C-ABI against its
numpy restatement (tests/_pipecg_ref.py, pinned on the CPU by tests/test_pipecg_ref.py) and against the classical solve.

Bars: the iteration count within IT_BAR = (measured rounding spread of the restatement, 1) + 2 of the restatement's;
initial norm 1e-12, solutions 1e-7 relative, final norm <= rtol x initial norm."""
import os
import subprocess
import threading

import numpy as np
import pytest

import zzz
import zzz_oracle as zo
from _pipecg_ref import CASES, IT_BAR, NORMS, pipecg_ref

pytestmark = pytest.mark.gpu

RTOL = 1e-9


class _Env:
    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _assembled(c, P):
    c.upload_part(P)
    c.pattern_build()
    c.assemble_matrix(P.form)
    c.assemble_vector(P.form)
    rp, cl, v = c.csr_download()
    return rp.astype(np.int64), cl, v, c.vec_download(zzz.VEC_B)


def _check_against_ref(c, rp, cl, v, b, pc, norm, label=""):
    """one pipelined solve on the assembled context against the restatement and the classical solve: the parity bars"""
    ito, uo, rno, r0o, _ = pipecg_ref(rp, cl, v, b, pc, norm, RTOL)
    it, rn, r0 = c.cg_solve(variant=zzz.CG_PIPE, pc=pc, norm=norm, rtol=RTOL)
    u = c.vec_download(zzz.VEC_U)
    hist = c.cg_history(it + 1)
    reason = c.cg_info()["reason"]
    itc, rnc, r0c = c.cg_solve(pc=pc, norm=norm, rtol=RTOL)
    uc = c.vec_download(zzz.VEC_U)
    res = np.linalg.norm(b - zo.spmv(rp, cl, v, u)) / np.linalg.norm(b)
    print(f"pipecg {label} pc {pc} norm {norm}: gpu {it}, restatement {ito}, classical {itc}; |u-uo|/|uo| "
          f"{np.linalg.norm(u - uo) / np.linalg.norm(uo):.2e}, |u-uc|/|uc| {np.linalg.norm(u - uc) / np.linalg.norm(uc):.2e}, "
          f"true residual {res:.2e}")
    assert abs(it - ito) <= IT_BAR
    assert abs(r0 - r0o) <= 1e-12 * r0o and rn <= RTOL * r0 and reason == 2
    assert hist.shape[0] == it + 1 and hist[0] == r0 and hist[-1] == rn
    assert np.linalg.norm(u - uo) <= 1e-7 * np.linalg.norm(uo)
    assert r0 == pytest.approx(r0c, rel=1e-13)
    assert np.linalg.norm(u - uc) <= 1e-7 * np.linalg.norm(uc)
    if norm == zzz.NORM_UNPRECONDITIONED:
        assert res <= 1.1e-9
    return it


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("problem,order,dims", CASES)
def test_pipecg_parity(problem, order, dims, norm):
    """the five cases of test_single_reduction_cg x the three norm types, PC_JACOBI; PC_NONE once per problem"""
    zo.set_num_threads(1)
    P = zzz.Part(problem, order, *dims)
    with zzz.Context(0) as c:
        rp, cl, v, b = _assembled(c, P)
        _check_against_ref(c, rp, cl, v, b, zzz.PC_JACOBI, norm, f"{problem} P{order} {dims}")
        if norm == zzz.NORM_PRECONDITIONED:
            _check_against_ref(c, rp, cl, v, b, zzz.PC_NONE, norm, f"{problem} P{order} {dims}")


@pytest.mark.parametrize("codes", [0, 2])
@pytest.mark.parametrize("form,problem,order,dims,knobs", [
    ("one-chunk stream", "poisson", 1, (20, 18, 22), dict(ZZZ_SELLP=2, ZZZ_SELLP_DICT=2)),
    ("block rows", "elasticity", 1, (20, 18, 22), dict(ZZZ_SELLP=2, ZZZ_SELLP_BLK=2)),
    ("block windows", "poisson", 3, (8, 7, 9), dict(ZZZ_SELLP=2, ZZZ_SELLP_BWIN=2)),
    ("generic stream", "poisson", 2, (8, 7, 9), dict(ZZZ_SELLP=2, ZZZ_SELLP_BWIN=0)),
    ("csr tiles", "poisson", 1, (12, 10, 14), dict(ZZZ_SELLP=0))])
def test_pipecg_on_every_product_form(form, problem, order, dims, knobs, codes):
    """n = A m runs on whatever form the matrix took (forced by the forms' knobs where size would decide), with the inverse
    diagonal as doubles (ZZZ_CG_DINV_CODES=0) and as 16-bit codes (2): same bars"""
    zo.set_num_threads(4)
    P = zzz.Part(problem, order, *dims)
    with _Env(ZZZ_CG_DINV_CODES=codes, **knobs):
        with zzz.Context(0) as c:
            rp, cl, v, b = _assembled(c, P)
            c.spmv(np.ones(P.n_owned * P.bs))  # (the form is settled by the first product at the latest)
            if form != "csr tiles":
                vi = c.spmv_values_info()
                got = vi["special_form"] or ("one-chunk stream" if vi["one_chunk_kernel"] else "generic stream")
                assert got == form, vi
            assert bool(c.spmv_info_raw()[5]) == (form != "csr tiles")
            _check_against_ref(c, rp, cl, v, b, zzz.PC_JACOBI, zzz.NORM_PRECONDITIONED, form)
            c.cg_solve(variant=zzz.CG_PIPE, pc=zzz.PC_JACOBI, rtol=RTOL)
            assert (c.cg_info()["dinv_codes"] > 0) == (codes == 2)


def _single_rank(problem, order, dims, rtol):
    G = zzz.Part(problem, order, *dims)
    with zzz.Context(0) as c0:
        _assembled(c0, G)
        it0, rn0, r00 = c0.cg_solve(variant=zzz.CG_PIPE, pc=zzz.PC_JACOBI, rtol=rtol)
        return it0, c0.vec_download(zzz.VEC_U)


PARTITIONS = [("poisson", 1, (10, 9, 12), 2), ("poisson", 1, (8, 8, 13), 4), ("poisson", 2, (5, 4, 9), 3),
              ("elasticity", 1, (5, 5, 8), 2)]


# the all-reduce through the communicator on every partition; through the mailboxes between contexts of ONE process on
# the two-rank ones (more spinning "ranks" of one process share its few hardware queues: those partitions take the
# mailboxes between processes, below)
_IN_PROCESS = [c + (False,) for c in PARTITIONS] + [c + (True,) for c in PARTITIONS if c[3] == 2]


@pytest.mark.parametrize("overlap", [1, 0], ids=["overlap", "no-overlap"])
@pytest.mark.parametrize("problem,order,dims,nparts,p2p", _IN_PROCESS)
def test_pipecg_partitioned_through_the_communicator(problem, order, dims, nparts, p2p, overlap):
    """nparts contexts of this process (one thread each) joined by the local communicator, as
    test_partitioned_solve_on_one_gpu: every rank reports the same count, within the bar of the single-rank pipelined solve,
    and the assembled solution is that solve's.  (In one process the all-reduce sits on the main stream, in the place of
    the sequence where the overlapped one begins: the local transport is host-synchronous, and mailbox kernels of one
    process must not wait for each other on extra streams.)"""
    zo.set_num_threads(1)
    it0, u0 = _single_rank(problem, order, dims, 1e-8)
    grp = zzz.LocalGroup(nparts)
    out, err = [None] * nparts, []
    handles = [None] * nparts
    bar = threading.Barrier(nparts)

    def run(rank):
        try:
            P = zzz.Part(problem, order, *dims, nparts, rank)
            with zzz.Context(0) as c:
                c.comm_init_local(grp.h, rank)
                if p2p:
                    handles[rank] = c.comm_p2p_export()
                    bar.wait()
                    assert c.comm_p2p_attach(b"".join(handles)), "peer-memory all-reduce refused on one GPU"
                if rank % 2 == 0:
                    c.upload_part(P)
                    c.upload_halo(P)
                else:
                    c.cube_generate(problem, order, *dims, nparts, rank)
                c.pattern_build()
                c.assemble_matrix(P.form)
                c.assemble_vector(P.form)
                assert bool(c.comm_info()["peer_memory_allreduce"]) == p2p
                it, rn, r0 = c.cg_solve(variant=zzz.CG_PIPE, pc=zzz.PC_JACOBI, rtol=1e-8)
                assert not c.cg_info()["allreduce_overlapped"]
                out[rank] = (it, rn, r0, P.own_offset, c.vec_download(zzz.VEC_U))
        except Exception as e:  # noqa: BLE001
            err.append((rank, repr(e)))

    with _Env(ZZZ_OVERLAP=overlap):
        th = [threading.Thread(target=run, args=(r,)) for r in range(nparts)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=300)
    grp.close()
    assert not err, err
    assert all(o is not None for o in out)
    its = {o[0] for o in out}
    print(f"pipecg {problem} P{order} {dims} on {nparts} ranks ({'mailboxes' if p2p else 'communicator'}, overlap {overlap}): "
          f"{sorted(its)}, one rank {it0}")
    assert len(its) == 1 and abs(its.pop() - it0) <= IT_BAR
    assert [o[3] for o in out] == sorted(o[3] for o in out)
    u = np.concatenate([o[4] for o in out])
    assert u.shape == u0.shape and np.linalg.norm(u - u0) <= 1e-7 * np.linalg.norm(u0)
    for o in out:
        assert o[1] == out[0][1] and o[2] == out[0][2] and o[1] <= 1e-8 * o[2]


@pytest.mark.parametrize("overlap,own_stream", [(1, True), (0, True), (1, False)], ids=["overlap", "no-overlap", "allreduce-on-main-stream"])
@pytest.mark.parametrize("problem,order,dims,nparts", PARTITIONS)
def test_pipecg_partitioned_between_processes(problem, order, dims, nparts, overlap, own_stream):
    """The same partitions with one PROCESS per rank on this GPU and the peer-memory mailboxes as the only transport (the
    production all-reduce kernel, the halo through the peer windows): here the all-reduce runs on its own stream beside the
    halo exchange and the product, and the next update waits for its event -- a missing event shows as a wrong count or a
    stale sum.  Two solves per rank.  ZZZ_CG_PIPE_STREAM=0 (the A/B knob) keeps it on the main stream: same results."""
    import multiprocessing as mp

    import pipecg_worker

    zo.set_num_threads(1)
    it0, u0 = _single_rank(problem, order, dims, 1e-8)
    mpx = mp.get_context("spawn")
    pipes = [mpx.Pipe() for _ in range(nparts)]
    procs = [mpx.Process(target=pipecg_worker.run, args=(r, nparts, pipes[r][1], problem, order, dims, overlap, own_stream))
             for r in range(nparts)]
    for p in procs:
        p.start()
    try:
        handles = []
        for r in range(nparts):
            assert pipes[r][0].poll(180), "worker did not export a handle"
            handles.append(pipes[r][0].recv())
            assert isinstance(handles[-1], bytes) and len(handles[-1]) == zzz.P2P_HANDLE_BYTES, handles[-1]
        for r in range(nparts):
            pipes[r][0].send(b"".join(handles))
        out = []
        for r in range(nparts):
            assert pipes[r][0].poll(240), "worker hung"
            out.append(pipes[r][0].recv())
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for o in out:
        assert o[0] == "ok", o
    assert [o[1] for o in out] == sorted(o[1] for o in out)
    for k in range(2):
        its = {o[2][k][0] for o in out}
        print(f"pipecg {problem} P{order} {dims} on {nparts} processes (mailboxes, overlap {overlap}, own stream {own_stream}), solve {k}: {sorted(its)}, "
              f"one rank {it0}")
        assert len(its) == 1 and abs(its.pop() - it0) <= IT_BAR
        u = np.concatenate([o[2][k][3] for o in out])
        assert u.shape == u0.shape and np.linalg.norm(u - u0) <= 1e-7 * np.linalg.norm(u0)
        assert all(o[2][k][4] == own_stream for o in out), "the all-reduce must have run on its own stream here, and only there"
        for o in out:
            assert o[2][k][1] == out[0][2][k][1] and o[2][k][2] == out[0][2][k][2] and o[2][k][1] <= 1e-8 * o[2][k][2]


def test_pipecg_limits_and_refusals():
    """max_it, dtol, the zero right-hand side, the refused combinations, and a second solve after a re-assembly"""
    P = zzz.Part("poisson", 1, 6, 6, 6)
    with zzz.Context(0) as c:
        _assembled(c, P)
        b = c.vec_download(zzz.VEC_B)
        it, rn, r0 = c.cg_solve(variant=zzz.CG_PIPE, pc=zzz.PC_JACOBI, rtol=1e-14, max_it=3)
        assert it == 3 and c.cg_info()["reason"] == -3 and c.cg_history(4).shape[0] == 4
        itc, rnc, _ = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-14, max_it=3)
        assert itc == 3 and rn == pytest.approx(rnc, rel=1e-9)
        with pytest.raises(zzz.ZzzError, match="KSP_DIVERGED_ITS"):
            c.cg_solve(variant=zzz.CG_PIPE, pc=zzz.PC_JACOBI, rtol=1e-14, max_it=3, error_if_not_converged=True)
        # KSPConvergedDefault's divergence test: norm >= dtol x initial norm (true at iteration 0 with dtol = 0.5)
        it, rn, r0 = c.cg_solve(variant=zzz.CG_PIPE, pc=zzz.PC_JACOBI, rtol=1e-8, dtol=0.5)
        assert c.cg_info()["reason"] == -4 and rn >= 0.5 * r0
        with pytest.raises(zzz.ZzzError, match="KSP_DIVERGED_DTOL"):
            c.cg_solve(variant=zzz.CG_PIPE, pc=zzz.PC_JACOBI, rtol=1e-8, dtol=0.5, error_if_not_converged=True)
        # zero right-hand side: converged at iteration 0 (0 <= atol), u = 0
        c.vec_upload(zzz.VEC_B, np.zeros_like(b))
        it, rn, r0 = c.cg_solve(variant=zzz.CG_PIPE, pc=zzz.PC_JACOBI, rtol=1e-8)
        assert it == 0 and rn == 0.0 and np.all(c.vec_download(zzz.VEC_U) == 0.0) and c.cg_info()["reason"] > 0
        c.vec_upload(zzz.VEC_B, b)
        for bad in (dict(op=zzz.OP_MATFREE), dict(pc=zzz.PC_CHEBYSHEV_JACOBI), dict(single_reduction=True)):
            with pytest.raises(zzz.ZzzError, match="pipecg"):
                c.cg_solve(variant=zzz.CG_PIPE, **bad)
        with pytest.raises(zzz.ZzzError):
            c.cg_solve(variant=3)
        # buffers reused, not stale: the same solve before and after a re-assembly, bit for bit
        it1, rn1, r01 = c.cg_solve(variant=zzz.CG_PIPE, pc=zzz.PC_JACOBI, rtol=RTOL)
        u1 = c.vec_download(zzz.VEC_U)
        c.assemble_matrix(P.form)
        c.assemble_vector(P.form)
        it2, rn2, r02 = c.cg_solve(variant=zzz.CG_PIPE, pc=zzz.PC_JACOBI, rtol=RTOL)
        assert (it2, rn2, r02) == (it1, rn1, r01)
        np.testing.assert_array_equal(c.vec_download(zzz.VEC_U), u1)


def _driver(args):
    exe = os.path.join(zzz.PKG, "dolfinx-scaling-test")
    o = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert o.returncode == 0, o.stderr
    return (int(o.stdout.split("*** Number of Krylov iterations: ")[1].split()[0]),
            float(o.stdout.split("*** Solution norm:  ")[1].split()[0]), o.stdout)


@pytest.mark.parametrize("ranks", [[], ["--ngpus", "2", "--comm", "local"]], ids=["one-rank", "two-ranks-local"])
def test_pipecg_through_the_driver(ranks):
    base = ["--problem_type", "poisson", "--scaling_type", "strong", "--ndofs", "50000", "-pc_type", "jacobi", "-ksp_rtol", "1e-8",
            "-ksp_view"] + ranks
    it_cg, nrm_cg, text_cg = _driver(base + ["-ksp_type", "cg"])
    it, nrm, text = _driver(base + ["-ksp_type", "pipecg"])
    print(f"driver {ranks}: cg {it_cg} iterations |u| {nrm_cg!r}, pipecg {it} iterations |u| {nrm!r}")
    assert "type: pipecg" in text and "type: cg" in text_cg
    assert abs(it - it_cg) <= IT_BAR and abs(nrm - nrm_cg) <= 1e-6 * nrm_cg
    exe = os.path.join(zzz.PKG, "dolfinx-scaling-test")
    for bad in (["--operator", "matfree"], ["-ksp_cg_single_reduction"], ["-pc_type", "chebyshev_jacobi"]):
        o = subprocess.run([exe] + base + ["-ksp_type", "pipecg"] + bad, capture_output=True, text=True, timeout=60)
        assert o.returncode != 0 and "-ksp_type pipecg" in (o.stderr + o.stdout), (bad, o.stderr)
