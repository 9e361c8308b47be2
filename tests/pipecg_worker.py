"""Worker of test_pipecg_partitioned_between_processes (tests/test_gpu_pipecg.py): one rank = one PROCESS, all on GPU 0,
each with its z-slab of one partitioned problem and a communicator that has NO transport but the peer memory
(zzz_comm_init_peer_only), as tests/p2p_worker.py's run_partition.  Between processes the mailbox all-reduce of the
pipelined CG runs on its own stream beside the halo exchange and the product: this is where a missing event shows."""
import os


def run(rank, nranks, conn, problem, order, dims, overlap, own_stream=True):
    try:
        os.environ["ZZZ_OVERLAP"] = "1" if overlap else "0"  # (both read when a context is created)
        os.environ["ZZZ_CG_PIPE_STREAM"] = "1" if own_stream else "0"
        import zzz

        P = zzz.Part(problem, order, *dims, nranks, rank)
        with zzz.Context(0) as c:
            c.comm_init_peer_only(nranks, rank)
            conn.send(c.comm_p2p_export())
            if not c.comm_p2p_attach(conn.recv()):
                conn.send(("disabled",))
                return
            c.upload_part(P)
            c.upload_halo(P)
            c.pattern_build()
            c.assemble_matrix(P.form)
            c.assemble_vector(P.form)
            out = []
            for _ in range(2):  # twice: the second solve meets the first one's streams, events and buffers
                it, rn, r0 = c.cg_solve(variant=zzz.CG_PIPE, pc=zzz.PC_JACOBI, rtol=1e-8)
                out.append((it, rn, r0, c.vec_download(zzz.VEC_U), c.cg_info()["allreduce_overlapped"]))
            conn.send(("ok", P.own_offset, out))
    except Exception as e:  # noqa: BLE001
        conn.send(("error", repr(e)))
