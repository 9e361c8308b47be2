#!/usr/bin/env python3
"""What -ksp_type pipecg (ZZZ_CG_PIPE) costs and saves against the two KSPCG forms, on ONE GPU.

  ab_pipecg.py c2    [--out FILE]                 BASELINE config C2 (10 M dofs) on one rank: `ZZZ Solve` and iterations of the
                                                  classical, single-reduction and pipelined forms in one process, in both orders
  ab_pipecg.py ranks [--forms sr,pipe] [--only SIZE] [--out FILE]
                                                  the per-rank sizes bench.py --full tracks (rank_sizes: C2's 2-, 4- and 8-GPU
                                                  slabs, C4's and C5's 8-GPU slabs) with the communication path attached as that
                                                  record attaches it (1-rank communicator, peer-memory mailboxes): us per
                                                  iteration of each form.  ZZZ_HIP_LIB=<another build's libzzz_hip.so> with
                                                  --forms classical,sr gives the figures of that build (the parent commit's) in
                                                  the same session.

One JSON record per run (stdout and --out).  On one GPU the all-reduce has no latency to hide: the `ranks` figures show the
launch-and-bytes side of the pipelined form only.  Whether it pays on real xGMI links cannot be measured on one GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zzz  # noqa: E402

CG_PIPE = getattr(zzz, "CG_PIPE", 2)
FORMS = {"classical": dict(variant=zzz.CG_PETSC), "sr": dict(variant=zzz.CG_PETSC, single_reduction=True),
         "pipe": dict(variant=CG_PIPE)}


def timed_solve(ctx, form):
    ctx.sync()
    t0 = time.perf_counter()
    it, rn, r0 = ctx.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8, max_it=10000, **FORMS[form])
    ctx.sync()
    return time.perf_counter() - t0, it, rn / r0


def measure(ctx, forms, rounds):
    """every form warmed once, then `rounds` passes over the forms, alternately in the given and in the reverse order"""
    for f in forms:
        ctx.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8, max_it=50, **FORMS[f])
    res = {f: [] for f in forms}
    for rnd in range(rounds):
        for f in (forms if rnd % 2 == 0 else forms[::-1]):
            res[f].append(timed_solve(ctx, f))
    out = {}
    for f in forms:
        t = np.array([a[0] for a in res[f]])
        it = res[f][0][1]
        out[f] = {"solve_ms_median": 1e3 * float(np.median(t)), "solve_ms_min": 1e3 * float(t.min()),
                  "solve_ms_all": [round(1e3 * float(x), 3) for x in t], "krylov_iterations": it,
                  "us_per_iteration": 1e6 * float(np.median(t)) / max(it, 1), "relative_residual_norm": res[f][0][2]}
    return out


def run_c2(forms):
    nx, ny, nz, r = zzz.mesh_size(10000000, True, 1, 1, 1)
    with zzz.Context(0) as ctx:
        info = ctx.cube_generate("poisson", 1, nx << r, ny << r, nz << r, 1, 0)
        ctx.pattern_build()
        ctx.assemble_matrix(zzz.FORM_POISSON)
        ctx.assemble_vector(zzz.FORM_POISSON)
        rec = measure(ctx, forms, 6)
        norms = {}
        for f in forms:
            ctx.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8, **FORMS[f])
            norms[f] = ctx.vec_norm(zzz.VEC_U)
        return {"what": "BASELINE C2 on one rank, no communicator", "dofs": int(info[0]), "forms": rec, "solution_norm": norms,
                "dinv_codes": ctx.cg_info()["dinv_codes"]}


def rank_meshes():
    """the meshes of bench.py's rank_sizes record"""
    lay = lambda n_, parts: -(-n_ // parts)  # noqa: E731 -- layers of the thickest z-slab
    m2 = zzz.mesh_size(10000000, True, 1, 1, 1)
    nx, ny, nz = (m2[i] << m2[3] for i in range(3))
    m4 = zzz.mesh_size(500000, False, 8, 3, 1)
    m5 = zzz.mesh_size(50000000, True, 1, 1, 3)
    return [("c3_n2", "poisson", 1, (nx, ny, lay(nz, 2))), ("c3_n4", "poisson", 1, (nx, ny, lay(nz, 4))),
            ("c3_n8", "poisson", 1, (nx, ny, lay(nz, 8))),
            ("c4_n8", "elasticity", 1, (m4[0] << m4[3], m4[1] << m4[3], lay(m4[2] << m4[3], 8))),
            ("c5_n8", "poisson", 3, (m5[0] << m5[3], m5[1] << m5[3], lay(m5[2] << m5[3], 8)))]


def run_ranks(forms, only=""):
    zzz.comm_load()
    out = {}
    for key, problem, order, mesh in rank_meshes():
        if only and key != only:
            continue
        form = zzz.FORM_ELASTICITY if problem == "elasticity" else zzz.FORM_POISSON
        with zzz.Context(0) as ctx:
            ctx.comm_init(1, 0, zzz.comm_unique_id())
            p2p = os.environ.get("ZZZ_P2P", "1") != "0" and ctx.comm_p2p_attach(ctx.comm_p2p_export())
            info = ctx.cube_generate(problem, order, *mesh, 1, 0)
            ctx.pattern_build()
            ctx.assemble_matrix(form)
            ctx.assemble_vector(form)
            rec = measure(ctx, forms, 4)
            overlapped = None
            if "pipe" in forms:
                ctx.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8, max_it=20, **FORMS["pipe"])
                overlapped = ctx.cg_info().get("allreduce_overlapped")
            out[key] = {"mesh": "x".join(str(m) for m in mesh) + " sub-cubes", "dofs": int(info[0]), "forms": rec,
                        "scalar_allreduce": "peer-memory mailboxes" if p2p else "ncclAllReduce",
                        "pipe_allreduce_on_its_own_stream": overlapped}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["c2", "ranks"])
    ap.add_argument("--forms", default="")
    ap.add_argument("--only", default="", help="ranks: this one size (c3_n2, c3_n4, c3_n8, c4_n8, c5_n8)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    forms = a.forms.split(",") if a.forms else (["classical", "sr", "pipe"] if a.mode == "c2" else ["sr", "pipe"])
    rec = {"tool": "ab_pipecg.py " + a.mode, "library": os.environ.get("ZZZ_HIP_LIB", "in-tree build"),
           "caveat": "one GPU: launches and bytes only; no link latency is there to hide, and no multi-GPU hardware run exists",
           "result": run_c2(forms) if a.mode == "c2" else run_ranks(forms, a.only)}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
