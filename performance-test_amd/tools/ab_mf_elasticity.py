#!/usr/bin/env python3
"""The matrix-free elasticity operator against the assembled path, on ONE GPU.

  ab_mf_elasticity.py [--configs el_p1_c4,el_p2_2m,el_p3_1m] [--rounds 3] [--paths matfree,assembled] [--out FILE]
  ab_mf_elasticity.py --child matfree|assembled --config NAME      one measurement in this process, one JSON line (internal)

Configurations: elasticity P1 at the 1.33 M nodes of bench.py's C4 (4 M dofs), P2 at 2 M dofs, P3 at 1 M dofs.  Every
(configuration, path) runs in a FRESH child process -- its own context, plan and clocks -- `rounds` times, the paths in
alternating order.  A child reports

  matfree    action ms (zzz_action_time, 20 launches with the <p, y> partials), the bytes one action addresses
             (zzz_matfree_info), Gdof/s of linalg::cg(u, b, action, 100, 1e-6) as the driver prints it, ms per iteration of
             KSPCG + Jacobi on the matrix-free operator (rtol 1e-8, at most 200 iterations), and the whole step: plan +
             diagonal + that solve;
  assembled  the product ms (zzz_spmv_time), ms per iteration of the same Jacobi solve on the matrix, and the whole step:
             pattern + matrix + block form + solve.

Both steps include the right-hand side's assembly outside the clock (it needs the dof -> cell adjacency either way).
ZZZ_HIP_LIB=<another build's libzzz_hip.so> --paths assembled gives that build's assembled figures (the parent commit's: they
must not move).  ZZZ_MF_NC / ZZZ_MF_T reach the child: `--paths matfree --rounds 1` under them is the block-size sweep
(tools/mf_el_sweep.sh).  One JSON record (stdout and --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zzz  # noqa: E402

CONFIGS = {"el_p1_c4": (1, 4000000), "el_p2_2m": (2, 2000000), "el_p3_1m": (3, 1000000)}
JAC = dict(pc=zzz.PC_JACOBI, rtol=1e-8, max_it=200)
CGH = dict(variant=zzz.CG_CGH, pc=zzz.PC_NONE, op=zzz.OP_MATFREE, rtol=1e-6, max_it=100)


def _timed(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    r = fn()
    ctx.sync()
    return time.perf_counter() - t0, r


def child(path, config, ndofs=0):
    order, nd = CONFIGS[config]
    nx, ny, nz, r = zzz.mesh_size(ndofs or nd, True, 1, 3, order)
    with zzz.Context(0) as ctx:
        info = ctx.cube_generate("elasticity", order, nx << r, ny << r, nz << r, 1, 0)
        n = int(info[0])
        rec = {"path": path, "config": config, "dofs": n}
        if path == "matfree":
            t_plan, _ = _timed(ctx, ctx.matfree_setup)
            ctx.pattern_build()  # (for the right-hand side alone: not in the step)
            ctx.assemble_vector(zzz.FORM_ELASTICITY)
            steps, its = [], 0
            for k in range(3):
                t, (its, _, _) = _timed(ctx, lambda: ctx.cg_solve(op=zzz.OP_MATFREE, **JAC))  # PCSetUp (the diagonal) inside
                steps.append(t)
            cgs = []
            for k in range(3):
                ctx.vec_upload(zzz.VEC_U, np.zeros(n))
                t, (itc, _, _) = _timed(ctx, lambda: ctx.cg_solve(**CGH))
                cgs.append(t)
            act = [ctx.action_time(20) for _ in range(3)]
            plan = ctx.matfree_info()
            tj = float(np.median(steps[1:]))
            rec.update(action_ms=float(np.median(act)), bytes_per_action=plan["bytes_per_action"], cells_per_block=plan["cells_per_block"],
                       threads=plan["threads"], blocks=plan["blocks"], nloc_max=plan["nloc_max"], shared_nodes=plan["shared_dofs"],
                       plan_ms=1e3 * t_plan, jacobi_iterations=its, jacobi_ms_per_iteration=1e3 * tj / max(its, 1),
                       cgh_iterations=itc, Gdof_per_s=itc * n / float(np.median(cgs[1:])) / 1e9,
                       step_ms=1e3 * (t_plan + steps[0]), solution_norm=ctx.vec_norm(zzz.VEC_U))
        else:
            t_pat, _ = _timed(ctx, ctx.pattern_build)
            t_mat, _ = _timed(ctx, lambda: ctx.assemble_matrix(zzz.FORM_ELASTICITY))  # (with the product's block form)
            ctx.assemble_vector(zzz.FORM_ELASTICITY)
            steps, its = [], 0
            for k in range(3):
                t, (its, _, _) = _timed(ctx, lambda: ctx.cg_solve(**JAC))
                steps.append(t)
            prod = [ctx.spmv_time(20) for _ in range(3)]
            tj = float(np.median(steps[1:]))
            rec.update(product_ms=float(np.median(prod)), pattern_ms=1e3 * t_pat, matrix_ms=1e3 * t_mat, jacobi_iterations=its,
                       jacobi_ms_per_iteration=1e3 * tj / max(its, 1), step_ms=1e3 * (t_pat + t_mat + steps[0]),
                       solution_norm=ctx.vec_norm(zzz.VEC_U))
        return rec


def parent(configs, paths, rounds, ndofs):
    out = {}
    for cfg in configs:
        runs = {p: [] for p in paths}
        for rnd in range(rounds):
            for p in (paths if rnd % 2 == 0 else paths[::-1]):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", p, "--config", cfg, "--ndofs", str(ndofs)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:  # (a failed child ends the measurement: nothing more is started on the card)
                    raise RuntimeError(f"{cfg} {p}: child ended with {r.returncode}: {r.stderr[-2000:]}")
                runs[p].append(json.loads(r.stdout.strip().splitlines()[-1]))
        rec = {}
        for p in paths:
            rec[p] = dict(runs[p][0])
            for key, v in runs[p][0].items():
                if isinstance(v, float) and key != "solution_norm":
                    rec[p][key] = float(np.median([x[key] for x in runs[p]]))
                    rec[p][key + "_runs"] = [round(x[key], 4) for x in runs[p]]
        out[cfg] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--config")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--paths", default="matfree,assembled")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ndofs", type=int, default=0, help="override the configurations' size (testing)")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.config, a.ndofs)))
        return
    rec = {"tool": "ab_mf_elasticity", "lib": os.environ.get("ZZZ_HIP_LIB", "in-tree"), "rounds": a.rounds,
           "ZZZ_MF_NC": os.environ.get("ZZZ_MF_NC"), "ZZZ_MF_T": os.environ.get("ZZZ_MF_T"),
           "configs": parent(a.configs.split(","), a.paths.split(","), a.rounds, a.ndofs)}
    text = json.dumps(rec)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
