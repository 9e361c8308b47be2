#!/usr/bin/env python3
"""What --scalar_type float32 buys the cgpoisson path against float64, on ONE GPU.

  ab_scalar.py [--configs cgpoisson_p1_c2,cgpoisson_p3_c5rank] [--rounds 3] [--out FILE]
  ab_scalar.py --child float64|float32 --config NAME          one measurement in this process, one JSON line (internal)

For each configuration (bench.py's cgpoisson_p1_c2: P1, the mesh of BASELINE configs[1], 10 M dofs; cgpoisson_p3_c5rank:
P3, the per-GPU share of configs[4], 6.2 M dofs) every precision runs in a FRESH child process -- its own context, plan and
clocks -- `rounds` times, alternately float64-first and float32-first, so that neither always runs on a warm or a cold
card.  A child reports the action's time from 20 back-to-back launches with the <p,y> partials, the bytes one action
addresses, and linalg::cg(u, b, action, 100, 1e-6): Gdof/s as the reference prints it (src/cgpoisson_problem.cpp:236-241:
iterations x dofs / time of the cg call alone) and ms per iteration, the median of three solves after one warm-up.
ZZZ_HIP_LIB=<another build's libzzz_hip.so> --scalars float64 gives that build's double figures (the parent commit's).
One JSON record (stdout and --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zzz  # noqa: E402

CONFIGS = {"cgpoisson_p1_c2": (1, 10000000), "cgpoisson_p3_c5rank": (3, 6250000)}
CGH = dict(variant=zzz.CG_CGH, pc=zzz.PC_NONE, op=zzz.OP_MATFREE, rtol=1e-6, max_it=100)


def child(scalar, config, ndofs=0):
    order, nd = CONFIGS[config]
    nx, ny, nz, r = zzz.mesh_size(ndofs or nd, True, 1, 1, order)
    f32 = scalar == "float32"
    with zzz.Context(0) as ctx:
        info = ctx.cube_generate("poisson", order, nx << r, ny << r, nz << r, 1, 0)
        n = int(info[0])
        ctx.matfree_setup()
        ctx.pattern_build()  # the right-hand side's assembly walks the dof -> cell adjacency
        ctx.assemble_vector(zzz.FORM_POISSON)
        solve = ctx.cg_solve_f32 if f32 else ctx.cg_solve
        ts, it, ratio = [], 0, 0.0
        for k in range(4):
            ctx.vec_upload(zzz.VEC_U, np.zeros(n))
            ctx.sync()
            t0 = time.perf_counter()
            it, rr, rr0 = solve(**CGH)
            ctx.sync()
            if k:
                ts.append(time.perf_counter() - t0)
            ratio = rr / rr0
        act = [ctx.action_time_f32(20) if f32 else ctx.action_time(20) for _ in range(3)]
        plan = ctx.matfree_info()
        extra = ctx.matfree_info_f32() if f32 else {}
        t = float(np.median(ts))
        return {"scalar": scalar, "config": config, "dofs": n, "action_ms": float(np.median(act)), "action_ms_all": [round(a, 4) for a in act],
                "bytes_per_action": extra["bytes_per_action"] if f32 else plan["bytes_per_action"],
                "cg_iterations": it, "cg_ms_per_iteration": 1e3 * t / max(it, 1), "Gdof_per_s": it * n / t / 1e9,
                "residual_ratio": ratio, "solution_norm": ctx.vec_norm(zzz.VEC_U), "cells_per_block": plan["cells_per_block"],
                "lds_bytes": extra.get("lds_bytes"), "workgroups_per_cu": extra.get("workgroups_per_cu")}


def parent(configs, scalars, rounds, ndofs):
    out = {}
    for cfg in configs:
        runs = {s: [] for s in scalars}
        for rnd in range(rounds):
            for s in (scalars if rnd % 2 == 0 else scalars[::-1]):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", s, "--config", cfg, "--ndofs", str(ndofs)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:  # (a failed child ends the measurement: nothing more is started on the card)
                    raise RuntimeError(f"{cfg} {s}: child ended with {r.returncode}: {r.stderr[-2000:]}")
                runs[s].append(json.loads(r.stdout.strip().splitlines()[-1]))
        rec = {}
        for s in scalars:
            med = lambda key: float(np.median([x[key] for x in runs[s]]))  # noqa: E731
            rec[s] = {"action_ms": med("action_ms"), "action_ms_runs": [round(x["action_ms"], 4) for x in runs[s]],
                      "bytes_per_action": runs[s][0]["bytes_per_action"], "cg_ms_per_iteration": med("cg_ms_per_iteration"),
                      "Gdof_per_s": med("Gdof_per_s"), "Gdof_per_s_runs": [round(x["Gdof_per_s"], 3) for x in runs[s]],
                      "cg_iterations": runs[s][0]["cg_iterations"], "residual_ratio": runs[s][0]["residual_ratio"],
                      "solution_norm": runs[s][0]["solution_norm"], "lds_bytes": runs[s][0]["lds_bytes"],
                      "workgroups_per_cu": runs[s][0]["workgroups_per_cu"]}
        if len(scalars) == 2:
            a, b = rec["float64"], rec["float32"]
            rec["float64_over_float32"] = {"action": a["action_ms"] / b["action_ms"], "cg_iteration": a["cg_ms_per_iteration"] / b["cg_ms_per_iteration"],
                                           "bytes": a["bytes_per_action"] / b["bytes_per_action"]}
        rec["dofs"] = runs[scalars[0]][0]["dofs"]
        out[cfg] = rec
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="", choices=["", "float64", "float32"])
    ap.add_argument("--config", default="")
    ap.add_argument("--configs", default="cgpoisson_p1_c2,cgpoisson_p3_c5rank")
    ap.add_argument("--scalars", default="float64,float32")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ndofs", type=int, default=0, help="another size for the same orders (0: the configuration's own)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.config, a.ndofs)))
        sys.exit(0)
    rec = {"tool": "ab_scalar.py", "library": os.environ.get("ZZZ_HIP_LIB", "in-tree build"), "rounds": a.rounds,
           "result": parent(a.configs.split(","), a.scalars.split(","), a.rounds, a.ndofs)}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
