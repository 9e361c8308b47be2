#!/usr/bin/env python3
"""The right-hand side of a matrix-free problem both ways, on ONE GPU: row-gather (zzz_csr_pattern_build + zzz_assemble_vector)
against cell-block (zzz_matfree_assemble_vector: no sparsity pattern).

  ab_rhs.py --problem cgpoisson|cgelasticity --order K --ndofs N [--rounds 3] [--out FILE]
  ab_rhs.py --child rowgather|cellblock --problem ... --order K --ndofs N      one measurement in this process (internal)

Every way runs in a FRESH child process -- its own context and clocks -- `rounds` times, alternately rowgather-first and
cellblock-first.  A child times the phases the driver puts under its `ZZZ Assemble` umbrella for these problem types (wall clock
around each call, the stream drained): what stands where the reference creates its matrix (the pattern build, or nothing), the
plan of the matrix-free kernels, `ZZZ Assemble vector` (first call, and the median of five more); and reports the device memory
in use after set-up (zzz_device_memory before the context and after the vector) with the vector's norm.  One JSON record."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zzz  # noqa: E402


def child(way, problem, order, ndofs):
    el = problem == "cgelasticity"
    form = zzz.FORM_ELASTICITY if el else zzz.FORM_POISSON
    nx, ny, nz, r = zzz.mesh_size(ndofs, True, 1, 3 if el else 1, order)
    free0, total = zzz.device_memory(0)
    with zzz.Context(0) as ctx:
        info = ctx.cube_generate("elasticity" if el else "poisson", order, nx << r, ny << r, nz << r, 1, 0)
        ctx.sync()

        def timed(call):
            ctx.sync()
            t0 = time.perf_counter()
            call()
            ctx.sync()
            return 1e3 * (time.perf_counter() - t0)

        t_pattern = timed(ctx.pattern_build) if way == "rowgather" else 0.0
        t_plan = timed(ctx.matfree_setup)
        vec = (lambda: ctx.assemble_vector(form)) if way == "rowgather" else (lambda: ctx.matfree_assemble_vector(form))
        t_first = timed(vec)
        t_more = [timed(vec) for _ in range(5)]
        free1, _ = zzz.device_memory(0)
        return {"way": way, "problem": problem, "order": order, "dofs": int(info[0]), "pattern_ms": t_pattern,
                "plan_ms": t_plan, "vector_first_ms": t_first, "vector_ms": float(np.median(t_more)),
                "assemble_umbrella_ms": t_pattern + t_plan + t_first, "device_bytes_in_use": free0 - free1, "device_bytes_total": total,
                "b_norm": ctx.vec_norm(zzz.VEC_B)}


def parent(a):
    ways = ["rowgather", "cellblock"]
    runs = {w: [] for w in ways}
    for rnd in range(a.rounds):
        for w in (ways if rnd % 2 == 0 else ways[::-1]):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", w, "--problem", a.problem, "--order", str(a.order), "--ndofs",
                   str(a.ndofs)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:  # (a failed child ends the measurement: nothing more is started on the card)
                raise RuntimeError(f"{w}: child ended with {r.returncode}: {r.stderr[-2000:]}")
            runs[w].append(json.loads(r.stdout.strip().splitlines()[-1]))
    rec = {"dofs": runs[ways[0]][0]["dofs"]}
    for w in ways:
        med = lambda key: float(np.median([x[key] for x in runs[w]]))  # noqa: E731
        rec[w] = {k: med(k) for k in ("pattern_ms", "plan_ms", "vector_first_ms", "vector_ms", "assemble_umbrella_ms", "device_bytes_in_use")}
        rec[w]["vector_ms_runs"] = [round(x["vector_ms"], 4) for x in runs[w]]
        rec[w]["b_norm"] = runs[w][0]["b_norm"]
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="", choices=["", "rowgather", "cellblock"])
    ap.add_argument("--problem", default="cgpoisson", choices=["cgpoisson", "cgelasticity"])
    ap.add_argument("--order", type=int, default=1)
    ap.add_argument("--ndofs", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.problem, a.order, a.ndofs)))
        sys.exit(0)
    rec = {"tool": "ab_rhs.py", "problem": a.problem, "order": a.order, "rounds": a.rounds, "result": parent(a)}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
