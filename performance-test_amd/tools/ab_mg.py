#!/usr/bin/env python3
"""What -pc_type mg (ZZZ_PC_MG) costs and saves against -pc_type jacobi, on ONE GPU, in ONE process.

  ab_mg.py [--configs c1,c2,c4] [--rounds N] [--out FILE]

BASELINE's cubes C1 (500 k dofs Poisson), C2 (10 M dofs Poisson) and C4-total (4 M dofs elasticity), P1, one rank, no
communicator.  Per configuration: both preconditioners warmed once (code objects, buffers, the product's form), then
`rounds` passes that alternate the order (jacobi, mg | mg, jacobi).  `ZZZ Solve` is the host clock around the synchronous
zzz_cg_solve between two zzz_sync calls, as the driver's timer takes it.  For mg it is taken twice per pass: with the
hierarchy THROWN AWAY first (the feed is generated again, so the solve pays the whole set-up: levels, assemblies, spectrum
estimates, the dense inverse -- what a one-shot run of the driver pays) and with the hierarchy kept (what every further
solve on the same matrix pays).  ms per V-cycle is the mean HIP-event time around the cycles of a profiled solve
(zzz_solver_opts.profile); the set-up's ms is the library's own host clock around it (zzz_mg_info).

One JSON record (stdout and --out).  Jacobi runs the same library with pc = ZZZ_PC_JACOBI: this change touches none of
its kernels, so it is the parent commit's Jacobi solve."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zzz  # noqa: E402

CONFIGS = {"c1": ("poisson", 500000, 1), "c2": ("poisson", 10000000, 1), "c4": ("elasticity", 4000000, 3)}


def generate(ctx, problem, dims):
    form = zzz.FORM_ELASTICITY if problem == "elasticity" else zzz.FORM_POISSON
    info = ctx.cube_generate(problem, 1, *dims, 1, 0)
    ctx.pattern_build()
    ctx.assemble_matrix(form)
    ctx.assemble_vector(form)
    return int(info[0])


def timed(ctx, **kw):
    ctx.sync()
    t0 = time.perf_counter()
    it, rn, r0 = ctx.cg_solve(rtol=1e-8, max_it=10000, **kw)
    ctx.sync()
    return 1e3 * (time.perf_counter() - t0), it


def run(key, rounds):
    problem, ndofs, per_node = CONFIGS[key]
    m = zzz.mesh_size(ndofs, True, 1, per_node, 1)
    dims = tuple(m[i] << m[3] for i in range(3))
    with zzz.Context(0) as ctx:
        dofs = generate(ctx, problem, dims)
        timed(ctx, pc=zzz.PC_JACOBI)
        timed(ctx, pc=zzz.PC_MG)
        res = {"jacobi": [], "mg_with_setup": [], "mg_hierarchy_kept": []}
        its = {}
        setup = []
        for rnd in range(rounds):
            def jacobi():
                t, its["jacobi"] = timed(ctx, pc=zzz.PC_JACOBI)
                res["jacobi"].append(t)

            def mg():
                generate(ctx, problem, dims)  # a new feed: the next mg solve builds its hierarchy from nothing
                t, its["mg"] = timed(ctx, pc=zzz.PC_MG)
                res["mg_with_setup"].append(t)
                setup.append(ctx.mg_info()["setup_ms"])
                t, _ = timed(ctx, pc=zzz.PC_MG)
                res["mg_hierarchy_kept"].append(t)

            for f in ((jacobi, mg) if rnd % 2 == 0 else (mg, jacobi)):
                f()
        timed(ctx, pc=zzz.PC_JACOBI)
        uj = ctx.vec_download(zzz.VEC_U)
        ctx.cg_solve(pc=zzz.PC_MG, rtol=1e-8, profile=True)
        um = ctx.vec_download(zzz.VEC_U)
        info = ctx.mg_info()
        levels = [ctx.mg_info(l) for l in range(info["levels"])]
        med = lambda v: float(np.median(np.array(v)))  # noqa: E731
        return {"problem": problem, "cells": "x".join(str(d) for d in dims), "dofs": dofs,
                "iterations": {"jacobi": its["jacobi"], "mg": its["mg"]},
                "zzz_solve_ms_median": {k: round(med(v), 3) for k, v in res.items()},
                "zzz_solve_ms_all": {k: [round(x, 3) for x in v] for k, v in res.items()},
                "mg_setup_ms_median": round(med(setup), 3), "mg_ms_per_vcycle": round(info["cycle_ms"], 4),
                "mg_levels": [dict(cells="x".join(str(c) for c in lv["cells"]), dofs=lv["dofs"], hi=lv["hi"]) for lv in levels],
                "mg_products_per_cycle_level0": info["products_per_cycle"], "mg_coarse_level_bytes": info["coarse_bytes"],
                "relative_difference_of_the_solutions": float(np.linalg.norm(um - uj) / np.linalg.norm(uj)),
                "mg_with_setup_below_jacobi": med(res["mg_with_setup"]) < med(res["jacobi"])}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c1,c2,c4")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rec = {"tool": "ab_mg.py", "rounds": a.rounds, "order": "alternating (jacobi, mg | mg, jacobi), one process",
           "result": {k: run(k, a.rounds) for k in a.configs.split(",")}}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
