#!/usr/bin/env python3
"""What -pc_type mg (ZZZ_PC_MG) or -pc_type pmg (ZZZ_PC_PMG) costs and saves against -pc_type jacobi, on ONE GPU, in ONE process.

  ab_mg.py [--configs c1,c2,c4] [--order K] [--pc mg|pmg] [--rounds N] [--out FILE]
  ab_mg.py --order 3 --pc pmg --configs c5_rank --rounds 3      (the P3 per-GPU share of BASELINE configs[4])
  ab_mg.py --order 2 --pc pmg --configs e2m --rounds 3          (elasticity P2, about 2 M dofs)

BASELINE's cubes C1 (500 k dofs Poisson), C2 (10 M dofs Poisson) and C4-total (4 M dofs elasticity), C5's per-GPU share
(6.25 M dofs Poisson) and a 2 M dofs elasticity cube, at --order (mg: 1 only), one rank, no
communicator.  Per configuration: both preconditioners warmed once (code objects, buffers, the product's form), then
`rounds` passes that alternate the order (jacobi, mg | mg, jacobi).  `ZZZ Solve` is the host clock around the synchronous
zzz_cg_solve between two zzz_sync calls, as the driver's timer takes it.  For mg it is taken twice per pass: with the
hierarchy THROWN AWAY first (the feed is generated again, so the solve pays the whole set-up: levels, assemblies, spectrum
estimates, the dense inverse -- what a one-shot run of the driver pays) and with the hierarchy kept (what every further
solve on the same matrix pays).  ms per V-cycle is the mean HIP-event time around the cycles of a profiled solve
(zzz_solver_opts.profile); the set-up's ms is the library's own host clock around it (zzz_mg_info).  With --pc pmg at
order > 1 the record also says what share of a cycle the P1 levels take: ms per V-cycle of ZZZ_PC_MG on the SAME cube at
order 1 (a second context, profiled the same way) over ms per cycle of pmg.

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

CONFIGS = {"c1": ("poisson", 500000, 1), "c2": ("poisson", 10000000, 1), "c4": ("elasticity", 4000000, 3),
           "c5_rank": ("poisson", 6250000, 1), "e2m": ("elasticity", 2000000, 3)}


def generate(ctx, problem, dims, order=1):
    form = zzz.FORM_ELASTICITY if problem == "elasticity" else zzz.FORM_POISSON
    info = ctx.cube_generate(problem, order, *dims, 1, 0)
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


def run(key, rounds, order=1, name="mg"):
    problem, ndofs, per_node = CONFIGS[key]
    pc = zzz.PC_PMG if name == "pmg" else zzz.PC_MG
    m = zzz.mesh_size(ndofs, True, 1, per_node, order)
    dims = tuple(m[i] << m[3] for i in range(3))
    with zzz.Context(0) as ctx:
        dofs = generate(ctx, problem, dims, order)
        timed(ctx, pc=zzz.PC_JACOBI)
        timed(ctx, pc=pc)
        res = {"jacobi": [], name + "_with_setup": [], name + "_hierarchy_kept": []}
        its = {}
        setup = []
        for rnd in range(rounds):
            def jacobi():
                t, its["jacobi"] = timed(ctx, pc=zzz.PC_JACOBI)
                res["jacobi"].append(t)

            def mg():
                generate(ctx, problem, dims, order)  # a new feed: the next mg solve builds its hierarchy from nothing
                t, its[name] = timed(ctx, pc=pc)
                res[name + "_with_setup"].append(t)
                setup.append(ctx.mg_info()["setup_ms"])
                t, _ = timed(ctx, pc=pc)
                res[name + "_hierarchy_kept"].append(t)

            for f in ((jacobi, mg) if rnd % 2 == 0 else (mg, jacobi)):
                f()
        timed(ctx, pc=zzz.PC_JACOBI)
        uj = ctx.vec_download(zzz.VEC_U)
        ctx.cg_solve(pc=pc, rtol=1e-8, profile=True)
        um = ctx.vec_download(zzz.VEC_U)
        info = ctx.mg_info()
        levels = [ctx.mg_info(l) for l in range(info["levels"])]
        med = lambda v: float(np.median(np.array(v)))  # noqa: E731
        rec = {"problem": problem, "order": order, "cells": "x".join(str(d) for d in dims), "dofs": dofs,
               "iterations": {"jacobi": its["jacobi"], name: its[name]},
               "zzz_solve_ms_median": {k: round(med(v), 3) for k, v in res.items()},
               "zzz_solve_ms_all": {k: [round(x, 3) for x in v] for k, v in res.items()},
               name + "_setup_ms_median": round(med(setup), 3), name + "_ms_per_vcycle": round(info["cycle_ms"], 4),
               name + "_levels": [dict(cells="x".join(str(c) for c in lv["cells"]), order=order if l < info["high_order_levels"] else 1,
                                       dofs=lv["dofs"], hi=lv["hi"]) for l, lv in enumerate(levels)],
               name + "_products_per_cycle_level0": info["products_per_cycle"], name + "_coarse_level_bytes": info["coarse_bytes"],
               "relative_difference_of_the_solutions": float(np.linalg.norm(um - uj) / np.linalg.norm(uj)),
               name + "_with_setup_below_jacobi": med(res[name + "_with_setup"]) < med(res["jacobi"]),
               # the condition of the P3 measurement: the slowest solve that pays its set-up against the fastest Jacobi solve
               name + "_slowest_with_setup_below_fastest_jacobi": max(res[name + "_with_setup"]) < min(res["jacobi"])}
    if info["high_order_levels"]:
        # the P1 levels alone: ZZZ_PC_MG's V-cycle on the same cube at order 1
        with zzz.Context(0) as c1:
            generate(c1, problem, dims, 1)
            timed(c1, pc=zzz.PC_MG)
            c1.cg_solve(pc=zzz.PC_MG, rtol=1e-8, profile=True)
            p1 = c1.mg_info()["cycle_ms"]
        rec["p1_levels_ms_per_vcycle"] = round(p1, 4)
        rec["share_of_the_cycle_in_the_p1_levels"] = round(p1 / info["cycle_ms"], 4) if info["cycle_ms"] > 0 else None
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c1,c2,c4")
    ap.add_argument("--order", type=int, default=1, help="polynomial order of the fine problem (2, 3: --pc pmg)")
    ap.add_argument("--pc", default="mg", choices=("mg", "pmg"))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rec = {"tool": "ab_mg.py", "rounds": a.rounds, "pc": a.pc, "order": f"alternating (jacobi, {a.pc} | {a.pc}, jacobi), one process",
           "result": {k: run(k, a.rounds, a.order, a.pc) for k in a.configs.split(",")}}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
