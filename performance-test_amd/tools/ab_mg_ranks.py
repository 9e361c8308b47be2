#!/usr/bin/env python3
"""-pc_type mg (ZZZ_PC_MG) on several ranks, as far as ONE GPU can show it: the ranks are threads of this process with the
host-mediated communicator (zzz.LocalGroup), every rank's slab and its copy of the coarse levels on the same device.

  ab_mg_ranks.py [--configs c2,c4] [--ranks 8] [--out FILE]

Per configuration (BASELINE's cubes C2, 10 M dofs Poisson, and C4-total, 4 M dofs elasticity; see tools/ab_mg.py):
  * the iteration counts of Jacobi and of mg on one rank and partitioned, and the difference of the two mg solutions;
  * what every rank holds for the replicated levels and the level table: the device bytes the ONE-RANK set-up took, alone on
    the device (zzz_mg_info), less level 0's three smoother vectors -- the same child contexts, and hipMemGetInfo says nothing
    per rank while N ranks allocate on one device;
  * the whole-cube coarse cycle every rank repeats: the one-rank V-cycle of the level-1 cube, HIP-event ms per cycle of a
    profiled solve on a context of its own, and beside it the one-rank cycle of the whole fine cube.
The partitioned run's clock is NOT reported as a timing: the local communicator's all-reduce and halo go through the host and
every call ends synchronised, N ranks share one device, and the coarse cycle runs N times on it.  One JSON record."""
import argparse
import json
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zzz  # noqa: E402

CONFIGS = {"c1": ("poisson", 500000, 1), "c2": ("poisson", 10000000, 1), "c4": ("elasticity", 4000000, 3)}


def generate(ctx, problem, dims, nparts=1, part=0):
    form = zzz.FORM_ELASTICITY if problem == "elasticity" else zzz.FORM_POISSON
    ctx.cube_generate(problem, 1, *dims, nparts, part)
    ctx.pattern_build()
    ctx.assemble_matrix(form)
    ctx.assemble_vector(form)


def one_rank(problem, dims, jacobi=True):
    with zzz.Context(0) as c:
        generate(c, problem, dims)
        itj = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)[0] if jacobi else None
        c.cg_solve(pc=zzz.PC_MG, rtol=1e-8)
        it = c.cg_solve(pc=zzz.PC_MG, rtol=1e-8, profile=True)[0]
        info = c.mg_info()
        return dict(jacobi=itj, mg=it, cycle_ms=info["cycle_ms"], coarse_bytes=info["coarse_bytes"], levels=[c.mg_info(l) for l in range(info["levels"])],
                    u=c.vec_download(zzz.VEC_U))


def partitioned(problem, dims, nparts):
    grp = zzz.LocalGroup(nparts)
    out, err = [None] * nparts, []

    def run(rank):
        try:
            with zzz.Context(0) as c:
                c.comm_init_local(grp.h, rank)
                generate(c, problem, dims, nparts, rank)
                itj = c.cg_solve(pc=zzz.PC_JACOBI, rtol=1e-8)[0]
                it = c.cg_solve(pc=zzz.PC_MG, rtol=1e-8)[0]
                info = c.mg_info()
                out[rank] = dict(jacobi=itj, mg=it, owned_dofs=c.n_owned * c.bs,
                                 levels=[c.mg_info(l) for l in range(info["levels"])], u=c.vec_download(zzz.VEC_U))
        except Exception as e:  # noqa: BLE001
            err.append((rank, repr(e)))
            grp.abort()

    th = [threading.Thread(target=run, args=(r,)) for r in range(nparts)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    grp.close()
    if err:
        raise RuntimeError(str(err))
    return out


def run(key, nparts):
    problem, ndofs, per_node = CONFIGS[key]
    m = zzz.mesh_size(ndofs, True, 1, per_node, 1)
    dims = tuple(m[i] << m[3] for i in range(3))
    one = one_rank(problem, dims)
    level1 = tuple(one["levels"][1]["cells"])
    coarse = one_rank(problem, level1, jacobi=False)
    ranks = partitioned(problem, dims, nparts)
    u = np.concatenate([r["u"] for r in ranks])
    table = lambda lv: [dict(cells="x".join(str(c) for c in v["cells"]), dofs=v["dofs"], nnz=v["nnz"]) for v in lv]  # noqa: E731
    return {"problem": problem, "cells": "x".join(str(d) for d in dims), "ranks": nparts,
            "iterations": {"jacobi_one_rank": one["jacobi"], "mg_one_rank": one["mg"],
                           "jacobi_partitioned": sorted({r["jacobi"] for r in ranks}), "mg_partitioned": sorted({r["mg"] for r in ranks})},
            "relative_difference_of_the_mg_solutions": float(np.linalg.norm(u - one["u"]) / np.linalg.norm(one["u"])),
            "level_table_partitioned_equals_one_rank": all(table(r["levels"]) == table(one["levels"]) for r in ranks),
            "levels": table(one["levels"]),
            "owned_dofs_per_rank": [r["owned_dofs"] for r in ranks],
            "replicated_levels_device_bytes_per_rank": int(one["coarse_bytes"] - 3 * 8 * one["levels"][0]["dofs"]),
            "one_rank_ms_per_vcycle_whole_cube": round(one["cycle_ms"], 4),
            "one_rank_ms_per_vcycle_level_1_cube": round(coarse["cycle_ms"], 4), "level_1_cube": "x".join(str(c) for c in level1),
            "note": "the partitioned run is not timed: host-mediated all-reduce and halo, all ranks and their coarse copies on one device"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c4")
    ap.add_argument("--ranks", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rec = {"tool": "ab_mg_ranks.py", "result": {k: run(k, a.ranks) for k in a.configs.split(",")}}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
