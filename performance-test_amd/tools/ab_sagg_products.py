#!/usr/bin/env python3
"""The two ways -pc_type sagg / sagg_rbm form their products -- sorted term lists (zzz_mg_products = ZZZ_MG_PRODUCTS_LISTS, the
default) against row by row (ZZZ_MG_PRODUCTS_ROWS, csrc/zzz_sagg_rows.hip) -- on ONE GPU, on the cubes of DESIGN.md 5e / 5f.

  ab_sagg_products.py [--cells p79,p215,e109,r82,r109] [--rounds 3] [--limit SECONDS] [--out FILE]

  p79   Poisson 79^3 (512 000 dofs), sagg          p215  Poisson 215^3 (10 077 696 dofs), sagg
  e109  elasticity 109^3 (3 993 000 dofs), sagg    r82   elasticity 82^3 (1 715 361 dofs: the largest the lists mode admits), sagg_rbm
  r109  elasticity 109^3, sagg_rbm: rows mode only (the lists mode declines it with ZZZ_ERR_LIMIT)

Every (cell, mode) measurement runs in a FRESH child process under a time limit of its own; the modes alternate (lists, rows |
rows, lists) for --rounds rounds; the tool stops at the first child that ends with a signal, a fault of the device or its time
limit and says which.  A child generates the cube, assembles, solves once with the hierarchy built inside the solve, assembles
the matrix again and refreshes (zzz_assemble_matrix + zzz_mg_setup), then solves with `profile` set.  It reports:
set-up ms and refresh ms (the library's own host clock around them, zzz_mg_info), the coarse levels' bytes, zzz_mg_products_info's
kept bytes, chunks and transient peak, the iteration count and ms per V-cycle.  The yardstick of the rows mode is the lists
mode on the same GPU in the same run: iteration counts must be equal, and the cycle -- the same kernels on the same arrays --
within the lists mode's own spread.  One JSON record (stdout and --out)."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CELLS = {"p79": ("poisson", 79, "sagg", ("lists", "rows")), "p215": ("poisson", 215, "sagg", ("lists", "rows")),
         "e109": ("elasticity", 109, "sagg", ("lists", "rows")), "r82": ("elasticity", 82, "sagg_rbm", ("lists", "rows")),
         "r109": ("elasticity", 109, "sagg_rbm", ("rows",))}


def child(cell, mode):
    import zzz

    problem, n, pcname, _ = CELLS[cell]
    pc = zzz.PC_SAGG_RBM if pcname == "sagg_rbm" else zzz.PC_SAGG
    form = zzz.FORM_ELASTICITY if problem == "elasticity" else zzz.FORM_POISSON
    with zzz.Context(0) as ctx:
        info = ctx.cube_generate(problem, 1, n, n, n, 1, 0)
        ctx.pattern_build()
        ctx.assemble_matrix(form)
        ctx.assemble_vector(form)
        if pcname == "sagg_rbm":
            dev = C.c_double()
            ctx._ck(ctx.L.zzz_near_nullspace_build(ctx.h, C.byref(dev)))
        ctx.mg_products(zzz.MG_PRODUCTS_ROWS if mode == "rows" else zzz.MG_PRODUCTS_LISTS)
        it, rn, r0 = ctx.cg_solve(pc=pc, rtol=1e-8, max_it=10000)
        ctx.sync()
        built = ctx.mg_info()
        ctx.assemble_matrix(form)  # (the same values, a new set of them as far as the hierarchy knows: the next set-up refreshes)
        ctx.mg_setup(pc=pc)
        refreshed = ctx.mg_info()
        it2, _, _ = ctx.cg_solve(pc=pc, rtol=1e-8, max_it=10000, profile=True)
        ctx.sync()
        solved = ctx.mg_info()
        pi = ctx.mg_products_info()
        rec = {"cell": cell, "mode": mode, "dofs": int(info[0]) if int(info[0]) > 0 else ctx.n_owned * ctx.bs,
               "levels": [ctx.mg_info(l)["dofs"] for l in range(built["levels"])], "iterations": it, "iterations_after_refresh": it2,
               "converged": bool(rn <= 1e-8 * r0), "setup_ms": round(built["setup_ms"], 2), "refresh_ms": round(refreshed["setup_ms"], 2),
               "refresh_was_a_refresh": refreshed["setups"] == built["setups"] + 1, "ms_per_vcycle": round(solved["cycle_ms"], 4),
               "coarse_bytes": built["coarse_bytes"], "kept_bytes": pi["kept_bytes"], "chunks": pi["chunks"],
               "peak_transient_bytes": pi["peak_transient_bytes"], "max_row_candidates": pi["max_row_candidates"]}
    print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="p79,p215,e109,r82,r109")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds one child may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", nargs=2, metavar=("CELL", "MODE"))
    a = ap.parse_args()
    if a.child:
        return child(*a.child)
    rec = {"tool": "ab_sagg_products.py", "rounds": a.rounds, "order": "alternating (lists, rows | rows, lists), a fresh process each",
           "result": [], "stopped": None}
    for cell in a.cells.split(","):
        modes = CELLS[cell][3]
        for rnd in range(a.rounds):
            for mode in (modes if rnd % 2 == 0 else modes[::-1]):
                try:
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", cell, mode], capture_output=True, text=True,
                                       timeout=a.limit)
                except subprocess.TimeoutExpired:
                    rec["stopped"] = f"{cell} {mode} round {rnd}: time limit of {a.limit} s"
                    break
                lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode == 0 and lines:
                    rec["result"].append(dict(json.loads(lines[-1][7:]), round=rnd))
                    print(lines[-1], flush=True)
                    continue
                declined = re.search(r"libzzz_hip error [15]:", r.stderr) is not None
                tail = r.stderr.strip().splitlines()[-1][:400] if r.stderr.strip() else ""
                if r.returncode > 0 and declined:  # (the library declined: a result, not a fault)
                    rec["result"].append({"cell": cell, "mode": mode, "round": rnd, "declined": tail})
                    print(f"DECLINED {cell} {mode}: {tail}", flush=True)
                    continue
                rec["stopped"] = f"{cell} {mode} round {rnd}: exit status {r.returncode}: {tail}"
                break
            if rec["stopped"]:
                break
        if rec["stopped"]:
            break
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 1 if rec["stopped"] else 0


if __name__ == "__main__":
    sys.exit(main())
