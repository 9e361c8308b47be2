#!/usr/bin/env python3
"""A/B of two BUILDS of libzzz_hip.so on the assembly phases: child processes alternate between the two libraries
(ZZZ_HIP_LIB), each times pattern build, matrix assembly and vector assembly on one device-generated system.
Usage: ab_lib.py <other libzzz_hip.so> [case ...] [--rounds N] [--json FILE]   (cases as in ab_sellp.py; the in-tree build is
"new"; per phase the median, minimum and maximum over the rounds of each build; --json keeps the per-round numbers)"""
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def child(case):
    import zzz
    from ab_sellp import CASES
    problem, order, ndofs, bs = CASES[case]
    nx, ny, nz, r = zzz.mesh_size(ndofs, True, 1, bs, order)
    form = zzz.FORM_POISSON if problem == "poisson" else zzz.FORM_ELASTICITY
    with zzz.Context(0) as ctx:
        ctx.cube_generate(problem, order, nx << r, ny << r, nz << r, 1, 0)
        t = {"pattern": [], "matrix": [], "vector": []}
        for rep in range(6):
            for name, fn in (("pattern", ctx.pattern_build), ("matrix", lambda: ctx.assemble_matrix(form)),
                             ("vector", lambda: ctx.assemble_vector(form))):
                ctx.sync()
                t0 = time.perf_counter()
                fn()
                ctx.sync()
                t[name].append(time.perf_counter() - t0)
        nrm = ctx.vec_norm(zzz.VEC_B)
        rowptr, cols, vals = ctx.csr_download()
        print("RES", " ".join(f"{1e3 * np.median(v[1:]):.4f}" for v in t.values()), repr(nrm), repr(float(np.abs(vals).sum())))


def main():
    args = sys.argv[1:]
    rounds, json_path = 3, None
    for flag in ("--rounds", "--json"):
        if flag in args:
            k = args.index(flag)
            if flag == "--rounds":
                rounds = int(args[k + 1])
            else:
                json_path = args[k + 1]
            del args[k:k + 2]
    other = os.path.abspath(args[0])
    cases = args[1:] or ["c2"]
    phases = ("pattern", "matrix", "vector")
    record = {"tool": "ab_lib.py", "old": other, "rounds": rounds, "unit": "ms (per child: median of its last five of six repetitions)",
              "cases": {}}
    for case in cases:
        res = {"old": [], "new": []}
        for rnd in range(rounds):
            for tag in ("old", "new"):
                env = dict(os.environ)
                if tag == "old":
                    env["ZZZ_HIP_LIB"] = other
                else:
                    env.pop("ZZZ_HIP_LIB", None)
                out = subprocess.run([sys.executable, __file__, "--child", case], env=env, capture_output=True, text=True, timeout=900)
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("RES")]
                if out.returncode != 0 or not line:
                    print(out.stdout[-2000:], out.stderr[-2000:])
                    sys.exit(1)
                res[tag].append(line[0].split()[1:])
        t = {tag: np.array([[float(x) for x in r[:3]] for r in res[tag]]) for tag in res}
        for tag in ("old", "new"):
            a = t[tag]
            print(f"[{case}] {tag}: " + "  ".join(f"{ph} {np.median(a[:, k]):.3f} [{a[:, k].min():.3f}, {a[:, k].max():.3f}] ms"
                                                   for k, ph in enumerate(phases))
                  + f"   (median [min, max] of {rounds} rounds; matrix with stream packing)   |b| {res[tag][0][3]}  sum|A| {res[tag][0][4]}")
        same = all(r[3:] == res["old"][0][3:] for tag in res for r in res[tag])
        print(f"[{case}] identical |b| and sum|A|:", same)
        # the new build's median against the old one's, with the old build's own spread over its rounds as the margin
        within = {ph: bool(np.median(t["new"][:, k]) - np.median(t["old"][:, k]) <= t["old"][:, k].max() - t["old"][:, k].min())
                  for k, ph in enumerate(phases)}
        print(f"[{case}] new median within old median + old (max - min):", within)
        record["cases"][case] = {"old": {ph: t["old"][:, k].tolist() for k, ph in enumerate(phases)},
                                 "new": {ph: t["new"][:, k].tolist() for k, ph in enumerate(phases)},
                                 "norm_b": res["old"][0][3], "sum_abs_A": res["old"][0][4], "identical_norms": same,
                                 "new_median_within_old_spread": within}
    if json_path:
        import json

        with open(json_path, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
