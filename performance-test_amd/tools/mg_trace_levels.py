#!/usr/bin/env python3
"""Where a V-cycle of -pc_type mg spends its time, level by level, from a rocprofv3 --kernel-trace of ONE solve.

  mg_trace_levels.py <dir with *_kernel_trace.csv> [--out FILE]

A cycle over L levels dispatches L - 1 restrictions on the way down and L - 1 prolongations on the way up, so the
dispatch order alone says which level a kernel belongs to: everything between the end of restriction k and the start of the
matching prolongation runs on levels >= k.  Reported per cycle (median over the cycles of the trace): the span of the cycle,
the span spent on levels >= 1, >= 2, ..., the kernels' busy time inside each span and the idle share (launch latency)."""
import argparse
import csv
import glob
import json
import os
import statistics


def load(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    return rows


def cycles(rows):
    """lists of dispatch indices [first smoother kernel of level 0 .. last kernel before the next k_dots_rz]"""
    out, cur = [], None
    for i, (_, _, name) in enumerate(rows):
        if "k_mg_" not in name and "k_cheb_first" not in name and cur is None:  # (the smoother's kernels are zzz_cg.hip's)
            continue
        if cur is None:
            cur = [i]
            continue
        if "k_dots_rz" in name:
            out.append(cur)
            cur = None
            continue
        cur.append(i)
    return out


def analyse(rows):
    per_level = {}
    spans = []
    for cyc in cycles(rows):
        names = [rows[i][2] for i in cyc]
        res = [i for i, n in zip(cyc, names) if "k_mg_restrict" in n]
        pro = [i for i, n in zip(cyc, names) if "k_mg_prolong" in n]
        if not res or len(res) != len(pro):
            continue
        spans.append(rows[cyc[-1]][1] - rows[cyc[0]][0])
        for k in range(len(res)):
            lo, hi = res[k], pro[len(pro) - 1 - k]  # restriction into level k + 1, prolongation out of it
            span = rows[hi][0] - rows[lo][1]
            busy = sum(rows[i][1] - rows[i][0] for i in range(lo + 1, hi))
            per_level.setdefault(k + 1, []).append((span, busy, hi - lo - 1))
    if not spans:
        return {"cycles": 0}
    med = statistics.median
    cyc_us = med(spans) / 1e3
    out = {"cycles": len(spans), "cycle_us_median": round(cyc_us, 1), "levels_from": {}}
    for k, v in sorted(per_level.items()):
        span, busy = med(x[0] for x in v) / 1e3, med(x[1] for x in v) / 1e3
        out["levels_from"][str(k)] = {"span_us": round(span, 1), "share_of_cycle": round(span / cyc_us, 3), "kernel_busy_us": round(busy, 1),
                                      "idle_share_of_span": round(1.0 - busy / span, 3) if span > 0 else 0.0, "dispatches": int(med(x[2] for x in v))}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rec = {"tool": "mg_trace_levels.py", "result": analyse(load(a.dir))}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
