#!/usr/bin/env python
"""Reduces the measurements behind profiles/own_row_loads/ (a row's own operands requested before its dot product): parent build against branch
build, from files of ONE GPU job.

    python scripts/own_row_loads_ab.py kernels STATS_PARENT STATS_PARENT [...] -- STATS_BRANCH [...]
        rocprofv3 --kernel-trace --stats per-kernel statistics (csv; every run a process of its own, no counters; the parent at least twice).
        Per gmgk:: kernel: calls per run, the mean duration over the parent's runs, the spread of its runs (max - min of the per-run means: the
        parent's own run-to-run difference), the same for the branch, and the verdict -- "faster" only where the branch's mean lies below the
        parent's by more than the parent's spread.
    python scripts/own_row_loads_ab.py steps DIR
        DIR/steps200_{parent,branch}_<i>.json and DIR/default_{parent,branch}_<i>.json: bench.py lines of alternating runs.  A gain only if
        the branch's slowest 200-step figure is below the parent's fastest.
"""
import csv
import glob
import json
import re
import sys


def _stats(path):
    out = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Name"]
            if "gmgk::" not in name:
                continue
            name = re.sub(r"\(.*", "", name).replace("void ", "").replace("gmgk::", "")
            out[name] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["TotalDurationNs"]) / 1e3)
    return out


def kernels(parents, branches):
    P, B = [_stats(p) for p in parents], [_stats(p) for p in branches]
    print("means in us; parent: %d runs, branch: %d runs, the two builds alternating in one job" % (len(P), len(B)))
    print("%-52s %6s %9s %9s %9s %9s %8s  %s" % ("kernel", "calls", "parent", "p.spread", "branch", "b.spread", "delta", "verdict"))
    tot = [0.0, 0.0]
    for name in sorted(B[0], key=lambda n: -B[0][n][2]):
        if any(name not in S for S in P + B):
            continue
        p, b = [S[name][1] for S in P], [S[name][1] for S in B]
        pm, bm, noise = sum(p) / len(p), sum(b) / len(b), max(p) - min(p)
        verdict = "faster" if bm < pm - noise else ("slower" if bm > pm + noise else "same")
        print("%-52s %6d %9.2f %9.2f %9.2f %9.2f %+8.2f  %s" % (name[:52], B[0][name][0], pm, noise, bm, max(b) - min(b), bm - pm, verdict))
        tot[0] += sum(S[name][2] for S in P) / len(P)
        tot[1] += sum(S[name][2] for S in B) / len(B)
    print("total time in gmgk:: kernels per run, us: parent %.0f branch %.0f" % tuple(tot))


def steps(d):
    rep = {}
    for kind in ("steps200", "default"):
        for who in ("parent", "branch"):
            v = [json.load(open(f))["ms_per_step"] for f in sorted(glob.glob(f"{d}/{kind}_{who}_*.json"))]
            rep[kind, who] = v
            if v:
                print(f"{kind:9s} {who:6s} ms per step:", " ".join(f"{x:.4f}" for x in v), f"  min {min(v):.4f} max {max(v):.4f}")
    p, b = rep["steps200", "parent"], rep["steps200", "branch"]
    print(f"200-step figures: branch slowest {max(b):.4f} ms, parent fastest {min(p):.4f} ms -> " +
          ("the ranges separate: a gain of %.1f us per step (medians)" % (1e3 * (sorted(p)[len(p) // 2] - sorted(b)[len(b) // 2])) if max(b) < min(p)
           else "the ranges do NOT separate: not a measured gain"))


if __name__ == "__main__":
    if len(sys.argv) >= 6 and sys.argv[1] == "kernels" and "--" in sys.argv:
        k = sys.argv.index("--")
        kernels(sys.argv[2:k], sys.argv[k + 1:])
    elif len(sys.argv) == 3 and sys.argv[1] == "steps":
        steps(sys.argv[2])
    else:
        sys.exit(__doc__)
