"""gmg_config::fold_head measured (profiles/fold_head/): the in-process A/B, the process a kernel trace wraps, and the trace's timeline.

    python scripts/fold_head_ab.py ab 3m,3m-d3,722k [rounds]      # loops of 200 run_cycles steps alternating between two handles that differ in
                                                                  # fold_head alone; first round dropped; one JSON line per workload
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/fold_head_ab.py trace FOLD      # bench.py's workload, 3 + 20 cycles
    python scripts/fold_head_ab.py timeline DIR/<host>/<pid>_kernel_trace.csv      # launches per cycle, mean duration per position, gaps

A change counts as a gain when the folded median lies below the unfolded one by more than the larger of the two min-max spreads."""
import collections
import csv
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = 200

def ab(label, H, mass, lhs, rhs, rounds):
    import numpy as np
    import torch
    from gravo_mg_amd import cabi
    rhs = np.asfortranarray(rhs)
    engs = {}
    for fold in (1, 0):
        e = cabi.Engine(fold_head=fold)
        e.use_hierarchy(H); e.set_mass(mass); e.set_system(lhs)
        engs[fold] = e
    times = {1: [], 0: []}
    res = {}
    for r in range(rounds):
        for fold in ((1, 0) if r % 2 == 0 else (0, 1)):
            e = engs[fold]
            e.load_problem(rhs, rhs); e.run_cycles(3, 2)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out = e.run_cycles(STEPS, 2)
            torch.cuda.synchronize(); times[fold].append(1e3 * (time.perf_counter() - t0) / STEPS)
            res[fold] = (out.copy(), e.fetch_solution())
    same = bool(np.array_equal(res[1][0].view(np.uint64), res[0][0].view(np.uint64)) and np.array_equal(res[1][1].view(np.uint64), res[0][1].view(np.uint64)))
    rep = {"workload": label, "d": int(rhs.shape[1]), "n": int(lhs.shape[0]), "rounds_kept": rounds - 1, "steps": STEPS, "bitwise_same": same,
           "colors": engs[1].level_info(0)["n_colors"]}
    for fold in (1, 0):
        t = np.array(times[fold][1:])
        rep["fold%d" % fold] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "all_ms": [round(float(v), 5) for v in times[fold]],
                                 "heads_enqueued": engs[fold].timing("heads_enqueued"), "heads_folded": engs[fold].timing("heads_folded")}
    spread = max(rep["fold1"]["max_ms"] - rep["fold1"]["min_ms"], rep["fold0"]["max_ms"] - rep["fold0"]["min_ms"])
    rep["gain_ms"] = rep["fold0"]["median_ms"] - rep["fold1"]["median_ms"]
    rep["larger_spread_ms"] = spread
    rep["counts_as_gain"] = bool(rep["gain_ms"] > spread)
    print(json.dumps(rep), flush=True)
    for e in engs.values():
        e.close()


def run_ab(which, rounds):
    from gravo_mg_amd import cabi, meshgen
    if "3m" in which or "3m-d3" in which:
        V, F = meshgen.torus_mesh(1732, 1732)
        S, mass = meshgen.cotan_laplacian(V, F)
        H = cabi.Hierarchy(V, meshgen.neighbors_from_stiffness(S), ratio=8.0, lower_bound=1000)
        if "3m" in which:
            lhs, rhs = meshgen.poisson_system(S, mass, tau=1e-6, seed=42, d=1)
            ab("torus1732x1732-poisson-tau1e-6-d1 (bench.py)", H, mass, lhs, rhs, rounds)
        if "3m-d3" in which:
            lhs, rhs = meshgen.smoothing_system(S, mass, V)
            ab("torus1732x1732 smoothing M + 1e-3 S, d = 3", H, mass, lhs, rhs, rounds)
        del V, F, S, H
    if "722k" in which:
        name, pos, S2, mass2, lhs2, rhs2 = meshgen.baseline_config("2")
        H2 = cabi.Hierarchy(pos, meshgen.neighbors_from_stiffness(S2), ratio=8.0, lower_bound=1000)
        ab(name, H2, mass2, lhs2, rhs2, rounds)


def trace(fold):
    """bench.py's workload on one handle, 3 + 20 cycles: the process rocprofv3 wraps."""
    import numpy as np
    import bench
    from gravo_mg_amd import cabi
    H, mass, lhs, rhs = bench.build_workload(1732, 1732)
    e = cabi.Engine(fold_head=fold)
    e.use_hierarchy(H); e.set_mass(mass); e.set_system(lhs)
    rhs = np.asfortranarray(rhs)
    e.load_problem(rhs, rhs); e.run_cycles(3, 2)
    print("residues", e.run_cycles(20, 2)[-3:], "heads", e.timing("heads_enqueued"), "folded", e.timing("heads_folded"))
    e.close()


def timeline(path):
    rows = []
    with open(path, newline="") as f:
        rd = csv.DictReader(f)
        for r in rd:
            if "gmgk::" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "").replace("gmgk::", ""), r["Grid_Size_X"]))
    rows.sort()
    ends = [i for i, r in enumerate(rows) if r[2].startswith("reduce_partials")]
    # a cycle = the launches behind one reduce_partials up to and including the next (the head enqueued behind the check belongs to the next cycle)
    cyc = [rows[ends[k] + 1: ends[k + 1] + 1] for k in range(len(ends) - 1)]
    last10 = cyc[-11:-1]          # (the run's last cycle has no head behind it: left out)
    print("launches per cycle (last 10):", [len(c) for c in last10])
    print("cycle span us (first start -> last end, last 10):", [round((c[-1][1] - c[0][0]) / 1e3, 1) for c in last10])
    print("sum of kernel durations us (last 10):", [round(sum(r[1] - r[0] for r in c) / 1e3, 1) for c in last10])
    agg = collections.OrderedDict()
    for c in last10:
        for i, r in enumerate(c):
            agg.setdefault((i, r[2], r[3]), []).append((r[1] - r[0]) / 1e3)
    print("\ntimeline of a cycle (position, kernel, grid size, mean us over the last 10 cycles, gap to the previous launch's end in the last cycle):")
    lc = last10[-1]
    for i, r in enumerate(lc):
        d = agg.get((i, r[2], r[3]), [0])
        gap = (r[0] - lc[i - 1][1]) / 1e3 if i else 0.0
        print("%3d %-52s grid %9s  %7.1f us   gap %5.1f" % (i, r[2][:52], r[3], sum(d) / len(d), gap))


if __name__ == "__main__":
    if sys.argv[1] == "ab":
        run_ab(sys.argv[2].split(","), int(sys.argv[3]) if len(sys.argv) > 3 else 8)
    elif sys.argv[1] == "trace":
        trace(int(sys.argv[2]))
    elif sys.argv[1] == "timeline":
        timeline(sys.argv[2])
    else:
        sys.exit(__doc__)
