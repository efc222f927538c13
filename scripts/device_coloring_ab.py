"""gmg_config::device_coloring measured (profiles/device_coloring/): per workload, option off / on, one JSON line with
  * the cold gmg_set_system in ms: median (and every sample) of several cold calls on one warm handle, each on a pattern digest the handle's
    ordering cache does not hold -- the system's pattern and the same pattern with one more coupling, alternating; no structure prepared;
  * device_coloring_ms and the rounds of the device colouring;
  * the number of colours and the class sizes of level 0;
  * ms per cycle (median of `loops` timed loops of 20 run_cycles steps) and the cycles of a solve to 1e-4 (M-norm stop).

    python scripts/device_coloring_ab.py 3m,3m-random,sphere1m,bilap3m [--reps 5] [--off-only]

--off-only measures the option-off column alone and passes no device_coloring argument: the form that runs on a tree from before the option
(copy this file into its scripts/), for the comparison against the parent commit in the same job."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gravo_mg_amd import cabi, meshgen  # noqa: E402

WORKLOADS = {"3m": "4", "3m-random": "4r", "sphere1m": "6", "bilap3m": "5", "722k": "2", "36k": "1"}      # meshgen.baseline_config


def timing(eng, key):
    try:
        return eng.timing(key)
    except cabi.GmgError:
        return None


def other_pattern(lhs):
    """lhs plus e (d_00 + d_kk - d_0k - d_k0), k = n / 2: positive semi-definite, one more coupling -- another pattern digest."""
    n = lhs.shape[0]
    k, e = n // 2, 1e-9 * abs(lhs[0, 0])
    E = sp.coo_matrix(([e, e, -e, -e], ([0, k, 0, k], [0, k, k, 0])), shape=lhs.shape)
    out = sp.csc_matrix(lhs + E)
    out.sort_indices()
    assert out.nnz == lhs.nnz + 2
    return out


def measure(H, mass, lhs, lhs_alt, rhs, option, reps, loops):
    kw = {} if option is None else {"device_coloring": option}
    eng = cabi.Engine(prepare_structure=0, **kw)
    eng.use_hierarchy(H); eng.set_mass(mass)
    eng.set_system(lhs_alt)                                   # warms the pools and the code objects
    cold, dev_ms = [], []
    for i in range(reps):                                     # (reps is odd: the last cold call leaves the system itself)
        a = lhs_alt if i % 2 else lhs
        t = time.perf_counter(); eng.set_system(a); cold.append(1e3 * (time.perf_counter() - t))
        assert eng.timing("setup_values_only") == 0.0 and eng.timing("setup_ordering_cached") == 0.0
        dev_ms.append(timing(eng, "device_coloring_ms"))
    new2old, cb = eng.level_ordering(0)
    sizes = [int((new2old[cb[c]:cb[c + 1]] >= 0).sum()) for c in range(len(cb) - 1)]
    B = np.asfortranarray(rhs)
    eng.load_problem(B, B); eng.run_cycles(3, 2)
    per_cycle = []
    for _ in range(loops):
        eng.load_problem(B, B)
        t = time.perf_counter(); eng.run_cycles(20, 2); per_cycle.append(1e3 * (time.perf_counter() - t) / 20)
    x, it, res, _ = eng.solve(B, tol=1e-4, stop_type=2, max_iter=100)
    out = {"cold_set_system_ms": round(statistics.median(cold), 3), "cold_samples_ms": [round(c, 3) for c in cold],
           "colored_on_device": timing(eng, "colored_on_device"), "colored_ahead": timing(eng, "setup_colored_ahead"),
           "device_coloring_ms": None if dev_ms[-1] is None else round(statistics.median(dev_ms), 3),
           "device_coloring_rounds": timing(eng, "device_coloring_rounds"), "wait_ordering_ms": round(eng.timing("setup_wait_ordering"), 3),
           "ordering_l0_ms": round(eng.timing("setup_ordering_l0"), 3), "colours": len(sizes), "class_sizes": sizes,
           "ms_per_cycle": round(statistics.median(per_cycle), 4), "ms_per_cycle_samples": [round(p, 4) for p in per_cycle],
           "cycles_to_1e-4": int(it), "residue": float(res), "reached": bool(res <= 1e-4 and not eng.diverged)}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--off-only", action="store_true")
    args = ap.parse_args()
    assert args.reps % 2 == 1
    if cabi.device_count() < 1:
        raise SystemExit("device_coloring_ab.py needs a HIP device")
    for w in args.workloads.split(","):
        name, pos, S, mass, lhs, rhs = meshgen.baseline_config(WORKLOADS[w])
        H = cabi.Hierarchy(pos, meshgen.neighbors_from_stiffness(S), ratio=8.0, lower_bound=1000)
        lhs_alt = other_pattern(lhs)
        line = {"workload": w, "name": name, "n": int(lhs.shape[0]), "nnz": int(lhs.nnz)}
        if args.off_only:
            line["off"] = measure(H, mass, lhs, lhs_alt, rhs, None, args.reps, args.loops)
        else:
            line["off"] = measure(H, mass, lhs, lhs_alt, rhs, 0, args.reps, args.loops)
            line["on"] = measure(H, mass, lhs, lhs_alt, rhs, 1, args.reps, args.loops)
        print(json.dumps(line), flush=True)
        del H, pos, S, mass, lhs, lhs_alt, rhs


if __name__ == "__main__":
    main()
