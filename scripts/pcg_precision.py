"""gmg_config::precond_precision on the large workloads: the CG loop of gmg_config::pcg = 1 with its preconditioner cycle in fp64 (0) and in
fp32 (1), the two handles ALTERNATING in one process, warmed up, median of --reps repetitions.  Per workload: iterations to 1e-4 (at most
--max-iter) x ms per iteration from fixed-length loops (tol = 0) for both, the device bytes each handle holds after its solves (their difference
is what the fp32 twins and fp32 level vectors add, less the one fp64 vector the mode does not allocate), and gmg_set_system cold and values-only
for both.  One JSON file per workload under profiles/pcg_precision/ (or --out).
  python scripts/pcg_precision.py [--configs 4 5b 5 6 3] [--small] [--only 0]
Configs are gravo_mg_amd/meshgen.baseline_config's (scripts/cheby_cycles.py lists them); config 5 (Bilaplacian, tau = 1e-3) is also timed over
loops of 100 and 1000 iterations; config 3 (the point cloud) runs with reorder_pointwise and zero_guess_step on.  --only 0 measures the
precond_precision = 0 handle alone and sets no new field: the same script then runs on the parent commit, which makes "0 is the parent" a
timing statement."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from gravo_mg_amd import cabi, meshgen
from scripts.cheby_cycles import small_config

TOL = 1e-4
CHEB = dict(smoother=cabi.SMOOTHER_CHEBYSHEV, pre_iters=2, post_iters=2, pcg=1)


def measure(cfg, args):
    t = time.perf_counter()
    name, pos, S, mass, lhs, rhs = small_config(cfg) if args.small else meshgen.baseline_config(cfg)
    H = cabi.Hierarchy(pos, meshgen.neighbors_from_stiffness(S), ratio=8.0, lower_bound=1000)
    rhs = np.asfortranarray(rhs)
    xbuf = np.empty(rhs.shape, order="F")
    print(f"[precision] {name}: n={lhs.shape[0]} nnz={lhs.nnz} d={rhs.shape[1]} built in {time.perf_counter() - t:.1f} s", flush=True)
    extra = dict(reorder_pointwise=1, zero_guess_step=1) if cfg == "3" else {}
    loops = [args.loop] + ([100, 1000] if cfg == "5" else [])
    max_iter = 1000 if cfg == "5" else args.max_iter
    out = {"config": cfg, "workload": name, "n": int(lhs.shape[0]), "nnz": int(lhs.nnz), "d": int(rhs.shape[1]), "tol": TOL, "max_iter": max_iter,
           "stop_type": 2, "reps": args.reps, "options": dict(CHEB, **extra), "handles": {}}
    settings = [0, 1] if args.only is None else [args.only]
    engs = {}
    for p in settings:
        label = f"precond_precision_{p}"
        eng = cabi.Engine(**dict(CHEB, **extra), **({"precond_precision": p} if args.only is None else {}))
        eng.use_hierarchy(H); eng.set_mass(mass)
        t = time.perf_counter(); eng.set_system(lhs); cold = (time.perf_counter() - t) * 1e3
        refresh = []
        for _ in range(3):
            t = time.perf_counter(); eng.set_system(lhs); refresh.append((time.perf_counter() - t) * 1e3)
        out["handles"][label] = {"set_system_cold_ms": cold, "set_system_values_only_ms": refresh, "set_system_values_only_ms_median": float(np.median(refresh))}
        print(f"[precision] {label}: set_system cold {cold:.1f} ms, values-only {np.median(refresh):.1f} ms", flush=True)
        engs[label] = eng
    for label, eng in engs.items():
        x, it, res, conv = eng.solve(rhs, tol=TOL, stop_type=2, max_iter=max_iter, out=xbuf)
        rec = out["handles"][label]
        rec.update({"iterations": int(it), "residue": float(res), "residue_recomputed": float(eng.residual_norm(rhs, x, 2)), "reached": bool(res <= TOL),
                    "diverged": bool(eng.diverged), "solve_loop_ms": eng.timing("cycles"), "device_bytes": eng.timing("device_bytes_now")})
        rec.update({k: eng.timing(k) for k in ("pcg_confirmations", "pcg_guard_steps", "pcg_restarts")})
        print(f"[precision] {label}: {it} iterations, residue {res:.3e}, reached {rec['reached']}, loop {rec['solve_loop_ms']:.1f} ms, {rec['device_bytes'] / 2**20:.0f} MiB", flush=True)
    for loop in loops:
        ms = {label: [] for label in engs}
        for eng in engs.values():
            eng.solve(rhs, tol=0.0, stop_type=2, max_iter=min(loop, 30), out=xbuf)              # warm-up
        for _ in range(args.reps):
            for label, eng in engs.items():
                x, it, res, conv = eng.solve(rhs, tol=0.0, stop_type=2, max_iter=loop, out=xbuf)
                ms[label].append(eng.timing("cycles") / max(it, 1))
        for label in engs:
            rec = out["handles"][label].setdefault("loops", {})
            rec[str(loop)] = {"ms_per_iteration": [float(v) for v in ms[label]], "ms_per_iteration_median": float(np.median(ms[label]))}
            print(f"[precision] {label}: {np.median(ms[label]):.4f} ms per iteration over {loop}", flush=True)
    for label in engs:
        rec = out["handles"][label]
        rec["ms_per_iteration_median"] = rec["loops"][str(args.loop)]["ms_per_iteration_median"]
        rec["ms_to_tolerance"] = rec["ms_per_iteration_median"] * rec["iterations"] if rec["reached"] else None
    if len(engs) == 2:
        a, b = out["handles"]["precond_precision_0"], out["handles"]["precond_precision_1"]
        out["fp32_over_fp64_ms_per_iteration"] = b["ms_per_iteration_median"] / a["ms_per_iteration_median"]
        out["device_bytes_added"] = b["device_bytes"] - a["device_bytes"]
        print(f"[precision] fp32 / fp64 per iteration {out['fp32_over_fp64_ms_per_iteration']:.3f}, bytes added {out['device_bytes_added'] / 2**20:.0f} MiB", flush=True)
    for e in engs.values():
        e.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["4", "5b", "5", "6", "3"])
    ap.add_argument("--small", action="store_true", help="36 k-row stand-ins (a quick functional run of this script)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcg_precision"))
    ap.add_argument("--only", type=int, default=None, choices=[0], help="the precond_precision = 0 handle alone, no new field set (runs on the parent commit too)")
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--loop", type=int, default=30, help="iterations per timed loop")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    for cfg in args.configs:
        res = measure(cfg, args)
        with open(os.path.join(args.out, ("small_" if args.small else "") + f"cfg{cfg}" + ("_only0" if args.only is not None else "") + ".json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
