"""The preconditioned CG solve loop (gmg_config::pcg = 1) on the large workloads, against the default handle, the plain Chebyshev loop and the
accelerated one: iterations to 1e-4 (at most --max-iter) and ms per iteration from fixed-length loops (tol = 0), the handles ALTERNATING in one
process, warmed up, median of --reps repetitions.  Handles: the default one; Chebyshev 2 + 2 plain, with accelerate = 3, with accelerate = 2 (the
cost the PCG iteration is compared against: DESIGN.md 5e) and with pcg = 1.  One JSON file per workload under profiles/pcg/ (or --out).
  python scripts/pcg_cycles.py [--configs 4 5b 5 3 6] [--small]
Configs are gravo_mg_amd/meshgen.baseline_config's (scripts/cheby_cycles.py lists them)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from gravo_mg_amd import cabi, meshgen
from scripts.cheby_cycles import small_config

TOL = 1e-4
CHEB = dict(smoother=cabi.SMOOTHER_CHEBYSHEV, pre_iters=2, post_iters=2)
HANDLES = (("default", {}), ("chebyshev_2+2", CHEB), ("chebyshev_2+2_accelerate3", dict(CHEB, accelerate=3)),
           ("chebyshev_2+2_accelerate2", dict(CHEB, accelerate=2)), ("chebyshev_2+2_pcg", dict(CHEB, pcg=1)))


def measure(cfg, args):
    t = time.perf_counter()
    name, pos, S, mass, lhs, rhs = small_config(cfg) if args.small else meshgen.baseline_config(cfg)
    H = cabi.Hierarchy(pos, meshgen.neighbors_from_stiffness(S), ratio=8.0, lower_bound=1000)
    rhs = np.asfortranarray(rhs)
    xbuf = np.empty(rhs.shape, order="F")
    print(f"[pcg] {name}: n={lhs.shape[0]} nnz={lhs.nnz} d={rhs.shape[1]} built in {time.perf_counter() - t:.1f} s", flush=True)
    out = {"config": cfg, "workload": name, "n": int(lhs.shape[0]), "nnz": int(lhs.nnz), "d": int(rhs.shape[1]), "tol": TOL, "max_iter": args.max_iter,
           "stop_type": 2, "loop_iterations": args.loop, "reps": args.reps, "handles": {},
           "note": "ms_per_iteration = loop time / iterations of a tol = 0 solve, median over the repetitions; the accelerated and the PCG loop end with ONE "
                   "confirmation (the ordinary residual check + a wait) whose cost is spread over loop_iterations; the plain loops' check is part of every cycle"}
    engs = {}
    for label, kw in HANDLES:
        eng = cabi.Engine(**kw)
        eng.use_hierarchy(H); eng.set_mass(mass); eng.set_system(lhs)
        engs[label] = eng
    for label, eng in engs.items():
        x, it, res, conv = eng.solve(rhs, tol=TOL, stop_type=2, max_iter=args.max_iter, out=xbuf)
        rec = {"iterations": int(it), "residue": float(res), "residue_recomputed": float(eng.residual_norm(rhs, x, 2)), "reached": bool(res <= TOL),
               "diverged": bool(eng.diverged), "loop_ms": eng.timing("cycles"),
               "residues": [float(v) for v in (conv[:, 1] if len(conv) <= 16 else np.concatenate([conv[:8, 1], conv[-8:, 1]]))]}
        if label.endswith("_pcg"):
            rec.update({k: eng.timing(k) for k in ("pcg", "pcg_confirmations", "pcg_guard_steps", "pcg_restarts")})
        out["handles"][label] = rec
        print(f"[pcg] {label}: {it} iterations, residue {res:.3e}, reached {rec['reached']}, diverged {eng.diverged}", flush=True)
    ms = {label: [] for label in engs}
    for eng in engs.values():
        eng.solve(rhs, tol=0.0, stop_type=2, max_iter=args.loop, out=xbuf)                  # warm-up (the loops' own vectors allocated)
    for _ in range(args.reps):
        for label, eng in engs.items():
            x, it, res, conv = eng.solve(rhs, tol=0.0, stop_type=2, max_iter=args.loop, out=xbuf)
            ms[label].append(eng.timing("cycles") / max(it, 1))                            # (a loop that blows up stops early: per iteration it ran)
    for label in engs:
        rec = out["handles"][label]
        rec["ms_per_iteration"] = [float(v) for v in ms[label]]
        rec["ms_per_iteration_median"] = float(np.median(ms[label]))
        rec["ms_to_tolerance"] = float(np.median(ms[label]) * rec["iterations"]) if rec["reached"] else None
        print(f"[pcg] {label}: {rec['ms_per_iteration_median']:.4f} ms per iteration, to the tolerance {rec['ms_to_tolerance']}", flush=True)
    a2 = out["handles"]["chebyshev_2+2_accelerate2"]["ms_per_iteration_median"]
    out["pcg_ms_over_accelerate2_ms"] = out["handles"]["chebyshev_2+2_pcg"]["ms_per_iteration_median"] / a2
    for e in engs.values():
        e.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["4", "5b", "5", "3", "6"])
    ap.add_argument("--small", action="store_true", help="36 k-row stand-ins (a quick functional run of this script)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcg"))
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--loop", type=int, default=30, help="iterations per timed loop")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    for cfg in args.configs:
        res = measure(cfg, args)
        with open(os.path.join(args.out, ("small_" if args.small else "") + f"cfg{cfg}.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
