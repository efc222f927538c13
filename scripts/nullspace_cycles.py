"""gmg_config::nullspace = 1 measured (profiles/nullspace/): the pure stiffness matrix S on a nullspace = 1 handle against the reference's
workaround S + 1e-6 M (experiments/python/comparisons.py:76) on a nullspace = 0 handle of the same configuration -- the same mesh, hierarchy,
sparsity pattern and kernels.  Per pair of handles, ALTERNATING in one process, warmed up, medians of --reps repetitions:
  * cycles (iterations) to 1e-4 from x0 = rhs, stop type 2, and the residues;
  * ms per iteration from fixed-length loops (tol = 0);
  * gmg_set_system as a values-only refresh: setup_total and coarse_inverse_ms -- the nullspace handle's carry the row-sum check and the two
    centring kernels (gmgs::inverse_col_sums, gmgs::inverse_center), the other handle's do not;
  * a solve of ONE iteration (solve_call): the difference is what the two projections and the read-back of their sums cost per solve.
Pairs: the default handle; Chebyshev 2 + 2 with pcg = 1.  One JSON file per workload under profiles/nullspace/ (or --out).
  python scripts/nullspace_cycles.py [--configs 4] [--small]
Configs are gravo_mg_amd/meshgen.baseline_config's (scripts/cheby_cycles.py lists them); only their mesh is used."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.sparse as sp
from gravo_mg_amd import cabi, meshgen
from scripts.cheby_cycles import small_config

TOL = 1e-4
CHEB_PCG = dict(smoother=cabi.SMOOTHER_CHEBYSHEV, pre_iters=2, post_iters=2, pcg=1)
PAIRS = (("default", {}), ("chebyshev_2+2_pcg", CHEB_PCG))


def measure(cfg, args):
    t = time.perf_counter()
    name, pos, S, mass, _, _ = small_config(cfg) if args.small else meshgen.baseline_config(cfg)
    H = cabi.Hierarchy(pos, meshgen.neighbors_from_stiffness(S), ratio=8.0, lower_bound=1000)
    pure = sp.csc_matrix(S); pure.sort_indices()
    workaround, rhs = meshgen.poisson_system(S, mass)                       # S + 1e-6 M, rhs = M y
    rhs = np.asfortranarray(rhs + 0.01 * mass.mean())                       # ... with a constant added
    xbuf = np.empty(rhs.shape, order="F")
    print(f"[nullspace] {name}: n={pure.shape[0]} nnz={pure.nnz} d={rhs.shape[1]} built in {time.perf_counter() - t:.1f} s", flush=True)
    out = {"config": cfg, "workload": name, "n": int(pure.shape[0]), "nnz": int(pure.nnz), "d": int(rhs.shape[1]), "tol": TOL, "max_iter": args.max_iter,
           "stop_type": 2, "loop_iterations": args.loop, "reps": args.reps, "pairs": {},
           "note": "per pair: 'nullspace' = pure S on a nullspace = 1 handle, 'workaround' = S + 1e-6 M on a nullspace = 0 handle; the handles alternate in "
                   "every timed loop; ms_per_iteration = loop time / iterations of a tol = 0 solve; refresh_* = gmg_set_system with the live pattern"}
    for label, kw in PAIRS:
        engs = {"nullspace": (cabi.Engine(nullspace=1, **kw), pure), "workaround": (cabi.Engine(**kw), workaround)}
        rec = {}
        for who, (eng, lhs) in engs.items():
            eng.use_hierarchy(H); eng.set_mass(mass); eng.set_system(lhs)
            x, it, res, conv = eng.solve(rhs, tol=TOL, stop_type=2, max_iter=args.max_iter, out=xbuf)
            rec[who] = {"iterations": int(it), "residue": float(res), "reached": bool(res <= TOL), "diverged": bool(eng.diverged),
                        "residues": [float(v) for v in conv[:16, 1]], "levels": int(eng.num_levels), "coarse_on_device": eng.timing("coarse_on_device")}
            if who == "nullspace":
                rec[who].update({k: eng.timing(k) for k in ("nullspace_rowsum_l0", "nullspace_rowsum_coarse", "nullspace_pinned_pivot", "nullspace_rhs_defect")})
                rec[who]["mass_weighted_mean_over_abs"] = float(np.abs(mass @ x).max() / (mass @ np.abs(x)).max())
            print(f"[nullspace] {label} {who}: {it} iterations, residue {res:.3e}", flush=True)
        ms = {who: [] for who in engs}
        one = {who: [] for who in engs}
        setup = {who: [] for who in engs}
        inverse = {who: [] for who in engs}
        for who, (eng, lhs) in engs.items():
            eng.solve(rhs, tol=0.0, stop_type=2, max_iter=args.loop, out=xbuf)                # warm-up (the loops' own vectors allocated)
        for _ in range(args.reps):
            for who, (eng, lhs) in engs.items():
                x, it, _, _ = eng.solve(rhs, tol=0.0, stop_type=2, max_iter=args.loop, out=xbuf)
                ms[who].append(eng.timing("cycles") / max(it, 1))
            for who, (eng, lhs) in engs.items():
                eng.solve(rhs, tol=0.0, stop_type=2, max_iter=1, out=xbuf)
                one[who].append(eng.timing("solve_call"))
            for who, (eng, lhs) in engs.items():
                eng.set_system(lhs)
                assert eng.timing("setup_values_only") == 1
                setup[who].append(eng.timing("setup_total")); inverse[who].append(eng.timing("coarse_inverse_ms"))
        for who in engs:
            rec[who].update({"ms_per_iteration_median": float(np.median(ms[who])), "ms_per_iteration": [float(v) for v in ms[who]],
                             "one_iteration_solve_call_ms_median": float(np.median(one[who])), "refresh_setup_total_ms_median": float(np.median(setup[who])),
                             "refresh_coarse_inverse_ms_median": float(np.median(inverse[who]))})
            rec[who]["ms_to_tolerance"] = rec[who]["ms_per_iteration_median"] * rec[who]["iterations"] if rec[who]["reached"] else None
        rec["projections_ms_per_solve"] = rec["nullspace"]["one_iteration_solve_call_ms_median"] - rec["workaround"]["one_iteration_solve_call_ms_median"]
        rec["centring_and_check_ms_per_setup"] = rec["nullspace"]["refresh_setup_total_ms_median"] - rec["workaround"]["refresh_setup_total_ms_median"]
        rec["centring_ms_in_coarse_inverse"] = rec["nullspace"]["refresh_coarse_inverse_ms_median"] - rec["workaround"]["refresh_coarse_inverse_ms_median"]
        out["pairs"][label] = rec
        print(f"[nullspace] {label}: ms per iteration {rec['nullspace']['ms_per_iteration_median']:.4f} (workaround {rec['workaround']['ms_per_iteration_median']:.4f}); "
              f"refresh {rec['nullspace']['refresh_setup_total_ms_median']:.3f} ms (workaround {rec['workaround']['refresh_setup_total_ms_median']:.3f}); "
              f"projections {rec['projections_ms_per_solve']:.4f} ms per solve", flush=True)
        for eng, _ in engs.values():
            eng.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["4"])
    ap.add_argument("--small", action="store_true", help="36 k-row stand-ins (a quick functional run of this script)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nullspace"))
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--loop", type=int, default=30, help="iterations per timed loop")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if cabi.device_count() < 1:
        raise SystemExit("nullspace_cycles.py needs a HIP device")
    os.makedirs(args.out, exist_ok=True)
    for cfg in args.configs:
        res = measure(cfg, args)
        with open(os.path.join(args.out, ("small_" if args.small else "") + f"cfg{cfg}.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
