"""The Chebyshev smoother (gmg_config::smoother = GMG_SMOOTHER_CHEBYSHEV) on the large workloads, against the default handle and the exact
Gauss-Seidel handle (block_rows = 0, gs_omega = 1): iterations to 1e-4, ms per iteration (fixed-length loops, tol = 0, warmed up, alternating in
one process), ms to the tolerance, with degrees 2 + 2 and 3 + 3, plain and with accelerate = 3; "setup_total" of a cold gmg_set_system
(prepare_structure = 0) with and without the level-0 colouring.  With --scan every Chebyshev handle is also run at each interval ratio of
RATIOS (per handle through gmg_debug_set "cheby_ratio": the process-wide GMG_CHEBY_RATIO is read once) and the cycles to 1e-4 go to
ratio_scan.json -- the scan kChebyRatio (csrc/cheby_coeffs.hpp) is chosen from.  One JSON file per workload under profiles/cheby/ (or --out).
  python scripts/cheby_cycles.py [--configs 4 5b 5 3 6] [--scan] [--small]
Configs are gravo_mg_amd/meshgen.baseline_config's: 4 / 4r the 3 M mesh Poisson (natural / random order), 2 the 722 k mesh, 1 the demos' 36 k
smoothing call, 3 the 2 M point cloud, 6 the irregular 1 M sphere, 5b / 5 the 3 M Bilaplacian with tau = 1e-9 / 1e-3."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from gravo_mg_amd import cabi, meshgen

RATIOS = (2, 3, 4, 6, 8, 12, 16, 30)
TOL = 1e-4


def small_config(cfg):
    """36 k-row stand-ins: a quick functional run of this script."""
    V, F = meshgen.torus_mesh(190, 190, order="random" if cfg == "4r" else "natural")
    S, mass = meshgen.cotan_laplacian(V, F)
    if cfg in ("5", "5b"):
        lhs, rhs = meshgen.smoothing_system(meshgen.bilaplacian(S, mass), mass, V[:, :1], tau=1e-3 if cfg == "5" else 1e-9)
    elif cfg == "1":
        lhs, rhs = meshgen.smoothing_system(S, mass, V)
    else:
        lhs, rhs = meshgen.poisson_system(S, mass)
    return "small stand-in of cfg" + cfg, V, S, mass, lhs, rhs


def run(eng, rhs, xbuf, max_iter, loop, reps):
    x, it, res, conv = eng.solve(rhs, tol=TOL, stop_type=2, max_iter=max_iter, out=xbuf)
    rec = {"iterations": int(it), "residue": float(res), "reached": bool(res <= TOL), "diverged": bool(eng.diverged),
           "residues": [float(v) for v in (conv[:, 1] if len(conv) <= 12 else np.concatenate([conv[:6, 1], conv[-6:, 1]]))]}
    eng.solve(rhs, tol=0.0, stop_type=2, max_iter=loop, out=xbuf)
    ms = []
    for _ in range(reps):
        x, it2, _, _ = eng.solve(rhs, tol=0.0, stop_type=2, max_iter=loop, out=xbuf)
        ms.append(eng.timing("cycles") / max(it2, 1))
    rec["ms_per_iteration"] = float(np.median(ms))
    rec["ms_to_tolerance"] = float(np.median(ms) * it) if rec["reached"] else None
    return rec


def measure(cfg, args):
    t = time.perf_counter()
    name, pos, S, mass, lhs, rhs = small_config(cfg) if args.small else meshgen.baseline_config(cfg)
    H = cabi.Hierarchy(pos, meshgen.neighbors_from_stiffness(S), ratio=8.0, lower_bound=1000)
    rhs = np.asfortranarray(rhs)
    xbuf = np.empty(rhs.shape, order="F")
    print(f"[cheby] {name}: n={lhs.shape[0]} nnz={lhs.nnz} d={rhs.shape[1]} built in {time.perf_counter() - t:.1f} s", flush=True)
    out = {"config": cfg, "workload": name, "n": int(lhs.shape[0]), "nnz": int(lhs.nnz), "d": int(rhs.shape[1]), "tol": TOL, "max_iter": args.max_iter,
           "stop_type": 2, "loop_iterations": args.loop, "handles": {}, "cold_setup_total_ms": {}}
    scan = {"config": cfg, "workload": name, "cycles_to_1e-4": {}}

    def engine(**kw):
        eng = cabi.Engine(**kw)
        eng.use_hierarchy(H); eng.set_mass(mass); eng.set_system(lhs)
        return eng

    for label, kw in (("default", {}), ("exact_gs", dict(block_rows=0, gs_omega=1.0))):
        eng = engine(**kw)
        out["handles"][label] = run(eng, rhs, xbuf, args.max_iter, args.loop, args.reps)
        eng.close()
        print(f"[cheby] {label}: {out['handles'][label]}", flush=True)
    for deg in (2, 3):
        for acc in (0, 3):
            eng = engine(smoother=cabi.SMOOTHER_CHEBYSHEV, pre_iters=deg, post_iters=deg, accelerate=acc)
            label = f"chebyshev_{deg}+{deg}" + ("_accelerate3" if acc else "")
            rec = run(eng, rhs, xbuf, args.max_iter, args.loop, args.reps)
            rec["cheby_ratio"] = eng.timing("cheby_ratio")
            rec["cheby_lambda"] = [eng.timing("cheby_lambda_l%d" % k) for k in range(eng.num_levels)]
            out["handles"][label] = rec
            print(f"[cheby] {label}: {rec}", flush=True)
            if args.scan and acc == 0:
                row = {}
                for ratio in RATIOS:
                    eng.debug_set("cheby_ratio", float(ratio))
                    x, it, res, conv = eng.solve(rhs, tol=TOL, stop_type=2, max_iter=args.max_iter, out=xbuf)
                    row[str(ratio)] = {"cycles": int(it) if res <= TOL else None, "residue": float(res), "diverged": bool(eng.diverged)}
                eng.debug_set("cheby_ratio", 0.0)
                scan["cycles_to_1e-4"][f"{deg}+{deg}"] = row
                print(f"[cheby] ratio scan {deg}+{deg}: " + "  ".join(f"{r}:{v['cycles']}" for r, v in row.items()), flush=True)
            eng.close()
    for label, kw in (("default", {}), ("chebyshev_2+2", dict(smoother=cabi.SMOOTHER_CHEBYSHEV))):
        eng = cabi.Engine(prepare_structure=False, **kw)
        eng.use_hierarchy(H); eng.set_mass(mass); eng.set_system(lhs)
        out["cold_setup_total_ms"][label] = eng.timing("setup_total")
        eng.close()
    print(f"[cheby] cold setup_total: {out['cold_setup_total_ms']}", flush=True)
    return out, scan


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["4", "5b", "5", "3", "6"])
    ap.add_argument("--scan", action="store_true", help="also scan the interval ratio (ratio_scan.json)")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cheby"))
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--loop", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    scan_path = os.path.join(args.out, "ratio_scan.json")
    scans = json.load(open(scan_path)) if os.path.exists(scan_path) else {"ratios": list(RATIOS), "tol": TOL, "workloads": {}}
    for cfg in args.configs:
        res, scan = measure(cfg, args)
        with open(os.path.join(args.out, f"cfg{cfg}.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        if args.scan:
            scans["workloads"]["cfg" + cfg] = scan
            with open(scan_path, "w") as f:
                json.dump(scans, f, indent=1)
                f.write("\n")
