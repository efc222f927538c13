"""The accelerated solve loop (gmg_config::accelerate = 0..4) on the large workloads: cycles to the tolerance, and ms per iteration of the
accelerated loop against the plain loop -- same process, alternating, warmed up, fixed-length loops (tol = 0).  Default configuration otherwise.
One JSON file per workload under profiles/accel/ (or --out).
  python scripts/accel_cycles.py [--only poisson_3M,bilaplacian_3M_tau1e-9,bilaplacian_3M_tau1e-3,pointcloud_2M] [--small]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from gravo_mg_amd import cabi, meshgen

DEPTHS = (0, 1, 2, 3, 4)


def workloads(small):
    n = 190 if small else 1732
    def mesh():
        V, F = meshgen.torus_mesh(n, n)
        S, mass = meshgen.cotan_laplacian(V, F)
        return V, S, mass
    def poisson():
        V, S, mass = mesh()
        return (V, S, mass) + tuple(meshgen.poisson_system(S, mass, tau=1e-6, seed=42, d=1))          # bench.py's flagship system
    def bilap(tau):
        def make():
            V, S, mass = mesh()
            return (V, S, mass) + tuple(meshgen.smoothing_system(meshgen.bilaplacian(S, mass), mass, V[:, :1], tau=tau))      # bench.py's Bilaplacian variant
        return make
    def cloud():
        P = meshgen.torus_points(30_000 if small else 2_000_000, noise=0.0005)
        S, mass = meshgen.knn_graph_laplacian(P, 8)
        return (P, S, mass) + tuple(meshgen.poisson_system(S, mass))
    tag = "36k" if small else "3M"
    return {f"poisson_{tag}": (poisson, 1e-4), f"bilaplacian_{tag}_tau1e-9": (bilap(1e-9), 1e-4), f"bilaplacian_{tag}_tau1e-3": (bilap(1e-3), 1e-4),
            ("pointcloud_30k" if small else "pointcloud_2M"): (cloud, 1e-4)}


def measure(name, make, tol, max_iter, loop, reps):
    t = time.perf_counter()
    pos, S, mass, lhs, rhs = make()
    H = cabi.Hierarchy(pos, meshgen.neighbors_from_stiffness(S), ratio=8.0, lower_bound=1000)
    rhs = np.asfortranarray(rhs)
    print(f"[accel] {name}: n={lhs.shape[0]} nnz={lhs.nnz} d={rhs.shape[1]} built in {time.perf_counter() - t:.1f} s", flush=True)
    out = {"workload": name, "n": int(lhs.shape[0]), "nnz": int(lhs.nnz), "d": int(rhs.shape[1]), "tol": tol, "max_iter": max_iter, "stop_type": 2,
           "loop_iterations": loop, "depths": {},
           "note": "ms_per_iteration = loop time / iterations of a tol = 0 solve; for accelerate > 0 that loop ends with ONE confirmation (the ordinary residual "
                   "check + a wait), so its cost is spread over loop_iterations; the plain loop's check is part of every cycle"}
    engs = {}
    for m in DEPTHS:
        eng = cabi.Engine(accelerate=m)
        eng.use_hierarchy(H); eng.set_mass(mass); eng.set_system(lhs)
        engs[m] = eng
    xbuf = np.empty(rhs.shape, order="F")
    for m in DEPTHS:
        eng = engs[m]
        x, it, res, conv = eng.solve(rhs, tol=tol, stop_type=2, max_iter=max_iter, out=xbuf)
        true_res = eng.residual_norm(rhs, x, 2)
        marks = {f"{mark:g}": int(next((i + 1 for i, r in enumerate(conv[:, 1]) if r <= mark), -1)) for mark in (3e-2, 1e-2, 1e-3, 1e-4)}
        out["depths"][str(m)] = {"iterations": int(it), "residue": float(res), "residue_recomputed": float(true_res), "diverged": bool(eng.diverged),
                                 "first_residue": float(conv[0, 1]), "iterations_to": marks, "loop_ms": eng.timing("cycles"),
                                 "confirmations": eng.timing("accel_confirmations"), "guard_steps": eng.timing("accel_guard_steps"),
                                 "residues": [float(v) for v in (conv[:, 1] if len(conv) <= 16 else np.concatenate([conv[:8, 1], conv[-8:, 1]]))]}
        print(f"[accel] {name} accelerate={m}: {it} iterations, residue {res:.3e}, to 3e-2 in {marks['0.03']}, diverged {eng.diverged}", flush=True)
    # ms per iteration: fixed-length loops (tol = 0), the plain loop and each depth alternating in the same process
    ms = {m: [] for m in DEPTHS}
    for m in DEPTHS:
        engs[m].solve(rhs, tol=0.0, stop_type=2, max_iter=loop, out=xbuf)                  # warm-up (vectors of the accelerated loop allocated)
    for r in range(reps):
        for m in DEPTHS:
            eng = engs[m]
            x, it, res, conv = eng.solve(rhs, tol=0.0, stop_type=2, max_iter=loop, out=xbuf)
            ms[m].append(eng.timing("cycles") / max(it, 1))                              # (a plain loop that blows up stops early: per iteration it ran)
    for m in DEPTHS:
        d = out["depths"][str(m)]
        d["ms_per_iteration"] = [float(v) for v in ms[m]]
        d["ms_per_iteration_median"] = float(np.median(ms[m]))
        d["ms_minus_plain_median"] = float(np.median(ms[m]) - np.median(ms[0]))        # a difference of medians, in ms
        d["ms_ratio_to_plain_median"] = float(np.median(ms[m]) / np.median(ms[0]))
        print(f"[accel] {name} accelerate={m}: {d['ms_per_iteration_median']:.4f} ms per iteration (plain loop {np.median(ms[0]):.4f})", flush=True)
    for e in engs.values():
        e.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--small", action="store_true", help="36 k-row stand-ins (a quick functional run of this script)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accel"))
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--loop", type=int, default=30, help="iterations per timed loop")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    todo = workloads(args.small)
    for name, (make, tol) in todo.items():
        if args.only and name not in args.only.split(","):
            continue
        res = measure(name, make, tol, args.max_iter, args.loop, args.reps)
        with open(os.path.join(args.out, name + ".json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
