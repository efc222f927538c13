"""gmg_config::reorder_pointwise and gmg_config::zero_guess_step measured (profiles/pointwise/), against the parent commit in the same job.

    python scripts/pointwise_ab.py job 4,4r,3,6,5b,5 --parent-tree DIR [--rounds 2] [--small]   # the job: per workload and round one process on the
                                                                                           # parent's tree, then one on this tree; one JSON line each
    python scripts/pointwise_ab.py run CFG [--tree DIR] [--small]                           # one such process (one workload, one tree)
    python scripts/pointwise_ab.py table FILE.jsonl                                         # the tables of DESIGN.md 5d / 5e from a job's lines

--parent-tree / --tree: a checkout of the parent commit with its library built (the configuration struct grew by the two fields, so this tree's
Python mirror refuses the parent's library through GMG_LIB_PATH: the parent runs with its own mirror).  A tree whose cabi.Engine does not know the
fields measures the handles with neither field alone.

Per process: the workload and its hierarchy are built once; the handles are Chebyshev 2 + 2 plain, with accelerate = 3 and with pcg = 1, each with
neither, either and both fields set, and the default (Gauss-Seidel) handle.  Per handle: iterations to 1e-4 (stop type 2, x0 = rhs), ms per
iteration from tol = 0 loops of --loop iterations with the handles ALTERNATING, warmed up, every sample kept (the job's own run-to-run spread is
what the two trees' neither-field rows are compared by); the first gmg_set_system of a handle whose structure was prepared at
gmg_finalize_hierarchy and a cold one (prepare_structure = 0; a second handle, made after a warm-up handle of the same configuration has loaded
the code objects); the launch count of one cycle -- the nodes (kernels, memsets, copies) of the cycle's captured graph on a use_graph = 1 twin
(timing key "graph_nodes").  Configs are gravo_mg_amd/meshgen.baseline_config's (scripts/cheby_cycles.py lists them); 4r is the 3 M mesh in
random vertex order."""
import argparse
import inspect
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
FIELDS = ((0, 0), (1, 0), (0, 1), (1, 1))          # (reorder_pointwise, zero_guess_step)
LOOPS = (("plain", {}), ("accelerate3", dict(accelerate=3)), ("pcg", dict(pcg=1)))


def small_config(meshgen, cfg):
    """36 k-row stand-ins: a quick functional run of this script (scripts/cheby_cycles.py::small_config, here without importing this tree's scripts)."""
    V, F = meshgen.torus_mesh(190, 190, order="random" if cfg == "4r" else "natural")
    S, mass = meshgen.cotan_laplacian(V, F)
    if cfg in ("5", "5b"):
        lhs, rhs = meshgen.smoothing_system(meshgen.bilaplacian(S, mass), mass, V[:, :1], tau=1e-3 if cfg == "5" else 1e-9)
    elif cfg == "3":
        P = meshgen.torus_points(36000, noise=0.002)
        S, mass = meshgen.knn_graph_laplacian(P, 8)
        lhs, rhs = meshgen.poisson_system(S, mass)
        V = P
    else:
        lhs, rhs = meshgen.poisson_system(S, mass)
    return "small stand-in of cfg" + cfg, V, S, mass, lhs, rhs


def run(args):
    tree = os.path.abspath(args.tree or ROOT)
    sys.path.insert(0, tree)
    import numpy as np
    from gravo_mg_amd import cabi, meshgen
    if cabi.device_count() < 1:
        raise SystemExit("pointwise_ab.py needs a HIP device")
    has_fields = "zero_guess_step" in inspect.signature(cabi.Engine.__init__).parameters
    t = time.perf_counter()
    name, pos, S, mass, lhs, rhs = small_config(meshgen, args.cfg) if args.small else meshgen.baseline_config(args.cfg)
    H = cabi.Hierarchy(pos, meshgen.neighbors_from_stiffness(S), ratio=8.0, lower_bound=1000)
    rhs = np.asfortranarray(rhs)
    xbuf = np.empty(rhs.shape, order="F")
    print(f"[pointwise] {name}: n={lhs.shape[0]} nnz={lhs.nnz} d={rhs.shape[1]} built in {time.perf_counter() - t:.1f} s ({tree})", file=sys.stderr, flush=True)
    cheb = dict(smoother=cabi.SMOOTHER_CHEBYSHEV, pre_iters=2, post_iters=2)

    def key(loop, f):
        return f"{loop}/reorder{f[0]}-zero{f[1]}"

    def kwargs(loop_kw, f):
        kw = dict(cheb, **loop_kw)
        if has_fields:
            kw.update(reorder_pointwise=f[0], zero_guess_step=f[1])
        return kw

    def engine(prepared=True, **kw):
        eng = cabi.Engine(prepare_structure=int(prepared), **kw)
        t0 = time.perf_counter(); eng.use_hierarchy(H); eng.set_mass(mass); t1 = time.perf_counter()
        eng.set_system(lhs)
        return eng, 1e3 * (time.perf_counter() - t1), 1e3 * (t1 - t0)

    def timing(eng, k):
        try:
            return eng.timing(k)
        except cabi.GmgError:
            return None

    out = {"config": args.cfg, "workload": name, "tree": "this" if tree == ROOT else "parent", "has_fields": has_fields, "n": int(lhs.shape[0]), "nnz": int(lhs.nnz),
           "d": int(rhs.shape[1]), "tol": TOL, "max_iter": args.max_iter, "loop_iterations": args.loop, "reps": args.reps, "handles": {}}
    fields = FIELDS if has_fields else FIELDS[:1]
    engs = {}
    warm, _, _ = engine(**cheb)                           # loads the code objects, warms the pools: no handle below pays for that
    warm.solve(rhs, tol=TOL, stop_type=2, max_iter=3, out=xbuf)
    for loop, loop_kw in LOOPS:
        for f in fields:
            eng, ms_set, ms_hier = engine(**kwargs(loop_kw, f))
            engs[key(loop, f)] = eng
            out["handles"][key(loop, f)] = {"prepared_set_system_ms": ms_set, "use_hierarchy_ms": ms_hier,
                                            "fine_level_reordered": timing(eng, "fine_level_reordered"), "base_order_choice": timing(eng, "base_order_choice")}
    engs["default"], ms_set, ms_hier = engine()
    out["handles"]["default"] = {"prepared_set_system_ms": ms_set, "use_hierarchy_ms": ms_hier}
    # cold set-ups and launch counts: per field combination, on the plain loop's configuration (the loops share the cycle; pcg: its own cycle graph)
    for f in fields:
        cold, ms_cold, _ = engine(prepared=False, **kwargs({}, f))
        out["handles"][key("plain", f)]["cold_set_system_ms"] = ms_cold
        cold.close()
        for loop, loop_kw in (LOOPS[0], LOOPS[2]):
            g, _, _ = engine(use_graph=True, **kwargs(loop_kw, f))
            g.solve(rhs, tol=0.0, stop_type=2, max_iter=2, out=xbuf)
            out["handles"][key(loop, f)]["cycle_graph_nodes"] = timing(g, "graph_nodes")
            g.close()
    for label, eng in engs.items():
        x, it, res, conv = eng.solve(rhs, tol=TOL, stop_type=2, max_iter=args.max_iter, out=xbuf)
        out["handles"][label].update({"iterations": int(it), "residue": float(res), "reached": bool(res <= TOL), "diverged": bool(eng.diverged)})
        for k in ("zero_guess_steps", "restrict_steps_fused"):
            out["handles"][label][k] = timing(eng, k)
    ms = {label: [] for label in engs}
    for eng in engs.values():
        eng.solve(rhs, tol=0.0, stop_type=2, max_iter=args.loop, out=xbuf)
    for _ in range(args.reps):
        for label, eng in engs.items():
            x, it, res, conv = eng.solve(rhs, tol=0.0, stop_type=2, max_iter=args.loop, out=xbuf)
            ms[label].append(eng.timing("cycles") / max(it, 1))
    for label in engs:
        rec = out["handles"][label]
        rec["ms_per_iteration"] = [float(v) for v in ms[label]]
        rec["ms_per_iteration_median"] = float(np.median(ms[label]))
        rec["ms_to_tolerance"] = float(np.median(ms[label]) * rec["iterations"]) if rec["reached"] else None
    for e in list(engs.values()) + [warm]:
        e.close()
    print(json.dumps(out), flush=True)


def job(args):
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, ("small_" if args.small else "") + "ab.jsonl")
    t_job, longest = time.perf_counter(), 0.0
    for cfg in args.cfgs.split(","):
        for rnd in range(args.rounds):
            for tree in (args.parent_tree, ROOT):
                # (--budget: a job that must end by itself starts no process it cannot expect to finish, and no half pair)
                if args.budget and tree == args.parent_tree and time.perf_counter() - t_job + 2.6 * max(longest, 40.0) > args.budget:
                    print(f"[pointwise] budget of {args.budget} s: stopping in front of cfg {cfg} round {rnd}", flush=True)
                    return
                t_child = time.perf_counter()
                cmd = [sys.executable, os.path.abspath(__file__), "run", cfg, "--tree", tree, "--max-iter", str(args.max_iter), "--loop", str(args.loop),
                       "--reps", str(args.reps)] + (["--small"] if args.small else [])
                env = dict(os.environ)
                env.pop("GMG_LIB_PATH", None)
                p = subprocess.run(cmd, stdout=subprocess.PIPE, env=env, timeout=args.child_timeout)
                if p.returncode != 0:              # (a child that failed ends the job: nothing more is started on the device behind it)
                    raise SystemExit(f"pointwise_ab.py: the run of cfg {cfg} on {tree} ended with status {p.returncode}")
                longest = max(longest, time.perf_counter() - t_child)
                line = p.stdout.decode().strip().splitlines()[-1]
                rec = json.loads(line)
                rec["round"] = rnd
                with open(path, "a") as f:
                    f.write(json.dumps(rec) + "\n")
                h = rec["handles"]
                print(f"[pointwise] cfg {cfg} round {rnd} {rec['tree']}: " + "  ".join(f"{k} {v['iterations']} x {v['ms_per_iteration_median']:.3f}" for k, v in h.items()), flush=True)


def table(args):
    import statistics
    recs = [json.loads(l) for l in open(args.file) if l.strip()]
    for cfg in dict.fromkeys(r["config"] for r in recs):
        rows = [r for r in recs if r["config"] == cfg]
        print(f"\ncfg {cfg}: {rows[0]['workload']} (n = {rows[0]['n']})")
        labels = list(dict.fromkeys(k for r in rows for k in r["handles"]))
        for label in labels:
            cells = []
            for tree in ("parent", "this"):
                hs = [r["handles"][label] for r in rows if r["tree"] == tree and label in r["handles"]]
                if not hs:
                    continue
                samples = [v for h in hs for v in h["ms_per_iteration"]]
                med = statistics.median(samples)
                it = hs[0]["iterations"] if hs[0]["reached"] else None
                cells.append(f"{tree}: {it if it is not None else 'not reached'} x {med:.3f} ms (samples {min(samples):.3f} .. {max(samples):.3f})"
                             + (f" = {it * med:.2f} ms" if it is not None else "")
                             + "".join(f", {k} {hs[0][k]:.1f}" for k in ("prepared_set_system_ms", "cold_set_system_ms") if hs[0].get(k) is not None)
                             + (f", nodes {hs[0]['cycle_graph_nodes']:.0f}" if hs[0].get("cycle_graph_nodes") is not None else ""))
            print(f"  {label:28s} " + " | ".join(cells))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    a = sub.add_parser("run"); a.add_argument("cfg"); a.add_argument("--tree", default=None)
    b = sub.add_parser("job"); b.add_argument("cfgs"); b.add_argument("--parent-tree", required=True); b.add_argument("--rounds", type=int, default=2)
    b.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointwise")); b.add_argument("--child-timeout", type=int, default=500)
    b.add_argument("--budget", type=float, default=0.0, help="seconds this job may take (0: no limit)")
    for p in (a, b):
        p.add_argument("--small", action="store_true", help="36 k-row stand-ins (a quick functional run of this script)")
        p.add_argument("--max-iter", type=int, default=100)
        p.add_argument("--loop", type=int, default=20, help="iterations per timed loop")
        p.add_argument("--reps", type=int, default=5)
    c = sub.add_parser("table"); c.add_argument("file")
    args = ap.parse_args()
    {"run": run, "job": job, "table": table}[args.mode](args)
