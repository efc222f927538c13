"""GMG_COARSE_DEVICE_TRIANGLE against GMG_COARSE_DEVICE_INVERSE at the coarsest sizes of the bench workloads (those of scripts/symv_sweep.py).

  python scripts/coarse_triangle.py [--out DIR] [--parent-lib PATH] [--workloads 36k-d3,36k-d1,...] [--rounds N]

Per workload one process measures BOTH modes, alternating, N rounds each: the coarsest leg of profile_cycle(2, 20), the cycle time in loops of
100 after warm-up, set_system, coarse_inverse_ms with its tile-kernel share and coarse_inverse_bytes; the spread of the rounds stands next to
every median.  --parent-lib: a libgravomg_hip.so built from the parent commit; mode 1 is then measured with it as well (GMG_LIB_PATH, a process of
its own) -- that is the yardstick, and it shows that the existing path did not move.  At n_L = 6 005 (36 k) a further process runs the new mode
with non-temporal instead of plain loads of the matrix (GMG_TRI_NT=1, read once per process).  Writes <out>/<workload>.json; default out:
profiles/coarse_triangle."""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"36k-d3": (190, 190, "smoothing", 3), "36k-d1": (190, 190, "poisson", 1), "152k-d3": (390, 390, "smoothing", 3),
             "722k-d1": (850, 850, "poisson", 1), "3M-d1": (1732, 1732, "poisson", 1), "3M-d3": (1732, 1732, "smoothing", 3)}


def measure(name, modes, rounds):
    """One process: the engines of `modes` on one problem, measured in turn, `rounds` times."""
    from gravo_mg_amd import cabi, meshgen
    n1, n2, kind, d = WORKLOADS[name]
    V, F = meshgen.torus_mesh(n1, n2)
    S, mass = meshgen.cotan_laplacian(V, F)
    H = cabi.Hierarchy(V, meshgen.neighbors_from_stiffness(S), lower_bound=1000)
    lhs, rhs = (meshgen.smoothing_system(S, mass, V) if kind == "smoothing" else meshgen.poisson_system(S, mass, d=d))
    engines, out = {}, {}
    for mode in modes:
        eng = cabi.Engine(coarse_mode=mode)
        eng.use_hierarchy(H); eng.set_mass(mass)
        t = time.perf_counter(); eng.set_system(lhs); cold = 1e3 * (time.perf_counter() - t)
        L = eng.num_levels
        out[mode] = {"n_L": eng.level_info(L)["n"], "set_system_cold_ms": cold, "set_system_ms": [], "coarse_inverse_ms": [], "coarse_inverse_tiles_ms": [],
                     "coarsest_leg_us": [], "cycle_us": []}
        try:
            out[mode]["coarse_inverse_bytes"] = eng.timing("coarse_inverse_bytes")
        except Exception:          # (a library from before the key)
            out[mode]["coarse_inverse_bytes"] = 8.0 * out[mode]["n_L"] * ((out[mode]["n_L"] + 7) // 8 * 8)
        eng.load_problem(rhs, rhs); eng.run_cycles(20, 2)
        engines[mode] = eng
    for r in range(rounds):
        for mode in modes:
            eng, o = engines[mode], out[mode]
            lhs2 = lhs.copy(); lhs2.data *= 1.0 + 1e-3 * (r + 1)
            t = time.perf_counter(); eng.set_system(lhs2); o["set_system_ms"].append(1e3 * (time.perf_counter() - t))
            o["coarse_inverse_ms"].append(eng.timing("coarse_inverse_ms")); o["coarse_inverse_tiles_ms"].append(eng.timing("coarse_inverse_tiles_ms"))
            eng.load_problem(rhs, rhs); eng.run_cycles(10, 2)
            t = time.perf_counter(); eng.run_cycles(100, 2); o["cycle_us"].append(1e4 * (time.perf_counter() - t))
            o["coarsest_leg_us"].append(1e3 * float(eng.profile_cycle(2, 20)[eng.num_levels]))
    for eng in engines.values():
        eng.close()
    for o in out.values():
        for k in ("set_system_ms", "coarse_inverse_ms", "coarse_inverse_tiles_ms", "coarsest_leg_us", "cycle_us"):
            v = o.pop(k)
            o[k] = {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}
    return {str(m): o for m, o in out.items()}


def child(name, modes, rounds, env):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--modes", ",".join(map(str, modes)), "--rounds", str(rounds)]
    p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **env), timeout=900)
    if p.returncode:
        raise SystemExit(f"{name} {env}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")       # (nothing more is started after a failure)
    return json.loads(p.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coarse_triangle"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", default=None)
    ap.add_argument("--modes", default="1,3")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.child, [int(m) for m in a.modes.split(",")], a.rounds)))
        sys.exit(0)
    os.makedirs(a.out, exist_ok=True)
    for name in a.workloads.split(","):
        res = {"workload": name, "rounds": a.rounds, "this_commit": child(name, [1, 3], a.rounds, {})}
        if a.parent_lib:
            res["parent_commit_mode_1"] = child(name, [1], a.rounds, {"GMG_LIB_PATH": os.path.abspath(a.parent_lib)})["1"]
        if name.startswith("36k"):
            res["mode_3_nontemporal_loads"] = child(name, [3], a.rounds, {"GMG_TRI_NT": "1"})["3"]
        m1, m3 = res["this_commit"]["1"], res["this_commit"]["3"]
        line = f"{name}: n_L={m1['n_L']} leg {m1['coarsest_leg_us']['median']:.1f} -> {m3['coarsest_leg_us']['median']:.1f} us, cycle {m1['cycle_us']['median']:.1f} -> {m3['cycle_us']['median']:.1f} us, "
        line += f"inverse {m1['coarse_inverse_ms']['median']:.2f} -> {m3['coarse_inverse_ms']['median']:.2f} ms, bytes {m1['coarse_inverse_bytes']:.0f} -> {m3['coarse_inverse_bytes']:.0f}"
        if "parent_commit_mode_1" in res:
            line += f"; parent mode 1 leg {res['parent_commit_mode_1']['coarsest_leg_us']['median']:.1f} us cycle {res['parent_commit_mode_1']['cycle_us']['median']:.1f} us"
        if "mode_3_nontemporal_loads" in res:
            line += f"; mode 3 non-temporal loads leg {res['mode_3_nontemporal_loads']['coarsest_leg_us']['median']:.1f} us cycle {res['mode_3_nontemporal_loads']['cycle_us']['median']:.1f} us"
        print(line, flush=True)
        with open(os.path.join(a.out, name + ".json"), "w") as f:
            json.dump(res, f, indent=1)
