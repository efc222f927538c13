#!/usr/bin/env python3
"""One time step of the demos' loop -- new system values, then a solve -- timed two ways on the same engine configuration:

  host:   gmg_set_system (a values-only refresh: the pattern is the live one) + gmg_solve_x0_rhs from host arrays, and
  device: gmg_set_system_values_device + gmg_solve_device from resident torch tensors,

at the benchmark's 3 M-vertex torus with d = 3 right-hand sides.  Both paths alternate inside one process (same machine state), every step
ends with the stream drained (both solve calls return after it), the first `--warmup` steps of each path are dropped, medians and spreads of
the rest are reported.  The results of the last step of both paths are compared bit for bit.  Needs a GPU; there is nothing to fall back to.

    python scripts/device_io_step.py [--n1 1732 --n2 1732 --d 3 --steps 12 --warmup 3 --out profiles/device_io/step_3m_d3.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n1", type=int, default=1732)
    ap.add_argument("--n2", type=int, default=1732)
    ap.add_argument("--d", type=int, default=3)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lower-bound", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_io", "step_3m_d3.json"))
    args = ap.parse_args()

    from gravo_mg_amd import cabi, meshgen
    if cabi.device_count() < 1:
        raise SystemExit("device_io_step.py needs a HIP device")
    import torch

    V, F = meshgen.torus_mesh(args.n1, args.n2)
    S, mass = meshgen.cotan_laplacian(V, F)
    H = cabi.Hierarchy(V, meshgen.neighbors_from_stiffness(S), ratio=8.0, lower_bound=args.lower_bound)
    S = sp.csc_matrix(S); S.sort_indices()
    n = S.shape[0]
    col = np.repeat(np.arange(n), np.diff(S.indptr))
    m, s = np.where(S.indices == col, mass[col], 0.0), S.data.astype(np.float64)
    indptr, indices = S.indptr.astype(np.int32), S.indices.astype(np.int32)
    rng = np.random.default_rng(42)
    rhs = np.asfortranarray(mass[:, None] * rng.standard_normal((n, args.d)))      # column-major: what the C-ABI takes without a copy
    taus = [1e-3 * (1.0 + 0.1 * k) for k in range(args.steps)]

    engs = []
    for _ in range(2):
        eng = cabi.Engine()
        eng.use_hierarchy(H); eng.set_mass(mass)
        eng.set_system(sp.csc_matrix((m + taus[0] * s, indices, indptr), shape=(n, n)))
        engs.append(eng)
    host, dev = engs
    m_t, s_t = torch.tensor(m, device="cuda:0"), torch.tensor(s, device="cuda:0")
    b_t = torch.tensor(np.ascontiguousarray(rhs), device="cuda:0")                  # torch-contiguous (n, d)
    x_t = torch.empty_like(b_t)
    x_h = np.empty(rhs.shape, order="F")
    torch.cuda.synchronize()

    rows = {"host": [], "device": []}
    for k, tau in enumerate(taus):
        lhs = sp.csc_matrix((m + tau * s, indices, indptr), shape=(n, n))            # (composing the matrix is the application's, outside both timers)
        t0 = time.perf_counter()
        host.set_system(lhs)
        t1 = time.perf_counter()
        _, it_h, res_h, _ = host.solve(rhs, tol=1e-4, stop_type=2, max_iter=100, out=x_h)
        t2 = time.perf_counter()
        assert host.timing("setup_values_only") == 1.0
        rows["host"].append({"set_system_ms": (t1 - t0) * 1e3, "solve_ms": (t2 - t1) * 1e3, "step_ms": (t2 - t0) * 1e3, "iterations": it_h,
                             "upload_A0_ms": host.timing("t_upload_A0"), "solve_load_ms": host.timing("solve_load"),
                             "solve_fetch_ms": host.timing("solve_fetch"), "cycles_ms": host.timing("cycles")})
        vals = m_t + tau * s_t
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev.set_system_values_device(vals.data_ptr(), vals.numel())
        t1 = time.perf_counter()
        it_d, res_d, _ = dev.solve_device(b_t.data_ptr(), b_t.stride(), x_t.data_ptr(), x_t.stride(), args.d, tol=1e-4, stop_type=2, max_iter=100)
        t2 = time.perf_counter()
        assert dev.timing("setup_values_only") == 1.0
        rows["device"].append({"set_values_ms": (t1 - t0) * 1e3, "solve_ms": (t2 - t1) * 1e3, "step_ms": (t2 - t0) * 1e3, "iterations": it_d,
                               "solve_load_ms": dev.timing("solve_load"), "solve_fetch_ms": dev.timing("solve_fetch"), "cycles_ms": dev.timing("cycles")})
    same = bool(np.array_equal(x_t.cpu().numpy().view(np.uint64), np.ascontiguousarray(x_h).view(np.uint64))) and it_h == it_d and res_h == res_d

    def summary(rs):
        rs = rs[args.warmup:]
        return {key: {"median": statistics.median(r[key] for r in rs), "min": min(r[key] for r in rs), "max": max(r[key] for r in rs)} for key in rs[0]}

    out = {"workload": f"torus {args.n1} x {args.n2}", "n": n, "nnz": int(S.nnz), "d": args.d, "steps": args.steps, "warmup": args.warmup,
           "values_MB": S.nnz * 8 / 1e6, "vector_MB": n * args.d * 8 / 1e6, "same_bits_last_step": same,
           "host": summary(rows["host"]), "device": summary(rows["device"]), "raw": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("workload", "n", "nnz", "d", "same_bits_last_step")} |
                     {"host_step_ms": out["host"]["step_ms"], "device_step_ms": out["device"]["step_ms"],
                      "host_upload_A0_ms": out["host"]["upload_A0_ms"], "host_solve_load_ms": out["host"]["solve_load_ms"]}))


if __name__ == "__main__":
    main()
