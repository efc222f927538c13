"""The cases behind tests/golden/own_row_loads/*.npz, shared by scripts/record_own_row_loads.py (which wrote the fixtures from the build BEFORE
the SELL row-dot kernels requested a row's own operands -- diag, b, x_i / y_i, weight -- in front of its dot product) and
tests/test_gpu_own_row_loads.py (which replays them bit for bit).  Moving a load changes no operand and no operation, so every number below
must come out with the same bits.

A case = one problem, one engine configuration, one stop type; its workload (run):
    load_problem(rhs, rhs), run_cycles(1), run_cycles(1) again (two steps, each with its check), fetch_solution  -> "cycles_hist", "cycles_x"
    solve(tol = the second step's residue, a little loosened; at most 50 iterations)                          -> "solve_x", "solve_it", "solve_res",
                                                                                                                  "solve_hist", "solve_dev" (x on the device)
    solve(tol = 1e300): stops at its first check -- the launch enqueued ahead of the decision must leave x    -> "first_x", "first_dev", "first_res"
                                                                                                                  the checked iterate

Shapes: jittered tori of 7 x 9 = 63 vertices (one slice with a padding row; every colour class smaller than a slice), 8 x 8 = 64 and 24 x 24; a
400-vertex hull-triangulated sphere (slices of differing width); the long-link chain "flagged-8" of tests/colcode_cases.py (level 0 with slices
flagged one by one: row_dot_sel mode 2).  Hierarchies (HIERARCHY: ratio, lower_bound): 24 x 24 with ratio 3 and lower_bound 30 has the three
levels 576 / 137 / 35 (quad-layout transfers and coarse operators); the default ratio 8 leaves the other meshes a single level, so they take
ratio 2 and lower_bound 8 (63 / 13, 64 / 16, 400 / ~100 / ...).

Storage (pack / check): an array of at most FULL_BYTES is stored whole; a larger one as its SHA-256 digest (bitwise equality of the whole array)
plus a strided sample of rows (so that a mismatch says where and by how much).  The chain's iterate alone is 720 kB per column."""
import hashlib

import numpy as np

import functools

from gravo_mg_amd import cabi as _cabi, meshgen
from tests import colcode_cases as cc
from tests import problems

GOLDEN_DIR = "tests/golden/own_row_loads"
FULL_BYTES = 576 * 8
SAMPLE_ROWS = 64

TORI = {"torus63": (7, 9), "torus64": (8, 8), "torus576": (24, 24)}
HIERARCHY = {"torus63": (2.0, 8), "torus64": (2.0, 8), "torus576": (3.0, 30), "sphere400": (2.0, 8)}
GROUPS = tuple(TORI) + ("sphere400", "chain-flagged")
COLOUR_SWEEPS = dict(block_rows=0)          # colour sweeps on every level (no block sweeps: gs_color / gs_color_residual below level 0 too)


def _torus_cases(group):
    small = group != "torus576"
    out = []
    for d in (1, 2, 3, 4, 5):                                                # (5 runs the 4 + 1 chunks)
        out.append((f"d{d}", d, 2, {}))
    for d in (1, 3):
        out.append((f"d{d}-omega1", d, 2, dict(gs_omega=1.0)))
        out.append((f"d{d}-colours", d, 2, dict(COLOUR_SWEEPS)))
        out.append((f"d{d}-colours-omega1", d, 2, dict(COLOUR_SWEEPS, gs_omega=1.0)))
        out.append((f"d{d}-fp32inner", d, 2, dict(inner_precision=1)))
        out.append((f"d{d}-nofold", d, 2, dict(fold_head=0)))
        out.append((f"d{d}-nospeculate", d, 2, dict(speculate_head=0)))
    for t in (0, 1, 3):                                                      # (2 is every case above; 0 and 2 weigh rows by the mass)
        out.append((f"d1-stop{t}", 1, t, {}))
        if small:
            out.append((f"d3-stop{t}-omega1", 3, t, dict(gs_omega=1.0)))
    out.append(("d2-nofold-omega1-stop0", 2, 0, dict(fold_head=0, gs_omega=1.0)))
    return out


def cases(group):
    """[(name, d, stop_type, engine keywords)] of a group."""
    if group in TORI:
        return _torus_cases(group)
    if group == "sphere400":
        return [("d1", 1, 2, {}), ("d3", 3, 2, {}), ("d1-colours", 1, 2, dict(COLOUR_SWEEPS)), ("d3-omega1-stop3", 3, 3, dict(gs_omega=1.0)),
                ("d1-fp32inner", 1, 2, dict(inner_precision=1))]
    if group == "chain-flagged":
        kw = cc.engine_settings("flagged-8")
        return [("d1", 1, 2, dict(kw)), ("d3-omega1", 3, 2, dict(kw, gs_omega=1.0)), ("d2-nofold-stop0", 2, 0, dict(kw, fold_head=0))]
    raise ValueError(group)


@functools.lru_cache(maxsize=None)
def _mesh_problem(group):
    V, F = meshgen.torus_mesh(*TORI[group]) if group in TORI else meshgen.sphere_mesh(400)
    S, mass = meshgen.cotan_laplacian(V, F)
    ratio, lower_bound = HIERARCHY[group]
    H = _cabi.Hierarchy(V, meshgen.neighbors_from_stiffness(S), ratio=ratio, lower_bound=lower_bound)
    lhs, _ = meshgen.poisson_system(S, mass)
    return problems.Problem(V, S, mass, H.U, lhs, None, group)


def problem(group, d):
    """(Problem, rhs with d columns)."""
    if group in HIERARCHY:
        P = _mesh_problem(group)
        assert len(P.U) >= (2 if group == "torus576" else 1), (group, [u.shape for u in P.U])
        return P, np.asfortranarray(np.random.default_rng(3).standard_normal((P.n, d)) * P.mass[:, None])
    P = cc.problem("flagged-8")
    return P, np.asfortranarray(P.rhs[:, :d])


def engine(cabi, P, kw):
    e = cabi.Engine(**kw)
    e.set_prolongations(P.U); e.set_mass(P.mass); e.set_system(P.lhs)
    return e


def run(eng, rhs, stop_type):
    out = {}
    eng.load_problem(rhs, rhs)
    h1 = eng.run_cycles(1, stop_type).copy()
    h2 = eng.run_cycles(1, stop_type).copy()
    out["cycles_hist"] = np.concatenate([np.ravel(h1), np.ravel(h2)])
    out["cycles_x"] = eng.fetch_solution()
    tol = float(np.ravel(h2)[-1]) * (1.0 + 1e-9)
    x, it, r, conv = eng.solve(rhs, tol=tol, stop_type=stop_type, max_iter=50)
    out["solve_x"], out["solve_it"], out["solve_res"] = x.copy(), np.array([it], np.int64), np.array([r])
    out["solve_hist"], out["solve_dev"] = np.array(conv[:it, 1], np.float64), eng.fetch_solution()
    x, it, r, conv = eng.solve(rhs, tol=1e300, stop_type=stop_type, max_iter=50)
    assert it == 1, it
    out["first_x"], out["first_res"], out["first_dev"] = x.copy(), np.array([r]), eng.fetch_solution()
    return out


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64) if np.asarray(a).dtype.kind == "f" else np.ascontiguousarray(a)


def _rows(a):
    a = np.asarray(a)
    a = a.reshape(a.shape[0], -1) if a.ndim else a.reshape(1, 1)
    return np.ascontiguousarray(a)


def bits(a):
    """The bit patterns of an array as rows x columns."""
    return _u64(_rows(a))


def pack(prefix, fields):
    """{key: array} to store for a case's fields."""
    out = {}
    for k, a in fields.items():
        a = _rows(a)
        if a.nbytes <= FULL_BYTES:
            out[f"{prefix}/{k}"] = a
        else:
            out[f"{prefix}/{k}#sha256"] = np.frombuffer(hashlib.sha256(_u64(a).tobytes()).digest(), np.uint8)
            out[f"{prefix}/{k}#sample"] = a[::max(1, a.shape[0] // SAMPLE_ROWS)][:, :1].copy()
            out[f"{prefix}/{k}#shape"] = np.array(a.shape, np.int64)
    return out


def check(prefix, fields, golden):
    """Every field of a replayed case against the stored one, bit for bit; returns the number of compared entries."""
    n = 0
    for k, a in fields.items():
        a = _rows(a)
        if f"{prefix}/{k}" in golden:
            g = golden[f"{prefix}/{k}"]
            assert g.shape == a.shape and g.dtype == a.dtype, (prefix, k, g.shape, a.shape)
            bad = np.flatnonzero(_u64(g).ravel() != _u64(a).ravel())
            assert len(bad) == 0, (prefix, k, len(bad), a.ravel()[bad[:4]], g.ravel()[bad[:4]])
        else:
            assert tuple(golden[f"{prefix}/{k}#shape"]) == a.shape, (prefix, k)
            s = a[::max(1, a.shape[0] // SAMPLE_ROWS)][:, :1]
            g = golden[f"{prefix}/{k}#sample"]
            bad = np.flatnonzero(_u64(g).ravel() != _u64(s).ravel())
            assert len(bad) == 0, (prefix, k, "sample", len(bad), s.ravel()[bad[:4]], g.ravel()[bad[:4]])
            digest = np.frombuffer(hashlib.sha256(_u64(a).tobytes()).digest(), np.uint8)
            assert np.array_equal(digest, golden[f"{prefix}/{k}#sha256"]), (prefix, k, "digest of the whole array")
        n += a.size
    return n
