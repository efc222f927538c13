"""What the V-cycle's launch code enqueues, as a comparable record: the same calls on the same small problems, every time.

    python scripts/launch_sequence.py [shape ...]          # the driver: one line per call (iterate digests, residue histories, timing keys)
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/launch_sequence.py
    python scripts/launch_sequence.py --reduce TRACE.csv [--list OUT.txt]      # ONE trace: DIR/<host>/<pid>_kernel_trace.csv of the driver's process

The driver walks the entry points that reach the cycle's launch helpers (solve, run_cycles, vcycle, smooth_residual, profile_cycle) over the
shapes and configurations at which those helpers hand something to one another: the head of the next cycle and both folds on a two-colour
level 0 (chain64), the fused restriction, the residual from the sweep and the interleaved copy (chain193 with three transfer levels; chain131072
for the entry-parallel form of the fused restriction, which needs a level of 65 536 rows), levels on which nothing is eligible (chain1, a
diagonal operator), a many-colour level 0 (clique65), and 1, 3 and 5 right-hand sides (5: two groups of columns, the folds and the head decline).  Two builds of the library enqueue the same launches exactly when both their printed lines and their
reduced traces agree: --reduce turns a kernel trace into the ordered list of (kernel, grid, workgroup, LDS bytes) of the gmgk:: kernels -- the
cycle's stream; the one kernel of the second stream is gmgs::rap_rows -- and prints its length and SHA-256."""
import csv
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [      # (name, tests/problems.synthetic_problem arguments, engine arguments): the specs of tests/test_gpu_boundary_shapes.py
    ("chain64", dict(graph=("chain", 64), sizes=[64, 16], kind="poisson", prolong=("pc",)), {}),
    ("chain193", dict(graph=("chain", 193), sizes=[193, 96, 24, 6], kind="smoothing", prolong=("smooth", "pc", "pc")), {}),
    ("chain1", dict(graph=("chain", 1), sizes=[1, 1], kind="poisson", prolong=("pc",)), {}),
    ("clique65", dict(graph=("clique", 48, 48, 65), sizes=[2369, 592, 148], kind="smoothing", prolong=("pc",)), dict(block_fine=False)),
    ("diagonal100", dict(graph=("diagonal", 100), sizes=[100, 25, 6], kind="poisson", prolong=("pc",)), {}),
    # (a level 1 of 65 536 rows keeps the entry-parallel sweep under the quad-layout restriction: the fused restriction in its restrict_sweep0 form)
    ("chain131072", dict(graph=("chain", 131072), sizes=[131072, 65536, 1024, 16], kind="smoothing", prolong=("smooth", "pc", "pc")), {}),
]
COLUMNS = (1, 3, 5)
CONFIGS = [
    ("default", {}), ("no-head", dict(speculate_head=False)), ("no-fused-restriction", dict(fuse_restrict_sweep=False)), ("graph", dict(use_graph=True)),
    ("mixed", dict(inner_precision=1)), ("jacobi", dict(smoother=1)), ("chebyshev", dict(smoother=2)), ("exact-gs", dict(block_rows=0)),
    ("lane-per-row-no-ep", dict(block_ep=False, block_lanes=1)), ("quad", dict(block_lanes=4)), ("host-ldlt", dict(coarse_mode=0)),
    ("accelerate2", dict(accelerate=2)),
    # (one lane per row: these small levels take the layout of big ones, whose entry-parallel block sweep is what the residual from the sweep, the
    # interleaved copy of level 1's x and the restriction fused into restrict_sweep0 belong to)
    ("lane-per-row", dict(block_lanes=1)), ("lane-per-row-graph", dict(block_lanes=1, use_graph=True)),
] + [("%ssweeps-%d-%d" % (name, a, b), dict(kw, pre_iters=a, post_iters=b)) for name, kw in (("", {}), ("lane-per-row-", dict(block_lanes=1)))
     for a in (0, 1, 2) for b in (0, 1, 2)]
TIMING_KEYS = ("heads_enqueued", "head_decision_differs", "restrict_sweeps_fused", "residual_from_sweep")


def digest(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()[:16]


def drive(only=()):
    import numpy as np
    from gravo_mg_amd import cabi
    from tests import problems

    def timings(eng):
        out = []
        for k in TIMING_KEYS:
            try:
                out.append("%s=%g" % (k, eng.timing(k)))
            except cabi.GmgError:
                out.append("%s=-" % k)
        return " ".join(out)

    def call(eng, tag, what, f):
        """One entry point: f() returns (arrays, numbers); the arrays are printed as digests, the numbers in full, then the timing keys."""
        try:
            arrays, numbers = f()
            print(tag, what, "|", " ".join(digest(a) for a in arrays), "|", " ".join(repr(float(t)) for t in np.ravel(numbers)), "|", timings(eng), flush=True)
        except cabi.GmgError as e:
            print(tag, what, "| error:", e, flush=True)

    def solve(eng, rhs, **kw):
        x, it, res, conv = eng.solve(rhs, **kw)
        return [x], np.concatenate([[it, res], conv[:, 1]])            # (conv[:, 0]: milliseconds)

    for sname, spec, skw in SHAPES:
        if only and sname not in only:
            continue
        for d in COLUMNS:
            P = problems.synthetic_problem(d=d, **spec)
            rng = np.random.default_rng(11)
            for cname, ckw in CONFIGS:
                eng = cabi.Engine(**dict(skw, **ckw))
                eng.set_prolongations(P.U); eng.set_mass(P.mass); eng.set_system(P.lhs)
                tag = "%s d=%d %s" % (sname, d, cname)
                call(eng, tag, "solve-1e-6", lambda: solve(eng, P.rhs, tol=1e-6))
                call(eng, tag, "solve-3-cycles", lambda: solve(eng, P.rhs, tol=1e-30, max_iter=3))
                call(eng, tag, "solve-first-cycle", lambda: solve(eng, P.rhs, tol=1e30))

                def cycles(n, stop):
                    eng.load_problem(P.rhs, P.rhs)
                    res = eng.run_cycles(n, stop)
                    return [eng.fetch_solution()], res
                call(eng, tag, "run_cycles-3-2", lambda: cycles(3, 2))
                call(eng, tag, "run_cycles-2-none", lambda: cycles(2, -1))
                call(eng, tag, "vcycle", lambda: ([eng.vcycle(P.rhs, P.rhs)], []))
                for k in (0, 1):
                    if k >= eng.num_levels:
                        continue
                    n_k = eng.level_info(k)["n"]
                    b = rng.standard_normal((n_k, d)); x = rng.standard_normal((n_k, d))
                    call(eng, tag, "smooth_residual-%d-zero" % k, lambda: (eng.smooth_residual(k, b, None, 2, from_zero=True), []))
                    call(eng, tag, "smooth_residual-%d" % k, lambda: (eng.smooth_residual(k, b, x, 2), []))

                def profile():
                    eng.load_problem(P.rhs, P.rhs)
                    eng.profile_cycle(2, 2)            # (the legs' times are no part of the record)
                    return [eng.fetch_solution()], []
                call(eng, tag, "profile_cycle", profile)
                eng.close()


def reduce_trace(path, list_out=None):
    """The dispatches of the gmgk:: kernels in the order they were made (one stream: the order they ran in)."""
    keyed = []
    with open(path, newline="") as f:
        reader = csv.DictReader(f)
        order = "Dispatch_Id" if "Dispatch_Id" in reader.fieldnames else "Start_Timestamp"
        lds = "LDS_Block_Size" if "LDS_Block_Size" in reader.fieldnames else "Group_Segment_Size"
        for r in reader:
            name = r["Kernel_Name"]
            if "gmgk::" not in name:
                continue
            grid = "x".join(r["Grid_Size_" + a] for a in "XYZ")
            wg = "x".join(r["Workgroup_Size_" + a] for a in "XYZ")
            keyed.append((int(r[order]), "%s grid %s workgroup %s lds %s" % (name, grid, wg, r[lds])))
    keyed.sort(key=lambda t: t[0])
    lines = [t[1] for t in keyed]
    text = "\n".join(lines) + "\n"
    if list_out:
        open(list_out, "w").write(text)
    print("%d launches, sha256 %s" % (len(lines), hashlib.sha256(text.encode()).hexdigest()))


if __name__ == "__main__":
    if "--reduce" in sys.argv:
        args = sys.argv[sys.argv.index("--reduce") + 1:]
        list_out = None
        if "--list" in args:
            j = args.index("--list")
            list_out = args[j + 1]
            del args[j:j + 2]
        if len(args) != 1:
            sys.exit("--reduce takes exactly one kernel trace, the driver's process (got %d: %s)" % (len(args), " ".join(args)))
        reduce_trace(args[0], list_out)
    else:
        drive(sys.argv[1:])
