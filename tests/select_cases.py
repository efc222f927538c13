"""Hand-built inputs for the per-point parent selection of one hierarchy level (multigrid_solver.cpp:291-452), branch by branch, and the
checks that hold its three implementations together: the host routine (HierarchyBuilder::select_point), the device kernel
(gmgh::select_parents) -- both through gmg_debug_select_parents -- and the Python restatement (oracle/hierarchy_restatement.py::select_point).
Shared by tests/test_select_parents_host.py (CPU: host against restatement) and tests/test_gpu_select_parents.py (device against both).

Every decision that sits exactly on a boundary (a point on an edge, equidistant neighbours, a clamp) is built from small-integer or dyadic
coordinates and axis-aligned planes, so that it is exact in all three implementations: unit normals are (0, 0, +-1), the doubled areas
and the cross products are small integers, equal distances are equal bit for bit."""
import ctypes as C

import numpy as np

TRIANGLE, EDGE, CLOSEST, SINGLE, NESTED = 0, 1, 2, 3, 4
OVERFLOW = 255                      # cnt of a point the device stage hands back (more than 32 edge keys)


class Job:
    """One level's selection inputs in the layout of HierarchyOptions::SelectJob, plus what every point was built to reach."""

    def __init__(self, P, Pc, nearest, sample, cadj, tris, NBc, weighting=0, nested=0, expect=None, overflow=None):
        self.P = np.ascontiguousarray(P, np.float64).reshape(-1, 3)
        self.Pc = np.ascontiguousarray(Pc, np.float64).reshape(-1, 3)
        self.nf, self.nc = len(self.P), len(self.Pc)
        self.nearest = np.ascontiguousarray(nearest, np.int32)
        self.sample = np.ascontiguousarray(sample, np.int32)
        self.cadj_lists = [sorted(int(v) for v in a) for a in cadj]
        self.cadj_ptr = np.zeros(self.nc + 1, np.int32)
        self.cadj_ptr[1:] = np.cumsum([len(a) for a in self.cadj_lists])
        self.cadj = np.array([v for a in self.cadj_lists for v in a] + [0], np.int32)       # (+ one spare entry: never an empty array)
        self.tris_list = [tuple(int(v) for v in t) for t in tris]
        self.ntri = len(self.tris_list)
        self.tris = np.array([v for t in self.tris_list for v in t] + [0, 0, 0], np.int32)
        self.tris_of = [[] for _ in range(self.nc)]                  # every cell's triangles in ascending id, as the builder lists them
        for t, tri in enumerate(self.tris_list):
            for v in tri:
                self.tris_of[v].append(t)
        self.tof_ptr = np.zeros(self.nc + 1, np.int32)
        self.tof_ptr[1:] = np.cumsum([len(a) for a in self.tris_of])
        self.tof = np.array([t for a in self.tris_of for t in a] + [0], np.int32)
        self.NBc = np.ascontiguousarray(NBc, np.int32).reshape(self.nc, -1)
        self.Kc = self.NBc.shape[1]
        self.weighting, self.nested = int(weighting), int(nested)
        self.expect = expect                                         # per point (kind, cnt, cols or None), or None
        self.overflow = np.zeros(self.nf, bool) if overflow is None else np.asarray(overflow, bool)
        assert self.nearest.shape == (self.nf,) and self.sample.shape == (self.nc,)

    def run(self, cabi, mode):
        """gmg_debug_select_parents: mode 0 host routine, 1 device stage (raw records), 2 the builder's combination."""
        cnt = np.full(self.nf, 77, np.uint8); kind = np.full(self.nf, 77, np.uint8)
        col = np.full(3 * self.nf, -7, np.int32); w = np.full(3 * self.nf, np.nan)
        ub = lambda a: a.ctypes.data_as(C.POINTER(C.c_ubyte))
        rc = cabi.lib().gmg_debug_select_parents(self.nf, self.nc, self.Kc, self.ntri, self.weighting, self.nested, cabi._pd(self.P), cabi._pd(self.Pc),
                                                 cabi._pi(self.nearest), cabi._pi(self.sample), cabi._pi(self.cadj_ptr), cabi._pi(self.cadj),
                                                 cabi._pi(self.tris), cabi._pi(self.tof_ptr), cabi._pi(self.tof), cabi._pi(self.NBc), int(mode),
                                                 ub(cnt), ub(kind), cabi._pi(col), cabi._pd(w))
        if rc:
            raise cabi.GmgError(rc, f"gmg_debug_select_parents(mode={mode}) failed")
        return cnt, kind, col.reshape(-1, 3), w.reshape(-1, 3)

    def restatement(self, points=None):
        """The Python per-point reference for `points` (default: all): list of (cols, weights)."""
        from oracle import hierarchy_restatement as ref
        if not hasattr(self, "_normals"):
            self._normals = [ref.triangle_normal(self.Pc, t) for t in self.tris_list]
        NBc = self.NBc.astype(np.int64)
        return [ref.select_point(int(f), self.P, self.Pc, self.nearest, self.sample, self.cadj_lists, self.tris_list, self._normals, self.tris_of,
                                 NBc, weighting=self.weighting, nested=bool(self.nested)) for f in (range(self.nf) if points is None else points)]


# ------------------------------------------------------------------------------------------------------------- the checks
def _rows_differ(A, B, skip=None):
    """Indices of the points whose records differ bit for bit: cnt, kind, col[:cnt], w[:cnt] as uint64 (a signed zero counts).  Entries
    beyond cnt are not compared (the device does not write them)."""
    (ca, ka, cola, wa), (cb, kb, colb, wb) = A, B
    live = np.arange(3)[None, :] < np.minimum(ca, 3)[:, None]
    bad = (ca != cb) | (ka != kb) | ((cola != colb) & live).any(axis=1) | ((wa.view(np.uint64) != wb.view(np.uint64)) & live).any(axis=1)
    if skip is not None:
        bad &= ~skip
    return np.flatnonzero(bad)


def _describe(job, f, recs):
    out = [f"point {f} p={job.P[f].tolist()} cell {int(job.nearest[f])}"]
    for name, (cnt, kind, col, w) in recs:
        n = min(int(cnt[f]), 3)
        out.append(f"  {name}: cnt={int(cnt[f])} kind={int(kind[f])} col={col[f, :n].tolist()} w={w[f, :n].tolist()} bits={[hex(int(b)) for b in w[f, :n].view(np.uint64)]}")
    return "\n".join(out)


def check_expectation(job, host):
    """(d) every point reached the branch it was built for -- from the host routine's records, the specification."""
    cnt, kind, col, _ = host
    assert job.expect is not None
    for f, (k, n, cols) in enumerate(job.expect):
        assert (int(kind[f]), int(cnt[f])) == (k, n), f"point {f} was built for kind {k} with {n} parents, reached kind {int(kind[f])} with {int(cnt[f])}"
        if cols is not None:
            assert col[f, :n].tolist() == list(cols), f"point {f}: parents {col[f, :n].tolist()}, built for {list(cols)}"


def check_against_restatement(job, rec, name, points=None):
    """(c) same cnt, same columns in the same order, weights within the bounds tests/test_gpu_hierarchy.py uses for U."""
    cnt, _, col, w = rec
    points = list(range(job.nf)) if points is None else [int(f) for f in points]
    for f, (cols, weights) in zip(points, job.restatement(points)):
        n = int(cnt[f])
        assert n == len(cols) and col[f, :n].tolist() == [int(c) for c in cols], \
            f"{name} against the restatement, " + _describe(job, f, [(name, rec)]) + f"\n  restatement: col={cols} w={weights}"
        np.testing.assert_allclose(w[f, :n], weights, rtol=1e-9, atol=1e-12, err_msg=f"{name} against the restatement, point {f}")


def check_host(cabi, job, sample_points=None):
    """The half that needs no device: the host routine reaches the branches the case was built for and agrees with the restatement."""
    host = job.run(cabi, 0)
    assert host[0].min() >= 1 and host[0].max() <= 3 and host[1].max() <= 4
    if job.expect is not None:
        check_expectation(job, host)
    check_against_restatement(job, host, "host", sample_points)
    return host


def check_device(cabi, job, host, sample_points=None):
    """(a) device against host bit for bit, (b) the builder's combination, (c) device against the restatement."""
    dev = job.run(cabi, 1)
    over = dev[0] == OVERFLOW
    assert np.array_equal(over, job.overflow), f"points handed back by the device stage: {np.flatnonzero(over).tolist()}, built for {np.flatnonzero(job.overflow).tolist()}"
    bad = _rows_differ(host, dev, skip=over)
    assert bad.size == 0, f"{bad.size} device rows differ from the host's, first:\n" + _describe(job, bad[0], [("host  ", host), ("device", dev)])
    both = job.run(cabi, 2)
    bad = _rows_differ(host, both)
    assert bad.size == 0, f"{bad.size} rows of the builder's combination differ from the host's, first:\n" + _describe(job, bad[0], [("host    ", host), ("combined", both)])
    pts = np.arange(job.nf) if sample_points is None else np.asarray(sample_points)
    check_against_restatement(job, dev, "device", pts[~over[pts]])
    return dev


# ------------------------------------------------------------------------------------------------------------- building scenes
class Scene:
    """Several independent configurations in one job: each brings its own cells (local indices, shifted on insertion -- the order of the
    keys inside a configuration is kept), triangles, table rows and points."""

    def __init__(self, weighting=0, nested=0, Kc=8):
        self.weighting, self.nested, self.Kc = weighting, nested, Kc
        self.Pc, self.cadj, self.tris, self.NBc, self.sample = [], [], [], [], []
        self.P, self.nearest, self.expect, self.overflow = [], [], [], []

    def add(self, Pc, cadj, tris, NBc, points, sample=None):
        """Pc: cell positions; cadj / NBc: {local cell: list}; tris: local triples in stored order; points: (xyz, local cell, kind, cnt, local
        cols or None[, overflow]); sample: {local cell: index into points} for `nested`."""
        o, pf = len(self.Pc), len(self.P)
        sh = lambda v: v + o if v >= 0 else v
        for c, xyz in enumerate(Pc):
            self.Pc.append(xyz)
            self.cadj.append([sh(v) for v in cadj.get(c, [])])
            row = [sh(v) for v in NBc.get(c, [])]
            assert len(row) <= self.Kc
            self.NBc.append(row + [-1] * (self.Kc - len(row)))
            self.sample.append(pf + sample[c] if sample and c in sample else -1)
        self.tris += [tuple(sh(v) for v in t) for t in tris]
        for pt in points:
            xyz, c, kind, cnt, cols = pt[:5]
            self.P.append(xyz); self.nearest.append(sh(c))
            self.expect.append((kind, cnt, None if cols is None else [sh(v) for v in cols]))
            self.overflow.append(len(pt) > 5 and bool(pt[5]))
        return self

    def job(self):
        return Job(self.P, self.Pc, self.nearest, self.sample, self.cadj, self.tris, self.NBc, self.weighting, self.nested, self.expect, self.overflow)


# ------------------------------------------------------------------------------------------------------------- the catalogue
def launch_edges(nf):
    """nc = 1, deg = 0: every row is (c, 1.0), one parent, kind 3 -- at point counts around the 128-thread block."""
    rng = np.random.default_rng(nf)
    return Job(rng.uniform(-1, 1, (nf, 3)), [[0.5, 0.25, 0.0]], np.zeros(nf, np.int32), [-1], [[]], [], [[-1]], expect=[(SINGLE, 1, [0])] * nf)


def one_neighbour(weighting):
    """deg == 1: the two-parent row along the only edge.  Projection before / on / inside / beyond the edge (the clamps at 0 and 1 hit
    exactly), coincident cell positions (e = 0, the 1e-8 floors), the point on its own cell with an all-negative edge vector and under
    coincident cells with p - pc negative (both make w2 = -0.0 before the clamp), the point on the other cell (distance 0 under weighting 2)."""
    s = Scene(weighting)
    row = lambda xyz, c=0: (xyz, c, SINGLE, 2, [c, 1 - c])
    s.add([(0, 0, 0), (2, 0, 0)], {0: [1], 1: [0]}, [], {0: [0, 1], 1: [1, 0]},
          [row((-1, 1, 0)), row((0, 1, 0)), row((0.5, 1, 0)), row((2, 1, 0)), row((3, 0, 1)), row((2, 0, 0)), row((0, 0, 0)),
           row((1.5, -2, 0.25), 1), row((2, 0, 0), 1), row((0.3, 0.7, -0.1)), row((1.9, 0.1, 0.2), 1)])
    s.add([(1, 1, 1), (1, 1, 1)], {0: [1], 1: [0]}, [], {0: [0, 1], 1: [1, 0]}, [row((1, 1, 1)), row((2, 3, 0)), row((0, 0, 0)), row((0.5, 0.25, -3), 1)])
    s.add([(4, 4, 4), (3, 2, 1)], {0: [1], 1: [0]}, [], {0: [0, 1], 1: [1, 0]}, [row((4, 4, 4)), row((3, 2, 1)), row((3, 2, 1), 1), row((5, 5, 5)), row((3.5, 3, 2.5))])
    return s.job()


def closest_three(weighting=0):
    """deg >= 2 and no triangles: the cell and its two nearest table neighbours, (distance, index) ascending like std::sort of pairs.
    The point is the origin, the candidates sit at distances 1, 1, 1, 2, 2, 3 (local cells 0..5); every configuration is one more cell
    (at distance 1) with its own table row."""
    near = [(1, 0, 0), (0, 1, 0), (0, 0, -1), (2, 0, 0), (0, 2, 0), (0, 0, 3)]
    rows = [                                                    # table row behind the cell's own index -> the parents after the cell
        ([-1, 3, -1, 0, 5], [0, 3]),                            # -1 padding inside the row
        ([3, 0], [0, 3]),                                       # two usable neighbours
        ([5], [5]),                                             # one
        ([], []),                                               # none
        ([0, 1, 3], [0, 1]),                                    # two equidistant, the lower index first
        ([1, 0, 3], [0, 1]),                                    # ... and second
        ([2, 1, 0], [0, 1]),                                    # three equidistant
        ([0, 2, 1], [0, 1]),
        ([0, 4, 3], [0, 3]),                                    # a tie between the second and the third candidate
        ([0, 3, 4], [0, 3]),
        ([5, 3, 0], [0, 3]),                                    # the nearest arrives last
        ([3, 5, 4, 1], [1, 3]),
        ([0, 3, 1], [0, 1]),                                    # a late candidate ties with the first, higher index
        ([5, 4, 3, 2, 1, 0], [0, 1]),                           # everything in descending order
    ]
    s = Scene(weighting, Kc=8)
    Pc = near + [(0, 0, 1)] * len(rows)
    cadj, NBc, pts = {}, {}, []
    for q, (row, want) in enumerate(rows):
        c = 6 + q
        cadj[c] = [0, 1]                                        # deg = 2, empty triangle range
        NBc[c] = ([c] + row) if q % 2 == 0 else (row[:1] + [c] + row[1:])      # the cell's own index in the row, first or second
        pts.append(((0, 0, 0), c, CLOSEST, 1 + len(want), [c] + want))
        if len(want) == 2:
            pts.append(((0.3, -0.2, 0.1), c, CLOSEST, 3, None))  # and a point without ties
    s.add(Pc, cadj, [], NBc, pts)
    return s.job()


def containing_triangle(weighting, nested=0):
    """A fan of four triangles round cell 0 in the plane z = 0, the cell stored at position 0, 1 and 2 and one triangle stored clockwise
    (normal flipped): found in the first, a middle and the last triangle; on an edge, on a shared edge (the first triangle wins), on a
    vertex, on the cell; off the plane with the projection inside."""
    Pc = [(0, 0, 0), (4, 0, 0), (0, 4, 0), (-4, 0, 0), (0, -4, 0)]
    tris = [(0, 1, 2), (3, 0, 2), (3, 4, 0), (0, 1, 4)]
    t = lambda xyz, cols, kind=TRIANGLE: (xyz, 0, kind, 3 if kind == TRIANGLE else 1, cols)
    pts = [t((1, 1, 0), [0, 1, 2]), t((-1, 1, 0), [0, 2, 3]), t((-1, -1, 0), [0, 3, 4]), t((1, -1, 0), [0, 1, 4]),
           t((2, 2, 0), [0, 1, 2]), t((0, 2, 0), [0, 1, 2]), t((-2, 0, 0), [0, 2, 3]), t((4, 0, 0), [0, 1, 2]), t((0, -4, 0), [0, 3, 4]),
           t((0, 0, 0), [0, 1, 2]), t((1, 1, 3), [0, 1, 2]), t((1, -1, -2), [0, 1, 4]), t((-0.5, -2.5, 0.75), [0, 3, 4]),
           t((1.3, 0.7, 0.2), [0, 1, 2]), t((-2.1, 0.3, -0.4), [0, 2, 3])]
    sample = None
    if nested:                                                  # the first point is its cell's sample: one parent, weight 1; the others are not
        pts[0] = t((1, 1, 0), [0], NESTED)
        sample = {0: 0, 1: 1, 2: 5}                             # (cells 1 and 2 name points that belong to cell 0: no effect)
    s = Scene(weighting, nested)
    s.add(Pc, {0: [1, 2, 3, 4], 1: [0, 2, 4], 2: [0, 1, 3], 3: [0, 2, 4], 4: [0, 1, 3]}, tris, {0: [0, 1, 2, 3, 4]}, pts, sample)
    if nested:                                                  # the sample of a cell without neighbours and of one with a single neighbour
        s.add([(9, 9, 9)], {}, [], {0: [0]}, [((9, 9, 8), 0, NESTED, 1, [0]), ((9, 8, 9), 0, SINGLE, 1, [0])], {0: 0})
        s.add([(20, 0, 0), (22, 0, 0)], {0: [1], 1: [0]}, [], {0: [0, 1], 1: [1, 0]}, [((21, 1, 0), 0, SINGLE, 2, [0, 1]), ((21, 1, 0), 1, NESTED, 1, [1])], {1: 1, 0: 1})
    return s.job()


def edge_fallback(weighting):
    """The point lies outside every triangle of its cell.  (1) one key keeps a non-negative value: the edge row to it; (2) two such keys,
    inserted in descending order: the lower one wins; (3) a key made non-negative by an early triangle and -1 by a later one, and (4) the
    other way round (set_if_absent must not revive it): no key is left, closest three."""
    s = Scene(weighting)
    s.add([(0, 0, 0), (4, 0, 0), (0, 4, 0)], {0: [1, 2]}, [(0, 1, 2)], {0: [0, 1, 2]},
          [((2, -1, 0), 0, EDGE, 2, [0, 1]), ((-1, 2, 0.5), 0, EDGE, 2, [0, 2]), ((5, -1, 0), 0, EDGE, 2, [0, 1]), ((1.7, -0.3, 0.2), 0, EDGE, 2, [0, 1]),
           ((-1, -1, 0), 0, CLOSEST, 3, [0, 1, 2])])
    # cells 3, 4 are the keys of the first stored triangle, 1, 2 of the second: insertion order 3, 4, 1, 2
    s.add([(0, 0, 0), (4, 0, 0), (0, 4, 0), (0, -4, 0), (-4, 0, 0)], {0: [1, 2, 3, 4]}, [(0, 3, 4), (0, 1, 2)], {0: [0, 1, 2, 3, 4]},
          [((2, -1, 0), 0, EDGE, 2, [0, 1]), ((2.5, -0.5, 1), 0, EDGE, 2, [0, 1])])
    for tris in ([(0, 1, 2), (0, 1, 3)], [(0, 1, 3), (0, 1, 2)]):
        s.add([(0, 0, 0), (4, 0, 0), (0, 4, 0), (-4, -1, 0)], {0: [1, 2, 3]}, tris, {0: [0, 1, 2, 3]}, [((2, -1, 0), 0, CLOSEST, 3, [0, 1, 2])])
    return s.job()


def degenerate_triangle(weighting=0):
    """Three collinear cell positions: zero normal, area2 == 0, NaN barycentrics -- every comparison is false, both keys keep their
    first value and the row is the edge to the lower key.  With a proper triangle behind the degenerate one the point is found there."""
    s = Scene(weighting)
    s.add([(0, 0, 0), (2, 0, 0), (4, 0, 0)], {0: [1, 2]}, [(0, 1, 2)], {0: [0, 1, 2]},
          [((1, 1, 0), 0, EDGE, 2, [0, 1]), ((0, 0, 0), 0, EDGE, 2, [0, 1]), ((-3, 0.5, 2), 0, EDGE, 2, [0, 1])])
    s.add([(0, 0, 0), (2, 0, 0), (4, 0, 0), (0, 4, 0)], {0: [1, 2, 3]}, [(0, 1, 2), (0, 1, 3)], {0: [0, 1, 2, 3]},
          [((1, 1, 0), 0, TRIANGLE, 3, [0, 1, 3]), ((1, -1, 0), 0, EDGE, 2, [0, 1])])
    return s.job()


def edge_map_capacity(weighting=0):
    """A planar fan round cell 0 over m ring cells on the line y = 8 (m - 1 triangles, m distinct keys) and a point far below it, outside
    every triangle, so that all of them are visited; the first ring cell is a key of the first triangle only and keeps its non-negative
    value there (b0, b1 > 0 > b2), so the row is the edge to it, the lowest key.  32 keys: the table is full, a normal row.  33 and 40 keys: the device stage hands
    the point back (cnt 255) and the host routine makes the row.  The 40-key fan with the point inside its first triangle: found before
    the table fills."""
    s = Scene(weighting, Kc=8)
    for m in (32, 33, 40):
        Pc = [(0, 0, 0)] + [(2 * i - (m - 1), 8, 0) for i in range(m)]
        tris = [(0, 1 + i, 2 + i) for i in range(m - 1)]
        r0, r1 = np.array(Pc[1], float), np.array(Pc[2], float)
        inside = tuple((0.25 * r0 + 0.25 * r1).tolist())
        s.add(Pc, {0: list(range(1, m + 1))}, tris, {0: list(range(8))},
              [((0, -20, 0), 0, EDGE, 2, [0, 1], m > 32), ((1, -20, 2), 0, EDGE, 2, [0, 1], m > 32), (inside, 0, TRIANGLE, 3, [0, 1, 2])])
    return s.job()


def nested_samples(weighting):
    return containing_triangle(weighting, nested=1)


def coarse_grid_job(nf, weighting, g=40, seed=2024):
    """nf points scattered with off-plane jitter over (and a margin round) a g x g coarse grid, jittered itself, every square cut
    into two triangles; `nearest` is the true nearest coarse point.  Interior points find a triangle, points beyond the rim take the edge
    and the closest-three rows."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(g), np.arange(g), indexing="ij")
    Pc = np.stack([ii.ravel() + rng.uniform(-0.15, 0.15, g * g), jj.ravel() + rng.uniform(-0.15, 0.15, g * g), rng.uniform(-0.1, 0.1, g * g)], axis=1)
    idx = lambda i, j: i * g + j
    tris, cadj = [], [set() for _ in range(g * g)]
    for i in range(g - 1):
        for j in range(g - 1):
            for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))):
                tris.append(t)
                for a in t:
                    cadj[a].update(b for b in t if b != a)
    tris.sort()                                                 # ids follow the lowest cell, as in the builder
    cadj = [sorted(a) for a in cadj]
    NBc = -np.ones((g * g, 7), np.int32)
    for c, a in enumerate(cadj):
        NBc[c, 0] = c
        NBc[c, 1:1 + len(a)] = a
    P = np.stack([rng.uniform(-1.5, g + 0.5, nf), rng.uniform(-1.5, g + 0.5, nf), rng.uniform(-0.3, 0.3, nf)], axis=1)
    nearest = cKDTree(Pc).query(P, workers=-1)[1].astype(np.int32)
    return Job(P, Pc, nearest, np.full(g * g, -1, np.int32), cadj, tris, NBc, weighting)


# (name, builder, arguments): the branch catalogue, every case a few hundred points at most
CASES = [(f"launch-{nf}", launch_edges, (nf,)) for nf in (1, 127, 128, 129, 257)]
CASES += [(f"one-neighbour-w{w}", one_neighbour, (w,)) for w in (0, 1, 2)]
CASES += [("closest-three", closest_three, ())]
CASES += [(f"triangle-w{w}", containing_triangle, (w,)) for w in (0, 1, 2)]
CASES += [(f"edge-fallback-w{w}", edge_fallback, (w,)) for w in (0, 1, 2)]
CASES += [("degenerate-triangle", degenerate_triangle, ()), ("edge-map-capacity", edge_map_capacity, ())]
CASES += [(f"nested-w{w}", nested_samples, (w,)) for w in (0, 2)]
CASE_IDS = [c[0] for c in CASES]
