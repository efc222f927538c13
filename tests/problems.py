"""Seeded synthetic problems shared by the tests (built with the product's host-side generator and
hierarchy builder; the oracle consumes the same U_k so both sides see identical inputs)."""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

from gravo_mg_amd import cabi, meshgen


class Problem:
    def __init__(self, V, S, mass, U, lhs, rhs, name):
        self.V, self.S, self.mass, self.U, self.lhs, self.rhs, self.name = V, S, mass, U, lhs, rhs, name

    @property
    def n(self):
        return self.lhs.shape[0]


@functools.lru_cache(maxsize=None)
def torus_problem(n1=48, n2=40, kind="poisson", lower_bound=60, order="natural", d=1, seed=42):
    V, F = meshgen.torus_mesh(n1, n2, order=order)
    S, mass = meshgen.cotan_laplacian(V, F)
    neigh = meshgen.neighbors_from_stiffness(S)
    H = cabi.Hierarchy(V, neigh, lower_bound=lower_bound)
    if kind == "poisson":
        lhs, rhs = meshgen.poisson_system(S, mass, seed=seed, d=d)
    elif kind == "smoothing":
        lhs, rhs = meshgen.smoothing_system(S, mass, V)
    elif kind == "bilaplacian":
        lhs, rhs = meshgen.poisson_system(meshgen.bilaplacian(S, mass), mass, tau=1.0, seed=seed, d=d)
    else:
        raise ValueError(kind)
    return Problem(V, S, mass, H.U, lhs, rhs, f"torus{n1}x{n2}-{kind}-{order}")


@functools.lru_cache(maxsize=None)
def pointcloud_problem(n=3000, k=8, lower_bound=80):
    P = meshgen.torus_points(n, noise=0.002)
    S, mass = meshgen.knn_graph_laplacian(P, k)
    neigh = meshgen.neighbors_from_stiffness(S)
    H = cabi.Hierarchy(P, neigh, lower_bound=lower_bound)
    lhs, rhs = meshgen.poisson_system(S, mass)
    return Problem(P, S, mass, H.U, lhs, rhs, f"pointcloud{n}")


@functools.lru_cache(maxsize=None)
def sphere_problem(n=6000, lower_bound=80, order="spatial"):
    """Irregular-valence mesh (random points on a sphere, convex-hull triangulation): 6-8 colours, ragged rows."""
    V, F = meshgen.sphere_mesh(n, order=order)
    S, mass = meshgen.cotan_laplacian(V, F)
    neigh = meshgen.neighbors_from_stiffness(S)
    H = cabi.Hierarchy(V, neigh, lower_bound=lower_bound)
    lhs, rhs = meshgen.poisson_system(S, mass)
    return Problem(V, S, mass, H.U, lhs, rhs, f"sphere{n}-{order}")


def _laplacian_of(W, extra=None):
    """Graph Laplacian S = diag(W 1) - W of a symmetric non-negative weight matrix (CSC, sorted); extra: a second weight matrix (further edges)
    added to W first."""
    W = sp.csc_matrix(W) if extra is None else sp.csc_matrix(W + extra)
    S = (sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W).tocsc()
    S.sort_indices()
    return S


def _weights(rows, cols, n, rng, distinct=False):
    """Symmetric weight matrix with seeded weights in [0.5, 1.5) on the undirected edges (rows[i], cols[i]).  distinct: loops are dropped and an
    edge given twice (in either direction) is kept once -- for edge lists that were drawn at random."""
    if distinct:
        rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
        keep = rows != cols
        key = np.unique(np.minimum(rows, cols)[keep] * n + np.maximum(rows, cols)[keep])
        rows, cols = key // n, key % n
    w = 0.5 + rng.random(len(rows))
    W = sp.coo_matrix((w, (rows, cols)), shape=(n, n)).tocsc()
    return W + W.T


def _grid_edges(n1, n2, offset=0):
    idx = np.arange(n1 * n2).reshape(n1, n2) + offset
    return (np.concatenate([idx[:-1, :].ravel(), idx[:, :-1].ravel()]), np.concatenate([idx[1:, :].ravel(), idx[:, 1:].ravel()]))


def aggregation(n_f, n_c):
    """Piecewise-constant prolongation: fine i -> coarse floor(i n_c / n_f), consecutive fine indices in exactly n_c non-empty groups."""
    assert 1 <= n_c <= n_f
    return sp.csc_matrix((np.ones(n_f), (np.arange(n_f), np.arange(n_f) * n_c // n_f)), shape=(n_f, n_c))


def smoothed_aggregation(n_f, n_c):
    """Rows of up to 3 entries: 1/2 on the fine row's own group, 1/4 on each neighbouring group (renormalised at the ends).  Every coarse
    column keeps the fine rows of its own group."""
    j = np.arange(n_f) * n_c // n_f
    rows, cols, vals = [np.arange(n_f)], [j], [np.full(n_f, 0.5)]
    for s in (-1, 1):
        ok = (j + s >= 0) & (j + s < n_c)
        rows.append(np.arange(n_f)[ok]); cols.append(j[ok] + s); vals.append(np.full(ok.sum(), 0.25))
    U = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n_f, n_c))
    U = sp.diags(1.0 / np.asarray(U.sum(axis=1)).ravel()) @ U
    return sp.csc_matrix(U)


def synthetic_problem(graph, sizes, kind="poisson", prolong=("pc",), d=8, seed=5):
    """A problem of exact level sizes: an operator from a made-up graph and hand-made prolongations instead of the hierarchy builder.

    graph: ("chain", n) | ("grid", n1, n2) | ("diagonal", n) | ("isolated", n1, n2) -- a grid with every 20th vertex cut loose (only its
    diagonal) | ("clique", n1, n2, m) -- a grid behind m vertices that form a clique, vertex i < m tied to grid vertex m + i | ("hub", n1, n2) --
    a grid whose last vertex is tied to the first vertex of every level-1 group (a dense row on level 1) | ("links", n, ring, a, b) -- a chain
    (ring: closed, n - 1 tied to 0) plus the long links a[i] <-> b[i] given as index arrays (loops and repeats are dropped); the chain keeps the
    weights of ("chain", n).
    sizes: [n_0, n_1, ..., n_L]; prolong: "pc" (aggregation) or "smooth" (3-entry rows) per level, the last one repeated.
    kind: "poisson" lhs = S + 1e-2 M, "smoothing" lhs = M + S; M a positive lumped mass.  rhs = M y with d seeded columns."""
    rng = np.random.default_rng(seed)
    name = graph[0]
    if name in ("chain", "diagonal"):
        n = graph[1]
        e = (np.arange(n - 1), np.arange(1, n)) if name == "chain" else (np.zeros(0, int), np.zeros(0, int))
    elif name in ("grid", "isolated", "hub"):
        n1, n2 = graph[1], graph[2]
        n = n1 * n2 + (name == "hub")
        e = _grid_edges(n1, n2)
        if name == "isolated":
            cut = np.arange(7, n, 20)
            keep = ~(np.isin(e[0], cut) | np.isin(e[1], cut))
            e = (e[0][keep], e[1][keep])
        if name == "hub":
            first = np.searchsorted(np.arange(n) * sizes[1] // n, np.arange(sizes[1]))
            first = first[first != n - 1]
            e = (np.concatenate([e[0], first]), np.concatenate([e[1], np.full(len(first), n - 1)]))
    elif name == "clique":
        n1, n2, m = graph[1], graph[2], graph[3]
        n = m + n1 * n2
        g = _grid_edges(n1, n2, offset=m)
        a, b = np.triu_indices(m, 1)
        e = (np.concatenate([g[0], a, np.arange(m)]), np.concatenate([g[1], b, m + np.arange(m)]))
    elif name == "links":
        n, ring = graph[1], graph[2]
        e = (np.arange(n - 1), np.arange(1, n))
        la, lb = np.asarray(graph[3], np.int64), np.asarray(graph[4], np.int64)
        assert la.shape == lb.shape and la.min(initial=0) >= 0 and lb.min(initial=0) >= 0 and la.max(initial=0) < n and lb.max(initial=0) < n
        if ring:
            la, lb = np.append(la, n - 1), np.append(lb, 0)
        far = np.abs(la - lb) != 1                                 # (a link along the chain is the chain's edge)
        extra = (la[far], lb[far])
    else:
        raise ValueError(graph)
    assert sizes[0] == n, (sizes, n)
    if name == "links":
        W = _weights(e[0], e[1], n, rng)
        S = _laplacian_of(W, extra=_weights(extra[0], extra[1], n, rng, distinct=True))
    else:
        S = _laplacian_of(_weights(e[0], e[1], n, rng)) if len(e[0]) else sp.csc_matrix((n, n))
    mass = 0.5 + rng.random(n)
    if kind == "poisson":
        lhs = (S + 1e-2 * sp.diags(mass)).tocsc()
    elif kind == "smoothing":
        lhs = (sp.diags(mass) + S).tocsc()
    else:
        raise ValueError(kind)
    lhs.sort_indices()
    rhs = mass[:, None] * rng.standard_normal((n, d))
    U = []
    for k in range(len(sizes) - 1):
        how = prolong[min(k, len(prolong) - 1)]
        U.append(aggregation(sizes[k], sizes[k + 1]) if how == "pc" else smoothed_aggregation(sizes[k], sizes[k + 1]))
    label = graph if name != "links" else (name, graph[1], "ring" if graph[2] else "chain", len(graph[3]))
    return Problem(None, S, mass, U, lhs, rhs, f"{'-'.join(map(str, label))}-{kind}-{'x'.join(map(str, sizes))}")


def permuted_system(A, new2old):
    """P A P^T restricted to the real rows of a device ordering (padding rows dropped)."""
    order = new2old[new2old >= 0]
    return A.tocsr()[order][:, order].tocsc(), order
