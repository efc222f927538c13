"""gmg_config::nullspace, the part that needs no device: the configuration mirror, the refusals gmg_create makes before it looks
for a device, the drop-in's option, the coarsest solver's "pin the last pivot" mode through its host-only hook (x = P G P b against
numpy.linalg.pinv), the row-sum rule with its two codes, the factor from a stand-alone program built with AddressSanitizer + UBSan, and the numpy
model (tests/nullspace_model.py: the existing model classes with a pseudo-inverse coarse solve plus the two projections).

Measured with the model on the torus' pure stiffness matrix (n = 1 073, n_L = 170; ChebyshevModel cycle, ratio 8, 2 + 2, x0 = rhs, stop type 2):
7 plain cycles to 1e-4; PCG to 1e-8 in 10 iterations without a guard, 1e-9 from the dense least-squares solution after centring."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import nullspace_model as nm
from tests import problems
from tests.chebyshev_model import ChebyshevModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "gravo_mg_amd", "dropin")


def test_config_mirror_has_nullspace_in_front_of_fold_head(cabi):
    """Directly in front of fold_head: the six names behind it are the ones earlier tests pin, and the size changes, so a binding built against
    the parent's header is refused."""
    names = [f[0] for f in cabi.GmgConfig._fields_]
    assert names[-7] == "nullspace" and cabi.GmgConfig._fields_[-7] == ("nullspace", C.c_int)
    assert names[-6] == "fold_head" and names[-5:] == ["reorder_pointwise", "zero_guess_step", "pcg", "device_coloring", "accelerate"]
    assert C.sizeof(cabi.GmgConfig) == cabi.lib().gmg_config_size()
    cfg = cabi.GmgConfig()
    cfg.nullspace = 7
    assert cabi.lib().gmg_config_default(C.byref(cfg)) == 0 and cfg.nullspace == 0 and cfg.fold_head == 1 and cfg.accelerate == 0


def test_create_refuses_without_a_device(cabi):
    """Values other than 0 / 1: GMG_ERR_INVALID with the field's name, before a device is looked for; 0 and 1 go through with every loop."""
    for bad in (-1, 2, 100):
        with pytest.raises(cabi.GmgError) as ei:
            cabi.Engine(nullspace=bad)
        assert ei.value.code == cabi.GMG_ERR_INVALID and "nullspace" in str(ei.value), str(ei.value)
    cheb = dict(smoother=cabi.SMOOTHER_CHEBYSHEV)
    for kw in (dict(nullspace=0), dict(nullspace=1), dict(nullspace=1, accelerate=3), dict(nullspace=1, pcg=1, **cheb), dict(nullspace=1, inner_precision=1),
               dict(nullspace=1, use_graph=True), dict(nullspace=1, coarse_mode=cabi.COARSE_HOST_LDLT), dict(nullspace=1, coarse_mode=cabi.COARSE_DEVICE_TRIANGLE)):
        try:
            cabi.Engine(**kw).close()
        except cabi.GmgError as e:
            assert cabi.device_count() == 0 and e.code == cabi.GMG_ERR_NO_DEVICE, (kw, str(e))
    # a refusal's message does not outlive the next gmg_create of the thread
    with pytest.raises(cabi.GmgError) as ei:
        cabi.Engine(accelerate=9)
    assert ei.value.code == cabi.GMG_ERR_INVALID and "nullspace" not in str(ei.value)


def test_dropin_accepts_the_option(cabi):
    import glob
    if not glob.glob(os.path.join(DROPIN, "gravomg_bindings*.so")):
        import __graft_entry__
        __graft_entry__.build()
    if DROPIN not in sys.path:
        sys.path.insert(0, DROPIN)
    import gravomg
    from gravo_mg_amd import meshgen
    V, F = meshgen.torus_mesh(24, 20)
    S, mass = meshgen.cotan_laplacian(V, F)
    solver = gravomg.MultigridSolver(V, gravomg.neighbors_from_stiffness(S), sp.diags(mass).tocsr(), lower_bound=40)
    solver.set_engine_option("nullspace", 1)
    with pytest.raises(Exception):
        solver.set_engine_option("nullspace_more", 1)
    assert "nullspace" in gravomg.MultigridSolver.set_engine_option.__doc__


# ---- the pinned factor ----------------------------------------------------------------------------------------------------------------

def _graph_laplacian(n, rows, cols, w=None):
    w = np.ones(len(rows)) if w is None else np.asarray(w, dtype=np.float64)
    W = sp.coo_matrix((w, (rows, cols)), shape=(n, n))
    W = (W + W.T).tocsr()
    return (sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W).tocsc()


def _ring(n):
    i = np.arange(n)
    return _graph_laplacian(n, i, (i + 1) % n, 1.0 + 0.25 * np.cos(i))


def _star(n, hub):
    leaves = np.array([i for i in range(n) if i != hub])
    return _graph_laplacian(n, np.full(n - 1, hub), leaves, 1.0 + (leaves % 7) / 7.0)


def _coarsest(P, A0):
    A = sp.csc_matrix(A0)
    for u in P.U:
        u = sp.csc_matrix(u)
        A = (u.T @ A @ u).tocsc()
    A = ((A + A.T) * 0.5).tocsc()
    A.sort_indices()
    return A


def _torus_coarsest(kind):
    P = problems.torus_problem(n1=37, n2=29, lower_bound=60)
    return _coarsest(P, P.S if kind == "poisson" else (P.S @ sp.diags(1.0 / P.mass) @ P.S).tocsc())


_FACTOR_CASES = {"1x1 zero": lambda: sp.csc_matrix(np.zeros((1, 1))),
                 "path of 2": lambda: _graph_laplacian(2, [0], [1]),
                 "ring of 65": lambda: _ring(65),
                 "star of 130, hub first": lambda: _star(130, 0),
                 "star of 130, hub last": lambda: _star(130, 129),
                 "star of 130, hub in the middle": lambda: _star(130, 64),
                 "torus coarsest operator": lambda: _torus_coarsest("poisson"),
                 "bilaplacian coarsest operator": lambda: _torus_coarsest("bilaplacian")}


@pytest.mark.parametrize("name", list(_FACTOR_CASES))
def test_pinned_factor_applies_the_pseudo_inverse(cabi, name):
    """x = P G P b on the columns of the identity against numpy.linalg.pinv, entry by entry: within 1e-10 of the largest entry of the
    pseudo-inverse (5e-15 measured on the Poisson operators, 8e-13 on the Bilaplacian's: two orders of margin for the threaded supernodal path)."""
    A = _FACTOR_CASES[name]()
    n = A.shape[0]
    if name.startswith("torus"):
        assert n == 170
    X, (rowsum, pivot) = cabi.host_pinv_solve(A, np.eye(n))
    ref = np.linalg.pinv(np.asarray(A.todense()), hermitian=True)
    scale = float(np.abs(ref).max())
    err = float(np.abs(X - ref).max())
    print(f"{name}: n = {n}, row sums {rowsum:.2e}, replaced pivot / largest {pivot:.2e}, max |P G P - pinv| = {err:.2e} of max |pinv| = {scale:.2e}")
    assert rowsum <= nm.ROWSUM_MAX
    if n == 1:
        assert X.shape == (1, 1) and X[0, 0] == 0.0
        return
    assert err <= 1e-10 * scale
    assert abs(pivot) <= 1e-9           # rounding noise beside the pivots of A11
    # the operator is the model's: the pinned inverse, double-centred (whichever unknown the ordering eliminated last)
    assert np.abs(nm.double_centre(nm.pinned_inverse(A)) - ref).max() <= 1e-10 * scale


def test_two_components_are_a_zero_pivot_before_the_last(cabi):
    """Two unit-weight paths: every pivot of a path eliminated from its leaves is exactly 1 and its last one exactly 0 -- one of the two zeros
    comes before the last pivot and keeps today's test."""
    A = sp.block_diag([_graph_laplacian(3, [0, 1], [1, 2]), _graph_laplacian(4, [0, 1, 2], [1, 2, 3])]).tocsc()
    assert cabi.host_nullspace_rowsum(A, coarsest=True)[0] == cabi.GMG_OK
    with pytest.raises(cabi.GmgError) as ei:
        cabi.host_pinv_solve(A, np.ones(7))
    assert ei.value.code == cabi.GMG_ERR_NUMERIC


def test_row_sum_rule_and_its_codes(cabi):
    """S passes on level 0 and on the coarsest level with figures of rounding size; a mass term of the size of the operator's entries fails as a
    level 0 (GMG_ERR_INVALID); a U with one row scaled by 1.01 no longer preserves constants and its coarsest operator fails (GMG_ERR_NUMERIC),
    through the factor's hook as well."""
    P = problems.torus_problem(n1=37, n2=29, lower_bound=60)
    rc, fig0 = cabi.host_nullspace_rowsum(P.S)
    rcc, figc = cabi.host_nullspace_rowsum(_coarsest(P, P.S), coarsest=True)
    print(f"row-sum figures: level 0 {fig0:.2e} (numpy {nm.rowsum_figure(P.S):.2e}), coarsest {figc:.2e}")
    assert rc == cabi.GMG_OK and rcc == cabi.GMG_OK and fig0 <= 1e-13 and figc <= 1e-13
    assert abs(fig0 - nm.rowsum_figure(P.S)) <= 1e-15
    rc, fig = cabi.host_nullspace_rowsum((P.S + 1e-3 * sp.diags(P.mass)).tocsc())          # (a row: 1e-3 x 1e-3 against entries of size 10)
    assert rc == cabi.GMG_ERR_INVALID and fig > nm.ROWSUM_MAX
    for u in P.U:
        assert np.abs(np.asarray(sp.csr_matrix(u).sum(axis=1)).ravel() - 1.0).max() <= 1e-14      # the built-in weighting preserves constants
    U = [sp.csr_matrix(u).copy() for u in P.U]
    row = U[0].shape[0] // 2
    U[0].data[U[0].indptr[row]:U[0].indptr[row + 1]] *= 1.01
    Q = problems.Problem(P.V, P.S, P.mass, [sp.csc_matrix(u) for u in U], P.S, P.rhs, "scaled")
    bad = _coarsest(Q, P.S)
    rc, fig = cabi.host_nullspace_rowsum(bad, coarsest=True)
    assert rc == cabi.GMG_ERR_NUMERIC and fig > nm.ROWSUM_MAX
    with pytest.raises(cabi.GmgError) as ei:
        cabi.host_pinv_solve(bad, np.ones(bad.shape[0]))
    assert ei.value.code == cabi.GMG_ERR_NUMERIC


def workaround_system(scale=10.0):
    """(S, mass, S + 1e-6 M) of the torus (37, 29) with its coordinates multiplied by `scale`.  The cotangent matrix S of a surface mesh does not
    depend on the unit of length, the lumped masses go with its square, so what a term tau M does to a row sum depends on the unit: the row-sum
    figure of S + tau M is max_i tau m_i / sum_j |a_ij| (the rows of S sum to zero), here tau m_i / (8 .. 16).  It passes the bound of 1e-9 exactly
    where tau m_i is more than about 1e-8: with tau = 1e-6 on meshes whose vertex areas exceed 1e-2.  The unit torus of the other tests has vertex
    areas of 5e-4 .. 1.5e-3 (figure 1.3e-10, below the bound: there the rule cannot tell the workaround from S); ten times the
    lengths give areas of 5e-2 .. 1.5e-1, an order of magnitude inside the range where it can."""
    from gravo_mg_amd import meshgen
    V, F = meshgen.torus_mesh(37, 29)
    S, mass = meshgen.cotan_laplacian(scale * V, F)
    lhs, _ = meshgen.poisson_system(S, mass)              # S + 1e-6 M, the reference's workaround (experiments/python/comparisons.py:76)
    return S, mass, lhs


def test_workaround_system_fails_the_rule(cabi):
    """The reference's workaround S + 1e-6 M handed to the rule as a level 0 is refused with GMG_ERR_INVALID at the bound of 1e-9 -- on a mesh in
    units in which a term of 1e-6 M is visible in double precision at that bound (workaround_system: vertex areas of 5e-2 .. 1.5e-1, figure
    tau m_i / sum_j |a_ij| = 1e-6 x 1e-1 / 10 = 1e-8); the same S alone passes with a figure of rounding size."""
    S, mass, lhs = workaround_system()
    assert 4e-2 <= mass.min() and mass.max() <= 2e-1
    rc0, fig0 = cabi.host_nullspace_rowsum(S)
    rc, fig = cabi.host_nullspace_rowsum(lhs)
    print(f"S + 1e-6 M: row-sum figure {fig:.3e} against the bound {nm.ROWSUM_MAX:.0e}, status {rc}; S alone {fig0:.3e}")
    assert rc0 == cabi.GMG_OK and fig0 <= 1e-13
    assert rc == cabi.GMG_ERR_INVALID and fig > nm.ROWSUM_MAX
    assert abs(fig - nm.rowsum_figure(lhs)) <= 1e-6 * fig


_FACTOR_MAIN = r"""
#include <cmath>
#include <cstdio>
#include <vector>
#include "host_ldlt.hpp"
using namespace gmg;
static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
int main() {
    {   // a ring of 65 nodes with varying weights: pinned factor, x = P G P b, then A x = P b
        const int n = 65;
        std::vector<double> w(n);
        for (int i = 0; i < n; ++i) w[i] = 1.0 + 0.25 * std::cos((double)i);          // edge i -- (i + 1) % n
        std::vector<int> ptr(n + 1), idx;
        std::vector<double> val;
        for (int j = 0; j < n; ++j) {
            const int a = (j + n - 1) % n, b = (j + 1) % n;
            int nb[3] = {a, j, b};
            double v[3] = {-w[a], w[a] + w[j], -w[j]};
            for (int s = 0; s < 3; ++s) for (int t = s + 1; t < 3; ++t) if (nb[t] < nb[s]) { std::swap(nb[s], nb[t]); std::swap(v[s], v[t]); }
            ptr[j] = (int)idx.size();
            for (int s = 0; s < 3; ++s) { idx.push_back(nb[s]); val.push_back(v[s]); }
        }
        ptr[n] = (int)idx.size();
        Compressed A;
        A.assign(n, n, ptr.data(), idx.data(), val.data());
        EXPECT(nullspace_rowsum(A) <= kNullspaceRowsumMax);
        SupernodalLDLT f;
        f.pin_last = true;
        EXPECT(f.factor(A));
        EXPECT(std::fabs(f.pinned_pivot) <= 1e-12);
        std::vector<double> b(n), x(n), work(n);
        for (int i = 0; i < n; ++i) b[i] = std::sin(1.0 + 0.7 * i) + 0.3;
        remove_means(b.data(), n, n, 1);
        f.solve_multi(b.data(), n, x.data(), n, 1, work.data());
        remove_means(x.data(), n, n, 1);
        double worst = 0.0, sum = 0.0;
        for (int i = 0; i < n; ++i) {
            const int a = (i + n - 1) % n, c = (i + 1) % n;
            const double r = (w[a] + w[i]) * x[i] - w[a] * x[a] - w[i] * x[c] - b[i];
            worst = std::fmax(worst, std::fabs(r));
            sum += x[i];
        }
        EXPECT(worst <= 1e-11 && std::fabs(sum) <= 1e-11);
        EXPECT(f.factor(A, true));                                                     // the numeric re-factorisation pins again
        SupernodalLDLT g;                                                              // without the mode the same matrix is refused or factored with a noise pivot
        (void)g.factor(A);
        EXPECT(!g.pin_last);
    }
    {   // the 1 x 1 matrix [0]: the only pivot is the last one, the answer is 0
        const int ptr[2] = {0, 1}, idx[1] = {0};
        const double val[1] = {0.0};
        Compressed A;
        A.assign(1, 1, ptr, idx, val);
        SupernodalLDLT f;
        f.pin_last = true;
        EXPECT(f.factor(A));
        double b = 3.0, x = 7.0, work = 0.0;
        remove_means(&b, 1, 1, 1);
        f.solve_multi(&b, 1, &x, 1, 1, &work);
        remove_means(&x, 1, 1, 1);
        EXPECT(x == 0.0 && f.pinned_pivot == 0.0);
        SupernodalLDLT g;
        EXPECT(!g.factor(A));                                                          // today's test: a zero pivot
    }
    std::printf(fails ? "%d checks failed\n" : "all checks passed\n", fails);
    return fails ? 1 : 0;
}
"""


def test_pinned_factor_under_address_and_ub_sanitizers(tmp_path):
    """The ring and the 1 x 1 case factored pinned and solved, from a stand-alone program that includes host_ldlt.hpp, under
    -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "pinned_factor_main.cpp"
    src.write_text(_FACTOR_MAIN)
    exe = tmp_path / "pinned_factor_main"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "gravo_mg_amd", "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout + run.stderr


# ---- the model ------------------------------------------------------------------------------------------------------------------------

def _poisson():
    P = problems.torus_problem(n1=37, n2=29, lower_bound=60)
    lhs = sp.csc_matrix(P.S)
    lhs.sort_indices()
    rhs = np.asarray(P.rhs, dtype=np.float64).reshape(P.n, -1) + 0.75          # a right-hand side with a constant added
    return P, lhs, rhs


def test_model_plain_loop_takes_the_cycles_of_the_regular_problem(oracle):
    """Poisson torus, pure S, Chebyshev 2 + 2, x0 = rhs, stop type 2: at most 8 cycles to 1e-4 (7 measured), the answer of zero M-weighted mean."""
    P, lhs, rhs = _poisson()
    M = nm.with_pinv_coarse(ChebyshevModel(None, P.U, P.mass, lhs, oracle, 8.0, pre=2, post=2))
    x, it, res, _ = nm.nullspace_solve(lhs, P.mass, M.vcycle, rhs, rhs, 2, 1e-4, 30)
    print(f"plain loop on S: {it} cycles, residue {res[-1]:.3e}, rhs defect {nm.rhs_defect(rhs):.3e}")
    assert it <= 8 and res[-1] <= 1e-4
    assert np.abs(P.mass @ x).max() <= 1e-12 * (P.mass @ np.abs(x)).max()
    r = nm.project_rhs(rhs) - lhs @ x
    assert np.sqrt((P.mass[:, None] * r * r).sum() / (P.mass[:, None] * nm.project_rhs(rhs) ** 2).sum()) <= 1e-4


def test_model_pcg_reaches_the_least_squares_solution(oracle):
    """PCG to 1e-8: at most 12 iterations (10 measured) without a guard; after centring within 1e-7 of the dense least-squares solution (1e-9
    measured), relative to its largest entry."""
    P, lhs, rhs = _poisson()
    M = nm.with_pinv_coarse(ChebyshevModel(None, P.U, P.mass, lhs, oracle, 8.0, pre=2, post=2))
    x, it, res, _ = nm.nullspace_solve(lhs, P.mass, M.vcycle, rhs, rhs, 2, 1e-8, 40, loop="pcg")
    ref = nm.least_squares_solution(lhs, nm.project_rhs(rhs), P.mass)
    dev = float(np.abs(x - ref).max() / np.abs(ref).max())
    print(f"PCG on S: {it} iterations, residue {res[-1]:.3e}, against least squares {dev:.3e}")
    assert it <= 12 and res[-1] <= 1e-8 and dev <= 1e-7
