"""GMG_SMOOTHER_CHEBYSHEV, the part that needs no device: the constant and the refusals gmg_create makes before it looks for a device, the
drop-in's option, the recurrence of gravo_mg_amd/csrc/cheby_coeffs.hpp (the code the launch code calls) run from a stand-alone program built
with AddressSanitizer + UBSan against the closed form of the Chebyshev polynomials, and the symmetry of the model cycle
(tests/chebyshev_model.py) with equal pre- and post-degrees."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import problems
from tests.chebyshev_model import ChebyshevModel, cheby_coefficients

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "gravo_mg_amd", "dropin")


def test_constant_and_range_check_without_a_device(cabi):
    """smoother outside 0 .. 2 is refused next to the other range checks: the same code on a box without a GPU."""
    assert (cabi.SMOOTHER_MULTICOLOR_GS, cabi.SMOOTHER_JACOBI, cabi.SMOOTHER_CHEBYSHEV) == (0, 1, 2)
    for s in (-1, 3, 100):
        with pytest.raises(cabi.GmgError) as ei:
            cabi.Engine(smoother=s)
        assert ei.value.code == cabi.GMG_ERR_INVALID
    for s in (0, 1, 2):
        try:
            cabi.Engine(smoother=s).close()
        except cabi.GmgError as e:
            assert cabi.device_count() == 0 and e.code == cabi.GMG_ERR_NO_DEVICE


def test_dropin_accepts_the_option(cabi):
    import glob
    if not glob.glob(os.path.join(DROPIN, "gravomg_bindings*.so")):
        import __graft_entry__
        __graft_entry__.build()
    if DROPIN not in sys.path:
        sys.path.insert(0, DROPIN)
    import gravomg
    import scipy.sparse as sp
    from gravo_mg_amd import meshgen
    V, F = meshgen.torus_mesh(24, 20)
    S, mass = meshgen.cotan_laplacian(V, F)
    solver = gravomg.MultigridSolver(V, gravomg.neighbors_from_stiffness(S), sp.diags(mass).tocsr(), lower_bound=40)
    solver.set_engine_option("smoother", 2)
    doc = gravomg.MultigridSolver.set_engine_option.__doc__
    assert "smoother" in doc and "Chebyshev" in doc


LAMBDAS, RATIOS, STEPS = (1.0, 1.5, 2.0, 7.3), (2.0, 4.0, 30.0), 5      # lambda: 1e-3 .. 0.9 Lambda (6 points), Lambda / ratio, theta, Lambda

_COEFFS_MAIN = r"""
#include <cstdio>
#include <initializer_list>
#include "cheby_coeffs.hpp"
using namespace gmg;
// the scalar problem a = lambda (D = 1), b = 0, x_0 = 1: prints "Lambda ratio lambda x_1 .. x_5" per line, then the coefficients of steps 0 .. 4
int main() {
    for (double L : {1.0, 1.5, 2.0, 7.3})
        for (double ratio : {2.0, 4.0, 30.0}) {
            const ChebyInterval iv = cheby_interval(L, ratio);
            const double pts[9] = {1e-3 * L, 0.07 * L, 0.2 * L, 0.4 * L, 0.6 * L, 0.9 * L, L / ratio, iv.theta, L};
            for (double lam : pts) {
                double x = 1.0, p = 0.0;
                std::printf("X %.17g %.17g %.17g", L, ratio, lam);
                for (int k = 0; k < 5; ++k) {
                    const ChebyStep st = cheby_step_coeffs(L, ratio, k);
                    const double z = 0.0 - lam * x;
                    p = k == 0 ? st.c2 * z : st.c1 * p + st.c2 * z;
                    x += p;
                    std::printf(" %.17g", x);
                }
                std::printf("\n");
            }
            std::printf("C %.17g %.17g", L, ratio);
            for (int k = 0; k < 5; ++k) { const ChebyStep st = cheby_step_coeffs(L, ratio, k); std::printf(" %.17g %.17g", st.c1, st.c2); }
            std::printf("\n");
        }
    if (!(cheby_ratio_usable(kChebyRatio) && !cheby_ratio_usable(1.0) && !cheby_ratio_usable(0.0) && !cheby_ratio_usable(-3.0))) { std::printf("FAILED ratio checks\n"); return 1; }
    std::printf("done\n");
    return 0;
}
"""


def _cheb_T(k, t):
    """T_k(t) from the cosine form on [-1, 1] and the cosh form outside."""
    if abs(t) <= 1.0:
        return np.cos(k * np.arccos(t))
    return (1.0 if t > 0 or k % 2 == 0 else -1.0) * np.cosh(k * np.arccosh(abs(t)))


def test_recurrence_is_the_chebyshev_polynomial_under_address_and_ub_sanitizers(tmp_path):
    """x_k of the header's recurrence on the scalar problem equals T_k((theta - lambda) / delta) / T_k(sigma) within 1e-12 absolute (at most 5
    steps of a handful of roundings on quantities of modulus <= 1), and |x_k| < 1 on all of (0, Lambda]: the convergence guarantee itself.
    The coefficients equal the model's (tests/chebyshev_model.py) to a few roundings."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "cheby_coeffs_main.cpp"
    src.write_text(_COEFFS_MAIN)
    exe = tmp_path / "cheby_coeffs_main"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gravo_mg_amd", "csrc"),
                            str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("done"), run.stdout + run.stderr
    seen, coeffs = {}, {}
    for line in run.stdout.splitlines():
        f = line.split()
        if f[0] == "X":
            v = [float(t) for t in f[1:]]
            seen.setdefault((v[0], v[1]), []).append((v[2], v[3:]))
        elif f[0] == "C":
            v = [float(t) for t in f[1:]]
            coeffs[(v[0], v[1])] = list(zip(v[2::2], v[3::2]))
    assert sorted(seen) == sorted((L, r) for L in LAMBDAS for r in RATIOS)
    worst = 0.0
    for (L, ratio), rows in seen.items():
        lmin = L / ratio
        theta, delta = 0.5 * (L + lmin), 0.5 * (L - lmin)
        sigma = theta / delta
        lams = [lam for lam, _ in rows]
        assert len(rows) == 9 and len(set(lams)) == 9 and all(0.0 < lam <= L for lam in lams)
        for special in (lmin, theta, L):
            assert any(abs(lam - special) <= 1e-15 * L for lam in lams), (L, ratio, special)
        for lam, xs in rows:
            assert len(xs) == STEPS
            for k, x in enumerate(xs, start=1):
                want = _cheb_T(k, (theta - lam) / delta) / _cheb_T(k, sigma)
                worst = max(worst, abs(x - want))
                assert abs(x - want) <= 1e-12, (L, ratio, lam, k, x, want)
                assert abs(x) < 1.0, (L, ratio, lam, k, x)
        for (c1, c2), (m1, m2) in zip(coeffs[(L, ratio)], cheby_coefficients(L, ratio, STEPS)):
            assert abs(c1 - m1) <= 1e-15 * max(abs(m1), 1.0) and abs(c2 - m2) <= 4e-16 * abs(m2) + 1e-300, (L, ratio, c1, m1, c2, m2)
    print("largest |x_k - T_k / T_k(sigma)|: %.3e" % worst)


def _problems():
    return {"torus": problems.torus_problem(),
            "chain193-L3": problems.synthetic_problem(graph=("chain", 193), sizes=[193, 96, 24, 6], kind="smoothing", prolong=("smooth", "pc", "pc"))}


def _gaps(oracle, name, pre, post):
    """[(|<u, B v> - <B u, v>|, ||u|| ||B v||)] for 4 random pairs; B: b -> one model cycle from the zero guess.

    The pairs are standard normal vectors with their mean taken off, on both problems.  Why: torus_problem() is the Poisson system S + 1e-6 M of a
    closed surface, whose right-hand sides are compatible (mean-free) ones; the constant vector is within 1e-6 of the kernel, every cycle acts on it
    as A^-1 whatever its smoothers are, and amplifies it 1e6 times.  A vector with a mean therefore has ||B v|| made of that one direction (6.9e10 ..
    1.2e11 for standard normal vectors of length 1 920), and a bound relative to ||u|| ||B v|| then says nothing about B on the other 1 919: with plain
    standard normal pairs the cycle with pre = 2, post = 1 -- which is not symmetric -- stayed at 5.9e-12 .. 2.8e-11 of that scale (gaps 0.57 .. 2.7),
    inside the 1e-10 bound the symmetric cycle is held to.  Mean-free pairs leave the bounds of both tests as they are and make the first one
    stricter in absolute terms (a smaller scale).  On the chain problem (M + S, no near-kernel) the projection changes nothing of substance."""
    P = _problems()[name]
    rng = np.random.default_rng(17)
    M = ChebyshevModel(None, P.U, P.mass, P.lhs, oracle, 4.0, pre=pre, post=post)
    out = []
    for _ in range(4):
        u, v = rng.standard_normal(P.n), rng.standard_normal(P.n)
        u -= u.mean(); v -= v.mean()
        Bu, Bv = M.vcycle(u, np.zeros_like(u)), M.vcycle(v, np.zeros_like(v))
        out.append((abs(u @ Bv - Bu @ v), np.linalg.norm(u) * np.linalg.norm(Bv)))
        print("%s pre=%d post=%d: gap %.3e, ||u|| ||B v|| %.3e, ratio %.3e" % (name, pre, post, out[-1][0], out[-1][1], out[-1][0] / out[-1][1]))
    return out


@pytest.mark.parametrize("name", ["torus", "chain193-L3"])
def test_model_cycle_with_equal_degrees_is_a_symmetric_operator(oracle, name):
    """pre = post = 2: |<u, B v> - <B u, v>| <= 1e-10 ||u|| ||B v|| for 4 random pairs (_gaps).  (The ratio is the model's argument: any value
    gives a symmetric cycle.)"""
    for gap, scale in _gaps(oracle, name, 2, 2):
        assert gap <= 1e-10 * scale, (gap, scale)


@pytest.mark.parametrize("name", ["torus", "chain193-L3"])
def test_unequal_degrees_violate_the_symmetry_bound(oracle, name):
    """The check above can fail: the same model with pre = 2, post = 1 violates its bound by at least 1e3 x, i.e. gap >= 1e-7 ||u|| ||B v||, for
    every one of the same pairs."""
    for gap, scale in _gaps(oracle, name, 2, 1):
        assert gap >= 1e3 * 1e-10 * scale, (gap, scale)
