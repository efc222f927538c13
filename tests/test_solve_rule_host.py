"""The solve loop's stopping rule (gravo_mg_amd/csrc/solve_rule.hpp: the residue from the check's sums, least / blown / goes on, the verdict), the
code gmgk::reduce_partials and the host loop both call, run from a stand-alone program built with AddressSanitizer + UBSan.  The program reads
cases (hex floats) and prints what the header gives; the expectations are here: residues recomputed with correctly rounded IEEE sqrt and
division and compared bit for bit, rule cases as (stops at, blown, diverged) written out by hand."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gravo_mg_amd", "csrc")

_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "solve_rule.hpp"
using namespace gmg;
// N type d s[2d]                 -> N <residue %a>
// R tol max_iter n r[n]          -> R <stops at> <blown> <diverged> <host goes-on words> <device goes-on words> <peek commits nothing>
// D tol first residue cycles blown -> D <diverged>
// C tol floor n r[n] confirmed   -> C <least %a> <blown> <diverged>
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char kind[8], tok[64];
    auto num = [&]() { if (std::fscanf(f, "%63s", tok) != 1) std::exit(3); return std::strtod(tok, nullptr); };
    while (std::fscanf(f, "%7s", kind) == 1) {
        if (kind[0] == 'N') {
            const int type = (int)num(), d = (int)num();
            std::vector<double> s((size_t)2 * d);                    // (exactly 2 d: a read past the sums is the sanitizer's to find)
            for (double& v : s) v = num();
            std::printf("N %a\n", norm_from_sums(s.data(), d, type));
        } else if (kind[0] == 'R') {
            const double tol = num();
            const int max_iter = (int)num(), n = (int)num();
            std::vector<double> r((size_t)n);
            for (double& v : r) v = num();
            // the host loop's use: the state in a SolveRule, advanced once per cycle
            SolveRule rule = rule_begin(tol, max_iter);
            // the device's use (gmgk::reduce_partials): `least` carried by the caller (d_watch), cycles_done passed in
            double least = 0.0;
            std::vector<char> host, dev;
            int peek_ok = 1;
            bool go;
            do {
                if (rule.cycles >= n) { std::printf("R sequence too short\n"); return 4; }
                const double res = r[(size_t)rule.cycles];
                const SolveRule before = rule;
                const bool would = rule_goes_on(rule_after(rule, res));              // the accelerated step's question
                if (rule.cycles != before.cycles || rule.blown != before.blown) peek_ok = 0;
                rule = rule_after(rule, res);
                go = rule_goes_on(rule);
                if (would != go) peek_ok = 0;
                least = rule_least(least, res, rule.cycles);
                dev.push_back(rule_wants_more(res, tol, rule_blown(res, least, rule.cycles)) ? '1' : '0');
                host.push_back(go ? '1' : '0');
            } while (go);
            host.push_back(0); dev.push_back(0);
            std::printf("R %d %d %d %s %s %d\n", rule.cycles, (int)rule.blown, (int)rule_diverged(rule), host.data(), dev.data(), peek_ok);
        } else if (kind[0] == 'D') {
            SolveRule rule = rule_begin(num(), 100);
            rule.first = rule.least = num();
            rule.residue = num();
            rule.cycles = (int)num();
            rule.blown = num() != 0.0;
            std::printf("D %d\n", (int)rule_diverged(rule));
        } else if (kind[0] == 'C') {
            // the accelerated loop: recurrence residues cycle by cycle, the last one replaced by `confirmed` (rule_confirmed, then rule_after)
            const double tol = num(), floor = num();
            const int n = (int)num();
            SolveRule rule = rule_begin(tol, n);
            double rec = 0.0;
            for (int i = 0; i < n; ++i) { rec = num(); if (i + 1 < n) rule = rule_after(rule, rec); }
            const double confirmed = num();
            rule = rule_after(rule_confirmed(rule, rec, confirmed, floor), confirmed);
            std::printf("C %a %d %d\n", rule.least, (int)rule.blown, (int)rule_diverged(rule));
        } else return 5;
    }
    std::fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def rule_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("solve_rule")
    src = tmp / "solve_rule_main.cpp"
    src.write_text(_MAIN)
    exe = tmp / "solve_rule_main"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return tmp, exe


def _run(rule_exe, lines):
    tmp, exe = rule_exe
    cases = tmp / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    run = subprocess.run([str(exe), str(cases)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout.split("\n")[:-1]
    assert len(out) == len(lines), run.stdout
    return out


def _hex(v):
    v = float(v)
    return "nan" if v != v else ("inf" if v == np.inf else ("-inf" if v == -np.inf else v.hex()))


def _bits(v):
    return "nan" if v != v else struct.pack("<d", v)


def _reference(s, d, type_):
    """today's expressions in correctly rounded IEEE double arithmetic (numpy scalars: a division by zero gives inf / NaN, no exception)"""
    s = [np.float64(v) for v in s]
    with np.errstate(all="ignore"):
        if type_ == 3:
            t = np.float64(0.0)
            for c in range(d):
                t = t + s[2 * c]
            return float(np.sqrt(t))
        out = np.float64(0.0)
        for c in range(d):
            v = np.sqrt(s[2 * c]) / np.sqrt(s[2 * c + 1]) if type_ == 0 else np.sqrt(s[2 * c] / s[2 * c + 1])
            if c == 0 or v > out:
                out = v
        return float(out)


def _largest_d():
    text = open(os.path.join(CSRC, "kernels.hip.hpp")).read()
    return int(re.search(r"constexpr int kReduceMaxComp = (\d+);", text).group(1)) // 2


def test_residue_from_the_sums_bit_for_bit(rule_exe):
    rng = np.random.RandomState(7)
    cases = []                                                           # (type, d, sums, pinned value or None)
    dims = sorted({1, 2, 3, 4, _largest_d()})
    assert dims[-1] == 4                                                 # (one group of columns: what launch_reduce hands the kernel)
    for type_ in range(4):
        for d in dims:
            for worst in sorted({0, d // 2, d - 1}):                     # the worst column first, in the middle, last
                s = rng.uniform(0.5, 2.0, 2 * d) * 10.0 ** rng.randint(-6, 6, 2 * d)
                s[2 * worst] = 1e9 * rng.uniform(1.0, 2.0)
                s[2 * worst + 1] = rng.uniform(1e-7, 2e-7)
                if type_ != 3:
                    ratios = [s[2 * c] / s[2 * c + 1] for c in range(d)]
                    assert int(np.argmax(ratios)) == worst
                cases.append((type_, d, s, None))
    inf, nan = float("inf"), float("nan")
    for type_ in range(3):
        cases.append((type_, 2, [1.0, 4.0, 4.0, 0.0], inf))              # a zero denominator: inf ...
        cases.append((type_, 2, [4.0, 0.0, 1.0, 4.0], inf))
        cases.append((type_, 1, [0.0, 0.0], nan))                        # ... or NaN (0 / 0)
        cases.append((type_, 2, [0.0, 0.0, 9.0, 1.0], nan))              # NaN in column 0 stays: no later v > NaN
        cases.append((type_, 3, [4.0, 1.0, nan, 1.0, 1.0, 1.0], 2.0))    # a NaN numerator behind column 0: v > out is false, the earlier value stays
        cases.append((type_, 3, [4.0, 1.0, 1.0, 1.0, nan, 1.0], 2.0))
        cases.append((type_, 2, [nan, 1.0, 4.0, 1.0], nan))
    cases.append((3, 2, [9.0, 0.0, 16.0, 0.0], 5.0))                     # type 3 never looks at the denominators
    cases.append((3, 3, [9.0, nan, 16.0, inf, 0.0, 0.0], 5.0))
    cases.append((3, 3, [1.0, 1.0, nan, 1.0, 1.0, 1.0], nan))
    out = _run(rule_exe, ["N %d %d %s" % (t, d, " ".join(_hex(v) for v in s)) for t, d, s, _ in cases])
    for (type_, d, s, pinned), line in zip(cases, out):
        kind, text = line.split()
        got = float.fromhex(text) if "0x" in text else float(text.replace("-nan", "nan"))
        assert kind == "N" and _bits(got) == _bits(_reference(s, d, type_)), (type_, d, list(s), text)
        if pinned is not None:
            assert _bits(got) == _bits(pinned), (type_, d, list(s), text)


_NAN, _INF = float("nan"), float("inf")
# (tol, max_iter, residues cycle by cycle) -> (stops at, blown, diverged)
_RULE_CASES = [
    ((1e-3, 10, [1.0, 0.1, 0.01, 1e-3, 1e-4]), (4, 0, 0)),               # contracting to the tolerance (residue <= tol ends it)
    ((1e-9, 3, [1.0, 0.5, 0.25, 0.125]), (3, 0, 0)),                     # contracting but out of max_iter
    ((1e-6, 10, [_NAN, 1.0]), (1, 1, 1)),                                # not finite at cycle 1
    ((1e-6, 10, [_INF, 1.0]), (1, 1, 1)),
    ((1e-6, 10, [1.0, _INF, 1.0]), (2, 1, 1)),
    ((1e-6, 10, [1.0, 1e5, 0.5, 1e-7]), (4, 0, 0)),                      # beyond 1e4 x least at cycle 2: the loop goes on
    ((1e-6, 10, [1.0, 0.5, 1e5, 1e-7]), (3, 1, 1)),                      # the same growth at cycle 3 stops it
    ((1e-6, 10, [2.0, 0.5, 5000.0, 1e-7]), (4, 0, 0)),                   # exactly 1e4 x least: the comparison is strict
    ((1e-6, 10, [2.0, 0.5, 5000.000000000001, 1e-7]), (3, 1, 1)),
    ((1e-6, 10, [2.0, 0.5, 1.0, 0.25, 2500.0000000000005, 1e-7]), (5, 1, 1)),      # the smallest SEEN, not the last
    ((1e-6, 3, [1.0, 2.0, 3.0]), (3, 0, 1)),                             # ends above tol, above the first residue, not blown
    ((1e-6, 3, [1.0, 0.5, 1.0]), (3, 0, 0)),                             # residue == first
    ((1e-6, 1, [5.0, 6.0]), (1, 0, 0)),                                  # a single allowed cycle above tol
    ((1.0, 10, [5.0, 0.5]), (2, 0, 0)),                                  # residue <= tol
    ((1.0, 10, [1.0, 5.0]), (1, 0, 0)),                                  # residue == tol
    ((_NAN, 10, [1.0, 0.5]), (1, 0, 0)),                                 # tol NaN: residue > tol is false at once, and one cycle cannot have diverged
    ((1e-9, 0, [1.0, 0.5]), (1, 0, 0)),                                  # max_iter 0 and negative: one cycle
    ((1e-9, -5, [1.0, 0.5]), (1, 0, 0)),
    ((1e-9, -5, [_NAN, 0.5]), (1, 1, 1)),
]


def test_rule_cases_and_host_and_device_in_step(rule_exe):
    lines = ["R %s %d %d %s" % (_hex(tol), max_iter, len(seq), " ".join(_hex(v) for v in seq)) for (tol, max_iter, seq), _ in _RULE_CASES]
    # residue <= tol is never diverged, whatever the first residue was and whether or not the loop had given up: (tol, first, residue, cycles, blown)
    direct = [((1.0, 0.1, 0.5, 3, 1), 0), ((1.0, 0.1, 1.0, 3, 0), 0), ((1.0, 0.1, 1.5, 3, 0), 1), ((1.0, 2.0, 1.5, 3, 0), 0), ((1.0, 2.0, 1.5, 3, 1), 1),
              ((1.0, 0.1, 1.5, 1, 0), 0)]
    lines += ["D %s %s %s %d %d" % (_hex(tol), _hex(first), _hex(res), cycles, blown) for (tol, first, res, cycles, blown), _ in direct]
    out = _run(rule_exe, lines)
    for ((tol, max_iter, seq), expected), line in zip(_RULE_CASES, out):
        kind, stops, blown, diverged, host, dev, peek_ok = line.split()
        assert kind == "R" and (int(stops), int(blown), int(diverged)) == expected, (tol, max_iter, seq, line)
        assert len(host) == len(dev) == int(stops) and host == "1" * (int(stops) - 1) + "0", line
        allowed = max(max_iter, 1)                                       # every iteration with it < max_iter: the two call patterns agree
        assert host[:allowed - 1] == dev[:allowed - 1], line
        assert peek_ok == "1", line
    for (case, expected), line in zip(direct, out[len(_RULE_CASES):]):
        assert line == "D %d" % expected, (case, line)


# (tol, the recurrence's residues, the confirmed residue of the last iterate) -> (least, blown, diverged)
_CONFIRMED_CASES = [
    ((1e-17, [1.0, 1e-8, 1e-16, 1e-24], 2e-16), (2e-16, 0, 0)),          # the recurrence ran on below the floor: what it reported is no smallest residue
    ((1e-17, [1.0, 1e-8, 1e-22, 1e-30], 2e-16), (2e-16, 0, 0)),          # (1e6 x the smallest reported: blown without the correction)
    ((1e-9, [1.0, 1e-3, 1e-6, 0.09], 0.1), (1e-6, 1, 1)),                # the recurrence agrees with the check: a real blow-up stays one
    ((1e-9, [1e-3, 1e-5, 1e-7, 1e-9], 5.0), (5.0, 0, 1)),                # lost touch and above the first residue: diverged
    ((1e-9, [1.0, 0.5, 0.25], 0.2), (0.2, 0, 0)),                        # confirmed below the recurrence
    ((1e-9, [1.0, 0.5, 0.25], 0.5), (0.5, 0, 0)),                        # exactly twice: the comparison is strict, least is the smaller one anyway
    ((1e-9, [1.0, 0.5, 0.25], _NAN), (0.5, 1, 1)),
    ((1e-9, [1.0, 0.5, _NAN], 0.25), (0.25, 0, 0)),                      # a NaN recurrence compares false: nothing is corrected
    ((1e-9, [0.5], 3.0), (3.0, 0, 0)),                                   # the first cycle: its residue is first and least whatever was reported
    ((1e-17, [1e-30, 1e-31, 1e-32], 2e-16), (2e-16, 0, 0)),              # solved by the first cycle (its recurrence undershoots): on the floor, not diverged
    ((1e-17, [1e-30, 1e-31, 1e-32], 2e-11), (2e-11, 0, 1)),              # ... but above the floor of 1e-12 it is
    ((1e-17, [1e-13, 5e-14, 4e-14], 5e-14), (5e-14, 0, 0)),              # on the floor and in touch, below the first residue
    ((1e-17, [1e-32, 3e-16, 3e-16, 3e-16], 3.1e-16), (3.1e-16, 0, 0)),    # the first recurrence undershot, the later ones are in touch (guarded steps)
]


def test_confirmed_residue_of_the_accelerated_loop(rule_exe):
    """rule_confirmed: a confirmed residue of more than twice the recurrence's raises `least` to itself (never lowers it), then rule_after."""
    out = _run(rule_exe, ["C %s %s %d %s %s" % (_hex(tol), _hex(1e-12), len(seq), " ".join(_hex(v) for v in seq), _hex(conf)) for (tol, seq, conf), _ in _CONFIRMED_CASES])
    for ((tol, seq, conf), (least, blown, diverged)), line in zip(_CONFIRMED_CASES, out):
        kind, got, b, dv = line.split()
        assert kind == "C" and float.fromhex(got) == least and (int(b), int(dv)) == (blown, diverged), (seq, conf, line)
