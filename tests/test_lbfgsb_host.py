"""CPU tests of the L-BFGS-B state machine (csrc/gpet_lbfgsb_dev.h) against scipy on box-constrained problems: the header
needs no HIP, so a small extern "C" shim around it is compiled with the host C++ compiler, without contraction as the kernels
that call it are, and driven through ctypes (tests/lbfgsb_cases.py has the corpus, the scipy driver and the margins)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import lbfgsb_cases as lc  # noqa: E402

# Stable problems on which the state machine leaves scipy's path, by seed, with what is known (gpet_lbfgsb.hip has the
# paragraph).  They are a strict xfail of their own below: a problem that starts to agree must be taken off the list.
#   292: scipy's subspace step runs on a K matrix whose rows for the older pairs were last formed for another free set and,
#        before the memory was dropped, for other pairs (formk is skipped in iterations without free variables and updates
#        its matrix incrementally afterwards); the state machine always steps on the B of the stored pairs.  Same minimum.
KNOWN_DIFFERENT = {292}


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    if lc.compiler() is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("lbfgsb")
    return lc.build_shim(d), lc.build_shim(d, census=True)


@pytest.fixture(scope="module")
def runs(libs):
    """every problem of the corpus: scipy's reference (with its stability) and the host build's run, computed once; the
    census build runs the corpus as well and leaves its branch counts"""
    lib, census_lib = libs
    out = []
    for pb in lc.corpus():
        ref = lc.reference(pb)
        host = lc.run_host(lib, pb["fun"], pb["x0"], pb["lo"], pb["hi"])
        counted = lc.run_host(census_lib, pb["fun"], pb["x0"], pb["lo"], pb["hi"])
        assert np.array_equal(counted["path"], host["path"]) and counted["why"] == host["why"]  # counting changes nothing
        out.append((pb, ref, host))
    return out


def _compare(pb, ref, host):
    """'' if the host run follows scipy's within the problem's margin, else what differs"""
    r, m = ref["ref"], lc.margin(ref["spread"])
    if host["nfev"] != r["nfev"]:
        return "evaluations %d, scipy %d" % (host["nfev"], r["nfev"])
    if lc.WHY_STOP[host["why"]] != r["stop"]:
        return "why %d, scipy %s" % (host["why"], r["stop"])
    dx = lc.path_diff(host["path"], r["path"])
    if dx > m:
        return "evaluation points %.3g apart, margin %.3g" % (dx, m)
    df = abs(host["f"] - r["f"]) / (1.0 + abs(r["f"]))
    if df > m:
        return "final f %.3g apart, margin %.3g" % (df, m)
    return ""


def test_corpus_enters_every_branch(libs, runs):
    counts = lc.census(libs[1])
    print(counts)
    assert sorted(counts) == sorted(lc.BRANCHES)
    never = [k for k, v in counts.items() if v == 0]
    assert not never, never


def test_reference_unstable_share_within_the_cap(runs):
    unstable = [pb["seed"] for pb, ref, _ in runs if not ref["stable"]]
    print("reference-unstable: %d of %d" % (len(unstable), len(runs)), unstable)
    assert 380 <= len(runs) <= 440
    assert len(unstable) <= lc.UNSTABLE_CAP * len(runs), unstable


def test_host_path_equals_scipy_on_stable_problems(runs):
    """evaluation count, stop reason, every evaluation point and the final f, on every problem on which scipy reproduces its
    own path under +-2 ulp of noise in f and g"""
    bad, worst_spread, worst_agree = [], 0.0, 0.0
    for pb, ref, host in runs:
        if not ref["stable"]:
            continue
        worst_spread = max(worst_spread, ref["spread"])
        if pb["seed"] in KNOWN_DIFFERENT:
            continue
        why = _compare(pb, ref, host)
        if why:
            bad.append((pb["seed"], pb["name"], why))
        else:
            worst_agree = max(worst_agree, lc.path_diff(host["path"], ref["ref"]["path"]))
    print("largest stable spread %.3g, largest agreeing difference %.3g" % (worst_spread, worst_agree))
    assert not bad, bad


@pytest.mark.parametrize("seed", sorted(KNOWN_DIFFERENT))
@pytest.mark.xfail(strict=True, reason="leaves scipy's path for a known cause (see KNOWN_DIFFERENT); same minimum")
def test_known_different_problem_follows_scipy(runs, seed):
    (pb, ref, host), = [t for t in runs if t[0]["seed"] == seed]
    assert ref["stable"]
    why = _compare(pb, ref, host)
    assert not why, why


def test_known_different_problems_reach_scipys_minimum(runs):
    """the problems on the list still end inside the box, stationary, and no worse than scipy by 1e-6 (1 + |f|)"""
    seen = set()
    for pb, ref, host in runs:
        if pb["seed"] in KNOWN_DIFFERENT:
            seen.add(pb["seed"])
            assert ref["stable"], pb["seed"]
            _check_end_point(pb, ref, host)
    assert seen == KNOWN_DIFFERENT


def _check_end_point(pb, ref, host):
    x, lo, hi = host["x"], pb["lo"], pb["hi"]
    assert np.all(x >= lo) and np.all(x <= hi), (pb["seed"], x)
    f, g = pb["fun"](x)
    assert f == host["f"] and np.array_equal(np.asarray(g, dtype=np.float64), host["g"]), pb["seed"]  # the record is the end point's
    r = ref["ref"]
    assert host["f"] - r["f"] <= 1e-6 * (1.0 + abs(r["f"])), (pb["seed"], pb["name"], host["f"], r["f"])
    if host["why"] in (1, 2):
        assert lc.projected_gradient(x, host["g"], lo, hi) <= lc.PGTOL, pb["seed"]
    else:
        # a legitimate stop on the reduction of f (3), or an abnormal one (4, 5) that scipy reports too
        assert host["why"] == 3 or r["stop"] == "abnormal", (pb["seed"], host["why"], r["stop"])


def test_reference_unstable_problems_end_at_a_valid_point(runs):
    n = 0
    for pb, ref, host in runs:
        if not ref["stable"]:
            n += 1
            _check_end_point(pb, ref, host)
    assert n > 0


def test_every_problem_ends_inside_its_box(runs):
    for pb, ref, host in runs:
        assert np.all(host["path"] >= pb["lo"]) and np.all(host["path"] <= pb["hi"]), pb["seed"]
        assert 1 <= host["why"] <= 5 and host["nfev_raw"] >= host["nfev"] >= 1


SANITIZED_MAIN = r"""
#include "gpet_lbfgsb_dev.h"
#include <stdio.h>
#include <string.h>
using namespace gpet;
// extended Rosenbrock in 3 variables
static double rosen(const double* x, double* g) {
  double f = 0.0;
  g[0] = g[1] = g[2] = 0.0;
  for (int i = 0; i < 2; ++i) {
    const double a = x[i + 1] - x[i] * x[i], b = 1.0 - x[i];
    f += 100.0 * a * a + b * b;
    g[i] += -400.0 * x[i] * a - 2.0 * b;
    g[i + 1] += 200.0 * a;
  }
  return f;
}
static double bowl(const double* x, double* g) {
  const double c[3] = {0.3, -0.7, 1.9}, w[3] = {1.0, 30.0, 900.0};
  double f = 0.0;
  for (int i = 0; i < 3; ++i) {
    f += 0.5 * w[i] * (x[i] - c[i]) * (x[i] - c[i]);
    g[i] = w[i] * (x[i] - c[i]);
  }
  return f;
}
static double uphill(const double* x, double* g) {  // the reported gradient contradicts f: the line search fails
  g[0] = g[1] = g[2] = 1.0;
  return -1e-3 * (x[0] + x[1] + x[2]);
}
typedef double (*Fun)(const double*, double*);
static int run(const char* name, Fun fun, const double* x0, const double* lo, const double* hi, int want_why, int min_iter) {
  LbProb* p = new LbProb;  // (on the heap: the sanitizer then sees reads and writes past the record)
  memset(p, 0, sizeof *p);
  lb_init(*p, x0, lo, hi);
  int evals = 0;
  while (p->task != LB_TASK_DONE && evals < 5000) {
    double g[3];
    const double f = fun(p->xe, g);
    lb_advance(*p, f, g, lo, hi);
    ++evals;
  }
  int ok = p->task == LB_TASK_DONE && p->why == want_why && p->iter >= min_iter && p->nfev == evals;
  for (int i = 0; i < 3; ++i) ok = ok && p->x[i] >= lo[i] && p->x[i] <= hi[i];
  printf("%s: why %d iter %d nfev %d x %.6f %.6f %.6f f %.6g %s\n", name, p->why, p->iter, p->nfev, p->x[0], p->x[1], p->x[2], p->f,
         ok ? "ok" : "WRONG");
  delete p;
  return ok ? 0 : 1;
}
int main() {
  int bad = 0;
  const double wide_lo[3] = {-5, -5, -5}, wide_hi[3] = {5, 5, 5};
  const double s0[3] = {-1.2, 1.0, 1.0};
  bad += run("rosenbrock, memory wraps", rosen, s0, wide_lo, wide_hi, 3, 12);  // (scipy stops on the reduction of f here too)
  const double cut_hi[3] = {0.5, 5, 5};
  bad += run("rosenbrock, optimum on a face", rosen, s0, wide_lo, cut_hi, 2, 5);
  const double deg_lo[3] = {-2, 0.25, -2}, deg_hi[3] = {2, 0.25, 1.0};
  const double s1[3] = {7.0, 9.0, -9.0};  // outside the box: projected
  bad += run("bowl, a degenerate interval and a binding bound", bowl, s1, deg_lo, deg_hi, 2, 1);
  const double all_lo[3] = {1, 2, 3};
  bad += run("bowl, every interval degenerate", bowl, s1, all_lo, all_lo, 1, 0);
  const double u_lo[3] = {0, 0, 0}, u_hi[3] = {1, 1, 1}, s2[3] = {0.5, 0.6, 0.7};
  bad += run("line search fails", uphill, s2, u_lo, u_hi, 5, 0);
  return bad;
}
"""


def test_host_build_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """a stand-alone program around the header, built with -fsanitize=address,undefined, over analytic problems with the
    memory wrap, binding bounds, degenerate intervals and a failed line search (its own process: nothing is loaded here)"""
    cxx = lc.compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    src, exe = tmp_path / "lbfgsb_san.cpp", tmp_path / "lbfgsb_san"
    src.write_text(SANITIZED_MAIN)
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", lc.CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0:
        if "sanitize" in build.stderr or "asan" in build.stderr or "ubsan" in build.stderr:
            pytest.skip("the compiler lacks the sanitizer runtime")
        raise AssertionError(build.stderr[-3000:])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.count(" ok\n") == 5 and "WRONG" not in out.stdout
