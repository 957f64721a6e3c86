"""Box-constrained 3-variable problems for the L-BFGS-B state machine of the converged fits (csrc/gpet_lbfgsb_dev.h), the
host build of that header, and scipy.optimize.minimize(method="L-BFGS-B") as its reference on the same float64 objective.

The corpus (``corpus()``, about 400 seeded problems) is built so that every branch of the state machine is entered: convex
and non-convex quadratics of condition up to 1e6, Rosenbrock, sums of exponentials, the GP objective of
``oracle.gpet_oracle.lml_and_grad`` on 8-20 training points; boxes that cut off the unconstrained optimum in 1, 2 and 3
variables; starts inside the box, on its corners and outside it; one and two degenerate intervals; and hand-made problems for
the memory wrap, the failed line search (a gradient inconsistent with f), the ascent direction, a vanishing step.

Reference and margins.  scipy is run unperturbed and three times with f and g perturbed by up to +-2 ulp (fixed seeds).  The
largest relative movement of an evaluation point, max |dx| / (1 + max |x|), under those perturbations is the problem's SPREAD; a
problem whose evaluation count changes or whose spread exceeds 1e-6 is REFERENCE-UNSTABLE and left out of the path comparison
(cap: 2 % of the corpus).  The state machine must then match scipy's evaluation count and stop reason, and every evaluation
point and the final f within ten times the problem's own spread (floor 1e-12): the factor of ten because a dense 3 x 3 B and
scipy's compact form round differently.

scipy does not call the objective again at the point it has just evaluated, so a line search that stalls in the last bit shows
fewer evaluations in scipy than the state machine counts: evaluation counts and paths are compared with such immediate repeats
left out (``run_host``: nfev against nfev_raw).

Measured with scipy 1.15.3 on x86-64, g++ -O2 -ffp-contract=off (``python -m tests.lbfgsb_cases`` prints them again):
    416 problems; 8 reference-unstable (1.92 %; 1.4 % of 3000 further problems of the same generator)
    largest spread of a stable problem                         1.17e-07  (the cut is 1e-6)
    largest difference of a problem that agrees with scipy     9.51e-09  (its margin: ten times its spread of 1.05e-08)
    stable problems that leave scipy's path                    1 (seed 292; 9 of the 3000 further ones, none to a worse minimum)
Before lb_subsm counted a noise-level descent test as "no descent" (csrc/gpet_lbfgsb.hip), the unstable problems 168 and 297
ended 37 % and 17 % above scipy's minimum.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_edge_trace_amd", "csrc")

UNSTABLE_CUT = 1e-6     # spread above which scipy does not reproduce its own path
UNSTABLE_CAP = 0.02     # share of the corpus that may be reference-unstable
MARGIN_FACTOR = 10.0
MARGIN_FLOOR = 1e-12
PGTOL = 1e-5
FACTR_EPS = 1e7 * 2.220446049250313e-16

BRANCHES = ("ls_continue", "ls_converged", "ls_warning", "dcstep_1", "dcstep_2", "dcstep_3", "dcstep_4", "cauchy_break",
            "subsm_projected", "subsm_backtrack", "restart_ascent", "restart_lnsrch", "restart_stale", "skip_update", "memory_shift",
            "why_1", "why_2", "why_3", "why_4", "why_5")

SHIM = r"""
#include "gpet_lbfgsb_dev.h"
#include <string.h>
using namespace gpet;
#ifdef LB_BRANCH_CENSUS
namespace gpet { long long lb_census[LB_NBRANCH]; }
#endif
extern "C" {
int shim_sizeof(void) { return (int)sizeof(LbProb); }
int shim_nbranch(void) { return (int)LB_NBRANCH; }
void shim_init(void* p, const double* start, const double* lo, const double* hi) {
  memset(p, 0, sizeof(LbProb));
  lb_init(*static_cast<LbProb*>(p), start, lo, hi);
}
// 1 while the problem wants the objective at xe, 0 when it is done
int shim_pending(const void* p, double* xe) {
  const LbProb& q = *static_cast<const LbProb*>(p);
  for (int i = 0; i < 3; ++i) xe[i] = q.xe[i];
  return q.task != LB_TASK_DONE;
}
void shim_advance(void* p, double f, const double* g, const double* lo, const double* hi) {
  lb_advance(*static_cast<LbProb*>(p), f, g, lo, hi);
}
// out = x[3], f, g[3], iter, nfev, why  (the layout gpet_final_problems returns)
void shim_record(const void* p, double* out) {
  const LbProb& q = *static_cast<const LbProb*>(p);
  for (int i = 0; i < 3; ++i) {
    out[i] = q.x[i];
    out[4 + i] = q.g[i];
  }
  out[3] = q.f;
  out[7] = q.iter;
  out[8] = q.nfev;
  out[9] = q.why;
}
// what the next iteration would start from: the dense B, the Cauchy point and its free set (for diagnosis)
void shim_model(const void* p, const double* lo, const double* hi, double* B9, double* xcp, int* free_) {
  const LbProb& q = *static_cast<const LbProb*>(p);
  double B[3][3];
  lb_dense_B(q, B);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) B9[3 * i + j] = B[i][j];
  lb_cauchy(q.x, q.g, lo, hi, B, lb_projgr(q.x, q.g, lo, hi), xcp, free_);
}
void shim_census(long long* out) {
#ifdef LB_BRANCH_CENSUS
  for (int i = 0; i < LB_NBRANCH; ++i) out[i] = lb_census[i];
#else
  (void)out;
#endif
}
}
"""


def compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = cxx and shutil.which(cxx)
        if path:
            return path
    return None


def build_shim(workdir, census=False):
    """The state machine's header compiled for the host as the kernels compile it (no contraction), behind a C ABI."""
    cxx = compiler()
    if cxx is None:
        return None
    name = "lbfgsb_census" if census else "lbfgsb_host"
    src, so = os.path.join(str(workdir), name + ".cpp"), os.path.join(str(workdir), "lib" + name + ".so")
    with open(src, "w") as fh:
        fh.write(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC]
                   + (["-DLB_BRANCH_CENSUS"] if census else []) + [src, "-o", so], check=True)
    lib = C.CDLL(so)
    assert lib.shim_nbranch() == len(BRANCHES)
    return lib


def census(lib):
    out = (C.c_longlong * len(BRANCHES))()
    lib.shim_census(out)
    return dict(zip(BRANCHES, list(out)))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def run_host(lib, fun, x0, lo, hi, max_evals=5000):
    """Drive the host build: fun(x) -> (f, g).  Returns dict(path [nfev, 3], x, f, g, iter, nfev, why)."""
    buf = np.zeros(lib.shim_sizeof() // 8 + 1)
    x0, lo, hi = (np.ascontiguousarray(a, dtype=np.float64) for a in (x0, lo, hi))
    lib.shim_init(_ptr(buf), _ptr(x0), _ptr(lo), _ptr(hi))
    xe = np.zeros(3)
    path = []
    while lib.shim_pending(_ptr(buf), _ptr(xe)):
        if len(path) >= max_evals:
            raise RuntimeError("host L-BFGS-B: %d evaluations" % len(path))
        path.append(xe.copy())
        f, g = fun(xe.copy())
        g = np.ascontiguousarray(g, dtype=np.float64)
        lib.shim_advance(_ptr(buf), C.c_double(float(f)), _ptr(g), _ptr(lo), _ptr(hi))
    rec = np.zeros(10)
    lib.shim_record(_ptr(buf), _ptr(rec))
    # scipy does not call the objective again at the point it has just evaluated (its ScalarFunction keeps the last value), which
    # happens when a line search stalls in the last bit: `path` / `nfev` leave such repeats out as scipy's do, `nfev_raw` counts them
    path = np.array(path).reshape(-1, 3)
    keep = np.ones(path.shape[0], dtype=bool)
    keep[1:] = np.any(path[1:] != path[:-1], axis=1)
    assert int(rec[8]) == path.shape[0]
    return dict(path=path[keep], x=rec[0:3].copy(), f=rec[3], g=rec[4:7].copy(), iter=int(rec[7]), nfev=int(keep.sum()),
                nfev_raw=int(rec[8]), why=int(rec[9]), state=buf)


def run_host_lockstep(lib, eval_batch, starts, lo, hi):
    """Many problems with one box, advanced round by round as the device's driver advances them: eval_batch(index [k],
    x [k, 3]) -> (f [k], g [k, 3]) evaluates the pending points of the problems `index` in one call.  Returns the records
    (x [P, 3], f, g, iter, nfev, why) -- nfev counts every evaluation, as the device's record does."""
    starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, 3)
    lo, hi = (np.ascontiguousarray(a, dtype=np.float64) for a in (lo, hi))
    P = starts.shape[0]
    bufs = [np.zeros(lib.shim_sizeof() // 8 + 1) for _ in range(P)]
    for i in range(P):
        lib.shim_init(_ptr(bufs[i]), _ptr(np.ascontiguousarray(starts[i])), _ptr(lo), _ptr(hi))
    xe = np.zeros(3)
    for _ in range(4000):
        idx, pts = [], []
        for i in range(P):
            if lib.shim_pending(_ptr(bufs[i]), _ptr(xe)):
                idx.append(i)
                pts.append(xe.copy())
        if not idx:
            break
        f, g = eval_batch(np.array(idx), np.array(pts))
        for k, i in enumerate(idx):
            gk = np.ascontiguousarray(g[k], dtype=np.float64)
            lib.shim_advance(_ptr(bufs[i]), C.c_double(float(f[k])), _ptr(gk), _ptr(lo), _ptr(hi))
    else:
        raise RuntimeError("host L-BFGS-B: problems still running after 4000 rounds")
    rec = np.zeros((P, 10))
    for i in range(P):
        lib.shim_record(_ptr(bufs[i]), _ptr(rec[i]))
    return dict(x=rec[:, 0:3].copy(), f=rec[:, 3].copy(), g=rec[:, 4:7].copy(), iter=rec[:, 7].astype(np.int64),
                nfev=rec[:, 8].astype(np.int64), why=rec[:, 9].astype(np.int64))


def host_model(lib, state, lo, hi):
    B, xcp, fr = np.zeros(9), np.zeros(3), np.zeros(3, dtype=np.int32)
    lo, hi = (np.ascontiguousarray(a, dtype=np.float64) for a in (lo, hi))
    lib.shim_model(_ptr(state), _ptr(lo), _ptr(hi), _ptr(B), _ptr(xcp), _ptr(fr))
    return B.reshape(3, 3), xcp, fr


def scipy_stop(message):
    """scipy's message -> the state machine's classes of `why`: 'pg' (1, 2), 'factr' (3), 'abnormal' (4, 5)."""
    if "PROJECTED GRADIENT" in message:
        return "pg"
    if "REDUCTION OF F" in message:
        return "factr"
    if "ABNORMAL" in message:
        return "abnormal"
    if "fixed by bounds" in message:  # (every interval degenerate: the projected gradient is zero)
        return "pg"
    return message


WHY_STOP = {1: "pg", 2: "pg", 3: "factr", 4: "abnormal", 5: "abnormal"}


def run_scipy(fun, x0, lo, hi, perturb_seed=None):
    """scipy's L-BFGS-B (defaults: m = 10, factr = 1e7, pgtol = 1e-5, maxls = 20) on fun, optionally with f and g
    moved by up to +-2 ulp per evaluation.  Returns dict(path, x, f, nfev, nit, stop)."""
    import scipy.optimize
    rng = None if perturb_seed is None else np.random.default_rng(perturb_seed)
    path = []

    def obj(x):
        path.append(np.array(x, dtype=np.float64))
        f, g = fun(np.array(x, dtype=np.float64))
        f, g = float(f), np.array(g, dtype=np.float64)
        if rng is not None and np.isfinite(f) and np.all(np.isfinite(g)):
            f = f + float(rng.integers(-2, 3)) * float(np.spacing(abs(f)))
            g = g + rng.integers(-2, 3, size=3) * np.spacing(np.abs(g))
        return f, g
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (a start outside the box is clipped, with a warning)
        res = scipy.optimize.minimize(obj, np.array(x0, dtype=np.float64), jac=True, method="L-BFGS-B",
                                      bounds=list(zip(lo, hi)), options=dict(maxiter=15000, maxfun=10 ** 6))
    return dict(path=np.array(path).reshape(-1, 3), x=np.array(res.x), f=float(res.fun), nfev=len(path), nit=int(res.get("nit", 0)),
                stop=scipy_stop(res.message))


def path_diff(a, b):
    """largest movement of an evaluation point between two paths of equal length, relative to 1 + max |x|"""
    if a.shape[0] == 0:
        return 0.0
    return float(np.max(np.max(np.abs(a - b), axis=1) / (1.0 + np.max(np.abs(b), axis=1))))


def reference(pb):
    """scipy's path on the problem and its stability: dict(ref, stable, spread, spread_f)."""
    ref = run_scipy(pb["fun"], pb["x0"], pb["lo"], pb["hi"])
    spread, spread_f, stable = 0.0, 0.0, True
    for s in (101, 202, 303):
        r = run_scipy(pb["fun"], pb["x0"], pb["lo"], pb["hi"], perturb_seed=s + 1000 * pb["seed"])
        if r["nfev"] != ref["nfev"] or r["stop"] != ref["stop"]:
            stable = False
            continue
        spread = max(spread, path_diff(r["path"], ref["path"]))
        spread_f = max(spread_f, abs(r["f"] - ref["f"]) / (1.0 + abs(ref["f"])))
    if spread > UNSTABLE_CUT:
        stable = False
    return dict(ref=ref, stable=stable, spread=spread, spread_f=spread_f)


def margin(spread):
    return max(MARGIN_FACTOR * spread, MARGIN_FLOOR)


def projected_gradient(x, g, lo, hi):
    pg = np.where(g < 0, np.maximum(x - hi, g), np.minimum(x - lo, g))
    return float(np.max(np.abs(pg)))


# ---- objectives -------------------------------------------------------------------------------------------------------
def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.diag(r))


class Quadratic:
    """0.5 (x - c)^T A (x - c), A = Q diag(lam) Q^T; lam may hold a negative value (non-convex: the box bounds it)"""
    def __init__(self, rng, cond, convex=True):
        lam = np.array([1.0, np.sqrt(cond) ** rng.uniform(0.5, 1.5), cond]) * 10.0 ** rng.uniform(-2, 1)
        if not convex:
            lam[int(rng.integers(0, 3))] *= -rng.uniform(0.05, 0.5)
        q = _rotation(rng)
        self.A = (q * lam) @ q.T
        self.A = 0.5 * (self.A + self.A.T)
        self.c = rng.uniform(-2, 2, size=3)

    def __call__(self, x):
        r = self.A @ (x - self.c)
        return 0.5 * float((x - self.c) @ r), r

    def centre(self):
        return self.c


class Wavy(Quadratic):
    """a convex quadratic plus cosines: many local minima, curvature of both signs along a line search"""
    def __init__(self, rng, cond):
        Quadratic.__init__(self, rng, cond)
        self.a = rng.uniform(0.5, 3.0) * self.A.diagonal().mean()
        self.w = rng.uniform(1.0, 4.0, size=3)
        self.ph = rng.uniform(0, 2 * np.pi, size=3)

    def __call__(self, x):
        f, g = Quadratic.__call__(self, x)
        return f + self.a * float(np.cos(self.w * x + self.ph).sum()), g - self.a * self.w * np.sin(self.w * x + self.ph)


class Rosenbrock:
    def __init__(self, rng=None):
        self.s = 1.0 if rng is None else rng.uniform(0.5, 2.0)

    def __call__(self, x):
        s = self.s
        a, b = x[1:] - s * x[:-1] ** 2, 1.0 - x[:-1]
        f = float((100.0 * a ** 2 + b ** 2).sum())
        g = np.zeros(3)
        g[:-1] += -400.0 * s * x[:-1] * a - 2.0 * b
        g[1:] += 200.0 * a
        return f, g

    def centre(self):
        return np.array([1.0, self.s, self.s ** 3])


class Exponential:
    """sum_k exp(a_k . x - b_k) + 0.5 mu |x|^2: convex, with a gradient that grows by orders of magnitude across the box"""
    def __init__(self, rng):
        self.a = rng.standard_normal((5, 3)) * rng.uniform(0.5, 2.0)
        self.b = rng.uniform(0, 2, size=5)
        self.mu = 10.0 ** rng.uniform(-3, 0)

    def __call__(self, x):
        e = np.exp(self.a @ x - self.b)
        return float(e.sum()) + 0.5 * self.mu * float(x @ x), self.a.T @ e + self.mu * x

    def centre(self):
        return np.zeros(3)


class GpObjective:
    """-log marginal likelihood of the tracer's GP (oracle.gpet_oracle.lml_and_grad) on n training points, in
    theta = log(constant, length_scale, noise_level)"""
    def __init__(self, rng, n, kernel="RBF"):
        x = np.sort(rng.choice(np.arange(0, 6 * n), size=n, replace=False)).astype(np.float64)
        y = 20.0 * np.sin(x / (1.5 * n)) + rng.standard_normal(n) * rng.uniform(0.2, 3.0)
        self.xs = (x - x.mean()) / x.std()
        self.yt = (y - y.mean()) / y.std()
        self.w = np.ones(n)
        self.w[[0, -1]] = 1e-7
        self.kernel = kernel

    @classmethod
    def from_training(cls, xs, yt, w, kernel="RBF"):
        self = cls.__new__(cls)
        self.xs, self.yt, self.w, self.kernel = np.asarray(xs), np.asarray(yt), np.asarray(w), kernel
        return self

    def __call__(self, th):
        from oracle import gpet_oracle as orc
        lml, g = orc.lml_and_grad(np.asarray(th, dtype=np.float64), self.xs, self.yt, self.w, self.kernel, 2.5)
        if not np.isfinite(lml):
            return np.inf, np.zeros(3)
        return -float(lml), -np.asarray(g, dtype=np.float64)

    def centre(self):
        return np.log([1.0, 1.0, 1e-2])


class WrongGradient:
    """f of `inner` with the gradient's sign flipped once |x - centre| < radius: no step along -g decreases f there"""
    def __init__(self, inner, radius):
        self.inner, self.radius = inner, radius

    def __call__(self, x):
        f, g = self.inner(x)
        if np.max(np.abs(x - self.inner.centre())) < self.radius:
            g = -g
        return f, g

    def centre(self):
        return self.inner.centre()


class Kinked:
    """|x - c| in one variable, smooth elsewhere: the gradient jumps at the kink, so a stored pair carries curvature that
    the next iterate contradicts"""
    def __init__(self, rng):
        self.q = Quadratic(rng, 10.0)
        self.k = rng.uniform(2.0, 20.0)

    def __call__(self, x):
        f, g = self.q(x)
        d = x[0] - self.q.c[0]
        g = g.copy()
        g[0] += self.k * np.sign(d)
        return f + self.k * abs(d), g

    def centre(self):
        return self.q.c


class Linear:
    def __init__(self, g):
        self.g = np.array(g, dtype=np.float64)

    def __call__(self, x):
        return float(self.g @ x), self.g.copy()


# ---- boxes and starts ---------------------------------------------------------------------------------------------------
def _box(rng, centre, n_cut, width):
    """a box around `centre` of which n_cut variables' intervals exclude the centre"""
    lo = centre - width * rng.uniform(0.5, 1.5, size=3)
    hi = centre + width * rng.uniform(0.5, 1.5, size=3)
    for i in rng.permutation(3)[:n_cut]:
        off = width * rng.uniform(0.05, 0.8)
        if rng.uniform() < 0.5:
            lo[i], hi[i] = centre[i] + off, centre[i] + off + width * rng.uniform(0.3, 1.5)
        else:
            lo[i], hi[i] = centre[i] - off - width * rng.uniform(0.3, 1.5), centre[i] - off
    return lo, hi


def _start(rng, lo, hi, kind):
    if kind == "inside":
        return lo + (hi - lo) * rng.uniform(0.05, 0.95, size=3)
    if kind == "corner":
        return np.where(rng.uniform(size=3) < 0.5, lo, hi)
    if kind == "face":
        x = lo + (hi - lo) * rng.uniform(0.05, 0.95, size=3)
        i = int(rng.integers(0, 3))
        x[i] = lo[i] if rng.uniform() < 0.5 else hi[i]
        return x
    return lo + (hi - lo) * rng.uniform(-0.5, 1.5, size=3)  # "outside": projected by the optimiser


N_RANDOM = 400
FAMILIES = ("quad", "quad_ill", "nonconvex", "wavy", "rosenbrock", "exponential", "gp", "gp_matern")
STARTS = ("inside", "corner", "face", "outside")


def random_problem(seed):
    rng = np.random.default_rng(77000 + seed)
    fam = FAMILIES[seed % len(FAMILIES)]
    kind = STARTS[(seed // len(FAMILIES)) % len(STARTS)]
    n_cut = (seed // (len(FAMILIES) * len(STARTS))) % 4
    width = 2.0
    if fam == "quad":
        fun = Quadratic(rng, 10.0 ** rng.uniform(0, 3))
    elif fam == "quad_ill":
        fun = Quadratic(rng, 10.0 ** rng.uniform(3, 6))
    elif fam == "nonconvex":
        fun = Quadratic(rng, 10.0 ** rng.uniform(0, 4), convex=False)
    elif fam == "wavy":
        fun = Wavy(rng, 10.0 ** rng.uniform(0, 2))
    elif fam == "rosenbrock":
        fun = Rosenbrock(rng)
    elif fam == "exponential":
        fun = Exponential(rng)
    elif fam in ("gp", "gp_matern"):
        fun = GpObjective(rng, int(rng.integers(8, 21)), "RBF" if fam == "gp" else "Matern")
        width = 3.0
    elif fam == "kinked":
        fun = Kinked(rng)
    else:
        fun = WrongGradient(Quadratic(rng, 10.0 ** rng.uniform(0, 2)), rng.uniform(0.05, 0.5))
        n_cut = 0
    lo, hi = _box(rng, fun.centre(), n_cut, width)
    x0 = _start(rng, lo, hi, kind)
    n_deg = (0, 0, 0, 1, 2)[seed % 5] if seed % 3 == 0 else 0
    for i in rng.permutation(3)[:n_deg]:  # degenerate intervals
        hi[i] = lo[i]
    return dict(seed=seed, name="%s/%s/cut%d/deg%d" % (fam, kind, n_cut, n_deg), fun=fun, x0=x0, lo=lo, hi=hi)


def kinked_problem(k):
    rng = np.random.default_rng(31000 + k)
    fun = Kinked(rng)
    lo, hi = _box(rng, fun.centre(), k % 3, 2.0)
    return fun, _start(rng, lo, hi, "inside"), lo, hi


def steep_exponential_problem(k):
    rng = np.random.default_rng(32000 + k)
    fun = Exponential(rng)
    fun.a *= rng.uniform(3.0, 12.0)
    lo, hi = _box(rng, fun.centre(), k % 3, 2.0)
    return fun, _start(rng, lo, hi, "inside"), lo, hi


def wrong_gradient_problem(k):
    rng = np.random.default_rng(33000 + k)
    fun = WrongGradient(Quadratic(rng, 10.0 ** rng.uniform(0, 2)), rng.uniform(0.05, 0.5))
    lo, hi = _box(rng, fun.centre(), 0, 2.0)
    return fun, _start(rng, lo, hi, "inside"), lo, hi


# members of the three families above that enter the rare branches (found by running the census build over k = 0..399)
KINKED_LNSRCH_RESTART = (88, 214, 383)
STEEP_ASCENT_RESTART = (1, 27, 32, 62)
WRONG_GRADIENT_LNSRCH_RESTART = ()


def special_problems():
    out = []

    def add(name, fun, x0, lo, hi):
        out.append(dict(seed=N_RANDOM + len(out), name=name, fun=fun, x0=np.array(x0, dtype=np.float64),
                        lo=np.array(lo, dtype=np.float64), hi=np.array(hi, dtype=np.float64)))
    # more than 10 iterations in a free box: the memory of 10 pairs wraps
    add("rosenbrock/memory_wrap", Rosenbrock(), [-1.2, 1.0, 1.0], [-5, -5, -5], [5, 5, 5])
    # the same with an optimum on a face
    add("rosenbrock/memory_wrap_bound", Rosenbrock(), [-1.2, 1.0, 1.0], [-5, -5, -5], [0.5, 5, 5])
    # f rises gently along the direction that the reported gradient calls steeply downhill: every trial step is halved, 20
    # trial points, no memory to drop (why 5)
    add("wrong_gradient/first_iteration", _Uphill(), [0.5, 0.6, 0.7], [0, 0, 0], [1, 1, 1])
    q = Quadratic(np.random.default_rng(5), 10.0)
    # the step vanishes in the rounding of a huge coordinate: d = 0 at the first iteration (why 4)
    add("linear/vanishing_step", Linear([1e-4, 0.0, 0.0]), [1e13, 0.5, 0.5], [0, 0, 0], [2e13, 1, 1])
    # stationary on a corner at the first evaluation (why 1)
    add("linear/stationary_corner", Linear([1.0, -2.0, 3.0]), [0, 1, 0], [0, 0, 0], [1, 1, 1])
    add("linear/to_corner", Linear([1.0, -2.0, 3.0]), [0.3, 0.4, 0.5], [0, 0, 0], [1, 1, 1])
    # every interval degenerate
    add("quad/all_degenerate", q, q.c + 1, q.c + 1, q.c + 1)
    # flat objective value: the reduction of f falls under factr * eps (why 3)
    add("quartic/flat", _Quartic(), [1.0, 1.0, 1.0], [-2, -2, -2], [2, 2, 2])
    add("quartic/flat_bound", _Quartic(), [1.0, 1.0, 1.0], [-2, 1e-3, -2], [2, 2, 2])
    # the gradient jumps at a kink: the line search fails with pairs in the memory, which is dropped (restart, then why 3 or 5)
    for k in KINKED_LNSRCH_RESTART:
        add("kinked/%d" % k, *kinked_problem(k))
    for k in WRONG_GRADIENT_LNSRCH_RESTART:
        add("wrong_gradient/%d" % k, *wrong_gradient_problem(k))
    # gradients that span many orders of magnitude: a stored pair leaves B indefinite in rounding and the next direction
    # points uphill (ascent restart)
    for k in STEEP_ASCENT_RESTART:
        add("steep_exponential/%d" % k, *steep_exponential_problem(k))
    return out


class _Uphill:
    def __call__(self, x):
        return -1e-3 * float(x.sum()), np.ones(3)


class _Quartic:
    def __call__(self, x):
        return 1e6 + float((x ** 4).sum()), 4.0 * x ** 3


_CORPUS = None


def corpus():
    global _CORPUS
    if _CORPUS is None:
        _CORPUS = [random_problem(s) for s in range(N_RANDOM)] + special_problems()
    return _CORPUS


def _measure():
    import tempfile
    d = tempfile.mkdtemp()
    lib = build_shim(d, census=True)
    n_unstable, worst_spread, worst_agree, bad = 0, 0.0, 0.0, []
    for pb in corpus():
        ref = reference(pb)
        h = run_host(lib, pb["fun"], pb["x0"], pb["lo"], pb["hi"])
        if not ref["stable"]:
            n_unstable += 1
            print("unstable %3d %-40s spread %.2e  nfev host %d scipy %d  f host %.10g scipy %.10g" %
                  (pb["seed"], pb["name"], ref["spread"], h["nfev"], ref["ref"]["nfev"], h["f"], ref["ref"]["f"]))
            continue
        worst_spread = max(worst_spread, ref["spread"])
        r = ref["ref"]
        same = h["nfev"] == r["nfev"] and WHY_STOP[h["why"]] == r["stop"]
        dx = path_diff(h["path"], r["path"]) if h["nfev"] == r["nfev"] else float("inf")
        df = abs(h["f"] - r["f"]) / (1 + abs(r["f"]))
        if same and dx <= margin(ref["spread"]) and df <= margin(ref["spread"]):
            worst_agree = max(worst_agree, dx)
        else:
            bad.append(pb["seed"])
            k = 0
            n = min(h["nfev"], r["nfev"])
            while k < n and np.max(np.abs(h["path"][k] - r["path"][k])) <= margin(ref["spread"]) * (1 + np.max(np.abs(r["path"][k]))):
                k += 1
            print("DIFFER   %3d %-40s spread %.2e dx %.2e df %.2e nfev %d/%d why %d/%s first differing eval %d  f %.10g/%.10g" %
                  (pb["seed"], pb["name"], ref["spread"], dx, df, h["nfev"], r["nfev"], h["why"], r["stop"], k, h["f"], r["f"]))
    print("problems %d, unstable %d (%.2f %%), largest stable spread %.2e, largest agreeing difference %.2e" %
          (len(corpus()), n_unstable, 100.0 * n_unstable / len(corpus()), worst_spread, worst_agree))
    print("differing:", bad)
    print("census:", census(lib))


if __name__ == "__main__":
    _measure()
