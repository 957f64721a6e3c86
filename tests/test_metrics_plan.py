"""CPU tests of the denoise quality metrics' arithmetic in csrc/gpet_metrics_plan.h (the header needs no HIP: a small extern "C" shim
around it is compiled with the host C++ compiler and -ffp-contract=off, as tests/test_label_plan.py does), of the words of its refusals
as _lib repeats them, and of the ABI surface of gpet_metrics_images.

The expected values come from tests/metrics_ref.py, the arithmetic restated with numpy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import metrics_ref as R
from tests.test_denoise_plan import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_edge_trace_amd", "csrc")
DT = (np.uint8, np.uint16, np.float32, np.float64)


# ---- ABI surface ---------------------------------------------------------------------------------------------------------------
def test_the_call_is_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_edge_trace_amd import _lib
    header = open(os.path.join(ROOT, "include", "gpet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(gpet_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(_lib.LIB_PATH)
    name = "gpet_metrics_images"
    assert name in declared and hasattr(lib, name) and name in _lib.SYMBOLS
    assert len(_lib.SYMBOLS[name][1]) == 12
    for line in ("#define GPET_METRICS_B_ON_DEVICE 32u\n", "#define GPET_METRICS_MAPS_ON_DEVICE 64u\n", "#define GPET_ABI_VERSION 1\n"):
        assert line in header, line
    assert (_lib.RAW_ON_DEVICE, _lib.METRICS_B_ON_DEVICE, _lib.METRICS_MAPS_ON_DEVICE) == (4, 32, 64)
    assert hasattr(_lib.Context, "metrics_images")
    assert '#include "gpet_k_metrics.inc"' in open(os.path.join(CSRC, "gpet_kernels.hip")).read()
    assert "gpet_api_metrics.hip" in ge.HIP_SOURCES
    import gaussian_process_edge_trace_amd as pkg
    assert hasattr(pkg.gpet_utils, "denoise_metrics")
    import inspect
    assert "return_metrics" in inspect.signature(pkg.gpet_utils.denoise_imgs).parameters


def test_struct_layout_matches_the_header(tmp_path):
    from gaussian_process_edge_trace_amd import _lib
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpet_hip.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(gpet_metrics), offsetof(gpet_metrics, use_sample_covariance), '
                    'offsetof(gpet_metrics, K1), offsetof(gpet_metrics, K2), offsetof(gpet_metrics, data_range));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    G = _lib.GpetMetrics
    assert got == [C.sizeof(G), G.use_sample_covariance.offset, G.K1.offset, G.K2.offset, G.data_range.offset]


# ---- the header through a host-compiled shim -------------------------------------------------------------------------------------
SHIM = r"""
#include "gpet_metrics_plan.h"
#include <vector>
using namespace gpet;
static char g_msg[512];
extern "C" {
void shim_limits(long long* out) { out[0] = METRICS_THREADS; out[1] = METRICS_COLS; out[2] = METRICS_ROWS; out[3] = METRICS_TILE; out[4] = METRICS_SORT_SEG;
                                   out[5] = (long long)METRICS_CHUNK_BUDGET; out[6] = METRICS_PX_MAX; out[7] = (long long)sizeof(MetricsAcc); }
double shim_sum(const double* t, long long n) { return metrics_sum(t, n); }
void shim_line(const double* line, int len, int size, double* out) { metrics_line(line, len, size, out); }
int shim_reflect(int s, int len) { return metrics_reflect(s, len); }
int shim_work_f64(int pa, int pb) { return metrics_work_f64(pa, pb) ? 1 : 0; }
double shim_sqdiff(double a, double b, int f64) { return metrics_sqdiff(a, b, f64 != 0); }
double shim_span(double lo, double hi, int f64) { return metrics_span(lo, hi, f64 != 0); }
void shim_const(int w, int usc, double K1, double K2, double R, double* out) {
  const MetricsSsimConst k = metrics_ssim_const(w, usc, K1, K2, R);
  out[0] = k.cov_norm; out[1] = k.C1; out[2] = k.C2;
}
double shim_S(double ux, double uy, double uxx, double uyy, double uxy, double cn, double C1, double C2) { return metrics_ssim_S(ux, uy, uxx, uyy, uxy, cn, C1, C2); }
// the S map of an f64 pair as the kernels put it together: five planes, axis 0 then axis 1 of metrics_line, metrics_ssim_S
void shim_ssim_map(const double* a, const double* b, int M, int N, int w, int usc, double K1, double K2, double R, double* S) {
  const size_t px = (size_t)M * N;
  std::vector<double> in(5 * px), mid(5 * px), fin(5 * px);
  for (size_t i = 0; i < px; ++i) {
    const double x = a[i], y = b[i];
    in[i] = x; in[px + i] = y; in[2 * px + i] = x * x; in[3 * px + i] = y * y; in[4 * px + i] = x * y;
  }
  for (int p = 0; p < 5; ++p) {
    for (int c = 0; c < N; ++c) metrics_line(in.data() + p * px + c, M, w, mid.data() + p * px + c, N, N);
    for (int r = 0; r < M; ++r) metrics_line(mid.data() + p * px + (size_t)r * N, N, w, fin.data() + p * px + (size_t)r * N);
  }
  const MetricsSsimConst k = metrics_ssim_const(w, usc, K1, K2, R);
  for (size_t i = 0; i < px; ++i) S[i] = metrics_ssim_S(fin[i], fin[px + i], fin[2 * px + i], fin[3 * px + i], fin[4 * px + i], k.cov_norm, k.C1, k.C2);
}
void shim_keys(const double* v, long long n, unsigned long long* out) { for (long long i = 0; i < n; ++i) out[i] = metrics_key(v[i]); }
unsigned long long shim_key_pad() { return METRICS_KEY_PAD; }
void shim_entropy_terms(const unsigned long long* keys, long long n, double* e) { metrics_entropy_terms((const uint64_t*)keys, n, e); }
long long shim_run_end(const unsigned long long* keys, long long i, long long n) { return metrics_run_end((const uint64_t*)keys, i, n); }
long long shim_pow2(long long n) { return metrics_pow2(n); }
unsigned long long shim_frame_bytes(long long px, unsigned long long sa, unsigned long long sb) { return metrics_frame_bytes(px, sa, sb); }
void shim_chunks(int n_img, unsigned long long fb, int* out) { const StagePlan p = metrics_chunks(n_img, fb); out[0] = p.per_chunk; out[1] = p.n_chunks; }
const char* shim_figures(const double* acc5, int w, double data_range, int pa, int pb, int M, int N, double* out) {
  MetricsAcc a{acc5[0], acc5[1], acc5[2], acc5[3], acc5[4]};
  MetricsSpec sp;
  sp.win_size = w;
  sp.data_range = data_range;
  g_msg[0] = 0;
  return metrics_figures(a, sp, pa, pb, M, N, out, g_msg, sizeof g_msg) ? g_msg : nullptr;
}
const char* shim_check(int null_arg, int n_img, int pa, int pb, long long M, long long N, int w, double K1, double K2, double dr, int spec_null,
                       unsigned long long sa, unsigned long long sb) {
  MetricsSpec sp;
  sp.win_size = w; sp.K1 = K1; sp.K2 = K2; sp.data_range = dr;
  g_msg[0] = 0;
  return metrics_check(null_arg != 0, n_img, pa, pb, M, N, spec_null ? nullptr : &sp, sa, sb, g_msg, sizeof g_msg) ? g_msg : nullptr;
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("metrics_plan")
    src, so = d / "shim.cpp", d / "libmetrics_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    I, D, LL, ULL, P = C.c_int, C.c_double, C.c_longlong, C.c_ulonglong, C.c_void_p
    lib.shim_limits.argtypes = [P]
    lib.shim_sum.restype, lib.shim_sum.argtypes = D, [P, LL]
    lib.shim_line.restype, lib.shim_line.argtypes = None, [P, I, I, P]
    lib.shim_reflect.restype, lib.shim_reflect.argtypes = I, [I, I]
    lib.shim_work_f64.restype, lib.shim_work_f64.argtypes = I, [I, I]
    lib.shim_sqdiff.restype, lib.shim_sqdiff.argtypes = D, [D, D, I]
    lib.shim_span.restype, lib.shim_span.argtypes = D, [D, D, I]
    lib.shim_const.restype, lib.shim_const.argtypes = None, [I, I, D, D, D, P]
    lib.shim_S.restype, lib.shim_S.argtypes = D, [D] * 8
    lib.shim_ssim_map.restype, lib.shim_ssim_map.argtypes = None, [P, P, I, I, I, I, D, D, D, P]
    lib.shim_keys.restype, lib.shim_keys.argtypes = None, [P, LL, P]
    lib.shim_key_pad.restype = ULL
    lib.shim_entropy_terms.restype, lib.shim_entropy_terms.argtypes = None, [P, LL, P]
    lib.shim_run_end.restype, lib.shim_run_end.argtypes = LL, [P, LL, LL]
    lib.shim_pow2.restype, lib.shim_pow2.argtypes = LL, [LL]
    lib.shim_frame_bytes.restype, lib.shim_frame_bytes.argtypes = ULL, [LL, ULL, ULL]
    lib.shim_chunks.restype, lib.shim_chunks.argtypes = None, [I, ULL, P]
    lib.shim_figures.restype, lib.shim_figures.argtypes = C.c_char_p, [P, I, D, I, I, I, I, P]
    lib.shim_check.restype, lib.shim_check.argtypes = C.c_char_p, [I, I, I, I, LL, LL, I, D, D, D, I, ULL, ULL]
    return lib


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def test_constants_workspace_and_chunks(shim):
    from gaussian_process_edge_trace_amd import _lib
    lim = (C.c_longlong * 8)()
    shim.shim_limits(lim)
    assert list(lim) == [256, 64, 64, 8, 2048, 512 << 20, 1 << 26, 40]
    assert R.THREADS == 256 and _lib.METRICS_CHUNK_BUDGET == 512 << 20 and _lib.METRICS_PX_MAX == 1 << 26
    assert [shim.shim_pow2(n) for n in (1, 2, 3, 49, 2048, 2049, 250000)] == [1, 2, 4, 64, 2048, 4096, 262144]
    # six float64 planes, then the staged host frames, each to 256 bytes; the sort's keys fit the five planes they lie over
    for px, sa, sb in ((49, 49, 0), (250000, 250000 * 8, 250000), (9100, 0, 0)):
        want = ((48 * px + 255) & ~255) + ((sa + 255) & ~255) + ((sb + 255) & ~255)
        assert shim.shim_frame_bytes(px, sa, sb) == want == _lib.metrics_frame_bytes(px, sa, sb)
        assert shim.shim_pow2(px) * 8 <= 5 * px * 8
    out = (C.c_int * 2)()
    fb = shim.shim_frame_bytes(250000, 250000, 250000 * 8)
    shim.shim_chunks(256, fb, out)
    assert list(out) == [(512 << 20) // fb, -(-256 // ((512 << 20) // fb))]
    shim.shim_chunks(3, fb, out)
    assert list(out) == [3, 1]


def test_working_type_rule(shim):
    for pa, da in enumerate(DT):
        for pb, db in enumerate(DT):
            assert bool(shim.shim_work_f64(pa, pb)) == (R.work_type(da, db) is np.float64) == (np.result_type(da, db, np.float32) == np.float64)
    rng = np.random.default_rng(0)
    # u16 values whose squared differences exceed 2^24: the float32 square rounds, the float64 one does not
    a = rng.integers(0, 65536, 400).astype(np.uint16)
    b = rng.integers(0, 65536, 400).astype(np.uint16)
    want32, want64 = R.sq_diffs(a, b), R.sq_diffs(a.astype(np.float64), b.astype(np.float64))
    got32 = np.array([shim.shim_sqdiff(float(x), float(y), 0) for x, y in zip(a, b)])
    got64 = np.array([shim.shim_sqdiff(float(x), float(y), 1) for x, y in zip(a, b)])
    assert np.array_equal(got32, want32) and np.array_equal(got64, want64) and not np.array_equal(want32, want64)
    # float32 pairs: the difference itself rounds in float32
    a, b = rng.random(400).astype(np.float32), rng.random(400).astype(np.float32)
    assert np.array_equal(np.array([shim.shim_sqdiff(float(x), float(y), 0) for x, y in zip(a, b)]), R.sq_diffs(a, b))
    # a mixed pair works in float64
    assert np.array_equal(np.array([shim.shim_sqdiff(float(x), float(y), 1) for x, y in zip(a, b.astype(np.float64))]), R.sq_diffs(a, b.astype(np.float64)))
    lo, hi = np.float32(0.1), np.float32(0.7)
    assert shim.shim_span(float(lo), float(hi), 0) == float(hi - lo) != float(hi) - float(lo) == shim.shim_span(float(lo), float(hi), 1)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000, 9100])
def test_summation_order(shim, n):
    rng = np.random.default_rng(n)
    for t in (rng.random(n), rng.random(n) * 10.0 ** rng.integers(-8, 8, n), -rng.random(n)):
        t = f64(t)
        assert shim.shim_sum(t.ctypes.data, n) == R.metrics_sum(t)
    if n > 300:  # (the order is its own: not numpy's pairwise sum, not the serial one -- on most inputs)
        t = f64(rng.random(n) * 10.0 ** rng.integers(-8, 8, n))
        import math
        assert abs(R.metrics_sum(t) - math.fsum(t)) <= 2 * (n - 1) * R.U * math.fsum(t)


@pytest.mark.parametrize("n,size", [(7, 7), (7, 3), (9, 7), (53, 7), (53, 11), (130, 3), (12, 11)])
def test_recurrence_of_a_line(shim, n, size):
    rng = np.random.default_rng(n * 100 + size)
    line = f64(rng.random(n) * 255.0)
    out = np.empty(n)
    shim.shim_line(line.ctypes.data, n, size, out.ctypes.data)
    assert np.array_equal(out, R.uniform_filter1d(line, size, 0))
    h = size // 2
    assert [shim.shim_reflect(s, n) for s in range(-h, n + h)] == [R.reflect(s, n) for s in range(-h, n + h)]
    assert shim.shim_reflect(-1, n) == 0 and shim.shim_reflect(n, n) == n - 1 and shim.shim_reflect(-h, n) == h - 1


@pytest.mark.parametrize("M,N,w,usc,K1,K2,Rg", [(7, 7, 7, 1, 0.01, 0.03, 2.0), (37, 53, 7, 1, 0.01, 0.03, 255.0), (37, 53, 3, 0, 0.01, 0.03, 2.0),
                                                 (70, 130, 11, 1, 0.02, 0.05, 65535.0)])
def test_S_formula_and_the_map(shim, M, N, w, usc, K1, K2, Rg):
    rng = np.random.default_rng(M + N + w)
    a = f64(np.rint(rng.random((M, N)) * Rg / 2 * 1024) / 1024)
    b = f64(a + rng.normal(0, Rg / 40, (M, N)))
    k = (C.c_double * 3)()
    shim.shim_const(w, usc, K1, K2, Rg, k)
    assert tuple(k) == R.ssim_const(w, bool(usc), K1, K2, Rg)
    S = np.empty((M, N))
    shim.shim_ssim_map(a.ctypes.data, b.ctypes.data, M, N, w, usc, K1, K2, Rg, S.ctypes.data)
    want = R.ssim_map(a, b, w, Rg, K1, K2, bool(usc))
    assert np.array_equal(S, want)
    u = [f64(R.uniform_filter(p, w)) for p in (a, b, a * a, b * b, a * b)]
    got = np.array([shim.shim_S(*(float(p[r, c]) for p in u), *k) for r, c in ((0, 0), (M // 2, N // 3), (M - 1, N - 1))])
    assert np.array_equal(got, np.array([want[0, 0], want[M // 2, N // 3], want[M - 1, N - 1]]))


def test_keys_counts_and_entropy_terms(shim):
    rng = np.random.default_rng(5)
    v = f64(np.concatenate([rng.normal(0, 1, 300), [-0.0, 0.0, 0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324], np.rint(rng.normal(0, 3, 500))]))
    keys = np.empty(v.shape[0], dtype=np.uint64)
    shim.shim_keys(v.ctypes.data, v.shape[0], keys.ctypes.data)
    assert np.array_equal(keys, R.keys_of(v)) and keys.max() < shim.shim_key_pad() == 2 ** 64 - 1
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(v[order], np.sort(v))  # (the keys order as the values do; the two zeros are one key)
    assert keys[300] == keys[301]
    ks = np.ascontiguousarray(keys[order])
    starts, counts = R.run_counts(ks)
    assert np.array_equal(counts, np.unique(v, return_counts=True)[1])
    assert [shim.shim_run_end(ks.ctypes.data, int(s), ks.shape[0]) for s in starts] == (starts + counts).tolist()
    e = np.empty(v.shape[0])
    shim.shim_entropy_terms(ks.ctypes.data, ks.shape[0], e.ctypes.data)
    want, wc = R.entropy_terms(v)
    assert np.array_equal(e, want) and np.array_equal(wc, counts)
    assert shim.shim_sum(e.ctypes.data, e.shape[0]) == R.metrics_sum(want)


def test_figures_from_the_sums(shim):
    """metrics_figures on the restatement's sums gives the restatement's figures (the host's log10 and sqrt against numpy's: equal on
    these inputs, and never more than a unit in the last place apart)."""
    from tests.denoise_ref import make_frame
    for pa, pb, seed in ((0, 0, 1), (1, 1, 2), (2, 2, 3), (3, 3, 4), (0, 3, 5), (2, 3, 6)):
        a = make_frame(seed, 20, 31, 0.1, DT[pa], levels=1024)
        b = make_frame(seed, 20, 31, 0.05, DT[pb], levels=64)
        m = R.figures(a, b)
        pad, e = 3, R.entropy_terms(b)[0]
        acc = f64([R.metrics_sum(R.sq_diffs(a, b)), float(a.min()), float(a.max()), R.metrics_sum(m["ssim_map"][pad:-pad, pad:-pad]), R.metrics_sum(e)])
        out = np.empty(4)
        assert shim.shim_figures(acc.ctypes.data, 7, 0.0, pa, pb, 20, 31, out.ctypes.data) is None
        want = np.array([m["psnr"], m["ssim"], m["nrmse"], m["entropy"]])
        assert np.array_equal(out[1:], want[1:]) and abs(out[0] - want[0]) <= np.spacing(want[0])
    # the range rule of PSNR: floats below 0 give 2, beyond [-1, 1] the library's refusal; an explicit range lifts it
    acc = f64([1.0, -0.5, 0.5, 0.0, 0.0])
    out = np.empty(4)
    assert shim.shim_figures(acc.ctypes.data, 7, 0.0, 3, 3, 10, 10, out.ctypes.data) is None and out[0] == 10.0 * np.log10(4.0 / 0.01)
    acc[2] = 1.5
    assert shim.shim_figures(acc.ctypes.data, 7, 0.0, 3, 3, 10, 10, out.ctypes.data).decode() == R.RANGE_WORDS
    assert shim.shim_figures(acc.ctypes.data, 7, 3.0, 3, 3, 10, 10, out.ctypes.data) is None and out[0] == 10.0 * np.log10(9.0 / 0.01)
    acc[0] = 0.0  # (an identical pair: what IEEE division gives)
    assert shim.shim_figures(acc.ctypes.data, 7, 3.0, 3, 3, 10, 10, out.ctypes.data) is None and out[0] == np.inf and out[2] == 0.0


REFUSALS = [
    (dict(null_arg=1), "metrics: a null pointer"),
    (dict(spec_null=1), "metrics: a null pointer"),
    (dict(n_img=0), "metrics: no frame"),
    (dict(pa=4), "metrics: unknown pixel type"),
    (dict(pb=-1), "metrics: unknown pixel type"),
    (dict(M=0), "metrics: empty frame"),
    (dict(M=6), R.EXTENT_WORDS),
    (dict(N=5, w=9), R.EXTENT_WORDS),
    (dict(w=4), R.ODD_WORDS),
    (dict(w=1), "metrics: win_size must be at least 3"),
    (dict(K1=-0.01), "K1 must be positive"),
    (dict(K2=-1.0), "K2 must be positive"),
    (dict(dr=-1.0), "metrics: data_range must be a finite number above 0 (0: the library's rule)"),
    (dict(dr=float("inf")), "metrics: data_range must be a finite number above 0 (0: the library's rule)"),
    (dict(M=1 << 14, N=(1 << 12) + 1), "metrics: a frame exceeds 2^26 pixels (M * N)"),
    (dict(M=4096, N=4096), "metrics: the workspace of one frame (805306368 bytes: six float64 planes of 4096 x 4096 and its staging) exceeds the chunk "
                           "budget of 536870912 bytes"),
]


@pytest.mark.parametrize("change,words", REFUSALS)
def test_words_of_the_refusals(shim, change, words):
    from gaussian_process_edge_trace_amd import _lib
    arg = dict(null_arg=0, n_img=2, pa=0, pb=3, M=37, N=53, w=7, K1=0.01, K2=0.03, dr=0.0, spec_null=0, sa=0, sb=0)
    assert shim.shim_check(*arg.values()) is None
    assert _lib.metrics_refusal(arg["n_img"], arg["pa"], arg["pb"], arg["M"], arg["N"], arg["w"], arg["K1"], arg["K2"], arg["dr"]) is None
    arg.update(change)
    assert shim.shim_check(*arg.values()).decode() == words
    if not (arg["null_arg"] or arg["spec_null"]):  # (the binding always passes its pointers)
        assert _lib.metrics_refusal(arg["n_img"], arg["pa"], arg["pb"], arg["M"], arg["N"], arg["w"], arg["K1"], arg["K2"], arg["dr"]) == words
    assert R.RANGE_WORDS == _lib.METRICS_RANGE_WORDS


def test_keywords_the_device_does_not_build_are_refused_by_name():
    from gaussian_process_edge_trace_amd import _lib
    for key in ("gaussian_weights", "gradient", "multichannel"):
        with pytest.raises(ValueError, match=key):
            _lib.metrics_spec(7, None, **{key: True})
        assert _lib.metrics_spec(7, None, **{key: False}).win_size == 7
    with pytest.raises(ValueError, match="sigma"):
        _lib.metrics_spec(7, None, sigma=1.5)
    s = _lib.metrics_spec(None, 2.5, K1=0.02, use_sample_covariance=False)
    assert (s.win_size, s.use_sample_covariance, s.K1, s.K2, s.data_range) == (7, 0, 0.02, 0.03, 2.5)
    assert _lib.metrics_spec().data_range == 0.0
