"""CPU tests of the launch rules of one loop iteration (csrc/gpet_iter_plan.h): the header needs no HIP, so a small extern "C" shim
around it is compiled with the host C++ compiler and driven through ctypes.  Every expectation below is a literal, derived by hand
from the rules as the launchers (csrc/gpet_k_launch.inc) had them before they moved into the header:

  K extent     ks = ceil(rank / 4) raised to the next of 8, 12, 16, 18, 20, 24; MT of k_struct_rows 2, 3, 4, 5, 5, 6
  sample GEMM  register form iff both capacities <= 96 (f32mma: and 4 * 24 * 80 * 4 + (Lg + 64) * 8 <= 150 KB); rank = rank_max if
               0 < rank_max <= r_cap else max(r_cap, a_rows_cap); rparts = ceil(S / 128); ncs = ceil(256 / (B * rparts)) clamped to
               [1, min(ceil(Lg / 64), 8)]; f64 LDS = (4 * ks * 80 + (Lg + 64 if the mean fits behind a KS 24 chunk)) * 8
  scorer       tiled iff 32 * (M | 1) * 4 <= 150 KB and S >= 64; tiles = ceil(((Lg - 2) // 2) / 15); curves per workgroup 1024, halved
               down to 128 while B * tiles * ceil(S / cpw) < 256
  fit          in LDS iff n_cap <= 128, (n_cap * (n_cap | 1) + n_cap) * 8 bytes; prediction 536 * n_cap bytes of LDS while that fits

The shapes of the GPU tests that restate one of these rules to name the kernel they reach (tests/test_gpu_sample_gemm_exact.py,
tests/test_gpu_score_injected.py) are held against the header here as well."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from tests import curve_cost_exact as cx
from tests import posterior_exact as px
from tests.test_gpu_sample_gemm_exact import CASES as GEMM_CASES

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussian_process_edge_trace_amd", "csrc")

DIMS = ("M", "N", "Lg", "S", "n_keep", "z_cols", "r_cap", "n_cap", "n_bins", "obs_cap", "z_ring", "a_rows_cap", "r0_max", "jlog", "y_f32",
        "rng4", "lg_even", "y_arith")
SHIM = r"""
#include "gpet_iter_plan.h"
using namespace gpet;
static_assert(sizeof(BatchDims) == 18 * sizeof(int), "BatchDims is eighteen ints");
static const BatchDims& dims(const int* d) { return *reinterpret_cast<const BatchDims*>(d); }
static void put(int* o, const Grid3& g) { o[0] = g.x; o[1] = g.y; o[2] = g.z; }
extern "C" {
int shim_const(int i) {
  const int v[] = {LDS_DYN_MAX, GEMM_LDS_MAX, STRUCT_H_LDS_MAX, GEMM_KMAX, GEMM_LDA, GEMM32_LDA, SC_PAIRS, SC_CURVES, SC_THREADS,
                   KDE_TX, KDE_H, KDE_NB, KDE_THREADS, KDE_PREP_MAXB, PIX_CX, SR_TJ, CB};
  return v[i];
}
void shim_k_extent(int rank, int* o) { const KExtent k = k_extent(rank); o[0] = k.ks; o[1] = k.mt; }
// o = {reg, ks, rl, y_f32, mu_in_lds, rparts, ncs, grid x y z, block}
long long shim_sample(const int* d, int B, int rank_max, int f32mma, int* o) {
  const SamplePlan p = sample_plan(dims(d), B, rank_max, f32mma != 0);
  o[0] = p.reg; o[1] = p.ks; o[2] = p.rl; o[3] = p.y_f32; o[4] = p.mu_in_lds; o[5] = p.rparts; o[6] = p.ncs; put(o + 7, p.grid); o[10] = p.block;
  return (long long)p.lds;
}
// o = {tiled, n_tiles, cpw, tile grid x y z, combine grid x y z, wave grid x y z}
long long shim_score(const int* d, int B, int S, int* o) {
  const ScorePlan p = score_plan(dims(d), B, S);
  o[0] = p.tiled; o[1] = p.n_tiles; o[2] = p.cpw; put(o + 3, p.tile_grid); put(o + 6, p.combine_grid); put(o + 9, p.wave_grid);
  return (long long)p.lds;
}
int shim_score_tiles(int Lg) { return score_tiles(Lg); }
int shim_topk_bitonic(const int* d, int topk_rank) { return topk_bitonic(dims(d), topk_rank); }
int shim_tail(const int* d, int topk_rank) { return score_tail_applies(dims(d), topk_rank); }
long long shim_kde(const int* d, int B, int* o) { const KdeFusedPlan p = kde_fused_plan(dims(d), B); put(o, p.grid); return (long long)p.lds; }
void shim_pixels(const int* d, int B, int* o) {
  const PixelPlan p = pixel_plan(dims(d), B);
  put(o, p.columns); put(o + 3, p.old); put(o + 6, p.argbest); put(o + 9, p.select);
}
long long shim_fit(const int* d, int* o) { const FitPlan p = fit_plan(dims(d)); o[0] = p.in_lds; return (long long)p.lds; }
const char* shim_predict(const int* d, int final_fit, long long* lds) {
  const PredictPlan p = predict_plan(dims(d), final_fit != 0);
  *lds = (long long)p.lds;
  return p.form == PredictForm::lds ? "lds" : p.form == PredictForm::global ? "global" : "through_hbm";
}
long long shim_struct_h(const int* d, int* o) { const StructHPlan p = struct_h_plan(dims(d)); o[0] = p.l_in_lds; return (long long)p.lds; }
long long shim_struct_rows(const int* d, int B, int* o) {
  const StructRowsPlan p = struct_rows_plan(dims(d), B);
  o[0] = p.mt; o[1] = p.ks; put(o + 2, p.grid);
  return (long long)p.lds;
}
}
"""


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = cxx and shutil.which(cxx)
        if path:
            return path
    return None


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("iter_plan")
    src, so = d / "shim.cpp", d / "libiter_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    for name in ("shim_sample", "shim_score", "shim_kde", "shim_fit", "shim_struct_h", "shim_struct_rows"):
        getattr(lib, name).restype = C.c_longlong
    lib.shim_predict.restype = C.c_char_p
    return lib


def dims(**kw):
    assert set(kw) <= set(DIMS)
    return (C.c_int * len(DIMS))(*[kw.get(k, 0) for k in DIMS])


def sample(shim, B=1, rank_max=0, f32mma=False, **kw):
    o = (C.c_int * 11)()
    lds = shim.shim_sample(dims(**kw), B, rank_max, int(f32mma), o)
    return dict(reg=bool(o[0]), ks=o[1], rl=bool(o[2]), y_f32=bool(o[3]), mu_in_lds=bool(o[4]), rparts=o[5], ncs=o[6], grid=tuple(o[7:10]),
                block=o[10], lds=lds)


def score(shim, B, rows, **kw):
    """score_plan for the first `rows` sample rows of every edge of a batch of dimensions kw."""
    o = (C.c_int * 12)()
    lds = shim.shim_score(dims(**kw), B, rows, o)
    return dict(tiled=bool(o[0]), n_tiles=o[1], cpw=o[2], tile_grid=tuple(o[3:6]), combine_grid=tuple(o[6:9]), wave_grid=tuple(o[9:12]), lds=lds)


def test_constants(shim):
    want = [153600, 153600, 153600, 96, 80, 80, 15, 1024, 1024, 16, 128, 128, 512, 1024, 32, 64, 64]
    assert [shim.shim_const(i) for i in range(len(want))] == want


@pytest.mark.parametrize("rank,ks,mt", [(0, 8, 2), (1, 8, 2), (32, 8, 2), (33, 12, 3), (48, 12, 3), (49, 16, 4), (64, 16, 4), (65, 18, 5),
                                        (72, 18, 5), (73, 20, 5), (80, 20, 5), (81, 24, 6), (96, 24, 6), (200, 24, 6)])
def test_k_extent(shim, rank, ks, mt):
    o = (C.c_int * 2)()
    shim.shim_k_extent(rank, o)
    assert (o[0], o[1]) == (ks, mt)


# ---- sample GEMM ----

def test_sample_f64_register_form(shim):
    p = sample(shim, S=129, Lg=577, r_cap=32, a_rows_cap=32)
    assert (p["reg"], p["ks"], p["rl"], p["rparts"], p["ncs"], p["grid"], p["block"]) == (True, 8, False, 2, 8, (16, 1, 1), 512)
    assert p["mu_in_lds"] and not p["y_f32"] and p["lds"] == 25608     # (4 * 8 * 80 + 577 + 64) * 8
    p = sample(shim, S=129, Lg=64, r_cap=32, a_rows_cap=32)
    assert (p["ncs"], p["grid"], p["lds"]) == (1, (2, 1, 1), 21504)     # one column tile; (2560 + 128) * 8
    # the row blocks alone fill the GPU: one column run however wide the edge; never fewer than one
    assert sample(shim, B=128, S=129, Lg=577, r_cap=32, a_rows_cap=32)["ncs"] == 1
    assert sample(shim, B=1024, S=1000, Lg=500, r_cap=96, a_rows_cap=96)["grid"] == (8, 1024, 1)
    p = sample(shim, B=16, S=1000, Lg=500, r_cap=96, a_rows_cap=96)     # ceil(256 / (16 * 8)) = 2 runs
    assert (p["rparts"], p["ncs"], p["grid"]) == (8, 2, (16, 16, 1))
    p = sample(shim, S=129, Lg=577, r_cap=32, a_rows_cap=32, y_f32=1)
    assert p["y_f32"] and p["lds"] == 25608


@pytest.mark.parametrize("rank_max,r_cap,ks,rl,lds", [(72, 96, 18, False, 51208), (73, 96, 20, True, 56328), (81, 96, 24, True, 66568),
                                                      (97, 96, 24, True, 66568), (5, 96, 8, False, 25608), (0, 96, 24, True, 66568),
                                                      (33, 32, 8, False, 25608), (0, 64, 16, False, 46088)])
def test_sample_rank_of_a_launch(shim, rank_max, r_cap, ks, rl, lds):
    """rank_max counts when it lies in 1 .. r_cap; else the larger capacity does."""
    p = sample(shim, rank_max=rank_max, S=129, Lg=577, r_cap=r_cap, a_rows_cap=r_cap)
    assert (p["reg"], p["ks"], p["rl"], p["lds"]) == (True, ks, rl, lds)   # (4 * ks * 80 + 641) * 8


def test_sample_generic_form(shim):
    for caps in ((97, 96), (96, 97), (577, 577)):
        p = sample(shim, B=3, S=129, Lg=577, r_cap=caps[0], a_rows_cap=caps[1])
        assert (p["reg"], p["grid"], p["block"], p["lds"]) == (False, (10, 3, 3), 256, 0)
    # a row capacity above the factor capacity decides the extent (z_cols == Lg: full-width rows)
    assert sample(shim, S=129, Lg=64, r_cap=32, a_rows_cap=64)["ks"] == 16


def test_sample_f64_mean_in_lds_up_to_11456_columns(shim):
    p = sample(shim, S=129, Lg=11456, r_cap=32, a_rows_cap=32)
    assert p["mu_in_lds"] and p["lds"] == (2560 + 11520) * 8
    p = sample(shim, S=129, Lg=11457, r_cap=32, a_rows_cap=32)
    assert p["reg"] and not p["mu_in_lds"] and p["lds"] == 20480     # the chunk alone
    assert p["ncs"] == 8 and p["grid"] == (16, 1, 1)


def test_sample_f32mma(shim):
    p = sample(shim, f32mma=True, S=129, Lg=577, r_cap=32, a_rows_cap=32, y_f32=1, y_arith=1)
    assert (p["reg"], p["ks"], p["rl"], p["mu_in_lds"], p["ncs"], p["grid"], p["block"]) == (True, 8, False, True, 8, (16, 1, 1), 512)
    assert p["lds"] == 15368     # 4 * 8 * 80 * 4 + (577 + 64) * 8
    p = sample(shim, f32mma=True, rank_max=73, S=129, Lg=577, r_cap=96, a_rows_cap=96)
    assert (p["ks"], p["rl"], p["lds"]) == (20, False, 30728)     # one kernel per extent: no _rl; 25600 + 5128
    p = sample(shim, f32mma=True, S=129, Lg=15296, r_cap=96, a_rows_cap=96)
    assert p["reg"] and p["ks"] == 24 and p["lds"] == 153600     # 30720 + 15360 * 8: the limit itself
    p = sample(shim, f32mma=True, B=2, S=129, Lg=15297, r_cap=96, a_rows_cap=96)
    assert (p["reg"], p["grid"], p["block"], p["lds"]) == (False, (240, 3, 2), 256, 0)
    assert not sample(shim, f32mma=True, S=129, Lg=577, r_cap=97, a_rows_cap=96)["reg"]


GEMM_KERNEL = {"r8": (8, False), "r12": (12, False), "r16": (16, False), "r18": (18, False), "rl20": (20, True), "rl24": (24, True)}


@pytest.mark.parametrize("case", list(GEMM_CASES))
def test_sample_plan_names_the_kernel_the_gemm_tests_expect(shim, case):
    spans, S, _, _, caps, kernel, _ = GEMM_CASES[case]
    for f32mma in (False, True):
        p = sample(shim, B=len(spans), f32mma=f32mma, S=S, Lg=max(lg for _, lg in spans), r_cap=caps[0], a_rows_cap=caps[1])
        if kernel == "generic":
            assert not p["reg"]
        else:
            ks, rl = GEMM_KERNEL[kernel]
            assert (p["reg"], p["ks"], p["rl"]) == (True, ks, rl and not f32mma)
    # "the register form's trip over more than one 64-column tile per workgroup runs in ks8_column_runs alone"
    p = sample(shim, B=len(spans), S=S, Lg=max(lg for _, lg in spans), r_cap=caps[0], a_rows_cap=caps[1])
    if p["reg"]:
        tiles = -(-max(lg for _, lg in spans) // 64)
        assert (tiles > p["ncs"]) == (case == "ks8_column_runs")


# ---- scorer, top-k, tail ----

@pytest.mark.parametrize("Lg,n", [(4, 1), (5, 1), (32, 1), (33, 1), (34, 2), (80, 3), (500, 17)])
def test_score_tiles(shim, Lg, n):
    assert shim.shim_score_tiles(Lg) == n
    assert score(shim, 1, 64, M=12, Lg=Lg, S=64)["n_tiles"] == n


def test_score_curves_per_workgroup(shim):
    p = score(shim, 1, 1000, M=500, Lg=500, S=1000)
    assert (p["tiled"], p["n_tiles"], p["cpw"], p["tile_grid"], p["combine_grid"]) == (True, 17, 128, (17, 8, 1), (4, 1, 1))
    assert p["lds"] == 64128     # 32 columns of 501 floats
    p = score(shim, 8, 1000, M=500, Lg=500, S=1000)
    assert (p["cpw"], p["tile_grid"], p["combine_grid"]) == (512, (17, 2, 8), (4, 8, 1))     # 8 * 17 * 2 = 272 workgroups
    p = score(shim, 16, 1000, M=500, Lg=500, S=1000)
    assert (p["cpw"], p["tile_grid"]) == (1024, (17, 1, 16))
    # the one-row views of the final costs: the batch's shape decides the variant, the rows scored the grid
    p = score(shim, 4, 1, M=500, Lg=500, S=1000)
    assert (p["tiled"], p["cpw"], p["tile_grid"], p["combine_grid"]) == (True, 128, (17, 1, 4), (1, 4, 1))


def test_score_variant(shim):
    assert score(shim, 1, 64, M=1199, Lg=40, S=64)["tiled"] and score(shim, 1, 64, M=1199, Lg=40, S=64)["lds"] == 153472
    assert score(shim, 1, 64, M=1198, Lg=40, S=64)["lds"] == 153472     # M | 1
    p = score(shim, 2, 64, M=1200, Lg=40, S=64)
    assert (p["tiled"], p["wave_grid"], p["lds"]) == (False, (16, 2, 1), 0)
    p = score(shim, 2, 63, M=12, Lg=40, S=63)
    assert (p["tiled"], p["wave_grid"]) == (False, (16, 2, 1))
    assert not score(shim, 3, 1, M=12, Lg=40, S=63)["tiled"] and score(shim, 3, 1, M=12, Lg=40, S=63)["wave_grid"] == (1, 3, 1)


def test_score_plan_on_the_shapes_of_the_scorer_tests(shim):
    """tests/test_gpu_score_injected.py: 26 edges of the first shape at S = 1100 keep 256 curves per workgroup; a case alone and
    the batch of three edges have the 128 of one pass; S = 40 takes the wave-per-curve form."""
    rows, _, _, Lg = cx.SHAPES[0]
    p = score(shim, 26, 1100, M=rows, Lg=Lg, S=1100)
    assert (p["cpw"], p["tile_grid"]) == (256, (2, 5, 26))
    for (rows, _, _, Lg), S, _ in cx.CASES:
        p = score(shim, 1, S, M=rows, Lg=Lg, S=S)
        assert (p["tiled"], p["cpw"]) == ((True, 128) if S >= 64 else (False, 0)), (Lg, S)
    p = score(shim, len(cx.BATCH_SPANS), cx.BATCH_S, M=33, Lg=max(lg for _, lg in cx.BATCH_SPANS), S=cx.BATCH_S)
    assert (p["cpw"], p["tile_grid"]) == (128, (3, 1, 3))


def test_topk_and_fused_tail(shim):
    def tail(topk_rank=0, **kw):
        return bool(shim.shim_tail(dims(**dict(dict(M=500, Lg=500, S=1000, n_keep=100), **kw)), topk_rank))
    assert tail() and tail(S=64, n_keep=64) and tail(S=1024) and tail(S=1024, n_keep=1024) and tail(M=1199)
    assert not tail(S=63, n_keep=63) and not tail(S=1025) and not tail(n_keep=1025) and not tail(topk_rank=1) and not tail(M=1200)
    assert shim.shim_topk_bitonic(dims(S=1024), 0) == 1 and shim.shim_topk_bitonic(dims(S=1025), 0) == 0
    assert shim.shim_topk_bitonic(dims(S=40), 0) == 1 and shim.shim_topk_bitonic(dims(S=1024), 1) == 0


# ---- KDE, pixels ----

def test_kde_fused_and_pixel_grids(shim):
    o = (C.c_int * 3)()
    assert shim.shim_kde(dims(N=500), 7, o) == 51904 and tuple(o) == (32, 7, 1)     # (24 * 137 + 128 * 24 + 128) * 8
    assert shim.shim_kde(dims(N=512), 1, o) == 51904 and tuple(o) == (32, 1, 1)
    assert shim.shim_kde(dims(N=513), 1, o) == 51904 and tuple(o) == (33, 1, 1)
    o = (C.c_int * 12)()
    shim.shim_pixels(dims(N=500, obs_cap=64), 5, o)
    assert tuple(o) == (16, 5, 1, 1, 5, 1, 2, 5, 1, 1, 5, 1)     # columns, old, argbest, select
    shim.shim_pixels(dims(N=500, obs_cap=600), 1, o)
    assert tuple(o) == (16, 1, 1, 3, 1, 1, 3, 1, 1, 1, 1, 1)
    shim.shim_pixels(dims(N=513, obs_cap=257), 1, o)
    assert tuple(o) == (17, 1, 1, 2, 1, 1, 3, 1, 1, 1, 1, 1)


# ---- fit, predict ----

def test_fit_and_predict(shim):
    o = (C.c_int * 1)()
    assert shim.shim_fit(dims(n_cap=128), o) == 133120 and o[0] == 1     # (128 * 129 + 128) * 8
    assert shim.shim_fit(dims(n_cap=45), o) == 16560 and o[0] == 1       # (45 * 45 + 45) * 8
    assert shim.shim_fit(dims(n_cap=129), o) == 0 and o[0] == 0
    lds = C.c_longlong()
    for final in (0, 1):
        assert shim.shim_predict(dims(n_cap=286), final, C.byref(lds)) == b"lds" and lds.value == 153296     # 536 * 286
        assert shim.shim_predict(dims(n_cap=45), final, C.byref(lds)) == b"lds" and lds.value == 24120
    assert shim.shim_predict(dims(n_cap=287), 0, C.byref(lds)) == b"through_hbm" and lds.value == 0
    assert shim.shim_predict(dims(n_cap=287), 1, C.byref(lds)) == b"global" and lds.value == 0


def test_posterior_table_capacities_reach_the_forms_they_name(shim):
    """The capacities of tests/posterior_exact.py's table, by regime, against the header: K in LDS / blocked, V in LDS / through
    HBM (loop) / global (converged fit) -- and both neighbours of each threshold are in the table."""
    o = (C.c_int * 1)()
    lds = C.c_longlong()
    want = {"lds": (1, b"lds", b"lds"), "blocked": (0, b"lds", b"lds"), "hbm": (0, b"through_hbm", b"global")}
    for regime, (caps, _) in px.REGIMES.items():
        for n_cap in caps:
            shim.shim_fit(dims(n_cap=n_cap), o)
            got = (o[0], shim.shim_predict(dims(n_cap=n_cap), 0, C.byref(lds)), shim.shim_predict(dims(n_cap=n_cap), 1, C.byref(lds)))
            assert got == want[regime] and px.regime_of(n_cap) == regime, (regime, n_cap, got)
    assert {128, 129, 286, 287} <= set(px.ALL_CAPS)


# ---- structured path ----

def test_struct_h(shim):
    o = (C.c_int * 1)()
    assert shim.shim_struct_h(dims(n_cap=100, r0_max=40, r_cap=96), o) == 73968 and o[0] == 1     # (100 * 41 + 5050 + 96) * 8
    assert shim.shim_struct_h(dims(n_cap=128, r0_max=96, r_cap=96), o) == 101120 and o[0] == 0    # L streamed: (128 * 97 + 128 + 96) * 8
    assert shim.shim_struct_h(dims(n_cap=118, r0_max=96, r_cap=96), o) == 148504 and o[0] == 1    # (118 * 97 + 7021 + 96) * 8
    assert shim.shim_struct_h(dims(n_cap=121, r0_max=96, r_cap=96), o) == 95632 and o[0] == 0     # full: 153712 > 153600


@pytest.mark.parametrize("r0_max,mt,ks,lds", [(0, 2, 8, 8704), (32, 2, 8, 8704), (33, 3, 12, 19200), (48, 3, 12, 19200), (49, 4, 16, 33792),
                                              (64, 4, 16, 33792), (65, 5, 18, 47296), (72, 5, 18, 47296), (73, 5, 20, 52480),
                                              (80, 5, 20, 52480), (81, 6, 24, 75264), (96, 6, 24, 75264)])
def test_struct_rows(shim, r0_max, mt, ks, lds):
    o = (C.c_int * 5)()
    assert shim.shim_struct_rows(dims(Lg=500, r0_max=r0_max), 9, o) == lds     # (4 * ks * (16 * mt + 1) + 16 * mt) * 8
    assert tuple(o) == (mt, ks, 8, 9, 1)
