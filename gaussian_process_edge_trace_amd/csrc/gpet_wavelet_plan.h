// What the wavelet stage (a0: gpet_wavelet_images) decides before anything is launched, as plain data: the spec and its
// validation, the filters, the level rule, every level's shapes and workspace offsets, tiles, grids and LDS bytes, and the one
// summation order the stage defines for itself.  No HIP, so the host compiler alone builds it (tests/test_wavelet_plan.py).
// The reference: gpet_utils.denoise 'wavelet' (gpet_utils.py:137-138) = scikit-image 0.18.3's denoise_wavelet on PyWavelets 1.1.1
// for a 2-D single-channel frame and an orthogonal wavelet.
//
// The arithmetic (all f64, no fused multiply-add, IEEE division and square root; sums start from +0.0 and add term by term).
// Input: f64 as it is, f32 widened, u8 / u16 times 1/255 / 1/65535 (their output is clipped to [0, 1] at the end).
// Filters: dec_lo has F taps (F even, 2..16); dec_hi[k] = (-1)^(k+1) dec_lo[F-1-k], rec_lo[k] = dec_lo[F-1-k],
// rec_hi[k] = (-1)^k dec_lo[k].
// Forward level (symmetric extension), axis 0 first, then axis 1; bands aa, ad, da, dd, first letter axis 0.  Along a line
// x[0..n-1], output o of (n + F - 1) / 2 is taken at i = 2 o + 1: for i < n the taps j = 0..F-1 ascending over xe[i - j],
// xe[k] = x[-k-1] for k < 0; for i >= n first j = i-n, i-n-1, .., 0 (the overhang, walking back from the edge: xe[k] = x[2n-1-k]),
// then j = i-n+1..F-1 (wv_fwd_tap).
// Noise: sigma = median(|dd1| over its non-zero entries) / ppf unless given; var = sigma sigma.
// Thresholds: BayesShrink per level and detail band t = var / sqrt(max(mean(x x) - var, 2^-52)), the mean in the order of
// wv_mean_squares below; VisuShrink t = sigma c for every band.
// Shrink: soft x max(1 - t / |x|, 0), hard |x| < t ? 0 : x.
// Inverse level, coarsest first, axis 1 first, then axis 0, the approximation cropped to the detail bands' shape: along a line with
// a, d of length n', for q = 0..n'-F/2 and parity p: s1 = sum_j rec_lo[2j+p] a[q+F/2-1-j], s2 = sum_j rec_hi[2j+p] d[q+F/2-1-j],
// j = 0..F/2-1 ascending, out[2q+p] = (0.0 + s1) + s2.  The last level is cropped to M x N.
#pragma once
#include <math.h>
#include <stddef.h>

#include "gpet_batch_plan.h"  // LDS_DYN_MAX
#include "gpet_conv_plan.h"   // pixel types, CONV_LDS_MAX, staging

#if defined(__HIPCC__)
#define GPET_WV_HD __host__ __device__
#else
#define GPET_WV_HD
#endif
// (no fused multiply-add in the functions the kernels share with the host, whatever the compiler's default)
#if defined(__clang__)
#define GPET_WV_NO_FMA _Pragma("clang fp contract(off)")
#else
#define GPET_WV_NO_FMA
#endif

namespace gpet {

// ---- the spec (include/gpet_hip.h: gpet_wavelet) --------------------------------------------------------------------------------
constexpr int WV_TAPS_MAX = 16;
constexpr int WV_LEVELS_MAX = 16;
enum { WV_SOFT = 0, WV_HARD = 1, WV_MODE_COUNT = 2 };
enum { WV_BAYES = 0, WV_VISU = 1, WV_METHOD_COUNT = 2 };
constexpr double WV_EPS = 2.220446049250313e-16;  // 2^-52
struct WvSpec {
  int n_taps = 0;                // F
  double dec_lo[WV_TAPS_MAX] = {};
  int levels = 0;                // 0: max(max_level - 3, 1)
  int mode = WV_SOFT, method = WV_BAYES;
  double sigma = NAN;            // NaN: estimated from dd1
  int rescale_sigma = 1;         // a given sigma of a u8 / u16 frame follows the frame's rescaling
  double ppf = 0.6744897501960817, c = 0.0;
  const double* thresholds = nullptr;  // host, [n_img * levels * 3] or null: used instead of the derived ones
  int n_thresholds = 0;
};
// the four filters as the kernels take them (by value)
struct WvFilters {
  double dec_lo[WV_TAPS_MAX], dec_hi[WV_TAPS_MAX], rec_lo[WV_TAPS_MAX], rec_hi[WV_TAPS_MAX];
};
inline WvFilters wv_filters(const double* dec_lo, int F) {
  WvFilters f = {};
  for (int k = 0; k < F; ++k) {
    f.dec_lo[k] = dec_lo[k];
    f.dec_hi[k] = ((k + 1) % 2 ? -1.0 : 1.0) * dec_lo[F - 1 - k];
    f.rec_lo[k] = dec_lo[F - 1 - k];
    f.rec_hi[k] = (k % 2 ? -1.0 : 1.0) * dec_lo[k];
  }
  return f;
}

// ---- levels ---------------------------------------------------------------------------------------------------------------------
// the largest L with (F - 1) 2^L <= n; 0 if there is none
inline int wv_max_level(int n, int F) {
  int L = 0;
  while (((long long)(F - 1) << (L + 1)) <= (long long)n) ++L;
  return L;
}
inline int wv_default_levels(int max_level) { return max_level - 3 > 1 ? max_level - 3 : 1; }
GPET_WV_HD inline int wv_out_len(int n, int F) { return (n + F - 1) / 2; }
// A level's input is m x n, its four bands mo x no each, one after the other (aa, ad, da, dd) from `off` doubles into the frame's
// workspace.  aa of level l is the input of level l + 1; on the way back it receives the reconstruction of level l + 1, cropped
// to its shape, so the workspace of a frame is the pyramid and nothing else: about 4/3 of the frame.
struct WvLevel {
  int m, n, mo, no;
  size_t off;
};
struct WvPlan {
  int F, levels;
  size_t frame_doubles;
  WvLevel lv[WV_LEVELS_MAX];
};
inline WvPlan wv_plan(int M, int N, int F, int levels) {
  WvPlan p = {};
  p.F = F;
  p.levels = levels;
  int m = M, n = N;
  for (int l = 0; l < levels && l < WV_LEVELS_MAX; ++l) {
    WvLevel& v = p.lv[l];
    v.m = m;
    v.n = n;
    v.mo = wv_out_len(m, F);
    v.no = wv_out_len(n, F);
    v.off = p.frame_doubles;
    p.frame_doubles += 4 * (size_t)v.mo * v.no;
    m = v.mo;
    n = v.no;
  }
  return p;
}

// ---- boundary and tap order -------------------------------------------------------------------------------------------------------
// position k of a line of length n under the symmetric extension (d c b a | a b c d | d c b a), one reflection
GPET_WV_HD inline int wv_sym(int k, int n) { return k < 0 ? -k - 1 : (k >= n ? 2 * n - 1 - k : k); }
// the tap added at step t = 0..F-1 of the output taken at i
GPET_WV_HD inline int wv_fwd_tap(int t, int i, int n) { return i < n ? t : (t <= i - n ? i - n - t : t); }

// ---- geometry --------------------------------------------------------------------------------------------------------------------
// Forward: a workgroup of 16 x 16 threads owns WV_TILE x WV_TILE coefficients of all four bands of one image; the
// (2 WV_TILE + F - 2)^2 input pixels they read sit in LDS as f64, then the axis-0 pass (2 x WV_TILE rows of that width), and the
// filters.  Inverse: a workgroup owns (2 WV_TILE)^2 output pixels; the (WV_TILE + F/2 - 1)^2 coefficients of each band they read
// sit in LDS, shrunk as they are loaded, then the axis-1 pass (2 planes of that many rows x 2 WV_TILE), and the filters.
constexpr int WV_TILE = 16;
constexpr int WV_THREADS = WV_TILE * WV_TILE;
constexpr int WV_THRESH_THREADS = 256;
constexpr int WV_SIGMA_THREADS = 1024;
constexpr size_t WV_LDS_MAX = CONV_LDS_MAX;
static_assert(WV_LDS_MAX <= (size_t)LDS_DYN_MAX, "the wavelet kernels stay inside the LDS rule of the batch plan");
GPET_WV_HD inline int wv_fwd_patch(int F) { return 2 * WV_TILE + F - 2; }
GPET_WV_HD inline int wv_inv_patch(int F) { return WV_TILE + F / 2 - 1; }
inline size_t wv_fwd_lds_bytes(int F) {
  const size_t P = (size_t)wv_fwd_patch(F);
  return (2 * WV_TAPS_MAX + P * P + 2 * WV_TILE * P) * sizeof(double);
}
inline size_t wv_inv_lds_bytes(int F) {
  const size_t P = (size_t)wv_inv_patch(F);
  return (2 * WV_TAPS_MAX + 4 * P * P + 2 * P * 2 * WV_TILE) * sizeof(double);
}
struct WvGrid {
  int gx, gy;  // workgroups along x and y; gridDim.z = images of the launch
};
inline WvGrid wv_fwd_grid(const WvLevel& v) { return WvGrid{(v.no + WV_TILE - 1) / WV_TILE, (v.mo + WV_TILE - 1) / WV_TILE}; }
// (the inverse of a level writes the level's input extent m x n: the crop)
inline WvGrid wv_inv_grid(const WvLevel& v) {
  return WvGrid{((v.n + 1) / 2 + WV_TILE - 1) / WV_TILE, ((v.m + 1) / 2 + WV_TILE - 1) / WV_TILE};
}
// images of a chunk: a chunk's staging (host frames, host results) and its workspace together stay inside the budget
constexpr size_t WV_CHUNK_BUDGET = (size_t)256 << 20;
constexpr int WV_CHUNK_MAX = STAGE_GRID_Z_MAX;  // gridDim.z
inline StagePlan wv_chunks(int n_img, size_t staged_bytes_per_img, size_t frame_doubles) {
  return stage_plan_z(n_img, staged_bytes_per_img + ((frame_doubles * sizeof(double) + 255) & ~(size_t)255), WV_CHUNK_BUDGET);
}

// ---- the summation order of a BayesShrink threshold ---------------------------------------------------------------------------------
// mean(x x) of a band of R x C coefficients, rows `pitch` apart: one partial sum per row, ascending within the row; thread t of
// WV_THRESH_THREADS adds the partial sums of rows t, t + 256, .. in that order (rows below 256: its row's alone; no row: +0.0);
// the thread sums are combined by halving strides, p[t] = p[t] + p[t + s] for s = 128, 64, .., 1; the total is divided by R C.
// numpy's own order on arrays of this size is another one: the two means differ by at most 2 (R C - 1) 2^-53 relative.
inline double wv_mean_squares(const double* x, int R, int C, size_t pitch) {
  GPET_WV_NO_FMA
  double part[WV_THRESH_THREADS];
  for (int t = 0; t < WV_THRESH_THREADS; ++t) {
    double p = 0.0;
    for (int r = t; r < R; r += WV_THRESH_THREADS) {
      double s = 0.0;
      for (int c = 0; c < C; ++c) s = s + x[(size_t)r * pitch + c] * x[(size_t)r * pitch + c];
      p = r == t ? s : p + s;
    }
    part[t] = p;
  }
  for (int s = WV_THRESH_THREADS / 2; s > 0; s /= 2)
    for (int t = 0; t < s; ++t) part[t] = part[t] + part[t + s];
  return part[0] / (double)((long long)R * C);
}
GPET_WV_HD inline double wv_bayes_thresh(double ms, double var) {
  GPET_WV_NO_FMA
  const double d = ms - var;
  return var / sqrt(WV_EPS > d ? WV_EPS : d);
}
GPET_WV_HD inline double wv_shrink(double x, double t, int mode) {
  GPET_WV_NO_FMA
  const double a = fabs(x);
  if (mode == WV_HARD) return a < t ? 0.0 : x;
  const double g = 1.0 - t / a;
  return x * (g > 0.0 ? g : 0.0);
}

// ---- validation ------------------------------------------------------------------------------------------------------------------
// levels the spec means on M x N frames: its own, or the default; 0 if the filter does not fit the frame at all
inline int wv_levels(const WvSpec& sp, int M, int N) {
  if (sp.n_taps < 2 || sp.n_taps > WV_TAPS_MAX) return 0;
  const int top = wv_max_level(M < N ? M : N, sp.n_taps);
  if (top < 1) return 0;
  return sp.levels > 0 ? sp.levels : wv_default_levels(top);
}
// nullptr if the spec can run on n_img frames of M x N pixels of type pix, else what is wrong with it
inline const char* wv_check(const WvSpec& sp, int pix, int M, int N, int n_img) {
  if (!pix_bytes(pix)) return "unknown pixel type";
  if (M < 1 || N < 1 || n_img < 1) return "empty frame";
  if (sp.n_taps < 2 || sp.n_taps > WV_TAPS_MAX || sp.n_taps % 2) return "filters of 2 to 16 taps, an even number, are built";
  for (int k = 0; k < sp.n_taps; ++k)
    if (!(fabs(sp.dec_lo[k]) < INFINITY)) return "the filter taps must be finite";
  const int top = wv_max_level(M < N ? M : N, sp.n_taps);
  if (top < 1) return "the frame's smaller extent is below the filter's reach (max_level is 0)";
  if (sp.levels < 0) return "wavelet_levels must not be negative (0 means the default)";
  if (sp.levels > top) return "wavelet_levels is above max_level, the largest L with (F - 1) 2^L <= min(M, N)";
  if (wv_levels(sp, M, N) > WV_LEVELS_MAX) return "more than 16 levels are not built";
  if (sp.mode < 0 || sp.mode >= WV_MODE_COUNT) return "unknown mode (soft, hard)";
  if (sp.method < 0 || sp.method >= WV_METHOD_COUNT) return "unknown method (BayesShrink, VisuShrink)";
  if (!(sp.sigma != sp.sigma) && !(sp.sigma > 0.0 && sp.sigma < INFINITY)) return "a given sigma must be above 0";
  if (!(sp.ppf > 0.0) || !(sp.ppf < INFINITY)) return "the ppf constant must be above 0";
  if (sp.method == WV_VISU && !sp.thresholds && !(sp.c > 0.0 && sp.c < INFINITY)) return "VisuShrink needs c = sqrt(2 log(M N))";
  if (sp.thresholds) {
    const long long want = (long long)n_img * wv_levels(sp, M, N) * 3;
    if ((long long)sp.n_thresholds != want) return "injected thresholds are one per frame, level and detail band";
    for (long long i = 0; i < want; ++i)
      if (!(sp.thresholds[i] >= 0.0 && sp.thresholds[i] < INFINITY)) return "injected thresholds must be finite and not negative";
  }
  if (wv_fwd_lds_bytes(sp.n_taps) > WV_LDS_MAX || wv_inv_lds_bytes(sp.n_taps) > WV_LDS_MAX) return "the tile's patch exceeds the LDS bound";
  return nullptr;
}

}  // namespace gpet
