// Denoise quality metrics (gpet_metrics_images): the four figures the reference's denoise(verbose=True) prints --
// PSNR, SSIM, min-max NRMSE of a pair (a = the frame as given, b = the denoised frame) and the Shannon entropy of b -- as plain data
// and plain arithmetic.  No HIP: the host compiler alone builds this header (tests/test_metrics_plan.py compiles it into a shim with
// -ffp-contract=off), the kernels of gpet_k_metrics.inc call the same functions on the device, and tests/metrics_ref.py restates them
// with numpy.  The reference: scikit-image 0.18.3's peak_signal_noise_ratio, structural_similarity (default call), normalized_root_mse
// (normalization='min-max') and shannon_entropy.
//
// Working type of the simple metrics: W = f64 as soon as a or b is f64, else f32 (np.result_type(a, b, float32)).  d = a - b and d d
// round in W; the squares are widened to f64 and summed (metrics_sum); mse = sum / n.
//   PSNR    10 log10(R R / mse); R given, or from a's type: 255, 65535, floats 1 when min(a) >= 0 else 2; a float frame outside
//           [-1, 1] is refused in the library's words.  mse = 0 gives what IEEE division gives.
//   NRMSE   sqrt(mse) / (max(a) - min(a)), the difference taken in W
//   SSIM    x, y = a, b widened to f64; planes x, y, x x, y y, x y (products rounded first); every plane through the running sum of
//           scipy.ndimage.uniform_filter1d along axis 0, then along axis 1 (metrics_line_*: reflect extension, tmp = the first `size`
//           extended samples added in ascending order from 0.0, then tmp += new - old; out = tmp / size); S from the five filtered
//           values by metrics_ssim_S; the mean of S over the map cropped by (win_size - 1) / 2 on every side (metrics_sum / count).
//           R given, or 255 / 65535 / 2 (floats: dmax - dmin of (-1, 1)) from a's type.
//   entropy of b: counts c of the distinct values (-0.0 and 0.0 are one value), p = 1.0 c / n, term -p log(p), sum, / log(2).
//
// The counts.  Method: every pixel of b, widened to f64 with -0.0 turned into 0.0, becomes an order-preserving 64-bit key
// (metrics_key); the frame's keys are sorted in workspace by a bitonic network over the next power of two (padded with the all-ones
// key, which no number that is not NaN maps to), and a run of equal keys is one distinct value, its length the count -- exact for
// every pixel type.  The frame size is bounded by METRICS_PX_MAX (2^26 pixels: the run lengths and the network's indices are int32 in
// the kernels) and by the workspace of one frame, which must fit the chunk budget.  Frames that hold a NaN have no defined figures.
//
// The orders the device owns are three sums, all in the ONE order of metrics_sum: the squared differences in raster order, S over the
// crop in raster order, and the entropy terms laid out at the sorted position where each run starts (+0.0 everywhere else).
// Accuracy of the device's log (entropy terms): one unit in the last place (the HIP math API's table for double precision log), the
// constant the bound of DESIGN section 9 uses; log10, sqrt and the final divisions run on the host, in metrics_figures.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "gpet_conv_plan.h"     // pixel types, staging
#include "gpet_denoise_plan.h"  // dn_align

#if defined(__HIPCC__)
#define GPET_METRICS_HD __host__ __device__
#else
#define GPET_METRICS_HD
#endif
// (no fused multiply-add in the functions the kernels share with the host, whatever the compiler's default)
#if defined(__clang__)
#define GPET_METRICS_NO_FMA _Pragma("clang fp contract(off)")
#else
#define GPET_METRICS_NO_FMA
#endif

namespace gpet {

// ---- the spec (include/gpet_hip.h: gpet_metrics) -------------------------------------------------------------------------------------
struct MetricsSpec {
  int win_size = 7;               // odd, at least 3, at most min(M, N)
  int use_sample_covariance = 1;
  double K1 = 0.01, K2 = 0.03;    // not negative
  double data_range = 0.0;        // above 0: R of PSNR and SSIM; 0: the library's rule from a's type
};
constexpr unsigned int METRICS_A_ON_DEVICE = 4u, METRICS_B_ON_DEVICE = 32u, METRICS_MAPS_ON_DEVICE = 64u;
constexpr long long METRICS_PX_MAX = 1LL << 26;

// ---- launch shapes -------------------------------------------------------------------------------------------------------------------
constexpr int METRICS_THREADS = 256;   // lanes of a reduction workgroup: the order of metrics_sum
constexpr int METRICS_COLS = 64;       // axis-0 pass: columns of a workgroup, one lane each
constexpr int METRICS_ROWS = 64;       // axis-1 pass: rows of a workgroup, one lane each
constexpr int METRICS_TILE = 8;        // axis-1 pass: columns staged through LDS at a time (per plane: the new and the old samples)
constexpr int METRICS_TILE_PITCH = METRICS_TILE + 1;  // doubles between the rows of a tile: 64-bit LDS reads of 32 rows hit 32 banks
constexpr int METRICS_SORT_SEG = 2048; // keys a workgroup sorts in LDS (16 KB)
constexpr size_t METRICS_CHUNK_BUDGET = (size_t)512 << 20;

// what a frame pair keeps in device memory besides its workspace; read back once per call
struct MetricsAcc {
  double sq_sum;    // the squared differences, metrics_sum order
  double a_min, a_max;
  double ssim_sum;  // S over the crop, metrics_sum order
  double ent_sum;   // the entropy terms, metrics_sum order
};

inline long long metrics_pow2(long long n) {
  long long p = 1;
  while (p < n) p *= 2;
  return p;
}
// workspace of one pair: five intermediate planes (the sort's keys lie over them afterwards: pow2(px) < 2 px <= 5 px) and the S
// map, f64 each; then the staged copies of a and b where they come from the host
inline size_t metrics_frame_bytes(long long px, size_t staged_a, size_t staged_b) {
  return dn_align((size_t)6 * (size_t)px * sizeof(double)) + dn_align(staged_a) + dn_align(staged_b);
}
inline StagePlan metrics_chunks(int n_img, size_t frame_bytes) { return stage_plan_z(n_img, frame_bytes, METRICS_CHUNK_BUDGET); }

// ---- the working type ----------------------------------------------------------------------------------------------------------------
GPET_METRICS_HD inline bool metrics_work_f64(int pix_a, int pix_b) { return pix_a == PIX_F64 || pix_b == PIX_F64; }
// (a - b)^2 in W, widened; a and b given as the f64 values of the pixels (exact for every pixel type)
GPET_METRICS_HD inline double metrics_sqdiff(double a, double b, bool f64) {
  GPET_METRICS_NO_FMA
  if (f64) {
    const double d = a - b;
    return d * d;
  }
  const float d = (float)a - (float)b;
  const float q = d * d;
  return (double)q;
}
// max(a) - min(a) in W, widened
GPET_METRICS_HD inline double metrics_span(double a_min, double a_max, bool f64) {
  if (f64) return a_max - a_min;
  const float s = (float)a_max - (float)a_min;
  return (double)s;
}

// ---- the one summation order -----------------------------------------------------------------------------------------------------------
// Lane l of METRICS_THREADS starts from +0.0 and adds t[l], t[l + METRICS_THREADS], .. in ascending order; the lane sums are combined by
// halving strides, p[l] = p[l] + p[l + s] for s = METRICS_THREADS / 2, .., 1.
inline double metrics_sum(const double* t, long long n) {
  GPET_METRICS_NO_FMA
  double part[METRICS_THREADS];
  for (int l = 0; l < METRICS_THREADS; ++l) {
    double p = 0.0;
    for (long long i = l; i < n; i += METRICS_THREADS) p = p + t[i];
    part[l] = p;
  }
  for (int s = METRICS_THREADS / 2; s > 0; s /= 2)
    for (int l = 0; l < s; ++l) part[l] = part[l] + part[l + s];
  return part[0];
}

// ---- the running-sum filter ------------------------------------------------------------------------------------------------------------
// sample e of the extended line (e = 0 .. len + size - 2) is sample metrics_reflect(e - size / 2, len) of the line
GPET_METRICS_HD inline int metrics_reflect(int s, int len) { return s < 0 ? -s - 1 : (s >= len ? 2 * len - 1 - s : s); }
GPET_METRICS_HD inline double metrics_line_step(double tmp, double fresh, double old) {
  GPET_METRICS_NO_FMA
  const double d = fresh - old;
  return tmp + d;
}
// the host's form of one line; the kernels run the same two loops with the samples formed on the fly
inline void metrics_line(const double* line, int len, int size, double* out, ptrdiff_t in_stride = 1, ptrdiff_t out_stride = 1) {
  GPET_METRICS_NO_FMA
  const int h = size / 2;
  double tmp = 0.0;
  for (int e = 0; e < size; ++e) tmp = tmp + line[metrics_reflect(e - h, len) * in_stride];
  out[0] = tmp / (double)size;
  for (int i = 1; i < len; ++i) {
    tmp = metrics_line_step(tmp, line[metrics_reflect(i + size - 1 - h, len) * in_stride], line[metrics_reflect(i - 1 - h, len) * in_stride]);
    out[i * out_stride] = tmp / (double)size;
  }
}

// ---- S -----------------------------------------------------------------------------------------------------------------------------
struct MetricsSsimConst {
  double cov_norm, C1, C2;
};
inline MetricsSsimConst metrics_ssim_const(int win_size, int use_sample_covariance, double K1, double K2, double R) {
  GPET_METRICS_NO_FMA
  MetricsSsimConst k;
  const double NP = (double)win_size * (double)win_size;
  k.cov_norm = use_sample_covariance ? NP / (NP - 1.0) : 1.0;
  const double k1 = K1 * R, k2 = K2 * R;
  k.C1 = k1 * k1;
  k.C2 = k2 * k2;
  return k;
}
GPET_METRICS_HD inline double metrics_ssim_S(double ux, double uy, double uxx, double uyy, double uxy, double cov_norm, double C1, double C2) {
  GPET_METRICS_NO_FMA
  const double pxx = ux * ux, pyy = uy * uy, pxy = ux * uy;
  const double vx = cov_norm * (uxx - pxx);
  const double vy = cov_norm * (uyy - pyy);
  const double vxy = cov_norm * (uxy - pxy);
  const double t2 = 2.0 * ux;
  const double A1 = t2 * uy + C1;
  const double A2 = 2.0 * vxy + C2;
  const double B1 = pxx + pyy + C1;
  const double B2 = vx + vy + C2;
  const double D = B1 * B2;
  return (A1 * A2) / D;
}

// ---- entropy ---------------------------------------------------------------------------------------------------------------------------
// the order-preserving key of a value that is not NaN; -0.0 and 0.0 share one
GPET_METRICS_HD inline uint64_t metrics_key(double v) {
  if (v == 0.0) v = 0.0;
  union {
    double d;
    uint64_t u;
  } c;
  c.d = v;
  return (c.u >> 63) ? ~c.u : (c.u | 0x8000000000000000ULL);
}
constexpr uint64_t METRICS_KEY_PAD = ~(uint64_t)0;
GPET_METRICS_HD inline double metrics_entropy_term(long long count, long long n) {
  GPET_METRICS_NO_FMA
  const double p = 1.0 * (double)count / (double)n;
  return -p * log(p);
}
// the end of the run that starts at i in keys sorted ascending (first index in (i, n] whose key differs)
GPET_METRICS_HD inline long long metrics_run_end(const uint64_t* keys, long long i, long long n) {
  const uint64_t k = keys[i];
  long long lo = i + 1, hi = n;
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (keys[mid] == k) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// e[i] of the sorted keys: the term of the run that starts at i, +0.0 elsewhere
inline void metrics_entropy_terms(const uint64_t* keys, long long n, double* e) {
  for (long long i = 0; i < n; ++i)
    e[i] = (i == 0 || keys[i] != keys[i - 1]) ? metrics_entropy_term(metrics_run_end(keys, i, n) - i, n) : 0.0;
}

// ---- the figures from the device's sums (host) ------------------------------------------------------------------------------------------
inline double metrics_default_range_ssim(int pix_a) { return pix_a == PIX_U8 ? 255.0 : pix_a == PIX_U16 ? 65535.0 : 2.0; }
// R of PSNR by the library's rule; 0 with the library's words in msg when a float frame leaves [-1, 1]
inline double metrics_default_range_psnr(int pix_a, double a_min, double a_max, char* msg, size_t cap) {
  if (pix_a == PIX_U8) return 255.0;
  if (pix_a == PIX_U16) return 65535.0;
  if (a_max > 1.0 || a_min < -1.0) {
    snprintf(msg, cap, "im_true has intensity values outside the range expected for its data type.  Please manually specify the data_range");
    return 0.0;
  }
  return a_min >= 0.0 ? 1.0 : 2.0;
}
// out[4] = psnr, ssim, nrmse, entropy; 0, or 1 with the refusal in msg
inline int metrics_figures(const MetricsAcc& acc, const MetricsSpec& sp, int pix_a, int pix_b, int M, int N, double* out, char* msg, size_t cap) {
  GPET_METRICS_NO_FMA
  const double n = (double)M * (double)N;
  const double R = sp.data_range > 0.0 ? sp.data_range : metrics_default_range_psnr(pix_a, acc.a_min, acc.a_max, msg, cap);
  if (!(R > 0.0)) return 1;
  const double mse = acc.sq_sum / n;
  const double rr = R * R;
  out[0] = 10.0 * log10(rr / mse);
  const int pad = (sp.win_size - 1) / 2;
  const double nc = (double)(M - 2 * pad) * (double)(N - 2 * pad);
  out[1] = acc.ssim_sum / nc;
  out[2] = sqrt(mse) / metrics_span(acc.a_min, acc.a_max, metrics_work_f64(pix_a, pix_b));
  out[3] = acc.ent_sum / log(2.0);
  return 0;
}

// ---- the refusals, in the order they are checked: 0, or 1 with the reason in msg ------------------------------------------------------------
inline int metrics_check(bool null_arg, int n_img, int pix_a, int pix_b, long long M, long long N, const MetricsSpec* sp, size_t staged_a,
                         size_t staged_b, char* msg, size_t cap) {
  if (null_arg || !sp) return snprintf(msg, cap, "metrics: a null pointer"), 1;
  if (n_img < 1) return snprintf(msg, cap, "metrics: no frame"), 1;
  if (!pix_bytes(pix_a) || !pix_bytes(pix_b)) return snprintf(msg, cap, "metrics: unknown pixel type"), 1;
  if (M < 1 || N < 1) return snprintf(msg, cap, "metrics: empty frame"), 1;
  if (sp->win_size > M || sp->win_size > N)
    return snprintf(msg, cap, "win_size exceeds image extent.  If the input is a multichannel (color) image, set multichannel=True."), 1;
  if (sp->win_size % 2 != 1) return snprintf(msg, cap, "Window size must be odd."), 1;
  if (sp->win_size < 3) return snprintf(msg, cap, "metrics: win_size must be at least 3"), 1;
  if (!(sp->K1 >= 0.0)) return snprintf(msg, cap, "K1 must be positive"), 1;
  if (!(sp->K2 >= 0.0)) return snprintf(msg, cap, "K2 must be positive"), 1;
  if (!(sp->data_range >= 0.0) || !(sp->data_range < INFINITY)) return snprintf(msg, cap, "metrics: data_range must be a finite number above 0 (0: the library's rule)"), 1;
  if (M > METRICS_PX_MAX / N) return snprintf(msg, cap, "metrics: a frame exceeds 2^26 pixels (M * N)"), 1;
  const size_t fb = metrics_frame_bytes(M * N, staged_a, staged_b);
  if (fb > METRICS_CHUNK_BUDGET)
    return snprintf(msg, cap, "metrics: the workspace of one frame (%zu bytes: six float64 planes of %lld x %lld and its staging) exceeds the chunk budget of %zu bytes",
                    fb, M, N, METRICS_CHUNK_BUDGET), 1;
  return 0;
}

}  // namespace gpet
