// What the non-local means stage (a0: gpet_nlmeans_images) decides before anything is launched, as plain data: the spec and its
// validation, the patch of the padded frame a workgroup keeps in LDS, launch geometry, the integer-trick exponential the kernel
// and the host share, and the taps for hosts that are not Python.  No HIP, so the host compiler alone builds it
// (tests/test_nlmeans_plan.py).  The reference: gpet_utils.denoise 'nl' (gpet_utils.py:133-134) = scikit-image 0.18.3's
// denoise_nl_means(image, patch_size, patch_distance, h, fast_mode=False, sigma) on a 2-D single-channel frame.
//
// The arithmetic (all f64, no fused multiply-add).  s = patch_size (+ 1 if even), off = s / 2, d = patch_distance, var2 = 2 sigma^2.
// P is the frame widened to f64 -- integer frames keep their range -- and padded by off with numpy's 'reflect' (c b | a b c | b a).
// Output pixel (row, col) of an M x N frame walks the candidates i = row - min(d, row) .. row + min(d + 1, M - row) - 1 (outer) and
// j likewise (inner).  A candidate's distance starts at 0; before patch row a = 0 .. s - 1 is added, a distance above 5.0 ends the
// candidate with weight exactly 0 (looked at only there; with var2 > 0 the distance may fall again: the decision stands); else for
// b = 0 .. s - 1: t = P[row + a][col + b] - P[i + a][j + b], dist = dist + w[a][b] * (t * t - var2).  After the rows
// weight = nlm_fexp(-max(0, dist)); wsum = wsum + weight, acc = acc + weight * P[i + off][j + off]; the result is acc / wsum.
#pragma once
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "gpet_denoise_plan.h"

#if defined(__HIPCC__)
#define GPET_NLM_HD __host__ __device__
#else
#define GPET_NLM_HD
#endif

namespace gpet {

// ---- the spec (include/gpet_hip.h: gpet_nlmeans) --------------------------------------------------------------------------------
struct NlmSpec {
  int patch_size = 7;      // as the caller wrote it: an even size means the next odd one
  int patch_distance = 11;
  double h = 0.1, sigma = 0.0;
  const double* taps = nullptr;  // [s * s], host memory: w[a][b] of the arithmetic above (nlm_taps_c, or numpy's in Python)
};
inline int nlm_patch(int patch_size) { return patch_size + (patch_size % 2 == 0 ? 1 : 0); }

// ---- geometry --------------------------------------------------------------------------------------------------------------------
// A workgroup of 16 x 16 threads owns NLM_TILE x NLM_TILE output pixels of one image, a pixel per thread.  Every patch any of its
// candidates reads lies in the (NLM_TILE + 2 d + 2 off)^2 pixels of the padded frame around the tile; they sit in LDS as f64, rows
// nlm_lds_stride apart: the smallest pitch at or above the extent that is 16 doubles mod 32, so that the two rows of 16 lanes an
// 8-byte LDS read serves at once fall into disjoint banks.
constexpr int NLM_TILE = 16;
constexpr int NLM_PATCH_MAX = 15;  // registers and sense: the reference's default is 7
constexpr int NLM_DIST_MAX = 31;   // the largest distance whose patch fits the LDS bound at the smallest patch
constexpr size_t NLM_LDS_MAX = CONV_LDS_MAX;
inline int nlm_extent(int s, int d) { return NLM_TILE + 2 * d + 2 * (s / 2); }
GPET_NLM_HD inline int nlm_lds_stride(int extent) { return ((extent + 15) / 32) * 32 + 16; }
inline size_t nlm_lds_bytes(int s, int d) {
  const int e = nlm_extent(s, d);
  return (size_t)e * nlm_lds_stride(e) * sizeof(double);
}
struct NlmGrid {
  int gx, gy;  // workgroups along x and y; gridDim.z = images of the launch
};
inline NlmGrid nlm_grid(int M, int N) { return NlmGrid{(N + NLM_TILE - 1) / NLM_TILE, (M + NLM_TILE - 1) / NLM_TILE}; }
// position q of an axis of length n, -n < q < 2 n - 1, under numpy's 'reflect' (scipy's 'mirror'): the edge pixel is not repeated
GPET_NLM_HD inline int nlm_mirror(int q, int n) {
  if (q < 0) q = -q;
  return q > n - 1 ? 2 * (n - 1) - q : q;
}

// ---- the exponential --------------------------------------------------------------------------------------------------------------
// Schraudolph's: the double whose low word is 0 and whose high word is the int32 (int)(C y) + 1072632447, C the double nearest
// 2^20 / ln 2, the product in f64, the conversion truncating.  nlm_fexp(0) = 0.9710078239440918.  The reference's conversion is
// undefined once the high word would go negative (y = -800 gave -1.18e269 there): HERE THE WEIGHT IS +0.0 FOR y < -708, and parity
// with the reference is claimed only where no candidate's final distance exceeds 708.
constexpr double NLM_FEXP_C = 1512775.3951951857;  // 1048576 / log(2)
constexpr int NLM_FEXP_BIAS = 1072632447;
constexpr double NLM_FEXP_MIN_ARG = -708.0;
constexpr double NLM_CUTOFF = 5.0;
GPET_NLM_HD inline double nlm_fexp(double y) {
  if (y < NLM_FEXP_MIN_ARG) return 0.0;
  const int hi = (int)(NLM_FEXP_C * y) + NLM_FEXP_BIAS;
  const unsigned long long bits = (unsigned long long)(unsigned int)hi << 32;
  double r;
  memcpy(&r, &bits, sizeof r);
  return r;
}

// ---- taps for hosts that are not Python ----------------------------------------------------------------------------------------
// w[a][b] = exp(-(x_a^2 + x_b^2) / (2 A^2)) * (1 / (sum * h * h)), x = -off .. off, A = (s - 1) / 4, sum = numpy's pairwise sum of
// the s * s exponentials, into out[s * s] (s odd).  The exponential is the C library's; numpy's vectorised one differs from it by
// one unit in the last place for some arguments, which is why the taps are an input of the call.
inline void nlm_taps_c(int s, double h, double* out) {
  const int off = s / 2;
  const double A = (s - 1.0) / 4.0;
  for (int a = 0; a < s; ++a)
    for (int b = 0; b < s; ++b) {
      const double xa = a - off, xb = b - off;
      out[a * s + b] = exp(-(xa * xa + xb * xb) / (2 * A * A));
    }
  const double sum = s * s > 1 ? out[0] + dn_pairwise_sum(out + 1, s * s - 1) : out[0];
  const double scale = 1.0 / (sum * h * h);
  for (int i = 0; i < s * s; ++i) out[i] = out[i] * scale;
}

// ---- validation ------------------------------------------------------------------------------------------------------------------
// nullptr if the spec can run on M x N frames of pixel type pix, else what is wrong with it
inline const char* nlm_check(const NlmSpec& sp, int pix, int M, int N) {
  if (!pix_bytes(pix)) return "unknown pixel type";
  if (M < 1 || N < 1) return "empty frame";
  if (sp.patch_size < 2) return "patch_size must be at least 2 (a patch of one pixel makes the reference's taps NaN)";
  const int s = nlm_patch(sp.patch_size);
  if (s > NLM_PATCH_MAX) return "patches of more than 15 x 15 pixels are not built";
  if (s / 2 >= (M < N ? M : N)) return "the patch radius must be below the frame's smaller extent (the padding reflects once)";
  if (sp.patch_distance < 0) return "patch_distance must not be negative";
  if (sp.patch_distance > NLM_DIST_MAX) return "patch distances above 31 are not built";
  if (!(sp.h > 0.0) || !(sp.h < INFINITY)) return "h must be above 0";
  if (!(sp.sigma >= 0.0) || !(sp.sigma < INFINITY)) return "sigma must not be negative";
  if (nlm_lds_bytes(s, sp.patch_distance) > NLM_LDS_MAX) return "the tile's padded neighbourhood exceeds the LDS bound";
  if (!sp.taps) return "the taps are a null pointer";
  for (int i = 0; i < s * s; ++i)
    if (!(fabs(sp.taps[i]) < INFINITY)) return "the taps must be finite";
  return nullptr;
}

}  // namespace gpet
