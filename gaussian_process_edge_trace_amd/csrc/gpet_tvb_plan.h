// What the split-Bregman stage (a0: gpet_tvb_images) decides before anything is launched, as plain data: the spec and its
// validation, the skewed workspace of a frame and its index function, the workgroup, how many sweeps a launch runs, the chunks,
// and the one summation order the stage defines for itself.  No HIP, so the host compiler alone builds it (tests/test_tvb_plan.py).
// The reference: gpet_utils.denoise 'tvb' = scikit-image 0.18.3's denoise_tv_bregman(image, weight, max_iter=100, eps=1e-3,
// isotropic=True) for a 2-D single-channel frame.
//
// The arithmetic (all f64, no fused multiply-add, IEEE division and square root; sums left to right as written).
// Input: f64 as it is, f32 widened, u8 / u16 times 1/255 / 1/65535 (a product with the rounded reciprocal).  The output is f64 and
// is not clipped.
// Arrays u, dx, dy, bx, by of (M + 2) x (N + 2), zero; u[1:M+1, 1:N+1] = image; the ring of u is written ONCE and never refreshed:
// top row = image row 1 (counted from 0: the second row), bottom row = the last image row, left column = image column 1 (the
// second), right column = the last image column, corners 0 (never read).  lam = 2 weight, norm = weight + 4 lam, total = M N.
// A sweep, for r = 1..M and c = 1..N in raster order:
//   up = u[r,c]; ux = u[r,c+1] - up; uy = u[r+1,c] - up
//   unew = (lam (u[r+1,c] + u[r-1,c] + u[r,c+1] + u[r,c-1] + dx[r,c-1] - dx[r,c] + dy[r-1,c] - dy[r,c] - bx[r,c-1] + bx[r,c]
//           - by[r-1,c] + by[r,c]) + weight image[r-1,c-1]) / norm
//   u[r,c] = unew; acc += (unew - up) (unew - up)
//   isotropic:   tx = ux + bx[r,c]; ty = uy + by[r,c]; s = sqrt(tx tx + ty ty); dxx = s lam tx / (s lam + 1); dyy = s lam ty / (s lam + 1)
//   anisotropic: s = ux + bx[r,c]; dxx = s > 1/lam ? s - 1/lam : (s < -1/lam ? s + 1/lam : 0); dyy likewise from uy + by[r,c]
//   dx[r,c] = dxx; dy[r,c] = dyy; bx[r,c] = bx[r,c] + (ux - dxx); by[r,c] = by[r,c] + (uy - dyy)
// After a sweep rmse = sqrt(acc / total); sweeps go on while i < max_iter and rmse > eps.  The result is u[1:M+1, 1:N+1].
//
// Cell (r, c) reads the new values of (r, c-1) and (r-1, c) and the old ones of (r, c+1) and (r+1, c): the cells of one
// anti-diagonal r + c = d are independent, and sweeping the diagonals in ascending d gives every cell the operands it had in
// raster order.  One workgroup per frame walks them, one barrier per diagonal.  The ONE deviation: acc is added in the order of
// tvb_acc_sum below, not in raster order (the two sums of n = M N non-negative terms lie within 2 (n - 1) 2^-53 relative).
#pragma once
#include <math.h>
#include <stddef.h>

#include "gpet_conv_plan.h"     // pixel types, CONV_LDS_MAX, staging
#include "gpet_denoise_plan.h"  // dn_align

#if defined(__HIPCC__)
#define GPET_TVB_HD __host__ __device__
#else
#define GPET_TVB_HD
#endif
#if defined(__clang__)
#define GPET_TVB_NO_FMA _Pragma("clang fp contract(off)")
#else
#define GPET_TVB_NO_FMA
#endif

namespace gpet {

// ---- the spec (include/gpet_hip.h: gpet_tvb) ------------------------------------------------------------------------------------
struct TvbSpec {
  double weight = 0.0;  // above 0
  double eps = 1e-3;    // not negative
  int max_iter = 100;   // at least 1
  int isotropic = 1;
};

// ---- the workgroup ---------------------------------------------------------------------------------------------------------------
// One workgroup of TVB_THREADS lanes per frame: eight waves, two per SIMD of a CU.  A step is a chain of dependent f64 operations
// (two or three divisions and a square root among them) behind an LDS read, so two waves to a SIMD fill each other's stalls, and
// a 500 x 500 frame has one cell per lane (profiles/tvb_timing.txt).  Cell k of a diagonal (counted from its first interior row)
// belongs to lane k % TVB_THREADS; a lane owns tvb_cells_per_lane cells of the longest diagonal and handles them in ascending k.
constexpr int TVB_THREADS = 512;
// sweeps one launch runs at most: the host enqueues ceil(max_iter / TVB_SWEEPS_PER_LAUNCH) launches, a finished frame's workgroup
// exits at once
constexpr int TVB_SWEEPS_PER_LAUNCH = 4;
constexpr int TVB_ARRAYS = 6;  // u | dx | dy | bx | by | image, each (M + 2)(N + 2) doubles in the skewed order
enum { TVB_U = 0, TVB_DX = 1, TVB_DY = 2, TVB_BX = 3, TVB_BY = 4, TVB_IMG = 5 };
GPET_TVB_HD inline int tvb_cells_per_lane(int M, int N) { return ((M < N ? M : N) + TVB_THREADS - 1) / TVB_THREADS; }

// ---- the skewed layout ------------------------------------------------------------------------------------------------------------
// An array of P x Q = (M + 2) x (N + 2) cells (R = 0..P-1, C = 0..Q-1, the ring included) is stored diagonal after diagonal,
// D = R + C ascending, and within a diagonal by ascending R: the cells a step touches are contiguous.
GPET_TVB_HD inline int tvb_diag_first(int P, int Q, int D) { return D - (Q - 1) > 0 ? D - (Q - 1) : 0; }
GPET_TVB_HD inline int tvb_diag_len(int P, int Q, int D) { return (D < P - 1 ? D : P - 1) - tvb_diag_first(P, Q, D) + 1; }
// cells of the diagonals before D (0 <= D <= P + Q - 1)
GPET_TVB_HD inline size_t tvb_diag_off(int P, int Q, int D) {
  const size_t a = (size_t)(P < Q ? P : Q), b = (size_t)(P < Q ? Q : P), d = (size_t)D;
  if (d <= a) return d * (d + 1) / 2;
  if (d <= b) return a * (a + 1) / 2 + (d - a) * a;
  const size_t rem = (size_t)P + (size_t)Q - 1 - d;
  return (size_t)P * (size_t)Q - rem * (rem + 1) / 2;
}
GPET_TVB_HD inline size_t tvb_index(int P, int Q, int R, int C) { return tvb_diag_off(P, Q, R + C) + (size_t)(R - tvb_diag_first(P, Q, R + C)); }
inline size_t tvb_cells(int M, int N) { return (size_t)(M + 2) * (size_t)(N + 2); }
inline size_t tvb_frame_doubles(int M, int N) { return TVB_ARRAYS * tvb_cells(M, N); }
inline size_t tvb_frame_bytes(int M, int N) { return dn_align(tvb_frame_doubles(M, N) * sizeof(double)); }
// what a frame keeps in device memory besides its arrays
struct TvbState {
  double acc;      // the sum of the last sweep, in the order of tvb_acc_sum
  int n_iter;      // sweeps run
  int done;        // not 0: n_iter reached max_iter or rmse <= eps
};

// ---- LDS ------------------------------------------------------------------------------------------------------------------------
// The new u, dx, bx, dy, by of the previous diagonal are handed over through LDS, double-buffered: 2 x 5 x min(M, N) doubles, and
// the lanes' partial sums of acc.  This is ALL the LDS of the sweep kernel (it declares no static LDS).
constexpr size_t TVB_LDS_MAX = CONV_LDS_MAX;
inline size_t tvb_lds_bytes(int M, int N) { return ((size_t)10 * (size_t)(M < N ? M : N) + TVB_THREADS) * sizeof(double); }
constexpr int TVB_DIAG_MAX = (int)((TVB_LDS_MAX / sizeof(double) - TVB_THREADS) / 10);  // 768
constexpr int TVB_CELLS_MAX = (TVB_DIAG_MAX + TVB_THREADS - 1) / TVB_THREADS;              // 2: the cells a lane owns at the most

// ---- chunks -----------------------------------------------------------------------------------------------------------------------
// frames of a chunk: a chunk's staging (host frames, host results) and its workspace together stay inside the budget
constexpr size_t TVB_CHUNK_BUDGET = (size_t)256 << 20;
constexpr int TVB_CHUNK_MAX = STAGE_GRID_Z_MAX;  // gridDim.z
inline StagePlan tvb_chunks(int n_img, size_t staged_bytes_per_img, int M, int N) {
  return stage_plan_z(n_img, staged_bytes_per_img + tvb_frame_bytes(M, N), TVB_CHUNK_BUDGET);
}
inline int tvb_launches(int max_iter) { return (max_iter + TVB_SWEEPS_PER_LAUNCH - 1) / TVB_SWEEPS_PER_LAUNCH; }

// ---- the order of acc ---------------------------------------------------------------------------------------------------------------
// t[(r - 1) N + (c - 1)] = (unew - up)^2 of cell (r, c).  Lane l starts from +0.0 and adds its own cells in step order: diagonals
// d = 2 .. M + N ascending, on a diagonal whose interior rows are r0 = max(1, d - N) .. min(M, d - 1) the cells r0 + k for
// k = l, l + TVB_THREADS, .. ascending.  The lane sums are combined by halving strides, p[l] = p[l] + p[l + s] for
// s = TVB_THREADS / 2, .., 1.
inline double tvb_acc_sum(const double* t, int M, int N) {
  GPET_TVB_NO_FMA
  double part[TVB_THREADS];
  for (int l = 0; l < TVB_THREADS; ++l) {
    double p = 0.0;
    for (int d = 2; d <= M + N; ++d) {
      const int r0 = d - N > 1 ? d - N : 1, r1 = d - 1 < M ? d - 1 : M;
      for (int k = l; k <= r1 - r0; k += TVB_THREADS) p = p + t[(size_t)(r0 + k - 1) * N + (d - r0 - k - 1)];
    }
    part[l] = p;
  }
  for (int s = TVB_THREADS / 2; s > 0; s /= 2)
    for (int l = 0; l < s; ++l) part[l] = part[l] + part[l + s];
  return part[0];
}
// whether another sweep follows the i-th (i counts the sweeps run)
GPET_TVB_HD inline bool tvb_goes_on(double acc, double total, double eps, int i, int max_iter) {
  GPET_TVB_NO_FMA
  return i < max_iter && sqrt(acc / total) > eps;
}

// ---- one cell ---------------------------------------------------------------------------------------------------------------------
struct TvbCellOut {
  double u, dx, dy, bx, by, diff2;
};
// up, dxo, dyo, bxo, byo: the cell's own old values; ur, ud: the old u of (r, c+1), (r+1, c); ul, dxl, bxl: the new values of
// (r, c-1); uu, dyu, byu: the new values of (r-1, c); inv_lam = 1 / lam
GPET_TVB_HD inline TvbCellOut tvb_cell(double up, double dxo, double dyo, double bxo, double byo, double im, double ur, double ud, double ul,
                                       double dxl, double bxl, double uu, double dyu, double byu, double lam, double weight, double norm,
                                       double inv_lam, int isotropic) {
  GPET_TVB_NO_FMA
  TvbCellOut o;
  const double ux = ur - up, uy = ud - up;
  const double unew = (lam * (ud + uu + ur + ul + dxl - dxo + dyu - dyo - bxl + bxo - byu + byo) + weight * im) / norm;
  o.u = unew;
  o.diff2 = (unew - up) * (unew - up);
  double dxx, dyy;
  if (isotropic) {
    const double tx = ux + bxo, ty = uy + byo;
    const double s = sqrt(tx * tx + ty * ty);
    dxx = s * lam * tx / (s * lam + 1.0);
    dyy = s * lam * ty / (s * lam + 1.0);
  } else {
    double s = ux + bxo;
    dxx = s > inv_lam ? s - inv_lam : (s < -inv_lam ? s + inv_lam : 0.0);
    s = uy + byo;
    dyy = s > inv_lam ? s - inv_lam : (s < -inv_lam ? s + inv_lam : 0.0);
  }
  o.dx = dxx;
  o.dy = dyy;
  o.bx = bxo + (ux - dxx);
  o.by = byo + (uy - dyy);
  return o;
}

// ---- validation ------------------------------------------------------------------------------------------------------------------
// nullptr if the spec can run on n_img frames of M x N pixels of type pix, else what is wrong with it
inline const char* tvb_check(const TvbSpec& sp, int pix, int M, int N, int n_img) {
  if (!pix_bytes(pix)) return "unknown pixel type";
  if (n_img < 1) return "no frame";
  if (M < 2 || N < 2) return "frames of at least 2 x 2 pixels (the library raises on a 1-pixel axis)";
  if (!(sp.weight > 0.0) || !(sp.weight < INFINITY)) return "weight must be above 0";
  if (!(sp.eps >= 0.0)) return "eps must not be negative";
  if (sp.max_iter < 1) return "max_iter must be at least 1";
  if ((M < N ? M : N) > TVB_DIAG_MAX) return "the frame's smaller extent exceeds what the LDS bound holds of a diagonal";
  return nullptr;
}

}  // namespace gpet
