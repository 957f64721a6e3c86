// What the denoising stage in front of the gradient-image convolution (a0: gpet_denoise_images, the *_dn raw-frame calls) decides
// before anything is launched, as plain data: the spec and its validation, window origin and rank, the Gaussian radius and taps,
// launch geometry and LDS bytes, the pixel type a technique leaves behind, the device workspace per image, and how many images of
// a chunk fit the staging budget once that workspace is counted.  No HIP, so the host compiler alone builds it
// (tests/test_denoise_plan.py).  The reference: gpet_utils.denoise (gpet_utils.py:122-158) = scipy.ndimage.median_filter /
// minimum_filter / gaussian_filter and skimage.restoration.denoise_tv_chambolle.
#pragma once
#include <math.h>
#include <stddef.h>

#include "gpet_conv_plan.h"

namespace gpet {

// ---- the spec (include/gpet_hip.h: gpet_denoise, GPET_DN_*, GPET_DN_MODE_*) ---------------------------------------------------
enum { DN_NONE = 0, DN_MEDIAN = 1, DN_MINIMUM = 2, DN_GAUSSIAN = 3, DN_TVC = 4, DN_COUNT = 5 };
enum { DN_MODE_REFLECT = 0, DN_MODE_NEAREST = 1, DN_MODE_COUNT = 2 };
struct DenoiseSpec {
  int technique = DN_NONE;
  int size_y = 0, size_x = 0;  // median / minimum: the window
  int mode = DN_MODE_REFLECT;  // median / minimum / gaussian: how the image continues beyond its border
  double sigma_y = 0.0, sigma_x = 0.0, truncate = 4.0;  // gaussian
  double weight = 0.1, eps = 2.0e-4;                    // tvc
  int n_iter_max = 200;
};

// ---- boundary: position i of an axis of length n, any i ------------------------------------------------------------------------
// reflect: d c b a | a b c d | d c b a (scipy's default), nearest: a a a a | a b c d | d d d d
inline int dn_extend(int i, int n, int mode) {
  if (mode == DN_MODE_NEAREST) return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
  const int period = 2 * n;
  int p = i % period;
  if (p < 0) p += period;
  return p < n ? p : period - 1 - p;
}

// ---- median / minimum ------------------------------------------------------------------------------------------------------------
// the window of extent k starts k / 2 pixels before the output pixel (scipy: the centre of an even window is its k / 2-th element)
inline int dn_origin(int k) { return k / 2; }
// element of the sorted window the filter returns
inline int dn_rank(int technique, int size_y, int size_x) { return technique == DN_MEDIAN ? (size_y * size_x) / 2 : 0; }
constexpr int DN_WINDOW_MAX = 81;  // 9 x 9
// a workgroup of 64 x 4 threads owns CONV_TILE_X columns x CONV_TILE_Y rows of one image, as the convolution does; its patch sits
// in LDS in the frame's own pixel type
inline size_t dn_rank_lds_bytes(int size_y, int size_x, int pix) {
  return (size_t)(CONV_TILE_Y + size_y - 1) * (CONV_TILE_X + size_x - 1) * (size_t)pix_bytes(pix);
}

// ---- gaussian --------------------------------------------------------------------------------------------------------------------
inline int dn_gauss_radius(double sigma, double truncate) { return (int)(truncate * sigma + 0.5); }
constexpr int DN_GAUSS_RADIUS_MAX = 255;
// (scipy skips an axis whose sigma is not above 1e-15; a spec needs both above 0)
// numpy's float64 add.reduce of a contiguous array: a[0] + pairwise_sum(a[1:]), eight partial sums per block of up to 128
inline double dn_pairwise_sum(const double* a, int n) {
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res = res + a[i];
    return res;
  }
  if (n <= 128) {
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res = res + a[i];
    return res;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  return dn_pairwise_sum(a, n2) + dn_pairwise_sum(a + n2, n - n2);
}
// scipy's _gaussian_kernel1d(sigma, 0, radius): w[x + r] = exp(-0.5 / sigma^2 x^2) / sum, x = -r .. r, into w[2 r + 1].  The
// exponential is the C library's; scipy's is numpy.exp, whose vectorised forms differ from it by one unit in the last place for
// some arguments.
inline void dn_gauss_taps(double sigma, int r, double* w) {
  const double c = -0.5 / (sigma * sigma);
  for (int x = -r; x <= r; ++x) w[x + r] = exp(c * (double)(x * x));
  const double s = r > 0 ? w[0] + dn_pairwise_sum(w + 1, 2 * r) : w[0];
  for (int i = 0; i <= 2 * r; ++i) w[i] = w[i] / s;
}

// ---- tvc -------------------------------------------------------------------------------------------------------------------------
// a workgroup of 64 x 4 threads owns CONV_TILE_X x CONV_TILE_Y pixels; `out` of its tile and of the row below / the column to the
// right sit in LDS as f64, and so does the tile's d
constexpr size_t DN_TVC_LDS_BYTES = 2 * (size_t)(CONV_TILE_Y + 1) * (CONV_TILE_X + 1) * sizeof(double);
// per image: E_0, E of the last iteration, the `done` flag and the iteration count (k_dn_tvc_check), in front of the partial sums
constexpr size_t DN_TVC_STATE_BYTES = 32;
// iterations enqueued between two reads of the images' `done` flags
constexpr int DN_TVC_GROUP = 8;
inline int dn_tvc_workgroups(int M, int N) {
  const ConvGrid g = conv_grid(M, N);
  return g.gx * g.gy;
}

// ---- validation ------------------------------------------------------------------------------------------------------------------
// nullptr if the spec can run on frames of pixel type pix, else what is wrong with it (DN_NONE is always fine)
inline const char* dn_check(const DenoiseSpec& s, int pix) {
  if (s.technique < 0 || s.technique >= DN_COUNT) return "unknown denoising technique";
  if (s.technique == DN_NONE) return nullptr;
  if (!pix_bytes(pix)) return "unknown pixel type";
  if (s.technique != DN_TVC && (s.mode < 0 || s.mode >= DN_MODE_COUNT)) return "unsupported boundary mode (reflect and nearest are built)";
  if (s.technique == DN_MEDIAN || s.technique == DN_MINIMUM) {
    if (s.size_y < 1 || s.size_x < 1) return "window extents must be at least 1";
    if (s.size_y > DN_WINDOW_MAX || s.size_x > DN_WINDOW_MAX || s.size_y * s.size_x > DN_WINDOW_MAX) return "windows of more than 81 pixels (9 x 9) are not built";
    if (dn_rank_lds_bytes(s.size_y, s.size_x, pix) > CONV_LDS_MAX) return "the window's patch exceeds the LDS bound";
  }
  if (s.technique == DN_GAUSSIAN) {
    if (!(s.sigma_y > 0.0) || !(s.sigma_x > 0.0)) return "sigma must be above 0";
    if (!(s.truncate > 0.0)) return "truncate must be above 0";
    if (!(s.truncate * s.sigma_y < DN_GAUSS_RADIUS_MAX) || !(s.truncate * s.sigma_x < DN_GAUSS_RADIUS_MAX)) return "Gaussian radius above 255";
  }
  if (s.technique == DN_TVC) {
    if (!(s.weight > 0.0)) return "weight must be above 0";
    if (!(s.eps >= 0.0)) return "eps must not be negative";
    if (s.n_iter_max < 1) return "n_iter_max must be at least 1";
  }
  return nullptr;
}

// ---- what a technique leaves behind ----------------------------------------------------------------------------------------------
// pixel type of the denoised frame, the reference's output dtype: the frame's own for the three filters (scipy quantises integer
// frames after each Gaussian pass), f64 for tvc (u8 / u16 through img_as_float; f32 promoted -- the reference iterates in f32)
inline int dn_out_pix(int technique, int pix) { return technique == DN_TVC ? PIX_F64 : pix; }

// ---- device workspace ------------------------------------------------------------------------------------------------------------
// One block per image of a chunk, every part a multiple of 256 bytes:
//   median / minimum   out[px] (T)
//   gaussian           out[px] (T) | tmp[px] (T): the frame between the two passes
//   tvc                out[px] (f64) | p[4][px] (f64): two planes of iteration parity 0, two of parity 1 | state | partials[2][workgroups] (f64)
struct DenoiseLayout {
  size_t off_out, off_tmp, off_p, off_part;  // byte offsets inside an image's block (0 where the part is absent but out)
  size_t plane_bytes;                        // bytes between tvc's p planes
  int n_wg;                                  // tvc: workgroups (= partial sums of each kind) per image
  size_t img_bytes;                          // bytes of the block
};
inline size_t dn_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline DenoiseLayout dn_layout(int technique, int pix, int M, int N) {
  DenoiseLayout L{0, 0, 0, 0, 0, 0, 0};
  if (technique == DN_NONE) return L;
  const size_t px = (size_t)M * N;
  const size_t frame = dn_align(px * (size_t)pix_bytes(dn_out_pix(technique, pix)));
  size_t off = frame;
  if (technique == DN_GAUSSIAN) {
    L.off_tmp = off;
    off += frame;
  }
  if (technique == DN_TVC) {
    L.plane_bytes = frame;
    L.off_p = off;
    off += 4 * frame;
    L.n_wg = dn_tvc_workgroups(M, N);
    L.off_part = off;
    off += dn_align(DN_TVC_STATE_BYTES + 2 * (size_t)L.n_wg * sizeof(double));
  }
  L.img_bytes = off;
  return L;
}

// ---- chunks ----------------------------------------------------------------------------------------------------------------------
// Frames are denoised in the chunks they are staged in: a chunk's host frames (not device frames: they are read where they lie)
// and its workspace share the staging budget, so an image costs stage_bytes + workspace bytes of it.  Without a technique this is
// stage_plan itself.
inline size_t dn_stage_bytes(size_t frame_bytes, bool on_dev, const DenoiseLayout& L) {  // of a frame in its chunk's slot
  return on_dev ? 0 : (L.img_bytes ? dn_align(frame_bytes) : frame_bytes);
}
inline StagePlan dn_stage_plan(int n_img, size_t frame_bytes, bool on_dev, const DenoiseLayout& L, size_t budget = STAGE_SLOT_BUDGET) {
  return stage_plan(n_img, dn_stage_bytes(frame_bytes, on_dev, L) + L.img_bytes, budget, STAGE_RING);
}

}  // namespace gpet
