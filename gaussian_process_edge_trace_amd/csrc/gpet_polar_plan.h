// Polar unwrap of raw frames: the rule that resamples an M x N frame to (radius x angle) around a centre, as plain
// data and plain arithmetic.  No HIP: the host compiler alone builds this header (tests/test_polar_plan.py compiles it into a shim
// with -ffp-contract=off), and k_polar calls polar_angle / polar_sample on the device.  No library function defines the arithmetic:
// this header does, and tests/polar_ref.py restates it with numpy float64.
//
// A spec is (cx, cy) per frame -- x the column, y the row --, r0 >= 0, dr > 0, n_r >= 1, n_theta >= 4, 0 <= pad <= n_theta and the
// tables cos_t, sin_t [n_theta]: cos and sin of theta0 + 2 pi j / n_theta, made on the HOST and handed over as data (the device never
// evaluates a trigonometric function).  Positive angles run clockwise on the screen: rows grow downwards.
//   output       one f64 frame of n_r rows and W = n_theta + 1 + 2 pad columns
//   column c     holds angle index a(c) = (c - pad) mod n_theta, non-negative: columns pad and pad + n_theta are the same ray, and
//                the pad columns either side repeat the far end, so filters see periodic data at the seam
//   position     rho = r0 + i dr;  x = cx + rho cos_t[a];  y = cy + rho sin_t[a]  -- one multiply and one add each, f64, NOT contracted
//   clamp        x = min(max(x, 0), N - 1), y = min(max(y, 0), M - 1): a ray that leaves the frame repeats the border pixel
//   taps         x0 = min(floor(x), N - 2), fx = x - x0; y0, fy likewise (frames are at least 2 x 2)
//   value        top = (1 - fx) p[y0, x0] + fx p[y0, x0 + 1];  bot the same on row y0 + 1;  out = (1 - fy) top + fy bot, in this order,
//                pixels of u8 / u16 / f32 frames widened exactly to f64 first
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gpet_conv_plan.h"  // pixel types

#if defined(__HIPCC__)
#define GPET_POLAR_HD __host__ __device__
#else
#define GPET_POLAR_HD
#endif
// (no fused multiply-add in the functions the kernel shares with the host, whatever the compiler's default)
#if defined(__clang__)
#define GPET_POLAR_NO_FMA _Pragma("clang fp contract(off)")
#else
#define GPET_POLAR_NO_FMA
#endif

namespace gpet {

constexpr int POLAR_THREADS = 256;              // one thread per output pixel, lanes along c
constexpr int POLAR_NTHETA_MIN = 4;
constexpr long long POLAR_CELLS_MAX = 1LL << 28;  // W n_r: an unwrapped frame's bytes (8 each) stay within 2^31
constexpr int POLAR_CHUNK_MAX = 65535;          // frames per launch (gridDim.z)

struct PolarSpec {
  double r0, dr;
  int n_r, n_theta, pad;
};

inline long long polar_width(int n_theta, int pad) { return (long long)n_theta + 1 + 2LL * pad; }

// a(c) for 0 <= c < W (c - pad >= -n_theta: one correction suffices)
GPET_POLAR_HD inline int polar_angle(int c, int pad, int n_theta) {
  const int a = (c - pad) % n_theta;
  return a < 0 ? a + n_theta : a;
}

// The refusals, in the order they are checked: nullptr when the spec can be unwrapped with.  cx, cy: n_centres values each (1: all
// frames share the centre; else one per frame of the n_img)
inline const char* polar_check(const PolarSpec& s, int pix, int M, int N, int n_centres, int n_img, const double* cx, const double* cy) {
  if (!pix_bytes(pix)) return "polar: unknown pixel type";
  if (M < 2 || N < 2) return "polar: frames must be at least 2 x 2 pixels";
  if (s.n_r < 1) return "polar: n_r must be at least 1";
  if (s.n_theta < POLAR_NTHETA_MIN) return "polar: n_theta must be at least 4";
  if (s.pad < 0 || s.pad > s.n_theta) return "polar: pad must lie in [0, n_theta]";
  if (!(s.r0 >= 0.0 && s.r0 < INFINITY)) return "polar: r0 must be finite and at least 0";
  if (!(s.dr > 0.0 && s.dr < INFINITY)) return "polar: dr must be finite and above 0";
  if (polar_width(s.n_theta, s.pad) > POLAR_CELLS_MAX / s.n_r) return "polar: the unwrapped frame exceeds 2^28 pixels (n_r * (n_theta + 1 + 2 * pad))";
  if (n_centres != 1 && n_centres != n_img) return "polar: one centre for all frames or one per frame";
  if (!cx || !cy) return "polar: the centres are a null pointer";
  for (int g = 0; g < n_centres; ++g)
    if (!(fabs(cx[g]) < INFINITY && fabs(cy[g]) < INFINITY)) return "polar: a centre is not finite";
  return nullptr;
}

// the clamped sample coordinate of one axis: centre + rho * t, into [0, extent - 1]
GPET_POLAR_HD inline double polar_coord(double centre, double rho, double t, int extent) {
  GPET_POLAR_NO_FMA
  const double prod = rho * t;
  double v = centre + prod;
  v = v > 0.0 ? v : 0.0;  // max(v, 0)
  const double hi = (double)(extent - 1);
  return v < hi ? v : hi;  // min(v, extent - 1)
}

// the bilinear value at the clamped position (x, y) of frame p [M x N]
template <typename T>
GPET_POLAR_HD inline double polar_bilinear(const T* p, int M, int N, double x, double y) {
  GPET_POLAR_NO_FMA
  const double xf = floor(x), yf = floor(y);
  const int x0 = (int)xf < N - 2 ? (int)xf : N - 2, y0 = (int)yf < M - 2 ? (int)yf : M - 2;
  const double fx = x - (double)x0, fy = y - (double)y0;
  const T* r0 = p + (size_t)y0 * (size_t)N + (size_t)x0;
  const T* r1 = r0 + N;
  const double p00 = (double)r0[0], p01 = (double)r0[1], p10 = (double)r1[0], p11 = (double)r1[1];
  const double gx = 1.0 - fx, gy = 1.0 - fy;
  const double t0 = gx * p00, t1 = fx * p01, top = t0 + t1;
  const double b0 = gx * p10, b1 = fx * p11, bot = b0 + b1;
  const double u = gy * top, w = fy * bot;
  return u + w;
}

// output pixel (i, c) of a frame with centre (cx, cy)
template <typename T>
GPET_POLAR_HD inline double polar_sample(const T* p, int M, int N, double cx, double cy, const PolarSpec& s, const double* cos_t,
                                         const double* sin_t, int i, int c) {
  GPET_POLAR_NO_FMA
  const int a = polar_angle(c, s.pad, s.n_theta);
  const double step = (double)i * s.dr;
  const double rho = s.r0 + step;
  return polar_bilinear(p, M, N, polar_coord(cx, rho, cos_t[a], N), polar_coord(cy, rho, sin_t[a], M));
}

// ---- the launch: blockIdx.x over the n_r W pixels of a frame in row-major order, blockIdx.z the frame of the chunk ----------------
inline unsigned int polar_blocks(const PolarSpec& s) {
  const long long cells = polar_width(s.n_theta, s.pad) * s.n_r;
  return (unsigned int)((cells + POLAR_THREADS - 1) / POLAR_THREADS);
}

}  // namespace gpet
