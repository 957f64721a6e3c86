// Endpoint tracking: the rule that moves an edge's init points onto the edge of the image the edge reads now, as plain
// data and plain arithmetic.  No HIP: the host compiler alone builds this header (tests/test_init_plan.py compiles it into a shim), and
// k_init_follow calls init_score / init_better on the device.
//
// G is the image the edge reads (EdgeDev::grad: M x N, f32 -- the H x N slot of a banded batch, init rows then in band coordinates), an
// init point is (x, y), window = w >= 0 rows, cols = a >= 0 columns on either side:
//   candidates   r in [max(0, y - w), min(M - 1, y + w)]
//   score        s(r) = sum over c = max(0, x - a) .. min(N - 1, x + a) of (double)G[r][c], added in ascending c
//   a candidate counts when s(r) > 0.0 (NaN fails the comparison); none counts: y stays
//   else the new row is the candidate of largest s; ties: the smallest |r - y|, then the smallest r
// x never changes.  Every init point of every edge is moved, interior ones included.  w = 0 moves nothing.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GPET_INIT_HD __host__ __device__
#else
#define GPET_INIT_HD
#endif

namespace gpet {

constexpr long long INIT_WINDOW_MAX = 4096;
constexpr long long INIT_COLS_MAX = 64;

// The refusals, in the order they are checked: nullptr when (window, cols) can be followed with.
inline const char* init_follow_check(long long window, long long cols) {
  if (window < 0) return "init_follow: window must be at least 0 rows";
  if (window > INIT_WINDOW_MAX) return "init_follow: window exceeds 4096 rows";
  if (cols < 0) return "init_follow: cols must be at least 0 columns";
  if (cols > INIT_COLS_MAX) return "init_follow: cols exceeds 64 columns";
  return nullptr;
}

// s(r): the f64 sum of row r over the clipped column window of x, ascending c (additions only: nothing a compiler could contract)
GPET_INIT_HD inline double init_score(const float* G, long long N, long long r, long long x, long long cols) {
  const long long c_lo = x - cols < 0 ? 0 : x - cols;
  const long long c_hi = x + cols > N - 1 ? N - 1 : x + cols;
  double s = 0.0;
  for (long long c = c_lo; c <= c_hi; ++c) s += (double)G[(size_t)r * (size_t)N + (size_t)c];
  return s;
}

// The rule's ordering: does candidate (s, d = |r - y|, r) beat (bs, bd, br)?  A candidate that does not count (s > 0.0 fails) beats
// nothing and is beaten by every one that counts; bs = 0.0 stands for "none so far".
GPET_INIT_HD inline bool init_better(double s, long long d, long long r, double bs, long long bd, long long br) {
  if (!(s > 0.0)) return false;
  if (!(bs > 0.0)) return true;
  if (s != bs) return s > bs;
  if (d != bd) return d < bd;
  return r < br;
}

// The rule for one init point, serially (the host's form; the kernel spreads the candidates over a wave and reduces with init_better)
GPET_INIT_HD inline long long init_follow_row(const float* G, long long M, long long N, long long x, long long y, long long window,
                                              long long cols) {
  const long long r_lo = y - window < 0 ? 0 : y - window;
  const long long r_hi = y + window > M - 1 ? M - 1 : y + window;
  double bs = 0.0;
  long long bd = 0, br = y;
  for (long long r = r_lo; r <= r_hi; ++r) {
    const double s = init_score(G, N, r, x, cols);
    const long long d = r < y ? y - r : r - y;
    if (init_better(s, d, r, bs, bd, br)) {
      bs = s;
      bd = d;
      br = r;
    }
  }
  return bs > 0.0 ? br : y;
}

}  // namespace gpet
