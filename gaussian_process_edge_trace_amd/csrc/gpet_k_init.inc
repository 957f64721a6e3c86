// Endpoint tracking (gpet_init_plan.h, DESIGN section 12): the init points of every edge move onto the edge of the image the edge reads now.

// One wave per edge e = blockIdx.x, a loop over the edge's init points.  For point (x, y) the lanes take the candidate rows
// max(0, y - w) .. min(M - 1, y + w), lane after lane and 64 at a time (2 w + 1 may exceed the wave), each lane forms init_score of its
// rows and keeps its best by init_better; the wave then reduces (s, |r - y|, r) with a butterfly of shuffles -- counted candidates have
// distinct rows, so the order is total and every lane ends with the same winner.  Lane 0 stores the new row into the edge's own
// init_xy[2 i + 1] (plain stores; x stays).  Every load of the image has 0 <= r <= M - 1 and 0 <= c <= N - 1 by the two clips.
// On a banded batch (r0_cur != nullptr) E.M is H, the rows are band rows, and lane 0 also writes two of the tables of gpet_band_plan.h:
// the point in full-frame rows (band row + r0_cur[e]) and the edge's (i_lo, i_hi), so that the next k_band_place clamps against the
// moved points.  The wave reads its own edge's EdgeDev, image and table entries only and writes its own edge's entries alone.
__global__ void __launch_bounds__(64) k_init_follow(const EdgeDev* __restrict__ edges, int window, int cols, int n_init_max,
                                                    const long long* __restrict__ r0_cur, long long* __restrict__ init_full,
                                                    long long* __restrict__ lohi) {
  const int e = blockIdx.x;
  const EdgeDev E = edges[e];
  const int lane = threadIdx.x;
  long long* init = const_cast<long long*>(E.init_xy);
  const long long r0 = r0_cur ? r0_cur[e] : 0;
  long long i_lo = 0, i_hi = 0;
  for (int i = 0; i < E.n_init; ++i) {
    const long long x = init[2 * i], y = init[2 * i + 1];
    const long long r_lo = y - window < 0 ? 0 : y - window;
    const long long r_hi = y + window > (long long)E.M - 1 ? (long long)E.M - 1 : y + window;
    double bs = 0.0;  // (0.0: no candidate counts so far)
    long long bd = 0, br = y;
    for (long long r = r_lo + lane; r <= r_hi; r += WAVE) {
      const double s = init_score(E.grad, E.N, r, x, cols);
      const long long d = r < y ? y - r : r - y;
      if (init_better(s, d, r, bs, bd, br)) {
        bs = s;
        bd = d;
        br = r;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double os = __shfl_xor(bs, o, WAVE);
      const long long od = __shfl_xor(bd, o, WAVE);
      const long long orow = __shfl_xor(br, o, WAVE);
      if (init_better(os, od, orow, bs, bd, br)) {
        bs = os;
        bd = od;
        br = orow;
      }
    }
    const long long y_new = bs > 0.0 ? br : y;
    i_lo = (i == 0 || y_new + r0 < i_lo) ? y_new + r0 : i_lo;
    i_hi = (i == 0 || y_new + r0 > i_hi) ? y_new + r0 : i_hi;
    if (lane == 0) {
      init[2 * i + 1] = y_new;
      if (init_full) init_full[(size_t)e * 2 * (size_t)n_init_max + 2 * (size_t)i + 1] = y_new + r0;
    }
  }
  if (lane == 0 && lohi) {
    lohi[2 * (size_t)e] = i_lo;
    lohi[2 * (size_t)e + 1] = i_hi;
  }
}

hipError_t launch_init_follow(hipStream_t st, const EdgeDev* d_edges, int B, int window, int cols, int n_init_max, const long long* d_r0_cur,
                              long long* d_init_full, long long* d_lohi) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_init_follow, dim3(B), dim3(64), 0, st, d_edges, window, cols, n_init_max, d_r0_cur, d_init_full, d_lohi);
  return hipGetLastError();
}
