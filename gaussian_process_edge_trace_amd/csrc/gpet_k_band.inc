// Tracking bands (gpet_band_plan.h, DESIGN section 11): the kernels a banded batch runs in addition -- placement of every edge's band from
// the last converged fits, the move of the slots to the placed bands, and the image step that reads a slot's band out of the full-frame
// gradient image.  The int64 tables (r0 of the slots, r0 placed, r0 of the last fits, init rows) live in device memory the batch owns;
// every r0 the kernels use is loaded from them, so the host waits nowhere between placement, swap and warm start.

// One wave per destination edge e = blockIdx.x.  The source's trace in full-frame rows is t[k] = rint(mean_s[k]) + r0_fit[s] over the
// DESTINATION's columns k < Lg (source and destination share the x-grid: warm_from_check / the group table, as for k_warm_start_src) --
// or the int64 consensus row of e's group plus the group's r0_fit.  Entries that are NaN or outside [0, M - 1] are ignored; min and max of
// the rest are reduced across the wave (a ballot says whether any is left), lane 0 applies band_place and stores r0_pend[e] -- plain
// stores, the wave's own entry alone.  Nothing left, no source, or the edge itself stopped with an error: r0_pend[e] = r0_cur[e].
// Of other edges this reads the EdgeDev entry and fin_out only, never their gpet_scalars (the discipline above k_warm_start_src); the
// status read is the wave's OWN edge's, and only where the edge is its own source.
__global__ void __launch_bounds__(64) k_band_place(const EdgeDev* __restrict__ edges, int B, const int32_t* __restrict__ src,
                                                   const int32_t* __restrict__ group_of, const char* __restrict__ kept, long long record_bytes,
                                                   long long off_trace, long long M, const long long* __restrict__ r0_fit,
                                                   const long long* __restrict__ r0_cur, const long long* __restrict__ lohi,
                                                   long long* __restrict__ r0_pend) {
  const int e = blockIdx.x;
  const EdgeDev E = edges[e];
  const int lane = threadIdx.x;
  const int s = src ? src[e] : e;  // (uniform over the wave)
  const double* __restrict__ mean = nullptr;
  const long long* __restrict__ cons = nullptr;
  if (s >= 0 && s < B) mean = edges[s].fin_out;
  else if (s == WARM_SRC_CONSENSUS && kept && group_of && group_of[e] >= 0)
    cons = reinterpret_cast<const long long*>(kept + (size_t)group_of[e] * (size_t)record_bytes + (size_t)off_trace);
  if (s == e && E.sc->status != GPET_OK) mean = nullptr;
  const long long r0s = (mean || cons) ? r0_fit[mean ? s : e] : 0;
  const double y_hi = (double)(M - 1);
  int lo = 0x7fffffff, hi = -1;  // (rows of a frame fit an int: M <= 2^31 - 1)
  bool any = false;
  if (mean || cons) {
    for (int k = lane; k < E.Lg; k += WAVE) {
      double t;
      if (mean) t = rint(mean[k]) + (double)r0s;  // (NaN fails both comparisons; integers below 2^53 add exactly)
      else {
        const long long c = cons[2 * k];
        t = c < -(1ll << 40) ? -1.0 : (double)(c + r0s);  // (INT64_MIN: the median was NaN)
      }
      if (t >= 0.0 && t <= y_hi) {
        const int ti = (int)t;
        lo = ti < lo ? ti : lo;
        hi = ti > hi ? ti : hi;
        any = true;
      }
    }
  }
  const bool left = __ballot(any) != 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = min(lo, __shfl_xor(lo, o, WAVE));
    hi = max(hi, __shfl_xor(hi, o, WAVE));
  }
  if (lane == 0) r0_pend[e] = left ? band_place(M, (long long)E.M, lo, hi, lohi[2 * e], lohi[2 * e + 1]) : r0_cur[e];
}

// The slots move to the placed bands: thread per edge, r0_cur[e] = r0_pend[e] and the edge's init rows in band coordinates,
// init_full - r0 (the x stay).  Each thread writes its own edge's entries alone.
__global__ void __launch_bounds__(256) k_band_apply(const EdgeDev* __restrict__ edges, int B, int n_init_max, const long long* __restrict__ r0_pend,
                                                    const long long* __restrict__ init_full, long long* __restrict__ r0_cur) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B) return;
  const long long r0 = r0_pend[e];
  r0_cur[e] = r0;
  long long* dst = const_cast<long long*>(edges[e].init_xy);
  const long long* full = init_full + (size_t)e * 2 * (size_t)n_init_max;
  for (int i = 0; i < edges[e].n_init; ++i) dst[2 * i + 1] = full[2 * i + 1] - r0;
}

// The image step of a banded slot, part 1: k_minmax_f32 over the band of edge e = blockIdx.y -- the H * N floats at G_of[e] + r0_cur[e] * N
// of its full-frame gradient image -- into the edge's (min, max) slot.  The band's base is 4-byte aligned and no more (N = 65: a row is
// 260 bytes), so every load is one float wide.
__global__ void k_band_minmax(const float* const* __restrict__ G_of, const long long* __restrict__ r0_cur, int N, size_t count,
                              unsigned int* minmax) {
  const int e = blockIdx.y;
  const float* __restrict__ in = G_of[e] + (size_t)r0_cur[e] * (size_t)N;
  unsigned int kmin = 0xFFFFFFFFu, kmax = 0u;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned int k = f32_order_key(in[i]);
    kmin = min(kmin, k);
    kmax = max(kmax, k);
  }
  wave_minmax_commit(kmin, kmax, threadIdx.x, &minmax[2 * (size_t)e], &minmax[2 * (size_t)e + 1]);
}

// Part 2: k_normalise_f32 of the same band into the edge's own image slot (EdgeDev::grad, H x N in the arena) -- the re-normalisation an
// unbanded batch applies to the cropped image (gpet.py:97), the same two operations per pixel.
__global__ void k_band_normalise(const EdgeDev* __restrict__ edges, const float* const* __restrict__ G_of, const long long* __restrict__ r0_cur,
                                 int N, size_t count, const unsigned int* __restrict__ minmax) {
  const int e = blockIdx.y;
  const float* __restrict__ in = G_of[e] + (size_t)r0_cur[e] * (size_t)N;
  float* __restrict__ out = const_cast<float*>(edges[e].grad);
  const float mn = f32_from_key(minmax[2 * (size_t)e]);
  const float mx = f32_from_key(minmax[2 * (size_t)e + 1]);
  const float span = mx - mn;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
    out[i] = f32_min_span(in[i], mn, span);
}

hipError_t launch_band_place(hipStream_t st, const EdgeDev* d_edges, int B, const int32_t* d_src, const int32_t* d_group_of, const char* d_kept,
                             long long record_bytes, long long off_trace, long long M, const long long* d_r0_fit, const long long* d_r0_cur,
                             const long long* d_lohi, long long* d_r0_pend) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_band_place, dim3(B), dim3(64), 0, st, d_edges, B, d_src, d_group_of, d_kept, record_bytes, off_trace, M, d_r0_fit,
                     d_r0_cur, d_lohi, d_r0_pend);
  return hipGetLastError();
}

hipError_t launch_band_apply(hipStream_t st, const EdgeDev* d_edges, int B, int n_init_max, const long long* d_r0_pend,
                             const long long* d_init_full, long long* d_r0_cur) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_band_apply, dim3(cdiv(B, 256)), dim3(256), 0, st, d_edges, B, n_init_max, d_r0_pend, d_init_full, d_r0_cur);
  return hipGetLastError();
}

// min / max and normalisation of every edge's band, edges in launches of at most 65535 (the grid's y extent); d_minmax [2 B] holds the
// reset values (0xFFFFFFFF, 0) when this is enqueued
hipError_t launch_band_images(hipStream_t st, const EdgeDev* d_edges, int B, const float* const* d_G_of, const long long* d_r0_cur, int H,
                              int N, unsigned int* d_minmax) {
  const size_t count = (size_t)H * (size_t)N;
  size_t blocks = (count + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  (void)hipGetLastError();
  for (int i = 0; i < B; i += 65535) {
    const int n = B - i < 65535 ? B - i : 65535;
    hipLaunchKernelGGL(k_band_minmax, dim3((unsigned)blocks, n), dim3(256), 0, st, d_G_of + i, d_r0_cur + i, N, count, d_minmax + 2 * (size_t)i);
    hipLaunchKernelGGL(k_band_normalise, dim3((unsigned)blocks, n), dim3(256), 0, st, d_edges + i, d_G_of + i, d_r0_cur + i, N, count,
                       d_minmax + 2 * (size_t)i);
  }
  return hipGetLastError();
}

hipError_t launch_warm_start_band(hipStream_t st, EdgeDev* d_edges, int B, const int32_t* d_src, const int32_t* d_group_of, const char* d_kept,
                                  long long record_bytes, long long off_trace, int warm_every, const long long* d_r0_fit,
                                  const long long* d_r0_cur) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_warm_start_src<true>, dim3(B), dim3(64), 0, st, d_edges, B, d_src, d_group_of, d_kept, record_bytes, off_trace, warm_every,
                     d_r0_fit, d_r0_cur);
  return hipGetLastError();
}
