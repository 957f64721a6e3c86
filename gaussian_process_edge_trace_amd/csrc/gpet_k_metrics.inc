// Part of gpet_kernels.hip (included there, inside namespace gpet): the denoise quality metrics of frame pairs -- the sums under PSNR /
// NRMSE, the SSIM map and its cropped sum, the counts behind the Shannon entropy.  The arithmetic, the one summation order and the method
// of the counts: gpet_metrics_plan.h.
// ---------------------------------------------------------------------------------------
// Pair blockIdx.z of a launch is pair img0 + blockIdx.z of the device pointer table (tab[2 g] = a, tab[2 g + 1] = b) and of the records,
// and workspace blockIdx.z of the chunk (`stride` bytes apart): five intermediate planes | S, f64 M x N each; the sort's keys lie over
// the planes once S is made.

__device__ inline double metrics_px(const void* __restrict__ p, int pix, size_t i) {
  switch (pix) {
    case PIX_U8: return (double)static_cast<const unsigned char*>(p)[i];
    case PIX_U16: return (double)static_cast<const unsigned short*>(p)[i];
    case PIX_F32: return (double)static_cast<const float*>(p)[i];
    default: return static_cast<const double*>(p)[i];
  }
}

// lane sums -> the tree of metrics_sum; the result in every lane
__device__ inline double metrics_tree(double p, double* s_part) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  __syncthreads();  // (s_part may still be read from the tree before)
  s_part[tid] = p;
  __syncthreads();
  for (int s = METRICS_THREADS / 2; s > 0; s /= 2) {
    if (tid < s) s_part[tid] = s_part[tid] + s_part[tid + s];
    __syncthreads();
  }
  return s_part[0];
}

// Pair pass: squared differences in the working type, their sum, a's extremes.  One workgroup per pair.
__global__ void __launch_bounds__(METRICS_THREADS) k_metrics_pair(const void* const* __restrict__ tab, MetricsAcc* __restrict__ acc, int img0,
                                                                  int pix_a, int pix_b, long long px) {
#pragma clang fp contract(off)
  __shared__ double s_part[METRICS_THREADS], s_min[METRICS_THREADS], s_max[METRICS_THREADS];
  const int g = img0 + blockIdx.z, tid = threadIdx.x;
  const void* __restrict__ a = tab[2 * g];
  const void* __restrict__ b = tab[2 * g + 1];
  const bool f64 = metrics_work_f64(pix_a, pix_b);
  double p = 0.0, mn = INFINITY, mx = -INFINITY;
  for (long long i = tid; i < px; i += METRICS_THREADS) {
    const double av = metrics_px(a, pix_a, (size_t)i), bv = metrics_px(b, pix_b, (size_t)i);
    p = p + metrics_sqdiff(av, bv, f64);
    mn = av < mn ? av : mn;
    mx = av > mx ? av : mx;
  }
  s_min[tid] = mn;
  s_max[tid] = mx;
  const double sum = metrics_tree(p, s_part);
  for (int s = METRICS_THREADS / 2; s > 0; s /= 2) {
    if (tid < s) {
      s_min[tid] = s_min[tid + s] < s_min[tid] ? s_min[tid + s] : s_min[tid];
      s_max[tid] = s_max[tid + s] > s_max[tid] ? s_max[tid + s] : s_max[tid];
    }
    __syncthreads();
  }
  if (tid == 0) {
    acc[g].sq_sum = sum;
    acc[g].a_min = s_min[0];
    acc[g].a_max = s_max[0];
  }
}

// SSIM, axis 0: one lane per column follows the five running sums down the frame; the samples are formed from a and b on the fly.
__global__ void __launch_bounds__(METRICS_COLS) k_metrics_axis0(const void* const* __restrict__ tab, int img0, int pix_a, int pix_b, int M, int N,
                                                                int w, char* __restrict__ ws, size_t stride) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * METRICS_COLS + threadIdx.x;
  if (c >= N) return;
  const int g = img0 + blockIdx.z, h = w / 2;
  const void* __restrict__ a = tab[2 * g];
  const void* __restrict__ b = tab[2 * g + 1];
  const size_t px = (size_t)M * N;
  double* __restrict__ P = reinterpret_cast<double*>(ws + (size_t)blockIdx.z * stride);
  const double dw = (double)w;
  double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, t4 = 0.0;
  for (int e = 0; e < w; ++e) {
    const size_t at = (size_t)metrics_reflect(e - h, M) * N + c;
    const double x = metrics_px(a, pix_a, at), y = metrics_px(b, pix_b, at);
    const double xx = x * x, yy = y * y, xy = x * y;
    t0 = t0 + x;
    t1 = t1 + y;
    t2 = t2 + xx;
    t3 = t3 + yy;
    t4 = t4 + xy;
  }
  for (int i = 0;; ++i) {
    const size_t o = (size_t)i * N + c;
    P[o] = t0 / dw;
    P[px + o] = t1 / dw;
    P[2 * px + o] = t2 / dw;
    P[3 * px + o] = t3 / dw;
    P[4 * px + o] = t4 / dw;
    if (i + 1 >= M) break;
    const size_t an = (size_t)metrics_reflect(i + w - h, M) * N + c, ao = (size_t)metrics_reflect(i - h, M) * N + c;
    const double xn = metrics_px(a, pix_a, an), yn = metrics_px(b, pix_b, an);
    const double xo = metrics_px(a, pix_a, ao), yo = metrics_px(b, pix_b, ao);
    const double xxn = xn * xn, yyn = yn * yn, xyn = xn * yn, xxo = xo * xo, yyo = yo * yo, xyo = xo * yo;
    t0 = metrics_line_step(t0, xn, xo);
    t1 = metrics_line_step(t1, yn, yo);
    t2 = metrics_line_step(t2, xxn, xxo);
    t3 = metrics_line_step(t3, yyn, yyo);
    t4 = metrics_line_step(t4, xyn, xyo);
  }
}

// a tile of METRICS_ROWS x METRICS_TILE samples of the five planes' extended rows, from extended column e0 on, into LDS: a load covers
// eight rows of eight neighbouring columns.  Samples outside the frame's rows or the extended line are 0 and never used.
__device__ inline void metrics_stage_tile(const double* __restrict__ P, size_t px, int r0, int M, int N, int w, int e0,
                                          double (*tile)[METRICS_ROWS][METRICS_TILE_PITCH]) {
  const int k = threadIdx.x & (METRICS_TILE - 1), rg = threadIdx.x / METRICS_TILE, e = e0 + k, h = w / 2;
  const bool col_ok = e >= 0 && e <= N + w - 2;
  const int sc = col_ok ? metrics_reflect(e - h, N) : 0;
  for (int rr = 0; rr < METRICS_ROWS / (METRICS_ROWS / METRICS_TILE); ++rr) {
    const int row = rr * (METRICS_ROWS / METRICS_TILE) + rg;
    const bool ok = col_ok && r0 + row < M;
    const size_t at = ok ? (size_t)(r0 + row) * N + sc : 0;
    for (int p = 0; p < 5; ++p) tile[p][row][k] = ok ? P[p * px + at] : 0.0;
  }
}

// SSIM, axis 1 and S: one lane per row follows the five running sums along the row of the intermediate planes, whose samples come
// through LDS tiles (the new and the old sample of a step lie w columns apart: two tiles); S of every pixel goes to the S plane
// through LDS as well.
__global__ void __launch_bounds__(METRICS_ROWS) k_metrics_axis1(int M, int N, int w, double cov_norm, double C1, double C2, char* __restrict__ ws,
                                                                size_t stride) {
#pragma clang fp contract(off)
  __shared__ double s_new[5][METRICS_ROWS][METRICS_TILE_PITCH], s_old[5][METRICS_ROWS][METRICS_TILE_PITCH];
  __shared__ double s_S[METRICS_ROWS][METRICS_TILE_PITCH];
  const int lane = threadIdx.x, r0 = blockIdx.x * METRICS_ROWS, r = r0 + lane;
  const size_t px = (size_t)M * N;
  const double* __restrict__ P = reinterpret_cast<const double*>(ws + (size_t)blockIdx.z * stride);
  double* __restrict__ S = reinterpret_cast<double*>(ws + (size_t)blockIdx.z * stride) + 5 * px;
  const double dw = (double)w;
  double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int e0 = 0; e0 < w; e0 += METRICS_TILE) {
    metrics_stage_tile(P, px, r0, M, N, w, e0, s_new);
    __syncthreads();
    for (int k = 0; k < METRICS_TILE && e0 + k < w; ++k)
      for (int p = 0; p < 5; ++p) t[p] = t[p] + s_new[p][lane][k];
    __syncthreads();
  }
  if (r < M) S[(size_t)r * N] = metrics_ssim_S(t[0] / dw, t[1] / dw, t[2] / dw, t[3] / dw, t[4] / dw, cov_norm, C1, C2);
  for (int i0 = 1; i0 < N; i0 += METRICS_TILE) {
    metrics_stage_tile(P, px, r0, M, N, w, i0 + w - 1, s_new);
    metrics_stage_tile(P, px, r0, M, N, w, i0 - 1, s_old);
    __syncthreads();
    for (int k = 0; k < METRICS_TILE && i0 + k < N; ++k) {
      for (int p = 0; p < 5; ++p) t[p] = metrics_line_step(t[p], s_new[p][lane][k], s_old[p][lane][k]);
      s_S[lane][k] = metrics_ssim_S(t[0] / dw, t[1] / dw, t[2] / dw, t[3] / dw, t[4] / dw, cov_norm, C1, C2);
    }
    __syncthreads();
    const int k = lane & (METRICS_TILE - 1), rg = lane / METRICS_TILE;
    for (int rr = 0; rr < METRICS_TILE; ++rr) {
      const int row = rr * (METRICS_ROWS / METRICS_TILE) + rg;
      if (r0 + row < M && i0 + k < N) S[(size_t)(r0 + row) * N + i0 + k] = s_S[row][k];
    }
  }
}

// the sum of S over the crop, in raster order of the crop.  One workgroup per pair.
__global__ void __launch_bounds__(METRICS_THREADS) k_metrics_crop_sum(MetricsAcc* __restrict__ acc, int img0, int M, int N, int pad,
                                                                      const char* __restrict__ ws, size_t stride) {
#pragma clang fp contract(off)
  __shared__ double s_part[METRICS_THREADS];
  const double* __restrict__ S = reinterpret_cast<const double*>(ws + (size_t)blockIdx.z * stride) + (size_t)5 * M * N;
  const long long Nc = N - 2 * pad, nc = (long long)(M - 2 * pad) * Nc;
  double p = 0.0;
  for (long long q = threadIdx.x; q < nc; q += METRICS_THREADS) {
    const long long rr = q / Nc, cc = q - rr * Nc;
    p = p + S[(size_t)(rr + pad) * N + (size_t)(cc + pad)];
  }
  const double sum = metrics_tree(p, s_part);
  if (threadIdx.x == 0) acc[img0 + blockIdx.z].ssim_sum = sum;
}

// entropy: b's keys, padded to the power of two the network sorts
__global__ void __launch_bounds__(METRICS_THREADS) k_metrics_keys(const void* const* __restrict__ tab, int img0, int pix_b, long long px,
                                                                  long long npow2, char* __restrict__ ws, size_t stride) {
  const long long i = (long long)blockIdx.x * METRICS_THREADS + threadIdx.x;
  if (i >= npow2) return;
  uint64_t* __restrict__ keys = reinterpret_cast<uint64_t*>(ws + (size_t)blockIdx.z * stride);
  keys[i] = i < px ? metrics_key(metrics_px(tab[2 * (img0 + blockIdx.z) + 1], pix_b, (size_t)i)) : METRICS_KEY_PAD;
}

// the steps of the bitonic network whose partners lie inside a segment of `seg` keys, in LDS: merge sizes k_first .. k_last, of each
// the distances min(k / 2, seg / 2) .. 1
__global__ void __launch_bounds__(METRICS_THREADS) k_metrics_sort_local(char* __restrict__ ws, size_t stride, int seg, long long k_first,
                                                                        long long k_last) {
  __shared__ uint64_t s_k[METRICS_SORT_SEG];
  const long long base = (long long)blockIdx.x * seg;
  uint64_t* __restrict__ keys = reinterpret_cast<uint64_t*>(ws + (size_t)blockIdx.z * stride) + base;
  for (int t = threadIdx.x; t < seg; t += METRICS_THREADS) s_k[t] = keys[t];
  __syncthreads();
  for (long long k = k_first; k <= k_last; k *= 2)
    for (int j = (int)(k / 2 < seg / 2 ? k / 2 : seg / 2); j >= 1; j /= 2) {
      for (int t = threadIdx.x; t < seg / 2; t += METRICS_THREADS) {
        const int i = (t / j) * 2 * j + (t % j);
        const bool asc = ((base + i) & k) == 0;
        const uint64_t lo = s_k[i], hi = s_k[i + j];
        if ((lo > hi) == asc) {
          s_k[i] = hi;
          s_k[i + j] = lo;
        }
      }
      __syncthreads();
    }
  for (int t = threadIdx.x; t < seg; t += METRICS_THREADS) keys[t] = s_k[t];
}

// one step of the network in global memory: merge size k, distance j
__global__ void __launch_bounds__(METRICS_THREADS) k_metrics_sort_global(char* __restrict__ ws, size_t stride, long long npow2, long long k,
                                                                         long long j) {
  const long long t = (long long)blockIdx.x * METRICS_THREADS + threadIdx.x;
  if (t >= npow2 / 2) return;
  uint64_t* __restrict__ keys = reinterpret_cast<uint64_t*>(ws + (size_t)blockIdx.z * stride);
  const long long i = (t / j) * 2 * j + (t % j);
  const bool asc = (i & k) == 0;
  const uint64_t lo = keys[i], hi = keys[i + j];
  if ((lo > hi) == asc) {
    keys[i] = hi;
    keys[i + j] = lo;
  }
}

// the entropy terms of the runs, summed in the plan's order over the sorted positions.  One workgroup per pair.
__global__ void __launch_bounds__(METRICS_THREADS) k_metrics_entropy(MetricsAcc* __restrict__ acc, int img0, long long px, const char* __restrict__ ws,
                                                                     size_t stride) {
#pragma clang fp contract(off)
  __shared__ double s_part[METRICS_THREADS];
  const uint64_t* __restrict__ keys = reinterpret_cast<const uint64_t*>(ws + (size_t)blockIdx.z * stride);
  double p = 0.0;
  for (long long i = threadIdx.x; i < px; i += METRICS_THREADS)
    if (i == 0 || keys[i] != keys[i - 1]) p = p + metrics_entropy_term(metrics_run_end(keys, i, px) - i, px);
  const double sum = metrics_tree(p, s_part);
  if (threadIdx.x == 0) acc[img0 + blockIdx.z].ent_sum = sum;
}

// Pairs img0 .. img0 + n - 1 of the device pointer table: every kernel above, in order, on one stream.
hipError_t launch_metrics(hipStream_t st, const void* const* d_tab, MetricsAcc* d_acc, int img0, int n, int pix_a, int pix_b, int M, int N,
                          const MetricsSpec& sp, double R_ssim, char* ws, size_t stride) {
  (void)hipGetLastError();
  const long long px = (long long)M * N;
  const MetricsSsimConst k = metrics_ssim_const(sp.win_size, sp.use_sample_covariance, sp.K1, sp.K2, R_ssim);
  const dim3 one(1, 1, n);
  hipLaunchKernelGGL(k_metrics_pair, one, dim3(METRICS_THREADS), 0, st, d_tab, d_acc, img0, pix_a, pix_b, px);
  hipLaunchKernelGGL(k_metrics_axis0, dim3(cdiv(N, METRICS_COLS), 1, n), dim3(METRICS_COLS), 0, st, d_tab, img0, pix_a, pix_b, M, N, sp.win_size, ws,
                     stride);
  hipLaunchKernelGGL(k_metrics_axis1, dim3(cdiv(M, METRICS_ROWS), 1, n), dim3(METRICS_ROWS), 0, st, M, N, sp.win_size, k.cov_norm, k.C1, k.C2, ws,
                     stride);
  hipLaunchKernelGGL(k_metrics_crop_sum, one, dim3(METRICS_THREADS), 0, st, d_acc, img0, M, N, (sp.win_size - 1) / 2, ws, stride);
  return hipGetLastError();
}
// ... and, once whoever wants the S maps has copied them (the keys lie over the planes, not over S): the counts and the entropy sum
hipError_t launch_metrics_entropy(hipStream_t st, const void* const* d_tab, MetricsAcc* d_acc, int img0, int n, int pix_b, int M, int N, char* ws,
                                  size_t stride) {
  (void)hipGetLastError();
  const long long px = (long long)M * N, npow2 = metrics_pow2(px);
  const int seg = (int)(npow2 < METRICS_SORT_SEG ? npow2 : METRICS_SORT_SEG);
  const dim3 thr(METRICS_THREADS), segs((unsigned int)(npow2 / seg), 1, n), half((unsigned int)cdiv((int)(npow2 / 2), METRICS_THREADS), 1, n);
  hipLaunchKernelGGL(k_metrics_keys, dim3((unsigned int)cdiv((int)npow2, METRICS_THREADS), 1, n), thr, 0, st, d_tab, img0, pix_b, px, npow2, ws, stride);
  hipLaunchKernelGGL(k_metrics_sort_local, segs, thr, 0, st, ws, stride, seg, 2LL, (long long)seg);
  for (long long k = 2LL * seg; k <= npow2; k *= 2) {
    for (long long j = k / 2; j >= seg; j /= 2) hipLaunchKernelGGL(k_metrics_sort_global, half, thr, 0, st, ws, stride, npow2, k, j);
    hipLaunchKernelGGL(k_metrics_sort_local, segs, thr, 0, st, ws, stride, seg, k, k);
  }
  hipLaunchKernelGGL(k_metrics_entropy, dim3(1, 1, n), thr, 0, st, d_acc, img0, px, ws, stride);
  return hipGetLastError();
}
