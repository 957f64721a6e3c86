// Part of gpet_kernels.hip (included there, inside namespace gpet): a0: split-Bregman total-variation denoising of raw frames, the
// reference's gpet_utils.denoise 'tvb' = scikit-image 0.18.3's denoise_tv_bregman for a 2-D frame.  The arithmetic, its order, the
// skewed layout and the order of acc: gpet_tvb_plan.h.
// ---------------------------------------------------------------------------------------
// Image blockIdx.z of a launch is frame img0 + blockIdx.z of the device pointer tables and of the states, and workspace
// blockIdx.z of the chunk (`stride` doubles apart): u | dx | dy | bx | by | image, each (M + 2)(N + 2) doubles, skewed.

// Prologue: frame -> workspace.  One thread per cell of the padded frame, the ring included.
template <typename T>
__global__ void __launch_bounds__(TVB_THREADS) k_tvb_unpack(const T* const* __restrict__ src, int img0, double* __restrict__ ws, size_t stride,
                                                            int M, int N, double scale) {
#pragma clang fp contract(off)
  const int P = M + 2, Q = N + 2;
  const size_t cells = (size_t)P * Q, e = (size_t)blockIdx.x * TVB_THREADS + threadIdx.x;
  if (e >= cells) return;
  const int R = (int)(e / Q), C = (int)(e - (size_t)R * Q);
  const T* __restrict__ img = src[img0 + blockIdx.z];
  const bool in_r = R >= 1 && R <= M, in_c = C >= 1 && C <= N;
  // (the ring, as the library writes it: above and left the image's row / column of index 1, below and right its last; corners 0)
  const int r = R < 1 ? 1 : (R > M ? M - 1 : R - 1), c = C < 1 ? 1 : (C > N ? N - 1 : C - 1);
  const double v = (in_r || in_c) ? wv_unit<T>(img[(size_t)r * N + c], scale) : 0.0;
  double* f = ws + (size_t)blockIdx.z * stride;
  const size_t at = tvb_index(P, Q, R, C);
  f[TVB_U * cells + at] = v;
  f[TVB_DX * cells + at] = 0.0;
  f[TVB_DY * cells + at] = 0.0;
  f[TVB_BX * cells + at] = 0.0;
  f[TVB_BY * cells + at] = 0.0;
  f[TVB_IMG * cells + at] = (in_r && in_c) ? v : 0.0;
}

// Epilogue: u[1:M+1, 1:N+1] -> dst[img0 + z] (f64, M x N).
__global__ void __launch_bounds__(TVB_THREADS) k_tvb_out(const double* __restrict__ ws, size_t stride, double* const* __restrict__ dst, int img0,
                                                         int M, int N) {
  const size_t e = (size_t)blockIdx.x * TVB_THREADS + threadIdx.x;
  if (e >= (size_t)M * N) return;
  const int r = (int)(e / N), c = (int)(e - (size_t)r * N);
  dst[img0 + blockIdx.z][e] = ws[(size_t)blockIdx.z * stride + tvb_index(M + 2, N + 2, r + 1, c + 1)];
}

// What a cell reads from device memory; none of it depends on the step before, so the loads of a lane's cells of diagonal d + 1
// are issued during step d.  Nothing a load reads is written while it can be in flight: the cell's own values are written by the
// same lane one step later, the u of diagonal d + 2 two steps later, and ul / uu are loaded for ring cells only, which are never
// written; a lane without a cell on the diagonal loads nothing.
struct TvbIn {
  double up, dxo, dyo, bxo, byo, im, ur, ud, ul, uu;  // ul / uu: the ring's u left of column 1 / above row 1 (else unused)
  size_t at;
};
__device__ inline TvbIn tvb_load(const double* f, size_t cells, int P, int Q, int N, int d, int k) {
  TvbIn in;
  const int r0 = d - N > 1 ? d - N : 1, R = r0 + k, C = d - R;
  const size_t i0 = tvb_diag_off(P, Q, d) + (size_t)(R - tvb_diag_first(P, Q, d));
  const size_t i1 = tvb_diag_off(P, Q, d + 1) + (size_t)(R - tvb_diag_first(P, Q, d + 1));  // (R, C + 1); (R + 1, C) follows it
  in.at = i0;
  in.up = f[TVB_U * cells + i0];
  in.dxo = f[TVB_DX * cells + i0];
  in.dyo = f[TVB_DY * cells + i0];
  in.bxo = f[TVB_BX * cells + i0];
  in.byo = f[TVB_BY * cells + i0];
  in.im = f[TVB_IMG * cells + i0];
  in.ur = f[TVB_U * cells + i1];
  in.ud = f[TVB_U * cells + i1 + 1];
  in.ul = 0.0;
  in.uu = 0.0;
  if (C == 1 || R == 1) {
    const size_t im1 = tvb_diag_off(P, Q, d - 1) + (size_t)(R - tvb_diag_first(P, Q, d - 1));  // (R, C - 1); (R - 1, C) precedes it
    if (C == 1) in.ul = f[TVB_U * cells + im1];
    if (R == 1) in.uu = f[TVB_U * cells + im1 - 1];
  }
  return in;
}

// The barrier of a step: it orders the LDS hand-over only and does not wait for the step's stores to device memory.  (What one
// lane wrote to device memory in a sweep is read by other lanes in the NEXT sweep only, behind the __syncthreads of the sweep's end.)
__device__ inline void tvb_step_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Up to TVB_SWEEPS_PER_LAUNCH sweeps of every frame that is not done; one workgroup per frame, no workgroup waits on another.
// CPL: the cells a lane owns of the longest diagonal (tvb_cells_per_lane); the loads of all of them for diagonal d + 1 are in
// flight while the lane computes diagonal d.
// LDS (dynamic, tvb_lds_bytes, and nothing besides): [2][5][L] the new u, dx, bx, dy, by of a diagonal by position (row - first
// interior row), L = min(M, N) | part [TVB_THREADS]: the lanes' sums of acc, and after their tree part[1] = whether another sweep follows.
template <int CPL>
__global__ void __launch_bounds__(TVB_THREADS) k_tvb_sweeps(double* __restrict__ ws, size_t stride, TvbState* __restrict__ state, int img0, int M,
                                                            int N, double lam, double weight, double norm, double inv_lam, double eps,
                                                            int max_iter, int isotropic) {
#pragma clang fp contract(off)
  extern __shared__ double s_tvb[];
  TvbState* st = state + img0 + blockIdx.z;
  if (st->done) return;
  const int tid = threadIdx.x, P = M + 2, Q = N + 2, L = M < N ? M : N;
  const size_t cells = (size_t)P * Q;
  double* f = ws + (size_t)blockIdx.z * stride;
  double* s_part = s_tvb + 10 * L;
  const double total = (double)((long long)M * N);
  int n_iter = st->n_iter;
  for (int sweep = 0; sweep < TVB_SWEEPS_PER_LAUNCH; ++sweep) {
    double p = 0.0;
    int cur = 0;
    TvbIn nxt[CPL] = {};
    if (tid == 0) nxt[0] = tvb_load(f, cells, P, Q, N, 2, 0);
    for (int d = 2; d <= M + N; ++d) {
      const int r0 = d - N > 1 ? d - N : 1, r1 = d - 1 < M ? d - 1 : M, cnt = r1 - r0 + 1;
      const int r0p = d - 1 - N > 1 ? d - 1 - N : 1;  // the first interior row of diagonal d - 1
      double* s_cur = s_tvb + cur * 5 * L;
      const double* s_prev = s_tvb + (cur ^ 1) * 5 * L;
      TvbIn in[CPL];
#pragma unroll
      for (int j = 0; j < CPL; ++j) in[j] = nxt[j];
      if (d < M + N) {
        const int r0n = d + 1 - N > 1 ? d + 1 - N : 1, r1n = d < M ? d : M;
#pragma unroll
        for (int j = 0; j < CPL; ++j)
          if (tid + j * TVB_THREADS <= r1n - r0n) nxt[j] = tvb_load(f, cells, P, Q, N, d + 1, tid + j * TVB_THREADS);
      }
#pragma unroll
      for (int j = 0; j < CPL; ++j) {  // (ascending k: the order of the lane's sum)
        const int k = tid + j * TVB_THREADS;
        if (k >= cnt) break;
        const int R = r0 + k, C = d - R;
        double ul = in[j].ul, dxl = 0.0, bxl = 0.0, uu = in[j].uu, dyu = 0.0, byu = 0.0;
        if (C > 1) {
          const int q = R - r0p;
          ul = s_prev[q];
          dxl = s_prev[L + q];
          bxl = s_prev[2 * L + q];
        }
        if (R > 1) {
          const int q = R - 1 - r0p;
          uu = s_prev[q];
          dyu = s_prev[3 * L + q];
          byu = s_prev[4 * L + q];
        }
        const TvbCellOut o = tvb_cell(in[j].up, in[j].dxo, in[j].dyo, in[j].bxo, in[j].byo, in[j].im, in[j].ur, in[j].ud, ul, dxl, bxl, uu, dyu,
                                      byu, lam, weight, norm, inv_lam, isotropic);
        s_cur[k] = o.u;
        s_cur[L + k] = o.dx;
        s_cur[2 * L + k] = o.bx;
        s_cur[3 * L + k] = o.dy;
        s_cur[4 * L + k] = o.by;
        f[TVB_U * cells + in[j].at] = o.u;
        f[TVB_DX * cells + in[j].at] = o.dx;
        f[TVB_DY * cells + in[j].at] = o.dy;
        f[TVB_BX * cells + in[j].at] = o.bx;
        f[TVB_BY * cells + in[j].at] = o.by;
        p = p + o.diff2;
      }
      tvb_step_barrier();
      cur ^= 1;
    }
    // the sweep's end: acc in the plan's order, the stopping rule, and every lane's writes of this sweep made visible to the others
    s_part[tid] = p;
    __syncthreads();
    for (int s = TVB_THREADS / 2; s > 0; s /= 2) {
      if (tid < s) s_part[tid] = s_part[tid] + s_part[tid + s];
      __syncthreads();
    }
    ++n_iter;
    if (tid == 0) {
      const double acc = s_part[0];
      const bool go = tvb_goes_on(acc, total, eps, n_iter, max_iter);
      st->acc = acc;
      st->n_iter = n_iter;
      st->done = go ? 0 : 1;
      s_part[1] = go ? 1.0 : 0.0;  // (part[1] went into part[0] in the tree's last step)
    }
    __syncthreads();
    if (s_part[1] == 0.0) return;  // (part is written again only behind the next sweep's step barriers)
  }
}
