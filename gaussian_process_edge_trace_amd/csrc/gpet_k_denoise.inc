// Part of gpet_kernels.hip (included there, inside namespace gpet): a0: denoising of raw frames in front of the gradient-image
// convolution (gpet_utils.py:122-158): median / minimum (scipy.ndimage.median_filter, minimum_filter), Gaussian
// (scipy.ndimage.gaussian_filter) and Chambolle total variation (skimage.restoration.denoise_tv_chambolle).
// ---------------------------------------------------------------------------------------
// Common to all: image i = blockIdx.z of a chunk is frame img0 + i of the device pointer table src; what the kernels write lies in
// the image's block of the chunk's workspace, ws + i * stride (layout: gpet_denoise_plan.h).  f64 arithmetic in the reference's
// order, no FMA contraction.
// ---------------------------------------------------------------------------------------
// position i of an axis of length n continued beyond its ends (dn_extend of gpet_denoise_plan.h)
__device__ __forceinline__ int dn_ext(int i, int n, int mode) {
  if (mode == DN_MODE_NEAREST) return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
  if (i >= 0 && i < n) return i;
  const int period = 2 * n;
  int p = i % period;
  if (p < 0) p += period;
  return p < n ? p : period - 1 - p;
}

// ---- median / minimum -----------------------------------------------------------------------------------------------------------
// Element `rank` of the sorted sy x sx window around every pixel, in the frame's own type (selection is exact).  A workgroup of
// 64 x 4 threads owns 64 columns x 16 rows; its (16 + sy - 1) x (64 + sx - 1) patch of the continued image goes through LDS once.
// Rank 0 is a running minimum.  Otherwise the element is found by counting: v is the answer when fewer than rank + 1 elements are
// below it and at least rank + 1 are not above it.  SY x SX > 0: the window is known at compile time and sits in registers
// (3 x 3, 5 x 5); SY = 0: any window up to 81 pixels, read from LDS.
template <typename T, int SY, int SX>
__global__ void __launch_bounds__(256) k_dn_rank(const T* const* __restrict__ src, int img0, char* __restrict__ ws, size_t stride,
                                                 size_t off_out, int M, int N, int sy_, int sx_, int rank, int mode) {
  extern __shared__ double s_dn[];
  T* s_p = (T*)s_dn;
  const int sy = SY > 0 ? SY : sy_, sx = SY > 0 ? SX : sx_;
  const T* __restrict__ img = src[img0 + blockIdx.z];
  T* __restrict__ out = (T*)(ws + (size_t)blockIdx.z * stride + off_out);
  const int tid = threadIdx.x + threadIdx.y * blockDim.x, nthr = blockDim.x * blockDim.y;
  const int pw = 64 + sx - 1, ph = CONV_RY + sy - 1, oy = sy / 2, ox = sx / 2;
  const int x0 = blockIdx.x * 64, y0 = blockIdx.y * CONV_RY;
  for (int e = tid; e < pw * ph; e += nthr) {
    const int py = e / pw, px = e - py * pw;
    s_p[e] = img[(size_t)dn_ext(y0 + py - oy, M, mode) * N + dn_ext(x0 + px - ox, N, mode)];
  }
  __syncthreads();
  const int x = x0 + threadIdx.x;
  for (int yl = threadIdx.y; yl < CONV_RY; yl += blockDim.y) {
    const int y = y0 + yl;
    if (x >= N || y >= M) continue;
    const T* base = s_p + yl * pw + threadIdx.x;
    T res = base[0];
    if (rank == 0) {
      for (int a = 0; a < sy; ++a)
        for (int b = 0; b < sx; ++b) {
          const T v = base[a * pw + b];
          res = v < res ? v : res;
        }
    } else if (SY > 0) {
      constexpr int NW = SY * SX > 0 ? SY * SX : 1;
      T v[NW];
#pragma unroll
      for (int a = 0; a < SY; ++a)
#pragma unroll
        for (int b = 0; b < SX; ++b) v[a * SX + b] = base[a * pw + b];
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        int lt = 0, le = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
          lt += v[i] < v[j] ? 1 : 0;
          le += v[i] <= v[j] ? 1 : 0;
        }
        if (lt <= rank && rank < le) res = v[j];
      }
    } else {
      for (int a = 0; a < sy; ++a)
        for (int b = 0; b < sx; ++b) {
          const T vj = base[a * pw + b];
          int lt = 0, le = 0;
          for (int a2 = 0; a2 < sy; ++a2)
            for (int b2 = 0; b2 < sx; ++b2) {
              const T vi = base[a2 * pw + b2];
              lt += vi < vj ? 1 : 0;
              le += vi <= vj ? 1 : 0;
            }
          if (lt <= rank && rank < le) res = vj;
        }
    }
    out[(size_t)y * N + x] = res;
  }
}

// ---- gaussian -------------------------------------------------------------------------------------------------------------------
// One pass of scipy's correlate1d with symmetric taps w[2 r + 1] along `axis`, summed in scipy's order:
//   acc = x[0] w[r];  for l = -r .. -1: acc += (x[l] + x[-l]) w[l + r]
// and stored as scipy stores a float64 line into an array of the frame's type: a C cast (f32 rounds, u8 / u16 truncate).
// The first pass reads the frame (src != nullptr), the second the first's output at off_in of the image's block.
template <typename T>
__global__ void __launch_bounds__(256) k_dn_gauss_pass(const T* const* __restrict__ src, int img0, char* __restrict__ ws, size_t stride,
                                                       size_t off_in, size_t off_out, int M, int N, int axis,
                                                       const double* __restrict__ w, int r, int mode) {
#pragma clang fp contract(off)
  char* blk = ws + (size_t)blockIdx.z * stride;
  const T* __restrict__ in = src ? src[img0 + blockIdx.z] : (const T*)(blk + off_in);
  T* __restrict__ out = (T*)(blk + off_out);
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= N || y >= M) return;
  const int n = axis == 0 ? M : N, pos = axis == 0 ? y : x;
  const size_t step = axis == 0 ? (size_t)N : 1, line = axis == 0 ? (size_t)x : (size_t)y * N;
  double acc = (double)in[line + (size_t)pos * step] * w[r];
  for (int l = -r; l < 0; ++l) {
    const double a = (double)in[line + (size_t)dn_ext(pos + l, n, mode) * step];
    const double b = (double)in[line + (size_t)dn_ext(pos - l, n, mode) * step];
    acc = acc + (a + b) * w[l + r];
  }
  out[(size_t)y * N + x] = (T)acc;
}

// ---- tvc ------------------------------------------------------------------------------------------------------------------------
// _denoise_tv_chambolle_nd (skimage restoration/_denoise.py:315-393) for 2-D images, one launch pair per iteration for all
// unfinished images of a chunk.
struct TvcState {
  double E_init, E_prev;
  int done, n_iter;
  double pad_;
};
// what the reference iterates on: u8 / u16 through img_as_float (x times the f64 reciprocal of the type's maximum), f32 promoted
__device__ __forceinline__ double tvc_pixel(unsigned char v) { return (double)v * (1.0 / 255.0); }
__device__ __forceinline__ double tvc_pixel(unsigned short v) { return (double)v * (1.0 / 65535.0); }
__device__ __forceinline__ double tvc_pixel(float v) { return (double)v; }
__device__ __forceinline__ double tvc_pixel(double v) { return v; }

// Iteration `it`: p of iteration it - 1 (planes of parity (it + 1) & 1; zero for it = 0) and the image give
//   d = -(p0 + p1);  d[y] += p0[y - 1];  d[x] += p1[x - 1];  out = image + d
// for the workgroup's 64 x 16 tile and the row below / column right of it (LDS), then the forward differences g, norm =
// sqrt(g0^2 + g1^2), and p = (p - tau g) / (norm (tau / weight) + 1) into the planes of parity it & 1.  `out` is stored; the
// workgroup's sums of d^2 and of norm go to its slots of the image's partials, in a fixed order.
template <typename T>
__global__ void __launch_bounds__(256) k_dn_tvc_iter(const T* const* __restrict__ src, int img0, char* __restrict__ ws, size_t stride,
                                                     size_t off_out, size_t off_p, size_t plane, size_t off_part, int M, int N, int it,
                                                     double tau_w) {
#pragma clang fp contract(off)
  __shared__ double s_o[(CONV_RY + 1) * 65], s_d[(CONV_RY + 1) * 65], s_r[8];
  char* blk = ws + (size_t)blockIdx.z * stride;
  const TvcState* st = (const TvcState*)(blk + off_part);
  if (it > 0 && st->done) return;
  const T* __restrict__ img = src[img0 + blockIdx.z];
  double* __restrict__ out = (double*)(blk + off_out);
  const int par = it & 1;
  const double* __restrict__ pp0 = (const double*)(blk + off_p + (size_t)(2 * (1 - par)) * plane);
  const double* __restrict__ pp1 = (const double*)(blk + off_p + (size_t)(2 * (1 - par) + 1) * plane);
  double* __restrict__ pn0 = (double*)(blk + off_p + (size_t)(2 * par) * plane);
  double* __restrict__ pn1 = (double*)(blk + off_p + (size_t)(2 * par + 1) * plane);
  const int tid = threadIdx.x + threadIdx.y * blockDim.x, nthr = blockDim.x * blockDim.y;
  const int x0 = blockIdx.x * 64, y0 = blockIdx.y * CONV_RY;
  for (int e = tid; e < (CONV_RY + 1) * 65; e += nthr) {
    const int py = e / 65, px = e - py * 65;
    const int y = y0 + py, x = x0 + px;
    double d = 0.0, o = 0.0;
    if (y < M && x < N) {
      const size_t idx = (size_t)y * N + x;
      const double f = tvc_pixel(img[idx]);
      if (it > 0) {
        d = -(pp0[idx] + pp1[idx]);
        if (y > 0) d = d + pp0[idx - N];
        if (x > 0) d = d + pp1[idx - 1];
        o = f + d;
      } else {
        o = f;
      }
    }
    s_o[e] = o;
    s_d[e] = d;
  }
  __syncthreads();
  const double tau = 0.25;
  const int x = x0 + threadIdx.x;
  double sum_d2 = 0.0, sum_n = 0.0;
  for (int yl = threadIdx.y; yl < CONV_RY; yl += blockDim.y) {
    const int y = y0 + yl;
    if (x < N && y < M) {
      const int e = yl * 65 + threadIdx.x;
      const size_t idx = (size_t)y * N + x;
      const double o = s_o[e], d = s_d[e];
      const double g0 = y < M - 1 ? s_o[e + 65] - o : 0.0;
      const double g1 = x < N - 1 ? s_o[e + 1] - o : 0.0;
      const double norm = sqrt(g0 * g0 + g1 * g1);
      sum_d2 = sum_d2 + d * d;
      sum_n = sum_n + norm;
      double nn = norm * tau_w;
      nn = nn + 1.0;
      const double q0 = it > 0 ? pp0[idx] : 0.0, q1 = it > 0 ? pp1[idx] : 0.0;
      pn0[idx] = (q0 - tau * g0) / nn;
      pn1[idx] = (q1 - tau * g1) / nn;
      out[idx] = o;
    }
  }
  // workgroup sums in a fixed order: butterfly inside each wave, then the four waves one after the other
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum_d2 = sum_d2 + __shfl_xor(sum_d2, o, WAVE);
    sum_n = sum_n + __shfl_xor(sum_n, o, WAVE);
  }
  if ((tid & 63) == 0) {
    s_r[tid >> 6] = sum_d2;
    s_r[4 + (tid >> 6)] = sum_n;
  }
  __syncthreads();
  if (tid == 0) {
    double* part = (double*)(blk + off_part + sizeof(TvcState));
    const int n_wg = gridDim.x * gridDim.y, wg = blockIdx.y * gridDim.x + blockIdx.x;
    part[wg] = ((s_r[0] + s_r[1]) + s_r[2]) + s_r[3];
    part[n_wg + wg] = ((s_r[4] + s_r[5]) + s_r[6]) + s_r[7];
  }
}

// After iteration `it`: one workgroup per image sums the image's partials in a fixed order (no floating-point atomics: the
// number of iterations must not vary from run to run), forms E = (sum d^2 + weight sum norm) / size and applies the reference's
// stopping test |E_prev - E| < eps E_0.  n_iter: iterations run (the one that met the test included); n_done: images of the
// chunk that have met it.
__global__ void __launch_bounds__(256) k_dn_tvc_check(char* __restrict__ ws, size_t stride, size_t off_part, int n_wg, int img0,
                                                      int it, double weight, double eps, double size, int* __restrict__ n_iter,
                                                      int* __restrict__ n_done) {
#pragma clang fp contract(off)
  __shared__ double s_r[8];
  char* blk = ws + (size_t)blockIdx.x * stride;
  TvcState* st = (TvcState*)(blk + off_part);
  if (it > 0 && st->done) return;
  const double* part = (const double*)(blk + off_part + sizeof(TvcState));
  double a = 0.0, b = 0.0;
  for (int j = threadIdx.x; j < n_wg; j += blockDim.x) {
    a = a + part[j];
    b = b + part[n_wg + j];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a = a + __shfl_xor(a, o, WAVE);
    b = b + __shfl_xor(b, o, WAVE);
  }
  if ((threadIdx.x & 63) == 0) {
    s_r[threadIdx.x >> 6] = a;
    s_r[4 + (threadIdx.x >> 6)] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sd2 = ((s_r[0] + s_r[1]) + s_r[2]) + s_r[3], sn = ((s_r[4] + s_r[5]) + s_r[6]) + s_r[7];
    double E = sd2 + weight * sn;
    E = E / size;
    n_iter[img0 + blockIdx.x] = it + 1;
    if (it == 0) {
      st->E_init = E;
      st->E_prev = E;
      st->done = 0;
    } else if (fabs(st->E_prev - E) < eps * st->E_init) {
      st->done = 1;
      atomicAdd(n_done, 1);
    } else {
      st->E_prev = E;
    }
    st->n_iter = it + 1;
  }
}

