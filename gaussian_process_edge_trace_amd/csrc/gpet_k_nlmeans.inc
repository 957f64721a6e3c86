// Part of gpet_kernels.hip (included there, inside namespace gpet): a0: non-local means of raw frames, the reference's
// gpet_utils.denoise 'nl' (gpet_utils.py:133-134) = scikit-image 0.18.3's denoise_nl_means(..., fast_mode=False) on a 2-D frame.
// The arithmetic, its order and the exponential: gpet_nlmeans_plan.h.
// ---------------------------------------------------------------------------------------
// Image blockIdx.z of the launch is frame img0 + blockIdx.z of the device pointer tables src / dst.  A workgroup of 16 x 16 threads
// owns 16 x 16 output pixels; the (16 + 2 d + 2 off)^2 pixels of the padded frame around them go through LDS once, widened to f64
// (positions outside the padded frame hold 0 and are never read by a candidate inside the image).  Every thread then walks its
// pixel's clipped search window in the reference's order.  S > 0: the patch extent is known at compile time and the pixel's own
// patch sits in registers, so a term costs one LDS read; S = 0: any extent, both patches read from LDS.  The taps are read through
// a uniform address (scalar loads).  A lane whose distance is above the cutoff at a row start leaves the row loop with weight 0;
// the hardware keeps a wave in the loop only while a lane of it is still adding rows.
template <typename T, int S>
__global__ void __launch_bounds__(256) k_nlmeans(const T* const* __restrict__ src, double* const* __restrict__ dst, int img0, int M, int N,
                                                 int s_, int d, const double* __restrict__ w, double var2) {
#pragma clang fp contract(off)
  extern __shared__ double s_nl[];
  const int s = S > 0 ? S : s_, off = s / 2;
  const int ext = NLM_TILE + 2 * d + 2 * off, stride = nlm_lds_stride(ext);
  const int x0 = blockIdx.x * NLM_TILE, y0 = blockIdx.y * NLM_TILE;
  const T* __restrict__ img = src[img0 + blockIdx.z];
  const int tid = threadIdx.x + threadIdx.y * NLM_TILE;
  // LDS (r, c) = P[y0 - d + r][x0 - d + c], P the padded frame: P[p][q] = img[mirror(p - off)][mirror(q - off)]
  for (int e = tid; e < ext * ext; e += NLM_TILE * NLM_TILE) {
    const int r = e / ext, c = e - r * ext;
    const int p = y0 - d + r, q = x0 - d + c;
    double v = 0.0;
    if (p >= 0 && p < M + 2 * off && q >= 0 && q < N + 2 * off) v = (double)img[(size_t)nlm_mirror(p - off, M) * N + nlm_mirror(q - off, N)];
    s_nl[r * stride + c] = v;
  }
  __syncthreads();
  const int col = x0 + threadIdx.x, row = y0 + threadIdx.y;
  if (col >= N || row >= M) return;
  const double* cen = s_nl + (threadIdx.y + d) * stride + threadIdx.x + d;  // P[row][col]
  constexpr int NC = S > 0 ? S * S : 1;
  double cp[NC];
  if (S > 0) {
#pragma unroll
    for (int a = 0; a < S; ++a)
#pragma unroll
      for (int b = 0; b < S; ++b) cp[a * S + b] = cen[a * stride + b];
  }
  const int i0 = row - (d < row ? d : row), i1 = row + (d + 1 < M - row ? d + 1 : M - row);
  const int j0 = col - (d < col ? d : col), j1 = col + (d + 1 < N - col ? d + 1 : N - col);
  double wsum = 0.0, acc = 0.0;
  for (int i = i0; i < i1; ++i) {
    const double* crow = s_nl + (i - y0 + d) * stride - x0 + d;
    for (int j = j0; j < j1; ++j) {
      const double* cand = crow + j;  // P[i][j]
      double dist = 0.0;
      bool cut = false;
      if (S > 0) {
#pragma unroll
        for (int a = 0; a < S; ++a) {
          if (dist > NLM_CUTOFF) cut = true;
          if (cut) break;
#pragma unroll
          for (int b = 0; b < S; ++b) {
            const double t = cp[a * S + b] - cand[a * stride + b];
            dist = dist + w[a * S + b] * (t * t - var2);
          }
        }
      } else {
        for (int a = 0; a < s; ++a) {
          if (dist > NLM_CUTOFF) {
            cut = true;
            break;
          }
          for (int b = 0; b < s; ++b) {
            const double t = cen[a * stride + b] - cand[a * stride + b];
            dist = dist + w[a * s + b] * (t * t - var2);
          }
        }
      }
      const double weight = cut ? 0.0 : nlm_fexp(-(dist > 0.0 ? dist : 0.0));
      wsum = wsum + weight;
      acc = acc + weight * cand[off * stride + off];
    }
  }
  dst[img0 + blockIdx.z][(size_t)row * N + col] = acc / wsum;
}
