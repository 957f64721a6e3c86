// Part of gpet_kernels.hip (included there, inside namespace gpet): polar unwrap of raw frames in front of the raw-frame path -- a frame
// resampled to (radius x angle) around its centre, so that a closed contour r(theta) is the horizontal edge the tracer follows.  The
// arithmetic and its order: gpet_polar_plan.h.
// ---------------------------------------------------------------------------------------
// One thread per output pixel, the pixels of a frame in row-major order: lanes run along c, so a wave's 8-byte stores are contiguous,
// and a wave shares one radius (two where it crosses a row end) and neighbouring angles -- its four taps per lane are neighbours in
// L2.  Image blockIdx.z of a launch is frame img0 + blockIdx.z of the device pointer tables; its centre is entry (img0 + blockIdx.z)
// of the centre tables, or entry 0 when all frames share one.  No LDS.
template <typename T>
__global__ void __launch_bounds__(POLAR_THREADS) k_polar(const T* const* __restrict__ src, double* const* __restrict__ dst, int img0, int M, int N,
                                                         PolarSpec s, int W, const double* __restrict__ cxy, int n_centres,
                                                         const double* __restrict__ cos_t, const double* __restrict__ sin_t) {
#pragma clang fp contract(off)
  const size_t cells = (size_t)s.n_r * (size_t)W, e = (size_t)blockIdx.x * POLAR_THREADS + threadIdx.x;
  if (e >= cells) return;
  const int g = img0 + (int)blockIdx.z, k = n_centres == 1 ? 0 : g;
  const int i = (int)(e / (size_t)W), c = (int)(e - (size_t)i * (size_t)W);
  dst[g][e] = polar_sample(src[g], M, N, cxy[k], cxy[n_centres + k], s, cos_t, sin_t, i, c);
}
