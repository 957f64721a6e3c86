// Part of gpet_kernels.hip (included there, inside namespace gpet, in this order): a1: gradient-image convolution, ReLU, float32 min-max normalisation (gpet_utils.py:65-119).
// ---------------------------------------------------------------------------------------
// a1  conv (scipy.ndimage.convolve mode='nearest') + clamp + f32 cast + min/max
//     gpet_utils.py:112-113.  Bit-exact: taps in scipy's order, no FMA contraction.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned int f32_order_key(float f) {
  unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_from_key(unsigned int k) {
  unsigned int u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  return __uint_as_float(u);
}
// a thread's order-key (min, max) -> the wave's, then one atomic pair per wave (lane_id: any index whose low six bits are the lane)
__device__ __forceinline__ void wave_minmax_commit(unsigned int kmin, unsigned int kmax, unsigned int lane_id, unsigned int* pmin,
                                                   unsigned int* pmax) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (unsigned int)__shfl_xor((int)kmin, o, WAVE));
    kmax = max(kmax, (unsigned int)__shfl_xor((int)kmax, o, WAVE));
  }
  if ((lane_id & 63) == 0) {
    atomicMin(pmin, kmin);
    atomicMax(pmax, kmax);
  }
}
// gpet_utils.py:84-89 in float32:  a = x - min;  a /= max(a);  (x1, +0 are no-ops) -- two operations, each rounded
__device__ __forceinline__ float f32_min_span(float v, float mn, float span) {
  const float a = v - mn;
  return a / span;
}

// ---------------------------------------------------------------------------------------
// The convolution has five entry points -- one f64 image (k_conv_relu), a stack of frames of pixel type T (k_conv_relu_batch), several
// kernels on shared frames (k_conv_relu_multi; the table: gpet_conv_multi_plan.h), and the two transposed-store forms of vertical
// batches (k_conv_tr_batch, k_conv_tr_multi; geometry: gpet_transpose_plan.h) -- and ONE body: conv_load, a barrier, conv_slot.  Per
// pixel the products, their order, the skipped zero taps, the clamp, the cast and the order key are therefore the same in all five, and
// so are an image's bits and its (min, max) pair, whichever form computed it.
//
// A workgroup of 64 x 4 threads owns a tile of one image's output.  Its edge-replicated patch goes through LDS once -- every thread
// fetching its kh kw taps from global memory took 1.5 ms per 2048 x 2048 image -- as f64, whatever T is (exact for u8, u16, f32), which
// keeps the LDS reads of the tap loop 8 bytes wide.  The patch load reads the image along its rows: consecutive lanes read consecutive
// pixels of a patch row (one or two cache lines of u8, nine of f64), and each image is read once.
//
// What differs between the row-major and the turned tile is the layout policy L:
//   ConvRows   64 columns x 16 rows; threadIdx.x is the column, threadIdx.y walks the rows; the patch lies row-major at pitch pw; pixel
//              (y, x) is stored at y * N + x.
//   ConvTurned 16 frame columns x 64 frame rows; threadIdx.x is the ROW, threadIdx.y walks the columns; pixel (y, x) is stored at
//              x * M + y of the N x M image, so the 64 lanes of a wave write 64 consecutive floats.  The patch lies in LDS TRANSPOSED,
//              pw columns of ph pixels at an odd pitch, so that the lanes of a tap read (one patch row apart) are consecutive doubles
//              as they are under ConvRows; the few writes of the patch load are the strided ones, and the odd pitch spreads them over
//              the banks.
// ---------------------------------------------------------------------------------------
#define CONV_RY 16
struct ConvRows {
  static constexpr int TILE_X = 64, TILE_Y = CONV_RY, SPAN = CONV_RY;  // SPAN: what threadIdx.y walks
  static __device__ __forceinline__ int x0() { return blockIdx.x * 64; }
  static __device__ __forceinline__ int y0() { return blockIdx.y * CONV_RY; }
  static __device__ __forceinline__ int yl(int j) { return j; }
  static __device__ __forceinline__ int xl(int) { return threadIdx.x; }
  static __device__ __forceinline__ int pitch(int, int pw) { return pw; }
  static __device__ __forceinline__ int cell(int py, int px, int pitch) { return py * pitch + px; }
  static __device__ __forceinline__ int tap_step(int) { return 1; }  // doubles from tap b to tap b + 1
  static __device__ __forceinline__ size_t out_offset(int y, int x, int, int N) { return (size_t)y * N + x; }
};
struct ConvTurned {
  static constexpr int TILE_X = CONV_T_TILE_X, TILE_Y = CONV_T_TILE_Y, SPAN = CONV_T_TILE_X;
  static __device__ __forceinline__ int x0() { return conv_t_col(blockIdx.x, 0); }
  static __device__ __forceinline__ int y0() { return conv_t_row(blockIdx.y, 0); }
  static __device__ __forceinline__ int yl(int) { return threadIdx.x; }
  static __device__ __forceinline__ int xl(int j) { return j; }
  static __device__ __forceinline__ int pitch(int ph, int) { return conv_t_pitch(ph); }
  static __device__ __forceinline__ int cell(int py, int px, int pitch) { return px * pitch + py; }
  static __device__ __forceinline__ int tap_step(int pitch) { return pitch; }
  static __device__ __forceinline__ size_t out_offset(int y, int x, int M, int) { return tr_offset(y, x, M); }
};

// The n_taps taps at wf into s_w, and behind them the ph x pw patch of img whose cell (0, 0) is pixel (y0 - top, x0 - left), clamped
// to the image, as f64 in L's layout.  Returns the patch; the caller's barrier follows.
template <typename L, typename T>
__device__ __forceinline__ const double* conv_load(double* s_w, const double* __restrict__ wf, int n_taps, const T* __restrict__ img, int M,
                                                   int N, int top, int left, int ph, int pw) {
  const int tid = threadIdx.x + threadIdx.y * blockDim.x, nthr = blockDim.x * blockDim.y;
  for (int i = tid; i < n_taps; i += nthr) s_w[i] = wf[i];
  double* s_p = s_w + n_taps;
  const int x0 = L::x0(), y0 = L::y0(), pitch = L::pitch(ph, pw);
  for (int e = tid; e < pw * ph; e += nthr) {
    const int py = e / pw, px = e - py * pw;
    int ry = y0 + py - top, rx = x0 + px - left;
    ry = ry < 0 ? 0 : (ry > M - 1 ? M - 1 : ry);
    rx = rx < 0 ? 0 : (rx > N - 1 ? N - 1 : rx);
    s_p[L::cell(py, px, pitch)] = (double)img[(size_t)ry * N + rx];
  }
  return s_p;
}

// One kernel's image of the workgroup's tile out of the patch: taps w [kh][kw], tap (0, 0) at (dy, dx) of the output pixel's patch
// cell; clamp, f32 cast, store, and the tile's order-key (min, max) into mm[0], mm[1] with one atomic pair per wave.
template <typename L>
__device__ __forceinline__ void conv_slot(const double* s_p, int pitch, const double* w, int kh, int kw, int dy, int dx, int M, int N,
                                          float* __restrict__ out, unsigned int* mm) {
#pragma clang fp contract(off)
  const int x0 = L::x0(), y0 = L::y0(), step = L::tap_step(pitch);
  unsigned int kmin = 0xFFFFFFFFu, kmax = 0u;
  for (int j = threadIdx.y; j < L::SPAN; j += blockDim.y) {
    const int yl = L::yl(j), xl = L::xl(j), y = y0 + yl, x = x0 + xl;
    if (x < N && y < M) {
      double acc = 0.0;
      for (int a = 0; a < kh; ++a) {
        const double* row = s_p + L::cell(yl + a + dy, xl + dx, pitch);
        for (int b = 0; b < kw; ++b) {
          const double wt = w[a * kw + b];
          if (wt == 0.0) continue;
          acc = acc + row[b * step] * wt;
        }
      }
      if (acc < 0.0) acc = 0.0;
      const float v = (float)acc;
      out[L::out_offset(y, x, M, N)] = v;
      const unsigned int key = f32_order_key(v);
      kmin = min(kmin, key);
      kmax = max(kmax, key);
    }
  }
  wave_minmax_commit(kmin, kmax, threadIdx.x + threadIdx.y * blockDim.x, mm, mm + 1);
}

// one kernel on one image: the image's patch, then its one slot with the whole tap array
template <typename L, typename T>
__device__ __forceinline__ void conv_single(const T* __restrict__ img, int M, int N, const double* __restrict__ wf, int kh, int kw, int oy,
                                            int ox, float* __restrict__ out, unsigned int* mm) {
  extern __shared__ double s_w[];  // [kh * kw] taps, then the patch
  const int ph = L::TILE_Y + kh - 1, pw = L::TILE_X + kw - 1;
  const double* s_p = conv_load<L>(s_w, wf, kh * kw, img, M, N, oy, ox, ph, pw);
  __syncthreads();
  conv_slot<L>(s_p, L::pitch(ph, pw), s_w, kh, kw, 0, 0, M, N, out, mm);
}
// blockIdx.z is a FRAME: the union patch of all kernels and their flipped taps, loaded once, then every slot of the frame out of it --
// slot g's kernel k reads patch row yl + a + kd[k].dy, column xl + b + kd[k].dx for its tap (a, b), the pixel the single-kernel form
// reads for it.  (min, max) per slot.
template <typename L, typename T>
__device__ __forceinline__ void conv_multi(const T* const* __restrict__ src, int frame0, int M, int N, const double* __restrict__ wf,
                                           int n_taps, const ConvKernDesc* __restrict__ kd, int top, int left, int ph, int pw,
                                           const int32_t* __restrict__ slot_off, const int32_t* __restrict__ slot_list,
                                           const int32_t* __restrict__ kernel_of, float* const* __restrict__ dst, unsigned int* minmax) {
  extern __shared__ double s_w[];  // [n_taps] taps of all kernels, then the union patch
  const int f = frame0 + blockIdx.z;
  const double* s_p = conv_load<L>(s_w, wf, n_taps, src[f], M, N, top, left, ph, pw);
  __syncthreads();
  for (int si = slot_off[f]; si < slot_off[f + 1]; ++si) {
    const int g = slot_list[si];
    const ConvKernDesc K = kd[kernel_of[g]];
    conv_slot<L>(s_p, L::pitch(ph, pw), s_w + K.w0, K.kh, K.kw, K.dy, K.dx, M, N, dst[g], minmax + 2 * (size_t)g);
  }
}

__global__ void k_conv_relu(const double* __restrict__ img, int M, int N, const double* __restrict__ wf,
                            int kh, int kw, int oy, int ox, float* __restrict__ out, unsigned int* minmax) {
  conv_single<ConvRows>(img, M, N, wf, kh, kw, oy, ox, out, minmax);
}
// image img0 + blockIdx.z of a stack (gpet_grad_images, gpet_batch_create_raw, gpet_batch_set_raw_images), into the image's own
// (min, max) slot
template <typename T>
__global__ void k_conv_relu_batch(const T* const* __restrict__ src, int img0, int M, int N, const double* __restrict__ wf,
                                  int kh, int kw, int oy, int ox, float* const* __restrict__ dst, unsigned int* minmax) {
  const int g = img0 + blockIdx.z;
  conv_single<ConvRows>(src[g], M, N, wf, kh, kw, oy, ox, dst[g], minmax + 2 * (size_t)g);
}
template <typename T>
__global__ void k_conv_tr_batch(const T* const* __restrict__ src, int img0, int M, int N, const double* __restrict__ wf,
                                    int kh, int kw, int oy, int ox, float* const* __restrict__ dst, unsigned int* minmax) {
  const int g = img0 + blockIdx.z;
  conv_single<ConvTurned>(src[g], M, N, wf, kh, kw, oy, ox, dst[g], minmax + 2 * (size_t)g);
}
// (gpet_grad_images_multi, gpet_batch_create_raw_multi, gpet_batch_set_raw_images_multi)
template <typename T>
__global__ void k_conv_relu_multi(const T* const* __restrict__ src, int frame0, int M, int N, const double* __restrict__ wf, int n_taps,
                                  const ConvKernDesc* __restrict__ kd, int top, int left, int ph, int pw,
                                  const int32_t* __restrict__ slot_off, const int32_t* __restrict__ slot_list,
                                  const int32_t* __restrict__ kernel_of, float* const* __restrict__ dst, unsigned int* minmax) {
  conv_multi<ConvRows>(src, frame0, M, N, wf, n_taps, kd, top, left, ph, pw, slot_off, slot_list, kernel_of, dst, minmax);
}
template <typename T>
__global__ void k_conv_tr_multi(const T* const* __restrict__ src, int frame0, int M, int N, const double* __restrict__ wf, int n_taps,
                                    const ConvKernDesc* __restrict__ kd, int top, int left, int ph, int pw,
                                    const int32_t* __restrict__ slot_off, const int32_t* __restrict__ slot_list,
                                    const int32_t* __restrict__ kernel_of, float* const* __restrict__ dst, unsigned int* minmax) {
  conv_multi<ConvTurned>(src, frame0, M, N, wf, n_taps, kd, top, left, ph, pw, slot_off, slot_list, kernel_of, dst, minmax);
}

__global__ void k_minmax_f32(const float* __restrict__ in, size_t count, unsigned int* minmax) {
  unsigned int kmin = 0xFFFFFFFFu, kmax = 0u;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned int k = f32_order_key(in[i]);
    kmin = min(kmin, k);
    kmax = max(kmax, k);
  }
  wave_minmax_commit(kmin, kmax, threadIdx.x, &minmax[0], &minmax[1]);
}

__global__ void k_normalise_f32(const float* __restrict__ in, size_t count, const unsigned int* minmax,
                                float* __restrict__ out) {
  const float mn = f32_from_key(minmax[0]);
  const float mx = f32_from_key(minmax[1]);
  const float span = mx - mn;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
    out[i] = f32_min_span(in[i], mn, span);
}

// k_normalise_f32 in place for image img0 + blockIdx.y of a stack, with that image's (min, max) slot
__global__ void k_normalise_f32_batch(float* const* __restrict__ imgs, int img0, size_t count, const unsigned int* minmax) {
  const int g = img0 + blockIdx.y;
  float* p = imgs[g];
  const float mn = f32_from_key(minmax[2 * (size_t)g]);
  const float mx = f32_from_key(minmax[2 * (size_t)g + 1]);
  const float span = mx - mn;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
    p[i] = f32_min_span(p[i], mn, span);
}

// A finished M x N f32 image into the N x M one (gradient images a caller hands a vertical batch): a TR_TILE x TR_TILE tile through
// LDS at pitch TR_PITCH -- consecutive lanes read a row of the source, then write a row of the destination.  NORM: every element
// goes through k_normalise_f32's arithmetic with the image's (min, max) on its way (upload_images); else a plain copy
// (band_load_full).
template <bool NORM>
__global__ void k_transpose_f32(const float* __restrict__ in, int M, int N, const unsigned int* minmax, float* __restrict__ out) {
  __shared__ float s_t[TR_TILE * TR_PITCH];
  float mn = 0.0f, span = 1.0f;
  if (NORM) {
    mn = f32_from_key(minmax[0]);
    span = f32_from_key(minmax[1]) - mn;
  }
  const int x0 = blockIdx.x * TR_TILE, y0 = blockIdx.y * TR_TILE;
  for (int r = threadIdx.y; r < TR_TILE; r += blockDim.y) {
    const int y = y0 + r, x = x0 + threadIdx.x;
    if (y < M && x < N) s_t[r * TR_PITCH + threadIdx.x] = in[(size_t)y * N + x];
  }
  __syncthreads();
  for (int cc = threadIdx.y; cc < TR_TILE; cc += blockDim.y) {
    const int x = x0 + cc, y = y0 + threadIdx.x;
    if (y < M && x < N) {
      float v = s_t[threadIdx.x * TR_PITCH + cc];
      if (NORM) v = f32_min_span(v, mn, span);
      out[tr_offset(y, x, M)] = v;
    }
  }
}
