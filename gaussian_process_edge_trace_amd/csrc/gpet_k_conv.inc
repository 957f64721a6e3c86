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

// (a workgroup of 64 x 4 threads owns 64 columns x 16 rows of the output; its (16 + kh - 1) x (64 + kw - 1) patch of the
//  edge-replicated image goes through LDS once -- every thread fetching its kh kw taps from global memory took 1.5 ms per
//  2048 x 2048 image; the products and their order are unchanged)
#define CONV_RY 16
__global__ void k_conv_relu(const double* __restrict__ img, int M, int N, const double* __restrict__ wf,
                            int kh, int kw, int oy, int ox, float* __restrict__ out, unsigned int* minmax) {
#pragma clang fp contract(off)
  extern __shared__ double s_w[];  // [kh * kw] taps, then the patch [CONV_RY + kh - 1][64 + kw - 1]
  const int tid = threadIdx.x + threadIdx.y * blockDim.x, nthr = blockDim.x * blockDim.y;
  for (int i = tid; i < kh * kw; i += nthr) s_w[i] = wf[i];
  const int pw = 64 + kw - 1, ph = CONV_RY + kh - 1;
  double* s_p = s_w + kh * kw;
  const int x0 = blockIdx.x * 64, y0 = blockIdx.y * CONV_RY;
  for (int e = tid; e < pw * ph; e += nthr) {
    const int py = e / pw, px = e - py * pw;
    int ry = y0 + py - oy, rx = x0 + px - ox;
    ry = ry < 0 ? 0 : (ry > M - 1 ? M - 1 : ry);
    rx = rx < 0 ? 0 : (rx > N - 1 ? N - 1 : rx);
    s_p[e] = img[(size_t)ry * N + rx];
  }
  __syncthreads();
  const int x = x0 + threadIdx.x;
  unsigned int kmin = 0xFFFFFFFFu, kmax = 0u;
  for (int yl = threadIdx.y; yl < CONV_RY; yl += blockDim.y) {
    const int y = y0 + yl;
    if (x < N && y < M) {
      double acc = 0.0;
      for (int a = 0; a < kh; ++a) {
        const double* row = s_p + (yl + a) * pw + threadIdx.x;
        for (int b = 0; b < kw; ++b) {
          const double w = s_w[a * kw + b];
          if (w == 0.0) continue;
          acc = acc + row[b] * w;
        }
      }
      if (acc < 0.0) acc = 0.0;
      const float v = (float)acc;
      out[(size_t)y * N + x] = v;
      const unsigned int key = f32_order_key(v);
      kmin = min(kmin, key);
      kmax = max(kmax, key);
    }
  }
  // workgroup min/max -> one atomic pair per wave
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (unsigned int)__shfl_xor((int)kmin, o, WAVE));
    kmax = max(kmax, (unsigned int)__shfl_xor((int)kmax, o, WAVE));
  }
  if ((tid & 63) == 0) {
    atomicMin(&minmax[0], kmin);
    atomicMax(&minmax[1], kmax);
  }
}

__global__ void k_minmax_f32(const float* __restrict__ in, size_t count, unsigned int* minmax) {
  unsigned int kmin = 0xFFFFFFFFu, kmax = 0u;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned int k = f32_order_key(in[i]);
    kmin = min(kmin, k);
    kmax = max(kmax, k);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (unsigned int)__shfl_xor((int)kmin, o, WAVE));
    kmax = max(kmax, (unsigned int)__shfl_xor((int)kmax, o, WAVE));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&minmax[0], kmin);
    atomicMax(&minmax[1], kmax);
  }
}

// gpet_utils.py:84-89 in float32:  a = x - min;  a /= max(a);  (x1, +0 are no-ops)
__global__ void k_normalise_f32(const float* __restrict__ in, size_t count, const unsigned int* minmax,
                                float* __restrict__ out) {
  const float mn = f32_from_key(minmax[0]);
  const float mx = f32_from_key(minmax[1]);
  const float span = mx - mn;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    const float a = in[i] - mn;
    out[i] = a / span;
  }
}

// ---------------------------------------------------------------------------------------
// a1, batched: raw frames -> gradient images of a whole batch (gpet_grad_images, gpet_batch_create_raw,
//     gpet_batch_set_raw_images).  k_conv_relu for image img0 + blockIdx.z of a stack: pixels of type T become f64 on their
//     way into the LDS patch (exact for u8, u16, f32), then the same taps in the same order, the same clamp, cast and
//     order-key min/max -- into the image's own (min, max) slot.  The patch load is k_conv_relu's: consecutive lanes read
//     consecutive pixels of a patch row (64 + kw - 1 of them: one or two cache lines of u8, nine of f64), each image is read
//     once, and the f64 patch keeps the LDS reads of the tap loop 8 bytes wide whatever T is.
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ void k_conv_relu_batch(const T* const* __restrict__ src, int img0, int M, int N, const double* __restrict__ wf,
                                  int kh, int kw, int oy, int ox, float* const* __restrict__ dst, unsigned int* minmax) {
#pragma clang fp contract(off)
  extern __shared__ double s_w[];  // [kh * kw] taps, then the patch [CONV_RY + kh - 1][64 + kw - 1]
  const int g = img0 + blockIdx.z;
  const T* __restrict__ img = src[g];
  float* __restrict__ out = dst[g];
  const int tid = threadIdx.x + threadIdx.y * blockDim.x, nthr = blockDim.x * blockDim.y;
  for (int i = tid; i < kh * kw; i += nthr) s_w[i] = wf[i];
  const int pw = 64 + kw - 1, ph = CONV_RY + kh - 1;
  double* s_p = s_w + kh * kw;
  const int x0 = blockIdx.x * 64, y0 = blockIdx.y * CONV_RY;
  for (int e = tid; e < pw * ph; e += nthr) {
    const int py = e / pw, px = e - py * pw;
    int ry = y0 + py - oy, rx = x0 + px - ox;
    ry = ry < 0 ? 0 : (ry > M - 1 ? M - 1 : ry);
    rx = rx < 0 ? 0 : (rx > N - 1 ? N - 1 : rx);
    s_p[e] = (double)img[(size_t)ry * N + rx];
  }
  __syncthreads();
  const int x = x0 + threadIdx.x;
  unsigned int kmin = 0xFFFFFFFFu, kmax = 0u;
  for (int yl = threadIdx.y; yl < CONV_RY; yl += blockDim.y) {
    const int y = y0 + yl;
    if (x < N && y < M) {
      double acc = 0.0;
      for (int a = 0; a < kh; ++a) {
        const double* row = s_p + (yl + a) * pw + threadIdx.x;
        for (int b = 0; b < kw; ++b) {
          const double w = s_w[a * kw + b];
          if (w == 0.0) continue;
          acc = acc + row[b] * w;
        }
      }
      if (acc < 0.0) acc = 0.0;
      const float v = (float)acc;
      out[(size_t)y * N + x] = v;
      const unsigned int key = f32_order_key(v);
      kmin = min(kmin, key);
      kmax = max(kmax, key);
    }
  }
  // workgroup min/max -> one atomic pair per wave, into the image's slot
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (unsigned int)__shfl_xor((int)kmin, o, WAVE));
    kmax = max(kmax, (unsigned int)__shfl_xor((int)kmax, o, WAVE));
  }
  if ((tid & 63) == 0) {
    atomicMin(&minmax[2 * (size_t)g], kmin);
    atomicMax(&minmax[2 * (size_t)g + 1], kmax);
  }
}

// k_normalise_f32 in place for image img0 + blockIdx.y of a stack, with that image's (min, max) slot
__global__ void k_normalise_f32_batch(float* const* __restrict__ imgs, int img0, size_t count, const unsigned int* minmax) {
  const int g = img0 + blockIdx.y;
  float* p = imgs[g];
  const float mn = f32_from_key(minmax[2 * (size_t)g]);
  const float mx = f32_from_key(minmax[2 * (size_t)g + 1]);
  const float span = mx - mn;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    const float a = p[i] - mn;
    p[i] = a / span;
  }
}

// ---------------------------------------------------------------------------------------
// a1, batched, several kernels on shared frames (gpet_grad_images_multi, gpet_batch_create_raw_multi,
//     gpet_batch_set_raw_images_multi; the table: gpet_conv_multi_plan.h).  blockIdx.z is a FRAME: its workgroup loads the union
//     patch of all kernels once -- k_conv_relu_batch's load, with the union's halo -- and the flipped taps of all kernels, then
//     evaluates every slot of the frame out of that patch: slot g's kernel k reads patch row yl + a + kd[k].dy, column
//     tx + b + kd[k].dx for its tap (a, b), which is the pixel k_conv_relu_batch reads for it.  Per output the products, their
//     order, the skipped zero taps, the clamp and the cast are k_conv_relu_batch's, so a slot's image has its bits.  One
//     order-key (min, max) atomic pair per wave and slot.
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ void k_conv_relu_multi(const T* const* __restrict__ src, int frame0, int M, int N, const double* __restrict__ wf, int n_taps,
                                  const ConvKernDesc* __restrict__ kd, int top, int left, int ph, int pw,
                                  const int32_t* __restrict__ slot_off, const int32_t* __restrict__ slot_list,
                                  const int32_t* __restrict__ kernel_of, float* const* __restrict__ dst, unsigned int* minmax) {
#pragma clang fp contract(off)
  extern __shared__ double s_w[];  // [n_taps] taps of all kernels, then the union patch [ph][pw]
  const int f = frame0 + blockIdx.z;
  const T* __restrict__ img = src[f];
  const int tid = threadIdx.x + threadIdx.y * blockDim.x, nthr = blockDim.x * blockDim.y;
  for (int i = tid; i < n_taps; i += nthr) s_w[i] = wf[i];
  double* s_p = s_w + n_taps;
  const int x0 = blockIdx.x * 64, y0 = blockIdx.y * CONV_RY;
  for (int e = tid; e < pw * ph; e += nthr) {
    const int py = e / pw, px = e - py * pw;
    int ry = y0 + py - top, rx = x0 + px - left;
    ry = ry < 0 ? 0 : (ry > M - 1 ? M - 1 : ry);
    rx = rx < 0 ? 0 : (rx > N - 1 ? N - 1 : rx);
    s_p[e] = (double)img[(size_t)ry * N + rx];
  }
  __syncthreads();
  const int x = x0 + threadIdx.x;
  for (int si = slot_off[f]; si < slot_off[f + 1]; ++si) {
    const int g = slot_list[si];
    const ConvKernDesc K = kd[kernel_of[g]];
    const double* __restrict__ w_k = s_w + K.w0;
    float* __restrict__ out = dst[g];
    unsigned int kmin = 0xFFFFFFFFu, kmax = 0u;
    for (int yl = threadIdx.y; yl < CONV_RY; yl += blockDim.y) {
      const int y = y0 + yl;
      if (x < N && y < M) {
        double acc = 0.0;
        for (int a = 0; a < K.kh; ++a) {
          const double* row = s_p + (yl + a + K.dy) * pw + threadIdx.x + K.dx;
          for (int b = 0; b < K.kw; ++b) {
            const double w = w_k[a * K.kw + b];
            if (w == 0.0) continue;
            acc = acc + row[b] * w;
          }
        }
        if (acc < 0.0) acc = 0.0;
        const float v = (float)acc;
        out[(size_t)y * N + x] = v;
        const unsigned int key = f32_order_key(v);
        kmin = min(kmin, key);
        kmax = max(kmax, key);
      }
    }
    // wave min/max -> one atomic pair per wave, into the slot's pair
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      kmin = min(kmin, (unsigned int)__shfl_xor((int)kmin, o, WAVE));
      kmax = max(kmax, (unsigned int)__shfl_xor((int)kmax, o, WAVE));
    }
    if ((tid & 63) == 0) {
      atomicMin(&minmax[2 * (size_t)g], kmin);
      atomicMax(&minmax[2 * (size_t)g + 1], kmax);
    }
  }
}

// ---------------------------------------------------------------------------------------
// a1, batched, transposed store (GPET_FRAMES_TRANSPOSED; geometry: gpet_transpose_plan.h).  k_conv_relu_batch with the tile turned:
//     a workgroup of 64 x 4 threads owns 16 frame columns x 64 frame rows, threadIdx.x is the ROW within the tile, and pixel (y, x)
//     is stored at x * M + y of the N x M image -- the 64 lanes of a wave write 64 consecutive floats.  The patch lies in LDS
//     TRANSPOSED, [16 + kw - 1] columns of 64 + kh - 1 pixels at an odd pitch, so the lanes of a tap read (one patch row apart) are
//     consecutive doubles, as they are in k_conv_relu_batch; the few writes of the patch load are the strided ones.
//     Per pixel the products, their order, the skipped zero taps, the clamp, the cast and the order key are k_conv_relu_batch's:
//     the image is that kernel's, transposed, bit for bit, and the (min, max) slot holds the same pair.
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ void k_conv_tr_batch(const T* const* __restrict__ src, int img0, int M, int N, const double* __restrict__ wf,
                                    int kh, int kw, int oy, int ox, float* const* __restrict__ dst, unsigned int* minmax) {
#pragma clang fp contract(off)
  extern __shared__ double s_w[];  // [kh * kw] taps, then the patch, column-major: [CONV_T_TILE_X + kw - 1][pitch]
  const int g = img0 + blockIdx.z;
  const T* __restrict__ img = src[g];
  float* __restrict__ out = dst[g];
  const int tid = threadIdx.x + threadIdx.y * blockDim.x, nthr = blockDim.x * blockDim.y;
  for (int i = tid; i < kh * kw; i += nthr) s_w[i] = wf[i];
  const int pw = CONV_T_TILE_X + kw - 1, ph = CONV_T_TILE_Y + kh - 1, pitch = conv_t_pitch(ph);
  double* s_p = s_w + kh * kw;
  const int x0 = conv_t_col(blockIdx.x, 0), y0 = conv_t_row(blockIdx.y, 0);
  for (int e = tid; e < pw * ph; e += nthr) {
    const int py = e / pw, px = e - py * pw;
    int ry = y0 + py - oy, rx = x0 + px - ox;
    ry = ry < 0 ? 0 : (ry > M - 1 ? M - 1 : ry);
    rx = rx < 0 ? 0 : (rx > N - 1 ? N - 1 : rx);
    s_p[px * pitch + py] = (double)img[(size_t)ry * N + rx];
  }
  __syncthreads();
  const int yl = threadIdx.x, y = y0 + yl;
  unsigned int kmin = 0xFFFFFFFFu, kmax = 0u;
  for (int xl = threadIdx.y; xl < CONV_T_TILE_X; xl += blockDim.y) {
    const int x = x0 + xl;
    if (x < N && y < M) {
      double acc = 0.0;
      for (int a = 0; a < kh; ++a) {
        const double* row = s_p + xl * pitch + yl + a;  // (patch row yl + a of column xl; the next column is `pitch` further)
        for (int b = 0; b < kw; ++b) {
          const double w = s_w[a * kw + b];
          if (w == 0.0) continue;
          acc = acc + row[b * pitch] * w;
        }
      }
      if (acc < 0.0) acc = 0.0;
      const float v = (float)acc;
      out[tr_offset(y, x, M)] = v;
      const unsigned int key = f32_order_key(v);
      kmin = min(kmin, key);
      kmax = max(kmax, key);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    kmin = min(kmin, (unsigned int)__shfl_xor((int)kmin, o, WAVE));
    kmax = max(kmax, (unsigned int)__shfl_xor((int)kmax, o, WAVE));
  }
  if ((tid & 63) == 0) {
    atomicMin(&minmax[2 * (size_t)g], kmin);
    atomicMax(&minmax[2 * (size_t)g + 1], kmax);
  }
}

// k_conv_relu_multi with the tile turned the same way: the union patch column-major at the odd pitch, every slot of the frame out of it
template <typename T>
__global__ void k_conv_tr_multi(const T* const* __restrict__ src, int frame0, int M, int N, const double* __restrict__ wf, int n_taps,
                                    const ConvKernDesc* __restrict__ kd, int top, int left, int ph, int pw,
                                    const int32_t* __restrict__ slot_off, const int32_t* __restrict__ slot_list,
                                    const int32_t* __restrict__ kernel_of, float* const* __restrict__ dst, unsigned int* minmax) {
#pragma clang fp contract(off)
  extern __shared__ double s_w[];  // [n_taps] taps of all kernels, then the union patch, column-major: [pw][pitch]
  const int f = frame0 + blockIdx.z;
  const T* __restrict__ img = src[f];
  const int tid = threadIdx.x + threadIdx.y * blockDim.x, nthr = blockDim.x * blockDim.y;
  for (int i = tid; i < n_taps; i += nthr) s_w[i] = wf[i];
  double* s_p = s_w + n_taps;
  const int pitch = conv_t_pitch(ph);
  const int x0 = conv_t_col(blockIdx.x, 0), y0 = conv_t_row(blockIdx.y, 0);
  for (int e = tid; e < pw * ph; e += nthr) {
    const int py = e / pw, px = e - py * pw;
    int ry = y0 + py - top, rx = x0 + px - left;
    ry = ry < 0 ? 0 : (ry > M - 1 ? M - 1 : ry);
    rx = rx < 0 ? 0 : (rx > N - 1 ? N - 1 : rx);
    s_p[px * pitch + py] = (double)img[(size_t)ry * N + rx];
  }
  __syncthreads();
  const int yl = threadIdx.x, y = y0 + yl;
  for (int si = slot_off[f]; si < slot_off[f + 1]; ++si) {
    const int g = slot_list[si];
    const ConvKernDesc K = kd[kernel_of[g]];
    const double* __restrict__ w_k = s_w + K.w0;
    float* __restrict__ out = dst[g];
    unsigned int kmin = 0xFFFFFFFFu, kmax = 0u;
    for (int xl = threadIdx.y; xl < CONV_T_TILE_X; xl += blockDim.y) {
      const int x = x0 + xl;
      if (x < N && y < M) {
        double acc = 0.0;
        for (int a = 0; a < K.kh; ++a) {
          const double* row = s_p + (xl + K.dx) * pitch + yl + a + K.dy;
          for (int b = 0; b < K.kw; ++b) {
            const double w = w_k[a * K.kw + b];
            if (w == 0.0) continue;
            acc = acc + row[b * pitch] * w;
          }
        }
        if (acc < 0.0) acc = 0.0;
        const float v = (float)acc;
        out[tr_offset(y, x, M)] = v;
        const unsigned int key = f32_order_key(v);
        kmin = min(kmin, key);
        kmax = max(kmax, key);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      kmin = min(kmin, (unsigned int)__shfl_xor((int)kmin, o, WAVE));
      kmax = max(kmax, (unsigned int)__shfl_xor((int)kmax, o, WAVE));
    }
    if ((tid & 63) == 0) {
      atomicMin(&minmax[2 * (size_t)g], kmin);
      atomicMax(&minmax[2 * (size_t)g + 1], kmax);
    }
  }
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
      if (NORM) {
        const float a = v - mn;
        v = a / span;
      }
      out[tr_offset(y, x, M)] = v;
    }
  }
}

