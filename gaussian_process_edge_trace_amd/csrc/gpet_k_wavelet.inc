// Part of gpet_kernels.hip (included there, inside namespace gpet): a0: wavelet denoising of raw frames, the reference's
// gpet_utils.denoise 'wavelet' (gpet_utils.py:137-138) = scikit-image 0.18.3's denoise_wavelet on PyWavelets 1.1.1 for a 2-D frame
// and an orthogonal wavelet.  The arithmetic, its order, the pyramid's layout and every tile: gpet_wavelet_plan.h.
// ---------------------------------------------------------------------------------------
// Image blockIdx.z of a launch is frame img0 + blockIdx.z of the device pointer tables and of the per-frame arrays (sigma,
// thresholds), and pyramid blockIdx.z of the chunk's workspace ws (frame_doubles apart).

template <typename T>
__device__ inline double wv_unit(T v, double scale) {
  return (double)v * scale;
}
template <>
__device__ inline double wv_unit<float>(float v, double) {
  return (double)v;
}
template <>
__device__ inline double wv_unit<double>(double v, double) {
  return v;
}

// One forward level.  src != nullptr: level 1, the input is frame img0 + z of src (pixel type T, integer pixels times `scale`);
// else the input is the m x n band at off_in of the pyramid (T = double).  Output: the four mo x no bands from off_out.
// LDS: filters [2][16] | patch [P][P], P = 2 WV_TILE + F - 2, by extended index | axis-0 pass lo [WV_TILE][P] | hi [WV_TILE][P].
template <typename T>
__global__ void __launch_bounds__(WV_THREADS) k_wv_fwd(const T* const* __restrict__ src, int img0, double* __restrict__ ws, size_t frame_doubles,
                                                       size_t off_in, int m, int n, size_t off_out, int mo, int no, int F, double scale,
                                                       WvFilters flt) {
#pragma clang fp contract(off)
  extern __shared__ double s_wv[];
  const int P = wv_fwd_patch(F);
  double* s_f = s_wv;
  double* s_p = s_f + 2 * WV_TAPS_MAX;
  double* s_lo = s_p + P * P;
  double* s_hi = s_lo + WV_TILE * P;
  const int tid = threadIdx.x + threadIdx.y * WV_TILE;
  if (tid < WV_TAPS_MAX) {
    s_f[tid] = flt.dec_lo[tid];
    s_f[WV_TAPS_MAX + tid] = flt.dec_hi[tid];
  }
  double* pyr = ws + (size_t)blockIdx.z * frame_doubles;
  const int oy0 = blockIdx.y * WV_TILE, ox0 = blockIdx.x * WV_TILE;
  const int by = 2 * oy0 - F + 2, bx = 2 * ox0 - F + 2;  // extended index of patch position (0, 0)
  const T* __restrict__ img = src ? src[img0 + blockIdx.z] : (const T*)(pyr + off_in);
  for (int e = tid; e < P * P; e += WV_THREADS) {
    const int r = e / P, c = e - r * P;
    const int gy = wv_sym(by + r, m), gx = wv_sym(bx + c, n);
    double v = 0.0;  // (beyond one reflection: read only by outputs outside the bands)
    if (gy >= 0 && gy < m && gx >= 0 && gx < n) v = wv_unit<T>(img[(size_t)gy * n + gx], scale);
    s_p[e] = v;
  }
  __syncthreads();
  // axis 0: output row oy of the tile at i = 2 (oy0 + oy) + 1 reads patch rows 2 oy + F - 1 - j
  for (int e = tid; e < WV_TILE * P; e += WV_THREADS) {
    const int oy = e / P, c = e - oy * P;
    const int i = 2 * (oy0 + oy) + 1;
    double a = 0.0, d = 0.0;
    if (oy0 + oy < mo) {
      for (int t = 0; t < F; ++t) {
        const int j = wv_fwd_tap(t, i, m);
        const double x = s_p[(2 * oy + F - 1 - j) * P + c];
        a = a + s_f[j] * x;
        d = d + s_f[WV_TAPS_MAX + j] * x;
      }
    }
    s_lo[e] = a;
    s_hi[e] = d;
  }
  __syncthreads();
  const int gy = oy0 + threadIdx.y, gx = ox0 + threadIdx.x;
  if (gy >= mo || gx >= no) return;
  const int i = 2 * gx + 1;
  const double* lo = s_lo + threadIdx.y * P + 2 * threadIdx.x + F - 1;
  const double* hi = s_hi + threadIdx.y * P + 2 * threadIdx.x + F - 1;
  double aa = 0.0, ad = 0.0, da = 0.0, dd = 0.0;
  for (int t = 0; t < F; ++t) {
    const int j = wv_fwd_tap(t, i, n);
    const double fl = s_f[j], fh = s_f[WV_TAPS_MAX + j];
    aa = aa + fl * lo[-j];
    ad = ad + fh * lo[-j];
    da = da + fl * hi[-j];
    dd = dd + fh * hi[-j];
  }
  const size_t band = (size_t)mo * no, at = (size_t)gy * no + gx;
  double* out = pyr + off_out;
  out[at] = aa;
  out[band + at] = ad;
  out[2 * band + at] = da;
  out[3 * band + at] = dd;
}

// The noise level of every frame, one workgroup per frame -> sigma[img0 + z].
// how == 0: median(|dd1| over its non-zero entries) / ppf, dd1 the `count` doubles at off_dd of the pyramid; NaN if all are zero.
//   The median is exact: non-negative doubles order as their bit patterns, so the middle order statistic (both, for an even
//   count) is found by radix select on the patterns, eight bits a pass, with LDS histograms; no floating-point arithmetic before
//   the final (a + b) / 2 / ppf.
// how == 1: the given sigma times (max/q - min/q) / (max - min) of the u8 / u16 frame (q = 255 / 65535, as 1/q products); NaN for
//   a flat frame.   how == 2: the given sigma.
__device__ inline unsigned long long wv_select(const unsigned long long* __restrict__ keys, int count, unsigned k, unsigned* s_hist,
                                               unsigned long long* s_prefix, unsigned* s_k) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    *s_prefix = 0ull;
    *s_k = k;
  }
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (tid < 256) s_hist[tid] = 0u;
    __syncthreads();
    const unsigned long long prefix = *s_prefix;
    for (int e = tid; e < count; e += WV_SIGMA_THREADS) {
      const unsigned long long key = keys[e] & 0x7FFFFFFFFFFFFFFFull;
      if (key != 0ull && (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8)))) atomicAdd(&s_hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned left = *s_k, d = 0;
      while (d < 255u && s_hist[d] <= left) {
        left -= s_hist[d];
        ++d;
      }
      *s_k = left;
      *s_prefix = prefix | ((unsigned long long)d << shift);
    }
    __syncthreads();
  }
  return *s_prefix;
}

__global__ void __launch_bounds__(WV_SIGMA_THREADS) k_wv_sigma(int how, const double* __restrict__ ws, size_t frame_doubles, size_t off_dd, int count,
                                                               const void* const* __restrict__ src, int pix, size_t n_px, int img0,
                                                               double given, double ppf, double* __restrict__ sigma) {
#pragma clang fp contract(off)
  __shared__ unsigned s_hist[256];
  __shared__ unsigned long long s_prefix;
  __shared__ unsigned s_k, s_nz, s_min, s_max;
  const int tid = threadIdx.x;
  if (how == 2) {
    if (tid == 0) sigma[img0 + blockIdx.x] = given;
    return;
  }
  if (tid == 0) {
    s_nz = 0u;
    s_min = 0xFFFFFFFFu;
    s_max = 0u;
  }
  __syncthreads();
  if (how == 1) {
    const void* p = src[img0 + blockIdx.x];
    unsigned lo = 0xFFFFFFFFu, hi = 0u;
    for (size_t e = tid; e < n_px; e += WV_SIGMA_THREADS) {
      const unsigned v = pix == PIX_U8 ? (unsigned)((const uint8_t*)p)[e] : (unsigned)((const uint16_t*)p)[e];
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
    atomicMin(&s_min, lo);
    atomicMax(&s_max, hi);
    __syncthreads();
    if (tid == 0) {
      const double inv = pix == PIX_U8 ? 1.0 / 255.0 : 1.0 / 65535.0;
      const double scale = ((double)s_max * inv - (double)s_min * inv) / (double)(s_max - s_min);
      sigma[img0 + blockIdx.x] = given * scale;  // (a flat frame: 0 / 0)
    }
    return;
  }
  const unsigned long long* keys = (const unsigned long long*)(ws + (size_t)blockIdx.x * frame_doubles + off_dd);
  unsigned nz = 0;
  for (int e = tid; e < count; e += WV_SIGMA_THREADS) nz += (keys[e] & 0x7FFFFFFFFFFFFFFFull) != 0ull ? 1u : 0u;
  atomicAdd(&s_nz, nz);
  __syncthreads();
  nz = s_nz;
  if (nz == 0u) {
    if (tid == 0) sigma[img0 + blockIdx.x] = __longlong_as_double(0x7FF8000000000000ll);
    return;
  }
  const unsigned long long ka = wv_select(keys, count, (nz - 1u) / 2u, s_hist, &s_prefix, &s_k);
  const unsigned long long kb = (nz % 2u) ? ka : wv_select(keys, count, nz / 2u, s_hist, &s_prefix, &s_k);
  if (tid == 0) {
    const double a = __longlong_as_double((long long)ka), b = __longlong_as_double((long long)kb);
    sigma[img0 + blockIdx.x] = (nz % 2u) ? a / ppf : (a + b) / 2.0 / ppf;
  }
}

// The thresholds: workgroup (band, level, image) -> thr / ms [((img0 + z) levels + level) 3 + band], level 0 the finest, bands ad,
// da, dd.  BayesShrink: mean(x x) in the order of wv_mean_squares (gpet_wavelet_plan.h), then wv_bayes_thresh; VisuShrink: sigma c.
__global__ void __launch_bounds__(WV_THRESH_THREADS) k_wv_thresh(const double* __restrict__ ws, WvPlan plan, int img0, int method, double c,
                                                                 const double* __restrict__ sigma, double* __restrict__ thr,
                                                                 double* __restrict__ ms) {
#pragma clang fp contract(off)
  __shared__ double s_part[WV_THRESH_THREADS];
  const int b = blockIdx.x, l = blockIdx.y, g = img0 + blockIdx.z, t = threadIdx.x;
  const size_t at = ((size_t)g * plan.levels + l) * 3 + b;
  const double sg = sigma[g];
  if (method == WV_VISU) {
    if (t == 0) thr[at] = sg * c;
    return;
  }
  const int R = plan.lv[l].mo, C = plan.lv[l].no;
  const double* x = ws + (size_t)blockIdx.z * plan.frame_doubles + plan.lv[l].off + (size_t)(b + 1) * R * C;
  double p = 0.0;
  for (int r = t; r < R; r += WV_THRESH_THREADS) {
    const double* row = x + (size_t)r * C;
    double s = 0.0;
    for (int q = 0; q < C; ++q) s = s + row[q] * row[q];
    p = r == t ? s : p + s;
  }
  s_part[t] = p;
  __syncthreads();
  for (int s = WV_THRESH_THREADS / 2; s > 0; s /= 2) {
    if (t < s) s_part[t] = s_part[t] + s_part[t + s];
    __syncthreads();
  }
  if (t == 0) {
    const double mean = s_part[0] / (double)((long long)R * C);
    ms[at] = mean;
    thr[at] = wv_bayes_thresh(mean, sg * sg);
  }
}

// One inverse level: the mo x no bands at off_in (aa as it is, the details shrunk with thr[0..2] as they are loaded) -> the m_out x
// n_out pixels of the reconstruction, cropped: into the band at off_out of the pyramid (rows n_out apart), or, dst != nullptr, into
// frame img0 + z of dst, clipped to [0, 1] if clip.
// LDS: filters [2][16] | aa, ad, da, dd [Q][Q] each, Q = WV_TILE + F/2 - 1 | axis-1 pass lo [Q][2 WV_TILE] | hi [Q][2 WV_TILE].
__global__ void __launch_bounds__(WV_THREADS) k_wv_inv(double* __restrict__ ws, size_t frame_doubles, size_t off_in, int mo, int no, size_t off_out,
                                                       double* const* __restrict__ dst, int img0, int m_out, int n_out, int F,
                                                       const double* __restrict__ thr, int thr_stride, int mode, int clip, WvFilters flt) {
#pragma clang fp contract(off)
  extern __shared__ double s_wv[];
  const int H = F / 2, Q = wv_inv_patch(F), W = 2 * WV_TILE;
  double* s_f = s_wv;
  double* s_b = s_f + 2 * WV_TAPS_MAX;
  double* s_lo = s_b + 4 * Q * Q;
  double* s_hi = s_lo + Q * W;
  const int tid = threadIdx.x + threadIdx.y * WV_TILE;
  if (tid < WV_TAPS_MAX) {
    s_f[tid] = flt.rec_lo[tid];
    s_f[WV_TAPS_MAX + tid] = flt.rec_hi[tid];
  }
  double* pyr = ws + (size_t)blockIdx.z * frame_doubles;
  const double* in = pyr + off_in;
  const double* th = thr + (size_t)(img0 + blockIdx.z) * thr_stride;
  const size_t band = (size_t)mo * no;
  const int qy0 = blockIdx.y * WV_TILE, qx0 = blockIdx.x * WV_TILE;
  for (int e = tid; e < 4 * Q * Q; e += WV_THREADS) {
    const int b = e / (Q * Q), k = e - b * Q * Q;
    const int r = k / Q, c = k - r * Q;
    const int gy = qy0 + r, gx = qx0 + c;
    double v = 0.0;
    if (gy < mo && gx < no) {
      v = in[b * band + (size_t)gy * no + gx];
      if (b > 0) v = wv_shrink(v, th[b - 1], mode);
    }
    s_b[e] = v;
  }
  __syncthreads();
  // axis 1: column 2 qx + p of patch row r, from (aa, ad) and from (da, dd)
  for (int e = tid; e < Q * W; e += WV_THREADS) {
    const int r = e / W, cc = e - r * W;
    const int qx = cc >> 1, p = cc & 1;
    const double* a0 = s_b + r * Q + qx + H - 1;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    for (int j = 0; j < H; ++j) s1 = s1 + s_f[2 * j + p] * a0[-j];
    for (int j = 0; j < H; ++j) s2 = s2 + s_f[WV_TAPS_MAX + 2 * j + p] * a0[Q * Q - j];
    for (int j = 0; j < H; ++j) s3 = s3 + s_f[2 * j + p] * a0[2 * Q * Q - j];
    for (int j = 0; j < H; ++j) s4 = s4 + s_f[WV_TAPS_MAX + 2 * j + p] * a0[3 * Q * Q - j];
    s_lo[e] = (0.0 + s1) + s2;
    s_hi[e] = (0.0 + s3) + s4;
  }
  __syncthreads();
  double* out = dst ? dst[img0 + blockIdx.z] : pyr + off_out;
#pragma unroll
  for (int py = 0; py < 2; ++py) {
    const int oy = 2 * (qy0 + threadIdx.y) + py;
#pragma unroll
    for (int px = 0; px < 2; ++px) {
      const int cc = 2 * threadIdx.x + px, ox = 2 * qx0 + cc;
      if (oy >= m_out || ox >= n_out) continue;
      const double* l0 = s_lo + (threadIdx.y + H - 1) * W + cc;
      const double* h0 = s_hi + (threadIdx.y + H - 1) * W + cc;
      double s1 = 0.0, s2 = 0.0;
      for (int j = 0; j < H; ++j) s1 = s1 + s_f[2 * j + py] * l0[-j * W];
      for (int j = 0; j < H; ++j) s2 = s2 + s_f[WV_TAPS_MAX + 2 * j + py] * h0[-j * W];
      double v = (0.0 + s1) + s2;
      if (clip) v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
      out[(size_t)oy * n_out + ox] = v;
    }
  }
}
