// Part of gpet_kernels.hip (included there, inside namespace gpet, in this order): launchers (and the kernels of the many-training-points predict, the Philox generator, small utilities).
// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------

hipError_t launch_conv(hipStream_t st, const double* d_img, int M, int N, const double* d_wf, int kh, int kw, int oy,
                       int ox, float* d_tmp, unsigned int* d_minmax) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  dim3 bs(64, 4), gs(cdiv(N, 64), cdiv(M, CONV_RY));
  const size_t lds = ((size_t)kh * kw + (size_t)(CONV_RY + kh - 1) * (64 + kw - 1)) * sizeof(double);
  if (lds > 64 * 1024) return hipErrorInvalidValue;  // (a kernel of hundreds of taps per side: not the reference's use)
  hipLaunchKernelGGL(k_conv_relu, gs, bs, lds, st, d_img, M, N, d_wf, kh, kw, oy, ox, d_tmp, d_minmax);
  return hipGetLastError();
}
hipError_t launch_minmax(hipStream_t st, const float* d_in, size_t count, unsigned int* d_minmax) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  int blocks = (int)((count + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_minmax_f32, dim3(blocks), dim3(256), 0, st, d_in, count, d_minmax);
  return hipGetLastError();
}
hipError_t launch_normalise(hipStream_t st, const float* d_in, size_t count, const unsigned int* d_minmax,
                            float* d_out) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  int blocks = (int)((count + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_normalise_f32, dim3(blocks), dim3(256), 0, st, d_in, count, d_minmax, d_out);
  return hipGetLastError();
}

// raw frames of a stack -> unnormalised f32 gradient images: images img0 .. img0 + n - 1 of the device pointer tables d_src /
// d_dst in ONE launch (geometry: gpet_conv_plan.h); d_minmax holds a (min, max) slot per image of the stack
static_assert(CONV_RY == CONV_TILE_Y && CONV_TILE_X == 64, "k_conv_relu_batch tiles as gpet_conv_plan.h says");
template <typename T>
static hipError_t launch_conv_batch_t(hipStream_t st, const void* const* d_src, int img0, int n, int M, int N, const double* d_wf,
                                      int kh, int kw, float* const* d_dst, unsigned int* d_minmax) {
  const ConvGrid cg = conv_grid(M, N);
  hipLaunchKernelGGL(k_conv_relu_batch<T>, dim3(cg.gx, cg.gy, n), dim3(64, 4), conv_lds_bytes(kh, kw), st, (const T* const*)d_src, img0,
                     M, N, d_wf, kh, kw, conv_origin(kh), conv_origin(kw), d_dst, d_minmax);
  return hipGetLastError();
}
// (a grid holds 65 535 images along z or y: a longer stack takes more than one launch)
hipError_t launch_conv_batch(hipStream_t st, int pix, const void* const* d_src, int img0, int n, int M, int N, const double* d_wf,
                             int kh, int kw, float* const* d_dst, unsigned int* d_minmax) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  if (!conv_fits_lds(kh, kw) || n < 1 || pix_bytes(pix) == 0) return hipErrorInvalidValue;
  for (int i = 0; i < n; i += 65535) {
    const int m = n - i < 65535 ? n - i : 65535;
    hipError_t e = hipSuccess;
    switch (pix) {
      case PIX_U8: e = launch_conv_batch_t<uint8_t>(st, d_src, img0 + i, m, M, N, d_wf, kh, kw, d_dst, d_minmax); break;
      case PIX_U16: e = launch_conv_batch_t<uint16_t>(st, d_src, img0 + i, m, M, N, d_wf, kh, kw, d_dst, d_minmax); break;
      case PIX_F32: e = launch_conv_batch_t<float>(st, d_src, img0 + i, m, M, N, d_wf, kh, kw, d_dst, d_minmax); break;
      default: e = launch_conv_batch_t<double>(st, d_src, img0 + i, m, M, N, d_wf, kh, kw, d_dst, d_minmax); break;
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
// frames frame0 .. frame0 + n - 1 of d_src -> the unnormalised f32 gradient images of all their slots in ONE launch: the device
// tables of gpet_conv_multi_plan.h (taps of all kernels, kernel descriptors, slots of each frame, kernel of each slot), d_dst and
// d_minmax per SLOT
template <typename T>
static hipError_t launch_conv_multi_t(hipStream_t st, const void* const* d_src, int frame0, int n, int M, int N, const double* d_wf,
                                      const ConvUnion& u, const ConvKernDesc* d_kd, const int32_t* d_slot_off, const int32_t* d_slot_list,
                                      const int32_t* d_kernel_of, float* const* d_dst, unsigned int* d_minmax) {
  const ConvGrid cg = conv_grid(M, N);
  hipLaunchKernelGGL(k_conv_relu_multi<T>, dim3(cg.gx, cg.gy, n), dim3(64, 4), conv_union_lds_bytes(u), st, (const T* const*)d_src, frame0,
                     M, N, d_wf, (int)u.taps, d_kd, u.top, u.left, conv_union_rows(u), conv_union_cols(u), d_slot_off, d_slot_list,
                     d_kernel_of, d_dst, d_minmax);
  return hipGetLastError();
}
hipError_t launch_conv_multi(hipStream_t st, int pix, const void* const* d_src, int frame0, int n, int M, int N, const double* d_wf,
                             const ConvUnion& u, const ConvKernDesc* d_kd, const int32_t* d_slot_off, const int32_t* d_slot_list,
                             const int32_t* d_kernel_of, float* const* d_dst, unsigned int* d_minmax) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  if (u.taps == 0 || conv_union_lds_bytes(u) > CONV_LDS_MAX || n < 1 || pix_bytes(pix) == 0) return hipErrorInvalidValue;
  for (int i = 0; i < n; i += 65535) {
    const int m = n - i < 65535 ? n - i : 65535;
    hipError_t e = hipSuccess;
    switch (pix) {
      case PIX_U8: e = launch_conv_multi_t<uint8_t>(st, d_src, frame0 + i, m, M, N, d_wf, u, d_kd, d_slot_off, d_slot_list, d_kernel_of, d_dst, d_minmax); break;
      case PIX_U16: e = launch_conv_multi_t<uint16_t>(st, d_src, frame0 + i, m, M, N, d_wf, u, d_kd, d_slot_off, d_slot_list, d_kernel_of, d_dst, d_minmax); break;
      case PIX_F32: e = launch_conv_multi_t<float>(st, d_src, frame0 + i, m, M, N, d_wf, u, d_kd, d_slot_off, d_slot_list, d_kernel_of, d_dst, d_minmax); break;
      default: e = launch_conv_multi_t<double>(st, d_src, frame0 + i, m, M, N, d_wf, u, d_kd, d_slot_off, d_slot_list, d_kernel_of, d_dst, d_minmax); break;
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
// the n images of d_imgs normalised in place, each by its own slot of d_minmax, in one launch
hipError_t launch_normalise_batch(hipStream_t st, float* const* d_imgs, int n, size_t count, const unsigned int* d_minmax) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  if (n < 1) return hipErrorInvalidValue;
  int blocks = (int)((count + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  for (int i = 0; i < n; i += 65535)
    hipLaunchKernelGGL(k_normalise_f32_batch, dim3(blocks, n - i < 65535 ? n - i : 65535), dim3(256), 0, st, d_imgs, i, count, d_minmax);
  return hipGetLastError();
}

// ---- a0: denoising of a chunk of raw frames (gpet_k_denoise.inc; geometry and workspace: gpet_denoise_plan.h) ----
static_assert(sizeof(TvcState) == DN_TVC_STATE_BYTES, "the plan reserves k_dn_tvc_check's state");
static_assert((CONV_RY + 1) * 65 * 2 * sizeof(double) == DN_TVC_LDS_BYTES, "k_dn_tvc_iter tiles as gpet_denoise_plan.h says");
template <typename T>
static void launch_dn_rank_t(hipStream_t st, const void* const* d_src, int img0, int n, int M, int N, const DenoiseSpec& s, char* ws,
                             const DenoiseLayout& L, int pix) {
  const ConvGrid cg = conv_grid(M, N);
  const dim3 gs(cg.gx, cg.gy, n), bs(64, 4);
  const size_t lds = dn_rank_lds_bytes(s.size_y, s.size_x, pix);
  const int rank = dn_rank(s.technique, s.size_y, s.size_x);
  const T* const* src = (const T* const*)d_src;
  if (s.size_y == 3 && s.size_x == 3)
    hipLaunchKernelGGL((k_dn_rank<T, 3, 3>), gs, bs, lds, st, src, img0, ws, L.img_bytes, L.off_out, M, N, 3, 3, rank, s.mode);
  else if (s.size_y == 5 && s.size_x == 5)
    hipLaunchKernelGGL((k_dn_rank<T, 5, 5>), gs, bs, lds, st, src, img0, ws, L.img_bytes, L.off_out, M, N, 5, 5, rank, s.mode);
  else
    hipLaunchKernelGGL((k_dn_rank<T, 0, 0>), gs, bs, lds, st, src, img0, ws, L.img_bytes, L.off_out, M, N, s.size_y, s.size_x, rank, s.mode);
}
// (a grid holds 65 535 images along z: a longer chunk takes more than one launch)
hipError_t launch_dn_rank(hipStream_t st, int pix, const void* const* d_src, int img0, int n, int M, int N, const DenoiseSpec& s,
                          char* ws, const DenoiseLayout& L) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  if (dn_check(s, pix) || (s.technique != DN_MEDIAN && s.technique != DN_MINIMUM) || n < 1) return hipErrorInvalidValue;
  for (int i = 0; i < n; i += 65535) {
    const int m = n - i < 65535 ? n - i : 65535;
    char* w = ws + (size_t)i * L.img_bytes;
    switch (pix) {
      case PIX_U8: launch_dn_rank_t<uint8_t>(st, d_src, img0 + i, m, M, N, s, w, L, pix); break;
      case PIX_U16: launch_dn_rank_t<uint16_t>(st, d_src, img0 + i, m, M, N, s, w, L, pix); break;
      case PIX_F32: launch_dn_rank_t<float>(st, d_src, img0 + i, m, M, N, s, w, L, pix); break;
      default: launch_dn_rank_t<double>(st, d_src, img0 + i, m, M, N, s, w, L, pix); break;
    }
  }
  return hipGetLastError();
}
// ---- a0: non-local means (gpet_k_nlmeans.inc; geometry: gpet_nlmeans_plan.h) ----
template <typename T>
static void launch_nlmeans_t(hipStream_t st, const void* const* d_src, double* const* d_dst, int img0, int n, int M, int N, int s, int d,
                             const double* d_taps, double var2) {
  const NlmGrid g = nlm_grid(M, N);
  const dim3 gs(g.gx, g.gy, n), bs(NLM_TILE, NLM_TILE);
  const size_t lds = nlm_lds_bytes(s, d);
  const T* const* src = (const T* const*)d_src;
  if (s == 7)
    hipLaunchKernelGGL((k_nlmeans<T, 7>), gs, bs, lds, st, src, d_dst, img0, M, N, s, d, d_taps, var2);
  else
    hipLaunchKernelGGL((k_nlmeans<T, 0>), gs, bs, lds, st, src, d_dst, img0, M, N, s, d, d_taps, var2);
}
hipError_t launch_nlmeans(hipStream_t st, int pix, const void* const* d_src, double* const* d_dst, int img0, int n, int M, int N, int s,
                          int d, const double* d_taps, double var2) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  const NlmGrid g = nlm_grid(M, N);
  if (!pix_bytes(pix) || n < 1 || s < 3 || s % 2 == 0 || s > NLM_PATCH_MAX || d < 0 || d > NLM_DIST_MAX || s / 2 >= (M < N ? M : N) ||
      nlm_lds_bytes(s, d) > NLM_LDS_MAX || g.gy > 65535)
    return hipErrorInvalidValue;
  for (int i = 0; i < n; i += 65535) {
    const int m = n - i < 65535 ? n - i : 65535;
    switch (pix) {
      case PIX_U8: launch_nlmeans_t<uint8_t>(st, d_src, d_dst, img0 + i, m, M, N, s, d, d_taps, var2); break;
      case PIX_U16: launch_nlmeans_t<uint16_t>(st, d_src, d_dst, img0 + i, m, M, N, s, d, d_taps, var2); break;
      case PIX_F32: launch_nlmeans_t<float>(st, d_src, d_dst, img0 + i, m, M, N, s, d, d_taps, var2); break;
      default: launch_nlmeans_t<double>(st, d_src, d_dst, img0 + i, m, M, N, s, d, d_taps, var2); break;
    }
  }
  return hipGetLastError();
}
template <typename T>
static void launch_dn_gauss_t(hipStream_t st, const void* const* d_src, int img0, int n, int M, int N, const DenoiseSpec& s,
                              const double* d_wy, const double* d_wx, char* ws, const DenoiseLayout& L) {
  const dim3 gs(cdiv(N, 64), cdiv(M, 4), n), bs(64, 4);
  // axis 0 first: frame -> tmp, then axis 1: tmp -> out, each stored in the frame's type as scipy stores it
  hipLaunchKernelGGL(k_dn_gauss_pass<T>, gs, bs, 0, st, (const T* const*)d_src, img0, ws, L.img_bytes, (size_t)0, L.off_tmp, M, N, 0, d_wy,
                     dn_gauss_radius(s.sigma_y, s.truncate), s.mode);
  hipLaunchKernelGGL(k_dn_gauss_pass<T>, gs, bs, 0, st, (const T* const*)nullptr, img0, ws, L.img_bytes, L.off_tmp, L.off_out, M, N, 1, d_wx,
                     dn_gauss_radius(s.sigma_x, s.truncate), s.mode);
}
hipError_t launch_dn_gauss(hipStream_t st, int pix, const void* const* d_src, int img0, int n, int M, int N, const DenoiseSpec& s,
                           const double* d_wy, const double* d_wx, char* ws, const DenoiseLayout& L) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  if (dn_check(s, pix) || s.technique != DN_GAUSSIAN || n < 1 || cdiv(M, 4) > 65535) return hipErrorInvalidValue;
  for (int i = 0; i < n; i += 65535) {
    const int m = n - i < 65535 ? n - i : 65535;
    char* w = ws + (size_t)i * L.img_bytes;
    switch (pix) {
      case PIX_U8: launch_dn_gauss_t<uint8_t>(st, d_src, img0 + i, m, M, N, s, d_wy, d_wx, w, L); break;
      case PIX_U16: launch_dn_gauss_t<uint16_t>(st, d_src, img0 + i, m, M, N, s, d_wy, d_wx, w, L); break;
      case PIX_F32: launch_dn_gauss_t<float>(st, d_src, img0 + i, m, M, N, s, d_wy, d_wx, w, L); break;
      default: launch_dn_gauss_t<double>(st, d_src, img0 + i, m, M, N, s, d_wy, d_wx, w, L); break;
    }
  }
  return hipGetLastError();
}
template <typename T>
static void launch_dn_tvc_t(hipStream_t st, const void* const* d_src, int img0, int n, int M, int N, int it, double tau_w, char* ws,
                            const DenoiseLayout& L) {
  const ConvGrid cg = conv_grid(M, N);
  hipLaunchKernelGGL(k_dn_tvc_iter<T>, dim3(cg.gx, cg.gy, n), dim3(64, 4), 0, st, (const T* const*)d_src, img0, ws, L.img_bytes, L.off_out,
                     L.off_p, L.plane_bytes, L.off_part, M, N, it, tau_w);
}
hipError_t launch_dn_tvc_iter(hipStream_t st, int pix, const void* const* d_src, int img0, int n, int M, int N, const DenoiseSpec& s,
                              int it, char* ws, const DenoiseLayout& L, int* d_n_iter, int* d_n_done) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  if (dn_check(s, pix) || s.technique != DN_TVC || n < 1 || it < 0) return hipErrorInvalidValue;
  const double tau_w = 0.25 / s.weight;  // (the reference's `tau / weight`, formed once)
  for (int i = 0; i < n; i += 65535) {
    const int m = n - i < 65535 ? n - i : 65535;
    char* w = ws + (size_t)i * L.img_bytes;
    switch (pix) {
      case PIX_U8: launch_dn_tvc_t<uint8_t>(st, d_src, img0 + i, m, M, N, it, tau_w, w, L); break;
      case PIX_U16: launch_dn_tvc_t<uint16_t>(st, d_src, img0 + i, m, M, N, it, tau_w, w, L); break;
      case PIX_F32: launch_dn_tvc_t<float>(st, d_src, img0 + i, m, M, N, it, tau_w, w, L); break;
      default: launch_dn_tvc_t<double>(st, d_src, img0 + i, m, M, N, it, tau_w, w, L); break;
    }
  }
  hipLaunchKernelGGL(k_dn_tvc_check, dim3(n), dim3(256), 0, st, ws, L.img_bytes, L.off_part, L.n_wg, img0, it, s.weight, s.eps,
                     (double)((size_t)M * N), d_n_iter, d_n_done);
  return hipGetLastError();
}

// ---- a5 for many training points (generic path): K_*^T rows into V, mean, blocked V = L^-1 K_*^T, std ----
__global__ void __launch_bounds__(256) k_kstar_build(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.z];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int n = sc->n, Lg = E.Lg;
  const int j = blockIdx.x * 64 + (threadIdx.x & 63);
  const double amp = sc->amp, length = E.length_scale;
  if (j >= Lg) return;
  const double xq = (double)(E.x_st + j) / length;
  for (int i = blockIdx.y * 4 + (threadIdx.x >> 6); i < n; i += gridDim.y * 4)
    E.V[(size_t)i * Lg + j] = amp * corr_px(E, (double)(E.x_st + j), E.xt[i], length);
}
// block k0 of V = L^-1 K_*^T for 32 columns of the grid per workgroup, on the matrix cores:
//   X = K_*^T[k0.., cols] - sum_{j0 < k0} L[k0.., j0..] V[j0.., cols]   (64 x 64 by 64 x 32 products, left-looking),
//   V[k0.., cols] = L_kk^-1 X   (the inverse of the diagonal block from k_chol_diag).
// Wave w owns rows 16 w .. 16 w + 15 of the block and both 16-column halves.
#ifndef VS_COLS
#define VS_COLS 16  // grid columns per workgroup (16, 32 or 64 by -DVS_COLS=..; at n = 1500, Lg = 2048: 3.42 / 3.62 / 4.09 ms per fit + predict + covariance)
#endif
#define VS_NH (VS_COLS / 16)          // 16-column halves per wave
#define VS_PU (CB * VS_COLS / 256)    // prefetch registers of the V block per thread
__global__ void __launch_bounds__(256) k_vsolve_mfma(EdgeDev* edges, int k0) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int n = sc->n, Lg = E.Lg, ld = E.n_cap;
  const int a0 = blockIdx.x * VS_COLS;
  if (k0 >= n || a0 >= Lg) return;
  const int nb = (n - k0) < CB ? (n - k0) : CB;
  __shared__ double sL[CB][CB + 1];
  __shared__ double sU[CB][VS_COLS + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lq = lane >> 4;
  v4f64c acc[VS_NH];
#pragma unroll
  for (int h = 0; h < VS_NH; ++h) acc[h] = (v4f64c){0.0, 0.0, 0.0, 0.0};
  // the blocks of the next j0 are loaded into registers while the matrix cores work on the current ones (a launch has
  // only Lg / 32 workgroups: nothing else hides the two dependent round trips per block otherwise -- 85 -> ~25 us)
  double pl[16], pu[VS_PU];
  auto fetch = [&](int j0) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int e = tid + 256 * u, i = e >> 6, t = e & 63;
      pl[u] = (i < nb) ? E.K[(size_t)(k0 + i) * ld + j0 + t] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < VS_PU; ++u) {
      const int e = tid + 256 * u, t = e / VS_COLS, a = e % VS_COLS;
      pu[u] = (a0 + a < Lg) ? E.V[(size_t)(j0 + t) * Lg + a0 + a] : 0.0;
    }
  };
  if (k0 > 0) fetch(0);
  for (int j0 = 0; j0 < k0; j0 += CB) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int e = tid + 256 * u;
      sL[e >> 6][e & 63] = pl[u];
    }
#pragma unroll
    for (int u = 0; u < VS_PU; ++u) {
      const int e = tid + 256 * u;
      sU[e / VS_COLS][e % VS_COLS] = pu[u];
    }
    __syncthreads();
    if (j0 + CB < k0) fetch(j0 + CB);
#pragma unroll
    for (int kk = 0; kk < CB; kk += 4) {
      const double a = sL[16 * w + li][kk + lq];
#pragma unroll
      for (int h = 0; h < VS_NH; ++h) acc[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sU[kk + lq][16 * h + li], acc[h], 0, 0, 0);
    }
  }
  __syncthreads();
  // X = B - acc into sU (rows of the block beyond n: zero), the inverse into sL
  const double* inv = E.chol_inv + (size_t)(k0 / CB) * CB * CB;
  for (int e = tid; e < CB * CB; e += 256) sL[e >> 6][e & 63] = inv[e];
#pragma unroll
  for (int h = 0; h < VS_NH; ++h)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int i = 16 * w + lq + 4 * g, a = 16 * h + li;
      sU[i][a] = (i < nb && a0 + a < Lg) ? E.V[(size_t)(k0 + i) * Lg + a0 + a] - acc[h][g] : 0.0;
    }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < VS_NH; ++h) acc[h] = (v4f64c){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < CB; kk += 4) {
    const double a = sL[16 * w + li][kk + lq];
#pragma unroll
    for (int h = 0; h < VS_NH; ++h) acc[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sU[kk + lq][16 * h + li], acc[h], 0, 0, 0);
  }
#pragma unroll
  for (int h = 0; h < VS_NH; ++h)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int i = 16 * w + lq + 4 * g, a = 16 * h + li;
      if (i < nb && a0 + a < Lg) E.V[(size_t)(k0 + i) * Lg + a0 + a] = acc[h][g];
    }
}

// Column sums over the n rows of V for many training points: a workgroup owns 16 grid columns, its 16 row-lanes take every
// sixteenth row each (independent loads, a wave reads four rows of 128 contiguous bytes per instruction) and their
// partial sums are added in row-lane order.  (One thread per column walking all n rows -- Lg / 256 workgroups on the
// whole GPU -- took 0.39 + 0.36 ms at n = 1500, Lg = 2048.)
//   STD = false: mean_j = y_std * sum_i K_*[i][j] alpha_i + y_mean   (sklearn_gpr.py:381-385; before V is overwritten)
//   STD = true:  std_j = sqrt(max(amp - sum_i V[i][j]^2, 0) * y_std^2)   (sklearn_gpr.py:414-436)
#define PB_COLS 16
#define PB_LANES 16
template <bool STD>
__global__ void __launch_bounds__(PB_COLS * PB_LANES) k_pred_colsum_big(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  __shared__ double s_part[PB_LANES][PB_COLS + 1];
  const int n = sc->n, Lg = E.Lg;
  const int c = threadIdx.x & (PB_COLS - 1), r = threadIdx.x / PB_COLS;
  const int j = blockIdx.x * PB_COLS + c;
  const GPET_GLOBAL double* __restrict__ Vg = as_global(E.V);
  const GPET_GLOBAL double* __restrict__ al = as_global(E.alpha);
  double sum = 0.0;
  if (j < Lg) {
#pragma unroll 8
    for (int i = r; i < n; i += PB_LANES) {
      const double v = Vg[(size_t)i * Lg + j];
      sum += STD ? v * v : v * al[i];
    }
  }
  s_part[r][c] = sum;
  __syncthreads();
  if (r == 0 && j < Lg) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < PB_LANES; ++q) t += s_part[q][c];
    if (STD) {
      double var = sc->amp - t;
      if (var < 0.0) var = 0.0;
      E.std[j] = sqrt(var * (sc->y_std * sc->y_std));
    } else {
      E.mean[j] = sc->y_std * t + sc->y_mean;
    }
  }
}

// hipFuncSetAttribute applies to the CURRENT device: remember per device what has been raised, so that one process
// may hold contexts on several GPUs (the launchers run with the context's device current).
struct PerDeviceOnce {
  bool done[64] = {};
  bool first() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return true;
    if (done[d]) return false;
    done[d] = true;
    return true;
  }
};

static void fit_predict_attrs() {
  static PerDeviceOnce once;
  if (!once.first()) return;
  (void)hipFuncSetAttribute((const void*)k_fit<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
  (void)hipFuncSetAttribute((const void*)k_fit<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
  (void)hipFuncSetAttribute((const void*)k_predict<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
  (void)hipFuncSetAttribute((const void*)k_predict<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
}

hipError_t launch_fit_predict(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, int want_cov, unsigned parts) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  fit_predict_attrs();
  if (!(parts & 1u)) {
  } else if (bd.n_cap <= 128)
    hipLaunchKernelGGL((k_fit<true, false>), dim3(1, B), dim3(576),
                       ((size_t)bd.n_cap * (bd.n_cap | 1) + bd.n_cap) * sizeof(double), st, d_edges);
  else
    launch_fit_blocked(st, d_edges, B, bd);
  const size_t plds = ((size_t)bd.n_cap * 64 + 3 * (size_t)bd.n_cap) * sizeof(double);
  if (!(parts & 2u)) {
  } else if (bd.n_cap > 128 && plds > 150 * 1024) {
    // many training points: V through HBM, blocked substitution with the panel kernel of the structured path
    hipLaunchKernelGGL(k_kstar_build, dim3(cdiv(bd.Lg, 64), 64, B), dim3(256), 0, st, d_edges);
    hipLaunchKernelGGL(k_pred_colsum_big<false>, dim3(cdiv(bd.Lg, PB_COLS), B), dim3(PB_COLS * PB_LANES), 0, st, d_edges);
    for (int k0 = 0; k0 < bd.n_cap; k0 += CB)
      hipLaunchKernelGGL(k_vsolve_mfma, dim3(cdiv(bd.Lg, VS_COLS), B), dim3(256), 0, st, d_edges, k0);
    hipLaunchKernelGGL(k_pred_colsum_big<true>, dim3(cdiv(bd.Lg, PB_COLS), B), dim3(PB_COLS * PB_LANES), 0, st, d_edges);
  } else if (plds <= 150 * 1024)
    hipLaunchKernelGGL((k_predict<true, false>), dim3(cdiv(bd.Lg, 64), B), dim3(64), plds, st, d_edges, 0);
  else
    hipLaunchKernelGGL((k_predict<false, false>), dim3(cdiv(bd.Lg, 64), B), dim3(64), 0, st, d_edges, 0);
  if (want_cov && (parts & 4u)) {
    const int t = cdiv(bd.Lg, 64);
    hipLaunchKernelGGL(k_cov_mfma, dim3(t, t, B), dim3(256), 0, st, d_edges, 0);
  }
  return hipGetLastError();
}

hipError_t launch_final_cov(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd) {
  (void)hipGetLastError();
  const int t = cdiv(bd.Lg, 64);
  hipLaunchKernelGGL(k_cov_mfma, dim3(t, t, B), dim3(256), 0, st, d_edges, 1);
  return hipGetLastError();
}

// converged fit at the optimum: factor + alpha, then mean/std on the standardised grid
hipError_t launch_final_predict(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd) {
  (void)hipGetLastError();
  fit_predict_attrs();
  if (bd.n_cap <= 128)
    hipLaunchKernelGGL((k_fit<true, true>), dim3(1, B), dim3(576),
                       ((size_t)bd.n_cap * (bd.n_cap | 1) + bd.n_cap) * sizeof(double), st, d_edges);
  else
    hipLaunchKernelGGL((k_fit<false, true>), dim3(1, B), dim3(256), (size_t)bd.n_cap * sizeof(double), st, d_edges);
  const size_t plds = ((size_t)bd.n_cap * 64 + 3 * (size_t)bd.n_cap) * sizeof(double);
  if (plds <= 150 * 1024)
    hipLaunchKernelGGL((k_predict<true, true>), dim3(cdiv(bd.Lg, 64), B), dim3(64), plds, st, d_edges, bd.Lg);
  else
    hipLaunchKernelGGL((k_predict<false, true>), dim3(cdiv(bd.Lg, 64), B), dim3(64), 0, st, d_edges, bd.Lg);
  return hipGetLastError();
}

static void launch_jacobi_small(hipStream_t st, EdgeDev* d_edges, int B, int rank_max, int scaled_out, bool logw) {
  const int mm = (rank_max + 1) & ~1;
  static PerDeviceOnce once;
  if (once.first()) {
    (void)hipFuncSetAttribute((const void*)k_jacobi_prerot<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    (void)hipFuncSetAttribute((const void*)k_jacobi_prerot<5>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    (void)hipFuncSetAttribute((const void*)k_jacobi_prerot<6>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
#define GPET_JS_ATTR(NU_, LOGW_) \
  (void)hipFuncSetAttribute((const void*)k_jacobi_seat<NU_, LOGW_>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024)
    GPET_JS_ATTR(2, true); GPET_JS_ATTR(3, true);
    GPET_JS_ATTR(2, false); GPET_JS_ATTR(3, false);
#undef GPET_JS_ATTR
#define GPET_JA_ATTR(NU_, LOGW_, RR_, NT_) \
  (void)hipFuncSetAttribute((const void*)k_jacobi_ahead<NU_, LOGW_, RR_, NT_>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024)
    GPET_JA_ATTR(2, true, 0, JA_NT_LOG); GPET_JA_ATTR(3, true, 0, JA_NT_LOG);
    GPET_JA_ATTR(3, false, 0, JS_NT); GPET_JA_ATTR(2, false, 6, JS_NT);
#undef GPET_JA_ATTR
  }
  // warm start (structured loop only: there the matrix of an iteration is a small change of the last one's)
  const int warm = scaled_out ? opt(Opt::jacobi_warm) : 0;
  if (warm) {
    const int nt = (rank_max + 15) >> 4;
#define GPET_PR_LAUNCH(NT_)                                                                                                \
  hipLaunchKernelGGL(k_jacobi_prerot<NT_>, dim3(1, B), dim3(64 * NT_),                                                       \
                     (size_t)2 * (16 * NT_) * ((16 * NT_) % 32 == 16 ? 16 * NT_ : 16 * NT_ + 16) * sizeof(double), st, d_edges, warm)
    if (nt <= 2) GPET_PR_LAUNCH(2);
    else if (nt == 3) GPET_PR_LAUNCH(3);
    else if (nt == 4) GPET_PR_LAUNCH(4);
    else if (nt == 5) GPET_PR_LAUNCH(5);
    else GPET_PR_LAUNCH(6);
#undef GPET_PR_LAUNCH
  }
  if (opt(Opt::jacobi_variant) != 0) {
    // parameters one round ahead, one barrier per round (k_jacobi_ahead): the matrix twice in LDS
    const size_t nblk = (size_t)(mm / 2) * (mm / 2 + 1) / 2, nbp = (nblk + 1) & ~(size_t)1;
    const dim3 grid(1, B);
    if (logw) {
      const size_t lds = (8 * nbp + 4) * sizeof(double);
      if (nblk <= 2 * (size_t)(JA_NT_LOG - 64)) hipLaunchKernelGGL((k_jacobi_ahead<2, true, 0, JA_NT_LOG>), grid, dim3(JA_NT_LOG), lds, st, d_edges, scaled_out, warm);
      else hipLaunchKernelGGL((k_jacobi_ahead<3, true, 0, JA_NT_LOG>), grid, dim3(JA_NT_LOG), lds, st, d_edges, scaled_out, warm);
      hipLaunchKernelGGL(k_jacobi_wpass, dim3((rank_max + 3) / 4, B), dim3(256), 0, st, d_edges, scaled_out, warm);
    } else {
      // two blocks per thread: the last 7 x 6 components of the eigenvectors in the worker waves' registers (RR = 6), the rest
      // in LDS; three blocks per thread (ranks above 82) have no registers to spare
      const bool three = nblk > 2 * (size_t)(JS_NT - 64);
      const int nreg = three ? 0 : ((7 * 6 < mm ? 7 * 6 : mm) & ~1);
      const size_t lds = (8 * nbp + 4 + (size_t)(mm - nreg) * mm) * sizeof(double);
      if (three) hipLaunchKernelGGL((k_jacobi_ahead<3, false, 0, JS_NT>), grid, dim3(JS_NT), lds, st, d_edges, scaled_out, warm);
      else hipLaunchKernelGGL((k_jacobi_ahead<2, false, 6, JS_NT>), grid, dim3(JS_NT), lds, st, d_edges, scaled_out, warm);
    }
  } else {
    const size_t nblk = (size_t)(mm / 2) * (mm / 2 + 1) / 2;
    const size_t lds = (4 * ((nblk + 1) & ~(size_t)1) + (size_t)mm * mm) * sizeof(double);
    const dim3 grid(1, B), block(JS_NT);
    if (logw) {
      // small batch: rotations logged, eigenvectors by a second kernel (one wave per row of W)
      if (nblk <= 2 * JS_NT) hipLaunchKernelGGL((k_jacobi_seat<2, true>), grid, block, lds, st, d_edges, scaled_out, warm);
      else hipLaunchKernelGGL((k_jacobi_seat<3, true>), grid, block, lds, st, d_edges, scaled_out, warm);
      hipLaunchKernelGGL(k_jacobi_wpass, dim3((rank_max + 3) / 4, B), dim3(256), 0, st, d_edges, scaled_out, warm);
    } else {
      if (nblk > 2 * JS_NT) hipLaunchKernelGGL((k_jacobi_seat<3, false>), grid, block, lds, st, d_edges, scaled_out, warm);
      else hipLaunchKernelGGL((k_jacobi_seat<2, false>), grid, block, lds, st, d_edges, scaled_out, warm);
    }
  }
}

hipError_t launch_factor(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, unsigned parts, const EdgeDev* h_edges,
                         bool single_wg_pchol) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  if (bd.r_cap > 96) return launch_factor_big(st, d_edges, B, bd, h_edges);  // (any rank: csrc/gpet_eig.hip)
  if (!(parts & 1u)) {
  } else if (!single_wg_pchol && pchol_multi_applies(bd)) {
    const hipError_t e = launch_pchol_multi(st, d_edges, B, bd);
    if (e != hipSuccess) return e;
  } else if (bd.Lg <= 512 && bd.r_cap <= PCH_R) {
    hipLaunchKernelGGL(k_pchol_reg, dim3(1, B), dim3(512), 0, st, d_edges);
  } else {
    int pth = bd.Lg >= 1024 ? 1024 : (bd.Lg > 512 ? 1024 : (bd.Lg > 256 ? 512 : 256));
    hipLaunchKernelGGL(k_pchol, dim3(1, B), dim3(pth), (size_t)(bd.Lg + bd.r_cap) * sizeof(double), st, d_edges);
  }
  const int t = cdiv(bd.r_cap, 16);
  if (parts & 2u) hipLaunchKernelGGL(k_gram, dim3(t, t, B), dim3(256), 0, st, d_edges);
  if (parts & 4u) launch_jacobi_small(st, d_edges, B, bd.r_cap, 0, bd.jlog != 0 && opt(Opt::jacobi_logw) != 0);
  if (parts & 8u)
    hipLaunchKernelGGL(k_factor_rows, dim3(bd.r_cap, B), dim3(256), (size_t)bd.r_cap * sizeof(double), st, d_edges);
  return hipGetLastError();
}

// structured loop path: fit -> (U, H, mean) -> Jacobi (the LDS kernel, on E.C) -> factor rows
hipError_t launch_struct_iteration(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, unsigned parts) {
  (void)hipGetLastError();
  fit_predict_attrs();
  static PerDeviceOnce once;
  if (once.first()) {
    (void)hipFuncSetAttribute((const void*)k_struct_H, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    (void)hipFuncSetAttribute((const void*)k_struct_rows<5, 20>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    (void)hipFuncSetAttribute((const void*)k_struct_rows<6, 24>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
  }
  if (!(parts & 1u)) {
  } else if (bd.n_cap <= 128)
    hipLaunchKernelGGL((k_fit<true, false>), dim3(1, B), dim3(576),
                       ((size_t)bd.n_cap * (bd.n_cap | 1) + bd.n_cap) * sizeof(double), st, d_edges);
  else  // (more possible training points than K fits LDS for: blocked factorisation in HBM)
    launch_fit_blocked(st, d_edges, B, bd);
  if ((parts & 2u) && bd.n_cap > 128) {
    // many training points: U through HBM, blocked substitution
    hipLaunchKernelGGL(k_structB_build, dim3(64, B), dim3(256), 0, st, d_edges);
    hipLaunchKernelGGL(k_struct_beta, dim3(1, B), dim3(128), 0, st, d_edges);
    const int cgroups = cdiv(bd.r0_max, SB_COLS);
    for (int k0 = 0; k0 < bd.n_cap; k0 += CB)
      hipLaunchKernelGGL(k_struct_trsm, dim3(cgroups, B), dim3(256), 0, st, d_edges, k0, 0);
    const int t16 = cdiv(bd.r0_max, 16);
    hipLaunchKernelGGL(k_struct_Hbig, dim3(t16, t16, B), dim3(256), 0, st, d_edges);
    hipLaunchKernelGGL(k_struct_mean, dim3(cdiv(bd.Lg, 256), B), dim3(256), 0, st, d_edges);
  } else if (parts & 2u) {
    const size_t full = ((size_t)bd.n_cap * (bd.r0_max | 1) + (size_t)bd.n_cap * (bd.n_cap + 1) / 2 + bd.r_cap) * sizeof(double);
    const size_t rowm = ((size_t)bd.n_cap * (bd.r0_max | 1) + bd.n_cap + bd.r_cap) * sizeof(double);
    const int l_in_lds = full <= (size_t)STRUCT_H_LDS_MAX ? 1 : 0;  // (gpet_batch_create checked that `rowm` fits)
    hipLaunchKernelGGL(k_struct_H, dim3(1, B), dim3(1024), l_in_lds ? full : rowm, st, d_edges, l_in_lds);
  }
  if (parts & 4u) launch_jacobi_small(st, d_edges, B, bd.r0_max > 0 ? bd.r0_max : bd.r_cap, 1, bd.jlog != 0 && opt(Opt::jacobi_logw) != 0);
  if (parts & 8u) {
    // the variant k_struct_rows picks for r0_max: [4 KS][16 MT + 1] eigenvector tile
    const int rm = bd.r0_max;
    const int mt = rm <= 32 ? 2 : rm <= 48 ? 3 : rm <= 64 ? 4 : rm <= 80 ? 5 : 6;
    const int ks = rm <= 32 ? 8 : rm <= 48 ? 12 : rm <= 64 ? 16 : rm <= 72 ? 18 : rm <= 80 ? 20 : 24;
    const size_t lds = ((size_t)4 * ks * (16 * mt + 1) + 16 * mt) * sizeof(double);  // (+ the signs of the rows)
    const dim3 grid(cdiv(bd.Lg, SR_TJ), B);
    if (rm <= 32) hipLaunchKernelGGL((k_struct_rows<2, 8>), grid, dim3(256), lds, st, d_edges);
    else if (rm <= 48) hipLaunchKernelGGL((k_struct_rows<3, 12>), grid, dim3(256), lds, st, d_edges);
    else if (rm <= 64) hipLaunchKernelGGL((k_struct_rows<4, 16>), grid, dim3(256), lds, st, d_edges);
    else if (rm <= 72) hipLaunchKernelGGL((k_struct_rows<5, 18>), grid, dim3(256), lds, st, d_edges);
    else if (rm <= 80) hipLaunchKernelGGL((k_struct_rows<5, 20>), grid, dim3(256), lds, st, d_edges);
    else hipLaunchKernelGGL((k_struct_rows<6, 24>), grid, dim3(256), lds, st, d_edges);
  }
  return hipGetLastError();
}

// construction: eigenbasis of the grid's correlation matrix through the generic factor pipeline
hipError_t launch_struct_basis(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_rho_fill, dim3(256, B), dim3(256), 0, st, d_edges);
  hipError_t e = launch_set_force(st, d_edges, B, 1);
  if (e != hipSuccess) return e;
  e = launch_factor(st, d_edges, B, bd, ~0u, nullptr, true);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_struct_basis, dim3(bd.r_cap, B), dim3(256), 0, st, d_edges);
  return launch_set_force(st, d_edges, B, 0);
}

// ---- opt-in counter-based normals (SURVEY K5 "fast Philox mode"; gpet_batch_set_rng) ---------------------------------
// Philox4x32-10 (Salmon, Moraes, Dror & Shaw, SC'11; the Random123 known-answer vectors are in the tests) + Box-Muller.
// The normal of (sample row s, column j) is a pure function of (seed of the iteration, s, j): counter = (j / 2, s, 0, 0),
// key = (seed, "Phlx"); its four words give two 53-bit uniforms u1, u2 in (0, 1) and the pair
// sqrt(-2 ln u1) (cos 2 pi u2, sin 2 pi u2) for columns j, j + 1.  No stream to walk: every thread writes its own pair, and
// only the columns the factor multiplies are generated at all.  NOT the reference's numbers (sklearn_gpr.py:464 draws from
// RandomState(seed)): a mode of its own with its own CPU twin in the tests (philox_standard_normal), never the default.
__device__ __forceinline__ void philox4x32_10(unsigned int c[4], unsigned int k0, unsigned int k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned int)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (unsigned int)p1;
    c[3] = (unsigned int)p0;
    c[0] = n0;
    c[2] = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}
__global__ void __launch_bounds__(256) k_philox_normals(EdgeDev* edges, const unsigned int* seeds, int add_iter, int iter_abs,
                                                        int z_store) {
  const EdgeDev E = edges[blockIdx.z];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int iter_idx = (iter_abs >= 0 ? iter_abs : sc->iter) + (int)blockIdx.y;
  double* __restrict__ Zs = E.Z + (size_t)(iter_idx % E.z_ring) * ((size_t)E.S * E.z_cols);
  const int zc = E.z_cols, zs = (z_store > 0 && z_store < zc) ? z_store : zc;
  const int hp = (zs + 1) >> 1;  // column pairs per row
  const unsigned int key = seeds[blockIdx.z] + (add_iter ? (unsigned int)(iter_idx + 1) : 0u);  // (the loop's seed rule, gpet.py:839)
  const long long total = (long long)E.S * hp;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int srow = (int)(e / hp), jp = (int)(e - (long long)srow * hp);
    unsigned int c[4] = {(unsigned int)jp, (unsigned int)srow, 0u, 0u};
    philox4x32_10(c, key, 0x50686c78u);
    const double u1 = ((double)(c[0] >> 5) * 67108864.0 + (double)(c[1] >> 6) + 0.5) * (1.0 / 9007199254740992.0);
    const double u2 = ((double)(c[2] >> 5) * 67108864.0 + (double)(c[3] >> 6) + 0.5) * (1.0 / 9007199254740992.0);
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);
    double* o = Zs + (size_t)srow * zc + 2 * jp;
    o[0] = r * cs;
    if (2 * jp + 1 < zs) o[1] = r * sn;
  }
}
hipError_t launch_normals_philox(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, const unsigned int* d_seeds, int add_iter,
                                 int iter_abs, int n_ahead, int z_store) {
  (void)hipGetLastError();
  const int zs = (z_store > 0 && z_store < bd.z_cols) ? z_store : bd.z_cols;
  const long long pairs = (long long)bd.S * ((zs + 1) / 2);
  int gx = (int)((pairs + 256 * 4 - 1) / (256 * 4));  // four pairs per thread
  gx = gx < 1 ? 1 : (gx > 4096 ? 4096 : gx);
  hipLaunchKernelGGL(k_philox_normals, dim3(gx, n_ahead, B), dim3(256), 0, st, d_edges, d_seeds, add_iter, iter_abs, z_store);
  return hipGetLastError();
}

hipError_t launch_normals(hipStream_t st, EdgeDev* d_edges, int B, const unsigned int* d_seeds, int add_iter,
                          int iter_abs, int n_ahead, int z_store) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  // (three waves per workgroup: four were measured 4 % slower, DESIGN 6b)
  hipLaunchKernelGGL((k_mt_normals<false, 3>), dim3(n_ahead, B), dim3(192), 0, st, d_edges, d_seeds, add_iter, iter_abs, z_store, MtjWork{});
  return hipGetLastError();
}

// mode 0: KDE of the best curves -> E.kde ; mode 1: KDE of the gradient image -> E.grad_kde
hipError_t launch_kde(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, int mode, unsigned parts,
                      int raw_band) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  if (mode == 0) {
    // per-iteration path: one prep kernel + one fused bin/convolve kernel + normalise
    const size_t lds = ((size_t)(KDE_TX + 8) * ((KDE_H + 8) | 1) + (size_t)KDE_NB * (KDE_TX + 8) + KDE_NB) * sizeof(double);
    if (parts & 1u) hipLaunchKernelGGL(k_kde_prep, dim3(1, B), dim3(1024), 0, st, d_edges);
    if (parts & 2u)
      hipLaunchKernelGGL(k_kde_fused, dim3(cdiv(bd.N, KDE_TX), B), dim3(KDE_THREADS), lds, st, d_edges, raw_band);
    if ((parts & 4u) && !raw_band) hipLaunchKernelGGL(k_kde_normalise, dim3(64, B), dim3(256), 0, st, d_edges, mode);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_kde_clear, dim3(64, B), dim3(256), 0, st, d_edges, mode);
  hipLaunchKernelGGL(k_kde_bin_gradient, dim3(bd.N, B), dim3(256), 0, st, d_edges);
  hipLaunchKernelGGL(k_kde_wsum, dim3(B), dim3(64), 0, st, d_edges, mode);
  hipLaunchKernelGGL(k_kde_conv_y, dim3(cdiv(bd.M + 2, 256), bd.N + 2, B), dim3(256), 0, st, d_edges, mode);
  hipLaunchKernelGGL(k_kde_conv_x, dim3(cdiv(bd.M, KCX_T), cdiv(bd.N, KCX_T), B), dim3(256), 0, st, d_edges, mode);
  hipLaunchKernelGGL(k_kde_normalise, dim3(64, B), dim3(256), 0, st, d_edges, mode);
  return hipGetLastError();
}

__global__ void __launch_bounds__(256) k_pix_reset(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  for (int i = threadIdx.x; i < E.n_bins; i += blockDim.x) {
    E.binbest[i] = 0ull;
    E.binarg[i] = 0x7FFFFFFFFFFFFFFFll;
  }
}

__global__ void k_set_force(EdgeDev* edges, int v) { edges[blockIdx.x].sc->force = v; }

// training sets of the converged fits: staged as three [B][stride] blocks (x | y | w), scattered to the edges
__global__ void __launch_bounds__(128) k_fin_scatter(EdgeDev* edges, const double* stage, const int* n, int stride, int B) {
  const int e = blockIdx.x;
  EdgeDev& E = edges[e];
  const int ne = n[e];
  for (int i = threadIdx.x; i < ne; i += blockDim.x) {
    E.fin_x[i] = stage[(size_t)e * stride + i];
    E.fin_y[i] = stage[((size_t)B + e) * stride + i];
    E.fin_w[i] = stage[((size_t)2 * B + e) * stride + i];
  }
  if (threadIdx.x == 0) E.fin_n = ne;
}

hipError_t launch_fin_scatter(hipStream_t st, EdgeDev* d_edges, int B, const double* d_stage, const int* d_n, int stride) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_fin_scatter, dim3(B), dim3(128), 0, st, d_edges, d_stage, d_n, stride, B);
  return hipGetLastError();
}

// general-nu Matern: correlation at the integer lags 0..N-1 of the pixel grid, once per edge at construction
__global__ void __launch_bounds__(256) k_rho_tab(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  if (E.kernel_type != GPET_KERNEL_MATERN || E.nu_code != 3) return;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= E.N) return;
  E.rho_tab[k] = matern_gen(E.nu_gen, E.inv_gamma_nu, (double)k / E.length_scale, nullptr);
}
hipError_t launch_rho_tab(hipStream_t st, EdgeDev* d_edges, int B, int N) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_rho_tab, dim3(cdiv(N, 256), B), dim3(256), 0, st, d_edges);
  return hipGetLastError();
}

hipError_t launch_set_force(hipStream_t st, EdgeDev* d_edges, int B, int v) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_set_force, dim3(B), dim3(1), 0, st, d_edges, v);
  return hipGetLastError();
}

hipError_t launch_pixels_reset(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  (void)bd;
  hipLaunchKernelGGL(k_pix_reset, dim3(1, B), dim3(256), 0, st, d_edges);
  return hipGetLastError();
}

hipError_t launch_pixels(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, int raw_band, unsigned parts) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  if (parts & 1u) hipLaunchKernelGGL(k_pix_columns, dim3(cdiv(bd.N, PIX_CX), B), dim3(256), 0, st, d_edges, raw_band);
  const int nt = bd.N > bd.obs_cap ? bd.N : bd.obs_cap;
  if (parts & 2u) hipLaunchKernelGGL(k_pix_old, dim3(cdiv(bd.obs_cap, 256), B), dim3(256), 0, st, d_edges, raw_band);
  if (parts & 4u) hipLaunchKernelGGL(k_pix_argbest, dim3(cdiv(nt, 256), B), dim3(256), 0, st, d_edges, raw_band);
  if (parts & 8u) hipLaunchKernelGGL(k_pix_select, dim3(1, B), dim3(64), 0, st, d_edges);
  return hipGetLastError();
}

// The sample GEMM on the f32 matrix cores (bd.y_arith, gpet_batch_set_sample_arith): the capacity rules of the f64 family below --
// GEMM_KMAX, the KS ladder, the column runs ncs -- with one kernel per K extent (every extent fits two workgroups per CU).  The
// register form keeps the posterior mean in LDS; an edge too wide for that (about 15 000 columns) takes the generic form.
static void launch_sample_f32(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, int rank_max) {
  const size_t lds_top = ((size_t)4 * 24 * GEMM32_LDA) * sizeof(float) + ((size_t)bd.Lg + 64) * sizeof(double);
  if (bd.r_cap <= GEMM_KMAX && bd.a_rows_cap <= GEMM_KMAX && lds_top <= (size_t)GEMM_LDS_MAX) {
    const int rm = rank_max > 0 && rank_max <= bd.r_cap ? rank_max : (bd.r_cap > bd.a_rows_cap ? bd.r_cap : bd.a_rows_cap);
    const int ks = (rm + 3) >> 2;
    const int rparts = cdiv(bd.S, 128), ctiles = cdiv(bd.Lg, 64);
    int ncs = cdiv(256, B * rparts);
    ncs = ncs > ctiles ? ctiles : (ncs < 1 ? 1 : ncs);
    if (ncs > 8) ncs = 8;
    const dim3 grid(rparts * ncs, B), block(512);
    {  // (the chunk plus the posterior mean of a wide edge exceed the 64 KB a kernel gets without asking)
      static PerDeviceOnce once;
      if (once.first()) {
        (void)hipFuncSetAttribute((const void*)k_sample_f32_r<8>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)k_sample_f32_r<12>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)k_sample_f32_r<16>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)k_sample_f32_r<18>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)k_sample_f32_r<20>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_MAX);
        (void)hipFuncSetAttribute((const void*)k_sample_f32_r<24>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_MAX);
      }
    }
#define GPET_GEMM32_LAUNCH(KS_)                                                                                     \
  hipLaunchKernelGGL((k_sample_f32_r<KS_>), grid, block,                                                            \
                     ((size_t)4 * KS_ * GEMM32_LDA) * sizeof(float) + ((size_t)bd.Lg + 64) * sizeof(double), st, d_edges, ncs)
    if (ks <= 8) GPET_GEMM32_LAUNCH(8);
    else if (ks <= 12) GPET_GEMM32_LAUNCH(12);
    else if (ks <= 16) GPET_GEMM32_LAUNCH(16);
    else if (ks <= 18) GPET_GEMM32_LAUNCH(18);
    else if (ks <= 20) GPET_GEMM32_LAUNCH(20);
    else GPET_GEMM32_LAUNCH(24);
#undef GPET_GEMM32_LAUNCH
  } else {
    hipLaunchKernelGGL(k_sample_f32, dim3(cdiv(bd.Lg, 64), cdiv(bd.S, 64), B), dim3(256), 0, st, d_edges);
  }
}

hipError_t launch_sample(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, int rank_max) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  if (bd.y_arith) {  // (opt-in; with it off everything below is enqueued as before)
    launch_sample_f32(st, d_edges, B, bd, rank_max);
    return hipGetLastError();
  }
  // rank <= 96 everywhere in the batch (factor capacity): Z rows stay in registers; otherwise
  // (full factors injected by tests, Matern ranks) the K-chunked kernel.  rank_max: the largest rank any
  // edge can have in this launch (r0_max inside the structured loop, else the factor capacity).
  if (bd.r_cap <= GEMM_KMAX && bd.a_rows_cap <= GEMM_KMAX) {
    const int rm = rank_max > 0 && rank_max <= bd.r_cap ? rank_max : (bd.r_cap > bd.a_rows_cap ? bd.r_cap : bd.a_rows_cap);
    const int ks = (rm + 3) >> 2;
    // column runs per row block: while the row blocks alone leave CUs empty (small batches are latency chains)
    const int rparts = cdiv(bd.S, 128), ctiles = cdiv(bd.Lg, 64);
    int ncs = cdiv(256, B * rparts);
    ncs = ncs > ctiles ? ctiles : (ncs < 1 ? 1 : ncs);
    if (ncs > 8) ncs = 8;
    const dim3 grid(rparts * ncs, B), block(512);
    {  // (the chunk plus the posterior mean of a wide edge exceed the 64 KB a kernel gets without asking: 66 KB at K = 96, Lg = 2048)
      static PerDeviceOnce once;
      if (once.first()) {
#define GPET_GEMM_ATTR(KERNEL, KS_)                                                                                       \
  (void)hipFuncSetAttribute((const void*)KERNEL<KS_, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_MAX);  \
  (void)hipFuncSetAttribute((const void*)KERNEL<KS_, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_MAX);   \
  (void)hipFuncSetAttribute((const void*)KERNEL<KS_, false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_MAX); \
  (void)hipFuncSetAttribute((const void*)KERNEL<KS_, true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_MAX)
        GPET_GEMM_ATTR(k_sample_gemm_mfma_r, 8);
        GPET_GEMM_ATTR(k_sample_gemm_mfma_r, 12);
        GPET_GEMM_ATTR(k_sample_gemm_mfma_r, 16);
        GPET_GEMM_ATTR(k_sample_gemm_mfma_r, 18);
        GPET_GEMM_ATTR(k_sample_gemm_mfma_rl, 20);
        GPET_GEMM_ATTR(k_sample_gemm_mfma_rl, 24);
#undef GPET_GEMM_ATTR
      }
    }
    // (an edge too wide for its posterior mean to sit behind the chunk reads it from global memory in the epilogue)
    const int mu_in_lds = ((size_t)4 * 24 * GEMM_LDA + bd.Lg + 64) * sizeof(double) <= (size_t)GEMM_LDS_MAX ? 1 : 0;
#define GPET_GEMM_LAUNCH(KERNEL, KS_)                                                                                                  \
  do {                                                                                                                                 \
    const size_t lds_ = ((size_t)4 * KS_ * GEMM_LDA + (mu_in_lds ? bd.Lg + 64 : 0)) * sizeof(double);                                         \
    if (bd.y_f32 && mu_in_lds) hipLaunchKernelGGL((KERNEL<KS_, true, true>), grid, block, lds_, st, d_edges, ncs);                        \
    else if (bd.y_f32) hipLaunchKernelGGL((KERNEL<KS_, true, false>), grid, block, lds_, st, d_edges, ncs);                               \
    else if (mu_in_lds) hipLaunchKernelGGL((KERNEL<KS_, false, true>), grid, block, lds_, st, d_edges, ncs);                              \
    else hipLaunchKernelGGL((KERNEL<KS_, false, false>), grid, block, lds_, st, d_edges, ncs);                                            \
  } while (0)
    if (ks <= 8) GPET_GEMM_LAUNCH(k_sample_gemm_mfma_r, 8);
    else if (ks <= 12) GPET_GEMM_LAUNCH(k_sample_gemm_mfma_r, 12);
    else if (ks <= 16) GPET_GEMM_LAUNCH(k_sample_gemm_mfma_r, 16);
    else if (ks <= 18) GPET_GEMM_LAUNCH(k_sample_gemm_mfma_r, 18);
    else if (ks <= 20) GPET_GEMM_LAUNCH(k_sample_gemm_mfma_rl, 20);
    else GPET_GEMM_LAUNCH(k_sample_gemm_mfma_rl, 24);
#undef GPET_GEMM_LAUNCH
  } else {
    hipLaunchKernelGGL(k_sample_gemm_mfma, dim3(cdiv(bd.Lg, 64), cdiv(bd.S, 64), B), dim3(256), 0, st, d_edges);
  }
  return hipGetLastError();
}

// the loop's scoring + curve KDE of a small batch with k_score_combine, k_topk_sort and k_kde_prep as ONE launch (k_score_tail);
// false: the shape does not allow it (the caller enqueues launch_score + launch_kde)
bool score_tail_applies(const BatchDims& bd) {
  const size_t lds = (size_t)(2 * SC_PAIRS + 2) * (bd.M | 1) * sizeof(float);
  return lds <= 150 * 1024 && bd.S >= 64 && bd.S <= 1024 && bd.n_keep <= KDE_PREP_MAXB && !opt(Opt::topk_rank);
}
hipError_t launch_score_kde_fused_tail(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd) {
  hipError_t e = launch_score(st, d_edges, B, bd, 1u, true);  // (the tiles only, their partial sums left for k_score_tail)
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_score_tail, dim3(1, B), dim3(1024), 0, st, d_edges);
  return launch_kde(st, d_edges, B, bd, 0, 2u, 1);  // (k_kde_fused, raw band: the loop's form)
}

// the costs of rows 0 .. S - 1 of every edge's sample matrix (S = bd.S: launch_score's first part; S = 1: the one-row views of
// launch_final_costs).  Which kernels run is decided by the BATCH's shape, bd, whatever S is: a row's cost does not depend on S
hipError_t launch_score_rows(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, int S, bool no_combine) {
  (void)hipGetLastError();
  const size_t lds = (size_t)(2 * SC_PAIRS + 2) * (bd.M | 1) * sizeof(float);
  if (lds <= 150 * 1024 && B * 1 > 0 && bd.S >= 64) {
    static PerDeviceOnce once;
    if (once.first())
    {
      (void)hipFuncSetAttribute((const void*)k_score_tile<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
      (void)hipFuncSetAttribute((const void*)k_score_tile<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    }
    const int n_tiles = cdiv((bd.Lg - 2) / 2, SC_PAIRS);
    // curves per workgroup: 1024, or down to 128 while the tiles alone leave CUs empty (every part stages the slab again)
    int cpw = SC_CURVES;
    while (cpw > 128 && B * n_tiles * cdiv(S, cpw) < 256) cpw >>= 1;
    if (bd.y_f32) hipLaunchKernelGGL(k_score_tile<true>, dim3(n_tiles, cdiv(S, cpw), B), dim3(SC_THREADS), lds, st, d_edges, cpw);
    else hipLaunchKernelGGL(k_score_tile<false>, dim3(n_tiles, cdiv(S, cpw), B), dim3(SC_THREADS), lds, st, d_edges, cpw);
    if (!no_combine) hipLaunchKernelGGL(k_score_combine, dim3(cdiv(S, 256), B), dim3(256), 0, st, d_edges, n_tiles);
  } else {
    if (bd.y_f32) hipLaunchKernelGGL(k_score<true>, dim3(cdiv(S, 4), B), dim3(256), 0, st, d_edges);
    else hipLaunchKernelGGL(k_score<false>, dim3(cdiv(S, 4), B), dim3(256), 0, st, d_edges);
  }
  return hipGetLastError();
}

hipError_t launch_score(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, unsigned parts, bool no_combine) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  hipError_t e_rows = hipSuccess;
  if (parts & 1u) e_rows = launch_score_rows(st, d_edges, B, bd, bd.S, no_combine);
  if (parts & 2u) {
    if (bd.S <= 1024 && !opt(Opt::topk_rank)) hipLaunchKernelGGL(k_topk_sort, dim3(1, B), dim3(512), 0, st, d_edges);
    else hipLaunchKernelGGL(k_topk, dim3(cdiv(bd.S, 256), B), dim3(256), 0, st, d_edges);
  }
  const hipError_t e_top = hipGetLastError();
  return e_rows != hipSuccess ? e_rows : e_top;
}

hipError_t launch_history(hipStream_t st, const EdgeDev* d_edges, int B, const gpet_history_plan& P, int iter_expect) {
  (void)hipGetLastError();
  // (the waves beyond four only serve the statistics of level 3: heads, observations and curve are a few hundred stores per edge)
  const int threads = (P.level >= 3 ? HISTORY_WAVES : 4) * WAVE;
  hipLaunchKernelGGL(k_history, dim3(history_tiles(P.level, P.len_cap), B), dim3(threads), 0, st, d_edges, P, iter_expect);
  return hipGetLastError();
}
