// Part of gpet_kernels.hip (included there, inside namespace gpet, in this order): launchers (and three one-line utility kernels).  The launchers of a loop
// iteration only dispatch: gpet_iter_plan.h decides the variant, the grid and the LDS of every step.
// ---------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------

hipError_t launch_conv(hipStream_t st, const double* d_img, int M, int N, const double* d_wf, int kh, int kw, int oy,
                       int ox, float* d_tmp, unsigned int* d_minmax) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  const ConvGrid cg = conv_grid(M, N);
  if (conv_lds_bytes(kh, kw) > CONV_LDS_MAX) return hipErrorInvalidValue;  // (a kernel of hundreds of taps per side: not the reference's use)
  hipLaunchKernelGGL(k_conv_relu, dim3(cg.gx, cg.gy), dim3(64, 4), conv_lds_bytes(kh, kw), st, d_img, M, N, d_wf, kh, kw, oy, ox, d_tmp, d_minmax);
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

// ---- what every launcher over raw frames shares ----
// f(PixTag<T>{}) with the pixel type of a code of gpet_conv_plan.h (any other code: double), and what f returns
template <typename T>
struct PixTag {
  using type = T;
};
template <typename F>
static auto for_pix(int pix, F&& f) {
  switch (pix) {
    case PIX_U8: return f(PixTag<uint8_t>{});
    case PIX_U16: return f(PixTag<uint16_t>{});
    case PIX_F32: return f(PixTag<float>{});
    default: return f(PixTag<double>{});
  }
}
// what the unit of an integer pixel type is worth in [0, 1] (1 for the floating types)
static double pix_unit(int pix) { return pix == PIX_U8 ? 1.0 / 255.0 : pix == PIX_U16 ? 1.0 / 65535.0 : 1.0; }
// a grid holds 65 535 images along z: f(offset, count) for n images in pieces of at most that, up to the first that fails
template <typename F>
static hipError_t for_grid_z(int n, F&& f) {
  for (int i = 0; i < n; i += 65535) {
    const hipError_t e = f(i, n - i < 65535 ? n - i : 65535);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// raw frames of a stack -> unnormalised f32 gradient images: images img0 .. img0 + n - 1 of the device pointer tables d_src /
// d_dst in ONE launch; d_minmax holds a (min, max) slot per image of the stack.  tr: the transposed-store form of a vertical batch --
// an N x M image G.T at every d_dst[g].  Geometry: gpet_conv_plan.h, turned: gpet_transpose_plan.h.
static_assert(CONV_RY == CONV_TILE_Y && CONV_TILE_X == 64, "ConvRows tiles as gpet_conv_plan.h says");
hipError_t launch_conv_batch(hipStream_t st, int pix, bool tr, const void* const* d_src, int img0, int n, int M, int N, const double* d_wf,
                             int kh, int kw, float* const* d_dst, unsigned int* d_minmax) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  if (!(tr ? conv_t_fits_lds(kh, kw) : conv_fits_lds(kh, kw)) || n < 1 || pix_bytes(pix) == 0) return hipErrorInvalidValue;
  const ConvGrid cg = tr ? conv_t_grid(M, N) : conv_grid(M, N);
  if (tr && cg.gy > 65535) return hipErrorInvalidValue;  // (a frame of more than 4 M rows)
  const size_t lds = tr ? conv_t_lds_bytes(kh, kw) : conv_lds_bytes(kh, kw);
  return for_pix(pix, [&](auto t) {
    using T = typename decltype(t)::type;
    const auto kern = tr ? k_conv_tr_batch<T> : k_conv_relu_batch<T>;
    return for_grid_z(n, [&](int i, int m) {
      hipLaunchKernelGGL(kern, dim3(cg.gx, cg.gy, m), dim3(64, 4), lds, st, (const T* const*)d_src, img0 + i, M, N, d_wf, kh, kw,
                         conv_origin(kh), conv_origin(kw), d_dst, d_minmax);
      return hipGetLastError();
    });
  });
}
// frames frame0 .. frame0 + n - 1 of d_src -> the unnormalised f32 gradient images of all their slots in ONE launch: the device
// tables of gpet_conv_multi_plan.h (taps of all kernels, kernel descriptors, slots of each frame, kernel of each slot), d_dst and
// d_minmax per SLOT; tr as above
hipError_t launch_conv_multi(hipStream_t st, int pix, bool tr, const void* const* d_src, int frame0, int n, int M, int N, const double* d_wf,
                             const ConvUnion& u, const ConvKernDesc* d_kd, const int32_t* d_slot_off, const int32_t* d_slot_list,
                             const int32_t* d_kernel_of, float* const* d_dst, unsigned int* d_minmax) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  const size_t lds = tr ? conv_union_t_lds_bytes(u) : conv_union_lds_bytes(u);
  if (u.taps == 0 || lds > CONV_LDS_MAX || n < 1 || pix_bytes(pix) == 0) return hipErrorInvalidValue;
  const ConvGrid cg = tr ? conv_t_grid(M, N) : conv_grid(M, N);
  if (tr && cg.gy > 65535) return hipErrorInvalidValue;
  const int ph = tr ? conv_union_t_rows(u) : conv_union_rows(u), pw = tr ? conv_union_t_cols(u) : conv_union_cols(u);
  return for_pix(pix, [&](auto t) {
    using T = typename decltype(t)::type;
    const auto kern = tr ? k_conv_tr_multi<T> : k_conv_relu_multi<T>;
    return for_grid_z(n, [&](int i, int m) {
      hipLaunchKernelGGL(kern, dim3(cg.gx, cg.gy, m), dim3(64, 4), lds, st, (const T* const*)d_src, frame0 + i, M, N, d_wf, (int)u.taps,
                         d_kd, u.top, u.left, ph, pw, d_slot_off, d_slot_list, d_kernel_of, d_dst, d_minmax);
      return hipGetLastError();
    });
  });
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

// an M x N f32 image -> the N x M one at d_out (d_out != d_in); d_minmax != nullptr: launch_normalise's arithmetic on the way
hipError_t launch_transpose(hipStream_t st, const float* d_in, int M, int N, const unsigned int* d_minmax, float* d_out) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  const TrGrid tg = tr_grid(M, N);
  if (M < 1 || N < 1 || tg.gy > 65535 || d_in == d_out) return hipErrorInvalidValue;
  if (d_minmax)
    hipLaunchKernelGGL(k_transpose_f32<true>, dim3(tg.gx, tg.gy), dim3(TR_TILE, 4), 0, st, d_in, M, N, d_minmax, d_out);
  else
    hipLaunchKernelGGL(k_transpose_f32<false>, dim3(tg.gx, tg.gy), dim3(TR_TILE, 4), 0, st, d_in, M, N, d_minmax, d_out);
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
hipError_t launch_dn_rank(hipStream_t st, int pix, const void* const* d_src, int img0, int n, int M, int N, const DenoiseSpec& s,
                          char* ws, const DenoiseLayout& L) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  if (dn_check(s, pix) || (s.technique != DN_MEDIAN && s.technique != DN_MINIMUM) || n < 1) return hipErrorInvalidValue;
  for_pix(pix, [&](auto t) {  // (here and in the stages below every piece is enqueued; the error is read after the last)
    using T = typename decltype(t)::type;
    (void)for_grid_z(n, [&](int i, int m) {
      launch_dn_rank_t<T>(st, d_src, img0 + i, m, M, N, s, ws + (size_t)i * L.img_bytes, L, pix);
      return hipSuccess;
    });
  });
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
  for_pix(pix, [&](auto t) {
    using T = typename decltype(t)::type;
    (void)for_grid_z(n, [&](int i, int m) {
      launch_nlmeans_t<T>(st, d_src, d_dst, img0 + i, m, M, N, s, d, d_taps, var2);
      return hipSuccess;
    });
  });
  return hipGetLastError();
}
// ---- a0: fast-mode non-local means (gpet_k_nlfast.inc; geometry: gpet_nlfast_plan.h) ----
hipError_t launch_nlfast(hipStream_t st, int pix, const void* const* d_src, double* const* d_dst, int img0, int n, int M, int N,
                         const NlfSpec& sp, const NlfPlan& p, char* ws) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  if (n < 1 || n > NLF_CHUNK_MAX || nlf_check(sp, pix, M, N) || p.rows_per_group < 1 || p.s != nlm_patch(sp.patch_size) || p.d != sp.patch_distance ||
      p.nr != M + 2 * p.pad || p.nc != N + 2 * p.pad)
    return hipErrorInvalidValue;
  const size_t stride = p.frame_bytes / sizeof(double);
  const double var2 = 2.0 * sp.sigma * sp.sigma, h2s2 = ((sp.h * sp.h) * p.s) * p.s;
  for_pix(pix, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((k_nlf_pad<T>), dim3(nlf_pad_blocks(p), 1, n), dim3(NLF_THREADS), 0, st, (const T* const*)d_src, img0, (double*)ws, stride, M, N,
                       p.pad);
  });
  for (int g = 0; g < p.n_groups; ++g) {
    const int first = nlf_group_first(p, g), cnt = nlf_group_count(p, g);
    hipLaunchKernelGGL(k_nlf_integral, dim3(cnt, 1, n), dim3(NLF_STRIP), 0, st, (double*)ws, stride, first, p.d, p.nr, p.nc, p.off_i, var2);
    hipLaunchKernelGGL(k_nlf_gather, dim3(nlf_gather_blocks(M, N), 1, n), dim3(NLF_THREADS), 0, st, (double*)ws, stride, d_dst, img0, M, N, p.off,
                       p.d, first, cnt, g == p.n_groups - 1 ? 1 : 0, p.off_w, p.off_r, p.off_i, h2s2);
  }
  return hipGetLastError();
}
// ---- polar unwrap (gpet_k_polar.inc; the rule and the grid: gpet_polar_plan.h) ----
hipError_t launch_polar(hipStream_t st, int pix, const void* const* d_src, double* const* d_dst, int img0, int n, int M, int N,
                        const PolarSpec& sp, const double* d_cxy, int n_centres, const double* d_cos, const double* d_sin) {
  (void)hipGetLastError();  // drop stale errors: report only this launch
  if (n < 1 || n > POLAR_CHUNK_MAX || !pix_bytes(pix) || M < 2 || N < 2 || sp.n_r < 1 || sp.n_theta < POLAR_NTHETA_MIN || sp.pad < 0 ||
      sp.pad > sp.n_theta || polar_width(sp.n_theta, sp.pad) > POLAR_CELLS_MAX / sp.n_r || n_centres < 1 || !d_cxy || !d_cos || !d_sin)
    return hipErrorInvalidValue;
  const int W = (int)polar_width(sp.n_theta, sp.pad);
  for_pix(pix, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((k_polar<T>), dim3(polar_blocks(sp), 1, n), dim3(POLAR_THREADS), 0, st, (const T* const*)d_src, d_dst, img0, M, N, sp, W, d_cxy,
                       n_centres, d_cos, d_sin);
  });
  return hipGetLastError();
}
// ---- a0: wavelet denoising (gpet_k_wavelet.inc; geometry: gpet_wavelet_plan.h) ----
template <typename T>
static void launch_wv_fwd1_t(hipStream_t st, const void* const* d_src, int img0, int n, char* ws, const WvPlan& p, double scale,
                             const WvFilters& flt) {
  const WvLevel& v = p.lv[0];
  const WvGrid g = wv_fwd_grid(v);
  hipLaunchKernelGGL((k_wv_fwd<T>), dim3(g.gx, g.gy, n), dim3(WV_TILE, WV_TILE), wv_fwd_lds_bytes(p.F), st, (const T* const*)d_src, img0,
                     (double*)ws, p.frame_doubles, (size_t)0, v.m, v.n, v.off, v.mo, v.no, p.F, scale, flt);
}
hipError_t launch_wavelet(hipStream_t st, int pix, const void* const* d_src, double* const* d_dst, int img0, int n, const WvPlan& p,
                          const WvSpec& sp, char* ws, double* d_sigma, double* d_thr, double* d_ms) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  if (!pix_bytes(pix) || n < 1 || n > WV_CHUNK_MAX || p.levels < 1 || p.levels > WV_LEVELS_MAX || p.F < 2 || p.F > WV_TAPS_MAX || p.F % 2 ||
      wv_fwd_lds_bytes(p.F) > WV_LDS_MAX || wv_inv_lds_bytes(p.F) > WV_LDS_MAX)
    return hipErrorInvalidValue;
  for (int l = 0; l < p.levels; ++l)
    if (wv_fwd_grid(p.lv[l]).gy > 65535 || wv_inv_grid(p.lv[l]).gy > 65535 || p.lv[l].m < p.F - 1 || p.lv[l].n < p.F - 1) return hipErrorInvalidValue;
  const WvFilters flt = wv_filters(sp.dec_lo, p.F);
  const bool integer = pix == PIX_U8 || pix == PIX_U16, given = !(sp.sigma != sp.sigma);
  for_pix(pix, [&](auto t) { launch_wv_fwd1_t<typename decltype(t)::type>(st, d_src, img0, n, ws, p, pix_unit(pix), flt); });
  for (int l = 1; l < p.levels; ++l) {
    const WvLevel& v = p.lv[l];
    const WvGrid g = wv_fwd_grid(v);
    hipLaunchKernelGGL((k_wv_fwd<double>), dim3(g.gx, g.gy, n), dim3(WV_TILE, WV_TILE), wv_fwd_lds_bytes(p.F), st, (const double* const*)nullptr,
                       img0, (double*)ws, p.frame_doubles, p.lv[l - 1].off, v.m, v.n, v.off, v.mo, v.no, p.F, 1.0, flt);
  }
  const int how = !given ? 0 : (integer && sp.rescale_sigma ? 1 : 2);
  const size_t band1 = (size_t)p.lv[0].mo * p.lv[0].no;
  hipLaunchKernelGGL(k_wv_sigma, dim3(n), dim3(WV_SIGMA_THREADS), 0, st, how, (const double*)ws, p.frame_doubles, p.lv[0].off + 3 * band1,
                     (int)band1, d_src, pix, (size_t)p.lv[0].m * p.lv[0].n, img0, given ? sp.sigma : 0.0, sp.ppf, d_sigma);
  if (!sp.thresholds)
    hipLaunchKernelGGL(k_wv_thresh, dim3(3, p.levels, n), dim3(WV_THRESH_THREADS), 0, st, (const double*)ws, p, img0, sp.method, sp.c,
                       (const double*)d_sigma, d_thr, d_ms);
  for (int l = p.levels - 1; l >= 0; --l) {
    const WvLevel& v = p.lv[l];
    const WvGrid g = wv_inv_grid(v);
    hipLaunchKernelGGL(k_wv_inv, dim3(g.gx, g.gy, n), dim3(WV_TILE, WV_TILE), wv_inv_lds_bytes(p.F), st, (double*)ws, p.frame_doubles, v.off, v.mo,
                       v.no, l > 0 ? p.lv[l - 1].off : (size_t)0, l > 0 ? (double* const*)nullptr : d_dst, img0, v.m, v.n, p.F,
                       (const double*)(d_thr + 3 * l), 3 * p.levels, sp.mode, l == 0 && integer ? 1 : 0, flt);
  }
  return hipGetLastError();
}
// ---- a0: split-Bregman TV denoising (gpet_k_tvb.inc; geometry: gpet_tvb_plan.h) ----
template <typename T>
static void launch_tvb_unpack_t(hipStream_t st, const void* const* d_src, int img0, int n, int M, int N, char* ws, double scale) {
  const size_t cells = tvb_cells(M, N);
  hipLaunchKernelGGL((k_tvb_unpack<T>), dim3((unsigned)((cells + TVB_THREADS - 1) / TVB_THREADS), 1, n), dim3(TVB_THREADS), 0, st,
                     (const T* const*)d_src, img0, (double*)ws, tvb_frame_bytes(M, N) / sizeof(double), M, N, scale);
}
hipError_t launch_tvb(hipStream_t st, int pix, const void* const* d_src, double* const* d_dst, int img0, int n, int M, int N,
                      const TvbSpec& sp, char* ws, TvbState* d_state) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  if (n < 1 || n > TVB_CHUNK_MAX || tvb_check(sp, pix, M, N, n) || tvb_lds_bytes(M, N) > TVB_LDS_MAX) return hipErrorInvalidValue;
  for_pix(pix, [&](auto t) { launch_tvb_unpack_t<typename decltype(t)::type>(st, d_src, img0, n, M, N, ws, pix_unit(pix)); });
  const size_t stride = tvb_frame_bytes(M, N) / sizeof(double);
  const double lam = 2.0 * sp.weight, norm = sp.weight + 4.0 * lam, inv_lam = 1.0 / lam;
  static_assert(TVB_CELLS_MAX == 2, "one instance of the sweep kernel per number of cells a lane can own");
  const auto sweeps = tvb_cells_per_lane(M, N) > 1 ? k_tvb_sweeps<2> : k_tvb_sweeps<1>;
  for (int k = 0; k < tvb_launches(sp.max_iter); ++k)
    hipLaunchKernelGGL(sweeps, dim3(1, 1, n), dim3(TVB_THREADS), tvb_lds_bytes(M, N), st, (double*)ws, stride, d_state, img0, M, N, lam, sp.weight,
                       norm, inv_lam, sp.eps, sp.max_iter, sp.isotropic);
  const size_t px = (size_t)M * N;
  hipLaunchKernelGGL(k_tvb_out, dim3((unsigned)((px + TVB_THREADS - 1) / TVB_THREADS), 1, n), dim3(TVB_THREADS), 0, st, (const double*)ws, stride,
                     d_dst, img0, M, N);
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
  for_pix(pix, [&](auto t) {
    using T = typename decltype(t)::type;
    (void)for_grid_z(n, [&](int i, int m) {
      launch_dn_gauss_t<T>(st, d_src, img0 + i, m, M, N, s, d_wy, d_wx, ws + (size_t)i * L.img_bytes, L);
      return hipSuccess;
    });
  });
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
  for_pix(pix, [&](auto t) {
    using T = typename decltype(t)::type;
    (void)for_grid_z(n, [&](int i, int m) {
      launch_dn_tvc_t<T>(st, d_src, img0 + i, m, M, N, it, tau_w, ws + (size_t)i * L.img_bytes, L);
      return hipSuccess;
    });
  });
  hipLaunchKernelGGL(k_dn_tvc_check, dim3(n), dim3(256), 0, st, ws, L.img_bytes, L.off_part, L.n_wg, img0, it, s.weight, s.eps,
                     (double)((size_t)M * N), d_n_iter, d_n_done);
  return hipGetLastError();
}

// f(std::integral_constant<int, KS>) for the K extent ks a plan chose (one of K_EXTENTS): the template instances of the sample GEMMs and of k_struct_rows
template <typename F>
static void for_k_extent(int ks, F&& f) {
  switch (ks) {
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 12: f(std::integral_constant<int, 12>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 18: f(std::integral_constant<int, 18>{}); break;
    case 20: f(std::integral_constant<int, 20>{}); break;
    default: f(std::integral_constant<int, 24>{}); break;
  }
}

static void fit_predict_attrs() {
  static PerDeviceOnce once;
  if (!once.first()) return;
  (void)hipFuncSetAttribute((const void*)k_fit<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_DYN_MAX);
  (void)hipFuncSetAttribute((const void*)k_fit<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_DYN_MAX);
  (void)hipFuncSetAttribute((const void*)k_predict<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_DYN_MAX);
  (void)hipFuncSetAttribute((const void*)k_predict<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_DYN_MAX);
}

// the fit with K in LDS where the plan has it there (false: more possible training points than K fits LDS for -- the caller's blocked form)
static bool launch_fit_in_lds(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, bool final_fit) {
  const FitPlan p = fit_plan(bd);
  if (!p.in_lds) return false;
  fit_predict_attrs();
  if (final_fit) hipLaunchKernelGGL((k_fit<true, true>), dim3(1, B), dim3(576), p.lds, st, d_edges);
  else hipLaunchKernelGGL((k_fit<true, false>), dim3(1, B), dim3(576), p.lds, st, d_edges);
  return true;
}

hipError_t launch_fit_predict(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, int want_cov, unsigned parts) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  fit_predict_attrs();
  if ((parts & 1u) && !launch_fit_in_lds(st, d_edges, B, bd, false)) launch_fit_blocked(st, d_edges, B, bd);
  const PredictPlan pp = predict_plan(bd, false);
  if (!(parts & 2u)) {
  } else if (pp.form == PredictForm::through_hbm) {
    // many training points: V through HBM, blocked substitution with the panel kernel of the structured path
    hipLaunchKernelGGL(k_kstar_build, dim3(cdiv(bd.Lg, 64), 64, B), dim3(256), 0, st, d_edges);
    hipLaunchKernelGGL(k_pred_colsum_big<false>, dim3(cdiv(bd.Lg, PB_COLS), B), dim3(PB_COLS * PB_LANES), 0, st, d_edges);
    for (int k0 = 0; k0 < bd.n_cap; k0 += CB)
      hipLaunchKernelGGL(k_vsolve_mfma, dim3(cdiv(bd.Lg, VS_COLS), B), dim3(256), 0, st, d_edges, k0);
    hipLaunchKernelGGL(k_pred_colsum_big<true>, dim3(cdiv(bd.Lg, PB_COLS), B), dim3(PB_COLS * PB_LANES), 0, st, d_edges);
  } else {
    hipLaunchKernelGGL((k_predict<true, false>), dim3(cdiv(bd.Lg, 64), B), dim3(64), pp.lds, st, d_edges, 0);
  }
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
  if (!launch_fit_in_lds(st, d_edges, B, bd, true))
    hipLaunchKernelGGL((k_fit<false, true>), dim3(1, B), dim3(256), (size_t)bd.n_cap * sizeof(double), st, d_edges);
  const PredictPlan pp = predict_plan(bd, true);
  if (pp.form == PredictForm::lds)
    hipLaunchKernelGGL((k_predict<true, true>), dim3(cdiv(bd.Lg, 64), B), dim3(64), pp.lds, st, d_edges, bd.Lg);
  else
    hipLaunchKernelGGL((k_predict<false, true>), dim3(cdiv(bd.Lg, 64), B), dim3(64), 0, st, d_edges, bd.Lg);
  return hipGetLastError();
}

// ---- eigen-factor stage of the LDS path: the plans of gpet_factor_plan.h decide, these name the template instances and launch ----
using JacobiKernel = void (*)(EdgeDev*, int, int);
static int jacobi_kernel_index(const JacobiSmallPlan& p) { return (p.ahead ? 4 : 0) + (p.nu == 3 ? 2 : 0) + (p.log ? 1 : 0); }
static JacobiKernel jacobi_kernel(int index) {
  switch (index) {
    case 0: return k_jacobi_seat<2, false>;
    case 1: return k_jacobi_seat<2, true>;
    case 2: return k_jacobi_seat<3, false>;
    case 3: return k_jacobi_seat<3, true>;
    case 4: return k_jacobi_ahead<2, false, JA_RR, JS_NT>;
    case 5: return k_jacobi_ahead<2, true, 0, JA_NT_LOG>;
    case 6: return k_jacobi_ahead<3, false, 0, JS_NT>;
    default: return k_jacobi_ahead<3, true, 0, JA_NT_LOG>;
  }
}
using PrerotKernel = void (*)(EdgeDev*, int);
static PrerotKernel prerot_kernel(int nt) {
  switch (nt) {
    case 2: return k_jacobi_prerot<2>;
    case 3: return k_jacobi_prerot<3>;
    case 4: return k_jacobi_prerot<4>;
    case 5: return k_jacobi_prerot<5>;
    default: return k_jacobi_prerot<6>;  // (no plan names it while its LDS does not fit: jacobi_small_plan)
  }
}

static void launch_jacobi_small(hipStream_t st, EdgeDev* d_edges, int B, int rank_max, int scaled_out, bool logw) {
  const JacobiSmallPlan p = jacobi_small_plan(B, rank_max, scaled_out != 0, logw, opt(Opt::jacobi_variant), opt(Opt::jacobi_warm));
  static PerDeviceOnce prerot_attr[7], jacobi_attr[8];
  if (p.prerot_nt) {
    const PrerotKernel k = prerot_kernel(p.prerot_nt);
    if (prerot_attr[p.prerot_nt].first()) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_DYN_MAX);
    hipLaunchKernelGGL(k, dim3(1, B), dim3(p.prerot_threads), p.prerot_lds, st, d_edges, p.warm);
  }
  const int ki = jacobi_kernel_index(p);
  const JacobiKernel k = jacobi_kernel(ki);
  if (jacobi_attr[ki].first()) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_DYN_MAX);
  hipLaunchKernelGGL(k, dim3(1, B), dim3(p.threads), p.lds, st, d_edges, scaled_out, p.warm);
  // (small batch: rotations logged, eigenvectors by a second kernel, one wave per row of W)
  if (p.log) hipLaunchKernelGGL(k_jacobi_wpass, dim3_of(p.wpass), dim3(256), 0, st, d_edges, scaled_out, p.warm);
}

hipError_t launch_factor(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, unsigned parts, const EdgeDev* h_edges,
                         bool single_wg_pchol) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  if (bd.r_cap > FACTOR_LDS_CAP) return launch_factor_big(st, d_edges, B, bd, h_edges);  // (any rank: csrc/gpet_eig.hip)
  const FactorLdsPlan p = factor_lds_plan(bd, B, opt(Opt::pchol_multi), single_wg_pchol);
  if (parts & 1u) switch (p.pchol.form) {
    case PcholForm::multi: {
      const hipError_t e = launch_pchol_multi(st, d_edges, B, p.pchol.multi);
      if (e != hipSuccess) return e;
    } break;
    case PcholForm::reg: hipLaunchKernelGGL(k_pchol_reg, dim3(1, B), dim3(p.pchol.threads), 0, st, d_edges); break;
    case PcholForm::one_wg: hipLaunchKernelGGL(k_pchol, dim3(1, B), dim3(p.pchol.threads), p.pchol.lds, st, d_edges); break;
  }
  if (parts & 2u) hipLaunchKernelGGL(k_gram, dim3_of(p.gram), dim3(256), 0, st, d_edges);
  if (parts & 4u) launch_jacobi_small(st, d_edges, B, bd.r_cap, 0, bd.jlog != 0 && opt(Opt::jacobi_logw) != 0);
  if (parts & 8u) hipLaunchKernelGGL(k_factor_rows, dim3_of(p.rows), dim3(256), p.rows_lds, st, d_edges);
  return hipGetLastError();
}

// structured loop path: fit -> (U, H, mean) -> Jacobi (the LDS kernel, on E.C) -> factor rows
hipError_t launch_struct_iteration(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, unsigned parts) {
  (void)hipGetLastError();
  static PerDeviceOnce once;
  if (once.first()) {
    (void)hipFuncSetAttribute((const void*)k_struct_H, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_DYN_MAX);
    (void)hipFuncSetAttribute((const void*)k_struct_rows<5, 20>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_DYN_MAX);
    (void)hipFuncSetAttribute((const void*)k_struct_rows<6, 24>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_DYN_MAX);
  }
  if ((parts & 1u) && !launch_fit_in_lds(st, d_edges, B, bd, false)) launch_fit_blocked(st, d_edges, B, bd);
  if ((parts & 2u) && !fit_plan(bd).in_lds) {
    // many training points (the blocked fit): U through HBM, blocked substitution
    hipLaunchKernelGGL(k_structB_build, dim3(64, B), dim3(256), 0, st, d_edges);
    hipLaunchKernelGGL(k_struct_beta, dim3(1, B), dim3(128), 0, st, d_edges);
    const int cgroups = cdiv(bd.r0_max, SB_COLS);
    for (int k0 = 0; k0 < bd.n_cap; k0 += CB)
      hipLaunchKernelGGL(k_struct_trsm, dim3(cgroups, B), dim3(256), 0, st, d_edges, k0, 0);
    const int t16 = cdiv(bd.r0_max, 16);
    hipLaunchKernelGGL(k_struct_Hbig, dim3(t16, t16, B), dim3(256), 0, st, d_edges);
    hipLaunchKernelGGL(k_struct_mean, dim3(cdiv(bd.Lg, 256), B), dim3(256), 0, st, d_edges);
  } else if (parts & 2u) {
    const StructHPlan hp = struct_h_plan(bd);
    hipLaunchKernelGGL(k_struct_H, dim3(1, B), dim3(1024), hp.lds, st, d_edges, hp.l_in_lds ? 1 : 0);
  }
  if (parts & 4u) launch_jacobi_small(st, d_edges, B, bd.r0_max > 0 ? bd.r0_max : bd.r_cap, 1, bd.jlog != 0 && opt(Opt::jacobi_logw) != 0);
  if (parts & 8u) {
    const StructRowsPlan rp = struct_rows_plan(bd, B);
    for_k_extent(rp.ks, [&](auto ks) {
      constexpr int KS = decltype(ks)::value;
      hipLaunchKernelGGL((k_struct_rows<k_extent(4 * KS).mt, KS>), dim3_of(rp.grid), dim3(256), rp.lds, st, d_edges);
    });
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

// opt-in counter-based normals (k_philox_normals, gpet_k_rng.inc; gpet_batch_set_rng)
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
    // (the register form where every kept curve fits one staging pass, else -- and as the cross-check, option kde_variant = 0 -- the staged form)
    const KdeFusedPlan kp = kde_fused_plan(bd, B);
    const KdeRegPlan rp = kde_reg_plan(bd, B, opt(Opt::kde_variant));
    if (parts & 1u) hipLaunchKernelGGL(k_kde_prep, dim3(1, B), dim3(1024), 0, st, d_edges);
    if ((parts & 2u) && rp.applies) hipLaunchKernelGGL(k_kde_fused_r, dim3_of(rp.grid), dim3(KDE_THREADS), rp.lds, st, d_edges, raw_band);
    else if (parts & 2u) hipLaunchKernelGGL(k_kde_fused, dim3_of(kp.grid), dim3(KDE_THREADS), kp.lds, st, d_edges, raw_band);
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
  const PixelPlan pp = pixel_plan(bd, B);
  if (parts & 1u) hipLaunchKernelGGL(k_pix_columns, dim3_of(pp.columns), dim3(256), 0, st, d_edges, raw_band);
  if (parts & 2u) hipLaunchKernelGGL(k_pix_old, dim3_of(pp.old), dim3(256), 0, st, d_edges, raw_band);
  if (parts & 4u) hipLaunchKernelGGL(k_pix_argbest, dim3_of(pp.argbest), dim3(256), 0, st, d_edges, raw_band);
  if (parts & 8u) hipLaunchKernelGGL(k_pix_select, dim3_of(pp.select), dim3(64), 0, st, d_edges);
  return hipGetLastError();
}

// The sample GEMM (sample_plan, gpet_iter_plan.h): f64 matrix cores, or the f32 ones (bd.y_arith, gpet_batch_set_sample_arith; with it
// off everything is enqueued as before).  The f64 register form has an instance per (K extent, f32 samples, mean in LDS), KS 20 and 24
// in the one-workgroup-per-CU kernel _rl; the f32 one an instance per K extent (every extent fits two workgroups per CU).
template <int KS, bool F32, bool MU_LDS>
static const void* sample_gemm_kernel() {
  if constexpr (KS >= 20) return (const void*)k_sample_gemm_mfma_rl<KS, F32, MU_LDS>;
  else return (const void*)k_sample_gemm_mfma_r<KS, F32, MU_LDS>;
}
hipError_t launch_sample(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, int rank_max) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  const bool f32mma = bd.y_arith != 0;
  const SamplePlan p = sample_plan(bd, B, rank_max, f32mma);
  if (!p.reg) {
    if (f32mma) hipLaunchKernelGGL(k_sample_f32, dim3_of(p.grid), dim3(p.block), 0, st, d_edges);
    else hipLaunchKernelGGL(k_sample_gemm_mfma, dim3_of(p.grid), dim3(p.block), 0, st, d_edges);
    return hipGetLastError();
  }
  // (the chunk plus the posterior mean of a wide edge exceed the 64 KB a kernel gets without asking: 66 KB at K = 96, Lg = 2048)
  static PerDeviceOnce once[2];
  if (once[f32mma].first())
    for (const int ks_ : K_EXTENTS)
      for_k_extent(ks_, [&](auto ks) {
        constexpr int KS = decltype(ks)::value;
        if (f32mma) {
          (void)hipFuncSetAttribute((const void*)k_sample_f32_r<KS>, hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_MAX);
        } else {
          (void)hipFuncSetAttribute(sample_gemm_kernel<KS, false, true>(), hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_MAX);
          (void)hipFuncSetAttribute(sample_gemm_kernel<KS, true, true>(), hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_MAX);
          (void)hipFuncSetAttribute(sample_gemm_kernel<KS, false, false>(), hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_MAX);
          (void)hipFuncSetAttribute(sample_gemm_kernel<KS, true, false>(), hipFuncAttributeMaxDynamicSharedMemorySize, GEMM_LDS_MAX);
        }
      });
  void* args[] = {(void*)&d_edges, (void*)&p.ncs};
  for_k_extent(p.ks, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    const void* k = f32mma                     ? (const void*)k_sample_f32_r<KS>
                    : p.y_f32 && p.mu_in_lds ? sample_gemm_kernel<KS, true, true>()
                    : p.y_f32                ? sample_gemm_kernel<KS, true, false>()
                    : p.mu_in_lds            ? sample_gemm_kernel<KS, false, true>()
                                             : sample_gemm_kernel<KS, false, false>();
    (void)hipLaunchKernel(k, dim3_of(p.grid), dim3(p.block), args, p.lds, st);
  });
  return hipGetLastError();
}

// the loop's scoring + curve KDE of a small batch with k_score_combine, k_topk_sort and k_kde_prep as ONE launch (k_score_tail);
// false: the shape does not allow it (the caller enqueues launch_score + launch_kde)
bool score_tail_applies(const BatchDims& bd) { return score_tail_applies(bd, opt(Opt::topk_rank)); }
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
  const ScorePlan p = score_plan(bd, B, S);
  if (p.tiled) {
    static PerDeviceOnce once;
    if (once.first()) {
      (void)hipFuncSetAttribute((const void*)k_score_tile<false>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_DYN_MAX);
      (void)hipFuncSetAttribute((const void*)k_score_tile<true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_DYN_MAX);
    }
    if (bd.y_f32) hipLaunchKernelGGL(k_score_tile<true>, dim3_of(p.tile_grid), dim3(SC_THREADS), p.lds, st, d_edges, p.cpw);
    else hipLaunchKernelGGL(k_score_tile<false>, dim3_of(p.tile_grid), dim3(SC_THREADS), p.lds, st, d_edges, p.cpw);
    if (!no_combine) hipLaunchKernelGGL(k_score_combine, dim3_of(p.combine_grid), dim3(256), 0, st, d_edges);
  } else {
    if (bd.y_f32) hipLaunchKernelGGL(k_score<true>, dim3_of(p.wave_grid), dim3(256), 0, st, d_edges);
    else hipLaunchKernelGGL(k_score<false>, dim3_of(p.wave_grid), dim3(256), 0, st, d_edges);
  }
  return hipGetLastError();
}

hipError_t launch_score(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, unsigned parts, bool no_combine) {
  (void)hipGetLastError();  // drop stale errors: report only these launches
  hipError_t e_rows = hipSuccess;
  if (parts & 1u) e_rows = launch_score_rows(st, d_edges, B, bd, bd.S, no_combine);
  if (parts & 2u) {
    if (topk_bitonic(bd, opt(Opt::topk_rank))) hipLaunchKernelGGL(k_topk_sort, dim3(1, B), dim3(512), 0, st, d_edges);
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
