// C ABI, a1 for stacks of raw frames: the one description of a raw-frame source (RawSource, gpet_api_internal.h) with its refusals,
// conv_frames -- every frame staged and denoised once, its gradient images made on the device --, the entry points on a context
// (gpet_grad_images*, gpet_denoise_images) and the four stages of their own in front of them (gpet_nlmeans_images,
// gpet_nlmeans_fast_images, gpet_wavelet_images, gpet_tvb_images), with the polar unwrap (gpet_polar_images) in front of those.
#include "gpet_api_internal.h"

static_assert(DN_NONE == GPET_DN_NONE && DN_MEDIAN == GPET_DN_MEDIAN && DN_MINIMUM == GPET_DN_MINIMUM && DN_GAUSSIAN == GPET_DN_GAUSSIAN &&
                  DN_TVC == GPET_DN_TVC && DN_MODE_REFLECT == GPET_DN_MODE_REFLECT && DN_MODE_NEAREST == GPET_DN_MODE_NEAREST,
              "gpet_denoise_plan.h numbers techniques and modes as include/gpet_hip.h does");

// (device memory of the context that only grows; the stream is idle when it is replaced)
static int ctx_grow(gpet_ctx* c, char** mem, size_t* cap, size_t bytes) {
  if (bytes <= *cap) return GPET_OK;
  HIPCHK(c, gpet_wait(c->stream));
  if (*mem) (void)hipFree(*mem);
  *mem = nullptr;
  *cap = 0;
  HIPCHK(c, hipMalloc((void**)mem, bytes));
  *cap = bytes;
  return GPET_OK;
}

// ---- refusals ------------------------------------------------------------------------------------------------------------------
int check_conv_multi(gpet_ctx* c, const RawSource& s) {
  if (!s.kern || !s.kh || !s.kw) return fail(c, GPET_ERR_BAD_ARG, "slot table: the kernels are a null pointer");
  if (const char* why = slot_table_check(s.n_frames, s.n_kern, s.n_img, s.frame_of, s.kernel_of))
    return fail(c, GPET_ERR_BAD_ARG, "slot table: %s (n_frames = %d, n_kern = %d, n_img = %d)", why, s.n_frames, s.n_kern, s.n_img);
  for (int k = 0; k < s.n_kern; ++k)
    if (!s.kern[k] || s.kh[k] <= 0 || s.kw[k] <= 0) return fail(c, GPET_ERR_BAD_ARG, "slot table: kernel %d is empty or a null pointer", k);
  if (!(s.tr ? conv_union_t_fits_lds(s.n_kern, s.kh, s.kw) : conv_union_fits_lds(s.n_kern, s.kh, s.kw))) {
    const ConvUnion u = conv_union(s.n_kern, s.kh, s.kw);
    return fail(c, GPET_ERR_BAD_ARG, "the %d kernels need %zu bytes of LDS for their taps and their union patch of %d x %d, more than %zu",
                s.n_kern, s.tr ? conv_union_t_lds_bytes(u) : conv_union_lds_bytes(u), s.tr ? conv_union_t_rows(u) : conv_union_rows(u),
                s.tr ? conv_union_t_cols(u) : conv_union_cols(u), CONV_LDS_MAX);
  }
  return GPET_OK;
}

// (a table answers for its own frame and kernel counts: "raw frames: bad argument" is the single-kernel form's)
int check_raw_source(gpet_ctx* c, const RawSource& s) {
  const bool dn_on = s.dn && s.dn->technique != DN_NONE;
  if (!s.frames || (!s.table && (s.n_frames <= 0 || (s.n_kern ? !s.kern[0] || s.kh[0] <= 0 || s.kw[0] <= 0 : !dn_on))))
    return fail(c, GPET_ERR_BAD_ARG, "raw frames: bad argument");
  if (!pix_bytes(s.pix)) return fail(c, GPET_ERR_BAD_ARG, "unknown pixel type %d (GPET_PIX_U8 = 0 .. GPET_PIX_F64 = 3)", s.pix);
  if (s.table) {
    const int rc = check_conv_multi(c, s);
    if (rc) return rc;
  } else if (s.n_kern && !(s.tr ? conv_t_fits_lds(s.kh[0], s.kw[0]) : conv_fits_lds(s.kh[0], s.kw[0])))
    return fail(c, GPET_ERR_BAD_ARG, "a %d x %d kernel needs %zu bytes of LDS for its patch, more than %zu", s.kh[0], s.kw[0],
                s.tr ? conv_t_lds_bytes(s.kh[0], s.kw[0]) : conv_lds_bytes(s.kh[0], s.kw[0]), CONV_LDS_MAX);
  if (s.dn)
    if (const char* why = dn_check(*s.dn, s.pix)) return fail(c, GPET_ERR_BAD_ARG, "denoise: %s", why);
  for (int g = 0; g < s.n_frames; ++g)
    if (!s.frames[g]) return fail(c, GPET_ERR_BAD_ARG, "raw frame %d is a null pointer", g);
  return GPET_OK;
}

// ---- conv_frames ---------------------------------------------------------------------------------------------------------------
// The frames of s -> normalised f32 gradient images dst[g] (device), everything enqueued on the context's stream: the taps and the
// pointer tables go up in one copy, host frames follow in the chunks of stage_plan (gpet_conv_plan.h) with ONE convolution launch
// per chunk, device frames are read where they lie by one launch; one launch normalises all images.  Host frames are copied
// straight out of the caller's (pageable) memory: packing each chunk into a ring of pinned slots first, so that the host packs
// chunk k + 1 while the device works on chunk k, was built and measured -- 256 frames of 500 x 500: u8 8.8 against 8.8 ms, f32 16.5
// against 14.5, f64 20.7 against 18.6 -- and removed.  Nothing is waited for at the end: the caller waits before host frames (and
// the context's tables) may change.
// With a denoising spec (s.dn, technique not NONE: gpet_denoise_plan.h) every chunk is denoised where it was staged before it is
// convolved: the chunk's workspace follows its frames in the staging slot, the convolution reads the denoised frames in the pixel
// type the technique leaves behind, and frames on the device go through chunks of the same budget too.  'tvc' iterates a chunk to
// its end -- groups of DN_TVC_GROUP iterations, the count of finished images read between groups -- before the next is staged.
// A slot table (gpet_conv_multi_plan.h): the frames are staged and denoised once each, in the same chunks, while dst[] and d_mm
// are per slot: one k_conv_relu_multi launch per chunk writes every slot of the chunk's frames, and the kernels' taps, descriptors
// and the slot lists go up in the same one table copy.  A table that is one kernel on every frame in frame order is the
// single-kernel form itself and takes its launches, in the same order.
int conv_frames(gpet_ctx* c, const RawSource& s, float* const* dst, unsigned int* d_mm, void* const* dn_out, int32_t* n_iter_out) {
  const int rc0 = check_raw_source(c, s);
  if (rc0) return rc0;
  if (s.M <= 0 || s.N <= 0 || (s.n_kern && !dst)) return fail(c, GPET_ERR_BAD_ARG, "raw frames: bad argument");
  const DenoiseSpec* const dn = s.dn;
  const bool conv = s.n_kern > 0, dn_on = dn && dn->technique != DN_NONE, on_dev = s.on_dev, tr = s.tr;
  const bool multi = s.table && !slot_table_is_identity(s.n_frames, s.n_kern, s.n_img, s.frame_of, s.kernel_of);
  const int n_fr = s.n_frames, n_out = s.n_img, pix = s.pix, M = s.M, N = s.N;  // frames staged; images written, one per slot
  const int kh = conv ? s.kh[0] : 0, kw = conv ? s.kw[0] : 0;                   // (the single-kernel form's)
  const size_t esz = (size_t)pix_bytes(pix);
  const ConvUnion cu = multi ? conv_union(s.n_kern, s.kh, s.kw) : ConvUnion{0, 0, 0, 0, 0};
  const size_t px = (size_t)M * N, img_bytes = px * esz, nt = multi ? cu.taps : (size_t)kh * kw;
  const DenoiseLayout L = dn_layout(dn_on ? dn->technique : DN_NONE, pix, M, N);
  const int cpix = dn_on ? dn_out_pix(dn->technique, pix) : pix;  // what the convolution reads
  const size_t stage_img = dn_stage_bytes(img_bytes, on_dev, L);
  const StagePlan sp = (on_dev && !dn_on) ? StagePlan{0, 0, 0, 0} : dn_stage_plan(n_fr, img_bytes, on_dev, L);
  const size_t o_ws = (size_t)sp.per_chunk * stage_img;  // a chunk's workspace, behind its frames
  int rc = ctx_grow(c, &c->raw_dev, &c->raw_dev_bytes, (size_t)sp.slots * sp.slot_bytes);
  if (rc) return rc;
  // one block, the same on both sides: source pointers | destination pointers | taps | reset values of the (min, max) slots
  // | pointers to the denoised frames | Gaussian taps of the two axes | iterations per image | finished images of the chunk
  const int ry = dn_on && dn->technique == DN_GAUSSIAN ? dn_gauss_radius(dn->sigma_y, dn->truncate) : 0;
  const int rx = dn_on && dn->technique == DN_GAUSSIAN ? dn_gauss_radius(dn->sigma_x, dn->truncate) : 0;
  // | with a slot table: kernel descriptors | slots of each frame (offsets, list) | kernel of each slot
  const size_t o_dst = sizeof(void*) * (size_t)n_fr, o_wf = o_dst + sizeof(void*) * (size_t)n_out, o_mm = o_wf + sizeof(double) * nt;
  const size_t o_dn = (o_mm + sizeof(unsigned int) * 2 * (size_t)n_out + 7) & ~(size_t)7;
  const size_t o_gw = o_dn + (dn_on ? o_dst : 0), o_it = o_gw + (dn_on ? sizeof(double) * (size_t)(2 * ry + 1 + 2 * rx + 1) : 0);
  const size_t o_end = dn_on ? o_it + sizeof(int) * ((size_t)n_fr + 1) : o_mm + sizeof(unsigned int) * 2 * (size_t)n_out;
  const size_t o_kd = (o_end + 7) & ~(size_t)7, o_so = o_kd + (multi ? sizeof(ConvKernDesc) * (size_t)s.n_kern : 0);
  const size_t o_sl = o_so + (multi ? sizeof(int32_t) * ((size_t)n_fr + 1) : 0), o_ko = o_sl + (multi ? sizeof(int32_t) * (size_t)n_out : 0);
  const size_t tab_bytes = multi ? o_ko + sizeof(int32_t) * (size_t)n_out : o_end;
  rc = ctx_grow(c, &c->raw_tab, &c->raw_tab_bytes, tab_bytes);
  if (rc) return rc;
  c->h_raw_tab.resize(tab_bytes);
  char* h = c->h_raw_tab.data();
  const void** h_src = (const void**)h;
  float** h_dst = (float**)(h + o_dst);
  unsigned int* h_mm = (unsigned int*)(h + o_mm);
  for (int k = 0; k < sp.n_chunks; ++k)
    for (int i = 0; i < stage_count(sp, k, n_fr); ++i) {
      char* slot = c->raw_dev + (size_t)stage_slot(sp, k) * sp.slot_bytes;
      if (!on_dev) h_src[stage_first(sp, k) + i] = slot + (size_t)i * stage_img;
      if (dn_on) ((const void**)(h + o_dn))[stage_first(sp, k) + i] = slot + o_ws + (size_t)i * L.img_bytes + L.off_out;
    }
  for (int g = 0; g < n_fr; ++g)
    if (on_dev) h_src[g] = s.frames[g];
  for (int g = 0; g < n_out; ++g) {
    h_dst[g] = dst ? dst[g] : nullptr;
    h_mm[2 * g] = 0xFFFFFFFFu;
    h_mm[2 * g + 1] = 0u;
  }
  if (multi) {
    ConvKernDesc* kd = (ConvKernDesc*)(h + o_kd);
    conv_kern_descs(s.n_kern, s.kh, s.kw, kd);
    for (int k = 0; k < s.n_kern; ++k) conv_flip_taps(s.kern[k], s.kh[k], s.kw[k], (double*)(h + o_wf) + kd[k].w0);
    frame_slots(n_fr, n_out, s.frame_of, (int32_t*)(h + o_so), (int32_t*)(h + o_sl));
    memcpy(h + o_ko, s.kernel_of, sizeof(int32_t) * (size_t)n_out);
  } else if (conv)
    conv_flip_taps(s.kern[0], kh, kw, (double*)(h + o_wf));
  if (dn_on && dn->technique == DN_GAUSSIAN) {
    dn_gauss_taps(dn->sigma_y, ry, (double*)(h + o_gw));
    dn_gauss_taps(dn->sigma_x, rx, (double*)(h + o_gw) + 2 * ry + 1);
  }
  HIPCHK(c, hipMemcpyAsync(c->raw_tab, h, tab_bytes, hipMemcpyHostToDevice, c->stream));
  if (conv)
    HIPCHK(c, hipMemcpyAsync(d_mm, c->raw_tab + o_mm, sizeof(unsigned int) * 2 * (size_t)n_out, hipMemcpyDeviceToDevice, c->stream));
  const void* const* d_src = (const void* const*)c->raw_tab;
  float* const* d_dst = (float* const*)(c->raw_tab + o_dst);
  const double* d_wf = (const double*)(c->raw_tab + o_wf);
  const void* const* d_conv_src = dn_on ? (const void* const*)(c->raw_tab + o_dn) : d_src;
  const double* d_gw = (const double*)(c->raw_tab + o_gw);
  int* d_it = (int*)(c->raw_tab + o_it);
  // frames first .. first + cnt - 1 of `from` (pixel type p) -> the gradient images of the frames, or of all their slots
  // (tr: the transposed-store forms -- the image at dst[g] is then N x M; the element-wise normaliser below does not care)
  auto convolve = [&](int p, const void* const* from, int first, int cnt) {
    if (multi)
      return launch_conv_multi(c->stream, p, tr, from, first, cnt, M, N, d_wf, cu, (const ConvKernDesc*)(c->raw_tab + o_kd),
                               (const int32_t*)(c->raw_tab + o_so), (const int32_t*)(c->raw_tab + o_sl),
                               (const int32_t*)(c->raw_tab + o_ko), d_dst, d_mm);
    return launch_conv_batch(c->stream, p, tr, from, first, cnt, M, N, d_wf, kh, kw, d_dst, d_mm);
  };
  if (on_dev && !dn_on) {
    HIPCHK(c, convolve(pix, d_src, 0, n_fr));
  } else {
    // plain copies out of the caller's memory, image by image, in stream order behind the kernels that last read the slot
    for (int k = 0; k < sp.n_chunks; ++k) {
      const int first = stage_first(sp, k), cnt = stage_count(sp, k, n_fr);
      char* d_slot = c->raw_dev + (size_t)stage_slot(sp, k) * sp.slot_bytes;
      if (!on_dev)
        for (int i = 0; i < cnt; ++i)
          HIPCHK(c, hipMemcpyAsync(d_slot + (size_t)i * stage_img, s.frames[first + i], img_bytes, hipMemcpyHostToDevice, c->stream));
      if (dn_on) {
        char* ws = d_slot + o_ws;
        if (dn->technique == DN_GAUSSIAN) {
          HIPCHK(c, launch_dn_gauss(c->stream, pix, d_src, first, cnt, M, N, *dn, d_gw, d_gw + 2 * ry + 1, ws, L));
        } else if (dn->technique == DN_TVC) {
          int* d_done = d_it + n_fr;
          HIPCHK(c, hipMemsetAsync(d_done, 0, sizeof(int), c->stream));
          for (int issued = 0, done = 0; issued < dn->n_iter_max && done < cnt;) {
            const int grp = dn->n_iter_max - issued < DN_TVC_GROUP ? dn->n_iter_max - issued : DN_TVC_GROUP;
            for (int j = 0; j < grp; ++j)
              HIPCHK(c, launch_dn_tvc_iter(c->stream, pix, d_src, first, cnt, M, N, *dn, issued + j, ws, L, d_it, d_done));
            issued += grp;
            if (issued < dn->n_iter_max) {
              HIPCHK(c, hipMemcpyAsync(&done, d_done, sizeof(int), hipMemcpyDeviceToHost, c->stream));
              HIPCHK(c, gpet_wait(c->stream));
            }
          }
        } else {
          HIPCHK(c, launch_dn_rank(c->stream, pix, d_src, first, cnt, M, N, *dn, ws, L));
        }
        if (dn_out)
          for (int i = 0; i < cnt; ++i)
            HIPCHK(c, hipMemcpyAsync(dn_out[first + i], ws + (size_t)i * L.img_bytes + L.off_out, px * (size_t)pix_bytes(cpix),
                                     hipMemcpyDeviceToHost, c->stream));
      }
      if (conv) HIPCHK(c, convolve(cpix, d_conv_src, first, cnt));
    }
  }
  if (n_iter_out) {
    if (dn_on && dn->technique == DN_TVC)
      HIPCHK(c, hipMemcpyAsync(n_iter_out, d_it, sizeof(int32_t) * (size_t)n_fr, hipMemcpyDeviceToHost, c->stream));
    else
      for (int g = 0; g < n_fr; ++g) n_iter_out[g] = 0;
  }
  if (conv) HIPCHK(c, launch_normalise_batch(c->stream, d_dst, n_out, px, d_mm));
  return GPET_OK;
}

// ---- the entry points on a context ---------------------------------------------------------------------------------------------
// the s.n_img gradient images of s into the host buffers out[g]
// (GPET_FRAMES_TRANSPOSED: every output is the N x M transpose of the frame's M x N gradient image)
static int grad_images_from(gpet_ctx* c, const RawSource& s, float* const* out) {
  const int n_img = s.n_img;
  if (!c || !s.frames || !out || n_img <= 0 || s.M <= 0 || s.N <= 0 || (!s.table && (!s.kern[0] || s.kh[0] <= 0 || s.kw[0] <= 0)))
    return fail(c, GPET_ERR_BAD_ARG, "gpet_grad_images: bad argument");
  if (s.table) {
    const int rc_t = check_conv_multi(c, s);  // (before the scratch is sized by the table, and so before the pixel type is looked at)
    if (rc_t) return rc_t;
  }
  for (int g = 0; g < n_img; ++g)
    if (!out[g]) return fail(c, GPET_ERR_BAD_ARG, "gpet_grad_images: output image %d is a null pointer", g);
  HIPCHK(c, hipSetDevice(c->device));
  const size_t px = (size_t)s.M * s.N;
  Carver meas;
  (void)meas.take<float>(px * (size_t)n_img);
  (void)meas.take<unsigned int>(2 * (size_t)n_img);
  int rc = ctx_scratch(c, meas.off + 256);
  if (rc) return rc;
  Carver cv;
  cv.base = c->scratch;
  float* d_out = cv.take<float>(px * (size_t)n_img);
  unsigned int* d_mm = cv.take<unsigned int>(2 * (size_t)n_img);
  std::vector<float*> dst((size_t)n_img);
  for (int g = 0; g < n_img; ++g) dst[(size_t)g] = d_out + (size_t)g * px;
  rc = conv_frames(c, s, dst.data(), d_mm);
  if (rc == GPET_OK)
    for (int g = 0; g < n_img; ++g) {
      hipError_t e = hipMemcpyAsync(out[g], dst[(size_t)g], px * sizeof(float), hipMemcpyDeviceToHost, c->stream);
      if (e != hipSuccess) {
        (void)gpet_wait(c->stream);
        return fail(c, GPET_ERR_HIP, "gpet_grad_images: copy of image %d failed: %s", g, hipGetErrorString(e));
      }
    }
  HIPCHK(c, gpet_wait(c->stream));  // (also after an error: host frames already enqueued must not be read after the return)
  return rc;
}

extern "C" {

int gpet_grad_images(gpet_ctx* c, const void* const* raw, int n_img, int pix, int M, int N, const double* kern, int kh, int kw,
                     unsigned int flags, float* const* out) {
  return gpet_grad_images_dn(c, raw, n_img, pix, M, N, kern, kh, kw, nullptr, flags, out);
}

int gpet_grad_images_dn(gpet_ctx* c, const void* const* raw, int n_img, int pix, int M, int N, const double* kern, int kh, int kw,
                        const gpet_denoise* dn, unsigned int flags, float* const* out) {
  RawSourceArgs a;
  a.frames(raw, n_img, pix, dn, flags, M, N);
  a.one_kernel(kern, kh, kw);
  return grad_images_from(c, a.raw, out);
}

int gpet_grad_images_multi(gpet_ctx* c, const void* const* raw, int n_frames, int pix, int M, int N, int n_kern, const double* const* kern,
                           const int32_t* kh, const int32_t* kw, const gpet_denoise* dn, int n_img, const int32_t* frame_of,
                           const int32_t* kernel_of, unsigned int flags, float* const* out) {
  RawSourceArgs a;
  a.frames(raw, n_frames, pix, dn, flags, M, N);
  a.slot_table(n_kern, kern, kh, kw, n_img, frame_of, kernel_of);
  return grad_images_from(c, a.raw, out);
}

int gpet_denoise_images(gpet_ctx* c, const void* const* raw, int n_img, int pix, int M, int N, const gpet_denoise* dn,
                        unsigned int flags, void* const* out, int32_t* n_iter_out) {
  if (!c || !raw || !dn || !out || n_img <= 0 || M <= 0 || N <= 0) return fail(c, GPET_ERR_BAD_ARG, "gpet_denoise_images: bad argument");
  if (dn->technique == GPET_DN_NONE) return fail(c, GPET_ERR_BAD_ARG, "gpet_denoise_images: no technique");
  for (int g = 0; g < n_img; ++g)
    if (!out[g]) return fail(c, GPET_ERR_BAD_ARG, "gpet_denoise_images: output image %d is a null pointer", g);
  HIPCHK(c, hipSetDevice(c->device));
  RawSourceArgs a;  // (no kernel: one denoised frame per frame; the transposed bit means nothing without a convolution)
  a.frames(raw, n_img, pix, dn, flags & ~GPET_FRAMES_TRANSPOSED, M, N);
  a.raw.n_img = n_img;
  const int rc = conv_frames(c, a.raw, nullptr, nullptr, out, n_iter_out);
  HIPCHK(c, gpet_wait(c->stream));  // (also after an error: host frames already enqueued must not be read after the return)
  return rc;
}

}  // extern "C"

// ---- the stages of their own in front of the raw-frame path --------------------------------------------------------------------
// What differs between the stages, as pre_stage takes it.  A stage's device block, the same on both sides: source pointers |
// destination pointers | the stage's extras.
struct PreStage {
  unsigned int out_dev_bit = 0;     // the stage's GPET_*_OUT_ON_DEVICE
  size_t extras_bytes = 0;          // zero on the way up, but for init_bytes at init_off copied from init (nullptr: none)
  const void* init = nullptr;
  size_t init_off = 0, init_bytes = 0;
  size_t ws_bytes = 0;              // what a frame keeps in the context's workspace (pre_ws)
  size_t out_px = 0;                // pixels of a result where it is not the frame's M N (the polar unwrap); 0: M N
  bool read_back = false;           // the extras come back at the end, in one copy the call waits for ...
  const char* h_extras = nullptr;   // ... into the host copy, which pre_stage leaves here
};
// a chunk as a stage's launch sees it: frames first .. first + cnt - 1 of the two pointer tables, the chunk's workspace
struct PreChunk {
  const void* const* d_src;
  double* const* d_dst;
  char* d_extras;
  char* ws;
  int first, cnt;
};
static const auto no_chunk_hook = [](const PreChunk&) { return hipSuccess; };

// Frames raw[] -> f64 results out[] through one stage, everything enqueued on the context's stream.  Host frames and host outputs
// go through the staging slot in the chunks of `chunks(staged bytes per frame)` -- a chunk's frames at i * st_in, then its results
// at per_chunk * st_in + i * st_out --, frames and outputs on the device are read and written where they lie; per chunk: the
// frames' copies, `launch`, the results' copies, `after_chunk`.  The call waits exactly when host memory of the caller is in flight
// or the extras are read back, and after any enqueue error (frames already enqueued must not be read after the return), which is
// reported in preference to the wait's own.
template <typename Chunks, typename Launch, typename Hook>
static int pre_stage(gpet_ctx* c, const void* const* raw, void* const* out, int n_img, int pix, int M, int N, unsigned int flags,
                     PreStage& st, Chunks&& chunks, Launch&& launch, Hook&& after_chunk) {
  HIPCHK(c, hipSetDevice(c->device));
  const bool in_dev = (flags & GPET_RAW_ON_DEVICE) != 0, out_dev = (flags & st.out_dev_bit) != 0;
  const size_t px = (size_t)M * N, img_bytes = px * (size_t)pix_bytes(pix), out_bytes = (st.out_px ? st.out_px : px) * sizeof(double);
  const size_t st_in = in_dev ? 0 : dn_align(img_bytes), st_out = out_dev ? 0 : dn_align(out_bytes);
  const StagePlan plan = chunks(st_in + st_out);
  int rc = ctx_grow(c, &c->raw_dev, &c->raw_dev_bytes, (size_t)plan.per_chunk * (st_in + st_out));
  if (rc) return rc;
  rc = ctx_grow(c, &c->pre_ws, &c->pre_ws_bytes, (size_t)plan.per_chunk * st.ws_bytes);
  if (rc) return rc;
  const size_t o_dst = sizeof(void*) * (size_t)n_img, o_ex = 2 * o_dst, tab_bytes = o_ex + st.extras_bytes;
  rc = ctx_grow(c, &c->raw_tab, &c->raw_tab_bytes, tab_bytes);
  if (rc) return rc;
  c->h_raw_tab.assign(tab_bytes, 0);
  char* h = c->h_raw_tab.data();
  const void** h_src = (const void**)h;
  void** h_dst = (void**)(h + o_dst);
  for (int k = 0; k < plan.n_chunks; ++k)
    for (int i = 0; i < stage_count(plan, k, n_img); ++i) {
      const int g = stage_first(plan, k) + i;
      h_src[g] = in_dev ? raw[g] : c->raw_dev + (size_t)i * st_in;
      h_dst[g] = out_dev ? out[g] : c->raw_dev + (size_t)plan.per_chunk * st_in + (size_t)i * st_out;
    }
  if (st.init) memcpy(h + o_ex + st.init_off, st.init, st.init_bytes);
  HIPCHK(c, hipMemcpyAsync(c->raw_tab, h, tab_bytes, hipMemcpyHostToDevice, c->stream));
  hipError_t e = hipSuccess;
  for (int k = 0; k < plan.n_chunks && e == hipSuccess; ++k) {
    const int first = stage_first(plan, k), cnt = stage_count(plan, k, n_img);
    const PreChunk ch{(const void* const*)c->raw_tab, (double* const*)(c->raw_tab + o_dst), c->raw_tab + o_ex, c->pre_ws, first, cnt};
    for (int i = 0; i < cnt && !in_dev && e == hipSuccess; ++i)
      e = hipMemcpyAsync((void*)h_src[first + i], raw[first + i], img_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch(ch);
    for (int i = 0; i < cnt && !out_dev && e == hipSuccess; ++i)
      e = hipMemcpyAsync(out[first + i], h_dst[first + i], out_bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = after_chunk(ch);
  }
  if (e == hipSuccess && st.read_back) e = hipMemcpyAsync(h + o_ex, c->raw_tab + o_ex, st.extras_bytes, hipMemcpyDeviceToHost, c->stream);
  if (!in_dev || !out_dev || st.read_back || e != hipSuccess) {
    const hipError_t ew = gpet_wait(c->stream);
    HIPCHK(c, e);
    HIPCHK(c, ew);
  }
  st.h_extras = h + o_ex;
  return GPET_OK;
}

extern "C" {

// Non-local means (gpet_nlmeans_plan.h).  Extras: the taps.  One launch per chunk of the staging slot; frames and outputs both on
// the device take one launch and no wait.
int gpet_nlmeans_images(gpet_ctx* c, const void* const* raw, int n_img, int pix, int M, int N, const gpet_nlmeans* spec,
                        unsigned int flags, void* const* out) {
  if (!c || !raw || !spec || !out || n_img <= 0 || M <= 0 || N <= 0) return fail(c, GPET_ERR_BAD_ARG, "gpet_nlmeans_images: bad argument");
  NlmSpec sp;
  sp.patch_size = spec->patch_size;
  sp.patch_distance = spec->patch_distance;
  sp.h = spec->h;
  sp.sigma = spec->sigma;
  sp.taps = spec->taps;
  const int s = nlm_patch(sp.patch_size), d = sp.patch_distance;
  if (const char* why = nlm_check(sp, pix, M, N)) {
    if (s >= 3 && s <= NLM_PATCH_MAX && d >= 0 && d <= NLM_DIST_MAX && nlm_lds_bytes(s, d) > NLM_LDS_MAX)
      return fail(c, GPET_ERR_BAD_ARG, "nlmeans: %s: patch %d, distance %d need %zu bytes, more than %zu", why, s, d, nlm_lds_bytes(s, d),
                  NLM_LDS_MAX);
    return fail(c, GPET_ERR_BAD_ARG, "nlmeans: %s (patch_size %d, patch_distance %d, h %g, sigma %g, frames %d x %d)", why, sp.patch_size, d,
                sp.h, sp.sigma, M, N);
  }
  for (int g = 0; g < n_img; ++g)
    if (!raw[g] || !out[g]) return fail(c, GPET_ERR_BAD_ARG, "gpet_nlmeans_images: frame or output %d is a null pointer", g);
  PreStage st;
  st.out_dev_bit = GPET_NLM_OUT_ON_DEVICE;
  st.init = sp.taps;
  st.extras_bytes = st.init_bytes = sizeof(double) * (size_t)(s * s);
  const double var2 = 2.0 * sp.sigma * sp.sigma;
  return pre_stage(
      c, raw, out, n_img, pix, M, N, flags, st,
      [&](size_t staged) { return staged ? stage_plan(n_img, staged) : StagePlan{n_img, 1, 0, 0}; },
      [&](const PreChunk& k) {
        return launch_nlmeans(c->stream, pix, k.d_src, k.d_dst, k.first, k.cnt, M, N, s, d, (const double*)k.d_extras, var2);
      },
      no_chunk_hook);
}

// Fast-mode non-local means (gpet_nlfast_plan.h).  No extras.  Frames go chunk by chunk (nlf_chunks), the padded frame, the
// accumulators and the integral images of a group of shifts through the context's workspace; per chunk one padding launch and
// per group one integral and one gather launch, enqueued without waiting.
int gpet_nlmeans_fast_images(gpet_ctx* c, const void* const* raw, int n_img, int pix, int M, int N, const gpet_nlmeans_fast* spec,
                             unsigned int flags, void* const* out) {
  if (!c || !raw || !spec || !out || n_img <= 0 || M <= 0 || N <= 0)
    return fail(c, GPET_ERR_BAD_ARG, "gpet_nlmeans_fast_images: bad argument");
  NlfSpec sp;
  sp.patch_size = spec->patch_size;
  sp.patch_distance = spec->patch_distance;
  sp.h = spec->h;
  sp.sigma = spec->sigma;
  if (const char* why = nlf_check(sp, pix, M, N))
    return fail(c, GPET_ERR_BAD_ARG, "nlmeans_fast: %s (patch_size %d, patch_distance %d, h %g, sigma %g, frames %d x %d)", why, sp.patch_size,
                sp.patch_distance, sp.h, sp.sigma, M, N);
  const NlfPlan np = nlf_plan(M, N, nlm_patch(sp.patch_size), sp.patch_distance);
  if (np.rows_per_group < 1)
    return fail(c, GPET_ERR_BAD_ARG,
                "nlmeans_fast: the workspace of a %d x %d frame with the integral images of one row of %d shifts needs %zu bytes, more than %zu",
                M, N, nlf_row_shifts(np.d), np.frame_bytes, NLF_CHUNK_BUDGET);
  for (int g = 0; g < n_img; ++g)
    if (!raw[g] || !out[g]) return fail(c, GPET_ERR_BAD_ARG, "gpet_nlmeans_fast_images: frame or output %d is a null pointer", g);
  PreStage st;
  st.out_dev_bit = GPET_NLM_OUT_ON_DEVICE;
  st.ws_bytes = np.frame_bytes;
  return pre_stage(
      c, raw, out, n_img, pix, M, N, flags, st, [&](size_t staged) { return nlf_chunks(n_img, staged, np); },
      [&](const PreChunk& k) { return launch_nlfast(c->stream, pix, k.d_src, k.d_dst, k.first, k.cnt, M, N, sp, np, k.ws); }, no_chunk_hook);
}

// Polar unwrap (gpet_polar_plan.h).  Extras: cx [n_centres] | cy [n_centres] | cos_t [n_theta] | sin_t [n_theta].  The one stage
// whose results have another shape than its frames: out[g] is n_r x W.  One launch per chunk of the staging slot, no workspace;
// frames and outputs both on the device take one launch per 65535 frames and no wait.
int gpet_polar_images(gpet_ctx* c, const void* const* raw, int n_img, int pix, int M, int N, const gpet_polar* spec, unsigned int flags,
                      void* const* out) {
  if (!c || !raw || !spec || !out || n_img <= 0) return fail(c, GPET_ERR_BAD_ARG, "gpet_polar_images: bad argument");
  PolarSpec sp;
  sp.r0 = spec->r0;
  sp.dr = spec->dr;
  sp.n_r = spec->n_r;
  sp.n_theta = spec->n_theta;
  sp.pad = spec->pad;
  const int nc = spec->n_centres;
  if (const char* why = polar_check(sp, pix, M, N, nc, n_img, spec->cx, spec->cy))
    return fail(c, GPET_ERR_BAD_ARG, "%s (n_r %d, n_theta %d, pad %d, r0 %g, dr %g, %d centres, %d frames of %d x %d)", why, sp.n_r, sp.n_theta,
                sp.pad, sp.r0, sp.dr, nc, n_img, M, N);
  if (!spec->cos_t || !spec->sin_t) return fail(c, GPET_ERR_BAD_ARG, "polar: the trig tables are a null pointer");
  for (int g = 0; g < n_img; ++g)
    if (!raw[g] || !out[g]) return fail(c, GPET_ERR_BAD_ARG, "gpet_polar_images: frame or output %d is a null pointer", g);
  std::vector<double> ex((size_t)2 * nc + (size_t)2 * sp.n_theta);
  memcpy(ex.data(), spec->cx, sizeof(double) * (size_t)nc);
  memcpy(ex.data() + nc, spec->cy, sizeof(double) * (size_t)nc);
  memcpy(ex.data() + 2 * (size_t)nc, spec->cos_t, sizeof(double) * (size_t)sp.n_theta);
  memcpy(ex.data() + 2 * (size_t)nc + sp.n_theta, spec->sin_t, sizeof(double) * (size_t)sp.n_theta);
  PreStage st;
  st.out_dev_bit = GPET_POLAR_OUT_ON_DEVICE;
  st.init = ex.data();
  st.extras_bytes = st.init_bytes = sizeof(double) * ex.size();
  st.out_px = (size_t)(polar_width(sp.n_theta, sp.pad) * sp.n_r);
  return pre_stage(
      c, raw, out, n_img, pix, M, N, flags, st,
      [&](size_t staged) {
        if (staged) return stage_plan_z(n_img, staged, STAGE_SLOT_BUDGET);
        const int per = n_img < POLAR_CHUNK_MAX ? n_img : POLAR_CHUNK_MAX;
        return StagePlan{per, (n_img + per - 1) / per, 0, 0};
      },
      [&](const PreChunk& k) {
        const double* d_cxy = (const double*)k.d_extras;
        return launch_polar(c->stream, pix, k.d_src, k.d_dst, k.first, k.cnt, M, N, sp, d_cxy, nc, d_cxy + 2 * (size_t)nc,
                            d_cxy + 2 * (size_t)nc + sp.n_theta);
      },
      no_chunk_hook);
}

// Wavelet denoising (gpet_wavelet_plan.h).  Extras: sigma [n_img] | thresholds [n_img * levels * 3] | means of squares [the same].
// Frames go chunk by chunk (wv_chunks), the pyramids through the context's workspace, 2 levels + 2 launches per chunk (+ 1 with
// injected thresholds).  The per-frame figures come back at the end, which the call waits for: a frame without a noise level is an
// error.
int gpet_wavelet_images(gpet_ctx* c, const void* const* raw, int n_img, int pix, int M, int N, const gpet_wavelet* spec,
                        unsigned int flags, void* const* out) {
  if (!c || !raw || !spec || !out || n_img <= 0 || M <= 0 || N <= 0) return fail(c, GPET_ERR_BAD_ARG, "gpet_wavelet_images: bad argument");
  WvSpec sp;
  sp.n_taps = spec->n_taps;
  for (int k = 0; k < WV_TAPS_MAX; ++k) sp.dec_lo[k] = spec->dec_lo[k];
  sp.levels = spec->levels;
  sp.mode = spec->mode;
  sp.method = spec->method;
  sp.sigma = spec->sigma;
  sp.rescale_sigma = spec->rescale_sigma;
  sp.ppf = spec->ppf;
  sp.c = spec->c;
  sp.thresholds = spec->thresholds;
  sp.n_thresholds = spec->n_thresholds;
  if (const char* why = wv_check(sp, pix, M, N, n_img))
    return fail(c, GPET_ERR_BAD_ARG, "wavelet: %s (%d taps, wavelet_levels %d, max_level %d, frames %d x %d, %d thresholds)", why, sp.n_taps,
                sp.levels, sp.n_taps >= 2 ? wv_max_level(M < N ? M : N, sp.n_taps) : 0, M, N, sp.n_thresholds);
  for (int g = 0; g < n_img; ++g)
    if (!raw[g] || !out[g]) return fail(c, GPET_ERR_BAD_ARG, "gpet_wavelet_images: frame or output %d is a null pointer", g);
  const WvPlan wp = wv_plan(M, N, sp.n_taps, wv_levels(sp, M, N));
  const size_t n_thr = (size_t)n_img * wp.levels * 3, frame_bytes = wp.frame_doubles * sizeof(double);
  PreStage st;
  st.out_dev_bit = GPET_WV_OUT_ON_DEVICE;
  st.extras_bytes = sizeof(double) * ((size_t)n_img + 2 * n_thr);
  if (sp.thresholds) {
    st.init = sp.thresholds;
    st.init_off = sizeof(double) * (size_t)n_img;
    st.init_bytes = sizeof(double) * n_thr;
  }
  st.ws_bytes = dn_align(frame_bytes);
  st.read_back = true;
  const int rc = pre_stage(
      c, raw, out, n_img, pix, M, N, flags, st, [&](size_t staged) { return wv_chunks(n_img, staged, wp.frame_doubles); },
      [&](const PreChunk& k) {
        double* d_sigma = (double*)k.d_extras;
        return launch_wavelet(c->stream, pix, k.d_src, k.d_dst, k.first, k.cnt, wp, sp, k.ws, d_sigma, d_sigma + n_img, d_sigma + n_img + n_thr);
      },
      [&](const PreChunk& k) {  // (the chunk's pyramids, by the frame's number in the stack)
        hipError_t e = hipSuccess;
        for (int i = 0; i < k.cnt && spec->coeffs_out && e == hipSuccess; ++i)
          e = hipMemcpyAsync(spec->coeffs_out + (size_t)(k.first + i) * wp.frame_doubles, k.ws + (size_t)i * frame_bytes, frame_bytes,
                             hipMemcpyDeviceToHost, c->stream);
        return e;
      });
  if (rc) return rc;
  const double *h_sigma = (const double*)st.h_extras, *h_thr = h_sigma + n_img, *h_ms = h_thr + n_thr;
  if (spec->sigma_out) memcpy(spec->sigma_out, h_sigma, sizeof(double) * (size_t)n_img);
  if (spec->thresholds_out) memcpy(spec->thresholds_out, h_thr, sizeof(double) * n_thr);
  if (spec->mean_sq_out) memcpy(spec->mean_sq_out, h_ms, sizeof(double) * n_thr);
  for (int g = 0; g < n_img; ++g)
    if (!(h_sigma[g] > 0.0 && h_sigma[g] < INFINITY))
      return fail(c, GPET_ERR_BAD_ARG, !(sp.sigma != sp.sigma)
                      ? "wavelet: frame %d is flat: a given sigma under rescale_sigma is scaled by (max - min) / (max - min) of the frame"
                      : "wavelet: frame %d has no noise level: its finest diagonal band (dd of level 1) is all zero", g);
  return GPET_OK;
}

// Split-Bregman TV denoising (gpet_tvb_plan.h).  Extras: states [n_img].  Frames go chunk by chunk (tvb_chunks), the skewed arrays
// through the context's workspace; per chunk one prologue, tvb_launches(max_iter) sweep launches and one epilogue, enqueued without
// waiting.  The sweep counts come back at the end, only when the caller asks for them.
int gpet_tvb_images(gpet_ctx* c, const void* const* raw, int n_img, int pix, int M, int N, const gpet_tvb* spec, unsigned int flags,
                    void* const* out, int32_t* n_iter_out) {
  if (!c || !raw || !spec || !out || n_img <= 0)
    return fail(c, GPET_ERR_BAD_ARG, "gpet_tvb_images: bad argument (%s)", !c ? "no context" : !raw ? "raw is a null pointer" : !spec ? "spec is a null pointer"
                                                                           : !out ? "out is a null pointer" : "no frame");
  TvbSpec sp;
  sp.weight = spec->weight;
  sp.eps = spec->eps;
  sp.max_iter = spec->max_iter;
  sp.isotropic = spec->isotropic != 0;
  if (const char* why = tvb_check(sp, pix, M, N, n_img))
    return fail(c, GPET_ERR_BAD_ARG, "tvb: %s (weight %g, eps %g, max_iter %d, frames %d x %d)", why, sp.weight, sp.eps, sp.max_iter, M, N);
  for (int g = 0; g < n_img; ++g)
    if (!raw[g] || !out[g]) return fail(c, GPET_ERR_BAD_ARG, "gpet_tvb_images: frame or output %d is a null pointer", g);
  PreStage st;
  st.out_dev_bit = GPET_TVB_OUT_ON_DEVICE;
  st.extras_bytes = sizeof(TvbState) * (size_t)n_img;
  st.ws_bytes = tvb_frame_bytes(M, N);
  st.read_back = n_iter_out != nullptr;
  const int rc = pre_stage(
      c, raw, out, n_img, pix, M, N, flags, st, [&](size_t staged) { return tvb_chunks(n_img, staged, M, N); },
      [&](const PreChunk& k) { return launch_tvb(c->stream, pix, k.d_src, k.d_dst, k.first, k.cnt, M, N, sp, k.ws, (TvbState*)k.d_extras); },
      no_chunk_hook);
  if (rc) return rc;
  if (n_iter_out) {
    const TvbState* hs = (const TvbState*)st.h_extras;
    for (int g = 0; g < n_img; ++g) n_iter_out[g] = hs[g].n_iter;
  }
  return GPET_OK;
}

}  // extern "C"

