// C ABI, part 2: batches of edges -- creation (a driver over gpet_batch_plan.h, which resolves the edges and lays out the arena),
// destruction, images, observation sets, reset, reads and writes.
#include "gpet_api_internal.h"

extern "C" {

namespace {
// frees a half-built batch (arena, streams, events, tables, staging buffer) on every early return
struct BatchGuard {
  gpet_batch* b = nullptr;
  ~BatchGuard() {
    if (b) gpet_batch_destroy(b);
  }
};
}  // namespace

// gradient image(s) as the user passes them -> re-normalised f32 on the device (gpet.py:97).
// GPET_GRAD_ON_DEVICE: grad[] are device pointers (e.g. the tensor an RCCL broadcast has just filled): consumed in
// place, no trip through host memory.
// A vertical batch (b->transposed) takes the images in the frame's layout, bd.N rows of bd.M pixels: the order-free min / max reads
// them as they lie, and the normaliser writes the transpose into the slot (launch_transpose) instead of the copy.
static int upload_images(gpet_batch* b, const float* const* grad, unsigned int flags) {
  gpet_ctx* c = b->ctx;
  const size_t px = (size_t)b->bd.M * b->bd.N;
  const int n_img = b->n_img;
  const bool on_dev = (flags & GPET_GRAD_ON_DEVICE) != 0;
  for (int g = 0; g < n_img; ++g)
    if (!grad[g]) return fail(c, GPET_ERR_BAD_ARG, "gradient image %d is a null pointer", g);
  // every image its own (min, max) slot, all of them reset by ONE copy; the images then follow each other on the stream --
  // staging copy -> min / max -> normalise -- with a single wait at the end (round 5 waited after every image: 0.8 ms per
  // image of a 256-image set_frame, most of it the waits).  A device image (GPET_GRAD_ON_DEVICE) is read where it lies.
  b->h_mm0.assign((size_t)2 * n_img, 0u);
  for (int g = 0; g < n_img; ++g) b->h_mm0[2 * (size_t)g] = 0xFFFFFFFFu;
  HIPCHK(c, hipMemcpyAsync(b->d_minmax, b->h_mm0.data(), sizeof(unsigned int) * 2 * n_img, hipMemcpyHostToDevice, c->stream));
  for (int g = 0; g < n_img; ++g) {
    unsigned int* mm = b->d_minmax + 2 * (size_t)g;
    const float* src = grad[g];
    if (!on_dev) {
      HIPCHK(c, hipMemcpyAsync(b->d_raw, grad[g], px * sizeof(float), hipMemcpyHostToDevice, c->stream));
      src = b->d_raw;
    }
    HIPCHK(c, launch_minmax(c->stream, src, px, mm));
    if (b->transposed)
      HIPCHK(c, launch_transpose(c->stream, src, b->bd.N, b->bd.M, mm, (float*)b->h_edges[b->img_rep[g]].grad));
    else
      HIPCHK(c, launch_normalise(c->stream, src, px, mm, (float*)b->h_edges[b->img_rep[g]].grad));
  }
  HIPCHK(c, gpet_wait(c->stream));  // (pageable sources and h_mm0 must stay valid until the copies have run)
  return GPET_OK;
}

// The images of a batch as a caller may hand them over: finished f32 gradient images (gpet_batch_create2,
// gpet_batch_set_images), or raw frames with the kernel that turns them into gradient images (gpet_batch_create_raw,
// gpet_batch_set_raw_images).  Either way the arena's EdgeDev::grad buffers hold the normalised images afterwards.
struct ImageSource {
  const float* const* grad = nullptr;  // gradient images, or
  RawSourceArgs args;                  // raw frames (args.raw) with their kernels, as the entry point's arguments describe them
  unsigned int flags = 0;              // GPET_GRAD_ON_DEVICE / GPET_RAW_ON_DEVICE (and GPET_IMAGES_NEXT_FRAME, not read here)
  ImageSource(const float* const* grad_, unsigned int flags_) : grad(grad_), flags(flags_) {}
  // raw frames with one kernel (one image per frame: the batch says how many, check_batch_source) or with a slot table
  ImageSource(const void* const* raw, int pix, const double* kern, int kh, int kw, const gpet_denoise* dn, unsigned int flags_) : flags(flags_) {
    args.frames(raw, 0, pix, dn, flags);
    args.one_kernel(kern, kh, kw);
  }
  ImageSource(const void* const* raw, int n_frames, int pix, const gpet_denoise* dn, unsigned int flags_) : flags(flags_) {
    args.frames(raw, n_frames, pix, dn, flags);
  }
  bool is_raw() const { return args.raw.frames != nullptr; }
};

// what a batch of `count` images, made of frames that lie as Mf x Nf (tr: transposed into the batch), fills in of a source: one
// kernel makes one image of every frame
static void batch_source(RawSource& s, int count, int Mf, int Nf, bool tr) {
  if (!s.table) s.n_frames = s.n_img = count;
  s.M = Mf;
  s.N = Nf;
  s.tr = tr;
}

// raw frames -> comp_grad_img of each, straight into the arena: one batched pass on the device (conv_frames), no trip of a
// gradient image through host memory.  One normalisation: the second one of the two-step path (comp_grad_img, then gpet.py:97)
// subtracts a minimum of exactly 0 and divides by a span of exactly 1.
static int convolve_images(gpet_batch* b, RawSource s) {
  gpet_ctx* c = b->ctx;
  const int n_img = b->n_img;
  std::vector<float*> dst((size_t)n_img);
  for (int g = 0; g < n_img; ++g) dst[(size_t)g] = (float*)b->h_edges[b->img_rep[g]].grad;
  const bool tr = b->transposed;  // (the frames are then bd.N rows of bd.M pixels, and the slots receive their transposes)
  batch_source(s, n_img, tr ? b->bd.N : b->bd.M, tr ? b->bd.M : b->bd.N, tr);
  const int rc = conv_frames(c, s, dst.data(), b->d_minmax);
  if (rc) (void)gpet_wait(c->stream);  // (host frames already enqueued must not be read after the return)
  return rc;
}

// ---- tracking bands (gpet_band_plan.h, gpet_k_band.inc) --------------------------------------------------------------------------
// The n_pair full-frame gradient images into the batch's own memory: raw frames through conv_frames with the full frame's rows (the
// convolution sees the rows above and below every band, the min-max is the full frame's); gradient images as they are.
// A vertical batch stores the transposes -- G.T of every frame, bs.M rows of bd.N pixels like any other G, so that G + r0 * N stays
// what it is: raw frames by the transposed-store convolution, gradient images by launch_transpose (host images through d_raw).
static int band_load_full(gpet_batch* b, const ImageSource& s) {
  gpet_ctx* c = b->ctx;
  BandState& bs = b->band;
  const size_t px = (size_t)bs.M * b->bd.N;
  std::vector<float*> dst((size_t)bs.n_pair);
  for (int p = 0; p < bs.n_pair; ++p) dst[(size_t)p] = bs.G + (size_t)p * px;
  const bool tr = b->transposed;
  const int Mf = tr ? b->bd.N : bs.M, Nf = tr ? bs.M : b->bd.N;  // the frame as it lies in the caller's memory
  if (s.is_raw()) {
    RawSource rs = s.args.raw;
    batch_source(rs, bs.n_pair, Mf, Nf, tr);
    const int rc = conv_frames(c, rs, dst.data(), b->d_minmax);
    if (rc) (void)gpet_wait(c->stream);  // (host frames already enqueued must not be read after the return)
    return rc;
  }
  const bool on_dev = (s.flags & GPET_GRAD_ON_DEVICE) != 0;
  for (int p = 0; p < bs.n_pair; ++p)
    if (!s.grad[p]) return fail(c, GPET_ERR_BAD_ARG, "gradient image %d is a null pointer", p);
  for (int p = 0; p < bs.n_pair; ++p) {
    if (!tr) {
      HIPCHK(c, hipMemcpyAsync(dst[(size_t)p], s.grad[p], px * sizeof(float), on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
      continue;
    }
    const float* from = s.grad[p];
    if (!on_dev) {  // (d_raw holds a full frame on a vertical banded batch; the stream orders its reuse)
      HIPCHK(c, hipMemcpyAsync(b->d_raw, s.grad[p], px * sizeof(float), hipMemcpyHostToDevice, c->stream));
      from = b->d_raw;
    }
    HIPCHK(c, launch_transpose(c->stream, from, Mf, Nf, nullptr, dst[(size_t)p]));
  }
  if (!on_dev) HIPCHK(c, gpet_wait(c->stream));  // (pageable sources must stay valid until the copies have run)
  return GPET_OK;
}

// The image step of the slots: they move to the bands placed since the last swap (r0 and the init rows, on the device), then every
// edge's band of its full-frame image -- G_pair + r0 * N, read where it lies -- goes through min / max and the normalisation into the
// edge's own slot, as upload_images treats the image an unbanded batch is given.
static int band_slots(gpet_batch* b) {
  gpet_ctx* c = b->ctx;
  BandState& bs = b->band;
  const int B = b->B;
  if (bs.pending) {
    HIPCHK(c, launch_band_apply(c->stream, b->d_edges, B, bs.n_init_max, bs.pend, bs.init, bs.r0));
    bs.pending = false;
  }
  b->h_mm0.assign((size_t)2 * B, 0u);  // (every caller waits for the stream before it returns)
  for (int e = 0; e < B; ++e) b->h_mm0[2 * (size_t)e] = 0xFFFFFFFFu;
  HIPCHK(c, hipMemcpyAsync(b->d_minmax, b->h_mm0.data(), sizeof(unsigned int) * 2 * B, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch_band_images(c->stream, b->d_edges, B, bs.d_G_of, bs.r0, bs.H, b->bd.N, b->d_minmax));
  return GPET_OK;
}

static int load_images(gpet_batch* b, const ImageSource& s) {
  if (b->band.H) {
    const int rc = band_load_full(b, s);
    return rc ? rc : band_slots(b);
  }
  return s.is_raw() ? convolve_images(b, s.args.raw) : upload_images(b, s.grad, s.flags);
}

// smallest and largest init row of an edge
static void init_row_span(const int64_t* init_xy, int n_init, long long* i_lo, long long* i_hi) {
  *i_lo = *i_hi = init_xy[1];
  for (int i = 1; i < n_init; ++i) {
    *i_lo = std::min<long long>(*i_lo, init_xy[2 * i + 1]);
    *i_hi = std::max<long long>(*i_hi, init_xy[2 * i + 1]);
  }
}

// the device memory and tables of a banded batch, once the arena is laid out (n_init_max) and before the images are loaded; r0: the
// bands of the first frame, init_full: the caller's init points
static int band_setup(gpet_batch* b, const gpet_band& band, int M_full, const long long* r0, const int64_t* const* init_full, int n_init_max) {
  gpet_ctx* c = b->ctx;
  BandState& bs = b->band;
  const int B = b->B;
  bs.M = M_full;
  bs.n_pair = band.n_pair;
  bs.n_init_max = n_init_max;
  bs.pair_of.assign(band.pair_of, band.pair_of + B);
  HIPCHK(c, hipMalloc(&bs.G, band_image_bytes(bs.n_pair, M_full, b->bd.N)));
  HIPCHK(c, hipMalloc(&bs.tab, band_table_bytes(B, n_init_max)));
  HIPCHK(c, hipMalloc(&bs.d_G_of, sizeof(float*) * (size_t)B));
  const BandTables t = band_tables(B, n_init_max);
  bs.r0 = bs.tab + t.off_r0;
  bs.pend = bs.tab + t.off_pend;
  bs.fit = bs.tab + t.off_fit;
  bs.lohi = bs.tab + t.off_lohi;
  bs.init = bs.tab + t.off_init;
  bs.h_tab.assign(t.count, 0);
  for (int e = 0; e < B; ++e) {
    bs.h_tab[t.off_r0 + e] = bs.h_tab[t.off_pend + e] = bs.h_tab[t.off_fit + e] = r0[e];
    init_row_span(init_full[e], b->h_edges[e].n_init, &bs.h_tab[t.off_lohi + 2 * (size_t)e], &bs.h_tab[t.off_lohi + 2 * (size_t)e + 1]);
    memcpy(&bs.h_tab[t.off_init + (size_t)e * 2 * (size_t)n_init_max], init_full[e], sizeof(long long) * 2 * (size_t)b->h_edges[e].n_init);
  }
  HIPCHK(c, hipMemcpyAsync(bs.tab, bs.h_tab.data(), sizeof(long long) * t.count, hipMemcpyHostToDevice, c->stream));
  std::vector<const float*> g_of((size_t)B);
  for (int e = 0; e < B; ++e) g_of[(size_t)e] = bs.G + (size_t)bs.pair_of[(size_t)e] * (size_t)M_full * (size_t)b->bd.N;
  HIPCHK(c, hipMemcpyAsync(bs.d_G_of, g_of.data(), sizeof(float*) * (size_t)B, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, gpet_wait(c->stream));  // (g_of is a local)
  bs.H = band.H;  // (from here on the batch is banded)
  return GPET_OK;
}

// gradient KDE of every image slot (gpet.py:127), once per slot through the slot's representative edge: where the representatives
// are not the first n_img edges, over a device copy of their EdgeDev in slot order (as setup_struct_basis runs its classes)
static int image_kde(gpet_batch* b) {
  gpet_ctx* c = b->ctx;
  if (b->rep_is_prefix) {
    HIPCHK(c, launch_kde(c->stream, b->d_edges, b->n_img, b->bd, 1));
    return GPET_OK;
  }
  for (int g = 0; g < b->n_img; ++g) b->h_img_edges[(size_t)g] = b->h_edges[b->img_rep[g]];
  HIPCHK(c, hipMemcpyAsync(b->d_img_edges, b->h_img_edges.data(), sizeof(EdgeDev) * (size_t)b->n_img, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch_kde(c->stream, b->d_img_edges, b->n_img, b->bd, 1));
  return GPET_OK;
}

// what can be refused before anything is allocated or enqueued, for a batch of `count` images (conv_frames checks the same on its own)
// (tr: for a vertical batch, against the LDS bounds of the transposed-store kernels)
static int check_batch_source(gpet_ctx* c, const ImageSource& src, int count, bool tr) {
  RawSource s = src.args.raw;
  batch_source(s, count, 0, 0, tr);
  // (between the pixel type and the table in check_raw_source's order; every entry point hands over the batch's own count today)
  if (s.frames && pix_bytes(s.pix) && s.n_img != count)
    return fail(c, GPET_ERR_BAD_ARG, "slot table: %d slots for a batch of %d image slots", s.n_img, count);
  return check_raw_source(c, s);
}

int gpet_batch_create(gpet_ctx* c, int B, int M, int N, const float* const* grad, int share_image,
                      const gpet_params* params, const int64_t* const* init_xy, gpet_batch** out) {
  return gpet_batch_create2(c, B, M, N, grad, share_image, params, init_xy, 0u, out);
}

// the edges' device scalars back to those of a fresh batch (enqueued on the context's stream; h_scalars is the staging copy)
static hipError_t upload_pristine_scalars(gpet_batch* b) {
  pristine_scalars(b->params.data(), b->h_edges.data(), b->B, b->h_scalars.data());
  return hipMemcpyAsync(b->d_scalars, b->h_scalars.data(), sizeof(gpet_scalars) * (size_t)b->B, hipMemcpyHostToDevice, b->ctx->stream);
}

// Structured loop path: eigenbasis of the grid's correlation matrix, once per class of edges (basis_classes).  Usable when the
// LDS Jacobi applies (capacity <= 96) and every training point lies on the grid; option "struct_path" = 0 disables it.
static int setup_struct_basis(gpet_batch* b, const int64_t* const* init_xy) {
  gpet_ctx* c = b->ctx;
  const int B = b->B;
  b->structured = false;
  if (b->bd.r_cap > 96 || !opt(Opt::struct_path) || !struct_eligible(b->h_edges.data(), B, b->bd.N, init_xy)) return GPET_OK;
  // The basis is computed for the first edge of every class only (a batch of 1 024 equal edges: one factorisation instead of 1 024,
  // 7.5 ms of the constructor) and the others read that edge's copy, which then stays in L2 for the whole batch (k_struct_H
  // gathers its rows, k_struct_rows streams it: 288 KB per edge at rank 72, Lg 500).
  std::vector<int> rep_of, reps;
  basis_classes(b->h_edges.data(), B, rep_of, reps);
  if ((int)reps.size() == B) {
    HIPCHK(c, launch_struct_basis(c->stream, b->d_edges, B, b->bd));
  } else {
    std::vector<EdgeDev> h_rep(reps.size());
    for (size_t k = 0; k < reps.size(); ++k) h_rep[k] = b->h_edges[reps[k]];
    EdgeDev* d_rep = nullptr;
    HIPCHK(c, hipMalloc(&d_rep, sizeof(EdgeDev) * reps.size()));
    hipError_t e1 = hipMemcpyAsync(d_rep, h_rep.data(), sizeof(EdgeDev) * reps.size(), hipMemcpyHostToDevice, c->stream);
    if (e1 == hipSuccess) e1 = launch_struct_basis(c->stream, d_rep, (int)reps.size(), b->bd);
    if (e1 == hipSuccess) e1 = gpet_wait(c->stream);
    (void)hipFree(d_rep);
    HIPCHK(c, e1);
  }
  int rc = fetch_all_scalars(b);
  if (rc) return rc;
  bool ok = true;
  int r0_max = 0;
  for (int e = 0; e < B; ++e) {
    EdgeDev& E = b->h_edges[e];
    const EdgeDev& F = b->h_edges[rep_of[(size_t)e]];
    const gpet_scalars& s = b->h_scalars[rep_of[(size_t)e]];
    if (s.status != GPET_OK || s.rank < 1 || s.rank >= E.r_cap) ok = false;  // rank capacity reached
    E.r0 = s.rank;
    if (rep_of[(size_t)e] != e) {
      E.Q0 = F.Q0;
      E.lam0 = F.lam0;
      E.h0 = F.h0;  // (the sign convention's weights in that basis)
    }
    if (s.rank > r0_max) r0_max = s.rank;
  }
  b->bd.r0_max = r0_max;
  if (!struct_h_fits_lds(b->bd, r0_max)) ok = false;
  // back to the pristine scalar state
  for (int e = 0; e < B; ++e) b->h_edges[e].structured = ok ? 1 : 0;
  HIPCHK(c, upload_pristine_scalars(b));
  HIPCHK(c, hipMemcpyAsync(b->d_edges, b->h_edges.data(), sizeof(EdgeDev) * B, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, gpet_wait(c->stream));
  b->structured = ok;
  return GPET_OK;
}

// the one body of batch creation, whatever the images come as
// image_of == nullptr: one image for all edges (share_image) or one per edge; else the image map (n_img, image_of[B])
// band != nullptr (gpet_batch_create_banded): M is the full frame's, init_xy in its rows; the batch's own shape becomes (band->H, N)
// with one image slot per edge, and src describes the band->n_pair full-frame images
// src.flags & GPET_FRAMES_TRANSPOSED: M, N are the frames' as they lie; the batch is the one on the N x M transposes of their gradient
// images -- everything below the swap, bands included, counts in the batch's own rows and columns
static int batch_create_from(gpet_ctx* c, int B, int M, int N, const ImageSource& src, int share_image, int n_img,
                             const int32_t* image_of, const gpet_params* params, const int64_t* const* init_xy, gpet_batch** out,
                             const gpet_band* band = nullptr) {
  if (!c || !out || !batch_shape_ok(B, M, N) || (!src.grad && !src.is_raw()) || !params || !init_xy)
    return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_create: bad argument");
  *out = nullptr;
  const bool tr = (src.flags & GPET_FRAMES_TRANSPOSED) != 0;
  if (tr) std::swap(M, N);
  const int M_full = M;
  const int64_t* const* const init_full = init_xy;
  std::vector<long long> band_r0;
  std::vector<std::vector<int64_t>> band_init;
  std::vector<const int64_t*> band_init_p;
  if (band) {
    if (!band->pair_of) return fail(c, GPET_ERR_BAD_ARG, "band: pair_of is a null pointer");
    if (const char* why = image_map_check(B, band->n_pair, band->pair_of))
      return fail(c, GPET_ERR_BAD_ARG, "band: image table: %s (B = %d, n_pair = %d)", why, B, band->n_pair);
    band_r0.resize((size_t)B);
    band_init.resize((size_t)B);
    band_init_p.resize((size_t)B);
    for (int e = 0; e < B; ++e) {
      if (!init_xy[e] || params[e].n_init < 1) return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_create_banded: edge %d has no init points", e);
      long long i_lo, i_hi;
      init_row_span(init_xy[e], params[e].n_init, &i_lo, &i_hi);
      const long long r0 = band->r0 ? (long long)band->r0[e] : -1;
      if (const char* why = band_check(M, band->H, r0, i_lo, i_hi, !band->r0))
        return fail(c, GPET_ERR_BAD_ARG, "band of edge %d: %s (M = %d, H = %d, r0 = %lld, init rows %lld .. %lld)", e, why, M, (int)band->H,
                    r0, i_lo, i_hi);
      if (i_lo < 0 || i_hi > M - 1)
        return fail(c, GPET_ERR_BAD_ARG, "band of edge %d: an init point lies outside the frame (init rows %lld .. %lld, M = %d)", e, i_lo, i_hi, M);
      band_r0[(size_t)e] = band->r0 ? r0 : band_place(M, band->H, i_lo, i_hi, i_lo, i_hi);  // (the first frame: t = the init rows)
      band_init[(size_t)e].assign(init_xy[e], init_xy[e] + 2 * (size_t)params[e].n_init);
      for (int i = 0; i < params[e].n_init; ++i) band_init[(size_t)e][2 * (size_t)i + 1] -= band_r0[(size_t)e];
      band_init_p[(size_t)e] = band_init[(size_t)e].data();
    }
    init_xy = band_init_p.data();
    M = band->H;
    share_image = 0;
    image_of = nullptr;
  }
  const bool mapped = image_of != nullptr;
  if (mapped) {
    if (const char* why = image_map_check(B, n_img, image_of)) return fail(c, GPET_ERR_BAD_ARG, "image map: %s (B = %d, n_img = %d)", why, B, n_img);
    share_image = 0;
  } else {
    n_img = share_image ? 1 : B;
  }
  if (src.is_raw()) {
    const int rc0 = check_batch_source(c, src, band ? band->n_pair : n_img, tr);
    if (rc0) return rc0;
  }
  HIPCHK(c, hipSetDevice(c->device));
  gpet_batch* b = new (std::nothrow) gpet_batch();
  if (!b) return fail(c, GPET_ERR_HIP, "out of host memory");
  BatchGuard guard;
  guard.b = b;
  option_snapshot(&b->opts);  // the process-wide table as it is NOW is this batch's for its lifetime
  GPET_BATCH_SCOPE(b);
  b->ctx = c;
  b->B = B;
  b->share_image = share_image ? 1 : 0;
  b->transposed = tr;
  b->n_img = n_img;
  b->image_of.resize((size_t)B);
  for (int e = 0; e < B; ++e) b->image_of[(size_t)e] = mapped ? image_of[e] : (share_image ? 0 : e);
  b->img_rep.resize((size_t)n_img);
  image_map_reps(B, n_img, b->image_of.data(), b->img_rep.data());
  b->rep_is_prefix = true;
  for (int g = 0; g < n_img; ++g) b->rep_is_prefix = b->rep_is_prefix && b->img_rep[(size_t)g] == g;
  b->h_edges.resize(B);
  b->h_scalars.resize(B);
  b->params.assign(params, params + B);
  // the edges' geometry and capacities, the batch's dimensions
  const bool any_big = any_big_edge(params, B);
  const int jlog_max_b = opt(Opt::jlog_max_b);
  bool any_gen_nu = false;
  for (int e = 0; e < B; ++e) {
    const EdgeCheck chk = resolve_edge(b->h_edges[e], params[e], B, M, N, any_big, jlog_max_b);
    if (chk == EdgeCheck::inconsistent)
      return fail(c, edge_check_status(chk), "gpet_batch_create: edge %d has inconsistent parameters", e);
    if (chk == EdgeCheck::matern_nu)
      return fail(c, edge_check_status(chk), "Matern nu=%g is outside 0.01 <= nu <= 1000 (nu = inf is the RBF kernel)", params[e].nu);
    if (b->h_edges[e].nu_code == 3) any_gen_nu = true;
  }
  b->bd = reduce_dims(b->h_edges.data(), B, M, N);
  b->bd.rng4 = normals4_applies(b->h_edges.data(), B) ? 1 : 0;
  // the arena: measure, allocate, place
  // (an image map takes its slots at the front of the arena; without one the two layouts are what they always were)
  auto lay = [&](Carver& cv) {
    return mapped ? layout_batch(cv, b->h_edges.data(), B, b->bd, n_img, b->image_of.data())
                  : layout_batch(cv, b->h_edges.data(), B, b->bd, b->share_image != 0);
  };
  Carver meas;
  lay(meas);
  b->arena_bytes = meas.off + 256;
  hipError_t he = hipMalloc(&b->arena, b->arena_bytes);
  if (he != hipSuccess) {  // (the store a destroyed batch left for the next one is in nobody's use: its room first)
    (void)hipGetLastError();
    zstore_pool_drain();
    he = hipMalloc(&b->arena, b->arena_bytes);
  }
  if (he != hipSuccess) {
    b->arena = nullptr;
    return fail(c, GPET_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", b->arena_bytes, hipGetErrorString(he));
  }
  HIPCHK(c, hipMemsetAsync(b->arena, 0, b->arena_bytes, c->stream));
  Carver cv;
  cv.base = b->arena;
  const BatchBlocks bb = lay(cv);
  b->d_scalars = bb.scalars;
  b->d_fin_out = bb.fin_out;
  b->d_fin_par = bb.fin_par;
  b->d_obs = bb.obs;
  b->d_init = bb.init;
  // small allocations, streams, events
  HIPCHK(c, hipMalloc(&b->d_edges, sizeof(EdgeDev) * B));
  HIPCHK(c, hipMalloc(&b->d_seeds, sizeof(unsigned int) * B));
  HIPCHK(c, hipMalloc(&b->d_minmax, sizeof(unsigned int) * 2 * (size_t)B));
  if (!b->rep_is_prefix) {
    b->h_img_edges.resize((size_t)n_img);
    HIPCHK(c, hipMalloc(&b->d_img_edges, sizeof(EdgeDev) * (size_t)n_img));
  }
  // (the stream the normals run ahead of the loop on: default priority -- lowest / highest were measured, +-0)
  HIPCHK(c, hipStreamCreateWithFlags(&b->side, hipStreamNonBlocking));
  // the stream the converged fits' objective runs on has the highest priority (its launches are small and many)
  int pr_least = 0, pr_greatest = 0;
  HIPCHK(c, hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest));
  HIPCHK(c, hipStreamCreateWithPriority(&b->fit, hipStreamNonBlocking, pr_greatest));
  for (int i = 0; i < 16; ++i) HIPCHK(c, hipEventCreateWithFlags(&b->ev_norm[i], hipEventDisableTiming));
  for (int i = 0; i < 16; ++i) HIPCHK(c, hipEventCreateWithFlags(&b->ev_gemm[i], hipEventDisableTiming));
  for (int i = 0; i < 16; ++i) HIPCHK(c, hipEventCreateWithFlags(&b->ev_pix[i], hipEventDisableTiming));
  HIPCHK(c, hipEventCreateWithFlags(&b->ev_main, hipEventDisableTiming));
  // upload: gradient image(s) re-normalised on the device (gpet.py:97) or made there from raw frames, inits, initial scalars
  HIPCHK(c, hipMalloc(&b->d_raw, (size_t)(band && tr ? M_full : M) * N * sizeof(float)));  // (vertical and banded: a full frame)
  int rc = GPET_OK;
  if (band) {  // (the full-frame images now; the slots once d_edges is on the device: the band kernels read it)
    rc = band_setup(b, *band, M_full, band_r0.data(), init_full, bb.n_init_max);
    if (!rc) rc = band_load_full(b, src);
  } else {
    rc = load_images(b, src);
  }
  if (rc) return rc;
  // (one copy each for the init points and the initial scalars of all edges: 3 x B small copies were most of the constructor)
  b->n_init_max = bb.n_init_max;
  std::vector<long long>& h_init = b->h_init;
  h_init.assign((size_t)B * 2 * (size_t)bb.n_init_max, 0);
  for (int e = 0; e < B; ++e)
    memcpy(&h_init[(size_t)e * 2 * (size_t)bb.n_init_max], init_xy[e], sizeof(long long) * 2 * (size_t)b->h_edges[e].n_init);
  HIPCHK(c, hipMemcpyAsync(b->d_init, h_init.data(), sizeof(long long) * h_init.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, upload_pristine_scalars(b));
  HIPCHK(c, hipMemcpyAsync(b->d_edges, b->h_edges.data(), sizeof(EdgeDev) * B, hipMemcpyHostToDevice, c->stream));
  if (any_gen_nu) HIPCHK(c, launch_rho_tab(c->stream, b->d_edges, B, N));
  if (band) {
    rc = band_slots(b);
    if (rc) return rc;
  }
  rc = image_kde(b);
  if (rc) return rc;
  HIPCHK(c, gpet_wait(c->stream));
  rc = setup_struct_basis(b, init_xy);
  if (rc) return rc;
  guard.b = nullptr;  // success: the caller owns the batch
  *out = b;
  return GPET_OK;
}

int gpet_batch_create2(gpet_ctx* c, int B, int M, int N, const float* const* grad, int share_image,
                       const gpet_params* params, const int64_t* const* init_xy, unsigned int flags, gpet_batch** out) {
  return batch_create_from(c, B, M, N, ImageSource(grad, flags), share_image, 0, nullptr, params, init_xy, out);
}

int gpet_batch_create_mapped(gpet_ctx* c, int B, int M, int N, int n_img, const int32_t* image_of, const float* const* grad,
                             const gpet_params* params, const int64_t* const* init_xy, unsigned int flags, gpet_batch** out) {
  if (!image_of) return fail(c, GPET_ERR_BAD_ARG, "image map: image_of is a null pointer");
  return batch_create_from(c, B, M, N, ImageSource(grad, flags), 0, n_img, image_of, params, init_xy, out);
}

int gpet_batch_create_raw_mapped(gpet_ctx* c, int B, int M, int N, int n_img, const int32_t* image_of, const void* const* raw, int pix,
                                 const double* kern, int kh, int kw, const gpet_denoise* dn, const gpet_params* params,
                                 const int64_t* const* init_xy, unsigned int flags, gpet_batch** out) {
  if (!raw || !kern) return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_create_raw_mapped: bad argument");
  if (!image_of) return fail(c, GPET_ERR_BAD_ARG, "image map: image_of is a null pointer");
  return batch_create_from(c, B, M, N, ImageSource(raw, pix, kern, kh, kw, dn, flags), 0, n_img, image_of, params, init_xy, out);
}

int gpet_batch_create_raw_multi(gpet_ctx* c, int B, int M, int N, int n_img, const int32_t* image_of, int n_frames, const void* const* raw,
                                int pix, int n_kern, const double* const* kern, const int32_t* kh, const int32_t* kw, const int32_t* frame_of,
                                const int32_t* kernel_of, const gpet_denoise* dn, const gpet_params* params, const int64_t* const* init_xy,
                                unsigned int flags, gpet_batch** out) {
  if (!raw || !kern) return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_create_raw_multi: bad argument");
  if (!image_of) return fail(c, GPET_ERR_BAD_ARG, "image map: image_of is a null pointer");
  ImageSource src(raw, n_frames, pix, dn, flags);
  src.args.slot_table(n_kern, kern, kh, kw, n_img, frame_of, kernel_of);
  return batch_create_from(c, B, M, N, src, 0, n_img, image_of, params, init_xy, out);
}

int gpet_batch_create_raw_dn(gpet_ctx* c, int B, int M, int N, const void* const* raw, int pix, const double* kern, int kh, int kw,
                             const gpet_denoise* dn, int share_image, const gpet_params* params, const int64_t* const* init_xy,
                             unsigned int flags, gpet_batch** out) {
  if (!raw || !kern) return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_create_raw_dn: bad argument");
  return batch_create_from(c, B, M, N, ImageSource(raw, pix, kern, kh, kw, dn, flags), share_image, 0, nullptr, params, init_xy, out);
}

int gpet_batch_create_raw(gpet_ctx* c, int B, int M, int N, const void* const* raw, int pix, const double* kern, int kh, int kw,
                          int share_image, const gpet_params* params, const int64_t* const* init_xy, unsigned int flags,
                          gpet_batch** out) {
  return gpet_batch_create_raw_dn(c, B, M, N, raw, pix, kern, kh, kw, nullptr, share_image, params, init_xy, flags, out);
}

int gpet_batch_create_banded(gpet_ctx* c, int B, int M, int N, const gpet_band* band, const gpet_band_images* im,
                             const gpet_params* params, const int64_t* const* init_xy, gpet_batch** out) {
  if (!band || !im || (!im->grad && !im->raw)) return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_create_banded: bad argument");
  if (im->grad) return batch_create_from(c, B, M, N, ImageSource(im->grad, im->flags), 0, 0, nullptr, params, init_xy, out, band);
  if (!im->kern || !im->kh || !im->kw || !im->frame_of || !im->kernel_of)
    return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_create_banded: raw frames need their kernels and the slot table");
  ImageSource src(im->raw, im->n_frames, im->pix, im->dn, im->flags);
  src.args.slot_table(im->n_kern, im->kern, im->kh, im->kw, band->n_pair, im->frame_of, im->kernel_of);
  return batch_create_from(c, B, M, N, src, 0, 0, nullptr, params, init_xy, out, band);
}

// the explicit table for the next swap (the placed one: gpet_batch_band_place, gpet_api_ensemble.hip)
int gpet_batch_band_set(gpet_batch* b, const int64_t* r0) {
  GPET_BATCH_SCOPE(b);
  if (!b || !r0) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  BandState& bs = b->band;
  if (!bs.H) return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_band_set: the batch has no bands (gpet_batch_create_banded makes one that has)");
  const BandTables t = band_tables(b->B, bs.n_init_max);
  const int rc_t = band_refresh_host(b);  // (the init points may have moved on the device since the host copy was made)
  if (rc_t) return rc_t;
  for (int e = 0; e < b->B; ++e) {
    const long long i_lo = bs.h_tab[t.off_lohi + 2 * (size_t)e], i_hi = bs.h_tab[t.off_lohi + 2 * (size_t)e + 1];
    if (const char* why = band_check(bs.M, bs.H, r0[e], i_lo, i_hi))
      return fail(c, GPET_ERR_BAD_ARG, "band of edge %d: %s (M = %d, H = %d, r0 = %lld, init rows %lld .. %lld)", e, why, bs.M, bs.H,
                  (long long)r0[e], i_lo, i_hi);
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gpet_wait(c->stream));  // (h_r0 may still be the source of an earlier copy)
  bs.h_r0.assign(r0, r0 + b->B);
  HIPCHK(c, hipMemcpyAsync(bs.pend, bs.h_r0.data(), sizeof(long long) * (size_t)b->B, hipMemcpyHostToDevice, c->stream));
  bs.pending = true;
  return GPET_OK;
}

int gpet_batch_band_r0(gpet_batch* b, int64_t* r0_out) {
  GPET_BATCH_SCOPE(b);
  if (!b || !r0_out) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  if (!b->band.H) return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_band_r0: the batch has no bands");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(r0_out, b->band.r0, sizeof(long long) * (size_t)b->B, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, gpet_wait(c->stream));
  return GPET_OK;
}

void gpet_batch_destroy(gpet_batch* b) {
  GPET_BATCH_SCOPE(b);
  if (!b) return;
  (void)hipSetDevice(b->ctx->device);
  (void)hipStreamSynchronize(b->ctx->stream);
  if (b->arena) (void)hipFree(b->arena);
  if (b->d_edges) (void)hipFree(b->d_edges);
  if (b->d_edges_act) (void)hipFree(b->d_edges_act);
  if (b->d_seeds_act) (void)hipFree(b->d_seeds_act);
  if (b->d_seeds) (void)hipFree(b->d_seeds);
  if (b->d_minmax) (void)hipFree(b->d_minmax);
  if (b->d_img_edges) (void)hipFree(b->d_img_edges);
  if (b->d_raw) (void)hipFree(b->d_raw);
  if (b->ev_l0) (void)hipEventDestroy(b->ev_l0);
  if (b->ev_l1) (void)hipEventDestroy(b->ev_l1);
  if (b->d_fin_stage) (void)hipFree(b->d_fin_stage);
  if (b->d_fin_n) (void)hipFree(b->d_fin_n);
  if (b->d_results) (void)hipFree(b->d_results);
  if (b->d_hist) (void)hipFree(b->d_hist);
  zstore_release(b);
  if (b->zst.d_edges) (void)hipFree(b->zst.d_edges);
  if (b->zst.d_seeds) (void)hipFree(b->zst.d_seeds);
  if (b->zst.d_running) (void)hipFree(b->zst.d_running);
  ensemble_free(b);
  label_free(b->lab);
  if (b->band.G) (void)hipFree(b->band.G);
  if (b->band.tab) (void)hipFree(b->band.tab);
  if (b->band.d_G_of) (void)hipFree(b->band.d_G_of);
  if (b->fit) {
    (void)hipStreamSynchronize(b->fit);
    (void)hipStreamDestroy(b->fit);
  }
  if (b->side) {
    (void)hipStreamSynchronize(b->side);
    (void)hipStreamDestroy(b->side);
  }
  for (int i = 0; i < 16; ++i)
    if (b->ev_norm[i]) (void)hipEventDestroy(b->ev_norm[i]);
  for (int i = 0; i < 16; ++i)
    if (b->ev_gemm[i]) (void)hipEventDestroy(b->ev_gemm[i]);
  for (int i = 0; i < 16; ++i)
    if (b->ev_pix[i]) (void)hipEventDestroy(b->ev_pix[i]);
  if (b->ev_main) (void)hipEventDestroy(b->ev_main);
  if (b->d_edge_of) (void)hipFree(b->d_edge_of);
  if (b->d_theta) (void)hipFree(b->d_theta);
  if (b->d_f) (void)hipFree(b->d_f);
  if (b->d_g) (void)hipFree(b->d_g);
  if (b->lb_mem) (void)hipFree(b->lb_mem);
  if (b->mtj_work) (void)hipFree(b->mtj_work);
  if (b->d_mtj_poly) (void)hipFree(b->d_mtj_poly);
  if (b->big_mem) (void)hipFree(b->big_mem);
  for (hipEvent_t ev : b->lb_events) (void)hipEventDestroy(ev);
  delete b;
}

int gpet_batch_size(const gpet_batch* b) { return b ? b->B : 0; }

int gpet_batch_image_count(const gpet_batch* b) { return b ? batch_source_count(b) : 0; }

int gpet_batch_info(const gpet_batch* b, int e, int32_t* out, int count) {
  if (!b || e < 0 || e >= b->B || !out) return GPET_ERR_BAD_ARG;
  const EdgeDev& E = b->h_edges[e];
  // (the last three: the normals store -- iterations held per edge (0: none, the batch runs on its ring alone), its size, and the
  //  (edge, iteration) streams the loop has generated so far for iterations the edge ran, then the streams its store launches drew,
  //  exactly; both saturating)
  const long long gen = b->zst.generated < 0x7fffffffll ? b->zst.generated : 0x7fffffffll;
  const long long drw = b->zst.drawn < 0x7fffffffll ? b->zst.drawn : 0x7fffffffll;
  const int32_t v[18] = {E.Lg, E.S, E.n_keep, E.n_cap, E.r_cap, E.z_cols, E.a_rows_cap, E.n_bins, E.obs_cap, E.algo_thresh,
                         b->structured ? 1 : 0, E.r0, E.z_ring, (int32_t)(b->arena_bytes >> 20),
                         b->zst.iters, (int32_t)(b->zst.bytes >> 20), (int32_t)gen, (int32_t)drw};
  for (int i = 0; i < count && i < 18; ++i) out[i] = v[i];
  return GPET_OK;
}

}  // extern "C"

// (shared with the other units: C++ linkage)
static int read_scalars(gpet_batch* b, int e, gpet_scalars* s) {
  gpet_ctx* c = b->ctx;
  HIPCHK(c, hipMemcpyAsync(s, b->h_edges[e].sc, sizeof *s, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, gpet_wait(c->stream));
  return GPET_OK;
}

int fetch_all_scalars(gpet_batch* b) {
  gpet_ctx* c = b->ctx;
  HIPCHK(c, hipMemcpyAsync(b->h_scalars.data(), b->d_scalars, sizeof(gpet_scalars) * b->B, hipMemcpyDeviceToHost,
                           c->stream));
  HIPCHK(c, gpet_wait(c->stream));
  return GPET_OK;
}

int check_device_status(gpet_batch* b) {
  gpet_ctx* c = b->ctx;
  int rc = fetch_all_scalars(b);
  if (rc) return rc;
  for (int e = 0; e < b->B; ++e) {
    const gpet_scalars& s = b->h_scalars[e];
    if (s.status == GPET_ERR_NOT_PD)
      return fail(c, GPET_ERR_NOT_PD, "edge %d: the kernel matrix is not positive definite (n=%d)", e, s.n);
    if (s.status == GPET_ERR_RANK_CAP)
      return fail(c, GPET_ERR_RANK_CAP, "edge %d: posterior covariance rank exceeds factor_cap=%d", e, b->h_edges[e].r_cap);
    if (s.status == GPET_ERR_ITER_CAP)
      return fail(c, GPET_ERR_ITER_CAP, "edge %d: no score threshold yields enough new pixels (the reference would loop forever, gpet.py:591-609)", e);
    if (s.status != GPET_OK) return fail(c, s.status, "edge %d: device status %d", e, s.status);
  }
  return GPET_OK;
}

// What every warm start does once its kernel is enqueued (gpet_batch_warm_start, gpet_batch_warm_start_groups / _from): the histories
// emptied, the flags of a new trace, the one copy of the scalars with the one wait -- the counts are in them.
int warm_start_finish(gpet_batch* b, int32_t* n_obs_out) {
  const int rc_h = history_clear(b, -1);
  if (rc_h) return rc_h;
  state_apply(b->st, StateEvent::observations_set);
  const int rc = fetch_all_scalars(b);  // (the one copy and the one wait: the counts are in the scalars)
  if (rc) return rc;
  b->h_nobs_prev.assign((size_t)b->B, 0);
  for (int e = 0; e < b->B; ++e) {
    b->h_nobs_prev[(size_t)e] = b->h_scalars[(size_t)e].n_obs;
    if (n_obs_out) n_obs_out[e] = b->h_scalars[(size_t)e].n_obs;
  }
  return GPET_OK;
}

extern "C" {

// The any-rank factor's rows of the trace that ends here may serve as the FIRST warm start of the next one -- only when
// the caller says the next trace is the next frame of a sequence (gpet_batch_set_images with GPET_IMAGES_NEXT_FRAME: the
// same chain, a similar covariance).  They are in slot (iters_done - 1) & 1 of the ring if its tag says "iteration
// iters_done - 1, full rank, converged".  Every other restart (gpet_batch_reset, gpet_batch_set_obs) clears all tags: a
// trace is then a function of (image, seed, observations) alone, whatever the batch object ran before.
static int clear_factor_rows(gpet_batch* b, int e) {
  gpet_ctx* c = b->ctx;
  HIPCHK(c, hipMemsetAsync(b->h_edges[e].ap_tag, 0, 3 * sizeof(int), c->stream));
  return GPET_OK;
}

// all edges at once: one wait for the tags, one for their replacements (iters[e] = iterations the edge's last trace ran)
static int carry_factor_rows_all(gpet_batch* b, const std::vector<int>& iters) {
  gpet_ctx* c = b->ctx;
  const int B = b->B;
  std::vector<int> tags((size_t)3 * B, 0);
  for (int e = 0; e < B; ++e)
    HIPCHK(c, hipMemcpyAsync(&tags[3 * e], b->h_edges[e].ap_tag, 3 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, gpet_wait(c->stream));
  for (int e = 0; e < B; ++e) {
    const int it = iters[e], slot = (it - 1) & 1;
    const int keep = (b->h_edges[e].r_cap > 96 && it >= 1 && tags[3 * e + slot] == it) ? slot + 1 : 0;
    tags[3 * e] = tags[3 * e + 1] = 0;
    tags[3 * e + 2] = keep;
    HIPCHK(c, hipMemcpyAsync(b->h_edges[e].ap_tag, &tags[3 * e], 3 * sizeof(int), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, gpet_wait(c->stream));  // (tags is a local)
  return GPET_OK;
}

int gpet_batch_set_obs(gpet_batch* b, int e, const int64_t* obs_xy, int n_obs) {
  GPET_BATCH_SCOPE(b);
  if (!b || e < 0 || e >= b->B || n_obs < 0 || (n_obs > 0 && !obs_xy)) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  EdgeDev& E = b->h_edges[e];
  if (n_obs > E.obs_cap) return fail(c, GPET_ERR_BAD_ARG, "n_obs=%d exceeds obs_cap=%d", n_obs, E.obs_cap);
  state_apply(b->st, StateEvent::set_obs_entry);  // (the trace that follows is not the one the fits in d_fin_out belong to)
  // the pixel kernels index the density images with the observations (gpet.py:568: kde_arr[pre_fobs[:,0], pre_fobs[:,1]]
  // raises IndexError in the reference for pixels outside the image)
  for (int i = 0; i < n_obs; ++i)
    if (obs_xy[2 * i] < 0 || obs_xy[2 * i] >= E.N || obs_xy[2 * i + 1] < 0 || obs_xy[2 * i + 1] >= E.M)
      return fail(c, GPET_ERR_BAD_ARG, "observation %d = (%lld, %lld) lies outside the %d x %d image", i,
                  (long long)obs_xy[2 * i], (long long)obs_xy[2 * i + 1], E.M, E.N);
  HIPCHK(c, hipSetDevice(c->device));
  gpet_scalars s;
  int rc = read_scalars(b, e, &s);
  if (rc) return rc;
  s.n_obs = n_obs;
  s.done = (n_obs >= E.algo_thresh) ? 1 : 0;
  s.status = GPET_OK;
  const int iters_done = s.iter;
  s.iter = 0;            // a new observation set restarts the edge's loop (gpet.py:820-828)
  HIPCHK(c, hipMemsetAsync(E.wq_tag, 0, 2 * sizeof(int), c->stream));  // (and forgets the last trace's eigenvectors)
  if (iters_done >= 1) {  // (0: gpet_batch_reset / gpet_batch_set_images has been here already and decided what stays)
    int rc3 = clear_factor_rows(b, e);
    if (rc3) return rc3;
  }
  state_apply(b->st, StateEvent::observations_set);  // (all edges of a batch are restarted together)
  int rc4 = history_clear(b, e);  // (the history is the trace's that ends here)
  if (rc4) return rc4;
  if ((int)b->h_nobs_prev.size() != b->B) b->h_nobs_prev.assign(b->B, 0);
  b->h_nobs_prev[e] = n_obs;  // (a batch of up to 64 edges sizes the loop's groups by the growth of its observation sets from here: next_group)
  if (b->structured)
    for (int i = 0; i < n_obs; ++i)
      if (obs_xy[2 * i] < E.x_st || obs_xy[2 * i] > E.x_en) {  // off-grid training point: generic path from now on
        b->structured = false;
        break;
      }
  if (n_obs > 0)
    HIPCHK(c, hipMemcpyAsync(E.obs_xy, obs_xy, sizeof(long long) * 2 * n_obs, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(E.sc, &s, sizeof s, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, gpet_wait(c->stream));
  return GPET_OK;
}

// GPET_OK when gpet_batch_warm_start can run, else its refusal -- for a caller that swaps the images first and must not find out after
int gpet_batch_warm_start_ready(gpet_batch* b) {
  if (!b) return GPET_ERR_BAD_ARG;
  if (state_missing(b->st, StateEvent::read_last_fit))
    return fail(b->ctx, GPET_ERR_BAD_ARG, "gpet_batch_warm_start: no converged fits of a last trace on the device (run a trace to its "
                                          "gpet_final_fit_all first; gpet_batch_set_obs or a warm start since then have used them up)");
  return GPET_OK;
}

// The observation sets of the next frame from the converged fits of the last trace, on the device (k_warm_start: the rule of
// sequence.warm_start_obs); leaves what B calls of gpet_batch_set_obs with those sets leave, with one wait in all.
int gpet_batch_warm_start(gpet_batch* b, int warm_every, int32_t* n_obs_out) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  const int ready = gpet_batch_warm_start_ready(b);
  if (ready) return ready;
  HIPCHK(c, hipSetDevice(c->device));
  if (b->band.H)  // (across bands: k_warm_start_src's banded form with every edge its own source)
    HIPCHK(c, launch_warm_start_band(c->stream, b->d_edges, b->B, nullptr, nullptr, nullptr, 0, 0, warm_every, b->band.fit, b->band.r0));
  else
    HIPCHK(c, launch_warm_start(c->stream, b->d_edges, b->B, warm_every));
  return warm_start_finish(b, n_obs_out);
}

int gpet_batch_read(gpet_batch* b, int e, int which, void* dst, size_t bytes) {
  GPET_BATCH_SCOPE(b);
  if (!b || e < 0 || e >= b->B || !dst) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  const EdgeDev& E = b->h_edges[e];
  gpet_scalars s;
  int rc = read_scalars(b, e, &s);
  if (rc) return rc;
  const void* src = nullptr;
  size_t avail = 0;
  const size_t Lg = E.Lg, n = s.n, px = (size_t)E.M * E.N;
  switch (which) {
    case GPET_BUF_X_TRAIN: src = E.xt; avail = n * 8; break;
    case GPET_BUF_Y_TRAIN: src = E.yt; avail = n * 8; break;
    case GPET_BUF_NOISE_W: src = E.wt; avail = n * 8; break;
    case GPET_BUF_ALPHA: src = E.alpha; avail = n * 8; break;
    case GPET_BUF_MEAN: src = E.mean; avail = Lg * 8; break;
    case GPET_BUF_STD: src = E.std; avail = Lg * 8; break;
    case GPET_BUF_COV: src = E.cov; avail = Lg * Lg * 8; break;
    case GPET_BUF_FACTOR: src = E.A; avail = (size_t)s.rank * Lg * 8; break;
    case GPET_BUF_EIGVALS: src = E.theta; avail = (size_t)s.rank * 8; break;
    case GPET_BUF_NORMALS: src = z_slot(E, s.iter); avail = (size_t)E.S * E.z_cols * 8; break;
    case GPET_BUF_SAMPLES: {
      // rows of Yp elements on the device (f32 after gpet_batch_set_sample_dtype); the interface is a dense [S][Lg] f64 matrix
      const size_t cnt = (size_t)E.S * Lg, pitch = (size_t)E.Yp, esz = E.y_f32 ? 4 : 8;
      if (bytes > cnt * 8) bytes = cnt * 8;
      std::vector<char> tmp((size_t)E.S * pitch * esz);
      HIPCHK(c, hipMemcpyAsync(tmp.data(), E.Y, tmp.size(), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, gpet_wait(c->stream));
      double* o = (double*)dst;
      for (size_t i = 0; i < bytes / 8; ++i) {
        const size_t at = (i / Lg) * pitch + i % Lg;
        o[i] = E.y_f32 ? (double)((const float*)tmp.data())[at] : ((const double*)tmp.data())[at];
      }
      return GPET_OK;
    }
    case GPET_BUF_COSTS: src = E.costs; avail = (size_t)E.S * 8; break;
    case GPET_BUF_BEST_IDX: src = E.best_idx; avail = (size_t)E.n_keep * 4; break;
    case GPET_BUF_BEST_COSTS: src = E.best_costs; avail = (size_t)E.n_keep * 8; break;
    case GPET_BUF_OBS: src = E.obs_xy; avail = (size_t)s.n_obs * 16; break;
    case GPET_BUF_KDE: src = E.kde; avail = px * 4; break;
    case GPET_BUF_GRAD_KDE: src = E.grad_kde; avail = px * 4; break;
    case GPET_BUF_GRAD: src = E.grad; avail = px * 4; break;
    case GPET_BUF_SCALARS:
      memcpy(dst, &s, bytes < sizeof s ? bytes : sizeof s);
      return GPET_OK;
    case GPET_BUF_FIN_PAR: src = E.fin_par; avail = 12 * 8; break;
    case GPET_BUF_KDE_TILES: {
      const size_t nt = ((size_t)E.N + KDE_TX - 1) / KDE_TX;
      if (bytes < (nt + 1) * 8) return fail(c, GPET_ERR_BAD_ARG, "KDE_TILES read needs %zu bytes", (nt + 1) * 8);
      HIPCHK(c, hipMemcpyAsync((char*)dst, E.kde_band, nt * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync((char*)dst + nt * 8, E.mm, 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, gpet_wait(c->stream));
      return GPET_OK;
    }
    case GPET_BUF_STRUCT_Q0: case GPET_BUF_STRUCT_LAM0: case GPET_BUF_STRUCT_H: {
      if (!b->structured) return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_read: buffer %d exists on a structured batch only", which);
      const size_t r0 = (size_t)E.r0;
      if (which == GPET_BUF_STRUCT_Q0) { src = E.Q0; avail = r0 * Lg * 8; break; }
      if (which == GPET_BUF_STRUCT_LAM0) { src = E.lam0; avail = r0 * 8; break; }
      // H: compact [r0][r0] out of E.C, whose rows have the stride r_cap
      if (bytes < r0 * r0 * 8) return fail(c, GPET_ERR_BAD_ARG, "STRUCT_H read needs %zu bytes", r0 * r0 * 8);
      HIPCHK(c, hipMemcpy2DAsync(dst, r0 * 8, E.C, (size_t)E.r_cap * 8, r0 * 8, r0, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, gpet_wait(c->stream));
      return GPET_OK;
    }
    case GPET_BUF_FIN_STARTS:
      if (!b->lb_starts) return fail(c, GPET_ERR_STATE, "no converged fit has run on this batch yet");
      src = b->lb_starts + (size_t)e * 39;
      avail = 39 * 8;
      break;
    case GPET_BUF_FIN_TRAIN: {
      const size_t nc = E.n_cap;
      if (bytes < 3 * nc * 8) return fail(c, GPET_ERR_BAD_ARG, "FIN_TRAIN read needs %zu bytes", 3 * nc * 8);
      HIPCHK(c, hipMemcpyAsync((char*)dst, E.fin_x, nc * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync((char*)dst + nc * 8, E.fin_y, nc * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync((char*)dst + 2 * nc * 8, E.fin_w, nc * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, gpet_wait(c->stream));
      return GPET_OK;
    }
    case GPET_BUF_FIN_OUT: {
      // dense [2][Lg]: on the device the std half sits at the widest edge's stride (bd.Lg), whatever this edge's width
      if (bytes < 2 * Lg * 8) return fail(c, GPET_ERR_BAD_ARG, "FIN_OUT read needs %zu bytes", 2 * Lg * 8);
      HIPCHK(c, hipMemcpyAsync((char*)dst, E.fin_out, Lg * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync((char*)dst + Lg * 8, E.fin_out + b->bd.Lg, Lg * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, gpet_wait(c->stream));
      return GPET_OK;
    }
    case GPET_BUF_CHOL: {
      // compact n x n lower-triangular copy (upper part zeroed)
      if (bytes < n * n * 8) return fail(c, GPET_ERR_BAD_ARG, "CHOL read needs %zu bytes", n * n * 8);
      std::vector<double> full((size_t)E.n_cap * E.n_cap);
      HIPCHK(c, hipMemcpyAsync(full.data(), E.K, full.size() * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, gpet_wait(c->stream));
      double* o = (double*)dst;
      for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j) o[i * n + j] = (j <= i) ? full[i * E.n_cap + j] : 0.0;
      return GPET_OK;
    }
    default:
      return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_read: unknown buffer %d", which);
  }
  if (bytes > avail) bytes = avail;
  if (which == GPET_BUF_EIGVALS) {
    std::vector<double> th(s.rank);
    std::vector<int> ord(s.rank);
    if (s.rank > 0) {
      HIPCHK(c, hipMemcpyAsync(th.data(), E.theta, (size_t)s.rank * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(ord.data(), E.order, (size_t)s.rank * 4, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, gpet_wait(c->stream));
    }
    // (the rows' squared norms in the rows' order, which the Jacobi's own diagonal decided: within a group of eigenvalues that
    //  are equal to rounding the norms need not follow it to the last bit -- the values leave in descending order)
    std::vector<double> ev(s.rank);
    for (int k = 0; k < s.rank; ++k) ev[k] = th[ord[k]];
    std::sort(ev.begin(), ev.end(), [](double a, double b) { return a > b; });
    double* o = (double*)dst;
    for (size_t k = 0; k < bytes / 8; ++k) o[k] = ev[k];
    return GPET_OK;
  }
  if (bytes) {
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, gpet_wait(c->stream));
  }
  return GPET_OK;
}

int gpet_batch_write(gpet_batch* b, int e, int which, const void* src, size_t bytes, int rows) {
  GPET_BATCH_SCOPE(b);
  if (!b || e < 0 || e >= b->B || !src) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  EdgeDev& E = b->h_edges[e];
  const size_t Lg = E.Lg, px = (size_t)E.M * E.N;
  void* dst = nullptr;
  size_t cap = 0;
  switch (which) {
    case GPET_BUF_FACTOR: {
      if (rows < 0 || rows > E.a_rows_cap || rows > E.z_cols)
        return fail(c, GPET_ERR_BAD_ARG, "factor rows=%d exceeds capacity (a_rows_cap=%d, z_cols=%d); create the batch with z_cols=Lg", rows, E.a_rows_cap, E.z_cols);
      dst = E.A;
      cap = (size_t)rows * Lg * 8;
      if (bytes != cap) return fail(c, GPET_ERR_BAD_ARG, "factor write: expected %zu bytes", cap);
      gpet_scalars s;
      int rc = read_scalars(b, e, &s);
      if (rc) return rc;
      s.rank = rows;
      HIPCHK(c, hipMemcpyAsync(E.sc, &s, sizeof s, hipMemcpyHostToDevice, c->stream));
      E.factor_injected = 1;
      HIPCHK(c, hipMemcpyAsync(b->d_edges + e, &E, sizeof E, hipMemcpyHostToDevice, c->stream));
      state_apply(b->st, StateEvent::write_factor);
      break;
    }
    case GPET_BUF_NORMALS: {
      gpet_scalars s;
      int rc = read_scalars(b, e, &s);
      if (rc) return rc;
      dst = z_slot(E, s.iter);
      if (uint64_t* t = zstore_tag_at(b->zst, e, s.iter)) *t = 0;  // (injected: not what any seed draws; store or ring slot)
      cap = (size_t)E.S * E.z_cols * 8;
      state_apply(b->st, StateEvent::write_normals);
      break;
    }
    case GPET_BUF_SAMPLES: {
      state_apply(b->st, StateEvent::write_samples);
      // (dense [S][Lg] f64 in, rows of Yp elements on the device; rounded to f32 here, as the GEMM does when it stores)
      const size_t cnt = (size_t)E.S * Lg, pitch = (size_t)E.Yp, esz = E.y_f32 ? 4 : 8, nel = bytes / 8;
      if (bytes > cnt * 8) return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_write: %zu bytes exceed capacity %zu", bytes, cnt * 8);
      const size_t full = nel / Lg, rest = nel % Lg;
      std::vector<char> tmp((full * pitch + rest) * esz, 0);
      const double* in = (const double*)src;
      for (size_t i = 0; i < nel; ++i) {
        const size_t at = (i / Lg) * pitch + i % Lg;
        if (E.y_f32) ((float*)tmp.data())[at] = (float)in[i];
        else ((double*)tmp.data())[at] = in[i];
      }
      if (!tmp.empty()) HIPCHK(c, hipMemcpyAsync(E.Y, tmp.data(), tmp.size(), hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, gpet_wait(c->stream));
      return GPET_OK;
    }
    case GPET_BUF_FIN_OUT: {
      // (dense [2][Lg] in; no state event: the batch goes on holding what the last converged fit left it holding)
      if (bytes != 2 * Lg * 8) return fail(c, GPET_ERR_BAD_ARG, "FIN_OUT write: expected %zu bytes", 2 * Lg * 8);
      HIPCHK(c, hipMemcpyAsync(E.fin_out, src, Lg * 8, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(E.fin_out + b->bd.Lg, (const char*)src + Lg * 8, Lg * 8, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, gpet_wait(c->stream));
      return GPET_OK;
    }
    case GPET_BUF_GRAD_KDE: dst = (void*)E.grad_kde; cap = px * 4; break;
    case GPET_BUF_KDE: dst = E.kde; cap = px * 4; break;
    case GPET_BUF_COSTS: dst = E.costs; cap = (size_t)E.S * 8; break;
    case GPET_BUF_BEST_IDX: dst = E.best_idx; cap = (size_t)E.n_keep * 4; state_apply(b->st, StateEvent::write_best_idx); break;
    case GPET_BUF_BEST_COSTS: dst = E.best_costs; cap = (size_t)E.n_keep * 8; break;
    case GPET_BUF_MEAN: dst = E.mean; cap = Lg * 8; break;
    case GPET_BUF_COV: dst = E.cov; cap = Lg * Lg * 8; state_apply(b->st, StateEvent::write_cov); break;
    case GPET_BUF_SCALARS: dst = E.sc; cap = sizeof(gpet_scalars); state_apply(b->st, StateEvent::write_scalars); break;
    default:
      return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_write: buffer %d is not writable", which);
  }
  if (bytes > cap) return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_write: %zu bytes exceed capacity %zu", bytes, cap);
  HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, gpet_wait(c->stream));
  return GPET_OK;
}

// the batch's own option table (a copy of the process-wide one taken at gpet_batch_create): returns like gpet_set_option
int gpet_batch_set_option(gpet_batch* b, const char* name, int value) {
  const int i = option_find(name);
  if (!b || i < 0) return -1;
  const int prev = option_set(&b->opts, i, value);
  return prev < 0 ? option_def(i).hi + 1 : prev;
}
int gpet_batch_get_option(const gpet_batch* b, const char* name, int* value) {
  const int i = option_find(name);
  if (!b || i < 0) return GPET_ERR_BAD_ARG;
  if (value) *value = option_get(&b->opts, i);
  return GPET_OK;
}

int gpet_batch_set_rng(gpet_batch* b, int mode) {
  GPET_BATCH_SCOPE(b);
  if (!b || (mode != 0 && mode != 1)) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gpet_wait(c->stream));
  if (b->side) HIPCHK(c, gpet_wait(b->side));
  b->rng_mode = mode;
  zstore_clear_tags(b->zst);  // (the store's and the ring's slots hold the other mode's numbers)
  state_apply(b->st, StateEvent::set_rng);
  return GPET_OK;
}

int gpet_batch_set_sample_dtype(gpet_batch* b, int f32) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gpet_wait(c->stream));
  if (b->side) HIPCHK(c, gpet_wait(b->side));
  const int v = f32 ? 1 : 0;
  for (int e = 0; e < b->B; ++e) b->h_edges[e].y_f32 = v;
  b->bd.y_f32 = v;
  b->bd.y_arith = GPET_SAMPLE_ARITH_F64;  // (no batch holds f64 storage with f32 arithmetic)
  HIPCHK(c, hipMemcpyAsync(b->d_edges, b->h_edges.data(), sizeof(EdgeDev) * (size_t)b->B, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, gpet_wait(c->stream));
  state_apply(b->st, StateEvent::set_sample_type);
  return GPET_OK;
}

int gpet_batch_set_sample_arith(gpet_batch* b, int arith) {
  GPET_BATCH_SCOPE(b);
  if (!b || (arith != GPET_SAMPLE_ARITH_F64 && arith != GPET_SAMPLE_ARITH_F32)) return GPET_ERR_BAD_ARG;
  if (arith == GPET_SAMPLE_ARITH_F32) {  // the storage goes with it
    const int rc = gpet_batch_set_sample_dtype(b, 1);
    if (rc != GPET_OK) return rc;
  }
  gpet_ctx* c = b->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gpet_wait(c->stream));
  if (b->side) HIPCHK(c, gpet_wait(b->side));
  b->bd.y_arith = arith;
  state_apply(b->st, StateEvent::set_sample_type);
  return GPET_OK;
}

int gpet_batch_clear_injected_factor(gpet_batch* b, int e) {
  GPET_BATCH_SCOPE(b);
  if (!b || e < 0 || e >= b->B) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  EdgeDev& E = b->h_edges[e];
  E.factor_injected = 0;
  HIPCHK(c, hipMemcpyAsync(b->d_edges + e, &E, sizeof E, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, gpet_wait(c->stream));
  return GPET_OK;
}

// ev: what restarts the batch (StateEvent::reset, StateEvent::images_swapped)
static int batch_reset(gpet_batch* b, bool next_frame, StateEvent ev) {
  gpet_ctx* c = b->ctx;
  state_apply(b->st, ev);
  b->h_nobs_prev.assign(b->B, 0);
  HIPCHK(c, hipSetDevice(c->device));
  if (b->bd.r_cap > 96) {  // (any-rank batches keep the last factor rows in a ring)
    if (next_frame && opt(Opt::oj_warm)) {  // where every edge's last rows are, before the iteration counters go
      int rc = fetch_all_scalars(b);
      if (rc) return rc;
      std::vector<int> iters((size_t)b->B);
      for (int e = 0; e < b->B; ++e) iters[e] = b->h_scalars[e].iter;
      rc = carry_factor_rows_all(b, iters);
      if (rc) return rc;
    } else {
      for (int e = 0; e < b->B; ++e) {
        int rc = clear_factor_rows(b, e);
        if (rc) return rc;
      }
    }
  }
  HIPCHK(c, upload_pristine_scalars(b));
  const int rc_h = history_clear(b, -1);
  if (rc_h) return rc_h;
  HIPCHK(c, gpet_wait(c->stream));
  return GPET_OK;
}

int gpet_batch_reset(gpet_batch* b) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  return batch_reset(b, false, StateEvent::reset);
}

// The orientation of a batch is decided at its creation: a vertical batch takes its frames in frame layout without the bit being
// repeated, and a set call that carries GPET_FRAMES_TRANSPOSED on a batch created without it is refused before anything is touched.
static int check_set_orientation(gpet_batch* b, unsigned int flags) {
  if ((flags & GPET_FRAMES_TRANSPOSED) && !b->transposed)
    return fail(b->ctx, GPET_ERR_BAD_ARG, "GPET_FRAMES_TRANSPOSED on a batch that was created without it: the orientation of a batch "
                                          "is decided at its creation");
  return GPET_OK;
}

// new images for an existing batch, whatever they come as (the one body of gpet_batch_set_images / gpet_batch_set_raw_images)
static int batch_set_images_from(gpet_batch* b, const ImageSource& src) {
  const unsigned int flags = src.flags;
  gpet_ctx* c = b->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gpet_wait(c->stream));
  int rc = load_images(b, src);
  if (rc) return rc;
  // gradient KDE of every distinct image (gpet.py:127), then the state of a fresh constructor
  rc = image_kde(b);
  if (rc) return rc;
  return batch_reset(b, (flags & GPET_IMAGES_NEXT_FRAME) != 0, StateEvent::images_swapped);
}

// raw frames: the orientation, then everything check_raw_source refuses, before the batch is touched
static int batch_set_raw_from(gpet_batch* b, const ImageSource& src) {
  const int rc_o = check_set_orientation(b, src.flags);
  if (rc_o) return rc_o;
  const int rc = check_batch_source(b->ctx, src, batch_source_count(b), b->transposed);
  if (rc) return rc;
  return batch_set_images_from(b, src);
}

int gpet_batch_set_images(gpet_batch* b, const float* const* grad, unsigned int flags) {
  GPET_BATCH_SCOPE(b);
  if (!b || !grad) return GPET_ERR_BAD_ARG;
  const int rc_o = check_set_orientation(b, flags);
  if (rc_o) return rc_o;
  return batch_set_images_from(b, ImageSource(grad, flags));
}

// (a refused call -- unknown pixel type, null frame, oversized kernel, a denoising spec that cannot run -- has touched nothing:
//  the batch traces on as it was)
int gpet_batch_set_raw_images_dn(gpet_batch* b, const void* const* raw, int pix, const double* kern, int kh, int kw,
                                 const gpet_denoise* dn, unsigned int flags) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  return batch_set_raw_from(b, ImageSource(raw, pix, kern, kh, kw, dn, flags));
}

// (refused as gpet_batch_set_raw_images_dn refuses, and for a table slot_table_check or the LDS bound refuses: nothing touched)
int gpet_batch_set_raw_images_multi(gpet_batch* b, int n_frames, const void* const* raw, int pix, int n_kern, const double* const* kern,
                                    const int32_t* kh, const int32_t* kw, const int32_t* frame_of, const int32_t* kernel_of,
                                    const gpet_denoise* dn, unsigned int flags) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  ImageSource src(raw, n_frames, pix, dn, flags);
  src.args.slot_table(n_kern, kern, kh, kw, batch_source_count(b), frame_of, kernel_of);
  return batch_set_raw_from(b, src);
}

int gpet_batch_set_raw_images(gpet_batch* b, const void* const* raw, int pix, const double* kern, int kh, int kw, unsigned int flags) {
  return gpet_batch_set_raw_images_dn(b, raw, pix, kern, kh, kw, nullptr, flags);
}

}  // extern "C"
