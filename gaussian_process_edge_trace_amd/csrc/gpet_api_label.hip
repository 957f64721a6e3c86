// C ABI: label maps (include/gpet_hip.h, "label maps") -- traces rasterised into uint8 masks on the device: rows at
// or below an edge, layers between stacked edges, the inside of closed outlines.  The rules, their refusals and the launch shapes:
// gpet_label_plan.h; the kernels: gpet_k_label.inc.  The stand-alone forms work on rows / vertices the caller gives; the batch forms read
// the converged fits where they lie (fin_out), as gpet_batch_results does, and touch nothing else of the batch.  The scratch -- tables,
// thresholds, vertices, the staging of maps that go to host memory -- is one allocation per context (stand-alone forms) or per batch,
// made on first use and grown on demand: a batch that never asks for a map holds and enqueues nothing for it.
#include "gpet_api_internal.h"

struct LabelScratch {
  char* mem = nullptr;
  size_t bytes = 0;
  std::vector<char> h_tab;   // what the tables of the last call were uploaded from
  hipEvent_t ev = nullptr;   // recorded behind that upload: once it has passed, h_tab may be rewritten
  bool ev_pending = false;
};

void label_free(LabelScratch*& s) {
  if (!s) return;
  if (s->mem) (void)hipFree(s->mem);
  if (s->ev) (void)hipEventDestroy(s->ev);
  delete s;
  s = nullptr;
}

// the scratch of `slot` with room for `bytes` on the device and its host tables free to be rewritten
static int label_scratch(gpet_ctx* c, LabelScratch** slot, size_t bytes, LabelScratch** out) {
  if (!*slot) {
    *slot = new (std::nothrow) LabelScratch();
    if (!*slot) return fail(c, GPET_ERR_BAD_ARG, "out of host memory");
  }
  LabelScratch* s = *slot;
  if (!s->ev) HIPCHK(c, hipEventCreateWithFlags(&s->ev, hipEventDisableTiming));
  if (s->ev_pending) {
    HIPCHK(c, hipEventSynchronize(s->ev));
    s->ev_pending = false;
  }
  if (bytes > s->bytes) {
    HIPCHK(c, gpet_wait(c->stream));  // (nothing enqueued may still use the old block)
    if (s->mem) (void)hipFree(s->mem);
    s->mem = nullptr;
    s->bytes = 0;
    HIPCHK(c, hipMalloc(&s->mem, bytes));
    s->bytes = bytes;
  }
  *out = s;
  return GPET_OK;
}

// What both rules share of a call: the members of every map in kernel order, where the maps go, and the way home of maps for the host.
struct LabelCall {
  gpet_ctx* c = nullptr;
  LabelScratch** slot = nullptr;
  int n_maps = 0, L = 0;
  long long map_bytes = 0;  // M * N
  unsigned int flags = 0;
  void* const* out = nullptr;
  std::vector<LabelEdge> le;        // the contributing edges, map after map
  std::vector<int32_t> map_off;     // [n_maps + 1] into le
  bool on_device() const { return (flags & LABELS_OUT_ON_DEVICE) != 0; }
  size_t stage_stride() const { return ((size_t)map_bytes + 15) & ~(size_t)15; }
  void members(int n, const int32_t* map_of) {
    std::vector<int32_t> used((size_t)n + 1);
    map_off.assign((size_t)n_maps + 1, 0);
    const int k = label_map_table(n, map_of, n_maps, used.data(), map_off.data());
    le.assign((size_t)k, LabelEdge{});
    for (int u = 0; u < k; ++u) le[u].edge = used[u];
    for (int f = 0; f < n_maps; ++f)
      for (int u = map_off[f]; u < map_off[f + 1]; ++u) le[u].map = f;
  }
  // out_off[f] of the kernels and the pointer they are relative to
  unsigned char* destinations(unsigned char* stage, long long* out_off) const {
    if (!on_device()) {
      for (int f = 0; f < n_maps; ++f) out_off[f] = (long long)((size_t)f * stage_stride());
      return stage;
    }
    unsigned char* const out0 = static_cast<unsigned char*>(out[0]);
    for (int f = 0; f < n_maps; ++f)
      out_off[f] = (long long)(reinterpret_cast<intptr_t>(out[f]) - reinterpret_cast<intptr_t>(out0));
    return out0;
  }
  // the staged maps into the host's out[] on the stream: one strided copy where the host's maps lie one behind the other
  int maps_home(const unsigned char* stage) const {
    bool packed = true;
    for (int f = 1; f < n_maps && packed; ++f)
      packed = static_cast<char*>(out[f]) == static_cast<char*>(out[0]) + (size_t)f * (size_t)map_bytes;
    if (packed) {
      HIPCHK(c, hipMemcpy2DAsync(out[0], (size_t)map_bytes, stage, stage_stride(), (size_t)map_bytes, (size_t)n_maps, hipMemcpyDeviceToHost,
                                 c->stream));
      return GPET_OK;
    }
    for (int f = 0; f < n_maps; ++f)
      HIPCHK(c, hipMemcpyAsync(out[f], stage + (size_t)f * stage_stride(), (size_t)map_bytes, hipMemcpyDeviceToHost, c->stream));
    return GPET_OK;
  }
};

// Rule 1 with the members of `k` filled in (x_st, len and the source of the rows): tables up, thresholds, maps, thick, maps home.
// rows / n_rows: the stand-alone form's int64 rows; b: the batch of the batch form (else nullptr)
static int run_rows(LabelCall& k, int M, int N, const int64_t* rows, size_t n_rows, gpet_batch* b, int32_t* thick) {
  gpet_ctx* c = k.c;
  const int n_used = (int)k.le.size(), n_maps = k.n_maps;
  const bool dev = k.on_device();
  const size_t n_thick = thick ? (size_t)label_thick_count(n_maps, k.L, N) : 0;
  HIPCHK(c, hipSetDevice(c->device));
  LabelEdge* t_le = nullptr;
  int32_t* t_off = nullptr;
  long long *t_out = nullptr, *t_rows = nullptr;
  int *d_T = nullptr, *d_thick = nullptr;
  unsigned char* d_stage = nullptr;
  size_t tab_bytes = 0;
  LabelScratch* s = nullptr;
  for (int pass = 0; pass < 3; ++pass) {  // measure; the host image of the tables; the device block
    Carver cv;
    cv.base = pass == 0 ? nullptr : (pass == 1 ? s->h_tab.data() : s->mem);
    t_le = cv.take<LabelEdge>((size_t)n_used);
    t_off = cv.take<int32_t>((size_t)n_maps + 1);
    t_out = cv.take<long long>((size_t)n_maps);
    t_rows = cv.take<long long>(n_rows + 1);
    tab_bytes = cv.off;
    d_T = cv.take<int>((size_t)n_used * (size_t)N);
    d_stage = cv.take<unsigned char>(dev ? 0 : (size_t)n_maps * k.stage_stride());
    d_thick = cv.take<int>(dev ? 0 : n_thick);
    if (pass == 0) {
      const int rc = label_scratch(c, k.slot, cv.off + 256, &s);
      if (rc) return rc;
      s->h_tab.assign(tab_bytes, 0);
    } else if (pass == 1) {
      std::copy(k.le.begin(), k.le.end(), t_le);
      std::copy(k.map_off.begin(), k.map_off.end(), t_off);
      if (n_rows) memcpy(t_rows, rows, sizeof(int64_t) * n_rows);
    }
  }
  // (after pass 2 the pointers are the device's; the destinations are written into the host image at the same offsets)
  long long* h_out = reinterpret_cast<long long*>(s->h_tab.data() + (reinterpret_cast<char*>(t_out) - s->mem));
  unsigned char* const d_out0 = k.destinations(d_stage, h_out);
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(s->mem, s->h_tab.data(), tab_bytes, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipEventRecord(s->ev, st));
  s->ev_pending = true;
  HIPCHK(c, launch_label_thresholds(st, t_le, n_used, t_rows, b ? b->d_edges : nullptr, b && b->band.H ? b->band.fit : nullptr, M, N,
                                    (k.flags & LABELS_EXTEND) != 0, d_T));
  HIPCHK(c, launch_label_fill(st, d_T, t_off, n_maps, k.L, d_out0, t_out, M, N, (k.flags & LABELS_TRANSPOSED) != 0));
  if (thick) HIPCHK(c, launch_label_thick(st, d_T, t_off, n_maps, M, N, k.L, dev ? thick : d_thick));
  if (dev) return GPET_OK;
  const int rc = k.maps_home(d_stage);
  if (rc) return rc;
  if (thick) HIPCHK(c, hipMemcpyAsync(thick, d_thick, sizeof(int) * n_thick, hipMemcpyDeviceToHost, st));
  HIPCHK(c, gpet_wait(st));
  return GPET_OK;
}

// Rule 2 with the members of `k` filled in.  Stand-alone form: xy / vert_off / n_vert of the contributing contours (host).  Batch form
// (b, polar): the vertices are made on the device, n_theta each.
static int run_outlines(LabelCall& k, int Ms, int Ns, const double* xy, const std::vector<long long>& vert_off, const std::vector<int32_t>& n_vert,
                        size_t n_pairs, gpet_batch* b, const gpet_polar* polar) {
  gpet_ctx* c = k.c;
  const int n_used = (int)k.le.size(), n_maps = k.n_maps;
  const bool dev = k.on_device();
  const int n_theta = polar ? polar->n_theta : 0, n_c = polar ? polar->n_centres : 0;
  int n_max = 0;
  for (int32_t n : n_vert) n_max = std::max(n_max, (int)n);
  HIPCHK(c, hipSetDevice(c->device));
  LabelEdge* t_le = nullptr;
  int32_t *t_off = nullptr, *t_nv = nullptr;
  long long *t_out = nullptr, *t_voff = nullptr;
  double *t_xy = nullptr, *t_cxy = nullptr, *t_cos = nullptr, *t_sin = nullptr, *d_xy = nullptr;
  unsigned char* d_stage = nullptr;
  size_t tab_bytes = 0;
  LabelScratch* s = nullptr;
  for (int pass = 0; pass < 3; ++pass) {
    Carver cv;
    cv.base = pass == 0 ? nullptr : (pass == 1 ? s->h_tab.data() : s->mem);
    t_le = cv.take<LabelEdge>((size_t)n_used);
    t_off = cv.take<int32_t>((size_t)n_maps + 1);
    t_nv = cv.take<int32_t>((size_t)n_used);
    t_out = cv.take<long long>((size_t)n_maps);
    t_voff = cv.take<long long>((size_t)n_used);
    t_xy = cv.take<double>(polar ? 0 : 2 * n_pairs);
    t_cxy = cv.take<double>(2 * (size_t)n_c);
    t_cos = cv.take<double>((size_t)n_theta);
    t_sin = cv.take<double>((size_t)n_theta);
    tab_bytes = cv.off;
    d_xy = cv.take<double>(polar ? 2 * n_pairs : 0);
    d_stage = cv.take<unsigned char>(dev ? 0 : (size_t)n_maps * k.stage_stride());
    if (pass == 0) {
      const int rc = label_scratch(c, k.slot, cv.off + 256, &s);
      if (rc) return rc;
      s->h_tab.assign(tab_bytes, 0);
    } else if (pass == 1) {
      std::copy(k.le.begin(), k.le.end(), t_le);
      std::copy(k.map_off.begin(), k.map_off.end(), t_off);
      std::copy(n_vert.begin(), n_vert.end(), t_nv);
      std::copy(vert_off.begin(), vert_off.end(), t_voff);
      if (!polar) {
        memcpy(t_xy, xy, 2 * sizeof(double) * n_pairs);
      } else {
        memcpy(t_cxy, polar->cx, sizeof(double) * (size_t)n_c);
        memcpy(t_cxy + n_c, polar->cy, sizeof(double) * (size_t)n_c);
        memcpy(t_cos, polar->cos_t, sizeof(double) * (size_t)n_theta);
        memcpy(t_sin, polar->sin_t, sizeof(double) * (size_t)n_theta);
      }
    }
  }
  long long* h_out = reinterpret_cast<long long*>(s->h_tab.data() + (reinterpret_cast<char*>(t_out) - s->mem));
  unsigned char* const d_out0 = k.destinations(d_stage, h_out);
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(s->mem, s->h_tab.data(), tab_bytes, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipEventRecord(s->ev, st));
  s->ev_pending = true;
  if (polar)
    HIPCHK(c, launch_label_vertices(st, t_le, n_used, b->d_edges, b->band.H ? b->band.fit : nullptr, t_cxy, n_c, t_cos, t_sin, polar->r0,
                                    polar->dr, n_theta, d_xy));
  HIPCHK(c, launch_label_fill_xy(st, polar ? d_xy : t_xy, t_voff, t_nv, t_off, n_maps, n_max, d_out0, t_out, Ms, Ns));
  if (dev) return GPET_OK;
  const int rc = k.maps_home(d_stage);
  if (rc) return rc;
  HIPCHK(c, gpet_wait(st));
  return GPET_OK;
}

static int check_flags(gpet_ctx* c, unsigned int flags) {
  if (flags & ~(LABELS_EXTEND | LABELS_TRANSPOSED | LABELS_OUT_ON_DEVICE)) return fail(c, GPET_ERR_BAD_ARG, "label maps: unknown flag bits 0x%x", flags);
  return GPET_OK;
}

// the state gpet_batch_results asks for, in its words
static int check_fit(gpet_batch* b, const char* who) {
  if (state_missing(b->st, StateEvent::read_results))
    return fail(b->ctx, GPET_ERR_BAD_ARG, "%s: no converged fit of the current trace (run gpet_final_fit_all first)", who);
  return GPET_OK;
}

extern "C" {

int gpet_label_thick_count(int n_maps, int L, int N, int64_t* count) {
  if (!count) return GPET_ERR_BAD_ARG;
  const long long n = label_thick_count(n_maps, L, N);
  if (n == 0) return GPET_ERR_BAD_ARG;
  *count = n;
  return GPET_OK;
}

int gpet_label_maps(gpet_ctx* c, int M, int N, int n_edges, const int32_t* x_st, const int32_t* len, const int64_t* rows, const int32_t* map_of,
                    int n_maps, unsigned int flags, void* const* out, int32_t* thick) {
  if (!c) return GPET_ERR_BAD_ARG;
  if (check_flags(c, flags)) return GPET_ERR_BAD_ARG;
  char msg[256];
  LabelCall k;
  bool out_null = !out;
  for (int f = 0; out && f < n_maps; ++f) out_null = out_null || !out[f];
  if (label_check(M, N, n_edges, x_st, len, !rows, map_of, n_maps, out_null, &k.L, msg, sizeof msg)) return fail(c, GPET_ERR_BAD_ARG, "%s", msg);
  k.c = c;
  k.slot = &c->lab;
  k.n_maps = n_maps;
  k.map_bytes = (long long)M * (long long)N;
  k.flags = flags;
  k.out = out;
  k.members(n_edges, map_of);
  std::vector<long long> row_off((size_t)n_edges + 1, 0);
  for (int e = 0; e < n_edges; ++e) row_off[(size_t)e + 1] = row_off[e] + len[e];
  for (LabelEdge& E : k.le) {
    const int e = E.edge;
    E.x_st = x_st[e];
    E.len = len[e];
    E.row_off = row_off[e];
    E.edge = -1;  // (the rows are the caller's)
  }
  return run_rows(k, M, N, rows, (size_t)row_off[n_edges], nullptr, thick);
}

int gpet_label_maps_xy(gpet_ctx* c, int Ms, int Ns, int n_contours, const int32_t* n_vert, const double* xy, const int32_t* map_of, int n_maps,
                       unsigned int flags, void* const* out) {
  if (!c) return GPET_ERR_BAD_ARG;
  if (check_flags(c, flags)) return GPET_ERR_BAD_ARG;
  char msg[256];
  LabelCall k;
  bool out_null = !out;
  for (int f = 0; out && f < n_maps; ++f) out_null = out_null || !out[f];
  if (label_check_xy(Ms, Ns, n_contours, n_vert, !xy, map_of, n_maps, out_null, &k.L, msg, sizeof msg))
    return fail(c, GPET_ERR_BAD_ARG, "%s", msg);
  k.c = c;
  k.slot = &c->lab;
  k.n_maps = n_maps;
  k.map_bytes = (long long)Ms * (long long)Ns;
  k.flags = flags;
  k.out = out;
  k.members(n_contours, map_of);
  std::vector<long long> off((size_t)n_contours + 1, 0);
  for (int e = 0; e < n_contours; ++e) off[(size_t)e + 1] = off[e] + n_vert[e];
  std::vector<long long> vert_off;
  std::vector<int32_t> nv;
  for (const LabelEdge& E : k.le) {
    vert_off.push_back(off[E.edge]);
    nv.push_back(n_vert[E.edge]);
  }
  return run_outlines(k, Ms, Ns, xy, vert_off, nv, (size_t)off[n_contours], nullptr, nullptr);
}

int gpet_batch_label_maps(gpet_batch* b, const int32_t* map_of, int n_maps, unsigned int flags, void* const* out, int32_t* thick) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  int rc = check_fit(b, "gpet_batch_label_maps");
  if (rc) return rc;
  if (check_flags(c, flags)) return GPET_ERR_BAD_ARG;
  const int B = b->B, M = b->band.H ? b->band.M : b->bd.M, N = b->bd.N;
  std::vector<int32_t> x_st((size_t)B), len((size_t)B);
  for (int e = 0; e < B; ++e) {
    x_st[e] = b->h_edges[e].x_st;
    len[e] = b->h_edges[e].Lg;
  }
  char msg[256];
  LabelCall k;
  bool out_null = !out;
  for (int f = 0; out && f < n_maps; ++f) out_null = out_null || !out[f];
  if (label_check(M, N, B, x_st.data(), len.data(), false, map_of, n_maps, out_null, &k.L, msg, sizeof msg))
    return fail(c, GPET_ERR_BAD_ARG, "%s", msg);
  k.c = c;
  k.slot = &b->lab;
  k.n_maps = n_maps;
  k.map_bytes = (long long)M * (long long)N;
  k.flags = flags;
  k.out = out;
  k.members(B, map_of);
  for (LabelEdge& E : k.le) {
    E.x_st = x_st[E.edge];
    E.len = len[E.edge];
  }
  return run_rows(k, M, N, nullptr, 0, b, thick);
}

int gpet_batch_label_maps_xy(gpet_batch* b, const gpet_polar* polar, int Ms, int Ns, const int32_t* map_of, int n_maps, unsigned int flags,
                             void* const* out) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  int rc = check_fit(b, "gpet_batch_label_maps_xy");
  if (rc) return rc;
  if (check_flags(c, flags)) return GPET_ERR_BAD_ARG;
  const int B = b->B;
  char msg[256];
  LabelCall k;
  bool out_null = !out;
  for (int f = 0; out && f < n_maps; ++f) out_null = out_null || !out[f];
  const bool polar_null = !polar || !polar->cx || !polar->cy || !polar->cos_t || !polar->sin_t;
  if (label_check_maps(polar_null || out_null, Ms, Ns, B, map_of, n_maps, "edge", &k.L, msg, sizeof msg)) return fail(c, GPET_ERR_BAD_ARG, "%s", msg);
  if (polar->n_theta < LABEL_VERTS_MIN || polar->n_theta > LABEL_VERTS_MAX)
    return fail(c, GPET_ERR_BAD_ARG, "label maps: contour %d has %d vertices, outside [4, 4096]", 0, (int)polar->n_theta);
  if (polar->n_centres != 1 && polar->n_centres != n_maps)
    return fail(c, GPET_ERR_BAD_ARG, "label maps: one centre for all maps or one per map (n_centres = %d, n_maps = %d)", (int)polar->n_centres, n_maps);
  k.c = c;
  k.slot = &b->lab;
  k.n_maps = n_maps;
  k.map_bytes = (long long)Ms * (long long)Ns;
  k.flags = flags;
  k.out = out;
  k.members(B, map_of);
  std::vector<long long> vert_off;
  std::vector<int32_t> nv;
  for (LabelEdge& E : k.le) {
    const EdgeDev& H = b->h_edges[E.edge];
    if (label_check_closed(E.edge, H.x_st, H.x_en, polar->pad, polar->n_theta, msg, sizeof msg)) return fail(c, GPET_ERR_BAD_ARG, "%s", msg);
    E.x_st = H.x_st;
    E.len = H.Lg;
    vert_off.push_back((long long)vert_off.size() * polar->n_theta);
    nv.push_back(polar->n_theta);
  }
  return run_outlines(k, Ms, Ns, nullptr, vert_off, nv, k.le.size() * (size_t)polar->n_theta, b, polar);
}

}  // extern "C"
