// C ABI: seed ensembles (include/gpet_hip.h, "seed ensembles") -- the final cost of every edge's converged mean and the per-column
// consensus over the traces of one edge, computed where the converged fits lie (fin_out).  Kernels: gpet_k_ensemble.inc; layout,
// validation and tiling: gpet_ensemble_plan.h.  Neither call touches the loop's state or the batch arena: their scratch is made on
// first use, and a batch that never calls them allocates and enqueues nothing for them.
#include "gpet_api_internal.h"

struct EnsembleScratch {
  // final costs: the one-row views of the scorer (launch_final_costs); sized by the batch's dimensions, so made once
  char* fc_mem = nullptr;
  EdgeDev* view = nullptr;
  gpet_scalars* view_sc = nullptr;
  double *rows = nullptr, *part = nullptr, *cost = nullptr;
  size_t row_stride = 0;
  // the reduction: the plan's tables on the device with their host copies (kept alive for the asynchronous copies), off per edge,
  // and the staging of a result that goes to host memory; grown on demand
  gpet::EnsemblePlan plan;
  char* tab_mem = nullptr;
  size_t tab_bytes = 0;
  int* off_acc = nullptr;
  char* stage = nullptr;
  size_t stage_bytes = 0;
  // the kept ensemble (gpet_batch_ensemble_keep; layout: gpet_warm_plan.h): the buffer of gpet_batch_ensemble for len_cap = the widest
  // edge with the group table behind it, valid while the batch's state says so (ST_ENS_KEPT); the host's copy of the table (kept alive for its copy)
  char* kept = nullptr;
  size_t kept_bytes = 0;
  int kept_G = 0;
  int64_t kept_len_cap = 0;
  std::vector<int32_t> kept_group_of;
  // the source of every edge's warm start (gpet_batch_warm_start_groups / _from): device [B], and where it is read back to
  int32_t* src = nullptr;
  std::vector<int32_t> h_src;
};

void ensemble_free(gpet_batch* b) {
  if (!b || !b->ens) return;
  EnsembleScratch* s = b->ens;
  if (s->fc_mem) (void)hipFree(s->fc_mem);
  if (s->tab_mem) (void)hipFree(s->tab_mem);
  if (s->off_acc) (void)hipFree(s->off_acc);
  if (s->stage) (void)hipFree(s->stage);
  if (s->kept) (void)hipFree(s->kept);
  if (s->src) (void)hipFree(s->src);
  delete s;
  b->ens = nullptr;
}

// the state gpet_batch_results asks for, with its status
static int check_fit(gpet_batch* b, const char* who) {
  if (state_missing(b->st, StateEvent::read_results))
    return fail(b->ctx, GPET_ERR_BAD_ARG, "%s: no converged fit of the current trace (run gpet_final_fit_all first)", who);
  return GPET_OK;
}

// a kept ensemble can be read: the state says it is valid, and the allocation it would be in exists
static bool ensemble_is_kept(const gpet_batch* b) {
  return !state_missing(b->st, StateEvent::read_kept_ensemble) && b->ens && b->ens->kept;
}

static int scratch(gpet_batch* b, EnsembleScratch** out) {
  if (!b->ens) {
    b->ens = new (std::nothrow) EnsembleScratch();
    if (!b->ens) return fail(b->ctx, GPET_ERR_BAD_ARG, "out of host memory");
  }
  *out = b->ens;
  return GPET_OK;
}

// cost[e] of every edge into s->cost on the context's stream (no wait)
static int enqueue_final_costs(gpet_batch* b, EnsembleScratch* s) {
  gpet_ctx* c = b->ctx;
  const int B = b->B;
  if (!s->fc_mem) {
    int pitch = 0;
    for (const EdgeDev& E : b->h_edges) pitch = std::max(pitch, E.Yp);
    s->row_stride = (size_t)((pitch + 15) & ~15);
    for (int pass = 0; pass < 2; ++pass) {
      Carver cv;
      cv.base = pass ? s->fc_mem : nullptr;
      s->view = cv.take<EdgeDev>((size_t)B);
      s->view_sc = cv.take<gpet_scalars>((size_t)B);
      s->rows = cv.take<double>((size_t)B * s->row_stride);
      s->part = cv.take<double>((size_t)B * fincost_part_stride(b->bd));
      s->cost = cv.take<double>((size_t)B);
      if (!pass) HIPCHK(c, hipMalloc(&s->fc_mem, cv.off + 256));
    }
  }
  HIPCHK(c, launch_final_costs(c->stream, b->d_edges, B, b->bd, s->view, s->view_sc, s->rows, s->row_stride, s->part, s->cost));
  return GPET_OK;
}

// The reduction of gpet_batch_ensemble into device memory on the context's stream (no wait after the launches).  d_dst == nullptr:
// into the staging buffer of a host destination, else into *d_dst_io; either way *d_dst_io is where the result lies.
static int enqueue_ensemble(gpet_batch* b, int n_groups, const int32_t* group_of, double tol, int64_t len_cap, char** d_dst_io,
                            EnsembleLayout* L_out) {
  gpet_ctx* c = b->ctx;
  const int B = b->B;
  const bool dst_on_device = *d_dst_io != nullptr;
  void* const dst = *d_dst_io;
  int rc = check_fit(b, "gpet_batch_ensemble");
  if (rc) return rc;
  int widest = 0;
  for (const EdgeDev& E : b->h_edges) widest = std::max(widest, E.Lg);
  const EnsembleLayout L = ensemble_layout(n_groups, B, len_cap);
  if (n_groups >= 1 && (L.total_bytes == 0 || len_cap < widest))
    return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_ensemble: len_cap=%lld is below the widest edge (%d points) or out of range", (long long)len_cap,
                widest);
  HIPCHK(c, hipSetDevice(c->device));
  rc = fetch_all_scalars(b);  // (which edges are excluded decides the members, the tile widths and the grid)
  if (rc) return rc;
  EnsembleScratch* s = nullptr;
  rc = scratch(b, &s);
  if (rc) return rc;
  {
    std::vector<int32_t> x_st((size_t)B), x_en((size_t)B), status((size_t)B);
    for (int e = 0; e < B; ++e) {
      x_st[e] = b->h_edges[e].x_st;
      x_en[e] = b->h_edges[e].x_en;
      status[e] = b->h_scalars[e].status;
    }
    char msg[256];
    HIPCHK(c, gpet_wait(c->stream));  // (the plan's host tables may still feed the copies of the call before)
    rc = ensemble_plan(n_groups, B, group_of, x_st.data(), x_en.data(), status.data(), tol, &s->plan, msg, sizeof msg);
    if (rc) return fail(c, rc, "%s", msg);
  }
  const EnsemblePlan& P = s->plan;
  const int G = n_groups, n_wg = (int)P.wg_group.size();
  // the tables on the device, one allocation: groups | members | member_group | wg_group | wg_tile
  EnsembleGroup* d_groups = nullptr;
  int32_t *d_members = nullptr, *d_member_group = nullptr, *d_wg_group = nullptr, *d_wg_tile = nullptr;
  for (int pass = 0; pass < 2; ++pass) {
    Carver cv;
    cv.base = pass ? s->tab_mem : nullptr;
    d_groups = cv.take<EnsembleGroup>((size_t)G);
    d_members = cv.take<int32_t>(P.members.size() + 1);
    d_member_group = cv.take<int32_t>((size_t)B);
    d_wg_group = cv.take<int32_t>((size_t)n_wg + 1);
    d_wg_tile = cv.take<int32_t>((size_t)n_wg + 1);
    if (!pass && cv.off + 256 > s->tab_bytes) {
      if (s->tab_mem) (void)hipFree(s->tab_mem);
      s->tab_mem = nullptr;
      s->tab_bytes = 0;
      HIPCHK(c, hipMalloc(&s->tab_mem, cv.off + 256));
      s->tab_bytes = cv.off + 256;
    }
  }
  if (!s->off_acc) HIPCHK(c, hipMalloc(&s->off_acc, sizeof(int) * (size_t)B));
  char* d_dst = static_cast<char*>(dst);
  if (!dst_on_device) {
    if ((size_t)L.total_bytes > s->stage_bytes) {
      if (s->stage) (void)hipFree(s->stage);
      s->stage = nullptr;
      s->stage_bytes = 0;
      HIPCHK(c, hipMalloc(&s->stage, (size_t)L.total_bytes));
      s->stage_bytes = (size_t)L.total_bytes;
    }
    d_dst = s->stage;
  }
  hipStream_t st = c->stream;
  HIPCHK(c, hipMemcpyAsync(d_groups, P.groups.data(), sizeof(EnsembleGroup) * (size_t)G, hipMemcpyHostToDevice, st));
  if (!P.members.empty())
    HIPCHK(c, hipMemcpyAsync(d_members, P.members.data(), sizeof(int32_t) * P.members.size(), hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(d_member_group, P.member_group.data(), sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, st));
  if (n_wg > 0) {
    HIPCHK(c, hipMemcpyAsync(d_wg_group, P.wg_group.data(), sizeof(int32_t) * (size_t)n_wg, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_wg_tile, P.wg_tile.data(), sizeof(int32_t) * (size_t)n_wg, hipMemcpyHostToDevice, st));
  }
  rc = enqueue_final_costs(b, s);
  if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(d_dst, 0, (size_t)L.total_bytes, st));  // (entries past a group's edge_len, groups without members)
  HIPCHK(c, hipMemsetAsync(s->off_acc, 0, sizeof(int) * (size_t)B, st));
  if (P.lds_bytes > (size_t)ENSEMBLE_LDS_BUDGET)
    return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_ensemble: a tile of %zu bytes exceeds the LDS budget", P.lds_bytes);
  HIPCHK(c, launch_ensemble(st, b->d_edges, B, G, d_groups, d_members, d_member_group, d_wg_group, d_wg_tile, n_wg, P.lds_bytes, tol,
                            (long long)len_cap, L, s->cost, s->off_acc, d_dst));
  *d_dst_io = d_dst;
  *L_out = L;
  return GPET_OK;
}

extern "C" {

int gpet_batch_final_costs(gpet_batch* b, double* dst, int dst_on_device) {
  GPET_BATCH_SCOPE(b);
  if (!b || !dst) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  int rc = check_fit(b, "gpet_batch_final_costs");
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  EnsembleScratch* s = nullptr;
  rc = scratch(b, &s);
  if (rc) return rc;
  rc = enqueue_final_costs(b, s);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(dst, s->cost, sizeof(double) * (size_t)b->B, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                           c->stream));
  if (!dst_on_device) HIPCHK(c, gpet_wait(c->stream));
  return GPET_OK;
}

int gpet_ensemble_bytes(int n_groups, int n_edges, int64_t len_cap, size_t* bytes) {
  if (!bytes) return GPET_ERR_BAD_ARG;
  const EnsembleLayout L = ensemble_layout(n_groups, n_edges, len_cap);
  if (L.total_bytes == 0) return GPET_ERR_BAD_ARG;
  *bytes = (size_t)L.total_bytes;
  return GPET_OK;
}


int gpet_batch_ensemble(gpet_batch* b, int n_groups, const int32_t* group_of, double tol, int64_t len_cap, void* dst, int dst_on_device) {
  GPET_BATCH_SCOPE(b);
  if (!b || !dst || !group_of) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  char* d_dst = dst_on_device ? static_cast<char*>(dst) : nullptr;
  EnsembleLayout L;
  const int rc = enqueue_ensemble(b, n_groups, group_of, tol, len_cap, &d_dst, &L);
  if (rc) return rc;
  if (!dst_on_device) {
    HIPCHK(c, hipMemcpyAsync(dst, d_dst, (size_t)L.total_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, gpet_wait(c->stream));
  }
  return GPET_OK;
}

// ---- seed ensembles in sequences (include/gpet_hip.h; sources and refusals: gpet_warm_plan.h; kernels: gpet_k_warm.inc) ---------
// The reduction into the batch's own allocation, with the group table behind it.  Before the swap: the final costs are scored on the
// images the edges read NOW.
int gpet_batch_ensemble_keep(gpet_batch* b, int n_groups, const int32_t* group_of, double tol) {
  GPET_BATCH_SCOPE(b);
  if (!b || !group_of) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  const int B = b->B;
  state_apply(b->st, StateEvent::ensemble_keep_begin);
  int rc = check_fit(b, "gpet_batch_ensemble_keep");
  if (rc) return rc;
  int widest = 0;
  for (const EdgeDev& E : b->h_edges) widest = std::max(widest, E.Lg);
  const int64_t bytes = warm_kept_bytes(n_groups, B, widest);
  if (bytes == 0) return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_ensemble_keep: bad argument (n_groups=%d, edges=%d)", n_groups, B);
  HIPCHK(c, hipSetDevice(c->device));
  EnsembleScratch* s = nullptr;
  rc = scratch(b, &s);
  if (rc) return rc;
  if ((size_t)bytes > s->kept_bytes) {
    HIPCHK(c, gpet_wait(c->stream));  // (nothing enqueued may still read the old one)
    if (s->kept) (void)hipFree(s->kept);
    s->kept = nullptr;
    s->kept_bytes = 0;
    HIPCHK(c, hipMalloc(&s->kept, (size_t)bytes));
    s->kept_bytes = (size_t)bytes;
  }
  char* d_dst = s->kept;
  EnsembleLayout L;
  rc = enqueue_ensemble(b, n_groups, group_of, tol, widest, &d_dst, &L);  // (waits for the stream before it plans: kept_group_of is free)
  if (rc) return rc;
  s->kept_group_of.assign(group_of, group_of + B);
  HIPCHK(c, hipMemcpyAsync(s->kept + warm_kept_group_off(n_groups, B, widest), s->kept_group_of.data(), sizeof(int32_t) * (size_t)B,
                           hipMemcpyHostToDevice, c->stream));
  s->kept_G = n_groups;
  s->kept_len_cap = widest;
  state_apply(b->st, StateEvent::ensemble_keep_end);
  return GPET_OK;
}

int gpet_batch_ensemble_kept(gpet_batch* b, int64_t len_cap, void* dst, int dst_on_device) {
  GPET_BATCH_SCOPE(b);
  if (!b || !dst) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  const int B = b->B;
  EnsembleScratch* const s = b->ens;
  if (!ensemble_is_kept(b))
    return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_ensemble_kept: no ensemble is kept (gpet_batch_ensemble_keep makes one; a warm start, "
                                     "gpet_batch_set_obs, gpet_batch_reset or another gpet_final_fit_all drop it)");
  const int G = s->kept_G;
  const int64_t kl = s->kept_len_cap;
  const EnsembleLayout K = ensemble_layout(G, B, kl), L = ensemble_layout(G, B, len_cap);
  if (L.total_bytes == 0 || len_cap < kl)
    return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_ensemble_kept: len_cap=%lld is below the widest edge (%lld points) or out of range",
                (long long)len_cap, (long long)kl);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const hipMemcpyKind kind = dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (len_cap == kl) {
    HIPCHK(c, hipMemcpyAsync(dst, s->kept, (size_t)K.total_bytes, kind, st));
  } else {  // a wider layout: section by section, zero between them as gpet_batch_ensemble leaves it
    char* const out = static_cast<char*>(dst);
    if (dst_on_device) HIPCHK(c, hipMemsetAsync(out, 0, (size_t)L.total_bytes, st));
    else memset(out, 0, (size_t)L.total_bytes);
    const int64_t from[8] = {0, K.off_trace, K.off_median, K.off_q_lo, K.off_q_hi, K.off_min, K.off_max, K.off_agree};
    const int64_t to[8] = {0, L.off_trace, L.off_median, L.off_q_lo, L.off_q_hi, L.off_min, L.off_max, L.off_agree};
    const int64_t len[8] = {(int64_t)sizeof(gpet_ensemble_head), kl * 16, kl * 8, kl * 8, kl * 8, kl * 8, kl * 8, kl * 4};
    for (int g = 0; g < G; ++g)
      for (int i = 0; i < 8; ++i)
        HIPCHK(c, hipMemcpyAsync(out + (size_t)g * (size_t)L.record_bytes + to[i], s->kept + (size_t)g * (size_t)K.record_bytes + from[i],
                                 (size_t)len[i], kind, st));
    HIPCHK(c, hipMemcpyAsync(out + L.off_cost, s->kept + K.off_cost, sizeof(double) * (size_t)B, kind, st));
    HIPCHK(c, hipMemcpyAsync(out + L.off_off, s->kept + K.off_off, sizeof(int32_t) * (size_t)B, kind, st));
  }
  if (!dst_on_device) HIPCHK(c, gpet_wait(st));
  return GPET_OK;
}

// the one body of the two calls: src_of == nullptr -- the group form
static int warm_start_sourced(gpet_batch* b, int from, const int32_t* src_of, int warm_every, int32_t* n_obs_out, int32_t* src_out) {
  gpet_ctx* c = b->ctx;
  const int B = b->B;
  const int ready = gpet_batch_warm_start_ready(b);
  if (ready) return ready;
  char msg[384];
  if (!src_of) {
    const int rc = warm_groups_check(from, ensemble_is_kept(b), msg, sizeof msg);
    if (rc) return fail(c, rc, "%s", msg);
  } else {
    std::vector<int32_t> x_st((size_t)B), x_en((size_t)B);
    for (int e = 0; e < B; ++e) {
      x_st[e] = b->h_edges[e].x_st;
      x_en[e] = b->h_edges[e].x_en;
    }
    const int rc = warm_from_check(B, src_of, x_st.data(), x_en.data(), msg, sizeof msg);
    if (rc) return fail(c, rc, "%s", msg);
  }
  HIPCHK(c, hipSetDevice(c->device));
  EnsembleScratch* s = nullptr;
  int rc = scratch(b, &s);
  if (rc) return rc;
  if (!s->src) HIPCHK(c, hipMalloc(&s->src, sizeof(int32_t) * (size_t)B));
  hipStream_t st = c->stream;
  s->h_src.resize((size_t)B);  // (every call that used it has waited for its copy)
  if (src_of) {
    std::copy(src_of, src_of + B, s->h_src.begin());
    HIPCHK(c, hipMemcpyAsync(s->src, s->h_src.data(), sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, st));
    if (b->band.H) HIPCHK(c, launch_warm_start_band(st, b->d_edges, B, s->src, nullptr, nullptr, 0, 0, warm_every, b->band.fit, b->band.r0));
    else HIPCHK(c, launch_warm_start_src(st, b->d_edges, B, s->src, nullptr, nullptr, 0, 0, warm_every));
  } else {
    const EnsembleLayout K = ensemble_layout(s->kept_G, B, s->kept_len_cap);
    const int32_t* d_group_of = reinterpret_cast<const int32_t*>(s->kept + warm_kept_group_off(s->kept_G, B, s->kept_len_cap));
    // the sources from the records' heads on the stream: the host does not wait for them, it reads them with the scalars below
    HIPCHK(c, launch_warm_sources(st, B, d_group_of, s->kept, (long long)K.record_bytes, from, s->src));
    if (b->band.H)
      HIPCHK(c, launch_warm_start_band(st, b->d_edges, B, s->src, d_group_of, s->kept, (long long)K.record_bytes, (long long)K.off_trace,
                                       warm_every, b->band.fit, b->band.r0));
    else
      HIPCHK(c, launch_warm_start_src(st, b->d_edges, B, s->src, d_group_of, s->kept, (long long)K.record_bytes, (long long)K.off_trace,
                                      warm_every));
    if (src_out) HIPCHK(c, hipMemcpyAsync(s->h_src.data(), s->src, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, st));
  }
  rc = warm_start_finish(b, n_obs_out);  // (the one copy of the scalars and the one wait, as gpet_batch_warm_start; drops the kept ensemble)
  if (rc) return rc;
  if (src_out) std::copy(s->h_src.begin(), s->h_src.end(), src_out);
  return GPET_OK;
}

// Placement of every edge's band for the next frame (k_band_place, the rule of band_place), enqueued: the refusals are those of the warm
// start that will follow with the same sources, checked the same way, and nothing is touched when one applies.
int gpet_batch_band_place(gpet_batch* b, const int32_t* src_of, int from) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  const int B = b->B;
  BandState& bs = b->band;
  if (!bs.H) return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_band_place: the batch has no bands (gpet_batch_create_banded makes one that has)");
  const int ready = gpet_batch_warm_start_ready(b);
  if (ready) return ready;
  const bool groups = !src_of && from >= 0;
  char msg[384];
  if (groups) {
    const int rc = warm_groups_check(from, ensemble_is_kept(b), msg, sizeof msg);
    if (rc) return fail(c, rc, "%s", msg);
  } else if (src_of) {
    std::vector<int32_t> x_st((size_t)B), x_en((size_t)B);
    for (int e = 0; e < B; ++e) {
      x_st[e] = b->h_edges[e].x_st;
      x_en[e] = b->h_edges[e].x_en;
    }
    const int rc = warm_from_check(B, src_of, x_st.data(), x_en.data(), msg, sizeof msg);
    if (rc) return fail(c, rc, "%s", msg);
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const int32_t* d_src = nullptr;
  const int32_t* d_group_of = nullptr;
  const char* d_kept = nullptr;
  long long record_bytes = 0, off_trace = 0;
  if (groups || src_of) {
    EnsembleScratch* s = nullptr;
    const int rc = scratch(b, &s);
    if (rc) return rc;
    if (!s->src) HIPCHK(c, hipMalloc(&s->src, sizeof(int32_t) * (size_t)B));
    if (src_of) {
      s->h_src.assign(src_of, src_of + B);  // (every call that used it has waited for its copy)
      HIPCHK(c, hipMemcpyAsync(s->src, s->h_src.data(), sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, st));
      HIPCHK(c, gpet_wait(st));             // (and so does this one: the explicit table is not the path of a sequence)
    } else {
      const EnsembleLayout K = ensemble_layout(s->kept_G, B, s->kept_len_cap);
      d_group_of = reinterpret_cast<const int32_t*>(s->kept + warm_kept_group_off(s->kept_G, B, s->kept_len_cap));
      d_kept = s->kept;
      record_bytes = (long long)K.record_bytes;
      off_trace = (long long)K.off_trace;
      HIPCHK(c, launch_warm_sources(st, B, d_group_of, d_kept, record_bytes, from, s->src));
    }
    d_src = s->src;
  }
  HIPCHK(c, launch_band_place(st, b->d_edges, B, d_src, d_group_of, d_kept, record_bytes, off_trace, bs.M, bs.fit, bs.r0, bs.lohi, bs.pend));
  bs.pending = true;
  return GPET_OK;
}

int gpet_batch_warm_start_groups(gpet_batch* b, int from, int warm_every, int32_t* n_obs_out, int32_t* src_out) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  return warm_start_sourced(b, from, nullptr, warm_every, n_obs_out, src_out);
}

int gpet_batch_warm_start_from(gpet_batch* b, const int32_t* src_of, int warm_every, int32_t* n_obs_out) {
  GPET_BATCH_SCOPE(b);
  if (!b || !src_of) return GPET_ERR_BAD_ARG;
  return warm_start_sourced(b, 0, src_of, warm_every, n_obs_out, nullptr);
}

}  // extern "C"
