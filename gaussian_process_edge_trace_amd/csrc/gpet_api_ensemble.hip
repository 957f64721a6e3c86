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
};

void ensemble_free(gpet_batch* b) {
  if (!b || !b->ens) return;
  EnsembleScratch* s = b->ens;
  if (s->fc_mem) (void)hipFree(s->fc_mem);
  if (s->tab_mem) (void)hipFree(s->tab_mem);
  if (s->off_acc) (void)hipFree(s->off_acc);
  if (s->stage) (void)hipFree(s->stage);
  delete s;
  b->ens = nullptr;
}

// the state gpet_batch_results asks for, with its status
static int check_fit(gpet_batch* b, const char* who) {
  if (!b->have_results)
    return fail(b->ctx, GPET_ERR_BAD_ARG, "%s: no converged fit of the current trace (run gpet_final_fit_all first)", who);
  return GPET_OK;
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
  const int B = b->B;
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
  if (!dst_on_device) {
    HIPCHK(c, hipMemcpyAsync(dst, d_dst, (size_t)L.total_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, gpet_wait(st));
  }
  return GPET_OK;
}

}  // extern "C"
