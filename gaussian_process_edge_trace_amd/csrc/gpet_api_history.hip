// C ABI: the iteration history of a batch (include/gpet_hip.h, "iteration history"): storage of its own beside the arena, laid out by
// gpet_history_plan.h, filled by k_history (gpet_k_history.inc) once per loop iteration (Loop::enqueue_iteration), read back in one copy.
#include "gpet_api_internal.h"

// empties edge e's region (e < 0: every region) on the context's stream; nothing to do with the history off
int history_clear(gpet_batch* b, int e) {
  if (!b->d_hist) return GPET_OK;
  gpet_ctx* c = b->ctx;
  const size_t per = (size_t)b->hist.edge_bytes;
  if (e < 0) HIPCHK(c, hipMemsetAsync(b->d_hist, 0, per * (size_t)b->B, c->stream));
  else HIPCHK(c, hipMemsetAsync(b->d_hist + per * (size_t)e, 0, per, c->stream));
  return GPET_OK;
}

static int history_off(gpet_batch* b, const char* who) {
  return fail(b->ctx, GPET_ERR_STATE, "%s: the batch keeps no iteration history (gpet_batch_set_history)", who);
}

extern "C" {

int gpet_batch_set_history(gpet_batch* b, int level, int iter_cap) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  if (level < 0 || level > HISTORY_LEVEL_MAX || (level > 0 && iter_cap < 1))
    return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_set_history: level %d (0..%d) with iter_cap %d (at least 1)", level, HISTORY_LEVEL_MAX, iter_cap);
  gpet_history_plan plan = {};
  if (level > 0) {
    plan = history_plan(level, iter_cap, b->bd.obs_cap, b->bd.Lg);
    if (plan.level == 0) return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_set_history: iter_cap %d is out of range for this batch", iter_cap);
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gpet_wait(c->stream));  // (launches that write the old storage may still be in flight)
  if (b->d_hist) (void)hipFree(b->d_hist);
  b->d_hist = nullptr;
  b->hist = gpet_history_plan{};
  if (level > 0) {
    const size_t bytes = (size_t)plan.edge_bytes * (size_t)b->B;
    hipError_t he = hipMalloc(&b->d_hist, bytes);
    if (he != hipSuccess) {
      b->d_hist = nullptr;
      for (EdgeDev& E : b->h_edges) E.hist = nullptr;
      (void)hipMemcpyAsync(b->d_edges, b->h_edges.data(), sizeof(EdgeDev) * (size_t)b->B, hipMemcpyHostToDevice, c->stream);
      (void)gpet_wait(c->stream);
      return fail(c, GPET_ERR_HIP, "hipMalloc(%zu bytes of iteration history) failed: %s", bytes, hipGetErrorString(he));
    }
    b->hist = plan;
    HIPCHK(c, hipMemsetAsync(b->d_hist, 0, bytes, c->stream));
  }
  for (int e = 0; e < b->B; ++e) b->h_edges[e].hist = b->d_hist ? b->d_hist + (size_t)plan.edge_bytes * (size_t)e : nullptr;
  HIPCHK(c, hipMemcpyAsync(b->d_edges, b->h_edges.data(), sizeof(EdgeDev) * (size_t)b->B, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, gpet_wait(c->stream));
  return GPET_OK;
}

int gpet_history_layout(gpet_batch* b, gpet_history_plan* out) {
  if (!b || !out) return GPET_ERR_BAD_ARG;
  if (!b->d_hist) return history_off(b, "gpet_history_layout");
  *out = b->hist;
  return GPET_OK;
}

int gpet_batch_history(gpet_batch* b, int e, void* dst, size_t bytes, int dst_on_device) {
  GPET_BATCH_SCOPE(b);
  if (!b || !dst || e < -1 || e >= b->B) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  if (!b->d_hist) return history_off(b, "gpet_batch_history");
  const size_t per = (size_t)b->hist.edge_bytes, need = e < 0 ? per * (size_t)b->B : per;
  if (bytes < need) return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_history: %zu bytes at dst, %zu needed", bytes, need);
  HIPCHK(c, hipSetDevice(c->device));
  const char* src = b->d_hist + (e < 0 ? 0 : per * (size_t)e);
  HIPCHK(c, hipMemcpyAsync(dst, src, need, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  if (!dst_on_device) HIPCHK(c, gpet_wait(c->stream));
  return GPET_OK;
}

int gpet_history_record(gpet_batch* b) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  if (!b->d_hist) return history_off(b, "gpet_history_record");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, launch_history(c->stream, b->d_edges, b->B, b->hist, 0));
  HIPCHK(c, gpet_wait(c->stream));
  return GPET_OK;
}

}  // extern "C"
