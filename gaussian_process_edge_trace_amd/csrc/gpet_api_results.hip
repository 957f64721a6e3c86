// C ABI: the finished result record of every edge (include/gpet_hip.h, "Result records").  What the host's
// GP_Edge_Tracing_Batch.finish computes from gpet_final_fit_all's mean / std (gpet.py:874-886) is computed here on the device,
// from the converged fit that is already in device memory, into one fixed-layout record per edge -- so a host that is not
// Python gets the credible interval and the statistics of a trace, and ranks exchange the records straight from device
// memory (gpet_gather_results, gpet_api_comm.hip).
#include "gpet_api_internal.h"

namespace gpet {

// One workgroup per edge, striding over len_cap.  fin_out of edge e: mean (pixels) at [0, Lg), std (standardised units, as
// the reference returns it) at [out_stride, out_stride + Lg); theta [B][4] = log(constant, length_scale, noise_level), -LML.
__global__ __launch_bounds__(256) void k_finish_results(const EdgeDev* __restrict__ edges, const double* __restrict__ theta,
                                                        int out_stride, long long len_cap, size_t rec_bytes, char* __restrict__ dst) {
  // numpy evaluates mean - 1.96 * std with two roundings: no contraction into a fused multiply-add here (the pragma covers
  // the expressions of this body only: the __dmul_rn family of the HIP headers is plain arithmetic that may still contract)
#pragma clang fp contract(off)
  const int e = blockIdx.x;
  const EdgeDev& E = edges[e];
  const int Lg = E.Lg;
  const long long x_st = E.x_st;
  const double* mean = E.fin_out;
  const double* sd = E.fin_out + out_stride;
  char* rec = dst + (size_t)e * rec_bytes;
  long long* trace = reinterpret_cast<long long*>(rec + sizeof(gpet_result_head));
  double* lower = reinterpret_cast<double*>(trace + 2 * len_cap);
  double* upper = lower + len_cap;
  if (threadIdx.x == 0) {
    const gpet_scalars& sc = *E.sc;
    gpet_result_head h;
    h.edge_len = Lg;
    h.n_iter = sc.iter;
    h.n_obs = sc.n_obs;
    h.status = sc.status;
    for (int k = 0; k < 3; ++k) h.theta[k] = theta[4 * (size_t)e + k];
    h.nlml = theta[4 * (size_t)e + 3];
    *reinterpret_cast<gpet_result_head*>(rec) = h;
  }
  for (long long k = threadIdx.x; k < len_cap; k += blockDim.x) {
    long long y = 0, x = 0;
    double lo = 0.0, up = 0.0;
    if (k < Lg) {
      const double m = mean[k];
      const double d = 1.96 * sd[k];
      lo = m - d;
      up = m + d;
      y = int_f64_to_i64(rint(m));  // np.rint: round half to even (gpet.py:885)
      x = x_st + k;            // x_grid (gpet.py:111)
    }
    trace[2 * k] = y;
    trace[2 * k + 1] = x;
    lower[k] = lo;
    upper[k] = up;
  }
}

}  // namespace gpet

size_t result_record_bytes(int64_t len_cap) {
  const int64_t per_point = 2 * (int64_t)sizeof(int64_t) + 2 * (int64_t)sizeof(double);
  if (len_cap < 0 || len_cap > ((int64_t)1 << 40) / per_point) return 0;
  return sizeof(gpet_result_head) + (size_t)len_cap * (size_t)per_point;
}

static int check_results(gpet_batch* b, int64_t len_cap) {
  gpet_ctx* c = b->ctx;
  if (state_missing(b->st, StateEvent::read_results))
    return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_results: no converged fit of the current trace (run gpet_final_fit_all first)");
  int widest = 0;
  for (const EdgeDev& E : b->h_edges) widest = std::max(widest, E.Lg);
  const size_t rec = result_record_bytes(len_cap);
  if (rec == 0 || len_cap < widest)
    return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_results: len_cap=%lld is below the widest edge (%d points) or out of range",
                (long long)len_cap, widest);
  return GPET_OK;
}

int enqueue_results(gpet_batch* b, int64_t len_cap, void* d_dst) {
  gpet_ctx* c = b->ctx;
  int rc = check_results(b, len_cap);
  if (rc) return rc;
  const size_t rec = result_record_bytes(len_cap);
  HIPCHK(c, hipSetDevice(c->device));
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_finish_results, dim3(b->B), dim3(256), 0, c->stream, b->d_edges, b->lb_theta_out, b->bd.Lg,
                     (long long)len_cap, rec, static_cast<char*>(d_dst));
  HIPCHK(c, hipGetLastError());
  return GPET_OK;
}

extern "C" {

int gpet_result_bytes(int64_t len_cap, size_t* bytes) {
  if (!bytes) return GPET_ERR_BAD_ARG;
  const size_t rec = result_record_bytes(len_cap);
  if (rec == 0) return GPET_ERR_BAD_ARG;
  *bytes = rec;
  return GPET_OK;
}

int gpet_batch_results(gpet_batch* b, int64_t len_cap, void* dst, int dst_on_device) {
  GPET_BATCH_SCOPE(b);
  if (!b || !dst) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  if (dst_on_device) return enqueue_results(b, len_cap, dst);
  int rc = check_results(b, len_cap);
  if (rc) return rc;
  const size_t need = (size_t)b->B * result_record_bytes(len_cap);
  HIPCHK(c, hipSetDevice(c->device));
  if (need > b->results_bytes) {
    if (b->d_results) (void)hipFree(b->d_results);
    b->d_results = nullptr;
    b->results_bytes = 0;
    HIPCHK(c, hipMalloc(&b->d_results, need));
    b->results_bytes = need;
  }
  rc = enqueue_results(b, len_cap, b->d_results);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(dst, b->d_results, need, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, gpet_wait(c->stream));
  return GPET_OK;
}

}  // extern "C"
