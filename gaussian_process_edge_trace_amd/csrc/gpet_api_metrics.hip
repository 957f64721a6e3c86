// C ABI: denoise quality metrics (include/gpet_hip.h, "denoise quality metrics") -- PSNR, SSIM, min-max NRMSE and the
// Shannon entropy of every pair of a stack, the sums and the SSIM map made on the device.  The arithmetic, its refusals and the launch
// shapes: gpet_metrics_plan.h; the kernels: gpet_k_metrics.inc.  The pairs go chunk by chunk (metrics_chunks) through the context's
// workspace (pre_ws, the block the stages in front of the raw-frame path share): the pointer table and the records of all pairs at its
// head, then per pair of a chunk six f64 planes and the staged copies of the frames that come from the host.
#include "gpet_api_internal.h"

static_assert(METRICS_A_ON_DEVICE == GPET_RAW_ON_DEVICE && METRICS_B_ON_DEVICE == GPET_METRICS_B_ON_DEVICE &&
                  METRICS_MAPS_ON_DEVICE == GPET_METRICS_MAPS_ON_DEVICE,
              "gpet_metrics_plan.h numbers the flags as include/gpet_hip.h does");

extern "C" {

int gpet_metrics_images(gpet_ctx* c, const void* const* raw_a, int pix_a, const void* const* raw_b, int pix_b, int n_img, int M, int N,
                        const gpet_metrics* spec, unsigned int flags, double* out, double* const* ssim_maps) {
  if (!c) return GPET_ERR_BAD_ARG;
  if (flags & ~(GPET_RAW_ON_DEVICE | GPET_METRICS_B_ON_DEVICE | GPET_METRICS_MAPS_ON_DEVICE))
    return fail(c, GPET_ERR_BAD_ARG, "metrics: unknown flag bits 0x%x", flags);
  const bool a_dev = (flags & GPET_RAW_ON_DEVICE) != 0, b_dev = (flags & GPET_METRICS_B_ON_DEVICE) != 0,
             maps_dev = (flags & GPET_METRICS_MAPS_ON_DEVICE) != 0;
  MetricsSpec sp;
  if (spec) {
    sp.win_size = spec->win_size;
    sp.use_sample_covariance = spec->use_sample_covariance;
    sp.K1 = spec->K1;
    sp.K2 = spec->K2;
    sp.data_range = spec->data_range;
  }
  const size_t px = (size_t)(M > 0 ? M : 0) * (size_t)(N > 0 ? N : 0);
  const size_t bytes_a = px * (size_t)pix_bytes(pix_a), bytes_b = px * (size_t)pix_bytes(pix_b);
  const size_t st_a = a_dev ? 0 : bytes_a, st_b = b_dev ? 0 : bytes_b;
  char msg[384];
  if (metrics_check(!raw_a || !raw_b || !out, n_img, pix_a, pix_b, M, N, spec ? &sp : nullptr, st_a, st_b, msg, sizeof msg))
    return fail(c, GPET_ERR_BAD_ARG, "%s", msg);
  for (int g = 0; g < n_img; ++g)
    if (!raw_a[g] || !raw_b[g] || (ssim_maps && !ssim_maps[g])) return fail(c, GPET_ERR_BAD_ARG, "metrics: frame, result or map %d is a null pointer", g);
  HIPCHK(c, hipSetDevice(c->device));
  const size_t frame_bytes = metrics_frame_bytes((long long)px, st_a, st_b), o_sa = dn_align(6 * px * sizeof(double)), o_sb = o_sa + dn_align(st_a);
  const StagePlan plan = metrics_chunks(n_img, frame_bytes);
  const size_t o_acc = dn_align(2 * sizeof(void*) * (size_t)n_img), head = o_acc + dn_align(sizeof(MetricsAcc) * (size_t)n_img);
  const size_t need = head + (size_t)plan.per_chunk * frame_bytes;
  if (need > c->pre_ws_bytes) {  // (device memory of the context that only grows; the stream is idle when it is replaced)
    HIPCHK(c, gpet_wait(c->stream));
    if (c->pre_ws) (void)hipFree(c->pre_ws);
    c->pre_ws = nullptr;
    c->pre_ws_bytes = 0;
    HIPCHK(c, hipMalloc((void**)&c->pre_ws, need));
    c->pre_ws_bytes = need;
  }
  char* const ws = c->pre_ws + head;
  const void** d_tab = reinterpret_cast<const void**>(c->pre_ws);
  MetricsAcc* d_acc = reinterpret_cast<MetricsAcc*>(c->pre_ws + o_acc);
  std::vector<const void*> h_tab(2 * (size_t)n_img);
  std::vector<MetricsAcc> h_acc((size_t)n_img);
  for (int k = 0; k < plan.n_chunks; ++k)
    for (int i = 0; i < stage_count(plan, k, n_img); ++i) {
      const int g = stage_first(plan, k) + i;
      h_tab[2 * (size_t)g] = a_dev ? raw_a[g] : ws + (size_t)i * frame_bytes + o_sa;
      h_tab[2 * (size_t)g + 1] = b_dev ? raw_b[g] : ws + (size_t)i * frame_bytes + o_sb;
    }
  hipStream_t st = c->stream;
  const double R_ssim = sp.data_range > 0.0 ? sp.data_range : metrics_default_range_ssim(pix_a);
  hipError_t e = hipMemcpyAsync(d_tab, h_tab.data(), sizeof(void*) * h_tab.size(), hipMemcpyHostToDevice, st);
  for (int k = 0; k < plan.n_chunks && e == hipSuccess; ++k) {
    const int first = stage_first(plan, k), cnt = stage_count(plan, k, n_img);
    for (int i = 0; i < cnt && e == hipSuccess; ++i) {
      if (!a_dev) e = hipMemcpyAsync(const_cast<void*>(h_tab[2 * (size_t)(first + i)]), raw_a[first + i], bytes_a, hipMemcpyHostToDevice, st);
      if (!b_dev && e == hipSuccess)
        e = hipMemcpyAsync(const_cast<void*>(h_tab[2 * (size_t)(first + i) + 1]), raw_b[first + i], bytes_b, hipMemcpyHostToDevice, st);
    }
    if (e == hipSuccess) e = launch_metrics(st, d_tab, d_acc, first, cnt, pix_a, pix_b, M, N, sp, R_ssim, ws, frame_bytes);
    for (int i = 0; i < cnt && ssim_maps && e == hipSuccess; ++i)
      e = hipMemcpyAsync(ssim_maps[first + i], ws + (size_t)i * frame_bytes + 5 * px * sizeof(double), px * sizeof(double),
                         maps_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = launch_metrics_entropy(st, d_tab, d_acc, first, cnt, pix_b, M, N, ws, frame_bytes);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h_acc.data(), d_acc, sizeof(MetricsAcc) * (size_t)n_img, hipMemcpyDeviceToHost, st);
  // (the call reads the records back: it always waits, also after an enqueue error, which is reported in preference to the wait's own)
  const hipError_t ew = gpet_wait(st);
  HIPCHK(c, e);
  HIPCHK(c, ew);
  for (int g = 0; g < n_img; ++g)
    if (metrics_figures(h_acc[g], sp, pix_a, pix_b, M, N, out + 4 * (size_t)g, msg, sizeof msg)) return fail(c, GPET_ERR_BAD_ARG, "%s (frame %d)", msg, g);
  return GPET_OK;
}

}  // extern "C"
