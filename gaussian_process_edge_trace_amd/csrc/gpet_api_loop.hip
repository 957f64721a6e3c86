// C ABI, part 5: the device-resident loop (a8) and the dispatch of its normal generators.
#include "gpet_api_internal.h"
#include "gpet_loop_plan.h"

// One sequential walk per stream: the register-resident generator (four streams per wave, gpet_rng.hip) when the batch is
// homogeneous and the launch has enough streams to fill the GPU with single waves (2 048 = half of its SIMDs; a wave of
// four streams takes ~2.5 ms against 0.6 ms for a three-wave workgroup per stream, so small launches keep the old kernel),
// else one workgroup per stream (k_mt_normals).  The same numbers either way.
hipError_t launch_normals_seq(gpet_batch* b, hipStream_t st, EdgeDev* edges_l, int B_l, const unsigned int* seeds_l,
                              int add_iter, int iter_abs, int n_ahead, int z_store) {
  const int o = opt(Opt::rng4);
  if (b->bd.rng4 && (o > 0 || (o < 0 && (long long)B_l * n_ahead >= 2048)))
    return launch_normals4(st, edges_l, B_l, seeds_l, add_iter, iter_abs, n_ahead, z_store, b->bd.Lg, b->bd.S, b->bd.z_cols);
  return launch_normals(st, edges_l, B_l, seeds_l, add_iter, iter_abs, n_ahead, z_store);
}

// The normals of `n_ahead` iterations of B_l edges: one workgroup per stream (k_mt_normals), or -- when that leaves
// most of the GPU idle and the streams are long -- every stream cut into chunks that many workgroups generate at once
// (MT19937 jump-ahead, launch_normals_chunked).  The same numbers either way.
int normals_auto(gpet_batch* b, hipStream_t st, EdgeDev* edges_l, int B_l, const unsigned int* seeds_l, int add_iter,
                 int iter_abs, int n_ahead, int z_store, bool allow_chunked) {
  gpet_ctx* c = b->ctx;
  if (b->rng_mode == 1) {  // opt-in Philox mode (gpet_batch_set_rng)
    HIPCHK(c, launch_normals_philox(st, edges_l, B_l, b->bd, seeds_l, add_iter, iter_abs, n_ahead, z_store));
    return GPET_OK;
  }
  const int streams = B_l * n_ahead;
  const int nc = mtj_chunks((long long)b->bd.S * b->bd.Lg);
  const int o = opt(Opt::rng_chunked);  // -1: by launch shape
  const bool force4 = opt(Opt::rng4) > 0 && b->bd.rng4;  // (tests: the register-resident generator on any launch shape)
  // (the chunked form works in the batch's ONE jump workspace: a launch that runs beside another chunked launch of the same batch
  //  -- the tail of a small batch's first normals on the fit stream, Loop::normals_side_deep -- must take the sequential kernel)
  const bool chunked = allow_chunked && !force4 && nc >= 2 && (o > 0 || (o < 0 && streams <= 32 && nc >= 4));
  if (!chunked) {
    HIPCHK(c, launch_normals_seq(b, st, edges_l, B_l, seeds_l, add_iter, iter_abs, n_ahead, z_store));
    return GPET_OK;
  }
  const size_t need = mtj_work_bytes(streams, nc);
  if (need > b->mtj_bytes) {
    if (b->mtj_work) {
      HIPCHK(c, hipDeviceSynchronize());  // (launches that use the old workspace may still be in flight)
      (void)hipFree(b->mtj_work);
      b->mtj_work = nullptr;
      b->mtj_bytes = 0;
    }
    HIPCHK(c, hipMalloc(&b->mtj_work, need));
    b->mtj_bytes = need;
  }
  if (!b->d_mtj_poly) {
    HIPCHK(c, hipMalloc(&b->d_mtj_poly, mtj_poly_bytes()));
    HIPCHK(c, hipMemcpy(b->d_mtj_poly, mtj_poly_host(), mtj_poly_bytes(), hipMemcpyHostToDevice));
  }
  HIPCHK(c, launch_normals_chunked(st, edges_l, B_l, seeds_l, add_iter, iter_abs, n_ahead, z_store, b->mtj_work, nc, b->d_mtj_poly));
  return GPET_OK;
}

namespace {

int read_active(gpet_batch* b, int* active) {  // the edges' state as of now on the host; *active = edges still running
  int rc = check_device_status(b);
  if (rc) return rc;
  *active = 0;
  for (int e = 0; e < b->B; ++e) *active += b->h_scalars[e].done ? 0 : 1;
  return GPET_OK;
}

// One call of gpet_trace_iterate: the batch, the plan and the tables of the group being enqueued.
struct Loop {
  gpet_batch* const b;
  gpet_ctx* const c;
  const uint32_t* const base_seeds;
  const int ring;
  const LoopPlan plan;  // the options, resolved once: the batch's table is installed for the whole call (GPET_BATCH_SCOPE)
  EdgeDev* edges_l;     // the batch's tables, or the compacted ones
  unsigned int* seeds_l;
  int B_l;
  int first = 0, horizon = 0;  // the group's iterations: first <= cur < horizon
  bool fit_used = false;       // the head of a small batch's normals put a launch on the fit stream (this group)

  // The tables of the edges still running.  Every kernel skips finished edges by itself, but it still starts one workgroup per edge
  // and tile to find that out: 2.2 ms per iteration for 1024 finished edges, and the last iterations of a batch run with a handful
  // of edges left.  (The previous group has completed -- check_device_status synchronised -- so the tables may be overwritten.)
  int compact_active() {
    b->h_edges_act.clear();
    b->h_seeds_act.clear();
    for (int e = 0; e < b->B; ++e)
      if (!b->h_scalars[e].done) {
        b->h_edges_act.push_back(b->h_edges[e]);
        b->h_seeds_act.push_back(base_seeds[e]);
      }
    B_l = (int)b->h_edges_act.size();
    if (!b->d_edges_act) {
      HIPCHK(c, hipMalloc(&b->d_edges_act, sizeof(EdgeDev) * b->B));
      HIPCHK(c, hipMalloc(&b->d_seeds_act, sizeof(unsigned int) * b->B));
    }
    HIPCHK(c, hipMemcpyAsync(b->d_edges_act, b->h_edges_act.data(), sizeof(EdgeDev) * B_l, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b->d_seeds_act, b->h_seeds_act.data(), sizeof(unsigned int) * B_l, hipMemcpyHostToDevice, c->stream));
    edges_l = b->d_edges_act;
    seeds_l = b->d_seeds_act;
    return GPET_OK;
  }

  // the normals of iterations [from, from + n) by one launch on st, and their events
  int normals(hipStream_t st, int from, int n, bool allow_chunked = true) {
    int rc = normals_auto(b, st, edges_l, B_l, seeds_l, 1, from, n, loop_z_store(b), allow_chunked);
    if (rc) return rc;
    for (int q = from; q < from + n; ++q) HIPCHK(c, hipEventRecord(b->ev_norm[q % 16], st));
    b->norm_issued = from + n;
    return GPET_OK;
  }
  int normals_inline_iteration(int cur) { return normals(c->stream, cur, 1); }
  int normals_inline_group(int cur) {  // at the group's first iteration (and again where a group is longer than the ring)
    return b->norm_issued > cur ? GPET_OK : normals(c->stream, cur, std::min(horizon - cur, ring - 1));
  }
  // The streams of the next n <= look iterations in ONE launch (blockIdx.x = iteration), side by side, whenever at most refill_at are
  // left.  Their ring slots were last read by the sample GEMMs of iterations <= cur - 1 (outstanding + n <= ring).
  int normals_side_deep(int cur) {
    if (b->norm_issued - cur > plan.refill_at) return GPET_OK;
    const int j = b->norm_issued, n = std::min(ring - (j - cur), plan.look);
    if (cur - 1 >= first) HIPCHK(c, hipStreamWaitEvent(b->side, b->ev_gemm[(cur - 1) % 16], 0));
    // the head of a trace: chunked, one launch per iteration on the side stream, while the sequential launch of the iterations
    // after them runs beside them on the (idle until the converged fits) fit stream
    const int head = head_iterations(plan, j, cur, B_l, b->rng_mode, n);
    for (int q = j; q < j + head; ++q) {
      int rc = normals(b->side, q, 1);
      if (rc) return rc;
    }
    if (head > 0) HIPCHK(c, hipStreamWaitEvent(b->fit, b->ev_main, 0));  // (the seeds and the edge table are on the device)
    // (later refills run on the side stream BESIDE this tail -- different ring slots, and the tail is the sequential kernel,
    //  which has no workspace; the host waits for the fit stream too at the end of the group)
    if (head > 0) fit_used = true;
    return n > head ? normals(head > 0 ? b->fit : b->side, j + head, n - head, head == 0) : GPET_OK;
  }
  // one launch per iteration, `look` iterations ahead of the loop, never past the horizon of the iterations enqueued together
  int normals_side_shallow(int cur) {
    while (b->norm_issued <= cur + plan.look && b->norm_issued < horizon) {
      const int j = b->norm_issued;
      if (plan.look == 0) {
        if (j - 1 >= first) HIPCHK(c, hipStreamWaitEvent(b->side, b->ev_pix[(j - 1) % 16], 0));
      } else if (j - ring >= first) {
        HIPCHK(c, hipStreamWaitEvent(b->side, b->ev_gemm[(j - ring) % 16], 0));
      }
      int rc = normals(b->side, j, 1);
      if (rc) return rc;
    }
    return GPET_OK;
  }

  // the kernel chain of iteration cur (every kernel skips edges whose `done` flag is set, so edges that finish inside a group cost little)
  int enqueue_iteration(int cur) {
    if (b->structured) {
      HIPCHK(c, launch_struct_iteration(c->stream, edges_l, B_l, b->bd));
    } else {
      HIPCHK(c, launch_fit_predict(c->stream, edges_l, B_l, b->bd, 1));
      HIPCHK(c, launch_factor(c->stream, edges_l, B_l, b->bd, ~0u, edges_l == b->d_edges ? b->h_edges.data() : b->h_edges_act.data()));
    }
    HIPCHK(c, hipStreamWaitEvent(c->stream, b->ev_norm[cur % 16], 0));
    // samples + scores: the GEMM writes all S rows and the scorer reads them back (two fused forms that never wrote the sample
    // matrix were built in rounds 3 and 4, bit-identical, and measured slower: an f64 matrix instruction and f64 vector
    // work do not overlap, DESIGN.md history)
    HIPCHK(c, launch_sample(c->stream, edges_l, B_l, b->bd, b->structured ? b->bd.r0_max : 0));
    HIPCHK(c, hipEventRecord(b->ev_gemm[cur % 16], c->stream));  // ring slot cur % ring may be refilled
    // loop form: the density stays raw and band-limited in HBM; the pixel kernels normalise on the fly
    if (plan.fused_tail) {
      HIPCHK(c, launch_score_kde_fused_tail(c->stream, edges_l, B_l, b->bd));
    } else {
      HIPCHK(c, launch_score(c->stream, edges_l, B_l, b->bd));
      HIPCHK(c, launch_kde(c->stream, edges_l, B_l, b->bd, 0, ~0u, 1));
    }
    HIPCHK(c, launch_pixels(c->stream, edges_l, B_l, b->bd, 1));
    HIPCHK(c, hipEventRecord(b->ev_pix[cur % 16], c->stream));
    // opt-in history: the record of this iteration for the edges that completed it (their counter is now iters_issued + 1)
    if (b->d_hist) HIPCHK(c, launch_history(c->stream, edges_l, B_l, b->hist, b->iters_issued + 1));
    b->iters_issued += 1;
    return GPET_OK;
  }

  // waits for the group (n_it iterations, of `group` planned), reads the edges' state and sizes the next group (*next = 0: stop)
  int end_group(int group, int n_it, int* active, int* next) {
    b->have_fit = b->have_factor = b->have_normals = b->have_samples = b->have_scores = true;
    HIPCHK(c, gpet_wait(b->side));  // (its launches read the compacted tables too)
    if (fit_used) HIPCHK(c, gpet_wait(b->fit));
    fit_used = false;
    int rc = read_active(b, active);
    if (rc) return rc;
    EdgeProgress prog[64];  // (next_group looks at the edges of a batch of up to 64 only)
    const int count = b->B <= 64 && *active > 0 ? b->B : 0;
    if (count && (int)b->h_nobs_prev.size() != b->B) b->h_nobs_prev.assign(b->B, 0);
    for (int e = 0; e < count; ++e) {
      prog[e] = {b->h_scalars[e].done, b->h_scalars[e].n_obs, b->h_nobs_prev[e], b->h_edges[e].algo_thresh};
      b->h_nobs_prev[e] = prog[e].n_obs;  // (of finished edges too)
    }
    *next = next_group(b->B, group, n_it, *active, prog, count);
    return GPET_OK;
  }
};

}  // namespace

extern "C" {

int gpet_trace_iterate(gpet_batch* b, const uint32_t* base_seeds, int max_iters, int* n_active) {
  GPET_BATCH_SCOPE(b);
  if (!b || !base_seeds || !n_active || max_iters < 0) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  b->have_results = false;
  b->have_last_fit = false;  // (another trace is under way: d_fin_out belongs to the one before until its own converged fit)
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(b->d_seeds, base_seeds, sizeof(uint32_t) * b->B, hipMemcpyHostToDevice, c->stream));
  *n_active = b->B;
  if (max_iters == 0) return read_active(b, n_active);
  LoopPlan plan = resolve_loop_plan(b->B, b->bd.z_ring, opt(Opt::rng_lookahead), opt(Opt::rng_inline), opt(Opt::rng_refill_at),
                                    opt(Opt::rng_head), opt(Opt::loop_fused_tail));
  plan.fused_tail = plan.fused_tail && score_tail_applies(b->bd);
  Loop l{b, c, base_seeds, b->bd.z_ring, plan, b->d_edges, b->d_seeds, b->B};
  // Groups of iterations (next_group): after every group the host reads the `done` flags, stops if no edge is left and otherwise
  // enqueues the next group for the edges still running.
  for (int remaining = max_iters, group = 8; remaining > 0 && group > 0;) {
    const int n_it = std::min(group, remaining);
    int rc = *n_active < b->B ? l.compact_active() : GPET_OK;
    if (rc) return rc;
    l.first = b->iters_issued;
    l.horizon = l.first + n_it;
    if (b->norm_issued < l.first) b->norm_issued = l.first;
    HIPCHK(c, hipEventRecord(b->ev_main, c->stream));  // the seeds and the edge table are on the device
    HIPCHK(c, hipStreamWaitEvent(b->side, b->ev_main, 0));
    for (int cur = l.first; cur < l.horizon && !rc; ++cur) {
      switch (plan.mode) {
        case NormalsMode::inline_per_iteration: rc = l.normals_inline_iteration(cur); break;
        case NormalsMode::inline_per_group: rc = l.normals_inline_group(cur); break;
        case NormalsMode::side_deep: rc = l.normals_side_deep(cur); break;
        case NormalsMode::side_shallow: rc = l.normals_side_shallow(cur); break;
      }
      if (!rc) rc = l.enqueue_iteration(cur);
    }
    if (!rc) rc = l.end_group(group, n_it, n_active, &group);
    if (rc) return rc;
    remaining -= n_it;
  }
  return GPET_OK;
}

}  // extern "C"
