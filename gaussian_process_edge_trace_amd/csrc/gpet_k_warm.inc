// Warm start of the next frame of a sequence on the device (gpet_batch_warm_start): every edge's observation set for the next
// trace from its own last converged fit, which gpet_final_fit_all left in fin_out -- the rule of sequence.warm_start_obs, so a
// frame-to-frame step needs no trip of the traces through the host.

// The trace is rint(mean) on the edge's x-grid (the rounding of k_finish_results and GP_Edge_Tracing_Batch.finish).  Candidates
// are the grid indices step, 2 step, ... < Lg - 1 (the end points never are), starting at step = max(1, warm_every); a candidate
// is kept when x_st < x < x_en and its row lies in the image.  `algo_thresh` or more kept pixels would let the next trace's
// loop not run at all (gpet.py:829): the stride is doubled until fewer are kept, or none.
// One wave per edge: a counting pass per stride (lanes stride over the candidates, ballot + popcount), then one compaction pass
// in ascending x (the lane's position is the number of kept candidates in the lanes below it), plain per-lane stores.
// Afterwards the edge is in the state gpet_batch_set_obs leaves: n_obs, done, status OK, iter 0, eigenvector tags cleared,
// and -- where iterations had run since the last reset -- the any-rank factor's row tags cleared.
__global__ void __launch_bounds__(64) k_warm_start(EdgeDev* edges, int warm_every) {
  const EdgeDev E = edges[blockIdx.x];
  gpet_scalars* sc = E.sc;
  const int lane = threadIdx.x;
  const double* __restrict__ mean = E.fin_out;
  const long long last = (long long)E.Lg - 1;  // candidates are grid indices below it
  const double y_max = (double)(E.M - 1);
  auto kept = [&](long long k) {  // (k < last) candidate k of the grid: strictly inside the end points, row inside the image
    const long long x = (long long)E.x_st + k;
    const double y = rint(mean[k]);  // (NaN fails both comparisons, as INT64_MIN does on the host)
    return x > E.x_st && x < E.x_en && y >= 0.0 && y <= y_max;
  };
  long long step = warm_every > 1 ? warm_every : 1;
  int n_keep = 0;
  for (;;) {
    int cnt = 0;
    for (long long k0 = step; k0 < last; k0 += step * WAVE) {  // (uniform trip count: every lane reaches the ballot)
      const long long k = k0 + step * lane;
      cnt += __popcll(__ballot(k < last && kept(k)));
    }
    n_keep = cnt;
    if (n_keep < E.algo_thresh || n_keep == 0) break;
    step *= 2;  // (ends: no candidate is left once step >= Lg - 1)
  }
  if (n_keep > E.obs_cap) n_keep = E.obs_cap;  // (cannot happen: algo_thresh < n_bins <= obs_cap; the stores below stay inside obs_xy)
  int base = 0;
  for (long long k0 = step; k0 < last; k0 += step * WAVE) {
    const long long k = k0 + step * lane;
    const bool take = k < last && kept(k);
    const unsigned long long bal = __ballot(take);
    const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
    if (take && pos < n_keep) {
      E.obs_xy[2 * pos] = (long long)E.x_st + k;
      E.obs_xy[2 * pos + 1] = (long long)rint(mean[k]);  // (an integer in [0, M - 1]: exact)
    }
    base += __popcll(bal);
  }
  if (lane == 0) {
    const int iters_done = sc->iter;
    sc->n_obs = n_keep;
    sc->done = (n_keep >= E.algo_thresh) ? 1 : 0;
    sc->status = GPET_OK;
    sc->iter = 0;  // a new observation set restarts the edge's loop (gpet.py:820-828)
    E.wq_tag[0] = 0;
    E.wq_tag[1] = 0;
    if (iters_done >= 1) {  // (0: gpet_batch_reset / gpet_batch_set_images has been here already and decided what stays)
      E.ap_tag[0] = 0;
      E.ap_tag[1] = 0;
      E.ap_tag[2] = 0;
    }
  }
}

hipError_t launch_warm_start(hipStream_t st, EdgeDev* d_edges, int B, int warm_every) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_warm_start, dim3(B), dim3(64), 0, st, d_edges, warm_every);
  return hipGetLastError();
}

// ---- warm start from a source other than the edge itself (gpet_batch_warm_start_groups, gpet_batch_warm_start_from) ------------
// src[e] of every edge from the heads of the kept ensemble's records: thread per edge, the rule of warm_source (gpet_warm_plan.h).
// The heads were written by k_ensemble_pick before the images were swapped; nothing here reads an edge's scalars.
__global__ void __launch_bounds__(256) k_warm_sources(int B, const int32_t* __restrict__ group_of, const char* __restrict__ kept,
                                                      long long record_bytes, int from, int32_t* __restrict__ src) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B) return;
  const int g = group_of[e];
  if (g < 0) {
    src[e] = warm_source(e, g, 0, -1, -1, from);
    return;
  }
  const gpet_ensemble_head* h = reinterpret_cast<const gpet_ensemble_head*>(kept + (size_t)g * (size_t)record_bytes);
  src[e] = warm_source(e, g, h->n_members, h->medoid, h->best_cost, from);
}

// k_warm_start for destination edge e = blockIdx.x with the trace taken from src[e] (gpet_warm_plan.h): s >= 0 -- rint of edge s's
// converged mean; WARM_SRC_CONSENSUS -- the int64 row c[k] of the kept record of e's group (INT64_MIN where the median was NaN: it
// fails the row test as on the host); anything else -- nothing, the empty set.  Candidate rule, ballots, compaction and end state are
// k_warm_start's, and every bound is the DESTINATION's (x_st, x_en, Lg, M, algo_thresh, obs_cap): source and destination share the
// x-grid (checked on the host: gpet_ensemble_plan.h for groups, warm_from_check for a caller's table), so index k < Lg - 1 is inside
// the source's fin_out and inside the record's len_cap rows.
// A wave writes only its OWN edge's obs_xy, scalars and tags, with plain per-lane stores (no atomics).  Of other edges it reads the
// EdgeDev entry (the table no kernel writes) and fin_out (written by the converged fit alone, long before this launch) -- never their
// gpet_scalars: the source's own wave is rewriting those in this very launch, so what is a member and what the source is was decided
// before it, by the ensemble reduction and the src table.
// BAND (gpet_k_band.inc launches it; gpet_band_plan.h): the rows of the source are in ITS band of the last converged fits, the
// destination's image is the band the swap has just moved it to -- every row goes through the offset r0_fit[source] - r0_cur[e]
// (the consensus row: the group shares one band, so the destination's own r0_fit) before the row test against the band's H = E.M rows.
// Without BAND the two tables are not read and the kernel is what it was.
template <bool BAND>
__global__ void __launch_bounds__(64) k_warm_start_src(EdgeDev* edges, int B, const int32_t* __restrict__ src,
                                                       const int32_t* __restrict__ group_of, const char* __restrict__ kept,
                                                       long long record_bytes, long long off_trace, int warm_every,
                                                       const long long* __restrict__ r0_fit, const long long* __restrict__ r0_cur) {
  const int e = blockIdx.x;
  const EdgeDev E = edges[e];
  gpet_scalars* sc = E.sc;  // (the destination's own)
  const int lane = threadIdx.x;
  const int s = (BAND && !src) ? e : src[e];  // (uniform over the wave: every branch on it is; BAND without a table: the edge itself)
  const double* __restrict__ mean = nullptr;
  const long long* __restrict__ cons = nullptr;
  if (s >= 0 && s < B) mean = edges[s].fin_out;
  else if (s == WARM_SRC_CONSENSUS && kept && group_of && group_of[e] >= 0)
    cons = reinterpret_cast<const long long*>(kept + (size_t)group_of[e] * (size_t)record_bytes + (size_t)off_trace);
  const long long last = (long long)E.Lg - 1;  // candidates are grid indices below it
  const double y_max = (double)(E.M - 1);
  const long long yi_max = (long long)E.M - 1;
  long long off = 0;  // (BAND: from the source's band into the destination's; |off| < M, exact as a double)
  if (BAND && (mean || cons)) off = r0_fit[mean ? s : e] - r0_cur[e];
  const double off_d = (double)off;
  auto kept_at = [&](long long k) {  // (k < last) as k_warm_start's; the row from the source
    const long long x = (long long)E.x_st + k;
    bool row_in;
    if (mean) {
      double y = rint(mean[k]);  // (NaN fails both comparisons)
      if (BAND) y += off_d;
      row_in = y >= 0.0 && y <= y_max;
    } else {
      long long y = cons[2 * k];
      if (BAND) y = y < -(1ll << 40) ? y : y + off;  // (INT64_MIN, the NaN median, stays what it is)
      row_in = y >= 0 && y <= yi_max;
    }
    return x > E.x_st && x < E.x_en && row_in;
  };
  long long step = warm_every > 1 ? warm_every : 1;
  int n_keep = 0;
  if (mean || cons) {
    for (;;) {
      int cnt = 0;
      for (long long k0 = step; k0 < last; k0 += step * WAVE) {  // (uniform trip count: every lane reaches the ballot)
        const long long k = k0 + step * lane;
        cnt += __popcll(__ballot(k < last && kept_at(k)));
      }
      n_keep = cnt;
      if (n_keep < E.algo_thresh || n_keep == 0) break;
      step *= 2;  // (ends: no candidate is left once step >= Lg - 1)
    }
    if (n_keep > E.obs_cap) n_keep = E.obs_cap;  // (cannot happen, as in k_warm_start; the stores below stay inside obs_xy)
    int base = 0;
    for (long long k0 = step; k0 < last; k0 += step * WAVE) {
      const long long k = k0 + step * lane;
      const bool take = k < last && kept_at(k);
      const unsigned long long bal = __ballot(take);
      const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
      if (take && pos < n_keep) {
        E.obs_xy[2 * pos] = (long long)E.x_st + k;
        long long y = mean ? (long long)rint(mean[k]) : cons[2 * k];  // (an integer in [0, M - 1]: exact)
        if (BAND) y += off;
        E.obs_xy[2 * pos + 1] = y;
      }
      base += __popcll(bal);
    }
  }
  if (lane == 0) {
    const int iters_done = sc->iter;
    sc->n_obs = n_keep;
    sc->done = (n_keep >= E.algo_thresh) ? 1 : 0;
    sc->status = GPET_OK;
    sc->iter = 0;
    E.wq_tag[0] = 0;
    E.wq_tag[1] = 0;
    if (iters_done >= 1) {
      E.ap_tag[0] = 0;
      E.ap_tag[1] = 0;
      E.ap_tag[2] = 0;
    }
  }
}

hipError_t launch_warm_sources(hipStream_t st, int B, const int32_t* d_group_of, const char* d_kept, long long record_bytes, int from,
                               int32_t* d_src) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_warm_sources, dim3(cdiv(B, 256)), dim3(256), 0, st, B, d_group_of, d_kept, record_bytes, from, d_src);
  return hipGetLastError();
}

hipError_t launch_warm_start_src(hipStream_t st, EdgeDev* d_edges, int B, const int32_t* d_src, const int32_t* d_group_of, const char* d_kept,
                                 long long record_bytes, long long off_trace, int warm_every) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_warm_start_src<false>, dim3(B), dim3(64), 0, st, d_edges, B, d_src, d_group_of, d_kept, record_bytes, off_trace, warm_every,
                     (const long long*)nullptr, (const long long*)nullptr);
  return hipGetLastError();
}
