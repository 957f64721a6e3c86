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
