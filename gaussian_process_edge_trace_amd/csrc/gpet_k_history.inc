// Iteration history on the device (gpet_batch_set_history; layout: gpet_history_plan.h, include/gpet_hip.h): one launch per loop
// iteration, after the pixel selection, appends the record of that iteration for every edge that completed it -- what
// __call__(return_lines=True) collects on the host per iteration (gpet.py:840-866) without a wait or a copy of the samples.

// Per-column sum over the rows w, w + HISTORY_WAVES, ... of a sample matrix, in ascending row order: sq == false the values, sq ==
// true the squared deviations from `mean`.  One lane per column: a wave's loads of a row are 64 consecutive elements.
template <typename T, bool SQ>
__device__ __forceinline__ double hist_col_part(const T* __restrict__ col, int S, int Yp, int w, double mean) {
#pragma clang fp contract(off)
  double acc = 0.0;
#pragma unroll 8
  for (int r = w; r < S; r += HISTORY_WAVES) {
    const double y = (double)col[(size_t)r * Yp];
    if (SQ) {
      const double d = y - mean;
      acc = acc + d * d;
    } else {
      acc = acc + y;
    }
  }
  return acc;
}

// Grid (history_tiles, edges), HISTORY_WAVES waves.  iter_expect > 0 (the loop): an edge has completed the iteration just enqueued
// exactly when its counter equals iter_expect -- an edge finished earlier, or stopped by an error, stays below it and records
// nothing, in the dead iterations at the end of a group too; an edge that finishes in this very iteration has the counter and gets
// its last record (its `done` flag, just set by k_pix_select, is not looked at).  iter_expect == 0 (gpet_history_record): every
// edge with a counter of at least 1.  The slot is iter - 1; past iter_cap the record is dropped and counted.
// Workgroup 0 of an edge writes the heads, the observations and the optimal curve; with level 3 workgroup t owns the columns
// [64 t, 64 t + 64) of the statistics: two passes (sum, then squared deviations from the mean), each wave over its fixed rows,
// the waves' parts added in wave order through LDS -- no atomics, and nothing depends on the grid or on the edge's place in the table.
__global__ void __launch_bounds__(HISTORY_WAVES * WAVE) k_history(const EdgeDev* __restrict__ edges, gpet_history_plan P, int iter_expect) {
#pragma clang fp contract(off)
  __shared__ double part[HISTORY_WAVES][WAVE];
  const EdgeDev& E = edges[blockIdx.y];
  char* const reg = E.hist;
  if (!reg) return;
  const gpet_scalars* sc = E.sc;
  const int it = sc->iter;  // (nothing in this kernel writes the scalars: every workgroup of the edge decides alike)
  if (iter_expect > 0 ? it != iter_expect : it < 1) return;
  const int tid = threadIdx.x, tile = blockIdx.x;
  gpet_history_edge_head* eh = reinterpret_cast<gpet_history_edge_head*>(reg);
  if (it > P.iter_cap) {
    if (tile == 0 && tid == 0) {
      eh->dropped = it - P.iter_cap;
      eh->n_iter = it;
    }
    return;
  }
  const int Lg = E.Lg < P.len_cap ? E.Lg : P.len_cap, S = E.S, Yp = E.Yp;
  char* const rec = reg + P.off_records + (size_t)(it - 1) * (size_t)P.record_bytes;
  const int best = E.best_idx[0];
  if (tile == 0) {
    int n_obs = sc->n_obs;
    if (n_obs > E.obs_cap) n_obs = E.obs_cap;
    if (tid == 0) {
      gpet_history_head h;
      h.iter = it;
      h.n_obs = sc->n_obs;
      h.best_idx = best;
      h.rank = sc->rank;
      h.n_removed = sc->n_removed;
      h.reserved = 0;
      h.score_thresh = sc->score_thresh;
      h.optimal_cost = E.best_costs[0];
      h.y_s = sc->y_s;
      *reinterpret_cast<gpet_history_head*>(rec) = h;
      eh->n_rec = it;
      eh->n_iter = it;
      eh->edge_len = E.Lg;
    }
    int* obs = reinterpret_cast<int*>(rec + P.off_obs);
    for (int i = tid; i < P.obs_cap; i += blockDim.x) {
      const bool in = i < n_obs;
      obs[2 * i] = in ? (int)E.obs_xy[2 * i] : 0;  // (pixel coordinates: inside the image)
      obs[2 * i + 1] = in ? (int)E.obs_xy[2 * i + 1] : 0;
    }
    if (P.level >= 2) {
      double* curve = reinterpret_cast<double*>(rec + P.off_curve);
      const bool have = best >= 0 && best < S;  // (an injected index outside the samples: no curve)
      for (int k = tid; k < P.len_cap; k += blockDim.x) {
        double y = 0.0;
        if (have && k < Lg)
          y = E.y_f32 ? (double)reinterpret_cast<const float*>(E.Y)[(size_t)best * Yp + k] : E.Y[(size_t)best * Yp + k];
        curve[k] = y;
      }
    }
  }
  if (P.level < 3) return;
  const int lane = tid & (WAVE - 1), w = tid >> 6;
  const int k = tile * HISTORY_COLS + lane;
  const bool col_in = k < Lg;
  const float* __restrict__ Yf = reinterpret_cast<const float*>(E.Y) + k;
  const double* __restrict__ Yd = E.Y + k;
  double p = 0.0;
  if (col_in) p = E.y_f32 ? hist_col_part<float, false>(Yf, S, Yp, w, 0.0) : hist_col_part<double, false>(Yd, S, Yp, w, 0.0);
  part[w][lane] = p;
  __syncthreads();
  double tot = 0.0;
  for (int i = 0; i < HISTORY_WAVES; ++i) tot = tot + part[i][lane];
  const double mean = tot / (double)S;
  __syncthreads();
  p = 0.0;
  if (col_in) p = E.y_f32 ? hist_col_part<float, true>(Yf, S, Yp, w, mean) : hist_col_part<double, true>(Yd, S, Yp, w, mean);
  part[w][lane] = p;
  __syncthreads();
  if (w == 0 && k < P.len_cap) {
    double m2 = 0.0;
    for (int i = 0; i < HISTORY_WAVES; ++i) m2 = m2 + part[i][lane];
    reinterpret_cast<double*>(rec + P.off_mean)[k] = col_in ? mean : 0.0;
    reinterpret_cast<double*>(rec + P.off_std)[k] = col_in ? sqrt(m2 / (double)S) : 0.0;
  }
}
