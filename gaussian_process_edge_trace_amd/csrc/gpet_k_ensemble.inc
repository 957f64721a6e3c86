// Part of gpet_kernels.hip (included there, inside namespace gpet): seed ensembles (include/gpet_hip.h, "seed ensembles"; layout and
// tiling: gpet_ensemble_plan.h) -- the final cost of every edge's converged mean, and per-column order statistics, agreement counts
// and the medoid over the members of a group, made where the converged fits lie (fin_out).

// ---- final costs -------------------------------------------------------------------------------------------------------------
// The cost of a converged mean is the SCORER's cost of that curve: the scoring kernels themselves (k_score_tile + k_score_combine, or
// k_score) run on a VIEW of the batch -- a copy of every EdgeDev whose sample matrix is one row holding the edge's mean, with costs,
// tile partials and scalars of its own --, so the arithmetic is theirs and the loop's buffers are neither read nor written.
// Block e builds view e: the row (pitch Yp, zero beyond the edge; rounded to f32 where the batch stores f32 samples, as a write of
// the samples rounds), the scalars (the edge's own with done = force = 0: the scorer then skips exactly the edges whose status is
// not GPET_OK) and cost[e] = +inf, which is what such an edge keeps.
__global__ void __launch_bounds__(256) k_fincost_view(const EdgeDev* __restrict__ edges, EdgeDev* __restrict__ view, gpet_scalars* __restrict__ view_sc,
                                                      double* __restrict__ rows, size_t row_stride, double* __restrict__ part, size_t part_stride,
                                                      double* __restrict__ cost) {
  const int e = blockIdx.x;
  const EdgeDev& E = edges[e];
  double* const row = rows + (size_t)e * row_stride;
  if (threadIdx.x == 0) {
    EdgeDev V = E;
    gpet_scalars s = *E.sc;
    s.done = 0;
    s.force = 0;
    view_sc[e] = s;
    V.sc = view_sc + e;
    V.Y = row;
    V.S = 1;
    V.costs = cost + e;
    V.cost_part = part + (size_t)e * part_stride;
    view[e] = V;
    cost[e] = INFINITY;
  }
  const int Lg = E.Lg, Yp = E.Yp;
  const double* __restrict__ mean = E.fin_out;
  for (int j = threadIdx.x; j < Yp; j += blockDim.x) {
    const double v = j < Lg ? mean[j] : 0.0;
    if (E.y_f32) reinterpret_cast<float*>(row)[j] = (float)v;
    else row[j] = v;
  }
}

// ---- the ensemble reduction ----------------------------------------------------------------------------------------------------
// Workgroup = one group x one tile of `cols` columns (cols a power of two: 64 up to 64 members, narrower for bigger groups).  Thread t
// owns column t & (cols - 1) and the members t >> log2(cols), + 256 / cols, ... of it, so a wave's load of a member's row is one
// contiguous run of that edge's fin_out block.  Order by counting: rank_i = #{j : v_j < v_i or (v_j == v_i and j < i)}, then
// sorted[rank_i] = v_i in LDS -- n^2 compares per column, no data-dependent loop, nothing that depends on the grid or on the batch's
// other groups.  The statistics are selections from the ordered tile and one exact add and halving.  agree is reduced in LDS, off per
// member in LDS over the tile's columns and then across the tiles by integer atomics into off_acc (zeroed before the launch):
// integers only, so the order of the additions does not matter.
__global__ void __launch_bounds__(ENSEMBLE_THREADS)
k_ensemble(const EdgeDev* __restrict__ edges, const EnsembleGroup* __restrict__ groups, const int32_t* __restrict__ members,
           const int32_t* __restrict__ wg_group, const int32_t* __restrict__ wg_tile, double tol, long long len_cap, EnsembleLayout L,
           char* __restrict__ dst, int* __restrict__ off_acc) {
#pragma clang fp contract(off)
  extern __shared__ double ens_lds[];
  const EnsembleGroup Q = groups[wg_group[blockIdx.x]];
  const int n = Q.n, W = Q.cols, lw = Q.log2_cols, len = Q.len;
  const int k0 = wg_tile[blockIdx.x] * W;
  double* const v = ens_lds;                   // [n][W] as loaded
  double* const srt = v + (size_t)n * W;       // [n][W] ascending per column
  double* const cons = srt + (size_t)n * W;    // [W] rint(median)
  const double** const ptr = reinterpret_cast<const double**>(cons + W);  // [n] the members' means
  int* const agree_l = reinterpret_cast<int*>(ptr + n);                   // [W]
  int* const off_l = agree_l + W;                                         // [n]
  const int tid = threadIdx.x;
  const int32_t* const mem = members + Q.member_off;
  for (int i = tid; i < n; i += ENSEMBLE_THREADS) {
    ptr[i] = edges[mem[i]].fin_out;
    off_l[i] = 0;
  }
  if (tid < W) agree_l[tid] = 0;
  __syncthreads();
  const int c = tid & (W - 1), sl = tid >> lw, nsl = ENSEMBLE_THREADS >> lw;
  const int k = k0 + c;
  const bool col_in = k < len;
  for (int i = sl; i < n; i += nsl) {
    v[i * W + c] = col_in ? ptr[i][k] : 0.0;
    srt[i * W + c] = __longlong_as_double(0x7ff8000000000000ll);  // (a slot no rank reaches -- NaN means -- reads as NaN)
  }
  __syncthreads();
  for (int i = sl; i < n; i += nsl) {
    const double vi = v[i * W + c];
    int rank = 0;
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
      const double vj = v[j * W + c];
      rank += ((vj < vi) || (vj == vi && j < i)) ? 1 : 0;
    }
    srt[rank * W + c] = vi;
  }
  __syncthreads();
  char* const rec = dst + (size_t)wg_group[blockIdx.x] * (size_t)L.record_bytes;
  if (tid < W && col_in) {
    const double mn = srt[c], mx = srt[(n - 1) * W + c];
    const double qlo = srt[((n - 1) / 4) * W + c], qhi = srt[(n - 1 - (n - 1) / 4) * W + c];
    const double med = (srt[((n - 1) / 2) * W + c] + srt[(n / 2) * W + c]) * 0.5;
    const double cc = rint(med);  // round half to even
    cons[c] = cc;
    long long* trace = reinterpret_cast<long long*>(rec + L.off_trace);
    trace[2 * (size_t)k] = int_f64_to_i64(cc);
    trace[2 * (size_t)k + 1] = (long long)Q.x_st + k;
    reinterpret_cast<double*>(rec + L.off_median)[k] = med;
    reinterpret_cast<double*>(rec + L.off_q_lo)[k] = qlo;
    reinterpret_cast<double*>(rec + L.off_q_hi)[k] = qhi;
    reinterpret_cast<double*>(rec + L.off_min)[k] = mn;
    reinterpret_cast<double*>(rec + L.off_max)[k] = mx;
  }
  __syncthreads();
  if (col_in) {
    const double cc = cons[c];
    int ok = 0;
    for (int i = sl; i < n; i += nsl) {
      const double d = fabs(rint(v[i * W + c]) - cc);
      ok += d <= tol ? 1 : 0;
      if (d > tol) atomicAdd(&off_l[i], 1);
    }
    if (ok) atomicAdd(&agree_l[c], ok);
  }
  __syncthreads();
  if (tid < W && col_in) reinterpret_cast<int*>(rec + L.off_agree)[k] = agree_l[c];
  for (int i = tid; i < n; i += ENSEMBLE_THREADS)
    if (off_l[i]) atomicAdd(&off_acc[mem[i]], off_l[i]);
  (void)len_cap;
}

// After k_ensemble: workgroup g < G picks group g's medoid -- smallest off, then smallest final cost, then smallest edge index -- and
// its member of smallest final cost (then smallest edge index) and writes the head; workgroup G writes the per-edge arrays behind
// the records: every edge's final cost, and off for the members, -1 for every other edge.  The order (off, cost, index) is total on
// the members, so the reduction's shape does not matter.
__global__ void __launch_bounds__(ENSEMBLE_THREADS) k_ensemble_pick(const EnsembleGroup* __restrict__ groups, int G, const int32_t* __restrict__ members,
                                                                    const int32_t* __restrict__ member_group, int B, const double* __restrict__ cost,
                                                                    const int* __restrict__ off_acc, double tol, EnsembleLayout L,
                                                                    char* __restrict__ dst) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x == G) {
    double* cost_out = reinterpret_cast<double*>(dst + L.off_cost);
    int* off_out = reinterpret_cast<int*>(dst + L.off_off);
    for (int e = tid; e < B; e += ENSEMBLE_THREADS) {
      cost_out[e] = cost[e];
      off_out[e] = member_group[e] >= 0 ? off_acc[e] : -1;
    }
    return;
  }
  __shared__ int s_off[ENSEMBLE_THREADS], s_e[ENSEMBLE_THREADS], s_be[ENSEMBLE_THREADS];
  __shared__ double s_cost[ENSEMBLE_THREADS], s_bcost[ENSEMBLE_THREADS];
  const EnsembleGroup Q = groups[blockIdx.x];
  const int32_t* const mem = members + Q.member_off;
  int m_off = 0x7fffffff, m_e = -1, b_e = -1;
  double m_cost = 0.0, b_cost = 0.0;
  auto medoid_before = [](int o0, double c0, int e0, int o1, double c1, int e1) {  // is (o0, c0, e0) the better medoid than (o1, c1, e1)?
    if (e1 < 0) return e0 >= 0;
    if (e0 < 0) return false;
    if (o0 != o1) return o0 < o1;
    if (c0 != c1) return c0 < c1;
    return e0 < e1;
  };
  auto cost_before = [](double c0, int e0, double c1, int e1) {
    if (e1 < 0) return e0 >= 0;
    if (e0 < 0) return false;
    if (c0 != c1) return c0 < c1;
    return e0 < e1;
  };
  for (int i = tid; i < Q.n; i += ENSEMBLE_THREADS) {
    const int e = mem[i], o = off_acc[e];
    const double cst = cost[e];
    if (medoid_before(o, cst, e, m_off, m_cost, m_e)) {
      m_off = o;
      m_cost = cst;
      m_e = e;
    }
    if (cost_before(cst, e, b_cost, b_e)) {
      b_cost = cst;
      b_e = e;
    }
  }
  s_off[tid] = m_off;
  s_cost[tid] = m_cost;
  s_e[tid] = m_e;
  s_bcost[tid] = b_cost;
  s_be[tid] = b_e;
  __syncthreads();
  for (int h = ENSEMBLE_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) {
      if (medoid_before(s_off[tid + h], s_cost[tid + h], s_e[tid + h], s_off[tid], s_cost[tid], s_e[tid])) {
        s_off[tid] = s_off[tid + h];
        s_cost[tid] = s_cost[tid + h];
        s_e[tid] = s_e[tid + h];
      }
      if (cost_before(s_bcost[tid + h], s_be[tid + h], s_bcost[tid], s_be[tid])) {
        s_bcost[tid] = s_bcost[tid + h];
        s_be[tid] = s_be[tid + h];
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    gpet_ensemble_head h;
    h.n_members = Q.n;
    h.edge_len = Q.len;
    h.x_st = Q.x_st;
    h.medoid = s_e[0];
    h.best_cost = s_be[0];
    h.reserved = 0;
    h.tol = tol;
    *reinterpret_cast<gpet_ensemble_head*>(dst + (size_t)blockIdx.x * (size_t)L.record_bytes) = h;
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
// cost[e] of every edge's converged mean on stream st.  view / view_sc: [B]; rows: [B][row_stride] doubles, row_stride >= the
// batch's widest row pitch; part: [B][part_stride] doubles, part_stride >= 2 * the scorer's tile count (fincost_part_stride)
size_t fincost_part_stride(const BatchDims& bd) {
  const int n_tiles = score_tiles(bd.Lg);
  return (size_t)2 * (n_tiles > 1 ? n_tiles : 1);
}
hipError_t launch_final_costs(hipStream_t st, const EdgeDev* d_edges, int B, const BatchDims& bd, EdgeDev* d_view, gpet_scalars* d_view_sc,
                              double* d_rows, size_t row_stride, double* d_part, double* d_cost) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_fincost_view, dim3(B), dim3(256), 0, st, d_edges, d_view, d_view_sc, d_rows, row_stride, d_part,
                     fincost_part_stride(bd), d_cost);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the scorer variant the BATCH's shape selects, on one row per edge
  return launch_score_rows(st, d_view, B, bd, 1, false);
}

hipError_t launch_ensemble(hipStream_t st, const EdgeDev* d_edges, int B, int G, const EnsembleGroup* d_groups, const int32_t* d_members,
                           const int32_t* d_member_group, const int32_t* d_wg_group, const int32_t* d_wg_tile, int n_wg, size_t lds,
                           double tol, long long len_cap, const EnsembleLayout& L, const double* d_cost, int* d_off_acc, char* d_dst) {
  (void)hipGetLastError();
  {
    static PerDeviceOnce once;
    if (once.first()) (void)hipFuncSetAttribute((const void*)k_ensemble, hipFuncAttributeMaxDynamicSharedMemorySize, ENSEMBLE_LDS_BUDGET);
  }
  if (n_wg > 0)
    hipLaunchKernelGGL(k_ensemble, dim3(n_wg), dim3(ENSEMBLE_THREADS), lds, st, d_edges, d_groups, d_members, d_wg_group, d_wg_tile, tol,
                       len_cap, L, d_dst, d_off_acc);
  hipLaunchKernelGGL(k_ensemble_pick, dim3(G + 1), dim3(ENSEMBLE_THREADS), 0, st, d_groups, G, d_members, d_member_group, B, d_cost,
                     d_off_acc, tol, L, d_dst);
  return hipGetLastError();
}
