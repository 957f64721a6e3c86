// Label maps (gpet_label_plan.h, DESIGN section 15): traces rasterised into uint8 masks where the converged fits lie.  Rule 1: the int32
// threshold table of every contributing edge (k_label_thresholds), the maps (k_label_fill), the thickness profiles (k_label_thick).
// Rule 2: the vertices of closed contours traced on polar frames (k_label_vertices), the frame maps (k_label_fill_xy).
//
// Both fill kernels store the same way: a map is its flattened bytes, a lane owns the 16 of them that lie in one 16-byte aligned block of
// the destination, and a wave's 64 lanes own 1 KB in a row -- one global_store_dwordx4 per lane.  N is no multiple of 16 in general, so a
// row end may lie inside a lane's bytes: (row, column) of a byte are stepped, not assumed.  Only the at most two blocks that stick out
// of a map at its ends (a destination that is not 16-byte aligned, a size that is no multiple of 16) are written byte by byte, the
// bytes of the map alone.  Every byte of every map is written by exactly one lane: plain stores, no atomics.

// The threshold table T[u][c] of the contributing edges u (in map order) at every frame column c.  One thread per (u, c).  Stand-alone form
// (le.edge < 0): the caller's rows at rows + le.row_off.  Batch form: t[k] = (int64) rint(mean[k]) + r0_fit[edge] as k_finish_results
// rounds it (int_f64_to_i64: a mean that is not finite gives LABEL_NO_ROW); an edge the device stopped with an error counts nowhere.
__global__ void __launch_bounds__(256) k_label_thresholds(const LabelEdge* __restrict__ le, const long long* __restrict__ rows,
                                                          const EdgeDev* __restrict__ edges, const long long* __restrict__ r0_fit, int M, int N,
                                                          int extend, int* __restrict__ T) {
  const int u = blockIdx.y;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= N) return;
  const LabelEdge L = le[u];
  int t = M;
  const long long k = label_col_index(c, L.x_st, L.len, extend != 0);
  if (k >= 0) {
    if (L.edge < 0) {
      t = label_clamp(rows[L.row_off + k], M);
    } else {
      const EdgeDev& E = edges[L.edge];
      if (E.sc->status == GPET_OK) {
        const long long y = int_f64_to_i64(rint(E.fin_out[k]));
        t = label_clamp(y == LABEL_NO_ROW ? y : y + (r0_fit ? r0_fit[L.edge] : 0ll), M);
      }
    }
  }
  T[(size_t)u * (size_t)N + (size_t)c] = t;
}

// The 16 label bytes v[p] of a lane (packed four to a word in w) to out + j0 .. j0 + 15, of which the map holds [0, total)
__device__ inline void label_store16(unsigned char* __restrict__ out, long long j0, long long total, const unsigned int w[4]) {
  if (j0 >= 0 && j0 + LABEL_CHUNK <= total) {
    *reinterpret_cast<uint4*>(out + j0) = make_uint4(w[0], w[1], w[2], w[3]);
    return;
  }
#pragma unroll
  for (int p = 0; p < LABEL_CHUNK; ++p) {
    const long long j = j0 + p;
    if (j >= 0 && j < total) out[j] = (unsigned char)((w[p >> 2] >> (8 * (p & 3))) & 0xffu);
  }
}

// The maps of Rule 1.  blockIdx.y: the map f; blockIdx.x: LABEL_SPAN flattened bytes of it, counted from the 16-byte boundary at or below
// the destination out0 + out_off[f].  The flattened index is j = r N + c (TR: j = c M + r, the N x M transpose -- lanes then run down
// a column and T_e[c] is uniform over a wave but for the few column ends inside it).  The thresholds of the columns the workgroup covers
// are staged in LDS, G edges at a time ([G][cols]; label_stage_cols / label_stage_edges), once for all of the workgroup's bytes.
template <bool TR>
__global__ void __launch_bounds__(LABEL_THREADS) k_label_fill(const int* __restrict__ T, const int32_t* __restrict__ map_off,
                                                              unsigned char* __restrict__ out0, const long long* __restrict__ out_off, int M,
                                                              int N, int cols, int G) {
  extern __shared__ int s_T[];
  const int f = blockIdx.y;
  const int e0 = map_off[f], n_e = map_off[f + 1] - e0;
  unsigned char* __restrict__ out = out0 + out_off[f];
  const int mis = (int)(reinterpret_cast<size_t>(out) & 15u);
  const long long total = (long long)M * (long long)N;
  const long long wg0 = (long long)blockIdx.x * LABEL_SPAN - mis;
  if (wg0 >= total) return;  // (uniform over the workgroup)
  const long long wg_first = wg0 < 0 ? 0 : wg0;
  const int inner = TR ? M : N;
  // column of staged index 0
  const int cbase = TR ? (int)(wg_first / M) : (N <= LABEL_SPAN ? 0 : (int)(wg_first % N));
  const long long j0 = wg0 + (long long)threadIdx.x * LABEL_CHUNK;
  const long long jf = j0 < 0 ? 0 : j0;
  int r[LABEL_CHUNK], q[LABEL_CHUNK];  // row and staged column of every byte; r < 0: not a byte of the map
  {
    long long major = jf / inner;
    int minor = (int)(jf % inner);
#pragma unroll
    for (int p = 0; p < LABEL_CHUNK; ++p) {
      const long long j = j0 + p;
      r[p] = -1;
      q[p] = 0;
      if (j >= 0 && j < total) {
        const int c = TR ? (int)major : minor;
        r[p] = TR ? minor : (int)major;
        q[p] = TR ? c - cbase : (N <= LABEL_SPAN ? c : (int)(j - wg_first));
        if (++minor == inner) {
          minor = 0;
          ++major;
        }
      }
    }
  }
  unsigned int w[4] = {0u, 0u, 0u, 0u};
  for (int eg = 0; eg < n_e; eg += G) {
    const int g = n_e - eg < G ? n_e - eg : G;
    __syncthreads();  // (the pass before has read its thresholds)
    for (int i = threadIdx.x; i < g * cols; i += LABEL_THREADS) {
      const int gi = i / cols, qq = i - gi * cols;
      const int c = TR ? cbase + qq : (N <= LABEL_SPAN ? qq : (cbase + qq) % N);
      s_T[i] = c < N ? T[(size_t)(e0 + eg + gi) * (size_t)N + (size_t)c] : M;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < LABEL_CHUNK; ++p)
      if (r[p] >= 0) w[p >> 2] += (unsigned int)label_count(s_T + q[p], g, (size_t)cols, r[p]) << (8 * (p & 3));
  }
  label_store16(out, j0, total, w);
}

// thick[f][l][c] for l = 0 .. L: one thread per (map f = blockIdx.y, column c).  With s_0 <= s_1 <= ... the sorted thresholds of the
// map's n edges at c, the rows of label l are [s_(l-1), s_l) with s_(-1) = 0 and s_n = M.  The thread writes S[l] = s_(l-1) into its own
// L + 1 entries -- the rank of every threshold by counting, ties by edge order, so nothing is sorted or kept in scratch; S[l] = M past
// the map's own edges -- then turns them into the differences S[l + 1] - S[l] in ascending l.
__global__ void __launch_bounds__(256) k_label_thick(const int* __restrict__ T, const int32_t* __restrict__ map_off, int M, int N, int L,
                                                     int* thick) {
  const int f = blockIdx.y;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= N) return;
  const int e0 = map_off[f], n_e = map_off[f + 1] - e0;
  const int* __restrict__ Tc = T + (size_t)e0 * (size_t)N + (size_t)c;
  int* th = thick + (size_t)f * (size_t)(L + 1) * (size_t)N + (size_t)c;
  th[0] = 0;
  for (int l = 1; l <= L; ++l) th[(size_t)l * N] = M;
  for (int e = 0; e < n_e; ++e) {
    const int te = Tc[(size_t)e * N];
    int rank = 0;
    for (int o = 0; o < n_e; ++o) {
      const int to = Tc[(size_t)o * N];
      rank += (to < te || (to == te && o < e)) ? 1 : 0;
    }
    th[(size_t)(rank + 1) * N] = te;
  }
  int cur = 0;
  for (int l = 0; l <= L; ++l) {
    const int next = l < L ? th[(size_t)(l + 1) * N] : M;
    th[(size_t)l * N] = next - cur;
    cur = next;
  }
}

// The vertices of the contributing edges of a polar batch: xy[u][j] = (X, Y) of grid index j = 0 .. n_theta - 1 (the seam's second
// column is no vertex) by label_vertex at the row k_label_thresholds would round to.  An edge stopped with an error and a mean that is
// not finite give NaN, which takes the contour out of its map.  cxy: cx [n_centres] | cy [n_centres], the centre of map f is centre f.
__global__ void __launch_bounds__(256) k_label_vertices(const LabelEdge* __restrict__ le, const EdgeDev* __restrict__ edges,
                                                        const long long* __restrict__ r0_fit, const double* __restrict__ cxy, int n_centres,
                                                        const double* __restrict__ cos_t, const double* __restrict__ sin_t, double r0, double dr,
                                                        int n_theta, double* __restrict__ xy) {
  const int u = blockIdx.y;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_theta) return;
  const LabelEdge L = le[u];
  const EdgeDev& E = edges[L.edge];
  double x = NAN, y = NAN;
  if (E.sc->status == GPET_OK) {
    const long long t = int_f64_to_i64(rint(E.fin_out[j]));
    if (t != LABEL_NO_ROW) {
      const int g = n_centres == 1 ? 0 : L.map;
      label_vertex(t + (r0_fit ? r0_fit[L.edge] : 0ll), r0, dr, cxy[g], cxy[n_centres + g], cos_t[j], sin_t[j], &x, &y);
    }
  }
  double* __restrict__ v = xy + 2 * ((size_t)u * (size_t)n_theta + (size_t)j);
  v[0] = x;
  v[1] = y;
}

// The maps of Rule 2, stored like k_label_fill's: a lane owns 16 pixels of the flattened Ms x Ns map.  Per contour of the map the
// workgroup stages the n vertices in LDS (2 n doubles, at most 64 KB) -- a vertex that is not finite is seen there and the contour
// skipped -- and every lane walks the n segments for its pixels with label_crossing: the straddle test rejects almost all of them, and
// a segment that lies wholly above or below the lane's rows is passed over without it.
__global__ void __launch_bounds__(LABEL_THREADS) k_label_fill_xy(const double* __restrict__ xy, const long long* __restrict__ vert_off,
                                                                 const int32_t* __restrict__ n_vert, const int32_t* __restrict__ map_off,
                                                                 int n_vert_max, unsigned char* __restrict__ out0,
                                                                 const long long* __restrict__ out_off, int Ms, int Ns) {
  extern __shared__ double s_xy[];  // [2 n_vert_max], then the flag "this contour has a vertex that is not finite"
  int& s_bad = *reinterpret_cast<int*>(s_xy + 2 * (size_t)n_vert_max);
  const int f = blockIdx.y;
  const int e0 = map_off[f], n_e = map_off[f + 1] - e0;
  unsigned char* __restrict__ out = out0 + out_off[f];
  const int mis = (int)(reinterpret_cast<size_t>(out) & 15u);
  const long long total = (long long)Ms * (long long)Ns;
  const long long wg0 = (long long)blockIdx.x * LABEL_SPAN - mis;
  if (wg0 >= total) return;  // (uniform over the workgroup)
  const long long j0 = wg0 + (long long)threadIdx.x * LABEL_CHUNK;
  const long long jf = j0 < 0 ? 0 : j0;
  double px[LABEL_CHUNK], py[LABEL_CHUNK];
  unsigned int valid = 0u;
  const double py_lo = (double)(jf / Ns);  // the rows of the lane's pixels: py_lo .. py_hi
  double py_hi = py_lo;
  {
    long long row = jf / Ns;
    int col = (int)(jf % Ns);
#pragma unroll
    for (int p = 0; p < LABEL_CHUNK; ++p) {
      const long long j = j0 + p;
      px[p] = 0.0;
      py[p] = 0.0;
      if (j >= 0 && j < total) {
        valid |= 1u << p;
        px[p] = (double)col;
        py[p] = (double)row;
        py_hi = py[p];
        if (++col == Ns) {
          col = 0;
          ++row;
        }
      }
    }
  }
  unsigned int w[4] = {0u, 0u, 0u, 0u};
  for (int e = 0; e < n_e; ++e) {
    const int n = n_vert[e0 + e];
    const double* __restrict__ src = xy + 2 * (size_t)vert_off[e0 + e];
    __syncthreads();  // (the contour before has been walked)
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * n; i += LABEL_THREADS) {
      const double v = src[i];
      s_xy[i] = v;
      if (!label_finite(v)) s_bad = 1;  // (every writer stores the same value)
    }
    __syncthreads();
    if (s_bad) continue;  // (uniform)
    unsigned int in = 0u;
    double xi = s_xy[0], yi = s_xy[1];
#pragma unroll 1
    for (int j = 1; j <= n; ++j) {
      const int k = j == n ? 0 : j;
      const double xj = s_xy[2 * k], yj = s_xy[2 * k + 1];
      // (a segment wholly above or wholly below the lane's rows straddles none of them: the same answer without the 16 tests)
      if (!((yi > py_hi && yj > py_hi) || (!(yi > py_lo) && !(yj > py_lo)))) {
#pragma unroll
        for (int p = 0; p < LABEL_CHUNK; ++p) in ^= (label_crossing(px[p], py[p], xi, yi, xj, yj) ? 1u : 0u) << p;
      }
      xi = xj;
      yi = yj;
    }
    in &= valid;
#pragma unroll
    for (int p = 0; p < LABEL_CHUNK; ++p) w[p >> 2] += ((in >> p) & 1u) << (8 * (p & 3));
  }
  label_store16(out, j0, total, w);
}

// ---- launchers: grids whose y extent is edges or maps go out in launches of at most 65535 -----------------------------------------
hipError_t launch_label_thresholds(hipStream_t st, const LabelEdge* d_le, int n_used, const long long* d_rows, const EdgeDev* d_edges,
                                   const long long* d_r0_fit, int M, int N, bool extend, int* d_T) {
  (void)hipGetLastError();
  for (int i = 0; i < n_used; i += 65535) {
    const int n = n_used - i < 65535 ? n_used - i : 65535;
    hipLaunchKernelGGL(k_label_thresholds, dim3(cdiv(N, 256), n), dim3(256), 0, st, d_le + i, d_rows, d_edges, d_r0_fit, M, N, extend ? 1 : 0,
                       d_T + (size_t)i * (size_t)N);
  }
  return hipGetLastError();
}

hipError_t launch_label_fill(hipStream_t st, const int* d_T, const int32_t* d_map_off, int n_maps, int L, unsigned char* d_out0,
                             const long long* d_out_off, int M, int N, bool transposed) {
  const int cols = label_stage_cols(M, N, transposed);
  const int G = label_stage_edges(cols, L);
  const size_t lds = sizeof(int) * (size_t)G * (size_t)cols;
  const unsigned int blocks = label_blocks((long long)M * (long long)N, 15);
  (void)hipGetLastError();
  for (int i = 0; i < n_maps; i += 65535) {
    const int n = n_maps - i < 65535 ? n_maps - i : 65535;
    if (transposed)
      hipLaunchKernelGGL(k_label_fill<true>, dim3(blocks, n), dim3(LABEL_THREADS), lds, st, d_T, d_map_off + i, d_out0, d_out_off + i, M, N, cols, G);
    else
      hipLaunchKernelGGL(k_label_fill<false>, dim3(blocks, n), dim3(LABEL_THREADS), lds, st, d_T, d_map_off + i, d_out0, d_out_off + i, M, N, cols, G);
  }
  return hipGetLastError();
}

hipError_t launch_label_thick(hipStream_t st, const int* d_T, const int32_t* d_map_off, int n_maps, int M, int N, int L, int* d_thick) {
  (void)hipGetLastError();
  for (int i = 0; i < n_maps; i += 65535) {
    const int n = n_maps - i < 65535 ? n_maps - i : 65535;
    hipLaunchKernelGGL(k_label_thick, dim3(cdiv(N, 256), n), dim3(256), 0, st, d_T, d_map_off + i, M, N, L,
                       d_thick + (size_t)i * (size_t)(L + 1) * (size_t)N);
  }
  return hipGetLastError();
}

hipError_t launch_label_vertices(hipStream_t st, const LabelEdge* d_le, int n_used, const EdgeDev* d_edges, const long long* d_r0_fit,
                                 const double* d_cxy, int n_centres, const double* d_cos, const double* d_sin, double r0, double dr, int n_theta,
                                 double* d_xy) {
  (void)hipGetLastError();
  for (int i = 0; i < n_used; i += 65535) {
    const int n = n_used - i < 65535 ? n_used - i : 65535;
    hipLaunchKernelGGL(k_label_vertices, dim3(cdiv(n_theta, 256), n), dim3(256), 0, st, d_le + i, d_edges, d_r0_fit, d_cxy, n_centres, d_cos,
                       d_sin, r0, dr, n_theta, d_xy + 2 * (size_t)i * (size_t)n_theta);
  }
  return hipGetLastError();
}

hipError_t launch_label_fill_xy(hipStream_t st, const double* d_xy, const long long* d_vert_off, const int32_t* d_n_vert,
                                const int32_t* d_map_off, int n_maps, int n_vert_max, unsigned char* d_out0, const long long* d_out_off, int Ms,
                                int Ns) {
  const size_t lds = 2 * sizeof(double) * (size_t)n_vert_max + 16;
  const unsigned int blocks = label_blocks((long long)Ms * (long long)Ns, 15);
  static PerDeviceOnce once;
  if (once.first()) (void)hipFuncSetAttribute((const void*)k_label_fill_xy, hipFuncAttributeMaxDynamicSharedMemorySize, LABEL_XY_LDS_MAX);
  (void)hipGetLastError();
  for (int i = 0; i < n_maps; i += 65535) {
    const int n = n_maps - i < 65535 ? n_maps - i : 65535;
    hipLaunchKernelGGL(k_label_fill_xy, dim3(blocks, n), dim3(LABEL_THREADS), lds, st, d_xy, d_vert_off, d_n_vert, d_map_off + i, n_vert_max,
                       d_out0, d_out_off + i, Ms, Ns);
  }
  return hipGetLastError();
}
