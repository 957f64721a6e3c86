// Part of gpet_kernels.hip (included there, inside namespace gpet, in this order): a6 + a7: sample GEMM on the f64 matrix cores, posterior covariance, curve scoring, the two fused forms, the kept rows, top-k.
// K6 on the matrix cores: v_mfma_f64_16x16x4_f64.  64x64 output tile per workgroup, 4 waves, wave w
// owns rows 16w..16w+15 and all 64 columns (4 accumulators of 4 f64 per lane); K streamed through
// LDS in chunks of 32.  Operand maps (cdna_hip_programming.md section 3): A lane l <- A[l&15][l>>4],
// B lane l <- B[l>>4][l&15]; D register g of lane l -> row (l>>4) + 4g, column l&15.
typedef double v4f64 __attribute__((ext_vector_type(4)));
// The samples are f64 (the reference's; every parity tier is stated on them).  Opt-in (gpet_batch_set_sample_dtype, BASELINE
// config 2's "fp32 posterior samples"): the GEMM rounds each sample to f32 when it stores it and every consumer widens
// it again -- all arithmetic stays f64, the buffer and its HBM traffic halve.  y_ld / y_st: the sites that are not hot.
__device__ __forceinline__ double y_ld(const EdgeDev& E, size_t idx) {
  return E.y_f32 ? (double)reinterpret_cast<const float*>(E.Y)[idx] : E.Y[idx];
}
__device__ __forceinline__ void y_st(const EdgeDev& E, size_t idx, double v) {
  if (E.y_f32) reinterpret_cast<float*>(E.Y)[idx] = (float)v;
  else E.Y[idx] = v;
}
template <bool F32>
struct YT {
  typedef double type;
};
template <>
struct YT<true> {
  typedef float type;
};

__global__ void __launch_bounds__(256) k_sample_gemm_mfma(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.z];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int Lg = E.Lg, S = E.S, zc = E.z_cols;
  const int s0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  if (s0 >= S || j0 >= Lg) return;
  const int rows = sc->rank;
  const double* __restrict__ Zs = z_slot(E, sc->iter);
  __shared__ double sz[64][33];  // [s][k]
  __shared__ double sa[32][65];  // [k][j]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  v4f64 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (v4f64){0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < rows; k0 += 32) {
    for (int e = tid; e < 64 * 32; e += 256) {
      const int kk = e & 31, ss = e >> 5;
      const int k = k0 + kk, sidx = s0 + ss;
      sz[ss][kk] = (k < rows && sidx < S) ? Zs[(size_t)sidx * zc + k] : 0.0;
    }
    for (int e = tid; e < 32 * 64; e += 256) {
      const int jj = e & 63, kk = e >> 6;
      const int k = k0 + kk, j = j0 + jj;
      sa[kk][jj] = (k < rows && j < Lg) ? E.A[(size_t)k * Lg + j] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 32; kk += 4) {
      const double a = sz[16 * w + li][kk + lq];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double b = sa[kk + lq][16 * t + li];
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  const double y_s = sc->y_s;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = j0 + 16 * t + li;
    if (j >= Lg) continue;
    const double mu = E.mean[j];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int sidx = s0 + 16 * w + lq + 4 * g;
      if (sidx < S) y_st(E, (size_t)sidx * E.Yp + j, (acc[t][g] + mu) * y_s);
    }
  }
}

// K6, rank <= 96 (the production case): each wave keeps its 16 rows of Z -- the whole K extent,
// 24 f64 per lane -- in registers for the entire sweep over the columns, so Z is read exactly
// once.  A workgroup is 8 waves = 128 sample rows; the K x 64 chunk of the factor for the
// current column tile sits in LDS (shared by the 8 waves) while the next chunk is already in
// flight from HBM/L2 into registers, so the matrix pipe does not wait for the staging.
// The MFMA loop only runs over the actual rank (rounded up to 4).
// The K extent is a template parameter (KS steps of 4, rank rounded up): a run-time bound inside the
// unrolled MFMA chain makes the compiler copy the accumulators around every step and drain the pipe.
// What bounds it: the 4.1 GB of samples it has to STORE per launch of 1 024 edges.  tools/ubench/gemm_pipe.hip rebuilds
// the loop piece by piece: matrix pipe + LDS operand + barriers + staging run at 68-70 TFLOP/s (1.13 ms); with the
// stores 1.56 ms, and the stores with 1/18 of the MFMAs still 1.51 ms (2.7 TB/s; 2.85 TB/s with 512-byte runs per
// instruction).  Measured slower or equal, and dropped: streaming (nontemporal) stores (+35 %), the chunk by LDS-DMA
// with four 4-wave workgroups per CU (+8 %), a half-tile phase offset between the workgroups of a CU (+-0).
// (GEMM_KMAX, the chunk's row stride GEMM_LDA and GEMM_LDS_MAX: gpet_iter_plan.h)
// MU_LDS (the posterior mean behind the chunk in LDS) is a COMPILE-TIME switch: as a run-time one the mean had two producers --
// an LDS read and a global load into the same registers -- and at their join the compiler waits for BOTH counters: every
// store of a column group then waited (vmcnt(0)) for all the stores before it.
template <int KS, bool F32, bool MU_LDS>
__device__ __forceinline__ void sample_gemm_body(const EdgeDev& E, const gpet_scalars* sc, double* s_fa, int part, int cpart, int ncs) {
  constexpr bool mu_lds = MU_LDS;
  typedef typename YT<F32>::type yt;
  typedef yt yt2 __attribute__((ext_vector_type(2)));
  const GPET_GLOBAL double* __restrict__ meang = as_global(E.mean);
  constexpr int PF = (KS * 4 * 64) / 512;  // prefetch registers per thread (KS even)
  const int Lg = E.Lg, S = E.S, zc = E.z_cols, Yp = E.Yp;
  const int s0 = part * 128;
  // the 64-column tiles [jlo, jhi) of this workgroup: all of them, or one of ncs runs of tiles when few edges leave the
  // GPU empty (a single edge: 8 row blocks x 8 column runs instead of 8 workgroups sweeping 500 columns each)
  const int tpc = ((Lg + 63) / 64 + ncs - 1) / ncs;
  const int jlo = cpart * tpc * 64;
  const int jhi = (jlo + tpc * 64 < Lg) ? (jlo + tpc * 64) : Lg;
  if (jlo >= Lg) return;
  const int rows = sc->rank;
  const GPET_GLOBAL double* __restrict__ Zs = as_global(z_slot(E, sc->iter));
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int srow = s0 + 16 * w + li;
  double areg[KS];
#pragma unroll
  for (int q = 0; q < KS; ++q) {
    const int k = 4 * q + lq;
    areg[q] = (k < rows && srow < S) ? Zs[(size_t)srow * zc + k] : 0.0;
  }
  const double y_s = sc->y_s;
  // the posterior mean sits in LDS behind the chunk: a global load in the epilogue would make every column group
  // wait (vmcnt counts in order) for ALL the stores issued before it
  double* s_mu = s_fa + 4 * KS * GEMM_LDA;  // [Yp] (zero beyond the grid)
  if (mu_lds)
    for (int j = tid; j < Yp; j += 512) s_mu[j] = j < Lg ? meang[j] : 0.0;
  // Addresses: every global access of the loop is a loop-invariant UNIFORM base (scalar registers) plus a 32-bit per-lane
  // byte offset that advances by one tile per trip (global_load/store ... v_off, s[base:base+1]) -- 9 + 2 offset registers.
  // As 64-bit per-lane addresses (9 loads + 8 stores) they took 34 registers, spilled, and every reload was a scratch access
  // in the same in-order queue as the stores.  (The offsets advance, not the bases: an invariant offset is zero-extended
  // outside the loop, where instruction selection no longer sees that its upper half is zero.)
  // The chunk is loaded WITHOUT bounds: element e = tid + 512 u is row kk = e >> 6 (clamped to the last factor row: beyond the
  // rank the normals in areg are exact zeros, any finite factor entry will do), column jj = e & 63 -- columns beyond the grid
  // (at most 63, the last tile's: the factor buffer is padded by that much) only reach output columns that are never
  // stored.
  unsigned aoff[PF];
  {
    const int kmax = rows > 0 ? rows - 1 : 0;
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int kk = (tid >> 6) + 8 * u;
      aoff[u] = (unsigned)(((kk < kmax ? kk : kmax) * Lg + jlo + (tid & 63)) * 8);
    }
  }
  const GPET_GLOBAL char* const Ab = (const GPET_GLOBAL char*)as_global(E.A);
  double pf[PF];
#pragma unroll
  for (int u = 0; u < PF; ++u) pf[u] = *(const GPET_GLOBAL double*)(Ab + aoff[u]);
  // The columns of a 32-column half are dealt to TWO accumulators -- even columns to the first, odd ones to the second (the
  // chunk is staged in that order: column c of the tile at position (c & 32) + 16 (c & 1) + (c >> 1 & 15), so an operand
  // read is still 16 consecutive doubles) -- and a lane ends up with two ADJACENT columns of its four rows: one 16-byte
  // store per row, 4 rows x 256 contiguous bytes per instruction and half the store instructions of one-column lanes.
  // With the 128-byte row pitch (EdgeDev::Yp) every run is whole cache lines: tools/ubench/gemm_store.hip, 1.72 -> 1.42 ms
  // for this loop (pitch alone 1.49, pairs alone 1.58; the epilogue's add and multiply 0.02).
  const int cpos = (tid & 32) + 16 * (tid & 1) + ((tid >> 1) & 15);  // (e & 63 == tid & 63 for every u)
  // EVERY store is issued: a lane whose row (beyond S, last row block) or column pair (beyond the grid, last tile) does not
  // exist writes its 16 bytes to a spare row behind the matrix instead.  A store under a branch has an unknown count, and
  // the wait for the next chunk (issued before this tile's stores, same in-order counter) became a wait for ALL stores.
  constexpr int esz = (int)sizeof(yt);
  unsigned yo0 = (unsigned)(((16 * w + lq) * Yp + jlo + 2 * li) * esz), yo1 = yo0 + 32u * esz;  // (row 16 w + lq, column 32 p + 2 li)
  GPET_GLOBAL char* const Yb = (GPET_GLOBAL char*)as_global(reinterpret_cast<yt*>(E.Y)) + (size_t)s0 * Yp * esz;
  const int rlim = S - s0 - (16 * w + lq);  // row 4 g of this lane exists when 4 g < rlim
  // (spare row 4 g behind the rows rounded up to whole blocks: one offset from the base of row group g for every g)
  const unsigned yspare = (unsigned)((((S + 127) & ~127) - s0) * Yp * esz + lane * 16);
  // The first chunk is staged before the loop and the next one at the END of a trip, after the trip's own stores: the wait
  // for its loads is then "all but the last 8" on every path.  Staged at the head of the trip, the first trip (nothing
  // issued after the loads) and the later ones (8 stores after them) met at the loop head and the wait became vmcnt(0):
  // every tile drained all of its stores before the next one started.
#pragma unroll
  for (int u = 0; u < PF; ++u) s_fa[((tid >> 6) + 8 * u) * GEMM_LDA + cpos] = pf[u];
  __syncthreads();
  for (int j0 = jlo; j0 < jhi; j0 += 64) {
    const bool more = j0 + 64 < jhi;
    if (more) {  // next tile's chunk: loads stay in flight during the MFMAs below
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        aoff[u] += 64 * 8;
        pf[u] = *(const GPET_GLOBAL double*)(Ab + aoff[u]);
      }
    }
    // one 32-column half at a time: its 4 stores go out while the matrix pipe works on the next half
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      v4f64 acc0 = (v4f64){0.0, 0.0, 0.0, 0.0}, acc1 = acc0;
      // (one operand base per half, opaque to the optimiser: every read is that register plus an immediate.  Left alone it
      //  kept a separate address register for every K step -- 17 registers, loop-invariant, and the reason K = 64 spilled)
      typedef const __attribute__((address_space(3))) double* lds_cptr;
      lds_cptr bp = (lds_cptr)(s_fa + lq * GEMM_LDA + li + 32 * p);
      asm volatile("" : "+v"(bp));
#pragma unroll
      for (int q = 0; q < KS; ++q) {
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(areg[q], bp[4 * q * GEMM_LDA], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(areg[q], bp[4 * q * GEMM_LDA + 16], acc1, 0, 0, 0);
      }
      const int j = j0 + 32 * p + 2 * li;
      const bool colok = j < Lg;
      // (column j + 1 may be the first padding column of an odd-width grid: its store lands inside the row pitch)
      double mu0, mu1;
      if (mu_lds) {
        mu0 = s_mu[j];
        mu1 = s_mu[j + 1];
      } else {
        mu0 = meang[colok ? j : 0];
        mu1 = meang[j + 1 < Lg ? j + 1 : 0];
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        yt2 o;
        o.x = (yt)((acc0[g] + mu0) * y_s);
        o.y = (yt)((acc1[g] + mu1) * y_s);
        // (streaming stores, __builtin_nontemporal_store, were measured 35 % slower here)
        const unsigned at = (colok && 4 * g < rlim) ? (p ? yo1 : yo0) : yspare;
        *(GPET_GLOBAL yt2*)(Yb + (size_t)(4 * g) * Yp * esz + at) = o;
      }
    }
    yo0 += 64u * esz;
    yo1 += 64u * esz;
    if (more) {
      __syncthreads();  // this tile's LDS reads are done
#pragma unroll
      for (int u = 0; u < PF; ++u) s_fa[((tid >> 6) + 8 * u) * GEMM_LDA + cpos] = pf[u];
      __syncthreads();
    }
  }
}

// One kernel per K extent (the launcher picks it from the batch's largest possible rank; an edge of smaller
// rank multiplies a few zero rows): register allocation is per kernel, and the variants up to K = 72 fit the
// 128 VGPRs that let two workgroups share a CU, so one's staging and stores overlap the other's MFMAs.
template <int KS, bool F32, bool MU_LDS>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) k_sample_gemm_mfma_r(EdgeDev* edges, int ncs) {
  int edge, part;  // the row blocks of an edge on one XCD: its factor comes out of HBM once, not once per row block
  xcd_edge_part((int)gridDim.x, edge, part);
  const EdgeDev E = edges[edge];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int rparts = (int)gridDim.x / ncs, rp = part % rparts, cp = part / rparts;
  if (rp * 128 >= E.S) return;
  extern __shared__ double s_fa[];  // [4 KS][GEMM_LDA]
  sample_gemm_body<KS, F32, MU_LDS>(E, sc, s_fa, rp, cp, ncs);
}
template <int KS, bool F32, bool MU_LDS>
__global__ void __launch_bounds__(512) k_sample_gemm_mfma_rl(EdgeDev* edges, int ncs) {  // (K > 72: one workgroup per CU)
  int edge, part;
  xcd_edge_part((int)gridDim.x, edge, part);
  const EdgeDev E = edges[edge];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int rparts = (int)gridDim.x / ncs, rp = part % rparts, cp = part / rparts;
  if (rp * 128 >= E.S) return;
  extern __shared__ double s_fa[];
  sample_gemm_body<KS, F32, MU_LDS>(E, sc, s_fa, rp, cp, ncs);
}

// cov = (amp*rho(x*,x*) - V^T V) * y_std^2 on the matrix cores (same tiling as k_sample_gemm_mfma):
// both operands are 32-row chunks of V; only tiles on or above the diagonal are computed and mirrored.
// final_mode: covariance of the converged fit (GaussianProcessRegressor.predict(return_cov=True) on the standardised
// grid, sklearn_gpr.py:398-403) from the V that k_predict<.., FINAL> left behind.
__global__ void __launch_bounds__(256) k_cov_mfma(EdgeDev* edges, int final_mode) {
  const EdgeDev E = edges[blockIdx.z];
  const gpet_scalars* sc = E.sc;
  if (!final_mode && ((sc->done && !sc->force) || sc->status != GPET_OK)) return;
  const int bx = blockIdx.x, by = blockIdx.y;
  if (bx < by) return;
  const int Lg = E.Lg;
  const int r0 = by * 64, c0 = bx * 64;
  if (r0 >= Lg || c0 >= Lg) return;
  const int n = sc->n;
  __shared__ double sr[32][65];  // [i][row j]
  __shared__ double sc_[32][65]; // [i][col j']
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  v4f64 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (v4f64){0.0, 0.0, 0.0, 0.0};
  for (int i0 = 0; i0 < n; i0 += 32) {
    for (int e = tid; e < 32 * 64; e += 256) {
      const int jj = e & 63, ii = e >> 6;
      const int i = i0 + ii;
      sr[ii][jj] = (i < n && r0 + jj < Lg) ? E.V[(size_t)i * Lg + r0 + jj] : 0.0;
      sc_[ii][jj] = (i < n && c0 + jj < Lg) ? E.V[(size_t)i * Lg + c0 + jj] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 32; kk += 4) {
      const double a = sr[kk + lq][16 * w + li];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double b = sc_[kk + lq][16 * t + li];
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  const double amp = sc->amp, s2 = sc->y_std * sc->y_std;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = c0 + 16 * t + li;
    if (c >= Lg) continue;
    const double xoff = final_mode ? E.fin_par[3] : 0.0, xsc = final_mode ? E.fin_par[4] : 1.0;
    const double length = final_mode ? E.fin_par[1] : E.length_scale;
    const double xc = (((double)(E.x_st + c) - xoff) / xsc) / length;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int r = r0 + 16 * w + lq + 4 * g;
      if (r >= Lg) continue;
      if (bx == by && c < r) continue;  // diagonal tile: the mirror write below covers it
      const double k = (r == c) ? amp
                              : amp * ((!final_mode && E.nu_code == 3) ? corr_px(E, (double)r, (double)c, length)
                                                                        : corr_fn(E, (((double)(E.x_st + r) - xoff) / xsc) / length, xc));
      const double val = (k - acc[t][g]) * s2;
      E.cov[(size_t)r * Lg + c] = val;
      E.cov[(size_t)c * Lg + r] = val;
    }
  }
}

// ---------------------------------------------------------------------------------------
// a7  cost of every sampled curve (gpet.py:391-408): one wave per curve, Simpson pairs
//     spread over the lanes.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double grad_at(const float* __restrict__ grad, int M, int N, double y, int x) {
  // RectBivariateSpline(kx=ky=1)(y, x) with integer x: clamped linear interpolation along y
  y = y < 0.0 ? 0.0 : (y > (double)(M - 1) ? (double)(M - 1) : y);
  int iy = (int)floor(y);
  if (iy > M - 2) iy = M - 2;
  if (iy < 0) iy = 0;
  const double w1 = y - (double)iy, w0 = ((double)iy + 1.0) - y;
  const int iy1 = (iy + 1 < M) ? iy + 1 : M - 1;
  return (double)grad[(size_t)iy * N + x] * w0 + (double)grad[(size_t)iy1 * N + x] * w1;
}

// Even number of Simpson samples (odd edge length): scipy >= 1.11 adds Cartwright's correction for the
// last interval, alpha*y[-1] + beta*y[-2] - eta*y[-3] with the last two spacings h0, h1
// (scipy/integrate/_quadrature.py simpson; version dependent in the reference, SURVEY a7).
template <typename T>
__device__ __forceinline__ void simpson_tail(const EdgeDev& E, const T* __restrict__ row, double& al, double& li) {
  const int Lg = E.Lg;
  if ((Lg & 1) == 0 || Lg < 5) return;
  const int k = Lg - 2;  // index of the last sample (N-1); samples are points 0..Lg-2
  const double ya = (double)row[k - 2], yb = (double)row[k - 1], yc = (double)row[k], yd = (double)row[k + 1];
  const double da = yb - ya, db = yc - yb, dc = yd - yc;
  const double l3 = sqrt(1.0 + da * da), l2 = sqrt(1.0 + db * db), l1 = sqrt(1.0 + dc * dc);  // l_{N-3}, l_{N-2}, l_{N-1}
  // arc length: unit spacing h0 = h1 = 1
  al += (5.0 / 12.0) * l1 + (2.0 / 3.0) * l2 - (1.0 / 12.0) * l3;
  // line integral: abscissae are the cumulative lengths -> h0 = l_{N-2}, h1 = l_{N-1}
  const double h0 = l2, h1 = l1;
  const double alpha = (2.0 * h1 * h1 + 3.0 * h0 * h1) / (6.0 * (h1 + h0));
  const double beta = (h1 * h1 + 3.0 * h0 * h1) / (6.0 * h0);
  const double eta = (h1 * h1 * h1) / (6.0 * h0 * (h0 + h1));
  const double g1 = grad_at(E.grad, E.M, E.N, yc, E.x_st + k) + 1e-3;
  const double g2 = grad_at(E.grad, E.M, E.N, yb, E.x_st + k - 1) + 1e-3;
  const double g3 = grad_at(E.grad, E.M, E.N, ya, E.x_st + k - 2) + 1e-3;
  li += alpha * g1 + beta * g2 - eta * g3;
}

// Lane i of a 64-pair chunk owns curve points 2i and 2i+1 (one 16-byte load, fully coalesced);
// the third point of its Simpson pair, that point's gradient value and the following segment
// length are the next lane's own values and arrive by wave shuffle -- each sample, each gather and
// each square root is done exactly once per curve.  (Lane 63 fetches its successor's data itself.)
typedef double v2f64 __attribute__((ext_vector_type(2)));
template <bool F32>
__global__ void __launch_bounds__(256) k_score(EdgeDev* edges) {
  typedef typename YT<F32>::type yt;
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (s >= E.S) return;
  const int Lg = E.Lg;
  const yt* __restrict__ row = reinterpret_cast<const yt*>(E.Y) + (size_t)s * E.Yp;
  const bool aligned = !F32 && ((((size_t)row) & 15) == 0);
  const int npair = (Lg - 2) / 2;  // Simpson over Lg-1 samples (odd count)
  double al = 0.0, li = 0.0;
  for (int i0 = 0; i0 < npair; i0 += WAVE) {
    const int i = i0 + lane;
    const int k = 2 * i;
    // own points: valid while k + 1 < Lg (the lane after the last pair still supplies its data)
    double y0 = 0.0, y1 = 0.0;
    if (k + 1 < Lg) {
      if (aligned) {
        const v2f64 v = *reinterpret_cast<const v2f64*>(row + k);
        y0 = v[0];
        y1 = v[1];
      } else {
        y0 = (double)row[k];
        y1 = (double)row[k + 1];
      }
    }
    // segment length l = sqrt(1 + d^2) and its reciprocal from ONE rsqrt each (the Simpson weights
    // need h1/h0, h0/h1 and hsum^2/(h0 h1): products of the reciprocals instead of three divisions)
    const double d0 = y1 - y0;
    const double q0 = 1.0 + d0 * d0;
    const double r0 = rsqrt(q0), l0 = q0 * r0;
    const double g0 = (k + 1 < Lg) ? grad_at(E.grad, E.M, E.N, y0, E.x_st + k) + 1e-3 : 0.0;
    const double g1 = (k + 1 < Lg) ? grad_at(E.grad, E.M, E.N, y1, E.x_st + k + 1) + 1e-3 : 0.0;
    double y2 = __shfl_down(y0, 1, WAVE), l2 = __shfl_down(l0, 1, WAVE), r2 = __shfl_down(r0, 1, WAVE);
    double g2 = __shfl_down(g0, 1, WAVE);
    if (lane == 63 && i < npair) {  // successor lives in the next chunk
      y2 = (double)row[k + 2];
      const double y3 = (double)row[k + 3];
      const double d2 = y3 - y2;
      const double q2 = 1.0 + d2 * d2;
      r2 = rsqrt(q2);
      l2 = q2 * r2;
      g2 = grad_at(E.grad, E.M, E.N, y2, E.x_st + k + 2) + 1e-3;
    }
    if (i < npair) {
      const double d1 = y2 - y1;
      const double q1 = 1.0 + d1 * d1;
      const double r1 = rsqrt(q1), l1 = q1 * r1;
      al += (2.0 / 6.0) * (l0 + 4.0 * l1 + l2);
      const double h0 = l1, h1 = l2, ih0 = r1, ih1 = r2;
      const double hsum = h0 + h1;
      li += hsum * (1.0 / 6.0) *
            (g0 * (2.0 - h1 * ih0) + g1 * (hsum * hsum * (ih0 * ih1)) + g2 * (2.0 - h0 * ih1));
    }
  }
  al = wave_sum(al);
  li = wave_sum(li);
  if (lane == 0) {
    simpson_tail(E, row, al, li);
    E.costs[s] = al / li;
  }
}

// a7, tiled variant (M <= 1100): a workgroup owns 15 Simpson pairs (32 image columns with the next pair's first) of up to 1024
// curves.  The 32 x M slab of the gradient image is staged in LDS (column-major, odd stride), so the
// 4-tap bilinear gathers -- the L1/TA-bound part of the wave-per-curve kernel -- become LDS reads.
// 16 consecutive lanes share a curve: one coalesced 256-byte read of its samples, successor data
// by shuffle inside the group, group reduction by shuffle, and one (arc, integral) partial per
// (tile, curve); k_score_combine adds the partials in tile order (deterministic) and divides.
// (SC_PAIRS = 15 Simpson pairs per tile, SC_CURVES, SC_THREADS: gpet_iter_plan.h)
// cross-lane moves of a double inside rows of 16 lanes by DPP (two v_mov_b32_dpp; __shfl_xor / __shfl_down with width 16
// go through ds_bpermute and recompute the lane index every time): CTRL = row_ror:8 / row_ror:4 / quad_perm for the
// butterfly, row_shl:1 for "the lane above" (lane 15 of a row has no source and reads 0: its callers replace the value)
template <int CTRL>
__device__ __forceinline__ double dpp_row(double v) {
  const long long b = __double_as_longlong(v);
  // (no "old" operand: a lane without a source -- lane 15 of a row under row_shl:1 -- reads 0 and its callers do not use
  //  the value; with old = the source the compiler copies every operand into the destination first: 24 moves per pair)
  const int lo = __builtin_amdgcn_mov_dpp((int)b, CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, 0xf, 0xf, true);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// 1 / sqrt(x) for x >= 1 (a segment's 1 + d^2): the arithmetic of the device library's rsqrt -- hardware estimate, then
// y + y e (0.5 + 0.375 e) with e = 1 - x y^2 -- without its test for zero / infinite arguments (a v_cmp_class and two
// selects per call in a kernel bound by vector-ALU issue); the same bits for every finite x > 0.
__device__ __forceinline__ double sc_rsqrt(double x) {
#pragma clang fp contract(off)
  const double y0 = __builtin_amdgcn_rsq(x);
  const double e = fma(-y0 * x, y0, 1.0);
  return fma(y0 * e, fma(e, 0.375, 0.5), y0);
}
template <bool F32>
// (eight waves per SIMD = TWO workgroups per CU, their 64 KB slabs side by side: the f64 form took 65 registers, one more than that allows)
__global__ void __launch_bounds__(SC_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) k_score_tile(EdgeDev* edges, int curves_per_wg) {
  typedef typename YT<F32>::type yt;
  // the tiles of an edge on one XCD: neighbouring tiles split cache lines of the sample rows (a tile's 256-byte runs
  // start on 32-byte boundaries), which then come out of HBM once instead of once per L2
  int edge, part;
  xcd_edge_part((int)(gridDim.x * gridDim.y), edge, part);
  const int bx = part % (int)gridDim.x, byy = part / (int)gridDim.x;
  const EdgeDev E = edges[edge];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  extern __shared__ float s_img[];  // [2 * SC_PAIRS + 2][ldm]
  const int M = E.M, N = E.N, Lg = E.Lg, S = E.S;
  const int npair = (Lg - 2) / 2;
  const int p0 = bx * SC_PAIRS;
  if (p0 >= npair) return;
  const int c0 = E.x_st + 2 * p0;   // first image column of the slab
  const int ncol = 2 * SC_PAIRS + 2;
  const int ldm = M | 1;
  const int tid = threadIdx.x;
  for (int e = tid; e < ncol * M; e += SC_THREADS) {
    const int y = e / ncol, c = e - y * ncol;
    const int x = c0 + c;
    s_img[c * ldm + y] = (x < N) ? as_global(E.grad)[(size_t)y * N + x] : 0.f;
  }
  __syncthreads();
  // EIGHT lanes per curve, two consecutive Simpson pairs per lane (round 5; sixteen lanes with one pair each before): a lane holds
  // four consecutive points, so pair A's third point, its gradient value and its following segment are the lane's own (pair
  // B's first), only pair B's come from the lane above by DPP (4 doubles per two pairs instead of 4 per pair), and the two
  // sums over a curve's pairs are one in-lane addition and a three-step butterfly over eight lanes instead of four steps over
  // sixteen: ~36 of ~240 instructions per two pairs less.  Per pair the arithmetic is that of the sixteen-lane form (rounds 2-4); the
  // partial sums of a tile are added in another (fixed) order.
  const int jl = tid & 7;             // lane within the curve: tile pairs 2 jl (A) and 2 jl + 1 (B; 15 = the next tile's first pair: data only)
  const int iA = p0 + 2 * jl, iB = iA + 1;
  const int k = 2 * iA;               // first of the lane's four points
  const bool onA = iA < npair, onB = (2 * jl + 1 < SC_PAIRS) && iB < npair;
  // (curves_per_wg: SC_CURVES, or fewer when few edges leave the GPU empty -- a multiple of the 128 curves of a pass)
  const int s_lo = byy * curves_per_wg;
  const int s_hi = (s_lo + curves_per_wg < S) ? (s_lo + curves_per_wg) : S;
  if (s_lo >= S) return;
  GPET_GLOBAL double* __restrict__ cpart = as_global(E.cost_part) + ((size_t)bx * S) * 2;
  // the samples of the NEXT group of curves are requested before this group is worked on.  EVERY load is issued -- a curve
  // beyond the block re-reads the block's first, points beyond the edge the edge's last four; the select comes after: a load
  // under a branch has a count the compiler does not know, and the wait in front of this group's arithmetic becomes a wait
  // for the prefetch that has just been issued.
  constexpr int CPP = SC_THREADS / 8;  // curves per pass
  // the lane's four points as two adjacent pairs, each clamped into the ROW PITCH on its own (Yp = the edge length rounded up to
  // 16 elements: memory that is there).  A point beyond the edge is read as whatever the padding holds -- it only reaches the
  // sums of pairs that the selects below leave out --, while every point that exists is read as it is: the lane BELOW takes
  // this lane's first point as its pair B's third even when this lane's own pairs lie beyond the edge.
  typedef yt yt2v __attribute__((ext_vector_type(2)));
  const int kA = k < E.Yp - 2 ? k : E.Yp - 2, kB = k + 2 < E.Yp - 2 ? k + 2 : E.Yp - 2;
  auto fetch = [&](int s0, double (&a)[4]) {
    const int s = s0 + (tid >> 3);
    const GPET_GLOBAL yt* __restrict__ row = as_global(reinterpret_cast<const yt*>(E.Y)) + (size_t)(s < s_hi ? s : s_lo) * E.Yp;
    const yt2v vA = *reinterpret_cast<const GPET_GLOBAL yt2v*>(row + kA), vB = *reinterpret_cast<const GPET_GLOBAL yt2v*>(row + kB);
    a[0] = (double)vA.x;
    a[1] = (double)vA.y;
    a[2] = (double)vB.x;
    a[3] = (double)vB.y;
  };
  const float* cols = s_img + (4 * jl) * ldm;  // slab columns of the lane's four points
  // (Two groups ahead was measured too: 1.26 against 1.21 ms per 1 024 edges -- and so was this whole form against the
  //  sixteen-lane one it replaces: 1.204-1.216 against 1.206-1.207 ms in the same run.  A sixth fewer vector instructions and
  //  the same time: the kernel is not bound by vector-ALU issue as rounds 3-4 concluded from SQ_ACTIVE_INST_VALU.)
  double y[4];
  fetch(s_lo, y);
  for (int s0 = s_lo; s0 < s_hi; s0 += CPP) {
    const int s = s0 + (tid >> 3);
    const bool live = s < s_hi;
    double yn[4];
    fetch(s0 + CPP, yn);
    double al, li;
    {
#pragma clang fp contract(off)
      // the 8 taps of the four bilinear lookups first (all LDS reads out before anything needs them), the segment lengths
      // under their latency, then the interpolation (= grad_lds(col, M, y) + 1e-3)
      double yc[4], g[4];
      float ta[4], tb[4];
      int iy[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        yc[t] = fmin(fmax(y[t], 0.0), (double)(M - 1));
        iy[t] = (int)yc[t];
        iy[t] = iy[t] > M - 2 ? M - 2 : iy[t];
        ta[t] = cols[t * ldm + iy[t]];
        tb[t] = cols[t * ldm + iy[t] + 1];
      }
      const double ynx = dpp_row<0x101>(y[0]);  // row_shl:1: the first point of the lane above (= point k + 4)
      double ls[4], rs[4];  // segments 0-1, 1-2, 2-3, 3-next: length and its reciprocal
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double d = (t < 3 ? y[t + 1] : ynx) - y[t];
        const double q = fma(d, d, 1.0);
        rs[t] = sc_rsqrt(q);
        ls[t] = q * rs[t];
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double w1 = yc[t] - (double)iy[t], w0 = ((double)iy[t] + 1.0) - yc[t];
        g[t] = fma((double)tb[t], w1, (double)ta[t] * w0) + 1e-3;
      }
      // pair A = points 0, 1, 2: l0 = ls[0], l1 = ls[1], l2 = ls[2]
      const double aA = (2.0 / 6.0) * (fma(4.0, ls[1], ls[0]) + ls[2]);
      const double hsA = ls[1] + ls[2];
      const double t0A = g[0] * fma(-ls[2], rs[1], 2.0), t1A = g[1] * ((hsA * hsA) * (rs[1] * rs[2])), t2A = g[2] * fma(-ls[1], rs[2], 2.0);
      const double lA = (hsA * (1.0 / 6.0)) * ((t0A + t1A) + t2A);
      // pair B = points 2, 3, next: l0 = ls[2], l1 = ls[3], l2 / r2 / g2 = the lane above's first segment and first point
      const double l2n = dpp_row<0x101>(ls[0]), r2n = dpp_row<0x101>(rs[0]), g2n = dpp_row<0x101>(g[0]);
      const double aB = (2.0 / 6.0) * (fma(4.0, ls[3], ls[2]) + l2n);
      const double hsB = ls[3] + l2n;
      const double t0B = g[2] * fma(-l2n, rs[3], 2.0), t1B = g[3] * ((hsB * hsB) * (rs[3] * r2n)), t2B = g2n * fma(-ls[3], r2n, 2.0);
      const double lB = (hsB * (1.0 / 6.0)) * ((t0B + t1B) + t2B);
      al = (onA ? aA : 0.0) + (onB ? aB : 0.0);
      li = (onA ? lA : 0.0) + (onB ? lB : 0.0);
      // sum over the curve's eight lanes, in every lane: lanes i and 7 - i, then the quads' xor 2 and xor 1
      al += dpp_row<0x141>(al);  // row_half_mirror
      li += dpp_row<0x141>(li);
      al += dpp_row<0x4E>(al);   // quad_perm:[2,3,0,1]
      li += dpp_row<0x4E>(li);
      al += dpp_row<0xB1>(al);   // quad_perm:[1,0,3,2]
      li += dpp_row<0xB1>(li);
    }
    if (jl == 0 && live) {
      cpart[2 * s] = al;
      cpart[2 * s + 1] = li;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) y[t] = yn[t];
  }
}

// the cost of sample s of a tiled launch: its partials added in tile order, the Simpson tail, the division (k_score_combine, k_score_tail)
__device__ __forceinline__ double score_combine_one(const EdgeDev& E, int s) {
  const int my_tiles = ((E.Lg - 2) / 2 + SC_PAIRS - 1) / SC_PAIRS;  // this edge's own tile count
  double al = 0.0, li = 0.0;
  for (int t = 0; t < my_tiles; ++t) {
    al += E.cost_part[((size_t)t * E.S + s) * 2];
    li += E.cost_part[((size_t)t * E.S + s) * 2 + 1];
  }
  if (E.y_f32) simpson_tail(E, reinterpret_cast<const float*>(E.Y) + (size_t)s * E.Yp, al, li);
  else simpson_tail(E, E.Y + (size_t)s * E.Yp, al, li);
  return al / li;
}
__global__ void __launch_bounds__(256) k_score_combine(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= E.S) return;
  E.costs[s] = score_combine_one(E, s);
}

// argsort(costs)[:n_keep] for S <= 1024 by a bitonic sort of (cost, index) in LDS: 55 compare-exchange steps of 512
// pairs instead of S^2 comparisons (rank counting, below: 0.20 ms per 1 024 edges).  Equal costs keep index order (the
// index is the second key); -0.0 and +0.0 compare equal, as `<` on doubles has it.
// the sort itself, (cost, index) ascending over all 1024 entries: 512 compare-exchange pairs per step, one per thread tid < 512.
// ALL_PAIR: the workgroup has exactly those 512 threads (else the others only keep the barriers company).  Entered after a barrier.
template <bool ALL_PAIR>
__device__ __forceinline__ void bitonic_sort_1024(double* s_k, int* s_i, int tid) {
  for (int k = 2; k <= 1024; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (ALL_PAIR || tid < 512) {
        const int i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), l = i | j;
        const double a = s_k[i], b = s_k[l];
        const int ia = s_i[i], ib = s_i[l];
        const bool a_first = (a < b) || (a == b && ia < ib);
        const bool up = (i & k) == 0;
        if (a_first != up) {
          s_k[i] = b;
          s_k[l] = a;
          s_i[i] = ib;
          s_i[l] = ia;
        }
      }
      __syncthreads();
    }
}
__global__ void __launch_bounds__(512) k_topk_sort(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  __shared__ double s_k[1024];
  __shared__ int s_i[1024];
  const int tid = threadIdx.x, S = E.S;
  for (int e = tid; e < 1024; e += 512) {
    s_k[e] = (e < S) ? E.costs[e] : INFINITY;  // (the padding sorts behind every finite cost, and behind +inf by index)
    s_i[e] = e;
  }
  __syncthreads();
  bitonic_sort_1024<true>(s_k, s_i, tid);
  for (int b = tid; b < E.n_keep; b += 512) {
    E.best_idx[b] = s_i[b];
    E.best_costs[b] = s_k[b];
  }
}

// argsort(costs)[:n_keep] by rank counting (ties -> lower index first)       gpet.py:443
__global__ void __launch_bounds__(256) k_topk(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  __shared__ __attribute__((aligned(16))) double s_c[1024];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const double ci = (i < E.S) ? E.costs[i] : 0.0;
  int rank = 0;
  for (int j0 = 0; j0 < E.S; j0 += 1024) {
    __syncthreads();
    // (entries beyond S are +inf: they never rank before a finite cost, and a tie on +inf needs a smaller index)
    for (int e = threadIdx.x; e < 1024; e += blockDim.x) s_c[e] = (j0 + e < E.S) ? E.costs[j0 + e] : INFINITY;
    __syncthreads();
    const int lim = (E.S - j0) < 1024 ? (E.S - j0) : 1024;
    const int lim2 = (lim + 1) & ~1;  // two costs per (broadcast) LDS read
#pragma unroll 4
    for (int e = 0; e < lim2; e += 2) {
      const double2 cj = *reinterpret_cast<const double2*>(&s_c[e]);
      rank += (cj.x < ci) || (cj.x == ci && (j0 + e) < i);
      rank += (cj.y < ci) || (cj.y == ci && (j0 + e + 1) < i && (j0 + e + 1) < E.S);
    }
  }
  if (i < E.S && rank < E.n_keep) {
    E.best_idx[rank] = i;
    E.best_costs[rank] = ci;
  }
}


