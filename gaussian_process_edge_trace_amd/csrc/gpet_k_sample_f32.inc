// Part of gpet_kernels.hip (included there, inside namespace gpet, after gpet_k_sample_score.inc): the sample GEMM on the f32
// matrix cores, v_mfma_f32_16x16x4_f32 -- gpet_batch_set_sample_arith(GPET_SAMPLE_ARITH_F32), Python sample_dtype="f32mma".
// The arithmetic is a CONTRACT (include/gpet_hip.h), pinned bit for bit by tests/test_gpu_sample_f32mma.py:
//   z = (float)Z[s][k], a = (float)A[k][j]                   round to nearest even, once each
//   acc_0 = +0.0f, acc_{k+1} = fmaf(z_k, a_k, acc_k)         k = 0 .. rank-1 ascending, ONE accumulator per (s, j)
//   Y[s][j] = (float)(((double)acc_rank + mean[j]) * y_s)    the add and the multiply in f64, each rounded
// The instruction is bit for bit that chain over its four k (one rounding per product, nothing wider inside), so: instruction q
// covers k = 4q .. 4q+3, K is never split over accumulators that are added afterwards (latency is hidden by the independent
// OUTPUT tiles of a wave and by the other waves), and where K goes through LDS in chunks the accumulator is carried from chunk to
// chunk.  The steps k >= rank that pad K to the kernel's extent have BOTH operands exactly zero (fmaf(0, 0, acc) = acc): the
// normals and factor rows beyond the rank may hold anything, NaN included.  f32 subnormals are kept (the default kernel mode).
// Operand maps (cdna_hip_programming.md section 3): A lane l <- A[l&15][l>>4], B lane l <- B[l>>4][l&15] as for the f64
// instruction, but D register g of lane l -> row 4 (l>>4) + g, column l&15 (f64: row (l>>4) + 4 g).
// Samples are stored as f32 in the buffer of the f32 storage mode: every consumer is the existing y_f32 instantiation.
typedef float v4f32 __attribute__((ext_vector_type(4)));

// Any capacity (Matern ranks, injected full factors, edges too wide for their mean to sit in LDS): the f32 counterpart of
// k_sample_gemm_mfma.  64x64 output tile per workgroup, wave w owns rows 16w..16w+15 and all 64 columns (4 accumulators of 4 f32
// per lane), K through LDS in chunks of 32, narrowed when staged, the accumulators carried across the chunks.
// Row strides (floats): a ds_read_b32 is served in two groups of 32 lanes over 32 banks.  Factor chunk, 80 (= 16 mod 32): the two
// k-rows a lane group reads (16 consecutive columns each) fall on disjoint bank halves.  Normals, 34 (= 2 mod 32): a group reads
// 16 rows x 2 adjacent k, row i at bank 2i (+ 0 / 1).
__global__ void __launch_bounds__(256) k_sample_f32(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.z];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int Lg = E.Lg, S = E.S, zc = E.z_cols;
  const int s0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  if (s0 >= S || j0 >= Lg) return;
  const int rows = sc->rank;
  const double* __restrict__ Zs = z_slot(E, sc->iter);
  __shared__ float sz[64][34];  // [s][k]
  __shared__ float sa[32][80];  // [k][j]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  v4f32 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (v4f32){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < rows; k0 += 32) {
    for (int e = tid; e < 64 * 32; e += 256) {
      const int kk = e & 31, ss = e >> 5;
      const int k = k0 + kk, sidx = s0 + ss;
      sz[ss][kk] = (k < rows && sidx < S) ? (float)Zs[(size_t)sidx * zc + k] : 0.f;
    }
    for (int e = tid; e < 32 * 64; e += 256) {
      const int jj = e & 63, kk = e >> 6;
      const int k = k0 + kk, j = j0 + jj;
      sa[kk][jj] = (k < rows && j < Lg) ? (float)E.A[(size_t)k * Lg + j] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 32; kk += 4) {
      const float a = sz[16 * w + li][kk + lq];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, sa[kk + lq][16 * t + li], acc[t], 0, 0, 0);
    }
    __syncthreads();
  }
  const double y_s = sc->y_s;
  float* __restrict__ Y = reinterpret_cast<float*>(E.Y);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = j0 + 16 * t + li;
    if (j >= Lg) continue;
    const double mu = E.mean[j];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma clang fp contract(off)
      const int sidx = s0 + 16 * w + 4 * lq + g;
      if (sidx < S) Y[(size_t)sidx * E.Yp + j] = (float)(((double)acc[t][g] + mu) * y_s);
    }
  }
}

// Capacities <= 96 (GEMM_KMAX, the production case), the structure of sample_gemm_body: a wave keeps its 16 rows of Z for the
// whole K extent in registers (KS floats per lane, narrowed on load from the f64 ring), a workgroup is 8 waves = 128 sample rows,
// the K x 64 factor chunk of the current column tile sits in LDS as f32 (narrowed when staged) while the next chunk is in
// flight in registers, the posterior mean sits in LDS as f64 behind the chunk, and the epilogue runs in f64.  Carried over from
// that kernel's comments: the K extent is a template parameter; every global access of the loop is a loop-invariant uniform base
// plus a 32-bit lane offset; EVERY store is issued, a lane whose rows or columns do not exist writes to the spare rows behind the
// matrix; no load or store under a branch inside a trip; the next chunk is staged at the END of a trip.
// Row stride of the chunk in LDS (floats): an operand read is a ds_read_b32, served in two groups of 32 lanes over 32 banks; a
// group reads 16 consecutive floats of TWO k-rows (k = 4q + lq, lq = 0, 1 or 2, 3).  With 80 (= 16 mod 32) the two rows fall on
// disjoint bank halves; 64 or 96 would put them on the same 16 banks, a 2-way conflict on every read.
// (GEMM32_LDA = 80: gpet_iter_plan.h)
template <int KS>
__device__ __forceinline__ void sample_f32_body(const EdgeDev& E, const gpet_scalars* sc, float* s_fb, int part, int cpart, int ncs) {
  const GPET_GLOBAL double* __restrict__ meang = as_global(E.mean);
  constexpr int PF = (KS * 4 * 64) / 512;  // prefetch registers per thread (KS even)
  const int Lg = E.Lg, S = E.S, zc = E.z_cols, Yp = E.Yp;
  const int s0 = part * 128;
  // (the 64-column tiles [jlo, jhi) of this workgroup, as in sample_gemm_body)
  const int tpc = ((Lg + 63) / 64 + ncs - 1) / ncs;
  const int jlo = cpart * tpc * 64;
  const int jhi = (jlo + tpc * 64 < Lg) ? (jlo + tpc * 64) : Lg;
  if (jlo >= Lg) return;
  const int rows = sc->rank;
  const GPET_GLOBAL double* __restrict__ Zs = as_global(z_slot(E, sc->iter));
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int srow = s0 + 16 * w + li;
  float areg[KS];
#pragma unroll
  for (int q = 0; q < KS; ++q) {
    const int k = 4 * q + lq;
    areg[q] = (k < rows && srow < S) ? (float)Zs[(size_t)srow * zc + k] : 0.f;
  }
  const double y_s = sc->y_s;
  double* s_mu = reinterpret_cast<double*>(s_fb + 4 * KS * GEMM32_LDA);  // [Yp] (zero beyond the grid)
  for (int j = tid; j < Yp; j += 512) s_mu[j] = j < Lg ? meang[j] : 0.0;
  // The 64 columns of a tile are dealt to FOUR accumulators by column mod 4: tile column c sits at position 16 (c & 3) + (c >> 2)
  // of a chunk row, so an operand read is still 16 consecutive floats and a lane ends up with FOUR ADJACENT columns (4 li + t in
  // accumulator t) of its four rows 4 lq + g: one 16-byte store per row, and one store instruction writes 4 rows x 256 contiguous
  // bytes -- whole cache lines with the 64-byte multiple row pitch (EdgeDev::Yp), the shape gemm_store.hip measured best in f64.
  // Thread tid stages position tid & 63 (a ds_write_b32 of 32 consecutive floats per lane group: no bank conflict), that is,
  // it loads tile column 4 (tid & 15) + (tid >> 4 & 3): a wave's load is the same 512 contiguous bytes in another lane order.
  // The chunk is loaded WITHOUT bounds, as in sample_gemm_body: the row is clamped to the last factor row and columns beyond
  // the grid (at most 63: the factor buffer is padded by that much) only reach output columns that are never stored; but a row
  // beyond the rank is staged as exact zero, not as the clamped row's value (the contract: both operands zero).
  unsigned aoff[PF];
  {
    const int kmax = rows > 0 ? rows - 1 : 0;
    const int ccol = 4 * (tid & 15) + ((tid >> 4) & 3);
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int kk = (tid >> 6) + 8 * u;
      aoff[u] = (unsigned)(((kk < kmax ? kk : kmax) * Lg + jlo + ccol) * 8);
    }
  }
  const GPET_GLOBAL char* const Ab = (const GPET_GLOBAL char*)as_global(E.A);
  double pf[PF];
#pragma unroll
  for (int u = 0; u < PF; ++u) pf[u] = *(const GPET_GLOBAL double*)(Ab + aoff[u]);
  // (row 16 w + 4 lq, column 4 li: register g of the accumulators is the row g below)
  unsigned yo = (unsigned)(((16 * w + 4 * lq) * Yp + jlo + 4 * li) * 4);
  GPET_GLOBAL char* const Yb = (GPET_GLOBAL char*)as_global(reinterpret_cast<float*>(E.Y)) + (size_t)s0 * Yp * 4;
  const int rlim = S - s0 - (16 * w + 4 * lq);  // row g of this lane exists when g < rlim
  // (spare row g behind the rows rounded up to whole blocks: one offset from the base of row g for every g; 4 rows x 1 KB)
  const unsigned yspare = (unsigned)((((S + 127) & ~127) - s0) * Yp * 4 + lane * 16);
#pragma unroll
  for (int u = 0; u < PF; ++u) s_fb[((tid >> 6) + 8 * u) * GEMM32_LDA + (tid & 63)] = ((tid >> 6) + 8 * u) < rows ? (float)pf[u] : 0.f;
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
    v4f32 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (v4f32){0.f, 0.f, 0.f, 0.f};
    // (one operand base, opaque to the optimiser: every read is that register plus an immediate)
    typedef const __attribute__((address_space(3))) float* lds_cptr;
    lds_cptr bp = (lds_cptr)(s_fb + lq * GEMM32_LDA + li);
    asm volatile("" : "+v"(bp));
#pragma unroll
    for (int q = 0; q < KS; ++q) {
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(areg[q], bp[4 * q * GEMM32_LDA + 16 * t], acc[t], 0, 0, 0);
    }
    const int j = j0 + 4 * li;
    const bool colok = j < Lg;
    // (columns j + 1 .. j + 3 may be padding columns of a grid whose width is no multiple of 4: they land inside the row pitch)
    double mu[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) mu[t] = s_mu[j + t];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma clang fp contract(off)
      v4f32 o;
#pragma unroll
      for (int t = 0; t < 4; ++t) o[t] = (float)(((double)acc[t][g] + mu[t]) * y_s);
      const unsigned at = (colok && g < rlim) ? yo : yspare;
      *(GPET_GLOBAL v4f32*)(Yb + (size_t)g * Yp * 4 + at) = o;
    }
    yo += 64u * 4;
    if (more) {
      __syncthreads();  // this tile's LDS reads are done
#pragma unroll
      for (int u = 0; u < PF; ++u) s_fb[((tid >> 6) + 8 * u) * GEMM32_LDA + (tid & 63)] = ((tid >> 6) + 8 * u) < rows ? (float)pf[u] : 0.f;
      __syncthreads();
    }
  }
}

// One kernel per K extent, as for the f64 form.  Every extent fits the 128 VGPRs that let two workgroups share a CU (the Z rows
// and the accumulators are half the f64 form's registers), so there is no one-workgroup variant.
template <int KS>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) k_sample_f32_r(EdgeDev* edges, int ncs) {
  int edge, part;  // the row blocks of an edge on one XCD: its factor comes out of HBM once, not once per row block
  xcd_edge_part((int)gridDim.x, edge, part);
  const EdgeDev E = edges[edge];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int rparts = (int)gridDim.x / ncs, rp = part % rparts, cp = part / rparts;
  if (rp * 128 >= E.S) return;
  extern __shared__ __attribute__((aligned(16))) float s_fb[];  // [4 KS][GEMM32_LDA], then the mean as f64
  sample_f32_body<KS>(E, sc, s_fb, rp, cp, ncs);
}
