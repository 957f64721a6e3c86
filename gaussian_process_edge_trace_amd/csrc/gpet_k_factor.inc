// Part of gpet_kernels.hip (included there, inside namespace gpet, in this order): a6, the factor: pivoted Cholesky, Gram matrix, LDS Jacobi (by row index / seated / rotation log), the structured loop path's prior eigenbasis, H and factor rows, round 1's whole-GPU scalar Jacobi.
// ---------------------------------------------------------------------------------------
// a6  factor of the posterior covariance (what numpy's SVD-based multivariate_normal builds)
//     step 1: pivoted Cholesky  cov ~= G^T G  (G rows = columns of the factor), rank-revealing
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) k_pchol(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK || E.factor_injected) return;
  extern __shared__ double s_d[];  // [Lg] remaining diagonal
  __shared__ double s_val[16];
  __shared__ int s_idx[16];
  __shared__ double s_piv;
  __shared__ int s_pidx;
  const int tid = threadIdx.x, bs = blockDim.x, Lg = E.Lg;
  const int lane = tid & 63, w = tid >> 6, nw = bs >> 6;
  for (int i = tid; i < Lg; i += bs) s_d[i] = E.cov[(size_t)i * Lg + i];
  __syncthreads();
  double tol = 0.0;
  int k = 0;
  for (; k < E.r_cap; ++k) {
    // argmax of the remaining diagonal (ties -> smallest index)
    double bv = -1.0;
    int bi = 0x7FFFFFFF;
    for (int i = tid; i < Lg; i += bs) {
      const double v = s_d[i];
      if (v > bv) {
        bv = v;
        bi = i;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(bv, o, WAVE);
      const int oi = __shfl_xor(bi, o, WAVE);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      s_val[w] = bv;
      s_idx[w] = bi;
    }
    __syncthreads();
    if (tid == 0) {
      double v = s_val[0];
      int ix = s_idx[0];
      for (int q = 1; q < nw; ++q)
        if (s_val[q] > v || (s_val[q] == v && s_idx[q] < ix)) {
          v = s_val[q];
          ix = s_idx[q];
        }
      s_piv = v;
      s_pidx = ix;
    }
    __syncthreads();
    const double dp = s_piv;
    const int p = s_pidx;
    if (k == 0) tol = dp * 1e-14;
    if (!(dp > tol) || !(dp > 0.0)) break;
    const double sq = sqrt(dp);
    if (tid == 0) E.perm[k] = p;
    double* s_gp = s_d + Lg;  // [r_cap] the pivot's entries of the previous columns
    for (int t = tid; t < k; t += bs) s_gp[t] = E.G[(size_t)t * Lg + p];
    __syncthreads();
    const double* __restrict__ crow = E.cov + (size_t)p * Lg;  // cov is exactly symmetric: row p == column p
    for (int i = tid; i < Lg; i += bs) {
      double g = 0.0;
      if (s_d[i] >= 0.0) {  // not yet pivoted
        g = crow[i];
        for (int t = 0; t < k; ++t) g -= E.G[(size_t)t * Lg + i] * s_gp[t];
        g = g / sq;
      }
      E.G[(size_t)k * Lg + i] = g;
    }
    __syncthreads();  // all reads of s_d / G row p done before the diagonal is downdated
    for (int i = tid; i < Lg; i += bs) {
      if (i == p) {
        s_d[i] = -1.0;  // mark as used
      } else if (s_d[i] >= 0.0) {
        const double g = E.G[(size_t)k * Lg + i];
        double nd = s_d[i] - g * g;
        s_d[i] = nd > 0.0 ? nd : 0.0;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    sc->rank = k;
    if (k == E.r_cap) {
      // capacity reached: check what is left
      double rem = 0.0;
      for (int i = 0; i < Lg; ++i) rem = s_d[i] > rem ? s_d[i] : rem;
      if (rem > tol * 1e4) sc->status = GPET_ERR_RANK_CAP;
    }
  }
}

// step 1, register-resident variant (Lg <= 512, r_cap <= 96): thread i owns row i of the factor and
// keeps its <= 96 entries in registers (zero until computed), so a step is 96 FMAs against the
// pivot row broadcast from LDS -- no global-load chain.  Same arithmetic order as k_pchol.
// (PCH_R = 96: gpet_factor_plan.h)
__global__ void __launch_bounds__(512) k_pchol_reg(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK || E.factor_injected) return;
  __shared__ double s_d[512];
  __shared__ double s_gp[PCH_R];
  __shared__ double s_val[8];
  __shared__ int s_idx[8];
  __shared__ double s_piv;
  __shared__ int s_pidx;
  const int tid = threadIdx.x, Lg = E.Lg;
  const int lane = tid & 63, w = tid >> 6;
  const bool live = tid < Lg;
  double gown[PCH_R];
#pragma unroll
  for (int t = 0; t < PCH_R; ++t) gown[t] = 0.0;
  double dloc = live ? E.cov[(size_t)tid * Lg + tid] : -1.0;  // remaining diagonal (-1: pivoted / absent)
  s_d[tid] = dloc;
  __syncthreads();
  double tol = 0.0;
  int k = 0;
  const int rcap = E.r_cap < PCH_R ? E.r_cap : PCH_R;
  for (; k < rcap; ++k) {
    double bv = dloc;
    int bi = live ? tid : 0x7FFFFFFF;
    if (!(bv >= 0.0)) {
      bv = -1.0;
      bi = 0x7FFFFFFF;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(bv, o, WAVE);
      const int oi = __shfl_xor(bi, o, WAVE);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      s_val[w] = bv;
      s_idx[w] = bi;
    }
    __syncthreads();
    if (tid == 0) {
      double v = s_val[0];
      int ix = s_idx[0];
      for (int q = 1; q < 8; ++q)
        if (s_val[q] > v || (s_val[q] == v && s_idx[q] < ix)) {
          v = s_val[q];
          ix = s_idx[q];
        }
      s_piv = v;
      s_pidx = ix;
    }
    __syncthreads();
    const double dp = s_piv;
    const int p = s_pidx;
    if (k == 0) tol = dp * 1e-14;
    if (!(dp > tol) || !(dp > 0.0)) break;
    const double sq = sqrt(dp);
    if (tid == p) {
      E.perm[k] = p;
#pragma unroll
      for (int t = 0; t < PCH_R; ++t) s_gp[t] = gown[t];
    }
    __syncthreads();
    double g = 0.0;
    if (live && dloc >= 0.0) {  // not yet pivoted
      g = E.cov[(size_t)p * Lg + tid];  // cov is exactly symmetric: row p == column p
#pragma unroll
      for (int t = 0; t < PCH_R; ++t) g -= gown[t] * s_gp[t];
      g = g / sq;
    }
    if (live) E.G[(size_t)k * Lg + tid] = g;
#pragma unroll
    for (int t = 0; t < PCH_R; ++t) gown[t] = (t == k) ? g : gown[t];
    if (tid == p) {
      dloc = -1.0;
    } else if (dloc >= 0.0) {
      const double nd = dloc - g * g;
      dloc = nd > 0.0 ? nd : 0.0;
    }
    // (s_gp / s_val are rewritten only after the next step's barriers)
  }
  s_d[tid] = dloc;
  __syncthreads();
  if (tid == 0) {
    sc->rank = k;
    if (k == rcap) {
      double rem = 0.0;
      for (int i = 0; i < Lg; ++i) rem = s_d[i] > rem ? s_d[i] : rem;
      if (rem > tol * 1e4) sc->status = GPET_ERR_RANK_CAP;
    }
  }
}

// step 2: Gram matrix C = G G^T (rank x rank)
__global__ void __launch_bounds__(256) k_gram(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.z];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK || E.factor_injected) return;
  const int r = sc->rank, Lg = E.Lg;
  const int a0 = blockIdx.y * 16, b0 = blockIdx.x * 16;
  if (a0 >= r || b0 >= r || b0 > a0) return;
  __shared__ double sa[16][65];
  __shared__ double sb[16][65];
  const int ta = threadIdx.x >> 4, tb = threadIdx.x & 15;
  double acc = 0.0;
  for (int i0 = 0; i0 < Lg; i0 += 64) {
    for (int e = threadIdx.x; e < 16 * 64; e += 256) {
      const int rr = e >> 6, ii = e & 63;
      const int i = i0 + ii;
      sa[rr][ii] = (a0 + rr < r && i < Lg) ? E.G[(size_t)(a0 + rr) * Lg + i] : 0.0;
      sb[rr][ii] = (b0 + rr < r && i < Lg) ? E.G[(size_t)(b0 + rr) * Lg + i] : 0.0;
    }
    __syncthreads();
#pragma unroll 16
    for (int ii = 0; ii < 64; ++ii) acc += sa[ta][ii] * sb[tb][ii];
    __syncthreads();
  }
  const int a = a0 + ta, b = b0 + tb;
  if (a < r && b < r) {
    E.C[(size_t)a * E.r_cap + b] = acc;
    E.C[(size_t)b * E.r_cap + a] = acc;
  }
}

// step 3 (r_cap <= 96): cyclic two-sided Jacobi on the Gram matrix, matrix and rotations resident in LDS, round-robin pair
// ordering (the circle method: pair 0 = (round, m - 1), pair k = (round + k, round - k) mod m - 1), "seated".  Round 1's
// kernel addressed the matrix by ROW INDEX: every round recomputed who meets whom and where their entries live, and wrote
// every off-diagonal block twice (k_jacobi_lds, removed in round 5).  Here the matrix is addressed by SEAT: the players of pair k always
// sit in slots 2k and 2k+1, and after every round each player of the circle moves one seat back (the pivot of pair 0
// stays; after m - 1 rounds everybody is back where they started).  The 2x2 block (pair a, pair b), a <= b, is then a
// FIXED record, and each of its four updated entries goes to a fixed place of the next round's layout, computed once
// per thread before the first sweep.  Only the upper triangle of blocks exists (the matrix is symmetric): no mirrored
// writes, no per-round index arithmetic, and the matrix takes half the space -- 21 KB + 41 KB of W at m = 72, so that TWO
// workgroups of 512 threads share a CU and one's barriers and rotation parameters hide behind the other's LDS work.
//   layout: four planes [r][c] of nblk doubles, block (a <= b) at index b (b + 1) / 2 + a: consecutive threads read and
//           (mostly) write consecutive doubles -- no bank conflicts; diagonal blocks keep [0][0], [0][1], [1][1].
//   W:      W2[ip][player] as 16-byte pairs (components 2 ip, 2 ip + 1 of the player's eigenvector): the lanes of a wave
//           are consecutive pairs, whose players are consecutive -- contiguous, conflict-free 16-byte accesses.
//   round:  read own block, rotate | barrier | write the four entries to next round's places | barrier |
//           last wave: rotation parameters of the next round; the other seven: W of this round | barrier.
// What bounds it: LDS STORES (VGPR -> LDS transfer, ~80 B/clk per CU: 13 cycles per ds_write_b128, 6 per ds_write_b64),
// 62 KB of them per round, two thirds for W.  Tried and measured slower (DESIGN.md section 6): two copies of the
// triangle with 2 barriers (85 KB: one workgroup per CU); 768 threads; W in registers moved along the wave with DPP
// shifts, inside the rounds or as a separate pass over logged rotations (tools/ubench/wpass.hip: VALU-bound at the
// same ~0.8 ms per 1 024 factorisations the LDS form of W costs).
__device__ __forceinline__ int seat_player(int slot, int round, int m1) {  // who sits in `slot` in round `round` (< m1)
  const int k = slot >> 1;
  if (slot & 1) {
    if (k == 0) return m1;
    const int v = m1 - k + round;
    return v >= m1 ? v - m1 : v;
  }
  const int v = k + round;
  return v >= m1 ? v - m1 : v;
}
__device__ __forceinline__ int seat_next_slot(int slot, int m1, int half) {  // where the player of `slot` sits next round
  const int k = slot >> 1;
  if (slot == 1) return 1;  // the pivot
  int seat = (slot & 1) ? m1 - k : k;
  seat = seat == 0 ? m1 - 1 : seat - 1;
  if (seat == 0) return 0;
  return seat < half ? 2 * seat : 2 * (m1 - seat) + 1;
}
// offset (in doubles) of entry (slot i, slot j) of the symmetric matrix in the four-plane triangle
__device__ __forceinline__ int seat_offset(int i, int j, int nblk) {
  int a = i >> 1, b = j >> 1, ri = i & 1, cj = j & 1;
  if (a > b || (a == b && ri > cj)) {
    int t = a; a = b; b = t;
    t = ri; ri = cj; cj = t;
  }
  return (2 * ri + cj) * nblk + b * (b + 1) / 2 + a;
}
__device__ __forceinline__ void seat_block_of(int e, int& a_, int& b_) {  // e = b (b + 1) / 2 + a, a <= b
  b_ = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
  while (b_ * (b_ + 1) / 2 > e) --b_;
  while ((b_ + 1) * (b_ + 2) / 2 <= e) ++b_;
  a_ = e - b_ * (b_ + 1) / 2;
}

// the four entries of the 2 x 2 block (pair a, pair b) after this round's rotations (c_a, s_a) and (c_b, s_b); ONE body
// for every kernel that forms them (contraction off)
__device__ __forceinline__ void jac_rot_block(double b00, double b01, double b10, double b11, double ca, double sa, double cb,
                                              double sb, double (&nv)[4]) {
#pragma clang fp contract(off)
  const double t00 = fma(cb, b00, -(sb * b01)), t01 = fma(sb, b00, cb * b01);
  const double t10 = fma(cb, b10, -(sb * b11)), t11 = fma(sb, b10, cb * b11);
  nv[0] = fma(ca, t00, -(sa * t10));
  nv[2] = fma(sa, t00, ca * t10);
  nv[1] = fma(ca, t01, -(sa * t11));
  nv[3] = fma(sa, t01, ca * t11);
}
// rotation (c, s) that annihilates a_pq of [[app, apq], [apq, aqq]]
__device__ __forceinline__ void jac_params(double app, double apq, double aqq, double& c, double& s) {
  c = 1.0;
  s = 0.0;
  if (fabs(apq) > 1e-300 && apq * apq > 1e-36 * fabs(app * aqq)) {
    // t = sgn(d) h / (|d| + sqrt(d^2 + h^2)): hardware rsqrt / reciprocal + one Newton step (an inexact
    // angle only leaves a ~1e-10 relative residue in a_pq); c = rsqrt(1 + t^2) gets two steps and
    // s = t c, so c^2 + s^2 = 1 to rounding whatever t is
    const double d = aqq - app, hh = 2.0 * apq;
    const double rho2 = d * d + hh * hh;
    double y = __builtin_amdgcn_rsq(rho2);
    y = y * (1.5 - 0.5 * rho2 * y * y);
    const double den = fabs(d) + rho2 * y;
    double iv = __builtin_amdgcn_rcp(den);
    iv = iv * (2.0 - den * iv);
    const double t = (d >= 0.0 ? hh : -hh) * iv;
    const double u = 1.0 + t * t;
    c = __builtin_amdgcn_rsq(u);
    c = c * (1.5 - 0.5 * u * c * c);
    c = c * (1.5 - 0.5 * u * c * c);
    s = t * c;
  }
}

// the same arithmetic without the two branches (the tests select at the end: the same bits; 215 instead of 276 cycles for one
// wave alone, tools/ubench/jac_params_chain.hip) -- for the wave whose chain IS the round (k_jacobi_ahead)
__device__ __forceinline__ void jac_params_nb(double app, double apq, double aqq, double& c, double& s) {
  const bool on = fabs(apq) > 1e-300 && apq * apq > 1e-36 * fabs(app * aqq);
  const double d = aqq - app, hh = 2.0 * apq;
  const double rho2 = d * d + hh * hh;
  double y = __builtin_amdgcn_rsq(rho2);
  y = y * (1.5 - 0.5 * rho2 * y * y);
  const double den = fabs(d) + rho2 * y;
  double iv = __builtin_amdgcn_rcp(den);
  iv = iv * (2.0 - den * iv);
  const double t = (d >= 0.0 ? hh : -hh) * iv;
  const double u = 1.0 + t * t;
  double cc = __builtin_amdgcn_rsq(u);
  cc = cc * (1.5 - 0.5 * u * cc * cc);
  cc = cc * (1.5 - 0.5 * u * cc * cc);
  c = on ? cc : 1.0;
  s = on ? t * cc : 0.0;
}

__device__ __forceinline__ double wp_lane_from_above(double v, double keep) {  // lane k <- lane k + 1 (the last lane keeps `keep`)
  const long long b = __double_as_longlong(v), o = __double_as_longlong(keep);
  const int lo = __builtin_amdgcn_update_dpp((int)o, (int)b, 0x130, 0xf, 0xf, false);  // wave_shl:1
  const int hi = __builtin_amdgcn_update_dpp((int)(o >> 32), (int)(b >> 32), 0x130, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double wp_lane_from_below(double v, double keep) {  // lane k <- lane k - 1 (lane 0 keeps `keep`)
  const long long b = __double_as_longlong(v), o = __double_as_longlong(keep);
  const int lo = __builtin_amdgcn_update_dpp((int)o, (int)b, 0x138, 0xf, 0xf, false);  // wave_shr:1
  const int hi = __builtin_amdgcn_update_dpp((int)(o >> 32), (int)(b >> 32), 0x138, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Warm start of the structured path's eigen-decomposition.  The r0 x r0 matrix H of an iteration differs from the last
// one's by the few observations the iteration added: in the basis of the last eigenvectors W it is already close to
// diagonal, and the cyclic Jacobi that follows needs 4-5 sweeps instead of 6-7 (tests/analysis/jacobi_warm_start.py).
// This kernel forms Cw = W^T C W on the matrix cores (two r0^3 products, 16x16x4 f64 tiles, operands in LDS); k_jacobi_seat
// then starts from Cw with W as its initial eigenvector matrix instead of the identity.  The product rounds to 1e-16 of
// the LARGEST eigenvalue, so the smallest eigenvalues (1e-13 of it) lose relative accuracy a cold start has -- to the
// level LAPACK's SVD of the full covariance (the reference's factor) has anyway.
// jac_warm_source: the eigenvectors of the previous iteration if they are there (same rank), else nullptr (cold start).
__device__ __forceinline__ const double* jac_warm_source(const EdgeDev& E, const gpet_scalars* sc, int warm) {
  const int k = sc->iter, r = sc->rank;
  if (!warm || !E.structured || k < 1) return nullptr;
  const int slot = (k - 1) & 1;
  if (E.wq_tag[slot] != k + 65536 * r) return nullptr;
  return E.Wq + (size_t)slot * E.r_cap * E.r_cap;
}
__device__ __forceinline__ double* jac_warm_slot(const EdgeDev& E, int iter) {  // where iteration `iter` leaves its eigenvectors
  return E.Wq + (size_t)(iter & 1) * E.r_cap * E.r_cap;
}
// One wave per 16-column tile J of the result (NT waves), C and W both in LDS ([k][column] with a row stride = 16 mod 32:
// every operand read is 16 consecutive doubles of four rows on disjoint banks; C is stored symmetric, so its rows serve as
// the A operand's columns).  T[:, J] = C W[:, J] stays in the wave's registers until every wave has finished with C, then
// goes into C's columns J, which only this wave reads in the second product W^T T[:, J].  102 KB at r0 = 72: one workgroup
// per CU, ~10 us each.  (Two earlier forms: 256 threads copying C and W with one dependent load per loop trip -- 0.34 ms
// per launch, as much as the warm start saved; C and W^T as A operands straight from global memory, 16 cache lines per
// load instruction -- 0.14-0.16 ms.)
template <int NT>
__global__ void __launch_bounds__(64 * NT) k_jacobi_prerot(EdgeDev* edges, int warm) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK || E.factor_injected) return;
  const double* Wp = jac_warm_source(E, sc, warm);
  if (!Wp) return;  // (uniform)
  constexpr int mp = 16 * NT, KQ = 4 * NT;
  constexpr int ld = prerot_ld(mp);  // = 16 mod 32
  const int r = sc->rank, ldg = E.r_cap;
  if (r > mp) return;  // (never: the launcher sizes NT for the batch's largest rank)
  extern __shared__ double s_pr[];
  double* s_w = s_pr;            // [mp][ld]: W[i][j] = component i of the eigenvector of player j, zero beyond the rank
  double* s_c = s_pr + mp * ld;  // [mp][ld]: C (symmetric), later T
  const int tid = threadIdx.x, lane = tid & 63, J = tid >> 6, li = lane & 15, lq = lane >> 4;
  {  // both copies: every load of a thread in flight at once (2 mp^2 / (64 NT) = 8 NT of them: a compile-time count)
    constexpr int NLD = (mp * mp) / (64 * NT);
    double wv[NLD], cv[NLD];
    const __attribute__((address_space(1))) double* Wg = (const __attribute__((address_space(1))) double*)Wp;
    const __attribute__((address_space(1))) double* Cg = (const __attribute__((address_space(1))) double*)E.C;
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int e = tid + 64 * NT * u;
      const int i = e / mp, j = e - i * mp;
      const bool in = i < r && j < r;
      const unsigned at = (unsigned)((in ? i : 0) * ldg + (in ? j : 0));
      const double w = Wg[at], c = Cg[at];
      wv[u] = in ? w : 0.0;
      cv[u] = in ? c : 0.0;
    }
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
      const int e = tid + 64 * NT * u;
      const int i = e / mp, j = e - i * mp;
      s_w[i * ld + j] = wv[u];
      s_c[i * ld + j] = cv[u];
    }
  }
  __syncthreads();
  const double* acol = s_c + lq * ld + li;            // A operand of tile row I, K step q: acol[4 q ld + 16 I] (C[k][row] = C[row][k])
  const double* bcol = s_w + lq * ld + 16 * J + li;   // B operand of K step q: bcol[4 q ld]
  v4f64c tacc[NT];
#pragma unroll
  for (int I = 0; I < NT; ++I) {
    v4f64c acc = (v4f64c){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < KQ; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(acol[4 * q * ld + 16 * I], bcol[4 * q * ld], acc, 0, 0, 0);
    tacc[I] = acc;
  }
  __syncthreads();  // every wave has finished with C
#pragma unroll
  for (int I = 0; I < NT; ++I)
#pragma unroll
    for (int g = 0; g < 4; ++g) s_c[(16 * I + lq + 4 * g) * ld + 16 * J + li] = tacc[I][g];
  // (T's columns J: written and read by this wave only -- LDS operations of a wave are ordered; rows beyond the rank are
  //  products with the zero rows of the copies)
  const double* a2 = s_w + lq * ld + li;             // A operand: W^T[16 I + li][k] = W[k][16 I + li]
  const double* b2 = s_c + lq * ld + 16 * J + li;    // B operand: T[k][16 J + li]
#pragma unroll
  for (int I = 0; I < NT; ++I) {
    v4f64c acc = (v4f64c){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < KQ; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a2[4 * q * ld + 16 * I], b2[4 * q * ld], acc, 0, 0, 0);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int i = 16 * I + lq + 4 * g, j = 16 * J + li;
      if (i < r && j < r) E.Cw[(size_t)i * ldg + j] = acc[g];
    }
  }
}

// (JS_NT, JS_LOG_SWEEPS, JA_NT_LOG and the LDS layout of these kernels -- jac_players, jac_blocks, jac_plane_stride, ...: gpet_factor_plan.h)
// LOGW (small batches, where the chain of rounds IS the time): the eigenvectors are not accumulated here -- 41 KB of LDS
// stores a round, 1 200-1 600 of its 2 650 cycles -- but the round's rotations (c, s) go to a log in global memory, and
// k_jacobi_wpass applies them to the rows of W afterwards, one wave per row in registers, on as many CUs as there are rows.
template <int NU, bool LOGW>  // NU blocks per thread: half (half + 1) / 2 <= 1024 up to m = 88, 1176 at m = 96
__global__ void __launch_bounds__(JS_NT) __attribute__((amdgpu_waves_per_eu(4, 4))) k_jacobi_seat(EdgeDev* edges, int scaled_out, int warm) {
  constexpr int NT = JS_NT;
  const EdgeDev E = edges[blockIdx.y];
  gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK || E.factor_injected) return;
  extern __shared__ __attribute__((aligned(16))) double s_mem[];
  __shared__ double s_red[16];
  __shared__ __attribute__((aligned(16))) double2 s_cs[2][48];
  __shared__ int s_pos[96];
  __shared__ double s_theta[96];
  const int r = sc->rank, ldg = E.r_cap;
  const int m = jac_players(r);
  const int half = m >> 1, m1 = m - 1;
  const int nblk = jac_blocks(m);
  double* A0 = s_mem;                                                       // [4][nblk]
  double2* W2 = reinterpret_cast<double2*>(s_mem + 4 * jac_plane_stride(nblk));  // [hl][m]
  const int tid = threadIdx.x;
  const int hl = half;  // component pairs of W in LDS
  if (nblk > NU * NT) {  // (the launcher picks NU from the batch's capacity)
    if (tid == 0) sc->status = GPET_ERR_RANK_CAP;
    return;
  }
  // warm start: the matrix in the basis of the previous iteration's eigenvectors (k_jacobi_prerot), which are then the
  // initial W; else the matrix itself and the identity
  const double* Wp = jac_warm_source(E, sc, warm);
  const double* Cin = Wp ? E.Cw : E.C;
  for (int e = tid; e < nblk; e += NT) {
    int a_, b_;
    seat_block_of(e, a_, b_);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = seat_player(2 * a_ + (q >> 1), 0, m1), j = seat_player(2 * b_ + (q & 1), 0, m1);
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      A0[q * nblk + e] = (hi < r) ? Cin[(size_t)lo * ldg + hi] : 0.0;
    }
  }
  if (!LOGW)
    for (int e = tid; e < hl * m; e += NT) {
      const int ip = e / m, pl = e - ip * m;
      double2 w0 = make_double2(pl == 2 * ip ? 1.0 : 0.0, pl == 2 * ip + 1 ? 1.0 : 0.0);
      if (Wp) w0 = make_double2((2 * ip < r && pl < r) ? Wp[(size_t)(2 * ip) * ldg + pl] : w0.x, (2 * ip + 1 < r && pl < r) ? Wp[(size_t)(2 * ip + 1) * ldg + pl] : w0.y);
      W2[e] = w0;
    }
  double2* jlog = reinterpret_cast<double2*>(E.jlog);
  // fixed roles: blocks tid, tid + NT, ... with the places of their four entries in the next round's layout
  int ba[NU], bb[NU], dst[NU][4];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int e = tid + u * NT;
    seat_block_of(e, ba[u], bb[u]);
    if (e >= nblk) ba[u] = -1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i2 = seat_next_slot(2 * ba[u] + (q >> 1), m1, half), j2 = seat_next_slot(2 * bb[u] + (q & 1), m1, half);
      dst[u][q] = (ba[u] < 0 || (ba[u] == bb[u] && q == 2)) ? -1 : seat_offset(i2, j2, nblk);
    }
  }
  // W workers: the first seven waves, in groups of `half` consecutive threads (thread = pair); group g takes the
  // component pairs g, g + ngrp, ...   The last wave owns the rotation parameters.
  constexpr int WT = NT - 64;
  const int ngrp = half > 0 ? WT / half : 1;
  const int wg = half > 0 ? tid / half : 0, wb = tid - wg * half;
  const bool w_on = tid < WT && wg < ngrp;
  const int pk = tid - WT;
  const int dk = pk * (pk + 1) / 2 + pk;  // diagonal block of pair pk
#ifdef GPET_JAC_TRACE
  double trace_rel = 0.0;
#endif
  auto params = [&](int nxt, int log_round) {
    if (pk >= 0 && pk < half) {
      double c = 1.0, s = 0.0;
      const double app = A0[dk], apq = A0[nblk + dk], aqq = A0[3 * nblk + dk];
#ifdef GPET_JAC_TRACE
      {
        const double den = fabs(app * aqq);
        const double rel2 = den > 0.0 ? apq * apq / den : 0.0;
        trace_rel = rel2 > trace_rel ? rel2 : trace_rel;
      }
#endif
      jac_params(app, apq, aqq, c, s);
      s_cs[nxt][pk] = make_double2(c, s);
      if (LOGW) jlog[(size_t)log_round * half + pk] = make_double2(c, s);
    }
  };
  __syncthreads();
  int sweeps = 0;
#ifdef GPET_JAC_PROF  // cycles per phase of a round, as seen by the first wave and by the parameter wave
  long long pq[7] = {0, 0, 0, 0, 0, 0, 0};
#define JAC_CLK(v) const long long v = clock64()
#else
#define JAC_CLK(v)
#endif
  if (r >= 2) {
    for (int sweep = 0; sweep < 40; ++sweep) {
      double off = 0.0, dg = 0.0;
      for (int e = tid; e < nblk; e += NT) {
        int a_, b_;
        seat_block_of(e, a_, b_);
        const double v00 = A0[e], v01 = A0[nblk + e], v10 = A0[2 * nblk + e], v11 = A0[3 * nblk + e];
        if (a_ == b_) {
          dg += v00 * v00 + v11 * v11;
          off += 2.0 * v01 * v01;
        } else {
          off += 2.0 * ((v00 * v00 + v01 * v01) + (v10 * v10 + v11 * v11));
        }
      }
      off = block_sum(off, s_red);
      dg = block_sum(dg, s_red);
#ifdef GPET_JAC_TRACE
      {
        double tr = trace_rel;
        for (int o = 32; o > 0; o >>= 1) {
          const double ov = __shfl_xor(tr, o, 64);
          tr = ov > tr ? ov : tr;
        }
        if (tid == NT - 64 && (blockIdx.y == 0 || blockIdx.y == 517))
          printf("jac trace blk %d sweep %d: off2/diag2 = %.3e   largest rel2 rotated in the previous sweep = %.3e\n", (int)blockIdx.y, sweep, off / dg, tr);
        trace_rel = 0.0;
      }
#endif
      // quadratic convergence: off^2 <= 1e-24 diag^2 now means <= 1e-48 after one more sweep
      if (off <= 1e-24 * dg || off == 0.0) break;
      ++sweeps;
      params(0, (sweeps - 1) * m1);
      __syncthreads();
      int pb = wb, qb = wb == 0 ? m1 : m1 - wb;  // players of this thread's W pair in round 0
      for (int round = 0; round < m1; ++round) {
        JAC_CLK(q0);
        const double2* cs = s_cs[round & 1];
        double nv[NU][4];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          if (ba[u] < 0) continue;
          const int e = tid + u * NT;
          const double2 ra = cs[ba[u]], rb = cs[bb[u]];
          const double ca = ra.x, sa = ra.y, cb = rb.x, sb = rb.y;
          const double b00 = A0[e], b01 = A0[nblk + e], b11 = A0[3 * nblk + e];
          const double b10 = (ba[u] == bb[u]) ? b01 : A0[2 * nblk + e];
          jac_rot_block(b00, b01, b10, b11, ca, sa, cb, sb, nv[u]);
        }
        JAC_CLK(q1);
        __syncthreads();  // every block has been read
        JAC_CLK(q2);
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (ba[u] >= 0 && dst[u][q] >= 0) A0[dst[u][q]] = nv[u][q];
        JAC_CLK(q3);
        __syncthreads();
        JAC_CLK(q4);
        if (!LOGW && w_on) {  // W: rotate the eigenvector entries of players pb, qb (needs only this round's cs)
          const double2 rb = cs[wb];
          const double cb = rb.x, sb = rb.y;
          if (sb != 0.0) {
            // three component pairs per pass, all loads first: the LDS latency is paid once per pass
            constexpr int BD = 3;
            for (int ip0 = wg; ip0 < hl; ip0 += BD * ngrp) {
              double2 wp[BD], wq[BD];
#pragma unroll
              for (int t = 0; t < BD; ++t) {
                const int ip = ip0 + t * ngrp;
                if (ip < hl) {
                  wp[t] = W2[ip * m + pb];
                  wq[t] = W2[ip * m + qb];
                }
              }
#pragma unroll
              for (int t = 0; t < BD; ++t) {
                const int ip = ip0 + t * ngrp;
                if (ip < hl) {
                  // (spelled out: k_jacobi_wpass does exactly this arithmetic)
                  W2[ip * m + pb] = make_double2(fma(cb, wp[t].x, -(sb * wq[t].x)), fma(cb, wp[t].y, -(sb * wq[t].y)));
                  W2[ip * m + qb] = make_double2(fma(sb, wp[t].x, cb * wq[t].x), fma(sb, wp[t].y, cb * wq[t].y));
                }
              }
            }
          }
        }
        if (round + 1 < m1) params((round + 1) & 1, (sweeps - 1) * m1 + round + 1);
        JAC_CLK(q5);
        __syncthreads();
#ifdef GPET_JAC_PROF
        const long long q6 = clock64();
        pq[0] += q1 - q0; pq[1] += q2 - q1; pq[2] += q3 - q2; pq[3] += q4 - q3; pq[4] += q5 - q4; pq[5] += q6 - q5; pq[6] += q6 - q0;
#endif
        // next round: everybody on the circle is one player further
        pb = pb + 1 >= m1 ? 0 : pb + 1;
        if (wb != 0) qb = qb + 1 >= m1 ? 0 : qb + 1;
      }
    }
  }
  // back in the initial seats: slot -> player of round 0
  for (int k = tid; k < half; k += NT) {
    const int d = k * (k + 1) / 2 + k;
    s_theta[seat_player(2 * k, 0, m1)] = A0[d];
    s_theta[seat_player(2 * k + 1, 0, m1)] = A0[3 * nblk + d];
  }
  __syncthreads();
  for (int k = tid; k < r; k += NT) E.theta[k] = s_theta[k];
  const double* Wd = reinterpret_cast<const double*>(W2);  // W[j][i] = Wd[((i >> 1) * m + j) * 2 + (i & 1)]
  const int r_lds = 2 * hl < r ? 2 * hl : r;  // components in LDS
  // (the eigenvectors also into this iteration's slot of the ring the next iteration's warm start reads)
  double* Wk = jac_warm_slot(E, sc->iter);
  if (!LOGW)
    for (int e = tid; e < r_lds * r; e += NT) {
      const int i = e / r, j = e - i * r;
      const double v = Wd[((i >> 1) * m + j) * 2 + (i & 1)];
      E.W[(size_t)i * ldg + j] = v;
      Wk[(size_t)i * ldg + j] = v;
    }
  if (!LOGW && tid == 0 && E.structured) E.wq_tag[sc->iter & 1] = (sc->iter + 1) + 65536 * r;
  for (int k = tid; k < r; k += NT) {
    const double v = s_theta[k];
    int pos = 0;
    for (int j = 0; j < r; ++j) {
      const double u = s_theta[j];
      pos += (u > v) || (u == v && j < k);
    }
    E.order[pos] = k;
    s_pos[k] = pos;
  }
  __syncthreads();
  // structured path (scaled_out): G (unused there) <- eigenvectors in descending eigenvalue order, scaled by
  // y_std sqrt(theta): column pos of row t is the coefficient of basis vector t in factor row pos
  if (scaled_out && !LOGW) {
    for (int e = tid; e < r_lds * r; e += NT) {
      const int i = e / r, j = e - i * r;
      const double th = s_theta[j];
      E.G[(size_t)i * ldg + s_pos[j]] = Wd[((i >> 1) * m + j) * 2 + (i & 1)] * (sc->y_std * sqrt(th > 0.0 ? th : 0.0));
    }
  }
  if (tid == 0) sc->lml = (double)sweeps;  // diagnostics: Jacobi sweeps of this factorisation
#ifdef GPET_JAC_PROF
  if ((tid == 0 || tid == NT - 64) && (blockIdx.y == 0 || blockIdx.y == 700) && sweeps > 0) {
    const double n = (double)sweeps * m1;
    printf("jac prof blk %d tid %d: per round: read+rotate %.0f | wait %.0f | write %.0f | wait %.0f | W / params %.0f | wait %.0f | total %.0f cycles\n",
           (int)blockIdx.y, tid, pq[0] / n, pq[1] / n, pq[2] / n, pq[3] / n, pq[4] / n, pq[5] / n, pq[6] / n);
  }
#endif
#undef JAC_CLK
}

// ---- the same cyclic Jacobi with the rotation parameters ONE ROUND AHEAD (round 5) ------------------------------------------
// k_jacobi_seat's round is read + rotate | barrier | write | barrier | parameters of the next round (one wave, a dependent
// chain of three transcendentals) | barrier: 1 770 cycles in the rotation-log form (rocprofv3: 314 us for 426 rounds), of which
// the blocks are idle for the last third and the parameter wave for the first two.  But the parameters of round g + 1 do not
// need round g's RESULT in LDS: the diagonal block of a pair of the next seating consists of three entries that round g's
// rotations produce from three blocks of the CURRENT layout -- (a, a), (b, b) and (a, b) for the two pairs a, b its players
// sit in now -- and the rotations of round g are known when the round starts.  So here the last wave forms those entries
// itself (the owners' arithmetic, jac_rot_entry) and the parameters of round g + 1 from them WHILE the other waves rotate the
// blocks of round g; the matrix is double-buffered (read layout g from one copy, write layout g + 1 into the other: 2 x 21 KB
// at rank 72), so a round is ONE barrier.
//   Parameter wave (lane k = pair k): it KEEPS the diagonal block and the rotation of its pair in registers from round to
//   round and publishes, next to the rotation, the pair's two diagonal entries AFTER that rotation.  The players of pair k of
//   the next seating are the top player of pair k + 1 and the bottom player of pair k - 1 (the circle moves one seat a round;
//   its two ends and the pivot take their own), so a lane reads two published diagonal entries, the two neighbours' rotations
//   and the one block that holds its pair's future off-diagonal entry: 8 reads at fixed per-lane addresses, issued first
//   thing after the barrier; then 6 multiply-adds, the branchless parameter chain (215 cycles alone on a SIMD,
//   tools/ubench/jac_params_chain.hip), three 16-byte writes.  No exec-mask branch in it: idle lanes compute on zeros and write
//   to a spare record / a spare row of the log.
//   Workers: the 2 x 2 blocks of k_jacobi_seat, with EVERY LDS address of a round a per-thread constant for the round's parity
//   (two address sets, the round loop is two copies of one body): no address arithmetic, no masked writes (an entry that is
//   not stored goes to a dump slot).
// What a round costs now (rank 72, rotation-log form, rocprofv3): ~1 070 cycles (190-200 us for 426 rounds; 1 350 before the
// address tables and the branchless chain).  tools/ubench/round_skeleton.hip puts the floor of this structure -- 8 reads ->
// chain -> 3 writes -> barrier, with the other waves' LDS traffic beside it -- at ~620-700 cycles; the rest is the second
// multiply-add stage (the published diagonal) behind the chain and the interleaving of eight waves on one LDS.
// Measured on the way and dropped: all 10 matrix entries gathered by the parameter wave (14 reads, same time: the chain, not
// the gather, was the round); the diagonal entries from the neighbouring lanes by whole-wave DPP shifts (same time; a pair of
// v_mov_b32_dpp wave_shl costs 12 cycles, tools/ubench/lane_shift.hip); 4 x 4 super-blocks on three worker waves (half the
// reads of rotations, a SIMD per wave: 16 reads + 48 multiply-adds + 16 writes are ~200 instructions of ONE wave's stream,
// 1 550-1 720 cycles a round); 5, 7, 11 or 15 worker waves (within 5 %); workers held back by s_sleep so that the parameter
// wave's reads reach the LDS first (no gain).  In-kernel cycle stamps mislead here: s_memtime returns through the same counter
// as LDS reads, so a stamp in front of an `s_waitcnt lgkmcnt(0)` makes that wait ~300 cycles longer.
// The pairs and their order are those of k_jacobi_seat and every rotation is formed from the same three numbers: eigenvalues
// and eigenvectors agree to rounding (1e-12 of the largest factor entry: the tests compare the two forms), traces are
// identical.  (c, s) records are six doubles (c, -s, s, c, d0', d1'): the half an EVEN seat's row or column needs is the first
// pair, an odd seat's the second -- one 16-byte read by parity instead of selects.
__device__ __forceinline__ int seat_prev_slot(int slot, int m1, int half) {  // inverse of seat_next_slot
  if (slot == 1) return 1;  // the pivot
  const int k = slot >> 1;
  int seat = ((slot & 1) ? m1 - k : k) + 1;  // the seat it came from: one on along the circle
  if (seat >= m1) seat = 0;
  return seat < half ? 2 * seat : 2 * (m1 - seat) + 1;
}
// entry (row seat of parity pr, column seat of parity pc) of a rotated 2 x 2 block: (xr, yr) / (xc, yc) = the parity's half
// of the row / column pair's record.  Spelled like jac_rot_block: the same bits as its nv[2 pr + pc].
__device__ __forceinline__ double jac_rot_entry(double b00, double b01, double b10, double b11, double xr, double yr, double xc, double yc) {
#pragma clang fp contract(off)
  const double t0 = fma(xc, b00, yc * b01), t1 = fma(xc, b10, yc * b11);
  return fma(xr, t0, yr * t1);
}

// RR > 0: the LAST 7 RR components of the eigenvectors (rows of W) are not in LDS but in the registers of the seven worker
// waves -- wave w rows 2 hl + w, 2 hl + w + 7, ..., lane k the pair k of the seating, exactly k_jacobi_wpass's form and
// arithmetic (rotate (x, y) by the pair's (c, s), then everybody on the circle moves one seat on by whole-wave DPP shifts).
// LDS stores bound the round and two thirds of them are W's; the register rows cost vector instructions instead, which the
// round has to spare: the two resources share W.
template <int NU, bool LOGW, int RR, int NTHR, bool PARAM>
__device__ __forceinline__ void ja_run(const EdgeDev& E, gpet_scalars* sc, int scaled_out, int warm, double* s_mem, double* s_red, double (*s_cs)[49][6], int* s_pos, double* s_theta);
template <int NU, bool LOGW, int RR, int NTHR, bool PARAM>  // PARAM: the parameter wave's copy of the body, else the workers'
__device__ __forceinline__ void ja_run(const EdgeDev& E, gpet_scalars* sc, int scaled_out, int warm, double* s_mem, double* s_red,
                                       double (*s_cs)[49][6], int* s_pos, double* s_theta) {
  constexpr int NT = NTHR, WT = NT - 64;
  // (readfirstlane: the rank comes out of memory through a vector load, and everything derived from it -- the round count, the
  //  round's parity -- would be "divergent" to the compiler: the round loop then runs on exec masks, the parity branch as two
  //  saveexec regions per round: 0.263 -> 0.252 ms per eigen stage of one edge.  Not in the big-batch form, which holds the
  //  eigenvector rows in registers: with a scalar loop it needs 106 scalar registers, spills 15 of them into vector lanes and
  //  runs 1.61 instead of 1.47 ms per 1 024 edges)
  const int r = LOGW ? __builtin_amdgcn_readfirstlane(sc->rank) : sc->rank, ldg = E.r_cap;
  // (m and nreg below are jac_players(r) and jac_reg_rows(RR, m) of gpet_factor_plan.h as text: through either function the compiler
  //  emits k_jacobi_ahead<2, false, 6>, the bench's kernel, one instruction longer.  Nothing but reading holds the two to the header.)
  const int m = (r + 1) & ~1;
  const int half = m >> 1, m1 = m - 1;
  const int nblk = jac_blocks(m);
  const int nbp = jac_plane_stride(nblk);                                      // plane stride
  const int bst = jac_ahead_copy_stride(nbp);                                  // copy stride: four planes + the dump slot
  double* A0 = s_mem;                                                          // [2][4 nbp + 2]
  double2* W2 = reinterpret_cast<double2*>(s_mem + 2 * bst);                   // [hl][m]
  const int tid = threadIdx.x;
  const int nreg = (LOGW || RR == 0) ? 0 : ((7 * RR < m ? 7 * RR : m) & ~1);
  const int hl = LOGW ? half : (m - nreg) >> 1;
  if (nblk > NU * WT) {  // (the launcher picks NU from the batch's capacity)
    if (tid == 0) sc->status = GPET_ERR_RANK_CAP;
    return;
  }
  const double* Wp = jac_warm_source(E, sc, warm);
  const double* Cin = Wp ? E.Cw : E.C;
  for (int e = tid; e < nblk; e += NT) {
    int a_, b_;
    seat_block_of(e, a_, b_);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = seat_player(2 * a_ + (q >> 1), 0, m1), j = seat_player(2 * b_ + (q & 1), 0, m1);
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      A0[q * nbp + e] = (hi < r) ? Cin[(size_t)lo * ldg + hi] : 0.0;
    }
  }
  if (!LOGW)
    for (int e = tid; e < hl * m; e += NT) {
      const int ip = e / m, pl = e - ip * m;
      double2 w0 = make_double2(pl == 2 * ip ? 1.0 : 0.0, pl == 2 * ip + 1 ? 1.0 : 0.0);
      if (Wp) w0 = make_double2((2 * ip < r && pl < r) ? Wp[(size_t)(2 * ip) * ldg + pl] : w0.x, (2 * ip + 1 < r && pl < r) ? Wp[(size_t)(2 * ip + 1) * ldg + pl] : w0.y);
      W2[e] = w0;
    }
  // register rows of the worker waves (RR > 0): component 2 hl + wave + 7 t; lane k = pair k (k_jacobi_wpass's form)
  constexpr int RN = RR > 0 ? RR : 1;
  double rx[RN], ry[RN];
  const int rlane = tid & 63, rwave = tid >> 6;
  const bool r_lane_on = rlane < half, r_lane0 = rlane == 0, r_lane_last = rlane == half - 1;
  const int r_pe = seat_player(2 * rlane, 0, m1), r_po = seat_player(2 * rlane + 1, 0, m1);
#pragma unroll
  for (int t = 0; t < RN; ++t) {
    const int i = 2 * hl + rwave + 7 * t;
    rx[t] = (RR > 0 && r_lane_on && r_pe == i) ? 1.0 : 0.0;
    ry[t] = (RR > 0 && r_lane_on && r_po == i) ? 1.0 : 0.0;
    if (RR > 0 && Wp && r_lane_on && i < r) {
      if (r_pe < r) rx[t] = Wp[(size_t)i * ldg + r_pe];
      if (r_po < r) ry[t] = Wp[(size_t)i * ldg + r_po];
    }
  }
  // workers: blocks tid, tid + WT, ... with the places of their four entries in the next round's layout
  int ba[NU], bb[NU], dst[NU][4];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int e = tid + u * WT;
    seat_block_of(e < nblk ? e : 0, ba[u], bb[u]);
    if (e >= nblk || tid >= WT) ba[u] = -1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i2 = seat_next_slot(2 * ba[u] + (q >> 1), m1, half), j2 = seat_next_slot(2 * bb[u] + (q & 1), m1, half);
      const int so = seat_offset(i2, j2, nblk);  // (plane * nblk + index: re-based on the padded plane stride)
      // (an entry that is not stored -- the [1][0] entry of a diagonal block -- goes to a dump slot behind the planes: four
      //  unconditional writes instead of four exec-masked ones)
      dst[u][q] = (ba[u] < 0 || (ba[u] == bb[u] && q == 2)) ? 4 * nbp : (so / nblk) * nbp + (so - (so / nblk) * nblk);
    }
  }
  // Every LDS access of a round is a per-thread CONSTANT address for the round's parity P = g & 1 (layout g lives in copy P,
  // layout g + 1 goes to copy P ^ 1, the rotations of round g in record set P): both sets of addresses are formed once, and
  // the round loop is two copies of one body -- no address arithmetic in it (it was ~20 of a block's ~55 instructions a
  // round; with eleven waves on four SIMDs the round was bound by instruction issue, not by the LDS).
  typedef __attribute__((address_space(3))) double lds_d;
  typedef double ja_d2 __attribute__((ext_vector_type(2)));
  typedef __attribute__((address_space(3))) ja_d2 lds_d2;
  lds_d* const Al = (lds_d*)A0;
  lds_d* const csl = (lds_d*)&s_cs[0][0][0];
  constexpr int CSS = 49 * 6;  // doubles per record set
  // (the record sets are a compile-time distance apart: one pointer per pair, the parity is an immediate offset.  The two
  //  copies of the matrix are a RUN-TIME distance apart: both address sets in registers where the registers are there -- the
  //  rotation-log form --, one set plus an add per access in the form that also carries W and has to fit 128 registers for two
  //  workgroups per CU.)
  constexpr bool TAB = LOGW;
  lds_d* rd[NU][TAB ? 2 : 1][4];
  lds_d* wr[NU][TAB ? 2 : 1][4];
  lds_d* cpa[NU];
  lds_d* cpb[NU];
#pragma unroll
  for (int u = 0; u < (PARAM ? 0 : NU); ++u) {
    const int e = tid + u * WT;
#pragma unroll
    for (int P = 0; P < (TAB ? 2 : 1); ++P)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        rd[u][P][q] = Al + P * bst + q * nbp + (ba[u] < 0 ? 0 : e);
        wr[u][P][q] = Al + (P ^ 1) * bst + dst[u][q];
      }
    cpa[u] = csl + 6 * (ba[u] < 0 ? 0 : ba[u]);
    cpb[u] = csl + 6 * (ba[u] < 0 ? 0 : bb[u]);
  }
  // W workers (not LOGW): groups of `half` consecutive threads (thread = pair); group g takes the component pairs g, g + ngrp, ...
  const int ngrp = half > 0 ? WT / half : 1;
  const int wg = half > 0 ? tid / half : 0, wb = tid - wg * half;
  const bool w_on = tid < WT && wg < ngrp;
  // the parameter wave: lane pk = pair pk.  Of the NEXT seating's pair pk, the top player sits in slot su of this one, the
  // bottom player in slot sv.
  const int pk = tid - WT;
  const bool p_on = PARAM && pk >= 0 && pk < half;
  int o_b[4] = {0, 0, 0, 0}, c_r = 0, c_c = 0, c_du = 0, c_dv = 0;
  if (p_on) {
    const int su = seat_prev_slot(2 * pk, m1, half), sv = seat_prev_slot(2 * pk + 1, m1, half);
    const int a = su >> 1, b = sv >> 1;
    c_du = 6 * a + 4 + (su & 1);  // where the top / bottom player's diagonal entry (after this round's rotation) is published
    c_dv = 6 * b + 4 + (sv & 1);
    // the off-diagonal entry H'[su][sv] from block (row pair <= column pair), the orientation its owner rotates it in
    int rs = su, cs_ = sv;
    if (a > b || (a == b && (su & 1))) { rs = sv; cs_ = su; }
    const int R = rs >> 1, Cc = cs_ >> 1, eb = Cc * (Cc + 1) / 2 + R;
    o_b[0] = eb; o_b[1] = nbp + eb; o_b[2] = (R == Cc ? 1 : 2) * nbp + eb; o_b[3] = 3 * nbp + eb;
    c_r = 6 * R + 2 * (rs & 1);  // offset (in doubles) of the half record the row seat needs
    c_c = 6 * Cc + 2 * (cs_ & 1);
  }
  lds_d* pbk[2][4];
  lds_d* prr[2];
  lds_d* prc[2];
  lds_d* pdu[2];
  lds_d* pdv[2];
  lds_d* pcw[2];
#pragma unroll
  for (int P = 0; P < 2; ++P) {
#pragma unroll
    for (int q = 0; q < 4; ++q) pbk[P][q] = Al + P * bst + o_b[q];
    prr[P] = csl + P * CSS + c_r;
    prc[P] = csl + P * CSS + c_c;
    pdu[P] = csl + P * CSS + c_du;
    pdv[P] = csl + P * CSS + c_dv;
    pcw[P] = csl + (P ^ 1) * CSS + 6 * (p_on ? pk : 48);  // (the records of round g + 1; lanes beyond the pairs: the spare record)
  }
  // the pair's state, carried in registers: diagonal block (app, apq, aqq) of the current layout and its rotation (pc, ps)
  double app = 0.0, apq = 0.0, aqq = 0.0, pc = 1.0, ps = 0.0;
  // (every lane of the wave runs the chain -- lanes beyond the pairs on zeros -- and writes: to its pair's record, or to a
  //  spare record / a spare row of the log: no exec-mask branches on the critical path)
  const int log_cap = JS_LOG_SWEEPS * m1;  // (the log has one spare row behind its JS_LOG_SWEEPS sweeps: gpet_api_batch.hip)
  GPET_GLOBAL ja_d2* const logp = (GPET_GLOBAL ja_d2*)E.jlog + (p_on ? pk : log_cap * half + (pk >= 0 ? pk - half : 0));
  const int lrow = p_on ? half : 0;  // (idle lanes: always their element of the spare row)
  auto params_store = [&](lds_d* csw, int g_next) {
    jac_params_nb(app, apq, aqq, pc, ps);
    *(lds_d2*)csw = (ja_d2){pc, -ps};
    *(lds_d2*)(csw + 2) = (ja_d2){ps, pc};
    // the pair's diagonal after this rotation (the owners' arithmetic): what the pairs of the NEXT seating start from
    *(lds_d2*)(csw + 4) = (ja_d2){jac_rot_entry(app, apq, apq, aqq, pc, -ps, pc, -ps), jac_rot_entry(app, apq, apq, aqq, ps, pc, ps, pc)};
    // (a global_store, not a flat one: a FLAT store counts in the LDS counter too, and the barrier's wait for this wave's LDS
    //  writes would wait for it)
    if (LOGW) logp[(size_t)(g_next < log_cap ? g_next : log_cap) * lrow] = (ja_d2){pc, ps};
  };
  // the parameter wave is the round's critical path: its instructions go first on its SIMD
  if constexpr (PARAM) __builtin_amdgcn_s_setprio(3);
  __syncthreads();
  int sweeps = 0, buf = 0, g = 0;  // g: global round = sweep * m1 + round
  if (r >= 2) {
    for (int sweep = 0; sweep < JS_LOG_SWEEPS; ++sweep) {
      const double* Ab = A0 + buf * bst;
      double off = 0.0, dg = 0.0;
      for (int e = tid; e < nblk; e += NT) {
        int a_, b_;
        seat_block_of(e, a_, b_);
        const double v00 = Ab[e], v01 = Ab[nbp + e], v10 = Ab[2 * nbp + e], v11 = Ab[3 * nbp + e];
        if (a_ == b_) {
          dg += v00 * v00 + v11 * v11;
          off += 2.0 * v01 * v01;
        } else {
          off += 2.0 * ((v00 * v00 + v01 * v01) + (v10 * v10 + v11 * v11));
        }
      }
      off = block_sum(off, s_red);
      dg = block_sum(dg, s_red);
      if (off <= 1e-24 * dg || off == 0.0) break;
      ++sweeps;
      if (sweep == 0) {  // (later sweeps: their first round's parameters came out of the previous sweep's last round)
        if (p_on) {
          const int dk = pk * (pk + 1) / 2 + pk;
          app = Ab[dk]; apq = Ab[nbp + dk]; aqq = Ab[3 * nbp + dk];
        }
        if constexpr (PARAM) params_store(csl + 6 * (p_on ? pk : 48), 0);
        __syncthreads();
      }
      int pb = wb, qb = wb == 0 ? m1 : m1 - wb;  // players of this thread's W pair in round 0
      auto round_body = [&](auto Pc) {
        constexpr int P = decltype(Pc)::value;
        if constexpr (PARAM) {
          // -- parameters of round g + 1 from layout g and its rotations: 8 reads, all issued at once
          const double b00 = *pbk[P][0], b01 = *pbk[P][1], b10 = *pbk[P][2], b11 = *pbk[P][3];
          const ja_d2 rr_ = *(lds_d2*)prr[P], rc = *(lds_d2*)prc[P];
          const double app_n = *pdu[P], aqq_n = *pdv[P];
          apq = jac_rot_entry(b00, b01, b10, b11, rr_.x, rr_.y, rc.x, rc.y);
          app = app_n;
          aqq = aqq_n;
          params_store(pcw[P], g + 1);
        } else {
#pragma unroll
          for (int u = 0; u < NU; ++u) {
            if (ba[u] < 0) continue;
            const ja_d2 ra = *(lds_d2*)(cpa[u] + P * CSS), rb = *(lds_d2*)(cpb[u] + P * CSS);
            // (all four planes read at once: a diagonal block's [1][0] plane holds nothing it uses, the select comes after)
            constexpr int PT = TAB ? P : 0;
            const int dr = TAB ? 0 : P * bst, dw = TAB ? 0 : -P * bst;  // (one address set: copy 1 is bst on / back)
            const double b00 = *(rd[u][PT][0] + dr), b01 = *(rd[u][PT][1] + dr), b10r = *(rd[u][PT][2] + dr), b11 = *(rd[u][PT][3] + dr);
            const double b10 = (ba[u] == bb[u]) ? b01 : b10r;
            double nv[4];
            jac_rot_block(b00, b01, b10, b11, ra.x, -ra.y, rb.x, -rb.y, nv);
#pragma unroll
            for (int q = 0; q < 4; ++q) *(wr[u][PT][q] + dw) = nv[q];
          }
          const double* cs = &s_cs[P][0][0];
          if (!LOGW && w_on) {  // W: rotate the eigenvector entries of players pb, qb (needs only this round's (c, s))
            const double2 rb = *reinterpret_cast<const double2*>(cs + 6 * wb);
            const double cb = rb.x, sb = -rb.y;
            if (sb != 0.0) {
              constexpr int BD = RR >= 6 ? 1 : RR > 0 ? 2 : 3;
              for (int ip0 = wg; ip0 < hl; ip0 += BD * ngrp) {
                double2 wp[BD], wq[BD];
#pragma unroll
                for (int t = 0; t < BD; ++t) {
                  const int ip = ip0 + t * ngrp;
                  if (ip < hl) {
                    wp[t] = W2[ip * m + pb];
                    wq[t] = W2[ip * m + qb];
                  }
                }
#pragma unroll
                for (int t = 0; t < BD; ++t) {
                  const int ip = ip0 + t * ngrp;
                  if (ip < hl) {
                    W2[ip * m + pb] = make_double2(fma(cb, wp[t].x, -(sb * wq[t].x)), fma(cb, wp[t].y, -(sb * wq[t].y)));
                    W2[ip * m + qb] = make_double2(fma(sb, wp[t].x, cb * wq[t].x), fma(sb, wp[t].y, cb * wq[t].y));
                  }
                }
              }
            }
          }
          if (!LOGW && RR > 0) {  // the register rows (whole waves: the seat change crosses lanes)
            const double2 rk = *reinterpret_cast<const double2*>(cs + 6 * (r_lane_on ? rlane : 0));
            const double c = r_lane_on ? rk.x : 1.0, sn = r_lane_on ? -rk.y : 0.0;
#pragma unroll
            for (int t = 0; t < RR; ++t) {
              if (2 * hl + rwave + 7 * t < m) {  // (uniform over the wave)
                const double xr = fma(c, rx[t], -(sn * ry[t])), yr = fma(sn, rx[t], c * ry[t]);
                const double xd = wp_lane_from_above(xr, xr);
                const double yu = wp_lane_from_below(r_lane0 ? xr : yr, yr);
                rx[t] = r_lane_last ? yr : xd;
                ry[t] = yu;
              }
            }
          }
        }
        __syncthreads();
      };
      for (int round = 0; round < m1; ++round, ++g) {
        if ((g & 1) == 0) round_body(std::integral_constant<int, 0>{});
        else round_body(std::integral_constant<int, 1>{});
        buf ^= 1;
        pb = pb + 1 >= m1 ? 0 : pb + 1;
        if (wb != 0) qb = qb + 1 >= m1 ? 0 : qb + 1;
      }
    }
  }
  if constexpr (PARAM) __builtin_amdgcn_s_setprio(0);
  // back in the initial seats: slot -> player of round 0
  const double* Af = A0 + buf * bst;
  for (int k = tid; k < half; k += NT) {
    const int d = k * (k + 1) / 2 + k;
    s_theta[seat_player(2 * k, 0, m1)] = Af[d];
    s_theta[seat_player(2 * k + 1, 0, m1)] = Af[3 * nbp + d];
  }
  __syncthreads();
  for (int k = tid; k < r; k += NT) E.theta[k] = s_theta[k];
  const double* Wd = reinterpret_cast<const double*>(W2);  // W[j][i] = Wd[((i >> 1) * m + j) * 2 + (i & 1)]
  const int r_lds = 2 * hl < r ? 2 * hl : r;  // components in LDS
  double* Wk = jac_warm_slot(E, sc->iter);
  if (!LOGW)
    for (int e = tid; e < r_lds * r; e += NT) {
      const int i = e / r, j = e - i * r;
      const double v = Wd[((i >> 1) * m + j) * 2 + (i & 1)];
      E.W[(size_t)i * ldg + j] = v;
      Wk[(size_t)i * ldg + j] = v;
    }
  if (!LOGW && tid == 0 && E.structured) E.wq_tag[sc->iter & 1] = (sc->iter + 1) + 65536 * r;
  for (int k = tid; k < r; k += NT) {
    const double v = s_theta[k];
    int pos = 0;
    for (int j = 0; j < r; ++j) {
      const double u = s_theta[j];
      pos += (u > v) || (u == v && j < k);
    }
    E.order[pos] = k;
    s_pos[k] = pos;
  }
  __syncthreads();
  if (scaled_out && !LOGW) {
    for (int e = tid; e < r_lds * r; e += NT) {
      const int i = e / r, j = e - i * r;
      const double th = s_theta[j];
      E.G[(size_t)i * ldg + s_pos[j]] = Wd[((i >> 1) * m + j) * 2 + (i & 1)] * (sc->y_std * sqrt(th > 0.0 ? th : 0.0));
    }
  }
  if (!LOGW && RR > 0 && tid < WT && r_lane_on) {  // the register rows: lane k holds component i of players r_pe and r_po
#pragma unroll
    for (int t = 0; t < RR; ++t) {
      const int i = 2 * hl + rwave + 7 * t;
      if (i < r) {
        if (r_pe < r) {
          E.W[(size_t)i * ldg + r_pe] = rx[t];
          Wk[(size_t)i * ldg + r_pe] = rx[t];
          const double th = s_theta[r_pe];
          if (scaled_out) E.G[(size_t)i * ldg + s_pos[r_pe]] = rx[t] * (sc->y_std * sqrt(th > 0.0 ? th : 0.0));
        }
        if (r_po < r) {
          E.W[(size_t)i * ldg + r_po] = ry[t];
          Wk[(size_t)i * ldg + r_po] = ry[t];
          const double th = s_theta[r_po];
          if (scaled_out) E.G[(size_t)i * ldg + s_pos[r_po]] = ry[t] * (sc->y_std * sqrt(th > 0.0 ? th : 0.0));
        }
      }
    }
  }
  if (tid == 0) sc->lml = (double)sweeps;  // diagnostics: Jacobi sweeps of this factorisation
}

template <int NU, bool LOGW, int RR, int NTHR>  // NTHR - 64 worker threads with NU blocks each + the parameter wave
__global__ void __launch_bounds__(NTHR) __attribute__((amdgpu_waves_per_eu(LOGW ? 1 : 4, LOGW ? (NTHR + 255) / 256 : 4)))
k_jacobi_ahead(EdgeDev* edges, int scaled_out, int warm) {
  constexpr int WT = NTHR - 64;
  const EdgeDev E = edges[blockIdx.y];
  gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK || E.factor_injected) return;
  extern __shared__ __attribute__((aligned(16))) double s_mem[];
  __shared__ double s_red[16];
  __shared__ __attribute__((aligned(16))) double s_cs[2][49][6];  // (c, -s, s, c, d0', d1') of the pairs (+ a spare record for the parameter wave's idle lanes), rounds g (even / odd): rotation, and the pair's two diagonal entries after it
  __shared__ int s_pos[96];
  __shared__ double s_theta[96];
  // Two copies of ONE body, by role: the parameter wave's and the workers'.  They execute the same barriers; what differs is
  // what each keeps in registers across the rounds (the workers' address tables and register rows of W, the parameter
  // wave's gather addresses and pair state), and as two code paths neither set is live in the other's loop -- as one path
  // with a branch per round the kernel needed both at every point and spilled in the form that has to fit 128 registers.
  if (threadIdx.x >= WT) ja_run<NU, LOGW, RR, NTHR, true>(E, sc, scaled_out, warm, s_mem, s_red, s_cs, s_pos, s_theta);
  else ja_run<NU, LOGW, RR, NTHR, false>(E, sc, scaled_out, warm, s_mem, s_red, s_cs, s_pos, s_theta);
}

// The eigenvectors from the rotation log of k_jacobi_seat<.., LOGW>: wave = component i (row i of W over the players), lane
// k = pair k of the seating: x = the entry of the player in slot 2k, y = of the player in slot 2k + 1.  A round rotates
// (x, y) by the pair's (c, s) -- the arithmetic of the LDS form, W[.][p] = c p - s q, W[.][q] = s p + c q -- and then moves
// every player of the circle one seat on: x one lane down, y one lane up, the two ends handed over (slot 0's player goes to
// slot 3, the last odd slot's player to the last even slot; the pivot in slot 1 stays), by whole-wave DPP shifts.  The log
// is read sixteen rounds at a time, the next sixteen requested before these are applied.  After whole sweeps everybody is
// back in the seats of round 0.
__global__ void __launch_bounds__(256) k_jacobi_wpass(EdgeDev* edges, int scaled_out, int warm) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK || E.factor_injected) return;
  const int r = sc->rank, ldg = E.r_cap;
  const int m = (r + 1) & ~1, half = m >> 1, m1 = m - 1;
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  __shared__ int s_pos[96];
  for (int k = threadIdx.x; k < r; k += 256) s_pos[E.order[k]] = k;  // player -> place in descending order (k_jacobi_seat wrote E.order)
  __syncthreads();
  if (i >= r || r < 1) return;
  // (sweeps of this factorisation x rounds; uniform, and the compiler has to know it: the per-round test below is then a scalar
  //  branch instead of a vector compare and an exec mask per round)
  const int total = __builtin_amdgcn_readfirstlane((int)sc->lml * m1);
  const double2* jlog = reinterpret_cast<const double2*>(E.jlog);
  const bool on = lane < half;
  const int pe = seat_player(2 * lane, 0, m1), po = seat_player(2 * lane + 1, 0, m1);
  double x = (on && pe == i) ? 1.0 : 0.0, y = (on && po == i) ? 1.0 : 0.0;
  const double* Wp = jac_warm_source(E, sc, warm);  // (warm start: the rotations continue from the previous eigenvectors)
  if (Wp && on) {
    if (pe < r) x = Wp[(size_t)i * ldg + pe];
    if (po < r) y = Wp[(size_t)i * ldg + po];
  }
  double* Wk = jac_warm_slot(E, sc->iter);
  const bool lane0 = lane == 0, lane_last = lane == half - 1;
  // The log is read 16 rounds at a time, TWO blocks ahead (a block is ~1 700 cycles of work; a row of the log written by another
  // CU a moment ago comes back from beyond this XCD's L2 in 1-2 us), every load unconditional: rows beyond the last round and
  // lanes beyond the pairs read a valid element that the scalar test below never lets through.
  constexpr int PF = 16;
  typedef double wp_d2 __attribute__((ext_vector_type(2)));
  const GPET_GLOBAL wp_d2* lg = (const GPET_GLOBAL wp_d2*)E.jlog + (on ? lane : 0);
  const int last = total > 0 ? total - 1 : 0;
  auto row = [&](int rr) { return lg[(size_t)(rr < last ? rr : last) * half]; };
  wp_d2 cur[PF], nx1[PF], nx2[PF];
#pragma unroll
  for (int u = 0; u < PF; ++u) cur[u] = row(u);
#pragma unroll
  for (int u = 0; u < PF; ++u) nx1[u] = row(PF + u);
  for (int r0 = 0; r0 < total; r0 += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) nx2[u] = row(r0 + 2 * PF + u);
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      if (r0 + u < total) {  // (scalar)
        const double c = on ? cur[u].x : 1.0, sn = on ? cur[u].y : 0.0;
        const double xr = fma(c, x, -(sn * y)), yr = fma(sn, x, c * y);
        const double xd = wp_lane_from_above(xr, xr);
        const double yu = wp_lane_from_below(lane0 ? xr : yr, yr);
        x = lane_last ? yr : xd;
        y = yu;
      }
    }
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      cur[u] = nx1[u];
      nx1[u] = nx2[u];
    }
  }
  if (!on) return;
  // lane k holds component i of the eigenvectors of players pe and po
  if (pe < r) E.W[(size_t)i * ldg + pe] = x, Wk[(size_t)i * ldg + pe] = x;
  if (po < r) E.W[(size_t)i * ldg + po] = y, Wk[(size_t)i * ldg + po] = y;
  // (the tag: by the wave of the last row, after its own stores -- the next reader is a later launch)
  if (i == r - 1 && lane == 0 && E.structured) E.wq_tag[sc->iter & 1] = (sc->iter + 1) + 65536 * r;
  if (scaled_out) {
    if (pe < r) {
      const double th = E.theta[pe];
      E.G[(size_t)i * ldg + s_pos[pe]] = x * (sc->y_std * sqrt(th > 0.0 ? th : 0.0));
    }
    if (po < r) {
      const double th = E.theta[po];
      E.G[(size_t)i * ldg + s_pos[po]] = y * (sc->y_std * sqrt(th > 0.0 ? th : 0.0));
    }
  }
}

// ---- structured loop path (training points on the pixel grid, rank(rho) <= 96) ---------------
// The prior covariance on the unit-spaced grid is c * rho with rho Toeplitz and FIXED for the whole
// trace: rho = Q Lam Q^T (rank r0 ~ 2.6 Lg / l for RBF) is factored once per edge at construction.
// With every training x on the grid, K_o* = c rho[obs, :] and the posterior covariance is
//     Sigma / y_std^2 = Q (c Lam - U^T U) Q^T,   U = L^-1 (c Q[obs, :] Lam)       (n x r0)
// so an iteration needs only the r0 x r0 matrix H = c Lam - U^T U and its Jacobi eigen-decomposition
// H = R Theta R^T:  the singular pairs of Sigma are (y_std^2 theta_k, Q r_k) -- no Lg x Lg covariance,
// no pivoted Cholesky, no Gram matrix; the posterior mean is y_std * Q (c Lam Q[obs,:]^T alpha) + m.
__global__ void __launch_bounds__(256) k_rho_fill(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  const int Lg = E.Lg;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < (size_t)Lg * Lg; e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / Lg), j = (int)(e - (size_t)i * Lg);
    E.cov[e] = (i == j) ? 1.0
                        : corr_fn(E, (double)(E.x_st + i) / E.length_scale,
                                  (double)(E.x_st + j) / E.length_scale);
  }
}

// rows of A = sqrt(lam_a) q_a^T (factor of rho)  ->  Q0 (unit rows) and lam0 = |row|^2
__global__ void __launch_bounds__(256) k_struct_basis(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  const int a = blockIdx.x;
  if (a >= sc->rank) return;
  __shared__ double s_red[16];
  double part = 0.0;
  for (int j = threadIdx.x; j < E.Lg; j += blockDim.x) {
    const double v = E.A[(size_t)a * E.Lg + j];
    part += v * v;
  }
  const double nrm2 = block_sum(part, s_red);
  const double inv = 1.0 / sqrt(nrm2);
  // (and the sign convention's weights in this basis: sum_j A[k][j] / (j + 1) of a factor row A[k] = sum_t g_t Q0[t] is
  //  sum_t g_t h0[t] -- k_struct_rows decides the sign of a row from the r0 coefficients before it writes the row)
  double hp = 0.0;
  for (int j = threadIdx.x; j < E.Lg; j += blockDim.x) {
    const double q = E.A[(size_t)a * E.Lg + j] * inv;
    E.Q0[(size_t)a * E.Lg + j] = q;
    hp += q / (double)(j + 1);
  }
  const double h = block_sum(hp, s_red);
  if (threadIdx.x == 0) {
    E.lam0[a] = nrm2;
    E.h0[a] = h;
  }
}

// H = c Lam - U^T U (into E.C, row stride r_cap), beta, posterior mean.  One workgroup per edge;
// U (n x r0) lives in LDS, one thread per column for the forward substitution, rows of L streamed
// through LDS.
__global__ void __launch_bounds__(1024) k_struct_H(EdgeDev* edges, int l_in_lds) {
  const EdgeDev E = edges[blockIdx.y];
  gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK || !E.structured) return;
  // (global_* instead of flat_* accesses: a FLAT load counts in the LDS counter too, and this kernel waits for LDS all the time)
  GPET_GLOBAL double* __restrict__ g_C = (GPET_GLOBAL double*)E.C;
  GPET_GLOBAL double* __restrict__ g_K = (GPET_GLOBAL double*)E.K;
  GPET_GLOBAL double* __restrict__ g_Q0 = (GPET_GLOBAL double*)E.Q0;
  GPET_GLOBAL double* __restrict__ g_alpha = (GPET_GLOBAL double*)E.alpha;
  GPET_GLOBAL double* __restrict__ g_beta = (GPET_GLOBAL double*)E.beta;
  GPET_GLOBAL double* __restrict__ g_lam0 = (GPET_GLOBAL double*)E.lam0;
  GPET_GLOBAL double* __restrict__ g_mean = (GPET_GLOBAL double*)E.mean;
  GPET_GLOBAL double* __restrict__ g_xt = (GPET_GLOBAL double*)E.xt;
  extern __shared__ double s_dyn[];
  const int n = sc->n, r0 = E.r0, Lg = E.Lg, ldk = E.n_cap, ldc = E.r_cap;
  const int ldu = r0 | 1;
  double* U = s_dyn;                                            // [n_cap][ldu]
  double* Lp = U + (size_t)E.n_cap * ldu;                       // l_in_lds: packed lower triangle of L (row i at i (i + 1) / 2);
                                                                // otherwise [n_cap]: the current row of L
  double* s_b = Lp + (l_in_lds ? (size_t)E.n_cap * (E.n_cap + 1) / 2 : (size_t)E.n_cap);  // [r_cap] beta
  const int tid = threadIdx.x, bs = blockDim.x;
  const double c = sc->amp;
#ifdef GPET_SH_PROF
  const long long p0 = clock64();
  const long long w0 = wall_clock64();
#endif
  // right-hand sides  Bo[i][a] = c * lam0[a] * Q0[a][idx_i];  the Cholesky factor comes into LDS once if it fits.
  // The grid indices of the training points go to LDS first (s_b is free until beta is formed): the gathers of Q0 then
  // depend on nothing and overlap with each other and with the copy of L -- two global round trips for the phase
  // instead of two per gathered element
  int* s_idx = reinterpret_cast<int*>(s_b);  // (n <= n_cap <= 128 ints in r_cap >= 4 doubles ... sized below)
  const bool idx_in_lds = (size_t)n * sizeof(int) <= (size_t)E.r_cap * sizeof(double);
  if (idx_in_lds)
    for (int i = tid; i < n; i += bs) s_idx[i] = (int)g_xt[i] - E.x_st;
  if (l_in_lds) {
    for (int e = tid; e < n * n; e += bs) {
      const int i = e / n, t = e - i * n;
      if (t <= i) Lp[i * (i + 1) / 2 + t] = g_K[(size_t)i * ldk + t];
    }
  }
  __syncthreads();
#pragma unroll 4
  for (int e = tid; e < n * r0; e += bs) {
    const int i = e / r0, a = e - i * r0;
    const int idx = idx_in_lds ? s_idx[i] : (int)g_xt[i] - E.x_st;
    U[i * ldu + a] = c * g_lam0[a] * g_Q0[(size_t)a * Lg + idx];
  }
  __syncthreads();
#ifdef GPET_SH_PROF
  const long long p1 = clock64();
#endif
  // beta_a = sum_i Bo[i][a] alpha_i
  for (int a = tid; a < r0; a += bs) {
    double acc = 0.0;
    for (int i = 0; i < n; ++i) acc += U[i * ldu + a] * g_alpha[i];
    s_b[a] = acc;
    g_beta[a] = acc;
  }
#ifdef GPET_SH_PROF
  const long long p1b = clock64();
#endif
  if (l_in_lds) {
    // U = L^-1 Bo in blocks of 16 rows: (a) every thread takes one (row of the block, column) entry and subtracts the
    // rows ABOVE the block -- independent inner products, all 16 waves busy; (b) one thread per column finishes the
    // block's 16 rows (<= 120 dependent steps).  The terms of an entry are subtracted in ascending row order, as by
    // the one-thread-per-column loop of round 1 (which left 14 of the 16 waves idle for n^2 / 2 dependent steps: 65 %
    // of this kernel at n = 90), so the result is the same to the bit.
    for (int i0 = 0; i0 < n; i0 += 16) {
      const int nb = (n - i0) < 16 ? (n - i0) : 16;
      if (i0 > 0) {
        for (int o = tid; o < nb * r0; o += bs) {
          const int ri = o / r0, ca = o - ri * r0;
          const int i = i0 + ri;
          const double* li = Lp + i * (i + 1) / 2;
          double acc = U[i * ldu + ca];
#pragma unroll 8
          for (int t = 0; t < i0; ++t) acc -= li[t] * U[t * ldu + ca];
          U[i * ldu + ca] = acc;
        }
        __syncthreads();
      }
      if (tid < r0) {
        // (the block's 16 entries of the column in registers, the triangle fully unrolled: the reads of L carry no
        //  dependence and are issued ahead of the chain instead of costing one LDS round trip per step)
        double u[16];
#pragma unroll
        for (int ri = 0; ri < 16; ++ri) u[ri] = (ri < nb) ? U[(i0 + ri) * ldu + tid] : 0.0;
#pragma unroll
        for (int ri = 0; ri < 16; ++ri) {
          if (ri < nb) {
            const int i = i0 + ri;
            const double* li = Lp + i * (i + 1) / 2 + i0;
            double acc = u[ri];
#pragma unroll
            for (int t = 0; t < ri; ++t) acc -= li[t] * u[t];
            u[ri] = acc / li[ri];
          }
        }
#pragma unroll
        for (int ri = 0; ri < 16; ++ri)
          if (ri < nb) U[(i0 + ri) * ldu + tid] = u[ri];
      }
      __syncthreads();
    }
  } else {
    // (many training points: L does not fit next to U; its rows are streamed through LDS one at a time)
    for (int i = 0; i < n; ++i) {
      __syncthreads();
      const double* ri = E.K + (size_t)i * ldk;
      for (int t = tid; t <= i; t += bs) Lp[t] = ri[t];
      __syncthreads();
      if (tid < r0) {
        double acc = U[i * ldu + tid];
        for (int t = 0; t < i; ++t) acc -= Lp[t] * U[t * ldu + tid];
        U[i * ldu + tid] = acc / Lp[i];
      }
    }
  }
  __syncthreads();
#ifdef GPET_SH_PROF
  const long long p2 = clock64();
#endif
  // H[a][b] = c lam0[a] delta_ab - sum_i U[i][a] U[i][b]: U^T U on the matrix cores, one 16 x 16 tile of the upper
  // triangle per wave (v_mfma_f64_16x16x4: A lane l <- U[4 q + (l >> 4)][16 ta + (l & 15)], B the same with tb; both
  // operands straight from the LDS copy of U), mirrored on the way out
  {
    typedef double v4d __attribute__((ext_vector_type(4)));
    const int lane = tid & 63, wv = tid >> 6, li = lane & 15, lq = lane >> 4;
    const int nt = (r0 + 15) >> 4, ntile = nt * (nt + 1) / 2, nwave = bs >> 6;
    for (int tile = wv; tile < ntile; tile += nwave) {
      int tb = (int)((sqrt(8.0 * (double)tile + 1.0) - 1.0) * 0.5);
      while (tb * (tb + 1) / 2 > tile) --tb;
      while ((tb + 1) * (tb + 2) / 2 <= tile) ++tb;
      const int ta = tile - tb * (tb + 1) / 2;  // ta <= tb
      const int ca = 16 * ta + li, cb = 16 * tb + li;
      v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
      for (int i0 = 0; i0 < n; i0 += 4) {
        const int i = i0 + lq;
        const double av = (i < n && ca < r0) ? U[i * ldu + ca] : 0.0;
        const double bv = (i < n && cb < r0) ? U[i * ldu + cb] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int a = 16 * ta + lq + 4 * g, b = cb;
        if (a < r0 && b < r0 && b >= a) {
          const double v = ((a == b) ? c * g_lam0[a] : 0.0) - acc[g];
          g_C[(size_t)a * ldc + b] = v;
          g_C[(size_t)b * ldc + a] = v;
        }
      }
    }
  }
#ifdef GPET_SH_PROF
  const long long p3 = clock64();
#endif
  // posterior mean on the grid: y_std * (Q beta) + y_mean        sklearn_gpr.py:382-385
  {  // (two threads per grid point, even and odd basis vectors, loads unrolled: the 72 reads of a thread were one chain)
    const int hh = tid & 1;
    const double y_std = sc->y_std, y_mean = sc->y_mean;
    for (int j = tid >> 1; j < Lg; j += bs >> 1) {
      double acc = 0.0;
#pragma unroll 6
      for (int a = hh; a < r0; a += 2) acc += g_Q0[(size_t)a * Lg + j] * s_b[a];
      acc += __shfl_xor(acc, 1, 2);
      if (hh == 0) g_mean[j] = y_std * acc + y_mean;
    }
  }
  if (tid == 0) sc->rank = r0;
#ifdef GPET_SH_PROF
  if (tid == 0 && blockIdx.y == 5) printf("k_struct_H n=%d: build+L %lld | beta %lld | substitution %lld | H %lld | mean %lld ticks; whole kernel %lld ticks = %lld wall ticks of 10 ns\n", n, p1 - p0, p1b - p1, p2 - p1b, p3 - p2, clock64() - p3, clock64() - p0, wall_clock64() - w0);
#endif
}

// ---- structured path with MANY training points (n_cap > 128): U lives in HBM (the V buffer, row stride r_cap) ----
// B rows -> blocked forward substitution U = L^-1 B (left-looking: block k subtracts the blocks before it, then
// solves against its diagonal block in LDS; the r0 columns are split over workgroups of 16) -> H, beta, mean.
#define SB_COLS 16
__global__ void __launch_bounds__(256) k_structB_build(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK || !E.structured) return;
  const int n = sc->n, r0 = E.r0, Lg = E.Lg, ldu = E.r_cap;
  const double c = sc->amp;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n * r0; e += gridDim.x * blockDim.x) {
    const int i = e / r0, a = e - i * r0;
    const int idx = (int)E.xt[i] - E.x_st;
    E.V[(size_t)i * ldu + a] = c * E.lam0[a] * E.Q0[(size_t)a * Lg + idx];
  }
}

// beta_a = sum_i B[i][a] alpha_i  (before the substitution overwrites B)
__global__ void __launch_bounds__(128) k_struct_beta(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK || !E.structured) return;
  const int n = sc->n, r0 = E.r0, ldu = E.r_cap;
  for (int a = threadIdx.x; a < r0; a += blockDim.x) {
    double acc = 0.0;
    for (int i = 0; i < n; ++i) acc += E.V[(size_t)i * ldu + a] * E.alpha[i];
    E.beta[a] = acc;
  }
}

// block k0 of U = L^-1 B for the 16 columns of this workgroup
// (predict != 0: the same substitution on the Lg columns of V = K_*^T, row stride Lg -- the generic path's
//  V = L^-1 K_*^T for many training points)
__global__ void __launch_bounds__(256) k_struct_trsm(EdgeDev* edges, int k0, int predict) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK || (!predict && !E.structured)) return;
  const int n = sc->n, r0 = predict ? E.Lg : E.r0, ld = E.n_cap, ldu = predict ? E.Lg : E.r_cap;
  const int a0 = blockIdx.x * SB_COLS;
  if (k0 >= n || a0 >= r0) return;
  const int nb = (n - k0) < CB ? (n - k0) : CB;
  __shared__ double sL[CB][CB + 1];       // L[k0 + i][j0 + t] of the block being subtracted, then the diagonal block
  __shared__ double sU[CB][SB_COLS + 1];  // U[j0 + t][a0 + a]
  __shared__ double sX[CB][SB_COLS + 1];  // the block being solved
  const int tid = threadIdx.x;
  const int ca = tid & (SB_COLS - 1), ri = tid >> 4;  // thread tile: column ca, rows ri, ri + 16, ri + 32, ri + 48
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j0 = 0; j0 < k0; j0 += CB) {
    __syncthreads();
    for (int e = tid; e < CB * CB; e += 256) {
      const int i = e >> 6, t = e & 63;
      sL[i][t] = (i < nb) ? E.K[(size_t)(k0 + i) * ld + j0 + t] : 0.0;
    }
    for (int e = tid; e < CB * SB_COLS; e += 256) {
      const int t = e >> 4, a = e & 15;
      sU[t][a] = (a0 + a < r0) ? E.V[(size_t)(j0 + t) * ldu + a0 + a] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int t = 0; t < CB; ++t) {
      const double u = sU[t][ca];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] += sL[ri + 16 * q][t] * u;
    }
  }
  __syncthreads();
  for (int e = tid; e < CB * CB; e += 256) {
    const int i = e >> 6, t = e & 63;
    sL[i][t] = (i < nb && t <= i) ? E.K[(size_t)(k0 + i) * ld + k0 + t] : 0.0;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = ri + 16 * q;
    sX[i][ca] = (i < nb && a0 + ca < r0) ? E.V[(size_t)(k0 + i) * ldu + a0 + ca] - acc[q] : 0.0;
  }
  __syncthreads();
  if (tid < SB_COLS) {  // forward substitution against the diagonal block, one column per thread
    for (int i = 0; i < nb; ++i) {
      double x = sX[i][tid];
      for (int t = 0; t < i; ++t) x -= sL[i][t] * sX[t][tid];
      sX[i][tid] = x / sL[i][i];
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = ri + 16 * q;
    if (i < nb && a0 + ca < r0) E.V[(size_t)(k0 + i) * ldu + a0 + ca] = sX[i][ca];
  }
}

// H = c Lam - U^T U (lower 16x16 tiles, mirrored) from U in HBM
__global__ void __launch_bounds__(256) k_struct_Hbig(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.z];
  gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK || !E.structured) return;
  const int n = sc->n, r0 = E.r0, ldu = E.r_cap, ldc = E.r_cap;
  const int a0 = blockIdx.y * 16, b0 = blockIdx.x * 16;
  if (b0 > a0 || a0 >= r0) return;
  __shared__ double sA[64][17], sB[64][17];
  const int tid = threadIdx.x, ta = tid >> 4, tb = tid & 15;
  double acc = 0.0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    __syncthreads();
    for (int e = tid; e < 64 * 16; e += 256) {
      const int i = e >> 4, q = e & 15;
      const bool in = i0 + i < n;
      sA[i][q] = (in && a0 + q < r0) ? E.V[(size_t)(i0 + i) * ldu + a0 + q] : 0.0;
      sB[i][q] = (in && b0 + q < r0) ? E.V[(size_t)(i0 + i) * ldu + b0 + q] : 0.0;
    }
    __syncthreads();
#pragma unroll 16
    for (int i = 0; i < 64; ++i) acc += sA[i][ta] * sB[i][tb];
  }
  const int a = a0 + ta, b = b0 + tb;
  if (a < r0 && b < r0 && b <= a) {
    const double v = ((a == b) ? sc->amp * E.lam0[a] : 0.0) - acc;
    E.C[(size_t)a * ldc + b] = v;
    E.C[(size_t)b * ldc + a] = v;
  }
}

// posterior mean on the grid: y_std * (Q beta) + y_mean, and the rank of the factorisation to come
__global__ void __launch_bounds__(256) k_struct_mean(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK || !E.structured) return;
  const int r0 = E.r0, Lg = E.Lg;
  __shared__ double s_b[96];
  for (int a = threadIdx.x; a < r0; a += blockDim.x) s_b[a] = E.beta[a];
  __syncthreads();
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < Lg) {
    double acc = 0.0;
    for (int a = 0; a < r0; ++a) acc += E.Q0[(size_t)a * Lg + j] * s_b[a];
    E.mean[j] = sc->y_std * acc + sc->y_mean;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) sc->rank = r0;
}

// factor rows of the structured path: A[k, :] = y_std * sqrt(theta_k) * (Q r_k)^T as a column-tiled product
// (r0 x r0) . (r0 x 64) on v_mfma_f64_16x16x4_f64: the Q0 tile and the scaled, ordered eigenvectors sit in
// LDS, wave w owns 16 of the 64 columns and all MT row tiles, so Q0 is read from HBM once per iteration.
// The sign convention is applied as the rows are written (below).
// MT (row tiles of 16) is a template parameter for the same reason as the K extent of the sample GEMM.
// (SR_TJ = 64 grid columns per workgroup: gpet_iter_plan.h)
typedef double v4f64_ __attribute__((ext_vector_type(4)));
template <int MT, int KS>
__device__ __forceinline__ void struct_rows_body(const EdgeDev& E, double* s_w, int tile) {
  const int r = E.r0, Lg = E.Lg;
  const int j0 = tile * SR_TJ;
  constexpr int kpad = 4 * KS;
  constexpr int ldw = 16 * MT + 1;  // [kpad][ldw]: s_w[t][k] = scaled coefficient of basis vector t in row k
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int j = j0 + 16 * w + li;
#ifdef GPET_SR_PROF
  const long long c0 = clock64();
#endif
  // B operand (Q0[t][j], this wave's 16 columns) straight into registers; A operand (E.G, written by the Jacobi
  // kernel) through LDS, shared by the four waves
  double breg[KS];
#pragma unroll
  for (int q = 0; q < KS; ++q) {
    const int t = 4 * q + lq;
    breg[q] = (t < r && j < Lg) ? E.Q0[(size_t)t * Lg + j] : 0.0;
  }
  // (all the loads of the coefficient matrix in flight at once -- the trip count is a compile-time constant --
  //  instead of six dependent batches of four: the staging was two thirds of this kernel's time)
  // (in two halves: with all 23 values of a thread live at once the kernel needs 172 registers, four more than three
  //  workgroups per CU allow)
  {
    constexpr int NE = kpad * 16 * MT, NL = (NE + 255) / 256, NH = (NL + 1) / 2;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      double gv[NH];
#pragma unroll
      for (int u = 0; u < NH; ++u) {
        const int e = tid + 256 * (u + NH * h);
        const int t = e / (16 * MT), k = e - t * (16 * MT);
        gv[u] = (e < NE && t < r && k < r) ? E.G[(size_t)t * E.r_cap + k] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < NH; ++u) {
        const int e = tid + 256 * (u + NH * h);
        const int t = e / (16 * MT), k = e - t * (16 * MT);
        if (e < NE) s_w[t * ldw + k] = gv[u];
      }
    }
  }
  __syncthreads();
#ifdef GPET_SR_PROF
  const long long c1 = clock64();
#endif
  // Sign convention sum_j A[k][j] / (j + 1) >= 0 (LAPACK's signs are implementation-defined), decided BEFORE the row exists:
  // A[k] = sum_t G[t][k] Q0[t], so the sum is sum_t G[t][k] h0[t] with the r0 weights k_struct_basis left in h0 -- every
  // workgroup of the edge forms the same r0 dot products (fixed order) from its LDS copy of G.  (Rounds 1-4 summed the
  // finished rows tile by tile and flipped them in place in a second kernel: 0.14 ms per launch for reading and writing
  // half of the factor again.)
  double* s_sg = s_w + kpad * ldw;  // [16 MT]
  for (int k = tid; k < 16 * MT; k += 256) {
    double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
    if (k < r) {
      int t = 0;
      for (; t + 3 < r; t += 4) {
        d0 = fma(s_w[t * ldw + k], E.h0[t], d0);
        d1 = fma(s_w[(t + 1) * ldw + k], E.h0[t + 1], d1);
        d2 = fma(s_w[(t + 2) * ldw + k], E.h0[t + 2], d2);
        d3 = fma(s_w[(t + 3) * ldw + k], E.h0[t + 3], d3);
      }
      for (; t < r; ++t) d0 = fma(s_w[t * ldw + k], E.h0[t], d0);
    }
    s_sg[k] = ((d0 + d1) + (d2 + d3)) < 0.0 ? -1.0 : 1.0;
  }
  v4f64_ acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = (v4f64_){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < KS; ++q) {
    const double* wr = s_w + (4 * q + lq) * ldw + li;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      acc[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(wr[16 * mt], breg[q], acc[mt], 0, 0, 0);
  }
#ifdef GPET_SR_PROF
  const long long c2 = clock64();
#endif
  __syncthreads();  // the signs are there
  if (j < Lg) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k = 16 * mt + lq + 4 * g;
        if (k < r) E.A[(size_t)k * Lg + j] = acc[mt][g] * s_sg[k];
      }
  }
#ifdef GPET_SR_PROF
  if (tid == 0 && blockIdx.y == 3 && blockIdx.x == 2)
    printf("k_struct_rows: loads + staging %lld | signs + mfma %lld | stores %lld cycles\n", c1 - c0, c2 - c1, clock64() - c2);
#endif
}

// (one kernel per variant, picked by the launcher for the batch's largest r0 -- an edge of smaller rank multiplies a few zero
//  rows: as ONE kernel that branched on the edge's rank, every variant paid the registers of the largest, 244)
template <int MT, int KS>
__global__ void __launch_bounds__(256) k_struct_rows(EdgeDev* edges) {
  int edge, tile;  // the column tiles of an edge on one XCD: its r x r coefficient matrix comes out of HBM once
  xcd_edge_part((int)gridDim.x, edge, tile);
  const EdgeDev E = edges[edge];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK || !E.structured) return;
  if (tile * SR_TJ >= E.Lg || E.r0 < 1 || E.r0 > 16 * MT) return;
  extern __shared__ __attribute__((aligned(16))) double s_rows[];
  struct_rows_body<MT, KS>(E, s_rows, tile);
}

// step 4: factor rows  A[k, :] = sum_t W[t, order[k]] * G[t, :]  (= sqrt(s_k) v_k up to sign).
// Sign convention (LAPACK's is implementation-defined): sum_j A[k, j] / (j + 1) >= 0.
// The eigenvalue the stage reports is the row's squared norm, as on the any-rank path (k_oj_norms): the Jacobi's diagonal entry,
// which has ordered the rows, carries the rounding of every rotation of every sweep and differs from |A_k|^2 by up to 2e-14 of
// it at rank 96 (tests/test_gpu_factor_injected.py), twice what the sum of squares itself can err by.
__global__ void __launch_bounds__(256) k_factor_rows(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK || E.factor_injected) return;
  const int r = sc->rank, Lg = E.Lg, k = blockIdx.x;
  if (k >= r) return;
  __shared__ double s_red[16];
  extern __shared__ double s_w[];  // [r]
  const int col = E.order[k];
  for (int t = threadIdx.x; t < r; t += blockDim.x) s_w[t] = E.W[(size_t)t * E.r_cap + col];
  __syncthreads();
  double part = 0.0, sq = 0.0;
  for (int j = threadIdx.x; j < Lg; j += blockDim.x) {
    double acc = 0.0;
    for (int t = 0; t < r; ++t) acc += s_w[t] * E.G[(size_t)t * Lg + j];
    E.A[(size_t)k * Lg + j] = acc;
    part += acc / (double)(j + 1);
    sq += acc * acc;
  }
  const double dot = block_sum(part, s_red);
  const double nrm2 = block_sum(sq, s_red);
  if (threadIdx.x == 0) E.theta[col] = nrm2;
  if (dot < 0.0)
    for (int j = threadIdx.x; j < Lg; j += blockDim.x) E.A[(size_t)k * Lg + j] = -E.A[(size_t)k * Lg + j];
}

