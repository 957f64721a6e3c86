// Part of gpet_kernels.hip (included there, inside namespace gpet, in this order): f2: objective of the converged fits (register tiles, f64 matrix cores, blocked in HBM).
// ---------------------------------------------------------------------------------------
// f2  converged fit: -log marginal likelihood and its gradient wrt theta = log(c, l, noise)
//     sklearn_gpr.py:512-585 on the standardised training set (gpet.py:235-248).
//     One workgroup per (edge, restart) problem; L and L^-1 packed-lower in LDS (n <= 128).
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void corr_and_dlog(const EdgeDev& E, double a, double b, double& R, double& dR) {
  const int kernel_type = E.kernel_type, nu_code = E.nu_code;
  const double d = a - b;
  const double D = d * d;
  if (kernel_type == GPET_KERNEL_RBF) {
    R = exp(-0.5 * D);
    dR = R * D;
    return;
  }
  const double r = sqrt(D);
  if (nu_code == 0) {
    R = exp(-r);
    dR = (r > 0.0) ? R * D / r : 0.0;
  } else if (nu_code == 3) {
    R = matern_gen(E.nu_gen, E.inv_gamma_nu, r, &dR);
  } else if (nu_code == 1) {
    const double k = r * 1.7320508075688772;
    R = (1.0 + k) * exp(-k);
    dR = 3.0 * D * exp(-sqrt(3.0 * D));
  } else {
    const double k = r * 2.23606797749979;
    const double t = sqrt(5.0 * D);
    R = (1.0 + k + k * k / 3.0) * exp(-k);
    dR = 5.0 / 3.0 * D * (t + 1.0) * exp(-t);
  }
}

// Symmetric sweep operator on the bordered matrix  A = [[0, y^T], [y, K]]  (index 0 = the y border,
// 1..n = K): sweeping the pivots 1..n in place leaves  A = [[-y^T K^-1 y, alpha^T], [alpha, -K^-1]]
// and the pivots d_k are the squared Cholesky diagonal (log|K| = sum log d_k).  The matrix lives in
// REGISTERS: thread t owns the 4x4 tile (ti, tj), tj <= ti, of the lower triangle (diagonal tiles
// keep both halves), so a step is: owners of column k publish it to LDS (double-buffered, n+1
// doubles), ONE barrier, everyone reads its 4+4 column entries and does 16 FMAs.  n^3/2 FMAs in
// total and n barriers, against the ~3n barriers and the LDS-resident L / L^-1 (2 x 66 KB, one
// workgroup per CU) of a Cholesky + triangular inverse; LDS use is ~3 KB so several problems share a CU.
#define LML_MAXD 136  // 4 * ceil((128 + 1) / 4) + slack
__global__ void __launch_bounds__(576) __attribute__((amdgpu_waves_per_eu(5, 5))) k_lml(EdgeDev* edges, const int* edge_of, const double* theta, double* f_out,
                                             double* g_out, const int* count) {
  const int pb = blockIdx.x;
  if (count != nullptr && pb >= *count) return;  // (launches are sized by the host's last KNOWN number of running problems)
  const EdgeDev E = edges[edge_of[pb]];
  const int n = E.fin_n;
  const int nb = (n + 1 + 3) >> 2;  // 4x4 tiles per side of the bordered matrix
  const int ntile = nb * (nb + 1) / 2;
  __shared__ __attribute__((aligned(16))) double s_col[2][LML_MAXD];
  __shared__ double s_x[LML_MAXD], s_y[LML_MAXD], s_w[LML_MAXD];  // x / l, y, noise weights at index 1..n
  __shared__ double s_piv[LML_MAXD];
  __shared__ double s_red[16];
  const int tid = threadIdx.x, bs = blockDim.x;
  const bool active = tid < ntile;
  int ti = (int)((sqrt(8.0 * (double)tid + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > tid) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= tid) ++ti;
  const int tj = tid - ti * (ti + 1) / 2;
  const double c = exp(theta[3 * pb]), ell = exp(theta[3 * pb + 1]), nl = exp(theta[3 * pb + 2]);
  for (int i = tid; i < 4 * nb; i += bs) {
    const bool in = (i >= 1 && i <= n);
    s_x[i] = in ? E.fin_x[i - 1] / ell : 0.0;
    s_y[i] = in ? E.fin_y[i - 1] : 0.0;
    s_w[i] = in ? E.fin_w[i - 1] : 0.0;
    s_piv[i] = 1.0;
  }
  __syncthreads();
  double T[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = 4 * ti + a, j = 4 * tj + b;
      double v = 0.0;
      if (active && i <= n && j <= n) {
        if (i == 0 || j == 0) {
          v = (i == j) ? 0.0 : s_y[i + j];
        } else if (i == j) {
          v = c + nl * s_w[i];
          v = v + 1e-6;
        } else {
          v = c * corr_fn(E, s_x[i], s_x[j]);
        }
      }
      T[a][b] = v;
    }
  bool bad = false, stop = false;
  for (int kb = 0; kb < nb && !stop; ++kb) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int k = 4 * kb + kk;
      const int buf = kk & 1;  // (= k & 1: a constant once the loop is unrolled -- no double-buffer address arithmetic per step)
      if (k == 0) continue;  // the y border is not a pivot
      if (k > n) {
        stop = true;
        break;
      }
      if (active) {
        if (tj == kb) {
#pragma unroll
          for (int a = 0; a < 4; ++a) s_col[buf][4 * ti + a] = T[a][kk];
          if (ti == kb) s_piv[k] = T[kk][kk];
        } else if (ti == kb) {
#pragma unroll
          for (int b = 0; b < 4; ++b) s_col[buf][4 * tj + b] = T[kk][b];
        }
      }
      __syncthreads();
      const double d = s_col[buf][k];
      if (!(d > 0.0)) {  // not positive definite (same for every thread)
        bad = true;
        stop = true;
        break;
      }
      if (active) {
        // 1 / d by every thread from the hardware reciprocal + two Newton steps: keeps the division off the
        // critical path in front of the barrier (the pivot owner would otherwise hold everyone up)
        double inv = __builtin_amdgcn_rcp(d);
        inv = inv * (2.0 - d * inv);
        inv = inv * (2.0 - d * inv);
        double ci[4], cj[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          ci[a] = s_col[buf][4 * ti + a];
          cj[a] = s_col[buf][4 * tj + a];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const double ma = -(ci[a] * inv);
#pragma unroll
          for (int b = 0; b < 4; ++b) T[a][b] = fma(ma, cj[b], T[a][b]);
        }
        if (ti == kb) {
#pragma unroll
          for (int b = 0; b < 4; ++b) T[kk][b] = cj[b] * inv;
        }
        if (tj == kb) {
#pragma unroll
          for (int a = 0; a < 4; ++a) T[a][kk] = ci[a] * inv;
          if (ti == kb) T[kk][kk] = -inv;
        }
      }
    }
  }
  if (bad) {  // sklearn returns (-inf, 0) -> objective (+inf, -0)
    if (tid == 0) {
      f_out[pb] = INFINITY;
      g_out[3 * pb] = g_out[3 * pb + 1] = g_out[3 * pb + 2] = 0.0;
    }
    return;
  }
  // alpha = column 0 of the swept matrix; its corner is -y^T alpha
  const int fbuf = (n + 1) & 1;  // (the last pivot n used buffer n & 1)
  if (active && tj == 0) {
#pragma unroll
    for (int a = 0; a < 4; ++a) s_col[fbuf][4 * ti + a] = T[a][0];
  }
  __syncthreads();
  const double* al = s_col[fbuf];
  double ld = 0.0;
  for (int k = 1 + tid; k <= n; k += bs) ld += log(sqrt(s_piv[k]));
  const double logdet = block_sum(ld, s_red);
  // gradient: 0.5 * sum_ij (alpha_i alpha_j - Kinv_ij) dK_ij; off-diagonal tiles stand for both triangles
  double gc = 0.0, gl = 0.0, gn = 0.0;
  if (active) {
    const double wt = (ti == tj) ? 1.0 : 2.0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int i = 4 * ti + a, j = 4 * tj + b;
        if (i >= 1 && j >= 1 && i <= n && j <= n) {
          const double inner = al[i] * al[j] + T[a][b];  // T = -Kinv
          if (i == j) {
            gc += inner * c;
            gn += inner * (nl * s_w[i]);
          } else {
            double R, dR;
            corr_and_dlog(E, s_x[i], s_x[j], R, dR);
            gc += wt * inner * (c * R);
            gl += wt * inner * (c * dR);
          }
        }
      }
  }
  gc = block_sum(gc, s_red);
  gl = block_sum(gl, s_red);
  gn = block_sum(gn, s_red);
  if (tid == 0) {
    const double yta = -al[0];
    const double lml = -0.5 * yta - logdet - 0.5 * (double)n * 1.8378770664093453;  // log(2 pi)
    f_out[pb] = -lml;
    g_out[3 * pb] = -0.5 * gc;
    g_out[3 * pb + 1] = -0.5 * gl;
    g_out[3 * pb + 2] = -0.5 * gn;
  }
}

// The same kernel for 128 < n <= 250 training points (small delta_x): two tiles per thread (t and t + blockDim), up to
// 63 x 64 / 2 = 2016 tiles on 1024 threads.  Kept separate so that the common sizes keep their lean single-tile code.
#define LML2_MAXD 260
__global__ void __launch_bounds__(1024) k_lml2(EdgeDev* edges, const int* edge_of, const double* theta, double* f_out,
                                               double* g_out, const int* count) {
  constexpr int SLOTS = 2;  // (three and four tiles per thread were measured: 163 / 203 VGPRs, 6-40 % slower)
  const int pb = blockIdx.x;
  if (count != nullptr && pb >= *count) return;
  const EdgeDev E = edges[edge_of[pb]];
  const int n = E.fin_n;
  const int nb = (n + 1 + 3) >> 2;
  const int ntile = nb * (nb + 1) / 2;
  __shared__ __attribute__((aligned(16))) double s_col[2][LML2_MAXD];
  __shared__ double s_x[LML2_MAXD], s_y[LML2_MAXD], s_w[LML2_MAXD];  // x / l, y, noise weights at index 1..n
  __shared__ double s_piv[LML2_MAXD];
  __shared__ double s_red[16];
  const int tid = threadIdx.x, bs = blockDim.x;
  bool active[SLOTS];
  int ti[SLOTS], tj[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int t = tid + s * bs;
    int r = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > t) --r;
    while ((r + 1) * (r + 2) / 2 <= t) ++r;
    ti[s] = r;
    tj[s] = t - r * (r + 1) / 2;
    active[s] = t < ntile;
  }
  const double c = exp(theta[3 * pb]), ell = exp(theta[3 * pb + 1]), nl = exp(theta[3 * pb + 2]);
  for (int i = tid; i < 4 * nb; i += bs) {
    const bool in = (i >= 1 && i <= n);
    s_x[i] = in ? E.fin_x[i - 1] / ell : 0.0;
    s_y[i] = in ? E.fin_y[i - 1] : 0.0;
    s_w[i] = in ? E.fin_w[i - 1] : 0.0;
    s_piv[i] = 1.0;
  }
  __syncthreads();
  double T[SLOTS][4][4];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s)
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int i = 4 * ti[s] + a, j = 4 * tj[s] + b;
        double v = 0.0;
        if (active[s] && i <= n && j <= n) {
          if (i == 0 || j == 0) {
            v = (i == j) ? 0.0 : s_y[i + j];
          } else if (i == j) {
            v = c + nl * s_w[i];
            v = v + 1e-6;
          } else {
            v = c * corr_fn(E, s_x[i], s_x[j]);
          }
        }
        T[s][a][b] = v;
      }
  bool bad = false, stop = false;
  for (int kb = 0; kb < nb && !stop; ++kb) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int k = 4 * kb + kk;
      const int buf = kk & 1;
      if (k == 0) continue;  // the y border is not a pivot
      if (k > n) {
        stop = true;
        break;
      }
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        if (active[s]) {
          if (tj[s] == kb) {
#pragma unroll
            for (int a = 0; a < 4; ++a) s_col[buf][4 * ti[s] + a] = T[s][a][kk];
            if (ti[s] == kb) s_piv[k] = T[s][kk][kk];
          } else if (ti[s] == kb) {
#pragma unroll
            for (int b = 0; b < 4; ++b) s_col[buf][4 * tj[s] + b] = T[s][kk][b];
          }
        }
      }
      __syncthreads();
      const double d = s_col[buf][k];
      if (!(d > 0.0)) {  // not positive definite (same for every thread)
        bad = true;
        stop = true;
        break;
      }
      double inv = __builtin_amdgcn_rcp(d);
      inv = inv * (2.0 - d * inv);
      inv = inv * (2.0 - d * inv);
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        if (active[s]) {
          double ci[4], cj[4];
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            ci[a] = s_col[buf][4 * ti[s] + a];
            cj[a] = s_col[buf][4 * tj[s] + a];
          }
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const double ma = -(ci[a] * inv);
#pragma unroll
            for (int b = 0; b < 4; ++b) T[s][a][b] = fma(ma, cj[b], T[s][a][b]);
          }
          if (ti[s] == kb) {
#pragma unroll
            for (int b = 0; b < 4; ++b) T[s][kk][b] = cj[b] * inv;
          }
          if (tj[s] == kb) {
#pragma unroll
            for (int a = 0; a < 4; ++a) T[s][a][kk] = ci[a] * inv;
            if (ti[s] == kb) T[s][kk][kk] = -inv;
          }
        }
      }
    }
  }
  if (bad) {  // sklearn returns (-inf, 0) -> objective (+inf, -0)
    if (tid == 0) {
      f_out[pb] = INFINITY;
      g_out[3 * pb] = g_out[3 * pb + 1] = g_out[3 * pb + 2] = 0.0;
    }
    return;
  }
  const int fbuf = (n + 1) & 1;
#pragma unroll
  for (int s = 0; s < SLOTS; ++s)
    if (active[s] && tj[s] == 0) {
#pragma unroll
      for (int a = 0; a < 4; ++a) s_col[fbuf][4 * ti[s] + a] = T[s][a][0];
    }
  __syncthreads();
  const double* al = s_col[fbuf];
  double ld = 0.0;
  for (int k = 1 + tid; k <= n; k += bs) ld += log(sqrt(s_piv[k]));
  const double logdet = block_sum(ld, s_red);
  double gc = 0.0, gl = 0.0, gn = 0.0;
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    if (active[s]) {
      const double wt = (ti[s] == tj[s]) ? 1.0 : 2.0;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int i = 4 * ti[s] + a, j = 4 * tj[s] + b;
          if (i >= 1 && j >= 1 && i <= n && j <= n) {
            const double inner = al[i] * al[j] + T[s][a][b];  // T = -Kinv
            if (i == j) {
              gc += inner * c;
              gn += inner * (nl * s_w[i]);
            } else {
              double R, dR;
              corr_and_dlog(E, s_x[i], s_x[j], R, dR);
              gc += wt * inner * (c * R);
              gl += wt * inner * (c * dR);
            }
          }
        }
    }
  }
  gc = block_sum(gc, s_red);
  gl = block_sum(gl, s_red);
  gn = block_sum(gn, s_red);
  if (tid == 0) {
    const double yta = -al[0];
    const double lml = -0.5 * yta - logdet - 0.5 * (double)n * 1.8378770664093453;  // log(2 pi)
    f_out[pb] = -lml;
    g_out[3 * pb] = -0.5 * gc;
    g_out[3 * pb + 1] = -0.5 * gl;
    g_out[3 * pb + 2] = -0.5 * gn;
  }
}

// ---------------------------------------------------------------------------------------
// f2 on the matrix cores (round 3; n <= 108 training points on a lattice): the same symmetric sweep of the bordered
// matrix, FOUR pivots at a time, on 16x16 tiles of v_mfma_f64_16x16x4_f64.
//
// Layout of the bordered matrix (size n4 + 1 <= 112, n4 = n rounded up to a multiple of 4): indices 0..n-1 = K,
// n..n4-1 = identity padding (pivots 1: log 1 = 0, no coupling), n4 = the y border (never a pivot), the rest zero.
// The lower triangle of 16x16 tiles (diagonal tiles whole) lives in the accumulator registers of TWO waves: wave
// `role` owns the tile rows {6, 3, 1, 0} (role 0) and {5, 4, 2} (role 1): 14 tiles each.  ONE instruction stream serves
// both: 16 static accumulator slots (g, J), J < 7 - 2 g, whose tile row l16_row(g, role) is a scalar of the wave; slot
// (g, J) is in use when J <= that row -- 12 slots in both waves, two in one of them each.  (Two separate streams were
// built first: the register allocator kept both sets of accumulators apart -- 224 + 165 registers, one wave per SIMD.
// On this chip the f64 MFMA runs on the vector unit's own FMA lanes -- SQ_VALU_MFMA_BUSY_CYCLES + the VALU issue cycles
// add up to the kernel's time, nothing overlaps between the waves of a SIMD -- so what counts is the SUM of MFMA and
// VALU cycles of the busier wave: the split 16 + 12 of {6, 4, 2, 0} / {5, 3, 1} cost 128 cycles a step more.)
// f64 C/D layout: lane (q = l >> 4, col = l & 15), register r holds element (row q + 4 r, column col) of its tile;
// A operand: lane holds A[row = col][k = q], B operand: B[k = q][column = col].
//
// A block step for the pivots k0..k0+3 (tile Jp, sub-block B; W = columns k0..k0+3 of the matrix = the PANEL, in LDS
// k-major, copied out of the tiles at the end of the previous step; P = its rows k0..k0+3):
//   P = L D L^T in every lane (unit lower L; the four pivots d are the squared Cholesky diagonal in the scalar order);
//   Y = W L^-T row by row, straight from the panel (each lane the rows 16 J + col of all seven tile columns: six FMAs
//   each; component q of them are its B operands, four of them -- its own tile rows -- its A operands);
//   the four rank-one updates of the scalar sweep as ONE MFMA per tile:  T -= (Y D^-1) Y^T,  A operand -Y[row][q] / d_q,
//   B operand Y[column][q] -- the scalar algorithm's own arithmetic, no product with an explicit P^-1;
//   the pivot rows and columns must become (W P^-1)^T and W P^-1: the A operand of the four pivot rows is
//   Linv[q][i'] / d_q - L[i'][q] instead, the B operand of the four pivot columns Y[j'][q] - Linv[q][j']: the MFMA
//   then yields T_pj - W_jp + (W P^-1)_jp with the first two cancelling to the rounding of Y -- no accumulator touched;
//   the 4x4 block of the pivots gets both and becomes 2 I - P^-1: the epilogue takes the 2 off the diagonal;
//   the next panel is copied into the other panel buffer (one scalar jump on its tile column); ONE barrier per step.
// n^3 / 2 FMAs of the scalar sweep become 25 x 28 MFMAs (1024 FMAs each, 68 % useful at n = 98).  The training x sit on
// a lattice (pixel columns), so the correlation and its length-scale derivative are tabulated at the integer lags once
// per problem: lagmax + 1 transcendentals instead of n^2 for the set-up and n^2 more for the gradient.
// ---------------------------------------------------------------------------------------
typedef double v4d __attribute__((ext_vector_type(4)));
// row stride of the panel planes in doubles (>= 112 rows).  120: 240 dwords = 48 mod the 64 banks, so the four k-planes start
// 0 / 48 / 32 / 16 banks apart -- the panel copy's writes (16 lanes: four planes x four consecutive rows) and the row writes
// (four planes x sixteen columns) fall on disjoint banks.  (112 = 32 mod 64 put planes 0 / 2 and 1 / 3 on the same banks:
// 35 % of the LDS-active cycles were bank conflicts; 836 -> 800 us per 13 312 problems, the same bits.)
#ifndef L16_WS
#define L16_WS 120
#endif
#define L16_MAXN 108  // 4 * ceil(n / 4) + 1 <= 112
#define L16_NT 7
#define L16_LAG_MAX 4096  // longest correlation table (2 x 32 KB of LDS per problem)
#define L16_NG 4
#define L16_NS 16
__host__ __device__ constexpr int l16_sg(int t) { return t < 7 ? 0 : (t < 12 ? 1 : (t < 15 ? 2 : 3)); }  // slot -> group
__host__ __device__ constexpr int l16_sj(int t) { return t < 7 ? t : (t < 12 ? t - 7 : (t < 15 ? t - 12 : 0)); }  // slot -> tile column
// tile row of group g of wave `role`: {6, 3, 1, 0} and {5, 4, 2} -- 14 tiles each (-1: role 1 has no fourth tile row)
__host__ __device__ constexpr int l16_row(int g, int role) { return g == 0 ? 6 - role : (g == 1 ? 3 + role : (g == 2 ? 1 + role : -role)); }
// slot (g, J) belongs to both waves / to one of them only (the widest tile of the group's lower tile row)
__host__ __device__ constexpr int l16_owner(int g, int J) {  // 2: both, 0 / 1: that role only
  return g == 0 ? (J == 6 ? 0 : 2) : (g == 1 ? (J == 4 ? 1 : 2) : (g == 2 ? (J == 2 ? 1 : 2) : 0));
}

struct L16Shared {
  double Wt[2][4][L16_WS];  // panel of the current / next block step, k-major
  double al[L16_WS];        // alpha (row n4 of the swept matrix)
  double y[L16_WS], w[L16_WS];
  double piv[L16_WS];
  int m[L16_WS];            // lattice coordinate of training point i
  double red[8];
};

__device__ __forceinline__ double l16_rcp(double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = r * (2.0 - d * r);
  r = r * (2.0 - d * r);
  return r;
}

__device__ __forceinline__ double l16_sel(const v4d& a, int r) {
  return r == 0 ? a[0] : (r == 1 ? a[1] : (r == 2 ? a[2] : a[3]));
}

struct L16Acc {
  v4d v[L16_NS];
};

// copy the panel of pivot block (Jn, BN) out of the tiles: W[row][a] = A[row][16 Jn + 4 BN + a].  Per tile row of the wave at
// most ONE tile has the panel's columns (tile column Jn: a scalar jump picks its slot) and at most one tile row has its
// rows (the tile row Jn itself, whose register BN holds the panel rows of the tile columns left of it, by symmetry).
// (the empty asm with a different immediate per case keeps the cases apart: merged, they become ONE store sequence behind
// a phi of accumulator ADDRESSES, and those accumulators then live in scratch memory)
#define L16_COLPART(slot)                                       \
  if (pcn) {                                                    \
    const double t0_ = A.v[slot][0], t1_ = A.v[slot][1], t2_ = A.v[slot][2], t3_ = A.v[slot][3]; \
    asm volatile("; l16 panel from slot %0" ::"n"(slot));      \
    wc[0] = t0_;                                                \
    wc[4] = t1_;                                                \
    wc[8] = t2_;                                                \
    wc[12] = t3_;                                               \
  }
// ONE scalar jump on the tile column Jn of the next pivots; inside a case everything but the wave's role is a constant:
// the tiles (I, Jn) of the tile rows I >= Jn hold the panel's columns, and the tile row Jn itself -- which exactly one
// of the two waves owns -- holds its rows for the tile columns left of it.
template <int BN, int JN, int G>
__device__ __forceinline__ void l16_extract_col(const L16Acc& A, double* Wn, int role, int q, int col) {
  constexpr int base = G == 0 ? 0 : (G == 1 ? 7 : (G == 2 ? 12 : 15));
  constexpr int lo = l16_row(G, 0) < l16_row(G, 1) ? l16_row(G, 0) : l16_row(G, 1);
  constexpr int hi = l16_row(G, 0) < l16_row(G, 1) ? l16_row(G, 1) : l16_row(G, 0);
  if constexpr (JN <= hi) {
    if (JN <= lo || role == (l16_row(G, 0) == hi ? 0 : 1)) {  // this wave's tile row of the group is not above the pivots
      const bool pcn = (col >> 2) == BN;
      double* wc = Wn + (col & 3) * L16_WS + 16 * l16_row(G, role) + q;
      L16_COLPART(base + JN)
    }
  }
}
template <int BN, int JN>
__device__ __forceinline__ void l16_extract_case(const L16Acc& A, double* Wn, int role, int q, int col) {
  l16_extract_col<BN, JN, 0>(A, Wn, role, q, col);
  l16_extract_col<BN, JN, 1>(A, Wn, role, q, col);
  l16_extract_col<BN, JN, 2>(A, Wn, role, q, col);
  l16_extract_col<BN, JN, 3>(A, Wn, role, q, col);
  // tile row JN = l16_row(G, par)
  constexpr int par = (JN == 5 || JN == 4 || JN == 2) ? 1 : 0, G = JN >= 5 ? 0 : (JN >= 3 ? 1 : (JN >= 1 ? 2 : 3));
  static_assert(l16_row(G, par) == JN, "owner of the tile row");
  constexpr int base = G == 0 ? 0 : (G == 1 ? 7 : (G == 2 ? 12 : 15));
  if (JN > 0 && role == par) {
    double* wr = Wn + q * L16_WS + col;
#pragma unroll
    for (int J = 0; J < JN; ++J) {
      const double t_ = A.v[base + J][BN];
      asm volatile("; l16 panel row from slot %0" ::"n"(base + J));
      wr[16 * J] = t_;
    }
  }
}
template <int BN>
__device__ __forceinline__ void l16_extract(const L16Acc& A, double* Wn, int Jn, int role, int q, int col) {
  switch (Jn) {
    case 0: l16_extract_case<BN, 0>(A, Wn, role, q, col); break;
    case 1: l16_extract_case<BN, 1>(A, Wn, role, q, col); break;
    case 2: l16_extract_case<BN, 2>(A, Wn, role, q, col); break;
    case 3: l16_extract_case<BN, 3>(A, Wn, role, q, col); break;
    case 4: l16_extract_case<BN, 4>(A, Wn, role, q, col); break;
    case 5: l16_extract_case<BN, 5>(A, Wn, role, q, col); break;
    default: l16_extract_case<BN, 6>(A, Wn, role, q, col); break;
  }
}

#ifdef GPET_L16_PROF  // cycles per phase of a block step (wave 0 of workgroup 0 prints them)
#define L16_STAMP(i) { const long long t_ = clock64(); prof[i] += t_ - tl; tl = t_; }
#else
#define L16_STAMP(i)
#endif
// one block step (pivots 16 Jp + 4 B ..); false: a pivot was not positive
template <int B>
__device__ __forceinline__ bool l16_step(L16Acc& A, L16Shared& S, int Jp, int n4, int role, int q, int col
#ifdef GPET_L16_PROF
                                         , long long* prof, long long& tl
#endif
) {
  constexpr int buf = B & 1;  // (four steps per tile: the parity of the step is the parity of B)
  const int k0 = 16 * Jp + 4 * B;
  const double* W = &S.Wt[buf][0][0];
  // P = L D L^T (uniform: every lane reads the same ten entries), the four pivots one after the other: d_k are the
  // squared Cholesky diagonal in the scalar order.  (Elimination by 2x2 blocks with adjugates halves this dependent
  // chain -- 740 instead of ~1100 cycles of a 3500-cycle step -- but forms X = Pb Pa^-1 and the Schur complement from
  // differences of products: 6e-7 relative on the objective at c / noise = 4e4 where this form gives 6e-12.  Dropped.)
  const double p00 = W[k0], p10 = W[k0 + 1], p20 = W[k0 + 2], p30 = W[k0 + 3];
  const double p11 = W[L16_WS + k0 + 1], p21 = W[L16_WS + k0 + 2], p31 = W[L16_WS + k0 + 3];
  const double p22 = W[2 * L16_WS + k0 + 2], p32 = W[2 * L16_WS + k0 + 3];
  const double p33 = W[3 * L16_WS + k0 + 3];
  const double i0 = l16_rcp(p00);
  const double l10 = p10 * i0, l20 = p20 * i0, l30 = p30 * i0;
  const double u11 = fma(-p10, l10, p11), u21 = fma(-p20, l10, p21), u31 = fma(-p30, l10, p31);
  const double i1 = l16_rcp(u11);
  const double l21 = u21 * i1, l31 = u31 * i1;
  const double u22 = fma(-u21, l21, fma(-p20, l20, p22));
  const double u32 = fma(-u31, l21, fma(-p30, l20, p32));
  const double i2 = l16_rcp(u22);
  const double l32 = u32 * i2;
  const double u33 = fma(-u32, l32, fma(-u31, l31, fma(-p30, l30, p33)));
  const double i3 = l16_rcp(u33);
  const bool ok = p00 > 0.0 && u11 > 0.0 && u22 > 0.0 && u33 > 0.0;  // (the same in every lane of both waves)
  if (role == 0 && (q | col) == 0) {
    S.piv[k0] = p00;
    S.piv[k0 + 1] = u11;
    S.piv[k0 + 2] = u22;
    S.piv[k0 + 3] = u33;
  }
  const bool pc = (col >> 2) == B;  // this lane's row (A operand) / column (tile) index is one of the pivots
  const int kc = col & 3;
  const int lb = q * L16_WS + col;
  // Per lane, from the uniform factors: row q of L^-1 (component q of a row of Y = W L^-T is its product with the four
  // panel entries of that row),  ykq = Linv[q][kc],  lkq = L[kc][q],  iq = 1 / d_q.
  const double m20 = fma(l21, l10, -l20), m31 = fma(l32, l21, -l31);  // L^-1 below its first subdiagonal (uniform)
  const double m30 = fma(-l32, m20, fma(l31, l10, -l30));
  const double cq0 = q == 0 ? 1.0 : (q == 1 ? -l10 : (q == 2 ? m20 : m30));
  const double cq1 = q == 1 ? 1.0 : (q == 2 ? -l21 : (q == 3 ? m31 : 0.0));
  const double cq2 = q == 2 ? 1.0 : (q == 3 ? -l32 : 0.0);
  const double cq3 = q == 3 ? 1.0 : 0.0;
  const double iq = q == 0 ? i0 : (q == 1 ? i1 : (q == 2 ? i2 : i3));
  const double ykq = kc == 0 ? cq0 : (kc == 1 ? cq1 : (kc == 2 ? cq2 : cq3));
  const double lrow1 = q == 0 ? l10 : (q == 1 ? 1.0 : 0.0);                                      // L[1][q]
  const double lrow2 = q == 0 ? l20 : (q == 1 ? l21 : (q == 2 ? 1.0 : 0.0));                   // L[2][q]
  const double lrow3 = q == 0 ? l30 : (q == 1 ? l31 : (q == 2 ? l32 : 1.0));                   // L[3][q]
  const double lkq = kc == 0 ? (q == 0 ? 1.0 : 0.0) : (kc == 1 ? lrow1 : (kc == 2 ? lrow2 : lrow3));
  L16_STAMP(0)
  // Y = W L^-T row by row (the scalar sweep's own arithmetic: four rank-one updates in a row), component q of it is what
  // a lane contributes: the rank-4 update is  T -= (Y D^-1) Y^T  -- A operand -Y[row][q] / d_q, B operand Y[column][q].
  // (The first form of this kernel multiplied W by the explicit P^-1: entries of size 1 / lambda_min(P) against W's
  // 433 cancel to O(1) -- 1e-6 relative on the objective at c / noise = 4e4 where the scalar sweep gives 6e-12.)
  // Pivot rows and columns through the operands: pivot row i' carries A = Linv[q][i'] / d_q - L[i'][q], so the MFMA
  // yields T_pj - W_jp + (W P^-1)_jp (the first two cancel to the rounding of Y); pivot column j' carries
  // B = Y[j'][q] - Linv[q][j'] for the mirror image.  The 4x4 block of the pivots gets both: with Y = L D on the
  // pivot rows the product is 2 I - P^-1 - P, so the block becomes 2 I - P^-1 (P cancels to its own rounding, 1e-16 of
  // entries a hundred times smaller than those of P^-1); the epilogue takes the 2 off the diagonal of the swept
  // matrix.  No accumulator is written outside the MFMAs.
  // Every wave forms ALL the rows of Y it needs from the panel itself: its B operands are component q of the rows of
  // all seven tile columns, its A operands those of its own four tile rows among them -- 7 instead of 4 short chains
  // per lane, and no plane of Y through LDS, no second barrier in the step.
  double yv[L16_NT];
#pragma unroll
  for (int J = 0; J < L16_NT; ++J) {
    const double* wr = W + 16 * J + col;
    yv[J] = fma(cq0, wr[0], fma(cq1, wr[L16_WS], fma(cq2, wr[2 * L16_WS], cq3 * wr[3 * L16_WS])));
  }
  double aop[L16_NG];
  {
    const double niq = -iq;
    aop[0] = (role ? yv[l16_row(0, 1)] : yv[l16_row(0, 0)]) * niq;
    aop[1] = (role ? yv[l16_row(1, 1)] : yv[l16_row(1, 0)]) * niq;
    aop[2] = (role ? yv[l16_row(2, 1)] : yv[l16_row(2, 0)]) * niq;
    aop[3] = yv[0] * niq;  // (role 1 has no fourth tile row: its slot 15 is never multiplied)
    const double apiv = fma(ykq, iq, -lkq);
#pragma unroll
    for (int g = 0; g < L16_NG; ++g) aop[g] = ((role ? l16_row(g, 1) : l16_row(g, 0)) == Jp && pc) ? apiv : aop[g];
  }
  L16_STAMP(1)
  double bop[L16_NT];
  {
    const double bdel = pc ? ykq : 0.0;
#pragma unroll
    for (int J = 0; J < L16_NT; ++J) bop[J] = fma(-bdel, (J == Jp) ? 1.0 : 0.0, yv[J]);  // (the factor is a scalar of the wave)
  }
  // one MFMA per tile
#pragma unroll
  for (int t = 0; t < L16_NS; ++t) {
    const int g = l16_sg(t), J = l16_sj(t);
    if (l16_owner(g, J) != 2) continue;
    A.v[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[g], bop[J], A.v[t], 0, 0, 0);
  }
  if (role == 0) {
#pragma unroll
    for (int t = 0; t < L16_NS; ++t) {
      const int g = l16_sg(t), J = l16_sj(t);
      if (l16_owner(g, J) != 0) continue;
      A.v[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[g], bop[J], A.v[t], 0, 0, 0);
    }
  } else {
#pragma unroll
    for (int t = 0; t < L16_NS; ++t) {
      const int g = l16_sg(t), J = l16_sj(t);
      if (l16_owner(g, J) != 1) continue;
      A.v[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[g], bop[J], A.v[t], 0, 0, 0);
    }
  }
  L16_STAMP(2)
  L16_STAMP(3)
  // next panel
  if (k0 + 4 < n4) l16_extract<(B + 1) & 3>(A, &S.Wt[buf ^ 1][0][0], B == 3 ? Jp + 1 : Jp, role, q, col);
  L16_STAMP(4)
  return ok;
}

__device__ __forceinline__ void l16_run(L16Shared& S, const double2* tab, int n, int n4, int nt, double c, double nl, int pb,
                                        double* f_out, double* g_out) {
  const int lane = threadIdx.x & 63, q = lane >> 4, col = lane & 15;
  const int role = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  L16Acc A;
#ifdef GPET_L16_PROF
  const long long t_entry = clock64();
#endif
  // tiles.  First every slot as if it were an off-diagonal tile of training points: correlation from the table only, all
  // loads independent of each other (the lattice coordinates are zero beyond the training set: any lag is inside the
  // table).  Then the special tiles again, properly: diagonal tiles and the tile row with the padding and the border.
  {
    int mi[L16_NG][4], mjv[L16_NT];
#pragma unroll
    for (int g = 0; g < L16_NG; ++g) {
      const int I = l16_row(g, role) < 0 ? 0 : l16_row(g, role);
#pragma unroll
      for (int r = 0; r < 4; ++r) mi[g][r] = S.m[16 * I + q + 4 * r];
    }
#pragma unroll
    for (int J = 0; J < L16_NT; ++J) mjv[J] = S.m[16 * J + col];
#pragma unroll
    for (int t = 0; t < L16_NS; ++t) {
      const int g = l16_sg(t), J = l16_sj(t);
#pragma unroll
      for (int r = 0; r < 4; ++r) A.v[t][r] = c * tab[abs(mi[g][r] - mjv[J])].x;
    }
  }
#pragma unroll
  for (int t = 0; t < L16_NS; ++t) {
    const int I = l16_row(l16_sg(t), role), J = l16_sj(t);
    const int j = 16 * J + col;
    if (J > I) {  // (a slot this wave does not use)
      A.v[t] = (v4d){0.0, 0.0, 0.0, 0.0};
    } else if (J < I && 16 * I + 16 > n) {
      // off-diagonal tile of a tile row that reaches beyond the training set: kernel entries where both indices are
      // training points, y in the border row, zero elsewhere (no diagonal, no padding pivot in it)
      const double yj = S.y[j];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ii = 16 * I + q + 4 * r;
        A.v[t][r] = (ii < n && j < n) ? A.v[t][r] : ((ii == n4 && j < n) ? yj : 0.0);
      }
    } else if (J == I) {
      // diagonal tile: every candidate value is loaded (the arrays are zero beyond the training set) and the right one
      // selected -- no divergent branches
      const double yj = S.y[j];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ii = 16 * I + q + 4 * r;
        const int ic = (ii >= 0 && ii < L16_WS) ? ii : 0;
        const double dg = (c + nl * S.w[ic]) + 1e-6;
        const double yi = S.y[ic];
        const bool in = ii < n && j < n;
        double v = in ? (ii == j ? dg : A.v[t][r]) : 0.0;
        v = (!in && ii == j && ii < n4) ? 1.0 : v;
        v = (ii == n4 && j < n) ? yj : v;
        v = (j == n4 && ii < n) ? yi : v;
        A.v[t][r] = v;
      }
    }
  }
  l16_extract<0>(A, &S.Wt[0][0][0], 0, role, q, col);
  __syncthreads();
  bool ok = true;
#ifdef GPET_L16_PROF
  long long prof[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  long long tl = clock64();
  const long long t_begin = tl;
#define L16_PROF_ARGS , prof, tl
#else
#define L16_PROF_ARGS
#endif
  for (int Jp = 0; 16 * Jp < n4; ++Jp) {
    ok = l16_step<0>(A, S, Jp, n4, role, q, col L16_PROF_ARGS) && ok;
    __syncthreads();
    L16_STAMP(5)
    if (16 * Jp + 4 < n4) ok = l16_step<1>(A, S, Jp, n4, role, q, col L16_PROF_ARGS) && ok;
    __syncthreads();
    L16_STAMP(5)
    if (16 * Jp + 8 < n4) ok = l16_step<2>(A, S, Jp, n4, role, q, col L16_PROF_ARGS) && ok;
    __syncthreads();
    L16_STAMP(5)
    if (16 * Jp + 12 < n4) ok = l16_step<3>(A, S, Jp, n4, role, q, col L16_PROF_ARGS) && ok;
    __syncthreads();
    L16_STAMP(5)
  }
#ifdef GPET_L16_PROF
  const long long t_loop_end = clock64();
#endif
  if (!ok) {  // sklearn returns (-inf, 0) -> objective (+inf, -0)
    if (threadIdx.x == 0) {
      f_out[pb] = INFINITY;
      g_out[3 * pb] = g_out[3 * pb + 1] = g_out[3 * pb + 2] = 0.0;
    }
    return;
  }
  // alpha = row n4 of the swept matrix, its corner = -y^T alpha
  const int It = n4 >> 4, rq = n4 & 15, qs = rq & 3, rs = rq >> 2;
#pragma unroll
  for (int t = 0; t < L16_NS; ++t) {
    const int I = l16_row(l16_sg(t), role), J = l16_sj(t);
    if (I == It && J <= I) {
      const double v = l16_sel(A.v[t], rs);
      if (q == qs) S.al[16 * J + col] = v;
    }
  }
  __syncthreads();
  const double* al = S.al;
  double ld = 0.0;
  for (int k = (int)threadIdx.x; k < n; k += 128) ld += log(sqrt(S.piv[k]));  // (both waves: a log is ~80 instructions)
  // gradient: 0.5 * sum_ij (alpha_i alpha_j - Kinv_ij) dK_ij; off-diagonal tiles stand for both triangles.
  // sR, sD: sums of inner_ij R_ij and inner_ij dR_ij over i != j (c applied at the end); gd, gn: the diagonal terms.
  // Same two passes as the set-up: every slot that is an off-diagonal tile of training points without a branch inside,
  // then the special tiles element by element with selects.
  double sR = 0.0, sD = 0.0, gd = 0.0, gn = 0.0;
  double ai[L16_NG][4];
  int mi[L16_NG][4], mjv[L16_NT];
#pragma unroll
  for (int g = 0; g < L16_NG; ++g) {
    const int I = l16_row(g, role) < 0 ? 0 : l16_row(g, role);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ai[g][r] = al[16 * I + q + 4 * r];
      mi[g][r] = S.m[16 * I + q + 4 * r];
    }
  }
#pragma unroll
  for (int J = 0; J < L16_NT; ++J) mjv[J] = S.m[16 * J + col];
#pragma unroll
  for (int t = 0; t < L16_NS; ++t) {
    const int g = l16_sg(t), J = l16_sj(t);
    const int I = l16_row(g, role);
    const int j = 16 * J + col;
    const double aj = al[j];
    if (J < I && 16 * I + 16 <= n) {  // (all rows and columns are training points, none on the diagonal)
      double tR = 0.0, tD = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double inner = fma(ai[g][r], aj, A.v[t][r]);  // T = -Kinv
        const double2 rd = tab[abs(mi[g][r] - mjv[J])];
        tR = fma(inner, rd.x, tR);
        tD = fma(inner, rd.y, tD);
      }
      sR = fma(2.0, tR, sR);
      sD = fma(2.0, tD, sD);
    } else if (J < I) {  // (off-diagonal tile of a tile row that reaches beyond the training set)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ii = 16 * I + q + 4 * r;
        const double inner = fma(ai[g][r], aj, A.v[t][r]);
        const double2 rd = tab[abs(mi[g][r] - mjv[J])];
        const bool od = ii < n && j < n;
        sR += od ? 2.0 * inner * rd.x : 0.0;
        sD += od ? 2.0 * inner * rd.y : 0.0;
      }
    } else if (J == I) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ii = 16 * I + q + 4 * r;
        const int ic = (ii >= 0 && ii < L16_WS) ? ii : 0;
        const double inner = fma(ai[g][r], aj, A.v[t][r] - ((ii == j) ? 2.0 : 0.0));  // (the pivot blocks hold 2 I - P^-1: l16_step)
        const double2 rd = tab[abs(mi[g][r] - mjv[J])];
        const bool in = ii < n && j < n;
        const bool dg = in && ii == j, od = in && ii != j;
        gd += dg ? inner : 0.0;
        gn += dg ? inner * (nl * S.w[ic]) : 0.0;
        sR += od ? inner * rd.x : 0.0;
        sD += od ? inner * rd.y : 0.0;
      }
    }
  }
  double gc = c * (sR + gd), gl = c * sD;
  ld = wave_sum(ld);
  gc = wave_sum(gc);
  gl = wave_sum(gl);
  gn = wave_sum(gn);
  if (role == 1 && lane == 0) {
    S.red[0] = gc;
    S.red[1] = gl;
    S.red[2] = gn;
    S.red[3] = ld;
  }
  __syncthreads();
#ifdef GPET_L16_PROF
  if (blockIdx.x == 0 && lane == 0)
    printf("l16 role %d: set-up %lld, loop %lld (solve %lld, operands %lld, mfma %lld, diag %lld, extract %lld, barrier %lld), epilogue %lld cycles\n",
           role, (long long)(t_begin - t_entry), (long long)(t_loop_end - t_begin), prof[0], prof[1], prof[2], prof[3], prof[4], prof[5],
           (long long)(clock64() - t_loop_end));
#endif
  if (threadIdx.x == 0) {
    gc += S.red[0];
    gl += S.red[1];
    gn += S.red[2];
    ld += S.red[3];
    const double yta = -al[n4];
    const double lml = -0.5 * yta - ld - 0.5 * (double)n * 1.8378770664093453;  // log(2 pi)
    f_out[pb] = -lml;
    g_out[3 * pb] = -0.5 * gc;
    g_out[3 * pb + 1] = -0.5 * gl;
    g_out[3 * pb + 2] = -0.5 * gn;
  }
}

#ifndef GPET_L16_WAVES
#define GPET_L16_WAVES 2  // waves per SIMD (3 spills 44 doubles in the block step: tools/build_instrumented.sh -DGPET_L16_WAVES=3 to try)
#endif
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(GPET_L16_WAVES, GPET_L16_WAVES))) k_lml16(EdgeDev* edges, const int* edge_of, const double* theta, double* f_out,
                                               double* g_out, const int* count, int lag_cap) {
  const int pb = blockIdx.x;
#ifdef GPET_L16_PROF
  const long long t_kernel = clock64();
#endif
  if (count != nullptr && pb >= *count) return;  // (launches are sized by the host's last KNOWN number of running problems)
  const EdgeDev E = edges[edge_of[pb]];
  const int n = E.fin_n;
  const int n4 = (n + 3) & ~3;
  const int nt = (n4 + 1 + 15) >> 4;
  __shared__ L16Shared S;
  extern __shared__ double2 l16_tab[];  // [lag_cap]: (correlation, d/dlog(length scale)) at the lattice lags
  const int tid = threadIdx.x;
  const double c = exp(theta[3 * pb]), ell = exp(theta[3 * pb + 1]), nl = exp(theta[3 * pb + 2]);
  const double hinv = E.fin_par[9];
  const int lagmax = (int)E.fin_par[10];
  if (!(hinv > 0.0) || lagmax < 0 || lagmax >= lag_cap || n > L16_MAXN) {  // the host routes such sets to k_lml / k_lml2: fail loudly
    if (tid == 0) {
      f_out[pb] = NAN;
      g_out[3 * pb] = g_out[3 * pb + 1] = g_out[3 * pb + 2] = 0.0;
      E.sc->status = GPET_ERR_STATE;
    }
    return;
  }
  const double x0 = E.fin_x[0];
  for (int i = tid; i < L16_WS; i += 128) {
    const bool in = i < n;
    S.y[i] = in ? E.fin_y[i] : 0.0;
    S.w[i] = in ? E.fin_w[i] : 0.0;
    S.m[i] = in ? (int)rint((E.fin_x[i] - x0) * hinv) : 0;
    S.piv[i] = 1.0;
    S.al[i] = 0.0;
  }
  // the zero fill of both panel buffers: rows beyond the matrix are never written but are read as operands of tiles
  // nobody uses
  for (int i = tid; i < 2 * 4 * L16_WS; i += 128) (&S.Wt[0][0][0])[i] = 0.0;
  // the correlation as sklearn evaluates it for two inputs a lag apart: a = x_i / l, b = x_j / l, d = a - b
  for (int m = tid; m <= lagmax; m += 128) {
    double R, dR;
    corr_and_dlog(E, ((double)m / hinv) / ell, 0.0, R, dR);
    l16_tab[m] = make_double2(R, dR);
  }
  __syncthreads();
#ifdef GPET_L16_PROF
  if (blockIdx.x == 0 && tid == 0) printf("l16 staging + table: %lld cycles\n", (long long)(clock64() - t_kernel));
#endif
  l16_run(S, l16_tab, n, n4, nt, c, nl, pb, f_out, g_out);
}

// The converged fit of one (edge, restart) problem from its start point to its optimum in ONE workgroup: objective
// (the block sweep above) -> L-BFGS-B state machine (lb_advance, thread 0, the problem's state in LDS) -> next trial
// point, until the machine says done.  Problems do not talk to each other, so there is nothing to synchronise across
// workgroups and no residency requirement: a launch of P workgroups of which only some fit the GPU just runs them in
// generations.  Against the round-based driver (one objective launch + one k_lb_advance launch per round of ALL running
// problems, a counter read-back every fourth round) this takes the launch gaps and the host round trips out of a
// problem's chain of ~50 evaluations and stages its training set once instead of once per evaluation.
// counters[0] += evaluations, counters[1] = max evaluations of a problem, counters[2] += problems cut off at max_evals.
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(GPET_L16_WAVES, GPET_L16_WAVES))) k_lml16_fit(EdgeDev* edges, LbProb* probs, LbCfg cfg, int lag_cap,
                                                                                                                 int max_evals, int* counters) {
  const int pb = blockIdx.x;
  __shared__ L16Shared S;
  __shared__ LbProb sp;
  __shared__ double s_fg[4];
  extern __shared__ double2 l16_tab[];
  const int tid = threadIdx.x;
  {
    const int* src = reinterpret_cast<const int*>(&probs[pb]);
    int* dst = reinterpret_cast<int*>(&sp);
    for (int i = tid; i < (int)(sizeof(LbProb) / sizeof(int)); i += 128) dst[i] = src[i];
  }
  __syncthreads();
  // (only what the loop needs of the edge's record.  The kernel still spills -- 114 vector registers around the set-up,
  //  the gradient epilogue and the call of the state machine, none inside the block steps)
  const EdgeDev* Ep = &edges[sp.edge];
  EdgeDev E = {};
  E.kernel_type = Ep->kernel_type;
  E.nu_code = Ep->nu_code;
  E.nu_gen = Ep->nu_gen;
  E.inv_gamma_nu = Ep->inv_gamma_nu;
  E.fin_n = Ep->fin_n;
  E.fin_par = Ep->fin_par;
  E.fin_x = Ep->fin_x;
  E.fin_y = Ep->fin_y;
  E.fin_w = Ep->fin_w;
  E.sc = Ep->sc;
  const int n = E.fin_n;
  const int n4 = (n + 3) & ~3;
  const int nt = (n4 + 1 + 15) >> 4;
  const double hinv = E.fin_par[9];
  const int lagmax = (int)E.fin_par[10];
  if (!(hinv > 0.0) || lagmax < 0 || lagmax >= lag_cap || n > L16_MAXN) {  // (the host routes such sets to the round-based driver)
    if (tid == 0) {
      E.sc->status = GPET_ERR_STATE;
      atomicAdd(&counters[2], 1);
    }
    return;
  }
  const double x0 = E.fin_x[0];
  for (int i = tid; i < L16_WS; i += 128) {
    const bool in = i < n;
    S.y[i] = in ? E.fin_y[i] : 0.0;
    S.w[i] = in ? E.fin_w[i] : 0.0;
    S.m[i] = in ? (int)rint((E.fin_x[i] - x0) * hinv) : 0;
  }
  int evals = 0;
  for (;;) {
    const double c = exp(sp.xe[0]), ell = exp(sp.xe[1]), nl = exp(sp.xe[2]);
    for (int i = tid; i < L16_WS; i += 128) {
      S.piv[i] = 1.0;
      S.al[i] = 0.0;
    }
    for (int i = tid; i < 2 * 4 * L16_WS; i += 128) (&S.Wt[0][0][0])[i] = 0.0;
    for (int m = tid; m <= lagmax; m += 128) {
      double R, dR;
      corr_and_dlog(E, ((double)m / hinv) / ell, 0.0, R, dR);
      l16_tab[m] = make_double2(R, dR);
    }
    __syncthreads();
    l16_run(S, l16_tab, n, n4, nt, c, nl, 0, &s_fg[0], &s_fg[1]);  // (thread 0 leaves f and the gradient in s_fg)
    ++evals;
    if (tid == 0) {
      double lo[3] = {cfg.lo[0], cfg.lo[1], cfg.lo[2]}, hi[3] = {cfg.hi[0], cfg.hi[1], cfg.hi[2]};
      const double gk[3] = {s_fg[1], s_fg[2], s_fg[3]};
      lb_advance(sp, s_fg[0], gk, lo, hi);
    }
    __syncthreads();
    if (sp.task == LB_TASK_DONE || evals >= max_evals) break;
  }
  {
    int* dst = reinterpret_cast<int*>(&probs[pb]);
    const int* src = reinterpret_cast<const int*>(&sp);
    for (int i = tid; i < (int)(sizeof(LbProb) / sizeof(int)); i += 128) dst[i] = src[i];
  }
  if (tid == 0) {
    atomicAdd(&counters[0], evals);
    atomicMax(&counters[1], evals);
    if (sp.task != LB_TASK_DONE) atomicAdd(&counters[2], 1);
  }
}

bool lml16_fit_applies(int n_max, int lag_cap) {
  return n_max <= L16_MAXN && lag_cap > 0 && lag_cap <= L16_LAG_MAX;
}

hipError_t launch_lml16_fit(hipStream_t st, EdgeDev* d_edges, void* d_probs, int P, const LbCfg& cfg, int lag_cap, int max_evals,
                            int* d_counters) {
  (void)hipGetLastError();
  const size_t dyn = (size_t)2 * lag_cap * sizeof(double);
  hipLaunchKernelGGL(k_lml16_fit, dim3(P), dim3(128), dyn, st, d_edges, static_cast<LbProb*>(d_probs), cfg, lag_cap, max_evals,
                     d_counters);
  return hipGetLastError();
}

hipError_t launch_lml(hipStream_t st, EdgeDev* d_edges, int P, int n_max, const int* d_edge_of, const double* d_theta,
                      double* d_f, double* d_g, const int* d_count, int lag_cap) {
  (void)hipGetLastError();
  if (n_max > 250) return hipErrorInvalidValue;
  // up to 108 training points on a lattice (lag_cap > 0: every training set of the launch sits on one with fewer than
  // lag_cap points; the caller knows): the block sweep on the matrix cores, two waves per problem, correlation tables
  // of lag_cap entries in dynamic LDS
  if (n_max <= L16_MAXN && lag_cap > 0 && lag_cap <= L16_LAG_MAX) {
    const size_t dyn = (size_t)2 * lag_cap * sizeof(double);
    hipLaunchKernelGGL(k_lml16, dim3(P), dim3(128), dyn, st, d_edges, d_edge_of, d_theta, d_f, d_g, d_count, lag_cap);
    return hipGetLastError();
  }
  // two tiles per thread: the only form above 128 training points, and the faster one for big launches (fewer
  // instructions per problem: 109 instead of 134 us at 900 problems of 98 points, 1.07 instead of 1.41 ms at 13312) --
  // small launches are latency-bound and keep one tile per thread (64 instead of 80 us at 256 problems)
  if (n_max > 128 || opt(Opt::lml_two_tiles_from) <= P) {
    const int nb2 = (n_max + 1 + 3) >> 2;
    const int tiles = nb2 * (nb2 + 1) / 2;
    int threads = (((tiles + 1) / 2 + 63) / 64) * 64;
    if (threads > 1024) threads = 1024;
    hipLaunchKernelGGL(k_lml2, dim3(P), dim3(threads), 0, st, d_edges, d_edge_of, d_theta, d_f, d_g, d_count);
    return hipGetLastError();
  }
  const int nb = (n_max + 1 + 3) >> 2;
  const int threads = ((nb * (nb + 1) / 2 + 63) / 64) * 64;  // one thread per 4x4 tile of the lower triangle
  hipLaunchKernelGGL(k_lml, dim3(P), dim3(threads), 0, st, d_edges, d_edge_of, d_theta, d_f, d_g, d_count);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// f2 for MORE than 250 training points (wide edges with a small delta_x): the objective of one L-BFGS-B problem is
// evaluated with the blocked HBM kernels of the many-point fit -- every problem becomes a VIRTUAL edge of a scratch
// table (training set = the edge's standardised set, K / L / alpha / L^-1 in per-problem scratch, amplitude, length
// scale and noise level = the problem's theta):
//   K tiles -> blocked Cholesky (MFMA SYRK) -> alpha -> X = L^-1 (blocked substitution on the identity) ->
//   tiles of K^-1 = X^T X on the matrix cores, contracted on the fly with dK/dtheta (k_lmlbig_grad) -> f, g.
// ~2.5 n^3 flops per evaluation instead of n^3, ~100 launches per round: a rare path, kept simple.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_lmlbig_setup(EdgeDev* edges, int P, const int* edge_of, const double* theta,
                                                     EdgeDev* vedges, gpet_scalars* vsc, double* scratch, size_t per_prob,
                                                     int ncap_v) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const EdgeDev E = edges[edge_of[p]];
  EdgeDev V = E;
  const double c = exp(theta[3 * p]), l = exp(theta[3 * p + 1]), nl = exp(theta[3 * p + 2]);
  double* base = scratch + (size_t)p * per_prob;
  V.xt = E.fin_x;
  V.yt = E.fin_y;
  V.wt = E.fin_w;
  V.K = base;
  V.V = base + (size_t)ncap_v * ncap_v;
  V.alpha = V.V + (size_t)ncap_v * ncap_v;
  V.chol_inv = nullptr;  // (the blocked objective solves by substitution: k_chol_trsm_sub, k_struct_trsm)
  V.n_cap = ncap_v;
  V.Lg = ncap_v;  // column count / stride of V in the blocked substitution; != n, so the weights are not zeroed again
  V.length_scale = l;
  V.noise_y = nl;
  V.jitter = 1e-6;
  V.structured = 0;
  V.tab_ok = 0;  // standardised coordinates, the problem's own length scale
  V.sc = vsc + p;
  gpet_scalars s;
  s.y_s = 1.0;
  s.amp = c;
  s.y_mean = 0.0;
  s.y_std = 1.0;
  s.score_thresh = 0.0;
  s.lml = 0.0;
  s.n = E.fin_n;
  s.n_obs = 0;
  s.rank = 0;
  s.status = GPET_OK;
  s.iter = 0;
  s.done = 0;
  s.n_removed = 0;
  s.force = 1;
  vsc[p] = s;
  vedges[p] = V;
}

__global__ void __launch_bounds__(256) k_lmlbig_identity(EdgeDev* vedges) {
  const EdgeDev E = vedges[blockIdx.y];
  const int n = E.sc->n, ldu = E.Lg;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < (size_t)n * ldu; e += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(e / ldu), j = (int)(e - (size_t)i * ldu);
    E.V[e] = (i == j) ? 1.0 : 0.0;
  }
}

// tile (bi >= bj) of K^-1 = X^T X, X = L^-1 rows in V, contracted with the three dK/dtheta: partial sums per tile
__global__ void __launch_bounds__(256) k_lmlbig_grad(EdgeDev* vedges, double* part, int nt) {
  const EdgeDev E = vedges[blockIdx.z];
  const gpet_scalars* sc = E.sc;
  const int bi = blockIdx.y, bj = blockIdx.x;
  double* out = part + ((size_t)blockIdx.z * nt * nt + (size_t)bi * nt + bj) * 3;
  const int tid = threadIdx.x;
  if (tid < 3) out[tid] = 0.0;
  if (sc->status != GPET_OK || bj > bi) return;
  const int n = sc->n, ldu = E.Lg;
  const int i0 = bi * 64, j0 = bj * 64;
  if (i0 >= n) return;
  __shared__ double sr[32][65];
  __shared__ double sc_[32][65];
  __shared__ double s_red[16];
  const int lane = tid & 63, w = tid >> 6, li = lane & 15, lq = lane >> 4;
  v4f64 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (v4f64){0.0, 0.0, 0.0, 0.0};
  // X is lower triangular: rows k < i0 contribute nothing to columns >= i0
  for (int k0 = (i0 / 32) * 32; k0 < n; k0 += 32) {
    for (int e = tid; e < 32 * 64; e += 256) {
      const int jj = e & 63, kk = e >> 6;
      const int k = k0 + kk;
      sr[kk][jj] = (k < n && i0 + jj < n) ? E.V[(size_t)k * ldu + i0 + jj] : 0.0;
      sc_[kk][jj] = (k < n && j0 + jj < n) ? E.V[(size_t)k * ldu + j0 + jj] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 32; kk += 4) {
      const double a = sr[kk + lq][16 * w + li];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sc_[kk + lq][16 * t + li], acc[t], 0, 0, 0);
    }
    __syncthreads();
  }
  const double c = sc->amp, length = E.length_scale, nl = E.noise_y;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = j0 + 16 * t + li;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int i = i0 + 16 * w + lq + 4 * g;
      if (i >= n || j > i) continue;
      const double inner = E.alpha[i] * E.alpha[j] - acc[t][g];
      if (i == j) {
        s1 += inner * c;            // d K / d log c on the diagonal: c * 1
        s3 += inner * nl * E.wt[i]; // d K / d log noise_level
      } else {
        double R, dR;
        corr_and_dlog(E, E.xt[i] / length, E.xt[j] / length, R, dR);
        s1 += 2.0 * inner * (c * R);
        s2 += 2.0 * inner * (c * dR);
      }
    }
  }
  s1 = block_sum(s1, s_red);
  s2 = block_sum(s2, s_red);
  s3 = block_sum(s3, s_red);
  if (tid == 0) {
    out[0] = s1;
    out[1] = s2;
    out[2] = s3;
  }
}

// f = -log marginal likelihood, g = its gradient (sklearn_gpr.py:521-585); non-PD -> +inf, 0
__global__ void __launch_bounds__(256) k_lmlbig_finish(EdgeDev* vedges, const double* part, int nt, double* f_out, double* g_out) {
  const int p = blockIdx.x;
  const EdgeDev E = vedges[p];
  const gpet_scalars* sc = E.sc;
  __shared__ double s_red[16];
  const int tid = threadIdx.x, n = sc->n, ld = E.n_cap;
  if (sc->status != GPET_OK) {
    if (tid == 0) {
      f_out[p] = INFINITY;
      g_out[3 * p] = g_out[3 * p + 1] = g_out[3 * p + 2] = 0.0;
    }
    return;
  }
  double ya = 0.0, ld_ = 0.0;
  for (int i = tid; i < n; i += blockDim.x) {
    ya += E.yt[i] * E.alpha[i];
    ld_ += log(E.K[(size_t)i * ld + i]);
  }
  ya = block_sum(ya, s_red);
  ld_ = block_sum(ld_, s_red);
  if (tid == 0) {
    double s[3] = {0.0, 0.0, 0.0};
    const double* pp = part + (size_t)p * nt * nt * 3;
    for (int t = 0; t < nt * nt; ++t)  // fixed order: reproducible sums
      for (int q = 0; q < 3; ++q) s[q] += pp[3 * t + q];
    f_out[p] = 0.5 * ya + ld_ + 0.5 * (double)n * 1.8378770664093453;  // log(2 pi)
    for (int q = 0; q < 3; ++q) g_out[3 * p + q] = -0.5 * s[q];
  }
}

size_t lmlbig_scratch_doubles(int ncap_v) { return 2 * (size_t)ncap_v * ncap_v + ncap_v; }

hipError_t launch_lml_big(hipStream_t st, EdgeDev* d_edges, int P, int n_max, const int* d_edge_of, const double* d_theta,
                          double* d_f, double* d_g, void* d_vedges, void* d_vsc, double* d_scratch, double* d_part,
                          int ncap_v) {
  (void)hipGetLastError();
  EdgeDev* ve = (EdgeDev*)d_vedges;
  const int nt = ncap_v / CB;
  hipLaunchKernelGGL(k_lmlbig_setup, dim3(cdiv(P, 64)), dim3(64), 0, st, d_edges, P, d_edge_of, d_theta, ve,
                     (gpet_scalars*)d_vsc, d_scratch, lmlbig_scratch_doubles(ncap_v), ncap_v);
  const int ntn = cdiv(n_max, CB);  // tiles that can hold training points
  hipLaunchKernelGGL(k_fit_kbuild, dim3(ntn, ntn, P), dim3(256), 0, st, ve);
  for (int k0 = 0; k0 < n_max; k0 += CB) {
    hipLaunchKernelGGL(k_chol_diag, dim3(1, P), dim3(256), 0, st, ve, k0, 0);
    const int below = cdiv(n_max - k0 - CB, CB);
    if (below > 0) {
      hipLaunchKernelGGL(k_chol_trsm_sub, dim3(below, P), dim3(256), 0, st, ve, k0);
      hipLaunchKernelGGL(k_chol_syrk, dim3(below, below, P), dim3(256), 0, st, ve, k0, 0);
    }
  }
  hipLaunchKernelGGL(k_chol_solve, dim3(1, P), dim3(256), (size_t)ncap_v * sizeof(double), st, ve);
  hipLaunchKernelGGL(k_lmlbig_identity, dim3(256, P), dim3(256), 0, st, ve);
  const int cgroups = cdiv(n_max, SB_COLS);
  for (int k0 = 0; k0 < n_max; k0 += CB) hipLaunchKernelGGL(k_struct_trsm, dim3(cgroups, P), dim3(256), 0, st, ve, k0, 1);
  hipLaunchKernelGGL(k_lmlbig_grad, dim3(nt, nt, P), dim3(256), 0, st, ve, d_part, nt);
  hipLaunchKernelGGL(k_lmlbig_finish, dim3(P), dim3(256), 0, st, ve, d_part, nt, d_f, d_g);
  return hipGetLastError();
}

