// Part of gpet_kernels.hip (included there, inside namespace gpet, in this order): a2-a5: training set, K, Cholesky, alpha (one workgroup per edge; blocked in HBM above 128 points) and predict, with the blocked predict of many training points.
// ---------------------------------------------------------------------------------------
// a2-a4  training-set assembly + K_obs + Cholesky + alpha   (one workgroup per edge)
//        gpet.py:209-231, sklearn_gpr.py:221-227, 304-320
// ---------------------------------------------------------------------------------------
// K_IN_LDS: the n x n matrix lives in LDS (n_cap <= 128, odd row stride) and only the finished
// factor is written to HBM; otherwise it is factored in place in HBM (large n, config 3).
// FINAL: the converged fit at the optimum found by L-BFGS-B (gpet.py:232-266): training set,
// amplitude, length scale and noise come from fin_x/fin_y/fin_w/fin_par instead of the loop state.
#define FIT_MAXD 136  // 4 * ceil((128 + 1) / 4) + slack
template <bool K_IN_LDS, bool FINAL>
__global__ void __launch_bounds__(576) k_fit(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  gpet_scalars* sc = E.sc;
  if (!FINAL && ((sc->done && !sc->force) || sc->status != GPET_OK)) return;
  extern __shared__ double s_dyn[];  // [n_cap] solve vector (+ [n_cap * ld] matrix when K_IN_LDS)
  __shared__ double s_red[16];
  __shared__ double s_diag;
  const int tid = threadIdx.x, bs = blockDim.x;
#ifdef GPET_FIT_PROF
  const long long f0 = clock64();
  long long f1 = f0;
#endif
  // (readfirstlane: a count that comes out of memory through a vector load is "divergent" to the compiler, and so is every loop
  //  bound derived from it -- the pivot loop then runs on exec masks)
  const int n_obs = __builtin_amdgcn_readfirstlane(sc->n_obs);
  const int n = FINAL ? E.fin_n : (E.n_init + n_obs);
  const int ld = K_IN_LDS ? (E.n_cap | 1) : E.n_cap;
  double* K = K_IN_LDS ? (s_dyn + E.n_cap) : E.K;
  double amp, length, noise_lvl, jit;
  if (FINAL) {
    for (int i = tid; i < n; i += bs) {
      E.xt[i] = E.fin_x[i];
      E.yt[i] = E.fin_y[i];
      E.wt[i] = E.fin_w[i];
    }
    amp = E.fin_par[0];
    length = E.fin_par[1];
    noise_lvl = E.fin_par[2];
    jit = 1e-6;
    if (tid == 0) {
      sc->amp = amp;
      sc->y_mean = E.fin_par[7];
      sc->y_std = E.fin_par[8];
      sc->n = n;
    }
    __syncthreads();
  } else {

  // 1. gather + stable rank sort by x (np.argsort, gpet.py:212)
  const double w_init = E.fix_endpoints ? 1e-7 : 0.5;  // gpet.py:161
  // (the x values go through LDS -- the solve vector is free until step 5 -- when they fit: the rank count then reads
  //  them as broadcasts instead of paying one global round trip per comparison)
  long long* s_xs = reinterpret_cast<long long*>(s_dyn);
  const bool x_in_lds = n <= E.n_cap;
  if (x_in_lds) {
    for (int j = tid; j < n; j += bs) s_xs[j] = (j < E.n_init) ? E.init_xy[2 * j] : E.obs_xy[2 * (j - E.n_init)];
    __syncthreads();
  }
  for (int i = tid; i < n; i += bs) {
    const long long* pi = (i < E.n_init) ? (E.init_xy + 2 * i) : (E.obs_xy + 2 * (i - E.n_init));
    const long long xi = pi[0], yi = pi[1];
    int r = 0;
    if (x_in_lds) {
#pragma unroll 8
      for (int j = 0; j < n; ++j) {
        const long long xj = s_xs[j];
        r += (xj < xi) || (xj == xi && j < i);
      }
    } else {
      for (int j = 0; j < n; ++j) {
        const long long xj = (j < E.n_init) ? E.init_xy[2 * j] : E.obs_xy[2 * (j - E.n_init)];
        r += (xj < xi) || (xj == xi && j < i);
      }
    }
    E.xt[r] = (double)xi;
    E.yt[r] = (double)yi;
    E.wt[r] = (i < E.n_init) ? w_init : 1.0;
  }
  __syncthreads();

#ifdef GPET_FIT_PROF
  f1 = clock64();
#endif
  // 2. y scaling (gpet.py:228-230) then centring (sklearn_gpr.py:222-227)
  double part = 0.0;
  for (int i = tid; i < n; i += bs) part += E.yt[i];
  const double m1 = block_sum(part, s_red) / n;
  part = 0.0;
  for (int i = tid; i < n; i += bs) {
    const double d = E.yt[i] - m1;
    part += d * d;
  }
  const double y_s = sqrt(block_sum(part, s_red) / n) + 1.0;
  part = 0.0;
  for (int i = tid; i < n; i += bs) {
    const double v = E.yt[i] / y_s;
    E.yt[i] = v;
    part += v;
  }
  const double m2 = block_sum(part, s_red) / n;
  part = 0.0;
  for (int i = tid; i < n; i += bs) {
    const double d = E.yt[i] - m2;
    part += d * d;
  }
  double sd2 = sqrt(block_sum(part, s_red) / n);
  if (sd2 == 0.0) sd2 = 1.0;  // _handle_zeros_in_scale scalar path
  for (int i = tid; i < n; i += bs) E.yt[i] -= m2;
  amp = E.sigma_f * E.sigma_f / (y_s * y_s);
  length = E.length_scale;
  noise_lvl = E.noise_y;
  jit = E.jitter;
  if (tid == 0) {
    sc->y_s = y_s;
    sc->amp = amp;
    sc->y_mean = m2;
    sc->y_std = sd2;
    sc->n = n;
  }
  __syncthreads();
  }  // !FINAL

#ifdef GPET_FIT_PROF
  const long long f2 = clock64();
#endif
  // 3. K = amp * rho + diag(noise_y * w) + jitter     (lower triangle only)
  //    inputs are divided by l exactly as sklearn does (X / length_scale)
  const bool zero_noise = (n == E.Lg);  // sklearn_gpr.py:673-677
  for (int idx = tid; idx < n * n; idx += bs) {
    const int i = idx / n, j = idx - i * n;
    if (j > i) continue;
    double v;
    if (i == j) {
      v = amp;
      v = v + ((zero_noise && !FINAL) ? 0.0 : noise_lvl * E.wt[i]);  // (FINAL: the host already zeroed w)
      v = v + jit;
    } else {
      v = amp * (FINAL ? corr_fn(E, E.xt[i] / length, E.xt[j] / length) : corr_px(E, E.xt[i], E.xt[j], length));
    }
    K[(size_t)i * ld + j] = v;
  }
  __syncthreads();

#ifdef GPET_FIT_PROF
  const long long f3 = clock64();
#endif
  // 4. Cholesky, in place.  K in LDS: right-looking -- per step the pivot column is scaled, then every trailing
  //    entry takes its rank-1 update independently (flat loop over the lower triangle of the trailing block):
  //    two barriers and no serial dot products per step.  K in HBM (n > 128): left-looking (read-mostly).
  bool bad = false;
  bool fwd_done = false;  // the forward solve z = L^-1 y came out of the factorisation (K_IN_LDS)
  if (K_IN_LDS) {
    // Right-looking Cholesky of the BORDERED matrix [K; y^T] in registers: thread t owns the 4 x 4 tile (ti, tj),
    // tj <= ti, of the lower triangle (diagonal tiles keep both halves); row n is y^T and is never a pivot, so when
    // the n pivots are done it holds z^T = (L^-1 y)^T -- the forward solve comes for free.  Per pivot: the owners of
    // column k publish it to LDS (double-buffered), ONE barrier, everyone scales its 4 + 4 column entries by
    // 1 / sqrt(d) and takes its rank-1 update (the structure of k_lml's sweep).  The LDS-resident form it replaces
    // needed three barriers, a column pass and a sqrt-indexed sweep over the trailing triangle per pivot: 2 700 cycles
    // a pivot against ~500 (238 k -> 45 k cycles at n = 89, -DGPET_FIT_PROF).
    __shared__ __attribute__((aligned(16))) double s_col[2][FIT_MAXD];
    const int nbt = (n + 1 + 3) >> 2;
    const int ntile = nbt * (nbt + 1) / 2;
    const bool active = tid < ntile;
    int ti = (int)((sqrt(8.0 * (double)tid + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1) / 2 > tid) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= tid) ++ti;
    const int tj = tid - ti * (ti + 1) / 2;
    if (ntile > bs) {  // (cannot happen: n_cap <= 128 and 576 threads)
      if (tid == 0) sc->status = GPET_ERR_RANK_CAP;
      return;
    }
    double T[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int i = 4 * ti + a, j = 4 * tj + b;
        double v = 0.0;
        if (active && i <= n && j < n) {
          if (i == n) v = E.yt[j];
          else v = (j <= i) ? K[(size_t)i * ld + j] : K[(size_t)j * ld + i];
        }
        T[a][b] = v;
      }
    bool stop = false;
    for (int kb = 0; kb < nbt && !stop; ++kb) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int k = 4 * kb + kk;
        const int buf = kk & 1;
        if (k >= n) {
          stop = true;
          break;
        }
        if (active && tj == kb) {
#pragma unroll
          for (int a = 0; a < 4; ++a) s_col[buf][4 * ti + a] = T[a][kk];
        }
        __syncthreads();
        const double d = s_col[buf][k];
        if (!(d > 0.0)) {  // not positive definite (the same value in every thread)
          bad = true;
          stop = true;
          break;
        }
        if (active && ti >= kb) {
          // 1 / sqrt(d) from the hardware seed + two Newton steps (full precision), sqrt(d) = d / sqrt(d): a sqrt and
          // a division per pivot would sit on every thread's critical path in front of the next barrier
          double inv = __builtin_amdgcn_rsq(d);
          inv = inv * (1.5 - 0.5 * d * inv * inv);
          inv = inv * (1.5 - 0.5 * d * inv * inv);
          const double dk = d * inv;
          double ci[4], cj[4];
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            ci[a] = s_col[buf][4 * ti + a] * inv;
            cj[a] = s_col[buf][4 * tj + a] * inv;
          }
          if (tj > kb) {  // strictly below and right of the pivot's tile row / column: no masks
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
              for (int b = 0; b < 4; ++b) T[a][b] = fma(-ci[a], cj[b], T[a][b]);
          } else if (tj == kb) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
              const int i = 4 * ti + a;
#pragma unroll
              for (int b = 0; b < 4; ++b)
                if (i > k && b > kk) T[a][b] = fma(-ci[a], cj[b], T[a][b]);
              if (i > k) T[a][kk] = ci[a];       // column k of L
              else if (i == k) T[a][kk] = dk;
            }
          }
        }
      }
    }
    if (!bad) {
      // the factor back to LDS (lower triangle) for the backward solve, k_struct_H and the readers; z to the solve vector
      __syncthreads();
      if (active) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const int i = 4 * ti + a, j = 4 * tj + b;
            if (i < n && j <= i) K[(size_t)i * ld + j] = T[a][b];
            else if (i == n && j < n) s_dyn[j] = T[a][b];
          }
      }
      __syncthreads();
      fwd_done = true;
    }
  } else {
    for (int j = 0; j < n; ++j) {
      const double* rj = K + (size_t)j * ld;
      for (int i = j + tid; i < n; i += bs) {
        const double* ri = K + (size_t)i * ld;
        double s = ri[j];
        for (int t = 0; t < j; ++t) s -= ri[t] * rj[t];
        if (i == j) s_diag = s; else K[(size_t)i * ld + j] = s;
      }
      __syncthreads();
      const double d = s_diag;
      if (!(d > 0.0)) {
        bad = true;
        break;
      }
      const double dj = sqrt(d);
      for (int i = j + tid; i < n; i += bs) {
        if (i == j) K[(size_t)i * ld + j] = dj; else K[(size_t)i * ld + j] = K[(size_t)i * ld + j] / dj;
      }
      __syncthreads();
    }
  }
  if (bad) {
    if (tid == 0) sc->status = GPET_ERR_NOT_PD;
    return;
  }

#ifdef GPET_FIT_PROF
  const long long f4 = clock64();
#endif
  // 5. alpha = L^-T L^-1 y by one wave in column (axpy) form: the solution vector lives in registers
  //    (rows lane, lane + 64), each step broadcasts one solved component -- no reductions, no barriers
  if (tid < WAVE) {
    const int lane = tid;
    double z0 = (lane < n) ? (fwd_done ? s_dyn[lane] : E.yt[lane]) : 0.0;
    double z1 = (lane + WAVE < n) ? (fwd_done ? s_dyn[lane + WAVE] : E.yt[lane + WAVE]) : 0.0;
    // (n <= 2 * WAVE on this path: n_cap <= 128 whenever K fits LDS; larger n takes the generic loop below)
    if (n <= 2 * WAVE) {
      for (int j = 0; j < n && !fwd_done; ++j) {  // forward: z_j = y_j / l_jj, then y_i -= l_ij z_j for i > j
        const double ljj = K[(size_t)j * ld + j];
        const double zj = __shfl((j < WAVE) ? z0 : z1, j & (WAVE - 1), WAVE) / ljj;
        if (lane == (j & (WAVE - 1))) {
          if (j < WAVE) z0 = zj; else z1 = zj;
        }
        if (lane > j && lane < n) z0 -= K[(size_t)lane * ld + j] * zj;
        if (lane + WAVE > j && lane + WAVE < n) z1 -= K[(size_t)(lane + WAVE) * ld + j] * zj;
      }
      // backward: a_j = z_j / l_jj, then z_i -= l_ji a_j for i < j.  The reciprocals of the diagonal are formed once,
      // before the chain: a step is multiply + shuffle + fused multiply-add instead of carrying a division
      const double ri0 = (lane < n) ? 1.0 / K[(size_t)lane * ld + lane] : 0.0;
      const double ri1 = (lane + WAVE < n) ? 1.0 / K[(size_t)(lane + WAVE) * ld + lane + WAVE] : 0.0;
#pragma unroll 4
      for (int j = n - 1; j >= 0; --j) {
        const double* rj = K + (size_t)j * ld;
        const double aj = wave_bcast((j < WAVE) ? z0 * ri0 : z1 * ri1, j & (WAVE - 1));  // (uniform lane: v_readlane, no LDS permute)
        if (lane == (j & (WAVE - 1))) {
          if (j < WAVE) z0 = aj; else z1 = aj;
        }
        if (lane < j) z0 -= rj[lane] * aj;
        if (lane + WAVE < j) z1 -= rj[lane + WAVE] * aj;
      }
      if (lane < n) E.alpha[lane] = z0;
      if (lane + WAVE < n) E.alpha[lane + WAVE] = z1;
    } else {
      double* z = s_dyn;
      for (int j = 0; j < n; ++j) {
        const double* rj = K + (size_t)j * ld;
        double p = 0.0;
        for (int t = lane; t < j; t += WAVE) p += rj[t] * z[t];
        p = wave_sum(p);
        if (lane == 0) z[j] = (E.yt[j] - p) / rj[j];
      }
      for (int j = n - 1; j >= 0; --j) {
        double p = 0.0;
        for (int t = j + 1 + lane; t < n; t += WAVE) p += K[(size_t)t * ld + j] * z[t];
        p = wave_sum(p);
        if (lane == 0) z[j] = (z[j] - p) / K[(size_t)j * ld + j];
      }
      for (int i = lane; i < n; i += WAVE) E.alpha[i] = z[i];
    }
  }
#ifdef GPET_FIT_PROF
  const long long f5 = clock64();
#endif
  if (K_IN_LDS) {  // publish the factor for k_predict / readers (row stride n_cap in HBM)
    for (int idx = tid; idx < n * n; idx += bs) {
      const int i = idx / n, j = idx - i * n;
      if (j <= i) E.K[(size_t)i * E.n_cap + j] = K[(size_t)i * ld + j];
    }
  }
#ifdef GPET_FIT_PROF
  if (!FINAL && tid == 0 && blockIdx.y == 5)
    printf("k_fit n=%d: sort %lld | scaling %lld | K %lld | cholesky %lld | solves %lld | publish %lld cycles\n", n, f1 - f0, f2 - f1, f3 - f2,
           f4 - f3, f5 - f4, clock64() - f5);
#endif
}

// ---------------------------------------------------------------------------------------
// a2-a4 for MANY training points (n_cap > 128, e.g. config 3's 1500): K and its factor live in HBM and the
// work is spread over the GPU in 64-wide blocks -- head (sort, scaling) -> K tiles -> right-looking blocked
// Cholesky (diagonal block in LDS / row-panel solve / trailing update on the f64 matrix cores) -> blocked solves
// for alpha.  The panel kernels are enqueued for every 64-block of n_cap and return at once past the actual n.
// ---------------------------------------------------------------------------------------
// (CB = 64, the block: gpet_iter_plan.h)
__global__ void __launch_bounds__(1024) k_fit_head(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  __shared__ double s_red[16];
  extern __shared__ long long s_key[];  // [n_cap] x coordinates (the rank of a point = a pass over all of them: from LDS,
                                        // not n global loads per thread -- 1.0 -> 0.05 ms at 1500 points)
  const int tid = threadIdx.x, bs = blockDim.x;
  const int n = E.n_init + sc->n_obs;
  // 1. gather + stable rank sort by x (np.argsort, gpet.py:212)
  const double w_init = E.fix_endpoints ? 1e-7 : 0.5;  // gpet.py:161
  for (int j = tid; j < n; j += bs) s_key[j] = (j < E.n_init) ? E.init_xy[2 * j] : E.obs_xy[2 * (j - E.n_init)];
  __syncthreads();
  for (int i = tid; i < n; i += bs) {
    const long long xi = s_key[i];
    const long long yi = (i < E.n_init) ? E.init_xy[2 * i + 1] : E.obs_xy[2 * (i - E.n_init) + 1];
    int r = 0;
#pragma unroll 8
    for (int j = 0; j < n; ++j) {
      const long long xj = s_key[j];
      r += (xj < xi) || (xj == xi && j < i);
    }
    E.xt[r] = (double)xi;
    E.yt[r] = (double)yi;
    E.wt[r] = (i < E.n_init) ? w_init : 1.0;
  }
  __syncthreads();
  // 2. y scaling (gpet.py:228-230) then centring (sklearn_gpr.py:222-227) -- same arithmetic as k_fit
  double part = 0.0;
  for (int i = tid; i < n; i += bs) part += E.yt[i];
  const double m1 = block_sum(part, s_red) / n;
  part = 0.0;
  for (int i = tid; i < n; i += bs) {
    const double d = E.yt[i] - m1;
    part += d * d;
  }
  const double y_s = sqrt(block_sum(part, s_red) / n) + 1.0;
  part = 0.0;
  for (int i = tid; i < n; i += bs) {
    const double v = E.yt[i] / y_s;
    E.yt[i] = v;
    part += v;
  }
  const double m2 = block_sum(part, s_red) / n;
  part = 0.0;
  for (int i = tid; i < n; i += bs) {
    const double d = E.yt[i] - m2;
    part += d * d;
  }
  double sd2 = sqrt(block_sum(part, s_red) / n);
  if (sd2 == 0.0) sd2 = 1.0;  // _handle_zeros_in_scale scalar path
  for (int i = tid; i < n; i += bs) E.yt[i] -= m2;
  if (tid == 0) {
    sc->y_s = y_s;
    sc->amp = E.sigma_f * E.sigma_f / (y_s * y_s);
    sc->y_mean = m2;
    sc->y_std = sd2;
    sc->n = n;
  }
}

// K = amp * rho + diag(noise_y * w) + jitter, lower 64x64 tiles (as step 3 of k_fit)
__global__ void __launch_bounds__(256) k_fit_kbuild(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.z];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int n = sc->n, ld = E.n_cap;
  const int i0 = blockIdx.y * CB, j0 = blockIdx.x * CB;
  if (j0 > i0 || i0 >= n) return;
  const double amp = sc->amp, length = E.length_scale;
  const bool zero_noise = (n == E.Lg);  // sklearn_gpr.py:673-677
  for (int e = threadIdx.x; e < CB * CB; e += blockDim.x) {
    const int i = i0 + (e >> 6), j = j0 + (e & 63);
    if (i >= n || j > i) continue;
    double v;
    if (i == j) {
      v = amp;
      v = v + (zero_noise ? 0.0 : E.noise_y * E.wt[i]);
      v = v + E.jitter;
    } else {
      v = amp * corr_px(E, E.xt[i], E.xt[j], length);  // (virtual edges of the blocked objective: tab_ok = 0)
    }
    E.K[(size_t)i * ld + j] = v;
  }
}

// diagonal block k0: Cholesky, written back in place, and -- with_inv -- its INVERSE to E.chol_inv: every triangular
// solve against this block (the rows of L below it, V = L^-1 K_*^T) then becomes a 64x64x64 product on the matrix cores.
// RIGHT-looking, four waves, one LDS barrier per pivot: every wave forms column k (lane i: l_ik = a_ik / sqrt(a_kk),
// through a refined reciprocal square root formed one step ahead) and row k of the inverse (lane c: x_kc = b_kc / l_kk, the
// column sweep of L X = I), then updates its own sixteen columns / rows:
//   a_ij -= l_ik l_jk      (lane i, column j of the wave)          b_jc -= l_jk x_kc      (lane c, row j of the wave)
// History: left-looking with one wave, a dot product of length k per pivot as a chain of LDS round trips: 101 us per block
// (2.4 of the 6.1 ms of config 3's fit); the block in LDS, right-looking on four waves in batches of eight columns: 54 us,
// two thirds of it LDS traffic; the block in registers (below).
// (the body: k_chol_diag is one launch of it; k_chol_syrk runs it on the NEXT diagonal block in the workgroup that has just
//  updated that block -- a launch less per panel in the chain of 24 at n = 1500)
__device__ __forceinline__ void chol_diag_body(const EdgeDev& E, gpet_scalars* sc, int k0, int with_inv) {
  const int n = sc->n, ld = E.n_cap;
  if (k0 >= n) return;
  const int nb = (n - k0) < CB ? (n - k0) : CB;
  // The block lives in REGISTERS: lane i = row i, wave w = columns 16 w .. 16 w + 15 of it (a[16]), and rows 16 w .. of the
  // inverse for column `lane` (x[16]).  Per pivot only column k, row k of the inverse and the next pivot's entry go through
  // LDS (published by their owners at the end of the previous step, two buffers by parity: a slow wave may still read the
  // old one), and the 16 l_jk a wave needs are broadcast reads of that column -- a fifth of the LDS traffic of the form that
  // kept the whole block in LDS (54 us per block, 2/3 of it LDS).
  __shared__ double s_col[2][CB];  // column k: a_ik of the partly factorised block
  __shared__ double s_xr[2][CB];   // row k of the inverse's right-hand side
  __shared__ double s_dn[2];       // a_{k+1,k+1} before the update of step k
  const int tid = threadIdx.x, i = tid & 63, w = tid >> 6;
  double a[16], x[16];
  {
    const double* __restrict__ row = E.K + (size_t)(k0 + i) * ld + k0 + 16 * w;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int j = 16 * w + u;
      a[u] = (i < nb && j <= i) ? row[u] : 0.0;
      x[u] = (j == i) ? 1.0 : 0.0;
    }
  }
  if (w == 0) {
    s_col[0][i] = a[0];
    s_xr[0][i] = x[0];
    if (i == 1) s_dn[0] = a[1];
  }
  __syncthreads();
  // (global_store, not flat_store: a FLAT instruction also counts in the LDS wait counter the barrier below waits for)
  __attribute__((address_space(1))) double* inv = (__attribute__((address_space(1))) double*)(E.chol_inv + (size_t)(k0 / CB) * CB * CB);
  __attribute__((address_space(1))) double* kcol = (__attribute__((address_space(1))) double*)(E.K + (size_t)(k0 + i) * ld + k0);
  // the pivot and its reciprocal square root are formed one step AHEAD (a_k+1,k+1 - l_k+1,k^2 is all the update does to the
  // next pivot), so the chain rsq + three Newton steps runs under the update
  double d = s_col[0][0];
  double r = __builtin_amdgcn_rsq(d);
#pragma unroll
  for (int it = 0; it < 3; ++it) r = fma(0.5 * r, fma(-d * r, r, 1.0), r);
#ifdef GPET_CD_PROF
  long long cp[5] = {0, 0, 0, 0, 0};
  long long ct = clock64();
#define CD_T(i) { const long long t_ = clock64(); cp[i] += t_ - ct; ct = t_; }
#else
#define CD_T(i)
#endif
  for (int kp = 0; kp < 4; ++kp) {
#pragma unroll
    for (int ku = 0; ku < 16; ++ku) {
      const int k = 16 * kp + ku;
      if (k >= nb) break;  // (uniform)
      if (!(d > 0.0)) {    // (the same value in every thread: the exit is uniform)
        if (tid == 0) sc->status = GPET_ERR_NOT_PD;
        return;
      }
      const int pb = k & 1;
      const double aik = s_col[pb][i], bk = s_xr[pb][i];
      const int kn = (k + 1 < CB) ? k + 1 : k;
      const double lnk = s_col[pb][kn] * r;
      const double dn = fma(-lnk, lnk, s_dn[pb]);
      double rn = __builtin_amdgcn_rsq(dn);
      const double dk = d * r;
      const double lik = (i > k) ? aik * r : (i == k ? dk : 0.0);
      const double xk = bk * r;
      CD_T(0)
      if (w == (k & 3)) {
        if (i >= k && i < nb) kcol[k] = lik;
        if (with_inv) inv[k * CB + i] = xk;
      }
      CD_T(1)
      // this wave's columns j > k (all sixteen behind the pivot's wave, the later ones in it, none before it)
      // (two straight-line forms, all the column reads of a form first: with the test inside the loop every column paid its
      //  own branch and its own LDS round trip, 1 060 of a pivot's 1 990 cycles on the last wave)
      if (w > kp) {
        double lj[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) lj[u] = s_col[pb][16 * w + u];  // (one address for the wave: a broadcast)
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const double ljk = lj[u] * r;
          a[u] = fma(-lik, ljk, a[u]);
          x[u] = fma(-ljk, xk, x[u]);
        }
      } else if (w == kp) {
        double lj[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) lj[u] = (u > ku) ? s_col[pb][16 * kp + u] : 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          if (u > ku) {  // (a compile-time test: ku and u are unrolled)
            const double ljk = lj[u] * r;
            a[u] = fma(-lik, ljk, a[u]);
            x[u] = fma(-ljk, xk, x[u]);
          }
        }
      }
      CD_T(2)
#pragma unroll
      for (int it = 0; it < 3; ++it) rn = fma(0.5 * rn, fma(-dn * rn, rn, 1.0), rn);
      d = dn;
      r = rn;
      // what the next step reads: column k + 1, row k + 1 of the inverse, the entry of the pivot after it
      if (k + 1 < CB && w == ((k + 1) >> 4)) {
        s_col[pb ^ 1][i] = a[(ku + 1) & 15];
        s_xr[pb ^ 1][i] = x[(ku + 1) & 15];
      }
      if (k + 2 < CB && w == ((k + 2) >> 4) && i == k + 2) s_dn[pb ^ 1] = a[(ku + 2) & 15];
      // (LDS only: __syncthreads() would also wait for the column and the row just stored to HBM)
      CD_T(3)
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      CD_T(4)
    }
  }
#ifdef GPET_CD_PROF
  if ((tid & 63) == 0 && blockIdx.y == 0 && k0 == 0)
    printf("chol_diag wave %d: per pivot: reads + column %lld | stores %lld | update %lld | newton + publish %lld | barrier %lld cycles\n", w,
           cp[0] / nb, cp[1] / nb, cp[2] / nb, cp[3] / nb, cp[4] / nb);
#endif
#undef CD_T
  if (with_inv)  // identity beyond a short last block
    for (int rr = nb + w; rr < CB; rr += 4) inv[rr * CB + i] = (rr == i) ? 1.0 : 0.0;
}
__global__ void __launch_bounds__(256) k_chol_diag(EdgeDev* edges, int k0, int with_inv) {
  const EdgeDev E = edges[blockIdx.y];
  gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  chol_diag_body(E, sc, k0, with_inv);
}

// row blocks below the diagonal block by SUBSTITUTION (one row per lane of the first wave), for the loop's blocked fit and the
// blocked objective of the converged fits alike.  A product with the explicit inverse of the diagonal block on the matrix cores
// (k_chol_trsm, removed) costs digits where the block is nearly singular: the optimiser visits noise levels of 1e-10 of the
// amplitude (2e-8 instead of 1e-9 relative on f = 1.2e8), and the loop's n == Lg sets have only the jitter on K's diagonal
__global__ void __launch_bounds__(256) k_chol_trsm_sub(EdgeDev* edges, int k0) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int n = sc->n, ld = E.n_cap;
  const int i0 = k0 + CB * ((int)blockIdx.x + 1);
  if (i0 >= n) return;
  const int nb = CB;  // (a block below exists only under a full diagonal block)
  const int rows = (n - i0) < CB ? (n - i0) : CB;
  __shared__ double sL[CB][CB + 1];
  __shared__ double sA[CB][CB + 1];
  const int tid = threadIdx.x, bs = blockDim.x;
  for (int e = tid; e < CB * CB; e += bs) {
    const int i = e >> 6, j = e & 63;
    sL[i][j] = (j <= i) ? E.K[(size_t)(k0 + i) * ld + k0 + j] : 0.0;
    sA[i][j] = (i < rows) ? E.K[(size_t)(i0 + i) * ld + k0 + j] : 0.0;
  }
  __syncthreads();
  // in sub-blocks of 16 columns (as k_struct_H's substitution): (a) every thread takes (row, column of the sub-block) entries and
  // subtracts the columns BEFORE the sub-block -- independent inner products, all four waves busy; (b) one lane per row finishes
  // the sub-block's 16 columns.  An entry's terms are subtracted in ascending order either way: the bits of the one-lane-per-row
  // loop over all 64 columns (2 016 dependent steps instead of 480)
  for (int j0 = 0; j0 < nb; j0 += 16) {
    if (j0 > 0) {
      for (int o = tid; o < rows * 16; o += bs) {
        const int i = o >> 4, j = j0 + (o & 15);
        double acc = sA[i][j];
        for (int t = 0; t < j0; ++t) acc -= sA[i][t] * sL[j][t];
        sA[i][j] = acc;
      }
      __syncthreads();
    }
    if (tid < rows) {
      for (int j = j0; j < j0 + 16; ++j) {
        double acc = sA[tid][j];
        for (int t = j0; t < j; ++t) acc -= sA[tid][t] * sL[j][t];
        sA[tid][j] = acc / sL[j][j];
      }
    }
    __syncthreads();
  }
  for (int e = tid; e < rows * CB; e += bs) {
    const int i = e >> 6, j = e & 63;
    E.K[(size_t)(i0 + i) * ld + k0 + j] = sA[i][j];
  }
}

typedef double v4f64c __attribute__((ext_vector_type(4)));

// trailing update A_ij -= X_i X_j^T for the 64x64 tiles (bj <= bi) behind panel k0, v_mfma_f64_16x16x4_f64
// next_diag: the workgroup of the first tile then factors it (the diagonal block of the next panel, with its inverse)
__global__ void __launch_bounds__(256) k_chol_syrk(EdgeDev* edges, int k0, int next_diag) {
  const EdgeDev E = edges[blockIdx.z];
  gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int n = sc->n, ld = E.n_cap;
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj > bi) return;
  const int i0 = k0 + CB * (bi + 1), j0 = k0 + CB * (bj + 1);
  if (i0 >= n) return;
  __shared__ double sI[CB][CB + 1];
  __shared__ double sJ[CB][CB + 1];
  const int tid = threadIdx.x;
  for (int e = tid; e < CB * CB; e += 256) {
    const int i = e >> 6, j = e & 63;
    sI[i][j] = (i0 + i < n) ? E.K[(size_t)(i0 + i) * ld + k0 + j] : 0.0;
    sJ[i][j] = (j0 + i < n) ? E.K[(size_t)(j0 + i) * ld + k0 + j] : 0.0;
  }
  __syncthreads();
  const int lane = tid & 63, w = tid >> 6, li = lane & 15, lq = lane >> 4;
  v4f64c acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (v4f64c){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < CB; kk += 4) {
    const double a = sI[16 * w + li][kk + lq];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sJ[16 * t + li][kk + lq], acc[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int i = i0 + 16 * w + lq + 4 * g, j = j0 + 16 * t + li;
      if (i < n && j <= i) E.K[(size_t)i * ld + j] -= acc[t][g];
    }
  if (next_diag && bi == 0 && bj == 0) {
    __syncthreads();  // (the tile is in memory: hipcc's barrier waits for vmcnt(0))
    chol_diag_body(E, sc, k0 + CB, 1);
  }
}

// alpha = L^-T L^-1 y on the factor in HBM, blocked by 64: diagonal blocks through LDS (column form, one wave).  The
// updates of the rest of the vector read L the way it lies in memory: forward -- the 64 columns of the block, one ROW per
// 64 consecutive lanes' ... per thread group of 16 (a 512-byte run per row); backward -- the 64 ROWS of the block, thread i
// owns vector entry i and walks down the rows (every load a coalesced run).  The vector stays in LDS.
// (One 256-thread workgroup reading the transposed block column by column took 3.2 ms at 1500 points: 5.6 GB/s.)
// the value lane `src` (a compile-time constant at the call sites) holds, in every lane
__device__ __forceinline__ double lane_f64(double v, int src) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, src), hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__global__ void __launch_bounds__(1024) k_chol_solve(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  extern __shared__ double s_z[];  // [n_cap]
  __shared__ double sL[CB][CB + 1];
  const int n = sc->n, ld = E.n_cap;
  const int tid = threadIdx.x, bs = blockDim.x;
  for (int i = tid; i < n; i += bs) s_z[i] = E.yt[i];
  __syncthreads();
  for (int k0 = 0; k0 < n; k0 += CB) {  // forward
    const int nb = (n - k0) < CB ? (n - k0) : CB;
    for (int e = tid; e < nb * nb; e += bs) {
      const int i = e / nb, j = e - i * nb;
      if (j <= i) sL[i][j] = E.K[(size_t)(k0 + i) * ld + k0 + j];
    }
    __syncthreads();
    if (tid < WAVE) {
      // (the 64 dependent steps of a block: lane j's value through v_readlane -- the loop is unrolled, j a constant -- and times
      //  the reciprocal of the diagonal formed by all lanes at once: a division and a ds_bpermute per step were 10 us per block)
      double z = (tid < nb) ? s_z[k0 + tid] : 0.0;
      const double rd = (tid < nb) ? 1.0 / sL[tid][tid] : 0.0;
#pragma unroll
      for (int j = 0; j < CB; ++j) {
        if (j < nb) {
          const double zj = lane_f64(z, j) * lane_f64(rd, j);
          if (tid == j) z = zj;
          if (tid > j && tid < nb) z -= sL[tid][j] * zj;
        }
      }
      if (tid < nb) s_z[k0 + tid] = z;
    }
    __syncthreads();
    // rows below: 16 lanes per row (four columns each, a 512-byte run), summed in the order t = 0..nb-1 per lane and
    // then across the 16 lanes
    for (int i = k0 + nb + (tid >> 4); i < n; i += bs >> 4) {
      const double* ri = E.K + (size_t)i * ld + k0;
      const int t0 = tid & 15;
      // (four loads in flight per lane; entries beyond nb of the last block are not read)
      const double v0 = ri[t0], v1 = t0 + 16 < nb ? ri[t0 + 16] : 0.0, v2 = t0 + 32 < nb ? ri[t0 + 32] : 0.0,
                   v3 = t0 + 48 < nb ? ri[t0 + 48] : 0.0;
      double acc = (t0 < nb ? v0 : 0.0) * s_z[k0 + t0];
      acc += v1 * s_z[k0 + ((t0 + 16) & 63)];
      acc += v2 * s_z[k0 + ((t0 + 32) & 63)];
      acc += v3 * s_z[k0 + ((t0 + 48) & 63)];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 16);
      if ((tid & 15) == 0) s_z[i] -= acc;
    }
    __syncthreads();
  }
  for (int k0 = ((n - 1) / CB) * CB; k0 >= 0; k0 -= CB) {  // backward (L^T)
    const int nb = (n - k0) < CB ? (n - k0) : CB;
    for (int e = tid; e < nb * nb; e += bs) {
      const int i = e / nb, j = e - i * nb;
      if (j <= i) sL[i][j] = E.K[(size_t)(k0 + i) * ld + k0 + j];
    }
    __syncthreads();
    if (tid < WAVE) {
      double z = (tid < nb) ? s_z[k0 + tid] : 0.0;
      const double rd = (tid < nb) ? 1.0 / sL[tid][tid] : 0.0;
#pragma unroll
      for (int j = CB - 1; j >= 0; --j) {
        if (j < nb) {
          const double aj = lane_f64(z, j) * lane_f64(rd, j);
          if (tid == j) z = aj;
          if (tid < j) z -= sL[j][tid] * aj;
        }
      }
      if (tid < nb) s_z[k0 + tid] = z;
    }
    __syncthreads();
    for (int i = tid; i < k0; i += bs) {
      const double* ci = E.K + (size_t)k0 * ld + i;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      int t = 0;
      for (; t + 8 <= nb; t += 8) {  // (eight rows in flight, four partial sums)
        const double u0 = ci[(size_t)t * ld], u1 = ci[(size_t)(t + 1) * ld], u2 = ci[(size_t)(t + 2) * ld], u3 = ci[(size_t)(t + 3) * ld];
        const double u4 = ci[(size_t)(t + 4) * ld], u5 = ci[(size_t)(t + 5) * ld], u6 = ci[(size_t)(t + 6) * ld], u7 = ci[(size_t)(t + 7) * ld];
        a0 = fma(u0, s_z[k0 + t], a0);
        a1 = fma(u1, s_z[k0 + t + 1], a1);
        a2 = fma(u2, s_z[k0 + t + 2], a2);
        a3 = fma(u3, s_z[k0 + t + 3], a3);
        a0 = fma(u4, s_z[k0 + t + 4], a0);
        a1 = fma(u5, s_z[k0 + t + 5], a1);
        a2 = fma(u6, s_z[k0 + t + 6], a2);
        a3 = fma(u7, s_z[k0 + t + 7], a3);
      }
      for (; t < nb; ++t) a0 = fma(ci[(size_t)t * ld], s_z[k0 + t], a0);
      s_z[i] -= (a0 + a1) + (a2 + a3);
    }
    __syncthreads();
  }
  for (int i = tid; i < n; i += bs) E.alpha[i] = s_z[i];
}

// alpha = L^-T L^-1 y for many training points on one workgroup PER 64-ROW BLOCK (k_chol_solve above is one workgroup per
// edge: its 2 x 9 MB of L at n = 1500 come through ONE CU's path to L2, 0.66 ms).  Forward (BACK = false): the workgroup
// of block i subtracts L_ij z_j for j < i as the z_j are published (a flag per block in global memory, its value the
// launch number: nothing to reset), runs the 64-step substitution of its diagonal block and publishes z_i.  Backward
// (BACK = true, a second launch): workgroup x owns block nt - 1 - x and subtracts L_ji^T alpha_j for j > i.  In both a
// workgroup waits only for workgroups with a SMALLER blockIdx.x of the same edge, which the dispatcher started before
// it: no residency requirement.  z / alpha cross XCDs: agent-scope accesses (as k_oj_persist, gpet_eig.hip); the waiting
// thread gives up after 4 s of wall time and fails the edge.  The chain per block: flag + 64 values + one 64 x 64 product + the
// substitution, ~2-3 us.
template <bool BACK>
__global__ void __launch_bounds__(256) k_chol_solve_mw(EdgeDev* edges, int epoch) {
  const EdgeDev E = edges[blockIdx.y];
  gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int n = sc->n, ld = E.n_cap;
  const int nt = (n + CB - 1) / CB;
  if ((int)blockIdx.x >= nt) return;
  const int ib = BACK ? nt - 1 - (int)blockIdx.x : (int)blockIdx.x;
  const int k0 = ib * CB;
  const int nb = (n - k0) < CB ? (n - k0) : CB;
  __shared__ double sL[CB][CB + 1];
  __shared__ double s_y[CB], s_v[CB];
  __shared__ double s_part[4][CB];
  __shared__ int s_ok;
  const int tid = threadIdx.x;
  int* flag_mine = E.solve_flag + (BACK ? (ld / CB + 1) : 0);
  const double* src = BACK ? E.solve_z : E.yt;
  double* dst = BACK ? E.alpha : E.solve_z;
  if (tid < CB) s_y[tid] = 0.0;
  for (int e = tid; e < nb * nb; e += 256) {
    const int i = e / nb, j = e - i * nb;
    if (j <= i) sL[i][j] = E.K[(size_t)(k0 + i) * ld + k0 + j];
  }
  // the off-diagonal blocks in the order their vectors become available; the next one is in registers before the wait
  //   forward:  block (ib, j), thread = (row r = tid >> 2, columns 16 (tid & 3) ..): rows of 512 contiguous bytes
  //   backward: block (j, ib)^T, thread = (column c = tid & 63, rows 16 (tid >> 6) ..): 512 contiguous bytes per row
  const int nsteps = BACK ? nt - 1 - ib : ib;
  double lb[16];
  auto fetch = [&](int step) {
    const int jb = BACK ? nt - 1 - step : step;
    const int j0 = jb * CB;
    const int njb = (n - j0) < CB ? (n - j0) : CB;
    if (!BACK) {
      const int r = tid >> 2, c0 = 16 * (tid & 3);
      const double* row = E.K + (size_t)(k0 + (r < nb ? r : 0)) * ld + j0 + c0;
#pragma unroll
      for (int u = 0; u < 16; ++u) lb[u] = (r < nb) ? row[u] : 0.0;  // (j < ib: a full block of columns)
    } else {
      const int c = tid & 63, r0 = 16 * (tid >> 6);
#pragma unroll
      for (int u = 0; u < 16; ++u) lb[u] = (r0 + u < njb && c < nb) ? E.K[(size_t)(j0 + r0 + u) * ld + k0 + c] : 0.0;
    }
  };
  if (nsteps > 0) fetch(0);
  bool ok = true;
  for (int step = 0; step < nsteps; ++step) {
    const int jb = BACK ? nt - 1 - step : step;
    const int j0 = jb * CB;
    const int njb = (n - j0) < CB ? (n - j0) : CB;
    if (tid == 0) {
      int good = 1;
      const unsigned long long t0 = wall_clock64();  // (constant 100 MHz)
      // acquire: the vector the flag announces is read after it (pairs with the release store below)
      while (__hip_atomic_load(flag_mine + jb, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != epoch) {
        __builtin_amdgcn_s_sleep(1);
        if (wall_clock64() - t0 > 400000000ull) {  // 4 s of wall time: a fault elsewhere, not contention (no residency needed)
          good = 0;
          break;
        }
      }
      s_ok = good;
    }
    __syncthreads();
    if (!s_ok) {
      ok = false;
      break;
    }
    if (tid < CB) s_v[tid] = (tid < njb) ? __hip_atomic_load(dst + j0 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    __syncthreads();
    double acc = 0.0;
    if (!BACK) {
      const int c0 = 16 * (tid & 3);
#pragma unroll
      for (int u = 0; u < 16; ++u) acc = fma(lb[u], s_v[c0 + u], acc);
    } else {
      const int r0 = 16 * (tid >> 6);
#pragma unroll
      for (int u = 0; u < 16; ++u) acc = fma(lb[u], s_v[r0 + u], acc);
    }
    if (step + 1 < nsteps) fetch(step + 1);
    if (!BACK) {
      acc += __shfl_xor(acc, 1, 4);
      acc += __shfl_xor(acc, 2, 4);
      if ((tid & 3) == 0) s_y[tid >> 2] += acc;
    } else {
      s_part[tid >> 6][tid & 63] = acc;
    }
    __syncthreads();
    if (BACK && tid < CB) s_y[tid] += (s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid]);
    // (s_v is rewritten only after the next wait's barrier; s_y is touched by the same threads every step)
  }
  if (!ok) {
    if (tid == 0) sc->status = GPET_ERR_STATE;
    return;
  }
  __syncthreads();
  if (tid < WAVE) {
    // the 64 dependent steps of the diagonal block (k_chol_solve's: lane j's value through v_readlane, reciprocal diagonal)
    double z = (tid < nb) ? src[k0 + tid] - s_y[tid] : 0.0;
    const double rd = (tid < nb) ? 1.0 / sL[tid][tid] : 0.0;
    if (!BACK) {
#pragma unroll
      for (int j = 0; j < CB; ++j) {
        if (j < nb) {
          const double zj = lane_f64(z, j) * lane_f64(rd, j);
          if (tid == j) z = zj;
          if (tid > j && tid < nb) z -= sL[tid][j] * zj;
        }
      }
    } else {
#pragma unroll
      for (int j = CB - 1; j >= 0; --j) {
        if (j < nb) {
          const double aj = lane_f64(z, j) * lane_f64(rd, j);
          if (tid == j) z = aj;
          if (tid < j) z -= sL[j][tid] * aj;
        }
      }
    }
    if (tid < nb) __hip_atomic_store(dst + k0 + tid, z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();  // (every lane's stores are issued and complete: hipcc's barrier waits for vmcnt(0))
  // release: the flag becomes visible at agent scope only after the vector it announces
  if (tid == 0) __hip_atomic_store(flag_mine + ib, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// the whole fit for n_cap > 128
static void launch_fit_blocked(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd) {
  const int nt = cdiv(bd.n_cap, CB);
  hipLaunchKernelGGL(k_fit_head, dim3(1, B), dim3(1024), (size_t)bd.n_cap * sizeof(long long), st, d_edges);
  hipLaunchKernelGGL(k_fit_kbuild, dim3(nt, nt, B), dim3(256), 0, st, d_edges);
  // per panel: [diagonal block] -> rows below it -> trailing update, whose first workgroup goes on to factor the next
  // diagonal block (option "diag_in_syrk" = 0: a launch of its own per diagonal block)
  const int diag_in_syrk = opt(Opt::diag_in_syrk) ? 1 : 0;
  for (int k0 = 0; k0 < bd.n_cap; k0 += CB) {
    if (k0 == 0 || !diag_in_syrk) hipLaunchKernelGGL(k_chol_diag, dim3(1, B), dim3(256), 0, st, d_edges, k0, 1);
    const int below = cdiv(bd.n_cap - k0 - CB, CB);
    if (below > 0) {
      // (by substitution: on n == Lg sets, where K is the jitter away from singular and a 64-column diagonal block has a
      //  condition number of 1e7, the product with the block's explicit inverse left |L L^T - K| at 1.41 times the
      //  factorisation's backward error bound -- tests/test_gpu_struct_injected.py, full130)
      hipLaunchKernelGGL(k_chol_trsm_sub, dim3(below, B), dim3(256), 0, st, d_edges, k0);
      hipLaunchKernelGGL(k_chol_syrk, dim3(below, below, B), dim3(256), 0, st, d_edges, k0, diag_in_syrk);
    }
  }
  // alpha: one workgroup per 64-row block and direction (option "solve_mw" = 0: the single-workgroup kernel)
  if (opt(Opt::solve_mw)) {
    static std::atomic<int> launch_no{0};
    const int epoch = ++launch_no;  // (flags hold the number of the launch that published them: never reset)
    hipLaunchKernelGGL(k_chol_solve_mw<false>, dim3(nt, B), dim3(256), 0, st, d_edges, epoch);
    hipLaunchKernelGGL(k_chol_solve_mw<true>, dim3(nt, B), dim3(256), 0, st, d_edges, epoch);
  } else {
    hipLaunchKernelGGL(k_chol_solve, dim3(1, B), dim3(1024), (size_t)bd.n_cap * sizeof(double), st, d_edges);
  }
}

// ---------------------------------------------------------------------------------------
// a5  predict: K_* on the fly, mean, V = L^-1 K_*^T, std          (thread per grid point)
//     sklearn_gpr.py:381-394, 414-436
//     One wave per 64 grid points.  V_LDS: the wave keeps its 64 columns of V in LDS
//     ([n][64], conflict-free) and streams the rows of L through LDS, so the forward
//     substitution has no global-load latency chain; the HBM copy of V is write-only here.
// ---------------------------------------------------------------------------------------
// FINAL: prediction of the converged fit on the standardised grid (gpet.py:264-266); results go
// to the batch's contiguous output block as mean in pixels and std in standardised units.
template <bool V_LDS, bool FINAL>
__global__ void __launch_bounds__(64) k_predict(EdgeDev* edges, int out_stride) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if (!FINAL && ((sc->done && !sc->force) || sc->status != GPET_OK)) return;
  extern __shared__ double s_dyn[];
  const int lane = threadIdx.x;
  const int j = blockIdx.x * 64 + lane;
  const int n = sc->n, ld = E.n_cap, Lg = E.Lg;
  const bool live = j < Lg;
  const double amp = sc->amp;
  const double length = FINAL ? E.fin_par[1] : E.length_scale;
  double xq = (double)(E.x_st + (live ? j : 0));
  if (FINAL) xq = (xq - E.fin_par[3]) / E.fin_par[4];  // (x_grid - X_m) / X_s
  xq = xq / length;
  double msum = 0.0, vsum = 0.0;
  if (V_LDS) {
    double* s_v = s_dyn;                      // [n_cap][64]
    double* s_l = s_dyn + (size_t)E.n_cap * 64;  // [n_cap] current row of L
    double* s_x = s_l + E.n_cap;              // [n_cap] x_i / l
    double* s_a = s_x + E.n_cap;              // [n_cap] alpha
    for (int i = lane; i < n; i += 64) {
      s_x[i] = E.xt[i] / length;
      s_a[i] = E.alpha[i];
    }
    for (int i = 0; i < n; ++i) {
      __syncthreads();
      const double* ri = E.K + (size_t)i * ld;
      for (int t = lane; t <= i; t += 64) s_l[t] = ri[t];
      __syncthreads();
      const double ki = amp * ((!FINAL && E.nu_code == 3) ? corr_px(E, (double)(E.x_st + (live ? j : 0)), E.xt[i], length) : corr_fn(E, xq, s_x[i]));
      double acc = ki;
      for (int t = 0; t < i; ++t) acc -= s_l[t] * s_v[t * 64 + lane];
      const double v = acc / s_l[i];
      s_v[i * 64 + lane] = v;
      if (live) E.V[(size_t)i * Lg + j] = v;
      msum += ki * s_a[i];
      vsum += v * v;
    }
  } else {
    if (!live) return;
    for (int i = 0; i < n; ++i) {
      const double ki = amp * ((!FINAL && E.nu_code == 3) ? corr_px(E, (double)(E.x_st + j), E.xt[i], length) : corr_fn(E, xq, E.xt[i] / length));
      const double* ri = E.K + (size_t)i * ld;
      double acc = ki;
      for (int t = 0; t < i; ++t) acc -= ri[t] * E.V[(size_t)t * Lg + j];
      const double v = acc / ri[i];
      E.V[(size_t)i * Lg + j] = v;
      msum += ki * E.alpha[i];
      vsum += v * v;
    }
  }
  if (!live) return;
  const double mean = sc->y_std * msum + sc->y_mean;
  double var = amp - vsum;
  if (var < 0.0) var = 0.0;
  const double sd = sqrt(var * (sc->y_std * sc->y_std));
  if (FINAL) {
    E.fin_out[j] = E.fin_par[6] * mean + E.fin_par[5];  // y_s * y_mean + y_m   (gpet.py:266)
    E.fin_out[out_stride + j] = sd;                      // not rescaled (gpet.py:266, quirk Q10)
  } else {
    E.mean[j] = mean;
    E.std[j] = sd;
  }
}

// ---- a5 for many training points (generic path): K_*^T rows into V, mean, blocked V = L^-1 K_*^T, std ----
__global__ void __launch_bounds__(256) k_kstar_build(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.z];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int n = sc->n, Lg = E.Lg;
  const int j = blockIdx.x * 64 + (threadIdx.x & 63);
  const double amp = sc->amp, length = E.length_scale;
  if (j >= Lg) return;
  const double xq = (double)(E.x_st + j) / length;
  for (int i = blockIdx.y * 4 + (threadIdx.x >> 6); i < n; i += gridDim.y * 4)
    E.V[(size_t)i * Lg + j] = amp * corr_px(E, (double)(E.x_st + j), E.xt[i], length);
}
// block k0 of V = L^-1 K_*^T for 32 columns of the grid per workgroup, on the matrix cores:
//   X = K_*^T[k0.., cols] - sum_{j0 < k0} L[k0.., j0..] V[j0.., cols]   (64 x 64 by 64 x 32 products, left-looking),
//   V[k0.., cols] = L_kk^-1 X   (the inverse of the diagonal block from k_chol_diag, with one step of refinement).
// Wave w owns rows 16 w .. 16 w + 15 of the block and both 16-column halves.
#ifndef VS_COLS
#define VS_COLS 16  // grid columns per workgroup (16, 32 or 64 by -DVS_COLS=..; at n = 1500, Lg = 2048: 3.42 / 3.62 / 4.09 ms per fit + predict + covariance, measured with the single product by the inverse, before the refinement step below)
#endif
#define VS_NH (VS_COLS / 16)          // 16-column halves per wave
#define VS_PU (CB * VS_COLS / 256)    // prefetch registers of the V block per thread
__global__ void __launch_bounds__(256) k_vsolve_mfma(EdgeDev* edges, int k0) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int n = sc->n, Lg = E.Lg, ld = E.n_cap;
  const int a0 = blockIdx.x * VS_COLS;
  if (k0 >= n || a0 >= Lg) return;
  const int nb = (n - k0) < CB ? (n - k0) : CB;
  __shared__ double sL[CB][CB + 1];
  __shared__ double sU[CB][VS_COLS + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lq = lane >> 4;
  v4f64c acc[VS_NH];
#pragma unroll
  for (int h = 0; h < VS_NH; ++h) acc[h] = (v4f64c){0.0, 0.0, 0.0, 0.0};
  // the blocks of the next j0 are loaded into registers while the matrix cores work on the current ones (a launch has
  // only Lg / 32 workgroups: nothing else hides the two dependent round trips per block otherwise -- 85 -> ~25 us)
  double pl[16], pu[VS_PU];
  auto fetch = [&](int j0) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int e = tid + 256 * u, i = e >> 6, t = e & 63;
      pl[u] = (i < nb) ? E.K[(size_t)(k0 + i) * ld + j0 + t] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < VS_PU; ++u) {
      const int e = tid + 256 * u, t = e / VS_COLS, a = e % VS_COLS;
      pu[u] = (a0 + a < Lg) ? E.V[(size_t)(j0 + t) * Lg + a0 + a] : 0.0;
    }
  };
  if (k0 > 0) fetch(0);
  for (int j0 = 0; j0 < k0; j0 += CB) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int e = tid + 256 * u;
      sL[e >> 6][e & 63] = pl[u];
    }
#pragma unroll
    for (int u = 0; u < VS_PU; ++u) {
      const int e = tid + 256 * u;
      sU[e / VS_COLS][e % VS_COLS] = pu[u];
    }
    __syncthreads();
    if (j0 + CB < k0) fetch(j0 + CB);
#pragma unroll
    for (int kk = 0; kk < CB; kk += 4) {
      const double a = sL[16 * w + li][kk + lq];
#pragma unroll
      for (int h = 0; h < VS_NH; ++h) acc[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sU[kk + lq][16 * h + li], acc[h], 0, 0, 0);
    }
  }
  __syncthreads();
  // X = B - acc into sU (rows of the block beyond n: zero; a copy stays in registers), the inverse into sL
  // (of a short last block only the leading nb x nb part of the inverse is taken: what the arena holds beyond it is not this
  //  factorisation's, and would meet the zero rows of X and the zero columns of L_kk below as 0 * stale)
  const double* inv = E.chol_inv + (size_t)(k0 / CB) * CB * CB;
  auto load_inverse = [&]() {
    for (int e = tid; e < CB * CB; e += 256) sL[e >> 6][e & 63] = ((e >> 6) < nb && (e & 63) < nb) ? inv[e] : 0.0;
  };
  load_inverse();
  double xr[VS_NH][4];
#pragma unroll
  for (int h = 0; h < VS_NH; ++h)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int i = 16 * w + lq + 4 * g, a = 16 * h + li;
      xr[h][g] = (i < nb && a0 + a < Lg) ? E.V[(size_t)(k0 + i) * Lg + a0 + a] - acc[h][g] : 0.0;
      sU[i][a] = xr[h][g];
    }
  __syncthreads();
  // V[k0.., cols] = L_kk^-1 X in three products on the matrix cores: v0 = Linv X, the residual r = X - L_kk v0, v = v0 + Linv r.
  // The product with the explicit inverse ALONE (what this kernel did) is not a backward-stable solve: its error grows with the
  // block's condition number, and on a training set with only the jitter on K's diagonal -- a point on every column of the edge --
  // the covariance missed the componentwise bound of a substitution by a factor 2.6 (tests/test_gpu_posterior_injected.py).  One
  // step of refinement with the residual formed from L_kk itself takes the inverse's error out to first order (Higham, Accuracy
  // and Stability, ch. 12: fixed-precision refinement of an unstable solver).  Timed on an MI355X as 20 calls of
  // gpet_gp_fit_predict without the covariance, one edge, n = 1500 training points, Lg = 2048, RBF: 2.49 ms with the single product,
  // 2.69 ms with the refinement (8 us for each of the 24 launches); a substitution by groups of 16 lanes, 64 dependent steps per
  // block, gave the same accuracy at 2.89 ms.
  auto block_product = [&](v4f64c* out) {
#pragma unroll
    for (int h = 0; h < VS_NH; ++h) out[h] = (v4f64c){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < CB; kk += 4) {
      const double a = sL[16 * w + li][kk + lq];
#pragma unroll
      for (int h = 0; h < VS_NH; ++h) out[h] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sU[kk + lq][16 * h + li], out[h], 0, 0, 0);
    }
  };
  auto to_sU = [&](const v4f64c* src, bool residual) {  // sU <- src, or <- X - src
#pragma unroll
    for (int h = 0; h < VS_NH; ++h)
#pragma unroll
      for (int g = 0; g < 4; ++g) sU[16 * w + lq + 4 * g][16 * h + li] = residual ? xr[h][g] - src[h][g] : src[h][g];
  };
  v4f64c v0[VS_NH], t[VS_NH];
  block_product(v0);  // v0 = Linv X
  __syncthreads();
  to_sU(v0, false);
  for (int e = tid; e < CB * CB; e += 256) {  // L_kk (zero above the diagonal and beyond a short last block, as the inverse and v0 are)
    const int i = e >> 6, c = e & 63;
    sL[i][c] = (i < nb && c <= i) ? E.K[(size_t)(k0 + i) * ld + k0 + c] : 0.0;
  }
  __syncthreads();
  block_product(t);  // L_kk v0
  __syncthreads();
  to_sU(t, true);    // r = X - L_kk v0
  load_inverse();
  __syncthreads();
  block_product(t);  // Linv r
#pragma unroll
  for (int h = 0; h < VS_NH; ++h)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int i = 16 * w + lq + 4 * g, a = 16 * h + li;
      if (i < nb && a0 + a < Lg) E.V[(size_t)(k0 + i) * Lg + a0 + a] = v0[h][g] + t[h][g];
    }
}

// Column sums over the n rows of V for many training points: a workgroup owns 16 grid columns, its 16 row-lanes take every
// sixteenth row each (independent loads, a wave reads four rows of 128 contiguous bytes per instruction) and their
// partial sums are added in row-lane order.  (One thread per column walking all n rows -- Lg / 256 workgroups on the
// whole GPU -- took 0.39 + 0.36 ms at n = 1500, Lg = 2048.)
//   STD = false: mean_j = y_std * sum_i K_*[i][j] alpha_i + y_mean   (sklearn_gpr.py:381-385; before V is overwritten)
//   STD = true:  std_j = sqrt(max(amp - sum_i V[i][j]^2, 0) * y_std^2)   (sklearn_gpr.py:414-436)
#define PB_COLS 16
#define PB_LANES 16
template <bool STD>
__global__ void __launch_bounds__(PB_COLS * PB_LANES) k_pred_colsum_big(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  __shared__ double s_part[PB_LANES][PB_COLS + 1];
  const int n = sc->n, Lg = E.Lg;
  const int c = threadIdx.x & (PB_COLS - 1), r = threadIdx.x / PB_COLS;
  const int j = blockIdx.x * PB_COLS + c;
  const GPET_GLOBAL double* __restrict__ Vg = as_global(E.V);
  const GPET_GLOBAL double* __restrict__ al = as_global(E.alpha);
  double sum = 0.0;
  if (j < Lg) {
#pragma unroll 8
    for (int i = r; i < n; i += PB_LANES) {
      const double v = Vg[(size_t)i * Lg + j];
      sum += STD ? v * v : v * al[i];
    }
  }
  s_part[r][c] = sum;
  __syncthreads();
  if (r == 0 && j < Lg) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < PB_LANES; ++q) t += s_part[q][c];
    if (STD) {
      double var = sc->amp - t;
      if (var < 0.0) var = 0.0;
      E.std[j] = sqrt(var * (sc->y_std * sc->y_std));
    } else {
      E.mean[j] = sc->y_std * t + sc->y_mean;
    }
  }
}
