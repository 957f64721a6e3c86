// Part of gpet_kernels.hip (included there, inside namespace gpet, in this order): f1 / f3: curve KDE (fused, band-limited) and gradient KDE, pixel scoring, binning, per-bin argmax.
// ---------------------------------------------------------------------------------------
// f1  KDE of the best curves + pixel scoring / binning / argmax        gpet.py:455-662
//     KDEpy.FFTKDE restated: linear binning on the unit grid x=-1..N, y=-1..M, 9x9 Gaussian
//     (bw=1, support 4), crop, float32 min-max.  (PARITY UNPINNED: KDEpy is not available.)
//     Grid layout is x-major like KDEpy's: cell (gx, gy) at gx*(M+2)+gy.
// ---------------------------------------------------------------------------------------
// threads of the workgroup: NT where the kernel fixes them, NT = 0: blockDim.x, read where it is used as the kernels always did
template <int NT>
__device__ __forceinline__ auto wg_threads() {
  if constexpr (NT != 0) return NT;
  else return blockDim.x;
}
// the per-bin best score and its candidate back to "none" (before every pixel selection), by the threads of a workgroup
template <int NT>
__device__ __forceinline__ void pix_bins_reset(const EdgeDev& E, int tid) {
  for (int i = tid; i < E.n_bins; i += wg_threads<NT>()) {
    E.binbest[i] = 0ull;
    E.binarg[i] = 0x7FFFFFFFFFFFFFFFll;
  }
}
__global__ void __launch_bounds__(256) k_pix_reset(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  pix_bins_reset<0>(E, threadIdx.x);
}

__global__ void __launch_bounds__(256) k_kde_clear(EdgeDev* edges, int mode) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if (mode == 0 && ((sc->done && !sc->force) || sc->status != GPET_OK)) return;
  const size_t cells = (size_t)(E.N + 2) * (E.M + 2);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < cells; i += (size_t)gridDim.x * blockDim.x)
    E.bins[i] = 0.0;
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) {
      E.mm[0] = 0xFFFFFFFFu;
      E.mm[1] = 0u;
    }
    pix_bins_reset<0>(E, threadIdx.x);
    for (int i = threadIdx.x; i < E.N; i += blockDim.x) E.colsum[i] = 0.0;
  }
}

// gradient KDE (ctor, gpet.py:505-509): points = pixels with grad > 1e-3, weight = grad
__global__ void __launch_bounds__(256) k_kde_bin_gradient(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  const int x = blockIdx.x;
  if (x >= E.N) return;
  __shared__ double s_red[16];
  double part = 0.0;
  for (int y = threadIdx.x; y < E.M; y += blockDim.x) {
    const double g = (double)E.grad[(size_t)y * E.N + x];
    if (g > 1e-3) {
      E.bins[(size_t)(x + 1) * (E.M + 2) + (y + 1)] = g;
      part += g;
    }
  }
  part = block_sum(part, s_red);
  if (threadIdx.x == 0) E.colsum[x] = part;
}

__constant__ double c_gauss9[9] = {3.3546262790251185e-04, 1.1108996538242306e-02, 1.3533528323661270e-01,
                                   6.0653065971263342e-01, 1.0,
                                   6.0653065971263342e-01, 1.3533528323661270e-01, 1.1108996538242306e-02,
                                   3.3546262790251185e-04};  // exp(-t^2/2), t=-4..4

// total weight W = sum of the column sums in index order, once per edge (every workgroup of the vertical pass used to
// walk the N column sums on its thread 0 before its 256 outputs: 1.4 ms per 2048 x 2048 image)
__global__ void __launch_bounds__(64) k_kde_wsum(EdgeDev* edges, int mode) {
  const EdgeDev E = edges[blockIdx.x];
  const gpet_scalars* sc = E.sc;
  if (mode == 0 && ((sc->done && !sc->force) || sc->status != GPET_OK)) return;
  if (threadIdx.x != 0) return;
  double w = 0.0;
#pragma unroll 8
  for (int i = 0; i < E.N; ++i) w += E.colsum[i];
  E.kde_wsum[0] = w;
}

// vertical pass (along y, contiguous): tmp = (bins / W) (*) g
__global__ void __launch_bounds__(256) k_kde_conv_y(EdgeDev* edges, int mode) {
  const EdgeDev E = edges[blockIdx.z];
  const gpet_scalars* sc = E.sc;
  if (mode == 0 && ((sc->done && !sc->force) || sc->status != GPET_OK)) return;
  const int H = E.M + 2, Wd = E.N + 2;
  const int gy = blockIdx.x * blockDim.x + threadIdx.x;
  const int gx = blockIdx.y;
  if (gy >= H || gx >= Wd) return;
  const double s_w = E.kde_wsum[0];
  const double* col = E.bins + (size_t)gx * H;
  double acc = 0.0;
#pragma unroll
  for (int t = -4; t <= 4; ++t) {
    const int yy = gy + t;
    if (yy >= 0 && yy < H) acc += (col[yy] / s_w) * c_gauss9[t + 4];
  }
  E.tmpk[(size_t)gx * H + gy] = acc;
}

// horizontal pass + crop + transpose to (M, N) float32 + min/max.  A workgroup owns a tile of 32 image rows x 32 image
// columns: the 40 grid columns it needs are read along y (the contiguous direction of the x-major grid) into LDS, the
// outputs are written along x (the contiguous direction of the image) -- one thread per image row writing one float per
// column made every store its own cache line: 1.5 ms per 2048 x 2048 image.  Same nine products in the same order.
#define KCX_T 32
__global__ void __launch_bounds__(256) k_kde_conv_x(EdgeDev* edges, int mode) {
  const EdgeDev E = edges[blockIdx.z];
  const gpet_scalars* sc = E.sc;
  if (mode == 0 && ((sc->done && !sc->force) || sc->status != GPET_OK)) return;
  const int H = E.M + 2, Wd = E.N + 2;
  const int y0 = blockIdx.x * KCX_T, x0 = blockIdx.y * KCX_T;  // first image row / column of the tile
  __shared__ double s_t[KCX_T + 8][KCX_T + 1];  // [grid column x0 + c - 3][image row]
  const int tid = threadIdx.x;
  for (int e = tid; e < (KCX_T + 8) * KCX_T; e += 256) {
    const int c = e / KCX_T, r = e - c * KCX_T;
    const int xx = x0 + 1 + c - 4, gy = y0 + r + 1;  // grid coordinates (image pixel (x, y) sits at grid (x + 1, y + 1))
    s_t[c][r] = (xx >= 0 && xx < Wd && gy < H) ? E.tmpk[(size_t)xx * H + gy] : 0.0;
  }
  __syncthreads();
  float* dst = (mode == 0) ? E.kde : (float*)E.grad_kde;
  unsigned int kmin = 0xFFFFFFFFu, kmax = 0u;
  const int xl = tid & (KCX_T - 1);
  for (int yl = tid / KCX_T; yl < KCX_T; yl += 256 / KCX_T) {
    const int x = x0 + xl, y = y0 + yl;
    if (x < E.N && y < E.M) {
      double acc = 0.0;
#pragma unroll
      for (int t = -4; t <= 4; ++t) {
        const int xx = x + 1 + t;
        if (xx >= 0 && xx < Wd) acc += s_t[xl + t + 4][yl] * c_gauss9[t + 4];
      }
      acc *= 0.15915494309189535;  // 1 / (2 pi): Gaussian pdf normalisation in 2-D
      const float v = (float)acc;
      dst[(size_t)y * E.N + x] = v;
      const unsigned int key = f32_order_key(v);
      kmin = min(kmin, key);
      kmax = max(kmax, key);
    }
  }
  wave_minmax_commit(kmin, kmax, threadIdx.x, &E.mm[0], &E.mm[1]);
}

__global__ void __launch_bounds__(256) k_kde_normalise(EdgeDev* edges, int mode) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if (mode == 0 && ((sc->done && !sc->force) || sc->status != GPET_OK)) return;
  const float mn = f32_from_key(E.mm[0]);
  const float span = f32_from_key(E.mm[1]) - mn;
  float* a = (mode == 0) ? E.kde : (float*)E.grad_kde;
  const size_t px = (size_t)E.M * E.N;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < px; i += (size_t)gridDim.x * blockDim.x)
    a[i] = f32_min_span(a[i], mn, span);
}

// ---- fused curve KDE (per-iteration path) ----------------------------------------------
// k_kde_prep: total kept weight W (KDEpy normalises the weights by their sum), points removed
// for lying outside the image (gpet.py:498-500), and the per-iteration resets.
// kde_prep_body: everything after the kept curves' reciprocals and sample rows are staged (s_ic, s_row; `staged`: n_keep <=
// KDE_PREP_MAXB, else they are read from global memory) and a barrier -- k_kde_prep's own, and k_score_tail's with staged = true.
template <int NT>
__device__ __forceinline__ void kde_prep_body(const EdgeDev& E, gpet_scalars* sc, double* s_ic, const int* s_row, double* s_red,
                                              double& s_inv, int tid, int nk, bool staged) {
  // the sum of the reciprocals by one thread in index order (the order of the sequential loop this replaces, which paid one
  // global round trip and one division per curve on a single thread)
  if (tid == 0) {
    double inv_sum = 0.0;
    if (staged)
      for (int b = 0; b < nk; ++b) inv_sum += s_ic[b];
    else
      for (int b = 0; b < nk; ++b) inv_sum += 1.0 / E.best_costs[b];
    s_inv = inv_sum;
    E.mm[0] = 0xFFFFFFFFu;
    E.mm[1] = 0u;
  }
  __syncthreads();
  const double inv_sum = s_inv, ymax = (double)(E.M - 1);
  if (staged) {
    for (int b = tid; b < nk; b += (int)wg_threads<NT>()) s_ic[b] = s_ic[b] / inv_sum;  // weight of curve b
    __syncthreads();
  }
  double wsum = 0.0;
  int removed = 0;
  if (staged) {
    // wave w takes curves w, w + 16, ...; its lanes walk the columns: coalesced rows, no division per point
    const int lane = tid & 63, wv = tid >> 6, nw = (int)wg_threads<NT>() >> 6;
    for (int b = wv; b < nk; b += nw) {
      const size_t row = (size_t)s_row[b] * E.Yp;
      const double wb = s_ic[b];
#pragma unroll 4
      for (int k = lane; k < E.Lg; k += 64) {
        const double y = y_ld(E, row + k);
        if (y < 0.0 || y > ymax) ++removed; else wsum += wb;
      }
    }
  } else {
    const int total = nk * E.Lg;
#pragma unroll 4
    for (int e = tid; e < total; e += (int)wg_threads<NT>()) {
      const int b = e / E.Lg, k = e - b * E.Lg;
      const double y = y_ld(E, (size_t)E.best_idx[b] * E.Yp + k);
      const double wb = (1.0 / E.best_costs[b]) / inv_sum;
      if (y < 0.0 || y > ymax) ++removed; else wsum += wb;
    }
  }
  wsum = block_sum(wsum, s_red);
  const double rem = block_sum((double)removed, s_red);
  // the finished weights once per edge, for the tiles of k_kde_fused_r: k_kde_fused's ((1 / cost) / inv_sum) / W on the same three values
  // (every thread holds thread 0's W: block_sum adds the waves' sums in one order)
  if (staged && nk <= KDE_NB && E.kde_wt)
    for (int b = tid; b < nk; b += (int)wg_threads<NT>()) E.kde_wt[b] = s_ic[b] / wsum;
  if (tid == 0) {
    E.colsum[0] = wsum;     // W
    E.colsum[1] = inv_sum;  // sum of 1/cost over the kept curves
    sc->n_removed = (int)rem;
  }
}
__global__ void __launch_bounds__(1024) k_kde_prep(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  __shared__ double s_red[16];
  __shared__ double s_inv;
  __shared__ double s_ic[KDE_PREP_MAXB];   // 1 / cost of the kept curves, then their weights
  __shared__ int s_row[KDE_PREP_MAXB];     // their sample rows
  const int tid = threadIdx.x, nk = E.n_keep;
  const bool staged = nk <= KDE_PREP_MAXB;
  if (staged)  // the reciprocals in parallel
    for (int b = tid; b < nk; b += blockDim.x) {
      s_ic[b] = 1.0 / E.best_costs[b];
      s_row[b] = E.best_idx[b];
    }
  pix_bins_reset<0>(E, tid);
  __syncthreads();
  kde_prep_body<0>(E, sc, s_ic, s_row, s_red, s_inv, tid, nk, staged);
}

// Small batches (round 6): the three one-workgroup-per-edge steps between the tiled scorer and the fused KDE -- k_score_combine,
// k_topk_sort, k_kde_prep -- as ONE launch.  A small batch is a latency chain in which every launch costs ~5 us of dispatch beside
// its few microseconds of work; the arithmetic is the three kernels' own, in their order -- their bodies, called from here (partials
// added in tile order, bitonic sort with the index as second key, reciprocal sum by one thread in index order) --, so costs, best_idx
// and the KDE weights are the same bits.  Needs S <= 1024, n_keep <= KDE_PREP_MAXB and the tiled scorer's partial sums (the launcher checks).
__global__ void __launch_bounds__(1024) k_score_tail(EdgeDev* edges) {
  const EdgeDev E = edges[blockIdx.y];
  gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  __shared__ double s_k[1024];
  __shared__ int s_i[1024];
  __shared__ double s_red[16];
  __shared__ double s_inv;
  __shared__ double s_ic[KDE_PREP_MAXB];
  __shared__ int s_row[KDE_PREP_MAXB];
  const int tid = threadIdx.x, S = E.S, nk = E.n_keep;
  // -- k_score_combine: sample tid
  {
    double cost = INFINITY;  // (the padding of the sort: behind every finite cost, and behind +inf by index)
    if (tid < S) {
      cost = score_combine_one(E, tid);
      E.costs[tid] = cost;
    }
    s_k[tid] = cost;
    s_i[tid] = tid;
  }
  pix_bins_reset<1024>(E, tid);  // (k_kde_prep's per-iteration reset: independent of everything else here)
  __syncthreads();
  // -- k_topk_sort (the upper half of the workgroup only keeps the barriers company)
  bitonic_sort_1024<false>(s_k, s_i, tid);
  for (int b = tid; b < nk; b += 1024) {
    E.best_idx[b] = s_i[b];
    E.best_costs[b] = s_k[b];
    s_ic[b] = 1.0 / s_k[b];
    s_row[b] = s_i[b];
  }
  __syncthreads();
  // -- k_kde_prep (its staged form: n_keep <= KDE_PREP_MAXB)
  kde_prep_body<1024>(E, sc, s_ic, s_row, s_red, s_inv, tid, nk, true);
}

// (KDE_TX = 16 columns per tile, KDE_H = 128 rows per chunk, KDE_NB = 128 curves per pass, KDE_THREADS = 512: gpet_iter_plan.h)
// One workgroup per (16-column tile, edge).  The tile's curve points are staged in LDS once; the
// rows that can receive weight are the band [ymin-4, ymax+5] of those points, and only that band is
// processed, in chunks of KDE_H rows through ONE (KDE_TX+8) x (KDE_H+8) f64 LDS tile (51 904 B per
// workgroup with the staging, kde_fused_plan -> 3 workgroups per CU, at 76 registers as well).  This is the STAGED form: the
// path of more than KDE_NB kept curves, and the cross-check (option kde_variant = 0) of the register form k_kde_fused_r below,
// which the launcher takes wherever every kept curve fits one staging pass (kde_reg_plan).  The steps of a chunk:
//   linear binning  one (curve, column) point per thread, 64-bit fixed-point LDS atomics (order-independent
//                    sums; KDEpy itself convolves by FFT, so no summation order is "the" reference);
//   vertical 9 taps  in place, register sliding window (halo rows saved before the barrier);
//   horizontal 9 taps + crop + f32 cast + min/max, straight to HBM.
// Rows outside the band are written as zeros.  No global binning grid, no boundary tests: rows and
// columns outside the padded grid never receive weight.
// (Round 4: clearing, conversion and the vertical pass per wave on its own three columns -- four barriers per chunk instead
//  of eight, the vertical pass on 63 lanes of every wave -- was built and is bit-identical: 0.85-0.88 against 0.89-0.90 ms
//  per 1 024 edges on a batch alone, 15.2 against 14.6 ms per step inside the bench; binning per wave as well: 0.90-0.92.
//  The kernel waits for its binning atomics and the gathers of the staged points, not for its barriers.  Dropped.)
//
// REG, the register form (k_kde_fused_r; n_keep <= KDE_NB, so the staging loop runs once): what differs from the staged form is
// where values wait, never what is computed -- the same loads, products, fixed-point sums and 9-tap sums in the same order.
//   points    The staging loop and the binning loop walk the same e = tid, tid + KDE_THREADS, ...: a thread bins exactly the
//             points it loaded, at most KDE_NB (KDE_TX + 8) / KDE_THREADS = 6.  They stay in registers across the band reduction (and
//             are binned from there again by every further chunk) instead of making the round trip through 24 576 B of LDS.
//             LDS per workgroup: 27 328 B (kde_reg_plan) + 520 B static -> by LDS five workgroups per CU, by wave slots four.
//   weights   read from E.kde_wt, where kde_prep_body left them once per edge (three f64 divisions per curve and tile, behind
//             a dependent load of best_costs, in the staged form); the load goes out beside that of the sample rows.
//   clearing  the FIRST chunk's tile is cleared while the points' loads are in flight (the band, hence the chunk's height, is
//             not known yet: the whole tile), and the barrier of the band reduction is its barrier; every further chunk clears
//             the rows its vertical pass reads.
//   fixed point -> f64  by the vertical pass's own reads (the same conversion of the same bits): the pass over the tile and its
//             barrier are gone.  Rows the vertical pass does not write keep fixed-point bits; the horizontal pass reads none of them.
template <bool REG>
__device__ __forceinline__ void kde_fused_body(EdgeDev* edges, int raw_band) {
  int edge, tile;  // the column tiles of an edge on one XCD: neighbours share 8 of their 24 staged columns of every curve
  xcd_edge_part((int)gridDim.x, edge, tile);
  const EdgeDev E = edges[edge];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  extern __shared__ double s_a[];
  __shared__ int s_band[2];
  __shared__ int s_brow[KDE_NB];
  const int M = E.M, N = E.N;
  const int x0 = tile * KDE_TX;
  if (x0 >= N) return;
  const int NC = KDE_TX + 8;
  const int ld = (KDE_H + 8) | 1;
  double* s_y = s_a + NC * ld;                              // [KDE_NB][NC] staged points (-1: none); REG: none
  double* s_wt = REG ? s_a + NC * ld : s_y + KDE_NB * NC;   // [KDE_NB] staged weights
  constexpr int PT = KDE_NB * (KDE_TX + 8) / KDE_THREADS;   // REG: points per thread
  const int tid = threadIdx.x;
  const bool band = (x0 + KDE_TX + 4 > E.x_st) && (x0 - 4 <= E.x_en);
  // (global_* instead of flat_* accesses: a FLAT instruction counts in the LDS counter as well, so every wait for an LDS
  //  operand -- and every barrier -- also waited for the chunk's outstanding stores and the staged points' loads)
  GPET_GLOBAL float* __restrict__ out = as_global(E.kde);
  const GPET_GLOBAL double* __restrict__ Yd = as_global(E.Y);
  const GPET_GLOBAL float* __restrict__ Yf = as_global(reinterpret_cast<const float*>(E.Y));
  const GPET_GLOBAL int* __restrict__ bidx = as_global(E.best_idx);
  const GPET_GLOBAL double* __restrict__ bcost = as_global(E.best_costs);
  const bool yf32 = E.y_f32 != 0;
  unsigned int kmin = 0xFFFFFFFFu, kmax = 0u;
  int y_lo = M, y_hi = -1;  // band of image rows with possibly non-zero density
  if (band) {
    const double W = E.colsum[0], inv_sum = E.colsum[1], ymax = (double)(M - 1);
    double g[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) g[t] = c_gauss9[t];
    const bool single = (E.n_keep <= KDE_NB);  // all kept curves fit one staging pass (the usual case)
    // fixed-point scale of the binning: a bin holds at most one column's weight, <= 1 / W, so
    // 2^(62 + floor(log2 W)) keeps every sum below 2^62 with an lsb of ~2^-70 (contributions are ~2^-17)
    const int kexp = 62 + ilogb(W > 0.0 ? W : 1.0);
    // (REG: the same in every lane, and told so to the compiler -- scalar registers, which the 64 vector registers of four
    //  workgroups per CU have no room to mirror)
    auto uni = [](double v) {
      if constexpr (REG) return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
      else return v;
    };
    const double fscale = uni(ldexp(1.0, kexp)), finv = uni(ldexp(1.0, -kexp));
    // stage curves [b0, b0+nb) of this tile's columns; returns the rows they touch through (lo, hi)
    auto stage = [&](int b0, int nb, int& lo, int& hi) {
      // (the sample rows of the curves of this pass through LDS first: the loads of the points then depend on nothing
      //  and are all in flight together, instead of one index load + one dependent sample load per point)
      for (int e = tid; e < nb; e += KDE_THREADS) s_brow[e] = bidx[b0 + e];
      __syncthreads();
#pragma unroll 6
      for (int e = tid; e < nb * NC; e += KDE_THREADS) {
        const int bb = e / NC, c = e - bb * NC;
        const int xc = x0 + c - 4;
        double y = -1.0;
        if (xc >= E.x_st && xc <= E.x_en) {
          const size_t at = (size_t)s_brow[bb] * E.Yp + (xc - E.x_st);
          y = yf32 ? (double)Yf[at] : Yd[at];
        }
        if (y < 0.0 || y > ymax) y = -1.0;  // gpet.py:498-500
        s_y[e] = y;
        if (y >= 0.0) {
          const int iy = (int)floor(y);
          lo = min(lo, iy);
          hi = max(hi, iy + 1);
        }
      }
      for (int e = tid; e < nb; e += KDE_THREADS) s_wt[e] = ((1.0 / bcost[b0 + e]) / inv_sum) / W;
    };
    // phase A: band of rows that receive weight
    double yv[PT];  // REG: this thread's points e = tid + k KDE_THREADS (-1: none), from here to the last chunk's binning
    if constexpr (REG) {
      if (tid < E.n_keep) {  // (n_keep <= KDE_NB < KDE_THREADS; two independent loads, one round trip)
        s_brow[tid] = bidx[tid];
        s_wt[tid] = as_global(E.kde_wt)[tid];
      }
    }
    if (tid == 0) {
      s_band[0] = 0x7FFFFFFF;
      s_band[1] = -1;
    }
    __syncthreads();
    {
      int mylo = 0x7FFFFFFF, myhi = -1;
      if constexpr (REG) {
        const int npt = E.n_keep * NC;
        auto load = [&](auto src) {  // (stage's loads, all in flight together)
#pragma unroll
          for (int k = 0; k < PT; ++k) {
            const int e = tid + k * KDE_THREADS;
            const int bb = e / NC, c = e - bb * NC;
            const int xc = x0 + c - 4;
            yv[k] = -1.0;
            if (e < npt && xc >= E.x_st && xc <= E.x_en) yv[k] = (double)src[(size_t)s_brow[bb] * E.Yp + (xc - E.x_st)];
          }
        };
        if (yf32) load(Yf);
        else load(Yd);
        for (int i = tid; i < NC * ld; i += KDE_THREADS) s_a[i] = 0.0;  // (the first chunk's tile, under the loads)
#pragma unroll
        for (int k = 0; k < PT; ++k) {
          if (yv[k] < 0.0 || yv[k] > ymax) yv[k] = -1.0;  // gpet.py:498-500
          if (yv[k] >= 0.0) {
            const int iy = (int)floor(yv[k]);
            mylo = min(mylo, iy);
            myhi = max(myhi, iy + 1);
          }
        }
      } else {
        for (int b0 = 0; b0 < E.n_keep; b0 += KDE_NB) {
          const int nb = (E.n_keep - b0) < KDE_NB ? (E.n_keep - b0) : KDE_NB;
          if (b0 > 0) __syncthreads();
          stage(b0, nb, mylo, myhi);
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        mylo = min(mylo, __shfl_xor(mylo, o, WAVE));
        myhi = max(myhi, __shfl_xor(myhi, o, WAVE));
      }
      if ((tid & 63) == 0) {
        atomicMin(&s_band[0], mylo);
        atomicMax(&s_band[1], myhi);
      }
    }
    __syncthreads();
    if (s_band[1] >= 0) {
      y_lo = max(0, s_band[0] - 4);
      y_hi = min(M - 1, s_band[1] + 4);
    }
    // phase B: the band, KDE_H image rows at a time
    for (int r0 = y_lo; r0 <= y_hi; r0 += KDE_H) {
      const int nrow = (y_hi + 1 - r0) < KDE_H ? (y_hi + 1 - r0) : KDE_H;
      // LDS row l <-> padded-grid row gy = r0 - 3 + l  (image row y sits at l = y - r0 + 4)
      // REG: the thread index of this chunk, a copy the optimiser cannot see through.  It otherwise computes every point's row, LDS
      // addresses and fixed-point addends and the passes' addresses ahead of the chunk loop and keeps them beside the points: over
      // 40 registers, spilled at four workgroups per CU (the points' values get the same treatment below)
      int tc = tid;
      if constexpr (REG) asm volatile("" : "+v"(tc));
      unsigned long long* s_bits = reinterpret_cast<unsigned long long*>(s_a);
      const int lmax = nrow + 8;
      // linear binning of one (curve, column) point: 64-bit fixed-point LDS atomics, so the sums do not depend on the
      // order the points arrive in (deterministic), at the resolution of f64 arithmetic
      auto bin = [&](int e, double y) {
        if (y < 0.0) return;
        const int bb = e / NC, bc = e - bb * NC;
        const double gy = y + 1.0;
        const int iy = (int)floor(gy);
        const int l = iy - (r0 - 3);
        if (l + 1 < 0 || l >= lmax) return;
        const double w = s_wt[bb] * fscale;
        const double fy = gy - (double)iy;
        unsigned long long* col = s_bits + bc * ld;
        if (l >= 0) atomicAdd(&col[l], (unsigned long long)__double2ll_rn((1.0 - fy) * w));
        if (l + 1 < lmax) atomicAdd(&col[l + 1], (unsigned long long)__double2ll_rn(fy * w));
      };
      if constexpr (REG) {
        if (r0 != y_lo) {
          // rows 0 .. lclr - 1: all that the vertical pass below reads (its last segment reaches lclr - 1).  A quarter of the
          // workgroup per column, a thread per row: no division by the run-time height
          const int lclr = min(((nrow + 7) & ~7) + 8, ld);
          const int l = tc & 127;
          for (int c = tc >> 7; c < NC; c += KDE_THREADS / 128) {
            if (l < lclr) s_a[c * ld + l] = 0.0;
            if (l + 128 < lclr) s_a[c * ld + l + 128] = 0.0;
          }
          __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < PT; ++k) {
          double y = yv[k];
          asm volatile("" : "+v"(y));
          bin(tc + k * KDE_THREADS, y);
        }
        __syncthreads();
      } else {
        for (int i = tid; i < NC * ld; i += KDE_THREADS) s_a[i] = 0.0;
        __syncthreads();
        for (int b0 = 0; b0 < E.n_keep; b0 += KDE_NB) {
          const int nb = (E.n_keep - b0) < KDE_NB ? (E.n_keep - b0) : KDE_NB;
          if (!single) {
            int dl = 0, dh = 0;
            __syncthreads();
            stage(b0, nb, dl, dh);
            __syncthreads();
          }
          for (int e = tid; e < nb * NC; e += KDE_THREADS) bin(e, s_y[e]);  // (one point per thread)
        }
        __syncthreads();
        for (int i = tid; i < NC * ld; i += KDE_THREADS) s_a[i] = (double)(long long)s_bits[i] * finv;
        __syncthreads();
      }
      // what the vertical pass reads: f64 (the staged form converted the tile), REG: fixed point, converted here
      auto rd = [&](const double* p) {
        if constexpr (REG) return (double)(long long)*reinterpret_cast<const unsigned long long*>(p) * finv;
        else return *p;
      };
      {  // vertical pass in place: filtered value of chunk row q is written to LDS row q + 4.  Thread = (column, segment of
         // EIGHT rows): the nine-row window then rotates through registers with compile-time roles (fully unrolled: one
         // LDS read, nine multiply-adds and one write per row; with run-time segment lengths the window was shifted by
         // sixteen register moves per row and all eight waves ran ~340 instructions where six now run ~110; sixteen-row segments need 88 registers: two workgroups per CU instead of three).  A last
         // segment that reaches beyond the chunk filters rows of zeros into rows nobody reads.
        constexpr int VR = 8;
        const int seg = tc / NC, c = tc - seg * NC;
        const int q0 = seg * VR;
        double* col = s_a + c * ld;
        double head[4], tail[4];
        const bool active = q0 < nrow;  // (seg < KDE_H / VR = 16 then: 384 threads)
        if (active) {
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            head[t] = rd(&col[q0 + t]);
            tail[t] = rd(&col[q0 + VR + 4 + t]);
          }
        }
        __syncthreads();
        if (active) {
          double wv[VR + 8];  // rows q0 .. q0 + VR + 7 as they were before anybody wrote
#pragma unroll
          for (int t = 0; t < 4; ++t) wv[t] = head[t];
#pragma unroll
          for (int t = 4; t < VR + 4; ++t) wv[t] = rd(&col[q0 + t]);  // (rows q0 + 4 .. q0 + VR + 3: this segment's own output rows)
#pragma unroll
          for (int t = 0; t < 4; ++t) wv[VR + 4 + t] = tail[t];
#pragma unroll
          for (int qq = 0; qq < VR; ++qq) {
            const double acc = wv[qq] * g[0] + wv[qq + 1] * g[1] + wv[qq + 2] * g[2] + wv[qq + 3] * g[3] + wv[qq + 4] * g[4] +
                               wv[qq + 5] * g[5] + wv[qq + 6] * g[6] + wv[qq + 7] * g[7] + wv[qq + 8] * g[8];
            col[q0 + qq + 4] = acc;
          }
        }
      }
      __syncthreads();
      if ((N & 3) == 0) {
        // horizontal pass, four adjacent lanes per image row, four output columns each: twelve LDS reads for four outputs (nine
        // per output before), one 16-byte store per lane -- 64 contiguous bytes per row as before
        const int yl = tc >> 2, xq = tc & 3;
        const int x = x0 + 4 * xq;
        if (yl < nrow && x < N) {
          double in[12];
#pragma unroll
          for (int t = 0; t < 12; ++t) in[t] = s_a[(4 * xq + t) * ld + yl + 4];
          typedef float kde_f4 __attribute__((ext_vector_type(4)));
          float ov[4];
#pragma unroll
          for (int jx = 0; jx < 4; ++jx) {
            double acc = 0.0;
#pragma unroll
            for (int t = 0; t < 9; ++t) acc += in[jx + t] * g[t];
            acc *= 0.15915494309189535;  // 1 / (2 pi): 2-D Gaussian pdf normalisation
            ov[jx] = (float)acc;
            const unsigned int key = f32_order_key(ov[jx]);
            kmin = min(kmin, key);
            kmax = max(kmax, key);
          }
          *reinterpret_cast<GPET_GLOBAL kde_f4*>(out + (size_t)(r0 + yl) * N + x) = (kde_f4){ov[0], ov[1], ov[2], ov[3]};
        }
      } else {
        for (int idx = tc; idx < KDE_TX * nrow; idx += KDE_THREADS) {
          const int xl = idx % KDE_TX, yl = idx / KDE_TX;
          const int x = x0 + xl;
          if (x >= N) continue;
          double acc = 0.0;
#pragma unroll
          for (int t = 0; t < 9; ++t) acc += s_a[(xl + t) * ld + yl + 4] * g[t];
          acc *= 0.15915494309189535;  // 1 / (2 pi): 2-D Gaussian pdf normalisation
          const float v = (float)acc;
          out[(size_t)(r0 + yl) * N + x] = v;
          const unsigned int key = f32_order_key(v);
          kmin = min(kmin, key);
          kmax = max(kmax, key);
        }
      }
      __syncthreads();
    }
  }
  // rows outside the band (all rows for tiles away from the edge): zeros.  raw_band (the loop form): they are
  // not written -- the pixel kernels take the band from kde_band and treat everything outside it as zero.
  bool wrote_zero = false;
  if (raw_band) {
    if (tid == 0) {
      E.kde_band[2 * tile] = y_lo;
      E.kde_band[2 * tile + 1] = y_hi;
    }
    wrote_zero = (tid == 0) && (y_hi - y_lo + 1 < M);
  } else {
    for (int idx = tid; idx < KDE_TX * M; idx += KDE_THREADS) {
      const int xl = idx % KDE_TX, y = idx / KDE_TX;
      if (y >= y_lo && y <= y_hi) continue;
      if (x0 + xl < N) {
        out[(size_t)y * N + x0 + xl] = 0.f;
        wrote_zero = true;
      }
    }
  }
  if (wrote_zero) {
    const unsigned int kz = f32_order_key(0.f);
    kmin = min(kmin, kz);
    kmax = max(kmax, kz);
  }
  wave_minmax_commit(kmin, kmax, tid, &E.mm[0], &E.mm[1]);
}
__global__ void __launch_bounds__(KDE_THREADS) k_kde_fused(EdgeDev* edges, int raw_band) { kde_fused_body<false>(edges, raw_band); }
// (four workgroups of eight waves per CU need at most 64 registers: tests/test_kde_reg_host.py reads the count from the code object)
__global__ void __launch_bounds__(KDE_THREADS, 8) k_kde_fused_r(EdgeDev* edges, int raw_band) { kde_fused_body<true>(edges, raw_band); }

// normalised curve KDE at a pixel.  raw_band: E.kde holds the raw density of the band rows only; the min-max
// normalisation of k_kde_normalise ((v - min) / span in float32, gpet_utils.py:81-91) is applied here instead.
__device__ __forceinline__ double kde_at(const EdgeDev& E, int x, int y, int raw_band, float mn, float span) {
  if (!raw_band) return (double)E.kde[(size_t)y * E.N + x];
  const int t = x / KDE_TX;
  const float raw = (y >= E.kde_band[2 * t] && y <= E.kde_band[2 * t + 1]) ? E.kde[(size_t)y * E.N + x] : 0.f;
  return (double)((raw - mn) / span);
}

// pixel_scores = 1/3 * (i*g + i + g) with numpy's rounding order (gpet.py:582)
__device__ __forceinline__ double pixel_score(double iv, double gv) {
#pragma clang fp contract(off)
  double t = iv * gv;
  t = t + iv;
  t = t + gv;
  return (1.0 / 3.0) * t;
}

__device__ __forceinline__ int bin_of(const EdgeDev& E, int x) {
  return (int)rint((double)(x - E.x_st) / (double)E.delta_x) - E.bin_lo;  // np.round = half-to-even
}

// best new candidate of every admissible column (first in row-major order among equals).
// 32 columns x 8 row-lanes per workgroup: each thread scans every 8th row of its column (independent loads; a wave reads
// two rows of 128 contiguous bytes per instruction: whole cache lines), then the 8 lanes of a column reduce in LDS.
// (PIX_CX = 32: gpet_iter_plan.h)
#define PIX_RY 8
__global__ void __launch_bounds__(256) k_pix_columns(EdgeDev* edges, int raw_band) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const GPET_GLOBAL float* __restrict__ g_kde = as_global(E.kde);
  const GPET_GLOBAL float* __restrict__ g_gk = as_global(E.grad_kde);
  __shared__ double s_best[PIX_RY][PIX_CX + 1];
  __shared__ int s_by[PIX_RY][PIX_CX + 1];
  const int cx = threadIdx.x & (PIX_CX - 1), ry = threadIdx.x / PIX_CX;
  const int x = blockIdx.x * PIX_CX + cx;
  double best = -1.0;
  int by = -1;
  const bool admissible = (x < E.N) && (E.fix_endpoints ? (x > E.x_st && x < E.x_en) : true);  // gpet.py:655-657
  const float mn = f32_from_key(E.mm[0]);
  const float span = f32_from_key(E.mm[1]) - mn;
  // raw_band: rows outside the band of the column's KDE tile hold density 0 -> normalised 0 <= 1e-3 unless the minimum
  // of the whole image is negative (it is not: densities are sums of non-negative terms), so only the band is scanned
  int y_first = 0, y_last = E.M - 1;
  if (raw_band && x < E.N) {
    y_first = E.kde_band[2 * (x / KDE_TX)];
    y_last = E.kde_band[2 * (x / KDE_TX) + 1];
  }
  if (admissible) {
    // eight rows per pass, their densities requested together (a row at a time the loop paid one memory round trip
    // per row: 62 dependent trips for a 500-row band); the gradient KDE only where the density passes the threshold
    for (int y0 = y_first + ry; y0 <= y_last; y0 += 8 * PIX_RY) {
      float kv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int y = y0 + u * PIX_RY;
        kv[u] = (y <= y_last) ? g_kde[(size_t)y * E.N + x] : -1.0f;
      }
      double ivs[8];
      float gk[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int y = y0 + u * PIX_RY;
        ivs[u] = (y <= y_last) ? (raw_band ? (double)((kv[u] - mn) / span) : (double)kv[u]) : 0.0;
        gk[u] = (ivs[u] > 1e-3) ? g_gk[(size_t)y * E.N + x] : 0.f;  // gpet.py:651
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (ivs[u] > 1e-3) {
          const double sv = pixel_score(ivs[u], (double)gk[u]);
          if (sv > best) {  // rows visited in increasing order: first maximum kept
            best = sv;
            by = y0 + u * PIX_RY;
          }
        }
      }
    }
  }
  s_best[ry][cx] = best;
  s_by[ry][cx] = by;
  __syncthreads();
  if (ry == 0 && x < E.N) {
    for (int q = 1; q < PIX_RY; ++q) {
      const double v = s_best[q][cx];
      const int yy = s_by[q][cx];
      if (yy >= 0 && (v > best || (v == best && yy < by))) {
        best = v;
        by = yy;
      }
    }
    E.colbest[x] = best;
    E.colbest_y[x] = by;
    if (by >= 0) atomicMax(&E.binbest[bin_of(E, x)], (unsigned long long)__double_as_longlong(best));
  }
}

// previously accepted observations are re-scored and compete first (gpet.py:568-579)
__global__ void __launch_bounds__(256) k_pix_old(EdgeDev* edges, int raw_band) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sc->n_obs) return;
  const long long x = E.obs_xy[2 * i], y = E.obs_xy[2 * i + 1];
  const float mn = f32_from_key(E.mm[0]);
  const double iv = kde_at(E, (int)x, (int)y, raw_band, mn, f32_from_key(E.mm[1]) - mn);
  if (iv > 1e-3) {
    const double sv = pixel_score(iv, (double)E.grad_kde[(size_t)y * E.N + x]);
    atomicMax(&E.binbest[bin_of(E, (int)x)], (unsigned long long)__double_as_longlong(sv));
  }
}

// among the candidates that reach their bin's best score, the first in the reference's candidate
// order wins (np.argmax): old observations in their order, then new pixels in row-major order.
__global__ void __launch_bounds__(256) k_pix_argbest(EdgeDev* edges, int raw_band) {
  const EdgeDev E = edges[blockIdx.y];
  const gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int n_obs = sc->n_obs;
  if (t < n_obs) {
    const long long x = E.obs_xy[2 * t], y = E.obs_xy[2 * t + 1];
    const float mn = f32_from_key(E.mm[0]);
    const double iv = kde_at(E, (int)x, (int)y, raw_band, mn, f32_from_key(E.mm[1]) - mn);
    if (iv > 1e-3) {
      const double sv = pixel_score(iv, (double)E.grad_kde[(size_t)y * E.N + x]);
      const int b = bin_of(E, (int)x);
      if ((unsigned long long)__double_as_longlong(sv) == E.binbest[b])
        atomicMin(&E.binarg[b], (long long)t - (long long)(1ll << 40));  // old: before every new pixel
    }
  }
  if (t < E.N) {
    const int by = E.colbest_y[t];
    if (by >= 0) {
      const int b = bin_of(E, t);
      if ((unsigned long long)__double_as_longlong(E.colbest[t]) == E.binbest[b])
        atomicMin(&E.binarg[b], (long long)by * E.N + t);
    }
  }
}

// adaptive threshold (gpet.py:589-609), one pixel per bin (gpet.py:613-616), loop bookkeeping
// (gpet.py:861-865).  One wave per edge.
__global__ void __launch_bounds__(64) k_pix_select(EdgeDev* edges) {
#pragma clang fp contract(off)
  const EdgeDev E = edges[blockIdx.y];
  gpet_scalars* sc = E.sc;
  if ((sc->done && !sc->force) || sc->status != GPET_OK) return;
  const int lane = threadIdx.x;
  const int n_pre = sc->n_obs;
  double thresh = sc->score_thresh;
  int n_pix = n_pre;
  int it = 0;
  bool stuck = false;
  int n_all = 0;  // bins that hold a candidate at all (counted by the first pass): once a pass has found every one of them, no
                  // smaller threshold finds more
  while ((n_pix - n_pre < E.pixel_thresh) && (n_pix < E.algo_thresh)) {
    if (it > 0) {
      // the reference would spin forever here (SURVEY 5, latent hang 1).  Not `thresh == 0`: a threshold decayed by 0.95
      // never gets there -- in f64 it stops at 9 units of the smallest subnormal, where x * 0.95 rounds back to x
      const double next = thresh * 0.95;
      if (n_pix >= n_all || !(next < thresh)) {  // (n_pix: the bins found by the last pass; !(next < thresh): the fixed point, or NaN)
        stuck = true;
        break;
      }
      thresh = next;
    }
    int cnt = 0, held = 0;
    for (int b = lane; b < E.n_bins; b += WAVE) {
      const unsigned long long bits = E.binbest[b];
      const bool holds = E.binarg[b] != 0x7FFFFFFFFFFFFFFFll;
      held += holds;
      cnt += holds && (__longlong_as_double((long long)bits) >= thresh);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, WAVE);
    if (it == 0) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) held += __shfl_xor(held, o, WAVE);
      n_all = held;
    }
    n_pix = cnt;
    ++it;
  }
  if (stuck) {
    if (lane == 0) sc->status = GPET_ERR_ITER_CAP;
    return;
  }
  // compact the winning pixels in ascending bin order (np.unique order)
  int base = 0;
  for (int b0 = 0; b0 < E.n_bins; b0 += WAVE) {
    const int b = b0 + lane;
    bool take = false;
    long long key = 0;
    if (b < E.n_bins) {
      key = E.binarg[b];
      take = (key != 0x7FFFFFFFFFFFFFFFll) && (__longlong_as_double((long long)E.binbest[b]) >= thresh);
    }
    const unsigned long long bal = __ballot(take);
    if (take) {
      const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
      long long x, y;
      if (key < 0) {  // an old observation
        const long long oi = key + (1ll << 40);
        x = E.obs_xy[2 * oi];
        y = E.obs_xy[2 * oi + 1];
      } else {
        y = key / E.N;
        x = key - y * E.N;
      }
      E.obs_new[2 * pos] = x;
      E.obs_new[2 * pos + 1] = y;
    }
    base += __popcll(bal);
  }
  // (same wave: obs_new fully written before it is copied back)
  for (int i = lane; i < 2 * n_pix; i += WAVE) E.obs_xy[i] = E.obs_new[i];
  if (lane == 0) {
    sc->score_thresh = thresh;
    sc->n_obs = n_pix;
    sc->iter = sc->iter + 1;
    sc->done = (n_pix >= E.algo_thresh) ? 1 : 0;
  }
}
