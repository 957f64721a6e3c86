// What gpet_batch_create2 (gpet_api_batch.hip) decides, as plain data: edge parameters in, the resolved EdgeDev fields, the batch's
// dimensions and the layout of its arena out.  No HIP, no gpet_batch and no device memory, so the host compiler alone builds it
// (tests/test_batch_plan.py).  layout_batch is the ONE place where the size of an arena buffer is written.
#pragma once
#include <math.h>
#include <stddef.h>
#include <string.h>

#include <vector>

#include "gpet_dev.h"

namespace gpet {

struct BatchDims {
  int M, N, Lg, S, n_keep, z_cols, r_cap, n_cap, n_bins, obs_cap, z_ring, a_rows_cap, r0_max;
  int jlog;   // the edges have a rotation log (small batches: k_jacobi_seat<.., LOGW> + k_jacobi_wpass)
  int y_f32;  // samples stored as f32 (gpet_batch_set_sample_dtype): which instantiation of the GEMM / scorer to launch
  int rng4;   // every edge has the same even grid length >= 64, the same S and z_cols: the register-resident generator k_mt_normals4 applies
  int lg_even;  // every edge of the batch has an even grid length (no Simpson tail: the fused sample + score kernel applies)
  int y_arith;  // sample GEMM on the f32 matrix cores (gpet_batch_set_sample_arith; implies y_f32): which family launch_sample takes
};

struct Carver {  // lays buffers out in one arena (256-byte aligned); with base == nullptr it only measures
  size_t off = 0;
  char* base = nullptr;
  template <typename T>
  T* take(size_t count) {
    off = (off + 255) & ~(size_t)255;
    T* p = base ? (T*)(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
  template <typename T>
  void skip(size_t count) {  // reserved space nothing points to
    (void)take<T>(count);
  }
};

// dynamic LDS a kernel may ask for (of the 160 KB of a CU): the limit of every capacity rule here and in gpet_iter_plan.h
#define LDS_DYN_MAX (150 * 1024)
// dynamic LDS available to k_struct_H (the structured path needs at least U + one row of L + beta in it)
#define STRUCT_H_LDS_MAX LDS_DYN_MAX
// curves the fused curve KDE stages per pass (k_kde_fused), and the most its register form takes (k_kde_fused_r): the capacity of kde_wt
constexpr int KDE_NB = 128;
// the eigen-factor stage (rules: gpet_factor_plan.h), as far as the arena is sized by it:
constexpr int FACTOR_LDS_CAP = 96;     // largest factor capacity of the LDS-resident Jacobi path; above it the any-rank factor
constexpr int PCH_ONE_WG_MAX = 1024;   // widest edge of that path whose pivoted Cholesky is always one workgroup's (k_pchol)
constexpr int PCX_COLS = 32;           // columns per workgroup of the multi-workgroup pivoted Cholesky
// doubles of pcx_cand per workgroup: two halves (current / next step) of one (value, index) pair per wave, four waves (k_pcx_step; the
// blocked form k_pcb_block keeps one pair per workgroup and half)
constexpr int PCX_CAND_PER_WG = 2 * 4 * 2;

inline int nu_to_code(double nu) {
  if (nu == 0.5) return 0;
  if (nu == 1.5) return 1;
  if (nu == 2.5) return 2;
  // any other smoothness: Bessel form by quadrature (gpet.py:134).  Both bounds keep its node count bounded: from above
  // the step shrinks as 0.45 / sqrt(nu); from below the node range reaches down to -40 / nu where q = nu r^2 / 2 is tiny
  // (and where q underflows to 0, below nu ~ 1e-291, the count is unbounded).  The tests pin both ends.
  if (nu >= 0.01 && nu <= 1000.0) return 3;
  return -1;
}

// ---- edges ----------------------------------------------------------------------------------------------------------------

inline bool batch_shape_ok(int B, int M, int N) { return B > 0 && M >= 2 && N >= 2; }

// A capacity above FACTOR_LDS_CAP on ANY edge selects the whole-GPU Jacobi on the full covariance; that path is chosen per batch.
inline bool any_big_edge(const gpet_params* params, int B) {
  for (int e = 0; e < B; ++e) {
    const int Lg = params[e].x_en - params[e].x_st + 1;
    const int cap = params[e].factor_cap > 0 ? params[e].factor_cap : FACTOR_LDS_CAP;
    if ((cap < Lg ? cap : Lg) > FACTOR_LDS_CAP) return true;
  }
  return false;
}

enum class EdgeCheck { ok, inconsistent, matern_nu };

inline int edge_check_status(EdgeCheck r) {
  return r == EdgeCheck::ok ? GPET_OK : r == EdgeCheck::inconsistent ? GPET_ERR_BAD_ARG : GPET_ERR_UNSUPPORTED;
}

// Checks one edge's parameters and fills every geometry / capacity field of E (its pointers stay null: layout_batch); B is the
// batch's size, any_big is any_big_edge of the whole batch, jlog_max_b the option of that name (32).
inline EdgeCheck resolve_edge(EdgeDev& E, const gpet_params& p, int B, int M, int N, bool any_big, int jlog_max_b) {
  memset(&E, 0, sizeof E);
  const int Lg = p.x_en - p.x_st + 1;
  if (p.x_st < 0 || p.x_en >= N || Lg < 4 || p.n_init < 1 || p.n_samples < 1 || p.n_keep < 0 ||
      p.n_keep > p.n_samples || p.delta_x < 1 || p.length_scale <= 0)
    return EdgeCheck::inconsistent;
  if (p.kernel_type == GPET_KERNEL_MATERN && nu_to_code(p.nu) < 0) return EdgeCheck::matern_nu;
  E.M = M;
  E.N = N;
  E.x_st = p.x_st;
  E.x_en = p.x_en;
  E.Lg = Lg;
  E.S = p.n_samples;
  E.n_keep = p.n_keep;
  E.n_init = p.n_init;
  // bins of np.round((x - x_st)/delta_x) over every image column (gpet.py:605-606)
  E.bin_lo = (int)rint((double)(0 - p.x_st) / (double)p.delta_x);
  E.n_bins = (int)rint((double)(N - 1 - p.x_st) / (double)p.delta_x) - E.bin_lo + 2;
  E.obs_cap = p.obs_cap > E.n_bins ? p.obs_cap : E.n_bins;
  E.n_cap = E.n_init + E.obs_cap;
  E.r_cap = p.factor_cap > 0 ? p.factor_cap : FACTOR_LDS_CAP;  // <= 96: the LDS-resident Jacobi path
  if (E.r_cap > Lg) E.r_cap = Lg;
  if (any_big) E.r_cap = Lg;  // (then every edge of the batch keeps all Lg directions)
  E.z_cols = p.z_cols > 0 ? p.z_cols : E.r_cap;
  if (E.z_cols > Lg) E.z_cols = Lg;
  if (any_big) E.z_cols = Lg;
  if (E.z_cols < E.r_cap) E.r_cap = E.z_cols;
  E.a_rows_cap = (E.z_cols >= Lg) ? Lg : E.r_cap;
  // slots of the ring of pre-generated normals (gpet_loop_plan.h): 16 up to 64 edges, which are latency-bound in the generator
  // and draw eight iterations ahead on the side stream; 9 above 64 edges, where one launch generates the (up to eight) iterations
  // of a group -- at 1 024 edges of the bench shape 7.1 GB instead of 12.6 GB, of an arena of 21.1 GB; 2 when a row holds the
  // whole grid (z_cols == Lg > 128: full-rank covariances, config 3), where one slot is a stream of S * Lg normals
  E.z_ring = (E.z_cols >= Lg && Lg > 128) ? 2 : (B <= 64 ? 16 : 9);
  // small batches are bound by the chain of Jacobi rounds: their rotations are logged and the eigenvectors formed by a
  // second kernel (k_jacobi_wpass); 40 sweeps x (m - 1) rounds x m / 2 pairs x 16 bytes = 2.9 MB per edge at rank 96
  // (jlog_max_b = 32: the rotation-log form pays while the chain of rounds is the time)
  E.jlog_cap = (B <= jlog_max_b && E.r_cap <= FACTOR_LDS_CAP) ? 40 : 0;
  E.kernel_type = p.kernel_type;
  E.nu_code = p.kernel_type == GPET_KERNEL_MATERN ? nu_to_code(p.nu) : 2;
  E.nu_gen = p.nu;
  // (1 / Gamma(nu); above nu = 170, where matern_gen's sum of ~Gamma(nu) / h would overflow, -lgamma(nu), which it
  //  folds into its exponent)
  E.inv_gamma_nu = (E.nu_code != 3) ? 1.0 : (p.nu <= 170.0 ? 1.0 / tgamma(p.nu) : -lgamma(p.nu));
  E.tab_ok = 1;
  E.fix_endpoints = p.fix_endpoints;
  E.delta_x = p.delta_x;
  E.pixel_thresh = p.pixel_thresh;
  E.algo_thresh = Lg / p.delta_x - (p.pixel_thresh - 1);  // gpet.py:117-119
  E.sigma_f = p.sigma_f;
  E.length_scale = p.length_scale;
  E.noise_y = p.noise_y;
  E.jitter = p.jitter;
  E.Yp = (Lg + 15) & ~15;
  return EdgeCheck::ok;
}

// The batch's dimensions: the largest of every capacity, the smallest ring.  (rng4 is the caller's: normals4_applies.)
inline BatchDims reduce_dims(const EdgeDev* edges, int B, int M, int N) {
  BatchDims bd{};
  bd.M = M;
  bd.N = N;
  bd.lg_even = 1;
  for (int e = 0; e < B; ++e) {
    const EdgeDev& E = edges[e];
    if (E.Lg > bd.Lg) bd.Lg = E.Lg;
    if (E.Lg & 1) bd.lg_even = 0;
    if (E.S > bd.S) bd.S = E.S;
    if (E.n_keep > bd.n_keep) bd.n_keep = E.n_keep;
    if (E.z_cols > bd.z_cols) bd.z_cols = E.z_cols;
    if (E.r_cap > bd.r_cap) bd.r_cap = E.r_cap;
    if (E.n_cap > bd.n_cap) bd.n_cap = E.n_cap;
    if (E.n_bins > bd.n_bins) bd.n_bins = E.n_bins;
    if (E.obs_cap > bd.obs_cap) bd.obs_cap = E.obs_cap;
    if (E.a_rows_cap > bd.a_rows_cap) bd.a_rows_cap = E.a_rows_cap;
    if (bd.z_ring == 0 || E.z_ring < bd.z_ring) bd.z_ring = E.z_ring;
    bd.jlog = E.jlog_cap > 0 ? 1 : 0;  // (the last edge's)
  }
  return bd;
}

// ---- arena ----------------------------------------------------------------------------------------------------------------

// the blocks that hold one slice per edge, contiguous over the batch: one copy moves them all
struct BatchBlocks {
  gpet_scalars* scalars;  // [B]
  double* fin_out;        // [B][2][bd.Lg]
  double* fin_par;        // [B][12]
  long long* obs;         // [B][bd.obs_cap][2]
  long long* init;        // [B][n_init_max][2]
  int n_init_max;
};

// ---- image map ------------------------------------------------------------------------------------------------------------
// Which image every edge of a batch reads: n_img image slots, edge e reads slot image_of[e] (a video frame or an OCT slice with a
// few edges on it: the layers of a retina, the two walls of a vessel).  "One image for all" is the map n_img = 1, all zeros;
// "one image per edge" keeps its own layout (the pair at the end of every edge's buffers).

// nullptr, or what is wrong with the map (every slot must be read by at least one edge; the edges of a slot need not be adjacent)
inline const char* image_map_check(int B, int n_img, const int32_t* image_of) {
  if (n_img < 1) return "n_img must be at least 1";
  if (n_img > B) return "more image slots than edges";
  if (!image_of) return "image_of is a null pointer";
  std::vector<char> used((size_t)n_img, 0);
  for (int e = 0; e < B; ++e) {
    if (image_of[e] < 0 || image_of[e] >= n_img) return "image_of holds an index outside [0, n_img)";
    used[(size_t)image_of[e]] = 1;
  }
  for (int g = 0; g < n_img; ++g)
    if (!used[(size_t)g]) return "an image slot is read by no edge";
  return nullptr;
}

// rep[g]: the slot's representative, the first edge that reads slot g (a checked map: every slot has one)
inline void image_map_reps(int B, int n_img, const int32_t* image_of, int* rep) {
  for (int g = 0; g < n_img; ++g) rep[g] = -1;
  for (int e = 0; e < B; ++e)
    if (rep[image_of[e]] < 0) rep[image_of[e]] = e;
}

// Lays out the whole arena and sets every pointer of every edge: the image slots, the batch-contiguous blocks, then edge by
// edge.  Called twice on the same edges: with cv.base == nullptr it measures (cv.off is the size; the pointers come out null),
// with the arena as base it places.  n_img (grad, grad_kde) pairs are taken at the front and edge e points at pair
// image_of[e] (image_of == nullptr: pair 0); n_img == 0: every edge takes a pair of its own behind its other buffers.
inline BatchBlocks layout_batch_slots(Carver& cv, EdgeDev* edges, int B, const BatchDims& bd, int n_img, const int32_t* image_of) {
  const size_t px = (size_t)bd.M * bd.N, gpx = (size_t)(bd.M + 2) * (bd.N + 2);
  std::vector<float*> slot_grad((size_t)n_img, nullptr), slot_kde((size_t)n_img, nullptr);
  for (int g = 0; g < n_img; ++g) {
    slot_grad[(size_t)g] = cv.take<float>(px);
    slot_kde[(size_t)g] = cv.take<float>(px);
  }
  BatchBlocks bb{};
  bb.n_init_max = 1;
  for (int e = 0; e < B; ++e) bb.n_init_max = edges[e].n_init > bb.n_init_max ? edges[e].n_init : bb.n_init_max;
  bb.scalars = cv.take<gpet_scalars>((size_t)B);
  bb.fin_out = cv.take<double>((size_t)B * 2 * bd.Lg);
  bb.fin_par = cv.take<double>((size_t)B * 12);
  bb.obs = cv.take<long long>((size_t)B * 2 * bd.obs_cap);
  bb.init = cv.take<long long>((size_t)B * 2 * (size_t)bb.n_init_max);
  auto slice = [](auto* block, size_t at) { return block ? block + at : nullptr; };  // (null while measuring)
  for (int e = 0; e < B; ++e) {
    EdgeDev& E = edges[e];
    const size_t Lg = E.Lg, nc = E.n_cap, rc = E.r_cap, S = E.S;
    E.sc = slice(bb.scalars, (size_t)e);
    E.fin_out = slice(bb.fin_out, (size_t)e * 2 * bd.Lg);
    E.fin_par = slice(bb.fin_par, (size_t)e * 12);
    E.obs_xy = slice(bb.obs, (size_t)e * 2 * bd.obs_cap);
    E.init_xy = slice(bb.init, (size_t)e * 2 * (size_t)bb.n_init_max);
    // (reserved: init_xy and obs_xy point into the batch blocks, but the space they once had per edge stays so that every address
    //  stays where it was measured; dropping it, here and below for fin_par, is a change of its own, to be timed)
    cv.skip<long long>(2 * (size_t)E.n_init);
    cv.skip<long long>(2 * (size_t)E.obs_cap);
    E.obs_new = cv.take<long long>(2 * (size_t)E.obs_cap);
    E.xt = cv.take<double>(nc);
    E.yt = cv.take<double>(nc);
    E.wt = cv.take<double>(nc);
    E.alpha = cv.take<double>(nc);
    // the scratch of the blocked fit (inverses of the diagonal blocks, the published solve vector, its flags), sized by the edge's
    // own capacity but taken whenever the BATCH is blocked: fit_plan (gpet_iter_plan.h) decides by bd.n_cap, so the blocked kernels
    // also run on an edge of 128 points or fewer that shares a batch with a larger one (and wrote past a one-element scratch)
    const bool blocked = bd.n_cap > 128;
    E.chol_inv = cv.take<double>(blocked ? (nc / 64 + 1) * 4096 : 1);
    E.solve_z = cv.take<double>(blocked ? nc : 1);
    E.solve_flag = cv.take<int>(blocked ? 2 * (nc / 64 + 1) : 2);
    E.K = cv.take<double>(nc * nc);
    E.V = cv.take<double>(nc * Lg);
    E.mean = cv.take<double>(Lg);
    E.std = cv.take<double>(Lg);
    E.cov = cv.take<double>(Lg * Lg);
    E.G = cv.take<double>(rc * Lg);
    E.perm = cv.take<int>(rc);
    E.C = cv.take<double>(rc * rc);
    E.W = cv.take<double>(rc * rc);
    E.Wq = cv.take<double>(2 * rc * rc);
    E.Cw = cv.take<double>(rc * rc);
    E.wq_tag = cv.take<int>(2);
    E.theta = cv.take<double>(rc);
    E.order = cv.take<int>(rc);
    E.Q0 = cv.take<double>(rc * Lg);
    E.lam0 = cv.take<double>(rc);
    E.beta = cv.take<double>(rc);
    E.h0 = cv.take<double>(rc);
    E.rho_tab = cv.take<double>((size_t)E.N);
    E.eig = cv.take<EigState>(1);
    // (transposed copy of G: the any-rank factor, and the multi-workgroup pivoted Cholesky -- which launch_factor picks per BATCH
    //  from the widest edge, pchol_plan of gpet_factor_plan.h, and which then writes Gt of EVERY edge of the batch: the condition is the
    //  batch's, and covers every width at which that plan can choose the multi-workgroup form)
    E.Gt = cv.take<double>((rc > (size_t)FACTOR_LDS_CAP || bd.Lg > PCH_ONE_WG_MAX) ? Lg * rc : 1);
    E.Ap = cv.take<double>(rc > (size_t)FACTOR_LDS_CAP ? 2 * Lg * rc : 1);
    E.ap_tag = cv.take<int>(3);
    E.pcx_d = cv.take<double>(Lg);
    E.pcx_cand = cv.take<double>(PCX_CAND_PER_WG * ((size_t)E.N / PCX_COLS + 2));  // (indexed with the widest edge of the batch)
    E.jlog = cv.take<double>(E.jlog_cap > 0 ? (size_t)E.jlog_cap * 2 * rc * (rc / 2 + 1) : 2);
    E.A = cv.take<double>((size_t)E.a_rows_cap * Lg + 64);  // (+ 64: the sample GEMM loads whole 64-column tiles of the last row)
    E.Z = cv.take<double>((size_t)E.z_ring * S * (size_t)E.z_cols);
    // (+ the spare region of the sample GEMM's idle lanes: they write 16 bytes at (Sround + 4 g) Yp + 2 lane doubles, g < 4, lane < 64 --
    //  up to 128 doubles into row Sround + 12 whatever the pitch is, so the slack is sized in elements, not in rows)
    E.Y = cv.take<double>((((S + 127) & ~(size_t)127) + 12) * (size_t)E.Yp + 128 + (size_t)E.Yp);
    E.costs = cv.take<double>(S);
    E.cost_part = cv.take<double>(S * 2 * (Lg / 30 + 2));  // (15 Simpson pairs = 30 columns per tile of the scorer)
    E.best_costs = cv.take<double>((size_t)E.n_keep + 1);
    E.best_idx = cv.take<int>((size_t)E.n_keep + 1);
    E.bins = cv.take<double>(gpx);
    E.tmpk = cv.take<double>(gpx);
    E.kde_wt = gpx >= (size_t)KDE_NB ? E.tmpk : nullptr;  // (the curve KDE's weights between k_kde_prep and k_kde_fused_r: see gpet_dev.h)
    E.kde = cv.take<float>(px);
    E.kde_band = cv.take<int>(2 * ((size_t)E.N / 16 + 2));
    E.colsum = cv.take<double>((size_t)E.N);
    E.kde_wsum = cv.take<double>(2);
    E.colbest = cv.take<double>((size_t)E.N);
    E.colbest_y = cv.take<int>((size_t)E.N);
    E.mm = cv.take<unsigned int>(4);
    E.binbest = cv.take<unsigned long long>((size_t)E.n_bins);
    E.binarg = cv.take<long long>((size_t)E.n_bins);
    E.fin_x = cv.take<double>(nc);
    E.fin_y = cv.take<double>(nc);
    E.fin_w = cv.take<double>(nc);
    cv.skip<double>(12);  // (reserved: fin_par points into the batch block)
    const size_t g = image_of ? (size_t)image_of[e] : 0;
    E.grad = n_img ? slot_grad[g] : cv.take<float>(px);
    E.grad_kde = n_img ? slot_kde[g] : cv.take<float>(px);
  }
  return bb;
}

// one image for all edges, or one per edge
inline BatchBlocks layout_batch(Carver& cv, EdgeDev* edges, int B, const BatchDims& bd, bool share_image) {
  return layout_batch_slots(cv, edges, B, bd, share_image ? 1 : 0, nullptr);
}

// a checked image map (image_map_check); n_img = 1 is the shared layout, offset for offset
inline BatchBlocks layout_batch(Carver& cv, EdgeDev* edges, int B, const BatchDims& bd, int n_img, const int32_t* image_of) {
  return layout_batch_slots(cv, edges, B, bd, n_img, image_of);
}

// ---- structured loop path -------------------------------------------------------------------------------------------------

// The prior eigenbasis indexes the grid [x_st, x_en]: every training point must lie on it.  Without fix_endpoints the pixel
// selection admits every image column (gpet.py:655-657 only filters when it is set), so the loop can accept observations outside
// the grid unless the edge spans the whole image; and every init x must lie on it.
inline bool struct_eligible(const EdgeDev* edges, int B, int N, const int64_t* const* init_xy) {
  for (int e = 0; e < B; ++e)
    if (!edges[e].fix_endpoints && !(edges[e].x_st == 0 && edges[e].x_en == N - 1)) return false;
  for (int e = 0; e < B; ++e)
    for (int i = 0; i < edges[e].n_init; ++i) {
      const int64_t x = init_xy[e][2 * i];
      if (x < edges[e].x_st || x > edges[e].x_en) return false;
    }
  return true;
}

// Edges of the same grid length, first column, kernel and length scale have the same prior eigenbasis bit for bit (k_rho_fill
// forms the lags as fl((x_st+i)/l) - fl((x_st+j)/l), which depends on x_st in the last bits unless l is a power of two -- so
// x_st is part of the match; the amplitude is not: the matrix has unit amplitude).  reps: the first edge of every such class, in
// order; rep_of[e]: the edge whose basis e reads.  Only the last eight representatives are searched (batches are homogeneous or
// nearly so), so an edge that matches an older one founds a class of its own.
inline void basis_classes(const EdgeDev* edges, int B, std::vector<int>& rep_of, std::vector<int>& reps) {
  rep_of.assign((size_t)B, 0);
  reps.clear();
  for (int e = 0; e < B; ++e) {
    const EdgeDev& E = edges[e];
    int found = -1;
    for (size_t k = reps.size() > 8 ? reps.size() - 8 : 0; k < reps.size() && found < 0; ++k) {
      const EdgeDev& F = edges[reps[k]];
      if (F.Lg == E.Lg && F.x_st == E.x_st && F.kernel_type == E.kernel_type && F.nu_code == E.nu_code && F.nu_gen == E.nu_gen &&
          F.length_scale == E.length_scale && F.r_cap == E.r_cap)
        found = reps[k];
    }
    if (found < 0) {
      found = e;
      reps.push_back(e);
    }
    rep_of[(size_t)e] = found;
  }
}

// (n_cap <= 128: k_struct_H keeps U in LDS -- it must fit with L streamed row by row; larger: U in HBM, blocked)
inline bool struct_h_fits_lds(const BatchDims& bd, int r0_max) {
  return bd.n_cap > 128 ||
         ((size_t)bd.n_cap * (r0_max | 1) + bd.n_cap + bd.r_cap) * sizeof(double) <= (size_t)STRUCT_H_LDS_MAX;
}

// ---- scalars --------------------------------------------------------------------------------------------------------------

// every edge's device scalars as a fresh batch has them
inline void pristine_scalars(const gpet_params* params, const EdgeDev* edges, int B, gpet_scalars* out) {
  for (int e = 0; e < B; ++e) {
    memset(&out[e], 0, sizeof out[e]);
    out[e].score_thresh = params[e].score_thresh;
    out[e].done = (0 >= edges[e].algo_thresh) ? 1 : 0;  // gpet.py:829 with no observations yet
  }
}

}  // namespace gpet
