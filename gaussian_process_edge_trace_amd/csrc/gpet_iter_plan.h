// What the launchers of one loop iteration (gpet_k_launch.inc) decide, as plain data: the batch's dimensions in, which kernel variant
// runs each step, its grid, its workgroup and its dynamic LDS out.  No HIP and no options (option values come in as integers), so the
// host compiler alone builds it (tests/test_iter_plan.py).  Every rule is written here ONCE; the tile constants the rules need are
// defined here and the kernels use them under the same names.
#pragma once
#include <stddef.h>

#include "gpet_batch_plan.h"  // BatchDims, LDS_DYN_MAX

namespace gpet {

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// ---- tile constants ---------------------------------------------------------------------------------------------------------
constexpr int GEMM_KMAX = 96;  // factor capacity up to which the sample GEMM keeps its rows of Z in registers
// row stride of the factor chunk in LDS (doubles): the operand read of a matrix instruction takes 16 consecutive columns of
// FOUR rows (k = 4 q + lq); with 80 (= 32 dwords mod 64) the rows of each half-wave fall on disjoint bank halves -- 65 put
// rows 2 banks apart and every read was a 2-way conflict
#ifndef GEMM_LDA
#define GEMM_LDA 80
#endif
constexpr int GEMM32_LDA = 80;  // the same stride in floats (gpet_k_sample_f32.inc)
constexpr int GEMM_LDS_MAX = LDS_DYN_MAX;
constexpr int SC_PAIRS = 15;  // Simpson pairs per tile: 8 lanes x 2 pairs per curve; the sixteenth pair (= the next tile's first) only supplies data
constexpr int SC_CURVES = 1024, SC_THREADS = 1024;
constexpr int KDE_TX = 16;
constexpr int KDE_H = 128;   // image rows per LDS row-chunk
// (KDE_NB = 128 curves staged per pass: gpet_batch_plan.h, which sizes kde_wt by it)
constexpr int KDE_THREADS = 512;
constexpr int KDE_PREP_MAXB = 1024;  // kept curves k_kde_prep stages in LDS
constexpr int PIX_CX = 32;   // columns per workgroup of k_pix_columns
constexpr int SR_TJ = 64;    // grid columns per workgroup of k_struct_rows
constexpr int CB = 64;       // block of the blocked Cholesky / substitution kernels

struct Grid3 {
  int x, y, z;
};

// ---- the K extent of a rank -------------------------------------------------------------------------------------------------
// KS steps of 4 (a template parameter of the sample GEMMs and of k_struct_rows): ceil(rank / 4) raised to the next of K_EXTENTS;
// mt: the 16-row tiles of k_struct_rows' eigenvector tile that go with it
constexpr int K_EXTENTS[6] = {8, 12, 16, 18, 20, 24};
constexpr int K_EXTENT_MT[6] = {2, 3, 4, 5, 5, 6};
struct KExtent {
  int ks, mt;
};
constexpr KExtent k_extent(int rank) {
  const int ks = (rank + 3) >> 2;
  for (int i = 0; i < 5; ++i)
    if (ks <= K_EXTENTS[i]) return {K_EXTENTS[i], K_EXTENT_MT[i]};
  return {K_EXTENTS[5], K_EXTENT_MT[5]};
}

// ---- sample GEMM ------------------------------------------------------------------------------------------------------------
// rank <= 96 everywhere in the batch (factor capacity): Z rows stay in registers (`reg`); otherwise (full factors injected by tests,
// Matern ranks) the K-chunked generic kernel.  rank_max: the largest rank any edge can have in this launch (r0_max inside the
// structured loop, else 0: the factor capacity).  f32mma (bd.y_arith): the GEMM on the f32 matrix cores, whose register form always
// keeps the posterior mean in LDS, so an edge too wide for that (about 15 000 columns) takes the generic form.
struct SamplePlan {
  bool reg;        // register form (k_sample_gemm_mfma_r / _rl, k_sample_f32_r), else generic (k_sample_gemm_mfma, k_sample_f32)
  int ks;          // register form: the K extent
  bool rl;         // f64 register form: the one-workgroup-per-CU kernel _rl (KS 20, 24)
  bool y_f32;      // f64 arithmetic: samples stored as f32
  bool mu_in_lds;  // the posterior mean sits behind the chunk in LDS (else the epilogue reads it from global memory)
  int rparts;      // row blocks of 128 samples
  int ncs;         // column runs per row block: while the row blocks alone leave CUs empty (small batches are latency chains)
  Grid3 grid;
  int block;
  size_t lds;
};
inline SamplePlan sample_plan(const BatchDims& bd, int B, int rank_max, bool f32mma) {
  SamplePlan p = {};
  p.y_f32 = bd.y_f32 != 0;
  const size_t mu_bytes = ((size_t)bd.Lg + 64) * sizeof(double);
  p.reg = bd.r_cap <= GEMM_KMAX && bd.a_rows_cap <= GEMM_KMAX &&
          (!f32mma || (size_t)4 * 24 * GEMM32_LDA * sizeof(float) + mu_bytes <= (size_t)GEMM_LDS_MAX);
  if (!p.reg) {
    p.grid = {cdiv(bd.Lg, 64), cdiv(bd.S, 64), B};
    p.block = 256;
    return p;
  }
  const int rm = rank_max > 0 && rank_max <= bd.r_cap ? rank_max : (bd.r_cap > bd.a_rows_cap ? bd.r_cap : bd.a_rows_cap);
  p.ks = k_extent(rm).ks;
  p.rl = !f32mma && p.ks >= 20;
  const int ctiles = cdiv(bd.Lg, 64);
  p.rparts = cdiv(bd.S, 128);
  p.ncs = cdiv(256, B * p.rparts);
  p.ncs = p.ncs > ctiles ? ctiles : (p.ncs < 1 ? 1 : p.ncs);
  if (p.ncs > 8) p.ncs = 8;
  p.grid = {p.rparts * p.ncs, B, 1};
  p.block = 512;
  // (an f64 edge too wide for its posterior mean to sit behind the largest chunk reads it from global memory in the epilogue)
  p.mu_in_lds = f32mma || (size_t)4 * 24 * GEMM_LDA * sizeof(double) + mu_bytes <= (size_t)GEMM_LDS_MAX;
  p.lds = (f32mma ? (size_t)4 * p.ks * GEMM32_LDA * sizeof(float) : (size_t)4 * p.ks * GEMM_LDA * sizeof(double)) +
          (p.mu_in_lds ? mu_bytes : 0);
  return p;
}

// ---- curve scorer -----------------------------------------------------------------------------------------------------------
inline int score_tiles(int Lg) { return cdiv((Lg - 2) / 2, SC_PAIRS); }
// the costs of rows 0 .. S - 1 of every edge's sample matrix.  Which kernels run is decided by the BATCH's shape, bd, whatever S is
// (a row's cost does not depend on S): the tiled scorer (k_score_tile + k_score_combine) where its image slab fits LDS and the
// batch has 64 samples, else the wave-per-curve k_score
struct ScorePlan {
  bool tiled;
  int n_tiles;
  int cpw;  // curves per workgroup: 1024, or down to 128 while the tiles alone leave CUs empty (every part stages the slab again)
  size_t lds;
  Grid3 tile_grid, combine_grid;  // tiled: k_score_tile (SC_THREADS), k_score_combine (256)
  Grid3 wave_grid;                // else: k_score (256)
};
inline ScorePlan score_plan(const BatchDims& bd, int B, int S) {
  ScorePlan p = {};
  p.lds = (size_t)(2 * SC_PAIRS + 2) * (bd.M | 1) * sizeof(float);
  p.tiled = p.lds <= (size_t)LDS_DYN_MAX && bd.S >= 64;
  if (!p.tiled) {
    p.lds = 0;
    p.wave_grid = {cdiv(S, 4), B, 1};
    return p;
  }
  p.n_tiles = score_tiles(bd.Lg);
  p.cpw = SC_CURVES;
  while (p.cpw > 128 && B * p.n_tiles * cdiv(S, p.cpw) < 256) p.cpw >>= 1;
  p.tile_grid = {p.n_tiles, cdiv(S, p.cpw), B};
  p.combine_grid = {cdiv(S, 256), B, 1};
  return p;
}
// top-k by the bitonic sort k_topk_sort (else rank counting, k_topk); topk_rank: the option of that name
inline bool topk_bitonic(const BatchDims& bd, int topk_rank) { return bd.S <= 1024 && !topk_rank; }
// k_score_combine, k_topk_sort and k_kde_prep's staged form as ONE launch (k_score_tail): needs the tiled scorer's partial sums
inline bool score_tail_applies(const BatchDims& bd, int topk_rank) {
  return score_plan(bd, 1, bd.S).tiled && topk_bitonic(bd, topk_rank) && bd.n_keep <= KDE_PREP_MAXB;
}

// ---- curve KDE, pixel selection ---------------------------------------------------------------------------------------------
struct KdeFusedPlan {
  Grid3 grid;  // k_kde_fused (KDE_THREADS): one workgroup per (tile of KDE_TX columns, edge)
  size_t lds;  // the (KDE_TX + 8) x (KDE_H + 8) tile, KDE_NB staged curves of KDE_TX + 8 points, their weights
};
inline KdeFusedPlan kde_fused_plan(const BatchDims& bd, int B) {
  return {{cdiv(bd.N, KDE_TX), B, 1},
          ((size_t)(KDE_TX + 8) * ((KDE_H + 8) | 1) + (size_t)KDE_NB * (KDE_TX + 8) + KDE_NB) * sizeof(double)};
}
// the register form k_kde_fused_r (option kde_variant = 1): every kept curve fits ONE staging pass, so a thread keeps its
// KDE_NB (KDE_TX + 8) / KDE_THREADS = 6 points in registers from the loads to the binning and LDS holds only the tile and the weights:
// 27 328 B, four workgroups of eight waves per CU (kde_fused_plan's 51 904 B: three).  Else (more curves, a grid too small to
// lend kde_wt its KDE_NB doubles, variant 0) the staged form
struct KdeRegPlan {
  bool applies;
  Grid3 grid;  // k_kde_fused_r (KDE_THREADS): as kde_fused_plan's
  size_t lds;  // the (KDE_TX + 8) x (KDE_H + 8) tile, KDE_NB weights
};
inline KdeRegPlan kde_reg_plan(const BatchDims& bd, int B, int kde_variant) {
  const bool applies = kde_variant != 0 && bd.n_keep <= KDE_NB && (size_t)(bd.M + 2) * (bd.N + 2) >= (size_t)KDE_NB;
  return {applies, {cdiv(bd.N, KDE_TX), B, 1}, ((size_t)(KDE_TX + 8) * ((KDE_H + 8) | 1) + KDE_NB) * sizeof(double)};
}
static_assert(KDE_NB * (KDE_TX + 8) % KDE_THREADS == 0, "k_kde_fused_r: a whole number of points per thread");
struct PixelPlan {
  Grid3 columns, old, argbest, select;  // k_pix_columns, k_pix_old, k_pix_argbest (256 threads each), k_pix_select (64)
};
inline PixelPlan pixel_plan(const BatchDims& bd, int B) {
  const int nt = bd.N > bd.obs_cap ? bd.N : bd.obs_cap;
  return {{cdiv(bd.N, PIX_CX), B, 1}, {cdiv(bd.obs_cap, 256), B, 1}, {cdiv(nt, 256), B, 1}, {1, B, 1}};
}

// ---- fit, predict -----------------------------------------------------------------------------------------------------------
struct FitPlan {
  bool in_lds;  // k_fit<true, .> (576 threads): K and a vector in LDS; else the blocked factorisation in HBM
  size_t lds;
};
inline FitPlan fit_plan(const BatchDims& bd) {
  const bool in_lds = bd.n_cap <= 128;
  return {in_lds, in_lds ? ((size_t)bd.n_cap * (bd.n_cap | 1) + bd.n_cap) * sizeof(double) : 0};
}
enum class PredictForm {
  lds,          // k_predict<true, .>: a wave keeps its 64 columns of V in LDS
  global,       // k_predict<false, true>: the converged fit of many training points
  through_hbm,  // the loop's fit of many training points: V through HBM, blocked substitution on the matrix cores
};
struct PredictPlan {
  PredictForm form;
  size_t lds;  // form lds: [n_cap][64] of V, a row of L, x / l, alpha
};
inline PredictPlan predict_plan(const BatchDims& bd, bool final_fit) {
  const size_t plds = ((size_t)bd.n_cap * 64 + 3 * (size_t)bd.n_cap) * sizeof(double);
  if (plds <= (size_t)LDS_DYN_MAX) return {PredictForm::lds, plds};
  return {final_fit ? PredictForm::global : PredictForm::through_hbm, 0};
}

// ---- structured path --------------------------------------------------------------------------------------------------------
struct StructHPlan {
  bool l_in_lds;  // k_struct_H keeps L beside U in LDS (else rows of L are streamed: gpet_batch_create checked that this fits)
  size_t lds;
};
inline StructHPlan struct_h_plan(const BatchDims& bd) {
  const size_t full = ((size_t)bd.n_cap * (bd.r0_max | 1) + (size_t)bd.n_cap * (bd.n_cap + 1) / 2 + bd.r_cap) * sizeof(double);
  const size_t rowm = ((size_t)bd.n_cap * (bd.r0_max | 1) + bd.n_cap + bd.r_cap) * sizeof(double);
  const bool l_in_lds = full <= (size_t)STRUCT_H_LDS_MAX;
  return {l_in_lds, l_in_lds ? full : rowm};
}
struct StructRowsPlan {
  int mt, ks;  // k_struct_rows<MT, KS> (256 threads): [4 KS][16 MT + 1] eigenvector tile
  size_t lds;  // (+ the signs of the rows)
  Grid3 grid;
};
inline StructRowsPlan struct_rows_plan(const BatchDims& bd, int B) {
  const KExtent k = k_extent(bd.r0_max);
  return {k.mt, k.ks, ((size_t)4 * k.ks * (16 * k.mt + 1) + 16 * k.mt) * sizeof(double), {cdiv(bd.Lg, SR_TJ), B, 1}};
}

}  // namespace gpet
