// Kernel launchers (internal).
#pragma once
#include <hip/hip_runtime.h>

#include "gpet_batch_plan.h"  // EdgeDev (gpet_dev.h), BatchDims, STRUCT_H_LDS_MAX
#include "gpet_iter_plan.h"   // one loop iteration: kernel variant, grid and LDS of every step; the tile constants
#include "gpet_factor_plan.h"  // eigen-factor stage: kernel variant, grid and LDS of every launch; the layouts its kernels share with it
#include "gpet_conv_plan.h"   // pixel types, conv geometry, staging plan
#include "gpet_conv_multi_plan.h"  // slot table of a multi-kernel source: validation, union patch, slots of each frame
#include "gpet_transpose_plan.h"  // vertical batches: the index map, the tile transpose, the transposed-store convolution
#include "gpet_denoise_plan.h"  // denoising spec, workspace layout, chunking
#include "gpet_nlmeans_plan.h"  // non-local means: spec, LDS patch, grid, the exponential
#include "gpet_nlfast_plan.h"   // fast-mode non-local means: spec, shift table, groups, workspace, launch geometry
#include "gpet_wavelet_plan.h"  // wavelet denoising: spec, levels, pyramid layout, tiles, the threshold's summation order
#include "gpet_metrics_plan.h"  // denoise quality metrics: working type, running-sum filter, S, keys, the one summation order
#include "gpet_tvb_plan.h"      // split-Bregman TV denoising: spec, skewed workspace, workgroup, sweeps per launch, the order of acc
#include "gpet_polar_plan.h"    // polar unwrap: spec, column-to-angle map, sample position, bilinear value, launch geometry
#include "gpet_history_plan.h"  // iteration history: record layout, workgroups per edge
#include "gpet_ensemble_plan.h"  // seed ensembles: layout of the returned buffer, validation, member tables, tile width
#include "gpet_band_plan.h"  // tracking bands: refusals, the placement rule, the sizes of what a banded batch owns in addition
#include "gpet_init_plan.h"  // endpoint tracking: the rule that moves the init points, its refusals
#include "gpet_label_plan.h"  // label maps: the two rules, their refusals, the fill kernels' launch shapes
#include "gpet_warm_plan.h"  // warm start from a group's medoid / best cost / consensus or from another edge: source per edge, refusals

namespace gpet {

// int64 of an integer-valued double, from its bits: what x86's truncating conversion (numpy's astype(int)) gives, INT64_MIN
// for NaN and out-of-range values included.  (The compiler's f64 -> i64 conversion splits the value with a fused
// multiply-add; this keeps the kernel free of them, so the disassembly shows that the interval is not contracted.)
__device__ inline long long int_f64_to_i64(double r) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(r);
  const int biased = (int)((u >> 52) & 0x7ff);
  if (biased < 1023) return 0;                             // |r| < 1: rint left +-0 (subnormals are not integers)
  const int ex = biased - 1075;                            // |r| = mant * 2^ex
  if (ex >= 11) return (long long)0x8000000000000000ull;   // |r| >= 2^63, inf, NaN
  const unsigned long long mant = (u & 0xfffffffffffffull) | (1ull << 52);
  const unsigned long long mag = ex >= 0 ? mant << ex : mant >> -ex;
  return (u >> 63) ? -(long long)mag : (long long)mag;
}

// hipFuncSetAttribute applies to the CURRENT device: remember per device what has been raised, so that one process
// may hold contexts on several GPUs (the launchers run with the context's device current).
struct PerDeviceOnce {
  bool done[64] = {};
  bool first() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return true;
    if (done[d]) return false;
    done[d] = true;
    return true;
  }
};
inline dim3 dim3_of(const Grid3& g) { return dim3(g.x, g.y, g.z); }

hipError_t launch_conv(hipStream_t st, const double* d_img, int M, int N, const double* d_wf, int kh, int kw, int oy,
                       int ox, float* d_tmp, unsigned int* d_minmax);
hipError_t launch_minmax(hipStream_t st, const float* d_in, size_t count, unsigned int* d_minmax);
hipError_t launch_normalise(hipStream_t st, const float* d_in, size_t count, const unsigned int* d_minmax,
                            float* d_out);
// a1 for a stack of raw frames (pix: PIX_* of gpet_conv_plan.h): images img0 .. img0 + n - 1 of the DEVICE pointer tables, one
// launch each; every image of the stack has its own (min, max) slot in d_minmax.  tr: a vertical batch (gpet_transpose_plan.h) -- the
// image at d_dst[g] is the N x M transpose of the M x N gradient image, per pixel the same bits and the same (min, max) slot
hipError_t launch_conv_batch(hipStream_t st, int pix, bool tr, const void* const* d_src, int img0, int n, int M, int N, const double* d_wf,
                             int kh, int kw, float* const* d_dst, unsigned int* d_minmax);
// the same for a slot table (gpet_conv_multi_plan.h): frames frame0 .. frame0 + n - 1 of d_src, every slot of each of them, one
// launch; d_dst and d_minmax are per slot
hipError_t launch_conv_multi(hipStream_t st, int pix, bool tr, const void* const* d_src, int frame0, int n, int M, int N, const double* d_wf,
                             const ConvUnion& u, const ConvKernDesc* d_kd, const int32_t* d_slot_off, const int32_t* d_slot_list,
                             const int32_t* d_kernel_of, float* const* d_dst, unsigned int* d_minmax);
hipError_t launch_normalise_batch(hipStream_t st, float* const* d_imgs, int n, size_t count, const unsigned int* d_minmax);
// an M x N f32 image on the device -> the N x M one at d_out, out of place; d_minmax != nullptr: every element through
// launch_normalise's arithmetic with that (min, max) pair on its way
hipError_t launch_transpose(hipStream_t st, const float* d_in, int M, int N, const unsigned int* d_minmax, float* d_out);
// a0 (gpet_denoise_plan.h): images img0 .. img0 + n - 1 of the DEVICE pointer table d_src (pixel type pix) are the n images of a chunk
// whose workspace starts at ws; the denoised frame lands at L.off_out of every image's block.  One launch (two for the Gaussian's
// passes) whatever n is; d_wy / d_wx: the Gaussian taps of the two axes on the device
hipError_t launch_dn_rank(hipStream_t st, int pix, const void* const* d_src, int img0, int n, int M, int N, const DenoiseSpec& s,
                          char* ws, const DenoiseLayout& L);
hipError_t launch_dn_gauss(hipStream_t st, int pix, const void* const* d_src, int img0, int n, int M, int N, const DenoiseSpec& s,
                           const double* d_wy, const double* d_wx, char* ws, const DenoiseLayout& L);
// iteration `it` of tvc for the chunk's unfinished images, then the stopping test (d_n_iter: per image of the stack, d_n_done: one
// counter of the chunk)
hipError_t launch_dn_tvc_iter(hipStream_t st, int pix, const void* const* d_src, int img0, int n, int M, int N, const DenoiseSpec& s,
                              int it, char* ws, const DenoiseLayout& L, int* d_n_iter, int* d_n_done);
// a0, non-local means (gpet_nlmeans_plan.h): frames img0 .. img0 + n - 1 of the DEVICE pointer table d_src (pixel type pix) -> the f64
// frames of the DEVICE pointer table d_dst at the same indices; s: the odd patch extent, d_taps: [s * s] on the device
hipError_t launch_nlmeans(hipStream_t st, int pix, const void* const* d_src, double* const* d_dst, int img0, int n, int M, int N, int s,
                          int d, const double* d_taps, double var2);
// a0, fast-mode non-local means (gpet_nlfast_plan.h): frames img0 .. img0 + n - 1 of the DEVICE pointer table d_src (pixel type pix) ->
// the f64 frames of the DEVICE pointer table d_dst at the same indices: one padding launch, then per group of shifts one integral
// and one gather launch.  p: nlf_plan of the frames and the spec; ws: the chunk's n workspaces (p.frame_bytes apart)
hipError_t launch_nlfast(hipStream_t st, int pix, const void* const* d_src, double* const* d_dst, int img0, int n, int M, int N,
                         const NlfSpec& sp, const NlfPlan& p, char* ws);
// polar unwrap (gpet_polar_plan.h): frames img0 .. img0 + n - 1 of the DEVICE pointer table d_src (pixel type pix, M x N) -> the f64
// frames [n_r x W] of the DEVICE pointer table d_dst at the same indices, one launch.  d_cxy: cx [n_centres] | cy [n_centres] on the
// device, indexed by frame like the tables (n_centres 1: one centre for all); d_cos / d_sin: [n_theta] on the device
hipError_t launch_polar(hipStream_t st, int pix, const void* const* d_src, double* const* d_dst, int img0, int n, int M, int N,
                        const PolarSpec& sp, const double* d_cxy, int n_centres, const double* d_cos, const double* d_sin);
// a0, wavelet denoising (gpet_wavelet_plan.h): frames img0 .. img0 + n - 1 of the DEVICE pointer table d_src (pixel type pix) -> the
// f64 frames of the DEVICE pointer table d_dst at the same indices, 2 levels + 2 launches (one fewer with injected thresholds).  ws: the
// chunk's n pyramids; d_sigma [frames], d_thr / d_ms [frames * levels * 3] on the device, indexed by frame like the tables -- with
// sp.thresholds the caller has filled d_thr.  sp.thresholds is only looked at for null.
hipError_t launch_wavelet(hipStream_t st, int pix, const void* const* d_src, double* const* d_dst, int img0, int n, const WvPlan& p,
                          const WvSpec& sp, char* ws, double* d_sigma, double* d_thr, double* d_ms);
// a0, split-Bregman TV denoising (gpet_tvb_plan.h): frames img0 .. img0 + n - 1 of the DEVICE pointer table d_src (pixel type pix) ->
// the f64 frames of the DEVICE pointer table d_dst at the same indices: one prologue, tvb_launches(max_iter) sweep launches, one
// epilogue.  ws: the chunk's n workspaces (tvb_frame_bytes apart); d_state [frames] on the device, zero before the first launch
hipError_t launch_tvb(hipStream_t st, int pix, const void* const* d_src, double* const* d_dst, int img0, int n, int M, int N,
                      const TvbSpec& sp, char* ws, TvbState* d_state);
// denoise quality metrics (gpet_metrics_plan.h): pairs img0 .. img0 + n - 1 of the DEVICE table d_tab (a, b per pair) -> the sums of
// d_acc and the S map in every pair's workspace (ws, `stride` bytes apart); launch_metrics_entropy, afterwards, sorts b's keys over the
// intermediate planes (S stays) and adds the entropy terms
hipError_t launch_metrics(hipStream_t st, const void* const* d_tab, MetricsAcc* d_acc, int img0, int n, int pix_a, int pix_b, int M, int N,
                          const MetricsSpec& sp, double R_ssim, char* ws, size_t stride);
hipError_t launch_metrics_entropy(hipStream_t st, const void* const* d_tab, MetricsAcc* d_acc, int img0, int n, int pix_b, int M, int N, char* ws,
                                  size_t stride);
hipError_t launch_fit_predict(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, int want_cov,
                              unsigned parts = ~0u);
hipError_t launch_final_predict(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd);
hipError_t launch_final_cov(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd);
// (single_wg_pchol: the pivoted Cholesky by k_pchol / k_pchol_reg whatever the width -- the prior eigenbasis, whose bits every trace inherits)
hipError_t launch_factor(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, unsigned parts = ~0u,
                         const EdgeDev* h_edges = nullptr, bool single_wg_pchol = false);
// csrc/gpet_eig.hip: the pivoted Cholesky of a wide edge of rank <= 96 by the multi-workgroup kernels of the any-rank factor
// (pchol_plan of gpet_factor_plan.h with the option pchol_multi chooses that form; p: that plan's `multi`)
bool pchol_multi_applies(const BatchDims& bd);
hipError_t launch_pchol_multi(hipStream_t st, EdgeDev* d_edges, int B, const PcholMultiPlan& p);
hipError_t launch_struct_iteration(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, unsigned parts = ~0u);
hipError_t launch_struct_basis(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd);
hipError_t launch_normals(hipStream_t st, EdgeDev* d_edges, int B, const unsigned int* d_seeds, int add_iter,
                          int iter_abs, int n_ahead, int z_store = 0);
// the same stream, state in registers, four streams per wave (gpet_rng.hip): where the batch allows it (option rng4 decides
// when, gpet_api_ctx.hip)
bool normals4_applies(const EdgeDev* h_edges, int B);
hipError_t launch_normals4(hipStream_t st, EdgeDev* d_edges, int B, const unsigned int* d_seeds, int add_iter, int iter_abs,
                           int n_ahead, int z_store, int Lg, int S, int zc);
// opt-in counter-based generator (Philox4x32-10 + Box-Muller; gpet_batch_set_rng): not the reference's stream
hipError_t launch_normals_philox(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, const unsigned int* d_seeds,
                                 int add_iter, int iter_abs, int n_ahead, int z_store);
// one long normal stream generated by many workgroups (MT19937 jump-ahead; gpet_kernels.hip, k_mtj_*): chunk count for a
// stream of `normals` values (0: beyond the jump tables), workspace size, the jump tables (to be copied to the device
// once), and the launch sequence
int mtj_chunks(long long normals);
size_t mtj_work_bytes(int streams, int nc);
const unsigned int* mtj_poly_host();
size_t mtj_poly_bytes();
hipError_t launch_normals_chunked(hipStream_t st, EdgeDev* d_edges, int B, const unsigned int* d_seeds, int add_iter,
                                  int iter_abs, int n_ahead, int z_store, void* work, int nc, const unsigned int* d_poly);
hipError_t launch_kde(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, int mode, unsigned parts = ~0u,
                      int raw_band = 0);
hipError_t launch_pixels(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, int raw_band = 0, unsigned parts = ~0u);
// any-rank factor (gpet_eig.hip): pivoted Cholesky over the whole GPU + one-sided block Jacobi on its rows
hipError_t launch_factor_big(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, const EdgeDev* h_edges = nullptr);
hipError_t launch_set_force(hipStream_t st, EdgeDev* d_edges, int B, int v);
hipError_t launch_rho_tab(hipStream_t st, EdgeDev* d_edges, int B, int N);
hipError_t launch_fin_scatter(hipStream_t st, EdgeDev* d_edges, int B, const double* d_stage, const int* d_n, int stride);
// the next frame's observation sets from the last converged fits (gpet_k_warm.inc): one wave per edge
hipError_t launch_warm_start(hipStream_t st, EdgeDev* d_edges, int B, int warm_every);
// d_src[e] of every edge from the heads of the kept ensemble's records (d_kept, records of record_bytes) and d_group_of, by warm_source
hipError_t launch_warm_sources(hipStream_t st, int B, const int32_t* d_group_of, const char* d_kept, long long record_bytes, int from,
                               int32_t* d_src);
// k_warm_start with the trace of edge e taken from d_src[e]: another edge's fit, the consensus row of its group's kept record (d_group_of,
// d_kept; both may be nullptr when no entry is WARM_SRC_CONSENSUS), or nothing
hipError_t launch_warm_start_src(hipStream_t st, EdgeDev* d_edges, int B, const int32_t* d_src, const int32_t* d_group_of, const char* d_kept,
                                 long long record_bytes, long long off_trace, int warm_every);
// tracking bands (gpet_k_band.inc; the rule: gpet_band_plan.h).  The int64 tables are the banded batch's own, on the device.
// r0_pend[e] = band_place of edge e from the trace of its source (d_src == nullptr: the edge itself; else as launch_warm_start_src)
hipError_t launch_band_place(hipStream_t st, const EdgeDev* d_edges, int B, const int32_t* d_src, const int32_t* d_group_of, const char* d_kept,
                             long long record_bytes, long long off_trace, long long M, const long long* d_r0_fit, const long long* d_r0_cur,
                             const long long* d_lohi, long long* d_r0_pend);
// r0_cur = r0_pend, and every edge's init rows in the coordinates of its new band
hipError_t launch_band_apply(hipStream_t st, const EdgeDev* d_edges, int B, int n_init_max, const long long* d_r0_pend,
                             const long long* d_init_full, long long* d_r0_cur);
// launch_minmax + launch_normalise of the band d_G_of[e] + r0_cur[e] * N (H x N) into EdgeDev::grad of every edge e
hipError_t launch_band_images(hipStream_t st, const EdgeDev* d_edges, int B, const float* const* d_G_of, const long long* d_r0_cur, int H,
                              int N, unsigned int* d_minmax);
// launch_warm_start_src across bands: every row through r0_fit[source] - r0_cur[e]
hipError_t launch_warm_start_band(hipStream_t st, EdgeDev* d_edges, int B, const int32_t* d_src, const int32_t* d_group_of, const char* d_kept,
                                  long long record_bytes, long long off_trace, int warm_every, const long long* d_r0_fit,
                                  const long long* d_r0_cur);
// endpoint tracking (gpet_k_init.inc; the rule: gpet_init_plan.h): every init row of every edge onto the edge of EdgeDev::grad.  A banded
// batch passes its tables (r0 of the slots, the full-frame init points, (i_lo, i_hi)), which are then written too; else three nullptr
hipError_t launch_init_follow(hipStream_t st, const EdgeDev* d_edges, int B, int window, int cols, int n_init_max, const long long* d_r0_cur,
                              long long* d_init_full, long long* d_lohi);
// the record of the iteration just completed for every edge whose counter equals iter_expect (0: every edge with a counter >= 1), gpet_k_history.inc
hipError_t launch_history(hipStream_t st, const EdgeDev* d_edges, int B, const gpet_history_plan& P, int iter_expect);
hipError_t launch_pixels_reset(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd);
hipError_t launch_sample(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, int rank_max = 0);
hipError_t launch_score(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, unsigned parts = ~0u, bool no_combine = false);
// part 1 of launch_score (the costs) over the first S rows of every edge's sample matrix, by the variant bd selects (launch_score: S = bd.S)
hipError_t launch_score_rows(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd, int S, bool no_combine);
bool score_tail_applies(const BatchDims& bd);  // (gpet_iter_plan.h's rule with the option topk_rank)
// seed ensembles (gpet_k_ensemble.inc).  Final costs: the scorer on a one-row view of every edge's converged mean -- view / view_sc
// [B], rows [B][row_stride] doubles (row_stride >= the widest row pitch), part [B][fincost_part_stride] doubles, cost [B]
size_t fincost_part_stride(const BatchDims& bd);
hipError_t launch_final_costs(hipStream_t st, const EdgeDev* d_edges, int B, const BatchDims& bd, EdgeDev* d_view, gpet_scalars* d_view_sc,
                              double* d_rows, size_t row_stride, double* d_part, double* d_cost);
// the reduction (k_ensemble over the plan's workgroups, then k_ensemble_pick) into DEVICE memory d_dst, zeroed by the caller like d_off_acc [B]
hipError_t launch_ensemble(hipStream_t st, const EdgeDev* d_edges, int B, int G, const EnsembleGroup* d_groups, const int32_t* d_members,
                           const int32_t* d_member_group, const int32_t* d_wg_group, const int32_t* d_wg_tile, int n_wg, size_t lds,
                           double tol, long long len_cap, const EnsembleLayout& L, const double* d_cost, int* d_off_acc, char* d_dst);
// label maps (gpet_k_label.inc; the rules: gpet_label_plan.h).  A contributing edge as the kernels read it, in map order: its grid, its
// map (the centre of Rule 2), and where its rows come from -- edge >= 0: the converged fit of that edge of the batch; edge < 0: the int64
// rows the caller gave, row_off into them
struct LabelEdge {
  int32_t x_st, len, edge, map;
  long long row_off;
};
// T [n_used][N] int32: d_rows for the stand-alone form (d_edges unused), d_edges / d_r0_fit (nullptr: no bands) for the batch form
hipError_t launch_label_thresholds(hipStream_t st, const LabelEdge* d_le, int n_used, const long long* d_rows, const EdgeDev* d_edges,
                                   const long long* d_r0_fit, int M, int N, bool extend, int* d_T);
// map f of n_maps (edges map_off[f] .. map_off[f + 1] of T; L the most on one map) to d_out0 + d_out_off[f]: M x N bytes, or N x M transposed
hipError_t launch_label_fill(hipStream_t st, const int* d_T, const int32_t* d_map_off, int n_maps, int L, unsigned char* d_out0,
                             const long long* d_out_off, int M, int N, bool transposed);
hipError_t launch_label_thick(hipStream_t st, const int* d_T, const int32_t* d_map_off, int n_maps, int M, int N, int L, int* d_thick);
// d_xy [n_used][n_theta][2] from the converged fits; d_cxy: cx [n_centres] | cy [n_centres]
hipError_t launch_label_vertices(hipStream_t st, const LabelEdge* d_le, int n_used, const EdgeDev* d_edges, const long long* d_r0_fit,
                                 const double* d_cxy, int n_centres, const double* d_cos, const double* d_sin, double r0, double dr, int n_theta,
                                 double* d_xy);
// contour u: d_n_vert[u] vertices from pair d_vert_off[u] of d_xy on; n_vert_max: the most of any
hipError_t launch_label_fill_xy(hipStream_t st, const double* d_xy, const long long* d_vert_off, const int32_t* d_n_vert,
                                const int32_t* d_map_off, int n_maps, int n_vert_max, unsigned char* d_out0, const long long* d_out_off, int Ms,
                                int Ns);
hipError_t launch_score_kde_fused_tail(hipStream_t st, EdgeDev* d_edges, int B, const BatchDims& bd);

// converged fit on the device (gpet_lbfgsb.hip): training sets + start points, L-BFGS-B state machines, best restart
// bounds of theta = log(constant, length_scale, noise_level) and the number of start points per edge
struct LbCfg {
  double lo[3], hi[3];
  int nstart;
};
LbCfg lb_default_cfg();  // the tracer's converged fit: gpet.py:246-248, theta0 + 12 restarts
size_t lb_prob_bytes();
// host copy of P problem records -> out[P][10] = x[3], f, g[3], iter, nfev, why (gpet_final_problems; LbProb stays private)
void lb_unpack_records(const void* h_probs, int P, double* out);
hipError_t launch_fin_prepare(hipStream_t st, EdgeDev* d_edges, int B, const unsigned int* d_seeds, double* d_starts,
                              double* d_scratch, int scratch_stride, int n_cap);
hipError_t launch_lb_init(hipStream_t st, void* d_probs, int P, const double* d_starts, int* slot_edge, double* slot_theta,
                          int* slot_src, const LbCfg& cfg);
hipError_t launch_lb_advance(hipStream_t st, void* d_probs, int n_upper, const int* cur_count, const int* slot_src,
                             const double* d_f, const double* d_g, int* next_count, int* next_edge, double* next_theta,
                             int* next_src, const LbCfg& cfg);
hipError_t launch_lb_pick(hipStream_t st, EdgeDev* d_edges, int B, const void* d_probs, double* d_theta_out, int nstart);
// one workgroup per (edge, restart) problem from start to optimum (gpet_kernels.hip: k_lml16_fit); applies to training
// sets the matrix-core objective serves (<= 108 points on a lattice with fewer than lag_cap lags)
bool lml16_fit_applies(int n_max, int lag_cap);
hipError_t launch_lml16_fit(hipStream_t st, EdgeDev* d_edges, void* d_probs, int P, const LbCfg& cfg, int lag_cap, int max_evals,
                            int* d_counters);

// objective for more than 250 training points: blocked HBM kernels over a scratch table of virtual edges
size_t lmlbig_scratch_doubles(int ncap_v);
hipError_t launch_lml_big(hipStream_t st, EdgeDev* d_edges, int P, int n_max, const int* d_edge_of, const double* d_theta,
                          double* d_f, double* d_g, void* d_vedges, void* d_vsc, double* d_scratch, double* d_part,
                          int ncap_v);
// d_count (may be null): device word with the true number of problems (workgroups beyond it return at once);
// lag_cap > 0: every training set of the launch sits on a lattice (fin_par[9..10]) with fewer than lag_cap points -- the
// matrix-core kernel k_lml16 and its correlation tables apply (n_max <= 108); 0: the vector kernels
hipError_t launch_lml(hipStream_t st, EdgeDev* d_edges, int P, int n_max, const int* d_edge_of, const double* d_theta,
                      double* d_f, double* d_g, const int* d_count, int lag_cap);

}  // namespace gpet
