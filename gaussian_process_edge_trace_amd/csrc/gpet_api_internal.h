// Internals shared by the translation units of the C ABI (include/gpet_hip.h): contexts and batches as the library sees them,
// the error / wait helpers, and the few host-side helpers more than one unit needs.  Host-side plumbing only: all arithmetic
// lives in the kernels (gpet_kernels.hip, gpet_eig.hip, gpet_lbfgsb.hip, gpet_rng.hip).
//   gpet_api_ctx.hip     contexts, options, timers, a1 for one image (gpet_grad_image, gpet_normalise_f32), the shared helpers'
//                        definitions (waits, errors, lattice, the context's scratch)
//   gpet_api_frames.hip  a1 for stacks of raw frames: RawSource and its refusals (check_raw_source), conv_frames, the entry points
//                        on a context (gpet_grad_images*, gpet_denoise_images) and the stages of their own in front of them
//                        (gpet_nlmeans_images, gpet_wavelet_images, gpet_tvb_images)
//   gpet_conv_plan.h     what a1 decides before a launch, as plain data (no HIP): flipped taps and origin, pixel types, grid and LDS
//                        bytes, the chunks host frames go up in
//   gpet_denoise_plan.h  what the denoising stage in front of a1 decides (no HIP): spec and validation, window origin and rank, Gaussian
//                        radius and taps, workspace per image, chunk sizes
//   gpet_api_batch.hip   batches: creation (a short driver over gpet_batch_plan.h), destruction, images, observations, reset,
//                        reads / writes
//   gpet_batch_plan.h    what batch creation decides, as plain data (no HIP): edge parameters -> EdgeDev fields and BatchDims, the
//                        arena's layout (layout_batch: the one place where buffer sizes live; Carver), structured-path planning
//   gpet_state_plan.h    what a batch knows about the validity of what it holds, as plain data (no HIP): the facts, the events, the
//                        one table of what every call needs, makes and drops
//   gpet_api_stages.hip  the per-stage entry points (a2-a7, f1) and gpet_profile_stage
//   gpet_api_final.hip   the converged fit (f2): objective, device L-BFGS-B, posterior at the optimum
//   gpet_api_loop.hip    the device-resident loop (a8): gpet_trace_iterate, a short driver over its pieces (compaction, one function
//                        per normals mode, the kernel chain of an iteration, the end of a group); the dispatch of the normal
//                        generators (normals_auto, launch_normals_seq)
//   gpet_loop_plan.h     the loop's scheduling decisions as plain data (no HIP): options -> LoopPlan, the chunked head, group sizes
//   gpet_zstore_plan.h   the normals store's decisions as plain data (no HIP): its size from the free memory and two options, the tag of
//                        a slot, which edges of a group miss
//   gpet_api_comm.hip    multi-GPU helpers on RCCL (8e): communicator, broadcast of the gradient image, gather of the traces
//                        and of the result records
//   gpet_api_results.hip the finished result record of every edge (k_finish_results): gpet_result_bytes, gpet_batch_results
//   gpet_api_history.hip the iteration history (k_history): gpet_batch_set_history, gpet_history_layout, gpet_batch_history,
//                        gpet_history_record
//   gpet_history_plan.h  the history's record layout and storage size as plain data (no HIP)
//   gpet_api_ensemble.hip seed ensembles: gpet_batch_final_costs, gpet_ensemble_bytes, gpet_batch_ensemble
//   gpet_ensemble_plan.h the layout of an ensemble's buffer, the validation of its arguments, member tables and tile width (no HIP)
//                        and, for sequences, gpet_batch_ensemble_keep / _kept, gpet_batch_warm_start_groups / _from
//   gpet_api_label.hip   label maps: gpet_label_maps[_xy], gpet_batch_label_maps[_xy], gpet_label_thick_count
//   gpet_label_plan.h    the two rasterisation rules, their refusals, the fill kernels' launch shapes (no HIP)
//   gpet_api_metrics.hip denoise quality metrics: gpet_metrics_images
//   gpet_metrics_plan.h  the four figures' arithmetic, the one summation order, the method of the counts, refusals, launch shapes (no HIP)
//   gpet_api_init.hip    endpoint tracking: gpet_batch_init_follow, gpet_batch_set_init, gpet_batch_init_xy
//   gpet_init_plan.h     the rule that moves an init point, its refusals (no HIP)
//   gpet_warm_plan.h     the source of every edge's warm start (medoid, best cost, consensus, another edge, none), the refusals, the
//                        kept ensemble's size (no HIP)
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <string>
#include <algorithm>
#include <vector>

#include "gpet_kernels.h"
#include "gpet_options.h"
#include "gpet_state_plan.h"

using namespace gpet;

struct gpet_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  char* scratch = nullptr;  // device scratch of the a1 entry points (gpet_grad_image / gpet_normalise_f32), grown on demand
  size_t scratch_bytes = 0;
  // raw frames (conv_frames): the device staging of host frames with the denoising workspace of a chunk behind them, the device
  // block of pointer tables / taps / slot reset values with its host copy; grown on demand, freed with the context
  char *raw_dev = nullptr, *raw_tab = nullptr;
  size_t raw_dev_bytes = 0, raw_tab_bytes = 0;
  std::vector<char> h_raw_tab;
  // the stages in front of the raw-frame path (pre_stage): the workspace of a chunk's frames -- the wavelet stage's coefficient
  // pyramids (gpet_wavelet_plan.h), the split-Bregman stage's skewed arrays (gpet_tvb_plan.h).  ONE block for all stages, as large
  // as the largest chunk so far: the stages share the context's one stream, and the stream is waited for before the block is
  // replaced, so a stage finds no other stage's work in it; grown on demand
  char* pre_ws = nullptr;
  size_t pre_ws_bytes = 0;
  struct LabelScratch* lab = nullptr;  // label maps on injected rows / vertices (gpet_api_label.hip): made on first use
  std::string err;
};

// what a banded batch owns in addition (gpet_band_plan.h): the full-frame gradient images, one per (frame, kernel) pair, and the int64
// tables the band kernels read.  H == 0: the batch has no bands, holds nothing of this and enqueues nothing for it
struct BandState {
  int H = 0, M = 0;                  // rows of a band, rows of the full frame (the batch's own image shape is (H, N))
  int n_pair = 0, n_init_max = 0;
  std::vector<int32_t> pair_of;      // [B] the full-frame image of every edge
  float* G = nullptr;                // [n_pair][M * N]
  const float** d_G_of = nullptr;    // [B] device table: G + pair_of[e] * M * N
  long long* tab = nullptr;          // band_tables(B, n_init_max), one allocation; the pointers below lie in it
  long long *r0 = nullptr, *pend = nullptr, *fit = nullptr, *lohi = nullptr, *init = nullptr;
  std::vector<long long> h_tab;      // the host copy the tables were uploaded from: (i_lo, i_hi) and the full-frame inits stay valid
  std::vector<long long> h_r0;       // staging of gpet_batch_band_set (kept alive for the asynchronous copy)
  bool pending = false;              // r0_pend holds bands the slots have not moved to yet (gpet_batch_band_place / _set)
  bool moved = false;                // gpet_batch_init_follow has rewritten (i_lo, i_hi) and the inits on the device since h_tab was current
};

// The normals store of a batch: one allocation OUTSIDE the arena (edge e owns iters slots of slot_bytes from e * iters * slot_bytes;
// EdgeDev::Zs / zs_iters), the tags on the HOST -- the host decides what is generated -- and the tables of the launches that
// generate for some edges only.  iters == 0: no store (never asked for, refused by the budget, or the allocation failed): the
// batch then runs on its ring alone, as every batch did before the store existed.
struct ZGenLaunch {      // a generator launch of the loop whose effect the host does not know yet (Loop::end_group settles it)
  int from, n;           // iterations [from, from + n)
  bool store;            // into store slots: their tags are set once it is certain the edge generated
  std::vector<int> idx;  // the batch's edges it ran for (empty: all of them)
  bool keep = false;     // into ring slots, with ring tags kept: the slots get their tags when the launch is settled (zring_settle)
  bool certain = false;  // ... and every stream of it was generated, whatever the edge's state afterwards
};
struct ZStore {
  bool decided = false;
  double* mem = nullptr;
  int iters = 0;
  size_t slot_bytes = 0, bytes = 0, alloc_bytes = 0;  // alloc_bytes >= bytes: a block taken over from a destroyed batch may be larger
  std::vector<uint64_t> tags;          // [B][iters]; 0: empty
  // ring tags (gpet_zstore_plan.h): what the ring slot of iteration k >= iters, k % ring, holds.  No device memory: made by the
  // batch's first gpet_trace_iterate with or without a store; ring == 0: none yet, or the edges' rings differ in length
  std::vector<uint64_t> rtags;         // [B][ring]; 0: empty
  int ring = 0;
  long long generated = 0;             // (edge, iteration) streams the loop generated for iterations the edge went on to run (gpet_batch_info)
  long long drawn = 0;                 // (edge, iteration) streams the loop's STORE launches generated, exactly: they always generate
  std::vector<ZGenLaunch> pending;
  // compacted edge / seed tables of the launches that generate for the edges with a miss: segments of one device block, taken in
  // order and reused when the same edges miss again; the host copies stay untouched while a copy may still read them
  EdgeDev* d_edges = nullptr;
  unsigned int* d_seeds = nullptr;
  std::vector<EdgeDev> h_edges;
  std::vector<unsigned int> h_seeds;
  size_t cap = 0, used = 0;
  std::vector<int> last_idx;           // the edges of the segment taken last, at last_off (emptied by every gpet_trace_iterate)
  size_t last_off = 0;
  hipStream_t last_stream = nullptr;
  gpet_scalars* d_running = nullptr;   // a record that says "running" (done = 0, status OK): what the entries of those tables read
};
// gpet_api_loop.hip: the store of a batch being destroyed goes to the process's pool or back to the device; the pool emptied
void zstore_release(gpet_batch* b);
void zstore_pool_drain();
// empties every tag (what the slots would hold has changed, or may have been overwritten: gpet_batch_set_rng, the stage generators)
static inline void zstore_clear_tags(ZStore& z) {
  std::fill(z.tags.begin(), z.tags.end(), (uint64_t)0);
  std::fill(z.rtags.begin(), z.rtags.end(), (uint64_t)0);
}
// the tag of the slot z_slot names for iteration `iter` of edge e, in the store or in the ring (nullptr: that slot has no tag)
static inline uint64_t* zstore_tag_at(ZStore& z, int e, int iter) {
  if (iter < 0) return nullptr;
  if (iter < z.iters) return &z.tags[(size_t)e * z.iters + iter];
  return z.ring > 0 ? &z.rtags[(size_t)e * z.ring + iter % z.ring] : nullptr;
}

struct gpet_batch {
  gpet_ctx* ctx = nullptr;
  int B = 0;
  BatchDims bd{};
  std::vector<EdgeDev> h_edges;
  std::vector<gpet_params> params;
  EdgeDev* d_edges = nullptr;
  EdgeDev* d_edges_act = nullptr;      // the edges still running, compacted (gpet_trace_iterate)
  unsigned int* d_seeds_act = nullptr;
  std::vector<EdgeDev> h_edges_act;
  std::vector<unsigned int> h_seeds_act;
  std::vector<int> h_idx_act;          // their indices in the batch
  char* arena = nullptr;
  size_t arena_bytes = 0;
  unsigned int* d_seeds = nullptr;
  std::vector<unsigned int> h_seeds_dev;  // what d_seeds was last written from (the stage generators' tags)
  gpet_scalars* d_scalars = nullptr;   // [B] contiguous: one copy reads every edge's state
  double* d_fin_out = nullptr;         // [B][2][Lg_max] contiguous results of the converged fits
  double* d_fin_par = nullptr;         // [B][12] contiguous hyper-parameters / transforms of the converged fits
  long long* d_obs = nullptr;          // [B][obs_cap_max][2] contiguous observations: one copy reads them all
  long long* d_init = nullptr;         // [B][n_init_max][2] contiguous init points: one copy writes them all
  int n_init_max = 0;
  std::vector<long long> h_init;       // what d_init was last written from on the host: the x stay valid (no call moves them), the rows
                                       // are stale after gpet_batch_init_follow; also the staging of gpet_batch_set_init
  std::vector<gpet_scalars> h_scalars;
  std::vector<int> h_nobs_prev;        // observations per edge at the last group boundary of the loop: batches up to 64 edges size
                                       // the next group by their growth (next_group, gpet_loop_plan.h)
  int rng_mode = 0;                    // 0: MT19937 + polar method = numpy's RandomState stream; 1: Philox4x32-10 + Box-Muller (opt-in)
  hipStream_t side = nullptr;          // RNG stream: normals of upcoming iterations run ahead of the loop
  double* d_fin_stage = nullptr;       // staging of the converged fits' training sets (x | y | w blocks)
  int* d_fin_n = nullptr;
  size_t fin_stage_cap = 0;
  hipStream_t fit = nullptr;           // high-priority stream of the final-fit objective launches: they are tiny and
                                       // latency-bound, and run while OTHER batches' loops keep the GPU busy
  hipEvent_t ev_norm[16] = {};
  hipEvent_t ev_gemm[16] = {};         // sample GEMM of iteration k done: ring slot k % ring may be refilled
  hipEvent_t ev_pix[16] = {};          // pixel selection of iteration k done: the `done` flags of iteration k + 1 are final
  hipEvent_t ev_main = nullptr;
  unsigned int* d_minmax = nullptr;    // [2 B]: (min, max) of every gradient image being uploaded
  std::vector<unsigned int> h_mm0;     // their reset values (kept alive for the asynchronous copy)
  float* d_raw = nullptr;  // [M*N] staging of a user gradient image before its re-normalisation (gpet.py:97)
  int share_image = 0;
  // the image map (gpet_batch_plan.h): n_img image slots, edge e reads slot image_of[e], img_rep[g] is the first edge of slot g --
  // its EdgeDev::grad / grad_kde are where image g is written and what its gradient KDE runs through.  One shared image: 1 slot;
  // one image per edge: B slots, the identity map
  int n_img = 0;
  std::vector<int32_t> image_of;
  std::vector<int> img_rep;
  bool rep_is_prefix = true;           // img_rep[g] == g for every slot: d_edges itself serves the per-slot launches
  std::vector<EdgeDev> h_img_edges;    // else: the representatives' EdgeDev, in slot order, and their device copy
  EdgeDev* d_img_edges = nullptr;
  bool structured = false;  // every edge can take the prior-eigenbasis loop path
  // converged-fit scratch (grown on demand)
  int lml_cap = 0;
  hipEvent_t ev_l0 = nullptr, ev_l1 = nullptr;  // around every LML kernel launch (gpet_lml_stats)
  double lml_ms = 0.0;
  long long lml_evals = 0;
  int lml_launches = 0;
  int* d_edge_of = nullptr;
  double *d_theta = nullptr, *d_f = nullptr, *d_g = nullptr;
  // device-resident converged fits (gpet_final_fit_all): one allocation, carved
  char* lb_mem = nullptr;
  int lb_cap_P = 0;  // problems the optimiser's workspace holds
  int lb_last_P = 0;  // problems of the last run of the optimiser (gpet_final_problems)
  void* lb_probs = nullptr;
  double *lb_starts = nullptr, *lb_scratch = nullptr, *lb_f = nullptr, *lb_g = nullptr, *lb_theta_out = nullptr;
  int* lb_slot_edge[2] = {nullptr, nullptr};
  double* lb_slot_theta[2] = {nullptr, nullptr};
  int* lb_slot_src[2] = {nullptr, nullptr};
  int* lb_count = nullptr;
  unsigned int* lb_seeds = nullptr;
  int lb_scratch_stride = 0;
  std::vector<hipEvent_t> lb_events;
  // objective for more than 250 training points (launch_lml_big): virtual-edge table + per-problem scratch
  char* big_mem = nullptr;
  int big_chunk = 0, big_ncap = 0;
  void *big_vedges = nullptr, *big_vsc = nullptr;
  double *big_scratch = nullptr, *big_part = nullptr;  // pairs around every objective launch of a converged fit (gpet_lml_stats)
  // chunked normal generator (one long MT19937 stream on many workgroups): workspace + the jump tables on the device
  void* mtj_work = nullptr;
  size_t mtj_bytes = 0;
  unsigned int* d_mtj_poly = nullptr;
  // largest lattice lag of every edge's converged-fit training set as the HOST knows it (fin_par[9..10] on the device):
  // -1 = no lattice (caller-supplied x off any grid) -> the vector objective kernels; see fin_lattice()
  std::vector<int> fin_lag;
  // what of all this is valid now, and the iterations enqueued since the last restart: changed by state_apply alone, asked through
  // state_missing alone (gpet_state_plan.h has the table of what every call needs, makes and drops)
  BatchState st;
  char* d_results = nullptr;           // device staging of gpet_batch_results into host memory (grown on demand)
  size_t results_bytes = 0;
  // seed ensembles (gpet_api_ensemble.hip): the scratch of gpet_batch_final_costs / gpet_batch_ensemble, allocations of their own made
  // on first use (nullptr: never called -- the batch then holds and enqueues nothing for them)
  struct EnsembleScratch* ens = nullptr;
  // label maps (gpet_api_label.hip): the scratch of gpet_batch_label_maps[_xy], an allocation of its own made on first use (nullptr: never
  // called -- the batch then holds and enqueues nothing for them)
  struct LabelScratch* lab = nullptr;
  // iteration history (gpet_batch_set_history): storage of its own, B regions of hist.edge_bytes (gpet_history_plan.h); hist.level == 0
  // and d_hist == nullptr: off -- the loop then enqueues nothing for it
  char* d_hist = nullptr;
  gpet_history_plan hist{};
  ZStore zst;      // the normals store (gpet_zstore_plan.h), decided and allocated by the batch's first gpet_trace_iterate
  BandState band;  // tracking bands (gpet_batch_create_banded)
  // a vertical batch (GPET_FRAMES_TRANSPOSED at creation): the caller's frames and gradient images are bd.N rows of (band.H ? band.M :
  // bd.M) pixels, and load_images writes their transposes -- everything behind it works on the batch's own (M, N) as ever
  bool transposed = false;
  OptionSet opts;  // the batch's own copy of the option table (gpet_options.h): taken at creation, gpet_batch_set_option changes it
};
// first statement of every entry point that works on a batch: its option table for the calling thread
#define GPET_BATCH_SCOPE(b) OptionScope option_scope_((b) ? &(b)->opts : nullptr)

// ---- helpers defined in gpet_api_ctx.hip ----------------------------------------------------------------------------------
hipError_t gpet_wait(hipStream_t st);  // host wait on a stream: spinning or sleeping (option blocking_sync)
int fail(gpet_ctx* ctx, int code, const char* fmt, ...);
#define HIPCHK(ctx, call)                                                                          \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return fail((ctx), GPET_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)
int fin_lattice(const double* x, int n, double* hinv);
// (device scratch of the a1 entry points in the context, grown on demand: c->scratch holds at least `bytes` afterwards)
int ctx_scratch(gpet_ctx* c, size_t bytes);
// ---- gpet_api_frames.hip --------------------------------------------------------------------------------------------------
// A stack of raw frames and what makes gradient images of them: the one description every raw-frame entry point fills in and
// conv_frames takes.  Image slot g of n_img is frame frame_of[g] convolved with kernel kernel_of[g] (gpet_conv_multi_plan.h);
// table == false: the entry point has one kernel, the two table pointers are null, and image g is frame g with kernel 0 (n_img ==
// n_frames).  n_kern == 0: no convolution, the frames are denoised alone (gpet_denoise_images).
struct RawSource {
  const void* const* frames = nullptr;  // [n_frames] host pointers, or device pointers with on_dev
  int n_frames = 0;
  int pix = 0;                          // GPET_PIX_*
  int M = 0, N = 0;                     // the frame as it lies in the caller's memory
  bool on_dev = false;                  // GPET_RAW_ON_DEVICE
  bool tr = false;                      // GPET_FRAMES_TRANSPOSED: every image is the N x M transpose of its frame's gradient image
  const DenoiseSpec* dn = nullptr;      // how the frames are denoised first (gpet_denoise_plan.h), or nullptr
  int n_kern = 0;
  const double* const* kern = nullptr;  // [n_kern] kernels of kh[k] x kw[k]
  const int32_t* kh = nullptr;
  const int32_t* kw = nullptr;
  bool table = false;                   // the caller gave a slot table: checked as one (check_conv_multi), whatever it holds
  int n_img = 0;
  const int32_t* frame_of = nullptr;
  const int32_t* kernel_of = nullptr;
};
// GPET_OK, or GPET_ERR_BAD_ARG with the reason, before anything is allocated or enqueued -- in this order: a missing argument, the
// pixel type, the kernels (one kernel: against the LDS bound of its own patch, conv[_t]_fits_lds; a table: check_conv_multi), the
// denoising spec, null frames.  conv_frames calls it itself; batch creation and the set calls call it ahead of any allocation
int check_raw_source(gpet_ctx* c, const RawSource& s);
// the table of s alone: a table slot_table_check refuses, an empty kernel, a union patch beyond the LDS (s.tr: against the bound of
// the transposed-store kernel)
int check_conv_multi(gpet_ctx* c, const RawSource& s);
// The frames of s -> normalised f32 gradient images at the device pointers dst[g], one per image slot (s.n_img), enqueued on the
// context's stream without a final wait; d_mm: device [2 s.n_img].  Every frame is staged and denoised once.  s.n_kern == 0:
// denoising alone, into the host buffers dn_out[] (iterations per image: n_iter_out).  s.tr: M, N stay the frame's as it lies, and
// every dst[g] receives the N x M transpose of its gradient image (gpet_transpose_plan.h)
int conv_frames(gpet_ctx* c, const RawSource& s, float* const* dst, unsigned int* d_mm, void* const* dn_out = nullptr,
                int32_t* n_iter_out = nullptr);
// the C ABI's gpet_denoise as the plan takes it (nullptr: no technique)
static inline DenoiseSpec dn_spec(const gpet_denoise* d) {
  DenoiseSpec s;
  if (!d) return s;
  s.technique = d->technique;
  s.size_y = d->size_y;
  s.size_x = d->size_x;
  s.mode = d->mode;
  s.sigma_y = d->sigma_y;
  s.sigma_x = d->sigma_x;
  s.truncate = d->truncate;
  s.weight = d->weight;
  s.eps = d->eps;
  s.n_iter_max = d->n_iter_max;
  return s;
}
// A RawSource as the arguments of a C entry point describe it, with what they leave no home for: the DenoiseSpec made of the
// gpet_denoise and, for an entry point with one kernel, the one-element kernel arrays.  raw points into the object, so it is filled
// where it stands and never copied.  A batch fills in M, N and, for one kernel, the frame count itself (batch_source)
struct RawSourceArgs {
  RawSource raw;
  DenoiseSpec spec;
  const double* kern1 = nullptr;
  int32_t kh1 = 0, kw1 = 0;
  RawSourceArgs() = default;
  RawSourceArgs(const RawSourceArgs&) = delete;
  RawSourceArgs& operator=(const RawSourceArgs&) = delete;
  void frames(const void* const* f, int n_frames, int pix, const gpet_denoise* dn, unsigned int flags, int M = 0, int N = 0) {
    spec = dn_spec(dn);
    raw.M = M;
    raw.N = N;
    raw.frames = f;
    raw.n_frames = n_frames;
    raw.pix = pix;
    raw.dn = dn ? &spec : nullptr;
    raw.on_dev = (flags & GPET_RAW_ON_DEVICE) != 0;
    raw.tr = (flags & GPET_FRAMES_TRANSPOSED) != 0;
  }
  // one kernel on every frame in order
  void one_kernel(const double* k, int kh, int kw) {
    kern1 = k;
    kh1 = kh;
    kw1 = kw;
    raw.n_kern = 1;
    raw.kern = &kern1;
    raw.kh = &kh1;
    raw.kw = &kw1;
    raw.n_img = raw.n_frames;
  }
  void slot_table(int n_kern, const double* const* k, const int32_t* kh, const int32_t* kw, int n_img, const int32_t* frame_of,
                  const int32_t* kernel_of) {
    raw.n_kern = n_kern;
    raw.kern = k;
    raw.kh = kh;
    raw.kw = kw;
    raw.table = true;
    raw.n_img = n_img;
    raw.frame_of = frame_of;
    raw.kernel_of = kernel_of;
  }
};
// ---- gpet_api_loop.hip ----------------------------------------------------------------------------------------------------
hipError_t launch_normals_seq(gpet_batch* b, hipStream_t st, EdgeDev* edges_l, int B_l, const unsigned int* seeds_l, int add_iter,
                              int iter_abs, int n_ahead, int z_store);
int normals_auto(gpet_batch* b, hipStream_t st, EdgeDev* edges_l, int B_l, const unsigned int* seeds_l, int add_iter, int iter_abs,
                 int n_ahead, int z_store, bool allow_chunked = true);
// ---- gpet_api_results.hip -------------------------------------------------------------------------------------------------
// bytes of one result record (gpet_result_head + its arrays) for len_cap points; 0 if len_cap is out of range
size_t result_record_bytes(int64_t len_cap);
// the records of every edge of b into DEVICE memory d_dst on the context's stream (no wait); fails (GPET_ERR_BAD_ARG, message
// set) before a converged fit of the current trace or when len_cap is below the batch's widest edge
int enqueue_results(gpet_batch* b, int64_t len_cap, void* d_dst);
// ---- gpet_api_history.hip -------------------------------------------------------------------------------------------------
// empties the iteration history of edge e (e < 0: of every edge) on the context's stream: whatever starts another trace calls it
int history_clear(gpet_batch* b, int e);
// ---- gpet_api_ensemble.hip ------------------------------------------------------------------------------------------------
// frees the scratch of the ensemble entry points (gpet_batch_destroy)
void ensemble_free(gpet_batch* b);
// ---- gpet_api_label.hip ---------------------------------------------------------------------------------------------------
// frees the scratch of the label-map entry points and clears the pointer (gpet_ctx_destroy, gpet_batch_destroy)
void label_free(struct LabelScratch*& s);
// ---- gpet_api_init.hip ----------------------------------------------------------------------------------------------------
// the host copy of a banded batch's (i_lo, i_hi) and full-frame init tables made current again after gpet_batch_init_follow (one wait;
// nothing to do when they are)
int band_refresh_host(gpet_batch* b);
// ---- gpet_api_batch.hip ---------------------------------------------------------------------------------------------------
int fetch_all_scalars(gpet_batch* b);
// the end of every warm start, after its kernel: histories, flags, the one copy of the scalars and the one wait; n_obs_out may be nullptr
int warm_start_finish(gpet_batch* b, int32_t* n_obs_out);
int check_device_status(gpet_batch* b);
// the images a caller hands over on a banded batch: n_pair of them (else the batch's image slots)
static inline int batch_source_count(const gpet_batch* b) { return b->band.H ? b->band.n_pair : b->n_img; }
// what the loop's generator stores of a sample row: the r0 (rounded to 4) leading normals a structured batch multiplies
static inline int loop_z_store(const gpet_batch* b) {
  if (!b->structured || b->bd.r0_max < 1) return 0;
  return (b->bd.r0_max + 3) & ~3;
}
