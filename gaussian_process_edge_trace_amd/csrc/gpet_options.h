// Process-wide tuning switches of the library: ONE list (GPET_OPTIONS below) behind gpet_set_option / gpet_get_option
// (include/gpet_hip.h).  An option's initial value comes from the environment variable GPET_<NAME IN CAPITALS> if it is
// set, else from the list's default; INTEGRATION.md section 3b lists them with their meaning.
#pragma once

namespace gpet {

// X(name, default, lo, hi, meaning): values outside [lo, hi] are clamped; lo == -1: -1 means "chosen automatically".
// The order is the order of gpet_option_info.
#define GPET_OPTIONS(X) \
  X(blocking_sync, -1, -1, 1, "host waits sleep on a hipEventBlockingSync event instead of spinning in hipStreamSynchronize; -1: on when WORLD_SIZE > 1 (several ranks per host share its cores)") \
  X(rng4, -1, -1, 1, "normals by the register-resident generator k_mt_normals4 (four MT19937 streams per wave): -1 = launches of >= 2048 streams, 0 = never, 1 = whenever the batch is homogeneous") \
  X(rng_chunked, -1, -1, 1, "one MT19937 stream on many workgroups by jump-ahead: -1 = launches of <= 32 streams of >= 4 chunks, 0 = never, 1 = always") \
  X(rng_lookahead, -1, -1, 15, "iterations the normals may run ahead of the device loop on the side stream; -1: 8 up to 64 edges, else 1") \
  X(rng_head, -1, -1, 8, "batches of 2..32 edges: leading iterations of a trace whose normals are generated chunked (jump-ahead, one launch per iteration) beside the sequential launch of the following ones; -1: 4, 0: off") \
  X(rng_refill_at, -1, -1, 15, "small batches: the side stream refills the normals ring when at most this many generated iterations are left ahead of the loop; -1: look-ahead - 2 (round 5: look-ahead / 2)") \
  X(loop_fused_tail, -1, -1, 1, "device loop: k_score_combine + k_topk_sort + k_kde_prep as one launch per iteration (k_score_tail, the same bits); -1: batches up to 64 edges (latency chains), 1: always where the shape allows, 0: never") \
  X(rng_inline, -1, -1, 2, "where the loop's normals are generated: 0 = side stream, 1 = one iteration per launch on the loop's stream, 2 = all iterations of a group in one launch on the loop's stream; -1: 2 above 64 edges, else 0") \
  X(fit_persistent, -1, -1, 1, "converged fits as one workgroup per (edge, restart) problem: -1 = problem sets resident at once (<= 1024), 0 = lock-step rounds, 1 = always") \
  X(lml_two_tiles_from, 600, 1, 0x3fffffff, "problems per launch from which k_lml2 (two 4x4 tiles per thread) replaces k_lml") \
  X(jacobi_variant, 1, 0, 1, "LDS Jacobi of ranks <= 96: 1 = seated, rotation parameters one round ahead, one barrier per round (k_jacobi_ahead); 0 = seated, three barriers per round (k_jacobi_seat: the cross-check)") \
  X(jacobi_warm, 1, 0, 1, "structured loop: the eigen-decomposition of an iteration starts from the previous iteration's eigenvectors (k_jacobi_prerot) instead of the identity") \
  X(jacobi_logw, 1, 0, 1, "batches that have a rotation log (<= jlog_max_b edges): eigenvectors by a separate pass over the logged rotations") \
  X(jlog_max_b, 32, 0, 4096, "largest batch that gets a rotation log (read when a batch is created): measured per step of a batch alone -- 32 edges 21.5 against 23.1 ms, 64 edges 27.1 either way, 1 024 edges slower (3.15 against 1.73 ms per launch)") \
  X(oj_warm, 1, 0, 1, "any-rank factor: rows of full rank start from the previous iteration's rows (k_ojw_*: A Sigma A^T, its Cholesky factor, one product) instead of the pivoted Cholesky (across the frames of a sequence only where the caller asks: gpet_batch_set_images with GPET_IMAGES_NEXT_FRAME)") \
  X(oj_warm_fail, 0, 0, 1, "testing: the warm start's Cholesky reports a non-positive pivot, so that the factor falls back to the pivoted Cholesky") \
  X(oj_persist, 1, 0, 1, "any-rank Jacobi: rounds and sweeps in one launch, pair slots handed out by ticket (k_oj_persist); 0: one launch per round") \
  X(oj_stage, 1, 0, 1, "any-rank Jacobi: a pair's 16 rows staged in LDS; 0: operands from global memory") \
  X(oj_half_stage, -1, -1, 1, "any-rank Jacobi (k_oj_persist), even widths above 512 columns: a pair's 16-row panel staged in LDS one 512-column half at a time (66 KB, two workgroups per CU, the first half read a second time for the row update) instead of whole (131 KB at 1 024 columns, one per CU); the same bits; -1: where a round has more pair slots than the GPU has CUs") \
  X(oj_args, 1, 0, 1, "any-rank factor: per-edge pointers of small batches in the kernel arguments; 0: through the edge table") \
  X(oj_tol_exp, 8, 4, 15, "any-rank Jacobi stops after a sweep whose pairs were all orthogonal to 10^-x relative") \
  X(oj_max_sweeps, 20, 1, 64, "sweep budget of the any-rank Jacobi") \
  X(comm_force_rccl, 0, 0, 1, "testing: gpet_comm_create builds an RCCL communicator also for a world of one (whose collectives are otherwise plain copies)") \
  X(pchol_multi, 2, 0, 2, "edges wider than 1 024 columns of rank <= 96: pivoted Cholesky over the GPU instead of one workgroup (k_pchol): 2 = blocks of pivots within a tenth of the block's first (k_pcb_block), 1 = one pivot per launch in the greedy order (k_pcx_step)") \
  X(pcx_one_pivot, 0, 0, 1, "1: multi-workgroup pivoted Cholesky one pivot per launch (cross-check of the blocked candidate selection)") \
  X(solve_mw, 1, 0, 1, "blocked fit: alpha by one workgroup per 64-row block and direction (k_chol_solve_mw); 0: one workgroup per edge") \
  X(diag_in_syrk, 1, 0, 1, "blocked fit: the trailing update's first workgroup factors the next diagonal block; 0: a launch of its own") \
  X(topk_rank, 0, 0, 1, "1: argsort of the costs by rank counting (k_topk) also where the bitonic sort applies") \
  X(struct_path, 1, 0, 1, "structured loop path (prior eigenbasis of the pixel grid) where it applies; 0: the generic kernels") \
  X(kde_variant, 1, 0, 1, "fused curve KDE of at most 128 kept curves: 1 = a tile's points stay in registers from the loads to the binning, weights once per edge, four workgroups per CU (k_kde_fused_r); 0 = points and weights staged in LDS by every tile (k_kde_fused: the cross-check, and the form of more curves)") \
  X(normals_store, -1, -1, 1, "normals store of a batch (read at its first trace): the normals of an edge's first iterations are kept, tagged with what drew them, and drawn again only where a tag does not match -- a trace repeated with the same seeds launches no generator; -1 = at least 8 iterations fit the budget (a quarter of the free device memory, outside the device's last eighth), 0 = never, 1 = whatever the budget allows") \
  X(normals_store_iters, -1, -1, 32, "iterations per edge the normals store holds: -1 = 12, 0 = a budget of zero (no store), n = n iterations or as many as the budget holds") \
  X(normals_ring_keep, -1, -1, 1, "ring tags: the slots of the normals ring are tagged like the store's, so a trace repeated with the same seeds draws a ring iteration again only where its slot was overwritten since; -1 = on where the generator runs on the loop's stream (rng_inline 1 or 2), 0 = never (every trace draws its ring iterations), 1 = as -1 (reserved)")

enum class Opt : int {
#define GPET_OPT_ENUM(name, def, lo, hi, doc) name,
  GPET_OPTIONS(GPET_OPT_ENUM)
#undef GPET_OPT_ENUM
};

struct OptionDef {
  const char* name;
  int def, lo, hi;
  const char* doc;
};

// A batch object carries its OWN copy of the table, taken when it is created (gpet_batch_create) and changed only through
// gpet_batch_set_option: every entry point that works on a batch installs that copy for the calling thread (OptionScope), so
// what a batch does never depends on what another thread sets while it runs.  Without a scope (context-level calls, batch
// creation before the copy exists) reads go to the process-wide table.
constexpr int kMaxOptions = 64;
struct OptionSet {
  int v[kMaxOptions];
};
void option_snapshot(OptionSet* out);  // the process-wide table as it is now
struct OptionScope {  // installs `s` (may be null: no change) as the calling thread's table for the scope's lifetime
  explicit OptionScope(OptionSet* s);
  ~OptionScope();
  OptionScope(const OptionScope&) = delete;
  OptionScope& operator=(const OptionScope&) = delete;
  OptionSet* prev;
  bool active;
};
// the value of option `o` in the calling thread's table (the batch's copy inside an OptionScope, else the process-wide
// table: reads see later gpet_set_option calls)
int opt(Opt o);

// By name, for the C ABI only: the index of option `name` (-1: unknown), then set / get it by that index in `s` (null: the
// process-wide table).  option_set clamps and returns the previous value.
int option_find(const char* name);
int option_set(OptionSet* s, int index, int value);
int option_get(const OptionSet* s, int index);
int option_count();
const OptionDef& option_def(int index);

}  // namespace gpet
