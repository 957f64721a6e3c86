// What the launchers of the eigen-factor stage decide (launch_factor, launch_jacobi_small: gpet_k_launch.inc; launch_pchol_multi,
// launch_factor_big: gpet_eig.hip), as plain data: the batch's dimensions in, which kernel variant runs, its grid, its workgroup and its
// dynamic LDS out.  No HIP and no options (option values, the CU count and the occupancy come in as integers), so the host compiler
// alone builds it (tests/test_factor_plan.py).  Every rule is written here ONCE.  The layout functions are what a kernel and its
// launcher must agree on -- one that disagrees writes outside the LDS allocation -- so both call them: the kernels with the edge's
// own rank or width, the plans with the batch's largest.
#pragma once
#include <stddef.h>

#include "gpet_iter_plan.h"  // BatchDims, LDS_DYN_MAX, FACTOR_LDS_CAP, PCH_ONE_WG_MAX, PCX_COLS (gpet_batch_plan.h), cdiv, Grid3

#if defined(__HIPCC__)
#define GPET_FACTOR_HD __host__ __device__
#else
#define GPET_FACTOR_HD
#endif

namespace gpet {

// ---- tile and capacity constants ------------------------------------------------------------------------------------------------
constexpr int PCH_R = 96;          // rows k_pchol_reg keeps in registers
constexpr int JS_NT = 512;         // workgroup of k_jacobi_seat and of k_jacobi_ahead without a log
constexpr int JS_LOG_SWEEPS = 40;  // sweeps a rotation log holds (= the sweep limit of the kernel)
constexpr int JA_NT_LOG = 512;     // k_jacobi_ahead, rotation-log form: seven worker waves (two blocks per thread up to rank 82, else three) + the parameter wave
constexpr int JA_RR = 6;           // k_jacobi_ahead<2, false, JA_RR>: 7 JA_RR rows of the eigenvectors in the worker waves' registers
// (PCX_COLS = 32 columns per workgroup of the multi-workgroup pivoted Cholesky: gpet_batch_plan.h, which sizes pcx_cand by it)
constexpr int PCB_NB = 16;         // pivots per launch of its blocked form (k_pcb_block)
constexpr int PCB_NW_MAX = 64;     // workgroups per edge up to which k_pcb_block selects candidates (one wave looks at all of them)
constexpr int OJ_B = 8;            // rows per block of the one-sided Jacobi
constexpr int OJ_M = 16;           // rows of a pair of blocks: one workgroup
constexpr int OJ_ARGS_MAXB = 8;    // batches up to this size get their per-edge pointers in the kernel arguments
constexpr int OJ_STAGE_MAX = 1024;  // widest edge whose 16-row panel (16 x Lg doubles) is staged in LDS
constexpr int OJ_LDS_ATTR = 136 * 1024;  // dynamic LDS the staged any-rank kernels are allowed (k_oj_round<true, .>, k_oj_persist)
constexpr int OJ_HALF_LD = 514;    // row stride of a panel staged one 512-column half at a time
constexpr int OJ_HALF_MIN = 512;   // ... for even widths above this
// LDS staging costs a workgroup a whole CU (131 KB): k_oj_round stages while a round's workgroups (pairs x edges) fit the 256 CUs of an
// MI355X side by side (one edge: 64 pairs; measured 54 vs 61 ms per factor); a bigger batch runs two register-fed workgroups per CU
// instead (8 edges: 85 vs 106 ms).  A measured constant, not the device's CU count.
constexpr int OJ_ROUND_STAGE_SLOTS = 256;
constexpr int OJ_PERSIST_SLOTS_PER_WG = 4;  // k_oj_persist up to this many pair slots per resident workgroup and round

// ---- layouts shared by the kernels and the plans ----------------------------------------------------------------------------------
// LDS Jacobi (k_jacobi_seat, k_jacobi_ahead): the rank padded to an even number m of players, the 2 x 2 blocks of the upper triangle,
// four planes of them (stride nbp)
GPET_FACTOR_HD constexpr int jac_players(int rank) { return (rank + 1) & ~1; }
GPET_FACTOR_HD constexpr int jac_blocks(int m) { return (m >> 1) * ((m >> 1) + 1) / 2; }
GPET_FACTOR_HD constexpr int jac_plane_stride(int nblk) { return (nblk + 1) & ~1; }
// k_jacobi_ahead keeps two copies of the planes, each with a dump slot
GPET_FACTOR_HD constexpr int jac_ahead_copy_stride(int nbp) { return 4 * nbp + 2; }
// rows of the eigenvectors in the worker waves' registers (RR per wave, seven waves; even, at most all m)
GPET_FACTOR_HD constexpr int jac_reg_rows(int rr, int m) { return (7 * rr < m ? 7 * rr : m) & ~1; }
// doubles of dynamic LDS: the planes, then W [m - nreg][m] (the log forms of k_jacobi_ahead keep no W)
GPET_FACTOR_HD constexpr size_t jac_seat_lds_doubles(int m) { return 4 * (size_t)jac_plane_stride(jac_blocks(m)) + (size_t)m * m; }
GPET_FACTOR_HD constexpr size_t jac_ahead_lds_doubles(int m, bool log, int rr) {
  return 2 * (size_t)jac_ahead_copy_stride(jac_plane_stride(jac_blocks(m))) + (log ? 0 : (size_t)(m - jac_reg_rows(rr, m)) * m);
}
// k_jacobi_prerot<NT>: W and C as [mp][ld], mp = 16 NT, row stride = 16 mod 32
GPET_FACTOR_HD constexpr int prerot_ld(int mp) { return (mp % 32 == 16) ? mp : mp + 16; }
GPET_FACTOR_HD constexpr size_t prerot_lds_doubles(int nt) { return (size_t)2 * (16 * nt) * prerot_ld(16 * nt); }
// k_oj_round / k_oj_persist: row stride of the staged [OJ_M][ldx] panel
GPET_FACTOR_HD constexpr int oj_panel_stride(int Lg, bool half_stage) { return half_stage ? OJ_HALF_LD : ((Lg + 31) & ~31) + 2; }

// ---- multi-workgroup pivoted Cholesky (k_pcb_* blocked, k_pcx_* one pivot per launch) ------------------------------------------------
struct PcholMultiPlan {
  bool blocked;   // k_pcb_init (64 threads), nblocks x k_pcb_block, k_pcb_fin; else k_pcx_init (256), steps x k_pcx_step, k_pcx_fin
  int nw;         // workgroups per edge: grid (nw, B), 256 threads
  int steps;      // pivots at most
  int nblocks;    // blocked: launches of k_pcb_block (a block that finds the factorisation finished returns at once)
  double accept;  // blocked: a block ends where the next pivot falls under this fraction of the block's first
};

// ---- pivoted Cholesky of the LDS path (capacity <= FACTOR_LDS_CAP) -------------------------------------------------------------------
// A WIDE edge of low rank (BASELINE config 3: 2 048 columns) over the GPU instead of k_pchol's one workgroup (1.2 ms of that factor's
// 2.2: every pivot streams all previous rows through one CU).  The pivot ORDER matters here: these factors end at the rank CAP, and the
// blocked candidate selection of the any-rank path, which is free to take pivots out of order when every pivot will be taken anyway,
// leaves 1e-7 of the largest entry at rank 96 where the greedy order leaves 1e-12 (measured).  Option pchol_multi: 2 = k_pcb_block with
// a block ending where the next pivot falls under a tenth of the block's first (the global maximum): the order stays within a
// constant of the greedy one -- every block takes at least its first candidate, so `steps` blocks always suffice; 1 = one pivot per
// launch in the greedy order itself; 0 = k_pchol.  The rows' last bits differ from k_pchol's either way, so the prior eigenbasis of the
// structured loop (single_wg: its bits every trace inherits) and edges of up to PCH_ONE_WG_MAX columns stay on k_pchol.
enum class PcholForm { reg, one_wg, multi };
struct PcholPlan {
  PcholForm form;  // k_pchol_reg (512 threads) | k_pchol (threads, lds) | multi
  int threads;
  size_t lds;
  PcholMultiPlan multi;
};
inline PcholPlan pchol_plan(const BatchDims& bd, int pchol_multi, bool single_wg) {
  PcholPlan p = {};
  const int nw = cdiv(bd.Lg, PCX_COLS);
  if (!single_wg && bd.Lg > PCH_ONE_WG_MAX && bd.r_cap <= FACTOR_LDS_CAP && pchol_multi != 0 && (pchol_multi == 1 || nw <= PCB_NW_MAX)) {
    const int steps = bd.r_cap < bd.Lg ? bd.r_cap : bd.Lg;
    p.form = PcholForm::multi;
    p.multi = {pchol_multi != 1, nw, steps, steps, 0.1};
  } else if (bd.Lg <= 512 && bd.r_cap <= PCH_R) {
    p.form = PcholForm::reg;
    p.threads = 512;
  } else {
    p.form = PcholForm::one_wg;
    p.threads = bd.Lg > 512 ? 1024 : (bd.Lg > 256 ? 512 : 256);
    p.lds = (size_t)(bd.Lg + bd.r_cap) * sizeof(double);
  }
  return p;
}
// the stage around it: k_gram (16 x 16 tiles of the Gram matrix of the rows, 256 threads), the LDS Jacobi (jacobi_small_plan with
// rank_max = r_cap), k_factor_rows (a workgroup of 256 per row, the row's eigenvector in LDS)
struct FactorLdsPlan {
  PcholPlan pchol;
  Grid3 gram, rows;
  size_t rows_lds;
};
inline FactorLdsPlan factor_lds_plan(const BatchDims& bd, int B, int pchol_multi, bool single_wg) {
  const int t = cdiv(bd.r_cap, 16);
  return {pchol_plan(bd, pchol_multi, single_wg), {t, t, B}, {bd.r_cap, B, 1}, (size_t)bd.r_cap * sizeof(double)};
}

// ---- LDS Jacobi ---------------------------------------------------------------------------------------------------------------------
// rank_max: the largest rank an edge of this launch can have.  Blocks per thread NU: two while the blocks fit two per worker
// (k_jacobi_seat: all NT threads; k_jacobi_ahead: NT - 64, the parameter wave apart), else three -- the kernels' guard is
// nblk <= NU * workers.  k_jacobi_ahead without a log: two blocks per thread keep the last 7 x JA_RR components of the eigenvectors in
// the worker waves' registers; three (ranks above 82) have no registers to spare.
// Warm start (structured loop only -- scaled_out: there the matrix of an iteration is a small change of the last one's):
// k_jacobi_prerot<NT>, NT = ceil(rank_max / 16) in 2 .. 6.  NT = 6 (ranks above 80) would need 172 032 bytes, more than LDS_DYN_MAX
// and than a CU has: such a batch starts cold, exactly as jacobi_warm = 0 does (`warm` is what the Jacobi kernels are passed).
struct JacobiSmallPlan {
  int warm;
  int prerot_nt;  // 0: no pre-rotation; else k_jacobi_prerot<prerot_nt>, grid (1, B), a wave per 16-column tile
  int prerot_threads;
  size_t prerot_lds;
  bool ahead;  // k_jacobi_ahead<nu, log, rr, threads> | k_jacobi_seat<nu, log>: grid (1, B)
  int nu, rr, threads;
  bool log;  // rotations logged, the eigenvectors by k_jacobi_wpass (256 threads)
  size_t lds;
  Grid3 wpass;
};
inline JacobiSmallPlan jacobi_small_plan(int B, int rank_max, bool scaled_out, bool logw, int jacobi_variant, int jacobi_warm) {
  JacobiSmallPlan p = {};
  const int m = jac_players(rank_max), nblk = jac_blocks(m);
  if (scaled_out && jacobi_warm) {
    const int nt = cdiv(rank_max, 16);
    p.prerot_nt = nt < 2 ? 2 : (nt > 6 ? 6 : nt);
    p.prerot_lds = prerot_lds_doubles(p.prerot_nt) * sizeof(double);
    if (p.prerot_lds > (size_t)LDS_DYN_MAX) p.prerot_nt = 0, p.prerot_lds = 0;
    p.prerot_threads = 64 * p.prerot_nt;
    p.warm = p.prerot_nt ? jacobi_warm : 0;
  }
  p.ahead = jacobi_variant != 0;
  p.log = logw;
  p.threads = p.ahead && logw ? JA_NT_LOG : JS_NT;
  p.nu = nblk <= 2 * (p.ahead ? p.threads - 64 : p.threads) ? 2 : 3;
  p.rr = p.ahead && !logw && p.nu == 2 ? JA_RR : 0;
  p.lds = (p.ahead ? jac_ahead_lds_doubles(m, logw, p.rr) : jac_seat_lds_doubles(m)) * sizeof(double);
  if (logw) p.wpass = {cdiv(rank_max, 4), B, 1};
  return p;
}

// ---- any-rank factor (capacity > FACTOR_LDS_CAP) ---------------------------------------------------------------------------------------
struct FactorBigOpts {  // the options of these names
  int oj_args, pcx_one_pivot, oj_warm, oj_stage, oj_half_stage, oj_persist;
};
// What of the panel staging does not depend on the occupancy (which the launcher asks for persist_lds).
// k_oj_persist with the panel staged one 512-column half at a time (even widths above 512 columns): 66 KB instead of 131 KB, two
// workgroups per CU -- a batch of eight 1 024-column edges (config 5's chains) holds all its 512 pair slots at once.  Automatic
// (oj_half_stage = -1) only where the whole panels cannot all be resident, one workgroup per CU: a single 1 024-column edge, 64 slots,
// is 3-4 % slower with the second read of the first half: 11.6 against 11.2 ms warm; eight edges, 512 slots: 20.9 against 22.6 ms --
// the rounds of a big batch are bound by what the 64 MB of panels pull from beyond the L2s, not by occupancy
// (profiles/r06_oj_half_stage.txt)
struct OjStagePlan {
  int nblk;            // blocks of OJ_B rows, even: nblk / 2 pair slots per edge and round
  bool lds_ok;         // the panel may be staged at all
  bool round_staged;   // k_oj_round<true, .>
  bool half_stage;     // k_oj_persist: half panels
  size_t stage_lds, persist_lds;
};
inline OjStagePlan oj_stage_plan(const BatchDims& bd, int B, const FactorBigOpts& o, int n_cus) {
  OjStagePlan s = {};
  const int steps = bd.r_cap < bd.Lg ? bd.r_cap : bd.Lg;
  s.nblk = 2 * cdiv(steps, 2 * OJ_B);
  const long long slots = (long long)(s.nblk / 2) * B;
  s.lds_ok = bd.Lg <= OJ_STAGE_MAX && o.oj_stage;
  s.round_staged = s.lds_ok && slots <= OJ_ROUND_STAGE_SLOTS;
  s.half_stage = bd.lg_even && bd.Lg > OJ_HALF_MIN && (o.oj_half_stage > 0 || (o.oj_half_stage < 0 && slots > n_cus));
  s.stage_lds = (size_t)OJ_M * oj_panel_stride(bd.Lg, false) * sizeof(double);
  s.persist_lds = (size_t)OJ_M * oj_panel_stride(bd.Lg, s.half_stage) * sizeof(double);
  return s;
}
// The whole factorisation is enqueued; nothing is read back: a fixed budget of pivot steps and sweeps is launched and the kernels turn
// into no-ops once the device-side tests (tolerance reached / converged) have fired.
struct FactorBigPlan {
  bool use_args;  // small batches: the per-edge pointers travel in the kernel arguments
  int steps;      // rows of G at most
  PcholMultiPlan pchol;
  // the warm start's launches (k_ojw_*: between the blocked Cholesky's init kernel and its blocks; only where every edge keeps all
  // its directions): 64 x 64 tiles of an n x n matrix, the Cholesky of it in steps of 64 columns (ojw_below)
  bool warm;
  int warm_n;
  Grid3 warm_begin, warm_tiles;
  OjStagePlan stage;
  // staged: the rounds and sweeps in ONE launch (k_oj_persist: pair slots by ticket -- no residency requirement, so the grid is sized to
  // what the device holds at once and a workgroup serves several slots per round when the batch has more slots than that; beyond
  // OJ_PERSIST_SLOTS_PER_WG the round launches' two register-fed workgroups per CU win); else nblk - 1 launches of k_oj_round + k_oj_check
  // per sweep
  bool persist;
  Grid3 persist_grid;  // (workgroups per edge, B)
  Grid3 round_grid;    // k_oj_round (k_oj_check: one wave per edge)
  Grid3 norms, order, rows;  // k_oj_norms, k_oj_order, k_oj_rows (256 threads each)
};
inline int ojw_below(int n, int k0) { return cdiv(n - k0 - 64, 64); }  // 64-row tiles below the diagonal tile at column k0
// have_h_edges: the caller has a host copy of the edge table; stage: oj_stage_plan of the same batch; resident: workgroups of
// k_oj_persist the device holds at once with stage.persist_lds of dynamic LDS (occupancy x CUs; looked at only where stage.lds_ok and
// oj_persist)
inline FactorBigPlan factor_big_plan(const BatchDims& bd, int B, bool have_h_edges, const FactorBigOpts& o, const OjStagePlan& stage,
                                     int resident) {
  FactorBigPlan p = {};
  p.use_args = have_h_edges && B <= OJ_ARGS_MAXB && o.oj_args;
  p.steps = bd.r_cap < bd.Lg ? bd.r_cap : bd.Lg;
  const int nw = cdiv(bd.Lg, PCX_COLS);
  // blocks of up to PCB_NB pivots (one candidate per 32-column workgroup: narrow edges offer fewer); rejected candidates cost extra
  // blocks, so the budget is generous
  const int per_block = nw < PCB_NB ? nw : PCB_NB;
  p.pchol = {nw <= PCB_NW_MAX && !o.pcx_one_pivot, nw, p.steps, 2 * cdiv(p.steps, per_block) + 8, 0.0};
  p.warm = p.pchol.blocked && o.oj_warm && bd.Lg <= bd.r_cap;
  p.warm_n = bd.Lg;
  p.warm_begin = {cdiv(bd.Lg, 4), B, 1};
  p.warm_tiles = {cdiv(bd.Lg, 64), cdiv(bd.Lg, 64), B};
  p.stage = stage;
  const int pairs = p.stage.nblk / 2;
  const long long slots = (long long)pairs * B;
  p.persist = p.stage.lds_ok && o.oj_persist && slots <= (long long)OJ_PERSIST_SLOTS_PER_WG * resident;
  p.persist_grid = {slots > resident ? (resident / B > 0 ? resident / B : 1) : pairs, B, 1};
  p.round_grid = {pairs, B, 1};
  p.norms = {cdiv(p.steps, 4), B, 1};
  p.order = {cdiv(p.steps, 256), B, 1};
  p.rows = {p.steps, B, 1};
  return p;
}

}  // namespace gpet
