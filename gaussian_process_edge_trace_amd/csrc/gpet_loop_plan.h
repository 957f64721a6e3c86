// The scheduling decisions of the device loop (gpet_trace_iterate, gpet_api_loop.hip) as plain data: ints in, a struct out, no HIP
// and no gpet_batch, so the host compiler alone builds it (tests/test_loop_plan.py).  Options: -1 = automatic (gpet_options.h).
#pragma once
#include <math.h>

namespace gpet {

// Where and when the normals of the loop's iterations are generated.  The seeds of upcoming iterations are known (gpet.py:839),
// so the generator may run ahead of the loop, into a ring of `ring` slots.
enum class NormalsMode {
  inline_per_iteration,  // rng_inline = 1: one launch per iteration on the loop's stream (179 ms per step of 1 024 traces)
  inline_per_group,      // rng_inline = 2, the default above 64 edges: ALL iterations of a group (up to ring - 1) in one launch on the
                         // loop's stream -- it fills the GPU and runs beside nothing: 157-159 ms, against 161-162 on the side stream
  side_deep,             // rng_inline = 0, the default up to 64 edges: `look` iterations per launch on the side stream, across groups
  side_shallow,          // rng_inline = 0 with a look-ahead <= 4: one launch per iteration on the side stream, `look` ahead
};

struct LoopPlan {
  int look;         // iterations the side stream runs ahead, <= ring - 1; 0: the draws of iteration k wait for the pixels of k - 1
  bool deep;
  NormalsMode mode;
  int refill_at;    // side_deep: refill the ring when at most this many generated iterations are left ahead of the loop
  int head;         // side_deep: rng_head as resolved (-1 -> 4), before the clamps of head_iterations
  bool fused_tail;  // the score tail as one launch (the caller ands score_tail_applies in)
};

// Once per call of gpet_trace_iterate; B is the BATCH's size, not the number of edges still running.
inline LoopPlan resolve_loop_plan(int B, int ring, int rng_lookahead, int rng_inline, int rng_refill_at, int rng_head, int loop_fused_tail) {
  LoopPlan p;
  // A batch that fills the GPU is throughput-bound in the generator: an edge that finishes still gets the draws already enqueued
  // for it, so one iteration ahead wastes the least (4 ahead: 19 % of the generator's work; loop time with 1, 2, 4 ahead within
  // 1 %; 0 ahead draws nothing for finished edges but competes with the eigen-solver for the start of every iteration: 187
  // instead of 179 ms per loop of 1 024 edges, 70 instead of 56 ms at 256).  A small batch is LATENCY-bound in it -- a stream is
  // sequential, one workgroup per (edge, iteration), 2.1 ms for the 500 k normals of a 500-column edge against 0.9 ms for the rest
  // of an iteration -- so the streams of the next 8 iterations are generated side by side by one launch.
  p.deep = rng_lookahead < 0 ? B <= 64 : rng_lookahead > 4;  // (an explicit look-ahead is judged before the clamp to the ring)
  p.look = rng_lookahead < 0 ? (p.deep ? 8 : 1) : rng_lookahead;
  if (p.look > ring - 1) p.look = ring - 1;
  const int where = rng_inline >= 0 ? rng_inline : (p.deep ? 0 : 2);
  p.mode = where == 1 ? NormalsMode::inline_per_iteration : where == 2 ? NormalsMode::inline_per_group
         : p.deep ? NormalsMode::side_deep : NormalsMode::side_shallow;
  // Refilling at look / 2 = 4 (round 5) stalled the loop: four iterations of a 32-edge batch take 2.4 ms, the sequential launch that
  // refills the ring 3 ms, and by how much depended on when the launch got going: 13.5 or 16.7 ms per loop from one run to the
  // next.  At 6 the launch has a 3.6 ms lead.
  p.refill_at = rng_refill_at >= 0 ? rng_refill_at : (p.look > 2 ? p.look - 2 : p.look / 2);
  p.head = rng_head >= 0 ? rng_head : 4;
  p.fused_tail = loop_fused_tail > 0 || (loop_fused_tail < 0 && B <= 64);  // (latency chains: three launches fewer per iteration)
  return p;
}

// The HEAD of a trace of 2..32 edges (round 6): how many of the n iterations of the first refill (j = iterations generated so far,
// cur = the loop's iteration, B_l = edges still running) are generated CHUNKED, one launch per iteration.  A stream is sequential
// -- one workgroup walks 1.27 M MT19937 words in ~3 ms -- and the first iteration of a trace has nothing to hide that behind: the
// loop of a 32-edge batch stood still for ~2.5 ms before its first sample GEMM.  Chunked (jump-ahead: a launch of <= 32 streams
// is cut into chunks on many workgroups) an iteration takes ~0.7 ms.  MT19937 (rng_mode 0) only.
inline int head_iterations(const LoopPlan& p, int j, int cur, int B_l, int rng_mode, int n) {
  if (j != 0 || cur != 0 || B_l < 2 || B_l > 32 || rng_mode != 0) return 0;
  const int head = p.head < n - 1 ? p.head : n - 1;
  return head > 0 ? head : 0;
}

struct EdgeProgress {
  int done, n_obs, n_obs_prev, algo_thresh;  // n_obs_prev: at the previous group boundary (or where the trace started)
};

// Iterations of the next group, after n_it (of `group` planned) left `active` of B edges running; 0: stop.  Above 64 edges: 8, then
// 4 and -- once the first edges have finished -- 2, so that the edge table is compacted often enough.  Up to 64 edges (round 6;
// `edges` = all B of them): a latency chain, where an iteration enqueued for edges that have finished costs its ~16 empty launches
// (~90 us) and a group boundary a host round trip of about the same -- the 8 / 4 / 2 / 2 ladder spent 0.5 ms of a 6.6 ms
// single-edge loop on the two.  The observation sets grow at a steady rate (pixel_thresh or a few more per iteration, SURVEY
// appendix A), so the next group is what the slowest running edge still needs at the rate of the group just finished, at most 8:
// usually ONE more group that ends on the last iteration.
inline int next_group(int B, int group, int n_it, int active, const EdgeProgress* edges, int count) {
  if (active == 0) return 0;
  if (B > 64) return active == B ? (group < 4 ? group : 4) : 2;
  int need = 1;
  for (int e = 0; e < count; ++e) {
    if (edges[e].done) continue;
    const int got = edges[e].n_obs - edges[e].n_obs_prev, left = edges[e].algo_thresh - edges[e].n_obs;
    const double rate = got > 0 ? (double)got / (double)n_it : 1.0;
    const int est = (int)ceil((double)(left > 0 ? left : 1) / rate);
    if (est > need) need = est;
  }
  return need > 8 ? 8 : need;
}

}  // namespace gpet
