// The normals store of a batch (gpet_api_loop.hip) as plain data: ints in, a struct or a count out, no HIP and no gpet_batch, so
// the host compiler alone builds it (tests/test_zstore_plan.py).  Options: -1 = automatic (gpet_options.h).
//
// What the store is.  The normals of iteration k of an edge are RandomState(seed + k + 1).standard_normal((S, Lg)) (gpet.py:839):
// a function of the seed, the iteration, the rng mode and the shape -- not of the image, the observations or the kernel.  A batch
// that is traced again with the same seeds (the frames of a sequence, an ensemble's K seeds on every frame, reset() + run_loop())
// walks the same MT19937 streams again to store the same columns.  The store keeps the normals of an edge's first `store_iters`
// iterations in slots of their own (one slot = one ring slot = 8 S z_cols bytes) with a TAG per (edge, iteration) that names what
// produced the slot's contents; the loop generates only where a tag does not match, and the sample GEMM reads the slot (z_slot,
// gpet_dev.h).  Iterations from store_iters on take the ring, whose slots are tagged too (ring tags, below): where the generator
// runs on the loop's own stream, a ring iteration is drawn again only if its slot has been overwritten since -- no memory added.
#pragma once
#include <stdint.h>

namespace gpet {

constexpr int kZStoreMaxIters = 32;   // the most iterations an edge's store holds (option normals_store_iters, explicit)
constexpr int kZStoreMinIters = 8;    // automatic: a store shorter than the loop's first group is not worth its bookkeeping
constexpr int kZStoreAutoIters = 12;  // automatic: the loop's first two groups (8 + 4 iterations), which every edge of a big batch
                                      // runs; a trace of the headline workload takes ~13, and the iterations after the twelfth run
                                      // with fewer and fewer edges (compacted tables).  16 were measured first: 11.7 GiB per
                                      // 1 024-edge object left 36 of 288 GiB free beside the bench's eight objects, and the sets of
                                      // 256-edge batches its secondary figures create beside them ran out of memory

// The store's budget in bytes.  A QUARTER of the memory free when the store is created, read with the process's stores created
// one at a time (gpet_api_loop.hip).  The bench's eight objects of 1 024 edges take 12 iterations x 1 024 slots of 768 KB (1 000
// rows of z_cols = 96) = 8.8 GiB each, 70 GiB in all, beside arenas of 19.6 GiB each: 130 GiB are free when the first store is
// made on a 288 GB part, 60 GiB after the last.  A process that creates MANY batches gets a geometric series instead of an exhausted device: every store leaves three
// quarters of what was free.  And never into the last EIGHTH of the device: a store is a cache, the arena of the batch created
// after it is not, and a store cannot be taken back when an arena needs the room.  With 36 GiB kept free on a 288 GB part a
// further 1 024-edge batch (bench.py --full creates them beside its eight headline objects) still finds its arena, and it is
// that batch which goes without a store: 60 - 19.6 = 40 GiB free leaves 4 GiB of budget, 5 iterations, fewer than automatic takes.
inline long long zstore_budget(long long free_bytes, long long total_bytes) {
  long long q = free_bytes / 4;
  const long long keep = total_bytes / 8;
  if (free_bytes - q < keep) q = free_bytes - keep;
  return q > 0 ? q : 0;
}

// Iterations held per edge; 0: no store.  B edges, slot_bytes = 8 S z_cols of the batch's largest edge.
//   normals_store: 0 never; -1 automatic: at least kZStoreMinIters or none; 1: whatever the budget allows, down to one iteration
//   normals_store_iters: -1 automatic (kZStoreAutoIters); 0: a budget of zero -- no store; n: n iterations (<= kZStoreMaxIters),
//   fewer if the budget holds fewer (an explicit n may be below kZStoreMinIters)
inline int zstore_iters(int B, long long slot_bytes, long long free_bytes, long long total_bytes, int normals_store, int normals_store_iters) {
  if (normals_store == 0 || normals_store_iters == 0 || B < 1 || slot_bytes < 1) return 0;
  int want = normals_store_iters > 0 ? normals_store_iters : kZStoreAutoIters;
  if (want > kZStoreMaxIters) want = kZStoreMaxIters;
  const long long fit = zstore_budget(free_bytes, total_bytes) / ((long long)B * slot_bytes);
  const int n = fit < want ? (int)fit : want;
  const int least = (normals_store > 0 || normals_store_iters > 0) ? 1 : kZStoreMinIters;
  return n >= least ? n : 0;
}

// What a slot holds: the effective seed (base seed + iteration + 1, or the seed itself for a stage call that names it), the rng
// mode (0 MT19937, 1 Philox) and the columns stored of every row.  S, Lg and z_cols are fixed per batch.  Never 0: 0 = empty.
inline uint64_t zstore_tag(uint32_t eff_seed, int rng_mode, int zs) {
  return (1ull << 63) | ((uint64_t)(rng_mode & 0xF) << 56) | ((uint64_t)((uint32_t)zs & 0xFFFFFFu) << 32) | (uint64_t)eff_seed;
}
inline uint32_t zstore_tag_seed(uint64_t t) { return (uint32_t)t; }
inline int zstore_tag_zs(uint64_t t) { return (int)((t >> 32) & 0xFFFFFFu); }
inline int zstore_tag_mode(uint64_t t) { return (int)((t >> 56) & 0xFu); }
// the tag the loop expects at (edge, iteration)
inline uint64_t zstore_loop_tag(uint32_t base_seed, int iter, int rng_mode, int zs) {
  return zstore_tag(base_seed + (uint32_t)iter + 1u, rng_mode, zs);
}

// how many of the iterations [from, from + n) live in the store (the leading ones: the rest are ring iterations)
inline int zstore_span(int from, int n, int store_iters) {
  const int k = store_iters - from;
  return k <= 0 ? 0 : (k < n ? k : n);
}

// Which edges of a launch table must generate for the store iterations of [from, from + n), and which of them.  tags:
// [.][store_iters], indexed by the ORIGINAL edge index edge_idx[i] of table entry i (nullptr: i itself), as base_seeds is.
// [lo[i], hi[i]] = the iterations from the first to the last one at which the store does not hold what edge i would draw (lo[i] >
// hi[i]: it holds them all).  An edge's misses are a run in practice -- a new seed: all; a trace that ran on: a tail; an injected
// slot: one -- so one launch per distinct range draws no stream twice.  Returns the number of edges with a miss (0: no launch).
inline int zstore_misses(const uint64_t* tags, int store_iters, const int* edge_idx, const uint32_t* base_seeds, int n_edges, int from,
                         int n, int rng_mode, int zs, int* lo, int* hi) {
  const int n_st = zstore_span(from, n, store_iters);
  int edges = 0;
  for (int i = 0; i < n_edges; ++i) {
    const int e = edge_idx ? edge_idx[i] : i;
    lo[i] = from + n;
    hi[i] = from - 1;
    for (int q = from; q < from + n_st; ++q)
      if (tags[(long long)e * store_iters + q] != zstore_loop_tag(base_seeds[e], q, rng_mode, zs)) {
        if (q < lo[i]) lo[i] = q;
        hi[i] = q;
      }
    edges += lo[i] <= hi[i] ? 1 : 0;
  }
  return edges;
}

// ---- ring tags ----------------------------------------------------------------------------------------------------------------
// The ring's slots carry tags of the same kind, [.][ring] per ORIGINAL edge: iteration k >= store_iters lies in slot k % ring, and
// the tag of a slot names the iteration it holds (two iterations that share a slot have different effective seeds).  A tag is
// CLEARED when a launch that may overwrite its slot is enqueued and SET once the launch is known to have generated (zring_settle),
// so a tag never promises what the slot does not hold.  Launch ranges have n <= ring: no range meets a slot twice.
constexpr int kZRingMax = 16;  // the longest ring a batch has (gpet_batch_plan.h: 2, 9 or 16 slots)

inline int zring_slot(int iter, int ring) { return iter % ring; }

// zstore_misses for the ring iterations [from, from + n) (from >= store_iters, n <= ring) of a launch table: [lo[i], hi[i]] = from
// the first to the last iteration whose slot does not hold what edge i would draw there.  Returns the number of edges with a miss.
inline int zring_misses(const uint64_t* rtags, int ring, const int* edge_idx, const uint32_t* base_seeds, int n_edges, int from, int n,
                        int rng_mode, int zs, int* lo, int* hi) {
  int edges = 0;
  for (int i = 0; i < n_edges; ++i) {
    const int e = edge_idx ? edge_idx[i] : i;
    lo[i] = from + n;
    hi[i] = from - 1;
    for (int q = from; q < from + n; ++q)
      if (rtags[(long long)e * ring + zring_slot(q, ring)] != zstore_loop_tag(base_seeds[e], q, rng_mode, zs)) {
        if (q < lo[i]) lo[i] = q;
        hi[i] = q;
      }
    edges += lo[i] <= hi[i] ? 1 : 0;
  }
  return edges;
}

// A launch for the ring iterations [from, from + n) of these edges has been enqueued: whatever their slots held is no longer promised
// (n >= ring: every slot of the edge).
inline void zring_clear(uint64_t* rtags, int ring, const int* edge_idx, int n_edges, int from, int n) {
  const int m = n < ring ? n : ring;
  for (int i = 0; i < n_edges; ++i) {
    const int e = edge_idx ? edge_idx[i] : i;
    for (int q = from; q < from + m; ++q) rtags[(long long)e * ring + zring_slot(q, ring)] = 0;
  }
}

// The launch for the ring iterations [from, from + n) of edge e has come back without a device error; the edge's state is (done,
// iter).  `certain`: every stream was generated -- a table whose entries never read `done`, or a launch enqueued before the first
// iteration of a group whose table held running edges only.  Otherwise the generators skipped the edge once it had finished: only
// the iterations it went on to run (those below its counter) are known to be there.
inline void zring_settle(uint64_t* rtags, int ring, int e, uint32_t base_seed, int from, int n, int done, int iter, int certain,
                         int rng_mode, int zs) {
  int end = from + n;
  if (!certain && done && iter < end) end = iter;
  for (int q = from; q < end; ++q) rtags[(long long)e * ring + zring_slot(q, ring)] = zstore_loop_tag(base_seed, q, rng_mode, zs);
}

// option normals_ring_keep (-1 automatic, 0 never, 1 reserved = automatic): ring tags are kept where the generator's launches go
// onto the loop's own stream (inline: rng_inline 1 or 2); the side-stream modes regenerate their ring iterations on every trace
inline bool zring_keep(int normals_ring_keep, bool inline_mode, int ring) {
  return normals_ring_keep != 0 && inline_mode && ring > 0 && ring <= kZRingMax;
}

}  // namespace gpet
