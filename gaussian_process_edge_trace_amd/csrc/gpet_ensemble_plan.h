// Seed ensembles (gpet_batch_ensemble; include/gpet_hip.h, "seed ensembles"): the layout of what the call returns, the validation
// of its arguments with their messages, the member tables and the tiling of the reduction kernel, as plain data (no HIP), so the
// host compiler alone builds it and a CPU test checks every number (tests/test_ensemble_plan.py).
//   dst    = G records | f64 cost[B] | int32 off[B] (padded to 8 bytes)
//   record = gpet_ensemble_head | int64 trace[len_cap][2] | f64 median | q_lo | q_hi | min | max [len_cap] each
//                               | int32 agree[len_cap] (padded to 8 bytes)
// The kernel (k_ensemble, gpet_k_ensemble.inc): a workgroup owns one group x one tile of columns and holds the tile of all n members
// twice in LDS -- as loaded, and in ascending order per column.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/gpet_hip.h"

namespace gpet {

constexpr int ENSEMBLE_MAX = GPET_ENSEMBLE_MAX;
constexpr int ENSEMBLE_THREADS = 256;
// widest tile: a wave's load of a member's row is 64 consecutive doubles of fin_out
constexpr int ENSEMBLE_COLS_MAX = 64;
// one copy of a tile (n members x cols columns of f64) stays inside this; the tile is narrowed for bigger groups
constexpr int ENSEMBLE_TILE_BYTES = 32 * 1024;
// everything a workgroup keeps in LDS stays inside this: two workgroups share a CU's 160 KB
constexpr int ENSEMBLE_LDS_BUDGET = 80 * 1024;

struct EnsembleLayout {
  int64_t record_bytes, off_trace, off_median, off_q_lo, off_q_hi, off_min, off_max, off_agree;  // offsets inside a record
  int64_t off_cost, off_off, total_bytes;                                                        // offsets inside dst
};

// all zero for arguments that describe no buffer (G < 1, B < 1, len_cap < 1 or beyond 2^24 points)
inline EnsembleLayout ensemble_layout(int G, int B, int64_t len_cap) {
  EnsembleLayout L = {};
  if (G < 1 || B < 1 || len_cap < 1 || len_cap > ((int64_t)1 << 24)) return L;
  int64_t off = (int64_t)sizeof(gpet_ensemble_head);
  L.off_trace = off;
  off += len_cap * 2 * (int64_t)sizeof(int64_t);
  int64_t* const f64_sections[5] = {&L.off_median, &L.off_q_lo, &L.off_q_hi, &L.off_min, &L.off_max};
  for (int64_t* p : f64_sections) {
    *p = off;
    off += len_cap * (int64_t)sizeof(double);
  }
  L.off_agree = off;
  off += (len_cap * (int64_t)sizeof(int32_t) + 7) & ~(int64_t)7;
  L.record_bytes = off;
  L.off_cost = (int64_t)G * L.record_bytes;
  L.off_off = L.off_cost + (int64_t)B * (int64_t)sizeof(double);
  L.total_bytes = L.off_off + (((int64_t)B * (int64_t)sizeof(int32_t) + 7) & ~(int64_t)7);
  return L;
}

// columns of a tile for a group of n members: the largest power of two <= ENSEMBLE_COLS_MAX whose tile fits ENSEMBLE_TILE_BYTES
// (n <= 64: 64, n = 65: 32, n = 1024: 4); 0 for an n outside [0, ENSEMBLE_MAX]
inline int ensemble_tile_cols(int n) {
  if (n < 0 || n > ENSEMBLE_MAX) return 0;
  int cols = ENSEMBLE_COLS_MAX;
  while (cols > 1 && (int64_t)n * cols * (int64_t)sizeof(double) > ENSEMBLE_TILE_BYTES) cols >>= 1;
  return cols;
}

// LDS of a workgroup: the tile as loaded | the tile in order | the consensus of every column (f64) | the members' fin_out pointers
// | agree per column (int32) | off per member (int32)
inline size_t ensemble_lds_bytes(int n, int cols) {
  return (size_t)2 * n * cols * sizeof(double) + (size_t)cols * sizeof(double) + (size_t)n * sizeof(void*) +
         (size_t)cols * sizeof(int32_t) + (size_t)n * sizeof(int32_t);
}

struct EnsembleGroup {  // as the kernels read it
  int32_t n;           // members
  int32_t x_st, len;   // the group's x-grid
  int32_t member_off;  // its members are members[member_off .. member_off + n)
  int32_t cols, log2_cols, tiles, pad;
};

struct EnsemblePlan {
  std::vector<EnsembleGroup> groups;
  std::vector<int32_t> members;       // edge indices, group by group, ascending inside a group
  std::vector<int32_t> member_group;  // [B] the group an edge is a MEMBER of, -1: in no group or excluded
  std::vector<int32_t> wg_group, wg_tile;  // one entry per workgroup of the reduction kernel
  size_t lds_bytes = 0;  // the largest group's
};

// GPET_OK, or GPET_ERR_BAD_ARG with the reason in msg.  x_st / x_en: every edge's grid; status (may be nullptr: all GPET_OK):
// every edge's gpet_scalars.status
inline int ensemble_plan(int G, int B, const int32_t* group_of, const int32_t* x_st, const int32_t* x_en, const int32_t* status,
                         double tol, EnsemblePlan* out, char* msg, size_t msg_cap) {
  auto bad = [&](const char* fmt, long long a, long long b, long long c, long long d) {
    if (msg && msg_cap) snprintf(msg, msg_cap, fmt, a, b, c, d);
    return (int)GPET_ERR_BAD_ARG;
  };
  if (msg && msg_cap) msg[0] = 0;
  if (G < 1 || B < 1 || !group_of || !x_st || !x_en) return bad("gpet_batch_ensemble: bad argument (n_groups=%lld, edges=%lld)", G, B, 0, 0);
  if (!(tol >= 0.0)) {
    if (msg && msg_cap) snprintf(msg, msg_cap, "gpet_batch_ensemble: tol=%g is negative (or not a number)", tol);
    return (int)GPET_ERR_BAD_ARG;
  }
  std::vector<int32_t> first((size_t)G, -1), count((size_t)G, 0);
  for (int e = 0; e < B; ++e) {
    const int g = group_of[e];
    if (g == -1) continue;
    if (g < 0 || g >= G) return bad("gpet_batch_ensemble: group_of[%lld]=%lld is outside [0, %lld) (-1: in no group)", e, g, G, 0);
    if (first[g] < 0) first[g] = e;
    const int f = first[g];
    if (x_st[e] != x_st[f] || x_en[e] != x_en[f])
      return bad("gpet_batch_ensemble: group %lld: edges %lld and %lld have different x-grids (%lld points against the first's)", g, f, e,
                 (long long)x_en[e] - x_st[e] + 1);
    if (!status || status[e] == GPET_OK) count[g] += 1;
  }
  for (int g = 0; g < G; ++g) {
    if (first[g] < 0) return bad("gpet_batch_ensemble: group %lld of %lld has no edge (every index must occur)", g, G, 0, 0);
    if (count[g] > ENSEMBLE_MAX) return bad("gpet_batch_ensemble: group %lld has %lld members, more than %lld", g, count[g], ENSEMBLE_MAX, 0);
  }
  if (!out) return GPET_OK;
  out->groups.assign((size_t)G, EnsembleGroup{});
  out->members.clear();
  out->member_group.assign((size_t)B, -1);
  out->wg_group.clear();
  out->wg_tile.clear();
  out->lds_bytes = 0;
  int32_t at = 0;
  for (int g = 0; g < G; ++g) {
    EnsembleGroup& Q = out->groups[g];
    Q.n = count[g];
    Q.x_st = x_st[first[g]];
    Q.len = x_en[first[g]] - x_st[first[g]] + 1;
    Q.member_off = at;
    at += count[g];
    Q.cols = ensemble_tile_cols(Q.n);
    Q.log2_cols = 0;
    while ((1 << Q.log2_cols) < Q.cols) Q.log2_cols += 1;
    Q.tiles = Q.n > 0 ? (Q.len + Q.cols - 1) / Q.cols : 0;  // (a group without members: nothing to reduce)
    for (int t = 0; t < Q.tiles; ++t) {
      out->wg_group.push_back(g);
      out->wg_tile.push_back(t);
    }
    const size_t lds = ensemble_lds_bytes(Q.n, Q.cols);
    if (Q.n > 0 && lds > out->lds_bytes) out->lds_bytes = lds;
  }
  out->members.assign((size_t)at, 0);
  std::vector<int32_t> fill((size_t)G, 0);
  for (int e = 0; e < B; ++e) {
    const int g = group_of[e];
    if (g < 0 || (status && status[e] != GPET_OK)) continue;
    out->members[(size_t)out->groups[g].member_off + fill[g]++] = e;
    out->member_group[e] = g;
  }
  return GPET_OK;
}

}  // namespace gpet
