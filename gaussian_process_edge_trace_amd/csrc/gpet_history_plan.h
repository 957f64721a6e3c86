// Iteration history of a batch (gpet_batch_set_history): sizes and offsets of its device storage as plain data (no HIP), so the
// host compiler alone builds it and a CPU test checks every number (tests/test_history_plan.py).  The storage is ONE allocation
// of its own, outside the batch arena: B edge regions of edge_bytes, each
//   gpet_history_edge_head | iter_cap records of record_bytes
// and a record (the state an edge is in after one loop iteration) is
//   gpet_history_head | int32 obs[obs_cap][2] | level >= 2: f64 curve[len_cap] | level 3: f64 mean[len_cap] | f64 std[len_cap]
// with every section padded to the batch's widest edge (len_cap) and largest observation capacity (obs_cap).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/gpet_hip.h"

namespace gpet {

constexpr int HISTORY_LEVEL_MAX = 3;
// columns of the sample matrix one workgroup of the level-3 statistics owns: a wave's 64 lanes read 512 contiguous bytes of a row
constexpr int HISTORY_COLS = 64;
// waves of that workgroup: wave w sums the rows w, w + HISTORY_WAVES, ... of its columns (the fixed partition of the rows)
constexpr int HISTORY_WAVES = 16;

// false: the arguments describe no history (level outside 1..3, a cap or a size below 1)
inline bool history_args_ok(int level, int iter_cap, int obs_cap, int len_cap) {
  return level >= 1 && level <= HISTORY_LEVEL_MAX && iter_cap >= 1 && obs_cap >= 1 && len_cap >= 1;
}

// the layout for (level, iter_cap, obs_cap, Lg_max); offsets of sections the level does not have are 0.  All zero for bad arguments.
inline gpet_history_plan history_plan(int level, int iter_cap, int obs_cap, int len_cap) {
  gpet_history_plan L = {};
  if (!history_args_ok(level, iter_cap, obs_cap, len_cap)) return L;
  L.level = level;
  L.iter_cap = iter_cap;
  L.obs_cap = obs_cap;
  L.len_cap = len_cap;
  L.off_records = (int64_t)sizeof(gpet_history_edge_head);
  int64_t off = (int64_t)sizeof(gpet_history_head);
  L.off_obs = off;
  off += (int64_t)obs_cap * 2 * (int64_t)sizeof(int32_t);  // (a multiple of 8: the f64 sections stay aligned)
  if (level >= 2) {
    L.off_curve = off;
    off += (int64_t)len_cap * (int64_t)sizeof(double);
  }
  if (level >= 3) {
    L.off_mean = off;
    off += (int64_t)len_cap * (int64_t)sizeof(double);
    L.off_std = off;
    off += (int64_t)len_cap * (int64_t)sizeof(double);
  }
  L.record_bytes = off;
  L.edge_bytes = L.off_records + (int64_t)iter_cap * L.record_bytes;
  if (L.edge_bytes > ((int64_t)1 << 40)) L = {};  // (no batch gets that far; keeps B * edge_bytes inside size_t arithmetic)
  return L;
}

// workgroups per edge of the history kernel: one per HISTORY_COLS columns for the statistics of level 3, else one
inline int history_tiles(int level, int len_cap) { return level >= 3 ? (len_cap + HISTORY_COLS - 1) / HISTORY_COLS : 1; }

}  // namespace gpet
