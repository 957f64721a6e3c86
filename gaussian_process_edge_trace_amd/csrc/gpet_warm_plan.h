// Warm start of a sequence's next frame from a source other than the edge itself (gpet_batch_ensemble_keep, gpet_batch_warm_start_groups,
// gpet_batch_warm_start_from; include/gpet_hip.h, "seed ensembles in sequences"): which edge -- or the consensus, or nothing -- every
// edge takes its observations from, the refusals with their messages, and the size of the kept ensemble, as plain data (no HIP), so the
// host compiler alone builds it and a CPU test checks every case (tests/test_warm_plan.py).
//   kept = the buffer of gpet_batch_ensemble for len_cap = the batch's widest edge | int32 group_of[B] (padded to 8 bytes)
// The source of an edge is decided from the kept records' HEADS and the table alone, before the warm-start kernel is launched: that
// kernel never looks at another edge's scalars (their own waves are writing them in the same launch).
#pragma once
#include "gpet_ensemble_plan.h"

#if defined(__HIPCC__)
#define GPET_WARM_HD __host__ __device__
#else
#define GPET_WARM_HD
#endif

namespace gpet {

// what src[e] holds besides an edge index
constexpr int32_t WARM_SRC_NONE = -1;       // the empty observation set
constexpr int32_t WARM_SRC_CONSENSUS = -2;  // the int64 consensus row of the kept record of the edge's group

// The source of edge e.  group: group_of[e] (-1: in no group -> its own fit, as gpet_batch_warm_start); n_members, medoid, best_cost:
// the head of that group's kept record; from: GPET_WARM_MEDOID / _BEST_COST / _CONSENSUS.  Every edge ASSIGNED to the group gets the
// group's source, a member or not; a group without members gives nothing.
GPET_WARM_HD inline int32_t warm_source(int32_t e, int32_t group, int32_t n_members, int32_t medoid, int32_t best_cost, int from) {
  if (group < 0) return e;
  if (n_members < 1) return WARM_SRC_NONE;
  if (from == GPET_WARM_MEDOID) return medoid;
  if (from == GPET_WARM_BEST_COST) return best_cost;
  return WARM_SRC_CONSENSUS;
}

// the whole table on the host (heads: one per group); the device fills its own with warm_source, thread per edge
inline void warm_sources(int B, const int32_t* group_of, const gpet_ensemble_head* heads, int from, int32_t* src) {
  for (int e = 0; e < B; ++e) {
    const int32_t g = group_of[e];
    src[e] = g < 0 ? warm_source(e, g, 0, -1, -1, from) : warm_source(e, g, heads[g].n_members, heads[g].medoid, heads[g].best_cost, from);
  }
}

// bytes of the kept ensemble; 0 for arguments that describe none
inline int64_t warm_kept_group_off(int G, int B, int64_t len_cap) { return ensemble_layout(G, B, len_cap).total_bytes; }
inline int64_t warm_kept_bytes(int G, int B, int64_t len_cap) {
  const int64_t ens = ensemble_layout(G, B, len_cap).total_bytes;
  return ens ? ens + (((int64_t)B * (int64_t)sizeof(int32_t) + 7) & ~(int64_t)7) : 0;
}

// gpet_batch_warm_start_groups: GPET_OK, or GPET_ERR_BAD_ARG with the reason in msg (kept: an ensemble is kept)
inline int warm_groups_check(int from, bool kept, char* msg, size_t msg_cap) {
  if (msg && msg_cap) msg[0] = 0;
  if (from != GPET_WARM_MEDOID && from != GPET_WARM_BEST_COST && from != GPET_WARM_CONSENSUS) {
    if (msg && msg_cap)
      snprintf(msg, msg_cap, "gpet_batch_warm_start_groups: from=%d is none of GPET_WARM_MEDOID, GPET_WARM_BEST_COST, GPET_WARM_CONSENSUS", from);
    return (int)GPET_ERR_BAD_ARG;
  }
  if (!kept) {
    if (msg && msg_cap)
      snprintf(msg, msg_cap, "gpet_batch_warm_start_groups: no ensemble is kept (call gpet_batch_ensemble_keep after the trace's "
                             "gpet_final_fit_all and before the images are swapped; a warm start, gpet_batch_set_obs, gpet_batch_reset "
                             "or another gpet_final_fit_all since then have dropped it)");
    return (int)GPET_ERR_BAD_ARG;
  }
  return GPET_OK;
}

// gpet_batch_warm_start_from: src_of[e] in [0, B) or WARM_SRC_NONE, and e and its source on one x-grid; the edge is named
inline int warm_from_check(int B, const int32_t* src_of, const int32_t* x_st, const int32_t* x_en, char* msg, size_t msg_cap) {
  if (msg && msg_cap) msg[0] = 0;
  if (B < 1 || !src_of || !x_st || !x_en) {
    if (msg && msg_cap) snprintf(msg, msg_cap, "gpet_batch_warm_start_from: bad argument (edges=%d)", B);
    return (int)GPET_ERR_BAD_ARG;
  }
  for (int e = 0; e < B; ++e) {
    const int32_t s = src_of[e];
    if (s == WARM_SRC_NONE) continue;
    if (s < 0 || s >= B) {
      if (msg && msg_cap)
        snprintf(msg, msg_cap, "gpet_batch_warm_start_from: edge %d: src_of=%d is outside [0, %d) (-1: no observations)", e, (int)s, B);
      return (int)GPET_ERR_BAD_ARG;
    }
    if (x_st[e] != x_st[s] || x_en[e] != x_en[s]) {
      if (msg && msg_cap)
        snprintf(msg, msg_cap, "gpet_batch_warm_start_from: edge %d spans columns %d..%d, its source edge %d spans %d..%d", e, (int)x_st[e],
                 (int)x_en[e], (int)s, (int)x_st[s], (int)x_en[s]);
      return (int)GPET_ERR_BAD_ARG;
    }
  }
  return GPET_OK;
}

}  // namespace gpet
