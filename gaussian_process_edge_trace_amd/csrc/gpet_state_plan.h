// What a batch knows about the validity of what it holds, and what every call of the C ABI needs of it, makes of it and drops of it,
// as plain data: eight facts, two counters, and ONE table with a row per event.  No HIP, so the host compiler alone builds it
// (tests/test_state_plan.py).  The entry points (gpet_api_*.hip) ask state_missing before they refuse and call state_apply where the
// event happens; codes and message texts are theirs, the rules are written here once.
#pragma once

namespace gpet {

// ---- the facts ----------------------------------------------------------------------------------------------------------------
enum StateBit : unsigned {
  ST_FIT = 1u << 0,       // the loop's fit of the current observation sets: L / alpha, mean and covariance
  ST_FACTOR = 1u << 1,    // the factor rows of that covariance
  ST_NORMALS = 1u << 2,   // normals of the batch's generator in the slot of every edge's iteration
  ST_SAMPLES = 1u << 3,   // the sample matrix, in the batch's sample type
  ST_SCORES = 1u << 4,    // costs and the kept curves' indices
  // gpet_final_fit_all has run on the CURRENT trace: d_fin_out / lb_theta_out hold what gpet_batch_results packs
  ST_RESULTS = 1u << 5,
  // the converged fits of the LAST trace are in d_fin_out: what a warm start derives the next frame's observations from.  No reset
  // and no image swap touches d_fin_out, which is why this fact outlives both where ST_RESULTS does not
  ST_LAST_FIT = 1u << 6,
  // gpet_batch_ensemble_keep has left the ensemble of the last converged fits in the batch's scratch, with its group table: what
  // gpet_batch_warm_start_groups takes its sources from.  It belongs to those fits, not to the images: a swap leaves it alone
  ST_ENS_KEPT = 1u << 7,
  // (never held: what state_missing reports for an event that needs a batch no iteration has run on)
  ST_ITERATIONS_RAN = 1u << 8,
};
constexpr unsigned ST_STAGES = ST_FIT | ST_FACTOR | ST_NORMALS | ST_SAMPLES | ST_SCORES;
constexpr unsigned ST_TRACE = ST_RESULTS | ST_LAST_FIT;  // what belongs to one trace's converged fit

struct BatchState {
  unsigned have = 0;
  int iters_issued = 0;  // iterations enqueued since the last restart (== sc->iter of active edges)
  int norm_issued = 0;   // iterations whose normals have been enqueued (the loop advances it itself; zeroed with iters_issued)
};

// ---- the events ---------------------------------------------------------------------------------------------------------------
enum class StateEvent {
  // per-stage entry points: the need is checked on entry, the row applied once the stage's launches are enqueued
  stage_fit,           // gpet_gp_fit_predict
  stage_factor,        // gpet_gp_factor
  stage_normals,       // gpet_gp_normals
  stage_sample,        // gpet_gp_sample
  stage_score,         // gpet_score_curves
  stage_kde,           // gpet_curve_kde
  final_cov,           // gpet_final_cov: the covariance of the converged fit where gpet_gp_factor reads it
  select_pixels,       // gpet_select_pixels, gpet_select_pixels_loop, after their refusal: a new observation set, another trace;
                       // iteration_enqueued follows behind the launches
  select_pixels_only,  // gpet_select_pixels_only: the same without the need
  // gpet_batch_write, by buffer (the other buffers change nothing)
  write_factor, write_normals, write_samples, write_best_idx, write_cov,
  write_scalars,       // (the scalars hold the observation count and the iteration: another trace)
  // settings
  set_rng,             // gpet_batch_set_rng: the slots hold the other generator's numbers
  set_sample_type,     // gpet_batch_set_sample_dtype, gpet_batch_set_sample_arith
  init_moved,          // gpet_batch_init_follow, gpet_batch_set_init: what the stages derived from the old init rows is not the next
                       // stage's input any more; normals do not depend on them
  // restarts
  reset,               // gpet_batch_reset
  images_swapped,      // gpet_batch_set_images and its raw forms: the state of a fresh constructor, but for the last converged fits
                       // and a kept ensemble
  set_obs_entry,       // gpet_batch_set_obs, before it looks at the pixels
  observations_set,    // gpet_batch_set_obs once nothing refuses any more; the end of every warm start (warm_start_finish)
  // the device loop
  trace_entry,         // gpet_trace_iterate: another trace is under way
  iteration_enqueued,  // the kernel chain of one iteration (the loop, the pixel-selection entry points)
  group_end,           // the loop has run every stage
  // converged fits
  final_predict_begin, // gpet_final_predict_all, after its refusal: a caller's own parameters
  final_predict_end,   // the loop's L / alpha were overwritten
  final_fit_begin,     // gpet_final_fit_all, before its first HIP call
  final_fit_end,
  final_optimize,      // lb_theta_out is about to hold another optimum
  // seed ensembles
  ensemble_keep_begin, ensemble_keep_end,
  // readers: rows with a need alone, never applied
  read_last_fit,       // gpet_batch_warm_start_ready and whatever asks it (every warm start, gpet_batch_band_place)
  read_results,        // gpet_batch_results, gpet_batch_final_costs, gpet_batch_ensemble[_keep]
  read_kept_ensemble,  // gpet_batch_ensemble_kept, gpet_batch_warm_start_groups, gpet_batch_band_place from a group
  count_
};

enum class StateIters { keep, zero, plus_one };

struct StateRow {
  StateEvent event;
  unsigned needs, sets, clears;
  StateIters iters;          // zero: norm_issued with it
  bool needs_no_iterations;  // refused once an iteration has been enqueued since the last restart
};

// ---- the table ----------------------------------------------------------------------------------------------------------------
constexpr StateRow STATE_TABLE[] = {
    //                                 needs                                sets          clears                     iterations
    {StateEvent::stage_fit,            0,                                   ST_FIT,       0,                         StateIters::keep, false},
    {StateEvent::stage_factor,         ST_FIT,                              ST_FACTOR,    0,                         StateIters::keep, false},
    {StateEvent::stage_normals,        0,                                   ST_NORMALS,   0,                         StateIters::keep, false},
    {StateEvent::stage_sample,         ST_FIT | ST_FACTOR | ST_NORMALS,     ST_SAMPLES,   0,                         StateIters::keep, false},
    {StateEvent::stage_score,          ST_SAMPLES,                          ST_SCORES,    0,                         StateIters::keep, false},
    {StateEvent::stage_kde,            ST_SCORES,                           0,            0,                         StateIters::keep, false},
    {StateEvent::final_cov,            0,                                   ST_FIT,       0,                         StateIters::keep, false},
    {StateEvent::select_pixels,        ST_SCORES,                           0,            ST_TRACE,                  StateIters::keep, false},
    {StateEvent::select_pixels_only,   0,                                   0,            ST_TRACE,                  StateIters::keep, false},
    {StateEvent::write_factor,         0,                                   ST_FACTOR,    0,                         StateIters::keep, false},
    {StateEvent::write_normals,        0,                                   ST_NORMALS,   0,                         StateIters::keep, false},
    {StateEvent::write_samples,        0,                                   ST_SAMPLES,   0,                         StateIters::keep, false},
    {StateEvent::write_best_idx,       0,                                   ST_SCORES,    0,                         StateIters::keep, false},
    {StateEvent::write_cov,            0,                                   ST_FIT,       0,                         StateIters::keep, false},
    {StateEvent::write_scalars,        0,                                   0,            ST_TRACE,                  StateIters::keep, false},
    {StateEvent::set_rng,              0,                                   0,            ST_NORMALS,                StateIters::keep, false},
    {StateEvent::set_sample_type,      0,                                   0,            ST_SAMPLES,                StateIters::keep, false},
    {StateEvent::init_moved,           0,                                   0,            ST_STAGES & ~ST_NORMALS,   StateIters::keep, true},
    {StateEvent::reset,                0,                                   0,            ST_RESULTS | ST_ENS_KEPT,  StateIters::zero, false},
    {StateEvent::images_swapped,       0,                                   0,            ST_STAGES | ST_RESULTS,    StateIters::zero, false},
    {StateEvent::set_obs_entry,        0,                                   0,            ST_TRACE | ST_ENS_KEPT,    StateIters::keep, false},
    {StateEvent::observations_set,     0,                                   0,            ST_TRACE | ST_ENS_KEPT,    StateIters::zero, false},
    {StateEvent::trace_entry,          0,                                   0,            ST_TRACE,                  StateIters::keep, false},
    {StateEvent::iteration_enqueued,   0,                                   0,            0,                         StateIters::plus_one, false},
    {StateEvent::group_end,            0,                                   ST_STAGES,    0,                         StateIters::keep, false},
    {StateEvent::final_predict_begin,  0,                                   0,            ST_TRACE,                  StateIters::keep, false},
    {StateEvent::final_predict_end,    0,                                   0,            ST_FIT,                    StateIters::keep, false},
    {StateEvent::final_fit_begin,      0,                                   0,            ST_TRACE | ST_ENS_KEPT,    StateIters::keep, false},
    {StateEvent::final_fit_end,        0,                                   ST_TRACE,     ST_FIT,                    StateIters::keep, false},
    {StateEvent::final_optimize,       0,                                   0,            ST_RESULTS,                StateIters::keep, false},
    {StateEvent::ensemble_keep_begin,  0,                                   0,            ST_ENS_KEPT,               StateIters::keep, false},
    {StateEvent::ensemble_keep_end,    0,                                   ST_ENS_KEPT,  0,                         StateIters::keep, false},
    {StateEvent::read_last_fit,        ST_LAST_FIT,                         0,            0,                         StateIters::keep, false},
    {StateEvent::read_results,         ST_RESULTS,                          0,            0,                         StateIters::keep, false},
    {StateEvent::read_kept_ensemble,   ST_ENS_KEPT,                         0,            0,                         StateIters::keep, false},
};
constexpr int STATE_ROWS = (int)(sizeof(STATE_TABLE) / sizeof(STATE_TABLE[0]));

// every event has its row, at its own index
constexpr bool state_table_in_order() {
  for (int i = 0; i < STATE_ROWS; ++i)
    if ((int)STATE_TABLE[i].event != i) return false;
  return true;
}
static_assert(STATE_ROWS == (int)StateEvent::count_ && state_table_in_order(), "STATE_TABLE: one row per StateEvent, in the enum's order");

constexpr const StateRow& state_row(StateEvent ev) { return STATE_TABLE[(int)ev]; }

// ---- the two questions --------------------------------------------------------------------------------------------------------
// what the event needs and the batch has not (0: go)
inline unsigned state_missing(const BatchState& st, StateEvent ev) {
  const StateRow& r = state_row(ev);
  return (r.needs & ~st.have) | (r.needs_no_iterations && st.iters_issued != 0 ? (unsigned)ST_ITERATIONS_RAN : 0u);
}
// the event has happened
inline void state_apply(BatchState& st, StateEvent ev) {
  const StateRow& r = state_row(ev);
  st.have = (st.have & ~r.clears) | r.sets;
  if (r.iters == StateIters::zero) st.iters_issued = st.norm_issued = 0;
  if (r.iters == StateIters::plus_one) st.iters_issued += 1;
}

}  // namespace gpet
