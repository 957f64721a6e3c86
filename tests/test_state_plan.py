"""CPU tests of the state rules of a batch (csrc/gpet_state_plan.h): the header needs no HIP, so a small extern "C" shim around it is
compiled with the host C++ compiler and driven through ctypes.  Every expectation below is a literal, written from the entry points as
they set and read the batch's ten state members before the rules moved into the header -- never computed by calling the header."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussian_process_edge_trace_amd", "csrc")

FIT, FACTOR, NORMALS, SAMPLES, SCORES, RESULTS, LAST_FIT, ENS_KEPT, ITERATIONS_RAN = (1 << i for i in range(9))
STAGES = FIT | FACTOR | NORMALS | SAMPLES | SCORES
KEEP, ZERO, PLUS_ONE = 0, 1, 2

# event: (needs, sets, clears, counters, needs a batch without iterations), in the enum's order
ROWS = {
    "stage_fit": (0, FIT, 0, KEEP, False),
    "stage_factor": (FIT, FACTOR, 0, KEEP, False),
    "stage_normals": (0, NORMALS, 0, KEEP, False),
    "stage_sample": (FIT | FACTOR | NORMALS, SAMPLES, 0, KEEP, False),
    "stage_score": (SAMPLES, SCORES, 0, KEEP, False),
    "stage_kde": (SCORES, 0, 0, KEEP, False),
    "final_cov": (0, FIT, 0, KEEP, False),
    "select_pixels": (SCORES, 0, RESULTS | LAST_FIT, KEEP, False),
    "select_pixels_only": (0, 0, RESULTS | LAST_FIT, KEEP, False),
    "write_factor": (0, FACTOR, 0, KEEP, False),
    "write_normals": (0, NORMALS, 0, KEEP, False),
    "write_samples": (0, SAMPLES, 0, KEEP, False),
    "write_best_idx": (0, SCORES, 0, KEEP, False),
    "write_cov": (0, FIT, 0, KEEP, False),
    "write_scalars": (0, 0, RESULTS | LAST_FIT, KEEP, False),
    "set_rng": (0, 0, NORMALS, KEEP, False),
    "set_sample_type": (0, 0, SAMPLES, KEEP, False),
    "init_moved": (0, 0, FIT | FACTOR | SAMPLES | SCORES, KEEP, True),
    "reset": (0, 0, RESULTS | ENS_KEPT, ZERO, False),
    "images_swapped": (0, 0, STAGES | RESULTS, ZERO, False),
    "set_obs_entry": (0, 0, RESULTS | LAST_FIT | ENS_KEPT, KEEP, False),
    "observations_set": (0, 0, RESULTS | LAST_FIT | ENS_KEPT, ZERO, False),
    "trace_entry": (0, 0, RESULTS | LAST_FIT, KEEP, False),
    "iteration_enqueued": (0, 0, 0, PLUS_ONE, False),
    "group_end": (0, STAGES, 0, KEEP, False),
    "final_predict_begin": (0, 0, RESULTS | LAST_FIT, KEEP, False),
    "final_predict_end": (0, 0, FIT, KEEP, False),
    "final_fit_begin": (0, 0, RESULTS | LAST_FIT | ENS_KEPT, KEEP, False),
    "final_fit_end": (0, RESULTS | LAST_FIT, FIT, KEEP, False),
    "final_optimize": (0, 0, RESULTS, KEEP, False),
    "ensemble_keep_begin": (0, 0, ENS_KEPT, KEEP, False),
    "ensemble_keep_end": (0, ENS_KEPT, 0, KEEP, False),
    "read_last_fit": (LAST_FIT, 0, 0, KEEP, False),
    "read_results": (RESULTS, 0, 0, KEEP, False),
    "read_kept_ensemble": (ENS_KEPT, 0, 0, KEEP, False),
}
EVENTS = list(ROWS)

SHIM = r"""
#include <string.h>
#include "gpet_state_plan.h"
using namespace gpet;
#define EV(x) {#x, (int)StateEvent::x}
static const struct { const char* name; int ev; } NAMES[] = {
  __NAMES__
};
extern "C" {
int shim_bit(int i) {
  const unsigned v[] = {ST_FIT, ST_FACTOR, ST_NORMALS, ST_SAMPLES, ST_SCORES, ST_RESULTS, ST_LAST_FIT, ST_ENS_KEPT, ST_ITERATIONS_RAN};
  return (int)v[i];
}
int shim_event_count() { return (int)StateEvent::count_; }
int shim_rows() { return STATE_ROWS; }
int shim_row_event(int i) { return (int)STATE_TABLE[i].event; }
int shim_event(const char* name) {
  for (const auto& n : NAMES)
    if (!strcmp(n.name, name)) return n.ev;
  return -1;
}
int shim_missing(unsigned have, int iters, int ev) {
  BatchState st;
  st.have = have;
  st.iters_issued = iters;
  return (int)state_missing(st, (StateEvent)ev);
}
// io = {have, iters_issued, norm_issued}
void shim_apply(int* io, int ev) {
  BatchState st;
  st.have = (unsigned)io[0];
  st.iters_issued = io[1];
  st.norm_issued = io[2];
  state_apply(st, (StateEvent)ev);
  io[0] = (int)st.have;
  io[1] = st.iters_issued;
  io[2] = st.norm_issued;
}
}
"""


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = cxx and shutil.which(cxx)
        if path:
            return path
    return None


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("state_plan")
    src, so = d / "shim.cpp", d / "libstate_plan_shim.so"
    src.write_text(SHIM.replace("__NAMES__", ", ".join("EV(%s)" % n for n in EVENTS)))
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    return C.CDLL(str(so))


def missing(shim, have, event, iters=0):
    return shim.shim_missing(have, iters, shim.shim_event(event.encode()))


def apply(shim, state, event):
    """state = (have, iters_issued, norm_issued) after the event"""
    io = (C.c_int * 3)(*state)
    shim.shim_apply(io, shim.shim_event(event.encode()))
    return tuple(io)


def run(shim, events, have=0):
    state = (have, 0, 0)
    for ev in events:
        state = apply(shim, state, ev)
    return state[0]


def test_bits(shim):
    assert [shim.shim_bit(i) for i in range(9)] == [FIT, FACTOR, NORMALS, SAMPLES, SCORES, RESULTS, LAST_FIT, ENS_KEPT, ITERATIONS_RAN]


def test_every_event_has_exactly_one_row(shim):
    assert shim.shim_event_count() == shim.shim_rows() == len(EVENTS)
    assert [shim.shim_event(n.encode()) for n in EVENTS] == list(range(len(EVENTS)))
    assert [shim.shim_row_event(i) for i in range(shim.shim_rows())] == list(range(len(EVENTS)))


@pytest.mark.parametrize("event", EVENTS)
def test_row(shim, event):
    needs, sets, clears, counters, no_iterations = ROWS[event]
    for iters in (0, 3):
        for have in range(256):
            want = needs & ~have
            if no_iterations and iters:
                want |= ITERATIONS_RAN
            assert missing(shim, have, event, iters) == want, (have, iters)
            after = ((have & ~clears) | sets,) + {KEEP: (iters, 7), ZERO: (0, 0), PLUS_ONE: (iters + 1, 7)}[counters]
            assert apply(shim, (have, iters, 7), event) == after, (have, iters)


# ---- the life cycles the comments at the members used to promise ----

FINAL_FIT = ["trace_entry", "iteration_enqueued", "group_end", "final_fit_begin", "final_fit_end"]


def test_last_fit_and_kept_ensemble_survive_an_image_swap(shim):
    have = run(shim, FINAL_FIT + ["ensemble_keep_begin", "ensemble_keep_end"])
    assert have == (STAGES & ~FIT) | RESULTS | LAST_FIT | ENS_KEPT
    assert run(shim, ["images_swapped"], have) == LAST_FIT | ENS_KEPT


def test_public_reset_drops_the_kept_ensemble_not_the_last_fit(shim):
    have = run(shim, FINAL_FIT + ["ensemble_keep_begin", "ensemble_keep_end", "reset"])
    assert have == (STAGES & ~FIT) | LAST_FIT


@pytest.mark.parametrize("event", ["set_obs_entry", "observations_set", "final_fit_begin"])
def test_what_drops_a_kept_ensemble_with_the_fits(shim, event):
    have = run(shim, FINAL_FIT + ["ensemble_keep_begin", "ensemble_keep_end", event])
    assert have == STAGES & ~FIT


def test_trace_entry_drops_the_last_fit_not_the_kept_ensemble(shim):
    have = run(shim, FINAL_FIT + ["ensemble_keep_begin", "ensemble_keep_end", "trace_entry"])
    assert have == (STAGES & ~FIT) | ENS_KEPT
    for event in ("select_pixels", "select_pixels_only", "write_scalars", "final_predict_begin"):
        assert run(shim, [event], RESULTS | LAST_FIT | ENS_KEPT) == ENS_KEPT
    assert run(shim, ["final_optimize"], RESULTS | LAST_FIT | ENS_KEPT) == LAST_FIT | ENS_KEPT


def test_moved_init_points_keep_the_normals(shim):
    assert run(shim, ["init_moved"], STAGES | RESULTS | LAST_FIT | ENS_KEPT) == NORMALS | RESULTS | LAST_FIT | ENS_KEPT
    assert missing(shim, 0, "init_moved", iters=0) == 0 and missing(shim, 255, "init_moved", iters=1) == ITERATIONS_RAN
    # one iteration by either route refuses the move; every restart allows it again
    for route in (["iteration_enqueued"], ["select_pixels", "iteration_enqueued"]):
        state = (SCORES, 0, 0)
        for ev in route:
            state = apply(shim, state, ev)
        assert state[1] == 1 and shim.shim_missing(state[0], state[1], shim.shim_event(b"init_moved")) == ITERATIONS_RAN
        for restart in ("reset", "images_swapped", "observations_set"):
            after = apply(shim, state, restart)
            assert after[1:] == (0, 0) and shim.shim_missing(after[0], after[1], shim.shim_event(b"init_moved")) == 0


def test_set_rng_makes_the_sampler_refuse_until_new_normals_exist(shim):
    have = run(shim, ["stage_fit", "stage_factor", "stage_normals"])
    assert missing(shim, have, "stage_sample") == 0
    have = run(shim, ["stage_sample", "set_rng"], have)
    assert missing(shim, have, "stage_sample") == NORMALS
    for again in ("stage_normals", "write_normals", "group_end"):
        assert missing(shim, run(shim, [again], have), "stage_sample") == 0


def test_set_sample_type_makes_the_scorer_refuse_until_new_samples_exist(shim):
    have = run(shim, ["stage_fit", "stage_factor", "stage_normals", "stage_sample"])
    assert missing(shim, have, "stage_score") == 0
    have = run(shim, ["stage_score", "set_sample_type"], have)
    assert missing(shim, have, "stage_score") == SAMPLES and missing(shim, have, "stage_kde") == 0
    for again in ("stage_sample", "write_samples", "group_end"):
        assert missing(shim, run(shim, [again], have), "stage_score") == 0


def test_stage_order(shim):
    assert missing(shim, 0, "stage_factor") == FIT
    assert missing(shim, 0, "stage_sample") == FIT | FACTOR | NORMALS
    assert missing(shim, FIT | NORMALS, "stage_sample") == FACTOR
    assert missing(shim, 0, "stage_score") == SAMPLES
    for event in ("stage_kde", "select_pixels"):
        assert missing(shim, STAGES & ~SCORES, event) == SCORES
    assert missing(shim, 0, "select_pixels_only") == 0
    # the converged fit overwrites the loop's fit: the factor stage refuses until final_cov or another fit
    have = run(shim, FINAL_FIT)
    assert missing(shim, have, "stage_factor") == FIT and missing(shim, run(shim, ["final_cov"], have), "stage_factor") == 0
    assert missing(shim, 0, "read_results") == RESULTS and missing(shim, 0, "read_last_fit") == LAST_FIT
    assert missing(shim, 0, "read_kept_ensemble") == ENS_KEPT and missing(shim, have, "read_results") == 0
