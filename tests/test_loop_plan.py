"""CPU tests of the device loop's scheduling decisions (csrc/gpet_loop_plan.h): the header needs no HIP, so a small extern "C"
shim around it is compiled with the host C++ compiler and driven through ctypes.  Every expectation below is a literal, derived by
hand from the rules INTEGRATION.md section 3b documents (look-ahead 8 up to 64 edges else 1, rng_inline 2 above 64 edges else 0,
refill at look-ahead - 2, head 4 for 2..32 edges, fused tail up to 64 edges) and from the loop as it stood before the split."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussian_process_edge_trace_amd", "csrc")

SHIM = r"""
#include "gpet_loop_plan.h"
using namespace gpet;
static LoopPlan plan_of(int B, int ring, const int* o) { return resolve_loop_plan(B, ring, o[0], o[1], o[2], o[3], o[4]); }
extern "C" {
// o = {rng_lookahead, rng_inline, rng_refill_at, rng_head, loop_fused_tail}; out = {look, deep, refill_at, head, fused_tail}
const char* shim_plan(int B, int ring, const int* o, int* out) {
  const LoopPlan p = plan_of(B, ring, o);
  out[0] = p.look; out[1] = p.deep; out[2] = p.refill_at; out[3] = p.head; out[4] = p.fused_tail;
  switch (p.mode) {
    case NormalsMode::inline_per_iteration: return "inline_per_iteration";
    case NormalsMode::inline_per_group: return "inline_per_group";
    case NormalsMode::side_deep: return "side_deep";
    case NormalsMode::side_shallow: return "side_shallow";
  }
  return "?";
}
int shim_head(int B, int ring, const int* o, int j, int cur, int B_l, int rng_mode, int n) {
  return head_iterations(plan_of(B, ring, o), j, cur, B_l, rng_mode, n);
}
int shim_next_group(int B, int group, int n_it, int active, const int* edges, int count) {  // edges: count x (done, n_obs, n_obs_prev, algo_thresh)
  static_assert(sizeof(EdgeProgress) == 4 * sizeof(int), "EdgeProgress is four ints");
  return next_group(B, group, n_it, active, reinterpret_cast<const EdgeProgress*>(edges), count);
}
}
"""
OPTS = ("rng_lookahead", "rng_inline", "rng_refill_at", "rng_head", "loop_fused_tail")
MT, PHILOX = 0, 1


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
    d = tmp_path_factory.mktemp("loop_plan")
    src, so = d / "shim.cpp", d / "libloop_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.shim_plan.restype = C.c_char_p
    return lib


def _opts(kw):
    assert set(kw) <= set(OPTS)
    return (C.c_int * 5)(*[kw.get(k, -1) for k in OPTS])


def plan(shim, B, ring, **kw):
    out = (C.c_int * 5)()
    mode = shim.shim_plan(B, ring, _opts(kw), out).decode()
    return dict(look=out[0], deep=bool(out[1]), mode=mode, refill_at=out[2], head=out[3], fused_tail=bool(out[4]))


def head(shim, B, ring, j=0, cur=0, B_l=None, rng_mode=MT, n=None, **kw):
    """head_iterations at a refill; n defaults to what the loop computes at (j, cur): min(ring - (j - cur), look)."""
    if n is None:
        n = min(ring - (j - cur), plan(shim, B, ring, **kw)["look"])
    return shim.shim_head(B, ring, _opts(kw), j, cur, B if B_l is None else B_l, rng_mode, n)


# B, ring, options, look, deep, mode, refill_at (None: the mode does not use it), head at (j=0, cur=0, B_l=B, MT19937)
PLAN_CASES = [
    (32, 16, {}, 8, True, "side_deep", 6, 4),
    (1, 16, {}, 8, True, "side_deep", 6, 0),      # one edge: no head
    (64, 16, {}, 8, True, "side_deep", 6, 0),     # more than 32 edges: no head
    (65, 9, {}, 1, False, "inline_per_group", None, 0),
    (1024, 9, {}, 1, False, "inline_per_group", None, 0),
    (1024, 9, dict(rng_lookahead=6), 6, True, "side_deep", 4, 0),
    (32, 16, dict(rng_lookahead=3), 3, False, "inline_per_group", None, 0),
    (32, 16, dict(rng_lookahead=3, rng_inline=0), 3, False, "side_shallow", None, 0),
    (32, 16, dict(rng_lookahead=0, rng_inline=0), 0, False, "side_shallow", None, 0),  # (waits on the pixel selection)
    (32, 2, {}, 1, True, "side_deep", 0, 0),      # n = 1: head <= n - 1
    (32, 16, dict(rng_head=8), 8, True, "side_deep", 6, 7),  # n = 8
    (32, 16, dict(rng_head=0), 8, True, "side_deep", 6, 0),
    (32, 16, dict(rng_refill_at=4), 8, True, "side_deep", 4, 4),
    (32, 16, dict(rng_inline=1), 8, True, "inline_per_iteration", None, 0),
    # the clamp to the ring comes after `deep` is judged and before the refill point is derived
    (32, 4, dict(rng_lookahead=15), 3, True, "side_deep", 1, 2),
    (32, 16, dict(rng_lookahead=4, rng_inline=0), 4, False, "side_shallow", None, 0),
    (32, 16, dict(rng_lookahead=5), 5, True, "side_deep", 3, 4),
    (32, 16, dict(rng_lookahead=2, rng_inline=2), 2, False, "inline_per_group", None, 0),
]


@pytest.mark.parametrize("B,ring,kw,look,deep,mode,refill_at,head0", PLAN_CASES)
def test_resolve_loop_plan(shim, B, ring, kw, look, deep, mode, refill_at, head0):
    p = plan(shim, B, ring, **kw)
    assert (p["look"], p["deep"], p["mode"]) == (look, deep, mode)
    if refill_at is not None:
        assert p["refill_at"] == refill_at
    # the head belongs to the deep side-stream mode: the loop asks for it nowhere else
    assert (head(shim, B, ring, **kw) if mode == "side_deep" else 0) == head0


def test_head_only_at_the_start_of_an_mt19937_trace_of_2_to_32_running_edges(shim):
    assert plan(shim, 32, 16)["head"] == 4 and plan(shim, 32, 16, rng_head=7)["head"] == 7
    assert head(shim, 32, 16) == 4
    assert head(shim, 32, 16, rng_mode=PHILOX) == 0
    assert head(shim, 32, 16, j=8, cur=2) == 0      # a later refill
    assert head(shim, 32, 16, j=3, cur=3) == 0      # a later call of the loop on the same trace
    assert head(shim, 64, 16, B_l=32) == 4          # the edges still RUNNING count ...
    assert head(shim, 32, 16, B_l=1) == 0           # ... on both ends
    assert head(shim, 2, 16) == 4 and head(shim, 33, 16) == 0
    assert head(shim, 32, 16, n=3) == 2 and head(shim, 32, 16, n=1) == 0 and head(shim, 32, 16, n=0) == 0


@pytest.mark.parametrize("opt,B,want", [(-1, 64, True), (-1, 65, False), (1, 1024, True), (0, 1, False), (-1, 1, True), (0, 1024, False)])
def test_fused_tail_wanted(shim, opt, B, want):
    assert plan(shim, B, 16 if B <= 64 else 9, loop_fused_tail=opt)["fused_tail"] is want


def next_group(shim, B, group, n_it, edges):
    """edges: (done, n_obs, n_obs_prev, algo_thresh) of every edge a batch of up to 64 passes; active is counted from them."""
    flat = [v for e in edges for v in e]
    active = sum(1 for e in edges if not e[0])
    return shim.shim_next_group(B, group, n_it, active, (C.c_int * max(1, len(flat)))(*flat), len(edges))


def test_next_group_ladder_above_64_edges(shim):
    def ladder(group, active, B=1024):
        return shim.shim_next_group(B, group, group, active, None, 0)
    assert ladder(8, 1024) == 4          # all edges running: 8, then 4 ...
    assert ladder(4, 1024) == 4
    assert ladder(8, 1000) == 2          # ... and 2 once the first have finished
    assert ladder(2, 1024) == 2          # (never back up)
    assert ladder(4, 1, B=65) == 2
    assert ladder(2, 0) == 0             # all done: the caller stops


def test_next_group_follows_the_observation_growth_up_to_64_edges(shim):
    RUN, DONE = 0, 1
    assert next_group(shim, 1, 8, 8, [(RUN, 30, 6, 39)]) == 3      # gained 24 in 8 iterations = 3 per iteration, needs 9 more
    assert next_group(shim, 1, 8, 8, [(RUN, 30, 6, 130)]) == 8     # needs 100 more: capped at 8
    assert next_group(shim, 1, 8, 8, [(RUN, 30, 6, 40)]) == 4      # 10 / 3 rounds up
    assert next_group(shim, 1, 8, 8, [(RUN, 30, 30, 35)]) == 5     # gained nothing: rate 1
    assert next_group(shim, 1, 8, 8, [(RUN, 30, 33, 35)]) == 5     # (nor does a loss count as a rate)
    assert next_group(shim, 1, 3, 3, [(RUN, 36, 30, 37)]) == 1     # at least one iteration
    assert next_group(shim, 1, 8, 8, [(RUN, 40, 16, 39)]) == 1     # (a running edge at its threshold still gets one)
    assert next_group(shim, 1, 8, 5, [(RUN, 30, 20, 39)]) == 5     # the rate is per iteration RUN (5 of a group of 8): 2, so ceil(9 / 2)
    # the slowest RUNNING edge decides; finished edges are ignored whatever they would need
    assert next_group(shim, 3, 8, 8, [(RUN, 30, 6, 36), (DONE, 10, 10, 500), (RUN, 20, 4, 30)]) == 5
    assert next_group(shim, 64, 8, 8, [(DONE, 40, 30, 40)] * 63 + [(RUN, 32, 16, 40)]) == 4
    assert next_group(shim, 2, 8, 8, [(DONE, 40, 30, 40), (DONE, 41, 30, 40)]) == 0   # all done: the caller stops
