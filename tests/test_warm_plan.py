"""CPU tests of the warm-start plan (csrc/gpet_warm_plan.h): the header needs no HIP, so a small extern "C" shim around it is compiled
with the host C++ compiler and driven through ctypes (as tests/test_ensemble_plan.py does).  It holds which edge -- or the consensus,
or nothing -- every edge of a batch takes the next frame's observations from, the refusals of the calls, and the size of the kept
ensemble; every expectation is a literal worked out by hand from include/gpet_hip.h, "seed ensembles in sequences"."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests.test_ensemble_plan import CSRC, _compiler

SHIM = r"""
#include "gpet_warm_plan.h"
using namespace gpet;
extern "C" {
int shim_const(int which) {
  return which == 0 ? GPET_WARM_MEDOID : which == 1 ? GPET_WARM_BEST_COST : which == 2 ? GPET_WARM_CONSENSUS : which == 3 ? WARM_SRC_NONE
                                                                                                             : WARM_SRC_CONSENSUS;
}
int shim_source(int e, int group, int n_members, int medoid, int best_cost, int from) {
  return warm_source(e, group, n_members, medoid, best_cost, from);
}
// heads: n_members, medoid, best_cost per group
void shim_sources(int B, const int* group_of, int G, const int* heads, int from, int* src) {
  std::vector<gpet_ensemble_head> h((size_t)G);
  for (int g = 0; g < G; ++g) {
    h[g] = gpet_ensemble_head{};
    h[g].n_members = heads[3 * g];
    h[g].medoid = heads[3 * g + 1];
    h[g].best_cost = heads[3 * g + 2];
  }
  warm_sources(B, group_of, h.data(), from, src);
}
long long shim_kept_bytes(int G, int B, long long len_cap) { return warm_kept_bytes(G, B, len_cap); }
long long shim_kept_group_off(int G, int B, long long len_cap) { return warm_kept_group_off(G, B, len_cap); }
long long shim_ensemble_bytes(int G, int B, long long len_cap) { return ensemble_layout(G, B, len_cap).total_bytes; }
int shim_groups_check(int from, int kept, char* msg, int cap) { return warm_groups_check(from, kept != 0, msg, (size_t)cap); }
int shim_from_check(int B, const int* src_of, const int* x_st, const int* x_en, char* msg, int cap) {
  return warm_from_check(B, src_of, x_st, x_en, msg, (size_t)cap);
}
}
"""
BAD_ARG = 1  # GPET_ERR_BAD_ARG


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("warm_plan")
    src, so = d / "shim.cpp", d / "libwarm_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    for f in (lib.shim_kept_bytes, lib.shim_kept_group_off, lib.shim_ensemble_bytes):
        f.restype = C.c_longlong
    return lib


def arr(v):
    return (C.c_int * max(1, len(v)))(*v)


def sources(shim, group_of, heads, frm):
    out = (C.c_int * len(group_of))()
    shim.shim_sources(len(group_of), arr(group_of), len(heads), arr([v for h in heads for v in h]), frm, out)
    return list(out)


def test_constants_are_the_headers_and_the_python_sides():
    import gaussian_process_edge_trace_amd._lib as L
    assert (L.WARM_MEDOID, L.WARM_BEST_COST, L.WARM_CONSENSUS, L.WARM_SRC_NONE, L.WARM_SRC_CONSENSUS) == (0, 1, 2, -1, -2)
    assert L.ERR_BAD_ARG == BAD_ARG
    for name in ("gpet_batch_ensemble_keep", "gpet_batch_ensemble_kept", "gpet_batch_warm_start_groups", "gpet_batch_warm_start_from"):
        assert name in L.SYMBOLS, name
    assert [L.warm_from(n) for n in ("medoid", "best_cost", "consensus", 0, 1, 2)] == [0, 1, 2, 0, 1, 2]
    for bad in ("median", None, 3, True):
        with pytest.raises(ValueError):
            L.warm_from(bad)


def test_constants(shim):
    assert [shim.shim_const(i) for i in range(5)] == [0, 1, 2, -1, -2]


def test_source_of_one_edge(shim):
    # in a group with members: the medoid, the best-cost member, the consensus -- whatever the edge is, member or not
    assert shim.shim_source(7, 2, 5, 9, 4, 0) == 9
    assert shim.shim_source(7, 2, 5, 9, 4, 1) == 4
    assert shim.shim_source(7, 2, 5, 9, 4, 2) == -2
    # an emptied group gives nothing, for every policy (its head says medoid = best_cost = -1)
    assert [shim.shim_source(7, 2, 0, -1, -1, f) for f in (0, 1, 2)] == [-1, -1, -1]
    # outside any group: the edge itself, for every policy
    assert [shim.shim_source(7, -1, 0, -1, -1, f) for f in (0, 1, 2)] == [7, 7, 7]
    assert shim.shim_source(0, -1, 3, 1, 2, 0) == 0


def test_source_table(shim):
    # groups: 0 = edges {0, 1, 2} (medoid 2, best cost 0), 1 = {4, 6} emptied, 2 = {5} alone; edges 3 and 7 in no group
    group_of = [0, 0, 0, -1, 1, 2, 1, -1]
    heads = [(3, 2, 0), (0, -1, -1), (1, 5, 5)]
    assert sources(shim, group_of, heads, 0) == [2, 2, 2, 3, -1, 5, -1, 7]
    assert sources(shim, group_of, heads, 1) == [0, 0, 0, 3, -1, 5, -1, 7]
    assert sources(shim, group_of, heads, 2) == [-2, -2, -2, 3, -1, -2, -1, 7]
    # a member the device stopped is no member (n_members 2 of 3 assigned) and still gets the group's source
    assert sources(shim, [0, 0, 0], [(2, 1, 2)], 0) == [1, 1, 1]
    # the Python side's restatement (what the tests of src_out compare with)
    import gaussian_process_edge_trace_amd._lib as L
    groups = [dict(medoid=m, best_cost=b) for _, m, b in heads]
    for f, name in enumerate(("medoid", "best_cost", "consensus")):
        assert L.warm_sources(group_of, groups, name).tolist() == sources(shim, group_of, heads, f)
        assert L.warm_sources(group_of, groups, name).dtype == np.int32


def test_kept_bytes(shim):
    # the buffer of gpet_batch_ensemble (tests/test_ensemble_plan.py: (3, 7, 70) -> 12784) with int32 group_of[B] padded to 8 behind it
    assert shim.shim_ensemble_bytes(3, 7, 70) == 12784
    assert shim.shim_kept_group_off(3, 7, 70) == 12784 and shim.shim_kept_bytes(3, 7, 70) == 12784 + 32
    assert shim.shim_kept_bytes(1, 1, 4) == 288 + 8 and shim.shim_kept_bytes(1, 2, 4) == 288 + 8 + 8
    assert shim.shim_kept_bytes(0, 7, 70) == 0 and shim.shim_kept_bytes(3, 0, 70) == 0 and shim.shim_kept_bytes(3, 7, 0) == 0


def check(fn, *args):
    msg = C.create_string_buffer(400)
    rc = fn(*args, msg, 400)
    return rc, msg.value.decode()


def test_group_form_refusals(shim):
    assert check(shim.shim_groups_check, 0, 1) == (0, "") and check(shim.shim_groups_check, 2, 1) == (0, "")
    rc, msg = check(shim.shim_groups_check, 1, 0)
    assert rc == BAD_ARG and msg.startswith("gpet_batch_warm_start_groups: no ensemble is kept") and "gpet_batch_ensemble_keep" in msg
    for frm in (-1, 3):
        rc, msg = check(shim.shim_groups_check, frm, 1)
        assert rc == BAD_ARG and msg.startswith("gpet_batch_warm_start_groups: from=%d is none of GPET_WARM_MEDOID" % frm)


def test_explicit_form_refusals(shim):
    x_st, x_en = [1, 1, 5, 5, 1], [70, 70, 44, 44, 69]
    ok = lambda src: check(shim.shim_from_check, 5, arr(src), arr(x_st), arr(x_en))
    assert ok([0, 1, 2, 3, 4]) == (0, "") and ok([1, 0, 3, 2, -1]) == (0, "") and ok([-1] * 5) == (0, "")
    rc, msg = ok([0, 5, 2, 3, 4])
    assert rc == BAD_ARG and msg == "gpet_batch_warm_start_from: edge 1: src_of=5 is outside [0, 5) (-1: no observations)"
    rc, msg = ok([0, 1, -2, 3, 4])
    assert rc == BAD_ARG and "edge 2: src_of=-2" in msg
    rc, msg = ok([0, 1, 2, 0, 4])  # another x_st
    assert rc == BAD_ARG and msg == "gpet_batch_warm_start_from: edge 3 spans columns 5..44, its source edge 0 spans 1..70"
    rc, msg = ok([4, 1, 2, 3, 4])  # the same x_st, another x_en
    assert rc == BAD_ARG and msg == "gpet_batch_warm_start_from: edge 0 spans columns 1..70, its source edge 4 spans 1..69"
    rc, msg = check(shim.shim_from_check, 0, arr([0]), arr([0]), arr([0]))
    assert rc == BAD_ARG and "bad argument" in msg
