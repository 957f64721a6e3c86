"""CPU tests of the iteration history's layout (csrc/gpet_history_plan.h): the header needs no HIP, so a small extern "C" shim
around it is compiled with the host C++ compiler and driven through ctypes (as tests/test_loop_plan.py does).  Every expectation
is a literal worked out by hand from the documented layout (include/gpet_hip.h, "iteration history"):
  region = 16-byte edge head | iter_cap records;  record = 48-byte head | int32 obs[obs_cap][2] | f64 curve[len_cap] (level >= 2)
           | f64 mean[len_cap] | f64 std[len_cap] (level 3)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_edge_trace_amd", "csrc")

SHIM = r"""
#include "gpet_history_plan.h"
using namespace gpet;
extern "C" {
// out: level, iter_cap, obs_cap, len_cap, edge_bytes, record_bytes, off_records, off_obs, off_curve, off_mean, off_std
void shim_plan(int level, int iter_cap, int obs_cap, int len_cap, long long* out) {
  const gpet_history_plan p = history_plan(level, iter_cap, obs_cap, len_cap);
  out[0] = p.level; out[1] = p.iter_cap; out[2] = p.obs_cap; out[3] = p.len_cap; out[4] = p.edge_bytes; out[5] = p.record_bytes;
  out[6] = p.off_records; out[7] = p.off_obs; out[8] = p.off_curve; out[9] = p.off_mean; out[10] = p.off_std;
}
int shim_tiles(int level, int len_cap) { return history_tiles(level, len_cap); }
int shim_const(int which) { return which == 0 ? HISTORY_COLS : which == 1 ? HISTORY_WAVES : HISTORY_LEVEL_MAX; }
}
"""
KEYS = ("level", "iter_cap", "obs_cap", "len_cap", "edge_bytes", "record_bytes", "off_records", "off_obs", "off_curve", "off_mean",
        "off_std")


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
    d = tmp_path_factory.mktemp("history_plan")
    src, so = d / "shim.cpp", d / "libhistory_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    return C.CDLL(str(so))


def plan(shim, level, iter_cap, obs_cap, len_cap):
    out = (C.c_longlong * 11)()
    shim.shim_plan(level, iter_cap, obs_cap, len_cap, out)
    return dict(zip(KEYS, list(out)))


# (level, iter_cap, obs_cap, Lg_max) -> record_bytes, edge_bytes, off_curve, off_mean, off_std
CASES = [
    # 48 + 10 * 8 = 128;  16 + 4 * 128
    ((1, 4, 10, 23), 128, 528, 0, 0, 0),
    # 48 + 47 * 8 = 424 -> curve;  424 + 96 * 8 = 1192;  16 + 64 * 1192
    ((2, 64, 47, 96), 1192, 76304, 424, 0, 0),
    # 48 + 8 = 56 -> curve, 88 -> mean, 120 -> std, 152;  16 + 3 * 152
    ((3, 3, 1, 4), 152, 472, 56, 88, 120),
]


@pytest.mark.parametrize("args,record,edge,off_curve,off_mean,off_std", CASES)
def test_sizes_and_offsets(shim, args, record, edge, off_curve, off_mean, off_std):
    p = plan(shim, *args)
    assert (p["level"], p["iter_cap"], p["obs_cap"], p["len_cap"]) == args
    assert p["off_records"] == 16 and p["off_obs"] == 48
    assert (p["record_bytes"], p["edge_bytes"]) == (record, edge)
    assert (p["off_curve"], p["off_mean"], p["off_std"]) == (off_curve, off_mean, off_std)


@pytest.mark.parametrize("args", [c[0] for c in CASES] + [(3, 7, 13, 501), (2, 1, 3, 1)])
def test_f64_sections_are_8_byte_aligned_and_disjoint(shim, args):
    p = plan(shim, *args)
    level, iter_cap, obs_cap, len_cap = args
    assert p["off_records"] % 8 == 0 and p["record_bytes"] % 8 == 0 and p["edge_bytes"] % 8 == 0 and p["off_obs"] % 8 == 0
    ends = [(p["off_obs"], p["off_obs"] + 8 * obs_cap)]
    for need, key in ((2, "off_curve"), (3, "off_mean"), (3, "off_std")):
        if level >= need:
            assert p[key] % 8 == 0 and p[key] > 0
            ends.append((p[key], p[key] + 8 * len_cap))
        else:
            assert p[key] == 0  # the level has no such section
    for (a0, a1), (b0, b1) in zip(ends, ends[1:]):
        assert a1 == b0  # back to back, in the documented order
    assert ends[-1][1] == p["record_bytes"]
    assert p["edge_bytes"] == 16 + iter_cap * p["record_bytes"]


def test_level_1_allocates_no_curve_or_statistics(shim):
    p1, p2, p3 = (plan(shim, lv, 5, 9, 40) for lv in (1, 2, 3))
    assert p1["record_bytes"] == 48 + 72 and p1["off_curve"] == p1["off_mean"] == p1["off_std"] == 0
    assert p2["record_bytes"] - p1["record_bytes"] == 320 and p2["off_mean"] == p2["off_std"] == 0
    assert p3["record_bytes"] - p2["record_bytes"] == 640


@pytest.mark.parametrize("args", [(0, 4, 10, 23), (4, 4, 10, 23), (1, 0, 10, 23), (1, -1, 10, 23), (1, 4, 0, 23), (1, 4, 10, 0)])
def test_bad_arguments_give_no_layout(shim, args):
    assert not any(plan(shim, *args).values())


def test_workgroups_per_edge(shim):
    assert shim.shim_const(0) == 64 and shim.shim_const(2) == 3
    assert shim.shim_const(1) * 64 <= 1024  # one workgroup
    assert shim.shim_tiles(1, 500) == 1 and shim.shim_tiles(2, 500) == 1
    assert [shim.shim_tiles(3, n) for n in (1, 23, 64, 65, 96, 500, 512)] == [1, 1, 1, 2, 2, 8, 8]


@pytest.mark.parametrize("args", [c[0] for c in CASES] + [(3, 64, 52, 500)])
def test_python_mirror_equals_the_header(shim, args):
    from gaussian_process_edge_trace_amd import _lib
    q = _lib.history_plan(*args)
    assert {k: getattr(q, k) for k in KEYS} == plan(shim, *args)
    with pytest.raises(ValueError):
        _lib.history_plan(0, 1, 1, 1)
