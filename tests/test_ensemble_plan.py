"""CPU tests of the seed-ensemble plan (csrc/gpet_ensemble_plan.h): the header needs no HIP, so a small extern "C" shim around it is
compiled with the host C++ compiler and driven through ctypes (as tests/test_history_plan.py does).  Every expectation is a literal
worked out by hand from the documented layout (include/gpet_hip.h, "seed ensembles"):
  dst    = G records | f64 cost[B] | int32 off[B] padded to 8 bytes
  record = 32-byte head | int64 trace[len_cap][2] | 5 x f64 [len_cap] (median, q_lo, q_hi, min, max) | int32 agree[len_cap] padded to 8
and from the tile rule: the widest power of two <= 64 columns with n * cols * 8 bytes <= 32 KB, everything in LDS within 80 KB."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_edge_trace_amd", "csrc")

SHIM = r"""
#include "gpet_ensemble_plan.h"
using namespace gpet;
extern "C" {
// out: record_bytes, off_trace, off_median, off_q_lo, off_q_hi, off_min, off_max, off_agree, off_cost, off_off, total_bytes
void shim_layout(int G, int B, long long len_cap, long long* out) {
  const EnsembleLayout L = ensemble_layout(G, B, len_cap);
  out[0] = L.record_bytes; out[1] = L.off_trace; out[2] = L.off_median; out[3] = L.off_q_lo; out[4] = L.off_q_hi; out[5] = L.off_min;
  out[6] = L.off_max; out[7] = L.off_agree; out[8] = L.off_cost; out[9] = L.off_off; out[10] = L.total_bytes;
}
int shim_cols(int n) { return ensemble_tile_cols(n); }
long long shim_lds(int n, int cols) { return (long long)ensemble_lds_bytes(n, cols); }
int shim_const(int which) {
  return which == 0 ? ENSEMBLE_MAX : which == 1 ? ENSEMBLE_THREADS : which == 2 ? ENSEMBLE_COLS_MAX : which == 3 ? ENSEMBLE_TILE_BYTES
                                                                                                                 : ENSEMBLE_LDS_BUDGET;
}
int shim_head_bytes(void) { return (int)sizeof(gpet_ensemble_head); }
// the plan of a call; members / member_group / groups (n, x_st, len, member_off, cols, tiles per group) copied out; returns the status
int shim_plan(int G, int B, const int* group_of, const int* x_st, const int* x_en, const int* status, double tol, char* msg, int msg_cap,
              int* members, int* member_group, int* groups, int* n_wg, long long* lds) {
  EnsemblePlan P;
  const int rc = ensemble_plan(G, B, group_of, x_st, x_en, status, tol, &P, msg, (size_t)msg_cap);
  if (rc) return rc;
  for (size_t i = 0; i < P.members.size(); ++i) members[i] = P.members[i];
  for (int e = 0; e < B; ++e) member_group[e] = P.member_group[e];
  for (int g = 0; g < G; ++g) {
    const EnsembleGroup& Q = P.groups[g];
    const int v[6] = {Q.n, Q.x_st, Q.len, Q.member_off, Q.cols, Q.tiles};
    for (int k = 0; k < 6; ++k) groups[6 * g + k] = v[k];
    if ((1 << Q.log2_cols) != Q.cols) return -1;
  }
  *n_wg = (int)P.wg_group.size();
  for (size_t w = 0; w + 1 < P.wg_group.size(); ++w)
    if (P.wg_group[w] > P.wg_group[w + 1]) return -2;
  *lds = (long long)P.lds_bytes;
  return 0;
}
}
"""
KEYS = ("record_bytes", "off_trace", "off_median", "off_q_lo", "off_q_hi", "off_min", "off_max", "off_agree", "off_cost", "off_off",
        "total_bytes")


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
    d = tmp_path_factory.mktemp("ensemble_plan")
    src, so = d / "shim.cpp", d / "libensemble_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.shim_lds.restype = C.c_longlong
    return lib


def layout(shim, G, B, L):
    out = (C.c_longlong * 11)()
    shim.shim_layout(G, B, C.c_longlong(L), out)
    return dict(zip(KEYS, list(out)))


def plan(shim, group_of, x_st, x_en, status=None, tol=2.0, G=None):
    B = len(group_of)
    G = max(group_of) + 1 if G is None else G
    arr = lambda v: (C.c_int * max(1, len(v)))(*v)
    msg = C.create_string_buffer(256)
    members, member_group, groups = (C.c_int * (B + 1))(), (C.c_int * B)(), (C.c_int * (6 * max(G, 1)))()
    n_wg, lds = C.c_int(), C.c_longlong()
    rc = shim.shim_plan(G, B, arr(group_of), arr(x_st), arr(x_en), arr(status) if status is not None else None, C.c_double(tol), msg, 256,
                        members, member_group, groups, C.byref(n_wg), C.byref(lds))
    if rc:
        return rc, msg.value.decode()
    gs = [dict(zip(("n", "x_st", "len", "member_off", "cols", "tiles"), list(groups)[6 * g:6 * g + 6])) for g in range(G)]
    return 0, dict(groups=gs, members=list(members)[:sum(q["n"] for q in gs)], member_group=list(member_group), n_wg=n_wg.value,
                   lds=lds.value)


# (G, B, len_cap) -> record_bytes, total_bytes
SIZES = [
    # 32 + 4 * 16 + 5 * 32 + 16 = 272;  272 + 8 + 8
    ((1, 1, 4), 272, 288),
    # 32 + 70 * 16 + 5 * 560 + 280 = 4232;  3 * 4232 + 56 + 32 (28 -> 32)
    ((3, 7, 70), 4232, 12784),
    # 32 + 8000 + 20000 + 2000 = 30032;  60064 + 8192 + 4096
    ((2, 1024, 500), 30032, 72352),
]


@pytest.mark.parametrize("args,record,total", SIZES)
def test_record_and_total_sizes(shim, args, record, total):
    G, B, L = args
    p = layout(shim, *args)
    assert shim.shim_head_bytes() == 32 and p["off_trace"] == 32
    assert (p["record_bytes"], p["total_bytes"]) == (record, total)
    assert p["off_median"] == 32 + 16 * L
    assert [p[k] - p["off_median"] for k in ("off_q_lo", "off_q_hi", "off_min", "off_max", "off_agree")] == [8 * L * i for i in range(1, 6)]
    assert p["off_cost"] == G * record and p["off_off"] == G * record + 8 * B
    assert all(v % 8 == 0 for v in p.values())


@pytest.mark.parametrize("args", [(0, 1, 4), (1, 0, 4), (1, 1, 0), (1, 1, -3), (1, 1, (1 << 24) + 1)])
def test_bad_sizes_give_no_layout(shim, args):
    assert not any(layout(shim, *args).values())


@pytest.mark.parametrize("args", [s[0] for s in SIZES] + [(5, 33, 41)])
def test_python_mirror_equals_the_header(shim, args):
    from gaussian_process_edge_trace_amd import _lib
    assert _lib.ensemble_layout(*args) == layout(shim, *args)
    assert C.sizeof(_lib.GpetEnsembleHead) == 32 and _lib.ENSEMBLE_MAX == shim.shim_const(0)
    with pytest.raises(ValueError):
        _lib.ensemble_layout(0, 1, 4)


def test_tile_width_rule_against_the_lds_budget(shim):
    assert [shim.shim_const(i) for i in range(5)] == [1024, 256, 64, 32 * 1024, 80 * 1024]
    # n * cols * 8 <= 32 KB, widest power of two up to 64: 64 members are the last to keep 64 columns, 65 halve them
    assert [shim.shim_cols(n) for n in (1, 64, 65, 1024)] == [64, 64, 32, 4]
    assert [shim.shim_cols(n) for n in (0, 2, 128, 129, 256, 257, 512, 513)] == [64, 64, 32, 16, 16, 8, 8, 4]
    assert shim.shim_cols(1025) == 0 and shim.shim_cols(-1) == 0
    for n in (1, 2, 63, 64, 65, 128, 129, 300, 512, 513, 1000, 1024):
        cols = shim.shim_cols(n)
        assert n * cols * 8 <= 32 * 1024 and (cols == 64 or n * 2 * cols * 8 > 32 * 1024)
        # two copies of the tile, the consensus (f64) and the counts (int32) per column, a pointer and a count per member
        assert shim.shim_lds(n, cols) == 2 * n * cols * 8 + cols * 8 + n * 8 + cols * 4 + n * 4
        assert shim.shim_lds(n, cols) <= 80 * 1024  # two workgroups in a CU's 160 KB
    assert shim.shim_lds(64, 64) == 67072 and shim.shim_lds(1024, 4) == 77872 and 256 % shim.shim_cols(1024) == 0


def test_members_tables_and_tiles(shim):
    # interleaved membership, one edge in no group, one excluded by its status; group 1 is narrower (40 against 70 points)
    group_of = [0, 1, 0, -1, 1, 0, 1]
    x_st = [0, 5, 0, 0, 5, 0, 5]
    x_en = [69, 44, 69, 69, 44, 69, 44]
    status = [0, 0, 3, 0, 0, 0, 0]
    rc, p = plan(shim, group_of, x_st, x_en, status)
    assert rc == 0
    assert p["groups"] == [dict(n=2, x_st=0, len=70, member_off=0, cols=64, tiles=2), dict(n=3, x_st=5, len=40, member_off=2, cols=64, tiles=1)]
    assert p["members"] == [0, 5, 1, 4, 6] and p["member_group"] == [0, 1, -1, -1, 1, 0, 1]
    assert p["n_wg"] == 3 and p["lds"] == 2 * 3 * 64 * 8 + 64 * 8 + 3 * 8 + 64 * 4 + 3 * 4
    # a group emptied by its statuses: no members, no workgroups, still a record
    rc, p = plan(shim, [0, 1, 1], [0, 0, 0], [9, 9, 9], [0, 4, 8])
    assert rc == 0 and p["groups"][1] == dict(n=0, x_st=0, len=10, member_off=1, cols=64, tiles=0) and p["n_wg"] == 1
    assert p["members"] == [0] and p["member_group"] == [0, -1, -1]
    # 70 members: 32 columns a tile, 3 tiles over 70 points
    rc, p = plan(shim, [0] * 70, [2] * 70, [71] * 70)
    assert rc == 0 and p["groups"] == [dict(n=70, x_st=2, len=70, member_off=0, cols=32, tiles=3)] and p["members"] == list(range(70))


def test_every_validation_message(shim):
    ok = ([0, 0], [0, 0], [9, 9])
    assert plan(shim, *ok)[0] == 0
    rc, msg = plan(shim, [0, 2], [0, 0], [9, 9], G=2)
    assert rc == 1 and "group_of[1]=2 is outside [0, 2)" in msg
    rc, msg = plan(shim, [0, -2], [0, 0], [9, 9], G=1)
    assert rc == 1 and "group_of[1]=-2 is outside [0, 1)" in msg
    rc, msg = plan(shim, [0, 2, 2], [0, 0, 0], [9, 9, 9])
    assert rc == 1 and "group 1 of 3 has no edge" in msg
    rc, msg = plan(shim, [0, 1, 0, 1], [0, 0, 0, 0], [9, 9, 9, 8])
    assert rc == 1 and "group 1: edges 1 and 3 have different x-grids" in msg
    rc, msg = plan(shim, [0, 0], [0, 1], [9, 10])  # (the same length on other columns is a mismatch too)
    assert rc == 1 and "group 0: edges 0 and 1 have different x-grids" in msg
    rc, msg = plan(shim, [0, 0, 0], [0, 0, 0], [9, 9, 8], status=[0, 0, 5])  # (an excluded edge must fit its group as well)
    assert rc == 1 and "edges 0 and 2" in msg
    rc, msg = plan(shim, [0] * 1025, [0] * 1025, [9] * 1025)
    assert rc == 1 and "group 0 has 1025 members, more than 1024" in msg
    assert plan(shim, [0] * 1025, [0] * 1025, [9] * 1025, status=[0] * 1024 + [3])[0] == 0  # (1024 members and one excluded)
    rc, msg = plan(shim, *ok, tol=-0.5)
    assert rc == 1 and "tol=-0.5 is negative" in msg
    rc, msg = plan(shim, *ok, tol=float("nan"))
    assert rc == 1 and "tol" in msg
    assert plan(shim, *ok, tol=0.0)[0] == 0
    rc, msg = plan(shim, [], [], [], G=1)
    assert rc == 1 and "bad argument" in msg
