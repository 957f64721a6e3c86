"""CPU tests of the launch rules of the eigen-factor stage (csrc/gpet_factor_plan.h): the header needs no HIP, so a small extern "C"
shim around it is compiled with the host C++ compiler and driven through ctypes (as tests/test_iter_plan.py does).  Every expectation
below is a literal, derived by hand from the rules as the launchers had them before they moved into the header (launch_factor and
launch_jacobi_small of csrc/gpet_k_launch.inc, launch_pchol_multi and launch_factor_big of csrc/gpet_eig.hip):

  pivoted Cholesky, capacity <= 96   multi-workgroup iff not the prior basis, Lg > 1024, pchol_multi != 0 and (pchol_multi == 1 or
                  ceil(Lg / 32) <= 64): `steps` = min(r_cap, Lg) blocks of accept ratio 0.1 (2) or steps (1); else k_pchol_reg (512
                  threads) iff Lg <= 512 and r_cap <= 96; else k_pchol, 1024 / 512 / 256 threads above 512 / 256 / 0 columns, (Lg + r_cap) * 8
  LDS Jacobi      m = rank rounded up to even, nblk = (m / 2)(m / 2 + 1) / 2, nbp = nblk rounded up to even; blocks per thread 2 iff
                  nblk <= 2 * workers (k_jacobi_seat 512, k_jacobi_ahead 448) else 3; LDS doubles: seat 4 nbp + m^2; ahead 8 nbp + 4, and
                  without a log + (m - nreg) m, nreg = min(42, m) rounded down to even with two blocks per thread, else 0
  pre-rotation    structured loop with jacobi_warm: NT = ceil(rank / 16) in 2 .. 6, 2 * mp * ld * 8 bytes, mp = 16 NT, ld = mp if
                  mp % 32 == 16 else mp + 16 -- and, NEW with the header, none where that exceeds 150 KB (NT = 6: 172 032)
  any rank        steps = min(r_cap, Lg), nblk = 2 ceil(steps / 16), nw = ceil(Lg / 32); pointers in the arguments iff a host edge table,
                  B <= 8 and oj_args; blocked Cholesky iff nw <= 64 and not pcx_one_pivot, 2 ceil(steps / min(nw, 16)) + 8 blocks, ratio 0;
                  warm start iff blocked, oj_warm and Lg <= r_cap; k_oj_round staged iff Lg <= 1024, oj_stage and slots = (nblk / 2) B
                  <= 256; half panels iff even widths, Lg > 512 and (oj_half_stage > 0 or (< 0 and slots > CUs)); panel 16 * (Lg up to a
                  multiple of 32, + 2) * 8, half 16 * 514 * 8; persistent iff stageable, oj_persist and slots <= 4 resident; workgroups per
                  edge nblk / 2, or max(resident / B, 1) where slots > resident

The shapes by which the GPU tests name the kernel they reach (tests/test_gpu_factor_injected.py, tests/test_gpu_configs.py) are held
against the header here as well, and the arena of tests/test_batch_plan.py's shapes against the buffers the plans' kernels index."""
import ctypes as C
import subprocess

import pytest

from tests import factor_exact as fx
from tests import test_batch_plan as bp

SHIM = bp.SHIM + r"""
#include "gpet_factor_plan.h"
static BatchDims dims_of(int Lg, int r_cap, int lg_even) { BatchDims bd{}; bd.Lg = Lg; bd.r_cap = r_cap; bd.lg_even = lg_even; return bd; }
static void put(int* o, const Grid3& g) { o[0] = g.x; o[1] = g.y; o[2] = g.z; }
static void put(int* o, const PcholMultiPlan& m) { o[0] = m.blocked; o[1] = m.nw; o[2] = m.steps; o[3] = m.nblocks; o[4] = (int)(m.accept * 10 + 0.5); }
extern "C" {
int shim_fconst(int i) {
  const int v[] = {PCH_R, JS_NT, JA_NT_LOG, JS_LOG_SWEEPS, PCX_COLS, PCB_NB, OJ_B, OJ_M, OJ_ARGS_MAXB, OJ_STAGE_MAX, OJ_LDS_ATTR, OJ_HALF_LD,
                   OJ_ROUND_STAGE_SLOTS, FACTOR_LDS_CAP, PCH_ONE_WG_MAX, LDS_DYN_MAX, PCB_NW_MAX, OJ_PERSIST_SLOTS_PER_WG, OJ_HALF_MIN, JA_RR,
                   PCX_CAND_PER_WG};
  return v[i];
}
// what the kernels call
long long shim_layout(int which, int a, int b) {
  switch (which) {
    case 0: return jac_players(a);
    case 1: return jac_blocks(a);
    case 2: return jac_plane_stride(a);
    case 3: return jac_reg_rows(a, b);
    case 4: return (long long)jac_seat_lds_doubles(a);
    case 5: return (long long)jac_ahead_lds_doubles(a, true, 0);
    case 6: return (long long)jac_ahead_lds_doubles(a, false, b);
    case 7: return prerot_ld(a);
    case 8: return (long long)prerot_lds_doubles(a);
    case 9: return oj_panel_stride(a, b != 0);
    case 10: return jac_ahead_copy_stride(a);
    default: return ojw_below(a, b);
  }
}
// o = {form (0 reg, 1 one workgroup, 2 multi), threads, blocked, nw, steps, nblocks, accept ratio in tenths, gram x y z, rows x y z, rows lds}
long long shim_pchol(int Lg, int r_cap, int B, int mode, int single_wg, int* o) {
  const FactorLdsPlan f = factor_lds_plan(dims_of(Lg, r_cap, 0), B, mode, single_wg != 0);
  const PcholPlan& p = f.pchol;
  o[0] = p.form == PcholForm::reg ? 0 : p.form == PcholForm::one_wg ? 1 : 2; o[1] = p.threads; put(o + 2, p.multi);
  put(o + 7, f.gram); put(o + 10, f.rows); o[13] = (int)f.rows_lds;
  return (long long)p.lds;
}
// o = {warm, prerot_nt, prerot_threads, prerot_lds, ahead, nu, rr, threads, log, wpass x y z}
long long shim_jacobi(int B, int rank_max, int scaled_out, int logw, int variant, int warm, int* o) {
  const JacobiSmallPlan p = jacobi_small_plan(B, rank_max, scaled_out != 0, logw != 0, variant, warm);
  o[0] = p.warm; o[1] = p.prerot_nt; o[2] = p.prerot_threads; o[3] = (int)p.prerot_lds; o[4] = p.ahead; o[5] = p.nu; o[6] = p.rr; o[7] = p.threads;
  o[8] = p.log; put(o + 9, p.wpass);
  return (long long)p.lds;
}
// opts = {oj_args, pcx_one_pivot, oj_warm, oj_stage, oj_half_stage, oj_persist};
// o = {use_args, steps, nblk, pchol (5), warm, warm_n, begin (3), tiles (3), lds_ok, round_staged, half_stage, persist, persist grid (3), round grid
//      (3), norms (3), order (3), rows (3)}; lds = {stage, persist}
void shim_big(int Lg, int r_cap, int lg_even, int B, int have_h, const int* opts, int n_cus, int resident, int* o, long long* lds) {
  const BatchDims bd = dims_of(Lg, r_cap, lg_even);
  const FactorBigOpts fo = {opts[0], opts[1], opts[2], opts[3], opts[4], opts[5]};
  const OjStagePlan s = oj_stage_plan(bd, B, fo, n_cus);
  const FactorBigPlan p = factor_big_plan(bd, B, have_h != 0, fo, s, resident);
  o[0] = p.use_args; o[1] = p.steps; o[2] = p.stage.nblk; put(o + 3, p.pchol); o[8] = p.warm; o[9] = p.warm_n; put(o + 10, p.warm_begin);
  put(o + 13, p.warm_tiles); o[16] = p.stage.lds_ok; o[17] = p.stage.round_staged; o[18] = p.stage.half_stage; o[19] = p.persist;
  put(o + 20, p.persist_grid); put(o + 23, p.round_grid); put(o + 26, p.norms); put(o + 29, p.order); put(o + 32, p.rows);
  lds[0] = (long long)p.stage.stage_lds; lds[1] = (long long)p.stage.persist_lds;
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = bp._compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("factor_plan")
    src, so = d / "shim.cpp", d / "libfactor_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", bp.CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    for name in ("shim_layout", "shim_pchol", "shim_jacobi"):
        getattr(lib, name).restype = C.c_longlong
    return lib


KB = 1024
LDS_DYN_MAX, OJ_LDS_ATTR = 150 * KB, 136 * KB


def pchol(shim, Lg, r_cap=96, mode=2, single=False, B=1):
    o = (C.c_int * 14)()
    lds = shim.shim_pchol(Lg, r_cap, B, mode, int(single), o)
    d = dict(form=("reg", "one_wg", "multi")[o[0]], threads=o[1], lds=lds, gram=tuple(o[7:10]), rows=tuple(o[10:13]), rows_lds=o[13])
    if d["form"] == "multi":
        d.update(blocked=bool(o[2]), nw=o[3], steps=o[4], nblocks=o[5], accept_tenths=o[6])
    return d


def jacobi(shim, rank_max, variant, log, scaled_out=False, warm=1, B=4):
    o = (C.c_int * 12)()
    lds = shim.shim_jacobi(B, rank_max, int(scaled_out), int(log), variant, warm, o)
    return dict(warm=o[0], prerot_nt=o[1], prerot_threads=o[2], prerot_lds=o[3], ahead=bool(o[4]), nu=o[5], rr=o[6], threads=o[7], log=bool(o[8]),
                wpass=tuple(o[9:12]), lds=lds)


def big(shim, Lg, r_cap=None, B=1, have_h=True, n_cus=256, resident=256, lg_even=None, **opts):
    ov = dict(oj_args=1, pcx_one_pivot=0, oj_warm=1, oj_stage=1, oj_half_stage=-1, oj_persist=1)
    assert set(opts) <= set(ov)
    ov.update(opts)
    o, lds = (C.c_int * 35)(), (C.c_longlong * 2)()
    shim.shim_big(Lg, Lg if r_cap is None else r_cap, int(Lg % 2 == 0 if lg_even is None else lg_even), B, int(have_h), (C.c_int * 6)(*ov.values()),
                  n_cus, resident, o, lds)
    return dict(use_args=bool(o[0]), steps=o[1], nblk=o[2], blocked=bool(o[3]), nw=o[4], pchol_steps=o[5], nblocks=o[6], accept_tenths=o[7],
                warm=bool(o[8]), warm_n=o[9], warm_begin=tuple(o[10:13]), warm_tiles=tuple(o[13:16]), lds_ok=bool(o[16]), round_staged=bool(o[17]),
                half_stage=bool(o[18]), persist=bool(o[19]), persist_grid=tuple(o[20:23]), round_grid=tuple(o[23:26]), norms=tuple(o[26:29]),
                order=tuple(o[29:32]), rows=tuple(o[32:35]), stage_lds=lds[0], persist_lds=lds[1])


def test_constants(shim):
    want = [96, 512, 512, 40, 32, 16, 8, 16, 8, 1024, 139264, 514, 256, 96, 1024, 153600, 64, 4, 512, 6, 16]
    assert [shim.shim_fconst(i) for i in range(len(want))] == want


# ---- layouts the kernels share with the plans ----

def test_layout_functions(shim):
    f = shim.shim_layout
    assert [f(0, r, 0) for r in (0, 1, 2, 41, 95, 96)] == [0, 2, 2, 42, 96, 96]                     # players
    assert [f(1, m, 0) for m in (2, 42, 82, 84, 88, 90, 96)] == [1, 231, 861, 903, 990, 1035, 1176]   # 2 x 2 blocks
    assert [f(2, n, 0) for n in (1, 231, 861, 1176)] == [2, 232, 862, 1176]                           # plane stride
    assert [f(10, n, 0) for n in (2, 862, 1176)] == [10, 3450, 4706]                                  # four planes + the dump slot
    # the register rows of k_jacobi_ahead<2, false, 6>: all of a padded rank up to 42, then 42; none without RR
    assert [f(3, 6, m) for m in (2, 40, 42, 44, 82)] == [2, 40, 42, 42, 42] and f(3, 0, 82) == 0
    assert f(4, 96, 0) * 8 == 111360 and f(5, 96, 0) * 8 == 75296 and f(6, 96, 0) * 8 == 149024 and f(6, 82, 6) * 8 == 81440
    assert [f(7, mp, 0) for mp in (32, 48, 64, 80, 96)] == [48, 48, 80, 80, 112]                      # = 16 mod 32
    assert [f(8, nt, 0) * 8 for nt in (2, 3, 4, 5, 6)] == [24576, 36864, 81920, 102400, 172032]
    assert [f(9, Lg, 0) for Lg in (97, 128, 129, 1024)] == [130, 130, 162, 1026] and f(9, 1024, 1) == 514 and f(9, 600, 1) == 514
    assert f(9, 1024, 0) * 16 * 8 == 131328 and f(9, 1024, 1) * 16 * 8 == 65792
    assert [f(11, 200, k0) for k0 in (0, 64, 128, 192)] == [3, 2, 1, 0] and f(11, 64, 0) == 0 and f(11, 65, 0) == 1


# ---- pivoted Cholesky of the LDS path ----

def test_pchol_one_workgroup_forms(shim):
    assert pchol(shim, 512)["form"] == "reg" and pchol(shim, 512)["threads"] == 512 and pchol(shim, 512)["lds"] == 0
    p = pchol(shim, 513)
    assert (p["form"], p["threads"], p["lds"]) == ("one_wg", 1024, 4872)          # (513 + 96) * 8
    assert pchol(shim, 4, r_cap=4)["form"] == "reg"
    # k_pchol's narrower workgroups: only a capacity above k_pchol_reg's 96 rows reaches them
    for Lg, threads in ((200, 256), (256, 256), (257, 512), (512, 512), (513, 1024), (1024, 1024)):
        p = pchol(shim, Lg, r_cap=97)
        assert (p["form"], p["threads"], p["lds"]) == ("one_wg", threads, (Lg + 97) * 8), Lg
    p = pchol(shim, 100, r_cap=90, B=3)
    assert (p["gram"], p["rows"], p["rows_lds"]) == ((6, 6, 3), (90, 3, 1), 720)


def test_pchol_multi_workgroup_from_1025_columns(shim):
    for mode in (0, 1, 2):
        p = pchol(shim, 1024, mode=mode)
        assert (p["form"], p["threads"], p["lds"]) == ("one_wg", 1024, 8960)
    assert pchol(shim, 1025, mode=0)["form"] == "one_wg"
    p = pchol(shim, 1025, mode=1)
    assert (p["form"], p["blocked"], p["nw"], p["steps"]) == ("multi", False, 33, 96)
    p = pchol(shim, 1025, mode=2)
    assert (p["form"], p["blocked"], p["nw"], p["steps"], p["nblocks"], p["accept_tenths"]) == ("multi", True, 33, 96, 96, 1)
    assert pchol(shim, 1025, r_cap=40, mode=2)["nblocks"] == 40
    # the blocked form's one wave looks at 64 workgroups' candidates at most
    assert pchol(shim, 2048, mode=2)["nw"] == 64 and pchol(shim, 2048, mode=2)["blocked"]
    p = pchol(shim, 2049, mode=2)
    assert (p["form"], p["threads"], p["lds"]) == ("one_wg", 1024, 17160)
    p = pchol(shim, 2049, mode=1)
    assert (p["form"], p["blocked"], p["nw"]) == ("multi", False, 65)
    # the prior eigenbasis stays on one workgroup whatever the width
    assert pchol(shim, 2048, mode=2, single=True)["form"] == "one_wg" and pchol(shim, 1025, mode=1, single=True)["form"] == "one_wg"


# ---- LDS Jacobi ----

@pytest.mark.parametrize("cap,nu,rr,lds", [(82, 2, 6, 81440), (84, 3, 0, 114336), (96, 3, 0, 149024), (40, 2, 6, 13472), (41, 2, 6, 14880),
                                           (42, 2, 6, 14880), (44, 2, 6, 16992)])
def test_jacobi_ahead_without_a_log(shim, cap, nu, rr, lds):
    """861 blocks at capacity 82 fit two per worker (896 slots), 903 at 84 do not; below a padded rank of 42 every row of W is a register
    row: (8 nbp + 4 + (m - nreg) m) * 8."""
    p = jacobi(shim, cap, 1, False)
    assert (p["ahead"], p["log"], p["nu"], p["rr"], p["threads"], p["lds"], p["wpass"]) == (True, False, nu, rr, 512, lds, (0, 0, 0))


@pytest.mark.parametrize("cap,nu,lds", [(82, 2, 55200), (84, 3, 57888), (96, 3, 75296), (2, 2, 160)])
def test_jacobi_ahead_with_a_log(shim, cap, nu, lds):
    p = jacobi(shim, cap, 1, True, B=4)
    assert (p["ahead"], p["log"], p["nu"], p["rr"], p["threads"], p["lds"]) == (True, True, nu, 0, 512, lds)
    assert p["wpass"] == ((cap + 3) // 4, 4, 1)


@pytest.mark.parametrize("cap,nu,lds", [(88, 2, 93632), (90, 3, 97952), (96, 3, 111360), (41, 2, 21536)])
def test_jacobi_seat(shim, cap, nu, lds):
    """990 blocks at capacity 88 fit two per thread (1 024 slots), 1 035 at 90 do not: (4 nbp + m^2) * 8."""
    for log in (False, True):
        p = jacobi(shim, cap, 0, log, B=2)
        assert (p["ahead"], p["log"], p["nu"], p["rr"], p["threads"], p["lds"]) == (False, log, nu, 0, 512, lds)
        assert p["wpass"] == (((cap + 3) // 4, 2, 1) if log else (0, 0, 0))


@pytest.mark.parametrize("rank,nt,lds", [(1, 2, 24576), (32, 2, 24576), (33, 3, 36864), (48, 3, 36864), (49, 4, 81920), (64, 4, 81920),
                                         (65, 5, 102400), (72, 5, 102400), (80, 5, 102400)])
def test_pre_rotation(shim, rank, nt, lds):
    p = jacobi(shim, rank, 1, False, scaled_out=True)
    assert (p["warm"], p["prerot_nt"], p["prerot_threads"], p["prerot_lds"]) == (1, nt, 64 * nt, lds)
    # only the structured loop, only with the option
    for q in (jacobi(shim, rank, 1, False, scaled_out=False), jacobi(shim, rank, 1, False, scaled_out=True, warm=0)):
        assert (q["warm"], q["prerot_nt"], q["prerot_threads"], q["prerot_lds"]) == (0, 0, 0, 0)


@pytest.mark.parametrize("rank", [81, 88, 95, 96])
def test_pre_rotation_that_cannot_launch_is_a_cold_start(shim, rank):
    """k_jacobi_prerot<6> would need 2 * 96 * 112 * 8 = 172 032 bytes: the plan is the one jacobi_warm = 0 gives."""
    for variant in (0, 1):
        for log in (False, True):
            assert jacobi(shim, rank, variant, log, scaled_out=True, warm=1) == jacobi(shim, rank, variant, log, scaled_out=True, warm=0)
    assert jacobi(shim, rank, 1, True, scaled_out=True)["warm"] == 0


def test_every_capacity_fits_its_kernel_and_the_lds(shim):
    for cap in range(2, 97):
        m = (cap + 1) // 2 * 2
        nblk = (m // 2) * (m // 2 + 1) // 2
        for variant in (0, 1):
            for log in (False, True):
                p = jacobi(shim, cap, variant, log, scaled_out=True, warm=1)
                workers = 512 - 64 if variant else 512
                assert nblk <= p["nu"] * workers, (cap, variant, log)      # the kernels' own guard (else GPET_ERR_RANK_CAP)
                assert p["nu"] == 2 or nblk > 2 * workers
                assert 0 < p["lds"] <= LDS_DYN_MAX, (cap, variant, log, p["lds"])
                assert (p["prerot_nt"] == 0) == (cap > 80) and p["warm"] == (1 if cap <= 80 else 0)
                assert p["prerot_lds"] <= LDS_DYN_MAX and (p["prerot_nt"] == 0 or 16 * p["prerot_nt"] >= cap)


# ---- any-rank factor ----

def test_any_rank_arguments_and_cholesky(shim):
    assert big(shim, 130, B=8)["use_args"] and not big(shim, 130, B=9)["use_args"]
    assert not big(shim, 130, B=8, have_h=False)["use_args"] and not big(shim, 130, B=8, oj_args=0)["use_args"]
    p = big(shim, 1024)
    assert (p["steps"], p["nblk"], p["blocked"], p["nw"], p["pchol_steps"], p["nblocks"], p["accept_tenths"]) == (1024, 128, True, 32, 1024, 136, 0)
    assert (p["norms"], p["order"], p["rows"], p["round_grid"]) == ((256, 1, 1), (4, 1, 1), (1024, 1, 1), (64, 1, 1))
    p = big(shim, 97, B=3)     # four 32-column workgroups offer four candidates a block: 2 * ceil(97 / 4) + 8
    assert (p["steps"], p["nblk"], p["nw"], p["nblocks"]) == (97, 14, 4, 58)
    assert (p["norms"], p["order"], p["rows"], p["round_grid"]) == ((25, 3, 1), (1, 3, 1), (97, 3, 1), (7, 3, 1))
    p = big(shim, 200, r_cap=136)
    assert (p["steps"], p["nblk"], p["nw"], p["nblocks"]) == (136, 18, 7, 48)
    assert not big(shim, 1024, pcx_one_pivot=1)["blocked"] and big(shim, 2048)["blocked"] and not big(shim, 2049)["blocked"]


def test_any_rank_warm_start_only_where_every_direction_is_kept(shim):
    p = big(shim, 200, B=2)
    assert (p["warm"], p["warm_n"], p["warm_begin"], p["warm_tiles"]) == (True, 200, (50, 2, 1), (4, 4, 2))
    assert not big(shim, 200, r_cap=136)["warm"] and not big(shim, 200, oj_warm=0)["warm"]
    assert not big(shim, 200, pcx_one_pivot=1)["warm"]     # (the launches stand between the BLOCKED Cholesky's init and its blocks)


def test_any_rank_round_kernel_stages_up_to_256_slots(shim):
    assert big(shim, 128, B=32)["round_staged"] and not big(shim, 128, B=33)["round_staged"]     # 8 pairs an edge
    assert big(shim, 1024, B=4)["round_staged"] and not big(shim, 1024, B=5)["round_staged"]     # 64
    assert not big(shim, 128, oj_stage=0)["round_staged"] and not big(shim, 128, oj_stage=0)["lds_ok"]
    p = big(shim, 1025)
    assert (p["lds_ok"], p["round_staged"], p["persist"]) == (False, False, False)
    assert big(shim, 1024)["stage_lds"] == 131328 and big(shim, 97)["stage_lds"] == 16640 and big(shim, 129)["stage_lds"] == 20736


def test_any_rank_half_staging(shim):
    """Only even widths above 512 columns; automatic only where a round has more pair slots than the device has CUs."""
    assert big(shim, 1024, B=5)["half_stage"] and big(shim, 1024, B=5)["persist_lds"] == 65792          # 320 slots
    assert not big(shim, 1024, B=4)["half_stage"] and big(shim, 1024, B=4)["persist_lds"] == 131328     # 256
    assert big(shim, 1024, B=1, n_cus=63)["half_stage"] and not big(shim, 1024, B=1, n_cus=64)["half_stage"]
    assert big(shim, 1024, oj_half_stage=1)["half_stage"] and not big(shim, 1024, B=8, oj_half_stage=0)["half_stage"]
    assert big(shim, 514, B=8)["half_stage"] and not big(shim, 514, B=7)["half_stage"]                 # 33 pairs an edge
    assert big(shim, 514, oj_half_stage=1)["half_stage"]
    for kw in (dict(Lg=512, B=40), dict(Lg=513, B=40), dict(Lg=1023, B=8), dict(Lg=1024, B=8, lg_even=False)):
        for half in (-1, 1):
            assert not big(shim, oj_half_stage=half, **kw)["half_stage"], kw


def test_any_rank_persistent_up_to_four_slots_per_resident_workgroup(shim):
    p = big(shim, 1024, resident=256)
    assert (p["persist"], p["persist_grid"]) == (True, (64, 1, 1))
    p = big(shim, 1024, B=8, oj_half_stage=0, resident=256)       # 512 slots on 256 resident workgroups: 32 an edge
    assert (p["persist"], p["persist_grid"]) == (True, (32, 8, 1))
    p = big(shim, 1024, B=8, resident=512)                         # half panels, two a CU: all 512 at once
    assert (p["half_stage"], p["persist"], p["persist_grid"]) == (True, True, (64, 8, 1))
    assert big(shim, 1024, B=16, resident=256)["persist"] and not big(shim, 1024, B=17, resident=256)["persist"]     # 1 024 | 1 088 slots
    assert not big(shim, 1024, oj_persist=0)["persist"] and not big(shim, 1024, oj_stage=0)["persist"]
    p = big(shim, 100, B=300, resident=600)                        # 7 pairs an edge: 2 100 slots, two workgroups an edge
    assert (p["persist"], p["persist_grid"]) == (True, (2, 300, 1))
    assert not big(shim, 100, B=300, resident=512)["persist"]
    p = big(shim, 40, B=300, resident=256)                         # more edges than resident workgroups: never fewer than one an edge
    assert (p["persist"], p["persist_grid"]) == (True, (1, 300, 1))


def test_every_staged_width_fits_the_attribute_limit(shim):
    for Lg in range(97, 1025):
        p = big(shim, Lg, oj_half_stage=1)
        assert p["lds_ok"] and 0 < p["stage_lds"] <= OJ_LDS_ATTR and 0 < p["persist_lds"] <= OJ_LDS_ATTR, Lg
        assert p["persist_lds"] == (65792 if Lg > 512 and Lg % 2 == 0 else p["stage_lds"])


# ---- the shapes by which the GPU tests name the kernel they reach ----

def test_shapes_of_the_injected_factor_tests(shim):
    """tests/test_gpu_factor_injected.py: "Paths"."""
    assert fx.LDS_CAPS == (40, 42, 44, 82, 84, 88, 90, 96)
    for cap in fx.LDS_CAPS:
        assert max(fx.lds_ranks(cap)) == cap and pchol(shim, 100, r_cap=cap)["form"] == "reg"
        for log in (False, True):
            assert jacobi(shim, cap, 1, log)["nu"] == (2 if cap <= 82 else 3)
            assert jacobi(shim, cap, 0, log)["nu"] == (2 if cap <= 88 else 3)
        assert jacobi(shim, cap, 1, False)["rr"] == (6 if cap <= 82 else 0)
    assert [shim.shim_layout(3, 6, cap) for cap in (40, 42, 44)] == [40, 42, 42]
    Lg, cap = max(m[0] for m in fx.MIXED), max(m[1] for m in fx.MIXED)
    assert (Lg, cap) == (97, 90) and pchol(shim, Lg, r_cap=cap)["form"] == "reg" and jacobi(shim, cap, 1, True)["nu"] == 3
    assert pchol(shim, 513)["form"] == "one_wg"
    assert [pchol(shim, 1030, mode=m)["form"] for m in (0, 1, 2)] == ["one_wg", "multi", "multi"]
    assert not pchol(shim, 1030, mode=1)["blocked"] and pchol(shim, 1030, mode=2)["blocked"] and pchol(shim, 1030, mode=2)["nw"] == 33
    for Lg, r in fx.BIG:
        assert Lg > 96 and r <= Lg
        p = big(shim, Lg)
        assert p["use_args"] and p["blocked"] and p["round_staged"] and p["persist"] and p["persist_grid"] == (p["nblk"] // 2, 1, 1)
        assert not big(shim, Lg, pcx_one_pivot=1)["blocked"] and not big(shim, Lg, oj_persist=0)["persist"]
        assert not big(shim, Lg, oj_stage=0)["round_staged"] and not big(shim, Lg, oj_args=0)["use_args"]
    p = big(shim, 200, B=9)                                                    # the batch of nine
    assert not p["use_args"] and p["persist"] and p["persist_grid"] == (13, 9, 1)


def test_shapes_of_the_half_panel_test(shim):
    """tests/test_gpu_configs.py::test_any_rank_jacobi_half_panel_staging_is_bit_identical on 256 CUs: one 1 024-column edge stages whole
    panels by default (one workgroup a CU), five edges half panels (two)."""
    p = big(shim, 1024, B=1, n_cus=256, resident=256)
    assert (p["half_stage"], p["persist"], p["persist_lds"], p["persist_grid"]) == (False, True, 131328, (64, 1, 1))
    p = big(shim, 1024, B=5, n_cus=256, resident=512)
    assert (p["half_stage"], p["persist"], p["persist_lds"], p["persist_grid"]) == (True, True, 65792, (64, 5, 1))
    for B, resident in ((1, 512), (5, 256)):     # the option set against the default: still one launch
        p = big(shim, 1024, B=B, oj_half_stage=int(B == 1), resident=resident)
        assert p["half_stage"] == (B == 1) and p["persist"]


# ---- the arena's buffers cover the plans ----

@pytest.mark.parametrize("name", list(bp.CASES))
def test_arena_covers_the_plans(shim, name):
    """pcx_cand holds 16 doubles -- two halves of a (value, index) pair per wave, four waves: what k_pcx_step indexes; k_pcb_block needs
    a quarter of it -- for every workgroup the plan launches, indexed with the batch's widest edge; Gt exists wherever the plan
    chooses a multi-workgroup Cholesky."""
    ps, M, N, share = bp.CASES[name][:4]
    p = bp.plan(shim, ps, M, N, share)
    bd = p["bd"]
    if bd["r_cap"] > 96:
        nws = [big(shim, bd["Lg"], r_cap=bd["r_cap"], B=len(ps), pcx_one_pivot=one)["nw"] for one in (0, 1)]
    else:
        plans = [pchol(shim, bd["Lg"], r_cap=bd["r_cap"], mode=mode, B=len(ps)) for mode in (0, 1, 2)]
        nws = [q["nw"] for q in plans if q["form"] == "multi"]
        assert bool(nws) == (bd["Lg"] > 1024)
    for E in p["edges"]:
        for nw in nws:
            assert nw == -(-bd["Lg"] // 32)
            assert E["off"]["jlog"] - E["off"]["pcx_cand"] >= 8 * 16 * nw, (name, nw)
            assert E["off"]["Ap"] - E["off"]["Gt"] >= 8 * E["Lg"] * E["r_cap"], name
