"""Host tests of the register form of the fused curve KDE (csrc/gpet_k_kde_pix.inc: k_kde_fused_r; csrc/gpet_iter_plan.h:
kde_reg_plan), no GPU needed.

(a) kde_reg_plan against literals, through a shim compiled with the host C++ compiler (as tests/test_iter_plan.py does for
    kde_fused_plan): 27 328 B = (24 * 137 + 128) * 8 of dynamic LDS, the grid of kde_fused_plan, and where the form applies --
    at most 128 kept curves anywhere in the batch, a padded grid of at least 128 cells (it lends the weights their space), option
    kde_variant != 0.
(b) the gfx950 code object of the shipped library (as tests/test_raw_frames_host.py::test_batched_kernels_use_no_scratch reads
    it): k_kde_fused_r has no private segment, no spilled register and at most 64 vector registers -- what eight waves per SIMD,
    four workgroups of eight waves per CU, allow -- and four times its LDS, static and dynamic, fit the CU's 160 KB.  The staged
    form k_kde_fused is the yardstick: found, no scratch either."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from tests.test_iter_plan import CSRC, DIMS, _compiler

SHIM = r"""
#include "gpet_iter_plan.h"
using namespace gpet;
static_assert(sizeof(BatchDims) == 18 * sizeof(int), "BatchDims is eighteen ints");
extern "C" long long shim_kde_reg(const int* d, int B, int variant, int* o) {
  const KdeRegPlan p = kde_reg_plan(*reinterpret_cast<const BatchDims*>(d), B, variant);
  o[0] = p.applies; o[1] = p.grid.x; o[2] = p.grid.y; o[3] = p.grid.z;
  return (long long)p.lds;
}
extern "C" int shim_threads() { return KDE_THREADS; }
"""

LDS_PER_CU = 160 * 1024
REG_LDS = 27328  # (24 * 137 + 128) * 8


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("kde_reg_plan")
    src, so = d / "shim.cpp", d / "libkde_reg_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.shim_kde_reg.restype = C.c_longlong
    return lib


def plan(shim, B=1, variant=1, **kw):
    d = (C.c_int * len(DIMS))(*[kw.get(k, 0) for k in DIMS])
    o = (C.c_int * 4)()
    lds = shim.shim_kde_reg(d, B, variant, o)
    return bool(o[0]), tuple(o[1:]), lds


def test_kde_reg_plan_against_literals(shim):
    assert shim.shim_threads() == 512
    assert plan(shim, B=7, M=500, N=500, n_keep=100) == (True, (32, 7, 1), REG_LDS)
    assert plan(shim, M=500, N=512, n_keep=128) == (True, (32, 1, 1), REG_LDS)
    assert plan(shim, M=24, N=37, n_keep=1) == (True, (3, 1, 1), REG_LDS)
    # more curves than one staging pass, the cross-check, a grid of fewer than 128 cells: the staged form
    assert plan(shim, M=500, N=513, n_keep=129) == (False, (33, 1, 1), REG_LDS)
    assert plan(shim, variant=0, M=500, N=500, n_keep=100)[0] is False
    assert plan(shim, M=6, N=14, n_keep=3)[0] is True       # 8 * 16 = 128 cells
    assert plan(shim, M=6, N=13, n_keep=3)[0] is False      # 8 * 15 = 120


def _kernel_notes(tmp_path):
    """{kernel name: {metadata key: int}} for the fused curve KDE's kernels in the gfx950 code objects of the shipped library."""
    import __graft_entry__ as ge
    ge.build()
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("no llvm-objdump / llvm-readelf")
    so = tmp_path / "lib.so"
    shutil.copy(ge.LIB, so)
    subprocess.run([objdump, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    found = {}
    for f in sorted(os.listdir(tmp_path)):
        if "amdgcn" not in f:
            continue
        notes = subprocess.run([readelf, "--notes", str(tmp_path / f)], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:  # one block per kernel; .agpr_count is its first key
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and "k_kde_fused" in name.group(1):
                found[name.group(1)] = {k: int(v) for k, v in re.findall(
                    r"\.(private_segment_fixed_size|group_segment_fixed_size|sgpr_spill_count|vgpr_spill_count|vgpr_count|"
                    r"max_flat_workgroup_size):\s+(\d+)", block)}
    return found


def test_register_form_fits_four_workgroups_per_cu(tmp_path):
    found = _kernel_notes(tmp_path)
    reg = [u for n, u in found.items() if "k_kde_fused_r" in n]
    staged = [u for n, u in found.items() if "k_kde_fused_r" not in n]
    assert len(reg) == 1 and len(staged) == 1, sorted(found)
    for use in reg + staged:
        assert use["private_segment_fixed_size"] == 0 and use["sgpr_spill_count"] == 0 and use["vgpr_spill_count"] == 0, use
        assert use["max_flat_workgroup_size"] == 512, use
    use = reg[0]
    print("k_kde_fused_r: %d vector registers, %d B static LDS; k_kde_fused: %d, %d B"
          % (use["vgpr_count"], use["group_segment_fixed_size"], staged[0]["vgpr_count"], staged[0]["group_segment_fixed_size"]))
    assert 0 < use["vgpr_count"] <= 64, use
    assert 4 * (REG_LDS + use["group_segment_fixed_size"]) <= LDS_PER_CU, use
