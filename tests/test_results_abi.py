"""CPU checks of the result records of the C ABI (include/gpet_hip.h, "Result records": gpet_result_bytes,
gpet_batch_results, gpet_gather_results): declared, exported, bound; the head's layout as a C compiler lays it out; the
record size; and the gfx950 code of k_finish_results (the interval rounds twice, as numpy does; y is rounded half to even)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gpet_result_bytes", "gpet_batch_results", "gpet_gather_results"]


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "gpet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gpet_[a-z0-9_]+)\s*\(", text)))


def _device_disassembly(tmp_path):
    """gfx950 disassembly of every code object in the shipped library (as tests/test_abi.py does it)."""
    import __graft_entry__ as ge
    ge.build()
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("no llvm-objdump")
    so = tmp_path / "lib.so"
    shutil.copy(ge.LIB, so)
    subprocess.run([objdump, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    text = []
    for f in sorted(os.listdir(tmp_path)):
        if "amdgcn" in f:
            text.append(subprocess.run([objdump, "-d", str(tmp_path / f)], check=True, capture_output=True, text=True).stdout)
    return "\n".join(text)


def test_result_calls_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_edge_trace_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _declared_symbols(), name
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS, name


def test_result_head_layout_matches_the_header(tmp_path):
    from gaussian_process_edge_trace_amd import _lib
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpet_hip.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(gpet_result_head), '
                    'offsetof(gpet_result_head, n_obs), offsetof(gpet_result_head, status), '
                    'offsetof(gpet_result_head, theta), offsetof(gpet_result_head, nlml));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    H = _lib.GpetResultHead
    assert got == [ctypes.sizeof(H), H.n_obs.offset, H.status.offset, H.theta.offset, H.nlml.offset]
    assert got[0] == 48


def test_result_bytes_is_the_documented_formula():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_edge_trace_amd import _lib
    lib = _lib.load()
    head = ctypes.sizeof(_lib.GpetResultHead)
    for L in [0, 1, 7, 64, 128, 1000]:
        n = ctypes.c_size_t()
        assert lib.gpet_result_bytes(L, ctypes.byref(n)) == _lib.OK
        # head | int64 trace[L][2] | f64 lower[L] | f64 upper[L]
        assert n.value == head + L * 2 * 8 + 2 * L * 8 == _lib.result_bytes(L)
    n = ctypes.c_size_t(12345)
    assert lib.gpet_result_bytes(-1, ctypes.byref(n)) == _lib.ERR_BAD_ARG
    assert n.value == 12345
    with pytest.raises(_lib.GpetError):
        _lib.result_bytes(-3)


def test_decode_reads_the_record_layout():
    """decode_results on a record written by hand in the documented layout."""
    import numpy as np
    from gaussian_process_edge_trace_amd import _lib
    L = 5
    rec = bytearray(_lib.result_bytes(L) * 2)
    for e in range(2):
        base = e * _lib.result_bytes(L)
        h = _lib.GpetResultHead.from_buffer(rec, base)
        h.edge_len, h.n_iter, h.n_obs, h.status = 3 + e, 10 + e, 20 + e, 0
        h.theta[:] = [0.5 + e, -1.0, 2.0]
        h.nlml = 7.25 + e
        tr = np.frombuffer(rec, dtype=np.int64, count=2 * L, offset=base + 48).reshape(L, 2)
        lo = np.frombuffer(rec, dtype=np.float64, count=L, offset=base + 48 + 16 * L)
        up = np.frombuffer(rec, dtype=np.float64, count=L, offset=base + 48 + 24 * L)
        tr[:3 + e] = [[y + e, 40 + y] for y in range(3 + e)]
        lo[:3 + e] = np.arange(3 + e) - 0.5
        up[:3 + e] = np.arange(3 + e) + 0.5
    d = _lib.decode_results(bytes(rec), 2, L)
    assert d["trace"].shape == (2, L, 2) and d["lower"].shape == (2, L) and d["theta"].shape == (2, 3)
    assert d["edge_len"].tolist() == [3, 4] and d["n_iter"].tolist() == [10, 11] and d["n_obs"].tolist() == [20, 21]
    assert d["nlml"].tolist() == [7.25, 8.25] and d["theta"][1].tolist() == [1.5, -1.0, 2.0]
    assert d["trace"][1, :4].tolist() == [[1, 40], [2, 41], [3, 42], [4, 43]] and not d["trace"][0, 3:].any()
    assert d["upper"][1, 3] == 3.5 and d["lower"][0, 4] == 0.0
    from gaussian_process_edge_trace_amd.gpet import results_from_records
    out, stats = results_from_records(d, True)
    assert out[0][0].shape == (3, 2) and out[1][1][0].shape == (4,) and stats["n_iter"].tolist() == [10, 11]


def test_isa_finish_kernel_rounds_like_numpy(tmp_path):
    """k_finish_results must reproduce the host's finish bit for bit: mean -/+ 1.96 std with two roundings each (a fused
    multiply-add would round once) and rint = round half to even (v_rndne_f64)."""
    dis = _device_disassembly(tmp_path)
    fns, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = fns.setdefault(m.group(1), []) if "k_finish_results" in m.group(1) else None
            continue
        if cur is not None and line.startswith("\t"):
            cur.append(line.strip().split(" ")[0])
    assert len(fns) == 1, list(fns)
    ops = next(iter(fns.values()))
    assert any(o.startswith("v_rndne_f64") for o in ops), ops
    assert not [o for o in ops if o.startswith(("v_fma_f64", "v_fmac_f64"))], ops
    assert any(o.startswith("v_mul_f64") for o in ops) and any(o.startswith("v_add_f64") for o in ops)
