"""CPU checks of the iteration-history calls of the C ABI (include/gpet_hip.h, "iteration history"): declared, exported, bound;
the three structs as a C compiler lays them out against their ctypes mirrors (as tests/test_results_abi.py does for the result
record)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gpet_batch_set_history", "gpet_history_layout", "gpet_batch_history", "gpet_history_record"]


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "gpet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gpet_[a-z0-9_]+)\s*\(", text)))


def test_history_calls_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_edge_trace_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _declared_symbols(), name
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS, name
    assert _lib.SYMBOLS["gpet_history_layout"][1][1]._type_ is _lib.GpetHistoryPlan


STRUCTS = {
    "gpet_history_plan": ("GpetHistoryPlan", 72),
    "gpet_history_edge_head": ("GpetHistoryEdgeHead", 16),
    "gpet_history_head": ("GpetHistoryHead", 48),
}


def test_history_structs_match_the_header(tmp_path):
    from gaussian_process_edge_trace_amd import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gpet_hip.h"', 'int main(void){']
    want = []
    for cname, (pyname, size) in STRUCTS.items():
        T = getattr(_lib, pyname)
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(ctypes.sizeof(T))
        assert ctypes.sizeof(T) == size, cname
        for fname, _ in T._fields_:
            lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, fname))
            want.append(getattr(T, fname).offset)
    lines.append('return 0;}')
    prog, exe = tmp_path / "layout.c", tmp_path / "layout"
    prog.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want


def test_levels_by_name():
    from gaussian_process_edge_trace_amd import _lib
    import pytest
    assert [_lib.history_level(v) for v in (None, "obs", "curves", "full", 0, 3)] == [0, 1, 2, 3, 0, 3]
    for bad in ("all", 4, -1, True, 1.5):
        with pytest.raises(ValueError):
            _lib.history_level(bad)
