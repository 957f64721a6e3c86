"""CPU tests of the label-map rules in csrc/gpet_label_plan.h (the header needs no HIP: a small extern "C" shim around it is compiled with
the host C++ compiler and -ffp-contract=off, as tests/test_polar_plan.py does), of the words of its refusals as _lib repeats them, and of
the ABI surface of the label-map calls.

The expected values come from tests/label_ref.py, the rules restated with numpy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import label_ref as R
from tests.test_denoise_plan import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_process_edge_trace_amd", "csrc")
CALLS = ("gpet_label_maps", "gpet_label_maps_xy", "gpet_batch_label_maps", "gpet_batch_label_maps_xy", "gpet_label_thick_count")


# ---- ABI surface ---------------------------------------------------------------------------------------------------------------
def test_the_calls_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from gaussian_process_edge_trace_amd import _lib
    header = open(os.path.join(ROOT, "include", "gpet_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(gpet_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(_lib.LIB_PATH)
    for name in CALLS:
        assert name in declared and hasattr(lib, name) and name in _lib.SYMBOLS, name
    assert [len(_lib.SYMBOLS[n][1]) for n in CALLS] == [12, 10, 6, 8, 4]
    for line in ("#define GPET_LABELS_EXTEND 1u\n", "#define GPET_LABELS_TRANSPOSED 2u\n", "#define GPET_LABELS_OUT_ON_DEVICE 4u\n",
                 "#define GPET_LABEL_EDGES_MAX 32\n", "#define GPET_LABEL_VERTS_MAX 4096\n", "#define GPET_LABEL_NO_ROW INT64_MIN\n",
                 "#define GPET_ABI_VERSION 1\n"):
        assert line in header, line
    assert (_lib.LABELS_EXTEND, _lib.LABELS_TRANSPOSED, _lib.LABELS_OUT_ON_DEVICE) == (1, 2, 4)
    assert (_lib.LABEL_EDGES_MAX, _lib.LABEL_VERTS_MAX, _lib.LABEL_NO_ROW) == (32, 4096, -(1 << 63)) and R.NO_ROW == _lib.LABEL_NO_ROW
    assert hasattr(_lib.Context, "label_maps") and hasattr(_lib.Context, "label_maps_xy")
    assert hasattr(_lib.Batch, "label_maps") and hasattr(_lib.Batch, "label_maps_xy")
    assert '#include "gpet_k_label.inc"' in open(os.path.join(CSRC, "gpet_kernels.hip")).read()
    assert "gpet_api_label.hip" in ge.HIP_SOURCES
    import gaussian_process_edge_trace_amd as pkg
    assert hasattr(pkg.gpet_utils, "label_maps") and hasattr(pkg.gpet_utils, "outline_label_maps")
    assert hasattr(pkg.GP_Edge_Tracing_Batch, "label_maps")


def test_thick_count_through_the_library():
    from gaussian_process_edge_trace_amd import _lib
    lib = _lib.load()
    assert _lib.label_thick_count(3, 2, 10) == 90 and _lib.label_thick_count(1, 32, 1) == 33
    n = C.c_int64(-1)
    for bad in ((0, 1, 5), (1, 0, 5), (1, 33, 5), (1, 1, 0)):
        assert lib.gpet_label_thick_count(*bad, C.byref(n)) == _lib.ERR_BAD_ARG and n.value == -1
    assert lib.gpet_label_thick_count(1, 1, 1, None) == _lib.ERR_BAD_ARG
    with pytest.raises(ValueError):
        _lib.label_thick_count(1, 33, 5)


# ---- the header through a host-compiled shim -------------------------------------------------------------------------------------
SHIM = r"""
#include "gpet_label_plan.h"
#include <vector>
using namespace gpet;
static char g_msg[256];
extern "C" {
long long shim_no_row() { return LABEL_NO_ROW; }
void shim_limits(int* out) { out[0] = LABEL_EDGES_MAX; out[1] = LABEL_VERTS_MIN; out[2] = LABEL_VERTS_MAX; out[3] = LABEL_CHUNK; out[4] = LABEL_SPAN;
                             out[5] = LABEL_LDS_INTS; }
long long shim_col_index(long long c, long long x_st, long long len, int extend) { return label_col_index(c, x_st, len, extend != 0); }
int shim_clamp(long long t, int M) { return label_clamp(t, M); }
// T [n_edges][N]
void shim_thresholds(int M, int N, int n_edges, const int32_t* x_st, const int32_t* len, const long long* rows, int extend, int* T) {
  size_t off = 0;
  for (int e = 0; e < n_edges; ++e) {
    for (int c = 0; c < N; ++c) T[(size_t)e * N + c] = label_threshold(rows + off, x_st[e], len[e], c, M, extend != 0);
    off += (size_t)len[e];
  }
}
// the maps [n_maps][M][N] and thick [n_maps][L + 1][N] from the member table and label_count, as the kernels put them together
int shim_row_maps(int M, int N, int n_edges, const int32_t* x_st, const int32_t* len, const long long* rows, const int32_t* map_of, int n_maps,
                  int extend, unsigned char* out, int L, int* thick) {
  std::vector<int> Tall((size_t)n_edges * N);
  shim_thresholds(M, N, n_edges, x_st, len, rows, extend, Tall.data());
  std::vector<int32_t> used((size_t)n_edges + 1), map_off((size_t)n_maps + 1);
  const int k = label_map_table(n_edges, map_of, n_maps, used.data(), map_off.data());
  std::vector<int> T((size_t)k * N + 1);
  for (int u = 0; u < k; ++u)
    for (int c = 0; c < N; ++c) T[(size_t)u * N + c] = Tall[(size_t)used[u] * N + c];
  for (int f = 0; f < n_maps; ++f) {
    const int e0 = map_off[f], n = map_off[f + 1] - e0;
    for (int r = 0; r < M; ++r)
      for (int c = 0; c < N; ++c) {
        const int v = label_count(T.data() + (size_t)e0 * N + c, n, (size_t)N, r);
        out[((size_t)f * M + r) * N + c] = (unsigned char)v;
        if (thick) thick[((size_t)f * (L + 1) + v) * N + c] += 1;
      }
  }
  return k;
}
int shim_crossing(double px, double py, double xi, double yi, double xj, double yj) { return label_crossing(px, py, xi, yi, xj, yj) ? 1 : 0; }
void shim_inside(int Ms, int Ns, const double* xy, int n, unsigned char* out) {
  for (int y = 0; y < Ms; ++y)
    for (int x = 0; x < Ns; ++x) out[(size_t)y * Ns + x] = label_inside((double)x, (double)y, xy, n) ? 1 : 0;
}
void shim_vertex(long long t, double r0, double dr, double cx, double cy, double ct, double st, double* xy) {
  label_vertex(t, r0, dr, cx, cy, ct, st, xy, xy + 1);
}
long long shim_thick_count(long long n_maps, long long L, long long N) { return label_thick_count(n_maps, L, N); }
int shim_stage_cols(int M, int N, int tr) { return label_stage_cols(M, N, tr != 0); }
int shim_stage_edges(int cols, int L) { return label_stage_edges(cols, L); }
unsigned int shim_blocks(long long bytes, int mis) { return label_blocks(bytes, mis); }
const char* shim_check(long long M, long long N, int n_edges, const int32_t* x_st, const int32_t* len, int rows_null, const int32_t* map_of,
                       int n_maps, int out_null, int* L) {
  g_msg[0] = 0;
  return label_check(M, N, n_edges, x_st, len, rows_null != 0, map_of, n_maps, out_null != 0, L, g_msg, sizeof g_msg) ? g_msg : nullptr;
}
const char* shim_check_xy(long long Ms, long long Ns, int n, const int32_t* n_vert, int xy_null, const int32_t* map_of, int n_maps, int out_null,
                          int* L) {
  g_msg[0] = 0;
  return label_check_xy(Ms, Ns, n, n_vert, xy_null != 0, map_of, n_maps, out_null != 0, L, g_msg, sizeof g_msg) ? g_msg : nullptr;
}
const char* shim_check_closed(int e, int x_st, int x_en, int pad, int n_theta) {
  g_msg[0] = 0;
  return label_check_closed(e, x_st, x_en, pad, n_theta, g_msg, sizeof g_msg) ? g_msg : nullptr;
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("label_plan")
    src, so = d / "shim.cpp", d / "liblabel_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    I, D, LL, IP, P = C.c_int, C.c_double, C.c_longlong, C.POINTER(C.c_int32), C.c_void_p
    lib.shim_no_row.restype = LL
    lib.shim_limits.argtypes = [P]
    lib.shim_col_index.restype, lib.shim_col_index.argtypes = LL, [LL, LL, LL, I]
    lib.shim_clamp.restype, lib.shim_clamp.argtypes = I, [LL, I]
    lib.shim_thresholds.restype, lib.shim_thresholds.argtypes = None, [I, I, I, P, P, P, I, P]
    lib.shim_row_maps.restype, lib.shim_row_maps.argtypes = I, [I, I, I, P, P, P, P, I, I, P, I, P]
    lib.shim_crossing.restype, lib.shim_crossing.argtypes = I, [D] * 6
    lib.shim_inside.restype, lib.shim_inside.argtypes = None, [I, I, P, I, P]
    lib.shim_vertex.restype, lib.shim_vertex.argtypes = None, [LL, D, D, D, D, D, D, P]
    lib.shim_thick_count.restype, lib.shim_thick_count.argtypes = LL, [LL, LL, LL]
    lib.shim_stage_cols.restype, lib.shim_stage_cols.argtypes = I, [I, I, I]
    lib.shim_stage_edges.restype, lib.shim_stage_edges.argtypes = I, [I, I]
    lib.shim_blocks.restype, lib.shim_blocks.argtypes = C.c_uint, [LL, I]
    lib.shim_check.restype, lib.shim_check.argtypes = C.c_char_p, [LL, LL, I, P, P, I, P, I, I, P]
    lib.shim_check_xy.restype, lib.shim_check_xy.argtypes = C.c_char_p, [LL, LL, I, P, I, P, I, I, P]
    lib.shim_check_closed.restype, lib.shim_check_closed.argtypes = C.c_char_p, [I, I, I, I, I]
    return lib


def i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def edges_case(seed, M, N, n_edges, full=False):
    """x_st, rows per edge -- grids inside [0, N), rows from below 0 to above M, NO_ROW here and there."""
    rng = np.random.default_rng(seed)
    x_st, rows = [], []
    for e in range(n_edges):
        x0 = 0 if full else int(rng.integers(0, N - 1))
        n = N if full else int(rng.integers(1, N - x0 + 1))
        t = rng.integers(-3, M + 4, size=n).astype(np.int64)
        t[rng.random(n) < 0.1] = R.NO_ROW
        x_st.append(x0)
        rows.append(t)
    return x_st, rows


def test_constants_and_launch_shapes(shim):
    lim = (C.c_int * 6)()
    shim.shim_limits(lim)
    assert list(lim) == [32, 4, 4096, 16, 4096, 12288] and shim.shim_no_row() == R.NO_ROW == np.iinfo(np.int64).min
    # a row-major map stages min(N, span) columns, a transposed one span / M + 2 (never more than N)
    assert [shim.shim_stage_cols(33, n, 0) for n in (2, 500, 4096, 5000)] == [2, 500, 4096, 4096]
    assert [shim.shim_stage_cols(m, 500, 1) for m in (2, 64, 500, 5000)] == [500, 66, 10, 2]
    # as many edges per pass as 48 KB of thresholds hold, at least 1, at most L
    assert [shim.shim_stage_edges(c, 32) for c in (2, 500, 4096, 20000)] == [32, 24, 3, 1] and shim.shim_stage_edges(500, 2) == 2
    # a destination that starts `mis` bytes past a 16-byte boundary needs the blocks of mis more bytes
    assert [shim.shim_blocks(b, m) for b, m in ((4, 0), (4096, 0), (4096, 1), (4097, 15), (1 << 31, 15))] == [1, 1, 2, 2, (1 << 19) + 1]
    for args in ((3, 2, 10), (1, 32, 1), (0, 1, 5), (1, 33, 5), (1, 1, 0), (256, 2, 500)):
        want = args[0] * (args[1] + 1) * args[2] if args[0] >= 1 and 1 <= args[1] <= 32 and args[2] >= 1 else 0
        assert shim.shim_thick_count(*args) == want


def test_column_index_and_clamp(shim):
    # grid [5, 9]: inside, left, right; extend takes the ends
    assert [shim.shim_col_index(c, 5, 5, 0) for c in (4, 5, 9, 10)] == [-1, 0, 4, -1]
    assert [shim.shim_col_index(c, 5, 5, 1) for c in (0, 4, 5, 9, 10, 99)] == [0, 0, 0, 4, 4, 4]
    M = 7
    assert [shim.shim_clamp(t, M) for t in (-(1 << 62), -1, 0, 3, 6, 7, 8, 1 << 62)] == [0, 0, 0, 3, 6, 7, 7, 7]
    assert shim.shim_clamp(R.NO_ROW, M) == M and shim.shim_clamp(R.NO_ROW + 1, M) == 0


@pytest.mark.parametrize("extend", [0, 1])
@pytest.mark.parametrize("shape", [(2, 2), (5, 7), (33, 64), (3, 17)])
def test_thresholds_equal_the_restated_rule(shim, shape, extend):
    M, N = shape
    x_st, rows = edges_case(11 + M + N, M, N, 6)
    x_st[0], rows[0] = 0, np.array([-1, 0, M - 1, M, M + 1, R.NO_ROW][:N] + [1] * max(0, N - 6), dtype=np.int64)[:N]  # a full grid with every special row
    flat = np.concatenate(rows)
    T = np.full((6, N), -7, dtype=np.int32)
    shim.shim_thresholds(M, N, 6, i32(x_st).ctypes.data_as(C.c_void_p), i32([len(r) for r in rows]).ctypes.data_as(C.c_void_p), flat.ctypes.data_as(C.c_void_p), extend, T.ctypes.data_as(C.c_void_p))
    want = R.thresholds(M, N, x_st, rows, bool(extend))
    assert np.array_equal(T, want) and T.min() >= 0 and T.max() <= M
    if not extend:  # a column outside the grid does not count
        for e in range(6):
            out = np.ones(N, dtype=bool)
            out[x_st[e]:x_st[e] + len(rows[e])] = False
            assert np.all(T[e][out] == M)


@pytest.mark.parametrize("extend", [0, 1])
@pytest.mark.parametrize("shape,n_edges", [((2, 2), 1), ((5, 7), 3), ((33, 64), 32), ((9, 17), 7)])
def test_maps_and_thickness_equal_the_restated_rule(shim, shape, n_edges, extend):
    M, N = shape
    x_st, rows = edges_case(5 + n_edges, M, N, n_edges + 2)
    map_of = [0] * n_edges + [-1, 1]  # (an edge on no map; a second map of one edge, not adjacent to nothing)
    if n_edges >= 3:
        map_of[1], map_of[-1] = 1, 0  # (the edges of a map are not adjacent in the table)
    n = len(map_of)
    L = R.most_edges(map_of, n)
    out = np.full((2, M, N), 99, dtype=np.uint8)
    thick = np.zeros((2, L + 1, N), dtype=np.int32)
    k = shim.shim_row_maps(M, N, n, i32(x_st).ctypes.data_as(C.c_void_p), i32([len(r) for r in rows]).ctypes.data_as(C.c_void_p), np.concatenate(rows).ctypes.data_as(C.c_void_p),
                           i32(map_of).ctypes.data_as(C.c_void_p), 2, extend, out.ctypes.data_as(C.c_void_p), L, thick.ctypes.data_as(C.c_void_p))
    want = R.row_maps((M, N), x_st, rows, map_of, bool(extend))
    assert k == n - 1 and np.array_equal(out, want)
    assert np.array_equal(thick, R.thick_of(want, L)) and np.array_equal(thick.sum(axis=1), np.full((2, N), M))


def test_the_crossing_predicate(shim):
    rng = np.random.default_rng(2)
    # hand cases: a rising and a falling segment left and right of the pixel, a horizontal segment, a vertex on the pixel's row
    cases = [(2.0, 3.0, 5.0, 1.0, 5.0, 6.0), (7.0, 3.0, 5.0, 1.0, 5.0, 6.0), (2.0, 3.0, 5.0, 6.0, 5.0, 1.0), (7.0, 3.0, 5.0, 6.0, 5.0, 1.0),
             (2.0, 3.0, 1.0, 3.0, 9.0, 3.0), (2.0, 3.0, 4.0, 3.0, 6.0, 8.0), (2.0, 3.0, 4.0, 8.0, 6.0, 3.0), (5.0, 3.0, 5.0, 1.0, 5.0, 6.0)]
    assert [shim.shim_crossing(*c) for c in cases] == [1, 0, 1, 0, 0, 1, 1, 0]
    v = rng.integers(-40, 41, size=(4000, 6)) / 8.0 + rng.normal(0, 1e-9, size=(4000, 6)) * (rng.random((4000, 1)) < 0.5)
    got = np.array([shim.shim_crossing(*row) for row in v], dtype=bool)
    want = np.array([bool(R.crossing(*row)) for row in v])
    assert np.array_equal(got, want) and 200 < got.sum() < 2000
    for row in v[:200]:  # NaN anywhere: no toggle from the straddle test's side that fails, the same answer both ways
        bad = row.copy()
        bad[int(rng.integers(0, 6))] = np.nan
        assert bool(shim.shim_crossing(*bad)) == bool(R.crossing(*bad))


@pytest.mark.parametrize("n", [4, 5, 64, 65])
def test_inside_equals_the_restated_rule(shim, n):
    Ms, Ns = 19, 23
    rng = np.random.default_rng(n)
    th = np.sort(rng.random(n)) * 2 * np.pi
    rad = 4.0 + 6.0 * rng.random(n)
    xy = np.ascontiguousarray(np.stack([11.3 + rad * np.cos(th), 9.1 + rad * np.sin(th)], axis=1))
    xy[0] = (np.floor(xy[0, 0]), 9.0)  # a vertex on a pixel
    out = np.zeros((Ms, Ns), dtype=np.uint8)
    shim.shim_inside(Ms, Ns, xy.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p))
    assert np.array_equal(out.astype(bool), R.inside((Ms, Ns), xy)) and out.sum() > 5


def test_vertex_is_polar_to_xys_arithmetic(shim):
    from gaussian_process_edge_trace_amd import gpet_utils as U
    pol = dict(centre=(47.3, 48.9), n_r=40, n_theta=90, r0=1.25, dr=0.7, theta0=0.3, pad=2)
    sp = U._lib.polar_spec(pol)
    rows = np.array([0, 3, 17, 39, 200, -5])
    for j in (0, 1, 44, 89):
        x, y = U.polar_to_xy(rows, np.full(rows.shape, j + sp.pad), sp)
        for t, wx, wy in zip(rows, x, y):
            xy = np.zeros(2)
            shim.shim_vertex(int(t), sp.r0, sp.dr, sp.centre[0, 0], sp.centre[0, 1], sp.cos_t[j], sp.sin_t[j], xy.ctypes.data_as(C.c_void_p))
            assert (xy[0], xy[1]) == (wx, wy)


# ---- every refusal with its words: the header's, and _lib's repetition of them ----------------------------------------------------------
def test_refusals_of_row_maps_and_their_words(shim):
    from gaussian_process_edge_trace_amd import _lib
    L = C.c_int(0)

    def both(M, N, x_st, ln, map_of, n_maps, rows_null=0, out_null=0, null_tables=False):
        n = len(map_of) if map_of is not None else 0
        got = shim.shim_check(M, N, n, None if null_tables else i32(x_st).ctypes.data_as(C.c_void_p), None if null_tables else i32(ln).ctypes.data_as(C.c_void_p), rows_null,
                              None if map_of is None else i32(map_of).ctypes.data_as(C.c_void_p), n_maps, out_null, C.byref(L))
        got = None if got is None else got.decode()
        mine = _lib.label_refusal(M, N, None if null_tables else x_st, None if null_tables else ln, map_of, n_maps,
                                  rows=None if rows_null else (), out=None if out_null else ())
        assert got == mine, (got, mine)
        return got

    ok = dict(M=8, N=10, x_st=[0, 2, 5], ln=[10, 8, 5], map_of=[0, 1, 0], n_maps=2)
    assert both(**ok) is None and L.value == 2
    assert both(**dict(ok, map_of=[0, -1, 1])) is None and L.value == 1
    for kw in (dict(rows_null=1), dict(out_null=1), dict(null_tables=True), dict(map_of=None)):
        assert both(**dict(ok, **kw)) == "label maps: a null pointer"
    assert both(**dict(ok, M=1)) == both(**dict(ok, N=1)) == "label maps: frames must be at least 2 x 2 pixels"
    assert both(**dict(ok, M=1 << 16, N=(1 << 15) + 1, x_st=[0] * 3, ln=[1] * 3)) == "label maps: a map exceeds 2^31 pixels (M * N)"
    assert both(**dict(ok, M=1 << 16, N=1 << 15)) is None  # (2^31 itself is in)
    assert both(**dict(ok, n_maps=0)) == "label maps: n_maps must be at least 1"
    assert both(**dict(ok, map_of=[0, 2, 1])) == "label maps: map_of[1] = 2 lies outside [-1, n_maps = 2)"
    assert both(**dict(ok, map_of=[0, -2, 1])) == "label maps: map_of[1] = -2 lies outside [-1, n_maps = 2)"
    assert both(**dict(ok, map_of=[0, -1, 0])) == "label maps: map 1 has no edge"
    many = dict(M=8, N=10, x_st=[0] * 34, ln=[10] * 34, map_of=[0] * 33 + [1], n_maps=2)
    assert both(**many) == "label maps: map 0 has more than 32 edges (33)"
    assert both(**dict(many, map_of=[0] * 32 + [1, 1])) is None and L.value == 32
    assert both(**dict(ok, x_st=[0, 3, 5])) == "label maps: the grid of edge 1 lies outside [0, N) (x_st = 3, len = 8, N = 10)"
    assert both(**dict(ok, x_st=[-1, 2, 5])) == "label maps: the grid of edge 0 lies outside [0, N) (x_st = -1, len = 10, N = 10)"
    assert both(**dict(ok, ln=[10, 8, 0])) == "label maps: the grid of edge 2 lies outside [0, N) (x_st = 5, len = 0, N = 10)"


def test_refusals_of_outline_maps_and_their_words(shim):
    from gaussian_process_edge_trace_amd import _lib
    L = C.c_int(0)

    def both(Ms, Ns, n_vert, map_of, n_maps, xy_null=0, out_null=0):
        got = shim.shim_check_xy(Ms, Ns, len(map_of), None if n_vert is None else i32(n_vert).ctypes.data_as(C.c_void_p), xy_null, i32(map_of).ctypes.data_as(C.c_void_p), n_maps,
                                 out_null, C.byref(L))
        got = None if got is None else got.decode()
        mine = _lib.label_refusal_xy(Ms, Ns, n_vert, map_of, n_maps, xy=None if xy_null else (), out=None if out_null else ())
        assert got == mine, (got, mine)
        return got

    ok = dict(Ms=9, Ns=9, n_vert=[4, 4096, 65], map_of=[0, 0, 1], n_maps=2)
    assert both(**ok) is None and L.value == 2
    for kw in (dict(xy_null=1), dict(out_null=1), dict(n_vert=None)):
        assert both(**dict(ok, **kw)) == "label maps: a null pointer"
    assert both(**dict(ok, Ms=1)) == "label maps: frames must be at least 2 x 2 pixels"
    assert both(**dict(ok, n_vert=[3, 5, 5])) == "label maps: contour 0 has 3 vertices, outside [4, 4096]"
    assert both(**dict(ok, n_vert=[4, 4097, 5])) == "label maps: contour 1 has 4097 vertices, outside [4, 4096]"
    assert both(**dict(ok, map_of=[0, 0, -1])) == "label maps: map 1 has no contour"
    assert both(Ms=9, Ns=9, n_vert=[4] * 33, map_of=[0] * 33, n_maps=1) == "label maps: map 0 has more than 32 contours (33)"
    # a contributing edge of a polar batch spans the contour from seam to seam
    assert shim.shim_check_closed(3, 2, 92, 2, 90) is None and _lib.label_closed_refusal(3, 2, 92, 2, 90) is None
    words = "label maps: edge 3 does not span the closed contour (x_st = 2, x_en = 91; pad = 2, pad + n_theta = 92)"
    assert shim.shim_check_closed(3, 2, 91, 2, 90).decode() == words == _lib.label_closed_refusal(3, 2, 91, 2, 90)


def test_python_refuses_before_the_library_is_asked():
    """What needs no device: SequenceTracer's and the utilities' own refusals."""
    from gaussian_process_edge_trace_amd.sequence import SequenceTracer, resolve_labels
    assert resolve_labels(None) is None and resolve_labels(False) is None
    assert resolve_labels(True) == dict(extend=False, thickness=False, space=None)
    assert resolve_labels(dict(thickness=True)) == dict(extend=False, thickness=True, space=None)
    for bad in (dict(colour=1), "yes", dict(space="screen"), dict(space="frame", thickness=True)):
        with pytest.raises(ValueError):
            resolve_labels(bad)
    frames = [np.zeros((16, 16), dtype=np.float32)] * 2
    init = np.array([[0, 5], [15, 5]])
    with pytest.raises(ValueError, match="labels and ensemble_seeds are alternatives"):
        SequenceTracer(frames, init, labels=True, ensemble_seeds=[1, 2])
    with pytest.raises(ValueError, match="needs polar"):
        SequenceTracer(frames, init, labels=dict(space="frame"))
