"""CPU tests of what gpet_batch_create2 decides (csrc/gpet_batch_plan.h): the header needs no HIP, so a small extern "C" shim around
it is compiled with the host C++ compiler and driven through ctypes (as tests/test_loop_plan.py does for the loop's plan).

Every expected figure below is a literal.  The resolved fields, the batch dimensions, the arena sizes, the offsets and the
hash over every pointer offset of every edge were dumped from gpet_batch_create2 and carve_edge as they stood BEFORE the
split (their text run on the host with a fake arena base, option jlog_max_b at its default 32); the basis classes come from
the same run of the old search loop.  None of them was produced by the header under test.  The buffer sizes the overlap
check uses are the documented ones of csrc/gpet_dev.h, written out here a second time on purpose."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussian_process_edge_trace_amd", "csrc")

INT_FIELDS = ("M N x_st x_en Lg S n_keep z_cols r_cap n_cap obs_cap n_init kernel_type nu_code tab_ok pad_tab fix_endpoints delta_x "
              "pixel_thresh algo_thresh n_bins a_rows_cap factor_injected z_ring r0 structured jlog_cap Yp y_f32 bin_lo fin_n").split()
PTR_FIELDS = ("grad grad_kde init_xy obs_xy obs_new sc xt yt wt K alpha chol_inv solve_z solve_flag V mean std cov G perm C W theta Wq "
              "Cw wq_tag order Q0 lam0 beta h0 jlog eig Gt Ap ap_tag pcx_d pcx_cand A Z Y costs cost_part best_costs best_idx bins tmpk "
              "kde kde_band kde_wsum colsum colbest colbest_y mm binbest binarg fin_x fin_y fin_w fin_par fin_out rho_tab").split()
BD_FIELDS = "M N Lg S n_keep z_cols r_cap n_cap n_bins obs_cap z_ring a_rows_cap r0_max jlog y_f32 rng4 lg_even".split()
PARAM_FIELDS = ("kernel_type nu sigma_f length_scale noise_y n_samples n_keep delta_x pixel_thresh score_thresh fix_endpoints x_st x_en "
                "n_init obs_cap factor_cap z_cols jitter").split()

SHIM = r"""
#include "gpet_batch_plan.h"
using namespace gpet;
#define INT_FIELDS(X) X(M) X(N) X(x_st) X(x_en) X(Lg) X(S) X(n_keep) X(z_cols) X(r_cap) X(n_cap) X(obs_cap) X(n_init) X(kernel_type) X(nu_code) \
  X(tab_ok) X(pad_tab) X(fix_endpoints) X(delta_x) X(pixel_thresh) X(algo_thresh) X(n_bins) X(a_rows_cap) X(factor_injected) X(z_ring) \
  X(r0) X(structured) X(jlog_cap) X(Yp) X(y_f32) X(bin_lo) X(fin_n)
#define PTR_FIELDS(X) X(grad) X(grad_kde) X(init_xy) X(obs_xy) X(obs_new) X(sc) X(xt) X(yt) X(wt) X(K) X(alpha) X(chol_inv) X(solve_z) \
  X(solve_flag) X(V) X(mean) X(std) X(cov) X(G) X(perm) X(C) X(W) X(theta) X(Wq) X(Cw) X(wq_tag) X(order) X(Q0) X(lam0) X(beta) X(h0) \
  X(jlog) X(eig) X(Gt) X(Ap) X(ap_tag) X(pcx_d) X(pcx_cand) X(A) X(Z) X(Y) X(costs) X(cost_part) X(best_costs) X(best_idx) X(bins) \
  X(tmpk) X(kde) X(kde_band) X(kde_wsum) X(colsum) X(colbest) X(colbest_y) X(mm) X(binbest) X(binarg) X(fin_x) X(fin_y) X(fin_w) \
  X(fin_par) X(fin_out) X(rho_tab)
#define BD_FIELDS(X) X(M) X(N) X(Lg) X(S) X(n_keep) X(z_cols) X(r_cap) X(n_cap) X(n_bins) X(obs_cap) X(z_ring) X(a_rows_cap) X(r0_max) \
  X(jlog) X(y_f32) X(rng4) X(lg_even)
static std::vector<gpet_params> params_of(const double* v, int B) {  // 18 doubles per edge, in the order of gpet_params
  std::vector<gpet_params> ps((size_t)B);
  for (int e = 0; e < B; ++e, v += 18) {
    gpet_params& p = ps[(size_t)e];
    memset(&p, 0, sizeof p);
    p.kernel_type = (int)v[0]; p.nu = v[1]; p.sigma_f = v[2]; p.length_scale = v[3]; p.noise_y = v[4]; p.n_samples = (int)v[5];
    p.n_keep = (int)v[6]; p.delta_x = (int)v[7]; p.pixel_thresh = (int)v[8]; p.score_thresh = v[9]; p.fix_endpoints = (int)v[10];
    p.x_st = (int)v[11]; p.x_en = (int)v[12]; p.n_init = (int)v[13]; p.obs_cap = (int)v[14]; p.factor_cap = (int)v[15];
    p.z_cols = (int)v[16]; p.jitter = v[17];
  }
  return ps;
}
// status of the first edge that fails (as gpet_batch_create2 returns it), else 0 with the edges resolved
static int resolve_all(std::vector<EdgeDev>& edges, const gpet_params* ps, int B, int M, int N, int jlog_max_b) {
  edges.resize((size_t)B);
  const bool any_big = any_big_edge(ps, B);
  for (int e = 0; e < B; ++e) {
    const EdgeCheck chk = resolve_edge(edges[(size_t)e], ps[e], B, M, N, any_big, jlog_max_b);
    if (chk != EdgeCheck::ok) return edge_check_status(chk);
  }
  return 0;
}
static long long off_of(const char* base, const void* p) { return p ? (long long)((const char*)p - base) : -1; }
extern "C" {
int shim_sizes(int which) { return which == 0 ? (int)sizeof(gpet_scalars) : which == 1 ? (int)sizeof(EigState) : STRUCT_H_LDS_MAX; }
int shim_shape_ok(int B, int M, int N) { return batch_shape_ok(B, M, N) ? 1 : 0; }
// ints: B x 31, dbl: B x inv_gamma_nu, offs: B x 62 pointer offsets (placing pass; -1 = null), bd: 17,
// batch: scalars, fin_out, fin_par, obs, init offsets, n_init_max, end of the measuring pass, end of the placing pass, non-null
// pointers left by the measuring pass
int shim_plan(int B, int M, int N, const double* pv, int share, int jlog_max_b, int* ints, double* dbl, long long* offs, int* bd_out,
              long long* batch) {
  const std::vector<gpet_params> ps = params_of(pv, B);
  std::vector<EdgeDev> edges;
  const int rc = resolve_all(edges, ps.data(), B, M, N, jlog_max_b);
  if (rc) return rc;
  const BatchDims bd = reduce_dims(edges.data(), B, M, N);
  Carver meas;
  layout_batch(meas, edges.data(), B, bd, share != 0);
  long long stray = 0;
  for (int e = 0; e < B; ++e) {
#define X(f) stray += edges[(size_t)e].f != nullptr;
    PTR_FIELDS(X)
#undef X
  }
  static char anchor;  // (a non-null base: the layout only does address arithmetic, nothing is dereferenced)
  const char* base = &anchor;
  Carver cv;
  cv.base = &anchor;
  const BatchBlocks bb = layout_batch(cv, edges.data(), B, bd, share != 0);
  for (int e = 0; e < B; ++e) {
    const EdgeDev& E = edges[(size_t)e];
#define X(f) *ints++ = E.f;
    INT_FIELDS(X)
#undef X
    *dbl++ = E.inv_gamma_nu;
#define X(f) *offs++ = off_of(base, E.f);
    PTR_FIELDS(X)
#undef X
  }
#define X(f) *bd_out++ = bd.f;
  BD_FIELDS(X)
#undef X
  batch[0] = off_of(base, bb.scalars); batch[1] = off_of(base, bb.fin_out); batch[2] = off_of(base, bb.fin_par);
  batch[3] = off_of(base, bb.obs); batch[4] = off_of(base, bb.init); batch[5] = bb.n_init_max;
  batch[6] = (long long)meas.off; batch[7] = (long long)cv.off; batch[8] = stray;
  return 0;
}
// init_x: B x n_init_max x-coordinates (row e holds those of edge e)
int shim_eligible(int B, int M, int N, const double* pv, const long long* init_x, int n_init_max) {
  const std::vector<gpet_params> ps = params_of(pv, B);
  std::vector<EdgeDev> edges;
  if (resolve_all(edges, ps.data(), B, M, N, 32)) return -1;
  std::vector<std::vector<int64_t>> xy((size_t)B);
  std::vector<const int64_t*> ptr((size_t)B);
  for (int e = 0; e < B; ++e) {
    for (int i = 0; i < ps[(size_t)e].n_init; ++i) { xy[(size_t)e].push_back(init_x[e * n_init_max + i]); xy[(size_t)e].push_back(7); }
    ptr[(size_t)e] = xy[(size_t)e].data();
  }
  return struct_eligible(edges.data(), B, N, ptr.data()) ? 1 : 0;
}
int shim_classes(int B, int M, int N, const double* pv, int* rep_of, int* reps) {
  const std::vector<gpet_params> ps = params_of(pv, B);
  std::vector<EdgeDev> edges;
  if (resolve_all(edges, ps.data(), B, M, N, 32)) return -1;
  std::vector<int> ro, rp;
  basis_classes(edges.data(), B, ro, rp);
  for (int e = 0; e < B; ++e) rep_of[e] = ro[(size_t)e];
  for (size_t k = 0; k < rp.size(); ++k) reps[k] = rp[k];
  return (int)rp.size();
}
int shim_lds_fit(int n_cap, int r_cap, int r0_max) {
  BatchDims bd{};
  bd.n_cap = n_cap; bd.r_cap = r_cap;
  return struct_h_fits_lds(bd, r0_max) ? 1 : 0;
}
// out: B x (done, n_obs + iter + status + rank + n + force + n_removed, score_thresh as an int, y_s + amp + y_mean + y_std + lml == 0)
int shim_pristine(int B, int M, int N, const double* pv, int* out) {
  const std::vector<gpet_params> ps = params_of(pv, B);
  std::vector<EdgeDev> edges;
  if (resolve_all(edges, ps.data(), B, M, N, 32)) return -1;
  std::vector<gpet_scalars> sc((size_t)B);
  memset(sc.data(), 0xAB, sizeof(gpet_scalars) * (size_t)B);
  pristine_scalars(ps.data(), edges.data(), B, sc.data());
  for (int e = 0; e < B; ++e) {
    const gpet_scalars& s = sc[(size_t)e];
    *out++ = s.done; *out++ = s.n_obs + s.iter + s.status + s.rank + s.n + s.force + s.n_removed; *out++ = (int)s.score_thresh;
    *out++ = (s.y_s == 0 && s.amp == 0 && s.y_mean == 0 && s.y_std == 0 && s.lml == 0) ? 1 : 0;
  }
  return 0;
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
    d = tmp_path_factory.mktemp("batch_plan")
    src, so = d / "shim.cpp", d / "libbatch_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    return C.CDLL(str(so))


def edge(**kw):
    """The bench edge (500 x 500 image, whole width, S = 1000), with changes."""
    p = dict(kernel_type=0, nu=2.5, sigma_f=75, length_scale=20, noise_y=1, n_samples=1000, n_keep=100, delta_x=5, pixel_thresh=5,
             score_thresh=1, fix_endpoints=1, x_st=0, x_en=499, n_init=2, obs_cap=0, factor_cap=0, z_cols=0, jitter=1e-6)
    assert set(kw) <= set(p)
    p.update(kw)
    return p


def _flat(ps):
    return (C.c_double * (18 * len(ps)))(*[float(p[k]) for p in ps for k in PARAM_FIELDS])


def plan(shim, ps, M, N, share, jlog_max_b=32):
    """status, or a dict of what the header resolved and laid out."""
    B = len(ps)
    ints, dbl, offs = (C.c_int * (31 * B))(), (C.c_double * B)(), (C.c_longlong * (62 * B))()
    bd, batch = (C.c_int * 17)(), (C.c_longlong * 9)()
    rc = shim.shim_plan(B, M, N, _flat(ps), share, jlog_max_b, ints, dbl, offs, bd, batch)
    if rc:
        return rc
    edges = []
    for e in range(B):
        E = dict(zip(INT_FIELDS, ints[31 * e:31 * e + 31]))
        E["inv_gamma_nu"] = dbl[e]
        E["off"] = dict(zip(PTR_FIELDS, offs[62 * e:62 * e + 62]))
        edges.append(E)
    return dict(edges=edges, bd=dict(zip(BD_FIELDS, bd)), blocks=dict(zip(("scalars", "fin_out", "fin_par", "obs", "init"), batch[:5])),
                n_init_max=batch[5], meas_end=batch[6], place_end=batch[7], stray=batch[8], arena_bytes=batch[6] + 256)


def offsets_hash(p):
    h = 1469598103934665603
    vals = [p["blocks"][k] for k in ("scalars", "fin_out", "fin_par", "obs", "init")]
    for E in p["edges"]:
        vals += [E["off"][f] for f in PTR_FIELDS]
    for v in vals:
        h = ((h ^ (v & 0xFFFFFFFFFFFFFFFF)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


_MIX = [edge(x_en=399, n_samples=700, n_keep=70, n_init=3), edge(x_st=50, x_en=250, n_samples=333, n_keep=0, n_init=5, fix_endpoints=0),
        edge(x_st=7, x_en=406, n_keep=1000, factor_cap=40)]
_ANY_BIG = [edge(x_en=299, n_samples=300, n_keep=30), edge(x_en=299, n_samples=300, n_keep=30, factor_cap=128),
            edge(x_st=10, x_en=209, n_samples=300, n_keep=30, z_cols=50)]
_WIDE, _NARROW = edge(x_en=1499, n_samples=500, n_keep=50), edge(x_st=100, x_en=399, n_samples=500, n_keep=50)
_ZC = dict(n_samples=256, n_keep=25)
_MATERN = [edge(kernel_type=1, nu=nu) for nu in (170.0, 171.0, 1.5, 0.7)]
# the integer fields of the bench edge, in the order of INT_FIELDS, but for (z_ring, jlog_cap)
_BENCH = lambda ring, jlog: (500, 500, 0, 499, 500, 1000, 100, 96, 96, 104, 102, 2, 0, 2, 1, 0, 1, 5, 5, 96, 102, 96, 0, ring, 0, 0, jlog, 512, 0, 0, 0)
_BENCH_BD = lambda ring, jlog: (500, 500, 500, 1000, 100, 96, 96, 104, 102, 102, ring, 96, 0, jlog, 0, 1, 1)

# name: (edges, M, N, shared image, arena_bytes, hash of all pointer offsets, BatchDims (rng4 as gpet_batch_create2 sets it),
#        {edge: (INT_FIELDS..., inv_gamma_nu, offset of Y, offset of costs)})
CASES = {
    "bench_B1_shared": ([edge()], 500, 500, 1, 30962016, 0x5812c7a063987681, _BENCH_BD(16, 1), {0: _BENCH(16, 40) + (1, 21366272, 25614848)}),
    "bench_B1_own": ([edge()], 500, 500, 0, 30961984, 0xcc4c23e694ed1281, _BENCH_BD(16, 1), {0: _BENCH(16, 40) + (1, 19365888, 23614464)}),
    "bench_B32_shared": ([edge()] * 32, 500, 500, 1, 928740448, 0x77641c5606239ba9, _BENCH_BD(16, 1),
                         {0: _BENCH(16, 40) + (1, 21670400, 25918976), 31: _BENCH(16, 40) + (1, 919144704, 923393280)}),
    "bench_B32_own": ([edge()] * 32, 500, 500, 0, 990752320, 0x7455fd12a0aed1a9, _BENCH_BD(16, 1),
                      {0: _BENCH(16, 40) + (1, 19670016, 23918592), 31: _BENCH(16, 40) + (1, 979156224, 983404800)}),
    "bench_B33_shared": ([edge()] * 33, 500, 500, 1, 858361952, 0xe303e51c0d6b8d81, _BENCH_BD(16, 0),
                         {0: _BENCH(16, 0) + (1, 18670848, 22919424), 32: _BENCH(16, 0) + (1, 848766208, 853014784)}),
    "bench_B33_own": ([edge()] * 33, 500, 500, 0, 922374208, 0x26017a43e46e3b81, _BENCH_BD(16, 0),
                      {0: _BENCH(16, 0) + (1, 16670464, 20919040), 32: _BENCH(16, 0) + (1, 910778112, 915026688)}),
    "bench_B64_shared": ([edge()] * 64, 500, 500, 1, 1662820960, 0xa2c503f518b78fa9, _BENCH_BD(16, 0),
                         {0: _BENCH(16, 0) + (1, 18974976, 23223552), 63: _BENCH(16, 0) + (1, 1653225216, 1657473792)}),
    "bench_B64_own": ([edge()] * 64, 500, 500, 0, 1788845120, 0x8d2d14be0ac6f1a9, _BENCH_BD(16, 0),
                      {0: _BENCH(16, 0) + (1, 16974592, 21223168), 63: _BENCH(16, 0) + (1, 1777249024, 1781497600)}),
    "bench_B65_shared": ([edge()] * 65, 500, 500, 1, 1339332192, 0x0de7d43bbdf17981, _BENCH_BD(9, 0),
                         {0: _BENCH(9, 0) + (1, 13609728, 17858304), 64: _BENCH(9, 0) + (1, 1329736448, 1333985024)}),
    "bench_B65_own": ([edge()] * 65, 500, 500, 0, 1467356736, 0x05ad591fbf5f5b81, _BENCH_BD(9, 0),
                      {0: _BENCH(9, 0) + (1, 11609344, 15857920), 64: _BENCH(9, 0) + (1, 1455760640, 1460009216)}),
    "bench_B1024_shared": ([edge()] * 1024, 500, 500, 1, 21070104160, 0xf08715e044c777a9, _BENCH_BD(9, 0),
                           {0: _BENCH(9, 0) + (1, 23045376, 27293952), 1023: _BENCH(9, 0) + (1, 21060508416, 21064756992)}),
    "bench_B1024_own": ([edge()] * 1024, 500, 500, 0, 23116496960, 0xec2259ff29c019a9, _BENCH_BD(9, 0),
                        {0: _BENCH(9, 0) + (1, 21044992, 25293568), 1023: _BENCH(9, 0) + (1, 23104900864, 23109149440)}),
    "odd65": ([edge(x_en=64, n_samples=200, n_keep=20, pixel_thresh=3)] * 2, 65, 65, 1, 7335520, 0xbf84e29f50e124e9,
              (65, 65, 65, 200, 20, 65, 65, 17, 15, 15, 16, 65, 0, 1, 0, 0, 0),
              {0: (65, 65, 0, 64, 65, 200, 20, 65, 65, 17, 15, 2, 0, 2, 1, 0, 1, 5, 3, 11, 15, 65, 0, 16, 0, 0, 40, 80, 0, 0, 0, 1, 3404544, 3577856),
               1: (65, 65, 0, 64, 65, 200, 20, 65, 65, 17, 15, 2, 0, 2, 1, 0, 1, 5, 3, 11, 15, 65, 0, 16, 0, 0, 40, 80, 0, 0, 0, 1, 7053312, 7226624)}),
    # factor_cap = 128 on the second edge only: every edge keeps all its Lg directions and stores whole rows of normals
    "any_big_mixed": (_ANY_BIG, 120, 300, 0, 31431040, 0x261bba4808559c61, (120, 300, 300, 300, 30, 300, 300, 64, 62, 62, 2, 300, 0, 0, 0, 0, 1),
                      {0: (120, 300, 0, 299, 300, 300, 30, 300, 300, 64, 62, 2, 0, 2, 1, 0, 1, 5, 5, 56, 62, 300, 0, 2, 0, 0, 0, 304, 0, 0, 0, 1, 10317312, 11283968),
                       1: (120, 300, 0, 299, 300, 300, 30, 300, 300, 64, 62, 2, 0, 2, 1, 0, 1, 5, 5, 56, 62, 300, 0, 2, 0, 0, 0, 304, 0, 0, 0, 1, 22675456, 23642112),
                       2: (120, 300, 10, 209, 200, 300, 30, 200, 200, 64, 62, 2, 0, 2, 1, 0, 1, 5, 5, 36, 62, 200, 0, 2, 0, 0, 0, 208, 0, -2, 0, 1, 29695488, 30357248)}),
    "zcols_full_100": ([edge(x_en=99, z_cols=100, **_ZC)], 100, 100, 1, 7568224, 0xe24fb27718e01c81, (100, 100, 100, 256, 25, 100, 96, 24, 22, 22, 16, 100, 0, 1, 0, 1, 1),
                       {0: (100, 100, 0, 99, 100, 256, 25, 100, 96, 24, 22, 2, 0, 2, 1, 0, 1, 5, 5, 16, 22, 100, 0, 16, 0, 0, 40, 112, 0, 0, 0, 1, 7090944, 7333120)}),
    "zcols_full_200": ([edge(x_en=199, z_cols=200, **_ZC)], 100, 200, 1, 6317664, 0x0ad647a4586b9881, (100, 200, 200, 256, 25, 200, 96, 44, 42, 42, 2, 200, 0, 1, 0, 1, 1),
                       {0: (100, 200, 0, 199, 200, 256, 25, 200, 96, 44, 42, 2, 0, 2, 1, 0, 1, 5, 5, 36, 42, 200, 0, 2, 0, 0, 40, 208, 0, 0, 0, 1, 5415424, 5864192)}),
    "zcols_full_200_B70": ([edge(x_en=199, z_cols=200, **_ZC)] * 70, 100, 200, 1, 220396384, 0x2603a4ea349ee7a9, (100, 200, 200, 256, 25, 200, 96, 44, 42, 42, 2, 200, 0, 0, 0, 1, 1),
                           {0: (100, 200, 0, 199, 200, 256, 25, 200, 96, 44, 42, 2, 0, 2, 1, 0, 1, 5, 5, 36, 42, 200, 0, 2, 0, 0, 0, 208, 0, 0, 0, 1, 2686208, 3134976),
                            69: (100, 200, 0, 199, 200, 256, 25, 200, 96, 44, 42, 2, 0, 2, 1, 0, 1, 5, 5, 36, 42, 200, 0, 2, 0, 0, 0, 208, 0, 0, 0, 1, 219494144, 219942912)}),
    "config3": ([edge(x_en=2047, n_samples=4000, n_keep=400, obs_cap=1498, sigma_f=300, length_scale=80)], 2048, 2048, 1, 325483616, 0xf74ac453db2cfd81,
                (2048, 2048, 2048, 4000, 400, 96, 96, 1500, 411, 1498, 16, 96, 0, 1, 0, 1, 1),
                {0: (2048, 2048, 0, 2047, 2048, 4000, 400, 96, 96, 1500, 1498, 2, 0, 2, 1, 0, 1, 5, 5, 405, 411, 96, 0, 16, 0, 0, 40, 2048, 0, 0, 0, 1, 169540096, 236862976)}),
    "wide_and_narrow": ([_WIDE, _NARROW], 64, 1500, 1, 62591328, 0x0c535d9396ca8ae9, (64, 1500, 1500, 500, 50, 96, 96, 304, 302, 302, 16, 96, 0, 1, 0, 0, 1),
                        {0: (64, 1500, 0, 1499, 1500, 500, 50, 96, 96, 304, 302, 2, 0, 2, 1, 0, 1, 5, 5, 296, 302, 96, 0, 16, 0, 0, 40, 1504, 0, 0, 0, 1, 37592064, 43909888),
                         1: (64, 1500, 100, 399, 300, 500, 50, 96, 96, 304, 302, 2, 0, 2, 1, 0, 1, 5, 5, 56, 302, 96, 0, 16, 0, 0, 40, 304, 0, -20, 0, 1, 59197696, 60475648)}),
    "narrow_alone": ([_NARROW], 64, 1500, 1, 16794208, 0xf9b09c2b16454d81, (64, 1500, 300, 500, 50, 96, 96, 304, 302, 302, 16, 96, 0, 1, 0, 1, 1),
                     {0: (64, 1500, 100, 399, 300, 500, 50, 96, 96, 304, 302, 2, 0, 2, 1, 0, 1, 5, 5, 56, 302, 96, 0, 16, 0, 0, 40, 304, 0, -20, 0, 1, 13400576, 14678528)}),
    "mixed_shapes_own": (_MIX, 77, 410, 0, 40509512, 0x44a80e431eb7d5b1, (77, 410, 400, 1000, 1000, 96, 96, 89, 84, 84, 16, 96, 0, 1, 0, 0, 0),
                         {0: (77, 410, 0, 399, 400, 700, 70, 96, 96, 87, 84, 3, 0, 2, 1, 0, 1, 5, 5, 76, 84, 96, 0, 16, 0, 0, 40, 400, 0, 0, 0, 1, 14574080, 17074432),
                          1: (77, 410, 50, 250, 201, 333, 0, 96, 96, 89, 84, 5, 0, 2, 1, 0, 0, 5, 5, 36, 84, 96, 0, 16, 0, 0, 40, 208, 0, -10, 0, 1, 26651392, 27313152),
                          2: (77, 410, 7, 406, 400, 1000, 1000, 40, 40, 85, 83, 2, 0, 2, 1, 0, 1, 5, 5, 76, 83, 40, 0, 16, 0, 0, 40, 400, 0, -1, 0, 1, 36015360, 39334912)}),
    "mixed_shapes_shared": (_MIX, 77, 410, 1, 40003680, 0x3bbb11bf639b31b1, (77, 410, 400, 1000, 1000, 96, 96, 89, 84, 84, 16, 96, 0, 1, 0, 0, 0),
                            {0: (77, 410, 0, 399, 400, 700, 70, 96, 96, 87, 84, 3, 0, 2, 1, 0, 1, 5, 5, 76, 84, 96, 0, 16, 0, 0, 40, 400, 0, 0, 0, 1, 14827008, 17327360),
                             1: (77, 410, 50, 250, 201, 333, 0, 96, 96, 89, 84, 5, 0, 2, 1, 0, 0, 5, 5, 36, 84, 96, 0, 16, 0, 0, 40, 208, 0, -10, 0, 1, 26651392, 27313152),
                             2: (77, 410, 7, 406, 400, 1000, 1000, 40, 40, 85, 83, 2, 0, 2, 1, 0, 1, 5, 5, 76, 83, 40, 0, 16, 0, 0, 40, 400, 0, -1, 0, 1, 35762432, 39081984)}),
    "obs_cap_300": ([edge(obs_cap=300)] * 2, 500, 500, 1, 63165024, 0x2d30c63214854b49, (500, 500, 500, 1000, 100, 96, 96, 302, 102, 300, 16, 96, 0, 1, 0, 1, 1),
                    {0: (500, 500, 0, 499, 500, 1000, 100, 96, 96, 302, 300, 2, 0, 2, 1, 0, 1, 5, 5, 96, 102, 96, 0, 16, 0, 0, 40, 512, 0, 0, 0, 1, 22995712, 27244288),
                     1: (500, 500, 0, 499, 500, 1000, 100, 96, 96, 302, 300, 2, 0, 2, 1, 0, 1, 5, 5, 96, 102, 96, 0, 16, 0, 0, 40, 512, 0, 0, 0, 1, 53564672, 57813248)}),
    "delta_7": ([edge(x_st=3, x_en=489, delta_x=7, pixel_thresh=4)], 500, 500, 1, 30527584, 0xdf8991c725361781, (500, 500, 487, 1000, 100, 96, 96, 75, 73, 73, 16, 96, 0, 1, 0, 0, 0),
                {0: (500, 500, 3, 489, 487, 1000, 100, 96, 96, 75, 73, 2, 0, 2, 1, 0, 1, 7, 4, 66, 73, 96, 0, 16, 0, 0, 40, 496, 0, 0, 0, 1, 21065728, 25181696)}),
    # general-nu Matern at nu = 170 (1 / Gamma(nu)) and 171 (-lgamma(nu)); nu = 1.5 is a closed form; RBF ignores nu
    "matern_nu": (_MATERN, 500, 500, 1, 117843552, 0xb9fb0496f1b0aa69, _BENCH_BD(16, 1),
                  {0: _BENCH(16, 40)[:12] + (1, 3) + _BENCH(16, 40)[14:] + (2.3424316452460099e-305, 21395456, 25644032),
                   1: _BENCH(16, 40)[:12] + (1, 3) + _BENCH(16, 40)[14:] + (-706.57306224578736, 50346240, 54594816),
                   2: _BENCH(16, 40)[:12] + (1, 1) + _BENCH(16, 40)[14:] + (1, 79297024, 83545600),
                   3: _BENCH(16, 40)[:12] + (1, 3) + _BENCH(16, 40)[14:] + (0.7703831838665659, 108247808, 112496384)}),
    "rbf_ignores_nu": ([edge(nu=5000.0)], 500, 500, 1, 30962016, 0x5812c7a063987681, _BENCH_BD(16, 1), {0: _BENCH(16, 40) + (1, 21366272, 25614848)}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_resolved_fields_dimensions_and_arena(shim, name):
    ps, M, N, share, arena_bytes, ohash, bd, edges = CASES[name]
    p = plan(shim, ps, M, N, share)
    assert not isinstance(p, int), p
    got_bd = p["bd"]
    # (rng4 is normals4_applies' verdict, which gpet_batch_create2 adds: not the header's)
    assert [got_bd[k] for k in BD_FIELDS if k != "rng4"] == [v for k, v in zip(BD_FIELDS, bd) if k != "rng4"]
    assert got_bd["rng4"] == 0
    for e, want in edges.items():
        E = p["edges"][e]
        assert tuple(E[k] for k in INT_FIELDS) == want[:31], e
        assert E["inv_gamma_nu"] == pytest.approx(want[31], rel=1e-13), e   # (tgamma / lgamma of the host's libm)
        assert (E["off"]["Y"], E["off"]["costs"]) == want[32:], e
    assert p["arena_bytes"] == arena_bytes
    assert p["meas_end"] == p["place_end"]          # the placing pass ends where the measuring pass did
    assert p["stray"] == 0                            # the measuring pass leaves no pointer behind
    assert offsets_hash(p) == ohash                   # every pointer of every edge where it has always been


def test_issue_table_of_the_bench_edge():
    """The figures the batch sizes are known by: ring slots, rotation log and arena per batch size (shared image, own images)."""
    table = {1: (16, 40, 30962016, 30961984), 32: (16, 40, 928740448, 990752320), 33: (16, 0, 858361952, 922374208),
             64: (16, 0, 1662820960, 1788845120), 65: (9, 0, 1339332192, 1467356736), 1024: (9, 0, 21070104160, 23116496960)}
    for B, (ring, jlog, shared, own) in table.items():
        for kind, want in (("shared", shared), ("own", own)):
            case = CASES["bench_B%d_%s" % (B, kind)]
            assert case[4] == want and case[7][0][23] == ring and case[7][0][26] == jlog


def test_jlog_follows_the_option_passed_in(shim):
    assert plan(shim, [edge()] * 33, 500, 500, 1, jlog_max_b=33)["edges"][0]["jlog_cap"] == 40
    assert plan(shim, [edge()] * 8, 500, 500, 1, jlog_max_b=7)["edges"][7]["jlog_cap"] == 0
    assert plan(shim, [edge()] * 8, 500, 500, 1, jlog_max_b=0)["bd"]["jlog"] == 0


BAD_ARG, UNSUPPORTED = 1, 6   # GPET_ERR_BAD_ARG, GPET_ERR_UNSUPPORTED (include/gpet_hip.h)


@pytest.mark.parametrize("kw,status", [
    (dict(x_st=-1), BAD_ARG), (dict(x_en=500), BAD_ARG), (dict(x_st=10, x_en=12), BAD_ARG), (dict(n_init=0), BAD_ARG),
    (dict(n_samples=0, n_keep=0), BAD_ARG), (dict(n_keep=-1), BAD_ARG), (dict(n_keep=1001), BAD_ARG), (dict(delta_x=0), BAD_ARG),
    (dict(length_scale=0.0), BAD_ARG), (dict(kernel_type=1, nu=1000.5), UNSUPPORTED), (dict(kernel_type=1, nu=0.009), UNSUPPORTED),
    (dict(kernel_type=0, nu=5000.0), 0), (dict(kernel_type=1, nu=1000.0), 0), (dict(kernel_type=1, nu=0.01), 0), (dict(x_st=10, x_en=13), 0),
])
def test_edge_validation_keeps_its_status_codes(shim, kw, status):
    p = plan(shim, [edge(**kw)], 500, 500, 1)
    assert (p if isinstance(p, int) else 0) == status
    if status:   # ... wherever the edge stands in the batch
        assert plan(shim, [edge(), edge(**kw)], 500, 500, 1) == status
    # (an inconsistent edge is reported before a Matern nu out of range, as the checks are ordered)
    assert plan(shim, [edge(kernel_type=1, nu=2000.0, delta_x=0)], 500, 500, 1) == BAD_ARG


def test_batch_shape_check(shim):
    assert shim.shim_shape_ok(1, 2, 2) == 1 and shim.shim_shape_ok(1024, 500, 500) == 1
    assert shim.shim_shape_ok(0, 500, 500) == 0 and shim.shim_shape_ok(-1, 500, 500) == 0
    assert shim.shim_shape_ok(1, 1, 500) == 0 and shim.shim_shape_ok(1, 500, 1) == 0


def _sizes(E, bd, scalars_bytes, eig_bytes):
    """Documented size in bytes of every buffer an EdgeDev points to (csrc/gpet_dev.h), written out independently."""
    M, N, Lg, S, nc, rc = E["M"], E["N"], E["Lg"], E["S"], E["n_cap"], E["r_cap"]
    big = bd["n_cap"] > 128   # (the blocked fit is chosen for the whole batch: every edge then has its scratch)
    s_round = (S + 127) // 128 * 128
    return dict(
        grad=4 * M * N, grad_kde=4 * M * N, init_xy=16 * E["n_init"], obs_xy=16 * E["obs_cap"], obs_new=16 * E["obs_cap"], sc=scalars_bytes,
        xt=8 * nc, yt=8 * nc, wt=8 * nc, K=8 * nc * nc, alpha=8 * nc, chol_inv=8 * (nc // 64 + 1) * 4096 if big else 8,
        solve_z=8 * nc if big else 8, solve_flag=4 * 2 * (nc // 64 + 1) if big else 8, V=8 * nc * Lg, mean=8 * Lg, std=8 * Lg, cov=8 * Lg * Lg,
        G=8 * rc * Lg, perm=4 * rc, C=8 * rc * rc, W=8 * rc * rc, theta=8 * rc, Wq=16 * rc * rc, Cw=8 * rc * rc, wq_tag=8, order=4 * rc,
        Q0=8 * rc * Lg, lam0=8 * rc, beta=8 * rc, h0=8 * rc, jlog=E["jlog_cap"] * (rc - 1) * (rc // 2) * 16 if E["jlog_cap"] else 8, eig=eig_bytes,
        Gt=8 * Lg * rc if (rc > 96 or bd["Lg"] > 1024) else 8, Ap=16 * rc * Lg if rc > 96 else 8, ap_tag=12, pcx_d=8 * Lg,
        pcx_cand=8 * 2 * 4 * (bd["Lg"] // 32 + 1) * 2, A=8 * E["a_rows_cap"] * Lg + 512, Z=8 * E["z_ring"] * S * E["z_cols"],
        Y=8 * ((s_round + 12) * E["Yp"] + 128),   # (rows up to a multiple of 128, then the idle lanes' stores: 128 doubles from row + 12)
        costs=8 * S, cost_part=16 * S * ((Lg + 29) // 30), best_costs=8 * E["n_keep"], best_idx=4 * E["n_keep"], bins=8 * (N + 2) * (M + 2),
        tmpk=8 * (N + 2) * (M + 2), kde=4 * M * N, kde_band=8 * (N // 16 + 1), kde_wsum=8, colsum=8 * N, colbest=8 * N, colbest_y=4 * N, mm=16,
        binbest=8 * E["n_bins"], binarg=8 * E["n_bins"], fin_x=8 * nc, fin_y=8 * nc, fin_w=8 * nc, fin_par=96, fin_out=16 * bd["Lg"], rho_tab=8 * N)


# an edge of at most 128 training points in one batch with an edge of 302: the blocked fit runs on both
_SMALL_WITH_BIG = [edge(x_st=100, x_en=199, delta_x=20), edge(obs_cap=300)]


def test_small_edge_of_a_blocked_batch_has_the_blocked_scratch(shim):
    p = plan(shim, _SMALL_WITH_BIG, 500, 500, 1)
    E = p["edges"][0]
    assert E["n_cap"] <= 128 < p["bd"]["n_cap"] == p["edges"][1]["n_cap"]
    nb = E["n_cap"] // 64 + 1
    assert E["off"]["solve_z"] - E["off"]["chol_inv"] >= 8 * 4096 * nb     # a 64 x 64 inverse per diagonal block
    assert E["off"]["solve_flag"] - E["off"]["solve_z"] >= 8 * E["n_cap"]
    assert E["off"]["K"] - E["off"]["solve_flag"] >= 4 * 2 * nb             # forward and backward flags of k_chol_solve_mw


@pytest.mark.parametrize("name", [n for n in CASES if "B1024" not in n] + ["bench_B1024_shared", "small_with_big"])
def test_layout_is_aligned_disjoint_and_inside_the_arena(shim, name):
    ps, M, N, share = (_SMALL_WITH_BIG, 500, 500, 1) if name == "small_with_big" else CASES[name][:4]
    p = plan(shim, ps, M, N, share)
    scalars_bytes, eig_bytes = shim.shim_sizes(0), shim.shim_sizes(1)
    assert (scalars_bytes, eig_bytes) == (80, 72)
    spans = set()
    for e, E in enumerate(p["edges"]):
        size = _sizes(E, p["bd"], scalars_bytes, eig_bytes)
        assert set(size) == set(PTR_FIELDS)
        for f in PTR_FIELDS:
            off = E["off"][f]
            assert off >= 0, (e, f)
            if f not in ("sc", "fin_out", "fin_par", "obs_xy", "init_xy"):   # (slices of the batch's blocks: those are aligned)
                assert off % 256 == 0, (e, f)
            if share and f in ("grad", "grad_kde"):   # one image for all: the same buffer, counted once
                assert off == p["edges"][0]["off"][f]
                if e:
                    continue
            spans.add((off, off + size[f], e, f))
        # the costs lie directly behind the sample matrix and its spare region: at the next 256-byte boundary
        y_end = E["off"]["Y"] + 8 * ((((E["S"] + 127) & ~127) + 12) * E["Yp"] + 128 + E["Yp"])
        assert E["off"]["costs"] == (y_end + 255) // 256 * 256, e
    for k in ("scalars", "fin_out", "fin_par", "obs", "init"):
        assert p["blocks"][k] % 256 == 0
    order = sorted(spans)
    for (a0, a1, ea, fa), (b0, b1, eb, fb) in zip(order, order[1:]):
        assert a1 <= b0, ("overlap", ea, fa, eb, fb)
    assert order[0][0] >= 0 and order[-1][1] <= p["meas_end"] and p["place_end"] == p["meas_end"]
    if not share and len(ps) > 1:
        assert len({E["off"]["grad"] for E in p["edges"]}) == len(ps) and len({E["off"]["grad_kde"] for E in p["edges"]}) == len(ps)


def test_batch_blocks_hold_one_slice_per_edge(shim):
    p = plan(shim, _MIX, 77, 410, 1)
    bl, bd = p["blocks"], p["bd"]
    assert p["n_init_max"] == 5 and (bd["Lg"], bd["obs_cap"]) == (400, 84)
    for e, E in enumerate(p["edges"]):
        o = E["off"]
        assert o["sc"] == bl["scalars"] + 80 * e
        assert o["fin_out"] == bl["fin_out"] + 8 * 2 * 400 * e
        assert o["fin_par"] == bl["fin_par"] + 8 * 12 * e
        assert o["obs_xy"] == bl["obs"] + 8 * 2 * 84 * e
        assert o["init_xy"] == bl["init"] + 8 * 2 * 5 * e


def test_gt_is_sized_by_the_widest_edge_of_the_batch(shim):
    """The multi-workgroup pivoted Cholesky is picked per batch (widest edge > 1 024 columns) and then writes Gt of EVERY edge."""
    alone = plan(shim, [_NARROW], 64, 1500, 1)["edges"][0]["off"]
    both = plan(shim, [_WIDE, _NARROW], 64, 1500, 1)["edges"][1]["off"]
    assert (alone["Gt"], alone["Ap"]) == (4005632, 4005888)              # one element
    assert (both["Gt"], both["Ap"]) == (49572608, 49803008)              # Lg * r_cap = 300 * 96 doubles
    assert both["Ap"] - both["Gt"] == 300 * 96 * 8


def _init_x(rows, width):
    flat = [x for r in rows for x in list(r) + [0] * (width - len(r))]
    return (C.c_longlong * len(flat))(*flat)


def test_structured_path_eligibility(shim):
    def ok(ps, rows, N=500):
        width = max(len(r) for r in rows)
        return shim.shim_eligible(len(ps), 500, N, _flat(ps), _init_x(rows, width), width)
    assert ok([edge()], [(0, 499)]) == 1
    assert ok([edge(fix_endpoints=0)], [(0, 499)]) == 1                       # free endpoints, but the edge spans the image
    assert ok([edge(fix_endpoints=0, x_st=1)], [(1, 499)]) == 0               # ... and here it does not
    assert ok([edge(fix_endpoints=0, x_en=498)], [(0, 498)]) == 0
    assert ok([edge(x_st=10, x_en=400)], [(10, 400)]) == 1                    # fixed endpoints: any span
    assert ok([edge(x_st=10, x_en=400)], [(9, 400)]) == 0                     # an init point left of the grid
    assert ok([edge(x_st=10, x_en=400)], [(10, 401)]) == 0
    assert ok([edge(x_st=10, x_en=400, n_init=3)], [(10, 200, 400)]) == 1
    assert ok([edge(x_st=10, x_en=400, n_init=3)], [(10, 5, 400)]) == 0       # (x_st / x_en come from the caller, not from the points)
    assert ok([edge(), edge(x_st=10, x_en=400)], [(0, 499), (10, 400)]) == 1
    assert ok([edge(), edge(x_st=10, x_en=400)], [(0, 499), (0, 400)]) == 0   # one edge spoils the batch


def _classes(shim, ps):
    rep_of, reps = (C.c_int * len(ps))(), (C.c_int * len(ps))()
    n = shim.shim_classes(len(ps), 500, 500, _flat(ps), rep_of, reps)
    return list(rep_of), list(reps[:n])


def test_basis_classes_and_the_look_back_of_eight(shim):
    assert _classes(shim, [edge()] * 5) == ([0] * 5, [0])
    # the amplitude is no part of the match; first column, kernel and capacity are
    ps = [edge(), edge(x_st=1), edge(kernel_type=1, nu=1.5), edge(factor_cap=50), edge(sigma_f=10), edge(x_st=1)]
    assert _classes(shim, ps) == ([0, 1, 2, 3, 0, 1], [0, 1, 2, 3])
    # ten classes, then edges equal to edge 0, 5, 0 and 1: only the last eight representatives are searched, so edge 10 founds a
    # class of its own although edge 0 matches (and edge 12 then reads edge 10's basis, not edge 0's); so does edge 13
    ps = [edge(length_scale=l) for l in (10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 10, 15, 10, 11)]
    assert _classes(shim, ps) == ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 5, 10, 13], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13])


def test_struct_h_lds_fit(shim):
    """Up to 128 training points k_struct_H keeps U [n_cap][r0 | 1], a row of L [n_cap] and beta [r_cap] in 150 KB of LDS."""
    assert shim.shim_sizes(2) == 150 * 1024
    assert shim.shim_lds_fit(104, 96, 95) == 1                 # the bench shape: (104 * 95 + 104 + 96) * 8 = 80 640 bytes
    assert shim.shim_lds_fit(128, 96, 146) == 1                # (128 * 147 + 224) * 8 = 152 320 <= 153 600
    assert shim.shim_lds_fit(128, 96, 147) == 1
    assert shim.shim_lds_fit(128, 96, 148) == 0                # (128 * 149 + 224) * 8 = 154 368
    assert shim.shim_lds_fit(129, 96, 1000) == 1               # above 128 training points U lives in HBM: nothing to fit


def test_pristine_scalars(shim):
    # algo_thresh = Lg / delta_x - (pixel_thresh - 1): 500 / 5 - 4 = 96; 8 / 5 - 4 < 0 -> a trace that is done before it starts
    ps = [edge(score_thresh=3), edge(x_st=0, x_en=7, score_thresh=9)]
    out = (C.c_int * 8)()
    assert shim.shim_pristine(2, 500, 500, _flat(ps), out) == 0
    assert list(out) == [0, 0, 3, 1, 1, 0, 9, 1]
