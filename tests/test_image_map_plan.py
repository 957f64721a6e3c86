"""CPU tests of the image map of a batch (csrc/gpet_batch_plan.h: image_map_check, image_map_reps, the layout_batch overload that
takes the map).  The header needs no HIP: a small extern "C" shim around it is compiled with the host C++ compiler and driven
through ctypes, as tests/test_batch_plan.py does -- whose shim (for the layouts without a map), edges and documented buffer sizes
are reused here, so the two layouts are compared through the same code."""
import ctypes as C
import subprocess

import pytest

from tests.test_batch_plan import CSRC, PTR_FIELDS, _MIX, _compiler, _flat, _sizes, edge, plan
from tests.test_batch_plan import shim  # noqa: F401  (the fixture that builds the layouts without a map)

SHIM = r"""
#include "gpet_batch_plan.h"
using namespace gpet;
#define PTR_FIELDS(X) X(grad) X(grad_kde) X(init_xy) X(obs_xy) X(obs_new) X(sc) X(xt) X(yt) X(wt) X(K) X(alpha) X(chol_inv) X(solve_z) \
  X(solve_flag) X(V) X(mean) X(std) X(cov) X(G) X(perm) X(C) X(W) X(theta) X(Wq) X(Cw) X(wq_tag) X(order) X(Q0) X(lam0) X(beta) X(h0) \
  X(jlog) X(eig) X(Gt) X(Ap) X(ap_tag) X(pcx_d) X(pcx_cand) X(A) X(Z) X(Y) X(costs) X(cost_part) X(best_costs) X(best_idx) X(bins) \
  X(tmpk) X(kde) X(kde_band) X(kde_wsum) X(colsum) X(colbest) X(colbest_y) X(mm) X(binbest) X(binarg) X(fin_x) X(fin_y) X(fin_w) \
  X(fin_par) X(fin_out) X(rho_tab)
static long long off_of(const char* base, const void* p) { return p ? (long long)((const char*)p - base) : -1; }
extern "C" {
// what image_map_check says (nullptr: the empty string)
const char* shim_map_check(int B, int n_img, const int* image_of) {
  const char* why = image_map_check(B, n_img, image_of);
  return why ? why : "";
}
void shim_map_reps(int B, int n_img, const int* image_of, int* rep) { image_map_reps(B, n_img, image_of, rep); }
// the layout with a map: offs B x 62 pointer offsets of the placing pass, batch: the five block offsets, end of the measuring
// pass, end of the placing pass
int shim_plan_mapped(int B, int M, int N, const double* v, int n_img, const int* image_of, long long* offs, long long* batch) {
  std::vector<gpet_params> ps((size_t)B);
  for (int e = 0; e < B; ++e, v += 18) {  // 18 doubles per edge, in the order of gpet_params
    gpet_params& p = ps[(size_t)e];
    memset(&p, 0, sizeof p);
    p.kernel_type = (int)v[0]; p.nu = v[1]; p.sigma_f = v[2]; p.length_scale = v[3]; p.noise_y = v[4]; p.n_samples = (int)v[5];
    p.n_keep = (int)v[6]; p.delta_x = (int)v[7]; p.pixel_thresh = (int)v[8]; p.score_thresh = v[9]; p.fix_endpoints = (int)v[10];
    p.x_st = (int)v[11]; p.x_en = (int)v[12]; p.n_init = (int)v[13]; p.obs_cap = (int)v[14]; p.factor_cap = (int)v[15];
    p.z_cols = (int)v[16]; p.jitter = v[17];
  }
  std::vector<EdgeDev> edges((size_t)B);
  const bool any_big = any_big_edge(ps.data(), B);
  for (int e = 0; e < B; ++e)
    if (resolve_edge(edges[(size_t)e], ps[(size_t)e], B, M, N, any_big, 32) != EdgeCheck::ok) return -1;
  const BatchDims bd = reduce_dims(edges.data(), B, M, N);
  Carver meas;
  layout_batch(meas, edges.data(), B, bd, n_img, image_of);
  static char anchor;  // (a non-null base: the layout only does address arithmetic)
  Carver cv;
  cv.base = &anchor;
  const BatchBlocks bb = layout_batch(cv, edges.data(), B, bd, n_img, image_of);
  for (int e = 0; e < B; ++e) {
    const EdgeDev& E = edges[(size_t)e];
#define X(f) *offs++ = off_of(&anchor, E.f);
    PTR_FIELDS(X)
#undef X
  }
  batch[0] = off_of(&anchor, bb.scalars); batch[1] = off_of(&anchor, bb.fin_out); batch[2] = off_of(&anchor, bb.fin_par);
  batch[3] = off_of(&anchor, bb.obs); batch[4] = off_of(&anchor, bb.init); batch[5] = (long long)meas.off; batch[6] = (long long)cv.off;
  return 0;
}
}
"""

MAP6 = [0, 1, 2, 0, 1, 2]
# B = 6: the bench edge at 500 x 500, and the mixed-width edges of test_batch_plan (77 x 410) twice over
LAYOUTS = {"bench": ([edge()] * 6, 500, 500), "mixed": (_MIX + _MIX, 77, 410)}


@pytest.fixture(scope="module")
def mshim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("image_map_plan")
    src, so = d / "shim.cpp", d / "libimage_map_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.shim_map_check.restype = C.c_char_p
    return lib


def _ints(v):
    return (C.c_int * max(1, len(v)))(*v)


def check(mshim, B, n_img, image_of):
    return mshim.shim_map_check(B, n_img, _ints(image_of)).decode()


def plan_mapped(mshim, ps, M, N, n_img, image_of):
    B = len(ps)
    offs, batch = (C.c_longlong * (62 * B))(), (C.c_longlong * 7)()
    assert mshim.shim_plan_mapped(B, M, N, _flat(ps), n_img, _ints(image_of), offs, batch) == 0
    edges = [dict(zip(PTR_FIELDS, offs[62 * e:62 * e + 62])) for e in range(B)]
    return dict(edges=edges, blocks=dict(zip(("scalars", "fin_out", "fin_par", "obs", "init"), batch[:5])), meas_end=batch[5],
                place_end=batch[6])


def test_checker_accepts_valid_maps(mshim):
    assert check(mshim, 6, 3, MAP6) == ""
    assert check(mshim, 6, 1, [0] * 6) == ""
    assert check(mshim, 6, 6, [5, 4, 3, 2, 1, 0]) == ""
    assert check(mshim, 1, 1, [0]) == ""


def test_checker_refuses_each_bad_map_with_its_own_message(mshim):
    why = dict(no_slot=check(mshim, 6, 0, [0] * 6), negative_slots=check(mshim, 6, -2, [0] * 6), too_many=check(mshim, 6, 7, [0, 1, 2, 3, 4, 5]),
               above=check(mshim, 6, 3, [0, 1, 3, 0, 1, 2]), below=check(mshim, 6, 3, [0, 1, -1, 0, 1, 2]), unused=check(mshim, 6, 3, [0, 1, 0, 0, 1, 1]))
    assert all(why.values()), why
    assert why["no_slot"] == why["negative_slots"] and why["above"] == why["below"]
    assert len({why["no_slot"], why["too_many"], why["above"], why["unused"]}) == 4, why
    assert "at least 1" in why["no_slot"] and "more image slots than edges" in why["too_many"]
    assert "outside" in why["above"] and "no edge" in why["unused"]


@pytest.mark.parametrize("image_of,n_img,want", [(MAP6, 3, [0, 1, 2]), ([2, 2, 0, 1, 0, 1], 3, [2, 3, 0]), ([0] * 6, 1, [0]),
                                                 ([5, 4, 3, 2, 1, 0], 6, [5, 4, 3, 2, 1, 0]), ([0, 0, 1, 1, 2, 2], 3, [0, 2, 4])])
def test_representative_of_a_slot_is_its_first_edge(mshim, image_of, n_img, want):
    rep = (C.c_int * n_img)()
    mshim.shim_map_reps(len(image_of), n_img, _ints(image_of), rep)
    assert list(rep) == want
    assert want == [image_of.index(g) for g in range(n_img)]


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_mapped_layout_shares_slots_and_is_aligned_disjoint_and_inside_the_arena(mshim, shim, name):
    ps, M, N = LAYOUTS[name]
    own = plan(shim, ps, M, N, 0)  # (the resolved fields and the batch dimensions: the map does not change them)
    p = plan_mapped(mshim, ps, M, N, 3, MAP6)
    scalars_bytes, eig_bytes = shim.shim_sizes(0), shim.shim_sizes(1)
    spans, slots = set(), {}
    for e, off in enumerate(p["edges"]):
        size = _sizes(own["edges"][e], own["bd"], scalars_bytes, eig_bytes)
        for f in PTR_FIELDS:
            assert off[f] >= 0, (e, f)
            if f not in ("sc", "fin_out", "fin_par", "obs_xy", "init_xy"):
                assert off[f] % 256 == 0, (e, f)
            if f in ("grad", "grad_kde"):  # the edges of a slot share the pair: the same buffer, counted once
                first = slots.setdefault((f, MAP6[e]), off[f])
                assert off[f] == first, (e, f)
                if MAP6.index(MAP6[e]) != e:
                    continue
            spans.add((off[f], off[f] + size[f], e, f))
    assert len(set(slots.values())) == 6  # three slots x (grad, grad_kde), all distinct
    for k in ("scalars", "fin_out", "fin_par", "obs", "init"):
        assert p["blocks"][k] % 256 == 0
    order = sorted(spans)
    for (a0, a1, ea, fa), (b0, b1, eb, fb) in zip(order, order[1:]):
        assert a1 <= b0, ("overlap", ea, fa, eb, fb)
    assert order[0][0] >= 0 and order[-1][1] <= p["meas_end"] and p["place_end"] == p["meas_end"]
    # the slots are at the front of the arena, where the shared pair is taken
    px = 4 * M * N
    pitch = (px + 255) // 256 * 256
    assert sorted(slots.values()) == [k * pitch for k in range(6)]
    assert p["blocks"]["scalars"] == 6 * pitch


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_all_zero_map_is_the_shared_layout_exactly(mshim, shim, name):
    ps, M, N = LAYOUTS[name]
    shared = plan(shim, ps, M, N, 1)
    p = plan_mapped(mshim, ps, M, N, 1, [0] * 6)
    assert p["meas_end"] == shared["meas_end"] and p["place_end"] == shared["place_end"]
    assert p["blocks"] == shared["blocks"]
    for e in range(6):
        assert p["edges"][e] == shared["edges"][e]["off"], e


@pytest.mark.parametrize("name", sorted(LAYOUTS))
@pytest.mark.parametrize("n_img,image_of", [(3, MAP6), (2, [0, 0, 0, 1, 1, 1]), (6, [0, 1, 2, 3, 4, 5]), (1, [0] * 6)])
def test_mapped_arena_is_the_own_image_arena_minus_the_saved_pairs(mshim, shim, name, n_img, image_of):
    """Every buffer starts on a 256-byte boundary, so the end of an arena, rounded up to one, is the sum of the rounded sizes
    of its buffers: a map with n_img slots has B - n_img pairs (grad, grad_kde) fewer than one image per edge, and nothing
    else differs."""
    ps, M, N = LAYOUTS[name]
    up = lambda v: (v + 255) // 256 * 256
    own = plan(shim, ps, M, N, 0)
    p = plan_mapped(mshim, ps, M, N, n_img, image_of)
    pair = 2 * up(4 * M * N)
    assert up(own["meas_end"]) - up(p["meas_end"]) == (len(ps) - n_img) * pair
