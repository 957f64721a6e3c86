"""CPU tests of the normals store's decisions (csrc/gpet_zstore_plan.h): the header needs no HIP, so a small extern "C" shim around
it is compiled with the host C++ compiler and driven through ctypes, as tests/test_loop_plan.py does.  Every expectation is a
literal derived by hand from the rules the header states: a budget of a quarter of the free memory that never reaches into the last
eighth of the device; automatic = 12 iterations, at least 8 or none; an explicit count up to 32, fewer if the budget holds fewer;
a tag of (effective seed, rng mode, stored columns) that is never 0; a group's leading iterations below store_iters live in the
store, and an edge misses where a tag differs from what the loop would draw there."""
import ctypes as C
import subprocess

import pytest

from tests.test_loop_plan import CSRC, _compiler

SHIM = r"""
#include "gpet_zstore_plan.h"
using namespace gpet;
extern "C" {
long long shim_budget(long long fr, long long tot) { return zstore_budget(fr, tot); }
int shim_iters(int B, long long slot, long long fr, long long tot, int store, int iters) { return zstore_iters(B, slot, fr, tot, store, iters); }
unsigned long long shim_tag(unsigned int seed, int mode, int zs) { return zstore_tag(seed, mode, zs); }
unsigned long long shim_loop_tag(unsigned int base, int iter, int mode, int zs) { return zstore_loop_tag(base, iter, mode, zs); }
void shim_untag(unsigned long long t, unsigned int* out) { out[0] = zstore_tag_seed(t); out[1] = zstore_tag_mode(t); out[2] = zstore_tag_zs(t); }
int shim_span(int from, int n, int store_iters) { return zstore_span(from, n, store_iters); }
int shim_misses(const unsigned long long* tags, int store_iters, const int* idx, const unsigned int* seeds, int n_edges, int from, int n,
                int mode, int zs, int* lo, int* hi) {
  return zstore_misses(reinterpret_cast<const uint64_t*>(tags), store_iters, idx, seeds, n_edges, from, n, mode, zs, lo, hi);
}
}
"""
GB = 1 << 30
SLOT = 8 * 1000 * 96  # the headline's slot: 1 000 sample rows of z_cols = 96


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("zstore_plan")
    src, so = d / "shim.cpp", d / "libzstore_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.shim_budget.restype = C.c_longlong
    lib.shim_budget.argtypes = [C.c_longlong] * 2
    lib.shim_iters.argtypes = [C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_int, C.c_int]
    lib.shim_tag.restype = lib.shim_loop_tag.restype = C.c_ulonglong
    lib.shim_tag.argtypes = [C.c_uint, C.c_int, C.c_int]
    lib.shim_loop_tag.argtypes = [C.c_uint, C.c_int, C.c_int, C.c_int]
    lib.shim_untag.argtypes = [C.c_ulonglong, C.POINTER(C.c_uint)]
    return lib


def test_budget_is_a_quarter_of_the_free_memory_outside_the_last_eighth(shim):
    assert shim.shim_budget(256 * GB, 288 * GB) == 64 * GB
    assert shim.shim_budget(40 * GB, 288 * GB) == 4 * GB       # 40 - 10 would leave 30 < 36: only 40 - 36
    assert shim.shim_budget(48 * GB, 288 * GB) == 12 * GB      # 48 - 12 = 36: exactly the eighth stays
    assert shim.shim_budget(36 * GB, 288 * GB) == 0 and shim.shim_budget(1 * GB, 288 * GB) == 0 and shim.shim_budget(0, 0) == 0


def test_store_iters_at_the_edges_of_the_budget(shim):
    B, tot = 1024, 288 * GB
    per_iter = B * SLOT

    def iters(budget, store=-1, n=-1, B=B):
        # free = 4 x budget; total = 0 keeps the last-eighth rule, which has its own test above, out of the way
        return shim.shim_iters(B, SLOT, 4 * budget, 0, store, n)
    assert iters(12 * per_iter) == 12 and iters(100 * per_iter) == 12          # automatic: 12, however much is free
    assert iters(12 * per_iter - 1) == 11
    assert iters(8 * per_iter) == 8 and iters(8 * per_iter - 1) == 0           # at least 8, or none
    assert iters(8 * per_iter - 1, store=1) == 7 and iters(per_iter, store=1) == 1 and iters(per_iter - 1, store=1) == 0
    assert iters(100 * per_iter, store=0) == 0 and iters(100 * per_iter, store=0, n=32) == 0
    assert iters(100 * per_iter, n=32) == 32 and iters(100 * per_iter, n=40) == 32 and iters(100 * per_iter, store=1, n=99) == 32  # the cap
    assert iters(100 * per_iter, n=2) == 2 and iters(100 * per_iter, store=1, n=2) == 2  # an explicit count may be below 8
    assert iters(5 * per_iter, n=24) == 5                                       # ... and takes what the budget holds
    assert iters(100 * per_iter, n=0) == 0 and iters(100 * per_iter, store=1, n=0) == 0  # a budget of zero
    assert iters(100 * per_iter, B=0) == 0 and shim.shim_iters(B, 0, 4 * 100 * per_iter, tot, -1, -1) == 0
    # the headline: eight objects of 1 024 edges on a 288 GB part (their arenas, 8 x 19.6 GiB, are there already: 130 GiB free) get
    # 12 iterations each, the last one included; a ninth batch beside them (another arena) gets none: 5 iterations are fewer than 8
    free = 130 * GB
    for _ in range(8):
        assert shim.shim_iters(B, SLOT, free, tot, -1, -1) == 12
        free -= 12 * per_iter
    assert shim.shim_iters(B, SLOT, free - 20 * GB, tot, -1, -1) == 0 and shim.shim_iters(B, SLOT, free - 20 * GB, tot, 1, -1) == 5


def test_tag_packs_seed_mode_and_columns_and_is_never_empty(shim):
    out = (C.c_uint * 3)()
    for seed, mode, zs in [(0, 0, 0), (1, 0, 72), (0xFFFFFFFF, 1, 72), (12345, 1, 1024), (7, 0, 0xFFFFFF)]:
        t = shim.shim_tag(seed, mode, zs)
        assert t != 0 and t >> 63 == 1
        shim.shim_untag(t, out)
        assert list(out) == [seed, mode, zs]
    tags = {shim.shim_tag(s, m, z) for s in (1, 2) for m in (0, 1) for z in (68, 72)}
    assert len(tags) == 8
    # the loop's tag: the effective seed of iteration k is base + k + 1, modulo 2^32 as the generators compute it
    assert shim.shim_loop_tag(10, 0, 0, 72) == shim.shim_tag(11, 0, 72)
    assert shim.shim_loop_tag(10, 5, 1, 72) == shim.shim_tag(16, 1, 72)
    assert shim.shim_loop_tag(0xFFFFFFFF, 0, 0, 72) == shim.shim_tag(0, 0, 72)
    # edge e at iteration k + 1 and edge e + 1 at iteration k draw the same stream: the same tag (sharing the slot is future work)
    assert shim.shim_loop_tag(10, 3, 0, 72) == shim.shim_loop_tag(11, 2, 0, 72)


def test_span_of_a_group_that_straddles_the_store(shim):
    assert shim.shim_span(0, 8, 16) == 8 and shim.shim_span(8, 8, 16) == 8
    assert shim.shim_span(12, 8, 16) == 4 and shim.shim_span(15, 2, 16) == 1
    assert shim.shim_span(16, 4, 16) == 0 and shim.shim_span(20, 4, 16) == 0
    assert shim.shim_span(0, 8, 0) == 0 and shim.shim_span(3, 0, 16) == 0


def misses(shim, tags, store_iters, seeds, from_, n, mode=0, zs=72, idx=None):
    """Per entry of the launch table: the (first, last) store iteration of [from_, from_ + n) it misses, or None."""
    n_edges = len(idx) if idx is not None else len(seeds)
    lo, hi = (C.c_int * n_edges)(), (C.c_int * n_edges)()
    flat = [t for row in tags for t in row]
    cnt = shim.shim_misses((C.c_ulonglong * len(flat))(*flat), store_iters, None if idx is None else (C.c_int * n_edges)(*idx),
                           (C.c_uint * len(seeds))(*seeds), n_edges, from_, n, mode, zs, lo, hi)
    out = [(a, b) if a <= b else None for a, b in zip(lo, hi)]
    assert cnt == sum(1 for r in out if r is not None)
    return out


def test_hit_and_miss_for_a_group_that_straddles_store_iters(shim):
    seeds = [100, 200, 300]
    K = 6  # store_iters
    full = [[shim.shim_loop_tag(s, q, 0, 72) for q in range(K)] for s in seeds]
    # everything there: no edge misses, whatever the group -- iterations 6 and 7 of [4, 8) are ring iterations and nobody's miss
    assert misses(shim, full, K, seeds, 0, 4) == [None] * 3
    assert misses(shim, full, K, seeds, 4, 4) == [None] * 3
    assert misses(shim, full, K, seeds, 6, 4) == [None] * 3
    # an empty store: every edge misses, on the store's part of the group only
    empty = [[0] * K for _ in seeds]
    assert misses(shim, empty, K, seeds, 4, 4) == [(4, 5)] * 3
    assert misses(shim, empty, K, seeds, 0, 8) == [(0, 5)] * 3
    assert misses(shim, empty, K, seeds, 6, 4) == [None] * 3
    # one slot of edge 1 emptied (an injected slot): that edge, that iteration
    t = [row[:] for row in full]
    t[1][5] = 0
    assert misses(shim, t, K, seeds, 4, 4) == [None, (5, 5), None]
    assert misses(shim, t, K, seeds, 0, 4) == [None] * 3
    # another seed for edge 2: all of its iterations; another mode or another column count: everybody's
    assert misses(shim, full, K, [100, 200, 301], 0, 8) == [None, None, (0, 5)]
    assert misses(shim, full, K, seeds, 0, 8, mode=1) == [(0, 5)] * 3
    assert misses(shim, full, K, seeds, 2, 3, zs=68) == [(2, 4)] * 3
    # a compacted table: entries 0, 1 are the batch's edges 2, 0 -- tags and seeds are indexed by the batch's edge
    t = [row[:] for row in full]
    t[2][3] = 0
    assert misses(shim, t, K, seeds, 2, 4, idx=[2, 0]) == [(3, 3), None]
    assert misses(shim, t, K, seeds, 2, 4, idx=[0, 1]) == [None, None]
    # edges that ran on: edge 0 holds 0..5, edge 1 only 0..2, edge 2 all but 5 -- every edge its own range
    t = [row[:] for row in full]
    t[1][3] = t[1][4] = t[1][5] = 0
    t[2][5] = 0
    assert misses(shim, t, K, seeds, 0, 8) == [None, (3, 5), (5, 5)]
    # two holes: from the first to the last
    t = [row[:] for row in full]
    t[0][1] = t[0][4] = 0
    assert misses(shim, t, K, seeds, 0, 6) == [(1, 4), None, None]
