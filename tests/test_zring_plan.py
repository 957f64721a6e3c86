"""CPU tests of the ring tags' rules (csrc/gpet_zstore_plan.h), through the shim pattern of tests/test_zstore_plan.py.  Every
expectation is a literal derived by hand from the rules the header states: iteration k >= store_iters lies in ring slot k % ring;
the tag of a slot is the loop's tag of the iteration it holds; an edge misses, from the first to the last iteration, where a slot's
tag is not what the loop would draw there; a launch empties the tags of the slots it may overwrite when it is enqueued and sets
them when it is settled -- for a finished edge of a table that reads `done` only below its iteration counter."""
import ctypes as C
import subprocess

import pytest

from tests.test_loop_plan import CSRC, _compiler

SHIM = r"""
#include "gpet_zstore_plan.h"
using namespace gpet;
extern "C" {
unsigned long long shim_loop_tag(unsigned int base, int iter, int mode, int zs) { return zstore_loop_tag(base, iter, mode, zs); }
int shim_slot(int iter, int ring) { return zring_slot(iter, ring); }
int shim_ring_max() { return kZRingMax; }
int shim_misses(const unsigned long long* rtags, int ring, const int* idx, const unsigned int* seeds, int n_edges, int from, int n, int mode,
                int zs, int* lo, int* hi) {
  return zring_misses(reinterpret_cast<const uint64_t*>(rtags), ring, idx, seeds, n_edges, from, n, mode, zs, lo, hi);
}
void shim_clear(unsigned long long* rtags, int ring, const int* idx, int n_edges, int from, int n) {
  zring_clear(reinterpret_cast<uint64_t*>(rtags), ring, idx, n_edges, from, n);
}
void shim_settle(unsigned long long* rtags, int ring, int e, unsigned int seed, int from, int n, int done, int iter, int certain, int mode, int zs) {
  zring_settle(reinterpret_cast<uint64_t*>(rtags), ring, e, seed, from, n, done, iter, certain, mode, zs);
}
int shim_keep(int option, int inline_mode, int ring) { return zring_keep(option, inline_mode != 0, ring) ? 1 : 0; }
}
"""
ZS = 72


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("zring_plan")
    src, so = d / "shim.cpp", d / "libzring_plan_shim.so"
    src.write_text(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.shim_loop_tag.restype = C.c_ulonglong
    lib.shim_loop_tag.argtypes = [C.c_uint, C.c_int, C.c_int, C.c_int]
    return lib


class Ring:
    """The ring tags of a batch, [edges][ring], as the host keeps them."""

    def __init__(self, shim, seeds, ring):
        self.shim, self.seeds, self.ring = shim, list(seeds), ring
        self.tags = (C.c_ulonglong * (len(seeds) * ring))()

    def _idx(self, idx):
        return None if idx is None else (C.c_int * len(idx))(*idx)

    def rows(self):
        return [list(self.tags[e * self.ring:(e + 1) * self.ring]) for e in range(len(self.seeds))]

    def tag(self, e, it, mode=0, zs=ZS):
        return self.shim.shim_loop_tag(self.seeds[e], it, mode, zs)

    def misses(self, from_, n, seeds=None, idx=None, mode=0, zs=ZS):
        seeds = self.seeds if seeds is None else seeds
        n_edges = len(idx) if idx is not None else len(seeds)
        lo, hi = (C.c_int * n_edges)(), (C.c_int * n_edges)()
        cnt = self.shim.shim_misses(self.tags, self.ring, self._idx(idx), (C.c_uint * len(seeds))(*seeds), n_edges, from_, n, mode, zs, lo, hi)
        out = [(a, b) if a <= b else None for a, b in zip(lo, hi)]
        assert cnt == sum(1 for r in out if r is not None)
        return out

    def clear(self, from_, n, idx=None):
        self.shim.shim_clear(self.tags, self.ring, self._idx(idx), len(idx) if idx is not None else len(self.seeds), from_, n)

    def settle(self, e, from_, n, done, it, certain=0, mode=0, zs=ZS):
        self.shim.shim_settle(self.tags, self.ring, e, self.seeds[e], from_, n, done, it, certain, mode, zs)

    def launch(self, from_, n, state, idx=None, certain=0):
        """enqueue + settle of one launch for the edges idx (None: all); state[e] = (done, iter) afterwards"""
        self.clear(from_, n, idx)
        for e in (range(len(self.seeds)) if idx is None else idx):
            self.settle(e, from_, n, state[e][0], state[e][1], certain)


def test_slot_of_an_iteration(shim):
    assert shim.shim_ring_max() == 16
    # ring 9 (batches above 64 edges) behind a store of 12: iterations 12 .. 20 take nine distinct slots, 21 comes back to 12's
    assert [shim.shim_slot(k, 9) for k in range(12, 22)] == [3, 4, 5, 6, 7, 8, 0, 1, 2, 3]
    assert [shim.shim_slot(k, 9) for k in (0, 8, 9, 17, 18)] == [0, 8, 0, 8, 0]
    # ring 16 (up to 64 edges)
    assert [shim.shim_slot(k, 16) for k in (0, 2, 15, 16, 17, 31, 32)] == [0, 2, 15, 0, 1, 15, 0]


def test_the_switch(shim):
    assert shim.shim_keep(-1, 1, 9) == 1 and shim.shim_keep(1, 1, 16) == 1    # automatic and its reserved twin: the inline modes
    assert shim.shim_keep(0, 1, 9) == 0                                       # never
    assert shim.shim_keep(-1, 0, 9) == 0 and shim.shim_keep(1, 0, 16) == 0    # the side-stream modes regenerate on every trace
    assert shim.shim_keep(-1, 1, 0) == 0 and shim.shim_keep(-1, 1, 17) == 0   # no tags (rings of different lengths), no such ring


def test_miss_ranges_empty_full_and_one_foreign_seed(shim):
    seeds = [100, 200, 300]
    r = Ring(shim, seeds, 9)
    # an empty ring: every edge misses the whole range (the cold trace: one launch for the table)
    assert r.misses(12, 4) == [(12, 15)] * 3
    assert r.misses(12, 1) == [(12, 12)] * 3
    # iterations 12 .. 17 drawn for running edges: tagged, nobody misses, whatever part of them is asked for
    running = [(0, 18)] * 3
    r.launch(12, 4, running)
    r.launch(16, 2, running)
    assert r.rows()[1] == [0, 0, 0, r.tag(1, 12), r.tag(1, 13), r.tag(1, 14), r.tag(1, 15), r.tag(1, 16), r.tag(1, 17)]
    assert r.misses(12, 4) == [None] * 3 and r.misses(16, 2) == [None] * 3 and r.misses(13, 5) == [None] * 3
    # ... the iterations after them were never drawn: a tail
    assert r.misses(16, 4) == [(18, 19)] * 3
    # one foreign seed: that edge, all of the range; another mode or stored column count: everybody's
    assert r.misses(12, 4, seeds=[100, 201, 300]) == [None, (12, 15), None]
    assert r.misses(12, 4, mode=1) == [(12, 15)] * 3 and r.misses(14, 2, zs=68) == [(14, 15)] * 3
    # seed 201 at iteration 12 draws what seed 200 draws at iteration 13 -- but into another slot: still a miss
    assert shim.shim_loop_tag(201, 12, 0, ZS) == shim.shim_loop_tag(200, 13, 0, ZS)
    # one slot emptied (an injected ring slot): that edge, that iteration; two holes: from the first to the last
    r.tags[2 * 9 + 14 % 9] = 0
    assert r.misses(12, 4) == [None, None, (14, 14)]
    r.tags[2 * 9 + 12 % 9] = 0
    assert r.misses(12, 6) == [None, None, (12, 14)]


def test_wrap_without_a_store(shim):
    """No store, ring 9, a trace of 10 iterations: iteration 9 lands on iteration 0's slot."""
    r = Ring(shim, [7], 9)
    done10 = [(1, 10)]
    assert shim.shim_slot(9, 9) == shim.shim_slot(0, 9) == 0
    # trace 1: groups [0, 8) and [8, 10), the edge runs all ten
    assert r.misses(0, 8) == [(0, 7)]
    r.launch(0, 8, [(0, 8)])
    assert r.misses(8, 2) == [(8, 9)]
    r.launch(8, 2, done10)
    assert r.rows()[0] == [r.tag(0, 9)] + [r.tag(0, k) for k in range(1, 9)]
    # trace 2: iteration 0 misses (its slot holds iteration 9), 1 .. 7 do not
    assert r.misses(0, 8) == [(0, 0)]
    r.launch(0, 1, [(0, 8)], idx=[0], certain=1)
    assert r.rows()[0][0] == r.tag(0, 0)
    # ... and once it is redrawn, iteration 9 misses; 8 does not
    assert r.misses(8, 2) == [(9, 9)]
    r.launch(9, 1, done10, idx=[0], certain=1)
    assert r.rows()[0] == [r.tag(0, 9)] + [r.tag(0, k) for k in range(1, 9)]
    # trace 3 finds what trace 2 found: two of ten iterations are drawn per repeat, not ten
    assert r.misses(0, 8) == [(0, 0)]


def test_clear_at_enqueue_set_at_settle(shim):
    seeds = [100, 200]
    r = Ring(shim, seeds, 9)
    r.launch(12, 4, [(0, 16)] * 2)
    before = r.rows()
    # enqueued: the slots of the launch's iterations are empty for its edges, the others untouched
    r.clear(14, 3, idx=[1])
    assert r.rows()[0] == before[0]
    assert r.rows()[1] == [0, 0, 0, r.tag(1, 12), r.tag(1, 13), 0, 0, 0, 0]
    assert r.misses(12, 4) == [None, (14, 15)]
    # a launch that is never settled (the call ended in an error) leaves them empty
    # settled, edge 1 finished with its counter at 15 (it ran 14, not 15 or 16) under a table that reads `done`: only 14 is known
    r.settle(1, 14, 3, 1, 15)
    assert r.rows()[1] == [0, 0, 0, r.tag(1, 12), r.tag(1, 13), r.tag(1, 14), 0, 0, 0]
    # ... still running: all three; finished, but every stream generated for certain (a never-`done` table): all three
    r.clear(14, 3, idx=[1])
    r.settle(1, 14, 3, 0, 17)
    assert r.rows()[1] == [0, 0, 0] + [r.tag(1, k) for k in range(12, 17)] + [0]
    r.clear(14, 3, idx=[1])
    r.settle(1, 14, 3, 1, 15, certain=1)
    assert r.rows()[1] == [0, 0, 0] + [r.tag(1, k) for k in range(12, 17)] + [0]
    # finished before the launch's first iteration: nothing is known to be there
    r.clear(14, 3, idx=[1])
    r.settle(1, 14, 3, 1, 13)
    assert r.rows()[1] == [0, 0, 0, r.tag(1, 12), r.tag(1, 13), 0, 0, 0, 0]
    # a launch of a whole ring's length or more empties every slot of its edges
    r.clear(12, 9, idx=[0])
    assert r.rows()[0] == [0] * 9
    r.clear(0, 40, idx=[1])
    assert r.rows()[1] == [0] * 9


def test_a_compacted_table_indexes_tags_by_the_original_edge(shim):
    seeds = [100, 200, 300, 400]
    r = Ring(shim, seeds, 16)
    state = [(0, 24)] * 4
    r.launch(16, 4, state)
    r.tags[3 * 16 + 18 % 16] = 0
    # entries 0, 1 of the table are the batch's edges 3, 1 -- tags and seeds are indexed by the batch's edge
    assert r.misses(16, 4, idx=[3, 1]) == [(18, 18), None]
    assert r.misses(16, 4, idx=[0, 2]) == [None, None]
    # a launch for the table (3, 1) clears and sets edges 3 and 1 only
    r.launch(20, 2, state, idx=[3, 1])
    rows = r.rows()
    assert rows[0][4:6] == [0, 0] and rows[2][4:6] == [0, 0]
    assert rows[1][4:6] == [r.tag(1, 20), r.tag(1, 21)] and rows[3][4:6] == [r.tag(3, 20), r.tag(3, 21)]
    assert rows[3][0:4] == [r.tag(3, 16), r.tag(3, 17), 0, r.tag(3, 19)]
