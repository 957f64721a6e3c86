"""The normals store of a batch (csrc/gpet_zstore_plan.h, gpet_api_loop.hip): a trace must be what a batch WITHOUT a store computes,
bit for bit -- iterations, observation sets, traces -- whatever was traced before, and ``normals_generated`` (gpet_batch_info) must
say that a repeated trace draws nothing again.

The reference of every comparison is the same calls on a batch with ``normals_store = 0``.  Shapes: three edges of 80 columns
(even and >= 64: what the register-resident generator accepts; not a multiple of a 64-column GEMM tile) on one 96 x 96 synthetic
image, 64 samples, RBF, and one single-edge batch (the side stream's deep look-ahead without the chunked head's table split; the
three-edge batches run the head).  64 samples are reachable through the C ABI only, so the batches come from tests/injected_batch.py
and the trace is driven as GP_Edge_Tracing_Batch drives it: gpet_trace_iterate until no edge is left, the converged fits seeded by
seed + iterations, the means rounded to pixels.

``normals_generated`` counts the (edge, iteration) streams generated for iterations the edge went on to run; ``normals_drawn``
counts what the launches into the store generated, exactly, look-ahead for edges that then finished included (those slots are
tagged and found by a later, longer trace).  A trace that finds everything stored moves neither.  In the new-image case no edge
may run longer on the second image than on the first -- such an edge would need streams nobody has drawn -- which the test states
as a precondition on its images; then neither count moves."""
import numpy as np
import pytest

from tests.injected_batch import make_batch

pytestmark = pytest.mark.gpu

M = N = 96
X_ST, LG, S = 8, 80, 64
SEEDS3 = [11, 1008, 2005]   # 997 apart: no (edge, iteration) shares a stream with another
GEN_OPTS = {"fast": dict(rng4=1), "default": {}}


def ridge_image(shift):
    """A bright ridge through (X_ST, 48) and (X_ST + LG - 1, 48) over noise; `shift` bends it between its ends."""
    rng = np.random.default_rng(5)
    x = np.arange(N, dtype=np.float64)
    f = 48.0 + 22.0 * np.sin(2 * np.pi * (x - X_ST) / (LG - 1)) + shift * np.sin(np.pi * (x - X_ST) / (LG - 1))
    y = np.arange(M, dtype=np.float64)[:, None]
    g = np.exp(-0.5 * ((y - f[None, :]) / 2.0) ** 2) + 0.2 * rng.random((M, N))
    return (g / g.max()).astype(np.float32)


IMG_A, IMG_B = ridge_image(0.0), ridge_image(9.0)
INIT = np.array([[X_ST, 48], [X_ST + LG - 1, 48]], dtype=np.int64)


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def new_batch(amd, ctx, n_edges, store, img=IMG_A, gen="fast", **options):
    b = make_batch(amd, ctx, img, [(X_ST, LG)] * n_edges, S, M=M, inits=[INIT] * n_edges)
    for name, value in dict(GEN_OPTS[gen], normals_store=store, **options).items():
        b.set_option(name, value)
    return b


def trace(b, seeds):
    """(iterations, observation sets, traces) of one whole trace from the batch's current state."""
    n, calls = b.B, 0
    while n > 0:
        n = b.iterate(seeds, 64)
        calls += 1
        assert calls <= 4, "no convergence"
    iters = [int(s.iter) for s in b.all_scalars()]
    obs = b.read_obs_all()
    mean = b.final_fit_all([s + k for s, k in zip(seeds, iters)])[0]
    return iters, obs, [np.rint(mean[e, :LG]) for e in range(b.B)]  # (whole pixels, kept as floats: a fit that failed is NaN on both sides)


def same(got, want):
    assert got[0] == want[0], (got[0], want[0])
    for e in range(len(want[0])):
        assert np.array_equal(got[1][e], want[1][e]), "observations of edge %d" % e
        assert np.array_equal(got[2][e], want[2][e], equal_nan=True), "trace of edge %d" % e


def generated(b):
    return b.info()["normals_generated"]


def drawn(b):
    return b.info()["normals_drawn"]


@pytest.fixture(scope="module")
def ref(amd, ctx):
    """Traces of fresh store-less batches, computed once per (edges, seeds, image, generator, state changes) and never modified."""
    memo = {}

    def get(seeds, img="A", gen="fast", rng=None, dtype=None):
        key = (tuple(seeds), img, gen, rng, dtype)
        if key not in memo:
            b = new_batch(amd, ctx, len(seeds), 0, IMG_A if img == "A" else IMG_B, gen)
            try:
                if rng:
                    b.set_rng(rng)
                if dtype:
                    b.set_sample_dtype(dtype)
                memo[key] = trace(b, list(seeds))
                assert b.info()["zstore_iters"] == 0 and b.info()["zstore_mib"] == 0
            finally:
                b.close()
        return memo[key]
    return get


@pytest.mark.parametrize("n_edges,gen", [(3, "fast"), (3, "default"), (1, "default")])
def test_repeat_trace_draws_nothing_again(amd, ctx, ref, n_edges, gen):
    seeds = SEEDS3[:n_edges]
    want = ref(seeds, gen=gen)
    assert min(want[0]) >= 3, want[0]  # (several iterations: the shapes were chosen for it)
    b = new_batch(amd, ctx, n_edges, -1, gen=gen)
    try:
        assert b.info()["zstore_iters"] == 0  # (not before the first trace)
        first = trace(b, seeds)
        inf = b.info()
        assert inf["zstore_iters"] == 12 and inf["zstore_mib"] == (12 * n_edges * 8 * S * inf["z_cols"]) >> 20
        g1, d1 = generated(b), drawn(b)
        print("iterations", first[0], "generated", g1, "drawn", d1)
        assert g1 == sum(first[0])
        # drawn: at least what was used of the store, at most every slot of it (look-ahead past the edges' last iterations)
        assert sum(min(k, 12) for k in first[0]) <= d1 <= 12 * n_edges
        same(first, want)
        for _ in range(2):
            b.reset()
            same(trace(b, seeds), want)
            assert generated(b) == g1 and drawn(b) == d1
    finally:
        b.close()


def test_one_seed_changed(amd, ctx, ref):
    b = new_batch(amd, ctx, 3, -1)
    try:
        same(trace(b, SEEDS3), ref(SEEDS3))
        g1 = generated(b)
        seeds = [SEEDS3[0], 4999, SEEDS3[2]]
        want = ref(seeds)
        b.reset()
        same(trace(b, seeds), want)
        assert generated(b) - g1 == want[0][1], (generated(b) - g1, want[0])
        g2 = generated(b)
        b.reset()  # ... and the old seed again: its slots were overwritten, the others' were not
        same(trace(b, SEEDS3), ref(SEEDS3))
        assert generated(b) - g2 == ref(SEEDS3)[0][1]
    finally:
        b.close()


def test_short_store_generates_its_ring_iterations_on_every_trace(amd, ctx, ref):
    want = ref(SEEDS3)
    assert min(want[0]) > 2
    b = new_batch(amd, ctx, 3, -1, normals_store_iters=2)
    try:
        same(trace(b, SEEDS3), want)
        assert b.info()["zstore_iters"] == 2
        g1 = generated(b)
        assert g1 == sum(want[0])
        for k in (1, 2):
            b.reset()
            same(trace(b, SEEDS3), want)
            assert generated(b) - g1 == k * sum(i - 2 for i in want[0])
    finally:
        b.close()


def test_new_image_same_seeds(amd, ctx, ref):
    on_a, on_b = ref(SEEDS3), ref(SEEDS3, img="B")
    assert on_a[1][0].tobytes() != on_b[1][0].tobytes() or on_a[0] != on_b[0]  # (another image: another trace)
    b = new_batch(amd, ctx, 3, -1)
    try:
        # the images were chosen so that no edge runs longer on B than on A: everything B needs was drawn for A
        assert all(kb <= ka for ka, kb in zip(on_a[0], on_b[0])), (on_a[0], on_b[0])
        same(trace(b, SEEDS3), on_a)
        g1, d1 = generated(b), drawn(b)
        b.set_images([IMG_B], next_frame=False)
        same(trace(b, SEEDS3), on_b)
        print("iterations", on_a[0], on_b[0], "generated", g1, generated(b), "drawn", d1, drawn(b))
        assert generated(b) == g1 and drawn(b) == d1
        b.set_images([IMG_A], next_frame=False)  # back: nothing the store has not seen
        same(trace(b, SEEDS3), on_a)
        assert generated(b) == g1 and drawn(b) == d1
    finally:
        b.close()


def test_invalidation(amd, ctx, ref):
    b = new_batch(amd, ctx, 3, -1)
    try:
        assert b.info()["structured"] == 1
        same(trace(b, SEEDS3), ref(SEEDS3))
        b.set_rng("philox")
        b.reset()
        same(trace(b, SEEDS3), ref(SEEDS3, rng="philox"))
        b.set_rng("mt19937")
        b.reset()
        same(trace(b, SEEDS3), ref(SEEDS3))
        b.set_sample_dtype("f32")
        b.reset()
        g = generated(b)
        same(trace(b, SEEDS3), ref(SEEDS3, dtype="f32"))
        assert generated(b) == g  # (the sample type changes nothing about the normals)
        b.set_sample_dtype("f64")
        # an off-grid observation takes the batch off the structured path for good (every column of a row is then multiplied):
        # the same calls on a store-less batch
        off = np.array([[2, 40]], dtype=np.int64)
        on = np.array([[40, 50]], dtype=np.int64)
        r = new_batch(amd, ctx, 3, 0)
        try:
            got, want = [], []
            for bb, out in ((b, got), (r, want)):
                bb.reset()
                bb.set_obs(1, off)
                assert bb.info()["structured"] == 0
                out.append(trace(bb, SEEDS3))
                bb.reset()
                bb.set_obs(1, on)
                out.append(trace(bb, SEEDS3))
                bb.reset()
                out.append(trace(bb, SEEDS3))
        finally:
            r.close()
        for g_, w_ in zip(got, want):
            same(g_, w_)
    finally:
        b.close()


def test_injected_normals_in_a_store_slot(amd, ctx, ref):
    """The injection pattern of tests/test_gpu_sample_gemm_exact.py (integers times multiples of 2^-20: every sum exact) on edge 1 of
    a batch whose iteration 0 lives in the store: 80 columns = one full 64-column tile and a ragged one, 64 rows."""
    L = amd._lib
    b = new_batch(amd, ctx, 3, -1)
    try:
        same(trace(b, SEEDS3), ref(SEEDS3))
        assert b.info()["zstore_iters"] == 12
        g1 = generated(b)
        b.reset()
        e, r = 1, 37
        inf = b.info(e)
        rng = np.random.default_rng(3)
        grain = lambda shape: rng.integers(-4 * 2 ** 20, 4 * 2 ** 20 + 1, size=shape).astype(np.float64) / 2.0 ** 20
        b.fit_predict(want_cov=False)
        assert b.scalars(e).iter == 0
        mu, A = grain(LG), grain((r, LG))
        b.write(L.BUF_MEAN, mu, e)
        s = b.scalars(e)
        s.y_s = 1.5
        b.write_scalars(s, e)
        Z = rng.integers(-8, 9, size=(S, inf["z_cols"])).astype(np.float64)
        exp = (Z[:, :r] @ A + mu) * 1.5
        Z[:, r:] = np.nan
        b.write(L.BUF_FACTOR, A, e, rows=r)
        b.write(L.BUF_NORMALS, Z, e)
        b.write(L.BUF_SAMPLES, np.full((S, LG), np.nan), e)
        assert np.array_equal(b.read(L.BUF_NORMALS, e)[:, :r], Z[:, :r])
        b.sample()
        got = b.read(L.BUF_SAMPLES, e)
        assert np.array_equal(got, exp), np.argwhere(got != exp)[:8].tolist()
        # a following loop draws that slot again, and only that one
        b.clear_injected_factor(e)
        b.reset()
        same(trace(b, SEEDS3), ref(SEEDS3))
        assert generated(b) - g1 == 1
    finally:
        b.close()


def test_stage_generators_leave_the_tags_right(amd, ctx, ref):
    """gpet_profile_stage 2 draws, by the loop's seed rule from the seeds on the device, what the loop would draw: the store stays
    valid and the next trace draws nothing.  gpet_gp_normals with seeds of the caller's writes every edge's slot of iteration 0:
    exactly those three are drawn again."""
    want = ref(SEEDS3)
    b = new_batch(amd, ctx, 3, -1)
    try:
        same(trace(b, SEEDS3), want)
        g1, d1 = generated(b), drawn(b)
        b.reset()
        b.profile_stage(2, 1)
        same(trace(b, SEEDS3), want)
        assert generated(b) == g1 and drawn(b) == d1
        b.reset()
        b.normals([900001, 900002, 900003])
        same(trace(b, SEEDS3), want)
        assert generated(b) - g1 == 3 and drawn(b) - d1 == 3
        b.reset()
        same(trace(b, SEEDS3), want)
        assert generated(b) - g1 == 3 and drawn(b) - d1 == 3
    finally:
        b.close()


def test_a_destroyed_batch_leaves_its_store_to_the_next(amd, ctx, ref):
    """Create, trace once, destroy, again and again: the store's block is handed on, and every batch computes the same."""
    want = ref(SEEDS3)
    for _ in range(3):
        b = new_batch(amd, ctx, 3, -1)
        try:
            same(trace(b, SEEDS3), want)
            assert b.info()["zstore_iters"] == 12 and generated(b) == sum(want[0])
        finally:
            b.close()


def test_refused_store(amd, ctx, ref):
    b = new_batch(amd, ctx, 3, 1, normals_store_iters=0)
    try:
        same(trace(b, SEEDS3), ref(SEEDS3))
        inf = b.info()
        assert inf["zstore_iters"] == 0 and inf["zstore_mib"] == 0
        g1 = generated(b)
        b.reset()
        same(trace(b, SEEDS3), ref(SEEDS3))
        assert generated(b) == 2 * g1 == 2 * sum(ref(SEEDS3)[0])
    finally:
        b.close()
