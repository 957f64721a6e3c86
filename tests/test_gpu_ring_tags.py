"""Ring tags (csrc/gpet_zstore_plan.h, gpet_api_loop.hip): the slots of the normals ring are tagged on the host like the store's,
so a trace repeated with the same seeds draws a ring iteration again only where its slot was overwritten since.  A trace must be
what a batch WITHOUT store and WITHOUT ring tags computes, bit for bit -- iterations, observation sets, rounded traces -- whatever
was traced before, and ``normals_generated`` / ``normals_drawn`` (gpet_batch_info) must say what was drawn.

Shapes: those of tests/test_gpu_normals_store.py (96 x 96 ridge image, 80 columns from X_ST = 8, 64 samples) with 72 edges, the
smallest batch size the suite uses above 64: ring of 9 slots, all iterations of a group in one launch on the loop's stream
(inline_per_group), seeds 11 + 997 e.  The reference of every comparison is the same calls on a batch with ``normals_store = 0`` and
``normals_ring_keep = 0``.  The store's length is chosen from the reference's longest trace so that the ring iterations do not
wrap (longest - store <= 9) and some edge runs past the store; both are asserted.  The wrap has a case of its own: no store, and an
edge long enough that the reference runs more than 9 iterations (asserted), so iteration k + 9 overwrites the slot of iteration k."""
import numpy as np
import pytest

from tests.injected_batch import make_batch
from tests.test_gpu_normals_store import IMG_A, INIT, LG, M, S, X_ST, drawn, generated, ridge_image, same, trace

pytestmark = pytest.mark.gpu

B = 72
RING = 9
SEEDS = [11 + 997 * e for e in range(B)]
OTHER = [500009 + 997 * e for e in range(B)]  # (no stream shared with SEEDS: 997 e + k + 1 stays far below)


def redrawn(img, rows=None, cols=None):
    """IMG_A with the noise of some rows or columns -- away from the ridge (rows 26 .. 70) or outside the edge's span -- replaced by
    other noise of the same height: another image for set_images to take in, whose traces differ little from IMG_A's."""
    rng = np.random.default_rng(99)
    out = img.copy()
    if rows is not None:
        out[rows, :] = (0.2 / 1.2) * rng.random(out[rows, :].shape).astype(np.float32)
    if cols is not None:
        out[:, cols] = (0.2 / 1.2) * rng.random(out[:, cols].shape).astype(np.float32)
    return out


def one_pixel(img):
    out = img.copy()
    out[2, 2] = out[2, 2] * 0.5 + 0.01
    return out


# The new-image case needs a second image on which NO edge runs longer than on the first.  The iteration count of an edge hardly
# depends on the image (the score threshold decays until pixel_thresh pixels pass: 2-3 of the 16 bins per iteration on any image) but
# moves by one or two with anything that changes a selected pixel, so among 72 edges some edge runs longer on any image that is
# really another one: a bent ridge, a faint one, gaps and more noise all gave 4-8 iterations per edge like IMG_A, never a pair.
# SECOND lists candidates from the most different to the least; the first one for which the REFERENCE satisfies the condition is
# used.  The choice looks at the reference alone, never at the batch under test.
IMAGES = {"A": IMG_A, "s4": ridge_image(4.0), "top_bottom": redrawn(IMG_A, rows=np.r_[0:12, 84:96]),
          "outside_span": redrawn(IMG_A, cols=np.r_[0:X_ST, X_ST + LG:96]), "corner_rows": redrawn(IMG_A, rows=np.r_[0:3]),
          "one_pixel": one_pixel(IMG_A)}
SECOND = ["s4", "top_bottom", "outside_span", "corner_rows", "one_pixel"]
# the wrap: one edge of 200 columns over a ridge of the same kind on a 96 x 216 image -- more bins to fill, more iterations
W_LG, W_N = 200, 216


def wide_image():
    rng = np.random.default_rng(7)
    x = np.arange(W_N, dtype=np.float64)
    f = 48.0 + 22.0 * np.sin(2 * np.pi * (x - X_ST) / (W_LG - 1))
    y = np.arange(M, dtype=np.float64)[:, None]
    g = np.exp(-0.5 * ((y - f[None, :]) / 2.0) ** 2) + 0.2 * rng.random((M, W_N))
    return (g / g.max()).astype(np.float32)


SHAPES = {
    "base": dict(img=IMG_A, span=(X_ST, LG), init=INIT),
    "wide": dict(img=wide_image(), span=(X_ST, W_LG), init=np.array([[X_ST, 48], [X_ST + W_LG - 1, 48]], dtype=np.int64)),
}


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def new_batch(amd, ctx, store, shape="base", img=None, **options):
    sh = SHAPES[shape]
    b = make_batch(amd, ctx, sh["img"] if img is None else img, [sh["span"]] * B, S, M=M, inits=[sh["init"]] * B)
    for name, value in dict(normals_store=store, **options).items():
        b.set_option(name, value)
    return b


def trace_of(b, seeds, lg):
    """tests/test_gpu_normals_store.trace for an edge of lg columns"""
    n, calls = b.B, 0
    while n > 0:
        n = b.iterate(seeds, 64)
        calls += 1
        assert calls <= 4, "no convergence"
    iters = [int(s.iter) for s in b.all_scalars()]
    obs = b.read_obs_all()
    mean = b.final_fit_all([s + k for s, k in zip(seeds, iters)])[0]
    return iters, obs, [np.rint(mean[e, :lg]) for e in range(b.B)]


@pytest.fixture(scope="module")
def ref(amd, ctx):
    """Traces of fresh batches without store and without ring tags, computed once per (seeds, image, shape, state changes)."""
    memo = {}

    def get(seeds, img="A", rng=None, shape="base"):
        key = (tuple(seeds), img, rng, shape)
        if key not in memo:
            b = new_batch(amd, ctx, 0, shape, img=IMAGES[img] if shape == "base" else None, normals_ring_keep=0)
            try:
                if rng:
                    b.set_rng(rng)
                memo[key] = trace(b, list(seeds)) if shape == "base" else trace_of(b, list(seeds), SHAPES[shape]["span"][1])
                inf = b.info()
                assert inf["zstore_iters"] == 0 and inf["z_ring"] == RING and inf["normals_generated"] == sum(memo[key][0])
            finally:
                b.close()
        return memo[key]
    return get


def store_for(iters):
    """The store's length for a reference's iteration counts: the ring iterations, up to six of them, do not wrap."""
    n = max(2, max(iters) - 6)
    print("iterations", iters, "store", n)
    assert max(iters) - n <= RING, (iters, n)           # no wrap: every ring iteration keeps its slot to itself
    assert max(iters) > n, (iters, n)                   # at least one edge runs past the store
    return n


@pytest.fixture(scope="module")
def store_len(ref):
    return store_for(ref(SEEDS)[0])


def ring_sum(iters, n):
    return sum(max(0, k - n) for k in iters)


def test_repeat_trace_draws_nothing_again(amd, ctx, ref, store_len):
    want = ref(SEEDS)
    b = new_batch(amd, ctx, -1, normals_store_iters=store_len)
    try:
        first = trace(b, SEEDS)
        assert b.info()["zstore_iters"] == store_len
        g1, d1 = generated(b), drawn(b)
        print("generated", g1, "drawn", d1)
        assert g1 == sum(first[0])
        assert sum(min(k, store_len) for k in first[0]) <= d1 <= store_len * B
        same(first, want)
        for _ in range(2):
            b.reset()
            same(trace(b, SEEDS), want)
            assert generated(b) == g1 and drawn(b) == d1
    finally:
        b.close()


def test_one_seed_changed_and_changed_back(amd, ctx, ref, store_len):
    want = ref(SEEDS)
    e = int(np.argmax(want[0]))  # (an edge that runs past the store)
    assert want[0][e] > store_len
    b = new_batch(amd, ctx, -1, normals_store_iters=store_len)
    try:
        same(trace(b, SEEDS), want)
        g1 = generated(b)
        seeds = list(SEEDS)
        seeds[e] = 4999
        want2 = ref(seeds)
        b.reset()
        same(trace(b, seeds), want2)
        assert generated(b) - g1 == want2[0][e], (generated(b) - g1, want2[0][e])
        g2 = generated(b)
        b.reset()  # ... and the old seed again: its slots were overwritten, the others' were not
        same(trace(b, SEEDS), want)
        assert generated(b) - g2 == want[0][e], (generated(b) - g2, want[0][e])
    finally:
        b.close()


def test_new_image_same_seeds(amd, ctx, ref):
    # the second image is chosen so that no edge runs longer on it than on the first: everything it needs was drawn for the first
    on_a = ref(SEEDS)
    second = next((n for n in SECOND if all(kb <= ka for ka, kb in zip(on_a[0], ref(SEEDS, img=n)[0]))), None)
    assert second is not None, {n: ref(SEEDS, img=n)[0] for n in IMAGES}
    on_b = ref(SEEDS, img=second)
    pair = ("A", second)
    assert not np.array_equal(IMAGES["A"], IMAGES[second])
    print("second image", second, "iterations", on_a[0], on_b[0], "edges with other observations",
          sum(x.tobytes() != y.tobytes() for x, y in zip(on_a[1], on_b[1])))
    store = store_for(on_a[0])
    b = new_batch(amd, ctx, -1, img=IMAGES[pair[0]], normals_store_iters=store)
    try:
        same(trace(b, SEEDS), on_a)
        g1, d1 = generated(b), drawn(b)
        assert g1 == sum(on_a[0])
        b.set_images([IMAGES[pair[1]]], next_frame=False)
        same(trace(b, SEEDS), on_b)
        assert generated(b) == g1 and drawn(b) == d1
        b.set_images([IMAGES[pair[0]]], next_frame=False)  # back: nothing store and ring have not seen
        same(trace(b, SEEDS), on_a)
        assert generated(b) == g1 and drawn(b) == d1
    finally:
        b.close()


def test_ring_keep_off_draws_the_ring_iterations_on_every_trace(amd, ctx, ref, store_len):
    want = ref(SEEDS)
    b = new_batch(amd, ctx, -1, normals_store_iters=store_len, normals_ring_keep=0)
    try:
        same(trace(b, SEEDS), want)
        g1 = generated(b)
        assert g1 == sum(want[0])
        for k in (1, 2):
            b.reset()
            same(trace(b, SEEDS), want)
            assert generated(b) - g1 == k * ring_sum(want[0], store_len)
    finally:
        b.close()


def test_an_option_flipped_between_traces_leaves_no_stale_tag(amd, ctx, ref, store_len):
    want = ref(SEEDS)
    b = new_batch(amd, ctx, -1, normals_store_iters=store_len)
    try:
        same(trace(b, SEEDS), want)
        b.reset()
        b.set_option("rng_inline", 0)   # the side stream: its launches write ring slots and keep no tags
        same(trace(b, SEEDS), want)
        b.reset()
        b.set_option("rng_inline", -1)
        same(trace(b, SEEDS), want)
        # the same with OTHER seeds on the side stream: the ring then holds numbers no tag of SEEDS may promise
        for name, value in (("rng_inline", 0), ("normals_ring_keep", 0)):
            b.reset()
            old = b.set_option(name, value)
            same(trace(b, OTHER), ref(OTHER))
            b.reset()
            b.set_option(name, old)
            same(trace(b, SEEDS), want)
    finally:
        b.close()


def test_set_rng_and_back(amd, ctx, ref, store_len):
    b = new_batch(amd, ctx, -1, normals_store_iters=store_len)
    try:
        same(trace(b, SEEDS), ref(SEEDS))
        b.set_rng("philox")
        b.reset()
        same(trace(b, SEEDS), ref(SEEDS, rng="philox"))
        b.reset()
        g = generated(b)
        same(trace(b, SEEDS), ref(SEEDS, rng="philox"))
        assert generated(b) == g  # (tags hold in the other mode too)
        b.set_rng("mt19937")
        b.reset()
        same(trace(b, SEEDS), ref(SEEDS))
    finally:
        b.close()


def test_injected_normals_in_a_ring_slot(amd, ctx, ref, store_len):
    """A GPET_BUF_NORMALS write at an edge's first ring iteration lands in ring slot store_len % 9: the next loop draws that slot
    again, and only that one."""
    L = amd._lib
    want = ref(SEEDS)
    e = int(np.argmax(want[0]))
    assert want[0][e] > store_len
    b = new_batch(amd, ctx, -1, normals_store_iters=store_len)
    try:
        same(trace(b, SEEDS), want)
        b.reset()
        same(trace(b, SEEDS), want)  # (a second trace: what the first one's look-ahead left untagged is settled)
        g1 = generated(b)
        b.reset()
        s = b.scalars(e)
        s.iter = store_len
        b.write_scalars(s, e)
        b.write(L.BUF_NORMALS, np.full((S, b.info(e)["z_cols"]), 3.0), e)
        b.reset()
        same(trace(b, SEEDS), want)
        assert generated(b) - g1 == 1
        b.reset()
        same(trace(b, SEEDS), want)
        assert generated(b) - g1 == 1
    finally:
        b.close()


def test_profile_stage_2_leaves_the_tags_right(amd, ctx, ref, store_len):
    want = ref(SEEDS)
    b = new_batch(amd, ctx, -1, normals_store_iters=store_len)
    try:
        same(trace(b, SEEDS), want)
        b.reset()
        same(trace(b, SEEDS), want)
        g1, d1 = generated(b), drawn(b)
        b.reset()
        b.profile_stage(2, 1)  # iterations 0 .. 8 of every edge by the loop's seed rule: store slots and ring slots
        same(trace(b, SEEDS), want)
        assert generated(b) == g1 and drawn(b) == d1
        # ... and gpet_gp_normals with seeds of the caller's: every edge's slot of iteration 0, drawn again by the next loop
        b.reset()
        b.normals(OTHER)
        same(trace(b, SEEDS), want)
        assert generated(b) - g1 == B
    finally:
        b.close()


def test_wrap_on_the_device(amd, ctx, ref):
    """No store: iteration k + 9 overwrites the slot of iteration k.  Every repeat equals the reference and draws again what the
    wrap overwrote -- at least one stream per iteration past the ninth, the iteration whose slot it took -- and not everything."""
    want = ref(SEEDS, shape="wide")
    iters = want[0]
    print("iterations", iters)
    assert max(iters) > RING, iters  # (the shape was chosen for it)
    wrapped = sum(max(0, k - RING) for k in iters)
    b = new_batch(amd, ctx, 0, shape="wide")
    try:
        g = 0
        for rep in range(4):
            if rep:
                b.reset()
            got = trace_of(b, SEEDS, W_LG)
            same(got, want)
            grown = generated(b) - g
            g = generated(b)
            print("repeat", rep, "generated", grown, "of", sum(iters), "wrapped", wrapped)
            if rep == 0:
                assert grown == sum(iters)
            else:
                assert wrapped <= grown < sum(iters), (grown, wrapped, sum(iters))
        assert b.info()["zstore_iters"] == 0
    finally:
        b.close()
