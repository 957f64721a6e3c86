"""GPU tests of endpoint tracking (GP_Edge_Tracing_Batch(init_follow=), set_frame(init=, init_follow=), trace_sequence(init_follow=);
gpet_batch_init_follow / _set_init / _init_xy; k_init_follow).

The reference in every test is the numpy rule of tests/init_follow_ref.py applied to the gradient image the edge reads, as read back
from the device (GPET_BUF_GRAD), so everything below is np.array_equal.  Frames of 96 x 72; the traced scenes are two layers 30 rows
apart that sink 4 rows per frame, end points included (init_follow_ref.layered_drift)."""
import numpy as np
import pytest

from gaussian_process_edge_trace_amd.sequence import chain_slices, warm_start_obs
from tests import band_ref as Rb
from tests import init_follow_ref as R

pytestmark = pytest.mark.gpu

M, N, T, H, WARM = 96, 72, 5, 40, 4
FOLLOW = dict(window=8, cols=4)
FOLLOW_SEQ = dict(window=14, cols=4)  # (sequences: a chain's first frame lies up to 12 rows below the given points)
KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 10, 'length_scale': 8}, noise_y=1, N_samples=128, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True)


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


@pytest.fixture(scope="module")
def scene(amd, ctx):
    """5 uint8 frames, the kernel, every frame's full-frame gradient image, and the init points that are right on frame 0: the two
    layers' end points, and three points of the upper layer."""
    frames, rows_a = R.layered_drift(M, N, T, 300)
    K = amd.gpet_utils.kernel_builder((11, 5))
    G = [amd.gpet_utils.comp_grad_img(f, K, ctx=ctx) for f in frames]
    a0 = rows_a[0]
    ia = np.array([[0, a0[0]], [N - 1, a0[-1]]], dtype=np.int64)
    ib = ia + np.array([0, 30])
    ic = np.array([[0, a0[0]], [N // 2, a0[N // 2]], [N - 1, a0[-1]]], dtype=np.int64)
    return dict(frames=frames, K=K, G=G, ia=ia, ib=ib, ic=ic, rows_a=rows_a)


def same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def sorted_init(i):
    i = np.asarray(i)
    return i[np.argsort(i[:, 0])].astype(np.int64)


def state(b):
    from gaussian_process_edge_trace_amd import _lib as L
    return ([i.tolist() for i in b._batch.init_xy()], [o.tolist() for o in b._batch.read_obs_all()],
            [b._batch.read(L.BUF_GRAD, e).tobytes() for e in range(b.B)], [bytes(s) for s in b._batch.all_scalars()])


# ---- 1: the rule on crafted gradient images ----------------------------------------------------------------------------------------
def crafted_images():
    """Values in [0, 1] with 0 and 1 present, so the batch's re-normalisation leaves every pixel as it is (the test does not rely on
    it: the reference reads the image back)."""
    G = np.zeros((M, N), dtype=np.float32)
    G[35, 12] = G[45, 12] = 0.5                     # (12, 40): equal score at equal distance
    G[36, 60] = G[43, 60] = 0.5                     # (60, 40): equal score, 43 is nearer
    G[14, 0:3], G[6, 0:2] = 0.25, 0.3               # (0, 10): the column window clipped at x = 0; cols = 1 and 2 disagree
    G[90, N - 3:], G[80, N - 2:] = 0.25, 0.3        # (N - 1, 85): clipped at x = N - 1
    G[0, 5] = 1.0                                   # (5, 3): the row window clipped at row 0
    G[M - 1, 66] = 0.9                              # (66, 93): clipped at row M - 1
    G[48 + 39, 30] = G[48 - 40, 30] = 0.7           # (30, 48): 39 and 40 rows away -- found only by lanes on their second round
    G2 = np.ascontiguousarray(G[::-1])
    G3 = (np.random.default_rng(9).random((M, N)) * (np.random.default_rng(10).random((M, N)) < 0.2)).astype(np.float32)
    G3 = np.rint(G3 * 8).astype(np.float32) / 8   # (few distinct values: exact ties everywhere)
    return G, G2, G3


CRAFTED_INITS = [np.array([[0, 10], [N - 1, 85]]), np.array([[5, 3], [30, 48], [66, 93]]), np.array([[12, 40], [60, 40]]),
                 np.array([[20, 20], [40, 60], [50, 30]])]
# (window, cols) in the order they are applied: every call starts from where the one before it left the points
CALLS = [(0, 2), (5, 0), (5, 2), (5, 1), (40, 1), (96, 64), (4096, 0)]


@pytest.mark.parametrize("layout", ["shared", "map", "per_edge"])
def test_rule_on_crafted_images(amd, ctx, layout):
    L = amd._lib
    G, G2, G3 = crafted_images()
    images = dict(shared=dict(grad_imgs=G), map=dict(grad_imgs=[G, G2], image_of=[0, 1, 1, 0]), per_edge=dict(grad_imgs=[G, G2, G, G3]))[layout]
    kw = dict(images)
    b = amd.GP_Edge_Tracing_Batch(CRAFTED_INITS, kw.pop("grad_imgs"), [1, 2, 3, 4], _ctx=ctx, **kw, **KW)
    imgs = [b._batch.read(L.BUF_GRAD, e) for e in range(4)]
    cur = [sorted_init(i) for i in CRAFTED_INITS]
    assert same(b._batch.init_xy(), cur) and same(b.inits, cur)
    if layout == "shared":
        assert all(np.array_equal(i, G) for i in imgs)
    seen = []
    for w, a in CALLS:
        cur = [R.follow(img, c, w, a) for img, c in zip(imgs, cur)]
        got = b._batch.init_follow(w, a)
        assert same(got, cur), (layout, w, a, got, cur)
        assert same(b._batch.init_xy(), cur), (layout, w, a)
        seen.append([c[:, 1].tolist() for c in cur])
    if layout == "shared":  # the cases the images were crafted for, as literals
        start = [sorted_init(i)[:, 1].tolist() for i in CRAFTED_INITS]
        assert seen[0] == start                                             # w = 0 moves nothing
        # w = 5, cols = 0: (0, 10): 0.3 in row 6 beats 0.25 in row 14;  (N - 1, 85): 80 likewise;  row 0 and row M - 1 are reached
        # through the clipped windows;  (30, 48): nothing within 5 rows;  ties: 35 (the smaller row), 43 (the nearer row);  edge 3: all zero
        assert seen[1] == [[6, 80], [0, 48, M - 1], [35, 43], [20, 60, 30]]
        # w = 5, cols = 2 from there: at x = 0 the window is columns 0 .. 2: row 6 holds 0.6, row 14 is 8 rows away -> stays 6
        assert seen[2] == seen[1]
        # w = 40, cols = 1: (30, 48) finds rows 8 and 87 with equal scores 40 and 39 rows away -> 87
        assert seen[4][1][1] == 87 and seen[3][1][1] == 48
    b._batch.close()


def test_more_than_64_candidates_and_cols_disagreeing(amd, ctx):
    """From fresh points each: (0, 10) with window 8 sees rows 6 and 14 -- cols = 1: 0.6 against 0.5, cols = 2: 0.6 against 0.75."""
    G, _, _ = crafted_images()
    for (w, a), want in (((8, 1), 6), ((8, 2), 14), ((40, 2), 14)):
        b = amd.GP_Edge_Tracing_Batch(CRAFTED_INITS[:1], G, [1], _ctx=ctx, **KW)
        got = b._batch.init_follow(w, a)
        assert same(got, [R.follow(b._batch.read(amd._lib.BUF_GRAD, 0), CRAFTED_INITS[0], w, a)]) and got[0][0, 1] == want, (w, a, got)
        b._batch.close()


# ---- 2: nothing stale ----------------------------------------------------------------------------------------------------------------
def test_followed_set_and_fresh_batches_trace_the_same(amd, ctx, scene):
    """Rough points (right on frame 0) on frame 2, where the layers lie 8 rows lower: a batch built with init_follow, a twin fed the
    rule's points through set_init, and a fresh batch built with those points."""
    L = amd._lib
    rough = [scene["ia"], scene["ib"], scene["ic"]]
    seeds = [3, 4, 5]
    opts = dict(return_std=True, history="obs", _ctx=ctx, **KW)
    a = amd.GP_Edge_Tracing_Batch(rough, scene["G"][2], seeds, init_follow=FOLLOW, **opts)
    ruled = [R.follow(a._batch.read(L.BUF_GRAD, e), rough[e], 8, 4) for e in range(3)]
    assert same(a.inits, ruled) and same(a._batch.init_xy(), ruled) and same([p["init"] for p in a._ps], [r.astype(int) for r in ruled])
    for r, g in zip(ruled, rough):
        assert np.array_equal(r[:, 0], g[:, 0]) and np.all(np.abs(r[:, 1] - g[:, 1] - 8) <= 2), (r, g)
    twin = amd.GP_Edge_Tracing_Batch(rough, scene["G"][2], seeds, **opts)
    twin._batch.set_init(ruled)
    assert same(twin._batch.init_xy(), ruled)
    fresh = amd.GP_Edge_Tracing_Batch(ruled, scene["G"][2], seeds, **opts)
    out = [b() for b in (a, twin, fresh)]
    assert same(out[0], out[2]) and same(out[1], out[2])
    assert list(a.timings["iters"]) == list(twin.timings["iters"]) == list(fresh.timings["iters"]) and min(fresh.timings["iters"]) >= 1
    hist = [b.history() for b in (a, twin, fresh)]
    for e in range(3):
        assert same(hist[0][e]["obs"], hist[2][e]["obs"]) and same(hist[1][e]["obs"], hist[2][e]["obs"]), e
    # and not what the rough points give
    stale = amd.GP_Edge_Tracing_Batch(rough, scene["G"][2], seeds, **opts)
    assert not same(stale(), out[2])
    # reset() keeps the moved points
    a.reset()
    assert same(a._batch.init_xy(), ruled) and same(a(), out[2])
    for b in (a, twin, fresh, stale):
        b._batch.close()


# ---- 3: state and refusals -------------------------------------------------------------------------------------------------------------
def test_state_rule_and_refusals(amd, ctx, scene):
    L = amd._lib
    inits, seeds = [scene["ia"], scene["ic"]], [3, 4]
    b = amd.GP_Edge_Tracing_Batch(inits, scene["G"][0], seeds, _ctx=ctx, **KW)
    twin = amd.GP_Edge_Tracing_Batch(inits, scene["G"][0], seeds, _ctx=ctx, **KW)
    # refused arguments, before the loop: nothing moves
    for w, a, words in ((-1, 4, "window must be at least 0"), (4097, 4, "window exceeds 4096"), (8, -1, "cols must be at least 0"),
                        (8, 65, "cols exceeds 64")):
        with pytest.raises(L.GpetError) as ei:
            b._batch.init_follow(w, a)
        assert ei.value.code == L.ERR_BAD_ARG and words in str(ei.value)
    bad_x = [inits[0] + np.array([[1, 0], [0, 0]]), inits[1]]
    with pytest.raises(L.GpetError) as ei:
        b._batch.set_init(bad_x)
    assert ei.value.code == L.ERR_BAD_ARG and "the x of an init point cannot change" in str(ei.value)
    with pytest.raises(L.GpetError) as ei:
        b._batch.set_init([inits[0], inits[1][:2]])
    assert ei.value.code == L.ERR_BAD_ARG and "init points" in str(ei.value)
    with pytest.raises(L.GpetError) as ei:
        b._batch.set_init([inits[0]])
    assert ei.value.code == L.ERR_BAD_ARG
    for y in (M, -1):
        pts = [inits[0].copy(), inits[1]]
        pts[0][0, 1] = y
        with pytest.raises(L.GpetError) as ei:
            b._batch.set_init(pts)
        assert ei.value.code == L.ERR_BAD_ARG and "outside the frame" in str(ei.value)
    assert state(b) == state(twin)
    # after the loop has started: ERR_STATE, and the trace continues unchanged
    b._batch.iterate(b.seeds, 2)
    before = state(b)
    with pytest.raises(L.GpetError) as ei:
        b._batch.init_follow(8, 4)
    assert ei.value.code == L.ERR_STATE
    with pytest.raises(L.GpetError) as ei:
        b._batch.set_init([i + np.array([0, 1]) for i in inits])
    assert ei.value.code == L.ERR_STATE
    assert state(b) == before
    iters = b.run_loop()
    got, want = b.finish(iters), twin()
    assert same(got, want) and list(iters) == list(twin.timings["iters"]) and min(iters) >= 1
    # after the trace: still refused, until the images are swapped or the batch is reset
    with pytest.raises(L.GpetError) as ei:
        b._batch.init_follow(8, 4)
    assert ei.value.code == L.ERR_STATE
    b.reset()
    assert same(b._batch.init_follow(0, 0), [sorted_init(i) for i in inits])
    b._batch.close()
    twin._batch.close()


def test_a_refused_init_table_leaves_a_banded_batch_as_it_was(amd, ctx, scene):
    L = amd._lib
    inits, seeds, r0s = [scene["ia"], scene["ib"]], [3, 4], [5, 33]
    make = lambda: amd.GP_Edge_Tracing_Batch(inits, None, seeds, raw_imgs=scene["frames"][0], grad_kernel=scene["K"], band_rows=H,
                                             band_r0=r0s, _ctx=ctx, **KW)
    band, twin = make(), make()
    first = band()
    assert same(first, twin())
    full = lambda b: state(b) + ([int(v) for v in b.band_r0], [int(v) for v in b._batch.band_r0()])
    before = full(band)
    nxt = scene["frames"][1]
    with pytest.raises(ValueError, match="need the bands too"):                      # a table without its bands
        band.set_frame(raw_imgs=nxt, warm_every=WARM, init=[i + np.array([0, 4]) for i in inits])
    with pytest.raises(ValueError, match="band of edge 1: an init point lies outside its band"):
        band.set_frame(raw_imgs=nxt, warm_every=WARM, band=[5, 33], init=[inits[0], inits[1] + np.array([0, 30])])
    with pytest.raises(ValueError, match="init of edge 0 has x"):
        band.set_frame(raw_imgs=nxt, warm_every=WARM, band=[5, 33], init=[inits[0] + np.array([1, 0]), inits[1]])
    with pytest.raises(ValueError, match="init='follow' needs init_follow"):
        band.set_frame(raw_imgs=nxt, warm_every=WARM, init="follow")
    with pytest.raises(L.GpetError) as ei:                                             # the library's own refusal: outside the band
        band._batch.set_init([inits[0] + np.array([0, 40]), inits[1]])
    assert ei.value.code in (L.ERR_BAD_ARG, L.ERR_STATE)
    band.reset()
    twin.reset()
    with pytest.raises(L.GpetError) as ei:
        band._batch.set_init([inits[0] + np.array([0, 40]), inits[1]])
    assert ei.value.code == L.ERR_BAD_ARG and "outside its band" in str(ei.value)
    assert full(band) == full(twin) and full(band)[0] == before[0] and full(band)[2] == before[2] and full(band)[4:] == before[4:]
    assert same(band(), first)
    # an accepted table: the bands and the points move together
    table, pts = [9, 37], [inits[0] + np.array([0, 4]), inits[1] + np.array([0, 4])]
    band.set_frame(raw_imgs=nxt, warm_every=WARM, band=table, init=pts)
    assert [int(v) for v in band.band_r0] == table and same(band.inits, pts) and same(band._batch.init_xy(), pts)
    crop = Rb.crop_batch(amd, ctx, pts, [scene["G"][1]] * 2, table, H, seeds,
                         obs=[o + np.array([0, r]) for o, r in zip(band._batch.read_obs_all(), table)], **KW)
    assert same(band(), [Rb.up(w, r, False) for w, r in zip(crop(), table)])
    for b in (band, twin, crop):
        b._batch.close()


# ---- 4: the frame change ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ensemble", [False, True])
def test_set_frame_follow_equals_the_host_driven_step(amd, ctx, scene, ensemble):
    L = amd._lib
    if ensemble:
        inits, seeds, group_of = [scene["ia"], scene["ia"], scene["ib"], scene["ib"]], [3, 4, 3, 4], np.array([0, 0, 1, 1], dtype=np.int32)
    else:
        inits, seeds, group_of = [scene["ia"], scene["ib"], scene["ic"]], [3, 4, 5], None
    dev = amd.GP_Edge_Tracing_Batch(inits, None, seeds, raw_imgs=scene["frames"][0], grad_kernel=scene["K"], _ctx=ctx, **KW)
    out0 = dev()
    warm = dict(warm_from="medoid", group_of=group_of, tol=2) if ensemble else {}
    dev.set_frame(raw_imgs=scene["frames"][1], warm_every=WARM, init="follow", init_follow=FOLLOW, **warm)
    # the host-driven step: comp_grad_imgs, the rule, a fresh batch with the warm start of the previous trace
    G1 = amd.gpet_utils.comp_grad_imgs([scene["frames"][1]], scene["K"], ctx=ctx)[0]
    for e in range(dev.B):
        assert np.array_equal(dev._batch.read(L.BUF_GRAD, e), G1)
    ruled = [R.follow(G1, i, 8, 4) for i in inits]
    assert same(dev.inits, ruled) and same(dev._batch.init_xy(), ruled)
    assert all(np.all(np.abs(r[:, 1] - i[:, 1] - 4) <= 2) for r, i in zip(ruled, inits)), ruled
    src = [int(dev.last_ensemble[g]["medoid"]) for g in group_of] if ensemble else list(range(dev.B))
    obs = [warm_start_obs(out0[src[e]], p["x_st"], p["x_en"], WARM, p["algo_thresh"], p["M"]) for e, p in enumerate(dev._ps)]
    assert same(dev._batch.read_obs_all(), obs) and min(len(o) for o in obs) >= 1
    fresh = amd.GP_Edge_Tracing_Batch(ruled, G1, seeds, obs=obs, _ctx=ctx, **KW)
    assert same(dev(), fresh()) and list(dev.timings["iters"]) == list(fresh.timings["iters"]) and min(fresh.timings["iters"]) >= 1
    # the next change follows from the moved points; 'keep' leaves them
    dev.set_frame(raw_imgs=scene["frames"][2], warm_every=WARM, init="keep", **warm)
    assert same(dev.inits, ruled) and same(dev._batch.init_xy(), ruled)
    dev.set_frame(raw_imgs=scene["frames"][2], init_follow=FOLLOW)
    G2 = amd.gpet_utils.comp_grad_imgs([scene["frames"][2]], scene["K"], ctx=ctx)[0]
    assert same(dev.inits, [R.follow(G2, r, 8, 4) for r in ruled])
    dev._batch.close()
    fresh._batch.close()


# ---- 5: bands ------------------------------------------------------------------------------------------------------------------------
def test_a_banded_batch_follows_inside_its_band_as_the_crop_does(amd, ctx, scene):
    L = amd._lib
    rough, seeds, r0s = [scene["ia"], scene["ib"]], [3, 4], [5, 33]
    opts = dict(return_std=True, history="obs", **KW)
    band = amd.GP_Edge_Tracing_Batch(rough, scene["G"][2], seeds, band_rows=H, band_r0=r0s, init_follow=FOLLOW, _ctx=ctx, **opts)
    crop = Rb.crop_batch(amd, ctx, rough, [scene["G"][2]] * 2, r0s, H, seeds, init_follow=FOLLOW, **opts)
    for e, r0 in enumerate(r0s):
        down = np.array([0, r0])
        slot = band._batch.read(L.BUF_GRAD, e)
        assert slot.shape == (H, N) and np.array_equal(slot, crop._batch.read(L.BUF_GRAD, e))
        want = R.follow(slot, rough[e] - down, 8, 4) + down          # the rule on the slot, in band rows
        assert same(band.inits[e], want) and same(crop.inits[e], want - down) and same(band._batch.init_xy()[e], want)
        assert np.all(np.abs(want[:, 1] - rough[e][:, 1] - 8) <= 2)
        assert band._init_span[e] == (int(want[:, 1].min()), int(want[:, 1].max()))
    got, want = band(), crop()
    assert list(band.timings["iters"]) == list(crop.timings["iters"]) and min(crop.timings["iters"]) >= 1
    for e, r0 in enumerate(r0s):
        assert same(got[e], Rb.up(want[e], r0, True)), e
        assert same(band.history()[e]["obs"], [o + np.array([0, r0]) for o in crop.history()[e]["obs"]])
    # the search is confined to the band: a band whose last row is the rough point's cannot look below it
    tight = amd.GP_Edge_Tracing_Batch(rough[1:], scene["G"][2], seeds[1:], band_rows=H, band_r0=[int(rough[1][0, 1]) - H + 1],
                                      init_follow=FOLLOW, _ctx=ctx, **KW)
    assert int(tight.inits[0][:, 1].max()) <= int(rough[1][0, 1])
    for b in (band, crop, tight):
        b._batch.close()


def test_bands_are_placed_against_the_moved_init_rows(amd, ctx, scene):
    L = amd._lib
    rough, seeds, r0s = [scene["ia"], scene["ib"]], [3, 4], [5, 33]
    band = amd.GP_Edge_Tracing_Batch(rough, scene["G"][2], seeds, band_rows=H, band_r0=r0s, init_follow=FOLLOW, _ctx=ctx, **KW)
    moved = [i.copy() for i in band.inits]
    assert all(int(m[:, 1].min()) > int(g[:, 1].max()) for m, g in zip(moved, rough))
    band()
    # fits injected far below the points: the band goes down until the init clamp holds it -- at the MOVED points
    Lg = band._batch.info(0)["Lg"]
    full_rows = [80, 90]
    for e in range(2):
        m = np.full(Lg, float(full_rows[e] - r0s[e]))
        band._batch.write(L.BUF_FIN_OUT, np.stack([m, np.ones_like(m)]), e)
    band.set_frame(scene["G"][3], band="follow", init="keep")
    want = [Rb.place(M, H, [full_rows[e]], moved[e][:, 1], r0s[e]) for e in range(2)]
    not_want = [Rb.place(M, H, [full_rows[e]], rough[e][:, 1], r0s[e]) for e in range(2)]
    assert want[0] == int(moved[0][:, 1].min()) and all(w != n for w, n in zip(want, not_want)), (want, not_want)
    assert [int(v) for v in band.band_r0] == want, (band.band_r0, want, not_want)
    assert same(band.inits, moved) and same(band._batch.init_xy(), moved)     # full-frame rows, whatever the bands do
    # an explicit table that holds the moved points and not the rough ones is accepted, by set_frame and by the library
    table = [int(rough[0][:, 1].max()) + 2, int(rough[1][:, 1].max()) + 2]
    band.set_frame(scene["G"][3], band=table, init="keep")
    assert [int(v) for v in band.band_r0] == table and same(band._batch.init_xy(), moved)
    band._batch.band_set([t + 1 for t in table])
    # and following in the new bands starts from the moved points, in band rows
    band.set_frame(scene["G"][4], band=table, init="follow")
    for e in range(2):
        down = np.array([0, table[e]])
        assert same(band.inits[e], R.follow(band._batch.read(L.BUF_GRAD, e), moved[e] - down, 8, 4) + down)
    band._batch.close()


# ---- 6: sequences ----------------------------------------------------------------------------------------------------------------------
def host_sequence(amd, ctx, scene, inits, n_chains, seeds_of_frame, band_rows=None, ensemble_seeds=None):
    w, a = FOLLOW_SEQ["window"], FOLLOW_SEQ["cols"]
    """The host loop, frame by frame and edge by edge: the gradient image of the frame (its band, placed against the points of the
    frame before), the rule on the image a probe batch reads back, a FRESH batch built with the rule's points and the warm start of
    the previous trace.  Returns (results, inits) per frame, each a list over the edges."""
    L = amd._lib
    results, inits_out = [None] * T, [None] * T
    for lo_f, hi_f in chain_slices(T, n_chains):
        cur = [np.array(i, dtype=np.int64) for i in inits]
        prev, r0_prev = [None] * len(inits), [None] * len(inits)
        for f in range(lo_f, hi_f):
            res_f = []
            for k in range(len(inits)):
                sd = list(ensemble_seeds) if ensemble_seeds is not None else [seeds_of_frame[f]]
                G, r0 = scene["G"][f], 0
                if band_rows is not None:
                    rows = cur[k][:, 1]
                    r0 = Rb.place(M, band_rows, rows if prev[k] is None else prev[k][:, 0], rows, r0_prev[k])
                    G = np.ascontiguousarray(G[r0:r0 + band_rows])
                down = np.array([0, r0])
                probe = amd.GP_Edge_Tracing_Batch([cur[k] - down], G, sd[:1], _ctx=ctx, **KW)
                p = probe._ps[0]
                ruled = R.follow(probe._batch.read(L.BUF_GRAD, 0), cur[k] - down, w, a)
                probe._batch.close()
                o = (np.zeros((0, 2), dtype=np.int64) if prev[k] is None else
                     warm_start_obs(prev[k] - np.array([r0, 0]), p["x_st"], p["x_en"], WARM, p["algo_thresh"], M=G.shape[0]))
                b = amd.GP_Edge_Tracing_Batch([ruled] * len(sd), G, sd, obs=[o] * len(sd), _ctx=ctx, **KW)
                out = [Rb.up(r, r0, False) for r in b()]
                if ensemble_seeds is None:
                    res_f.append(out[0])
                    prev[k] = out[0]
                else:
                    d = b.ensemble(None, 2)[0]
                    res_f.append(dict(trace=d["trace"] + np.array([r0, 0]), medoid=int(d["medoid"]), result=out[d["medoid"]]))
                    prev[k] = out[d["medoid"]]
                b._batch.close()
                cur[k], r0_prev[k] = ruled + down, r0
            results[f], inits_out[f] = res_f, [c.copy() for c in cur]
    return results, inits_out


def test_trace_sequence_with_init_follow_equals_the_host_loop(amd, ctx, scene):
    """5 frames in 2 chains of 3 and 2: the batch of 4 edges is rebuilt with 2 at the last step, from the points carried on the host."""
    inits, seeds = [scene["ia"], scene["ib"]], [11, 12, 13, 14, 15]
    st = amd.SequenceTracer(scene["frames"], inits, n_chains=2, warm_every=WARM, seeds=seeds, grad_kernel=scene["K"], init_follow=FOLLOW_SEQ,
                            _ctx=ctx, **KW)
    got = st()
    want, want_inits = host_sequence(amd, ctx, scene, inits, 2, seeds)
    assert st._tracer.B == 2
    for t in range(T):
        assert same(st.inits[t], want_inits[t]), (t, st.inits[t], want_inits[t])
        assert same(got[t], want[t]), t
    # the end points have followed the layers down, 16 rows by the last frame; the second chain's first frame, 12 rows below the given
    # points, is within the window of 14
    for t in range(T):
        for k in range(2):
            assert np.all(np.abs(st.inits[t][k][:, 1] - (scene["rows_a"][t][[0, -1]] + 30 * k)) <= 2), (t, k, st.inits[t][k])
    st._tracer._batch.close()


def test_sequence_with_bands_and_seed_ensembles_follows_too(amd, ctx, scene):
    inits, ens = [scene["ia"], scene["ib"]], [3, 4]
    st = amd.SequenceTracer(scene["frames"], inits, n_chains=2, warm_every=WARM, ensemble_seeds=ens, warm_from="medoid",
                            grad_kernel=scene["K"], band_rows=H, init_follow=FOLLOW_SEQ, _ctx=ctx, **KW)
    got = st()
    want, want_inits = host_sequence(amd, ctx, scene, inits, 2, None, band_rows=H, ensemble_seeds=ens)
    for t in range(T):
        assert same(st.inits[t], want_inits[t]), (t, st.inits[t], want_inits[t])
        for k in range(2):
            assert same(got[t][k]["trace"], want[t][k]["trace"]), (t, k)
            assert same(got[t][k]["result"], want[t][k]["result"]), (t, k)
            assert got[t][k]["medoid"] % 2 == want[t][k]["medoid"]
    st._tracer._batch.close()
