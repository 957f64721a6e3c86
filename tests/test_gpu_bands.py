"""GPU tests of tracking bands (GP_Edge_Tracing_Batch(band_rows=, band_r0=), set_frame(band=), trace_sequence(band_rows=);
gpet_batch_create_banded, gpet_batch_band_place / _set / _r0; k_band_place, k_band_apply, k_band_minmax, k_band_normalise and the
banded k_warm_start_src).

Tracing in a band is DEFINED as tracing the cropped full-frame gradient image with the objects the package has without bands
(tests/band_ref.py), so everything below is np.array_equal.  Frames of 64 rows and 64, 65 or 70 columns (a band's first pixel is then
16-byte, 4-byte and 8-byte aligned for an odd r0), bands of 32 rows, two layers per frame 22 rows apart."""
import numpy as np
import pytest

from gaussian_process_edge_trace_amd.sequence import warm_start_obs
from tests import band_ref as R
from tests.test_gpu_denoise import DeviceFrames

pytestmark = pytest.mark.gpu

M, H, WARM = 64, 32, 4
KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 10, 'length_scale': 8}, noise_y=1, N_samples=128, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True)
# per width: (r0 of the upper layer's edge, r0 of the lower layer's): 0 and M - H; two odd middle values; an odd one and M - H
R0 = {64: (0, 32), 65: (7, 13), 70: (7, 32)}


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


@pytest.fixture(scope="module")
def kernels(amd):
    return [amd.gpet_utils.kernel_builder((11, 5)), amd.gpet_utils.kernel_builder((7, 3))]


@pytest.fixture(scope="module")
def scenes(amd, ctx, kernels):
    """Per width: 5 uint8 frames, the two inits, and the full-frame gradient image of every frame (the first kernel)."""
    out = {}
    for N in (64, 65, 70):
        frames, init_a, init_b, rows_a = R.layered_frames(M, N, 5, 100 + N, "uint8", base=14, gap=22, step=4.5)
        G = [amd.gpet_utils.comp_grad_img(f, kernels[0], ctx=ctx) for f in frames]
        out[N] = dict(frames=frames, inits=[init_a, init_b], G=G, rows=[rows_a, [r + 22 for r in rows_a]])
    return out


def same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def assert_band_equals_crop(amd, band, crop, r0s, what, groups=None):
    """Slot images, then (run both) traces, intervals, iteration counts, final observation sets, history rows, ensemble row fields and
    result records: the banded batch in full-frame rows against the crop batch raised by r0."""
    L = amd._lib
    assert [int(v) for v in band.band_r0] == [int(v) for v in r0s], (what, band.band_r0, r0s)
    for e in range(band.B):
        assert np.array_equal(band._batch.read(L.BUF_GRAD, e), crop._batch.read(L.BUF_GRAD, e)), (what, "grad", e)
        assert np.array_equal(band._batch.read(L.BUF_GRAD_KDE, e), crop._batch.read(L.BUF_GRAD_KDE, e)), (what, "grad kde", e)
    got, want = band(), crop()
    assert band.timings["iters"] == crop.timings["iters"] and min(crop.timings["iters"]) >= 1, (what, band.timings, crop.timings)
    for e, (g, w) in enumerate(zip(got, want)):
        assert same(g, R.up(w, r0s[e], True)), (what, "result", e)
    for e, (g, w) in enumerate(zip(band._batch.read_obs_all(), crop._batch.read_obs_all())):
        assert np.array_equal(g, w), (what, "final observations (band rows on the device)", e)
    hb, hc = band.history(), crop.history()
    for e in range(band.B):
        r0 = int(r0s[e])
        assert hb[e]["n_iter"] == hc[e]["n_iter"] >= 1
        assert same(hb[e]["obs"], [o + np.array([0, r0]) for o in hc[e]["obs"]]), (what, "history obs", e)
        assert same(hb[e]["optimal_curves"], [c + np.array([0.0, r0]) for c in hc[e]["optimal_curves"]]), (what, "history curves", e)
        assert same(hb[e]["mean"], hc[e]["mean"] + r0) and same(hb[e]["std"], hc[e]["std"]), (what, "history mean / std", e)
        assert same(hb[e]["optimal_cost"], hc[e]["optimal_cost"]) and same(hb[e]["score_thresh"], hc[e]["score_thresh"])
    groups = np.arange(band.B, dtype=np.int32) if groups is None else groups
    eb, ec = band.ensemble(groups, 2), crop.ensemble(groups, 2)
    for g, (db, dc) in enumerate(zip(eb, ec)):
        r0 = int(r0s[int(np.flatnonzero(groups == g)[0])])
        assert same(db["trace"], dc["trace"] + np.array([r0, 0])), (what, "ensemble trace", g)
        for key in ("median", "q_lo", "q_hi", "min", "max"):
            assert same(db[key], dc[key] + r0), (what, key, g)
        for key in ("agree", "members", "off", "cost", "medoid", "best_cost"):
            assert same(db[key], dc[key]), (what, key, g)
    rb, sb = band.results()
    rc, sc = crop.results()
    assert same(rb, [R.up(w, r0s[e], True) for e, w in enumerate(rc)]), (what, "results()")
    assert all(same(sb[k], sc[k]) for k in sb)
    assert same(band.final_costs(), crop.final_costs())


# ---- 1, 2: static bands -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["uint8", "float64", "device", "grad"])
@pytest.mark.parametrize("N", [64, 65, 70])
def test_static_bands_equal_the_cropped_oracle(amd, ctx, kernels, scenes, N, source):
    sc = scenes[N]
    r0s, seeds = R0[N], [3, 4]
    opts = dict(return_std=True, history="full", **KW)
    frame, dev = sc["frames"][1], None
    if source == "grad":
        band = amd.GP_Edge_Tracing_Batch(sc["inits"], sc["G"][1], seeds, band_rows=H, band_r0=r0s, _ctx=ctx, **opts)
        G = sc["G"][1]
    else:
        if source == "float64":
            frame = frame.astype(np.float64) / 255.0
        G = amd.gpet_utils.comp_grad_img(frame, kernels[0], ctx=ctx)
        if source == "device":
            dev = DeviceFrames(ctx, [frame])
            band = amd.GP_Edge_Tracing_Batch(sc["inits"], None, seeds, raw_device_ptrs=dev.ptrs, raw_dtype=frame.dtype, grad_shape=(M, N),
                                             grad_kernel=kernels[0], band_rows=H, band_r0=r0s, _ctx=ctx, **opts)
        else:
            band = amd.GP_Edge_Tracing_Batch(sc["inits"], None, seeds, raw_imgs=frame, grad_kernel=kernels[0], band_rows=H, band_r0=r0s,
                                             _ctx=ctx, **opts)
    assert band._batch.M == H and band._batch.frame_M == M and band._batch.n_img == 1
    crop = R.crop_batch(amd, ctx, sc["inits"], [G, G], r0s, H, seeds, **opts)
    assert_band_equals_crop(amd, band, crop, r0s, (N, source))
    band._batch.close()
    crop._batch.close()
    if dev is not None:
        dev.free()


def test_two_edges_on_one_frame_with_different_bands_and_kernels(amd, ctx, kernels, scenes):
    sc = scenes[65]
    r0s, seeds = (3, 21), [5, 6]
    opts = dict(return_std=True, history="full", **KW)
    band = amd.GP_Edge_Tracing_Batch(sc["inits"], None, seeds, raw_imgs=sc["frames"][0], grad_kernel=kernels, kernel_of=[0, 1],
                                     band_rows=H, band_r0=r0s, _ctx=ctx, **opts)
    Gs = [amd.gpet_utils.comp_grad_img(sc["frames"][0], k, ctx=ctx) for k in kernels]
    assert band._batch.n_img == 2 and not np.array_equal(Gs[0], Gs[1])
    crop = R.crop_batch(amd, ctx, sc["inits"], Gs, r0s, H, seeds, **opts)
    assert_band_equals_crop(amd, band, crop, r0s, "two kernels")
    band._batch.close()
    crop._batch.close()


def test_bands_of_denoised_frames_and_placement_from_the_inits(amd, ctx, kernels, scenes):
    """denoise=('median', ...): the full frame is denoised and convolved, then cropped.  band_r0=None: every band is placed from its
    edge's init rows."""
    sc = scenes[70]
    spec = ("median", dict(size=3))
    seeds = [7, 8]
    opts = dict(return_std=True, history="full", **KW)
    band = amd.GP_Edge_Tracing_Batch(sc["inits"], None, seeds, raw_imgs=sc["frames"][2], grad_kernel=kernels[0], denoise=spec,
                                     band_rows=H, _ctx=ctx, **opts)
    r0s = [R.place(M, H, i[:, 1], i[:, 1]) for i in sc["inits"]]
    assert r0s == [0, 20]  # (14 + 14) // 2 - 16 = -2 -> 0;  (36 + 36) // 2 - 16 = 20
    G = amd.gpet_utils.comp_grad_imgs([sc["frames"][2]], kernels[0], ctx=ctx, denoise=spec)[0]
    assert not np.array_equal(G, sc["G"][2])
    crop = R.crop_batch(amd, ctx, sc["inits"], [G, G], r0s, H, seeds, **opts)
    assert_band_equals_crop(amd, band, crop, r0s, "median")
    band._batch.close()
    crop._batch.close()


# ---- 3: set_frame -----------------------------------------------------------------------------------------------------------------
def rule_obs(b, traces, src_of, r0_new):
    """sequence.warm_start_obs on the source's trace lowered into the destination's new band, M = H; -1: none."""
    out = []
    for e, p in enumerate(b._ps):
        if src_of[e] < 0:
            out.append(np.zeros((0, 2), dtype=np.int64))
        else:
            out.append(warm_start_obs(traces[src_of[e]] - np.array([int(r0_new[e]), 0]), p["x_st"], p["x_en"], WARM, p["algo_thresh"], M=H))
    return out


@pytest.mark.parametrize("N", [65, 70])
def test_set_frame_follows_the_edges_and_warm_starts_across_bands(amd, ctx, kernels, scenes, N):
    sc = scenes[N]
    inits = [sc["inits"][0], sc["inits"][1], sc["inits"][0]]
    seeds = [3, 4, 5]
    # (the first bands are NOT where placement would put them, so the step below has to move every one of them)
    band = amd.GP_Edge_Tracing_Batch(inits, None, seeds, raw_imgs=sc["frames"][0], grad_kernel=kernels[0], band_rows=H, band_r0=[3, 17, 5],
                                     _ctx=ctx, **KW)
    traces = band()
    r0_old = [int(v) for v in band.band_r0]
    assert r0_old == [3, 17, 5]
    spans = [i[:, 1] for i in inits]

    def check(frame, r0_want, src_of, what):
        assert [int(v) for v in band.band_r0] == r0_want, (what, band.band_r0, r0_want)
        obs = rule_obs(band, traces, src_of, r0_want)
        got = band._batch.read_obs_all()
        assert all(np.array_equal(g, o) for g, o in zip(got, obs)) and max(len(o) for o in obs) >= 1, (what, got, obs)
        crop = R.crop_batch(amd, ctx, inits, [sc["G"][frame]] * 3, r0_want, H, seeds,
                            obs=[o + np.array([0, r]) for o, r in zip(obs, r0_want)], **KW)
        for e in range(3):
            assert np.array_equal(band._batch.read(amd._lib.BUF_GRAD, e), crop._batch.read(amd._lib.BUF_GRAD, e)), (what, "grad", e)
        new, want = band(), crop()
        assert band.timings["iters"] == crop.timings["iters"], what
        assert same(new, [R.up(w, r, False) for w, r in zip(want, r0_want)]), what
        crop._batch.close()
        return new

    # 'follow' is the default with warm_every: two frames on, the middle of the edges has moved 10 rows
    band.set_frame(raw_imgs=sc["frames"][2], warm_every=WARM)
    placed = [R.place(M, H, t[:, 0], s, r) for t, s, r in zip(traces, spans, r0_old)]
    assert all(p != r for p, r in zip(placed, r0_old)), (placed, r0_old)
    traces = check(2, placed, [0, 1, 2], "follow")
    # an explicit table
    table = [5, 9, 14]
    band.set_frame(raw_imgs=sc["frames"][3], warm_every=WARM, band=table)
    traces = check(3, table, [0, 1, 2], "explicit")
    # bands set without a warm start, then the warm start from a table: edge 0 from edge 2's trace, edge 1 none, edge 2 from edge 0's
    table = [0, 20, 11]
    band.set_frame(raw_imgs=sc["frames"][4], band=table)
    cnt = band.warm_start_from([2, -1, 0], WARM)
    assert cnt[1] == 0 and cnt[0] >= 1
    check(4, table, [2, -1, 0], "warm_start_from")
    band._batch.close()


def test_placement_ignores_rows_that_are_not_in_the_frame(amd, ctx, kernels, scenes):
    """Fits injected into fin_out: all NaN (the band stays), rows outside the frame and NaN among usable ones (placed from the rest)."""
    sc, L = scenes[64], amd._lib
    inits = [sc["inits"][0], sc["inits"][0], sc["inits"][1]]
    band = amd.GP_Edge_Tracing_Batch(inits, None, [3, 4, 5], raw_imgs=sc["frames"][0], grad_kernel=kernels[0], band_rows=H,
                                     band_r0=[2, 1, 20], _ctx=ctx, **KW)
    band()
    Lg = band._batch.info(0)["Lg"]
    means = [np.full(Lg, np.nan), np.linspace(10.0, 30.0, Lg), np.linspace(-30.0, 50.0, Lg)]
    means[1][[3, 9]] = [np.nan, 1e12]
    for e, m in enumerate(means):
        band._batch.write(L.BUF_FIN_OUT, np.stack([m, np.ones_like(m)]), e)
    band.set_frame(raw_imgs=sc["frames"][1], band="follow")
    old = [2, 1, 20]
    want = [R.place(M, H, np.rint(m) + r, i[:, 1], r) for m, r, i in zip(means, old, inits)]
    assert want[0] == 2 and [int(v) for v in band.band_r0] == want, (band.band_r0, want)
    band._batch.close()


# ---- 4: sequences -------------------------------------------------------------------------------------------------------------------
def test_trace_sequence_in_bands_equals_the_host_chained_oracle(amd, ctx, kernels, scenes):
    sc = scenes[65]
    T, seeds = 5, [11, 12, 13, 14, 15]
    got = amd.trace_sequence(sc["frames"], sc["inits"], n_chains=2, warm_every=WARM, seeds=seeds, grad_kernel=kernels[0], band_rows=H,
                             _ctx=ctx, **KW)
    want, _, r0 = R.chained(amd, ctx, [[G, G] for G in sc["G"]], sc["inits"], H, M, 2, WARM, seeds, **KW)
    for t in range(T):
        assert same(got[t], want[t]), (t, r0[t])
    # the middle of both edges has moved by 17 rows, more than H / 2: the band placed from the inits (the first frame of a chain) no
    # longer holds the edge of the last frame, and the second chain's bands have followed
    for k in range(2):
        assert int(sc["rows"][k][4].max()) - int(sc["rows"][k][0].max()) > H // 2 and int(sc["rows"][k][4].max()) > r0[3][k] + H - 1
        assert r0[4][k] > r0[3][k] == r0[0][k]


def test_sequence_of_ensembles_in_bands(amd, ctx, kernels, scenes):
    sc = scenes[70]
    T, ens = 5, [3, 4, 5]
    st = amd.SequenceTracer(sc["frames"], sc["inits"], n_chains=2, warm_every=WARM, ensemble_seeds=ens, warm_from="medoid",
                            grad_kernel=kernels[0], band_rows=H, _ctx=ctx, **KW)
    got = st()
    want, want_it, r0 = R.chained(amd, ctx, [[G, G] for G in sc["G"]], sc["inits"], H, M, 2, WARM, None, ensemble_seeds=ens,
                                  warm_from="medoid", **KW)
    for t in range(T):
        for k in range(2):
            for key in ("trace", "median", "q_lo", "q_hi", "min", "max", "agree", "off", "cost", "result"):
                assert same(got[t][k][key], want[t][k][key]), (t, k, key)
            # (edge indices: the oracle's batch holds this group alone, the step's batch all groups, member-minor)
            for key in ("medoid", "best_cost"):
                assert got[t][k][key] % 3 == want[t][k][key], (t, k, key)
            assert [int(e) % 3 for e in got[t][k]["members"]] == [int(e) for e in want[t][k]["members"]] == [0, 1, 2]
            assert got[t][k]["medoid_seed"] == ens[want[t][k]["medoid"]]
            assert list(st.iterations[t][k]) == want_it[t][k]
    # one band per group: the last step's batch holds the last frame of the longer chain, init-major, three members each
    assert [int(v) for v in st._tracer.band_r0] == [r0[2][0]] * 3 + [r0[2][1]] * 3
    st._tracer._batch.close()


# ---- 5, 6: refusals, reset ------------------------------------------------------------------------------------------------------------
def test_a_refused_band_leaves_the_batch_as_it_was(amd, ctx, kernels, scenes):
    sc, L = scenes[65], amd._lib
    make = lambda: amd.GP_Edge_Tracing_Batch(sc["inits"], None, [3, 4], raw_imgs=sc["frames"][0], grad_kernel=kernels[0], band_rows=H,
                                             _ctx=ctx, **KW)
    band, twin = make(), make()
    assert same(band(), twin())
    state = lambda b: ([int(v) for v in b.band_r0], [int(v) for v in b._batch.band_r0()], [o.tolist() for o in b._batch.read_obs_all()],
                       [b._batch.read(L.BUF_GRAD, e).tobytes() for e in range(2)], [bytes(s) for s in b._batch.all_scalars()])
    before = state(band)
    with pytest.raises(ValueError, match="band of edge 0: an init point lies outside its band"):
        band.set_frame(raw_imgs=sc["frames"][1], warm_every=WARM, band=[20, 20])
    with pytest.raises(ValueError, match=r"band of edge 1: r0 lies outside \[0, M - H\]"):
        band.set_frame(raw_imgs=sc["frames"][1], warm_every=WARM, band=[0, 33])
    with pytest.raises(L.GpetError) as ei:  # (the library's own refusal, with band_check's reason)
        band._batch.band_set([20, 20])
    assert ei.value.code == L.ERR_BAD_ARG and "an init point lies outside its band" in str(ei.value)
    with pytest.raises(ValueError, match="H > M"):
        amd.GP_Edge_Tracing_Batch(sc["inits"], None, [3, 4], raw_imgs=sc["frames"][0], grad_kernel=kernels[0], band_rows=M + 1, _ctx=ctx, **KW)
    assert state(band) == before == state(twin)
    for b in (band, twin):
        b.set_frame(raw_imgs=sc["frames"][1], warm_every=WARM)
    assert state(band) == state(twin) and same(band(), twin())
    band._batch.close()
    twin._batch.close()


def test_reset_and_rerun_equals_a_fresh_batch(amd, ctx, kernels, scenes):
    sc = scenes[64]
    make = lambda: amd.GP_Edge_Tracing_Batch(sc["inits"], None, [3, 4], raw_imgs=sc["frames"][0], grad_kernel=kernels[0], band_rows=H,
                                             band_r0=[1, 19], return_std=True, _ctx=ctx, **KW)
    band, fresh = make(), make()
    first = band()
    band.reset()
    assert same(band(), first) and same(fresh(), first)
    # and after a step of a sequence: reset() restores the warm start in the band the step placed
    for b in (band, fresh):
        b.set_frame(raw_imgs=sc["frames"][2], warm_every=WARM, next_frame=False)
    second = band()
    band.reset()
    assert same(band(), second) and same(fresh(), second) and [int(v) for v in band.band_r0] == [int(v) for v in fresh.band_r0]
    band._batch.close()
    fresh._batch.close()
