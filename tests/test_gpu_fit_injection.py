"""GPU tests of the two kernels that turn a converged fit into integers that leave the library, on fits no scene produces:
k_finish_results (the result records: int_f64_to_i64(rint(mean)) and mean -+ 1.96 std) and k_warm_start (the next frame's
observation sets).  The fits are written into the converged fit's output block through GPET_BUF_FIN_OUT.  Every comparison is
exact.  The records' oracle is an explicit table and numpy on the host; the warm start's is sequence.warm_start_obs
(tests/test_warm_start_rule.py) on the trace of the record of the same injected fit -- which ties the roundings of the two
kernels to each other -- and a twin batch given those observations through gpet_batch_set_obs."""
import math
from fractions import Fraction

import numpy as np
import pytest

from gaussian_process_edge_trace_amd import _lib as L
from gaussian_process_edge_trace_amd.sequence import warm_start_obs

pytestmark = pytest.mark.gpu

M, N = 48, 256
IMIN = -2 ** 63
KW_B = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 10, 'length_scale': 12}, noise_y=1, N_samples=200, score_thresh=1,
            delta_x=6, keep_ratio=0.1, pixel_thresh=4, fix_endpoints=True)
KW_A = dict(KW_B, delta_x=2, pixel_thresh=1)  # (a pixel_thresh below 2 is 2, gpet.py:102: algo_thresh = 256 // 2 - 1)
KW_C = dict(KW_B, delta_x=5, pixel_thresh=5)
SPANS3 = [(0, 255), (64, 192), (20, 118)]  # 256, 129 and 99 points
SPANS2 = [(0, 255), (64, 192)]


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


@pytest.fixture(scope="module")
def scene(amd, ctx):
    """Two 48 x 256 gradient images of a sinusoidal edge (a frame and the next) and the edge itself."""
    k = amd.gpet_utils.kernel_builder((11, 5))
    grads = []
    for seed in (3, 4):
        img, edge = amd.gpet_utils.construct_test_img((M, N), int(0.4 * M), 4, 0.05, 'sinusoidal', 0.3, gaps=True, seed=seed)
        grads.append(amd.gpet_utils.comp_grad_img(img, k, ctx=ctx))
    return dict(first=grads[0], second=grads[1], edge=edge)


def make(amd, ctx, scene, kw, spans):
    # (the end point three rows off the edge: two init points on ONE row have no spread, and the converged fit of the init points
    # alone, which standardises the rows by it as the reference does, is then NaN throughout)
    inits = [np.array([[a, scene["edge"][a, 0]], [b, scene["edge"][b, 0] + 3]]) for a, b in spans]
    return amd.GP_Edge_Tracing_Batch(inits, scene["first"], list(range(1, len(spans) + 1)), _ctx=ctx, **kw)


def full_mantissa(rs, n, e_lo, e_hi):
    """n doubles of either sign with exponents uniform over [e_lo, e_hi] and all 52 mantissa bits random."""
    e = rs.randint(e_lo, e_hi + 1, n).astype(np.int64)
    bits = (rs.randint(0, 2, n).astype(np.int64) << 63) | ((e + 1023) << 52) | rs.randint(0, 2 ** 52, n, dtype=np.int64)
    return bits.view(np.float64)


def inject(batch, e, mean, std):
    blk = np.stack([np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)])
    batch.write(L.BUF_FIN_OUT, blk, e)
    back = batch.read(L.BUF_FIN_OUT, e)
    assert back.shape == blk.shape and np.array_equal(back.view(np.int64), blk.view(np.int64)), e  # bit for bit, NaN included


# ---- result records ------------------------------------------------------------------------------------------------------------

# (mean, the row k_finish_results must give): np.rint -- round half to even -- then x86's truncating conversion, which is
# INT64_MIN for NaN, the infinities and every |r| >= 2^63
TABLE = [(0.0, 0), (-0.0, 0), (5e-324, 0), (0.4, 0), (-0.4, 0), (0.5, 0), (-0.5, 0), (1.5, 2), (-1.5, -2), (2.5, 2), (-2.5, -2),
         (254.5, 254), (255.5, 256), (2.0 ** 52 + 1, 4503599627370497), (-(2.0 ** 52 + 1), -4503599627370497),
         (2.0 ** 53 + 2, 9007199254740994), (2.0 ** 62, 4611686018427387904), (-2.0 ** 62, -4611686018427387904),
         (float(np.nextafter(2.0 ** 63, 0.0)), 9223372036854774784), (2.0 ** 63, IMIN), (-2.0 ** 63, IMIN), (9.3e18, IMIN),
         (-9.3e18, IMIN), (1e300, IMIN), (-1e300, IMIN), (np.inf, IMIN), (-np.inf, IMIN), (np.nan, IMIN)]


def fused(m, s):
    """m - 1.96 s and m + 1.96 s with ONE rounding each: what a kernel that contracts the interval would give."""
    if hasattr(math, "fma"):
        return math.fma(-1.96, s, m), math.fma(1.96, s, m)
    d = Fraction(1.96) * Fraction(s)
    return float(Fraction(m) - d), float(Fraction(m) + d)


def injected_fit(e, Lg):
    """(mean, std, expected rows as Python integers, the grid indices that hold TABLE's means) of edge e: TABLE at seeded places
    -- another permutation per edge, so that an offset between the edges shows --, the rest seeded doubles with exponents over
    [-30, 60]; stds over [2^-19, 2^19), inside [1e-6, 1e6]."""
    rs = np.random.RandomState(40 + e)
    m = full_mantissa(rs, Lg, -30, 60)
    want = [int(np.rint(v)) for v in m.tolist()]  # (exact: |v| < 2^61)
    at = rs.permutation(Lg)[:len(TABLE)].tolist()
    for i, (v, r) in zip(at, TABLE):
        m[i] = v
        want[i] = r
    s = np.abs(full_mantissa(rs, Lg, -19, 18))
    assert s.min() >= 1e-6 and s.max() <= 1e6
    return m, s, want, set(at)


@pytest.fixture(scope="module")
def injected_records(amd, ctx, scene):
    """One batch of three edges brought to a converged fit, then given the injected fits; everything the record tests read."""
    b = make(amd, ctx, scene, KW_B, SPANS3)
    bt = b._batch
    mean0, std0 = bt.final_fit_all([11, 12, 13])[:2]
    lgs = [p["edge_length"] for p in b._ps]
    assert lgs == [256, 129, 99] and bt._max_info("Lg") == 256
    fit_blocks = [bt.read(L.BUF_FIN_OUT, e) for e in range(3)]
    head0 = bt.results()
    means, stds, rows = [], [], []
    for e, Lg in enumerate(lgs):
        m, s, want, at = injected_fit(e, Lg)
        inject(bt, e, m, s)
        means.append(m)
        stds.append(s)
        rows.append((want, at))
    out = dict(b=b, lgs=lgs, mean0=mean0, std0=std0, fit_blocks=fit_blocks, head0=head0, means=means, stds=stds, rows=rows,
               rec=bt.results(), rec300=bt.results(len_cap=300))
    yield out
    bt.close()


def test_fin_out_reads_what_the_converged_fit_returned(injected_records):
    r = injected_records
    for e, Lg in enumerate(r["lgs"]):
        blk = r["fit_blocks"][e]
        assert blk.shape == (2, Lg) and blk.dtype == np.float64
        assert np.array_equal(blk[0], r["mean0"][e, :Lg]) and np.array_equal(blk[1], r["std0"][e, :Lg]), e
        assert np.all(np.isfinite(blk)) and np.all(blk[1] > 0)  # (a fit, not an untouched buffer)


def test_fin_out_write_takes_exactly_two_rows_of_the_edge(injected_records):
    bt = injected_records["b"]._batch
    before = [bt.read(L.BUF_FIN_OUT, e) for e in range(3)]
    for e, n in [(0, 2 * 256 - 1), (0, 2 * 256 + 1), (1, 2 * 256), (1, 129), (2, 2 * 99 + 2)]:
        with pytest.raises(L.GpetError) as ei:
            bt.write(L.BUF_FIN_OUT, np.zeros(n), e)
        assert ei.value.code == L.ERR_BAD_ARG, (e, n)
    for e in range(3):  # a refused write wrote nothing
        assert np.array_equal(bt.read(L.BUF_FIN_OUT, e).view(np.int64), before[e].view(np.int64))


@pytest.mark.parametrize("which", ["rec", "rec300"])
def test_record_rows_of_injected_means(injected_records, which):
    r = injected_records
    rec = r[which]
    cap = 256 if which == "rec" else 300
    assert rec["trace"].shape == (3, cap, 2) and rec["trace"].dtype == np.int64
    for e, (Lg, p) in enumerate(zip(r["lgs"], r["b"]._ps)):
        want, table_at = r["rows"][e]
        got = rec["trace"][e, :Lg, 0].tolist()
        bad = [(k, r["means"][e][k], got[k], want[k]) for k in range(Lg) if got[k] != want[k]]
        assert not bad, (e, bad[:8])
        assert len(table_at) == len(TABLE)
        assert rec["trace"][e, :Lg, 1].tolist() == [p["x_st"] + k for k in range(Lg)], e  # the x column
        # past the edge's own length everything is zero
        assert not rec["trace"][e, Lg:].any() and not rec["lower"][e, Lg:].any() and not rec["upper"][e, Lg:].any(), e


def test_seeded_fits_would_fail_a_contracted_interval(injected_records):
    """A condition on the inputs: on at least 10 % of the seeded points the interval with one rounding differs from numpy's
    with two, so a kernel that contracts mean -+ 1.96 std into a fused multiply-add cannot pass the test below."""
    r = injected_records
    n = differ = 0
    for e, Lg in enumerate(r["lgs"]):
        m, s = r["means"][e], r["stds"][e]
        lo, up = m - 1.96 * s, m + 1.96 * s
        for k in range(Lg):
            if k in r["rows"][e][1]:
                continue
            flo, fup = fused(float(m[k]), float(s[k]))
            n += 1
            differ += (flo != lo[k]) or (fup != up[k])
    print("fused differs on %d of %d seeded points" % (differ, n))
    assert n == sum(r["lgs"]) - 3 * len(TABLE) and differ >= 0.1 * n, (differ, n)


@pytest.mark.parametrize("which", ["rec", "rec300"])
def test_record_interval_is_numpys_two_roundings_bit_for_bit(injected_records, which):
    r = injected_records
    rec = r[which]
    for e, Lg in enumerate(r["lgs"]):
        m, s = r["means"][e], r["stds"][e]
        with np.errstate(invalid="ignore", over="ignore"):
            lo, up = m - 1.96 * s, m + 1.96 * s
        for name, want in (("lower", lo), ("upper", up)):
            got = rec[name][e, :Lg]
            bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
            assert bad.size == 0, (e, name, [(int(k), m[k], s[k], got[k], want[k]) for k in bad[:8]])


def test_record_head_is_unchanged_by_the_write(injected_records):
    r = injected_records
    for rec in (r["rec"], r["rec300"]):
        for k in ("edge_len", "n_obs", "n_iter", "status", "theta", "nlml"):
            assert np.array_equal(rec[k], r["head0"][k]), k
        assert rec["edge_len"].tolist() == r["lgs"]
    # and before the write the record was the converged fit's
    for e, Lg in enumerate(r["lgs"]):
        assert r["head0"]["trace"][e, :Lg, 0].tolist() == [int(v) for v in np.rint(r["mean0"][e, :Lg]).tolist()]


# ---- warm start ----------------------------------------------------------------------------------------------------------------

def irregular(seed, Lg, lo=-6.0, hi=M + 5.0):
    """Means on both sides of both borders of the image: uniform rows, every 7th a NaN, one +inf, and -- twice, at grid indices
    that no stride up to 8 skips together -- -0.4 (row 0, kept), M - 1 + 0.5 (rounds to M, dropped), M - 0.51 (row M - 1, kept)."""
    m = np.random.RandomState(seed).uniform(lo, hi, Lg)
    m[::7] = np.nan
    m[100] = np.inf
    for k, v in ((10, -0.4), (12, M - 1 + 0.5), (16, M - 0.51), (66, -0.4), (68, M - 1 + 0.5), (72, M - 0.51)):
        m[k] = v
    return m


def state(b):
    return b._batch.read_obs_all(), [(s.n_obs, s.done, s.iter, s.status) for s in b._batch.all_scalars()]


def canary(b, e):
    """obs_cap in-image points that no warm start yields: descending x."""
    p, cap = b._ps[e], b._batch.info(e)["obs_cap"]
    i = np.arange(cap, dtype=np.int64)
    return np.stack([p["x_en"] - i % p["edge_length"], (5 * i + 3) % M], axis=1)


def converged_with_stale_obs(b):
    """A fresh converged fit (a warm start uses the last one up) of the init points alone, with obs_xy full of the canary."""
    for e in range(b.B):
        b._batch.set_obs(e, canary(b, e))
        b._batch.set_obs(e, np.zeros((0, 2), dtype=np.int64))  # (n_obs = 0; the points stay in obs_xy)
    b._batch.final_fit_all(list(range(5, 5 + b.B)))


def oracle(b):
    """warm_start_obs on the trace of the record of the fit that is on the device now, for every warm_every asked."""
    rec = b._batch.results()

    def of(warm_every):
        return [warm_start_obs(rec["trace"][e, :p["edge_length"]], p["x_st"], p["x_en"], warm_every, p["algo_thresh"], p["M"])
                for e, p in enumerate(b._ps)]
    return of


def warm_and_compare(dev, twin, means, warm_every):
    """Injects `means` after a fresh converged fit, warm-starts on the device, gives the twin the oracle's sets through
    gpet_batch_set_obs; both must be in the same state, with exactly the oracle's observations.  Returns the oracle's sets."""
    converged_with_stale_obs(dev)
    for e, m in enumerate(means):
        inject(dev._batch, e, m, np.full(len(m), 0.75))
    want = oracle(dev)(warm_every)
    cnt = dev._batch.warm_start(warm_every)
    for e in range(twin.B):
        twin._batch.set_obs(e, want[e])
    (obs_d, sc_d), (obs_t, sc_t) = state(dev), state(twin)
    assert cnt.dtype == np.int32 and cnt.tolist() == [len(o) for o in want], (cnt.tolist(), [len(o) for o in want])
    assert sc_d == sc_t, (sc_d, sc_t)
    for e, p in enumerate(dev._ps):
        assert cnt[e] <= dev._batch.info(e)["obs_cap"]
        assert sc_d[e] == (len(want[e]), int(len(want[e]) >= p["algo_thresh"]), 0, 0), (e, sc_d[e])
        assert obs_d[e].dtype == np.int64 and obs_d[e].shape == want[e].shape, (e, obs_d[e].shape, want[e].shape)
        assert np.array_equal(obs_d[e], want[e]) and np.array_equal(obs_t[e], want[e]), e
    return want


@pytest.fixture(scope="module")
def pair_a(amd, ctx, scene):
    dev, twin = make(amd, ctx, scene, KW_A, SPANS2), make(amd, ctx, scene, KW_A, SPANS2)
    # (pixel_thresh = 1 is clamped to 2 as in the reference, so the full-width threshold is 256 // 2 - 1 = 127, not 128)
    assert [p["algo_thresh"] for p in dev._ps] == [127, 63] and [p["edge_length"] for p in dev._ps] == [256, 129]
    assert [dev._batch.info(e)["algo_thresh"] for e in range(2)] == [127, 63]
    assert dev._batch.info(0)["obs_cap"] == 130 and dev._batch.info(1)["obs_cap"] >= 64
    yield dev, twin
    dev._batch.close()
    twin._batch.close()


@pytest.fixture(scope="module")
def pair_b(amd, ctx, scene):
    dev, twin = make(amd, ctx, scene, KW_B, SPANS2), make(amd, ctx, scene, KW_B, SPANS2)
    assert [p["algo_thresh"] for p in dev._ps] == [39, 18] and [dev._batch.info(e)["algo_thresh"] for e in range(2)] == [39, 18]
    yield dev, twin
    dev._batch.close()
    twin._batch.close()


def test_warm_start_all_rows_inside(pair_a):
    """254 candidates, then 127 -- not below the threshold of 127 --, then 63: solid ballot masks."""
    dev, twin = pair_a
    rs = np.random.RandomState(7)
    want = warm_and_compare(dev, twin, [rs.uniform(-0.49, M - 0.51, 256), rs.uniform(-0.49, M - 0.51, 129)], 1)
    assert [len(o) for o in want] == [63, 31]
    assert np.all(np.diff(want[0][:, 0]) == 4) and np.all(np.diff(want[1][:, 0]) == 4)


def test_warm_start_a_solid_run_over_two_passes(pair_a):
    """The first 126 inner pixels inside the image, the rest outside: 126 < 127 kept at stride 1, compacted in two passes of 64
    and 62 with solid masks (the running base of the second pass is 64), then two passes that keep nothing.  (With 256
    columns no set of 127 can be kept: pixel_thresh is at least 2, so the threshold is at most 127.)"""
    dev, twin = pair_a
    rs = np.random.RandomState(8)
    m0 = np.full(256, np.nan)
    m0[1:127] = rs.uniform(-0.49, M - 0.51, 126)
    m1 = np.full(129, float(M))
    m1[60:122] = rs.uniform(-0.49, M - 0.51, 62)  # 62 < 63, across the boundary between the two passes
    want = warm_and_compare(dev, twin, [m0, m1], 1)
    assert [len(o) for o in want] == [126, 62] and want[0][:, 0].tolist() == list(range(1, 127))


def test_warm_start_irregular_rows(pair_a):
    """Rows on both sides of both borders, NaN and inf: at stride 2 the full-width edge keeps more than 64 of its 127 candidates
    -- two passes with broken ballot masks."""
    dev, twin = pair_a
    want = warm_and_compare(dev, twin, [irregular(1, 256), irregular(2, 129)], 1)
    assert len(want[0]) > 64, len(want[0])
    for e, x_st in enumerate((0, 64)):
        pts = {tuple(p) for p in want[e].tolist()}
        xs = set(want[e][:, 0].tolist())
        assert np.all(np.diff(want[e][:, 0]) % 2 == 0) and np.any(np.diff(want[e][:, 0]) > 2), e  # stride 2, with holes
        assert {(x_st + 10, 0), (x_st + 16, M - 1), (x_st + 66, 0), (x_st + 72, M - 1)} <= pts, e
        assert not {x_st + 12, x_st + 68, x_st + 14, x_st + 100} & xs, e  # M, NaN and inf are dropped


def test_warm_start_sparse_rows_over_four_passes(pair_a):
    """Rows spread far beyond the image: fewer than half are inside, so stride 1 stays below the threshold and the compaction
    runs four passes (three for the half-width edge) with broken masks."""
    dev, twin = pair_a
    want = warm_and_compare(dev, twin, [irregular(3, 256, -40.0, M + 40.0), irregular(4, 129, -40.0, M + 40.0)], 1)
    assert 64 < len(want[0]) < 127 and np.any(np.diff(want[0][:, 0]) == 1) and want[0][-1, 0] > 192
    assert 32 < len(want[1]) < 63 and np.any(np.diff(want[1][:, 0]) == 1)


def test_warm_start_irregular_rows_sparse_thresholds(pair_b):
    """Thresholds 39 and 18: several doublings, then a sparse set."""
    dev, twin = pair_b
    want = warm_and_compare(dev, twin, [irregular(1, 256), irregular(2, 129)], 1)
    assert 0 < len(want[0]) < 39 and 0 < len(want[1]) < 18
    assert np.all(np.diff(want[0][:, 0]) % 4 == 0)  # (at least two doublings)


@pytest.mark.parametrize("warm_every", [0, -5, 3, 64, 254, 255, 256, 2 ** 31 - 1])
def test_warm_start_strides(pair_a, pair_b, warm_every):
    """warm_every below 1 is 1; Lg - 2 leaves one candidate of the full-width edge, Lg - 1 and above none."""
    for dev, twin in (pair_a, pair_b):
        means = [irregular(1, 256), irregular(2, 129)]
        if warm_every == 254:
            means[0][254] = 20.2  # (the one candidate is inside the image)
        want = warm_and_compare(dev, twin, means, warm_every)
        if warm_every == 254:
            assert want[0].tolist() == [[254, 20]] and len(want[1]) == 0
        if warm_every >= 255:
            assert [len(o) for o in want] == [0, 0]
        if warm_every == 64:
            assert set(want[0][:, 0].tolist()) <= {64, 128, 192} and set(want[1][:, 0].tolist()) <= {128}


@pytest.mark.parametrize("row", [np.nan, float(M), -1.0, M - 0.5, -0.5000001], ids=["nan", "M", "minus1", "M-0.5", "below-0.5"])
def test_warm_start_all_rows_outside(pair_a, row):
    dev, twin = pair_a
    want = warm_and_compare(dev, twin, [np.full(256, row), np.full(129, row)], 1)
    assert [len(o) for o in want] == [0, 0]
    assert [s[1] for s in state(dev)[1]] == [0, 0]  # not done: the next trace's loop runs


def test_warm_start_of_an_edge_without_a_threshold(amd, ctx, scene):
    """8 columns with delta_x = 5 and pixel_thresh = 5: algo_thresh = 1 - 4 <= 0, which no count is below -- the stride doubles
    until nothing is kept, and the edge is done, as gpet_batch_set_obs leaves it."""
    dev, twin = make(amd, ctx, scene, KW_C, [(100, 107)]), make(amd, ctx, scene, KW_C, [(100, 107)])
    assert dev._ps[0]["algo_thresh"] == -3 and dev._batch.info(0)["algo_thresh"] == -3 and dev._ps[0]["edge_length"] == 8
    want = warm_and_compare(dev, twin, [np.full(8, 20.0)], 1)
    assert len(want[0]) == 0 and state(dev)[1] == [(0, 1, 0, 0)]
    dev._batch.close()
    twin._batch.close()


def test_warm_start_leaves_nothing_stale(pair_a):
    """obs_xy is full of recognisable points before the warm start; afterwards exactly the oracle's are read, and with the
    count raised by hand to obs_cap the points past the oracle's are still the canary's: the kernel wrote its own and no more."""
    dev, twin = pair_a
    for e in range(2):
        dev._batch.set_obs(e, canary(dev, e))
    filled = dev._batch.read_obs_all()
    assert all(np.array_equal(filled[e], canary(dev, e)) and len(filled[e]) == dev._batch.info(e)["obs_cap"] for e in range(2))
    want = warm_and_compare(dev, twin, [irregular(1, 256), irregular(2, 129)], 1)  # (fills obs_xy the same way once more)
    for e in range(2):
        cap = dev._batch.info(e)["obs_cap"]
        assert 0 < len(want[e]) < cap
        s = dev._batch.scalars(e)
        s.n_obs = cap
        dev._batch.write_scalars(s, e)
        every = dev._batch.read(L.BUF_OBS, e)
        assert np.array_equal(every[:len(want[e])], want[e]) and np.array_equal(every[len(want[e]):], canary(dev, e)[len(want[e]):]), e


@pytest.mark.parametrize("kw", [KW_A, KW_B], ids=["A", "B"])
def test_traces_after_a_device_warm_start_equal_the_twins(amd, ctx, scene, kw):
    """set_frame(..., warm_every=1) on the injected irregular fit against set_frame(..., obs=oracle): the same state, then the
    same traces in the same number of iterations."""
    dev, twin = make(amd, ctx, scene, kw, SPANS2), make(amd, ctx, scene, kw, SPANS2)
    converged_with_stale_obs(dev)
    for e, m in enumerate([irregular(1, 256), irregular(2, 129)]):
        inject(dev._batch, e, m, np.full(len(m), 0.75))
    want = oracle(dev)(1)
    dev.set_frame(scene["second"], None, [21, 22], warm_every=1)
    twin.set_frame(scene["second"], want, [21, 22])
    (obs_d, sc_d), (obs_t, sc_t) = state(dev), state(twin)
    assert sc_d == sc_t and [s[0] for s in sc_d] == [len(o) for o in want] and min(len(o) for o in want) >= 1
    assert all(np.array_equal(a, w) and np.array_equal(t, w) for a, t, w in zip(obs_d, obs_t, want))
    out_d, out_t = dev(), twin()
    assert list(dev.timings["iters"]) == list(twin.timings["iters"]) and min(dev.timings["iters"]) >= 1
    for e in range(2):
        assert out_d[e].shape == (dev._ps[e]["edge_length"], 2) and np.array_equal(out_d[e], out_t[e]), e
    dev._batch.close()
    twin._batch.close()
