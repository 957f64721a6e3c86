"""CPU tests of endpoint tracking above the library: how the init keywords are resolved before anything touches a device
(gpet.resolve_init_follow, gpet.resolve_frame_init), how SequenceTracer carries the init points from frame to frame and across a
rebuilt batch (the batch class replaced by a stub), and a quality check of the rule alone (tests/init_follow_ref.py) on drifting
frames."""
import types

import numpy as np
import pytest

from gaussian_process_edge_trace_amd import gpet, gpet_utils, sequence
from tests import init_follow_ref as R

M, N, H = 64, 65, 24
CUR = [np.array([[0, 20], [N - 1, 24]]), np.array([[0, 40], [30, 39], [N - 1, 38]])]


# ---- init_follow=dict(window=, cols=) ------------------------------------------------------------------------------------------------
def test_init_follow_keyword():
    assert gpet.resolve_init_follow(None) is None
    assert gpet.resolve_init_follow(dict(window=8, cols=4)) == (8, 4)
    assert gpet.resolve_init_follow(dict(window=np.int64(0), cols=np.int32(64))) == (0, 64)
    assert gpet.resolve_init_follow(dict(window=4096, cols=0)) == (4096, 0)
    for bad in (8, (8, 4), dict(window=8), dict(cols=4), dict(window=8, cols=4, gate=0.5), "follow"):
        with pytest.raises(ValueError, match=r"init_follow must be None or dict\(window=w, cols=a\)"):
            gpet.resolve_init_follow(bad)
    for bad, words in ((dict(window=8.0, cols=4), "window must be an integer"), (dict(window=8, cols="4"), "cols must be an integer"),
                       (dict(window=True, cols=4), "window must be an integer"), (dict(window=-1, cols=4), "window must be at least 0"),
                       (dict(window=4097, cols=4), "window exceeds 4096"), (dict(window=8, cols=-1), "cols must be at least 0"),
                       (dict(window=8, cols=65), "cols exceeds 64")):
        with pytest.raises(ValueError, match=words):
            gpet.resolve_init_follow(bad)


def test_the_sequence_tracer_refuses_a_bad_window_before_it_looks_at_a_frame():
    frames = [np.zeros((M, N), dtype=np.float32)] * 3
    with pytest.raises(ValueError, match="window exceeds 4096"):
        sequence.SequenceTracer(frames, CUR[0], init_follow=dict(window=5000, cols=2))
    st = sequence.SequenceTracer(frames, CUR[0], init_follow=dict(window=5, cols=2))
    assert st.init_follow == dict(window=5, cols=2) and st.inits == [None] * 3


# ---- set_frame(init=, init_follow=) --------------------------------------------------------------------------------------------------
def test_what_set_frame_does_with_the_init_points():
    f = gpet.resolve_frame_init
    assert f(None, None, None, CUR, M) == ("keep", None)                     # no keyword anywhere: what is enqueued today
    assert f(None, None, (8, 4), CUR, M) == ("follow", (8, 4))               # the constructor's setting is the default
    assert f(None, dict(window=3, cols=1), (8, 4), CUR, M) == ("follow", (3, 1))   # this call's wins
    assert f(None, dict(window=3, cols=1), None, CUR, M) == ("follow", (3, 1))
    assert f("follow", None, (8, 4), CUR, M) == ("follow", (8, 4))
    assert f("keep", None, (8, 4), CUR, M) == ("keep", None)
    mode, pts = f([CUR[0] + [0, 3], CUR[1][::-1] + [0, -2]], None, (8, 4), CUR, M)
    assert mode == "set" and all(p.dtype == np.int64 for p in pts)
    assert np.array_equal(pts[0], CUR[0] + [0, 3]) and np.array_equal(pts[1], CUR[1] + [0, -2])   # (sorted by x, as the batch holds them)


def test_set_frame_conflicts_are_value_errors():
    f = gpet.resolve_frame_init
    with pytest.raises(ValueError, match="init='follow' needs init_follow"):
        f("follow", None, None, CUR, M)
    with pytest.raises(ValueError, match="init='keep' and init_follow are alternatives"):
        f("keep", dict(window=8, cols=4), None, CUR, M)
    with pytest.raises(ValueError, match="must be None, 'keep', 'follow'"):
        f("track", None, (8, 4), CUR, M)
    with pytest.raises(ValueError, match="arrays and init_follow are alternatives"):
        f(list(CUR), dict(window=8, cols=4), None, CUR, M)
    with pytest.raises(ValueError, match="window must be at least 0"):
        f("follow", dict(window=-2, cols=4), (8, 4), CUR, M)
    with pytest.raises(ValueError, match="init has 1 entries for 2 edges"):
        f([CUR[0]], None, None, CUR, M)
    with pytest.raises(ValueError, match="init of edge 1 has shape"):
        f([CUR[0], CUR[1][:2]], None, None, CUR, M)
    with pytest.raises(ValueError, match="init of edge 0 has x = .* cannot change"):
        f([CUR[0] + [1, 0], CUR[1]], None, None, CUR, M)
    with pytest.raises(ValueError, match="init of edge 0 is not integral"):
        f([CUR[0] + 0.5, CUR[1]], None, None, CUR, M)
    with pytest.raises(ValueError, match="init of edge 1: an init point lies outside the frame"):
        f([CUR[0], CUR[1] + [0, 30]], None, None, CUR, M)
    with pytest.raises(ValueError, match="init of edge 0: an init point lies outside the frame"):
        f([CUR[0] - [0, 21], CUR[1]], None, None, CUR, M)


def test_init_arrays_on_a_banded_batch_need_their_bands():
    f = gpet.resolve_frame_init
    for band in (None, "follow"):
        with pytest.raises(ValueError, match=r"need the bands too: band=\[r0 of every edge\]"):
            f(list(CUR), None, None, CUR, M, band_rows=H, band=band)
    assert f(list(CUR), None, None, CUR, M, band_rows=H, band=[10, 20])[0] == "set"
    with pytest.raises(ValueError, match="band of edge 1: an init point lies outside its band"):
        f(list(CUR), None, None, CUR, M, band_rows=H, band=[10, 16])           # rows 38 .. 40 in rows 16 .. 39
    with pytest.raises(ValueError, match="band of edge 0: the init rows span more rows"):
        f([CUR[0] + [[0, 0], [0, 30]], CUR[1]], None, None, CUR, M, band_rows=H, band=[10, 20])
    # following needs no table: the search is confined to the band by the rule itself
    assert f(None, None, (8, 4), CUR, M, band_rows=H, band="follow") == ("follow", (8, 4))


# ---- SequenceTracer: the init points travel with the chains, the device stubbed out ----------------------------------------------------
class StubBatch(object):
    """Stands where GP_Edge_Tracing_Batch stands in sequence.py: 'following' lowers every init point by one row per frame."""
    built = []

    def __init__(self, inits, seeds=None, obs=None, device=0, _ctx=None, image_of=None, init_follow=None, grad_imgs=None, **kw):
        self.B, self.return_std, self._ctx = len(inits), False, object()
        self._batch = types.SimpleNamespace(close=lambda: None)
        self.given = list(inits)
        self.follow, self.frames_set, self.width = init_follow, 0, np.asarray(grad_imgs[0]).shape[1]
        self.inits = [self._step(np.asarray(i)[np.argsort(np.asarray(i)[:, 0])].astype(np.int64)) for i in inits]
        StubBatch.built.append(self)

    def _step(self, i):
        return i + np.array([0, 1]) if self.follow is not None else i

    def set_frame(self, imgs, obs, seeds, raw_imgs=None, **warm):
        assert "init" not in warm and "init_follow" not in warm   # (the batch remembers the constructor's setting)
        self.frames_set += 1
        self.inits = [self._step(i) for i in self.inits]

    def __call__(self, max_iter):
        self.timings = dict(iters=[1] * self.B)
        return [np.stack([np.full(self.width, 10), np.arange(self.width)], axis=1)] * self.B


@pytest.fixture
def stubbed(monkeypatch):
    StubBatch.built = []
    monkeypatch.setattr(sequence, "GP_Edge_Tracing_Batch", StubBatch)
    return StubBatch


def test_inits_are_carried_per_chain_and_across_a_rebuild(stubbed):
    """5 frames in 2 chains of 3 and 2: steps 0 and 1 run both chains in one batch, step 2 the longer chain alone in a rebuilt one."""
    frames = [np.zeros((32, 40), dtype=np.float32)] * 5
    a = np.array([[39, 12], [0, 10]])              # given right to left: filed in this order, handed to the batch as given
    b = np.array([[5, 20], [20, 21], [35, 22]])
    st = sequence.SequenceTracer(frames, [a, b], n_chains=2, warm_every=4, init_follow=dict(window=3, cols=1), delta_x=5)
    st()
    assert len(stubbed.built) == 2 and [x.B for x in stubbed.built] == [4, 2] and [x.frames_set for x in stubbed.built] == [1, 0]
    first, rebuilt = stubbed.built
    assert first.follow == rebuilt.follow == dict(window=3, cols=1)
    for g, w in zip(first.given, [a, b, a, b]):    # every chain's first frame starts from the user's points
        assert np.array_equal(g, w)
    for g, w in zip(rebuilt.given, [a + [0, 2], b + [0, 2]]):   # the rebuilt batch from where chain 0 stood after two frames
        assert np.array_equal(g, w) and g.dtype == np.int64
    steps = [1, 2, 3, 1, 2]                         # frames 0 .. 2 are chain 0, frames 3 .. 4 chain 1
    for t in range(5):
        assert np.array_equal(st.inits[t][0], a + [0, steps[t]]) and np.array_equal(st.inits[t][1], b + [0, steps[t]]), t


def test_without_init_follow_every_frame_has_the_given_points(stubbed):
    frames = [np.zeros((32, 40), dtype=np.float32)] * 5
    a = np.array([[0, 10], [39, 12]])
    st = sequence.SequenceTracer(frames, a, n_chains=2, warm_every=4, delta_x=5)
    st()
    assert [x.follow for x in stubbed.built] == [None, None] and all(x.given[0] is st._inits[0] for x in stubbed.built)
    assert all(np.array_equal(i, a) for i in st.inits) and st._cur == {}


# ---- the rule alone, on drifting frames ----------------------------------------------------------------------------------------------
def test_followed_end_points_stay_on_a_drifting_edge():
    """96 x 72 frames whose edge sinks 3 rows per frame (tests/init_follow_ref.drifting_frames), t = 0 .. 9, seeds 0 .. 15, window = 8,
    cols = 4, end points at x = 0 and x = N - 1: every followed end point stays within 4 rows of the true edge row on every frame (the
    worst case of the numpy rule was 2), while the frame-0 points are 27 rows off at t = 9."""
    import scipy.ndimage as ndi
    Mq, Nq, T = 96, 72, 10
    K = gpet_utils.kernel_builder((11, 5))
    worst, stale = 0, 0
    for seed in range(16):
        frames, rows = R.drifting_frames(Mq, Nq, T, seed)
        init = np.array([[0, rows[0][0]], [Nq - 1, rows[0][-1]]], dtype=np.int64)
        cur = init
        for t in range(T):
            g = np.maximum(ndi.convolve(frames[t], K, mode="nearest"), 0.0)
            g = ((g - g.min()) / (g.max() - g.min())).astype(np.float32)
            cur = R.follow(g, cur, 8, 4)
            assert np.array_equal(cur[:, 0], init[:, 0])
            truth = np.array([rows[t][0], rows[t][-1]])
            worst = max(worst, int(np.abs(cur[:, 1] - truth).max()))
            stale = max(stale, int(np.abs(init[:, 1] - truth).max()))
            assert np.abs(cur[:, 1] - truth).max() <= 4, (seed, t, cur, truth)
    print("worst followed end point: %d rows off; frame-0 end points: %d rows off" % (worst, stale))
    assert stale == 27
