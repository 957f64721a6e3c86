"""What the Python layer of the wavelet stage decides without a device: how the kwargs of gpet_utils.denoise(image, 'wavelet',
kwargs) become a gpet_wavelet spec, which keys and values are refused (by name), that the stage runs only when kwargs names the
``wavelet`` key, the level rule, and how resolve_image_source / RawFrames carry the spec through the one pre-stage seam that
non-local means uses too."""
import math

import numpy as np
import pytest

from gaussian_process_edge_trace_amd import _lib, gpet, gpet_utils

K = np.array([[1.0, 2.0, 1.0], [0.0, 0.0, 0.0], [-1.0, -2.0, -1.0]])
FRAME = np.zeros((40, 60), dtype=np.uint8)


def test_spec_carries_skimages_defaults():
    sp = _lib.wavelet_spec(dict(wavelet="db1"))
    c = sp.c
    assert (c.n_taps, c.levels, c.mode, c.method, c.rescale_sigma, c.ppf) == (2, 0, 0, 0, 1, 0.6744897501960817)
    assert math.isnan(c.sigma) and list(c.dec_lo)[:2] == [0.70710678118654757, 0.70710678118654757] and not any(list(c.dec_lo)[2:])
    assert sp.thresholds is None and not c.thresholds and sp.name == "db1"
    sp = _lib.wavelet_spec(dict(wavelet="db4", sigma=0.05, mode="hard", method="VisuShrink", wavelet_levels=2, rescale_sigma=False,
                                multichannel=False, convert2ycbcr=False))
    c = sp.c
    assert (c.n_taps, c.levels, c.mode, c.method, c.rescale_sigma, c.sigma) == (8, 2, 1, 1, 0, 0.05)
    assert list(c.dec_lo)[:8] == _lib.wavelet_table()["db4"]
    assert _lib.wavelet_spec(dict(wavelet="haar")).dec_lo == _lib.wavelet_spec(dict(wavelet="db1")).dec_lo


@pytest.mark.parametrize("kw", [{}, dict(sigma=0.1), dict(mode="soft", method="BayesShrink"), None])
def test_without_the_wavelet_key_the_technique_stays_not_built(kw):
    for call in (lambda: _lib.wavelet_spec(kw), lambda: gpet_utils.denoise(FRAME, "wavelet", kw), lambda: gpet_utils.denoise_imgs([FRAME], "wavelet", kw),
                 lambda: gpet.resolve_image_source(1, raw_imgs=FRAME, grad_kernel=K, denoise=("wavelet", kw)),
                 lambda: _lib.denoise_spec(("wavelet", kw))):
        with pytest.raises(NotImplementedError, match="names the wavelet"):
            call()


@pytest.mark.parametrize("key", ["preserve_range", "size", "weight", "channel_axis", "threshold", "patch_size"])
def test_other_keys_are_refused_by_name(key):
    with pytest.raises(ValueError, match=key):
        _lib.wavelet_spec(dict(wavelet="db1", **{key: 1}))
    with pytest.raises(ValueError, match=key):
        gpet_utils.denoise(FRAME, "wavelet", dict(wavelet="db1", **{key: 1}))  # (refused before a device is looked for)


@pytest.mark.parametrize("kw, match", [
    (dict(wavelet="bior2.2"), "wavelet_table"), (dict(wavelet="db9"), "wavelet_table"), (dict(wavelet="dmey"), "wavelet_table"),
    (dict(wavelet=3), "wavelet_table"), (dict(wavelet="db1", multichannel=True), "multichannel"),
    (dict(wavelet="db1", convert2ycbcr=True), "convert2ycbcr"), (dict(wavelet="db1", mode="garrote"), "garrote"),
    (dict(wavelet="db1", method="SureShrink"), "SureShrink"), (dict(wavelet="db1", wavelet_levels=0), "wavelet_levels"),
    (dict(wavelet="db1", wavelet_levels=1.5), "wavelet_levels"), (dict(wavelet="db1", sigma=0.0), "sigma"),
    (dict(wavelet="db1", sigma=-1.0), "sigma"), (dict(wavelet="db1", sigma=[0.1, 0.2]), "sigma"), (dict(wavelet="db1", sigma=float("inf")), "sigma")])
def test_values_the_device_refuses(kw, match):
    with pytest.raises(ValueError, match=match):
        _lib.wavelet_spec(kw)
    with pytest.raises(ValueError, match=match):
        gpet_utils.denoise(FRAME, "wavelet", kw)


def test_the_table_names_what_it_holds():
    table = _lib.wavelet_table()
    assert list(table) == ["haar"] + ["db%d" % k for k in range(1, 9)] + ["sym%d" % k for k in range(2, 9)] + ["coif1", "coif2"]
    assert [len(table[n]) for n in ("haar", "db1", "db8", "sym2", "sym8", "coif1", "coif2")] == [2, 2, 16, 4, 16, 6, 12]
    for name, lo in table.items():  # an orthogonal low-pass filter: unit norm, sum sqrt(2) (PyWavelets tabulates some to 11 digits)
        assert abs(sum(v * v for v in lo) - 1.0) < 1e-10 and abs(sum(lo) - math.sqrt(2.0)) < 1e-10, name
    with pytest.raises(ValueError) as e:
        _lib.wavelet_spec(dict(wavelet="bior1.3"))
    assert all(n in str(e.value) for n in table)


def test_level_rule():
    # the largest L with (F - 1) 2^L <= n
    assert [_lib.wavelet_max_level(n, F) for n, F in ((37, 4), (64, 2), (40, 8), (30, 16), (29, 16), (500, 2), (500, 8))] == [3, 6, 2, 1, 0, 8, 6]
    assert [_lib.wavelet_out_len(n, F) for n, F in ((37, 4), (50, 4), (30, 16), (33, 2))] == [20, 26, 22, 17]
    sp = _lib.wavelet_spec(dict(wavelet="db2"))
    assert [sp.levels_on(s) for s in ((37, 50), (130, 150), (500, 500), (6, 900))] == [1, 2, 4, 1]  # max(max_level - 3, 1)
    assert _lib.wavelet_spec(dict(wavelet="db1")).levels_on((500, 500)) == 5
    assert _lib.wavelet_spec(dict(wavelet="db2", wavelet_levels=3)).levels_on((37, 50)) == 3
    with pytest.raises(ValueError, match="above max_level 3"):
        _lib.wavelet_spec(dict(wavelet="db2", wavelet_levels=4)).levels_on((37, 50))
    with pytest.raises(ValueError, match="above max_level 1"):  # (taken over the SMALLER extent: 80 alone would allow two)
        _lib.wavelet_spec(dict(wavelet="db8", wavelet_levels=2)).levels_on((48, 80))
    with pytest.raises(ValueError, match="max_level is 0"):
        _lib.wavelet_spec(dict(wavelet="db8")).levels_on((29, 500))
    # ... and frames refuse such a spec before a device is needed
    with pytest.raises(ValueError, match="above max_level"):
        gpet_utils.denoise(FRAME, "wavelet", dict(wavelet="db4", wavelet_levels=3))
    with pytest.raises(ValueError, match="max_level is 0"):
        gpet_utils.denoise_imgs([np.zeros((10, 40))], "wavelet", dict(wavelet="db8"))


def test_pyramid_layout():
    sp = _lib.wavelet_spec(dict(wavelet="db2"))
    assert sp.pyramid((37, 50)) == ([(20, 26, 0)], 2080)
    assert sp.pyramid((130, 150)) == ([(66, 76, 0), (34, 39, 20064)], 25368)


def test_for_frames_fills_in_what_depends_on_the_frames():
    sp = _lib.wavelet_spec(dict(wavelet="db2", method="VisuShrink"))
    c, keep = sp.for_frames(3, (37, 50))
    assert keep is None and c.c == float(np.sqrt(2 * np.log(37 * 50))) and sp.c.c == 0.0 and c.n_thresholds == 0
    t = np.arange(6, dtype=np.float64).reshape(2, 3)
    sp = _lib.wavelet_spec(dict(wavelet="db2", wavelet_levels=2), thresholds=t)
    c, keep = sp.for_frames(3, (37, 50))
    assert keep.shape == (6, 3) and np.array_equal(keep, np.tile(t, (3, 1))) and c.n_thresholds == 18 and c.thresholds == keep.ctypes.data
    per_frame = np.arange(18, dtype=np.float64).reshape(3, 2, 3)
    c, keep = _lib.wavelet_spec(dict(wavelet="db2", wavelet_levels=2), thresholds=per_frame).for_frames(3, (37, 50))
    assert np.array_equal(keep, per_frame.reshape(6, 3))
    with pytest.raises(ValueError, match="injected thresholds"):
        _lib.wavelet_spec(dict(wavelet="db2"), thresholds=t).for_frames(3, (37, 50))  # (two rows for one level)
    for bad in (np.zeros((2, 2)), np.full((1, 3), np.nan), np.full((1, 3), -1.0), np.zeros(3)):
        with pytest.raises(ValueError, match="injected thresholds"):
            _lib.wavelet_spec(dict(wavelet="db2"), thresholds=bad)


def test_raw_frames_and_resolve_image_source_carry_the_spec_through_the_pre_stage_seam():
    src = gpet.resolve_image_source(1, raw_imgs=FRAME, grad_kernel=K, denoise=("wavelet", dict(wavelet="sym4", sigma=0.1)))
    raw = src["batch"]["raw"]
    assert src["kind"] == "raw" and raw.dn is None and raw.nlm is None and raw.wv is raw.pre and raw.wv.c.n_taps == 8 and raw.wv.c.sigma == 0.1
    assert _lib.RawFrames(K, frames=[FRAME], denoise=raw.wv).wv is raw.wv  # (a spec passes through)
    assert _lib.RawFrames(K, frames=[FRAME], denoise=("median", dict(size=3))).pre is None
    nl = _lib.RawFrames(K, frames=[FRAME], denoise=("nl", dict(fast_mode=False)))
    assert nl.nlm is nl.pre and nl.wv is None
    src = gpet.resolve_image_source(2, raw_device_ptrs=[4096, 8192], raw_dtype=np.float32, grad_shape=(40, 60), grad_kernel=K,
                                    denoise=("wavelet", dict(wavelet="db1")))
    assert src["on_device"] and src["batch"]["raw"].wv is not None
    # frames to denoise only need no kernel
    assert _lib.RawFrames(None, frames=[FRAME], denoise=("wavelet", dict(wavelet="db1"))).kernel is None
