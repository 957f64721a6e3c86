"""What the Python layer of the fast-mode non-local means stage decides without a device: how the kwargs of
gpet_utils.denoise(image, 'nl_fast', kwargs) become a gpet_nlmeans_fast spec, which keys and values are refused (by name), that
'nl' keeps meaning the classic algorithm and only that, and how resolve_image_source / RawFrames carry the spec."""
import numpy as np
import pytest

from gaussian_process_edge_trace_amd import _lib, gpet, gpet_utils

K = np.array([[1.0, 2.0, 1.0], [0.0, 0.0, 0.0], [-1.0, -2.0, -1.0]])
FRAME = np.zeros((8, 9), dtype=np.uint8)


def test_spec_carries_skimages_defaults_and_the_odd_patch():
    for kw in ({}, None, dict(fast_mode=True), dict(fast_mode=1, multichannel=False)):
        sp = _lib.nlmeans_fast_spec(kw)
        assert (sp.c.patch_size, sp.c.patch_distance, sp.c.h, sp.c.sigma, sp.s) == (7, 11, 0.1, 0.0, 7)
    sp = _lib.nlmeans_fast_spec(dict(patch_size=4, patch_distance=2, h=0.3, sigma=0.05, fast_mode=True))
    assert (sp.c.patch_size, sp.c.patch_distance, sp.c.h, sp.c.sigma, sp.s) == (4, 2, 0.3, 0.05, 5)  # an even size is the next odd one
    assert _lib.nlmeans_fast_spec(dict(patch_size=2)).s == 3 and _lib.nlmeans_fast_spec(dict(patch_size=15, patch_distance=31)).s == 15
    assert _lib.nlmeans_fast_spec(dict(patch_distance=0)).c.patch_distance == 0
    assert _lib.NLM_KEYS == ("patch_size", "patch_distance", "h", "sigma", "fast_mode", "multichannel")


@pytest.mark.parametrize("key", ["preserve_range", "size", "mode", "weight", "channel_axis", "sigma_x", "taps"])
def test_other_keys_are_refused_by_name(key):
    with pytest.raises(ValueError, match=key):
        _lib.nlmeans_fast_spec({key: 1})
    with pytest.raises(ValueError, match=key):
        gpet_utils.denoise(FRAME, "nl_fast", {key: 1})  # (refused before a device is looked for)
    with pytest.raises(ValueError, match=key):
        gpet_utils.denoise_imgs([FRAME], "nl_fast", {key: 1})


@pytest.mark.parametrize("kw,name", [(dict(patch_size=1), "patch_size"), (dict(patch_size=0), "patch_size"), (dict(patch_size=16), "patch_size"),
                                     (dict(patch_size=5.5), "patch_size"), (dict(patch_distance=-1), "patch_distance"),
                                     (dict(patch_distance=32), "patch_distance"), (dict(patch_distance=2.5), "patch_distance"),
                                     (dict(h=0.0), "h "), (dict(h=-1.0), "h "), (dict(h=float("nan")), "h "), (dict(h=float("inf")), "h "),
                                     (dict(h=[0.1, 0.2]), "h "), (dict(sigma=-0.1), "sigma"), (dict(sigma=float("nan")), "sigma"),
                                     (dict(sigma=float("inf")), "sigma"), (dict(multichannel=True), "multichannel")])
def test_values_the_device_refuses_are_named(kw, name):
    for call in (lambda: _lib.nlmeans_fast_spec(kw), lambda: gpet_utils.denoise(FRAME, "nl_fast", kw),
                 lambda: gpet.resolve_image_source(1, raw_imgs=FRAME, grad_kernel=K, denoise=("nl_fast", kw))):
        with pytest.raises(ValueError) as e:
            call()
        assert name in str(e.value) and "nl_fast" in str(e.value)


@pytest.mark.parametrize("value", [False, 0])
def test_fast_mode_false_points_to_the_classic_technique(value):
    for call in (lambda: _lib.nlmeans_fast_spec(dict(fast_mode=value)), lambda: gpet_utils.denoise(FRAME, "nl_fast", dict(fast_mode=value))):
        with pytest.raises(ValueError) as e:
            call()
        assert "fast_mode=False" in str(e.value) and "'nl'" in str(e.value)


def test_both_technique_names_resolve_as_described():
    # 'nl' is the classic algorithm and nothing else: without fast_mode=False it raises as it always did, now naming 'nl_fast'
    for kw in ({}, dict(fast_mode=True), dict(patch_size=5)):
        for call in (lambda: _lib.nlmeans_spec(kw), lambda: gpet_utils.denoise(FRAME, "nl", kw), lambda: _lib.RawFrames(K, frames=[FRAME], denoise=("nl", kw))):
            with pytest.raises(NotImplementedError) as e:
                call()
            assert "'nl'" in str(e.value) and "fast_mode=False" in str(e.value) and "'nl_fast'" in str(e.value)
    with pytest.raises(NotImplementedError, match="'nl_fast'"):
        _lib.denoise_spec(("nl", {}))
    with pytest.raises(NotImplementedError, match="nlmeans_fast_spec"):  # (no gpet_denoise technique either: a stage of its own)
        _lib.denoise_spec(("nl_fast", {}))
    assert isinstance(_lib.RawFrames(K, frames=[FRAME], denoise=("nl", dict(fast_mode=False))).pre, _lib.NlmeansSpec)
    assert isinstance(_lib.RawFrames(K, frames=[FRAME], denoise=("nl_fast", {})).pre, _lib.NlmeansFastSpec)
    assert gpet_utils.denoise(FRAME, "bilateral", {}) is None  # (an unknown technique: the reference's message, None)


def test_raw_frames_and_resolve_image_source_carry_the_spec():
    kw = dict(patch_size=5, patch_distance=3, h=0.2)
    src = gpet.resolve_image_source(1, raw_imgs=FRAME, grad_kernel=K, denoise=("nl_fast", kw))
    raw = src["batch"]["raw"]
    assert src["kind"] == "raw" and raw.dn is None and raw.nlf is not None and raw.nlm is None and raw.wv is None and raw.tvb is None
    assert (raw.nlf.c.patch_size, raw.nlf.c.patch_distance, raw.nlf.c.h, raw.nlf.s) == (5, 3, 0.2, 5)
    assert _lib.RawFrames(K, frames=[FRAME], denoise=raw.nlf).nlf is raw.nlf  # (a spec passes through)
    assert _lib.RawFrames(K, frames=[FRAME], denoise=("median", dict(size=3))).nlf is None
    assert _lib.RawFrames(K, frames=[FRAME], denoise=("nl", dict(fast_mode=False))).nlf is None
    assert _lib.RawFrames(None, frames=[FRAME], denoise=("nl_fast", kw)).kernel is None  # (denoising alone)
    src = gpet.resolve_image_source(2, raw_imgs=[FRAME, FRAME], grad_kernel=[K, -K], denoise=("nl_fast", kw), kernel_of=[0, 1, 0, 1], image_of=[0, 0, 1, 1])
    assert src["batch"]["raw"].nlf is not None and src["batch"]["raw"].n_slots == 4
    with pytest.raises(ValueError, match="raw frames"):
        gpet.resolve_image_source(1, grad_imgs=np.zeros((8, 9), np.float32), denoise=("nl_fast", kw))


def test_plan_mirror_on_hand_worked_figures():
    # 20 x 70 at the defaults: pad 15, 50 x 100 padded, 276 shifts in one group; (5000 + 2800 + 276 * 5000) * 8 = 11102400 -> 11102464
    assert _lib.nlmeans_fast_plan(20, 70, 7, 11) == dict(pad=15, nr=50, nc=100, n_shifts=276, rows_per_group=23, n_groups=1, strips=1,
                                                         frame_bytes=11102464, frames_per_chunk=24)
    p = _lib.nlmeans_fast_plan(500, 500, 7, 11)
    assert (p["rows_per_group"], p["n_groups"], p["strips"], p["frame_bytes"], p["frames_per_chunk"]) == (9, 3, 9, 248944896, 1)
    assert _lib.nlmeans_fast_plan(1000, 1000, 15, 31)["rows_per_group"] == 0
