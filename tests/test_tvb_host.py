"""What the Python layer of the split-Bregman stage decides without a device: how the kwargs of gpet_utils.denoise(image, 'tvb',
kwargs) become a gpet_tvb spec, which keys and values are refused (by name), that the stage runs only when kwargs gives
``weight`` (the library's required argument), and how resolve_image_source / RawFrames carry the spec through the pre-stage seam
that non-local means and the wavelet stage use too."""
import numpy as np
import pytest

from gaussian_process_edge_trace_amd import _lib, gpet, gpet_utils

K = np.array([[1.0, 2.0, 1.0], [0.0, 0.0, 0.0], [-1.0, -2.0, -1.0]])
FRAME = np.zeros((40, 60), dtype=np.uint8)


def test_spec_carries_skimages_defaults():
    c = _lib.tvb_spec(dict(weight=5)).c
    assert (c.weight, c.eps, c.max_iter, c.isotropic) == (5.0, 1e-3, 100, 1)
    c = _lib.tvb_spec(dict(weight=0.5, eps=0, max_iter=7, isotropic=False, multichannel=False)).c
    assert (c.weight, c.eps, c.max_iter, c.isotropic) == (0.5, 0.0, 7, 0)
    assert _lib.TVB_KEYS == ("weight", "max_iter", "eps", "isotropic", "multichannel")


@pytest.mark.parametrize("kw", [{}, dict(eps=1e-4), dict(max_iter=10, isotropic=False), None])
def test_without_weight_the_technique_stays_not_built(kw):
    for call in (lambda: _lib.tvb_spec(kw), lambda: gpet_utils.denoise(FRAME, "tvb", kw), lambda: gpet_utils.denoise_imgs([FRAME], "tvb", kw),
                 lambda: gpet.resolve_image_source(1, raw_imgs=FRAME, grad_kernel=K, denoise=("tvb", kw))):
        with pytest.raises(NotImplementedError, match="'tvb'.*weight"):
            call()


def test_denoise_spec_points_to_the_stage():
    for kw in ({}, dict(weight=5)):
        with pytest.raises(NotImplementedError, match="tvb_spec"):
            _lib.denoise_spec(("tvb", kw))


@pytest.mark.parametrize("key", ["n_iter_max", "size", "sigma", "channel_axis", "wavelet", "patch_size"])
def test_other_keys_are_refused_by_name(key):
    with pytest.raises(ValueError, match=key):
        _lib.tvb_spec(dict(weight=5, **{key: 1}))
    with pytest.raises(ValueError, match=key):
        gpet_utils.denoise(FRAME, "tvb", dict(weight=5, **{key: 1}))  # (refused before a device is looked for)


@pytest.mark.parametrize("kw, match", [
    (dict(weight=0), "weight"), (dict(weight=-1.0), "weight"), (dict(weight=float("nan")), "weight"), (dict(weight=float("inf")), "weight"),
    (dict(weight=[1.0, 2.0]), "weight"), (dict(weight=5, eps=-1e-3), "eps"), (dict(weight=5, eps=float("nan")), "eps"),
    (dict(weight=5, max_iter=0), "max_iter"), (dict(weight=5, max_iter=2.5), "max_iter"), (dict(weight=5, multichannel=True), "multichannel")])
def test_values_the_device_refuses(kw, match):
    with pytest.raises(ValueError, match=match):
        _lib.tvb_spec(kw)
    with pytest.raises(ValueError, match=match):
        gpet_utils.denoise(FRAME, "tvb", kw)


def test_frames_the_stage_does_not_take_are_refused_before_a_device_is_needed():
    for shape in ((1, 40), (40, 1), (800, 900)):
        with pytest.raises(ValueError, match="2 x 2"):
            gpet_utils.denoise_imgs([np.zeros(shape)], "tvb", dict(weight=5))
    assert _lib.RawFrames(None, frames=[np.zeros((2, 2))], denoise=("tvb", dict(weight=5))).tvb is not None
    assert _lib.RawFrames(None, frames=[np.zeros((768, 2000), dtype=np.uint8)], denoise=("tvb", dict(weight=5))).tvb is not None


def test_raw_frames_and_resolve_image_source_carry_the_spec_through_the_pre_stage_seam():
    src = gpet.resolve_image_source(1, raw_imgs=FRAME, grad_kernel=K, denoise=("tvb", dict(weight=2, eps=1e-4)))
    raw = src["batch"]["raw"]
    assert src["kind"] == "raw" and raw.dn is None and raw.nlm is None and raw.wv is None and raw.tvb is raw.pre
    assert (raw.tvb.c.weight, raw.tvb.c.eps) == (2.0, 1e-4)
    assert _lib.RawFrames(K, frames=[FRAME], denoise=raw.tvb).tvb is raw.tvb  # (a spec passes through)
    assert _lib.RawFrames(K, frames=[FRAME], denoise=("median", dict(size=3))).tvb is None
    assert _lib.RawFrames(K, frames=[FRAME], denoise=("wavelet", dict(wavelet="db1"))).tvb is None
    src = gpet.resolve_image_source(2, raw_device_ptrs=[4096, 8192], raw_dtype=np.float32, grad_shape=(40, 60), grad_kernel=K,
                                    denoise=("tvb", dict(weight=5)))
    assert src["on_device"] and src["batch"]["raw"].tvb is not None
    # frames to denoise only need no kernel
    assert _lib.RawFrames(None, frames=[FRAME], denoise=("tvb", dict(weight=5))).kernel is None
