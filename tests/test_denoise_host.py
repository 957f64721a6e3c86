"""What the Python layer of the denoising stage decides without a device: how (technique, kwargs) of gpet_utils.denoise becomes a
gpet_denoise spec, which keywords and values are refused (by name), which techniques are not built, what an unknown technique
does, and how resolve_image_source / RawFrames carry the spec."""
import numpy as np
import pytest

from gaussian_process_edge_trace_amd import _lib, gpet, gpet_utils

K = np.array([[1.0, 2.0, 1.0], [0.0, 0.0, 0.0], [-1.0, -2.0, -1.0]])
FRAME = np.zeros((8, 9), dtype=np.uint8)


def spec(technique, **kw):
    return _lib.denoise_spec((technique, kw))


def test_specs_carry_scipys_and_skimages_defaults():
    d = spec("median", size=3)
    assert (d.technique, d.size_y, d.size_x, d.mode) == (_lib.DN_MEDIAN, 3, 3, 0)
    d = spec("minimum", size=(4, 3), mode="nearest")
    assert (d.technique, d.size_y, d.size_x, d.mode) == (_lib.DN_MINIMUM, 4, 3, 1)
    d = spec("gaussian", sigma=1.5)
    assert (d.technique, d.sigma_y, d.sigma_x, d.truncate, d.mode) == (_lib.DN_GAUSSIAN, 1.5, 1.5, 4.0, 0)
    d = spec("gaussian", sigma=[2.0, 0.7], truncate=3.0, order=0, mode="reflect")
    assert (d.sigma_y, d.sigma_x, d.truncate) == (2.0, 0.7, 3.0)
    d = spec("tvc")
    assert (d.technique, d.weight, d.eps, d.n_iter_max) == (_lib.DN_TVC, 0.1, 2.0e-4, 200)
    d = spec("tvc", weight=0.3, eps=1e-3, n_iter_max=7)
    assert (d.weight, d.eps, d.n_iter_max) == (0.3, 1e-3, 7)
    assert _lib.denoise_spec(None) is None and _lib.denoise_spec(d) is d


@pytest.mark.parametrize("technique,kw,key", [
    ("median", dict(size=3, footprint=np.ones((3, 3))), "footprint"), ("median", dict(size=3, origin=1), "origin"),
    ("minimum", dict(size=3, cval=0.0), "cval"), ("gaussian", dict(sigma=1.0, cval=1.0), "cval"),
    ("gaussian", dict(sigma=1.0, output=None), "output"), ("tvc", dict(weight=0.1, multichannel=False), "multichannel"),
    ("tvc", dict(size=3), "size"), ("median", dict(size=3, sigma=1.0), "sigma"),
    ("median", dict(size=3, mode="constant"), "mode"), ("gaussian", dict(sigma=1.0, mode="mirror"), "mode"),
    ("minimum", dict(size=3, mode="wrap"), "mode"), ("gaussian", dict(sigma=1.0, order=1), "order"),
    ("gaussian", dict(sigma=1.0, order=(0, 1)), "order")])
def test_unsupported_keywords_are_refused_by_name(technique, kw, key):
    with pytest.raises(ValueError, match=key):
        _lib.denoise_spec((technique, kw))
    with pytest.raises(ValueError, match=key):
        gpet_utils.denoise(FRAME, technique, kw)  # (refused before a device is looked for)


@pytest.mark.parametrize("technique,kw", [
    ("median", {}), ("median", dict(size=0)), ("median", dict(size=(10, 9))), ("minimum", dict(size=(82, 1))), ("median", dict(size=(3, 3, 3))),
    ("gaussian", {}), ("gaussian", dict(sigma=0.0)), ("gaussian", dict(sigma=(1.0, -1.0))), ("gaussian", dict(sigma=1.0, truncate=0.0)),
    ("tvc", dict(weight=0.0)), ("tvc", dict(weight=-1.0)), ("tvc", dict(n_iter_max=0)), ("tvc", dict(eps=-1e-3))])
def test_values_the_device_refuses(technique, kw):
    with pytest.raises(ValueError):
        _lib.denoise_spec((technique, kw))


def test_window_of_81_pixels_is_the_largest():
    assert spec("median", size=9).size_y == 9 and spec("minimum", size=(81, 1)).size_y == 81


@pytest.mark.parametrize("technique", ["nl", "wavelet", "tvb"])
def test_techniques_not_built(technique):
    with pytest.raises(NotImplementedError, match=technique):
        gpet_utils.denoise(FRAME, technique, {})
    with pytest.raises(NotImplementedError, match=technique):
        gpet_utils.denoise_imgs([FRAME], technique, {})
    with pytest.raises(NotImplementedError, match=technique):
        gpet.resolve_image_source(1, raw_imgs=FRAME, grad_kernel=K, denoise=(technique, {}))


def test_unknown_technique_prints_the_references_message_and_returns_none(capsys):
    assert gpet_utils.denoise(FRAME, "bilateral", {}) is None
    assert capsys.readouterr().out == "Denoising technique not implemented.\n"
    with pytest.raises(ValueError, match="bilateral"):
        _lib.denoise_spec(("bilateral", {}))


def test_resolve_image_source_carries_the_spec():
    src = gpet.resolve_image_source(1, raw_imgs=FRAME, grad_kernel=K, denoise=("median", dict(size=3)))
    raw = src["batch"]["raw"]
    assert src["kind"] == "raw" and raw.dn.technique == _lib.DN_MEDIAN and raw.dn.size_x == 3
    assert gpet.resolve_image_source(1, raw_imgs=FRAME, grad_kernel=K)["batch"]["raw"].dn is None
    src = gpet.resolve_image_source(2, raw_device_ptrs=[4096, 8192], raw_dtype=np.float32, grad_shape=(8, 9), grad_kernel=K,
                                    denoise=("tvc", dict(weight=0.2)))
    assert src["on_device"] and src["batch"]["raw"].dn.weight == 0.2


def test_denoise_without_raw_frames_is_refused():
    g = np.zeros((8, 9), dtype=np.float32)
    with pytest.raises(ValueError, match="denoise needs raw frames"):
        gpet.resolve_image_source(1, grad_imgs=g, denoise=("median", dict(size=3)))
    with pytest.raises(ValueError, match="denoise needs raw frames"):
        gpet.resolve_image_source(1, grad_device_ptrs=[4096], grad_shape=(8, 9), denoise=("median", dict(size=3)))
    from gaussian_process_edge_trace_amd.sequence import SequenceTracer
    with pytest.raises(ValueError, match="denoise needs raw frames"):
        SequenceTracer([g, g], np.array([[0, 4], [8, 4]]), denoise=("median", dict(size=3)))


def test_raw_frames_without_kernel_need_a_technique():
    with pytest.raises(ValueError):
        _lib.RawFrames(None, frames=[FRAME])
    raw = _lib.RawFrames(None, frames=[FRAME], denoise=("gaussian", dict(sigma=1.0)))
    assert raw.kernel is None and raw.dn.technique == _lib.DN_GAUSSIAN and raw.pix == _lib.PIX_U8


def test_denoised_dtype():
    for dt, pix in _lib.PIX_OF_DTYPE.items():
        assert _lib.denoised_dtype(spec("median", size=3), pix) == dt
        assert _lib.denoised_dtype(spec("gaussian", sigma=1.0), pix) == dt
        assert _lib.denoised_dtype(spec("tvc"), pix) == np.float64
