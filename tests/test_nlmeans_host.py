"""What the Python layer of the non-local means stage decides without a device: how the kwargs of gpet_utils.denoise(image, 'nl',
kwargs) become a gpet_nlmeans spec, which keys and values are refused (by name), that only fast_mode=False is built, how the
patch weights are derived and how far they may differ from the fixture's, and how resolve_image_source / RawFrames carry the spec."""
import os

import numpy as np
import pytest

from gaussian_process_edge_trace_amd import _lib, gpet, gpet_utils
from tests import nlmeans_ref as R

K = np.array([[1.0, 2.0, 1.0], [0.0, 0.0, 0.0], [-1.0, -2.0, -1.0]])
FRAME = np.zeros((8, 9), dtype=np.uint8)
FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nlmeans.npz"))
SLOW = dict(fast_mode=False)


def test_spec_carries_skimages_defaults_and_the_odd_patch():
    sp = _lib.nlmeans_spec(SLOW)
    assert (sp.c.patch_size, sp.c.patch_distance, sp.c.h, sp.c.sigma, sp.s) == (7, 11, 0.1, 0.0, 7)
    assert sp.taps.shape == (7, 7) and sp.c.taps == sp.taps.ctypes.data
    sp = _lib.nlmeans_spec(dict(patch_size=4, patch_distance=2, h=0.3, sigma=0.05, fast_mode=False, multichannel=False))
    assert (sp.c.patch_size, sp.c.patch_distance, sp.c.h, sp.c.sigma, sp.s) == (4, 2, 0.3, 0.05, 5)
    assert sp.taps.shape == (5, 5)  # an even size is the next odd one
    assert np.array_equal(_lib.nlmeans_spec(dict(patch_size=4, h=0.3, fast_mode=False)).taps, _lib.nlmeans_spec(dict(patch_size=5, h=0.3, fast_mode=False)).taps)
    assert _lib.nlmeans_spec(dict(patch_size=2, fast_mode=False)).s == 3 and _lib.nlmeans_spec(dict(patch_size=15, patch_distance=31, fast_mode=False)).s == 15


@pytest.mark.parametrize("key", ["preserve_range", "size", "mode", "weight", "channel_axis", "sigma_x"])
def test_other_keys_are_refused_by_name(key):
    with pytest.raises(ValueError, match=key):
        _lib.nlmeans_spec(dict(SLOW, **{key: 1}))
    with pytest.raises(ValueError, match=key):
        gpet_utils.denoise(FRAME, "nl", dict(SLOW, **{key: 1}))  # (refused before a device is looked for)


@pytest.mark.parametrize("kw", [{}, dict(fast_mode=True), dict(patch_size=5), dict(fast_mode=1)])
def test_fast_mode_is_not_built_and_the_message_says_what_is(kw):
    for call in (lambda: _lib.nlmeans_spec(kw), lambda: gpet_utils.denoise(FRAME, "nl", kw), lambda: gpet_utils.denoise_imgs([FRAME], "nl", kw),
                 lambda: gpet.resolve_image_source(1, raw_imgs=FRAME, grad_kernel=K, denoise=("nl", kw)),
                 lambda: _lib.denoise_spec(("nl", kw))):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert "'nl'" in str(e.value) and "fast_mode" in str(e.value) and "fast_mode=False" in str(e.value)


@pytest.mark.parametrize("kw", [dict(patch_size=1), dict(patch_size=0), dict(patch_size=16), dict(patch_distance=-1), dict(patch_distance=32),
                                dict(h=0.0), dict(h=-1.0), dict(h=float("nan")), dict(sigma=-0.1), dict(multichannel=True)])
def test_values_the_device_refuses(kw):
    with pytest.raises(ValueError):
        _lib.nlmeans_spec(dict(SLOW, **kw))


def test_injected_taps_override_the_derived_ones():
    t = np.arange(25.0).reshape(5, 5)
    sp = _lib.nlmeans_spec(dict(patch_size=5, fast_mode=False), taps=t)
    assert np.array_equal(sp.taps, t) and sp.taps.flags["C_CONTIGUOUS"] and sp.taps.dtype == np.float64
    with pytest.raises(ValueError, match="taps"):
        _lib.nlmeans_spec(dict(patch_size=5, fast_mode=False), taps=np.zeros((7, 7)))


@pytest.mark.parametrize("key", sorted(k for k in FIX.files if k.startswith("taps_")))
def test_derived_taps_are_within_one_ulp_of_the_fixtures(key):
    """The fixture's taps came from the numpy its generator ran under (texp_s<s>: the s * s exponentials they were made of).
    Where this numpy's exp gives the same s * s values the derived taps must equal the fixture's; in any case every tap is
    held to within one unit in the last place of the fixture's, the bound the issue sets.

    The fixture's generator runs the library with numpy's AVX-512 kernel of exp switched off, so its exponentials are the C
    library's (asserted there): a numpy that has no kernel of its own for these arguments gives the same ones and must give the
    same taps.  Where exp does differ the bound can be missed -- measured with the AVX-512 kernel of numpy 1.26.4 against the C
    library's exponentials: one unit on 4 of 9 (s = 3), 8 of 25 (s = 5) and 4 of 49 (s = 7) arguments, and then up to 4 units per
    tap (s = 3, h = 0.1), 2 (s = 3, h = 6500; s = 7, h = 0.1) and 1 (the other five sets), because the normalising sum moves by a
    unit or two and a unit of an exponential can be two of its tap.  The GPU parity tests inject the fixture's
    taps and do not depend on this."""
    m = key.split("_")
    s, h = int(m[1][1:]), float(m[2][1:])
    fix = FIX[key]
    mine = _lib.nlmeans_taps(s, h)
    assert mine.shape == fix.shape == (s, s) and np.array_equal(mine, _lib.nlmeans_spec(dict(patch_size=s, h=h, fast_mode=False)).taps)
    here, there = np.exp(R.tap_arguments(s)), FIX["texp_s%d" % s]
    exp_ulps = np.abs(here.view(np.int64) - there.view(np.int64))
    tap_ulps = np.abs(mine.view(np.int64) - fix.view(np.int64))
    print("%s: numpy %s against the fixture's (%s): %d of %d exponentials differ (at most %d ulp), taps differ by at most %d ulp"
          % (key, np.__version__, str(FIX["versions"]), int((exp_ulps > 0).sum()), s * s, int(exp_ulps.max()), int(tap_ulps.max())))
    assert exp_ulps.max() <= 1
    if exp_ulps.max() == 0:
        assert np.array_equal(mine, fix)
    assert tap_ulps.max() <= 1


def test_raw_frames_and_resolve_image_source_carry_the_spec():
    kw = dict(patch_size=5, patch_distance=3, h=0.2, fast_mode=False)
    src = gpet.resolve_image_source(1, raw_imgs=FRAME, grad_kernel=K, denoise=("nl", kw))
    raw = src["batch"]["raw"]
    assert src["kind"] == "raw" and raw.dn is None and raw.nlm is not None
    assert (raw.nlm.c.patch_size, raw.nlm.c.patch_distance, raw.nlm.c.h, raw.nlm.s) == (5, 3, 0.2, 5)
    assert _lib.RawFrames(K, frames=[FRAME], denoise=raw.nlm).nlm is raw.nlm  # (a spec passes through)
    assert _lib.RawFrames(K, frames=[FRAME], denoise=("median", dict(size=3))).nlm is None
    assert _lib.RawFrames(None, frames=[FRAME], denoise=("nl", kw)).kernel is None  # (denoising alone)
    src = gpet.resolve_image_source(2, raw_imgs=[FRAME, FRAME], grad_kernel=[K, -K], denoise=("nl", kw), kernel_of=[0, 1, 0, 1], image_of=[0, 0, 1, 1])
    assert src["batch"]["raw"].nlm is not None and src["batch"]["raw"].n_slots == 4
    with pytest.raises(ValueError, match="raw frames"):
        gpet.resolve_image_source(1, grad_imgs=np.zeros((8, 9), np.float32), denoise=("nl", kw))
