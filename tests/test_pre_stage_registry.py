"""The one table of the stages of their own in front of the raw-frame path (_lib.PRE_STAGES) and the protocol its spec classes
share, decided without a device: which techniques there are, that every class names a call the binding declares and the header
has, with the header's flag, what denoise_spec answers for each technique, what the frames' check refuses, and that the names the
table replaced are gone."""
import os
import re

import numpy as np
import pytest

from gaussian_process_edge_trace_amd import _lib, gpet_utils

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpet_hip.h")
# technique -> (spec class, the smallest kwargs from_kwargs accepts, the header's flag, what denoise_spec says: recorded, not derived)
STAGES = {
    "nl": (_lib.NlmeansSpec, dict(fast_mode=False), "GPET_NLM_OUT_ON_DEVICE",
           "denoising technique 'nl' is no gpet_denoise technique: with fast_mode=False it is built as a stage of its own (nlmeans_spec, "
           "Context.nlmeans_images); fast_mode=True is not built under this name: it is the technique 'nl_fast' (nlmeans_fast_spec, "
           "Context.nlmeans_fast_images)"),
    "nl_fast": (_lib.NlmeansFastSpec, {}, "GPET_NLM_OUT_ON_DEVICE",
                "denoising technique 'nl_fast' is no gpet_denoise technique: it is built as a stage of its own (nlmeans_fast_spec, "
                "Context.nlmeans_fast_images)"),
    "wavelet": (_lib.WaveletSpec, dict(wavelet="db1"), "GPET_WV_OUT_ON_DEVICE",
                "denoising technique 'wavelet' is no gpet_denoise technique: it is built as a stage of its own (wavelet_spec, "
                "Context.wavelet_images) and runs when kwargs names the wavelet, e.g. dict(wavelet='db1')"),
    "tvb": (_lib.TvbSpec, dict(weight=5), "GPET_TVB_OUT_ON_DEVICE",
            "denoising technique 'tvb' is no gpet_denoise technique: it is built as a stage of its own (tvb_spec, Context.tvb_images) "
            "and runs when kwargs gives weight, e.g. dict(weight=5)"),
}
CALLS = [(cls, flag) for cls, _, flag, _ in STAGES.values()] + [(_lib.PolarSpec, "GPET_POLAR_OUT_ON_DEVICE")]
RETIRED = ("PRE_STAGE_OF", "PRE_STAGE_BY_NAME", "PRE_SPECS", "PRE_SPEC_TYPES", "DN_NOT_BUILT", "NLF_KEYS", "NlmFrames")


@pytest.fixture(scope="module")
def header():
    with open(HEADER) as f:
        return f.read()


def test_the_table_holds_exactly_the_four_techniques():
    assert list(_lib.PRE_STAGES) == ["nl", "nl_fast", "wavelet", "tvb"] == list(STAGES)
    for technique, (cls, kwargs, _, _) in STAGES.items():
        assert _lib.PRE_STAGES[technique] is cls and cls.technique == technique
        assert type(cls.from_kwargs(kwargs)) is cls
    assert _lib.nlmeans_spec(dict(fast_mode=False)).technique == "nl" and _lib.wavelet_spec(dict(wavelet="db2")).name == "db2"
    assert not hasattr(_lib.PolarSpec, "technique") and not hasattr(_lib.PolarSpec, "from_kwargs") and not hasattr(_lib.PolarSpec, "not_a_filter")


@pytest.mark.parametrize("cls, flag", CALLS, ids=[c.__name__ for c, _ in CALLS])
def test_every_class_names_a_call_of_the_header_with_the_headers_flag(header, cls, flag):
    assert cls.symbol in _lib.SYMBOLS
    assert re.search(r"^int %s\(gpet_ctx\* ctx, " % re.escape(cls.symbol), header, re.M)
    value = re.search(r"^#define %s (\d+)u$" % flag, header, re.M)
    assert value and cls.out_on_device == int(value.group(1))
    assert callable(cls.call_arg)


@pytest.mark.parametrize("technique", list(STAGES))
def test_denoise_spec_answers_a_stage_of_its_own_with_the_recorded_words(technique):
    for kwargs in ({}, STAGES[technique][1]):
        with pytest.raises(NotImplementedError) as e:
            _lib.denoise_spec((technique, kwargs))
        assert str(e.value) == STAGES[technique][3]


def test_an_unknown_technique(capsys):
    with pytest.raises(ValueError, match="unknown denoising technique 'bilateral'"):
        _lib.denoise_spec(("bilateral", {}))
    assert gpet_utils.denoise(np.zeros((8, 9), dtype=np.uint8), "bilateral", {}) is None
    assert capsys.readouterr().out == "Denoising technique not implemented.\n"


def test_the_names_the_table_replaced_are_gone():
    for name in RETIRED:
        assert not hasattr(_lib, name), name
    assert not hasattr(_lib.RawFrames, "nlm_resolved")


def test_check_frames_refuses_what_raw_frames_refused():
    tvb = _lib.tvb_spec(dict(weight=5))
    for shape in ((1, 5), (769, 800)):
        with pytest.raises(ValueError, match="'tvb' takes frames of at least 2 x 2 pixels whose smaller extent is at most 768, not %d x %d" % shape):
            tvb.check_frames(shape)
        with pytest.raises(ValueError, match="not %d x %d" % shape):  # (and RawFrames asks it)
            _lib.RawFrames(None, frames=[np.zeros(shape, dtype=np.uint8)], denoise=tvb)
    tvb.check_frames((2, 2))
    tvb.check_frames((768, 2000))
    with pytest.raises(ValueError, match="max_level is 0"):
        _lib.wavelet_spec(dict(wavelet="db2")).check_frames((2, 2))
    with pytest.raises(ValueError, match="wavelet_levels 5 is above max_level 3"):
        _lib.wavelet_spec(dict(wavelet="db1", wavelet_levels=5)).check_frames((8, 8))
    with pytest.raises(ValueError, match="wavelet_levels 5 is above max_level 3"):
        _lib.RawFrames(None, frames=[np.zeros((8, 8))], denoise=("wavelet", dict(wavelet="db1", wavelet_levels=5)))
    _lib.wavelet_spec(dict(wavelet="db1", wavelet_levels=3)).check_frames((8, 8))
    for spec in (_lib.nlmeans_spec(dict(fast_mode=False)), _lib.nlmeans_fast_spec({})):
        for shape in ((1, 1), (2, 2), (1, 5), (769, 800), (100000, 100000)):
            spec.check_frames(shape)
