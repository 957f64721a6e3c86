"""GPU tests of the denoise quality metrics (gpet_metrics_images, gpet_utils.denoise_metrics, denoise_imgs(return_metrics=True),
denoise(verbose=True)) against tests/golden/denoise_metrics.npz, what scikit-image 0.18.3 computes: the SSIM map bit for bit, the four
figures within the bounds of DESIGN.md section 9 (tests/metrics_ref.py: bounds), from host frames and from frames on the device, alone
and in a stack of three different pairs."""
import json
import os

import numpy as np
import pytest

from tests import metrics_ref as R
from tests.test_gpu_denoise import DeviceFrames
from tests.test_metrics_fixture import CASES, FIGS, FIX, case_bounds

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def stack_of(a):
    """Three different frames of a's shape and dtype: a itself, a rolled by one row and three columns, a upside down."""
    return np.stack([a, np.roll(a, (1, 3), axis=(0, 1)), a[::-1]])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_figures_and_map_against_the_library(amd, ctx, case):
    name, kw = case["name"], case["kwargs"]
    a, b, lib, S = FIX["a_" + name], FIX["b_" + name], FIX["lib_" + name], FIX["map_" + name]
    bd, ref = case_bounds(case), R.figures(a, b, **kw)
    one = amd.gpet_utils.denoise_metrics([a], [b], full=True, ctx=ctx, **kw)
    assert one["ssim_map"].shape == (1,) + a.shape and np.array_equal(one["ssim_map"][0], S)
    for j, fig in enumerate(FIGS):
        print(name, fig, one[fig][0], lib[j], ref[fig], bd[fig])
        assert one[fig].shape == (1,) and one[fig].dtype == np.float64
        assert R.within(float(one[fig][0]), float(lib[j]), bd[fig]), (fig, one[fig][0], lib[j], bd[fig])
    # the counts are exact: the entropy agrees with the restatement's, whose counts are numpy's, within the bound as well
    assert R.within(float(one["entropy"][0]), ref["entropy"], bd["entropy"])
    # a stack of three different pairs, from the host and from the device: every pair's result is its single-pair result
    sa, sb = stack_of(a), stack_of(b)
    singles = [one] + [amd.gpet_utils.denoise_metrics([sa[t]], [sb[t]], full=True, ctx=ctx, **kw) for t in (1, 2)]
    host = amd.gpet_utils.denoise_metrics(sa, sb, full=True, ctx=ctx, **kw)
    L = amd._lib
    da, db = DeviceFrames(ctx, sa), DeviceFrames(ctx, sb)
    try:
        fig, maps = ctx.metrics_images(L.metrics_frames(device_ptrs=da.ptrs, dtype=sa.dtype, shape=a.shape),
                                       L.metrics_frames(device_ptrs=db.ptrs, dtype=sb.dtype, shape=a.shape),
                                       L.metrics_spec(kw.get("win_size", 7), kw.get("data_range"), **{k: v for k, v in kw.items()
                                                                                                    if k not in ("win_size", "data_range")}), full=True)
        one_dev = ctx.metrics_images(L.metrics_frames(device_ptrs=da.ptrs[:1], dtype=sa.dtype, shape=a.shape),
                                     L.metrics_frames(device_ptrs=db.ptrs[:1], dtype=sb.dtype, shape=a.shape),
                                     L.metrics_spec(kw.get("win_size", 7), kw.get("data_range"), **{k: v for k, v in kw.items()
                                                                                                  if k not in ("win_size", "data_range")}), full=True)
    finally:
        da.free()
        db.free()
    assert np.array_equal(one_dev[1][0], S) and np.array_equal(one_dev[0][0], np.array([one[f][0] for f in FIGS]), equal_nan=True)
    for t in range(3):
        assert np.array_equal(host["ssim_map"][t], singles[t]["ssim_map"][0]) and np.array_equal(maps[t], singles[t]["ssim_map"][0])
        for j, f in enumerate(FIGS):
            assert np.array_equal(host[f][t], singles[t][f][0], equal_nan=True), (t, f)
            assert np.array_equal(fig[t, j], singles[t][f][0], equal_nan=True), (t, f)
    assert np.array_equal(host["ssim_map"][0], S)
    # without full there is no map, and the figures are the same
    plain = amd.gpet_utils.denoise_metrics(sa, sb, ctx=ctx, **kw)
    assert set(plain) == set(FIGS) and all(np.array_equal(plain[f], host[f], equal_nan=True) for f in FIGS)


@pytest.mark.parametrize("technique,kwargs,dt", [("median", dict(size=3), np.uint8), ("tvb", dict(weight=2.0, max_iter=12), np.float64)])
def test_return_metrics_equals_scoring_the_result(amd, ctx, technique, kwargs, dt):
    a = FIX["a_mid_u8"] if dt == np.uint8 else FIX["a_mid_f64"]
    stack = stack_of(a)
    out, m = amd.gpet_utils.denoise_imgs(stack, technique, kwargs, ctx=ctx, return_metrics=True)
    plain = amd.gpet_utils.denoise_imgs(stack, technique, kwargs, ctx=ctx)
    assert out.dtype == plain.dtype and np.array_equal(out, plain)
    want = amd.gpet_utils.denoise_metrics(stack, plain, ctx=ctx)
    assert set(m) == set(FIGS)
    for f in FIGS:
        assert m[f].shape == (3,) and np.array_equal(m[f], want[f]), f
    out2, n_iter, m2 = amd.gpet_utils.denoise_imgs(stack, technique, kwargs, ctx=ctx, return_n_iter=True, return_metrics=True)
    assert np.array_equal(out2, plain) and n_iter.shape == (3,) and all(np.array_equal(m2[f], want[f]) for f in FIGS)


def test_verbose_prints_what_the_reference_prints(amd, ctx, capsys):
    spec = json.loads(str(FIX["print_kwargs"]))
    out = amd.gpet_utils.denoise(FIX["a_print_u8"], spec["technique"], spec["kwargs"], verbose=True, ctx=ctx)
    assert capsys.readouterr().out == str(FIX["print_text"])
    assert np.array_equal(out, FIX["b_print_u8"])


def test_refusals(amd, ctx):
    import ctypes as C
    L = amd._lib
    a = FIX["a_one_window_f64"]
    with pytest.raises(ValueError, match="win_size exceeds image extent"):
        amd.gpet_utils.denoise_metrics([a], [a], win_size=9, ctx=ctx)
    with pytest.raises(ValueError, match="Window size must be odd"):
        amd.gpet_utils.denoise_metrics([a], [a], win_size=4, ctx=ctx)
    with pytest.raises(ValueError, match="gaussian_weights"):
        amd.gpet_utils.denoise_metrics([a], [a], gaussian_weights=True, ctx=ctx)
    with pytest.raises(ValueError, match="same dimensions"):
        amd.gpet_utils.denoise_metrics([a], [a[:, :5]], ctx=ctx)
    # the library itself refuses what the binding would: the C call, in the header's words, with nothing launched
    fa, spec, out = L.metrics_frames(frames=[a]), L.metrics_spec(9), np.full(4, -1.0)
    P = (C.c_void_p * 1)(*fa.ptrs)
    rc = ctx.lib.gpet_metrics_images(ctx.h, P, fa.pix, P, fa.pix, 1, 7, 7, C.byref(spec), 0, out.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert rc == L.ERR_BAD_ARG and ctx.lib.gpet_last_error(ctx.h).decode() == R.EXTENT_WORDS and np.all(out == -1.0)
    rc = ctx.lib.gpet_metrics_images(ctx.h, P, fa.pix, P, fa.pix, 1, 7, 7, C.byref(L.metrics_spec(7)), 128, out.ctypes.data_as(C.POINTER(C.c_double)), None)
    assert rc == L.ERR_BAD_ARG and "unknown flag bits" in ctx.lib.gpet_last_error(ctx.h).decode()
    # a float frame outside [-1, 1]: the library's ValueError, which data_range lifts
    big = FIX["a_mid_f64"] * 3.0
    with pytest.raises(ValueError, match="im_true has intensity values outside the range expected for its data type"):
        amd.gpet_utils.denoise_metrics([big], [FIX["b_mid_f64"]], ctx=ctx)
    m = amd.gpet_utils.denoise_metrics([big], [FIX["b_mid_f64"]], data_range=3.0, ctx=ctx)
    ref = R.figures(big, FIX["b_mid_f64"], data_range=3.0)
    crop = ref["ssim_map"][3:-3, 3:-3]
    bd = R.bounds(big.size, crop.size, float(np.abs(crop).mean()), len(ref["counts"]), ref["psnr"], ref["nrmse"], ref["entropy"])
    assert all(R.within(float(m[f][0]), ref[f], bd[f]) for f in FIGS)
