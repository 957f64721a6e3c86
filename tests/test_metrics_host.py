"""Host tests of the Python surface of the denoise quality metrics that need no GPU: ``denoise(verbose=True)`` prints exactly the
reference's four lines (gpet_utils.py:151-156) -- ``denoise_imgs`` and ``denoise_metrics`` are monkeypatched --, ``plot`` keeps its
warning, and frames the metrics refuse are refused before a device is needed."""
import warnings

import numpy as np
import pytest

import gaussian_process_edge_trace_amd as pkg

U = pkg.gpet_utils


def fake_metrics(psnr, ssim, nrmse, entropy):
    return dict(psnr=np.array([psnr]), ssim=np.array([ssim]), nrmse=np.array([nrmse]), entropy=np.array([entropy]))


@pytest.mark.parametrize("figs,text", [
    ((20.184321, 0.41449, 0.0979349, 6.46449), "Peak-SNR: 20.18.\nStructural Similarity: 0.41.\nMean Square Error: 0.09793.\nShannon Entropy: 6.464.\n\n"),
    ((float("inf"), 1.0, 0.0, 0.0), "Peak-SNR: inf.\nStructural Similarity: 1.0.\nMean Square Error: 0.0.\nShannon Entropy: 0.0.\n\n"),
    ((7.0, -0.004, 1.5, 13.1), "Peak-SNR: 7.0.\nStructural Similarity: -0.0.\nMean Square Error: 1.5.\nShannon Entropy: 13.1.\n\n"),
])
def test_verbose_prints_the_references_lines(monkeypatch, capsys, figs, text):
    img = np.arange(48, dtype=np.uint8).reshape(6, 8)
    seen = {}

    def fake_denoise_imgs(imgs, technique, kwargs, ctx=None, return_n_iter=False, polar=None, return_metrics=False):
        seen["args"] = (len(imgs), technique, dict(kwargs), return_metrics)
        out = np.stack([np.asarray(f) + 1 for f in imgs])
        return (out, U.denoise_metrics(imgs, out)) if return_metrics else out

    monkeypatch.setattr(U, "denoise_imgs", fake_denoise_imgs)
    monkeypatch.setattr(U, "denoise_metrics", lambda imgs, den, **kw: fake_metrics(*figs))
    # the reference formats round(figure, places) of numpy float64 values: the same text
    ref = (f'Peak-SNR: {round(np.float64(figs[0]), 2)}.\nStructural Similarity: {round(np.float64(figs[1]), 2)}.\n'
           f'Mean Square Error: {round(np.float64(figs[2]), 5)}.\nShannon Entropy: {round(np.float64(figs[3]), 3)}.\n\n')
    assert ref == text
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = U.denoise(img, "median", dict(size=3), verbose=True)
    assert capsys.readouterr().out == text
    assert np.array_equal(out, img + 1) and seen["args"] == (1, "median", dict(size=3), True)
    # without verbose nothing is printed and nothing scored
    out = U.denoise(img, "median", dict(size=3))
    assert capsys.readouterr().out == "" and seen["args"][3] is False and np.array_equal(out, img + 1)
    # plot alone keeps its warning; with verbose the lines are printed as well
    with pytest.warns(UserWarning, match="ignored"):
        U.denoise(img, "median", dict(size=3), plot=True)
    assert capsys.readouterr().out == ""
    with pytest.warns(UserWarning, match="ignored"):
        U.denoise(img, "median", dict(size=3), plot=True, verbose=True)
    assert capsys.readouterr().out == text


def test_an_unknown_technique_still_prints_the_references_message(capsys):
    assert U.denoise(np.zeros((8, 8)), "no_such", {}, verbose=True) is None
    assert capsys.readouterr().out == "Denoising technique not implemented.\n"


def test_refusals_before_a_device_is_needed():
    a = np.zeros((9, 9), dtype=np.float64)
    for key in ("gaussian_weights", "gradient", "multichannel"):
        with pytest.raises(ValueError, match=key):
            U.denoise_metrics([a], [a], **{key: True})
    bad = a.copy()
    bad[3, 3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        U.denoise_metrics([a], [bad])
    with pytest.raises(ValueError, match="NaN"):
        U.denoise_metrics([bad], [a])
    with pytest.raises(ValueError, match="polar"):
        U.denoise_imgs([a], "median", dict(size=3), polar=dict(centre=(4, 4), n_r=4, n_theta=8), return_metrics=True)
