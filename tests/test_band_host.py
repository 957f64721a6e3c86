"""CPU tests of how the band keywords are resolved before anything touches a device (gpet.resolve_image_source, resolve_bands,
resolve_frame_band): every refusal is a ValueError that names its cause, and without band_rows nothing changes."""
import numpy as np
import pytest

from gaussian_process_edge_trace_amd import gpet

M, N, H = 64, 65, 24
INIT_A = np.array([[0, 20], [N - 1, 24]])
INIT_B = np.array([[0, 40], [N - 1, 38]])
FRAME = np.zeros((M, N), dtype=np.uint8)
K = np.ones((3, 3))


def test_band_rows_without_images():
    with pytest.raises(ValueError, match="band_rows needs images"):
        gpet.resolve_image_source(2, band_rows=H, inits=[INIT_A, INIT_B])


def test_band_r0_without_band_rows():
    with pytest.raises(ValueError, match="needs band_rows"):
        gpet.resolve_image_source(2, raw_imgs=FRAME, grad_kernel=K, band_r0=[0, 0])


def test_band_r0_of_the_wrong_length():
    with pytest.raises(ValueError, match="band_r0 has 3 entries for 2 edges"):
        gpet.resolve_image_source(2, raw_imgs=FRAME, grad_kernel=K, band_rows=H, band_r0=[10, 20, 30], inits=[INIT_A, INIT_B])


def test_band_taller_than_the_frame():
    with pytest.raises(ValueError, match=r"H > M"):
        gpet.resolve_image_source(2, raw_imgs=FRAME, grad_kernel=K, band_rows=M + 1, inits=[INIT_A, INIT_B])


def test_inits_that_do_not_fit():
    wide = np.array([[0, 5], [N - 1, 40]])  # 36 rows apart
    with pytest.raises(ValueError, match="band of edge 1: the init rows span more rows"):
        gpet.resolve_image_source(2, raw_imgs=FRAME, grad_kernel=K, band_rows=H, inits=[INIT_A, wide])
    with pytest.raises(ValueError, match="band of edge 0: an init point lies outside its band"):
        gpet.resolve_image_source(2, raw_imgs=FRAME, grad_kernel=K, band_rows=H, band_r0=[22, 30], inits=[INIT_A, INIT_B])
    with pytest.raises(ValueError, match=r"band of edge 1: r0 lies outside \[0, M - H\]"):
        gpet.resolve_image_source(2, raw_imgs=FRAME, grad_kernel=K, band_rows=H, band_r0=[10, M - H + 1], inits=[INIT_A, INIT_B])


def test_band_on_an_unbanded_batch():
    with pytest.raises(ValueError, match="no tracking bands"):
        gpet.resolve_frame_band(None, "follow", 4, 2)
    with pytest.raises(ValueError, match="no tracking bands"):
        gpet.resolve_frame_band(None, [0, 0], None, 2)
    assert gpet.resolve_frame_band(None, None, 4, 2) is None


def test_what_set_frame_does_with_the_bands():
    assert gpet.resolve_frame_band(H, None, 4, 2) == "follow"      # the default with warm_every
    assert gpet.resolve_frame_band(H, None, None, 2) is None        # without: the bands stay
    assert gpet.resolve_frame_band(H, "follow", None, 2) == "follow"
    assert gpet.resolve_frame_band(H, np.array([3, 9]), 4, 2) == [3, 9]
    with pytest.raises(ValueError, match="band has 3 entries for 2 edges"):
        gpet.resolve_frame_band(H, [1, 2, 3], 4, 2)
    with pytest.raises(ValueError, match="'follow'"):
        gpet.resolve_frame_band(H, "track", 4, 2)


def test_without_band_rows_the_dict_is_todays():
    frames = [FRAME, FRAME + 1]
    for kw in (dict(raw_imgs=frames, grad_kernel=K), dict(grad_imgs=[f.astype(np.float32) for f in frames]),
               dict(raw_imgs=FRAME, grad_kernel=K, denoise=("median", dict(size=3)))):
        a = gpet.resolve_image_source(2, **kw)
        b = gpet.resolve_image_source(2, band_rows=None, band_r0=None, inits=None, **kw)
        assert sorted(a) == sorted(b) and "band" not in a and "trace_shape" not in a
        assert a["kind"] == b["kind"] and a["share"] == b["share"] and a["shape"] == b["shape"] == (M, N)


def test_a_banded_source_keeps_the_full_frame_and_traces_the_crop():
    src = gpet.resolve_image_source(2, raw_imgs=[FRAME, FRAME], grad_kernel=K, band_rows=H, band_r0=[10, 30], inits=[INIT_A, INIT_B])
    assert src["shape"] == (M, N) and src["trace_shape"] == (H, N) and src["band"] == (H, [10, 30])
    src = gpet.resolve_image_source(2, grad_imgs=np.zeros((M, N), dtype=np.float32), band_rows=H, inits=[INIT_A, INIT_B])
    assert src["band"] == (H, None) and src["share"]
    # presets that depend on the image height see H, as the cropped oracle does
    p = gpet.resolve_params(INIT_A, src["trace_shape"], kernel_options=(1, 3, 3))
    assert p["sigma_f"] == H // 6 and p["M"] == H
