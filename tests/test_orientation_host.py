"""CPU tests of vertical edges (``orientation='vertical'``, GPET_FRAMES_TRANSPOSED): the flag between header and Python, the pair of
swap helpers every decoded record goes through, what is refused before a device is needed, the shapes a vertical batch resolves
its parameters for, and the machine code of the transposed-store convolution.  The plan header: tests/test_transpose_plan.py."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_text():
    return open(os.path.join(ROOT, "include", "gpet_hip.h")).read()


# ---- ABI surface ---------------------------------------------------------------------------------------------------------------
def test_flag_agrees_between_header_and_python_and_is_a_free_bit():
    from gaussian_process_edge_trace_amd import _lib
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(GPET_[A-Z_]+)\s+(\d+)u\b", _header_text())}
    assert defs["GPET_FRAMES_TRANSPOSED"] == 16 == _lib.FRAMES_TRANSPOSED
    others = {k: v for k, v in defs.items() if k != "GPET_FRAMES_TRANSPOSED"}
    assert {"GPET_GRAD_ON_DEVICE", "GPET_IMAGES_NEXT_FRAME", "GPET_RAW_ON_DEVICE", "GPET_NLM_OUT_ON_DEVICE"} <= set(others)
    assert all(v & 16 == 0 for v in others.values()), others
    assert "#define GPET_ABI_VERSION 1\n" in _header_text()   # (the surface only grew: one flag bit, no new export)


def test_no_new_export():
    from gaussian_process_edge_trace_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    declared = set(re.findall(r"\b(gpet_[a-z0-9_]+)\s*\(", text))
    assert not [n for n in declared | set(_lib.SYMBOLS) if "transpos" in n or "orient" in n or "vertical" in n]


def test_keyword_is_on_every_layer():
    import gaussian_process_edge_trace_amd as pkg
    assert inspect.signature(pkg.GP_Edge_Tracing_Batch.__init__).parameters["orientation"].default == "horizontal"
    assert inspect.signature(pkg.SequenceTracer.__init__).parameters["orientation"].default == "horizontal"
    assert inspect.signature(pkg.gpet_utils.comp_grad_imgs).parameters["transpose"].default is False
    assert inspect.signature(pkg._lib.Batch.__init__).parameters["transposed"].default is False
    assert inspect.signature(pkg._lib.Context.grad_images).parameters["transpose"].default is False
    assert "orientation" not in inspect.signature(pkg.GP_Edge_Tracing.__init__).parameters   # (the single edge: grad.T on the host)


# ---- the swap helpers ------------------------------------------------------------------------------------------------------------
def test_swap_xy_round_trips_points():
    from gaussian_process_edge_trace_amd.gpet import swap_xy
    pts = np.array([[3, 40], [9, 41], [27, 39]], dtype=np.int64)
    got = swap_xy(pts)
    assert got.dtype == pts.dtype and got.flags["C_CONTIGUOUS"] and np.array_equal(got, [[40, 3], [41, 9], [39, 27]])
    assert np.array_equal(swap_xy(got), pts) and not np.shares_memory(got, pts)
    curves = np.arange(24, dtype=np.float64).reshape(3, 4, 2)                  # (a stack of curves: the last axis is the point)
    assert np.array_equal(swap_xy(curves), curves[..., ::-1]) and np.array_equal(swap_xy(swap_xy(curves)), curves)
    lst = [pts, pts[:1], np.zeros((0, 2), dtype=np.int64)]                     # (one array per edge, an empty observation set)
    back = swap_xy(swap_xy(lst))
    assert isinstance(back, list) and all(np.array_equal(a, b) and a.shape == b.shape for a, b in zip(back, lst))
    assert swap_xy(np.array([])).size == 0
    with pytest.raises(ValueError):
        swap_xy(np.zeros((4, 3)))


def test_swap_record_round_trips_intervals_and_the_ensemble_dict():
    from gaussian_process_edge_trace_amd.gpet import swap_record
    rows = np.arange(10, 15)
    ens = dict(trace=np.stack([np.array([7, 8, 8, 9, 9]), rows], -1), median=np.array([7.2, 7.9, 8.1, 8.8, 9.3]),
               q_lo=np.full(5, 7.0), q_hi=np.full(5, 9.5), min=np.full(5, 6.0), max=np.full(5, 10.0), agree=np.full(5, 3),
               members=np.array([0, 1, 2]), off=np.array([0, 1, 0]), cost=np.array([1.0, 2.0, 3.0]), medoid=0, best_cost=0)
    got = swap_record(ens, ("trace",))
    assert np.array_equal(got["trace"], np.stack([rows, ens["trace"][:, 0]], -1))      # (frame row, frame column)
    for k in ens:
        if k != "trace":                                                              # positions, counts, costs: as they are
            assert got[k] is ens[k], k
    back = swap_record(got, ("trace",))
    assert set(back) == set(ens) and all(np.array_equal(back[k], ens[k]) for k in ens)
    # an interval is a pair of position vectors: frame columns indexed by frame row, whatever the orientation
    rec = dict(trace=np.zeros((2, 5, 2), dtype=np.int64), lower=np.ones((2, 5)), upper=2 * np.ones((2, 5)), edge_len=np.array([5, 5]))
    got = swap_record(rec, ("trace",))
    assert got["lower"] is rec["lower"] and got["upper"] is rec["upper"] and got["trace"].shape == (2, 5, 2)
    # a history: lists of per-iteration arrays; a missing level stays missing
    hist = dict(obs=[np.array([[1, 2]]), np.array([[1, 2], [3, 4]])], score_thresh=np.array([1.0, 0.9]), mean=np.ones((2, 5)))
    got = swap_record(hist, ("obs", "optimal_curves"))
    assert np.array_equal(got["obs"][1], [[2, 1], [4, 3]]) and "optimal_curves" not in got and got["mean"] is hist["mean"]
    assert all(np.array_equal(a, b) for a, b in zip(swap_record(got, ("obs", "optimal_curves"))["obs"], hist["obs"]))


# ---- refusals that need no device ----------------------------------------------------------------------------------------------
def test_two_init_points_in_one_row_are_refused():
    import gaussian_process_edge_trace_amd as pkg
    from gaussian_process_edge_trace_amd.gpet import vertical_inits
    ok = np.array([[40, 0], [42, 159]])
    assert np.array_equal(vertical_inits([ok])[0], [[0, 40], [159, 42]])
    bad = np.array([[40, 7], [42, 100], [50, 7]])
    with pytest.raises(ValueError, match="same row"):
        vertical_inits([ok, bad])
    frame = np.zeros((160, 96), dtype=np.uint8)
    K = pkg.gpet_utils.kernel_builder((11, 5), vertical_edges=True)
    with pytest.raises(ValueError, match="same row"):
        pkg.GP_Edge_Tracing_Batch([bad], None, [1], raw_imgs=frame, grad_kernel=K, orientation="vertical")
    with pytest.raises(ValueError, match="same row"):
        pkg.SequenceTracer([frame, frame], bad, grad_kernel=K, orientation="vertical")
    with pytest.raises(ValueError, match="same row"):
        pkg.trace_ensemble(bad, None, [1, 2], raw_imgs=frame, grad_kernel=K, orientation="vertical")


def test_unknown_orientation_is_refused():
    import gaussian_process_edge_trace_amd as pkg
    from gaussian_process_edge_trace_amd.gpet import resolve_orientation
    assert resolve_orientation("horizontal") is False and resolve_orientation("vertical") is True
    init = np.array([[40, 0], [42, 159]])
    frame = np.zeros((160, 96), dtype=np.uint8)
    K = pkg.gpet_utils.kernel_builder((11, 5), vertical_edges=True)
    for bad in ("diagonal", "Vertical", None, True, 1):
        with pytest.raises(ValueError, match="orientation"):
            resolve_orientation(bad)
        with pytest.raises(ValueError, match="orientation"):
            pkg.GP_Edge_Tracing_Batch([init], None, [1], raw_imgs=frame, grad_kernel=K, orientation=bad)
        with pytest.raises(ValueError, match="orientation"):
            pkg.SequenceTracer([frame], init, grad_kernel=K, orientation=bad)
        with pytest.raises(ValueError, match="orientation"):
            pkg.trace_ensemble(init, None, [1, 2], raw_imgs=frame, grad_kernel=K, orientation=bad)


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
def test_presets_see_the_transposed_image():
    """``kernel_options=(1, 3, 3)`` on a 160 x 96 frame: sigma_f = height // 6 and length_scale = edge length // 2 of the 96 x 160
    image the batch traces -- 16 and 80 -- not the frame's 26 and 48."""
    from gaussian_process_edge_trace_amd.gpet import resolve_image_source, resolve_params, vertical_inits
    K = np.ones((5, 11))
    frame = np.zeros((160, 96), dtype=np.uint8)
    init = np.array([[40, 0], [42, 159]])                       # (x, y) of the frame: rows 0 .. 159
    src = resolve_image_source(1, raw_imgs=frame, grad_kernel=K, transposed=True)
    assert src["shape"] == (160, 96) and src["trace_shape"] == (96, 160) and src["kind"] == "raw"
    p = resolve_params(vertical_inits([init])[0], src["trace_shape"], (1, 3, 3))
    assert (p["M"], p["N"], p["x_st"], p["x_en"], p["edge_length"]) == (96, 160, 0, 159, 160)
    assert (p["sigma_f"], p["sigma_l"]) == (96 // 6, 160 // 2) == (16, 80)
    q = resolve_params(init[:, ::-1], (96, 160), (1, 3, 3))     # what the transposed call of a reference user sees
    assert all(np.array_equal(p[k], q[k]) for k in p if k not in ("obs",))
    h = resolve_params(np.array([[0, 40], [95, 42]]), (160, 96), (1, 3, 3))
    assert (h["sigma_f"], h["sigma_l"]) == (26, 48)
    # a shorter edge: the row span counts
    p = resolve_params(vertical_inits([np.array([[40, 20], [42, 119]])])[0], src["trace_shape"], (1, 3, 3))
    assert (p["edge_length"], p["sigma_l"]) == (100, 50)
    # caller-given gradient images are in the frame's layout too
    g = resolve_image_source(1, grad_imgs=np.zeros((160, 96), np.float32), transposed=True)
    assert g["shape"] == (160, 96) and g["trace_shape"] == (96, 160) and g["kind"] == "grad"
    g = resolve_image_source(1, grad_device_ptrs=[4096], grad_shape=(160, 96), transposed=True)
    assert g["shape"] == (160, 96) and g["trace_shape"] == (96, 160)
    # the horizontal dict is what it was
    assert "trace_shape" not in resolve_image_source(1, raw_imgs=frame, grad_kernel=K)


def test_bands_of_a_vertical_batch_are_frame_columns():
    from gaussian_process_edge_trace_amd.gpet import resolve_image_source, vertical_inits
    K = np.ones((5, 11))
    frame = np.zeros((160, 96), dtype=np.uint8)
    inits = vertical_inits([np.array([[40, 0], [42, 159]])])
    src = resolve_image_source(1, raw_imgs=frame, grad_kernel=K, band_rows=48, inits=inits, transposed=True)
    assert src["band"] == (48, None) and src["trace_shape"] == (48, 160) and src["shape"] == (160, 96)
    src = resolve_image_source(1, raw_imgs=frame, grad_kernel=K, band_rows=48, band_r0=[20], inits=inits, transposed=True)
    assert src["band"] == (48, [20])
    with pytest.raises(ValueError, match="band of edge 0"):      # 97 columns of a frame 96 wide
        resolve_image_source(1, raw_imgs=frame, grad_kernel=K, band_rows=97, inits=inits, transposed=True)
    with pytest.raises(ValueError, match="band of edge 0"):      # init columns 10 and 90 do not fit 48 columns
        resolve_image_source(1, raw_imgs=frame, grad_kernel=K, band_rows=48, inits=vertical_inits([np.array([[10, 0], [90, 159]])]),
                             transposed=True)
    with pytest.raises(ValueError, match="band of edge 0"):      # a band that starts at column 60 does not hold column 40
        resolve_image_source(1, raw_imgs=frame, grad_kernel=K, band_rows=30, band_r0=[60], inits=inits, transposed=True)
    with pytest.raises(ValueError, match="band_rows"):
        resolve_image_source(1, raw_imgs=frame, grad_kernel=K, band_r0=[3], transposed=True)


# ---- machine code ----------------------------------------------------------------------------------------------------------------
def _code_objects(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("no llvm-objdump")
    so = tmp_path / "lib.so"
    shutil.copy(ge.LIB, so)
    subprocess.run([objdump, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    return objdump, [str(tmp_path / f) for f in sorted(os.listdir(tmp_path)) if "amdgcn" in f]


def test_transposed_store_convolution_has_no_fused_multiply_add_and_no_scratch(tmp_path):
    """The bits of a pixel are those of the horizontal kernels only if every product is rounded before it is added: no v_fma_f64 /
    v_fmac_f64 in any instantiation of k_conv_tr_batch / k_conv_tr_multi, four pixel types each; and nothing spilled."""
    objdump, objs = _code_objects(tmp_path)
    bodies = {}
    for f in objs:
        text = subprocess.run([objdump, "-d", f], check=True, capture_output=True, text=True).stdout
        for m in re.finditer(r"^[0-9a-f]+ <(\S*k_conv_tr_\S*)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", text, flags=re.S | re.M):
            bodies[m.group(1)] = m.group(2)
    for stem in ("k_conv_tr_batch", "k_conv_tr_multi"):
        for tag in ("Ih", "It", "If", "Id"):  # uint8_t, uint16_t, float, double
            assert any(stem + tag in n for n in bodies), (stem, tag, sorted(bodies))
    assert len(bodies) == 8, sorted(bodies)
    for name, body in bodies.items():
        assert "v_mul_f64" in body and "v_add_f64" in body, name
        assert not re.search(r"v_fmac?_f64", body), name
        assert "scratch_" not in body, name
