"""CPU tests of the host side of the polar unwrap: polar_spec's defaults and refusals (no device), closed_init, polar_to_xy, and the
restated rule (tests/polar_ref.py) checked against an independent interpolator, scipy's map_coordinates, and for its seam identities."""
import numpy as np
import pytest

from tests import polar_ref as R

DTYPES = (np.uint8, np.uint16, np.float32, np.float64)


def test_polar_spec_defaults_and_shape():
    from gaussian_process_edge_trace_amd import _lib, gpet_utils as U
    sp = _lib.polar_spec(dict(centre=(10.5, 7.25), n_r=30, n_theta=90))
    assert (sp.r0, sp.dr, sp.theta0, sp.pad) == (0.0, 1.0, 0.0, None)
    assert sp.centre.shape == (1, 2) and sp.centre.dtype == np.float64 and sp.centre.tolist() == [[10.5, 7.25]]
    assert _lib.polar_spec(sp) is sp
    # pad=None: half the width of the widest gradient kernel, 0 where there is none
    K53, K37 = U.kernel_builder((5, 3)), U.kernel_builder((3, 7))
    frames = np.zeros((2, 12, 14), dtype=np.uint8)
    pol = dict(centre=(6, 5), n_r=6, n_theta=16)
    assert _lib.RawFrames(K53, frames=frames, polar=pol).polar.pad == 1
    assert _lib.RawFrames([K53, K37], frames=frames, polar=pol, slots=([0, 0, 1, 1], [0, 1, 0, 1])).polar.pad == 3
    assert _lib.RawFrames(None, frames=frames, polar=pol).polar.pad == 0
    assert _lib.RawFrames(None, frames=frames, polar=pol, denoise=("median", dict(size=3))).polar.pad == 0
    raw = _lib.RawFrames(K53, frames=frames, polar=dict(pol, pad=4))
    assert raw.polar.pad == 4 and raw.shape == (6, 16 + 1 + 8) and raw.src_shape == (12, 14) and raw.polar.shape == raw.shape
    assert raw.needs_resolve and not _lib.RawFrames(K53, frames=frames).needs_resolve
    assert _lib.RawFrames(K53, frames=frames).src_shape == (12, 14) and _lib.RawFrames(K53, frames=frames).polar is None
    # per-frame centres
    raw = _lib.RawFrames(K53, frames=frames, polar=dict(pol, centre=[(6, 5), (7.5, 4)]))
    assert raw.polar.centre.shape == (2, 2) and raw.polar.with_centre((7.5, 4)).centre.tolist() == [[7.5, 4.0]]
    # the tables are numpy's own
    c, s = R.tables(16, 0.25)
    sp = _lib.polar_spec(dict(pol, theta0=0.25))
    assert np.array_equal(sp.cos_t, c) and np.array_equal(sp.sin_t, s)
    assert np.array_equal(c, np.cos(0.25 + 2.0 * np.pi * np.arange(16) / 16.0))


def test_polar_spec_refusals_need_no_device():
    from gaussian_process_edge_trace_amd import _lib, gpet_utils as U
    ok = dict(centre=(10.0, 7.0), n_r=30, n_theta=90)
    bad = [(dict(n_r=0), "n_r must be at least 1"), (dict(n_theta=3), "n_theta must be at least 4"), (dict(pad=-1), "pad must lie in [0, n_theta]"),
           (dict(pad=91), "pad must lie in [0, n_theta]"), (dict(r0=-1.0), "r0 must be finite and at least 0"),
           (dict(dr=0.0), "dr must be finite and above 0"), (dict(dr=float("nan")), "dr must be finite"),
           (dict(centre=(1.0, float("inf"))), "a centre is not finite"), (dict(centre=(1.0, 2.0, 3.0)), "centre must be"),
           (dict(n_r=2.5), "a whole number"), (dict(theta0=float("nan")), "theta0 must be finite"), (dict(radius=3), "unknown key 'radius'"),
           (dict(n_r=1 << 20, n_theta=1 << 20), "exceeds 2^28"), (dict(n_theta=None), "n_theta is required")]
    for change, words in bad:
        with pytest.raises(ValueError, match=words.replace("[", r"\[").replace("]", r"\]").replace("^", r"\^")):
            _lib.polar_spec(dict(ok, **change))
    with pytest.raises(ValueError, match="centre is required"):
        _lib.polar_spec(dict(n_r=3, n_theta=8))
    with pytest.raises(ValueError, match="must be a dict"):
        _lib.polar_spec([1, 2, 3])
    K = U.kernel_builder((5, 3))
    # what depends on the frames is refused when they are seen, still without a device
    with pytest.raises(ValueError, match="at least 2 x 2"):
        _lib.RawFrames(K, frames=np.zeros((1, 1, 9)), polar=ok)
    with pytest.raises(ValueError, match="one centre for all frames or one per frame"):
        _lib.RawFrames(K, frames=np.zeros((3, 9, 9)), polar=dict(ok, centre=[(1, 1), (2, 2)]))
    with pytest.raises(ValueError, match="pad must lie in"):  # (the default pad of a kernel wider than 2 n_theta + 1)
        _lib.RawFrames(np.ones((3, 11)), frames=np.zeros((1, 9, 9)), polar=dict(ok, n_theta=4))
    # polar needs raw frames, and is no vertical batch
    from gaussian_process_edge_trace_amd import gpet
    with pytest.raises(ValueError, match="polar needs raw frames"):
        gpet.resolve_image_source(1, grad_imgs=np.zeros((9, 9), dtype=np.float32), polar=ok)
    with pytest.raises(ValueError, match="orientation='vertical'"):
        gpet.resolve_image_source(1, raw_imgs=np.zeros((9, 9)), grad_kernel=K, polar=ok, transposed=True)
    with pytest.raises(ValueError, match="polar and transpose"):
        U.comp_grad_imgs(np.zeros((1, 9, 9)), K, polar=ok, transpose=True)
    src = gpet.resolve_image_source(1, raw_imgs=np.zeros((9, 12), dtype=np.uint8), grad_kernel=K, polar=ok)
    assert src["shape"] == (30, 93) and src["src_shape"] == (9, 12)


def test_closed_init():
    from gaussian_process_edge_trace_amd import _lib, gpet_utils as U
    pol = dict(centre=(10, 7), n_r=30, n_theta=90, pad=2)
    got = U.closed_init(17, pol)
    assert got.dtype == np.int64 and got.tolist() == [[2, 17], [92, 17]]
    assert U.closed_init(0, dict(pol, pad=0)).tolist() == [[0, 0], [90, 0]]
    raw = _lib.RawFrames(U.kernel_builder((5, 7)), frames=np.zeros((1, 20, 20)), polar=dict(centre=(10, 7), n_r=30, n_theta=90))
    assert U.closed_init(5, raw.polar).tolist() == [[3, 5], [93, 5]]
    with pytest.raises(ValueError, match="needs pad"):
        U.closed_init(5, dict(centre=(10, 7), n_r=30, n_theta=90))


def test_polar_to_xy_is_the_rules_arithmetic():
    from gaussian_process_edge_trace_amd import gpet_utils as U
    shape, n_r, n_theta, pad = (37, 53), 40, 48, 5
    centres = [(46.3, 4.6), (20.25, 17.5)]
    pol = dict(centre=centres, n_r=n_r, n_theta=n_theta, r0=1.5, dr=0.75, theta0=0.2, pad=pad)
    W = R.width(n_theta, pad)
    rows, cols = np.meshgrid(np.arange(n_r), np.arange(W), indexing="ij")
    for t in range(2):
        rx, ry = R.positions(shape, centres[t], n_r, n_theta, 1.5, 0.75, 0.2, pad)
        x, y = U.polar_to_xy(rows, cols, pol, frame=t, shape=shape)
        assert x.dtype == np.float64 and np.array_equal(x, rx) and np.array_equal(y, ry)
        ux, uy = U.polar_to_xy(rows, cols, pol, frame=t)  # (unclamped: the same wherever the ray is inside)
        inside = (ux >= 0) & (ux <= shape[1] - 1) & (uy >= 0) & (uy <= shape[0] - 1)
        assert inside.any() and not inside.all()
        assert np.array_equal(ux[inside], rx[inside]) and np.array_equal(uy[inside], ry[inside])
    # a trace and its intervals: first and last column of a closed trace are one ray, so equal rows give equal points to the bit
    trace = np.stack([np.full(n_theta + 1, 7), np.arange(pad, pad + n_theta + 1)], axis=1)
    xy = U.polar_trace_xy(trace, pol, frame=1)
    assert xy.shape == (n_theta + 1, 2) and np.array_equal(xy[0], xy[-1])
    lower, upper = trace[:, 0] - 1.25, trace[:, 0] + 2.5
    xy2, (lo, hi) = U.polar_trace_xy((trace, (lower, upper)), pol, frame=1)
    assert np.array_equal(xy2, xy) and lo.shape == hi.shape == xy.shape
    ex, ey = U.polar_to_xy(lower, trace[:, 1], pol, frame=1)
    assert np.array_equal(lo[:, 0], ex) and np.array_equal(lo[:, 1], ey)
    assert np.all(np.hypot(lo[:, 0] - 20.25, lo[:, 1] - 17.5) < np.hypot(hi[:, 0] - 20.25, hi[:, 1] - 17.5))


@pytest.mark.parametrize("dtype", DTYPES)
def test_restated_rule_against_map_coordinates(dtype):
    """The independent check: scipy's bilinear interpolation (order=1, mode='nearest') on the rule's clamped coordinates.  scipy adds
    the four weighted taps in another order, so the two differ by a few roundings of a convex combination of the pixels: the bound is
    8 * 2^-53 * max|pixel| (measured when this test was written: at most 2.01 such units)."""
    from scipy.ndimage import map_coordinates
    shape, centre, n_r, n_theta, r0, dr, theta0, pad = (37, 53), (46.3, 4.6), 40, 48, 0.0, 0.75, 0.0, 5
    frame = R.frame_of(dtype, shape, 21)
    x, y = R.positions(shape, centre, n_r, n_theta, r0, dr, theta0, pad)
    assert (x == 52).any() and (y == 0).any()  # rays leave on two sides
    ref = R.unwrap([frame], centre, n_r, n_theta, r0, dr, theta0, pad)[0]
    sci = map_coordinates(frame.astype(np.float64), [y, x], order=1, mode="nearest")
    unit = 2.0 ** -53 * float(np.abs(frame.astype(np.float64)).max())
    err = np.abs(ref - sci).max()
    print("dtype %s: max |polar_ref - map_coordinates| = %.3g = %.2f units of 2^-53 max|pixel|" % (np.dtype(dtype).name, err, err / unit))
    assert err <= 8 * unit
    # and the values are convex combinations of the frame's pixels
    assert ref.min() >= float(frame.min()) and ref.max() <= float(frame.max())


@pytest.mark.parametrize("n_theta,pad", [(48, 5), (70, 3), (12, 0), (12, 12), (4, 1)])
def test_seam_identities_of_the_restated_rule(n_theta, pad):
    frames = [R.frame_of(np.float64, (23, 31), s) for s in (1, 2)]
    out = R.unwrap(frames, [(15.5, 11.25), (9.0, 14.0)], 17, n_theta, 0.5, 0.8, 0.1, pad)
    assert out.shape == (2, 17, n_theta + 1 + 2 * pad)
    R.seam_identities(out, n_theta, pad)
    assert not np.array_equal(out[0], out[1])
    # pad = 0 of the same spec is the middle of the padded frame
    assert np.array_equal(R.unwrap(frames, [(15.5, 11.25), (9.0, 14.0)], 17, n_theta, 0.5, 0.8, 0.1, 0), out[..., pad:pad + n_theta + 1])
