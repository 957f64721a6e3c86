"""The polar unwrap (gaussian_process_edge_trace_amd/csrc/gpet_polar_plan.h) restated with numpy float64: every
product and every sum is one numpy operation on float64 arrays, so nothing is contracted, in the order the header states.  No device,
no library, nothing of the package: the tests compare the header (through a host shim), the package's host functions and the kernel
against this file, and this file against scipy's map_coordinates."""
import numpy as np

NTHETA_MIN, CELLS_MAX = 4, 1 << 28


def tables(n_theta, theta0=0.0):
    theta = float(theta0) + (2.0 * np.pi * np.arange(int(n_theta), dtype=np.float64)) / float(int(n_theta))
    return np.cos(theta), np.sin(theta)


def width(n_theta, pad):
    return n_theta + 1 + 2 * pad


def angle_of_column(c, pad, n_theta):
    """a(c) = (c - pad) mod n_theta, non-negative (Python's and numpy's % already are)."""
    return np.mod(np.asarray(c, dtype=np.int64) - pad, n_theta)


def positions(shape, centre, n_r, n_theta, r0=0.0, dr=1.0, theta0=0.0, pad=0):
    """(x, y), each (n_r, W) float64: the clamped sample positions of one frame of ``shape`` = (M, N) around ``centre`` = (cx, cy)."""
    M, N = shape
    cos_t, sin_t = tables(n_theta, theta0)
    a = angle_of_column(np.arange(width(n_theta, pad)), pad, n_theta)
    rho = (np.float64(r0) + np.arange(n_r, dtype=np.float64) * np.float64(dr))[:, None]
    x = np.float64(centre[0]) + rho * cos_t[a][None, :]
    y = np.float64(centre[1]) + rho * sin_t[a][None, :]
    x = np.minimum(np.maximum(x, 0.0), np.float64(N - 1))
    y = np.minimum(np.maximum(y, 0.0), np.float64(M - 1))
    return x, y


def bilinear(frame, x, y):
    """The rule's value at clamped positions: taps x0 = min(floor(x), N - 2), y0 likewise; top, bot, out in the header's order."""
    M, N = frame.shape
    p = frame.astype(np.float64)  # (exact for uint8, uint16, float32)
    x0 = np.minimum(np.floor(x).astype(np.int64), N - 2)
    y0 = np.minimum(np.floor(y).astype(np.int64), M - 2)
    fx, fy = x - x0.astype(np.float64), y - y0.astype(np.float64)
    gx, gy = 1.0 - fx, 1.0 - fy
    top = gx * p[y0, x0] + fx * p[y0, x0 + 1]
    bot = gx * p[y0 + 1, x0] + fx * p[y0 + 1, x0 + 1]
    return gy * top + fy * bot


def unwrap(frames, centre, n_r, n_theta, r0=0.0, dr=1.0, theta0=0.0, pad=0):
    """(T, n_r, W) float64: ``frames`` a (T, M, N) array or a list of (M, N) frames, ``centre`` (cx, cy) or (T, 2)."""
    frames = [np.asarray(f) for f in frames]
    centre = np.asarray(centre, dtype=np.float64).reshape(-1, 2)
    out = []
    for t, f in enumerate(frames):
        x, y = positions(f.shape, centre[0 if centre.shape[0] == 1 else t], n_r, n_theta, r0, dr, theta0, pad)
        out.append(bilinear(f, x, y))
    return np.stack(out)


def refusal(n_r, n_theta, pad, r0, dr, pix_known=True, M=2, N=2, n_centres=1, n_img=1, cx=(0.0,), cy=(0.0,)):
    """polar_check's refusals, same order, same words; None when the spec can be unwrapped with."""
    if not pix_known:
        return "polar: unknown pixel type"
    if M < 2 or N < 2:
        return "polar: frames must be at least 2 x 2 pixels"
    if n_r < 1:
        return "polar: n_r must be at least 1"
    if n_theta < NTHETA_MIN:
        return "polar: n_theta must be at least 4"
    if pad < 0 or pad > n_theta:
        return "polar: pad must lie in [0, n_theta]"
    if not (0.0 <= r0 < float("inf")):
        return "polar: r0 must be finite and at least 0"
    if not (0.0 < dr < float("inf")):
        return "polar: dr must be finite and above 0"
    if width(n_theta, pad) > CELLS_MAX // n_r:
        return "polar: the unwrapped frame exceeds 2^28 pixels (n_r * (n_theta + 1 + 2 * pad))"
    if n_centres != 1 and n_centres != n_img:
        return "polar: one centre for all frames or one per frame"
    if cx is None or cy is None:
        return "polar: the centres are a null pointer"
    if not all(abs(float(v)) < float("inf") for v in list(cx)[:n_centres] + list(cy)[:n_centres]):
        return "polar: a centre is not finite"
    return None


def seam_identities(out, n_theta, pad):
    """The three identities every unwrapped frame (.., n_r, W) satisfies: the seam and the two pads."""
    assert np.array_equal(out[..., pad], out[..., pad + n_theta])
    assert np.array_equal(out[..., :pad], out[..., n_theta:n_theta + pad])
    assert np.array_equal(out[..., pad + n_theta + 1:], out[..., pad + 1:2 * pad + 1])


def frame_of(dtype, shape, seed):
    """A test frame of the dtype with values over its range."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt == np.uint8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if dt == np.uint16:
        return rng.integers(0, 65536, shape, dtype=np.uint16)
    return (rng.random(shape) * 200.0 - 50.0).astype(dt)


def outline(theta, R0, a):
    """The star-shaped outline of the test discs: R(theta) = R0 + a cos 3 theta."""
    return R0 + a * np.cos(3.0 * theta)


def disc_frame(shape, centre, outlines=((14.0, 2.0), (26.0, 4.0)), levels=(40.0, 120.0, 200.0), seed=0, dtype=np.uint8):
    """A frame of nested dark discs (a lumen) around ``centre`` = (cx, cy): level k inside outline k (R0, a), anti-aliased over one
    pixel of radius, plus seeded noise of +-6 grey levels.  Every outline is a dark-to-bright step going outwards, the step
    ``kernel_builder``'s default kernel answers to on the unwrapped frame."""
    M, N = shape
    yy, xx = np.mgrid[0:M, 0:N].astype(np.float64)
    dx, dy = xx - centre[0], yy - centre[1]
    r, theta = np.hypot(dx, dy), np.arctan2(dy, dx)
    img = np.full(shape, levels[-1], dtype=np.float64)
    for k in range(len(outlines) - 1, -1, -1):
        inside = np.clip(outline(theta, *outlines[k]) - r + 0.5, 0.0, 1.0)
        img = img + inside * (levels[k] - levels[k + 1])
    img = img + np.random.default_rng(seed).integers(-6, 7, shape)
    return np.clip(np.rint(img), 0, 255).astype(dtype)


def radial_error(trace, polar, R0, a):
    """Mean absolute radial error of a trace ((n, 2) rows, columns) on polar frames against the outline (R0, a)."""
    trace = np.asarray(trace)
    ang = angle_of_column(trace[:, 1], polar["pad"], polar["n_theta"])
    theta = polar.get("theta0", 0.0) + 2.0 * np.pi * ang / polar["n_theta"]
    radius = polar.get("r0", 0.0) + trace[:, 0] * polar.get("dr", 1.0)
    return float(np.mean(np.abs(radius - outline(theta, R0, a))))
