"""The denoise quality metrics of csrc/gpet_metrics_plan.h restated with numpy: the working type of the simple metrics, the running-sum
uniform filter, S, the counts behind the entropy and the ONE summation order the device owns (metrics_sum).  Python and numpy round
every operation once and fuse nothing, which is what the header asks of its compilers.

``figures(a, b, ...)`` gives what gpet_metrics_images gives for one pair, with the sums in the device's order; ``bounds(...)`` the
distances DESIGN.md section 9 allows between these and scikit-image 0.18.3's own."""
import math

import numpy as np

THREADS = 256  # METRICS_THREADS
RANGE_WORDS = "im_true has intensity values outside the range expected for its data type.  Please manually specify the data_range"
EXTENT_WORDS = "win_size exceeds image extent.  If the input is a multichannel (color) image, set multichannel=True."
ODD_WORDS = "Window size must be odd."
U = 2.0 ** -53


def work_type(dt_a, dt_b):
    """np.result_type(a, b, float32) for the four pixel types: float64 as soon as either side is float64."""
    return np.float64 if np.float64 in (np.dtype(dt_a).type, np.dtype(dt_b).type) else np.float32


def metrics_sum(t):
    """Lane l of 256 adds t[l], t[l + 256], .. from +0.0 in ascending order; the lane sums are combined by halving strides."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    rows = -(-t.shape[0] // THREADS)
    pad = np.zeros(rows * THREADS, dtype=np.float64)  # (x + 0.0 == x for every x a lane can hold: it starts from +0.0)
    pad[:t.shape[0]] = t
    part = np.zeros(THREADS, dtype=np.float64)
    for row in pad.reshape(rows, THREADS):
        part = part + row
    s = THREADS // 2
    while s > 0:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return float(part[0])


def sq_diffs(a, b):
    """(a - b)^2 rounded in the working type, widened to float64, in raster order."""
    W = work_type(a.dtype, b.dtype)
    d = a.astype(W) - b.astype(W)
    return (d * d).astype(np.float64).reshape(-1)


def reflect(s, n):
    return -s - 1 if s < 0 else (2 * n - 1 - s if s >= n else s)


def uniform_filter1d(x, size, axis):
    """scipy.ndimage.uniform_filter1d(x, size, axis, mode='reflect') of a float64 array by its own recurrence, all lines at once."""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, 0)
    n, h = x.shape[0], size // 2
    ext = x[[reflect(e - h, n) for e in range(n + size - 1)]]
    out = np.empty_like(x)
    tmp = np.zeros(x.shape[1:], dtype=np.float64)
    for e in range(size):
        tmp = tmp + ext[e]
    out[0] = tmp / float(size)
    for i in range(1, n):
        tmp = tmp + (ext[i + size - 1] - ext[i - 1])
        out[i] = tmp / float(size)
    return np.moveaxis(out, 0, axis)


def uniform_filter(x, size):
    return uniform_filter1d(uniform_filter1d(x, size, 0), size, 1)


def ssim_const(win_size, use_sample_covariance, K1, K2, R):
    NP = float(win_size) * float(win_size)
    cov_norm = NP / (NP - 1.0) if use_sample_covariance else 1.0
    k1, k2 = float(K1) * float(R), float(K2) * float(R)
    return cov_norm, k1 * k1, k2 * k2


def ssim_S(ux, uy, uxx, uyy, uxy, cov_norm, C1, C2):
    pxx, pyy, pxy = ux * ux, uy * uy, ux * uy
    vx = cov_norm * (uxx - pxx)
    vy = cov_norm * (uyy - pyy)
    vxy = cov_norm * (uxy - pxy)
    A1 = (2.0 * ux) * uy + C1
    A2 = 2.0 * vxy + C2
    B1 = pxx + pyy + C1
    B2 = vx + vy + C2
    with np.errstate(divide="ignore", invalid="ignore"):
        return (A1 * A2) / (B1 * B2)


def default_range_ssim(dt):
    return {np.uint8: 255.0, np.uint16: 65535.0}.get(np.dtype(dt).type, 2.0)


def default_range_psnr(a):
    if a.dtype == np.uint8:
        return 255.0
    if a.dtype == np.uint16:
        return 65535.0
    lo, hi = float(a.min()), float(a.max())
    if hi > 1.0 or lo < -1.0:
        raise ValueError(RANGE_WORDS)
    return 1.0 if lo >= 0.0 else 2.0


def check_window(shape, win_size):
    if win_size > min(shape):
        raise ValueError(EXTENT_WORDS)
    if win_size % 2 != 1:
        raise ValueError(ODD_WORDS)
    if win_size < 3:
        raise ValueError("metrics: win_size must be at least 3")


def ssim_map(a, b, win_size=7, data_range=None, K1=0.01, K2=0.03, use_sample_covariance=True):
    check_window(a.shape, win_size)
    x, y = a.astype(np.float64), b.astype(np.float64)
    R = default_range_ssim(a.dtype) if data_range is None else float(data_range)
    planes = [uniform_filter(p, win_size) for p in (x, y, x * x, y * y, x * y)]
    return ssim_S(*planes, *ssim_const(win_size, use_sample_covariance, K1, K2, R))


def keys_of(b):
    """The order-preserving 64-bit keys of b's values (metrics_key): -0.0 and 0.0 share one."""
    v = b.astype(np.float64).reshape(-1) + 0.0  # (-0.0 + 0.0 = +0.0; nothing else changes)
    u = v.view(np.uint64)
    neg = (u >> np.uint64(63)).astype(bool)
    return np.where(neg, ~u, u | np.uint64(1 << 63))


def run_counts(sorted_keys):
    """(start positions, counts) of the runs of equal keys."""
    n = sorted_keys.shape[0]
    starts = np.flatnonzero(np.concatenate([[True], sorted_keys[1:] != sorted_keys[:-1]]))
    return starts, np.diff(np.concatenate([starts, [n]]))


def entropy_terms(b):
    """e[i] over the sorted positions: -p log(p) of the run that starts at i (C's log, as the header on the host), +0.0 elsewhere."""
    k = np.sort(keys_of(b))
    n = k.shape[0]
    starts, counts = run_counts(k)
    e = np.zeros(n, dtype=np.float64)
    for s, c in zip(starts.tolist(), counts.tolist()):
        p = 1.0 * float(c) / float(n)
        e[s] = -p * math.log(p)
    return e, counts


def figures(a, b, win_size=7, data_range=None, K1=0.01, K2=0.03, use_sample_covariance=True):
    """dict(psnr, ssim, nrmse, entropy, ssim_map, counts, mse) of one pair in the header's arithmetic and the device's orders."""
    a, b = np.asarray(a), np.asarray(b)
    S = ssim_map(a, b, win_size, data_range, K1, K2, use_sample_covariance)
    W = work_type(a.dtype, b.dtype)
    n = float(a.size)
    R = default_range_psnr(a) if data_range is None else float(data_range)
    mse = metrics_sum(sq_diffs(a, b)) / n
    pad = (win_size - 1) // 2
    crop = S[pad:S.shape[0] - pad, pad:S.shape[1] - pad]
    e, counts = entropy_terms(b)
    span = float(W(a.max()) - W(a.min()))
    with np.errstate(divide="ignore", invalid="ignore"):
        psnr = float(10.0 * np.log10(np.float64(R * R) / np.float64(mse)))
        nrmse = float(np.sqrt(np.float64(mse)) / np.float64(span))
    return dict(psnr=psnr, ssim=metrics_sum(crop) / float(crop.size), nrmse=nrmse, entropy=metrics_sum(e) / math.log(2.0), ssim_map=S,
                counts=counts, mse=mse)


def bounds(n, n_crop, mean_abs_S, k, psnr, nrmse, entropy):
    """The distances allowed per figure between two evaluations that differ in the three summation orders (and a log on either side):
    dict(psnr, ssim, nrmse, entropy), absolute.  MSE: 2 (n - 1) 2^-53 relative -- two orders of adding n non-negative terms."""
    mse_rel = 2.0 * (n - 1) * U
    ulp = lambda v: float(np.spacing(abs(v))) if np.isfinite(v) else 0.0
    return dict(psnr=mse_rel * 10.0 / math.log(10.0) + 2.0 * ulp(psnr), ssim=2.0 * (n_crop - 1) * U * mean_abs_S,
                nrmse=0.5 * mse_rel * abs(nrmse) + ulp(nrmse), entropy=(2.0 * (k - 1) + 8.0) * U * abs(entropy))


def within(got, want, bound):
    """|got - want| <= bound, with equal infinities and equal NaNs agreeing."""
    if got == want or (got != got and want != want):
        return True
    return abs(got - want) <= bound
