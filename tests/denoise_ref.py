"""NumPy restatement of the four denoising techniques the device runs (gpet_utils.denoise: 'median', 'minimum', 'gaussian',
'tvc'), operation by operation in the order scipy.ndimage 1.7.1 and scikit-image 0.18.3 perform them, so that the result is the
reference's bit for bit (tests/test_denoise_fixture.py pins it against tests/golden/denoise.npz, which the unmodified
reference wrote).  A test helper like tests/matern_exact.py: nothing in the package imports it.

The Gaussian taps use math.exp (the C library's exp, what the HIP library's host code calls), not numpy.exp.
"""
import math

import numpy as np

MODES = ("reflect", "nearest")


def extend_index(i, n, mode):
    """Index into an axis of length n for position i outside it: 'reflect' is d c b a | a b c d | d c b a, 'nearest' clamps."""
    i = np.asarray(i, dtype=np.int64)
    if mode == "nearest":
        return np.clip(i, 0, n - 1)
    if mode != "reflect":
        raise ValueError("mode %r" % (mode,))
    p = np.mod(i, 2 * n)
    return np.where(p < n, p, 2 * n - 1 - p)


def window_origin(k):
    """The window of extent k starts this many pixels before the output pixel (scipy: the centre is k // 2)."""
    return k // 2


def _pair(v):
    return (v, v) if np.isscalar(v) else (v[0], v[1])


def rank_filter(img, size, rank, mode="reflect"):
    """Element `rank` of the sorted size_y x size_x window around every pixel; the dtype stays."""
    img = np.asarray(img)
    sy, sx = (int(s) for s in _pair(size))
    M, N = img.shape
    iy = extend_index(np.arange(M)[:, None] - window_origin(sy) + np.arange(sy)[None, :], M, mode)  # [M, sy]
    ix = extend_index(np.arange(N)[:, None] - window_origin(sx) + np.arange(sx)[None, :], N, mode)  # [N, sx]
    win = img[iy[:, None, :, None], ix[None, :, None, :]].reshape(M, N, sy * sx)
    return np.ascontiguousarray(np.sort(win, axis=-1)[:, :, rank])


def median(img, size, mode="reflect"):
    sy, sx = (int(s) for s in _pair(size))
    return rank_filter(img, (sy, sx), (sy * sx) // 2, mode)


def minimum(img, size, mode="reflect"):
    return rank_filter(img, size, 0, mode)


def gaussian_radius(sigma, truncate=4.0):
    return int(truncate * float(sigma) + 0.5)


def numpy_sum(a):
    """numpy's float64 add.reduce of a contiguous 1-D array: a[0] + pairwise_sum(a[1:]) with eight partial sums per block."""
    def pairwise(v):
        n = len(v)
        if n < 8:
            res = 0.0
            for t in v:
                res = res + t
            return res
        if n <= 128:
            r = [v[j] for j in range(8)]
            i = 8
            while i < n - (n % 8):
                for j in range(8):
                    r[j] = r[j] + v[i + j]
                i += 8
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
            while i < n:
                res = res + v[i]
                i += 1
            return res
        n2 = n // 2
        n2 -= n2 % 8
        return pairwise(v[:n2]) + pairwise(v[n2:])
    a = [float(t) for t in a]
    return a[0] + pairwise(a[1:]) if len(a) > 1 else a[0]


def gaussian_taps(sigma, truncate=4.0, bump=None):
    """scipy's _gaussian_kernel1d(sigma, 0, radius): exp(-0.5 / sigma^2 x^2) / sum, x = -radius .. radius.  scipy calls
    numpy.exp, whose vectorised forms differ from the C library's exp by one unit in the last place for some arguments (which
    ones depends on numpy's version and the CPU); the device library calls the C library's, and so does this.  ``bump`` =
    (j, s): the exponential of |x| = j moved by s = +-1 unit in the last place -- the size of that disagreement."""
    sigma = float(sigma)
    r = gaussian_radius(sigma, truncate)
    c = -0.5 / (sigma * sigma)
    phi = [math.exp(c * float(x * x)) for x in range(-r, r + 1)]
    if bump is not None:
        j, sgn = bump
        for x in range(-r, r + 1):
            if abs(x) == j:
                phi[x + r] = float(np.nextafter(phi[x + r], math.inf if sgn > 0 else -math.inf))
    s = numpy_sum(phi)
    return np.array([p / s for p in phi], dtype=np.float64)


def quantise(acc, dtype):
    """scipy's store of a float64 line into the output array: a C cast (truncation towards zero for the unsigned types)."""
    dtype = np.dtype(dtype)
    if dtype.kind == "u":
        return np.trunc(acc).astype(dtype)
    return acc.astype(dtype)


def gaussian_pass(img, w, axis, mode="reflect", return_acc=False):
    """One correlate1d pass with symmetric taps w (2 r + 1 of them), summed in scipy's order; stored in img's dtype."""
    img = np.asarray(img)
    r = (len(w) - 1) // 2
    x = np.moveaxis(img, axis, 0).astype(np.float64)
    n = x.shape[0]
    pos = np.arange(n)
    acc = x * w[r]
    for l in range(-r, 0):
        a = x[extend_index(pos + l, n, mode)]
        b = x[extend_index(pos - l, n, mode)]
        acc = acc + (a + b) * w[l + r]
    acc = np.moveaxis(acc, 0, axis)
    out = np.ascontiguousarray(quantise(acc, img.dtype))
    return (out, acc) if return_acc else out


def gaussian(img, sigma, truncate=4.0, mode="reflect", return_acc=False, taps=None):
    """gaussian_filter(img, sigma, truncate=truncate, mode=mode): axis 0, then axis 1; an axis with sigma <= 1e-15 is skipped.
    ``taps``: the two axes' taps, where they are not to come from gaussian_taps."""
    cur = np.asarray(img)
    accs = []
    for axis, s in enumerate(_pair(sigma)):
        if float(s) > 1e-15:
            w = gaussian_taps(s, truncate) if taps is None else np.asarray(taps[axis], dtype=np.float64)
            cur, acc = gaussian_pass(cur, w, axis, mode, return_acc=True)
            accs.append(acc)
    cur = np.array(cur, copy=True)
    return (cur, accs) if return_acc else cur


def as_float(img):
    """What denoise_tv_chambolle iterates on: float frames as they are, u8 / u16 through img_as_float, which multiplies
    by the float64 reciprocal: x * (1 / 255), x * (1 / 65535)."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img.astype(np.float64) * (1.0 / 255.0)
    if img.dtype == np.uint16:
        return img.astype(np.float64) * (1.0 / 65535.0)
    return img


def tvc(img, weight=0.1, eps=2.0e-4, n_iter_max=200, return_info=False):
    """_denoise_tv_chambolle_nd for a 2-D image.  Returns the image; with return_info also the number of iterations run
    and, per iteration after the first, the margin (|E_prev - E| - eps E_0) / (eps E_0) of the stopping test."""
    image = as_float(img)
    p0 = np.zeros_like(image)
    p1 = np.zeros_like(image)
    d = np.zeros_like(image)
    tau = 1.0 / 4.0
    margins = []
    i = 0
    out = image
    while i < n_iter_max:
        if i > 0:
            d = -(p0 + p1)
            d[1:, :] += p0[:-1, :]
            d[:, 1:] += p1[:, :-1]
            out = image + d
        else:
            out = image
        E = (d ** 2).sum()
        g0 = np.zeros_like(image)
        g1 = np.zeros_like(image)
        g0[:-1, :] = out[1:, :] - out[:-1, :]
        g1[:, :-1] = out[:, 1:] - out[:, :-1]
        norm = np.sqrt(g0 ** 2 + g1 ** 2)
        E += weight * norm.sum()
        norm = norm * (tau / weight)
        norm = norm + 1.0
        p0 = (p0 - tau * g0) / norm
        p1 = (p1 - tau * g1) / norm
        E /= float(image.size)
        if i == 0:
            E_init = E
            E_prev = E
        else:
            margins.append((abs(E_prev - E) - eps * E_init) / (eps * E_init))
            if abs(E_prev - E) < eps * E_init:
                i += 1
                break
            E_prev = E
        i += 1
    out = np.array(out, copy=True)
    return (out, i, np.array(margins, dtype=np.float64)) if return_info else out


def gaussian_exp_spread(img, sigma, truncate=4.0, mode="reflect"):
    """The largest change of gaussian()'s float64 result when ONE exponential of the taps moves by one unit in the last place
    (every |x| of either axis, both directions)."""
    base = gaussian(img, sigma, truncate, mode).astype(np.float64)
    sig = _pair(sigma)
    worst = 0.0
    for axis in (0, 1):
        if not float(sig[axis]) > 1e-15:
            continue
        for j in range(gaussian_radius(sig[axis], truncate) + 1):
            for sgn in (1, -1):
                taps = [gaussian_taps(sig[a], truncate, bump=(j, sgn) if a == axis else None) for a in (0, 1)]
                worst = max(worst, float(np.abs(gaussian(img, sigma, truncate, mode, taps=taps).astype(np.float64) - base).max()))
    return worst


def make_frame(seed, M, N, noise, dtype, levels=None):
    """A noisy step image (0.3 above a sine-shaped edge, 0.7 below) from numpy's frozen legacy stream, clipped to [0, 1];
    ``levels``: values rounded to multiples of 1 / levels.  u8 / u16: scaled to the type's range and rounded."""
    rs = np.random.RandomState(seed)
    rows = np.arange(M)[:, None]
    edge = M / 2.0 + (M / 5.0) * np.sin(np.linspace(0.0, 2.0 * np.pi, N))[None, :]
    x = np.where(rows >= edge, 0.7, 0.3) + rs.normal(0.0, noise, (M, N))
    x = np.clip(x, 0.0, 1.0)
    if levels:
        x = np.rint(x * levels) / levels
    dtype = np.dtype(dtype)
    if dtype.kind == "u":
        return np.rint(x * np.iinfo(dtype).max).astype(dtype)
    return x.astype(dtype)


def denoise(img, technique, kwargs):
    """The reference's gpet_utils.denoise for the four techniques."""
    kw = dict(kwargs)
    if technique == "median":
        return median(img, kw["size"], kw.get("mode", "reflect"))
    if technique == "minimum":
        return minimum(img, kw["size"], kw.get("mode", "reflect"))
    if technique == "gaussian":
        return gaussian(img, kw["sigma"], kw.get("truncate", 4.0), kw.get("mode", "reflect"))
    if technique == "tvc":
        return tvc(img, kw.get("weight", 0.1), kw.get("eps", 2.0e-4), kw.get("n_iter_max", 200))
    raise ValueError(technique)
