"""Restatement of scikit-image 0.18.3's classic non-local means, ``denoise_nl_means(image, patch_size, patch_distance, h,
fast_mode=False, sigma)`` for 2-D single-channel frames (the reference's gpet_utils.denoise 'nl', gpet_utils.py:133-134), in
float64 and in the reference's order of operations.  tests/golden/make_nlmeans_fixture.py pins it against the library itself,
the device kernel (csrc/gpet_k_nlmeans.inc) is pinned against it.

``pixel`` is the plain loop of ONE output pixel: candidates in row-major order over the clipped search window, the patch rows
top to bottom with the 5.0 cutoff looked at before each row, the integer-trick exponential, weight sum and weighted sum kept
side by side.  ``nlmeans`` runs the same loops over candidates and patch taps and holds every output pixel's scalars in
arrays: one element of an array sees exactly the operations ``pixel`` performs for it, in the same order (float64 element-wise
operations round as the scalar ones do) -- only the independent pixel axis is spread out.
"""
import math

import numpy as np

from tests.denoise_ref import numpy_sum

CUTOFF = 5.0                         # a patch row is not added once the distance exceeds this: the weight is exactly 0
FEXP_C = 1048576 / math.log(2)       # 2^20 / ln 2
FEXP_BIAS = 1072632447
FEXP_DEFINED_FROM = -708.0           # below, the library's int conversion is undefined; the device returns +0.0
DEFAULTS = dict(patch_size=7, patch_distance=11, h=0.1, sigma=0.0)


def odd_patch(patch_size):
    s = int(patch_size)
    return s + 1 if s % 2 == 0 else s


def fexp(y):
    """The double whose low word is 0 and whose high word is the int32 (int)(C y) + 1072632447; +0.0 below -708."""
    y = float(y)
    if y < FEXP_DEFINED_FROM:
        return 0.0
    hi = int(FEXP_C * y) + FEXP_BIAS  # (int() truncates towards zero, as the C conversion does)
    return float(np.array([hi << 32], dtype=np.int64).view(np.float64)[0])


def fexp_array(y):
    y = np.asarray(y, dtype=np.float64)
    safe = np.where(y < FEXP_DEFINED_FROM, 0.0, y)
    hi = np.trunc(FEXP_C * safe).astype(np.int64) + FEXP_BIAS
    return np.where(y < FEXP_DEFINED_FROM, 0.0, (hi << 32).view(np.float64))


def tap_arguments(patch_size):
    """The s * s arguments of the taps' exponential, row-major."""
    s = odd_patch(patch_size)
    off = s // 2
    A = (s - 1.0) / 4.0
    x = np.arange(-off, off + 1, dtype=np.float64)
    xr, xc = np.meshgrid(x, x, indexing="ij")
    return -(xr * xr + xc * xc) / (2 * A * A)


def taps(patch_size, h, exp=None):
    """w[a][b] = exp(-(x_a^2 + x_b^2) / (2 A^2)) * (1 / (sum(w) h h)), A = (s - 1) / 4, sum = numpy's pairwise sum; ``exp``: a
    scalar exponential to use instead of numpy's vectorised one (math.exp: the C library's)."""
    args = tap_arguments(patch_size).ravel()
    e = np.exp(args) if exp is None else np.array([exp(float(v)) for v in args])
    scale = 1.0 / (numpy_sum(e) * h * h)
    s = odd_patch(patch_size)
    return (e * scale).reshape(s, s)


def pad(img, off):
    """numpy's 'reflect': c b | a b c | b a, the edge pixel not repeated."""
    img = np.asarray(img)
    M, N = img.shape
    assert off < min(M, N)
    r = np.abs(np.arange(-off, M + off))
    r = np.where(r > M - 1, 2 * (M - 1) - r, r)
    c = np.abs(np.arange(-off, N + off))
    c = np.where(c > N - 1, 2 * (N - 1) - c, c)
    return np.ascontiguousarray(img.astype(np.float64)[r[:, None], c[None, :]])


def window(pos, n, d):
    """First and one-past-last candidate along an axis of length n for output position pos."""
    return pos - min(d, pos), pos + min(d + 1, n - pos)


def pixel(P, w, row, col, M, N, d, var2, info=None):
    """One output pixel from the padded frame P and the taps w.  ``info``: a dict that collects the largest final distance of
    the candidates that reached the exponential ('dmax')."""
    s = w.shape[0]
    off = s // 2
    wsum, acc = 0.0, 0.0
    i0, i1 = window(row, M, d)
    j0, j1 = window(col, N, d)
    for i in range(i0, i1):
        for j in range(j0, j1):
            dist, cut = 0.0, False
            for a in range(s):
                if dist > CUTOFF:
                    cut = True
                    break
                for b in range(s):
                    t = P[row + a, col + b] - P[i + a, j + b]
                    dist = dist + w[a, b] * (t * t - var2)
            if cut:
                weight = 0.0
            else:
                weight = fexp(-max(0.0, dist))
                if info is not None:
                    info["dmax"] = max(info.get("dmax", 0.0), dist)
            wsum = wsum + weight
            acc = acc + weight * P[i + off, j + off]
    return acc / wsum


def nlmeans(img, patch_size=7, patch_distance=11, h=0.1, sigma=0.0, w=None, return_info=False):
    """The whole frame -> float64 (M, N).  ``w``: taps to use instead of the derived ones."""
    img = np.asarray(img)
    M, N = img.shape
    s = odd_patch(patch_size)
    off, d = s // 2, int(patch_distance)
    var2 = 2.0 * float(sigma) * float(sigma)
    w = taps(s, h) if w is None else np.asarray(w, dtype=np.float64).reshape(s, s)
    P = pad(img, off)
    rows, cols = np.arange(M)[:, None], np.arange(N)[None, :]
    wsum, acc = np.zeros((M, N)), np.zeros((M, N))
    dmax, fell_back = 0.0, False
    for di in range(-d, d + 1):
        for dj in range(-d, d + 1):
            valid = (rows + di >= 0) & (rows + di < M) & (cols + dj >= 0) & (cols + dj < N)  # the window clipped to the image
            if not valid.any():
                continue
            ci = np.clip(rows + di, 0, M - 1)
            cj = np.clip(cols + dj, 0, N - 1)
            dist = np.zeros((M, N))
            cut = np.zeros((M, N), dtype=bool)
            for a in range(s):
                cut |= dist > CUTOFF  # latched at the start of a patch row: the distance may fall again when var2 > 0
                for b in range(s):
                    t = P[rows + a, cols + b] - P[ci + a, cj + b]
                    dist = dist + w[a, b] * (t * t - var2)
            live = valid & ~cut
            weight = np.where(live, fexp_array(-np.maximum(0.0, dist)), 0.0)
            if live.any():
                dmax = max(dmax, float(dist[live].max()))
            fell_back = fell_back or bool((valid & cut & (dist <= CUTOFF)).any())
            wsum = np.where(valid, wsum + weight, wsum)
            acc = np.where(valid, acc + weight * P[ci + off, cj + off], acc)
    out = acc / wsum
    return (out, dict(dmax=dmax, fell_back=fell_back)) if return_info else out


def nlmeans_kwargs(img, kwargs, w=None, return_info=False):
    kw = dict(DEFAULTS)
    kw.update({k: v for k, v in kwargs.items() if k in DEFAULTS})
    return nlmeans(img, w=w, return_info=return_info, **kw)
