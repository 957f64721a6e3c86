"""Restatements of scikit-image 0.18.3's fast-mode non-local means, ``denoise_nl_means(image, patch_size, patch_distance, h,
fast_mode=True, sigma)`` -- the library's default -- for 2-D single-channel frames (the reference's gpet_utils.denoise 'nl'), in
float64 and in the library's order of operations.  tests/golden/make_nlmeans_fast_fixture.py pins both against the library itself,
the device kernels (csrc/gpet_k_nlfast.inc) are pinned against them.  The arithmetic is stated in csrc/gpet_nlfast_plan.h.

``nlmeans_fast_loops`` is the plain loops: per shift an integral image of squared differences in raster order, then the weights
scattered to both pixels of every pair.  ``nlmeans_fast`` walks the integral images along anti-diagonals (the cells of one are
independent, so ascending diagonals give every cell the operands it had in raster order), several shifts side by side, and
GATHERS: every output pixel adds its terms in the order the scatter reaches it (``terms_in_order``).
"""
import struct

import numpy as np

from tests.nlmeans_ref import CUTOFF, FEXP_BIAS, FEXP_C, fexp_array, odd_patch

DEFAULTS = dict(patch_size=7, patch_distance=11, h=0.1, sigma=0.0)


def geometry(M, N, patch_size, patch_distance):
    """(s, off, d, pad, nr, nc) of an M x N frame."""
    s = odd_patch(patch_size)
    off, d = s // 2, int(patch_distance)
    pad = off + d + 1
    return s, off, d, pad, M + 2 * pad, N + 2 * pad


def shifts(d):
    """The shift table in the library's order: (t_row, t_col, alpha), t_row = -d .. d outer, t_col = 0 .. d inner."""
    return [(tr, tc, 0.5 if (tc == 0 and tr != 0) else 1.0) for tr in range(-d, d + 1) for tc in range(0, d + 1)]


def integral_range(n, t):
    """First and one-past-last index of an axis of padded length n the integral of shift component t is formed over."""
    return max(1, -t), min(n, n - t)


def weight_range(n, t, off):
    """First and one-past-last index of an axis of padded length n whose pairs of shift component t get a weight."""
    return max(off, off - t), min(n - off, n - off - t)


def pad_reflect(img, pad):
    """numpy's 'reflect' by pad pixels, reflecting once; integer frames keep their range."""
    img = np.asarray(img)
    assert pad <= min(img.shape) - 1
    return np.pad(img.astype(np.float64), pad, mode="reflect")


def fexp_scalar(y):
    hi = int(FEXP_C * y) + FEXP_BIAS  # (int() truncates towards zero, as the C conversion does)
    return struct.unpack("<d", struct.pack("<q", hi << 32))[0]


def h2s2_of(h, s):
    return ((h * h) * s) * s


def nlmeans_fast_loops(img, patch_size=7, patch_distance=11, h=0.1, sigma=0.0):
    """The whole frame -> float64 (M, N), as the library's loops run."""
    M, N = np.asarray(img).shape
    s, off, d, pad, nr, nc = geometry(M, N, patch_size, patch_distance)
    var2 = 2.0 * float(sigma) * float(sigma)
    h2s2 = h2s2_of(float(h), s)
    P = pad_reflect(img, pad).tolist()
    W = [[0.0] * nc for _ in range(nr)]
    R = [[0.0] * nc for _ in range(nr)]
    for t_row, t_col, alpha in shifts(d):
        I = [[0.0] * nc for _ in range(nr)]
        c0, c1 = integral_range(nc, t_col)
        for r in range(*integral_range(nr, t_row)):
            Pr, Ps, Ir, Iu = P[r], P[r + t_row], I[r], I[r - 1]
            for c in range(c0, c1):
                t = Pr[c] - Ps[c + t_col]
                q = (0.0 + t * t) - var2
                Ir[c] = ((q + Iu[c]) + Ir[c - 1]) - Iu[c - 1]
        c0, c1 = weight_range(nc, t_col, off)
        for row in range(*weight_range(nr, t_row, off)):
            Ip, Im = I[row + off], I[row - off]
            Wo, Wp, Ro, Rp, Po, Pp = W[row], W[row + t_row], R[row], R[row + t_row], P[row], P[row + t_row]
            for col in range(c0, c1):
                dd = ((Ip[col + off] + Im[col - off]) - Im[col + off]) - Ip[col - off]
                dist = max(dd, 0.0) / h2s2
                if dist > CUTOFF:
                    continue
                w = alpha * fexp_scalar(-dist)
                Wo[col] += w
                Wp[col + t_col] += w
                Ro[col] += w * Pp[col + t_col]
                Rp[col + t_col] += w * Po[col]
    W, R = np.array(W), np.array(R)
    return R[pad:pad + M, pad:pad + N] / W[pad:pad + M, pad:pad + N]


def terms_in_order(t_row, t_col):
    """The terms one pixel p receives from shift t, in the order the scatter reaches it: 'own' is the pair (p, p + t), whose
    weight is looked up at p and which adds P[p + t]; 'partner' is the pair (p - t, p), looked up at p - t, adding P[p - t]."""
    if t_row == 0 and t_col == 0:
        return ("own", "own")
    if t_row > 0 or (t_row == 0 and t_col > 0):
        return ("partner", "own")
    return ("own", "partner")


def integrals(P, table, var2):
    """The integral images of the shifts of ``table`` -> (len(table), nr, nc), along anti-diagonals."""
    nr, nc = P.shape
    n = len(table)
    Q = np.zeros((n, nr, nc))
    valid = np.zeros((n, nr, nc), dtype=bool)
    for k, (t_row, t_col, _) in enumerate(table):
        r0, r1 = integral_range(nr, t_row)
        c0, c1 = integral_range(nc, t_col)
        t = P[r0:r1, c0:c1] - P[r0 + t_row:r1 + t_row, c0 + t_col:c1 + t_col]
        Q[k, r0:r1, c0:c1] = (0.0 + t * t) - var2
        valid[k, r0:r1, c0:c1] = True
    I = np.zeros((n, nr, nc))
    for D in range(2, nr + nc - 1):  # (row 0 and column 0 are outside every range)
        rr = np.arange(max(1, D - (nc - 1)), min(nr - 1, D - 1) + 1)
        cc = D - rr
        v = ((Q[:, rr, cc] + I[:, rr - 1, cc]) + I[:, rr, cc - 1]) - I[:, rr - 1, cc - 1]
        I[:, rr, cc] = np.where(valid[:, rr, cc], v, 0.0)
    return I


def nlmeans_fast(img, patch_size=7, patch_distance=11, h=0.1, sigma=0.0, batch_bytes=32 << 20):
    """The whole frame -> float64 (M, N): integrals along anti-diagonals, every output pixel gathering its terms in order."""
    M, N = np.asarray(img).shape
    s, off, d, pad, nr, nc = geometry(M, N, patch_size, patch_distance)
    var2 = 2.0 * float(sigma) * float(sigma)
    h2s2 = h2s2_of(float(h), s)
    P = pad_reflect(img, pad)
    table = shifts(d)
    per = max(1, int(batch_bytes // (nr * nc * 8)))
    W, R = np.zeros((M, N)), np.zeros((M, N))
    rows, cols = np.arange(pad, pad + M)[:, None], np.arange(pad, pad + N)[None, :]
    for first in range(0, len(table), per):
        group = table[first:first + per]
        I = integrals(P, group, var2)
        for k, (t_row, t_col, alpha) in enumerate(group):
            r0, r1 = weight_range(nr, t_row, off)
            c0, c1 = weight_range(nc, t_col, off)
            for term in terms_in_order(t_row, t_col):
                # the pair's first pixel (row, col) and the pixel whose value this pixel adds
                if term == "own":
                    row, col, vr, vc = rows, cols, rows + t_row, cols + t_col
                else:
                    row, col, vr, vc = rows - t_row, cols - t_col, rows - t_row, cols - t_col
                # (pad = off + d + 1 puts every pair of an OUTPUT pixel inside the weight ranges)
                assert r0 <= row.min() and row.max() < r1 and c0 <= col.min() and col.max() < c1
                dd = ((I[k, row + off, col + off] + I[k, row - off, col - off]) - I[k, row - off, col + off]) - I[k, row + off, col - off]
                dist = np.maximum(dd, 0.0) / h2s2
                keep = ~(dist > CUTOFF)
                w = alpha * fexp_array(-np.where(keep, dist, 0.0))
                W = np.where(keep, W + w, W)
                R = np.where(keep, R + w * P[vr, vc], R)
    return R / W


def with_kwargs(fn, img, kwargs, **more):
    kw = dict(DEFAULTS)
    kw.update({k: v for k, v in kwargs.items() if k in DEFAULTS})
    return fn(img, **dict(kw, **more))
