"""Restatement of the reference's gpet_utils.denoise(image, 'wavelet', kwargs) (gpet_utils.py:137-138) = scikit-image 0.18.3's
denoise_wavelet on PyWavelets 1.1.1, for a 2-D single-channel frame and an orthogonal wavelet, in plain loops: every sum below
is formed term by term in the order written, in float64 (numpy serves only as elementwise arithmetic over the lines of the other
axis, which does not touch the order within a line).  tests/test_wavelet_fixture.py pins it to tests/golden/wavelet.npz bit for
bit; the one quantity that follows the DEVICE's order and not numpy's is the mean of squares under a BayesShrink threshold
(mean_squares: csrc/gpet_wavelet_plan.h states the order), which is why thresholds can be injected."""
import math

import numpy as np

PPF75 = 0.6744897501960817  # scipy.stats.norm.ppf(0.75), as the library divides by it
EPS = 2.0 ** -52
BANDS = ("ad", "da", "dd")  # the detail bands of a level: first letter axis 0, second axis 1
THRESH_GROUP = 256          # threads of the workgroup that sums a band (gpet_wavelet_plan.h: WV_THRESH_THREADS)


# ---- filters and levels -------------------------------------------------------------------------------------------------------------
def filters(dec_lo):
    """dec_lo of an orthogonal wavelet -> (dec_lo, dec_hi, rec_lo, rec_hi) as PyWavelets tabulates them."""
    lo = [float(v) for v in dec_lo]
    F = len(lo)
    dec_hi = [(-1.0 if (k + 1) % 2 else 1.0) * lo[F - 1 - k] for k in range(F)]
    rec_lo = lo[::-1]
    rec_hi = [(-1.0 if k % 2 else 1.0) * lo[k] for k in range(F)]
    return lo, dec_hi, rec_lo, rec_hi


def max_level(n, F):
    """The largest L with (F - 1) * 2^L <= n (0 if there is none)."""
    L = 0
    while (F - 1) * 2 ** (L + 1) <= n:
        L += 1
    return L


def levels_of(shape, F, wavelet_levels=None, strict=True):
    """Default max(max_level - 3, 1); an explicit value above max_level is refused (``strict=False``: taken, as PyWavelets takes
    it with a warning -- the fixture's generator runs the library that way)."""
    top = max_level(min(shape), F)
    if wavelet_levels is None:
        return max(top - 3, 1)
    if wavelet_levels < 1 or (strict and wavelet_levels > top):
        raise ValueError("wavelet_levels %r: 1 to %d for this frame and filter" % (wavelet_levels, top))
    return int(wavelet_levels)


def out_len(n, F):
    return (n + F - 1) // 2


# ---- one forward level (symmetric extension) --------------------------------------------------------------------------------------------
def dwt_lines(x, f):
    """x: (n, lines), the transform runs along axis 0 -> (out_len(n), lines)."""
    n, F = x.shape[0], len(f)
    assert n >= F - 1
    out = np.empty((out_len(n, F),) + x.shape[1:])
    for o in range(out.shape[0]):
        i = 2 * o + 1
        s = np.zeros(x.shape[1:])
        if i < n:
            for j in range(F):
                k = i - j
                s = s + f[j] * x[k if k >= 0 else -k - 1]
        else:
            for m in range(i - n + 1):        # the overhang, walking back from the edge
                s = s + f[i - n - m] * x[n - 1 - m]
            for j in range(i - n + 1, F):
                s = s + f[j] * x[i - j]
        out[o] = s
    return out


def dwt2(a, lo, hi):
    """One level: axis 0 first, then axis 1 -> dict(aa, ad, da, dd)."""
    a = np.asarray(a, dtype=np.float64)
    a0, d0 = dwt_lines(a, lo), dwt_lines(a, hi)
    t = lambda v: np.ascontiguousarray(v.T)  # noqa: E731
    return dict(aa=t(dwt_lines(t(a0), lo)), ad=t(dwt_lines(t(a0), hi)), da=t(dwt_lines(t(d0), lo)), dd=t(dwt_lines(t(d0), hi)))


def wavedec2(a, dec_lo, levels):
    """-> [level 1 (finest), ..., level L], each dict(aa, ad, da, dd); aa of level l is the input of level l + 1."""
    lo, hi, _, _ = filters(dec_lo)
    out = []
    for _ in range(levels):
        out.append(dwt2(a, lo, hi))
        a = out[-1]["aa"]
    return out


# ---- one inverse level ----------------------------------------------------------------------------------------------------------------
def idwt_lines(a, d, rec_lo, rec_hi):
    """a, d: (n', lines) -> (2 n' - F + 2, lines) along axis 0."""
    F = len(rec_lo)
    n1, h = a.shape[0], F // 2
    out = np.empty((2 * n1 - F + 2,) + a.shape[1:])
    for i in range(h - 1, n1):
        for p in (0, 1):
            s1 = np.zeros(a.shape[1:])
            s2 = np.zeros(a.shape[1:])
            for j in range(h):
                s1 = s1 + rec_lo[2 * j + p] * a[i - j]
            for j in range(h):
                s2 = s2 + rec_hi[2 * j + p] * d[i - j]
            out[2 * (i - h + 1) + p] = (0.0 + s1) + s2
    return out


def idwt2(aa, ad, da, dd, rec_lo, rec_hi):
    """Axis 1 first, then axis 0; the approximation is cropped to the detail bands' shape first."""
    aa = aa[:ad.shape[0], :ad.shape[1]]
    t = lambda v: np.ascontiguousarray(v.T)  # noqa: E731
    lo0 = t(idwt_lines(t(aa), t(ad), rec_lo, rec_hi))
    hi0 = t(idwt_lines(t(da), t(dd), rec_lo, rec_hi))
    return idwt_lines(lo0, hi0, rec_lo, rec_hi)


# ---- noise and thresholds ---------------------------------------------------------------------------------------------------------------
def sigma_est(dd1, ppf=PPF75):
    """median(|dd1| over its non-zero entries) / ppf; None if every entry is zero (the library returns NaN there)."""
    v = sorted(abs(float(x)) for x in np.asarray(dd1).ravel() if x != 0)
    if not v:
        return None
    n = len(v)
    med = v[n // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2
    return med / ppf


def mean_squares(x):
    """mean(x * x) in the device's order (gpet_wavelet_plan.h): a partial sum per row, ascending within the row; thread t of 256
    adds the partial sums of rows t, t + 256, ... in that order; the 256 thread sums are combined by halving strides (t += t + s
    for s = 128, 64, ..., 1); the total is divided by the element count."""
    x = np.asarray(x, dtype=np.float64)
    R, Cn = x.shape
    part = [0.0] * THRESH_GROUP
    for r in range(R):
        s = 0.0
        for c in range(Cn):
            v = float(x[r, c])
            s = s + v * v
        part[r % THRESH_GROUP] = part[r % THRESH_GROUP] + s if r >= THRESH_GROUP else s
    s = THRESH_GROUP // 2
    while s:
        for t in range(s):
            part[t] = part[t] + part[t + s]
        s //= 2
    return part[0] / float(R * Cn)


def bayes_thresh(ms, var):
    return var / math.sqrt(max(ms - var, EPS))


def mean_bound(n):
    """Relative distance two summation orders of n non-negative terms can be apart, to first order: 2 (n - 1) 2^-53."""
    return 2.0 * (n - 1) * 2.0 ** -53


def shrink(x, t, mode):
    x = np.asarray(x, dtype=np.float64)
    if mode == "hard":
        return np.where(np.abs(x) < t, 0.0, x)
    with np.errstate(divide="ignore"):
        g = 1.0 - t / np.abs(x)
    return x * np.where(g > 0.0, g, 0.0)


# ---- the whole technique -----------------------------------------------------------------------------------------------------------------
def as_unit(img):
    """(float64 frame, clip the output?): integer frames times 1 / max of the type."""
    img = np.asarray(img)
    if img.dtype.kind == "u":
        return img.astype(np.float64) * (1.0 / np.iinfo(img.dtype).max), True
    return img.astype(np.float64), False


def rescaled_sigma(img, sigma):
    """sigma of an integer frame under rescale_sigma=True."""
    mx, mn = int(img.max()), int(img.min())
    inv = 1.0 / np.iinfo(img.dtype).max
    return float(sigma) * ((mx * inv - mn * inv) / float(mx - mn))


def denoise_wavelet(img, dec_lo, sigma=None, mode="soft", wavelet_levels=None, method="BayesShrink", rescale_sigma=True,
                    thresholds=None, ppf=PPF75, c=None, strict=True, return_info=False):
    """-> the denoised frame (float64); ``thresholds``: (levels, 3) to use instead of the derived ones, level 1 (finest) first,
    bands in the order ad, da, dd; ``c``: VisuShrink's sqrt(2 log(M N)) as the caller's numpy formed it.  info: sigma, var, coeffs (wavedec2's list), ms and thresholds as (levels, 3) arrays."""
    img = np.asarray(img)
    x, clip = as_unit(img)
    M, N = x.shape
    lo, hi, rec_lo, rec_hi = filters(dec_lo)
    L = levels_of((M, N), len(lo), wavelet_levels, strict)
    if sigma is not None and img.dtype.kind == "u" and rescale_sigma:
        sigma = rescaled_sigma(img, sigma)
    co = wavedec2(x, dec_lo, L)
    if sigma is None:
        sigma = sigma_est(co[0]["dd"], ppf)
        if sigma is None:
            raise ValueError("the finest diagonal band is all zero")
    sigma = float(sigma)
    var = sigma * sigma
    ms = np.full((L, 3), np.nan)
    if method == "BayesShrink":
        thr = np.empty((L, 3))
        for l in range(L):
            for b, key in enumerate(BANDS):
                ms[l, b] = mean_squares(co[l][key])
                thr[l, b] = bayes_thresh(ms[l, b], var)
    elif method == "VisuShrink":
        thr = np.full((L, 3), sigma * (math.sqrt(2 * math.log(M * N)) if c is None else float(c)))
    else:
        raise ValueError(method)
    if thresholds is not None:
        thr = np.asarray(thresholds, dtype=np.float64).reshape(L, 3)
    a = co[L - 1]["aa"]
    for l in range(L - 1, -1, -1):
        det = [shrink(co[l][key], thr[l, b], mode) for b, key in enumerate(BANDS)]
        a = idwt2(a, det[0], det[1], det[2], rec_lo, rec_hi)
    out = np.ascontiguousarray(a[:M, :N])
    if clip:
        out = np.clip(out, 0.0, 1.0)
    if return_info:
        return out, dict(sigma=sigma, var=var, coeffs=co, ms=ms, thresholds=thr, levels=L)
    return out
