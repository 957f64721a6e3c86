"""Mirror of ``gp_edge_tracing/gpet_utils.py`` for the parts on (or feeding) the hot path.

``comp_grad_img`` / ``comp_grad_imgs`` / ``normalise`` run on the GPU through libgpet_hip.so (a1), and so do ``denoise`` /
``denoise_imgs`` (a0) for the reference's 'median', 'minimum', 'gaussian', 'tvc', 'nl' (fast_mode=False), 'wavelet' (the
wavelet named) and 'tvb' (weight given), and for 'nl_fast', the reference's 'nl' with the library's default fast_mode=True;
``kernel_builder``
is host-side setup (a 11x5 table).  ``construct_test_img`` is this package's own generator of the
reference's synthetic test image recipe (gpet_utils.py:163-253).  Called like the reference (no ``seed``) it returns the
reference's own image bit for bit: scikit-image 0.18's ``random_noise(..., seed=1)`` (gpet_utils.py:251) is
``np.random.seed(1); image + np.random.normal(0, sqrt(var), shape)`` clipped to [0, 1] -- numpy's frozen legacy stream, which
needs no scikit-image (pinned by tests/golden/readme_image.npz, made by the unmodified reference under skimage 0.18.3).  With an
explicit ``seed`` the noise comes from numpy's Generator: independent images for batches.  Metrics restate gpet_utils.py:256-313.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib

_default_ctx = None


def _ctx():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = _lib.Context(0)
    return _default_ctx


def kernel_builder(size, b2d=False, normalize=False, vertical_edges=False, unit=False):
    """Sobel-like (rows x cols) edge kernel (gpet_utils.py:10-61)."""
    rows, cols = size
    mid_r, mid_c = rows // 2, cols // 2
    kernel = np.zeros(size)
    for i in range(mid_r):
        for j in range(cols):
            kernel[i, j] = 1 if unit else 1 + max(0, mid_r + 1 - abs(i - mid_r) - abs(j - mid_c))
    kernel[mid_r + 1:, :] = -kernel[0:mid_r, :][::-1]
    if b2d:
        kernel = np.flipud(kernel)
    if vertical_edges:
        kernel = kernel.T
    if normalize:
        kernel = kernel / kernel.max()
    return kernel


def normalise(img, minmax_val=(0, 1), astyp=np.float32, ctx=None):
    """float32 min-max normalisation on the GPU (gpet_utils.py:65-91)."""
    lo, hi = minmax_val
    out = (ctx or _ctx()).normalise_f32(np.asarray(img).astype(np.float32))
    if (lo, hi) != (0, 1):
        out = out * np.float32(hi - lo) + np.float32(lo)
    return out.astype(astyp)


def comp_grad_img(img, kernel, norm=True, astyp=np.float32, ctx=None):
    """Image gradient: convolution (clamp-to-edge) + ReLU + float32 min-max, one fused GPU pass
    (gpet_utils.py:95-119).  Like the reference it always normalises (``norm`` is ignored there:
    ``if normalise:`` tests the function object, gpet_utils.py:114)."""
    out = (ctx or _ctx()).grad_image(np.asarray(img, dtype=np.float64), np.asarray(kernel, dtype=np.float64))
    return out.astype(astyp)


def comp_grad_imgs(imgs, kernel, ctx=None, denoise=None, transpose=False, polar=None):
    """``comp_grad_img`` of every frame of a stack in ONE batched GPU pass (gpet_grad_images): ``imgs`` is a (T, M, N) array
    or a sequence of (M, N) frames, the result a (T, M, N) float32 array whose frame t equals ``comp_grad_img(imgs[t],
    kernel)`` bit for bit.  uint8, uint16, float32 and float64 frames go to the device as they are (integer pixels mean their
    exact float64 values); any other dtype is converted to float64 first, as ``comp_grad_img`` does with every image.
    ``denoise=(technique, kwargs)``: the frames are denoised on the device first, in the same pass -- the result equals
    ``comp_grad_imgs(denoise_imgs(imgs, technique, kwargs), kernel)`` bit for bit.
    ``kernel`` may also be a list or tuple of 2-D kernels, or a 3-D array (a 2-D array or a nested list of numbers is ONE
    kernel): the result is then (T, n_kern, M, N) and ``[t, k]`` equals ``comp_grad_imgs(imgs, kernel[k])[t]`` bit for bit, with
    and without ``denoise``; every frame is uploaded and denoised once, however many kernels read it
    (gpet_grad_images_multi).
    ``transpose=True``: the stage a vertical batch (``orientation='vertical'``) runs -- denoising and the kernel applied to the frames
    as they lie, every image stored transposed on the device: (T, N, M), or (T, n_kern, N, M), equal to the result without it with
    the last two axes swapped, bit for bit.
    ``polar=dict(centre=, n_r=, n_theta=, ...)`` (``unwrap_polar_imgs``' arguments; ``pad=None``: half the widest kernel's width): the
    frames are unwrapped to (radius x angle) on the device first -- the result equals the same call on
    ``unwrap_polar_imgs(imgs, **polar)`` bit for bit, (T, n_r, W) or (T, n_kern, n_r, W).  Not with ``transpose``."""
    if polar is not None and transpose:
        raise ValueError("polar and transpose are alternatives: a closed contour is traced as a horizontal edge of the unwrapped frame")
    kernels, multi = _lib.split_kernels(kernel)
    if not multi:
        raw = _lib.RawFrames(kernel, frames=imgs, denoise=denoise, polar=polar)  # (refuses a bad spec before a device is needed)
        return (ctx or _ctx()).grad_images(raw, transpose)
    T, K = len(imgs), len(kernels)
    raw = _lib.RawFrames(kernels, frames=imgs, denoise=denoise, slots=([t for t in range(T) for _ in range(K)], list(range(K)) * T),
                         polar=polar)
    out = (ctx or _ctx()).grad_images(raw, transpose)
    return out.reshape((T, K) + out.shape[1:])


def denoise_imgs(imgs, technique, kwargs, ctx=None, return_n_iter=False, polar=None, return_metrics=False):
    """``denoise`` of every frame of a stack in ONE batched GPU pass (gpet_denoise_images): ``imgs`` is a (T, M, N) array or a
    sequence of (M, N) frames of one dtype, the result a (T, M, N) array whose frame t equals ``denoise(imgs[t], technique,
    kwargs)`` bit for bit.  ``return_n_iter``: also the iterations 'tvc' ran per frame (0 for the filters).  'nl' with
    ``fast_mode=False``, 'nl_fast', 'wavelet' with the ``wavelet`` key and 'tvb' with ``weight`` are stages of their own
    (gpet_nlmeans_images, gpet_nlmeans_fast_images, gpet_wavelet_images, gpet_tvb_images): float64 frames whatever the frames' dtype; for 'tvb' ``return_n_iter`` gives the sweeps
    every frame ran (0 for 'nl' and 'wavelet').
    ``polar=dict(...)``: the frames are unwrapped to (radius x angle) first (``pad`` defaults to 0: there is no kernel) -- the result
    equals ``denoise_imgs(unwrap_polar_imgs(imgs, **polar), technique, kwargs)`` bit for bit.
    ``return_metrics``: also ``denoise_metrics(imgs, result)`` -- the dict comes last in the returned tuple, and equals that call bit
    for bit.  A stage of its own leaves its float64 frames on the device (``out_device_ptrs``), where they are scored before they come
    home; the in-pass techniques (median, minimum, gaussian, tvc) hand their result to the host through gpet_denoise_images, and it
    goes up again to be scored.  Not with ``polar`` (the frames as given and the result differ in shape)."""
    raw = _lib.RawFrames(None, frames=imgs, denoise=(technique, kwargs), polar=polar)  # (refuses a bad spec before a device is needed)
    if not return_metrics:
        out, n_iter = (ctx or _ctx()).denoise_images(raw)
        return (out, n_iter) if return_n_iter else out
    if polar is not None:
        raise ValueError("return_metrics scores the result against the frames as given: not with polar, which changes their shape")
    _refuse_nan(raw.frames)
    out, n_iter, fig = (ctx or _ctx()).denoise_images_scored(raw, _lib.metrics_spec())
    m = _metrics_dict(fig)
    return (out, n_iter, m) if return_n_iter else (out, m)


def _refuse_nan(frames):
    for t, f in enumerate(frames):
        if f.dtype.kind == "f" and np.isnan(f).any():
            raise ValueError("frame %d holds a NaN: the metrics of such a frame are not defined" % t)


def _metrics_dict(fig, maps=None):
    m = dict(psnr=fig[:, 0].copy(), ssim=fig[:, 1].copy(), nrmse=fig[:, 2].copy(), entropy=fig[:, 3].copy())
    if maps is not None:
        m["ssim_map"] = maps
    return m


def denoise_metrics(imgs, denoised, win_size=7, data_range=None, full=False, ctx=None, **ssim_kwargs):
    """The four figures the reference's ``denoise(..., verbose=True)`` prints (gpet_utils.py:151-156), for every frame of a stack, on
    the GPU (gpet_metrics_images): ``imgs`` the frames as given, ``denoised`` the denoised frames -- (T, M, N) arrays or sequences of
    (M, N) frames; the two stacks may differ in dtype.  Returns a dict of (T,) float64 arrays: ``psnr``
    (peak_signal_noise_ratio), ``ssim`` (structural_similarity, the library's default call: uniform window), ``nrmse``
    (normalized_root_mse, normalization='min-max') and ``entropy`` (shannon_entropy of the denoised frame), as scikit-image 0.18.3
    computes them; with ``full`` also ``ssim_map``, (T, M, N), the library's S map bit for bit.  The figures differ from the library's
    only by the order of three sums (DESIGN.md 9 has the bounds).  ``win_size`` (odd, 3 .. the smaller extent), ``data_range`` (of
    PSNR and SSIM; None: the library's rule from ``imgs``' dtype), ``K1``, ``K2``, ``use_sample_covariance`` as in the library;
    ``gaussian_weights``, ``gradient``, ``multichannel`` set True raise ValueError.  A mixed pair is scored as the library scores it:
    a uint8 frame against a float64 result in [0, 1] is compared with data_range 255 -- pass ``data_range`` (and frames of one scale)
    for figures that mean something.  Frames that hold a NaN are refused."""
    spec = _lib.metrics_spec(win_size, data_range, **ssim_kwargs)
    a, b = _lib.metrics_frames(frames=imgs), _lib.metrics_frames(frames=denoised)
    _refuse_nan(a.frames)
    _refuse_nan(b.frames)
    res = (ctx or _ctx()).metrics_images(a, b, spec, full=full)
    return _metrics_dict(*res) if full else _metrics_dict(res)


def denoise(image, technique, kwargs, plot=False, verbose=False, ctx=None):
    """The reference's ``denoise`` (gpet_utils.py:122-158) on the GPU for its four deterministic stencils: 'median' and
    'minimum' (scipy.ndimage: ``size``, ``mode``), 'gaussian' (scipy.ndimage: ``sigma``, ``truncate``, ``order=0``, ``mode``)
    and 'tvc' (scikit-image's Chambolle total variation: ``weight``, ``eps``, ``n_iter_max``); modes 'reflect' (the default) and
    'nearest'.  The result has the reference's dtype and, for uint8 / uint16 / float32 / float64 images, its values: the
    filters' bit for bit (the Gaussian taps come from the C library's exp, which differs from numpy's by one unit in the last
    place for some arguments -- visible in float64 results only), 'tvc' bit for bit with one deviation: a float32 image is
    iterated in float64 (the result is the reference's on ``image.astype(float64)``).  Images of any other dtype are converted
    to float64 first.  Any other keyword raises ValueError naming it; an
    unknown technique prints the reference's message and returns None, as the reference does.  ``plot`` is accepted and ignored
    with a warning; ``verbose`` prints the reference's four lines -- Peak-SNR, Structural Similarity, Mean Square Error (the min-max
    NRMSE), Shannon Entropy, rounded to 2, 2, 5 and 3 places -- from ``denoise_imgs(..., return_metrics=True)``.
    'nl' is scikit-image's non-local means with ``fast_mode=False`` (``patch_size``, ``patch_distance``, ``h``, ``sigma``): the
    library's classic algorithm bit for bit, in float64 -- integer frames keep their range, a float32 frame gives the library's
    result on ``image.astype(float64)``, and a candidate whose final patch distance exceeds 708 weighs 0.
    ``fast_mode=True``, the library's default and another algorithm, has a name of its own here: 'nl' without ``fast_mode=False``
    raises NotImplementedError as it always did, and 'nl_fast' (``patch_size``, ``patch_distance``, ``h``, ``sigma``) is the
    reference's ``denoise(image, 'nl', dict(kwargs, fast_mode=True))`` bit for bit, in float64 with the same two deviations
    (integer frames keep their range, a float32 frame gives the library's result on ``image.astype(float64)``); the frame's smaller
    extent must exceed ``patch_size // 2 + patch_distance + 1`` (the padding reflects once).
    'wavelet' is scikit-image's ``denoise_wavelet`` on PyWavelets (``wavelet``, ``sigma``, ``mode``, ``wavelet_levels``, ``method``,
    ``rescale_sigma``) for the orthogonal wavelets of ``_lib.wavelet_table()``, in float64: integer frames enter as x / 255,
    x / 65535 and come back clipped to [0, 1], a float32 frame gives the library's result on ``image.astype(float64)``, and the
    mean of squares under a BayesShrink threshold is summed in the device's own order (within 2 (n - 1) 2^-53 relative of numpy's;
    DESIGN.md 9) -- everything else is the library's bit for bit.  It runs only when kwargs names the ``wavelet`` key
    (``dict(wavelet='db1')`` is the library's default call); without the key 'wavelet' raises NotImplementedError as it always
    did.  A frame whose finest diagonal band is all zero raises GpetError naming the frame (the library returns NaN).
    'tvb' is scikit-image's split-Bregman ``denoise_tv_bregman`` (``weight``, ``max_iter``, ``eps``, ``isotropic``) in float64: integer
    frames enter as x / 255, x / 65535, a float32 frame gives the library's result on ``image.astype(float64)``, the result is not
    clipped.  The sweeps keep the library's raster order (one workgroup walks a frame's anti-diagonals); only the sum of squared
    changes under the stopping rule is added in the device's own order (within 2 (n - 1) 2^-53 relative of the library's;
    DESIGN.md 9), so the output is the library's bit for bit wherever the sweep counts agree.  It runs only when kwargs gives
    ``weight``, the library's required argument; without it 'tvb' raises NotImplementedError as it always did.  Frames of at least
    2 x 2 pixels whose smaller extent is at most 768."""
    if technique not in _lib.DN_OF_TECHNIQUE and technique not in _lib.PRE_STAGES:
        print("Denoising technique not implemented.")
        return None
    if plot:
        import warnings
        warnings.warn("plot is accepted for API compatibility but ignored by the GPU denoiser")
    if not verbose:
        return denoise_imgs([np.asarray(image)], technique, kwargs, ctx=ctx)[0]
    out, m = denoise_imgs([np.asarray(image)], technique, kwargs, ctx=ctx, return_metrics=True)
    psnr, ss = round(float(m["psnr"][0]), 2), round(float(m["ssim"][0]), 2)
    nmse, entropy = round(float(m["nrmse"][0]), 5), round(float(m["entropy"][0]), 3)
    print(f'Peak-SNR: {psnr}.\nStructural Similarity: {ss}.\nMean Square Error: {nmse}.\nShannon Entropy: {entropy}.\n')
    return out[0]


def construct_test_img(size, amplitude, curvature, noise_level, ltype, intensity, gaps=False, seed=None):
    """Synthetic step-edge image + ground-truth edge (yx), recipe of gpet_utils.py:163-253.  ``seed=None`` (the reference's
    signature has no seed): the reference's own noise, ``random_noise(..., seed=1)`` of scikit-image 0.18 = numpy's legacy
    ``RandomState(1).normal``; an integer: numpy ``Generator(seed)`` noise (this package's extension)."""
    M, N = size
    img = np.zeros((M, N))
    x = np.linspace(-np.pi, np.pi, N)
    A = M // 2 if amplitude > M else amplitude // 2
    cols = np.arange(N)
    wave2 = None  # second edge of the two multi-sinusoidal types (gpet_utils.py:203-220)
    if ltype in ("sinusoidal", "multi-sinusoidal", "close multi-sinusoidal"):
        wave = (np.rint(A * np.sin(N * curvature * x)) + M // 2).astype(int)
        if ltype != "sinusoidal":
            wave2 = wave + (A // 2 if ltype == "multi-sinusoidal" else A // 6)
    elif ltype == "co-sinusoidal":
        wave = (np.rint(A * np.cos(N * curvature * x)) + M // 2).astype(int)
    elif ltype == "diag":
        wave = cols.copy()
    elif ltype == "straight":
        wave = np.full(N, M // 2, dtype=int)
    else:
        raise ValueError("ltype must be one of sinusoidal, multi-sinusoidal, close multi-sinusoidal, co-sinusoidal, "
                         "diag, straight")
    rows = np.arange(M)[:, None]
    img[rows >= wave[None, :]] = intensity
    if wave2 is not None:  # the band below the second edge is 1 - intensity
        img[rows >= wave2[None, :]] = 1 - intensity
    if gaps:
        img[:, 20:30] = 0
        img[:, N // 2:(N // 2 + 10)] = 0
        img[:, N - 100:N - 90] = 0
        img[:, N // 4:(N // 4 + 20)] = 0
    if seed is None:  # gpet_utils.py:251 under scikit-image 0.18: np.random.seed(1); np.random.normal(mean, var ** 0.5, shape)
        noise = np.random.RandomState(1).normal(0.0, noise_level ** 0.5, img.shape)
    else:
        noise = np.random.default_rng(seed).normal(0.0, math.sqrt(noise_level), img.shape)
    img = np.clip(img + noise, 0.0, 1.0)
    edge = np.stack([wave, cols], axis=1)
    if wave2 is not None:  # both edges, one after the other (2N rows), as the reference returns them
        edge = np.concatenate([edge, np.stack([wave2, cols], axis=1)], axis=0)
    return img, edge


def trace_MSE(edge_pred, edge_true):
    n = edge_pred.shape[0]
    return np.round((1 / n) * np.sum((edge_pred.reshape(n, -1)[:, 0] - edge_true[:, 0]) ** 2), 4)


def trace_relarea(edge_pred, edge_true):
    n = edge_pred.shape[0]
    ta = np.sum(n - edge_true[:, 0]) / n ** 2
    pa = np.sum(n - edge_pred.reshape(n, -1)[:, 0]) / n ** 2
    return np.round(np.abs((ta - pa) / ta), 5)


def trace_dicecoef(edge_pred, edge_true, jaccard=False):
    n = edge_pred.shape[0]
    rows = np.arange(n)[:, None]
    pb = (rows >= edge_pred.reshape(n, -1)[:, 0].astype(int)[None, :]).astype(float)
    tb = (rows >= edge_true[:, 0].astype(int)[None, :]).astype(float)
    jacc = np.sum(pb * tb) / np.sum(np.clip(pb + tb, 0, 1))
    return np.round(jacc, 4) if jaccard else np.round(2 * jacc / (jacc + 1), 4)


# ---- closed contours: the polar unwrap (csrc/gpet_polar_plan.h) -----------------------------------------------------
def unwrap_polar_imgs(frames, centre, n_r, n_theta, r0=0.0, dr=1.0, theta0=0.0, pad=0, ctx=None):
    """Every frame of a stack resampled to (radius x angle) around ``centre`` in ONE batched GPU pass (gpet_polar_images):
    ``frames`` is a (T, M, N) array or a sequence of (M, N) frames (uint8, uint16, float32 and float64 go to the device as they are),
    ``centre`` = (cx, cy) -- x the column, y the row -- or a (T, 2) array with one centre per frame; the result is (T, n_r, W)
    float64 with W = n_theta + 1 + 2 pad.  Row i is the radius ``r0 + i dr``; column c the angle ``theta0 + 2 pi a / n_theta`` with
    a = (c - pad) mod n_theta, clockwise on the screen: columns ``pad`` and ``pad + n_theta`` are the same ray (the seam), and the
    ``pad`` columns either side repeat the far end, so a filter sees periodic data there.  Bilinear, a ray that leaves the frame
    repeats the border pixel; integer frames keep their range.  A closed, roughly star-shaped contour around the centre is a
    horizontal edge of the result: trace it between ``closed_init(row, polar)``."""
    raw = _lib.RawFrames(None, frames=frames, polar=dict(centre=centre, n_r=n_r, n_theta=n_theta, r0=r0, dr=dr, theta0=theta0, pad=pad))
    return (ctx or _ctx()).polar_images(raw)


def closed_init(row, polar):
    """The two init points that close a contour traced on polar frames: ``[[pad, row], [pad + n_theta, row]]`` -- the same ray at
    both ends of the traced columns, pinned to one radius row.  ``polar``: the dict (``pad`` given) or a resolved ``_lib.PolarSpec``."""
    sp = _lib.polar_spec(polar)
    if sp.pad is None:
        raise ValueError("closed_init needs pad: give it in the dict, or pass the resolved spec (the tracing object's .polar)")
    return np.array([[sp.pad, int(row)], [sp.pad + sp.n_theta, int(row)]], dtype=np.int64)


def polar_to_xy(rows, cols, polar, frame=0, shape=None):
    """Frame coordinates (x, y), float64, of the polar pixels (rows, cols) by the rule's own arithmetic (csrc/gpet_polar_plan.h):
    rho = r0 + row dr; x = cx + rho cos_t[a]; y = cy + rho sin_t[a]; a = (col - pad) mod n_theta.  Host numpy.  ``rows`` may be
    fractional (an interval curve).  ``frame``: whose centre, where there is one per frame.  ``shape`` = (M, N) of the frames: the
    positions are clamped into the frame as the unwrap clamps them; without it they are the ray's own, which is the same wherever
    the ray stays inside the frame."""
    sp = _lib.polar_spec(polar)
    if sp.pad is None:
        raise ValueError("polar_to_xy needs pad: give it in the dict, or pass the resolved spec (the tracing object's .polar)")
    rows, cols = np.asarray(rows, dtype=np.float64), np.asarray(cols, dtype=np.int64)
    a = np.mod(cols - sp.pad, sp.n_theta)
    cx, cy = sp.centre[0 if sp.centre.shape[0] == 1 else int(frame)]
    rho = sp.r0 + rows * sp.dr
    x, y = cx + rho * sp.cos_t[a], cy + rho * sp.sin_t[a]
    if shape is not None:
        x, y = np.minimum(np.maximum(x, 0.0), shape[1] - 1.0), np.minimum(np.maximum(y, 0.0), shape[0] - 1.0)
    return x, y


def polar_trace_xy(result, polar, frame=0):
    """What a tracer returned on polar frames, in frame coordinates: a trace -- an (n, 2) array of (row, column) -- becomes an (n, 2)
    float64 array of (x, y); with ``return_std`` the result is ``(trace, (lower, upper))`` and the two interval curves, radii rows
    indexed like the trace, are mapped along the trace's rays: ``(xy, (xy_lower, xy_upper))``."""
    if isinstance(result, tuple):
        trace, (lower, upper) = result
        cols = np.asarray(trace)[:, 1]
        return (polar_trace_xy(trace, polar, frame), tuple(np.stack(polar_to_xy(np.asarray(c).reshape(-1), cols, polar, frame), axis=1)
                                                           for c in (lower, upper)))
    trace = np.asarray(result)
    return np.stack(polar_to_xy(trace[:, 0], trace[:, 1], polar, frame), axis=1)


# ---- label maps: traces rasterised into masks on the device (csrc/gpet_label_plan.h) -----------------------------------
def _trace_list(traces):
    if isinstance(traces, np.ndarray) and traces.ndim == 2:
        return [traces]
    return [np.asarray(t) for t in traces]


def label_maps(traces, shape, map_of=None, extend=False, thickness=False, transpose=False, ctx=None):
    """The regions between traced edges as uint8 label maps, made on the GPU (gpet_label_maps; Rule 1 of include/gpet_hip.h "label
    maps").  ``traces``: one (Lg, 2) yx trace as every tracer returns it, or a list of them -- consecutive columns, the rows integers;
    ``shape`` = (M, N) of the frame; ``map_of[e]`` the map edge e goes on, -1 for none (None: all edges on one map).  Returns
    (n_maps, M, N) uint8 with ``label[f, r, c]`` = the number of edges of map f whose row at column c is <= r: for one edge the
    reference's ``pred_bin`` (gpet_utils.py:303-307, "at or below the trace"), for E stacked edges the layer index 0 .. E; edges may
    cross.  Rows outside the frame are clamped, ``_lib.LABEL_NO_ROW`` does not count.  A column outside an edge's grid is not counted
    for it -- with ``extend`` the edge's first / last row is used there.  ``thickness``: also (n_maps, L + 1, N) int32, the number of
    rows of label l in every column (its sum over the columns is the layer's area), L the most edges on one map.
    ``transpose``: the traces are those of vertical edges -- (row, column) of the frame, one entry per consecutive row -- and
    ``label[f, r, c]`` counts the edges whose column at row r is <= c; the thickness is then per frame row."""
    tr = _trace_list(traces)
    M, N = int(shape[0]), int(shape[1])
    a, b = (1, 0) if transpose else (0, 1)  # (the traced coordinate, the grid coordinate)
    for e, t in enumerate(tr):
        if t.ndim != 2 or t.shape[1] != 2 or t.shape[0] < 1:
            raise ValueError("trace %d has shape %s, not (Lg, 2)" % (e, t.shape))
        if not np.array_equal(t[:, b], t[0, b] + np.arange(t.shape[0])):
            raise ValueError("trace %d does not run over consecutive %s" % (e, "rows" if transpose else "columns"))
    out = (ctx or _ctx()).label_maps((N, M) if transpose else (M, N), [int(t[0, b]) for t in tr], [t[:, a] for t in tr], map_of, extend=extend,
                                     transposed=transpose, thickness=thickness)
    return out


def outline_label_maps(outlines_xy, shape, map_of=None, ctx=None):
    """The inside of closed outlines as uint8 label maps, made on the GPU (gpet_label_maps_xy; Rule 2 of include/gpet_hip.h "label
    maps").  ``outlines_xy``: one (n, 2) float64 array of (x, y) vertices in frame coordinates, 4 <= n <= 4096, or a list of them --
    for instance ``polar_trace_xy(result, polar)[:-1]`` (the seam's second column repeats the first vertex); ``shape`` = (Ms, Ns).
    Returns (n_maps, Ms, Ns) uint8: how many outlines of its map the pixel (x = column, y = row) lies inside by the even-odd rule --
    two nested outlines give lumen 2, wall 1, outside 0.  An outline with a vertex that is not finite contributes nothing."""
    outs = _trace_list(outlines_xy)
    return (ctx or _ctx()).label_maps_xy(shape, outs, map_of)
