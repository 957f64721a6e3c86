"""ctypes binding of libgpet_hip.so (include/gpet_hip.h).

The HIP library is the product's only compute path: if it is missing or fails to load this
module raises -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GPET_LIB_PATH") or os.path.join(_HERE, "libgpet_hip.so")  # (override: instrumented builds)

# status codes (gpet_status)
OK, ERR_BAD_ARG, ERR_HIP, ERR_NOT_PD, ERR_ITER_CAP, ERR_RANK_CAP, ERR_UNSUPPORTED, ERR_NO_DEVICE, ERR_STATE = range(9)

# gpet_buf
(BUF_X_TRAIN, BUF_Y_TRAIN, BUF_CHOL, BUF_ALPHA, BUF_MEAN, BUF_STD, BUF_COV, BUF_FACTOR, BUF_EIGVALS, BUF_NORMALS,
 BUF_SAMPLES, BUF_COSTS, BUF_BEST_IDX, BUF_BEST_COSTS, BUF_SCALARS, BUF_OBS, BUF_KDE, BUF_GRAD_KDE, BUF_GRAD,
 BUF_NOISE_W, BUF_FIN_TRAIN, BUF_FIN_PAR, BUF_FIN_STARTS, BUF_FIN_OUT, BUF_KDE_TILES, BUF_STRUCT_Q0, BUF_STRUCT_LAM0,
 BUF_STRUCT_H) = range(28)

KERNEL_RBF, KERNEL_MATERN = 0, 1
GRAD_ON_DEVICE = 1  # gpet_batch_create2 / gpet_batch_set_images flag: the gradient image pointers are device pointers
IMAGES_NEXT_FRAME = 2  # gpet_batch_set_images: the images continue the sequences just traced
RAW_ON_DEVICE = 4  # gpet_grad_images / gpet_batch_create_raw / gpet_batch_set_raw_images: the frame pointers are device pointers
FRAMES_TRANSPOSED = 16  # the raw-frame calls and every batch creation with flags: a vertical batch -- frames in frame layout, images and batch shape (N, M)
# pixel types of raw frames (GPET_PIX_*): the dtypes that go to the device as they are
PIX_U8, PIX_U16, PIX_F32, PIX_F64 = range(4)
PIX_BYTES = (1, 2, 4, 8)
PIX_OF_DTYPE = {np.dtype(np.uint8): PIX_U8, np.dtype(np.uint16): PIX_U16, np.dtype(np.float32): PIX_F32,
                np.dtype(np.float64): PIX_F64}


# denoising techniques / boundary modes of gpet_denoise (GPET_DN_*, GPET_DN_MODE_*)
DN_NONE, DN_MEDIAN, DN_MINIMUM, DN_GAUSSIAN, DN_TVC = range(5)
DN_OF_TECHNIQUE = {"median": DN_MEDIAN, "minimum": DN_MINIMUM, "gaussian": DN_GAUSSIAN, "tvc": DN_TVC}
DN_MODE_OF_NAME = {"reflect": 0, "nearest": 1}
DN_WINDOW_MAX = 81


class GpetDenoise(C.Structure):
    _fields_ = [("technique", C.c_int32), ("size_y", C.c_int32), ("size_x", C.c_int32), ("mode", C.c_int32),
                ("sigma_y", C.c_double), ("sigma_x", C.c_double), ("truncate", C.c_double), ("weight", C.c_double),
                ("eps", C.c_double), ("n_iter_max", C.c_int32)]


def _dn_pair(v, conv, name):
    if np.ndim(v) == 0:
        return conv(v), conv(v)
    v = list(v)
    if len(v) != 2:
        raise ValueError("denoise: %r must be a scalar or one value per image axis, not %r" % (name, v))
    return conv(v[0]), conv(v[1])


def denoise_spec(denoise):
    """``(technique, kwargs)`` as gpet_utils.denoise takes them -> GpetDenoise, decided from the arguments alone (no device).
    kwargs carry scipy's / scikit-image's own names: ``size`` and ``mode`` for 'median' / 'minimum'; ``sigma``, ``truncate``,
    ``order`` (0 only) and ``mode`` for 'gaussian'; ``weight``, ``eps`` and ``n_iter_max`` for 'tvc'.  ValueError names a key
    the device does not take (footprint, origin, cval, multichannel, ...) or a value it refuses; NotImplementedError names a
    technique that is a stage of its own and no gpet_denoise technique (PRE_STAGES).  A GpetDenoise passes through; None stays None."""
    if denoise is None or isinstance(denoise, GpetDenoise):
        return denoise
    try:
        technique, kwargs = denoise
    except (TypeError, ValueError):
        raise ValueError("denoise must be a (technique, kwargs) pair")
    if technique in PRE_STAGES:  # (a stage of its own: RawFrames takes it through the stage's from_kwargs)
        raise NotImplementedError(PRE_STAGES[technique].not_a_filter)
    if technique not in DN_OF_TECHNIQUE:
        raise ValueError("unknown denoising technique %r" % (technique,))
    kw = dict(kwargs or {})
    allowed = {"median": ("size", "mode"), "minimum": ("size", "mode"), "gaussian": ("sigma", "truncate", "order", "mode"),
               "tvc": ("weight", "eps", "n_iter_max")}[technique]
    for k in kw:
        if k not in allowed:
            raise ValueError("denoise: keyword %r of %r is not supported on the device (supported: %s)"
                             % (k, technique, ", ".join(allowed)))
    d = GpetDenoise(technique=DN_OF_TECHNIQUE[technique], size_y=0, size_x=0, mode=0, sigma_y=0.0, sigma_x=0.0, truncate=4.0,
                    weight=0.1, eps=2.0e-4, n_iter_max=200)
    if "mode" in kw:
        if kw["mode"] not in DN_MODE_OF_NAME:
            raise ValueError("denoise: mode %r is not supported on the device (supported: reflect, nearest)" % (kw["mode"],))
        d.mode = DN_MODE_OF_NAME[kw["mode"]]
    if technique in ("median", "minimum"):
        if "size" not in kw:
            raise ValueError("denoise: %r needs size" % (technique,))
        d.size_y, d.size_x = _dn_pair(kw["size"], int, "size")
        if d.size_y < 1 or d.size_x < 1 or d.size_y * d.size_x > DN_WINDOW_MAX:
            raise ValueError("denoise: size %r: windows of 1 to %d pixels (9 x 9) are built" % (kw["size"], DN_WINDOW_MAX))
    elif technique == "gaussian":
        if "sigma" not in kw:
            raise ValueError("denoise: 'gaussian' needs sigma")
        if np.ndim(kw.get("order", 0)) != 0 or kw.get("order", 0) != 0:
            raise ValueError("denoise: order %r is not supported on the device (0 only)" % (kw["order"],))
        d.sigma_y, d.sigma_x = _dn_pair(kw["sigma"], float, "sigma")
        d.truncate = float(kw.get("truncate", 4.0))
        if not (d.sigma_y > 0 and d.sigma_x > 0 and d.truncate > 0):
            raise ValueError("denoise: sigma and truncate must be above 0")
    else:
        d.weight = float(kw.get("weight", 0.1))
        d.eps = float(kw.get("eps", 2.0e-4))
        d.n_iter_max = int(kw.get("n_iter_max", 200))
        if not d.weight > 0 or not d.eps >= 0 or d.n_iter_max < 1:
            raise ValueError("denoise: weight must be above 0, eps not negative, n_iter_max at least 1")
    return d


def denoised_dtype(dn, pix):
    """numpy dtype of a denoised frame of pixel type ``pix``: the frame's own for the filters, float64 for 'tvc'."""
    if dn.technique == DN_TVC:
        return np.dtype(np.float64)
    return [dt for dt, code in PIX_OF_DTYPE.items() if code == pix][0]


class PreSpec(object):
    """What the specs of the stages of their own share (PRE_STAGES below).  Every such class says: ``technique`` its name in
    gpet_utils.denoise, ``symbol`` the library call, ``out_on_device`` that call's flag for device outputs, ``not_a_filter`` what
    denoise_spec answers for the technique, ``from_kwargs`` (kwargs -> spec; the module function of the stage) -- and may replace
    the three defaults here.  ``c`` is the C struct of the call."""
    reports_n_iter = False  # the call ends with an int32 n_iter[] (or null) behind out[]

    def check_frames(self, shape):
        """Refuses (M, N) frames the stage does not take, before a device is needed (ValueError); by default none."""

    def arg(self):
        return C.byref(self.c)

    def call_arg(self, T, shape):
        """-> (the spec argument of a call on T frames of ``shape``, what must stay alive while it runs)."""
        return C.byref(self.c), None


# non-local means (gpet_nlmeans, GPET_NLM_*): a stage of its own in front of the raw-frame path, not a gpet_denoise technique
NLM_OUT_ON_DEVICE = 8  # gpet_nlmeans_images: out[] are device pointers
NLM_PATCH_MAX, NLM_DIST_MAX = 15, 31
NLM_KEYS = ("patch_size", "patch_distance", "h", "sigma", "fast_mode", "multichannel")


class GpetNlmeans(C.Structure):
    _fields_ = [("patch_size", C.c_int32), ("patch_distance", C.c_int32), ("h", C.c_double), ("sigma", C.c_double),
                ("taps", C.c_void_p)]


def nlmeans_taps(patch_size, h):
    """The Gaussian patch weights of scikit-image's classic non-local means, formed with numpy exactly as the library forms them:
    ``exp(-(x_a^2 + x_b^2) / (2 A^2))`` over ``x = -off .. off`` with ``A = (s - 1) / 4``, times ``1 / (sum * h * h)`` -> (s, s)."""
    s = int(patch_size) + (1 if int(patch_size) % 2 == 0 else 0)
    off = s // 2
    A = (s - 1.0) / 4.0
    x = np.arange(-off, off + 1, dtype=np.float64)
    xr, xc = np.meshgrid(x, x, indexing="ij")
    w = np.ascontiguousarray(np.exp(-(xr * xr + xc * xc) / (2 * A * A)))
    w *= 1.0 / (np.sum(w) * h * h)
    return w


class NlmeansSpec(PreSpec):
    """What nlmeans_spec returns: ``c`` the gpet_nlmeans of the call, ``taps`` the (s, s) float64 array it points to (kept alive
    here), ``s`` the odd patch extent."""
    technique, symbol, out_on_device = "nl", "gpet_nlmeans_images", NLM_OUT_ON_DEVICE
    not_a_filter = ("denoising technique 'nl' is no gpet_denoise technique: with fast_mode=False it is built as a "
                    "stage of its own (nlmeans_spec, Context.nlmeans_images); fast_mode=True is not built under "
                    "this name: it is the technique 'nl_fast' (nlmeans_fast_spec, Context.nlmeans_fast_images)")

    def __init__(self, patch_size, patch_distance, h, sigma, taps):
        self.s = patch_size + (1 if patch_size % 2 == 0 else 0)
        self.taps = np.ascontiguousarray(taps, dtype=np.float64)
        self.c = GpetNlmeans(patch_size=patch_size, patch_distance=patch_distance, h=h, sigma=sigma, taps=self.taps.ctypes.data)


def nlmeans_spec(kwargs, taps=None):
    """The keyword arguments of ``gpet_utils.denoise(image, 'nl', kwargs)`` = scikit-image's ``denoise_nl_means`` -> NlmeansSpec,
    decided from the arguments alone (no device): ``patch_size`` (7), ``patch_distance`` (11), ``h`` (0.1), ``sigma`` (0.0),
    ``fast_mode`` and ``multichannel=False``.  Only the classic algorithm is built: a missing or true ``fast_mode`` (the library's
    default, another algorithm) raises NotImplementedError.  Any other key raises ValueError naming it, and so does a value the
    device refuses.  ``taps``: (s, s) patch weights to use instead of the ones nlmeans_taps derives (a numpy whose exp differs in
    the last place gives taps one unit apart; tests inject a fixture's)."""
    kw = dict(kwargs or {})
    for k in kw:
        if k not in NLM_KEYS:
            raise ValueError("denoise: keyword %r of 'nl' is not supported on the device (supported: %s)" % (k, ", ".join(NLM_KEYS)))
    if kw.get("fast_mode", True):
        raise NotImplementedError("denoising technique 'nl' is built for fast_mode=False only (scikit-image's classic non-local "
                                  "means); fast_mode=True, the library's default, is another algorithm and not built for the "
                                  "device: pass fast_mode=False (the fast algorithm is the technique 'nl_fast')")
    if kw.get("multichannel", False):
        raise ValueError("denoise: multichannel=True of 'nl' is not supported on the device (frames are 2-D, single-channel)")
    ps, d = int(kw.get("patch_size", 7)), int(kw.get("patch_distance", 11))
    h, sigma = float(kw.get("h", 0.1)), float(kw.get("sigma", 0.0))
    s = ps + (1 if ps % 2 == 0 else 0)
    if ps < 2 or s > NLM_PATCH_MAX:
        raise ValueError("denoise: patch_size %r: patches of 3 x 3 to %d x %d pixels are built" % (ps, NLM_PATCH_MAX, NLM_PATCH_MAX))
    if d < 0 or d > NLM_DIST_MAX:
        raise ValueError("denoise: patch_distance %r: distances of 0 to %d are built" % (d, NLM_DIST_MAX))
    if not (h > 0 and np.isfinite(h)) or not (sigma >= 0 and np.isfinite(sigma)):
        raise ValueError("denoise: h must be above 0 and sigma not negative")
    if taps is None:
        taps = nlmeans_taps(s, h)
    taps = np.ascontiguousarray(taps, dtype=np.float64)
    if taps.shape != (s, s):
        raise ValueError("denoise: the taps of a %d x %d patch are an array of that shape, not %r" % (s, s, taps.shape))
    return NlmeansSpec(ps, d, h, sigma, taps)


# fast-mode non-local means (gpet_nlmeans_fast): scikit-image's DEFAULT denoise_nl_means, the technique 'nl_fast'; a stage of its
# own with the classic stage's flags and keys
NLF_STRIP = 64  # rows a wave takes at a time (gpet_nlfast_plan.h: NLF_STRIP)
NLF_CHUNK_BUDGET = 256 << 20  # bytes a chunk's workspaces and staging stay inside (gpet_nlfast_plan.h: NLF_CHUNK_BUDGET)


class GpetNlmeansFast(C.Structure):
    _fields_ = [("patch_size", C.c_int32), ("patch_distance", C.c_int32), ("h", C.c_double), ("sigma", C.c_double)]


class NlmeansFastSpec(PreSpec):
    """What nlmeans_fast_spec returns: ``c`` the gpet_nlmeans_fast of the call, ``s`` the odd patch extent."""
    technique, symbol, out_on_device = "nl_fast", "gpet_nlmeans_fast_images", NLM_OUT_ON_DEVICE
    not_a_filter = ("denoising technique 'nl_fast' is no gpet_denoise technique: it is built as a stage of its own "
                    "(nlmeans_fast_spec, Context.nlmeans_fast_images)")

    def __init__(self, patch_size, patch_distance, h, sigma):
        self.s = patch_size + (1 if patch_size % 2 == 0 else 0)
        self.c = GpetNlmeansFast(patch_size=patch_size, patch_distance=patch_distance, h=h, sigma=sigma)


def nlmeans_fast_spec(kwargs):
    """The keyword arguments of ``gpet_utils.denoise(image, 'nl_fast', kwargs)`` -> NlmeansFastSpec, decided from the arguments
    alone (no device).  'nl_fast' is the reference's ``denoise(image, 'nl', dict(kwargs, fast_mode=True))`` = scikit-image's
    ``denoise_nl_means`` as the library runs it by default: ``patch_size`` (7), ``patch_distance`` (11), ``h`` (0.1), ``sigma``
    (0.0); ``fast_mode`` only as true and ``multichannel`` only as false.  Any other key raises ValueError naming it, and so does
    a value the device refuses; ``fast_mode=False`` raises a ValueError that points to 'nl', the classic algorithm."""
    kw = dict(kwargs or {})
    for k in kw:
        if k not in NLM_KEYS:
            raise ValueError("denoise: keyword %r of 'nl_fast' is not supported on the device (supported: %s)" % (k, ", ".join(NLM_KEYS)))
    if not kw.get("fast_mode", True):
        raise ValueError("denoise: fast_mode=False of 'nl_fast': the technique is the library's fast algorithm; the classic one "
                         "is the technique 'nl' with fast_mode=False")
    if kw.get("multichannel", False):
        raise ValueError("denoise: multichannel=True of 'nl_fast' is not supported on the device (frames are 2-D, single-channel)")
    for k in ("patch_size", "patch_distance"):
        if k in kw and not (np.ndim(kw[k]) == 0 and int(kw[k]) == kw[k]):
            raise ValueError("denoise: %s %r of 'nl_fast': a whole number" % (k, kw[k]))
    for k in ("h", "sigma"):
        if k in kw and np.ndim(kw[k]) != 0:
            raise ValueError("denoise: %s %r of 'nl_fast': one number" % (k, kw[k]))
    ps, d = int(kw.get("patch_size", 7)), int(kw.get("patch_distance", 11))
    h, sigma = float(kw.get("h", 0.1)), float(kw.get("sigma", 0.0))
    s = ps + (1 if ps % 2 == 0 else 0)
    if ps < 2 or s > NLM_PATCH_MAX:
        raise ValueError("denoise: patch_size %r of 'nl_fast': patches of 3 x 3 to %d x %d pixels are built" % (ps, NLM_PATCH_MAX, NLM_PATCH_MAX))
    if d < 0 or d > NLM_DIST_MAX:
        raise ValueError("denoise: patch_distance %r of 'nl_fast': distances of 0 to %d are built" % (d, NLM_DIST_MAX))
    if not (h > 0 and np.isfinite(h)):
        raise ValueError("denoise: h %r of 'nl_fast': one finite number above 0" % (h,))
    if not (sigma >= 0 and np.isfinite(sigma)):
        raise ValueError("denoise: sigma %r of 'nl_fast': one finite number, not negative" % (sigma,))
    return NlmeansFastSpec(ps, d, h, sigma)


def nlmeans_fast_plan(M, N, s, d, budget=NLF_CHUNK_BUDGET):
    """A mirror of gpet_nlfast_plan.h's nlf_plan for M x N frames, odd patch extent ``s`` and distance ``d`` -> dict: ``pad``,
    ``nr`` x ``nc`` the padded frame, ``n_shifts`` = (2 d + 1)(d + 1), ``rows_per_group`` whole rows of d + 1 shifts whose integral
    images a frame's workspace holds at a time (0: not one fits ``budget``), ``n_groups``, ``strips`` of NLF_STRIP rows,
    ``frame_bytes`` of workspace (the padded frame, two accumulators of M N and the group's planes, float64, to 256 bytes) and
    ``frames_per_chunk`` when nothing is staged."""
    M, N, s, d = int(M), int(N), int(s), int(d)
    pad = s // 2 + d + 1
    nr, nc = M + 2 * pad, N + 2 * pad
    plane = nr * nc

    def frame_bytes(rows):
        return ((plane + 2 * M * N + rows * (d + 1) * plane) * 8 + 255) & ~255

    rows = 0
    while rows < 2 * d + 1 and frame_bytes(rows + 1) <= budget:
        rows += 1
    fb = frame_bytes(max(rows, 1))
    return dict(pad=pad, nr=nr, nc=nc, n_shifts=(2 * d + 1) * (d + 1), rows_per_group=rows, n_groups=-(-(2 * d + 1) // rows) if rows else 0,
                strips=-(-nr // NLF_STRIP), frame_bytes=fb, frames_per_chunk=max(1, min(budget // fb, 65535)))


# wavelet denoising (gpet_wavelet, GPET_WV_*): the second stage of its own in front of the raw-frame path
WV_OUT_ON_DEVICE = 8  # gpet_wavelet_images: out[] are device pointers
WV_TAPS_MAX, WV_LEVELS_MAX = 16, 16
WV_MODES = {"soft": 0, "hard": 1}
WV_METHODS = {"BayesShrink": 0, "VisuShrink": 1}
WV_PPF75 = 0.6744897501960817  # scipy.stats.norm.ppf(0.75)
WV_KEYS = ("sigma", "wavelet", "mode", "wavelet_levels", "method", "rescale_sigma", "multichannel", "convert2ycbcr")
WV_TABLE_PATH = os.path.join(_HERE, "wavelet_table.json")
_wv_table = None


class GpetWavelet(C.Structure):
    _fields_ = [("n_taps", C.c_int32), ("levels", C.c_int32), ("mode", C.c_int32), ("method", C.c_int32),
                ("dec_lo", C.c_double * 16), ("sigma", C.c_double), ("rescale_sigma", C.c_int32), ("n_thresholds", C.c_int32),
                ("ppf", C.c_double), ("c", C.c_double), ("thresholds", C.c_void_p), ("sigma_out", C.c_void_p),
                ("thresholds_out", C.c_void_p), ("mean_sq_out", C.c_void_p), ("coeffs_out", C.c_void_p)]


def wavelet_table():
    """name -> dec_lo (list of floats) of the orthogonal wavelets the package carries (wavelet_table.json: PyWavelets' tables,
    written by tests/golden/make_wavelet_fixture.py with 17 significant digits)."""
    global _wv_table
    if _wv_table is None:
        import json
        with open(WV_TABLE_PATH) as f:
            _wv_table = {k: [float(v) for v in taps] for k, taps in json.load(f).items()}
    return _wv_table


def wavelet_max_level(n, n_taps):
    """The largest L with (F - 1) * 2^L <= n (PyWavelets' dwt_max_level); 0 if there is none."""
    L = 0
    while (n_taps - 1) * 2 ** (L + 1) <= n:
        L += 1
    return L


def wavelet_out_len(n, n_taps):
    return (n + n_taps - 1) // 2


class WaveletSpec(PreSpec):
    """What wavelet_spec returns: ``c`` the gpet_wavelet of the call without what depends on the frames (VisuShrink's constant,
    the injected thresholds: for_frames fills them in), ``name`` the wavelet, ``thresholds`` the injected table or None."""
    technique, symbol, out_on_device = "wavelet", "gpet_wavelet_images", WV_OUT_ON_DEVICE
    not_a_filter = ("denoising technique 'wavelet' is no gpet_denoise technique: it is built as a stage of its own "
                    "(wavelet_spec, Context.wavelet_images) and runs when kwargs names the wavelet, e.g. "
                    "dict(wavelet='db1')")

    def __init__(self, name, dec_lo, levels, mode, method, sigma, rescale_sigma, thresholds=None, ppf=WV_PPF75):
        self.name, self.dec_lo = name, [float(v) for v in dec_lo]
        self.thresholds = None if thresholds is None else np.ascontiguousarray(thresholds, dtype=np.float64)
        self.c = GpetWavelet(n_taps=len(self.dec_lo), levels=levels, mode=mode, method=method,
                             dec_lo=(C.c_double * 16)(*self.dec_lo), sigma=sigma, rescale_sigma=int(rescale_sigma), ppf=ppf)

    def levels_on(self, shape):
        """The levels this spec means on (M, N) frames: its own, or max(max_level - 3, 1); ValueError for a frame the filter does
        not fit and for an explicit value above max_level."""
        top = wavelet_max_level(min(int(shape[0]), int(shape[1])), self.c.n_taps)
        if top < 1:
            raise ValueError("denoise: frames of %d x %d are below the reach of wavelet %r (%d taps): max_level is 0"
                             % (shape[0], shape[1], self.name, self.c.n_taps))
        if self.c.levels > top:
            raise ValueError("denoise: wavelet_levels %d is above max_level %d of %d x %d frames under wavelet %r (the largest L with "
                             "(F - 1) 2^L <= min(M, N))" % (self.c.levels, top, shape[0], shape[1], self.name))
        L = self.c.levels if self.c.levels > 0 else max(top - 3, 1)
        if L > WV_LEVELS_MAX:
            raise ValueError("denoise: more than %d wavelet levels are not built" % WV_LEVELS_MAX)
        return L

    def pyramid(self, shape):
        """[(mo, no, offset in doubles)] per level, finest first, and the doubles of one frame's pyramid (gpet_wavelet_plan.h:
        wv_plan): a level's bands aa, ad, da, dd lie one after the other from its offset."""
        m, n, off, out = int(shape[0]), int(shape[1]), 0, []
        for _ in range(self.levels_on(shape)):
            m, n = wavelet_out_len(m, self.c.n_taps), wavelet_out_len(n, self.c.n_taps)
            out.append((m, n, off))
            off += 4 * m * n
        return out, off

    def for_frames(self, T, shape):
        """-> (gpet_wavelet of a call on T frames of ``shape``, what must stay alive as long as it is used)."""
        L = self.levels_on(shape)
        c = GpetWavelet.from_buffer_copy(self.c)
        c.c = float(np.sqrt(2 * np.log(int(shape[0]) * int(shape[1]))))  # (as skimage forms it: numpy's log and sqrt)
        keep = None
        if self.thresholds is not None:
            t = self.thresholds.reshape(-1, 3) if self.thresholds.size % 3 == 0 else self.thresholds.reshape(-1, 1)
            if t.shape == (L, 3):
                t = np.tile(t, (T, 1))
            if t.shape != (T * L, 3):
                raise ValueError("denoise: injected thresholds are (levels, 3) or (frames, levels, 3) = (%d, %d, 3), not %r"
                                 % (T, L, self.thresholds.shape))
            keep = np.ascontiguousarray(t)
            c.thresholds, c.n_thresholds = keep.ctypes.data, keep.size
        return c, keep

    check_frames = levels_on  # (refuses levels the frames do not allow)
    call_arg = for_frames


def wavelet_spec(kwargs, thresholds=None):
    """The keyword arguments of ``gpet_utils.denoise(image, 'wavelet', kwargs)`` = scikit-image's ``denoise_wavelet`` ->
    WaveletSpec, decided from the arguments alone (no device): ``wavelet`` (a name of wavelet_table()), ``sigma`` (None: estimated
    per frame), ``mode`` ('soft' / 'hard'), ``wavelet_levels`` (None: max(max_level - 3, 1)), ``method`` ('BayesShrink' /
    'VisuShrink'), ``rescale_sigma`` (True); ``multichannel`` and ``convert2ycbcr`` only as False.  THE ``wavelet`` KEY MUST BE
    SPELLED OUT: kwargs without it raise NotImplementedError, as 'wavelet' did before the stage was built (the library's default
    would be 'db1').  Any other key raises ValueError naming it, and so does a wavelet that is not in the table (biorthogonal ones
    among them) or a value the device refuses.  ``thresholds``: (levels, 3) or (frames, levels, 3) thresholds to use instead of
    the derived ones -- level 1 (the finest) first, bands ad, da, dd; tests inject a fixture's, because the mean of squares under a
    BayesShrink threshold is summed in the device's order, not numpy's."""
    kw = dict(kwargs or {})
    for k in kw:
        if k not in WV_KEYS:
            raise ValueError("denoise: keyword %r of 'wavelet' is not supported on the device (supported: %s)" % (k, ", ".join(WV_KEYS)))
    if "wavelet" not in kw:
        raise NotImplementedError("denoising technique 'wavelet' runs on the device only when kwargs names the wavelet key, e.g. "
                                  "dict(wavelet='db1') (the library's default); without it 'wavelet' is not built")
    for k in ("multichannel", "convert2ycbcr"):
        if kw.get(k, False):
            raise ValueError("denoise: %s=True of 'wavelet' is not supported on the device (frames are 2-D, single-channel)" % k)
    name = kw["wavelet"]
    table = wavelet_table()
    if not isinstance(name, str) or name not in table:
        raise ValueError("denoise: wavelet %r is not in the table of orthogonal wavelets the device runs (wavelet_table.json: %s)"
                         % (name, ", ".join(table)))
    mode, method = kw.get("mode", "soft"), kw.get("method", "BayesShrink")
    if mode not in WV_MODES:
        raise ValueError("denoise: mode %r of 'wavelet' is not supported (supported: soft, hard)" % (mode,))
    if method not in WV_METHODS:
        raise ValueError("denoise: method %r of 'wavelet' is not supported (supported: BayesShrink, VisuShrink)" % (method,))
    levels = kw.get("wavelet_levels")
    if levels is not None and (int(levels) != levels or int(levels) < 1):
        raise ValueError("denoise: wavelet_levels %r: a whole number of at least 1, or None" % (levels,))
    sigma = kw.get("sigma")
    if sigma is not None and not (np.ndim(sigma) == 0 and float(sigma) > 0 and np.isfinite(float(sigma))):
        raise ValueError("denoise: sigma %r of 'wavelet': one number above 0, or None" % (sigma,))
    if thresholds is not None:
        thresholds = np.ascontiguousarray(thresholds, dtype=np.float64)
        if thresholds.ndim not in (2, 3) or thresholds.shape[-1] != 3 or not (np.isfinite(thresholds).all() and (thresholds >= 0).all()):
            raise ValueError("denoise: injected thresholds are finite, not negative and (levels, 3) or (frames, levels, 3)")
    return WaveletSpec(name, table[name], 0 if levels is None else int(levels), WV_MODES[mode], WV_METHODS[method],
                       float("nan") if sigma is None else float(sigma), bool(kw.get("rescale_sigma", True)), thresholds)


# split-Bregman TV denoising (gpet_tvb, GPET_TVB_*): the third stage of its own in front of the raw-frame path
TVB_OUT_ON_DEVICE = 8  # gpet_tvb_images: out[] are device pointers
TVB_KEYS = ("weight", "max_iter", "eps", "isotropic", "multichannel")
TVB_DIAG_MAX = 768  # min(M, N) at most: the hand-over of a diagonal stays inside 64 KB of LDS (gpet_tvb_plan.h)
TVB_CHUNK_BUDGET = 256 << 20  # bytes a chunk's workspaces and staging stay inside (gpet_tvb_plan.h: TVB_CHUNK_BUDGET)


def tvb_frame_bytes(M, N):
    """Bytes of one frame's workspace (gpet_tvb_plan.h: tvb_frame_bytes): six skewed float64 arrays of (M + 2)(N + 2), to 256 bytes."""
    return (6 * (int(M) + 2) * (int(N) + 2) * 8 + 255) & ~255


class GpetTvb(C.Structure):
    _fields_ = [("weight", C.c_double), ("eps", C.c_double), ("max_iter", C.c_int32), ("isotropic", C.c_int32)]


class TvbSpec(PreSpec):
    """What tvb_spec returns: ``c`` the gpet_tvb of the call."""
    technique, symbol, out_on_device = "tvb", "gpet_tvb_images", TVB_OUT_ON_DEVICE
    not_a_filter = ("denoising technique 'tvb' is no gpet_denoise technique: it is built as a stage of its own "
                    "(tvb_spec, Context.tvb_images) and runs when kwargs gives weight, e.g. dict(weight=5)")
    reports_n_iter = True

    def __init__(self, weight, eps, max_iter, isotropic):
        self.c = GpetTvb(weight=weight, eps=eps, max_iter=max_iter, isotropic=int(bool(isotropic)))

    def check_frames(self, shape):
        if min(shape) < 2 or min(shape) > TVB_DIAG_MAX:
            raise ValueError("denoise: 'tvb' takes frames of at least 2 x 2 pixels whose smaller extent is at most %d, not %d x %d"
                             % (TVB_DIAG_MAX, shape[0], shape[1]))


def tvb_spec(kwargs):
    """The keyword arguments of ``gpet_utils.denoise(image, 'tvb', kwargs)`` = scikit-image's ``denoise_tv_bregman`` -> TvbSpec,
    decided from the arguments alone (no device): ``weight`` (above 0), ``max_iter`` (100), ``eps`` (1e-3), ``isotropic`` (True);
    ``multichannel`` only as False.  THE ``weight`` KEY MUST BE GIVEN: it is a required argument of the library (the reference
    itself fails without it), and kwargs without it raise NotImplementedError, as 'tvb' did before the stage was built.  Any other
    key raises ValueError naming it, and so does a value the device refuses."""
    kw = dict(kwargs or {})
    for k in kw:
        if k not in TVB_KEYS:
            raise ValueError("denoise: keyword %r of 'tvb' is not supported on the device (supported: %s)" % (k, ", ".join(TVB_KEYS)))
    if "weight" not in kw:
        raise NotImplementedError("denoising technique 'tvb' runs on the device only when kwargs gives weight, the library's required "
                                  "argument, e.g. dict(weight=5); without it 'tvb' is not built")
    if kw.get("multichannel", False):
        raise ValueError("denoise: multichannel=True of 'tvb' is not supported on the device (frames are 2-D, single-channel)")
    weight, eps, max_iter = kw["weight"], kw.get("eps", 1e-3), kw.get("max_iter", 100)
    if not (np.ndim(weight) == 0 and float(weight) > 0 and np.isfinite(float(weight))):
        raise ValueError("denoise: weight %r of 'tvb': one finite number above 0" % (weight,))
    if not (np.ndim(eps) == 0 and float(eps) >= 0):
        raise ValueError("denoise: eps %r of 'tvb': one number, not negative" % (eps,))
    if not (np.ndim(max_iter) == 0 and int(max_iter) == max_iter and int(max_iter) >= 1):
        raise ValueError("denoise: max_iter %r of 'tvb': a whole number of at least 1" % (max_iter,))
    return TvbSpec(float(weight), float(eps), int(max_iter), bool(kw.get("isotropic", True)))


# the stages of their own in front of the raw-frame path: technique -> spec class (see PreSpec).  RawFrames.pre holds the spec,
# RawFrames.pre_resolved runs it (Context.pre_images) into a PreFrames and hands float64 device frames on.  A new stage is one
# spec class, its from_kwargs and one entry here
NlmeansSpec.from_kwargs, NlmeansFastSpec.from_kwargs = staticmethod(nlmeans_spec), staticmethod(nlmeans_fast_spec)
WaveletSpec.from_kwargs, TvbSpec.from_kwargs = staticmethod(wavelet_spec), staticmethod(tvb_spec)
PRE_STAGES = {cls.technique: cls for cls in (NlmeansSpec, NlmeansFastSpec, WaveletSpec, TvbSpec)}


# polar unwrap (gpet_polar, csrc/gpet_polar_plan.h): raw frames resampled to (radius x angle) in front of everything else, so that a
# closed contour r(theta) is the horizontal edge the tracer follows
POLAR_OUT_ON_DEVICE = 8  # gpet_polar_images: out[] are device pointers
POLAR_NTHETA_MIN, POLAR_CELLS_MAX = 4, 1 << 28
POLAR_KEYS = ("centre", "n_r", "n_theta", "r0", "dr", "theta0", "pad")


class GpetPolar(C.Structure):
    _fields_ = [("cx", C.POINTER(C.c_double)), ("cy", C.POINTER(C.c_double)), ("n_centres", C.c_int32), ("n_r", C.c_int32),
                ("n_theta", C.c_int32), ("pad", C.c_int32), ("r0", C.c_double), ("dr", C.c_double), ("cos_t", C.POINTER(C.c_double)),
                ("sin_t", C.POINTER(C.c_double))]


def polar_refusal(n_r, n_theta, pad, r0, dr, pix=PIX_F64, M=2, N=2, n_centres=1, n_img=1, cx=(0.0,), cy=(0.0,)):
    """Why this spec cannot be unwrapped with (polar_check of csrc/gpet_polar_plan.h, same order, same words), or None.  The defaults
    of the frame's side pass, so the spec alone can be asked about."""
    if pix not in (PIX_U8, PIX_U16, PIX_F32, PIX_F64):
        return "polar: unknown pixel type"
    if M < 2 or N < 2:
        return "polar: frames must be at least 2 x 2 pixels"
    if n_r < 1:
        return "polar: n_r must be at least 1"
    if n_theta < POLAR_NTHETA_MIN:
        return "polar: n_theta must be at least 4"
    if pad < 0 or pad > n_theta:
        return "polar: pad must lie in [0, n_theta]"
    if not (r0 >= 0.0 and r0 < np.inf):
        return "polar: r0 must be finite and at least 0"
    if not (dr > 0.0 and dr < np.inf):
        return "polar: dr must be finite and above 0"
    if n_theta + 1 + 2 * pad > POLAR_CELLS_MAX // n_r:
        return "polar: the unwrapped frame exceeds 2^28 pixels (n_r * (n_theta + 1 + 2 * pad))"
    if n_centres != 1 and n_centres != n_img:
        return "polar: one centre for all frames or one per frame"
    if cx is None or cy is None:
        return "polar: the centres are a null pointer"
    if not (np.all(np.isfinite(np.asarray(cx, dtype=np.float64)[:n_centres]))
            and np.all(np.isfinite(np.asarray(cy, dtype=np.float64)[:n_centres]))):
        return "polar: a centre is not finite"
    return None


def polar_tables(n_theta, theta0=0.0):
    """(cos_t, sin_t): numpy's cos and sin of ``theta0 + 2 pi j / n_theta``, j = 0 .. n_theta - 1, float64 -- the tables the device
    takes as data."""
    theta = float(theta0) + (2.0 * np.pi * np.arange(int(n_theta), dtype=np.float64)) / float(int(n_theta))
    return np.ascontiguousarray(np.cos(theta)), np.ascontiguousarray(np.sin(theta))


class PolarSpec(object):
    """What polar_spec returns: ``centre`` (n_centres, 2) float64 (cx, cy) rows, ``n_r``, ``n_theta``, ``r0``, ``dr``, ``theta0``,
    ``pad`` (None until the gradient kernel is known: ``resolved``), the tables ``cos_t`` / ``sin_t``; ``shape`` = (n_r, W) and
    ``width`` = W = n_theta + 1 + 2 pad once pad is resolved.  No denoising technique, but its call has the shape of theirs:
    ``symbol``, ``out_on_device`` and ``call_arg`` as PreSpec describes them."""
    symbol, out_on_device, reports_n_iter = "gpet_polar_images", POLAR_OUT_ON_DEVICE, False

    def __init__(self, centre, n_r, n_theta, r0, dr, theta0, pad):
        self.centre, self.n_r, self.n_theta, self.r0, self.dr, self.theta0, self.pad = centre, n_r, n_theta, r0, dr, theta0, pad
        self.cos_t, self.sin_t = polar_tables(n_theta, theta0)

    @property
    def width(self):
        return self.n_theta + 1 + 2 * self.pad

    @property
    def shape(self):
        return (self.n_r, self.width)

    def as_dict(self):
        return dict(centre=self.centre.copy(), n_r=self.n_r, n_theta=self.n_theta, r0=self.r0, dr=self.dr, theta0=self.theta0, pad=self.pad)

    def resolved(self, default_pad):
        """This spec with ``pad=None`` replaced by ``default_pad`` (half the width of the widest gradient kernel; 0 without one)."""
        if self.pad is not None:
            return self
        return polar_spec(dict(self.as_dict(), pad=int(default_pad)))

    def with_centre(self, centre):
        """This spec around other centres (the shape stays)."""
        return polar_spec(dict(self.as_dict(), centre=centre))

    def refusal(self, pix, shape, n_img):
        return polar_refusal(self.n_r, self.n_theta, self.pad, self.r0, self.dr, pix, int(shape[0]), int(shape[1]), self.centre.shape[0],
                             n_img, self.centre[:, 0], self.centre[:, 1])

    def call_arg(self, T=None, shape=None):
        """(gpet_polar of the call, what must stay alive while it runs) -- whatever the frames: the signature is PreSpec's."""
        cx, cy = np.ascontiguousarray(self.centre[:, 0]), np.ascontiguousarray(self.centre[:, 1])
        dp = C.POINTER(C.c_double)
        c = GpetPolar(cx=cx.ctypes.data_as(dp), cy=cy.ctypes.data_as(dp), n_centres=cx.shape[0], n_r=self.n_r, n_theta=self.n_theta,
                      pad=self.pad, r0=self.r0, dr=self.dr, cos_t=self.cos_t.ctypes.data_as(dp), sin_t=self.sin_t.ctypes.data_as(dp))
        return c, (cx, cy, self.cos_t, self.sin_t)


def polar_spec(polar):
    """``polar=dict(centre=(cx, cy) | (T, 2) array, n_r=, n_theta=, r0=0.0, dr=1.0, theta0=0.0, pad=None)`` -> PolarSpec, decided from
    the arguments alone (no device); a PolarSpec passes through.  ``centre``: x is the column, y the row; one pair for all frames or
    one per frame.  ``pad=None``: half the width of the widest gradient kernel, 0 where there is none (``PolarSpec.resolved``).  An
    unknown or missing key and every value the device would refuse (``polar_refusal``) raise ValueError."""
    if isinstance(polar, PolarSpec):
        return polar
    if not isinstance(polar, dict):
        raise ValueError("polar must be a dict(centre=, n_r=, n_theta=, r0=0.0, dr=1.0, theta0=0.0, pad=None)")
    for k in polar:
        if k not in POLAR_KEYS:
            raise ValueError("polar: unknown key %r (known: %s)" % (k, ", ".join(POLAR_KEYS)))
    for k in ("centre", "n_r", "n_theta"):
        if polar.get(k) is None:
            raise ValueError("polar: %s is required" % k)
    for k in ("n_r", "n_theta", "pad"):
        v = polar.get(k)
        if v is not None and not (np.ndim(v) == 0 and int(v) == v):
            raise ValueError("polar: %s %r: a whole number" % (k, v))
    for k in ("r0", "dr", "theta0"):
        if np.ndim(polar.get(k, 0.0)) != 0:
            raise ValueError("polar: %s %r: one number" % (k, polar[k]))
    centre = np.array(polar["centre"], dtype=np.float64)
    if centre.shape == (2,):
        centre = centre.reshape(1, 2)
    if centre.ndim != 2 or centre.shape[1] != 2 or centre.shape[0] < 1:
        raise ValueError("polar: centre must be (cx, cy) or a (T, 2) array of them")
    n_r, n_theta, pad = int(polar["n_r"]), int(polar["n_theta"]), polar.get("pad")
    r0, dr, theta0 = float(polar.get("r0", 0.0)), float(polar.get("dr", 1.0)), float(polar.get("theta0", 0.0))
    if not np.isfinite(theta0):
        raise ValueError("polar: theta0 must be finite")
    why = polar_refusal(n_r, n_theta, 0 if pad is None else int(pad), r0, dr, cx=centre[:, 0], cy=centre[:, 1], n_centres=centre.shape[0],
                        n_img=centre.shape[0])
    if why is not None:
        raise ValueError(why)
    return PolarSpec(np.ascontiguousarray(centre), n_r, n_theta, r0, dr, theta0, None if pad is None else int(pad))


def polar_default_pad(kernels):
    """Half the width of the widest of ``kernels`` (2-D arrays); 0 for none."""
    return max([int(k.shape[1]) // 2 for k in kernels] or [0])


class GpetParams(C.Structure):
    _fields_ = [("kernel_type", C.c_int32), ("nu", C.c_double), ("sigma_f", C.c_double),
                ("length_scale", C.c_double), ("noise_y", C.c_double), ("n_samples", C.c_int32),
                ("n_keep", C.c_int32), ("delta_x", C.c_int32), ("pixel_thresh", C.c_int32),
                ("score_thresh", C.c_double), ("fix_endpoints", C.c_int32), ("x_st", C.c_int32),
                ("x_en", C.c_int32), ("n_init", C.c_int32), ("obs_cap", C.c_int32), ("factor_cap", C.c_int32),
                ("z_cols", C.c_int32), ("jitter", C.c_double)]


class GpetScalars(C.Structure):
    _fields_ = [("y_s", C.c_double), ("amp", C.c_double), ("y_mean", C.c_double), ("y_std", C.c_double),
                ("score_thresh", C.c_double), ("lml", C.c_double), ("n", C.c_int32), ("n_obs", C.c_int32),
                ("rank", C.c_int32), ("status", C.c_int32), ("iter", C.c_int32), ("done", C.c_int32),
                ("n_removed", C.c_int32), ("force", C.c_int32)]


class GpetResultHead(C.Structure):
    """gpet_result_head: the head of one edge's result record (gpet_batch_results / gpet_gather_results)."""
    _fields_ = [("edge_len", C.c_int32), ("n_iter", C.c_int32), ("n_obs", C.c_int32), ("status", C.c_int32),
                ("theta", C.c_double * 3), ("nlml", C.c_double)]


def result_bytes(len_cap):
    """Bytes of one result record for ``len_cap`` points (gpet_result_bytes)."""
    n = C.c_size_t()
    rc = load().gpet_result_bytes(int(len_cap), C.byref(n))
    if rc:
        raise GpetError(rc, "gpet_result_bytes(%d)" % int(len_cap))
    return n.value


def decode_results(raw, n, len_cap):
    """numpy views of ``n`` result records (include/gpet_hip.h, "Result records"): trace (n, len_cap, 2) int64 yx,
    lower / upper (n, len_cap) f64, and per edge edge_len, n_iter, n_obs, status, theta (n, 3), nlml."""
    L = int(len_cap)
    dt = np.dtype([("edge_len", "<i4"), ("n_iter", "<i4"), ("n_obs", "<i4"), ("status", "<i4"), ("theta", "<f8", (3,)),
                   ("nlml", "<f8"), ("trace", "<i8", (L, 2)), ("lower", "<f8", (L,)), ("upper", "<f8", (L,))])
    assert dt.itemsize == result_bytes(L) and C.sizeof(GpetResultHead) == dt.fields["trace"][1]
    rec = np.frombuffer(raw, dtype=dt, count=int(n))
    return {k: np.array(rec[k]) for k in dt.names}


# seed ensembles (gpet_batch_ensemble)
ENSEMBLE_MAX = 1024  # GPET_ENSEMBLE_MAX: members of one group


class GpetEnsembleHead(C.Structure):
    """gpet_ensemble_head: the head of one group's record (gpet_batch_ensemble)."""
    _fields_ = [("n_members", C.c_int32), ("edge_len", C.c_int32), ("x_st", C.c_int32), ("medoid", C.c_int32),
                ("best_cost", C.c_int32), ("reserved", C.c_int32), ("tol", C.c_double)]


ENSEMBLE_F64 = ("median", "q_lo", "q_hi", "min", "max")  # the f64 sections of a record, in order


def ensemble_layout(n_groups, n_edges, len_cap):
    """The layout csrc/gpet_ensemble_plan.h computes, for hosts and tests that build or decode an ensemble buffer without a
    device: dict(record_bytes, off_trace, off_median, off_q_lo, off_q_hi, off_min, off_max, off_agree, off_cost, off_off,
    total_bytes); ValueError for arguments that describe no buffer."""
    G, B, L = int(n_groups), int(n_edges), int(len_cap)
    if G < 1 or B < 1 or L < 1 or L > 1 << 24:
        raise ValueError("no ensemble buffer for n_groups=%d n_edges=%d len_cap=%d" % (G, B, L))
    d = dict(off_trace=C.sizeof(GpetEnsembleHead))
    off = d["off_trace"] + 16 * L
    for k in ENSEMBLE_F64:
        d["off_" + k] = off
        off += 8 * L
    d["off_agree"] = off
    d["record_bytes"] = off + ((4 * L + 7) & ~7)
    d["off_cost"] = G * d["record_bytes"]
    d["off_off"] = d["off_cost"] + 8 * B
    d["total_bytes"] = d["off_off"] + ((4 * B + 7) & ~7)
    return d


def ensemble_bytes(n_groups, n_edges, len_cap):
    """Bytes gpet_batch_ensemble writes for ``n_groups`` groups over ``n_edges`` edges of up to ``len_cap`` points
    (gpet_ensemble_bytes)."""
    n = C.c_size_t()
    rc = load().gpet_ensemble_bytes(int(n_groups), int(n_edges), int(len_cap), C.byref(n))
    if rc:
        raise GpetError(rc, "gpet_ensemble_bytes(%d, %d, %d)" % (int(n_groups), int(n_edges), int(len_cap)))
    return n.value


def decode_ensemble(raw, n_groups, n_edges, len_cap, group_of=None):
    """What gpet_batch_ensemble wrote (include/gpet_hip.h, "seed ensembles"), plain numpy, no device: (groups, cost, off) with
    ``cost`` (n_edges,) f64 the final cost of every edge, ``off`` (n_edges,) int32 (-1: not a member of any group) and one dict per
    group: ``n_members``, ``edge_len``, ``x_st``, ``tol``, ``medoid``, ``best_cost`` (edge indices, -1 without members), ``trace``
    (edge_len, 2) int64 yx, ``median``, ``q_lo``, ``q_hi``, ``min``, ``max`` (edge_len,) f64 and ``agree`` (edge_len,) int32 --
    and, with ``group_of`` (the table the call was given), ``members`` (edge indices, ascending) with their ``off`` and ``cost``."""
    G, B, L = int(n_groups), int(n_edges), int(len_cap)
    lay = ensemble_layout(G, B, L)
    buf = np.frombuffer(raw, dtype=np.uint8)
    if buf.size < lay["total_bytes"]:
        raise ValueError("an ensemble of %d groups, %d edges, len_cap %d needs %d bytes, got %d" % (G, B, L, lay["total_bytes"], buf.size))
    dt = np.dtype([("n_members", "<i4"), ("edge_len", "<i4"), ("x_st", "<i4"), ("medoid", "<i4"), ("best_cost", "<i4"),
                   ("reserved", "<i4"), ("tol", "<f8"), ("trace", "<i8", (L, 2))] + [(k, "<f8", (L,)) for k in ENSEMBLE_F64]
                  + [("agree", "<i4", (L,)), ("pad", "u1", (lay["record_bytes"] - lay["off_agree"] - 4 * L,))])
    assert dt.itemsize == lay["record_bytes"] and dt.fields["trace"][1] == lay["off_trace"] and dt.fields["agree"][1] == lay["off_agree"]
    rec = np.frombuffer(buf[:lay["off_cost"]].tobytes(), dtype=dt, count=G)
    cost = np.frombuffer(buf[lay["off_cost"]:lay["off_off"]].tobytes(), dtype="<f8").copy()
    off = np.frombuffer(buf[lay["off_off"]:lay["off_off"] + 4 * B].tobytes(), dtype="<i4").copy()
    if group_of is not None:
        group_of = np.asarray(group_of).reshape(-1)
        if group_of.shape[0] != B:
            raise ValueError("group_of has %d entries for %d edges" % (group_of.shape[0], B))
    groups = []
    for g in range(G):
        n = max(0, min(int(rec["edge_len"][g]), L))
        d = dict(n_members=int(rec["n_members"][g]), edge_len=n, x_st=int(rec["x_st"][g]), tol=float(rec["tol"][g]),
                 medoid=int(rec["medoid"][g]), best_cost=int(rec["best_cost"][g]), trace=np.array(rec["trace"][g, :n]),
                 agree=np.array(rec["agree"][g, :n]))
        for k in ENSEMBLE_F64:
            d[k] = np.array(rec[k][g, :n])
        if group_of is not None:
            d["members"] = np.flatnonzero((group_of == g) & (off >= 0)).astype(np.int64)
            d["off"] = off[d["members"]]
            d["cost"] = cost[d["members"]]
        groups.append(d)
    return groups, cost, off


def check_group_table(group_of, n_edges):
    """``group_of`` as the int32 table gpet_batch_ensemble takes and its number of groups; ValueError for a table of the wrong
    length, an index below -1 or a group index that does not occur (what needs no device to be refused)."""
    g = np.asarray(group_of)
    if g.ndim != 1 or g.shape[0] != int(n_edges):
        raise ValueError("group_of must hold one group index per edge (%d), got shape %s" % (int(n_edges), g.shape))
    if g.size and not np.issubdtype(g.dtype, np.integer):
        raise ValueError("group_of must hold integers")
    g = g.astype(np.int32)
    if (g < -1).any():
        raise ValueError("group_of holds an index below -1 (-1 means: in no group)")
    n_groups = int(g.max()) + 1 if g.size else 0
    if n_groups < 1:
        raise ValueError("group_of assigns no edge to a group")
    missing = sorted(set(range(n_groups)) - set(g.tolist()))
    if missing:
        raise ValueError("group_of never uses group %d of %d (every index must occur)" % (missing[0], n_groups))
    return np.ascontiguousarray(g), n_groups


# seed ensembles in sequences (gpet_batch_warm_start_groups): where a group's edges take the next frame's observations from
WARM_MEDOID, WARM_BEST_COST, WARM_CONSENSUS = 0, 1, 2
WARM_FROM = {"medoid": WARM_MEDOID, "best_cost": WARM_BEST_COST, "consensus": WARM_CONSENSUS}
WARM_SRC_NONE, WARM_SRC_CONSENSUS = -1, -2  # what src_out holds besides an edge index


def warm_from(name):
    """``'medoid'`` / ``'best_cost'`` / ``'consensus'`` (or the GPET_WARM_* value) as the library takes it; ValueError otherwise."""
    if name in WARM_FROM:
        return WARM_FROM[name]
    if isinstance(name, (int, np.integer)) and not isinstance(name, bool) and int(name) in WARM_FROM.values():
        return int(name)
    raise ValueError("warm_from must be one of %s, not %r" % (sorted(WARM_FROM), name))


def warm_sources(group_of, groups, frm):
    """The source of every edge's warm start, as gpet_batch_warm_start_groups reports it in ``src_out`` (csrc/gpet_warm_plan.h),
    from ``group_of`` and the groups' dicts (``medoid``, ``best_cost``; -1 in a group without members): the edge itself outside any
    group, else the group's medoid / best-cost member, WARM_SRC_CONSENSUS, or WARM_SRC_NONE for a group without members."""
    frm = warm_from(frm)
    out = np.empty(len(group_of), dtype=np.int32)
    for e, g in enumerate(np.asarray(group_of).tolist()):
        if g < 0:
            out[e] = e
        elif groups[g]["medoid"] < 0:
            out[e] = WARM_SRC_NONE
        else:
            out[e] = (groups[g]["medoid"], groups[g]["best_cost"], WARM_SRC_CONSENSUS)[frm]
    return out


# iteration history (gpet_batch_set_history): what a record holds beyond its head
HISTORY_LEVELS = {None: 0, "off": 0, "obs": 1, "curves": 2, "full": 3}


class GpetHistoryPlan(C.Structure):
    """gpet_history_plan: sizes and offsets of a batch's iteration history (gpet_history_layout)."""
    _fields_ = [("level", C.c_int32), ("iter_cap", C.c_int32), ("obs_cap", C.c_int32), ("len_cap", C.c_int32),
                ("edge_bytes", C.c_int64), ("record_bytes", C.c_int64), ("off_records", C.c_int64), ("off_obs", C.c_int64),
                ("off_curve", C.c_int64), ("off_mean", C.c_int64), ("off_std", C.c_int64)]


class GpetHistoryEdgeHead(C.Structure):
    """gpet_history_edge_head: in front of every edge's records."""
    _fields_ = [("n_rec", C.c_int32), ("dropped", C.c_int32), ("n_iter", C.c_int32), ("edge_len", C.c_int32)]


class GpetHistoryHead(C.Structure):
    """gpet_history_head: the head of one iteration's record."""
    _fields_ = [("iter", C.c_int32), ("n_obs", C.c_int32), ("best_idx", C.c_int32), ("rank", C.c_int32),
                ("n_removed", C.c_int32), ("reserved", C.c_int32), ("score_thresh", C.c_double),
                ("optimal_cost", C.c_double), ("y_s", C.c_double)]


def history_level(level):
    """0..3 of None / 'obs' / 'curves' / 'full' (or the number itself); ValueError for anything else."""
    if isinstance(level, (int, np.integer)) and not isinstance(level, bool) and 0 <= int(level) <= 3:
        return int(level)
    if level is None or (isinstance(level, str) and level in HISTORY_LEVELS):
        return HISTORY_LEVELS[level]
    raise ValueError("history must be None, 'obs', 'curves' or 'full', not %r" % (level,))


def history_plan(level, iter_cap, obs_cap, len_cap):
    """The layout csrc/gpet_history_plan.h computes (the library reports its own through gpet_history_layout): for hosts and
    tests that build or decode a history without a device."""
    level, iter_cap, obs_cap, len_cap = int(level), int(iter_cap), int(obs_cap), int(len_cap)
    if not (1 <= level <= 3 and iter_cap >= 1 and obs_cap >= 1 and len_cap >= 1):
        raise ValueError("no history for level=%d iter_cap=%d obs_cap=%d len_cap=%d" % (level, iter_cap, obs_cap, len_cap))
    p = GpetHistoryPlan(level=level, iter_cap=iter_cap, obs_cap=obs_cap, len_cap=len_cap)
    p.off_records = C.sizeof(GpetHistoryEdgeHead)
    off = p.off_obs = C.sizeof(GpetHistoryHead)
    off += 8 * obs_cap
    if level >= 2:
        p.off_curve = off
        off += 8 * len_cap
    if level >= 3:
        p.off_mean = off
        p.off_std = off + 8 * len_cap
        off += 16 * len_cap
    p.record_bytes = off
    p.edge_bytes = p.off_records + iter_cap * off
    return p


def decode_history(raw, layout, lens, obs_caps, x_sts=None):
    """The iteration histories of ``len(lens)`` edges from the bytes gpet_batch_history returns (include/gpet_hip.h,
    "iteration history"); plain numpy, no device.  ``layout``: the GpetHistoryPlan of the batch; ``lens`` / ``obs_caps``: every
    edge's own grid length and observation capacity; ``x_sts``: every edge's first grid column (default 0), the x of the curves.
    One dict per edge: ``n_iter`` (records kept), ``dropped``, ``obs`` (list of (n, 2) int64 xy), ``n_obs``, ``score_thresh``,
    ``optimal_cost``, ``best_idx``, ``rank``, ``n_removed``, ``y_s`` (arrays of n_iter); from level 2 ``optimal_curves`` (list of
    (Lg, 2) float64 xy, like the reference's iter_optimal_curves); with level 3 ``mean`` and ``std`` (n_iter, Lg)."""
    P = layout
    buf = np.frombuffer(raw, dtype=np.uint8)
    n = len(lens)
    if buf.size < n * P.edge_bytes:
        raise ValueError("history of %d edges needs %d bytes, got %d" % (n, n * P.edge_bytes, buf.size))
    head = np.dtype([("iter", "<i4"), ("n_obs", "<i4"), ("best_idx", "<i4"), ("rank", "<i4"), ("n_removed", "<i4"),
                     ("reserved", "<i4"), ("score_thresh", "<f8"), ("optimal_cost", "<f8"), ("y_s", "<f8")])
    assert head.itemsize == C.sizeof(GpetHistoryHead) == P.off_obs and C.sizeof(GpetHistoryEdgeHead) == P.off_records
    out = []
    for e in range(n):
        reg = buf[e * P.edge_bytes:(e + 1) * P.edge_bytes]
        n_rec, dropped = (int(v) for v in reg[:8].view("<i4"))
        n_rec = max(0, min(n_rec, P.iter_cap))
        recs = reg[P.off_records:P.off_records + n_rec * P.record_bytes].reshape(n_rec, P.record_bytes)
        Lg, x0 = int(lens[e]), 0 if x_sts is None else int(x_sts[e])
        h = np.ascontiguousarray(recs[:, :P.off_obs]).view(head).reshape(n_rec)

        def sect(off, count, dt):
            return np.ascontiguousarray(recs[:, off:off + count * np.dtype(dt).itemsize]).view(dt).reshape(n_rec, count)
        obs = sect(P.off_obs, 2 * P.obs_cap, "<i4").reshape(n_rec, P.obs_cap, 2).astype(np.int64)
        d = dict(n_iter=n_rec, dropped=dropped,
                 obs=[obs[i, :max(0, min(int(h["n_obs"][i]), int(obs_caps[e]), P.obs_cap))] for i in range(n_rec)])
        for k in ("n_obs", "score_thresh", "optimal_cost", "best_idx", "rank", "n_removed", "y_s"):
            d[k] = np.array(h[k])
        if P.level >= 2:
            x = (x0 + np.arange(Lg)).astype(np.float64)
            cur = sect(P.off_curve, P.len_cap, "<f8")
            d["optimal_curves"] = [np.stack((x, cur[i, :Lg]), -1) for i in range(n_rec)]
        if P.level >= 3:
            d["mean"] = sect(P.off_mean, P.len_cap, "<f8")[:, :Lg].copy()
            d["std"] = sect(P.off_std, P.len_cap, "<f8")[:, :Lg].copy()
        out.append(d)
    return out


def pix_code(dtype):
    """GPET_PIX_* of a numpy dtype (or its name); ValueError for a dtype the device does not read."""
    dt = np.dtype(dtype)
    if dt not in PIX_OF_DTYPE:
        raise ValueError("raw frames on the device must be uint8, uint16, float32 or float64, not %s" % dt)
    return PIX_OF_DTYPE[dt]


def native_frames(imgs):
    """Raw frames as the library takes them: (list of C-contiguous (M, N) arrays of ONE dtype, GPET_PIX_* code).  ``imgs`` is a
    (T, M, N) array or a sequence of (M, N) arrays.  uint8, uint16, float32 and float64 frames (native byte order) go up as
    they are -- no copy of a contiguous one; a stack of any other dtype, or of mixed dtypes, is converted to float64, which is
    what comp_grad_img does with every image."""
    frames = [np.asarray(f) for f in imgs]
    if not frames:
        raise ValueError("no frames")
    dts = {f.dtype for f in frames}
    dt = dts.pop() if len(dts) == 1 else None
    if dt is None or dt not in PIX_OF_DTYPE or not dt.isnative:
        dt = np.dtype(np.float64)
    frames = [np.ascontiguousarray(f, dtype=dt) for f in frames]
    if frames[0].ndim != 2 or any(f.shape != frames[0].shape for f in frames):
        raise ValueError("raw frames must be 2-D arrays of one shape")
    return frames, PIX_OF_DTYPE[dt]


class metrics_frames(object):
    """One side of the pairs ``Context.metrics_images`` scores: host frames (``frames``: a (T, M, N) array or a sequence of (M, N)
    arrays of ONE dtype among uint8, uint16, float32, float64 -- any other dtype is converted to float64, as native_frames does) or,
    with ``device_ptrs``, ``dtype`` and ``shape``, frames that lie on the context's device."""

    def __init__(self, frames=None, device_ptrs=None, dtype=None, shape=None):
        if (frames is None) == (device_ptrs is None):
            raise ValueError("frames come either from the host or as device pointers")
        if device_ptrs is not None:
            self.frames, self.pix, self.flags = None, pix_code(dtype), RAW_ON_DEVICE
            self.ptrs, self.shape = [int(p) for p in device_ptrs], (int(shape[0]), int(shape[1]))
        else:
            self.frames, self.pix = native_frames(frames)
            self.flags, self.ptrs, self.shape = 0, [f.ctypes.data for f in self.frames], tuple(self.frames[0].shape)


def split_kernels(kernel):
    """(list of float64 2-D kernels, multi): a list or tuple of 2-D kernels, or a 3-D array, is several kernels; a 2-D array or a
    nested list of numbers is ONE kernel (multi False), as it always was."""
    if isinstance(kernel, (list, tuple)):
        multi = len(kernel) > 0 and np.ndim(kernel[0]) == 2
    else:
        multi = np.ndim(kernel) == 3
    ks = [np.ascontiguousarray(k, dtype=np.float64) for k in (kernel if multi else [kernel])]
    if any(k.ndim != 2 or k.size == 0 for k in ks):
        raise ValueError("the gradient kernel must be a non-empty 2-D array (grad_kernel: one, or a list of them)")
    return ks, multi


def derive_slots(frame_of_edge, kernel_of):
    """The slot table of a batch whose edge e reads raw frame ``frame_of_edge[e]`` through kernel ``kernel_of[e]``: the distinct
    (frame, kernel) pairs in order of first occurrence are the image slots.  Returns ``(frame_of, kernel_of_slot, image_of)``:
    slot g is made of frame ``frame_of[g]`` with kernel ``kernel_of_slot[g]``, edge e reads slot ``image_of[e]``.  Pure: no
    device, no library."""
    frame_of_edge, kernel_of = [int(v) for v in frame_of_edge], [int(v) for v in kernel_of]
    if len(frame_of_edge) != len(kernel_of):
        raise ValueError("kernel_of has %d entries for %d edges" % (len(kernel_of), len(frame_of_edge)))
    slot, frame_of, kernel_of_slot, image_of = {}, [], [], []
    for pair in zip(frame_of_edge, kernel_of):
        if pair not in slot:
            slot[pair] = len(frame_of)
            frame_of.append(pair[0])
            kernel_of_slot.append(pair[1])
        image_of.append(slot[pair])
    return frame_of, kernel_of_slot, image_of


class RawFrames(object):
    """The ``raw=`` argument of Batch / Batch.set_images: frames plus the kernel that makes gradient images of them.
    Host frames (``frames``: see native_frames) or, with ``device_ptrs`` (integer device addresses of (M, N) arrays of
    ``dtype`` on the context's device, e.g. ``tensor.data_ptr()``) and ``shape``, nothing on the host at all.
    ``denoise``: optionally how the frames are denoised on the device before the kernel is applied, a ``(technique, kwargs)``
    pair of gpet_utils.denoise (see denoise_spec); 'nl', 'nl_fast', 'wavelet' and 'tvb' are stages of their own (PRE_STAGES: the
    spec is ``pre``, and pre_resolved runs it first).  ``kernel=None``: frames to denoise only (Context.denoise_images).
    ``slots=(frame_of, kernel_of)``: a slot table -- ``kernel`` is then a list of kernels (split_kernels) and image g is made of
    frame ``frame_of[g]`` with kernel ``kernel_of[g]`` (the library's *_multi calls); ``len()`` stays the number of frames,
    ``n_slots`` is the number of images.
    ``polar``: a polar spec (polar_spec: a dict or a PolarSpec) -- the frames are unwrapped to (radius x angle) before anything else
    happens to them (pre_resolved); ``shape`` is then the polar shape (n_r, W), ``src_shape`` the frames' own, ``polar`` the resolved
    spec (``pad=None`` became half the width of the widest kernel)."""

    def __init__(self, kernel, frames=None, device_ptrs=None, dtype=None, shape=None, denoise=None, slots=None, polar=None):
        if (frames is None) == (device_ptrs is None):
            raise ValueError("raw frames come either from the host or as device pointers")
        # (the techniques of PRE_STAGES are stages of their own: the frames go through Context.pre_images into device memory first --
        # see pre_resolved)
        self.pre = None
        if isinstance(denoise, tuple(PRE_STAGES.values())):
            self.pre, denoise = denoise, None
        elif isinstance(denoise, (tuple, list)) and len(denoise) == 2 and isinstance(denoise[0], str) and denoise[0] in PRE_STAGES:
            self.pre, denoise = PRE_STAGES[denoise[0]].from_kwargs(denoise[1]), None
        self.dn = denoise_spec(denoise)
        self.slots = None
        if slots is not None:
            self.kernels = split_kernels(kernel)[0]
            self.slots = ([int(v) for v in slots[0]], [int(v) for v in slots[1]])
            if len(self.slots[0]) != len(self.slots[1]) or not self.slots[0]:
                raise ValueError("a slot table has one frame index and one kernel index per image slot")
            kernel = self.kernels[0]
        self.kernel = None if kernel is None else np.ascontiguousarray(kernel, dtype=np.float64)
        if kernel is None and self.dn is None and self.pre is None and polar is None:
            raise ValueError("raw frames need a gradient kernel or a denoising technique")
        if self.kernel is not None and (self.kernel.ndim != 2 or self.kernel.size == 0):
            raise ValueError("the gradient kernel must be a non-empty 2-D array")
        if device_ptrs is not None:
            if dtype is None or shape is None:
                raise ValueError("device frames need their dtype and shape")
            self.frames, self.pix, self.flags = None, pix_code(dtype), RAW_ON_DEVICE
            self.ptrs = [int(p) for p in device_ptrs]
            self.shape = (int(shape[0]), int(shape[1]))
        else:
            self.frames, self.pix = native_frames(frames)
            self.flags = 0
            self.ptrs = [f.ctypes.data for f in self.frames]
            self.shape = self.frames[0].shape
        # (a polar spec: the frames are unwrapped first -- see pre_resolved --, and everything behind sees the polar shape)
        self.src_shape, self.polar = tuple(self.shape), None
        if polar is not None:
            kernels = self.kernels if self.slots is not None else ([] if self.kernel is None else [self.kernel])
            self.polar = polar_spec(polar).resolved(polar_default_pad(kernels))
            why = self.polar.refusal(self.pix, self.src_shape, len(self))
            if why is not None:
                raise ValueError("%s (%d frames of %d x %d, %d centres)" % ((why, len(self)) + self.src_shape + (self.polar.centre.shape[0],)))
            self.shape = self.polar.shape
        if self.pre is not None:
            self.pre.check_frames(self.shape)  # (refuses frames the stage does not take before a device is needed)

    def __len__(self):
        return len(self.ptrs)

    @property
    def nlm(self):
        """The non-local means spec of these frames, or None."""
        return self.pre if isinstance(self.pre, NlmeansSpec) else None

    @property
    def nlf(self):
        """The fast-mode non-local means spec of these frames, or None."""
        return self.pre if isinstance(self.pre, NlmeansFastSpec) else None

    @property
    def wv(self):
        """The wavelet spec of these frames, or None."""
        return self.pre if isinstance(self.pre, WaveletSpec) else None

    @property
    def tvb(self):
        """The split-Bregman spec of these frames, or None."""
        return self.pre if isinstance(self.pre, TvbSpec) else None

    @property
    def needs_resolve(self):
        """True when pre_resolved has work to do: a polar spec or a stage of its own."""
        return self.pre is not None or self.polar is not None

    def pre_resolved(self, ctx, buf):
        """These frames as the raw-frame calls take them: without a stage of its own (PRE_STAGES), self; with one, the frames
        denoised into the device memory of ``buf`` (a PreFrames; enqueued on the context's stream) as float64 device frames with
        the same kernels and slot table and no further denoising.  With a polar spec the frames are unwrapped into ``buf`` first
        (Context.polar_images), and whatever else these frames carry -- a stage of its own, which then writes into ``buf.second()``, an
        in-pass technique, kernels, slot table -- goes on from the unwrapped float64 frames as if the caller had given those."""
        if self.polar is not None:
            ptrs = buf.reserve(len(self), self.shape[0] * self.shape[1] * 8)
            ctx.polar_images(self, out_device_ptrs=ptrs)
            kernel = self.kernels if self.slots is not None else self.kernel
            flat = RawFrames(kernel, device_ptrs=ptrs, dtype=np.float64, shape=self.shape, slots=self.slots,
                             denoise=self.pre if self.pre is not None else self.dn)
            return flat.pre_resolved(ctx, buf.second())
        if self.pre is None:
            return self
        M, N = self.shape
        ptrs = buf.reserve(len(self), M * N * 8)
        ctx.pre_images(self, out_device_ptrs=ptrs)
        kernel = self.kernels if self.slots is not None else self.kernel
        return RawFrames(kernel, device_ptrs=ptrs, dtype=np.float64, shape=(M, N), slots=self.slots)

    def pointer_array(self):
        return (_P * len(self.ptrs))(*self.ptrs)

    def kernel_args(self):
        return self.kernel.ctypes.data, self.kernel.shape[0], self.kernel.shape[1]

    def dn_arg(self):
        return None if self.dn is None else C.byref(self.dn)

    @property
    def n_slots(self):
        return len(self.slots[0]) if self.slots is not None else len(self.ptrs)

    def multi_args(self):
        """n_kern, kern, kh, kw, frame_of, kernel_of as the *_multi calls and gpet_band_images take them (the arrays live as long as
        the tuple).  Without a slot table: the one kernel on every frame in order, the slot table of the single-kernel calls."""
        ks = self.kernels if self.slots is not None else [self.kernel]
        fo, ko = self.slots if self.slots is not None else (range(len(self)), [0] * len(self))
        nk, ns = len(ks), len(fo)
        return (nk, (_P * nk)(*[k.ctypes.data for k in ks]), (C.c_int32 * nk)(*[k.shape[0] for k in ks]),
                (C.c_int32 * nk)(*[k.shape[1] for k in ks]), (C.c_int32 * ns)(*fo), (C.c_int32 * ns)(*ko))


class GpetBand(C.Structure):
    """gpet_band (include/gpet_hip.h): the bands of gpet_batch_create_banded."""
    _fields_ = [("H", C.c_int32), ("n_pair", C.c_int32), ("r0", C.POINTER(C.c_int64)), ("pair_of", C.POINTER(C.c_int32))]


class GpetBandImages(C.Structure):
    """gpet_band_images: the full-frame images of a banded batch, gradient images or raw frames with a slot table."""
    _fields_ = [("grad", C.POINTER(C.c_void_p)), ("raw", C.POINTER(C.c_void_p)), ("pix", C.c_int32), ("n_frames", C.c_int32),
                ("n_kern", C.c_int32), ("reserved", C.c_int32), ("kern", C.POINTER(C.c_void_p)), ("kh", C.POINTER(C.c_int32)),
                ("kw", C.POINTER(C.c_int32)), ("frame_of", C.POINTER(C.c_int32)), ("kernel_of", C.POINTER(C.c_int32)),
                ("dn", C.POINTER(GpetDenoise)), ("flags", C.c_uint)]


def band_place(M, H, lo, hi, i_lo, i_hi):
    """The placement rule of a tracking band (csrc/gpet_band_plan.h, band_place): ``lo`` / ``hi`` the smallest and largest usable row
    of the source's trace in full-frame rows, ``i_lo`` / ``i_hi`` those of the edge's init points.  Python integers, floor division."""
    r0 = (int(lo) + int(hi)) // 2 - int(H) // 2
    r0 = min(max(r0, 0), int(M) - int(H))
    return max(min(r0, int(i_lo)), int(i_hi) - int(H) + 1)


def band_refusal(M, H, r0, i_lo, i_hi):
    """Why (r0, H) cannot be the band of an edge with init rows ``i_lo .. i_hi`` on an M-row frame (band_check of
    csrc/gpet_band_plan.h, same order, same words), or None; ``r0=None``: the band is still to be placed."""
    if H < 1:
        return "band_rows must be at least 1"
    if H > M:
        return "band_rows exceeds the rows of the frame (H > M)"
    if i_hi - i_lo + 1 > H:
        return "the init rows span more rows than the band holds (i_hi - i_lo + 1 > H)"
    if r0 is None:
        return None
    if r0 < 0 or r0 > M - H:
        return "r0 lies outside [0, M - H]"
    if i_lo < r0 or i_hi > r0 + H - 1:
        return "an init point lies outside its band"
    return None


INIT_WINDOW_MAX, INIT_COLS_MAX = 4096, 64


def init_follow_refusal(window, cols):
    """Why (window, cols) cannot be followed with (init_follow_check of csrc/gpet_init_plan.h, same order, same words), or None."""
    if window < 0:
        return "init_follow: window must be at least 0 rows"
    if window > INIT_WINDOW_MAX:
        return "init_follow: window exceeds 4096 rows"
    if cols < 0:
        return "init_follow: cols must be at least 0 columns"
    if cols > INIT_COLS_MAX:
        return "init_follow: cols exceeds 64 columns"
    return None


# label maps (csrc/gpet_label_plan.h; include/gpet_hip.h "label maps"): traces rasterised into uint8 masks on the device
LABELS_EXTEND, LABELS_TRANSPOSED, LABELS_OUT_ON_DEVICE = 1, 2, 4
LABEL_EDGES_MAX, LABEL_VERTS_MIN, LABEL_VERTS_MAX = 32, 4, 4096
LABEL_NO_ROW = -(1 << 63)  # GPET_LABEL_NO_ROW: a row that does not count
LABEL_CELLS_MAX = 1 << 31


def _label_refusal_maps(null_arg, M, N, map_of, n_maps, noun):
    """label_check_maps of csrc/gpet_label_plan.h, same order, same words: (reason or None, L)."""
    if null_arg or map_of is None:
        return "label maps: a null pointer", 0
    if M < 2 or N < 2:
        return "label maps: frames must be at least 2 x 2 pixels", 0
    if M > LABEL_CELLS_MAX // N:
        return "label maps: a map exceeds 2^31 pixels (M * N)", 0
    if n_maps < 1:
        return "label maps: n_maps must be at least 1", 0
    for e, f in enumerate(map_of):
        if f < -1 or f >= n_maps:
            return "label maps: map_of[%d] = %d lies outside [-1, n_maps = %d)" % (e, f, n_maps), 0
    L = 0
    for f in range(n_maps):
        cnt = sum(1 for v in map_of if v == f)
        if cnt == 0:
            return "label maps: map %d has no %s" % (f, noun), 0
        if cnt > LABEL_EDGES_MAX:
            return "label maps: map %d has more than 32 %ss (%d)" % (f, noun, cnt), 0
        L = max(L, cnt)
    return None, L


def label_refusal(M, N, x_st, length, map_of, n_maps, rows=(), out=()):
    """Why row maps cannot be made of these edges (label_check of csrc/gpet_label_plan.h, same order, same words), or None.  ``rows`` /
    ``out`` None: the null pointer's case."""
    why, _ = _label_refusal_maps(rows is None or out is None or x_st is None or length is None, M, N, map_of, n_maps, "edge")
    if why is not None:
        return why
    for e, (x0, n) in enumerate(zip(x_st, length)):
        if n < 1 or x0 < 0 or x0 + n > N:
            return "label maps: the grid of edge %d lies outside [0, N) (x_st = %d, len = %d, N = %d)" % (e, x0, n, N)
    return None


def label_refusal_xy(Ms, Ns, n_vert, map_of, n_maps, xy=(), out=()):
    """The same for maps of closed outlines (label_check_xy)."""
    why, _ = _label_refusal_maps(xy is None or out is None or n_vert is None, Ms, Ns, map_of, n_maps, "contour")
    if why is not None:
        return why
    for e, n in enumerate(n_vert):
        if n < LABEL_VERTS_MIN or n > LABEL_VERTS_MAX:
            return "label maps: contour %d has %d vertices, outside [4, 4096]" % (e, n)
    return None


def label_closed_refusal(e, x_st, x_en, pad, n_theta):
    """Why edge e of a polar batch is no closed contour (label_check_closed), or None."""
    if x_st == pad and x_en == pad + n_theta:
        return None
    return ("label maps: edge %d does not span the closed contour (x_st = %d, x_en = %d; pad = %d, pad + n_theta = %d)"
            % (e, x_st, x_en, pad, pad + n_theta))


def label_thick_count(n_maps, L, N):
    """gpet_label_thick_count: the int32 elements of ``thick`` for n_maps maps of at most L edges and N columns."""
    n = C.c_int64()
    if load().gpet_label_thick_count(int(n_maps), int(L), int(N), C.byref(n)) != OK:
        raise ValueError("label maps: thick of %d maps, %d edges, %d columns is out of range" % (n_maps, L, N))
    return n.value


def label_map_table(map_of, n_edges):
    """``map_of`` as the int32 table the library takes and the number of maps it names; None: every edge on map 0."""
    if map_of is None:
        return np.zeros(int(n_edges), dtype=np.int32), 1
    m = np.ascontiguousarray(np.asarray(map_of).reshape(-1), dtype=np.int32)
    if m.shape[0] != n_edges:
        raise ValueError("map_of has %d entries for %d edges" % (m.shape[0], n_edges))
    return m, int(m.max()) + 1 if m.size and m.max() >= 0 else 1


def _label_out(n_maps, shape, out_device_ptrs, thick_count, thick_device_ptr):
    """(maps or None, pointer array, thick or None, thick pointer, flag) of a label-map call."""
    if out_device_ptrs is not None:
        ptrs = [int(p) for p in out_device_ptrs]
        if len(ptrs) != n_maps:
            raise ValueError("%d output pointers for %d maps" % (len(ptrs), n_maps))
        if thick_count and thick_device_ptr is None:
            raise ValueError("maps on the device need thick_device_ptr for the thickness too")
        return None, (_P * n_maps)(*ptrs), None, (C.cast(_P(int(thick_device_ptr)), C.POINTER(C.c_int32)) if thick_count else None), LABELS_OUT_ON_DEVICE
    maps = np.empty((n_maps,) + tuple(shape), dtype=np.uint8)
    step = int(shape[0]) * int(shape[1])
    op = (_P * n_maps)(*[maps.ctypes.data + f * step for f in range(n_maps)])
    thick = np.empty(thick_count, dtype=np.int32) if thick_count else None
    return maps, op, thick, (thick.ctypes.data_as(C.POINTER(C.c_int32)) if thick_count else None), 0


# denoise quality metrics (gpet_metrics, GPET_METRICS_*; csrc/gpet_metrics_plan.h)
METRICS_B_ON_DEVICE, METRICS_MAPS_ON_DEVICE = 32, 64  # gpet_metrics_images: raw_b[] / ssim_maps[] are device pointers
METRICS_PX_MAX = 1 << 26
METRICS_CHUNK_BUDGET = 512 << 20
METRICS_KEYS = ("K1", "K2", "use_sample_covariance")
METRICS_RANGE_WORDS = ("im_true has intensity values outside the range expected for its data type.  Please manually specify the "
                       "data_range")


class GpetMetrics(C.Structure):
    _fields_ = [("win_size", C.c_int32), ("use_sample_covariance", C.c_int32), ("K1", C.c_double), ("K2", C.c_double),
                ("data_range", C.c_double)]


def metrics_frame_bytes(px, staged_a, staged_b):
    """Bytes of one pair's workspace (gpet_metrics_plan.h: metrics_frame_bytes): six float64 planes and the staged host frames."""
    al = lambda b: (int(b) + 255) & ~255
    return al(6 * px * 8) + al(staged_a) + al(staged_b)


def metrics_refusal(n_img, pix_a, pix_b, M, N, win_size=7, K1=0.01, K2=0.03, data_range=0.0, staged_a=0, staged_b=0):
    """The words gpet_metrics_images refuses these arguments with (gpet_metrics_plan.h: metrics_check, in its order), or None."""
    if n_img < 1:
        return "metrics: no frame"
    if pix_a not in range(4) or pix_b not in range(4):
        return "metrics: unknown pixel type"
    if M < 1 or N < 1:
        return "metrics: empty frame"
    if win_size > M or win_size > N:
        return "win_size exceeds image extent.  If the input is a multichannel (color) image, set multichannel=True."
    if win_size % 2 != 1:
        return "Window size must be odd."
    if win_size < 3:
        return "metrics: win_size must be at least 3"
    if not K1 >= 0:
        return "K1 must be positive"
    if not K2 >= 0:
        return "K2 must be positive"
    if not (data_range >= 0 and data_range < float("inf")):
        return "metrics: data_range must be a finite number above 0 (0: the library's rule)"
    if M * N > METRICS_PX_MAX:
        return "metrics: a frame exceeds 2^26 pixels (M * N)"
    fb = metrics_frame_bytes(M * N, staged_a, staged_b)
    if fb > METRICS_CHUNK_BUDGET:
        return ("metrics: the workspace of one frame (%d bytes: six float64 planes of %d x %d and its staging) exceeds the chunk budget of "
                "%d bytes" % (fb, M, N, METRICS_CHUNK_BUDGET))
    return None


def metrics_spec(win_size=7, data_range=None, **ssim_kwargs):
    """The keyword arguments of scikit-image's ``structural_similarity`` that the device builds -> GpetMetrics.  ``gaussian_weights``,
    ``gradient`` and ``multichannel`` set True, and any other key, raise ValueError naming the key."""
    for k in ("gaussian_weights", "gradient", "multichannel"):
        if ssim_kwargs.pop(k, False):
            raise ValueError("metrics: %s=True is not supported on the device (uniform window, no gradient, 2-D single-channel frames)" % k)
    for k in ssim_kwargs:
        if k not in METRICS_KEYS:
            raise ValueError("metrics: keyword %r is not supported on the device (supported: %s)" % (k, ", ".join(METRICS_KEYS)))
    w = 7 if win_size is None else win_size
    if int(w) != w:
        raise ValueError("metrics: win_size %r: a whole number" % (win_size,))
    return GpetMetrics(int(w), 1 if ssim_kwargs.get("use_sample_covariance", True) else 0, float(ssim_kwargs.get("K1", 0.01)),
                       float(ssim_kwargs.get("K2", 0.03)), 0.0 if data_range is None else float(data_range))


class GpetError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libgpet_hip status {code}: {msg}")
        self.code = code


# every symbol include/gpet_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "gpet_abi_version": (C.c_int, []),
    "gpet_set_option": (C.c_int, [C.c_char_p, C.c_int]),
    "gpet_get_option": (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    "gpet_option_count": (C.c_int, []),
    "gpet_option_info": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int), C.POINTER(C.c_char_p)]),
    "gpet_ctx_create": (C.c_int, [C.c_int, _P, C.POINTER(_P)]),
    "gpet_ctx_destroy": (None, [_P]),
    "gpet_last_error": (C.c_char_p, [_P]),
    "gpet_sync": (C.c_int, [_P]),
    "gpet_ctx_stream": (_P, [_P]),
    "gpet_timer_start": (C.c_int, [_P]),
    "gpet_timer_stop_ms": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "gpet_grad_image": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P]),
    "gpet_grad_images": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_uint,
                                   C.POINTER(_P)]),
    "gpet_denoise_images": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(GpetDenoise), C.c_uint,
                                      C.POINTER(_P), C.POINTER(C.c_int32)]),
    "gpet_nlmeans_images": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(GpetNlmeans), C.c_uint,
                                      C.POINTER(_P)]),
    "gpet_nlmeans_fast_images": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(GpetNlmeansFast), C.c_uint,
                                           C.POINTER(_P)]),
    "gpet_polar_images": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(GpetPolar), C.c_uint,
                                    C.POINTER(_P)]),
    "gpet_tvb_images": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(GpetTvb), C.c_uint,
                                  C.POINTER(_P), C.POINTER(C.c_int32)]),
    "gpet_wavelet_images": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(GpetWavelet), C.c_uint,
                                      C.POINTER(_P)]),
    "gpet_grad_images_dn": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int,
                                      C.POINTER(GpetDenoise), C.c_uint, C.POINTER(_P)]),
    "gpet_grad_images_multi": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(GpetDenoise), C.c_int,
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint, C.POINTER(_P)]),
    "gpet_normalise_f32": (C.c_int, [_P, _P, C.c_size_t, _P]),
    "gpet_batch_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(_P), C.c_int,
                                    C.POINTER(GpetParams), C.POINTER(_P), C.POINTER(_P)]),
    "gpet_batch_create2": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(_P), C.c_int,
                                     C.POINTER(GpetParams), C.POINTER(_P), C.c_uint, C.POINTER(_P)]),
    "gpet_batch_create_raw": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(_P), C.c_int, _P, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(GpetParams), C.POINTER(_P), C.c_uint, C.POINTER(_P)]),
    "gpet_batch_create_raw_dn": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(_P), C.c_int, _P, C.c_int, C.c_int,
                                           C.POINTER(GpetDenoise), C.c_int, C.POINTER(GpetParams), C.POINTER(_P), C.c_uint,
                                           C.POINTER(_P)]),
    "gpet_batch_create_mapped": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(_P),
                                           C.POINTER(GpetParams), C.POINTER(_P), C.c_uint, C.POINTER(_P)]),
    "gpet_batch_create_raw_mapped": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(_P), C.c_int,
                                               _P, C.c_int, C.c_int, C.POINTER(GpetDenoise), C.POINTER(GpetParams), C.POINTER(_P),
                                               C.c_uint, C.POINTER(_P)]),
    "gpet_batch_create_raw_multi": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(_P),
                                              C.c_int, C.c_int, C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(GpetDenoise),
                                              C.POINTER(GpetParams), C.POINTER(_P), C.c_uint, C.POINTER(_P)]),
    "gpet_batch_image_count": (C.c_int, [_P]),
    "gpet_batch_warm_start": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32)]),
    "gpet_batch_warm_start_ready": (C.c_int, [_P]),
    "gpet_batch_set_images": (C.c_int, [_P, C.POINTER(_P), C.c_uint]),
    "gpet_batch_set_raw_images_dn": (C.c_int, [_P, C.POINTER(_P), C.c_int, _P, C.c_int, C.c_int, C.POINTER(GpetDenoise), C.c_uint]),
    "gpet_batch_set_raw_images": (C.c_int, [_P, C.POINTER(_P), C.c_int, _P, C.c_int, C.c_int, C.c_uint]),
    "gpet_batch_set_raw_images_multi": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.c_int, C.c_int, C.POINTER(_P), C.POINTER(C.c_int32),
                                                  C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                  C.POINTER(GpetDenoise), C.c_uint]),
    "gpet_batch_destroy": (None, [_P]),
    "gpet_batch_size": (C.c_int, [_P]),
    "gpet_batch_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "gpet_batch_reset": (C.c_int, [_P]),
    "gpet_profile_stage": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "gpet_batch_set_obs": (C.c_int, [_P, C.c_int, _P, C.c_int]),
    "gpet_batch_read": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_size_t]),
    "gpet_batch_write": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_size_t, C.c_int]),
    "gpet_batch_clear_injected_factor": (C.c_int, [_P, C.c_int]),
    "gpet_gp_fit_predict": (C.c_int, [_P, C.c_int]),
    "gpet_gp_factor": (C.c_int, [_P]),
    "gpet_gp_normals": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "gpet_gp_sample": (C.c_int, [_P]),
    "gpet_score_curves": (C.c_int, [_P]),
    "gpet_select_pixels": (C.c_int, [_P]),
    "gpet_curve_kde": (C.c_int, [_P]),
    "gpet_final_cov": (C.c_int, [_P]),
    "gpet_select_pixels_only": (C.c_int, [_P]),
    "gpet_select_pixels_loop": (C.c_int, [_P]),
    "gpet_final_set_training": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int]),
    "gpet_lml_batch": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "gpet_lml_stats": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "gpet_final_set_training_all": (C.c_int, [_P, _P, _P, _P, _P, C.c_int]),
    "gpet_batch_read_obs_all": (C.c_int, [_P, _P, _P, C.c_int]),
    "gpet_batch_read_scalars_all": (C.c_int, [_P, _P]),
    "gpet_final_predict_all": (C.c_int, [_P, _P, _P, _P, C.c_int]),
    "gpet_final_fit_all": (C.c_int, [_P, C.POINTER(C.c_uint32), _P, _P, _P, C.c_int, C.POINTER(C.c_int32)]),
    "gpet_final_optimize": (C.c_int, [_P, C.c_int, _P, _P, _P, C.POINTER(C.c_int32)]),
    "gpet_final_problems": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int32)]),
    "gpet_batch_set_sample_dtype": (C.c_int, [_P, C.c_int]),
    "gpet_batch_set_sample_arith": (C.c_int, [_P, C.c_int]),
    "gpet_batch_set_rng": (C.c_int, [_P, C.c_int]),
    "gpet_batch_set_option": (C.c_int, [_P, C.c_char_p, C.c_int]),
    "gpet_batch_get_option": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int)]),
    "gpet_trace_iterate": (C.c_int, [_P, C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_int)]),
    "gpet_comm_unique_id": (C.c_int, [_P]),
    "gpet_comm_create": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(_P)]),
    "gpet_comm_destroy": (None, [_P]),
    "gpet_comm_rank": (C.c_int, [_P]),
    "gpet_comm_world": (C.c_int, [_P]),
    "gpet_comm_block": (C.c_int, [_P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "gpet_bcast_grad": (C.c_int, [_P, _P, C.c_size_t, C.c_int]),
    "gpet_dev_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "gpet_dev_free": (C.c_int, [_P, _P]),
    "gpet_dev_copy": (C.c_int, [_P, _P, _P, C.c_size_t, C.c_int]),
    "gpet_allgather_i64": (C.c_int, [_P, _P, _P, _P]),
    "gpet_gather_traces": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P]),
    "gpet_result_bytes": (C.c_int, [C.c_int64, C.POINTER(C.c_size_t)]),
    "gpet_batch_results": (C.c_int, [_P, C.c_int64, _P, C.c_int]),
    "gpet_gather_results": (C.c_int, [_P, _P, C.c_int64, C.c_int64, _P]),
    "gpet_batch_set_history": (C.c_int, [_P, C.c_int, C.c_int]),
    "gpet_history_layout": (C.c_int, [_P, C.POINTER(GpetHistoryPlan)]),
    "gpet_batch_history": (C.c_int, [_P, C.c_int, _P, C.c_size_t, C.c_int]),
    "gpet_history_record": (C.c_int, [_P]),
    "gpet_batch_final_costs": (C.c_int, [_P, _P, C.c_int]),
    "gpet_ensemble_bytes": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_size_t)]),
    "gpet_batch_ensemble": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32), C.c_double, C.c_int64, _P, C.c_int]),
    "gpet_batch_ensemble_keep": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int32), C.c_double]),
    "gpet_batch_ensemble_kept": (C.c_int, [_P, C.c_int64, _P, C.c_int]),
    "gpet_batch_warm_start_groups": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "gpet_batch_warm_start_from": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32)]),
    "gpet_batch_create_banded": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(GpetBand), C.POINTER(GpetBandImages),
                                           C.POINTER(GpetParams), C.POINTER(_P), C.POINTER(_P)]),
    "gpet_batch_band_place": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int]),
    "gpet_batch_band_set": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "gpet_batch_band_r0": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "gpet_batch_init_follow": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "gpet_batch_set_init": (C.c_int, [_P, C.POINTER(_P)]),
    "gpet_batch_init_xy": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "gpet_label_maps": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int32), C.c_int, C.c_uint, C.POINTER(_P), C.POINTER(C.c_int32)]),
    "gpet_label_maps_xy": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                     C.c_int, C.c_uint, C.POINTER(_P)]),
    "gpet_batch_label_maps": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int, C.c_uint, C.POINTER(_P), C.POINTER(C.c_int32)]),
    "gpet_batch_label_maps_xy": (C.c_int, [_P, C.POINTER(GpetPolar), C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_uint,
                                           C.POINTER(_P)]),
    "gpet_label_thick_count": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "gpet_metrics_images": (C.c_int, [_P, C.POINTER(_P), C.c_int, C.POINTER(_P), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(GpetMetrics),
                                      C.c_uint, C.POINTER(C.c_double), C.POINTER(_P)]),
}
COMM_ID_BYTES = 128
SAMPLE_ARITH_F64, SAMPLE_ARITH_F32 = 0, 1  # gpet_batch_set_sample_arith

_lib = None


def get_option(name):
    """Current value of a process-wide tuning switch (gpet_get_option; -1 = chosen automatically)."""
    v = C.c_int()
    if load().gpet_get_option(name.encode(), C.byref(v)) != 0:
        raise ValueError("unknown option %r" % (name,))
    return v.value


_live_batches = []  # weak references to the Batch objects of this process (set_option(..., live_batches=True))


def set_option(name, value, live_batches=True):
    """Process-wide tuning switch of the library (gpet_set_option); returns the previous value (-1 = automatic).
    The library gives every batch its own copy of the table when the batch is created (gpet_batch_set_option changes that
    copy), so a switch set here reaches only batches created afterwards -- unless ``live_batches`` (the default, what tools
    and tests that flip a switch on an existing object mean): then it is also written into every live Batch of this process."""
    old = get_option(name)
    if load().gpet_set_option(name.encode(), int(value)) < 0:
        raise ValueError("unknown option %r" % (name,))
    if live_batches:
        for ref in list(_live_batches):
            b = ref()
            if b is None or not getattr(b, "h", None):
                _live_batches.remove(ref)
            else:
                b.set_option(name, value)
    return old


def options():
    """The table of tuning switches: {name: dict(value, default, lo, hi, doc)} (gpet_option_info)."""
    lib = load()
    out = {}
    for i in range(lib.gpet_option_count()):
        name, doc = C.c_char_p(), C.c_char_p()
        v, d, lo, hi = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        lib.gpet_option_info(i, C.byref(name), C.byref(v), C.byref(d), C.byref(lo), C.byref(hi), C.byref(doc))
        out[name.value.decode()] = dict(value=v.value, default=d.value, lo=lo.value, hi=hi.value, doc=doc.value.decode())
    return out


def load():
    """Load libgpet_hip.so (once).  Raises if it is absent: the product has no other path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  gaussian_process_edge_trace_amd has no CPU fallback.")
    # Deployment setting of the package: eight HIP hardware queues per process instead of the runtime's four.  A tracer drives
    # three streams per batch object (loop, RNG look-ahead, converged fits) and a server keeps several objects in flight; on four
    # queues they alias (+2-3 % throughput at 1 024 edges, +9 % at 256 with eight: profiles/r05_hw_queues.txt; 12 and more
    # hurt the latency of small batches).  The runtime reads the variable when it initialises, i.e. at the first HIP call of the
    # process: a value already in the environment wins, and a process that touched the GPU before importing this keeps its own.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.gpet_abi_version() != 1:
        raise ImportError("libgpet_hip.so ABI version mismatch")
    _lib = lib
    return lib


class PreFrames(object):
    """Device memory (gpet_dev_alloc) for the float64 frames a stage of its own ('nl', 'wavelet', 'tvb') leaves behind: owned by the
    object that feeds them to the raw-frame path, grown on demand, reused from frame to frame, freed on close()."""

    def __init__(self, ctx):
        self.ctx, self.ptr, self.bytes, self.next = ctx, None, 0, None

    def second(self):
        """A second buffer that lives and dies with this one: the unwrapped frames stay in this one while a stage of its own writes."""
        if self.next is None:
            self.next = PreFrames(self.ctx)
        return self.next

    def reserve(self, n, frame_bytes):
        """Room for n frames of frame_bytes each -> their device addresses."""
        pitch = (int(frame_bytes) + 255) & ~255
        if n * pitch > self.bytes:
            self.close()
            d = _P()
            self.ctx.check(self.ctx.lib.gpet_dev_alloc(self.ctx.h, n * pitch, C.byref(d)))
            self.ptr, self.bytes = d, n * pitch
        return [self.ptr.value + g * pitch for g in range(n)]

    def close(self):
        if self.next is not None:
            self.next.close()
        if self.ptr is not None and getattr(self.ctx, "h", None):
            self.ctx.lib.gpet_dev_free(self.ctx.h, self.ptr)  # (hipFree waits for the device)
        self.ptr, self.bytes = None, 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """gpet_ctx: one device + one HIP stream."""

    def __init__(self, device=0, stream=None):
        self.lib = load()
        h = _P()
        rc = self.lib.gpet_ctx_create(int(device), _P(stream) if stream else None, C.byref(h))
        if rc == ERR_NO_DEVICE:
            raise GpetError(rc, "no HIP device visible (this package needs an MI355X; there is no CPU fallback)")
        if rc != OK:
            raise GpetError(rc, "gpet_ctx_create failed")
        self.h = h
        self.device = device
        self._comms = []  # (weak references to the communicators built on this context: close() closes them first)
        # A batch is destroyed THROUGH its context (gpet_batch_destroy waits on the context's stream), so the context must go
        # last: close() closes the batches built on it first (weak references), and when the garbage collector finalises a
        # context before batches of the same garbage (their weak references are dead by then, the count is not) the handle is
        # kept until the last of them has closed.
        self._batches, self._open_batches, self._close_pending = [], 0, False

    def check(self, rc):
        if rc != OK:
            raise GpetError(rc, (self.lib.gpet_last_error(self.h) or b"").decode())

    def sync(self):
        self.check(self.lib.gpet_sync(self.h))

    def timer_start(self):
        self.check(self.lib.gpet_timer_start(self.h))

    def timer_stop_ms(self):
        ms = C.c_float()
        self.check(self.lib.gpet_timer_stop_ms(self.h, C.byref(ms)))
        return ms.value

    def grad_image(self, img, kernel):
        img = np.ascontiguousarray(img, dtype=np.float64)
        kernel = np.ascontiguousarray(kernel, dtype=np.float64)
        out = np.empty(img.shape, dtype=np.float32)
        self.check(self.lib.gpet_grad_image(self.h, img.ctypes.data, img.shape[0], img.shape[1], kernel.ctypes.data,
                                            kernel.shape[0], kernel.shape[1], out.ctypes.data))
        return out

    def grad_images(self, raw, transpose=False):
        """gpet_grad_images: comp_grad_img of every frame of ``raw`` (a RawFrames) in one batched pass -> (T, M, N) float32.
        ``transpose`` (GPET_FRAMES_TRANSPOSED): (T, N, M), every image the transpose of its frame's gradient image, made on the device."""
        M, N = raw.shape
        if raw.needs_resolve:  # (the polar unwrap and 'nl' / 'wavelet' / 'tvb' first, into device memory of this call; the calls below end with a wait)
            buf = PreFrames(self)
            try:
                return self.grad_images(raw.pre_resolved(self, buf), transpose)
            finally:
                buf.close()
        if transpose:
            return self._grad_images(raw, N, M, raw.flags | FRAMES_TRANSPOSED)
        return self._grad_images(raw, M, N, raw.flags)

    def _grad_images(self, raw, Mo, No, flags):
        """``grad_images`` behind the non-local means stage: outputs of shape (Mo, No), the library called with ``flags``."""
        M, N = raw.shape
        if raw.slots is not None:  # (a slot table: gpet_grad_images_multi -> (n_slots, M, N), slot g of frame_of[g], kernel_of[g])
            ns = raw.n_slots
            out = np.empty((ns, Mo, No), dtype=np.float32)
            op = (_P * ns)(*[out[g].ctypes.data for g in range(ns)])
            nk, kp, kh, kw, fo, ko = raw.multi_args()
            self.check(self.lib.gpet_grad_images_multi(self.h, raw.pointer_array(), len(raw), raw.pix, M, N, nk, kp, kh, kw, raw.dn_arg(),
                                                       ns, fo, ko, flags, op))
            return out
        out = np.empty((len(raw), Mo, No), dtype=np.float32)
        op = (_P * len(raw))(*[out[g].ctypes.data for g in range(len(raw))])
        kp, kh, kw = raw.kernel_args()
        if raw.dn is not None:
            self.check(self.lib.gpet_grad_images_dn(self.h, raw.pointer_array(), len(raw), raw.pix, M, N, kp, kh, kw, raw.dn_arg(),
                                                    flags, op))
            return out
        self.check(self.lib.gpet_grad_images(self.h, raw.pointer_array(), len(raw), raw.pix, M, N, kp, kh, kw, flags, op))
        return out

    def denoise_images(self, raw):
        """gpet_denoise_images: every frame of ``raw`` (a RawFrames with a denoising technique) denoised in one batched pass ->
        ((T, M, N) array of the reference's dtype, iterations per frame: 0 for the filters, 'nl' and 'wavelet'; the sweeps of 'tvb')."""
        if raw.polar is not None:  # (unwrapped into device memory of this call; every call below ends with a wait)
            buf = PreFrames(self)
            try:
                ptrs = buf.reserve(len(raw), raw.shape[0] * raw.shape[1] * 8)
                self.polar_images(raw, out_device_ptrs=ptrs)
                return self.denoise_images(RawFrames(None, device_ptrs=ptrs, dtype=np.float64, shape=raw.shape,
                                                     denoise=raw.pre if raw.pre is not None else raw.dn))
            finally:
                buf.close()
        if raw.pre is not None:  # (a stage of its own: its sweeps where it counts them, zeros where not)
            n_iter = np.zeros(len(raw), dtype=np.int32)
            return self._run_stage(raw, raw.pre, raw.shape, None, n_iter), n_iter
        if raw.dn is None:
            raise ValueError("no denoising technique")
        M, N = raw.shape
        out = np.empty((len(raw), M, N), dtype=denoised_dtype(raw.dn, raw.pix))
        op = (_P * len(raw))(*[out[g].ctypes.data for g in range(len(raw))])
        n_iter = np.zeros(len(raw), dtype=np.int32)
        self.check(self.lib.gpet_denoise_images(self.h, raw.pointer_array(), len(raw), raw.pix, M, N, raw.dn_arg(), raw.flags, op,
                                                n_iter.ctypes.data_as(C.POINTER(C.c_int32))))
        return out, n_iter

    def pre_images(self, raw, out_device_ptrs=None):
        """The stage of its own that ``raw`` carries (RawFrames.pre): nlmeans_images, nlmeans_fast_images, wavelet_images or
        tvb_images.  Frames that carry a polar spec are unwrapped first (RawFrames.pre_resolved): the stage runs on those."""
        if raw.polar is not None:
            raise ValueError("frames with a polar spec are unwrapped first: run the stage on raw.pre_resolved(ctx, buf)")
        if raw.pre is None:
            raise ValueError("no stage of its own")
        return self._run_stage(raw, raw.pre, raw.shape, out_device_ptrs)

    def _run_stage(self, raw, spec, shape, out_device_ptrs, n_iter=None, fill=None):
        """One batched call of a stage of its own, or of the polar unwrap, on the frames of ``raw``: ``spec`` names the call (``symbol``,
        ``out_on_device``, ``call_arg``: see PreSpec), ``shape`` is the frames' as the call takes them.  ``n_iter``: (T,) int32 the
        call fills where the stage counts sweeps (``reports_n_iter``) and leaves alone where not.  ``fill``: called with the spec
        argument before the call.  -> what _pre_out made: the (T, M, N) float64 result, or None with ``out_device_ptrs``."""
        T, (M, N) = len(raw), shape
        out, op, flags = self._pre_out(raw, out_device_ptrs, spec.out_on_device)
        arg, keep = spec.call_arg(T, (M, N))
        if fill is not None:
            fill(arg)
        tail = (None if n_iter is None else n_iter.ctypes.data_as(C.POINTER(C.c_int32)),) if spec.reports_n_iter else ()
        self.check(getattr(self.lib, spec.symbol)(self.h, raw.pointer_array(), T, raw.pix, M, N, arg, flags, op, *tail))
        del keep
        return out

    @staticmethod
    def _pre_out(raw, out_device_ptrs, on_device):
        """Where a stage of its own writes -> (array or None, pointers, flags): the device addresses given, one per frame, with the
        stage's ``on_device`` flag, or a fresh (T, M, N) float64 array."""
        T = len(raw)
        if out_device_ptrs is not None:
            if len(out_device_ptrs) != T:
                raise ValueError("%d output frames for %d frames" % (len(out_device_ptrs), T))
            return None, (_P * T)(*[int(p) for p in out_device_ptrs]), raw.flags | on_device
        out = np.empty((T,) + tuple(raw.shape), dtype=np.float64)
        return out, (_P * T)(*[out[g].ctypes.data for g in range(T)]), raw.flags

    def wavelet_images(self, raw, out_device_ptrs=None, report=False):
        """gpet_wavelet_images: wavelet denoising of every frame of ``raw`` (a RawFrames made with ``denoise=('wavelet', kwargs)``
        or a WaveletSpec) in one batched pass -> (T, M, N) float64.  ``out_device_ptrs``: device addresses of float64 (M, N)
        frames to write instead (GPET_WV_OUT_ON_DEVICE; returns None).  The call waits for the stream: a frame whose finest
        diagonal band is all zero has no noise level and raises GpetError naming the frame.  ``report=True``: also a dict of
        ``sigma`` (T,), ``thresholds`` and ``mean_sq`` (T, levels, 3; level 1 = finest first, bands ad, da, dd) and ``coeffs``, per
        frame a list of dict(aa, ad, da, dd) per level (aa of every level but the coarsest holds the reconstruction)."""
        if raw.wv is None:
            raise ValueError("no wavelet spec")
        if not report:
            return self._run_stage(raw, raw.wv, raw.shape, out_device_ptrs)
        T = len(raw)
        levels, fd = raw.wv.pyramid(raw.shape)
        L = len(levels)
        rep = dict(sigma=np.empty(T), thresholds=np.empty((T, L, 3)), mean_sq=np.full((T, L, 3), np.nan), pyramid=np.empty((T, fd)))

        def fill(c):
            c.sigma_out, c.thresholds_out = rep["sigma"].ctypes.data, rep["thresholds"].ctypes.data
            c.mean_sq_out, c.coeffs_out = rep["mean_sq"].ctypes.data, rep["pyramid"].ctypes.data
        out = self._run_stage(raw, raw.wv, raw.shape, out_device_ptrs, fill=fill)
        pyr = rep.pop("pyramid")
        rep["coeffs"] = [[{k: pyr[g, off + b * mo * no: off + (b + 1) * mo * no].reshape(mo, no).copy()
                           for b, k in enumerate(("aa", "ad", "da", "dd"))} for mo, no, off in levels] for g in range(T)]
        if raw.wv.c.method != WV_METHODS["BayesShrink"] or raw.wv.thresholds is not None:
            rep["mean_sq"] = None
        return out, rep

    def tvb_images(self, raw, out_device_ptrs=None, return_n_iter=False):
        """gpet_tvb_images: split-Bregman TV denoising of every frame of ``raw`` (a RawFrames made with ``denoise=('tvb', kwargs)``
        or a TvbSpec) in one batched pass, one workgroup per frame -> (T, M, N) float64.  ``out_device_ptrs``: device addresses of
        float64 (M, N) frames to write instead (GPET_TVB_OUT_ON_DEVICE; returns None) -- with frames on the device too and
        without ``return_n_iter``, nothing is waited for.  ``return_n_iter``: also the sweeps every frame ran, (T,) int32."""
        if raw.tvb is None:
            raise ValueError("no split-Bregman spec")
        n_iter = np.zeros(len(raw), dtype=np.int32) if return_n_iter else None
        out = self._run_stage(raw, raw.tvb, raw.shape, out_device_ptrs, n_iter)
        return (out, n_iter) if return_n_iter else out

    def polar_images(self, raw, out_device_ptrs=None):
        """gpet_polar_images: every frame of ``raw`` (a RawFrames made with ``polar=``) unwrapped to (radius x angle) in one batched
        pass -> (T, n_r, W) float64; nothing else ``raw`` carries is applied.  ``out_device_ptrs``: device addresses of float64
        (n_r, W) frames to write instead (GPET_POLAR_OUT_ON_DEVICE; returns None) -- with frames on the device too, nothing is
        waited for."""
        if raw.polar is None:
            raise ValueError("no polar spec")
        return self._run_stage(raw, raw.polar, raw.src_shape, out_device_ptrs)

    def nlmeans_images(self, raw, out_device_ptrs=None):
        """gpet_nlmeans_images: non-local means of every frame of ``raw`` (a RawFrames made with ``denoise=('nl', kwargs)`` or a
        NlmeansSpec) in one batched pass -> (T, M, N) float64.  ``out_device_ptrs``: device addresses of float64 (M, N) frames to
        write instead (GPET_NLM_OUT_ON_DEVICE; returns None) -- with frames on the device too, nothing is waited for."""
        if raw.nlm is None:
            raise ValueError("no non-local means spec")
        return self._run_stage(raw, raw.nlm, raw.shape, out_device_ptrs)

    def nlmeans_fast_images(self, raw, out_device_ptrs=None):
        """gpet_nlmeans_fast_images: fast-mode non-local means of every frame of ``raw`` (a RawFrames made with
        ``denoise=('nl_fast', kwargs)`` or a NlmeansFastSpec) in one batched pass -> (T, M, N) float64.  ``out_device_ptrs``: device
        addresses of float64 (M, N) frames to write instead (GPET_NLM_OUT_ON_DEVICE; returns None) -- with frames on the device
        too, nothing is waited for."""
        if raw.nlf is None:
            raise ValueError("no fast-mode non-local means spec")
        return self._run_stage(raw, raw.nlf, raw.shape, out_device_ptrs)

    def label_maps(self, shape, x_st, rows, map_of=None, extend=False, transposed=False, thickness=False, out_device_ptrs=None,
                   thick_device_ptr=None):
        """gpet_label_maps: Rule 1 of include/gpet_hip.h "label maps" on injected rows -- ``shape`` = (M, N), ``x_st[e]`` the first
        column of edge e and ``rows[e]`` its int64 rows (``LABEL_NO_ROW``: the row does not count), ``map_of[e]`` its map or -1.  Returns
        (n_maps, M, N) uint8 -- (n_maps, N, M) with ``transposed`` -- and, with ``thickness``, also (n_maps, L + 1, N) int32.
        ``out_device_ptrs`` (one device address per map; ``thick_device_ptr`` for the thickness): written there instead, enqueued on
        the context's stream, nothing waited for, None returned."""
        M, N = int(shape[0]), int(shape[1])
        rows = [np.ascontiguousarray(np.asarray(r).reshape(-1), dtype=np.int64) for r in rows]
        n = len(rows)
        m, n_maps = label_map_table(map_of, n)
        xs = np.ascontiguousarray(np.asarray(x_st).reshape(-1), dtype=np.int32)
        ln = np.array([r.shape[0] for r in rows], dtype=np.int32)
        why = label_refusal(M, N, xs.tolist(), ln.tolist(), m.tolist(), n_maps) if xs.shape[0] == n else "x_st has %d entries for %d edges" % (xs.shape[0], n)
        if why is not None:
            raise ValueError(why)
        L = int(np.bincount(m[m >= 0], minlength=1).max())
        maps, op, thick, tp, flag = _label_out(n_maps, (N, M) if transposed else (M, N), out_device_ptrs,
                                               label_thick_count(n_maps, L, N) if thickness else 0, thick_device_ptr)
        flat = np.concatenate(rows) if n else np.zeros(0, dtype=np.int64)
        ip = C.POINTER(C.c_int32)
        flags = flag | (LABELS_EXTEND if extend else 0) | (LABELS_TRANSPOSED if transposed else 0)
        self.check(self.lib.gpet_label_maps(self.h, M, N, n, xs.ctypes.data_as(ip), ln.ctypes.data_as(ip), flat.ctypes.data_as(C.POINTER(C.c_int64)),
                                            m.ctypes.data_as(ip), n_maps, flags, op, tp))
        if maps is None:
            return None
        return (maps, thick.reshape(n_maps, L + 1, N)) if thickness else maps

    def label_maps_xy(self, shape, outlines, map_of=None, out_device_ptrs=None):
        """gpet_label_maps_xy: Rule 2 on injected vertices -- ``outlines[e]`` an (n, 2) float64 array of (x, y), 4 <= n <= 4096, in the
        coordinates of the (Ms, Ns) = ``shape`` frame.  Returns (n_maps, Ms, Ns) uint8: how many outlines of its map a pixel is inside."""
        Ms, Ns = int(shape[0]), int(shape[1])
        outs = [np.ascontiguousarray(np.asarray(o, dtype=np.float64).reshape(-1, 2)) for o in outlines]
        n = len(outs)
        m, n_maps = label_map_table(map_of, n)
        nv = np.array([o.shape[0] for o in outs], dtype=np.int32)
        why = label_refusal_xy(Ms, Ns, nv.tolist(), m.tolist(), n_maps)
        if why is not None:
            raise ValueError(why)
        maps, op, _, _, flag = _label_out(n_maps, (Ms, Ns), out_device_ptrs, 0, None)
        flat = np.ascontiguousarray(np.concatenate(outs, axis=0))
        ip = C.POINTER(C.c_int32)
        self.check(self.lib.gpet_label_maps_xy(self.h, Ms, Ns, n, nv.ctypes.data_as(ip), flat.ctypes.data_as(C.POINTER(C.c_double)),
                                               m.ctypes.data_as(ip), n_maps, flag, op))
        return maps

    def metrics_images(self, raw_a, raw_b, spec=None, full=False, maps_device_ptrs=None):
        """gpet_metrics_images: the four figures of the reference's ``denoise(verbose=True)`` for every pair of two stacks -- ``raw_a``
        the frames as given, ``raw_b`` the denoised frames, each a RawFrames-like object (``ptrs``, ``pix``, ``flags``, ``shape``; see
        ``metrics_frames``) on the host or on the device, of any two pixel types.  ``spec``: a GpetMetrics (``metrics_spec``).  Returns
        a (T, 4) float64 array -- psnr, ssim, nrmse, entropy -- and, with ``full``, the (T, M, N) float64 SSIM maps;
        ``maps_device_ptrs``: the maps are written to these device addresses instead (None returned for them).  A refusal in the
        words of scikit-image (the window, a float frame outside [-1, 1] without ``data_range``) raises ValueError, as the library does."""
        T, (M, N) = len(raw_a.ptrs), raw_a.shape
        if len(raw_b.ptrs) != T or tuple(raw_b.shape) != (M, N):
            raise ValueError("Input images must have the same dimensions.")
        spec = spec if spec is not None else metrics_spec()
        why = metrics_refusal(T, raw_a.pix, raw_b.pix, M, N, spec.win_size, spec.K1, spec.K2, spec.data_range,
                              0 if raw_a.flags & RAW_ON_DEVICE else M * N * PIX_BYTES[raw_a.pix],
                              0 if raw_b.flags & RAW_ON_DEVICE else M * N * PIX_BYTES[raw_b.pix])
        if why is not None:
            raise ValueError(why)
        out = np.empty((T, 4), dtype=np.float64)
        flags = (RAW_ON_DEVICE if raw_a.flags & RAW_ON_DEVICE else 0) | (METRICS_B_ON_DEVICE if raw_b.flags & RAW_ON_DEVICE else 0)
        maps, mp = None, None
        if maps_device_ptrs is not None:
            if len(maps_device_ptrs) != T:
                raise ValueError("%d maps for %d frames" % (len(maps_device_ptrs), T))
            mp, flags = (_P * T)(*[int(p) for p in maps_device_ptrs]), flags | METRICS_MAPS_ON_DEVICE
        elif full:
            maps = np.empty((T, M, N), dtype=np.float64)
            mp = (_P * T)(*[maps[g].ctypes.data for g in range(T)])
        rc = self.lib.gpet_metrics_images(self.h, (_P * T)(*raw_a.ptrs), raw_a.pix, (_P * T)(*raw_b.ptrs), raw_b.pix, T, M, N, C.byref(spec),
                                          flags, out.ctypes.data_as(C.POINTER(C.c_double)), mp)
        if rc == ERR_BAD_ARG:
            msg = (self.lib.gpet_last_error(self.h) or b"").decode()
            if msg.startswith(METRICS_RANGE_WORDS):
                raise ValueError(msg)
        self.check(rc)
        return (out, maps) if full or maps_device_ptrs is not None else out

    def denoise_images_scored(self, raw, spec=None):
        """``denoise_images`` of host frames and ``metrics_images`` of (the frames, the result) -> (result, iterations, (T, 4)
        figures).  A stage of its own writes into device memory of this call (``out_device_ptrs``), the frames are scored there and
        copied home afterwards; an in-pass technique's result comes home first and goes up again."""
        if raw.polar is not None or raw.frames is None:
            raise ValueError("scoring takes host frames without a polar spec")
        a = metrics_frames(frames=raw.frames)
        if raw.pre is None:
            out, n_iter = self.denoise_images(raw)
            return out, n_iter, self.metrics_images(a, metrics_frames(frames=out), spec)
        T, (M, N) = len(raw), raw.shape
        buf = PreFrames(self)
        try:
            ptrs = buf.reserve(T, M * N * 8)
            n_iter = np.zeros(T, dtype=np.int32)
            self._run_stage(raw, raw.pre, raw.shape, ptrs, n_iter)
            fig = self.metrics_images(a, metrics_frames(device_ptrs=ptrs, dtype=np.float64, shape=(M, N)), spec)
            out = np.empty((T, M, N), dtype=np.float64)
            for g in range(T):
                self.check(self.lib.gpet_dev_copy(self.h, out[g].ctypes.data, ptrs[g], M * N * 8, 1))
            return out, n_iter, fig
        finally:
            buf.close()

    def normalise_f32(self, img):
        a = np.ascontiguousarray(img, dtype=np.float32)
        out = np.empty_like(a)
        self.check(self.lib.gpet_normalise_f32(self.h, a.ctypes.data, a.size, out.ctypes.data))
        return out

    def close(self):
        if getattr(self, "h", None):
            for ref in list(getattr(self, "_comms", [])):  # (their buffers are freed through this context's handle)
                cm = ref()
                if cm is not None:
                    cm.close()
            self._comms = []
            for ref in list(getattr(self, "_batches", [])):
                b = ref()
                if b is not None:
                    b.close()
            self._batches = []
            if getattr(self, "_open_batches", 0) > 0:
                self._close_pending = True
                return
            self._destroy()

    def _destroy(self):
        self.lib.gpet_ctx_destroy(self.h)
        self.h = None

    def _batch_closed(self):
        self._open_batches -= 1
        if self._close_pending and self._open_batches == 0 and self.h:
            self._destroy()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id():
    """gpet_comm_unique_id: the 128 bytes rank 0 ships to every rank (any transport) before Comm(ctx, id, world, rank)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = load().gpet_comm_unique_id(buf)
    if rc:
        raise GpetError(rc, "gpet_comm_unique_id failed (is RCCL installed?)")
    return buf.raw


class Comm:
    """gpet_comm: the C ABI's RCCL communicator of one rank (one process per GPU) and its two collectives --
    the broadcast of the shared gradient image(s) into device memory and the gather of the finished traces."""

    def __init__(self, ctx: Context, unique_id, world, rank):
        self.ctx, self.lib = ctx, ctx.lib
        h = _P()
        idbuf = C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES) if unique_id is not None else None
        ctx.check(self.lib.gpet_comm_create(ctx.h, idbuf, int(world), int(rank), C.byref(h)))
        self.h = h
        self.world, self.rank = int(world), int(rank)
        self._bufs = []
        import weakref
        ctx._comms.append(weakref.ref(self))

    def block(self, n_units):
        lo, hi = C.c_int64(), C.c_int64()
        self.ctx.check(self.lib.gpet_comm_block(self.h, int(n_units), C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def bcast_grad(self, grad, shape, root=0):
        """Broadcast float32 image(s) of ``shape`` from ``root`` (``grad`` is read there only); returns the DEVICE pointer the
        collective filled, for GP_Edge_Tracing_Batch(..., grad_device_ptrs=[ptr], grad_shape=...) -- no trip through host memory
        on the receiving ranks.  The buffer lives until close()."""
        count = int(np.prod(shape))
        d = _P()
        self.ctx.check(self.lib.gpet_dev_alloc(self.ctx.h, count * 4, C.byref(d)))
        self._bufs.append(d)
        if self.rank == root:
            a = np.ascontiguousarray(grad, dtype=np.float32).reshape(-1)
            assert a.size == count
            self.ctx.check(self.lib.gpet_dev_copy(self.ctx.h, d, a.ctypes.data, count * 4, 0))
        self.ctx.check(self.lib.gpet_bcast_grad(self.h, d, count, int(root)))
        return d.value

    def download(self, dev_ptr, shape, dtype=np.float32):
        out = np.empty(shape, dtype=dtype)
        self.ctx.check(self.lib.gpet_dev_copy(self.ctx.h, out.ctypes.data, _P(dev_ptr), out.nbytes, 1))
        return out

    def gather_traces(self, local, n_edges, edge_len):
        """(n_local, edge_len, 2) int64 traces of this rank's block -> (n_edges, edge_len, 2) in global order on every rank."""
        loc = np.ascontiguousarray(np.asarray(local, dtype=np.int64).reshape(-1, int(edge_len), 2))
        lo, hi = self.block(n_edges)
        assert loc.shape[0] == hi - lo, (loc.shape, lo, hi)
        out = np.empty((int(n_edges), int(edge_len), 2), dtype=np.int64)
        self.ctx.check(self.lib.gpet_gather_traces(self.h, loc.ctypes.data if loc.size else None, int(n_edges), int(edge_len),
                                                   out.ctypes.data))
        return out

    def gather_results(self, batch, n_edges, len_cap):
        """Result records of every edge (gpet_gather_results): ``batch`` is this rank's Batch (its block of edges, after
        its converged fits) or None on a rank that owns no edges.  Returns decode_results of the n_edges records in global
        order, the same on every rank."""
        n = int(n_edges)
        raw = np.empty(max(1, n * result_bytes(len_cap)), dtype=np.uint8)
        self.ctx.check(self.lib.gpet_gather_results(self.h, batch.h if batch is not None else None, n, int(len_cap),
                                                    raw.ctypes.data))
        return decode_results(raw, n, len_cap)

    def allgather_i64(self, local, counts):
        loc = np.ascontiguousarray(np.asarray(local, dtype=np.int64).reshape(-1))
        cn = np.ascontiguousarray(np.asarray(counts, dtype=np.int64))
        assert cn.size == self.world and loc.size == cn[self.rank]
        out = np.empty(int(cn.sum()), dtype=np.int64)
        self.ctx.check(self.lib.gpet_allgather_i64(self.h, loc.ctypes.data if loc.size else None, cn.ctypes.data, out.ctypes.data))
        return out

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):  # (a context closed first has already closed this communicator: see Context.close)
                for d in self._bufs:
                    self.lib.gpet_dev_free(self.ctx.h, d)
            self._bufs = []
            self.lib.gpet_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_DT = {BUF_X_TRAIN: np.float64, BUF_Y_TRAIN: np.float64, BUF_CHOL: np.float64, BUF_ALPHA: np.float64,
       BUF_MEAN: np.float64, BUF_STD: np.float64, BUF_COV: np.float64, BUF_FACTOR: np.float64,
       BUF_EIGVALS: np.float64, BUF_NORMALS: np.float64, BUF_SAMPLES: np.float64, BUF_COSTS: np.float64,
       BUF_BEST_IDX: np.int32, BUF_BEST_COSTS: np.float64, BUF_OBS: np.int64, BUF_KDE: np.float32,
       BUF_GRAD_KDE: np.float32, BUF_GRAD: np.float32, BUF_NOISE_W: np.float64, BUF_FIN_TRAIN: np.float64,
       BUF_FIN_PAR: np.float64, BUF_FIN_STARTS: np.float64, BUF_FIN_OUT: np.float64, BUF_KDE_TILES: np.int32,
       BUF_STRUCT_Q0: np.float64, BUF_STRUCT_LAM0: np.float64, BUF_STRUCT_H: np.float64}


class Batch:
    """gpet_batch: B independent edges processed together."""

    def __init__(self, ctx: Context, grads, params, inits, share_image=False, device_ptrs=None, shape=None, raw=None,
                 image_of=None, band=None, transposed=False):
        """``grads``: float32 (M, N) arrays on the host -- or, with ``device_ptrs`` (a list of integer device
        addresses of f32 [M*N] images on the context's device, e.g. ``tensor.data_ptr()`` after an RCCL broadcast) and
        ``shape`` = (M, N), nothing on the host at all: the library consumes the device images in place.  Or ``raw`` (a
        RawFrames: frames + gradient kernel) instead of both: the gradient images are made on the device
        (gpet_batch_create_raw).  ``image_of``: an image map -- B indices into the images, of which there are then ``n_img``
        (the length of the list of images given, ``grads`` a list of (M, N) arrays or an (n_img, M, N) stack) instead of one
        or B; the library checks the map against that count (gpet_batch_create_mapped / gpet_batch_create_raw_mapped).
        ``band`` = (H, r0): tracking bands (gpet_batch_create_banded) -- the images are full frames, ``inits`` in full-frame rows,
        ``r0`` one first row per edge or None (placed from the inits); the batch's own shape ``(M, N)`` becomes (H, N),
        ``frame_M`` stays the frames', and every row the batch returns is a band row (``band_r0()`` has the offsets).
        ``transposed`` (GPET_FRAMES_TRANSPOSED): a vertical batch -- the images, of whatever kind, are (Mf, Nf) in the frame's layout
        and stay so for ``set_images`` (``frame_shape``); the batch is the one on the transposes of their gradient images, made on the
        device: ``(M, N)`` is (Nf, Mf) (banded: (H, Mf), ``frame_M`` = Nf), and ``params``, ``inits``, a band and everything the
        batch takes or returns later are in THAT image's coordinates."""
        self.ctx = ctx
        self.transposed = bool(transposed)
        tf = FRAMES_TRANSPOSED if transposed else 0
        self.lib = ctx.lib
        B = len(params)
        self._pre_buf = None  # device frames of a stage of its own in front of the raw-frame path (PreFrames), kept for set_images
        if raw is not None and raw.needs_resolve:
            self._pre_buf = PreFrames(ctx)
            raw = raw.pre_resolved(ctx, self._pre_buf)
        if image_of is not None:
            if share_image:
                raise ValueError("share_image and image_of are alternatives")
            image_of = [int(v) for v in image_of]
            if len(image_of) != B:
                raise ValueError("image_of has %d entries for %d edges" % (len(image_of), B))
            if raw is None and device_ptrs is None and np.ndim(grads) == 2:
                grads = [grads]  # (a 2-D array is ONE image)
            n_img = raw.n_slots if raw is not None else len(device_ptrs if device_ptrs is not None else grads)
            io = (C.c_int32 * B)(*image_of)
        inits = [np.ascontiguousarray(i, dtype=np.int64) for i in inits]
        if raw is not None:
            if grads is not None or device_ptrs is not None:
                raise ValueError("gradient images and raw frames are alternatives")
            self.M, self.N = raw.shape
            grads = raw  # (kept alive with the batch, like host gradient images)
        elif device_ptrs is not None:
            self.M, self.N = int(shape[0]), int(shape[1])
            gp = (_P * len(device_ptrs))(*[int(p) for p in device_ptrs])
            flags = GRAD_ON_DEVICE
            grads = None
        else:
            grads = [np.ascontiguousarray(g, dtype=np.float32) for g in grads]
            self.M, self.N = grads[0].shape
            gp = (_P * len(grads))(*[g.ctypes.data for g in grads])
            flags = 0
        ip = (_P * B)(*[i.ctypes.data for i in inits])
        pa = (GpetParams * B)(*params)
        h = _P()
        self.frame_M = self.M  # (rows of the frames set_images takes; a banded batch's own M is H)
        self.band_rows = None
        if band is not None:
            H, r0 = int(band[0]), band[1]
            pair_of = image_of if image_of is not None else ([0] * B if share_image else list(range(B)))
            n_pair = max(pair_of) + 1
            r0a = None if r0 is None else np.ascontiguousarray(np.asarray(r0).reshape(-1), dtype=np.int64)
            if r0a is not None and r0a.shape[0] != B:
                raise ValueError("band_r0 has %d entries for %d edges" % (r0a.shape[0], B))
            bd = GpetBand(H, n_pair, None if r0a is None else r0a.ctypes.data_as(C.POINTER(C.c_int64)), (C.c_int32 * B)(*pair_of))
            im = GpetBandImages()
            if raw is not None:
                nk, kp, kh, kw, fo, ko = raw.multi_args()  # (one kernel: on every frame in order)
                pr = raw.pointer_array()
                im.raw, im.pix, im.n_frames, im.n_kern = C.cast(pr, C.POINTER(C.c_void_p)), raw.pix, len(raw), nk
                im.kern, im.kh, im.kw, im.frame_of, im.kernel_of = C.cast(kp, C.POINTER(C.c_void_p)), kh, kw, fo, ko
                if raw.dn is not None:
                    im.dn = C.pointer(raw.dn)
                im.flags = raw.flags | tf
            else:
                im.grad, im.flags = C.cast(gp, C.POINTER(C.c_void_p)), flags | tf
            ctx.check(self.lib.gpet_batch_create_banded(ctx.h, B, self.M, self.N, C.byref(bd), C.byref(im), pa, ip, C.byref(h)))
            self.band_rows = H
        elif image_of is not None:  # (the library checks the map: its message says what is wrong with it)
            if raw is not None and raw.slots is not None:
                ctx.check(self.lib.gpet_batch_create_raw_multi(ctx.h, B, self.M, self.N, n_img, io, len(raw), raw.pointer_array(), raw.pix,
                                                               *raw.multi_args(), raw.dn_arg(), pa, ip, raw.flags | tf, C.byref(h)))
            elif raw is not None:
                ctx.check(self.lib.gpet_batch_create_raw_mapped(ctx.h, B, self.M, self.N, n_img, io, raw.pointer_array(), raw.pix,
                                                                *raw.kernel_args(), raw.dn_arg(), pa, ip, raw.flags | tf, C.byref(h)))
            else:
                ctx.check(self.lib.gpet_batch_create_mapped(ctx.h, B, self.M, self.N, n_img, io, gp, pa, ip, flags | tf, C.byref(h)))
        elif raw is not None:
            if raw.slots is not None:
                raise ValueError("a slot table comes with the image map of its slots (image_of)")
            assert len(raw) == (1 if share_image else B)
            if raw.dn is not None:
                ctx.check(self.lib.gpet_batch_create_raw_dn(ctx.h, B, self.M, self.N, raw.pointer_array(), raw.pix, *raw.kernel_args(),
                                                            raw.dn_arg(), 1 if share_image else 0, pa, ip, raw.flags | tf, C.byref(h)))
            else:
                ctx.check(self.lib.gpet_batch_create_raw(ctx.h, B, self.M, self.N, raw.pointer_array(), raw.pix, *raw.kernel_args(),
                                                         1 if share_image else 0, pa, ip, raw.flags | tf, C.byref(h)))
        else:
            ctx.check(self.lib.gpet_batch_create2(ctx.h, B, self.M, self.N, gp, 1 if share_image else 0, pa, ip, flags | tf,
                                                  C.byref(h)))
        if transposed:  # (from here on the batch's own shape: rows of G.T are the frame's columns)
            self.M, self.N = self.N, self.M
            self.frame_M = self.M
        if self.band_rows is not None:
            self.M = self.band_rows
        self.h = h
        self.B = B
        import weakref
        ctx._batches.append(weakref.ref(self))
        ctx._open_batches += 1
        if len(ctx._batches) > 4096:
            ctx._batches[:] = [r for r in ctx._batches if r() is not None and getattr(r(), "h", None)]
        _live_batches.append(weakref.ref(self))
        if len(_live_batches) > 4096:  # (drop the references of batches that are gone)
            _live_batches[:] = [r for r in _live_batches if r() is not None and getattr(r(), "h", None)]
        self._scored = False
        self.share_image = bool(share_image)
        self.n_img = self.lib.gpet_batch_image_count(h)  # images the batch holds: 1 shared, B own, or the map's
        self.image_of = image_of
        self._keep = (grads, inits)
        self._x_st = [int(p.x_st) for p in params]
        self._n_init = [int(p.n_init) for p in params]

    @property
    def frame_shape(self):
        """The shape of the images ``set_images`` takes, as they lie in the caller's memory."""
        return (self.N, self.frame_M) if self.transposed else (self.frame_M, self.N)

    def set_images(self, grads=None, device_ptrs=None, next_frame=False, raw=None):
        """New gradient image(s) for the same edges, gradient KDE recomputed, loop state reset (gpet_batch_set_images).
        ``next_frame``: the images are the next frames of the sequences just traced, so an any-rank factor may start from
        the last trace's rows (GPET_IMAGES_NEXT_FRAME); otherwise nothing of an earlier trace is used."""
        n_img = self.n_img
        nf = IMAGES_NEXT_FRAME if next_frame else 0
        if raw is not None:  # (a RawFrames: gpet_batch_set_raw_images)
            if grads is not None or device_ptrs is not None:
                raise ValueError("gradient images and raw frames are alternatives")
            assert raw.n_slots == n_img and tuple(raw.shape) == self.frame_shape
            if raw.needs_resolve:  # (refused before the images are swapped: the batch stays on its old frames)
                if self._pre_buf is None:
                    self._pre_buf = PreFrames(self.ctx)
                raw = raw.pre_resolved(self.ctx, self._pre_buf)
            if raw.slots is not None:  # (gpet_batch_set_raw_images_multi: the library checks the table)
                self.ctx.check(self.lib.gpet_batch_set_raw_images_multi(self.h, len(raw), raw.pointer_array(), raw.pix, *raw.multi_args(),
                                                                        raw.dn_arg(), raw.flags | nf))
            elif raw.dn is not None:
                self.ctx.check(self.lib.gpet_batch_set_raw_images_dn(self.h, raw.pointer_array(), raw.pix, *raw.kernel_args(),
                                                                     raw.dn_arg(), raw.flags | nf))
            else:
                self.ctx.check(self.lib.gpet_batch_set_raw_images(self.h, raw.pointer_array(), raw.pix, *raw.kernel_args(), raw.flags | nf))
            return
        if device_ptrs is not None:
            assert len(device_ptrs) == n_img
            gp = (_P * n_img)(*[int(p) for p in device_ptrs])
            self.ctx.check(self.lib.gpet_batch_set_images(self.h, gp, GRAD_ON_DEVICE | nf))
            return
        grads = [np.ascontiguousarray(g, dtype=np.float32) for g in grads]
        assert len(grads) == n_img and all(g.shape == self.frame_shape for g in grads)
        gp = (_P * n_img)(*[g.ctypes.data for g in grads])
        self.ctx.check(self.lib.gpet_batch_set_images(self.h, gp, nf))

    def _max_info(self, key):
        """max over the edges of a creation-time constant of gpet_batch_info (cached)."""
        cache = self.__dict__.setdefault("_info_max", {})
        if key not in cache:
            cache[key] = max(self.info(e)[key] for e in range(self.B))
        return cache[key]

    def info(self, e=0):
        v = (C.c_int32 * 18)()
        self.ctx.check(self.lib.gpet_batch_info(self.h, e, v, 18))
        # (the last four are the batch's normals store: iterations held per edge -- 0 before the first trace and where there is
        #  none --, its size, the (edge, iteration) streams the loop has generated so far for iterations the edge went on to run, and
        #  the streams its store launches drew, exactly)
        keys = ["Lg", "S", "n_keep", "n_cap", "factor_cap", "z_cols", "factor_rows_cap", "n_bins", "obs_cap",
                "algo_thresh", "structured", "r0", "z_ring", "arena_mib", "zstore_iters", "zstore_mib", "normals_generated", "normals_drawn"]
        return dict(zip(keys, list(v)))

    def scalars(self, e=0) -> GpetScalars:
        s = GpetScalars()
        self.ctx.check(self.lib.gpet_batch_read(self.h, e, BUF_SCALARS, C.byref(s), C.sizeof(s)))
        return s

    def write_scalars(self, s, e=0):
        self.ctx.check(self.lib.gpet_batch_write(self.h, e, BUF_SCALARS, C.byref(s), C.sizeof(s), 0))

    @property
    def have_scores(self):
        """True once a scoring pass has left costs / best indices on the device (gpet_score_curves or the loop)."""
        return bool(self._scored)

    def all_scalars(self):
        arr = (GpetScalars * self.B)()
        self.ctx.check(self.lib.gpet_batch_read_scalars_all(self.h, arr))
        return list(arr)

    def set_obs(self, e, obs_xy):
        o = np.ascontiguousarray(np.asarray(obs_xy).reshape(-1, 2), dtype=np.int64)
        self.ctx.check(self.lib.gpet_batch_set_obs(self.h, e, o.ctypes.data if o.size else None, o.shape[0]))

    def warm_start(self, warm_every):
        """gpet_batch_warm_start: every edge's observation set for the next frame from its last converged fit, on the device
        (the rule of sequence.warm_start_obs).  Returns the sizes of the sets."""
        cnt = np.zeros(self.B, dtype=np.int32)
        self.ctx.check(self.lib.gpet_batch_warm_start(self.h, int(warm_every), cnt.ctypes.data_as(C.POINTER(C.c_int32))))
        return cnt

    def warm_start_ready(self):
        """Raises what warm_start would raise now (GpetError: no converged fits of a last trace), and touches nothing."""
        self.ctx.check(self.lib.gpet_batch_warm_start_ready(self.h))

    def read(self, which, e=0):
        inf = self.info(e)
        s = self.scalars(e)
        Lg, S = inf["Lg"], inf["S"]
        shape = {BUF_X_TRAIN: (s.n,), BUF_Y_TRAIN: (s.n,), BUF_NOISE_W: (s.n,), BUF_ALPHA: (s.n,),
                 BUF_CHOL: (s.n, s.n), BUF_MEAN: (Lg,), BUF_STD: (Lg,), BUF_COV: (Lg, Lg),
                 BUF_FACTOR: (s.rank, Lg), BUF_EIGVALS: (s.rank,), BUF_NORMALS: (S, inf["z_cols"]),
                 BUF_SAMPLES: (S, Lg), BUF_COSTS: (S,), BUF_BEST_IDX: (inf["n_keep"],),
                 BUF_BEST_COSTS: (inf["n_keep"],), BUF_OBS: (s.n_obs, 2), BUF_KDE: (self.M, self.N),
                 BUF_GRAD_KDE: (self.M, self.N), BUF_GRAD: (self.M, self.N), BUF_FIN_TRAIN: (3, inf["n_cap"]),
                 BUF_FIN_PAR: (12,), BUF_FIN_STARTS: (13, 3), BUF_FIN_OUT: (2, Lg),
                 BUF_KDE_TILES: ((self.N + 15) // 16 + 1, 2),  # (the last row: the two u32 keys of the raw minimum / maximum)
                 BUF_STRUCT_Q0: (inf["r0"], Lg), BUF_STRUCT_LAM0: (inf["r0"],), BUF_STRUCT_H: (inf["r0"], inf["r0"])}[which]
        out = np.zeros(shape, dtype=_DT[which])
        if which in (BUF_STRUCT_Q0, BUF_STRUCT_LAM0, BUF_STRUCT_H) and not inf["structured"]:
            out = np.zeros(1, dtype=np.float64)  # (the library refuses these on a batch that is not structured: let it say so)
        if out.size:
            self.ctx.check(self.lib.gpet_batch_read(self.h, e, which, out.ctypes.data, out.nbytes))
        return out

    def write(self, which, arr, e=0, rows=0):
        a = np.ascontiguousarray(arr, dtype=_DT[which])
        self.ctx.check(self.lib.gpet_batch_write(self.h, e, which, a.ctypes.data, a.nbytes, int(rows)))

    def clear_injected_factor(self, e=0):
        self.ctx.check(self.lib.gpet_batch_clear_injected_factor(self.h, e))

    def fit_predict(self, want_cov=True):
        self.ctx.check(self.lib.gpet_gp_fit_predict(self.h, 1 if want_cov else 0))

    def factor(self):
        self.ctx.check(self.lib.gpet_gp_factor(self.h))

    def normals(self, seeds):
        s = (C.c_uint32 * self.B)(*[int(v) & 0xFFFFFFFF for v in seeds])
        self.ctx.check(self.lib.gpet_gp_normals(self.h, s))

    def sample(self):
        self.ctx.check(self.lib.gpet_gp_sample(self.h))

    def score(self):
        self.ctx.check(self.lib.gpet_score_curves(self.h))
        self._scored = True

    def reset(self):
        self.ctx.check(self.lib.gpet_batch_reset(self.h))

    def profile_stage(self, stage, reps=10):
        ms = C.c_float()
        self.ctx.check(self.lib.gpet_profile_stage(self.h, int(stage), int(reps), C.byref(ms)))
        return ms.value

    def final_set_training(self, e, xs, ys, w):
        xs, ys, w = (np.ascontiguousarray(a, dtype=np.float64) for a in (xs, ys, w))
        self.ctx.check(self.lib.gpet_final_set_training(self.h, e, xs.ctypes.data, ys.ctypes.data, w.ctypes.data,
                                                        xs.shape[0]))

    def read_obs_all(self):
        cap = self._max_info("obs_cap")
        dst = np.zeros((self.B, cap, 2), dtype=np.int64)
        cnt = np.zeros(self.B, dtype=np.int32)
        self.ctx.check(self.lib.gpet_batch_read_obs_all(self.h, dst.ctypes.data, cnt.ctypes.data, cap))
        return [dst[e, :cnt[e]].copy() for e in range(self.B)]

    def final_set_training_all(self, xs_list, ys_list, w_list):
        n = np.asarray([len(x) for x in xs_list], dtype=np.int32)
        stride = int(n.max())

        def pack(lst):
            out = np.zeros((len(lst), stride))
            for i, a in enumerate(lst):
                out[i, :n[i]] = a
            return out
        xs, ys, w = pack(xs_list), pack(ys_list), pack(w_list)
        self.ctx.check(self.lib.gpet_final_set_training_all(self.h, xs.ctypes.data, ys.ctypes.data, w.ctypes.data,
                                                            n.ctypes.data, stride))

    def final_predict_all(self, par):
        par = np.ascontiguousarray(par, dtype=np.float64).reshape(self.B, 12)
        Lg = self._max_info("Lg")
        mean = np.zeros((self.B, Lg))
        std = np.zeros((self.B, Lg))
        self.ctx.check(self.lib.gpet_final_predict_all(self.h, par.ctypes.data, mean.ctypes.data, std.ctypes.data, Lg))
        return mean, std

    def final_fit_all(self, seeds):
        """Converged fits of every edge on the device (gpet_final_fit_all).  Returns (mean [B, Lg_max] in pixels,
        std [B, Lg_max] in standardised units, theta [B, 3], minimum of -LML [B], objective launches)."""
        s = (C.c_uint32 * self.B)(*[int(v) & 0xFFFFFFFF for v in seeds])
        Lg = self._max_info("Lg")
        mean = np.zeros((self.B, Lg))
        std = np.zeros((self.B, Lg))
        th = np.zeros((self.B, 4))
        rounds = C.c_int32()
        self.ctx.check(self.lib.gpet_final_fit_all(self.h, s, mean.ctypes.data, std.ctypes.data, th.ctypes.data, Lg,
                                                   C.byref(rounds)))
        return mean, std, th[:, :3].copy(), th[:, 3].copy(), rounds.value

    def results(self, len_cap=None):
        """Result records of every edge (gpet_batch_results), valid after final_fit_all on the current trace: a dict of
        numpy arrays as decode_results returns it.  ``len_cap`` defaults to the widest edge."""
        L = self._max_info("Lg") if len_cap is None else int(len_cap)
        raw = np.empty(max(1, self.B * result_bytes(L)), dtype=np.uint8)
        self.ctx.check(self.lib.gpet_batch_results(self.h, L, raw.ctypes.data, 0))
        return decode_results(raw, self.B, L)

    def label_maps(self, map_of=None, extend=False, transposed=False, thickness=False, out_device_ptrs=None, thick_device_ptr=None):
        """gpet_batch_label_maps: Rule 1 of include/gpet_hip.h "label maps" from the converged fits where they lie -- valid when
        ``results`` is.  ``map_of`` one map index per edge, -1 for none (None: all edges on map 0).  Returns (n_maps, M, N) uint8 in the
        batch's full-frame shape -- ``(frame_M, N)``; with ``transposed`` (N, frame_M) -- and with ``thickness`` also (n_maps, L + 1, N)
        int32.  ``out_device_ptrs`` / ``thick_device_ptr``: written there instead, enqueued only, None returned."""
        m, n_maps = label_map_table(map_of, self.B)
        why, L = _label_refusal_maps(False, self.frame_M, self.N, m.tolist(), n_maps, "edge")
        if why is not None:
            raise ValueError(why)
        M, N = self.frame_M, self.N
        maps, op, thick, tp, flag = _label_out(n_maps, (N, M) if transposed else (M, N), out_device_ptrs,
                                               label_thick_count(n_maps, L, N) if thickness else 0, thick_device_ptr)
        flags = flag | (LABELS_EXTEND if extend else 0) | (LABELS_TRANSPOSED if transposed else 0)
        self.ctx.check(self.lib.gpet_batch_label_maps(self.h, m.ctypes.data_as(C.POINTER(C.c_int32)), n_maps, flags, op, tp))
        if maps is None:
            return None
        return (maps, thick.reshape(n_maps, L + 1, N)) if thickness else maps

    def label_maps_xy(self, polar, shape, map_of=None, out_device_ptrs=None):
        """gpet_batch_label_maps_xy: Rule 2 from the converged fits of a batch on polar frames -- ``polar`` the resolved PolarSpec the
        frames were unwrapped with (one centre, or one per map), ``shape`` = (Ms, Ns) of the source frames.  Returns (n_maps, Ms, Ns)
        uint8."""
        Ms, Ns = int(shape[0]), int(shape[1])
        m, n_maps = label_map_table(map_of, self.B)
        why, _ = _label_refusal_maps(polar is None, Ms, Ns, m.tolist(), n_maps, "edge")
        if why is not None:
            raise ValueError(why)
        maps, op, _, _, flag = _label_out(n_maps, (Ms, Ns), out_device_ptrs, 0, None)
        c, keep = polar.call_arg()
        self.ctx.check(self.lib.gpet_batch_label_maps_xy(self.h, C.byref(c), Ms, Ns, m.ctypes.data_as(C.POINTER(C.c_int32)), n_maps, flag, op))
        del keep
        return maps

    def final_costs(self):
        """The scorer's cost of every edge's converged mean curve on its own gradient image, (B,) f64 (gpet_batch_final_costs:
        the reference's cost_funct(optim_mean_curve), gpet.py:888-890); +inf for an edge whose device status is not OK.  Valid
        when ``results`` is; the loop's samples and scores are not touched."""
        out = np.empty(self.B, dtype=np.float64)
        self.ctx.check(self.lib.gpet_batch_final_costs(self.h, out.ctypes.data, 0))
        return out

    def ensemble(self, group_of, tol=2.0, len_cap=None, device_ptr=None):
        """Per-column consensus over the converged fits of every group of edges (gpet_batch_ensemble; include/gpet_hip.h has the
        definition): ``group_of`` one group index per edge (-1: in no group), ``tol`` in pixels.  Returns ``decode_ensemble``'s
        (groups, cost, off).  ``device_ptr``: the buffer (``ensemble_bytes`` bytes of device memory) is filled on the device
        instead and nothing is returned; the call is then only enqueued on the context's stream."""
        g, n_groups = check_group_table(group_of, self.B)
        if not float(tol) >= 0.0:
            raise ValueError("tol must be >= 0 pixels, not %r" % (tol,))
        L = self._max_info("Lg") if len_cap is None else int(len_cap)
        gp = g.ctypes.data_as(C.POINTER(C.c_int32))
        if device_ptr is not None:
            self.ctx.check(self.lib.gpet_batch_ensemble(self.h, n_groups, gp, float(tol), L, int(device_ptr), 1))
            return None
        raw = np.empty(ensemble_layout(n_groups, self.B, L)["total_bytes"], dtype=np.uint8)
        self.ctx.check(self.lib.gpet_batch_ensemble(self.h, n_groups, gp, float(tol), L, raw.ctypes.data, 0))
        return decode_ensemble(raw, n_groups, self.B, L, g)

    def ensemble_keep(self, group_of, tol=2.0):
        """gpet_batch_ensemble_keep: the reduction of ``ensemble`` into an allocation the batch owns, to warm-start the next frame
        from (``warm_start_groups``).  Call it before the images are swapped: the final costs are scored on the current ones."""
        g, n_groups = check_group_table(group_of, self.B)
        if not float(tol) >= 0.0:
            raise ValueError("tol must be >= 0 pixels, not %r" % (tol,))
        self._kept_groups = None
        self.ctx.check(self.lib.gpet_batch_ensemble_keep(self.h, n_groups, g.ctypes.data_as(C.POINTER(C.c_int32)), float(tol)))
        self._kept_groups = (g, n_groups)

    def ensemble_kept(self, len_cap=None, device_ptr=None, raw=False):
        """gpet_batch_ensemble_kept: the kept ensemble as ``ensemble`` returns it -- ``decode_ensemble``'s (groups, cost, off), or
        with ``raw`` the bytes themselves; ``device_ptr``: copied there on the device instead, nothing returned.  GpetError when
        none is kept."""
        L = self._max_info("Lg") if len_cap is None else int(len_cap)
        if device_ptr is not None:
            self.ctx.check(self.lib.gpet_batch_ensemble_kept(self.h, L, int(device_ptr), 1))
            return None
        kept = getattr(self, "_kept_groups", None)
        n_groups = kept[1] if kept else 1
        buf = np.empty(ensemble_layout(n_groups, self.B, L)["total_bytes"], dtype=np.uint8)
        self.ctx.check(self.lib.gpet_batch_ensemble_kept(self.h, L, buf.ctypes.data, 0))
        return buf if raw else decode_ensemble(buf, n_groups, self.B, L, kept[0] if kept else None)

    def warm_start_groups(self, frm, warm_every):
        """gpet_batch_warm_start_groups: every edge's observation set for the next frame from the source of its group in the kept
        ensemble -- ``frm`` 'medoid', 'best_cost' or 'consensus' -- on the device; edges in no group from their own fit, the edges
        of a group without members get none.  Returns (sizes of the sets, source per edge: an edge index, WARM_SRC_NONE or
        WARM_SRC_CONSENSUS)."""
        cnt, src = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        p = C.POINTER(C.c_int32)
        self.ctx.check(self.lib.gpet_batch_warm_start_groups(self.h, warm_from(frm), int(warm_every), cnt.ctypes.data_as(p),
                                                             src.ctypes.data_as(p)))
        return cnt, src

    def warm_start_from(self, src_of, warm_every):
        """gpet_batch_warm_start_from: edge e's observation set for the next frame from the last converged fit of edge
        ``src_of[e]`` (-1: the empty set).  Returns the sizes of the sets."""
        src = np.ascontiguousarray(np.asarray(src_of).reshape(-1), dtype=np.int32)
        if src.shape[0] != self.B:
            raise ValueError("src_of has %d entries for %d edges" % (src.shape[0], self.B))
        cnt = np.zeros(self.B, dtype=np.int32)
        p = C.POINTER(C.c_int32)
        self.ctx.check(self.lib.gpet_batch_warm_start_from(self.h, src.ctypes.data_as(p), int(warm_every), cnt.ctypes.data_as(p)))
        return cnt

    def band_place(self, src_of=None, frm=None):
        """gpet_batch_band_place: every edge's band for the next frame from the trace of its source, on the device, before the images
        are swapped -- ``src_of`` a table as ``warm_start_from`` takes it; else ``frm`` ('medoid', 'best_cost', 'consensus': the source of
        the edge's group in the kept ensemble); else the edge itself.  Enqueued only: ``band_r0()`` reads the table after the swap."""
        p = C.POINTER(C.c_int32)
        if src_of is not None:
            src = np.ascontiguousarray(np.asarray(src_of).reshape(-1), dtype=np.int32)
            if src.shape[0] != self.B:
                raise ValueError("src_of has %d entries for %d edges" % (src.shape[0], self.B))
            self.ctx.check(self.lib.gpet_batch_band_place(self.h, src.ctypes.data_as(p), -1))
            return
        self.ctx.check(self.lib.gpet_batch_band_place(self.h, None, -1 if frm is None else warm_from(frm)))

    def band_set(self, r0):
        """gpet_batch_band_set: the bands of the next swap, one first row per edge; GpetError (nothing touched) for a band that cannot
        hold its edge's init points."""
        a = np.ascontiguousarray(np.asarray(r0).reshape(-1), dtype=np.int64)
        if a.shape[0] != self.B:
            raise ValueError("band has %d entries for %d edges" % (a.shape[0], self.B))
        self.ctx.check(self.lib.gpet_batch_band_set(self.h, a.ctypes.data_as(C.POINTER(C.c_int64))))

    def band_r0(self):
        """gpet_batch_band_r0: the first row of every edge's band as the image slots are now, (B,) int64."""
        out = np.zeros(self.B, dtype=np.int64)
        self.ctx.check(self.lib.gpet_batch_band_r0(self.h, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def _init_table(self, flat):
        return [flat[e, :n].copy() for e, n in enumerate(self._n_init)]

    def init_follow(self, window, cols):
        """gpet_batch_init_follow: every init point of every edge moves onto the edge of the image its edge reads now, by the rule of
        csrc/gpet_init_plan.h (rows within ``window`` of the point, scored over ``cols`` columns on either side; x stays), on the device.
        Legal before the first iteration after creation, ``reset`` or ``set_images`` (GpetError ERR_STATE otherwise, nothing touched).
        Returns the moved points, a list of (n_init, 2) int64 xy arrays in full-frame rows, after one wait."""
        out = np.zeros((self.B, max(self._n_init), 2), dtype=np.int64)
        self.ctx.check(self.lib.gpet_batch_init_follow(self.h, int(window), int(cols), out.ctypes.data_as(C.POINTER(C.c_int64))))
        return self._init_table(out)

    def set_init(self, inits):
        """gpet_batch_set_init: the caller's init points, one (n_init, 2) xy array per edge in full-frame rows, sorted by x as the batch
        holds them.  The counts and the x of every point must be the batch's, the rows inside the frame and, on a banded batch, inside
        the edge's current band: GpetError ERR_BAD_ARG naming the cause otherwise, ERR_STATE after the first iteration; nothing is
        touched by a refused call."""
        inits = [np.ascontiguousarray(np.asarray(i).reshape(-1, 2), dtype=np.int64) for i in inits]
        if len(inits) != self.B:
            raise GpetError(ERR_BAD_ARG, "set_init: %d init arrays for %d edges" % (len(inits), self.B))
        for e, (i, n) in enumerate(zip(inits, self._n_init)):
            if i.shape[0] != n:
                raise GpetError(ERR_BAD_ARG, "set_init: edge %d has %d init points, the batch was created with %d" % (e, i.shape[0], n))
        ip = (_P * self.B)(*[i.ctypes.data for i in inits])
        self.ctx.check(self.lib.gpet_batch_set_init(self.h, ip))

    def init_xy(self):
        """gpet_batch_init_xy: the current init points, a list of (n_init, 2) int64 xy arrays in full-frame rows."""
        out = np.zeros((self.B, max(self._n_init), 2), dtype=np.int64)
        self.ctx.check(self.lib.gpet_batch_init_xy(self.h, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return self._init_table(out)

    def set_history(self, level, iter_cap=64):
        """Iteration history of the traces this batch runs (gpet_batch_set_history): ``level`` None / 'obs' / 'curves' / 'full'
        (or 0..3), ``iter_cap`` records per edge.  None frees the storage."""
        self.ctx.check(self.lib.gpet_batch_set_history(self.h, history_level(level), int(iter_cap)))

    def history_layout(self):
        p = GpetHistoryPlan()
        self.ctx.check(self.lib.gpet_history_layout(self.h, C.byref(p)))
        return p

    def history_record(self):
        """gpet_history_record: the history kernel once on what the buffers hold (tests inject their own)."""
        self.ctx.check(self.lib.gpet_history_record(self.h))

    def history(self):
        """The iteration history of the current trace, one dict per edge (decode_history): one copy, one wait.  GpetError
        (ERR_STATE) when the batch keeps none."""
        p = self.history_layout()
        raw = np.empty(self.B * p.edge_bytes, dtype=np.uint8)
        self.ctx.check(self.lib.gpet_batch_history(self.h, -1, raw.ctypes.data, raw.nbytes, 0))
        cache = self.__dict__.setdefault("_hist_dims", None)
        if cache is None:
            inf = [self.info(e) for e in range(self.B)]
            cache = self._hist_dims = ([i["Lg"] for i in inf], [i["obs_cap"] for i in inf])
        return decode_history(raw, p, cache[0], cache[1], self._x_st)

    def set_option(self, name, value):
        """This batch's own copy of a tuning switch (gpet_batch_set_option); returns the previous value (-1 = automatic)."""
        old = self.get_option(name)
        if self.lib.gpet_batch_set_option(self.h, name.encode(), int(value)) < 0:
            raise ValueError("unknown option %r" % (name,))
        return old

    def get_option(self, name):
        v = C.c_int()
        if self.lib.gpet_batch_get_option(self.h, name.encode(), C.byref(v)) != 0:
            raise ValueError("unknown option %r" % (name,))
        return v.value

    def set_rng(self, rng):
        """Random numbers of the batch: "mt19937" (default: numpy's RandomState stream, the reference's) or "philox"
        (gpet_batch_set_rng: counter-based Philox4x32-10 + Box-Muller, opt-in, not the reference's numbers)."""
        if rng not in (None, "mt19937", "philox"):
            raise ValueError("rng must be 'mt19937' or 'philox'")
        self.ctx.check(self.lib.gpet_batch_set_rng(self.h, 1 if rng == "philox" else 0))

    def set_sample_dtype(self, dtype):
        """Type of the posterior samples: "f64" (default, the reference's), "f32" (gpet_batch_set_sample_dtype: the GEMM
        multiplies in f64 and rounds on store, consumers widen; opt-in, BASELINE config 2's "fp32 posterior samples") or
        "f32mma" (gpet_batch_set_sample_arith: f32 storage AND the GEMM on the f32 matrix cores -- per sample a k-ascending
        chain of fmaf over the narrowed normals and factor, then (acc + mean) * y_s in f64; include/gpet_hip.h has the
        definition, tests/f32_chain.py evaluates it; opt-in, not the reference's numbers)."""
        if dtype not in (None, "f64", "f32", "f32mma", "float64", "float32"):
            raise ValueError("sample_dtype must be 'f64', 'f32' or 'f32mma'")
        if dtype == "f32mma":
            self.ctx.check(self.lib.gpet_batch_set_sample_arith(self.h, SAMPLE_ARITH_F32))
        else:  # (sets the arithmetic back to f64 as well)
            self.ctx.check(self.lib.gpet_batch_set_sample_dtype(self.h, 1 if dtype in ("f32", "float32") else 0))

    def final_optimize(self, starts, bounds):
        """Device L-BFGS-B on the training sets of final_set_training(_all) (gpet_final_optimize): starts
        (B, n_starts, 3) = log(constant, length_scale, noise_level), bounds (3, 2) in the same space.  Returns
        (theta [B, 3] of the best start per edge, its -LML [B], objective rounds)."""
        starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(self.B, -1, 3)
        bounds = np.ascontiguousarray(bounds, dtype=np.float64).reshape(3, 2)
        th = np.zeros((self.B, 4))
        rounds = C.c_int32()
        self.ctx.check(self.lib.gpet_final_optimize(self.h, starts.shape[1], starts.ctypes.data, bounds.ctypes.data,
                                                    th.ctypes.data, C.byref(rounds)))
        return th[:, :3].copy(), th[:, 3].copy(), rounds.value

    def final_problems(self):
        """Every (edge, start) problem of the last final_fit_all / final_optimize (gpet_final_problems), edge-major: dict of
        x [P, 3], f [P], g [P, 3], iter, nfev, why [P] (integers)."""
        n = C.c_int32()
        self.ctx.check(self.lib.gpet_final_problems(self.h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 10))
        self.ctx.check(self.lib.gpet_final_problems(self.h, out.ctypes.data, n.value, C.byref(n)))
        return dict(x=out[:, 0:3].copy(), f=out[:, 3].copy(), g=out[:, 4:7].copy(), iter=out[:, 7].astype(np.int64),
                    nfev=out[:, 8].astype(np.int64), why=out[:, 9].astype(np.int64))

    def lml_batch(self, edge_of, theta):
        edge_of = np.ascontiguousarray(edge_of, dtype=np.int32)
        theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(-1, 3)
        P = theta.shape[0]
        f = np.empty(P)
        g = np.empty((P, 3))
        self.ctx.check(self.lib.gpet_lml_batch(self.h, P, edge_of.ctypes.data, theta.ctypes.data, f.ctypes.data,
                                               g.ctypes.data))
        return f, g

    def lml_stats(self, reset=False):
        ms, ev, la = C.c_double(), C.c_int64(), C.c_int32()
        self.ctx.check(self.lib.gpet_lml_stats(self.h, int(bool(reset)), C.byref(ms), C.byref(ev), C.byref(la)))
        return dict(kernel_ms=ms.value, evaluations=ev.value, launches=la.value)

    def select_pixels(self):
        self.ctx.check(self.lib.gpet_select_pixels(self.h))

    def select_pixels_only(self):
        self.ctx.check(self.lib.gpet_select_pixels_only(self.h))

    def select_pixels_loop(self):
        """gpet_select_pixels_loop: select_pixels by the launches of the device loop -- BUF_KDE keeps the raw density of the
        tiles' row bands only."""
        self.ctx.check(self.lib.gpet_select_pixels_loop(self.h))

    def curve_kde(self):
        self.ctx.check(self.lib.gpet_curve_kde(self.h))

    def final_cov(self):
        self.ctx.check(self.lib.gpet_final_cov(self.h))

    def iterate(self, base_seeds, max_iters):
        s = (C.c_uint32 * self.B)(*[int(v) & 0xFFFFFFFF for v in base_seeds])
        n = C.c_int()
        self.ctx.check(self.lib.gpet_trace_iterate(self.h, s, int(max_iters), C.byref(n)))
        self._scored = self._scored or int(max_iters) > 0
        return n.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.gpet_batch_destroy(self.h)
            self.h = None
            if getattr(self, "_pre_buf", None) is not None:
                self._pre_buf.close()
            self.ctx._batch_closed()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
