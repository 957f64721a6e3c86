"""A restatement of scikit-image 0.18.3's ``denoise_tv_bregman(image, weight, max_iter=100, eps=1e-3, isotropic=True)`` for a 2-D
single-channel frame, in plain Python floats (IEEE float64, no fused multiply-add, sums left to right as written), as
csrc/gpet_tvb_plan.h states it: ``raster`` sweeps the cells in raster order as the library does, ``diagonal`` sweeps the
anti-diagonals r + c = d in ascending d, a whole diagonal at a time with numpy (every cell then has the operands it had in raster
order).  ``order`` says how the squared changes under the stopping rule are added: 'raster' as the library adds them, 'device' as
the plan header's tvb_acc_sum does (THREADS lanes, each adding its own cells in step order, then a halving tree)."""
import math

import numpy as np

THREADS = 512           # TVB_THREADS
SWEEPS_PER_LAUNCH = 4   # TVB_SWEEPS_PER_LAUNCH
DIAG_MAX = 768          # TVB_DIAG_MAX


def acc_bound(n):
    """Relative distance two orders of adding n non-negative terms can lie apart."""
    return 2.0 * (n - 1) * 2.0 ** -53


def as_input(img):
    """The frame as the stage takes it: f64 as it is, f32 widened, u8 / u16 times the rounded reciprocal of 255 / 65535."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img.astype(np.float64) * (1.0 / 255.0)
    if img.dtype == np.uint16:
        return img.astype(np.float64) * (1.0 / 65535.0)
    return img.astype(np.float64)


def acc_device(t):
    """The sum of the (M, N) terms t in the order of tvb_acc_sum."""
    M, N = t.shape
    part = [0.0] * THREADS
    for d in range(2, M + N + 1):
        r0, r1 = max(1, d - N), min(M, d - 1)
        for k in range(r1 - r0 + 1):
            part[k % THREADS] = part[k % THREADS] + float(t[r0 + k - 1, d - r0 - k - 1])
    s = THREADS // 2
    while s > 0:
        for l in range(s):
            part[l] = part[l] + part[l + s]
        s //= 2
    return part[0]


def acc_raster(t):
    acc = 0.0
    for v in t.ravel():
        acc = acc + float(v)
    return acc


def _start(image):
    x = as_input(image)
    M, N = x.shape
    if M < 2 or N < 2:
        raise ValueError("frames of at least 2 x 2 pixels")
    u = np.zeros((M + 2, N + 2))
    u[1:M + 1, 1:N + 1] = x
    # (the ring as the library writes it, once: above and left the row / column of index 1, below and right the last)
    u[0, 1:N + 1] = x[1]
    u[M + 1, 1:N + 1] = x[M - 1]
    u[1:M + 1, 0] = x[:, 1]
    u[1:M + 1, N + 1] = x[:, N - 1]
    z = [np.zeros((M + 2, N + 2)) for _ in range(4)]
    return x, u, z[0], z[1], z[2], z[3]


def sweep_raster(x, u, dx, dy, bx, by, weight, isotropic):
    """One sweep in raster order, in place -> the (M, N) squared changes."""
    M, N = x.shape
    lam = 2.0 * weight
    norm = weight + 4.0 * lam
    inv = 1.0 / lam
    t = np.zeros((M, N))
    for r in range(1, M + 1):
        for c in range(1, N + 1):
            up = float(u[r, c])
            ur, ud = float(u[r, c + 1]), float(u[r + 1, c])
            ux = ur - up
            uy = ud - up
            unew = (lam * (ud + float(u[r - 1, c]) + ur + float(u[r, c - 1]) + float(dx[r, c - 1]) - float(dx[r, c]) + float(dy[r - 1, c])
                           - float(dy[r, c]) - float(bx[r, c - 1]) + float(bx[r, c]) - float(by[r - 1, c]) + float(by[r, c]))
                    + weight * float(x[r - 1, c - 1])) / norm
            u[r, c] = unew
            t[r - 1, c - 1] = (unew - up) * (unew - up)
            bxx, byy = float(bx[r, c]), float(by[r, c])
            if isotropic:
                tx = ux + bxx
                ty = uy + byy
                s = math.sqrt(tx * tx + ty * ty)
                dxx = s * lam * tx / (s * lam + 1.0)
                dyy = s * lam * ty / (s * lam + 1.0)
            else:
                s = ux + bxx
                dxx = s - inv if s > inv else (s + inv if s < -inv else 0.0)
                s = uy + byy
                dyy = s - inv if s > inv else (s + inv if s < -inv else 0.0)
            dx[r, c] = dxx
            dy[r, c] = dyy
            bx[r, c] = bxx + (ux - dxx)
            by[r, c] = byy + (uy - dyy)
    return t


def sweep_diagonal(x, u, dx, dy, bx, by, weight, isotropic):
    """One sweep diagonal by diagonal, a whole diagonal at a time, in place -> the (M, N) squared changes."""
    M, N = x.shape
    lam = 2.0 * weight
    norm = weight + 4.0 * lam
    inv = 1.0 / lam
    t = np.zeros((M, N))
    for d in range(2, M + N + 1):
        r = np.arange(max(1, d - N), min(M, d - 1) + 1)
        c = d - r
        up = u[r, c]
        ur, ud = u[r, c + 1], u[r + 1, c]
        ux = ur - up
        uy = ud - up
        unew = (lam * (ud + u[r - 1, c] + ur + u[r, c - 1] + dx[r, c - 1] - dx[r, c] + dy[r - 1, c] - dy[r, c] - bx[r, c - 1] + bx[r, c]
                       - by[r - 1, c] + by[r, c]) + weight * x[r - 1, c - 1]) / norm
        u[r, c] = unew
        t[r - 1, c - 1] = (unew - up) * (unew - up)
        bxx, byy = bx[r, c], by[r, c]
        if isotropic:
            tx = ux + bxx
            ty = uy + byy
            s = np.sqrt(tx * tx + ty * ty)
            dxx = s * lam * tx / (s * lam + 1.0)
            dyy = s * lam * ty / (s * lam + 1.0)
        else:
            s = ux + bxx
            dxx = np.where(s > inv, s - inv, np.where(s < -inv, s + inv, 0.0))
            s = uy + byy
            dyy = np.where(s > inv, s - inv, np.where(s < -inv, s + inv, 0.0))
        dx[r, c] = dxx
        dy[r, c] = dyy
        bx[r, c] = bxx + (ux - dxx)
        by[r, c] = byy + (uy - dyy)
    return t


def denoise_tv_bregman(image, weight, max_iter=100, eps=1e-3, isotropic=True, form="raster", order="raster", return_info=False):
    """-> the (M, N) float64 result; ``return_info``: also dict(n_iter, rmse_raster [per sweep], rmse_device [per sweep]).  The
    stopping rule reads the rmse of ``order``."""
    x, u, dx, dy, bx, by = _start(image)
    M, N = x.shape
    total = float(M * N)
    sweep = sweep_raster if form == "raster" else sweep_diagonal
    i, rr, rd = 0, [], []
    rmse = math.inf
    while i < max_iter and rmse > eps:
        t = sweep(x, u, dx, dy, bx, by, float(weight), bool(isotropic))
        rr.append(math.sqrt(acc_raster(t) / total))
        rd.append(math.sqrt(acc_device(t) / total))
        rmse = rr[-1] if order == "raster" else rd[-1]
        i += 1
    out = u[1:M + 1, 1:N + 1].copy()
    if return_info:
        return out, dict(n_iter=i, rmse_raster=np.array(rr), rmse_device=np.array(rd))
    return out


def margin_ok(rmses, eps, n):
    """Every rmse is farther from eps than 2 (n - 1) 2^-53 relative (of the sum; the square root halves a relative distance, so
    the bound on the sum bounds the rmse as well)."""
    return all(abs(v - eps) > acc_bound(n) * max(v, eps) for v in rmses)
