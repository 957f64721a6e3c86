"""Injected inputs of the curve KDE and the pixel selection (csrc/gpet_k_kde_pix.inc: k_kde_prep, k_kde_fused, k_pix_columns,
k_pix_old, k_pix_argbest, k_pix_select) and an extended-precision reference of the density.  Plain NumPy, no GPU import: the
host tests (tests/test_kde_pix_cases_host.py) pin the reference against the f64 oracle and check that every case still reaches
the path it is named for; the GPU tests (tests/test_gpu_kde_pix_injected.py) run the kernels on the same data.

The constants of the kernels that the cases are built around (restated here, and in the host tests' properties):
a workgroup of k_kde_fused owns KDE_TX = 16 image columns and stages the points of the 24 columns x0 - 4 .. x0 + 19; it
processes its band of rows in chunks of KDE_H = 128 and stages KDE_NB = 128 curves per pass."""
import numpy as np

from oracle import gpet_oracle as orc

KDE_TX, KDE_H, KDE_NB = 16, 128, 128
LD = np.longdouble

_CACHE = {}


class Case(dict):
    """A dict with attribute access: M, N, x_st, Lg, S, n_keep, Y (S, Lg) f64, best_idx (n_keep,) int32, best_costs (n_keep,) f64,
    obs (k, 2) int64 xy, grad_kde (M, N) f32, delta_x, pixel_thresh, score_thresh, fix_endpoints, sample_dtype."""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


# ---- the pieces every case is made of ----------------------------------------------------------------------------------------------
def _pick_rows(rng, S, n_keep):
    """n_keep distinct sample rows, not in increasing order, some of them >= n_keep."""
    rows = rng.permutation(S)[:n_keep].astype(np.int32)
    if np.all(np.diff(rows) > 0) or rows.max() < n_keep:  # (cannot happen with S = 2 n_keep >= 60; kept as a guard)
        rows = rows[::-1].copy()
        rows[0] = S - 1
    return rows


def _finish(name, M, N, x_st, curves, rng, costs=None, sample_dtype=None, **params):
    """The case around the kept curves `curves` (n_keep, Lg): they go to the sample rows best_idx, every other row holds a decoy
    curve inside the image (a slip in the row indexing puts weight where none belongs)."""
    n_keep, Lg = curves.shape
    S = 2 * n_keep
    best_idx = _pick_rows(rng, S, n_keep)
    Y = rng.uniform(0.0, M - 1.0, size=(S, Lg))
    Y[best_idx] = curves
    if costs is None:
        costs = rng.uniform(0.5, 4.0, size=n_keep)
    grad_kde = (rng.integers(0, 1025, size=(M, N)) / 1024.0).astype(np.float32)
    # previous observations, fewer than algo_thresh (the reference's loop needs one pass): on the heaviest curve in the middle of
    # the edge, at x_st, in the corner of the image, on the last column of the edge, on the curve again
    w = int(np.argmin(costs))
    on_curve = lambda k: (x_st + k, int(np.clip(np.rint(curves[w, k]), 0, M - 1)))
    obs = [on_curve(Lg // 2), on_curve(0), (N - 1, M - 1), on_curve(Lg - 1), on_curve(Lg // 4)]
    delta_x = params.get("delta_x", 5)
    obs = obs[:max(1, min(5, Lg // delta_x - 1 - 2))]
    for x, y in obs[:2]:  # (the largest gradient KDE there, so that an old observation can hold its bin)
        grad_kde[y, x] = 1.0
    c = Case(name=name, M=M, N=N, x_st=x_st, Lg=Lg, S=S, n_keep=n_keep, Y=Y, best_idx=best_idx,
             best_costs=np.ascontiguousarray(costs, dtype=np.float64), obs=np.array(obs, dtype=np.int64).reshape(-1, 2),
             grad_kde=grad_kde, delta_x=delta_x, pixel_thresh=2, score_thresh=1.0, fix_endpoints=True, sample_dtype=sample_dtype)
    c.update(params)
    return c


def _tall_curves(rng, n_keep, Lg, lo, hi):
    """Curves spread over the rows lo .. hi (curve b around lo + (hi - lo) b / (n_keep - 1)), so that the points of ANY 24
    adjacent columns span that range: one tile's band is as tall as the spread."""
    base = lo + (hi - lo) * np.arange(n_keep) / (n_keep - 1.0)
    k = np.arange(Lg)
    return base[:, None] + 3.0 * np.sin(k[None, :] / 3.0 + np.arange(n_keep)[:, None]) + rng.uniform(-0.5, 0.5, size=(n_keep, Lg))


def _chunk_boundary_points(curves, M):
    """Points on and next to the boundaries of the 128-row chunks of a band that starts at row 0 (curve 0 is fixed at y = 0):
    a point at image row y is binned into padded-grid rows y + 1 and y + 2; chunk j holds the grid rows 128 j - 3 .. 128 j + 132."""
    pts = [123.0, 123.5, 127.0, 128.5, 131.5, 131.75, 132.0, 255.999, 251.25, 256.0, 259.5]
    for i, y in enumerate(pts):
        for j, col in enumerate((3, 17, 30)):  # (a column of each 16-column tile of a 37 .. 48 column image)
            if col < curves.shape[1]:
                curves[2 + (i + 5 * j) % (curves.shape[0] - 4), col] = y
    curves[0, :] = 0.0
    curves[-1, :] = M - 1.0


def tall_single():
    rng = np.random.default_rng(101)
    M, N, x_st, n_keep = 300, 40, 1, 30
    curves = np.clip(_tall_curves(rng, n_keep, N - 2, 20.0, 280.0), 0, M - 1)
    _chunk_boundary_points(curves, M)
    return _finish("tall_single", M, N, x_st, curves, rng)


def tall_restage():
    rng = np.random.default_rng(102)
    M, N, x_st, n_keep = 300, 37, 1, 150
    curves = np.clip(_tall_curves(rng, n_keep, N - 2, 20.0, 280.0), 0, M - 1)
    _chunk_boundary_points(curves, M)
    return _finish("tall_restage", M, N, x_st, curves, rng)


def restage_129():
    rng = np.random.default_rng(103)
    M, N, x_st, n_keep = 140, 48, 2, 129
    curves = np.clip(_tall_curves(rng, n_keep, N - 4, 6.0, 133.0), 0, M - 1)
    curves[0, :] = 0.0
    curves[-1, :] = M - 1.0
    curves[5, 7], curves[6, 20], curves[7, 33] = 123.5, 127.0, 128.5
    # the one curve of the second staging pass (position 128 of best_idx) carries a weight of its own size
    costs = rng.uniform(0.5, 4.0, size=n_keep)
    costs[128] = 0.05
    return _finish("restage_129", M, N, x_st, curves, rng, costs=costs)


def leaving():
    """Columns x < 19 inside the image, x >= 19 outside (alternately above and below): no point of the tile x0 = 32 (staged
    columns 28 .. 35) survives; columns 5 and 13 are outside for every curve."""
    rng = np.random.default_rng(104)
    M, N, x_st, n_keep = 64, 37, 1, 30
    Lg = N - 2
    x = x_st + np.arange(Lg)
    curves = rng.uniform(2.0, M - 3.0, size=(n_keep, Lg))
    out = np.where((np.arange(n_keep)[:, None] + x[None, :]) % 2 == 0, -rng.uniform(1e-9, 30.0, size=(n_keep, Lg)),
                   M - 1.0 + rng.uniform(1e-9, 30.0, size=(n_keep, Lg)))
    curves[:, x >= 19] = out[:, x >= 19]
    curves[:, x == 5] = -2.5
    curves[:, x == 13] = M + 1.25
    edge = [-0.0, 0.0, M - 1.0, np.nextafter(M - 1.0, np.inf), np.nextafter(M - 1.0, 0.0), np.nextafter(0.0, -1.0),
            np.nextafter(0.0, 1.0), 0.5, M - 1.5]
    for i, y in enumerate(edge):
        curves[i, 2] = y
        curves[n_keep - 1 - i, 16] = y
    # (delta_x = 2: the surviving half of the edge alone has bins enough for the selection to end)
    return _finish("leaving", M, N, x_st, curves, rng, delta_x=2)


def tiny_M():
    rng = np.random.default_rng(105)
    M, N, x_st, n_keep = 5, 37, 1, 30
    curves = rng.uniform(-1.0, M, size=(n_keep, N - 2))
    for i, y in enumerate([-0.0, 0.0, 4.0, np.nextafter(4.0, np.inf), 3.999, 0.001, 2.0]):
        curves[i, 4] = y
        curves[i + 8, 20] = y
    return _finish("tiny_M", M, N, x_st, curves, rng)


def _log_uniform_costs(rng, n):
    return 10.0 ** rng.uniform(-3.0, 3.0, size=n)


def small_W():
    """More than 90 % of the points outside and none of the twelve heaviest curves inside: W < 1."""
    rng = np.random.default_rng(106)
    M, N, x_st, n_keep = 64, 32, 1, 30
    Lg = N - 2
    costs = _log_uniform_costs(rng, n_keep)
    curves = np.where(rng.random((n_keep, Lg)) < 0.5, -rng.uniform(0.1, 9.0, size=(n_keep, Lg)),
                      M - 1.0 + rng.uniform(0.1, 9.0, size=(n_keep, Lg)))
    light = np.argsort(costs)[12:]
    inside = rng.random((n_keep, Lg)) < 0.12
    inside[np.argsort(costs)[:12]] = False
    inside[light[0], 3] = inside[light[1], 14] = inside[light[2], 27] = True  # (each tile keeps a survivor)
    curves[inside] = rng.uniform(0.0, M - 1.0, size=int(inside.sum()))
    return _finish("small_W", M, N, x_st, curves, rng, costs=costs)


def small_W_pow2():
    """Eight columns on which every curve survives, every other column outside: W = 8 up to the rounding of the weights."""
    rng = np.random.default_rng(107)
    M, N, x_st, n_keep = 64, 32, 1, 30
    Lg = N - 2
    costs = _log_uniform_costs(rng, n_keep)
    curves = np.where(rng.random((n_keep, Lg)) < 0.5, -rng.uniform(0.1, 9.0, size=(n_keep, Lg)),
                      M - 1.0 + rng.uniform(0.1, 9.0, size=(n_keep, Lg)))
    for k in (0, 3, 4, 11, 14, 15, 22, 29):
        curves[:, k] = rng.uniform(0.0, M - 1.0, size=n_keep)
    return _finish("small_W_pow2", M, N, x_st, curves, rng, costs=costs)


SPANS = [(19, 43), (20, 44), (21, 59), (4, 27)]  # (x_st, x_en) of span_edges


def span_edges():
    """Four edges on one 64 x 64 image (a list of four cases with one grad_kde: edges on one image share its gradient KDE)."""
    out = []
    for i, (x_st, x_en) in enumerate(SPANS):
        rng = np.random.default_rng(108 + i)
        M, N, n_keep = 64, 64, 30
        Lg = x_en - x_st + 1
        curves = np.clip(_tall_curves(rng, n_keep, Lg, 12.0 + 3 * i, 50.0 - 2 * i), 0, M - 1)
        curves[3, :] = rng.uniform(-4.0, 3.0, size=Lg)  # (one curve that leaves and re-enters at the top)
        out.append(_finish("span_edges[%d,%d]" % (x_st, x_en), M, N, x_st, curves, rng))
    shared = out[0].grad_kde.copy()  # (edges on one image share its gradient KDE)
    for c in out:
        shared[c.obs[:2, 1], c.obs[:2, 0]] = 1.0
    for c in out:
        c["grad_kde"] = shared
    return out


def f32_samples():
    """tall_single's curves seen through a 64-row image whose row 0 is tall_single's row 118 (the chunk-boundary points land on
    rows 5 .. 14), as float32 samples."""
    rng = np.random.default_rng(112)
    t = tall_single()
    M, N = 64, 40
    curves = t.Y[t.best_idx] - 118.0 + rng.uniform(0.0, 1e-4, size=(t.n_keep, t.Lg))  # (off the f32 grid: rounding matters)
    return _finish("f32_samples", M, N, t.x_st, curves, rng, sample_dtype="f32")


BUILDERS = dict(tall_single=tall_single, tall_restage=tall_restage, restage_129=restage_129, leaving=leaving, tiny_M=tiny_M,
                small_W=small_W, small_W_pow2=small_W_pow2, f32_samples=f32_samples)
NAMES = list(BUILDERS)


def case(name):
    if name not in _CACHE:
        _CACHE[name] = BUILDERS[name]() if name in BUILDERS else span_edges()
    return _CACHE[name]


# ---- what the kernels see, and the reference ------------------------------------------------------------------------------------------
def kept_curves(c):
    """(n_keep, Lg) f64: the kept curves as the device reads them (rounded to float32 for float32 samples)."""
    y = c.Y[c.best_idx]
    return y.astype(np.float32).astype(np.float64) if c.sample_dtype == "f32" else y


def survives(c):
    y = kept_curves(c)
    return ~((y < 0) | (y > c.M - 1))


def tile_bands(c):
    """[(y_lo, y_hi)] per 16-column tile: the rows of the surviving points of the tile's 24 staged columns (a point at y touches
    rows floor(y) and floor(y) + 1), +-4, clipped to the image; (M, -1) for a tile without any."""
    y, ok = kept_curves(c), survives(c)
    x = c.x_st + np.arange(c.Lg)
    out = []
    for x0 in range(0, c.N, KDE_TX):
        cols = (x >= x0 - 4) & (x <= x0 + KDE_TX + 3)
        ys = y[:, cols][ok[:, cols]]
        if ys.size == 0:
            out.append((c.M, -1))
        else:
            out.append((max(0, int(np.floor(ys.min())) - 4), min(c.M - 1, int(np.floor(ys.max())) + 1 + 4)))
    return out


def total_weight(c):
    """W: the sum over the surviving points of their curve's weight (1 / cost, normalised over the kept curves)."""
    inv = 1.0 / c.best_costs
    return float(np.sum((inv / inv.sum())[:, None] * survives(c)))


def reference(c):
    """(raw f32 (M, N), normalised f32 (M, N), removed count): linear binning on the padded grid x = -1 .. N, y = -1 .. M, the 9 x 9
    Gaussian of oracle.kde_stencil, crop -- all in np.longdouble from the f64 inputs -- then the cast to f32 and, in f32,
    (v - min) / (max - min)."""
    key = ("ref", c.name)
    if key in _CACHE:
        return _CACHE[key]
    M, N = c.M, c.N
    y, ok = kept_curves(c), survives(c)
    inv = LD(1.0) / c.best_costs.astype(LD)
    w = np.broadcast_to((inv / inv.sum())[:, None], y.shape)[ok]
    w = w / w.sum()
    gx = np.broadcast_to((c.x_st + np.arange(c.Lg) + 1)[None, :], y.shape)[ok]
    gy = y[ok].astype(LD) + LD(1.0)
    iy = np.floor(gy).astype(np.int64)
    fy = gy - iy
    grid = np.zeros((N + 2 + 8, M + 2 + 8), dtype=LD)  # [x][y], four cells of zeros all round
    np.add.at(grid, (gx + 4, iy + 4), (LD(1.0) - fy) * w)
    np.add.at(grid, (gx + 4, iy + 5), fy * w)
    kern, half = orc.kde_stencil(1.0)
    assert half == 4 and kern.shape == (9, 9)
    dens = np.zeros((N + 2, M + 2), dtype=LD)
    for i in range(9):
        for j in range(9):  # (a symmetric stencil: correlation and convolution agree)
            dens += grid[i:i + N + 2, j:j + M + 2] * LD(kern[i, j])
    raw = np.ascontiguousarray(dens.T[1:-1, 1:-1]).astype(np.float32)
    mn, mx = raw.min(), raw.max()
    norm = (raw - mn) / (mx - mn)
    assert norm.dtype == np.float32
    _CACHE[key] = (raw, norm, int((~ok).sum()))
    return _CACHE[key]


def oracle_kde(c):
    """The f64 oracle's normalised density (direct convolution), as f64 values that are exactly f32."""
    y = kept_curves(c)
    x = np.broadcast_to((c.x_st + np.arange(c.Lg)).astype(np.float64)[:, None], y.T.shape)
    return orc.kde_of_curves(np.stack([x, y.T], axis=-1), c.best_costs, c.M, c.N, method="direct")


def pixel_state(c):
    return dict(score_thresh=float(c.score_thresh), pixel_thresh=int(c.pixel_thresh), algo_thresh=c.Lg // c.delta_x - (c.pixel_thresh - 1),
                x_st=c.x_st, delta_x=c.delta_x)


def expected_selection(c, kde_f32):
    """(observations xy, score_thresh, done) of the reference's get_best_pixels on the density kde_f32 (widened to f64)."""
    st = pixel_state(c)
    fobs, _ = orc.get_best_pixels(None, None, c.obs[:, [1, 0]], c.grad_kde.astype(np.float64), c.M, c.N, st, c.fix_endpoints, c.x_st,
                                  c.x_st + c.Lg - 1, kde_arr=np.asarray(kde_f32).astype(np.float64))
    return fobs, st["score_thresh"], int(fobs.shape[0] >= st["algo_thresh"])


# ---- pixel rules on injected densities --------------------------------------------------------------------------------------------------
RULE_SHAPES = {"140x150-dx2": (140, 150, 1, 148, 2), "64x40-dx5": (64, 40, 2, 36, 5)}  # M, N, x_st, Lg, delta_x
RULES = ["column_ties", "bin_ties", "old_ties_new", "old_on_low_kde", "old_at_x_st-fixed", "old_at_x_st-free", "kde_threshold",
         "five_decays", "algo_thresh_ends"]
F32_THRESH = np.float32(1e-3)  # widened to f64 it is 0.001000000047..., above the rule's 1e-3; its predecessor is below


def _eighths(rng, shape, density):
    """A sparse f32 field of multiples of 1/8 in (0, 1]: only 8 values, so equal scores are the rule, not the exception."""
    v = rng.integers(1, 9, size=shape) / 8.0
    return np.where(rng.random(shape) < density, v, 0.0).astype(np.float32)


def rule_case(rule, shape_name):
    """The injected density, gradient KDE, previous observations and parameters of one pixel rule; `marks` holds what the host test
    asserts about the case (and the GPU test about the result)."""
    key = ("rule", rule, shape_name)
    if key in _CACHE:
        return _CACHE[key]
    M, N, x_st, Lg, dx = RULE_SHAPES[shape_name]
    rng = np.random.default_rng(1000 + 10 * RULES.index(rule) + (M > 100))
    x_en = x_st + Lg - 1
    kde = _eighths(rng, (M, N), 0.15)
    grad = (rng.integers(0, 9, size=(M, N)) / 8.0).astype(np.float32)
    c = Case(name="%s-%s" % (rule, shape_name), M=M, N=N, x_st=x_st, Lg=Lg, delta_x=dx, pixel_thresh=2, score_thresh=1.0,
             fix_endpoints=True, obs=np.zeros((0, 2), dtype=np.int64), marks={})
    cb = x_st + 6 * dx  # a column in the middle of bin 6: cb - x_st is a multiple of delta_x
    near = [x for x in range(cb - 2, cb + 3) if x != cb]  # the other columns of bin 6, and their neighbours
    if rule == "column_ties":
        rows = [r for r in (9, 9 + 8, 9 + 64) if r < M]  # (same row lane of k_pix_columns; the third one a 64-row stride on)
        kde[:, near], kde[:, cb], grad[:, cb] = 0.0, 0.0, 0.0
        kde[rows, cb], grad[rows, cb] = 1.0, 1.0
        kde[12, cb], grad[12, cb] = 1.0, 1.0  # (and another lane, between the first two)
        c.marks = dict(winner=(cb, 9), tied=[(cb, r) for r in rows + [12]])
    elif rule == "bin_ties":
        c1, c2 = cb, cb + 1  # (delta_x = 2: (c2 - x_st) / 2 = 6.5 rounds to the even 6; delta_x = 5: 6.2 -> 6)
        kde[:, near], kde[:, cb], grad[:, [c1, c2]] = 0.0, 0.0, 0.0
        kde[30, c1], grad[30, c1] = 1.0, 1.0
        kde[21, c2], grad[21, c2] = 1.0, 1.0  # the later column on the earlier row: first in row-major order
        c.marks = dict(winner=(c2, 21), tied=[(c2, 21), (c1, 30)])
    elif rule == "old_ties_new":
        kde[:, cb], grad[:, cb] = 0.0, 0.0
        kde[[20, 40], cb], grad[[20, 40], cb] = 1.0, 1.0
        c.obs = np.array([[x_st + 2 * dx, 5], [cb, 40]], dtype=np.int64)  # the old observation below the equal new pixel
        c.marks = dict(winner=(cb, 40), tied=[(cb, 40), (cb, 20)])
    elif rule == "old_on_low_kde":
        kde[:, cb] = 0.0
        grad[33, cb] = 1.0
        kde[34, cb - dx], grad[34, cb - dx] = F32_THRESH, 1.0
        c.obs = np.array([[cb, 33], [cb - dx, 34]], dtype=np.int64)  # density 0: dropped; density float32(1e-3): competes
        c.marks = dict(absent=(cb, 33))
    elif rule.startswith("old_at_x_st"):
        c.fix_endpoints = rule.endswith("fixed")
        kde[:, x_st], grad[:, x_st] = 0.0, 0.0
        kde[[17, 44], x_st], grad[[17, 44], x_st] = 1.0, 1.0
        kde[50, x_en], grad[50, x_en] = 1.0, 1.0
        c.obs = np.array([[x_st, 44]], dtype=np.int64)
        # the old observation wins its bin either way: ahead of the equal new pixel (x_st, 17) when the endpoints are free,
        # without it when they are fixed
        c.marks = dict(winner=(x_st, 44), tied=[(x_st, 44), (x_st, 17)])
    elif rule == "kde_threshold":
        kde[:], grad[:] = 0.0, 1.0
        below = np.nextafter(F32_THRESH, np.float32(0))
        cols = [x_st + i * dx for i in (1, 2, 3, 4, 5)]
        kde[10, cols[0]] = kde[11, cols[1]] = kde[12, cols[2]] = 0.125
        kde[13, cols[3]] = F32_THRESH            # passes `> 1e-3` once widened
        kde[14, cols[4]] = below                 # does not: with it a fifth bin would be found
        kde[9, cols[3]] = below                  # (nor does this one, above the passing pixel in its column)
        c.pixel_thresh = 4
        c.marks = dict(present=(cols[3], 13), absent=(cols[4], 14), count=4)
    elif rule == "five_decays":
        kde, grad = kde * np.float32(0.5), grad * np.float32(0.5)  # the best score is (0.25 + 0.5 + 0.5) / 3 < 0.95 ** 5
        c.marks = dict(min_decays=5)
    elif rule == "algo_thresh_ends":
        # algo_thresh - 1 bins hold a pixel of score 1, the next two bins one of a lower score each, and there are algo_thresh - 1
        # previous observations (all on density 0): the first threshold finds as many bins as there were observations, the
        # decays then add ONE, which is too few for pixel_thresh = 2 and enough for algo_thresh
        algo = Lg // dx - 1
        kde[:], grad[:] = 0.0, 0.0
        xs = np.arange(x_st + 1, x_en)
        bins = np.round((xs - x_st) / dx).astype(int)
        for i, bn in enumerate(np.unique(bins)[:algo + 1]):
            x, y = int(xs[bins == bn][0]), (5 + 3 * i) % M
            kde[y, x], grad[y, x] = 1.0, (1.0 if i < algo - 1 else (0.5 if i == algo - 1 else 0.25))
        c.obs = np.array([[x_st + 1 + i, M - 1] for i in range(algo - 1)], dtype=np.int64)
        c.marks = dict(count=algo, ends_by_algo=True)
    else:
        raise KeyError(rule)
    c.kde, c.grad_kde = np.ascontiguousarray(kde, dtype=np.float32), np.ascontiguousarray(grad, dtype=np.float32)
    _CACHE[key] = c
    return c
