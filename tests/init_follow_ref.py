"""The rule of endpoint tracking, restated for the tests (csrc/gpet_init_plan.h has the rule the library runs).

For an init point (x, y) of an edge that reads the M x N image G, ``window = w >= 0`` rows and ``cols = a >= 0`` columns:

    candidates   r in [max(0, y - w), min(M - 1, y + w)]
    score        s(r) = sum over c = max(0, x - a) .. min(N - 1, x + a) of float64(G[r, c]), added in ascending c
    a candidate counts when s(r) > 0.0 (NaN fails the comparison); none counts: y stays
    else the new row is the candidate of largest s; ties: the smallest |r - y|, then the smallest r

x never changes, every init point is moved.  Python floats are IEEE doubles and the additions below run in ascending c one by one, so
the scores are the header's bit for bit.  Nothing here calls an init keyword of the package."""
import numpy as np

WINDOW_MAX, COLS_MAX = 4096, 64


def refusal(window, cols):
    """The reason (window, cols) is refused, in the order and the words of init_follow_check, or None."""
    if window < 0:
        return "init_follow: window must be at least 0 rows"
    if window > WINDOW_MAX:
        return "init_follow: window exceeds 4096 rows"
    if cols < 0:
        return "init_follow: cols must be at least 0 columns"
    if cols > COLS_MAX:
        return "init_follow: cols exceeds 64 columns"
    return None


def score(G, r, x, cols):
    N = G.shape[1]
    s = 0.0
    for c in range(max(0, x - cols), min(N - 1, x + cols) + 1):
        s += float(G[r, c])
    return s


def follow_row(G, x, y, window, cols):
    """The new row of the init point (x, y) on image ``G``."""
    G = np.asarray(G)
    x, y = int(x), int(y)
    best = None  # (s, |r - y|, r)
    for r in range(max(0, y - window), min(G.shape[0] - 1, y + window) + 1):
        s = score(G, r, x, cols)
        if not s > 0.0:
            continue
        d = abs(r - y)
        if best is None or s > best[0] or (s == best[0] and (d < best[1] or (d == best[1] and r < best[2]))):
            best = (s, d, r)
    return y if best is None else best[2]


def follow(G, init, window, cols):
    """``init`` ((n, 2) xy) with every row moved by the rule; int64."""
    out = np.array(np.asarray(init).reshape(-1, 2), dtype=np.int64, copy=True)
    for i in range(out.shape[0]):
        out[i, 1] = follow_row(G, out[i, 0], out[i, 1], window, cols)
    return out


def drifting_frames(M, N, T, seed):
    """The frames of the quality check: the edge row at column j is rint(5 sin(x_j)) + M // 2 - 12 + 3 t, x = linspace(-pi, pi, N); rows
    from that row down hold 0.3; plus RandomState(1000 seed + t).normal(0, sqrt(0.02)), clipped to [0, 1].  Returns (frames, rows)."""
    x = np.linspace(-np.pi, np.pi, N)
    frames, rows = [], []
    for t in range(T):
        edge = np.rint(5.0 * np.sin(x)).astype(int) + M // 2 - 12 + 3 * t
        img = np.zeros((M, N))
        img[np.arange(M)[:, None] >= edge[None, :]] = 0.3
        img = np.clip(img + np.random.RandomState(1000 * seed + t).normal(0.0, np.sqrt(0.02), img.shape), 0.0, 1.0)
        frames.append(img)
        rows.append(edge)
    return frames, rows


def layered_drift(M, N, T, seed0, base=18, gap=30, step=4):
    """T uint8 frames of M x N with two dark-to-bright edges one above the other that sink together: edge A's row at column j is
    rint(3 sin(x_j)) + base + step t, x = linspace(-pi, pi, N), edge B lies ``gap`` rows below.  Unlike band_ref.layered_frames the END
    POINTS move.  Returns (frames, rows_a per frame)."""
    x = np.linspace(-np.pi, np.pi, N)
    frames, rows_a = [], []
    for t in range(T):
        a = np.rint(3.0 * np.sin(x)).astype(int) + base + step * t
        rows = np.arange(M)[:, None]
        img = np.zeros((M, N))
        img[rows >= a[None, :]] = 0.4
        img[rows >= (a + gap)[None, :]] = 0.8
        img = np.clip(img + np.random.default_rng(seed0 + t).normal(0.0, 0.05, img.shape), 0.0, 1.0)
        frames.append(np.rint(img * 255.0).astype(np.uint8))
        rows_a.append(a)
    return frames, rows_a
