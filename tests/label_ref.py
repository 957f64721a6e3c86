"""The two rules of csrc/gpet_label_plan.h (include/gpet_hip.h, "label maps") restated with numpy: what the label-map tests compare the
device and the header against, np.array_equal.  tests/test_label_ref.py checks this restatement itself -- against the reference's own mask,
the package's Dice score, exact rational arithmetic and the convex-polygon test."""
import numpy as np

NO_ROW = -(1 << 63)


def map_table(map_of, n):
    """(int array of n map indices, n_maps); None: all on map 0."""
    if map_of is None:
        return np.zeros(n, dtype=np.int64), 1
    m = np.asarray(map_of, dtype=np.int64).reshape(-1)
    assert m.shape[0] == n
    return m, int(m.max()) + 1 if m.size and m.max() >= 0 else 1


def thresholds(M, N, x_st, rows, extend=False):
    """T [n_edges, N] int64: edge e's threshold at every frame column (steps 1 - 5 of Rule 1)."""
    T = np.full((len(rows), N), M, dtype=np.int64)
    c = np.arange(N)
    for e, (x0, t) in enumerate(zip(x_st, rows)):
        t = np.asarray(t, dtype=np.int64).reshape(-1)
        k = c - int(x0)
        inside = (k >= 0) & (k < t.shape[0])
        if extend:
            k = np.clip(k, 0, t.shape[0] - 1)
            inside = np.ones(N, dtype=bool)
        tk = t[np.where(inside, k, 0)]
        counts = inside & (tk != NO_ROW)
        T[e] = np.where(counts, np.minimum(np.maximum(tk, 0), M), M)
    return T


def row_maps(shape, x_st, rows, map_of=None, extend=False, transposed=False):
    """label [n_maps, M, N] uint8 -- [n_maps, N, M] with ``transposed`` -- by Rule 1."""
    M, N = int(shape[0]), int(shape[1])
    m, n_maps = map_table(map_of, len(rows))
    T = thresholds(M, N, x_st, rows, extend)
    r = np.arange(M)[:, None]
    out = np.zeros((n_maps, M, N), dtype=np.uint8)
    for e in range(len(rows)):
        if m[e] >= 0:
            out[m[e]] += (r >= T[e][None, :]).astype(np.uint8)
    return np.ascontiguousarray(out.transpose(0, 2, 1)) if transposed else out


def most_edges(map_of, n):
    m, n_maps = map_table(map_of, n)
    return int(max(np.count_nonzero(m == f) for f in range(n_maps)))


def thick_of(label, L):
    """thick [n_maps, L + 1, N] int32 by counting the (untransposed) maps: rows of label l per column."""
    return np.stack([(label == l).sum(axis=1) for l in range(L + 1)], axis=1).astype(np.int32)


def crossing(px, py, xi, yi, xj, yj):
    """Does the segment (xi, yi) -> (xj, yj) toggle the pixels (px, py) (arrays)?  float64: every difference and product rounded once."""
    px, py = np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    xi, yi, xj, yj = np.float64(xi), np.float64(yi), np.float64(xj), np.float64(yj)
    straddle = (yi > py) != (yj > py)
    a = (px - xi) * (yj - yi)
    b = (xj - xi) * (py - yi)
    return straddle & ((a < b) if yj > yi else (a > b))


def inside(shape, xy):
    """bool [Ms, Ns]: the pixels inside the closed outline xy [n, 2] of (x, y) by Rule 2; all False for an outline with a vertex that is
    not finite."""
    Ms, Ns = int(shape[0]), int(shape[1])
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    out = np.zeros((Ms, Ns), dtype=bool)
    if not np.all(np.isfinite(xy)):
        return out
    py, px = np.meshgrid(np.arange(Ms, dtype=np.float64), np.arange(Ns, dtype=np.float64), indexing="ij")
    n = xy.shape[0]
    for j in range(n):
        (xi, yi), (xj, yj) = xy[j], xy[(j + 1) % n]
        out ^= crossing(px, py, xi, yi, xj, yj)
    return out


def outline_maps(shape, outlines, map_of=None):
    """label_xy [n_maps, Ms, Ns] uint8 by Rule 2."""
    m, n_maps = map_table(map_of, len(outlines))
    out = np.zeros((n_maps, int(shape[0]), int(shape[1])), dtype=np.uint8)
    for e, xy in enumerate(outlines):
        if m[e] >= 0:
            out[m[e]] += inside(shape, xy).astype(np.uint8)
    return out


def trace_maps(traces, shape, map_of=None, extend=False, transpose=False):
    """``gpet_utils.label_maps`` restated: (Lg, 2) yx traces over consecutive columns (``transpose``: (row, column) over consecutive rows
    of the frame, the maps in the frame's orientation)."""
    a, b = (1, 0) if transpose else (0, 1)
    M, N = (shape[1], shape[0]) if transpose else shape
    return row_maps((M, N), [int(t[0, b]) for t in traces], [np.asarray(t)[:, a] for t in traces], map_of, extend, transposed=transpose)
