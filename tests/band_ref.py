"""The definition of tracking bands, restated for the tests (csrc/gpet_band_plan.h has the rule the library runs).

A band is (r0, H): rows r0 .. r0 + H - 1 of an M x N frame.  Tracing edge e in its band is DEFINED as tracing the cropped full-frame
gradient image with the objects the package has without bands:

    GP_Edge_Tracing_Batch([init - (0, r0)], [G[r0:r0 + H]], [seed], **ctor_kwargs)

with every row-valued output raised by r0 again.  ``place`` is the placement rule, ``crop_batch`` the oracle route, ``chained`` the
host-chained sequence loop.  Nothing here calls a band keyword of the package."""
import numpy as np

from gaussian_process_edge_trace_amd.gpet import resolve_params
from gaussian_process_edge_trace_amd.sequence import chain_slices, warm_start_obs


def place(M, H, trace_rows, init_rows, r0_old=None):
    """r0 of the band of an edge with init rows ``init_rows`` from the source's trace in full-frame rows ``trace_rows`` (floats or ints;
    NaN and rows outside [0, M - 1] are ignored; none left: ``r0_old``).  Python integers, floor division."""
    t = np.asarray(trace_rows, dtype=np.float64).reshape(-1)
    t = t[np.isfinite(t)]
    t = t[(t >= 0) & (t <= M - 1)]
    if t.size == 0:
        return r0_old
    lo, hi = int(t.min()), int(t.max())
    i_lo, i_hi = int(np.min(init_rows)), int(np.max(init_rows))
    r0 = (lo + hi) // 2 - H // 2
    r0 = min(max(r0, 0), M - H)
    r0 = max(min(r0, i_lo), i_hi - H + 1)
    return r0


def refusal(M, H, r0, i_lo, i_hi):
    """The reason a band is refused, in the order and the words of band_check, or None; ``r0=None``: still to be placed."""
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


def layered_frames(M, N, T, seed0, dtype="uint8", base=14, gap=12, step=5, amp=2.0):
    """T frames of M x N with two dark-to-bright edges one above the other (two layers of a retina): edge A runs from row ``base`` at
    both ends through a bulge that grows by ``step`` rows per frame in the middle, edge B lies ``gap`` rows below it.  The end points
    do not move (the init points of a sequence are fixed), the middle drifts by ``step * (T - 1)`` rows.  Returns (frames, init_a,
    init_b, rows_a): raw frames of ``dtype``, the two inits (xy), and edge A's rows per frame."""
    x = np.arange(N)
    bump = np.sin(np.pi * x / (N - 1))
    frames, rows_a = [], []
    for t in range(T):
        a = np.rint(base + step * t * bump + amp * np.sin(4 * np.pi * x / (N - 1))).astype(int)
        b = a + gap
        rows = np.arange(M)[:, None]
        img = np.zeros((M, N))
        img[rows >= a[None, :]] = 0.4
        img[rows >= b[None, :]] = 0.8
        rng = np.random.default_rng(seed0 + t)
        img = np.clip(img + rng.normal(0.0, 0.05, img.shape), 0.0, 1.0)
        rows_a.append(a)
        if dtype == "uint8":
            frames.append(np.rint(img * 255.0).astype(np.uint8))
        else:
            frames.append(img.astype(dtype))
    a0 = rows_a[0]
    init_a = np.array([[0, a0[0]], [N - 1, a0[-1]]], dtype=np.int64)
    init_b = np.array([[0, a0[0] + gap], [N - 1, a0[-1] + gap]], dtype=np.int64)
    return frames, init_a, init_b, rows_a


def crop_batch(amd, ctx, inits, Gs, r0s, H, seeds, obs=None, **ctor):
    """The oracle route: one batch without bands on the crops ``Gs[e][r0:r0 + H]`` (``Gs``: every edge's full-frame f32 gradient image)
    with the inits -- and ``obs``, full-frame xy -- lowered by r0."""
    down = [np.array([0, int(r0)], dtype=np.int64) for r0 in r0s]
    crops = [np.ascontiguousarray(np.asarray(G, dtype=np.float32)[int(r0):int(r0) + H]) for G, r0 in zip(Gs, r0s)]
    if obs is not None:
        obs = [np.asarray(o, dtype=np.int64).reshape(-1, 2) - d for o, d in zip(obs, down)]
    return amd.GP_Edge_Tracing_Batch([np.asarray(i) - d for i, d in zip(inits, down)], crops, seeds, obs=obs, _ctx=ctx, **ctor)


def up(result, r0, return_std):
    """A result of ``finish`` raised from band rows to full-frame rows: one int64 / f64 addition of r0."""
    if return_std:
        et, (lo, hi) = result
        return et + np.array([int(r0), 0]), (lo + int(r0), hi + int(r0))
    return result + np.array([int(r0), 0])


def chained(amd, ctx, Gs_of_frame, inits, H, M, n_chains, warm_every, seeds_of_frame, ensemble_seeds=None, warm_from="medoid", tol=2,
            return_std=False, **ctor):
    """The host-chained sequence loop on crops: ``Gs_of_frame[f][k]`` the full-frame gradient image of init k on frame f.  Every (frame,
    init) is a fresh batch without bands -- of one edge, or of the K ensemble members on one shared crop -- at the band placed from the
    previous frame's source trace (the first frame of a chain: from the init rows), warm-started from that trace lowered into the
    band.  Returns (results, iterations, r0) per frame, each a list over the inits; with ``ensemble_seeds`` a result is the dict of
    ``ensemble`` in full-frame rows plus ``result`` (the medoid's own) and r0 is the group's."""
    T = len(Gs_of_frame)
    results, iterations, r0_out = [None] * T, [None] * T, [None] * T
    for lo_f, hi_f in chain_slices(T, n_chains):
        prev = [None] * len(inits)
        r0_prev = [None] * len(inits)
        for f in range(lo_f, hi_f):
            res_f, it_f, r0_f = [], [], []
            for k, init in enumerate(inits):
                rows = np.asarray(init)[:, 1]
                if prev[k] is None and r0_prev[k] is not None:  # (a group without members hands nothing on: the band stays)
                    r0 = r0_prev[k]
                else:
                    r0 = place(M, H, rows if prev[k] is None else prev[k][:, 0], rows, r0_prev[k])
                sd = list(ensemble_seeds) if ensemble_seeds is not None else [seeds_of_frame[f]]
                K = len(sd)
                G = np.asarray(Gs_of_frame[f][k], dtype=np.float32)
                probe = resolve_params(np.asarray(init) - np.array([0, r0]), (H, G.shape[1]), **ctor)
                if prev[k] is None:
                    o = np.zeros((0, 2), dtype=np.int64)
                else:
                    o = warm_start_obs(prev[k] - np.array([r0, 0]), probe["x_st"], probe["x_en"], warm_every, probe["algo_thresh"], M=H)
                b = amd.GP_Edge_Tracing_Batch([np.asarray(init) - np.array([0, r0])] * K, np.ascontiguousarray(G[r0:r0 + H]), sd,
                                              obs=[o] * K, return_std=return_std, _ctx=ctx, **ctor)
                out = [up(r, r0, return_std) for r in b()]
                if ensemble_seeds is None:
                    res_f.append(out[0])
                    it_f.append(b.timings["iters"][0])
                    prev[k] = out[0][0] if return_std else out[0]
                else:
                    d = dict(b.ensemble(None, tol)[0])
                    d["trace"] = d["trace"] + np.array([r0, 0])
                    for key in ("median", "q_lo", "q_hi", "min", "max"):
                        d[key] = d[key] + r0
                    d["result"] = out[d["medoid"]] if d["medoid"] >= 0 else None
                    res_f.append(d)
                    it_f.append(list(b.timings["iters"]))
                    if d["medoid"] < 0:
                        prev[k] = None
                    elif warm_from == "consensus":
                        prev[k] = d["trace"]
                    else:
                        src = out[d[warm_from]]
                        prev[k] = src[0] if return_std else src
                b._batch.close()
                r0_prev[k] = r0
                r0_f.append(r0)
            results[f], iterations[f], r0_out[f] = res_f, it_f, r0_f
    return results, iterations, r0_out
