"""Batches for the tests that inject a stage's inputs (tests/test_gpu_sample_gemm_exact.py, tests/test_gpu_score_injected.py,
tests/test_gpu_kde_pix_injected.py, tests/test_gpu_posterior_injected.py, tests/test_gpu_factor_injected.py).

They come from the constructor's own parameter functions (gpet.resolve_params, gpet.to_abi_params) and _lib.Batch rather than
from GP_Edge_Tracing: the constructor, like the reference's, turns N_samples <= 100 into 1000, and these tests need the exact
count -- 63 sample rows for a row block that is not full, 40 for the wave-per-curve scorer.  Sample counts below 101 are
therefore reachable through the C ABI only, never through the Python constructor."""
import numpy as np

KERNEL = {'kernel': 'RBF', 'sigma_f': 2, 'length_scale': 10}


def _of_edge(v, e):
    return v[e] if isinstance(v, (list, tuple)) else v


def make_batch(amd, ctx, grad, spans, S, factor_cap=0, z_cols=0, sample_dtype=None, delta_x=5, fix_endpoints=True, pixel_thresh=2,
               score_thresh=1, keep_ratio=0.25, M=None, kernel=None, obs_cap=None, inits=None):
    """A batch of the edges spans = [(x_st, Lg)] on the one image grad with S samples per edge, of any S >= 1.

    delta_x, fix_endpoints, pixel_thresh, score_thresh: the constructor's, through its own clamping (delta_x <= 3 becomes 2).
    keep_ratio: n_keep = max(1, int(keep_ratio * S)) curves are kept.  M: the row count the init points are placed by (the second
    one on row M - 2), the image's own by default.
    kernel: the constructor's kernel_options dict (KERNEL by default).  obs_cap: the capacity of the observation set, so that
    n_cap = n_init + max(obs_cap, the edge's own bin count) -- by default the bin count alone, as the constructor has it.
    factor_cap: the capacity of the factor (0: 96 rows, or what the kernel's length scale asks for).
    delta_x, fix_endpoints, kernel, obs_cap and factor_cap may be lists with one entry per edge.
    inits: one [n_init, 2] array of (x, y) init points per edge, sorted by x, instead of the two on the span's ends; the span
    stays spans[e], so any count from one init point up is reachable (the constructor reads the span off the init points)."""
    from gaussian_process_edge_trace_amd.gpet import resolve_params, to_abi_params
    rows = grad.shape[0] if M is None else int(M)
    params, init_list = [], []
    for e, (x_st, Lg) in enumerate(spans):
        init = np.array([[x_st, 1], [x_st + Lg - 1, rows - 2]])
        p = resolve_params(init, grad.shape, KERNEL if kernel is None else _of_edge(kernel, e), noise_y=1, N_samples=max(S, 101),
                           score_thresh=score_thresh, delta_x=_of_edge(delta_x, e), keep_ratio=keep_ratio, pixel_thresh=pixel_thresh, seed=1,
                           fix_endpoints=_of_edge(fix_endpoints, e))
        q = to_abi_params(p, obs_cap=None if obs_cap is None else _of_edge(obs_cap, e), factor_cap=_of_edge(factor_cap, e), z_cols=z_cols)
        q.n_samples, q.n_keep = S, max(1, int(keep_ratio * S))
        if inits is not None:
            p["init"] = np.ascontiguousarray(inits[e], dtype=np.int64).reshape(-1, 2)
            q.n_init = p["init"].shape[0]
        params.append(q)
        init_list.append(p["init"])
    inits = init_list
    b = amd._lib.Batch(ctx, [grad], params, inits, share_image=len(spans) > 1)
    if sample_dtype is not None:
        b.set_sample_dtype(sample_dtype)
    return b
