"""Drop-in ``GP_Edge_Tracing`` whose arithmetic runs in libgpet_hip.so on an MI355X.

Mirrors the constructor / ``__call__`` surface of the reference
(``gp_edge_tracing/gpet.py:22-35, 768-773``): same argument names, order, defaults, silent
clamping (gpet.py:95-119) and return conventions (gpet.py:902-908).  The per-iteration
stages keep the reference's method names -- ``fit_predict_GP`` (gpet.py:182),
``get_best_curves`` (:414), ``cost_funct`` (:371), ``get_best_pixels`` (:622) -- and are thin
calls into the C ABI (include/gpet_hip.h).  There is no CPU fallback: without the HIP
library / a GPU the constructor raises.
"""
from __future__ import annotations

import time as t

import numpy as np

from . import _lib
from . import gpet_utils


def resolve_params(init, grad_shape, kernel_options=(1, 3, 3), noise_y=1, obs=np.array([], dtype=np.int8),
                   N_samples=500, score_thresh=1, delta_x=20, keep_ratio=0.1, pixel_thresh=5, seed=42,
                   return_std=False, fix_endpoints=True):
    """Host-side parameter clamping and derived sizes of the reference constructor
    (gpet.py:95-151), including its quirks: x_st/x_en come from the UNSORTED ``init``
    (gpet.py:96), ``N_keep`` uses the raw ``keep_ratio*N_samples`` (gpet.py:118), the 3-tuple
    presets index with ``[opt-1]`` (gpet.py:146,150), the dict needs key 'kernel' (gpet.py:133)."""
    init = np.asarray(init)
    p = dict(noise_y=noise_y, seed=seed, return_std=return_std, fix_endpoints=fix_endpoints)
    p["init"] = init[np.argsort(init[:, 0])].astype(int)
    p["x_st"], p["x_en"] = int(init[0, 0]), int(init[-1, 0])
    p["N_samples"] = int(N_samples) if N_samples > 100 else 1000
    p["obs"] = np.asarray(obs).reshape(-1, 2).astype(np.int64)
    p["keep_ratio"] = float(keep_ratio) if 0 < keep_ratio <= 1 else 0.1
    p["pixel_thresh"] = int(pixel_thresh) if pixel_thresh >= 2 else 2
    p["score_thresh"] = float(score_thresh) if 0 < score_thresh <= 1 else 1
    p["delta_x"] = int(delta_x) if delta_x > 3 else 2
    p["half_delta"] = p["delta_x"] // 2
    p["N_inits"] = p["init"].shape[0]
    p["M"], p["N"] = grad_shape
    p["x_grid"] = p["x_st"] + np.arange(p["x_en"] - p["x_st"] + 1).astype(int)
    p["edge_length"] = p["x_grid"].shape[0]
    p["N_subints"] = int(p["edge_length"] // p["delta_x"])
    p["N_keep"] = int(keep_ratio * N_samples)
    p["algo_thresh"] = p["N_subints"] - (p["pixel_thresh"] - 1)
    if type(kernel_options) == dict:
        p["sigma_f"] = kernel_options["sigma_f"]
        p["sigma_l"] = kernel_options["length_scale"]
        p["kernel_type"] = kernel_options["kernel"]
        p["kernel_nu"] = kernel_options["nu"] if kernel_options["kernel"] == "Matern" else 2.5
    else:
        rbf_matern, sigmaf_opt, sigmal_opt = kernel_options
        p["kernel_type"] = ["RBF", "Matern"][int(rbf_matern > 0)]
        p["kernel_nu"] = [2.5, 1.5][int(rbf_matern > 1)]
        sf = [10, 8, 6, 4, 2, 1][sigmaf_opt - 1] if (sigmaf_opt >= 0) and (sigmaf_opt <= 5) else 1
        p["sigma_f"] = p["M"] // sf
        sl = [1, 4 / 3, 2, 4, 10][sigmal_opt - 1] if (sigmal_opt >= 0) and (sigmal_opt <= 4) else 10
        p["sigma_l"] = p["edge_length"] // sl
    return p


def auto_factor_cap(p):
    """Rows kept by the eigen-factor sampler.  The RBF correlation matrix on a unit grid has
    eigenvalues ~ exp(-(pi k l / N)^2 / 2): they fall below 1e-14 of the largest at
    k ~ 2.6 N / l, and the posterior covariance cannot have higher rank.  <= 96 rows take the
    LDS-resident Jacobi path; Matern spectra decay polynomially, so keep every row."""
    Lg = p["edge_length"]
    if p["kernel_type"] != "RBF":
        return Lg
    est = int(2.6 * Lg / float(p["sigma_l"])) + 12
    return 0 if est <= 96 else min(Lg, int(est * 1.2))


def to_abi_params(p, obs_cap=None, factor_cap=0, z_cols=0):
    """gpet_params (include/gpet_hip.h) from the resolved constructor state."""
    if not factor_cap:
        factor_cap = auto_factor_cap(p)
    q = _lib.GpetParams()
    q.kernel_type = _lib.KERNEL_MATERN if p["kernel_type"] == "Matern" else _lib.KERNEL_RBF
    q.nu = float(p["kernel_nu"])
    if q.kernel_type == _lib.KERNEL_MATERN and np.isinf(q.nu):  # sklearn's Matern(nu=inf) IS the RBF kernel
        q.kernel_type, q.nu = _lib.KERNEL_RBF, 2.5
    q.sigma_f = float(p["sigma_f"])
    q.length_scale = float(p["sigma_l"])
    q.noise_y = float(p["noise_y"])
    q.n_samples = int(p["N_samples"])
    q.n_keep = int(p["N_keep"])
    q.delta_x = int(p["delta_x"])
    q.pixel_thresh = int(p["pixel_thresh"])
    q.score_thresh = float(p["score_thresh"])
    q.fix_endpoints = 1 if p["fix_endpoints"] else 0
    q.x_st, q.x_en = int(p["x_st"]), int(p["x_en"])
    q.n_init = int(p["N_inits"])
    n_bins = (p["edge_length"] - 1) // p["delta_x"] + 3
    q.obs_cap = int(obs_cap if obs_cap is not None else max(n_bins, p["obs"].shape[0] + 1))
    q.factor_cap = int(factor_cap)
    q.z_cols = int(z_cols)
    q.jitter = 1e-6  # gpet.py:155
    return q


class GP_Edge_Tracing(object):
    """Traces one edge with Gaussian-process regression on the GPU (gpet.py:17-35).

    The seam methods of the reference class are device calls on ONE resident state (observation set, samples, scores,
    KDE, score threshold).  Unlike the reference's pure functions, ``fit_predict_GP(obs)``, ``compute_new_obs(...,
    pre_fobs)`` and ``get_best_pixels(..., pre_fobs=...)`` leave the observation set they were given on the device, and
    ``get_best_curves(y_samples)`` the samples: a later argument-less call continues from there.  ``__call__`` starts
    from ``self.obs`` again (it resets the device state first), so a trace is not affected by earlier seam calls.

    Keywords beyond the reference's signature (keyword-only): ``device``, ``stream``, ``factor_cap``, ``z_cols``,
    ``sample_dtype`` ("f32": samples stored in single precision; "f32mma": that, and the sample GEMM on the f32 matrix cores, an
    ordered fmaf chain per sample -- ``_lib.Batch.set_sample_dtype``) and ``rng`` ("philox": counter-based generator) --
    the last two are opt-in modes outside the reference-parity statements -- and ``history`` ('obs', 'curves' or 'full') with
    ``history_cap``: what ``return_lines=True`` collects per iteration is recorded on the device instead, the loop runs in
    its normal groups without a wait per iteration, and ``history()`` returns it after ``__call__``."""

    def __init__(self, init, grad_img, kernel_options=(1, 3, 3), noise_y=1, obs=np.array([], dtype=np.int8),
                 N_samples=500, score_thresh=1, delta_x=20, keep_ratio=0.1, pixel_thresh=5, seed=42,
                 return_std=False, fix_endpoints=True, *, device=0, stream=None, factor_cap=0, z_cols=0,
                 sample_dtype=None, rng=None, history=None, history_cap=64, _ctx=None):
        p = resolve_params(init, np.asarray(grad_img).shape, kernel_options, noise_y, obs, N_samples, score_thresh,
                           delta_x, keep_ratio, pixel_thresh, seed, return_std, fix_endpoints)
        self._p = p
        for k in ("init", "x_st", "x_en", "noise_y", "N_samples", "obs", "seed", "keep_ratio", "pixel_thresh",
                  "score_thresh", "delta_x", "half_delta", "return_std", "fix_endpoints", "N_inits", "M", "N",
                  "x_grid", "edge_length", "N_subints", "N_keep", "algo_thresh", "sigma_f", "sigma_l",
                  "kernel_type", "kernel_nu"):
            setattr(self, k, p[k])
        self.kde_thresh = 1e-3
        self.X = np.repeat(self.x_grid.reshape(-1, 1), self.N_samples, axis=-1)
        self._ctx = _ctx if _ctx is not None else _lib.Context(device, stream)
        # the library re-normalises the gradient image in float32 (gpet.py:97)
        g32 = np.asarray(grad_img).astype(np.float32)
        self._abi = to_abi_params(p, factor_cap=factor_cap, z_cols=z_cols)
        self._batch = _lib.Batch(self._ctx, [g32], [self._abi], [p["init"]])
        if sample_dtype is not None:  # (keyword beyond the reference's signature: "f32" stores the samples in single precision, "f32mma" also multiplies in it)
            self._batch.set_sample_dtype(sample_dtype)
        if rng is not None:  # ("philox": the counter-based generator instead of numpy's RandomState stream)
            self._batch.set_rng(rng)
        self._history = _lib.history_level(history)
        if self._history:  # (keyword beyond the reference's signature: per-iteration records kept on the device, see history())
            self._batch.set_history(self._history, history_cap)
        self.grad_img = self._batch.read(_lib.BUF_GRAD).astype(np.float64)
        self._n_iter = 0

    # ---- gpet.py:182-268 ---------------------------------------------------------------
    def fit_predict_GP(self, obs, converged=False, seed=0):
        """Not-converged branch: returns ``N_samples`` posterior curves, shape (N, N_samples),
        exactly like the reference (a transposed view of the row-per-sample device buffer)."""
        b = self._batch
        if converged:
            # gpet.py:232-248,262-266: hyper-parameters optimised (1 + 12 L-BFGS-B starts), returns (mean in pixels,
            # std in standardised units -- the reference does not rescale it)
            obs = np.asarray(obs).reshape(-1, 2).astype(np.int64)
            fits, _ = device_final_fits(b, [dict(self._p, seed=int(seed))], [obs], [0])
            y_mean_optim, y_std, self._theta = fits[0]
            return y_mean_optim, y_std
        b.set_obs(0, obs)
        b.fit_predict(want_cov=True)
        b.factor()
        b.normals([seed])
        b.sample()
        return b.read(_lib.BUF_SAMPLES).T

    # ---- gpet.py:371-451 ---------------------------------------------------------------
    def get_best_curves(self, y_samples=None):
        """Scores the samples currently on the device (``y_samples`` given => they are
        uploaded first) and returns (best_curves, best_costs, (optimal_curve, optimal_cost))."""
        b = self._batch
        if y_samples is not None:
            b.write(_lib.BUF_SAMPLES, np.ascontiguousarray(np.asarray(y_samples, dtype=np.float64).T))
        b.score()
        idx = b.read(_lib.BUF_BEST_IDX)
        costs = b.read(_lib.BUF_BEST_COSTS)
        Y = b.read(_lib.BUF_SAMPLES)
        curves = np.stack((np.repeat(self.x_grid.reshape(-1, 1), idx.shape[0], axis=-1).astype(np.float64),
                           Y[idx].T), axis=-1)
        return curves, costs, (curves[:, 0, :], costs[0])

    def cost_funct(self, edge):
        """Cost of one curve given as (N, 2) xy (gpet.py:371-410).  The device scores whole sample sets, so the curve
        takes the place of sample 0 for one scoring pass; the samples and the scores of the set are restored after it."""
        edge = np.asarray(edge, dtype=np.float64)
        edge = edge[edge[:, 0].argsort(), :]
        b = self._batch
        have = b.have_scores
        Y = b.read(_lib.BUF_SAMPLES)
        saved = (Y[0].copy(), b.read(_lib.BUF_COSTS), b.read(_lib.BUF_BEST_IDX), b.read(_lib.BUF_BEST_COSTS))
        Y[0] = edge[:, 1]
        b.write(_lib.BUF_SAMPLES, Y)
        b.score()
        cost = float(b.read(_lib.BUF_COSTS)[0])
        Y[0] = saved[0]
        b.write(_lib.BUF_SAMPLES, Y)
        if have:
            b.write(_lib.BUF_COSTS, saved[1])
            b.write(_lib.BUF_BEST_IDX, saved[2])
            b.write(_lib.BUF_BEST_COSTS, saved[3])
        return cost

    # ---- gpet.py:455-662 ---------------------------------------------------------------
    def _upload_best(self, best_curves, costs):
        """A caller's own best curves (N, n_keep, 2) xy + costs (n_keep,) become samples 0..n_keep-1 of the device's
        sample set, selected in that order."""
        bc = np.asarray(best_curves, dtype=np.float64)
        costs = np.asarray(costs, dtype=np.float64).reshape(-1)
        b = self._batch
        inf = b.info()
        if bc.ndim != 3 or bc.shape[0] != inf["Lg"] or bc.shape[1] != inf["n_keep"] or costs.shape[0] != inf["n_keep"]:
            raise ValueError("best_curves must be (edge_length, N_keep, 2) = (%d, %d, 2) with N_keep costs"
                             % (inf["Lg"], inf["n_keep"]))
        if not np.array_equal(bc[:, 0, 0], self.x_grid.astype(np.float64)):
            raise ValueError("best_curves must be sampled on the tracer's x-grid")
        Y = b.read(_lib.BUF_SAMPLES)
        Y[:inf["n_keep"]] = bc[:, :, 1].T
        b.write(_lib.BUF_SAMPLES, Y)
        b.write(_lib.BUF_BEST_IDX, np.arange(inf["n_keep"], dtype=np.int32))
        b.write(_lib.BUF_BEST_COSTS, costs)

    def kernel_density_estimate(self, best_curves=None, costs=None):
        """(M, N) float64 density image, min-max normalised in float32 (gpet.py:455-529): of the gradient image when
        called without curves (what the constructor stores as ``grad_kde``, gpet.py:127), else the cost-weighted KDE of
        ``best_curves`` (N, N_keep, 2) with ``costs`` (N_keep,)."""
        b = self._batch
        if best_curves is None:
            return b.read(_lib.BUF_GRAD_KDE).astype(np.float64)
        self._upload_best(best_curves, costs)
        b.curve_kde()
        return b.read(_lib.BUF_KDE).astype(np.float64)

    def compute_new_obs(self, pixel_idx, kde_arr, pre_fobs):
        """Pixel scoring, threshold decay, binning and per-bin argmax (gpet.py:532-618) on ``kde_arr``.
        ``pre_fobs`` is in yx order like in the reference; the new observation set comes back as xy int64.
        ``pixel_idx`` is implied by ``kde_arr`` (gpet.py:651-657); a different candidate list is rejected."""
        kde_arr = np.asarray(kde_arr)
        cand = np.argwhere(kde_arr > self.kde_thresh)
        if self.fix_endpoints:
            cand = cand[(cand[:, 1] > self.x_st) & (cand[:, 1] < self.x_en)]
        if pixel_idx is not None and not np.array_equal(np.asarray(pixel_idx), cand):
            raise ValueError("pixel_idx must be the candidates get_best_pixels derives from kde_arr (gpet.py:651-657)")
        b = self._batch
        thresh = b.scalars().score_thresh
        pre = np.asarray(pre_fobs).reshape(-1, 2)[:, [1, 0]].astype(np.int64)
        b.set_obs(0, pre)
        sc = b.scalars()
        sc.score_thresh = thresh
        b.write_scalars(sc)
        b.write(_lib.BUF_KDE, kde_arr.astype(np.float32))
        b.select_pixels_only()
        self.score_thresh = b.scalars().score_thresh
        return b.read(_lib.BUF_OBS)

    def get_best_pixels(self, best_curves=None, costs=None, pre_fobs=None):
        """KDE of the best curves + pixel scoring / binning / non-max suppression on the device (gpet.py:622-662).
        Arguments given => they are what is used (``pre_fobs`` in yx order, as the reference passes it); arguments
        omitted => the curves scored last and the observation set already on the device.  Returns the new
        observation set (xy int64)."""
        b = self._batch
        if pre_fobs is not None:
            thresh = b.scalars().score_thresh
            b.set_obs(0, np.asarray(pre_fobs).reshape(-1, 2)[:, [1, 0]].astype(np.int64))
            sc = b.scalars()
            sc.score_thresh = thresh
            b.write_scalars(sc)
        if best_curves is not None:
            self._upload_best(best_curves, costs)
        b.select_pixels()
        self.score_thresh = b.scalars().score_thresh
        return b.read(_lib.BUF_OBS)

    def final_cost(self):
        """The cost of the converged mean curve of the last ``__call__`` -- the reference's ``cost_funct(optim_mean_curve)``, the
        last entry of its ``iter_optimal_costs`` (gpet.py:888-890) -- computed on the device from the converged fit
        (gpet_batch_final_costs); the samples and scores of the loop stay as they are.  GpetError before ``__call__``."""
        return float(self._batch.final_costs()[0])

    def history(self):
        """The iteration history of the last ``__call__`` (constructor keyword ``history``): the dict ``_lib.decode_history``
        gives for this edge -- ``obs``, ``score_thresh``, ``optimal_cost``, ``best_idx`` per iteration, from 'curves'
        ``optimal_curves``, with 'full' ``mean`` and ``std`` of the samples per column.  GpetError without ``history``."""
        return self._batch.history()[0]

    def __call__(self, print_final_diagnostics=False, show_init_post=False, show_post_iter=False, verbose=False,
                 return_lines=False, max_iter=1000):
        """Runs the trace (gpet.py:768-908).  The while-loop of the reference (gpet.py:829-870)
        lives on the device; the host only polls the per-edge ``done`` flag."""
        all_samples, all_obs = [], [self.obs]
        iter_optimal_curves, iter_optimal_costs = [], []
        if show_init_post or show_post_iter or print_final_diagnostics:
            import warnings
            warnings.warn("plotting flags are accepted for API compatibility but ignored by the GPU tracer")
        alg_st = t.time()
        b = self._batch
        b.set_obs(0, self.obs)
        n_iter = 0
        while not b.scalars().done:
            if n_iter >= max_iter:
                raise _lib.GpetError(_lib.ERR_ITER_CAP, f"trace did not converge in {max_iter} iterations")
            # (with a device history and nothing to show per iteration: whole groups, the loop returns when the edge is done)
            step = min(1 if (return_lines or verbose) else (64 if self._history else 4), max_iter - n_iter)
            st = t.time()
            if verbose:
                print('Fitting Gaussian process and computing next set of observations...')
            b.iterate([self.seed], step)
            s = b.scalars()
            n_iter = s.iter
            if return_lines:
                all_samples.append(b.read(_lib.BUF_SAMPLES).T)
                idx = b.read(_lib.BUF_BEST_IDX)
                iter_optimal_curves.append(np.stack((self.x_grid.astype(np.float64), all_samples[-1][:, idx[0]]), -1))
                iter_optimal_costs.append(b.read(_lib.BUF_BEST_COSTS)[0])
                all_obs.append(b.read(_lib.BUF_OBS))
            if verbose:
                print(f'Number of observations: {s.n_obs}')
                print(f'Iteration {n_iter + 1} - Time Elapsed: {round(t.time() - st, 4)}\n\n')
        self._n_iter = n_iter
        self.iter_optimal_costs = iter_optimal_costs  # (with return_lines: best_costs[0] of every iteration, gpet.py:449)
        pre_fobs = b.read(_lib.BUF_OBS)
        self.score_thresh = b.scalars().score_thresh
        # final hyper-parameter-optimised fit (gpet.py:874-876), seed = seed + N_iter; on the device
        fits, _ = device_final_fits(b, [dict(self._p, seed=self.seed)], None, [n_iter])
        y_mean_optim, y_std, self._theta = fits[0]
        cred_interval = (y_mean_optim - 1.96 * y_std, y_mean_optim + 1.96 * y_std)
        all_samples.append(y_mean_optim)
        all_obs.append(pre_fobs)
        optim_mean_curve = np.concatenate([self.x_grid[:, np.newaxis], y_mean_optim[:, np.newaxis]], axis=1)
        edge_trace = np.rint(optim_mean_curve[:, [1, 0]]).astype(int)
        iter_optimal_curves.append(edge_trace[:, [1, 0]])
        if verbose:
            print(f'Time elapsed before algorithm converged: {round(t.time() - alg_st, 3)}')
        if self.return_std:
            return edge_trace, cred_interval
        if not return_lines:
            return edge_trace
        return edge_trace, (all_samples, all_obs, iter_optimal_curves)


def device_final_fits(batch, ps, obs_list, iters):
    """Converged fits (gpet.py:874) of every edge of a batch at once, entirely on the device (gpet_final_fit_all):
    training sets from the observation sets on the device (``obs_list`` given => those are set first), standardised
    like the reference does, theta0 + 12 restarts from ``RandomState(seed + iters[e])``, L-BFGS-B for all 13 B
    problems in lock step with one batched objective launch per round, best restart, posterior at the optimum.
    Returns ([(mean in pixels, std in standardised units, theta)] per edge, number of optimiser rounds)."""
    if obs_list is not None:
        for e, o in enumerate(obs_list):
            batch.set_obs(e, np.asarray(o).reshape(-1, 2).astype(np.int64))
    mean, std, theta, fmin, rounds = batch.final_fit_all([p["seed"] + iters[e] for e, p in enumerate(ps)])
    out = [(mean[e, :len(p["x_grid"])].copy(), std[e, :len(p["x_grid"])].copy(), theta[e].copy()) for e, p in enumerate(ps)]
    return out, rounds


def results_from_records(rec, return_std):
    """Per-edge results in the form ``finish`` returns them -- edge_trace (edge_len, 2) int64 yx, or (edge_trace, (lower,
    upper)) with ``return_std`` -- from decoded result records (_lib.decode_results), trimmed to each edge's own length;
    and the statistics dict(n_iter, n_obs, theta, nlml), one entry per edge."""
    out = []
    for e, L in enumerate(rec["edge_len"].tolist()):
        et = rec["trace"][e, :L]
        out.append((et, (rec["lower"][e, :L], rec["upper"][e, :L])) if return_std else et)
    stats = dict(n_iter=rec["n_iter"], n_obs=rec["n_obs"], theta=rec["theta"], nlml=rec["nlml"])
    return out, stats


def resolve_orientation(orientation):
    """True for ``orientation='vertical'``, False for ``'horizontal'`` (the default everywhere); ValueError for anything else."""
    if orientation == "horizontal":
        return False
    if orientation == "vertical":
        return True
    raise ValueError("orientation must be 'horizontal' or 'vertical', not %r" % (orientation,))


def swap_xy(points):
    """The coordinate swap of a vertical batch, its own inverse: point-valued data -- an (..., 2) array, or a list of arrays -- with
    the two coordinates of every point exchanged (a copy).  A vertical batch is the horizontal batch on the transposed gradient image:
    a frame point (x, y) is the batch's (y, x), and a trace the batch returns as (row, column) of the transposed image is (column,
    row) of the frame.  Position-valued vectors (``lower`` / ``upper``, ``mean``, an ensemble's ``median`` ...) are frame columns
    indexed by frame row as they are, and are not touched."""
    if isinstance(points, (list, tuple)) and all(isinstance(p, np.ndarray) for p in points):
        return [swap_xy(p) for p in points]
    a = np.asarray(points)
    if a.ndim == 0 or a.shape[-1] != 2:
        if a.size == 0:
            return np.array(a, copy=True)
        raise ValueError("points are (..., 2) arrays, not of shape %s" % (a.shape,))
    return np.ascontiguousarray(a[..., ::-1])


def swap_record(d, keys=("trace", "obs", "optimal_curves")):
    """A copy of the dict ``d`` (a history, an ensemble, decoded result records) with its point-valued entries ``keys`` swapped by
    ``swap_xy``; entries that are missing or None stay so, everything else is shared."""
    out = dict(d)
    for k in keys:
        if out.get(k) is not None:
            out[k] = swap_xy(out[k])
    return out


def vertical_inits(inits):
    """The init points of vertical edges, given as (x, y) of the frame, in the batch's coordinates: swapped, after the check that the
    points of an edge lie in distinct rows (they are what the trace is a function of)."""
    out = []
    for e, init in enumerate(inits):
        a = np.asarray(init)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError("init of edge %d has shape %s, not (n_init, 2)" % (e, a.shape))
        if len(np.unique(a[:, 1])) != a.shape[0]:
            raise ValueError("init of edge %d: two init points of a vertical edge lie in the same row (y = %s)" % (e, a[:, 1].tolist()))
        out.append(swap_xy(a))
    return out


def _as_list(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


def _raw_stack(raw_imgs):
    """(frames, shared): a 2-D array is ONE frame shared by all edges; a list / tuple or a (B, M, N) array one frame per edge."""
    if isinstance(raw_imgs, (list, tuple)):
        return list(raw_imgs), False
    a = np.asarray(raw_imgs)
    if a.ndim == 2:
        return [a], True
    if a.ndim == 3:
        return list(a), False
    raise ValueError("raw_imgs must be an (M, N) frame, a (B, M, N) stack or a list of (M, N) frames")


_BAND_R0_ALONE = "band_r0 places the bands of band_rows: it needs band_rows"


def refuse_polar_vertical(polar, transposed):
    """The one refusal of ``polar`` on a vertical batch or sequence (``transposed``: what ``resolve_orientation`` returned)."""
    if polar is not None and transposed:
        raise ValueError("polar and orientation='vertical' are alternatives: a closed contour is traced as a horizontal edge of "
                         "the unwrapped frame")


def check_kernel_of(kernel_of, n_kernels):
    """``kernel_of`` as a list of ints, every one an index into ``n_kernels`` gradient kernels; ValueError otherwise."""
    kernel_of = [int(v) for v in np.asarray(kernel_of).reshape(-1)]
    if any(k < 0 or k >= n_kernels for k in kernel_of):
        raise ValueError("kernel_of holds an index outside grad_kernel's %d kernels" % n_kernels)
    return kernel_of


def resolve_image_source(n_edges, grad_imgs=None, grad_device_ptrs=None, grad_shape=None, raw_imgs=None, raw_device_ptrs=None,
                         raw_dtype=None, grad_kernel=None, denoise=None, kernel_of=None, image_of=None, band_rows=None, band_r0=None,
                         inits=None, transposed=False, polar=None):
    """What a batch's images come as, decided from the arguments alone (no device): a dict with ``kind`` ("grad" or "raw"),
    ``share`` (one image for all edges), ``shape`` (M, N) and the keyword arguments ``batch`` of ``_lib.Batch`` that carry the
    images.  Gradient images and raw frames are alternatives; raw frames need ``grad_kernel``; device pointers need their
    shape (``grad_shape``) and, raw ones, their dtype (``raw_dtype``).  ``denoise`` = (technique, kwargs) of
    ``gpet_utils.denoise``: raw frames are denoised on the device first; gradient images cannot be.
    ``grad_kernel`` a list of kernels with ``kernel_of`` (one index per edge): edge e reads its raw frame -- ``image_of[e]`` if
    ``image_of`` is given (``n_edges`` then counts the frames), else the shared one or its own -- through
    ``grad_kernel[kernel_of[e]]``.  The dict then also has ``image_of``, the edge-to-slot map of the slot table
    (``_lib.derive_slots``) the ``raw`` of ``batch`` carries, and ``edge_frames``, the frame of every edge.
    ``band_rows=H`` (with ``inits``, the init points of every edge, and optionally ``band_r0``): tracking bands -- the images are
    full frames, and the dict also has ``band`` = (H, r0 list or None) as ``resolve_bands`` checked it and ``trace_shape`` = (H, N),
    the shape the edges' parameters are resolved for.  ``band_rows=None``: exactly the dict described above.
    ``transposed`` (a vertical batch): the images are (M, N) in the frame's layout -- ``shape`` says so -- and ``trace_shape`` is that
    of the transposed gradient image the batch traces, (N, M); a band is then H of its N rows (frame columns), ``trace_shape``
    (H, M), and ``inits`` are in the batch's coordinates.
    ``polar`` (a dict as ``_lib.polar_spec`` takes it, or a PolarSpec; raw frames only, not with ``transposed``): the frames are
    unwrapped to (radius x angle) first -- ``shape`` is the polar shape (n_r, W), the dict also has ``src_shape``, the frames' own, and
    ``grad_shape`` of device frames is the frames' own.  ``polar=None``: exactly the dict described above."""
    have_grad = grad_imgs is not None or grad_device_ptrs is not None
    have_raw = raw_imgs is not None or raw_device_ptrs is not None
    if polar is not None:
        refuse_polar_vertical(polar, transposed)
        if not have_raw:
            raise ValueError("polar needs raw frames (raw_imgs / raw_device_ptrs with grad_kernel): gradient images are past that stage")
    # (a horizontal batch hears what is wrong with the band keywords themselves before its images are looked at; a vertical one has
    #  always heard of its images first -- the order of two simultaneous refusals is kept)
    if band_rows is not None and not transposed and not have_grad and not have_raw:
        raise ValueError("band_rows needs images: the full frames (raw_imgs / raw_device_ptrs with grad_kernel) or full-frame "
                         "gradient images (grad_imgs / grad_device_ptrs) the bands are cut from")
    if band_rows is None and band_r0 is not None and not transposed:
        raise ValueError(_BAND_R0_ALONE)
    if denoise is not None and not have_raw:
        raise ValueError("denoise needs raw frames (raw_imgs / raw_device_ptrs with grad_kernel): gradient images are past that stage")
    if have_grad and have_raw:
        raise ValueError("pass gradient images (grad_imgs / grad_device_ptrs) or raw frames (raw_imgs / raw_device_ptrs), not both")
    if not have_grad and not have_raw:
        raise ValueError("no images: pass grad_imgs, grad_device_ptrs, raw_imgs or raw_device_ptrs")
    if grad_imgs is not None and grad_device_ptrs is not None:
        raise ValueError("grad_imgs and grad_device_ptrs are alternatives")
    if kernel_of is not None and not have_raw:
        raise ValueError("kernel_of picks the gradient kernel of raw frames (raw_imgs / raw_device_ptrs with grad_kernel): "
                         "gradient images are past that stage")
    if have_raw:
        if raw_imgs is not None and raw_device_ptrs is not None:
            raise ValueError("raw_imgs and raw_device_ptrs are alternatives")
        if grad_kernel is None:
            raise ValueError("raw frames need grad_kernel, the kernel comp_grad_img would be called with")
        kernels, multi = _lib.split_kernels(grad_kernel)
        if multi and kernel_of is None:
            raise ValueError("a list of %d kernels in grad_kernel needs kernel_of, the kernel index of every edge" % len(kernels))
        if kernel_of is not None:
            kernel_of = check_kernel_of(kernel_of, len(kernels))
            if set(kernel_of) != set(range(len(kernels))):
                raise ValueError("kernel_of never uses kernel %d of grad_kernel" % min(set(range(len(kernels))) - set(kernel_of)))
            if image_of is not None and len(image_of) != len(kernel_of):
                raise ValueError("kernel_of has %d entries, image_of %d" % (len(kernel_of), len(image_of)))
        if raw_device_ptrs is not None:
            if grad_shape is None or raw_dtype is None:
                raise ValueError("raw_device_ptrs need grad_shape = (M, N) and raw_dtype")
            frames = _as_list(raw_device_ptrs)
            share, where = len(frames) == 1, dict(device_ptrs=frames, dtype=raw_dtype, shape=grad_shape)
        else:
            frames, share = _raw_stack(raw_imgs)
            where = dict(frames=frames)
        # (a slot table: the distinct (frame, kernel) pairs are the images, and the batch's image map is the edge-to-slot map)
        slots, table = None, {}
        if kernel_of is not None:
            B = len(kernel_of)
            if image_of is None and not share and len(frames) != B:
                raise ValueError("kernel_of has %d entries for %d raw frames, one per edge" % (B, len(frames)))
            edge_frames = [int(v) for v in image_of] if image_of is not None else ([0] * B if share else list(range(B)))
            if image_of is not None and len(frames) != n_edges:
                raise ValueError("%d raw frames for %d frames of the image map" % (len(frames), n_edges))
            frame_of, kernel_of_slot, edge_slot = _lib.derive_slots(edge_frames, kernel_of)
            slots, share, table = (frame_of, kernel_of_slot), False, dict(image_of=edge_slot, edge_frames=edge_frames)
        raw = _lib.RawFrames(kernels if slots is not None else kernels[0], denoise=denoise, slots=slots, polar=polar, **where)
        if slots is None and not share and len(raw) != n_edges:
            raise ValueError("%d raw frames for %d edges" % (len(raw), n_edges))
        src = dict(kind="raw", share=share, shape=tuple(raw.shape), pix=raw.pix, on_device=raw.frames is None,
                   batch=dict(grads=None, raw=raw), **table)
        if polar is not None:
            src["src_shape"] = raw.src_shape
    elif grad_device_ptrs is not None:
        if grad_shape is None:
            raise ValueError("grad_device_ptrs need grad_shape = (M, N)")
        ptrs = _as_list(grad_device_ptrs)
        share = len(ptrs) == 1
        assert share or len(ptrs) == n_edges
        src = dict(kind="grad", share=share, shape=tuple(grad_shape), on_device=True, batch=dict(grads=None, device_ptrs=ptrs, shape=grad_shape))
    else:
        share = not isinstance(grad_imgs, (list, tuple))
        imgs = [grad_imgs] if share else list(grad_imgs)
        assert share or len(imgs) == n_edges
        g32 = [np.ascontiguousarray(g, dtype=np.float32) for g in imgs]
        src = dict(kind="grad", share=share, shape=tuple(g32[0].shape), on_device=False, batch=dict(grads=g32))
    # (the image the batch traces: the transposed gradient image of a vertical batch, and of that the H rows of a band)
    M, N = src["shape"][::-1] if transposed else src["shape"]
    if transposed:
        src["trace_shape"] = (M, N)
    if band_rows is not None:
        src["band"] = resolve_bands(inits, M, band_rows, band_r0)
        src["trace_shape"] = (src["band"][0], N)
    elif band_r0 is not None:
        raise ValueError(_BAND_R0_ALONE)
    return src


def init_row_span(init):
    """(i_lo, i_hi): the smallest and largest row of an edge's init points ((n, 2) xy)."""
    rows = np.asarray(init).reshape(-1, 2)[:, 1].astype(np.int64)
    return int(rows.min()), int(rows.max())


def resolve_bands(inits, M, band_rows, band_r0=None):
    """(H, r0): the tracking bands of a batch as the constructor accepts them, decided without a device -- ``H = band_rows`` rows for
    every edge, ``r0`` a list with one first row per edge, or None when ``band_r0`` is None (the library then places every band from
    its edge's init rows, ``_lib.band_place``).  ValueError naming the edge and the cause (the words of csrc/gpet_band_plan.h's
    band_check) for H > M, a ``band_r0`` of the wrong length, an r0 outside [0, M - H], init rows that span more than H rows, an init
    outside its band."""
    if inits is None:
        raise ValueError("band_rows needs the init points of every edge")
    H, M = int(band_rows), int(M)
    r0 = None
    if band_r0 is not None:
        r0 = [int(v) for v in np.asarray(band_r0).reshape(-1)]
        if len(r0) != len(inits):
            raise ValueError("band_r0 has %d entries for %d edges" % (len(r0), len(inits)))
    for e, init in enumerate(inits):
        i_lo, i_hi = init_row_span(init)
        why = _lib.band_refusal(M, H, None if r0 is None else r0[e], i_lo, i_hi)
        if why is None and (i_lo < 0 or i_hi > M - 1):
            why = "an init point lies outside the frame"
        if why is not None:
            raise ValueError("band of edge %d: %s (M = %d, band_rows = %d, r0 = %s, init rows %d .. %d)"
                             % (e, why, M, H, "placed" if r0 is None else r0[e], i_lo, i_hi))
    return H, r0


def resolve_frame_band(band_rows, band, warm_every, n_edges):
    """What ``set_frame(band=...)`` does with the bands, decided without a device: None (they stay), 'follow' (placed on the device
    from the last traces) or a list of n_edges first rows.  ``band=None`` means 'follow' when ``warm_every`` is given on a banded
    batch, else None.  ValueError for ``band`` on a batch without bands, an unknown word, a table of the wrong length."""
    if band_rows is None:
        if band is not None:
            raise ValueError("band=%r: the batch has no tracking bands (it was built without band_rows)" % (band,))
        return None
    if band is None:
        return "follow" if warm_every is not None else None
    if isinstance(band, str):
        if band != "follow":
            raise ValueError("band must be 'follow' or one first row per edge, not %r" % (band,))
        return band
    r0 = [int(v) for v in np.asarray(band).reshape(-1)]
    if len(r0) != n_edges:
        raise ValueError("band has %d entries for %d edges" % (len(r0), n_edges))
    return r0


def resolve_init_follow(init_follow):
    """``init_follow`` as the constructor, ``set_frame`` and ``SequenceTracer`` accept it, decided without a device: None, or
    ``dict(window=w, cols=a)`` -> (w, a), integers within the limits of csrc/gpet_init_plan.h (``_lib.init_follow_refusal``).
    ValueError naming the cause otherwise."""
    if init_follow is None:
        return None
    if not isinstance(init_follow, dict) or set(init_follow) != {"window", "cols"}:
        raise ValueError("init_follow must be None or dict(window=w, cols=a), not %r" % (init_follow,))
    w, a = init_follow["window"], init_follow["cols"]
    for name, v in (("window", w), ("cols", a)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("init_follow: %s must be an integer, not %r" % (name, v))
    why = _lib.init_follow_refusal(int(w), int(a))
    if why is not None:
        raise ValueError("%s (window = %d, cols = %d)" % (why, w, a))
    return int(w), int(a)


def resolve_frame_init(init, init_follow, default_follow, cur_inits, frame_M, band_rows=None, band=None):
    """What ``set_frame(init=..., init_follow=...)`` does with the init points, decided without a device: ('keep', None), ('follow',
    (window, cols)) or ('set', list of (n_init, 2) int64 xy arrays sorted by x).  ``default_follow``: the constructor's setting as
    ``resolve_init_follow`` returned it; ``cur_inits``: the batch's current table; ``band``: what ``resolve_frame_band`` decided.
    ``init=None`` means 'follow' when the constructor or this call has ``init_follow``, else 'keep'.  ValueError for an unknown word,
    'follow' without a window, ``init_follow`` next to 'keep' or a list, a list that differs from the batch in the number of edges, of
    points or in an x, a row outside the frame and, on a banded batch, a list without an explicit ``band=[r0_e]`` or outside it
    (``_lib.band_refusal``'s words)."""
    call = resolve_init_follow(init_follow)
    follow = call if call is not None else default_follow
    if init is None:
        return ("follow", follow) if follow is not None else ("keep", None)
    if isinstance(init, str):
        if init == "keep":
            if call is not None:
                raise ValueError("init='keep' and init_follow are alternatives: the window is what 'follow' searches")
            return "keep", None
        if init == "follow":
            if follow is None:
                raise ValueError("init='follow' needs init_follow=dict(window=w, cols=a), here or in the constructor")
            return "follow", follow
        raise ValueError("init must be None, 'keep', 'follow' or one array of init points per edge, not %r" % (init,))
    if call is not None:
        raise ValueError("init points given as arrays and init_follow are alternatives: nothing is searched for")
    given = list(init)
    if len(given) != len(cur_inits):
        raise ValueError("init has %d entries for %d edges" % (len(given), len(cur_inits)))
    if band_rows is not None and not isinstance(band, list):
        raise ValueError("init points given as arrays on a batch with tracking bands need the bands too: band=[r0 of every edge]")
    out = []
    for e, (new, cur) in enumerate(zip(given, cur_inits)):
        a = np.asarray(new)
        if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] != len(cur):
            raise ValueError("init of edge %d has shape %s, the batch holds %d init points (n, 2)" % (e, a.shape, len(cur)))
        if not np.array_equal(a, np.rint(a)):
            raise ValueError("init of edge %d is not integral" % e)
        a = a[np.argsort(a[:, 0])].astype(np.int64)
        if not np.array_equal(a[:, 0], np.asarray(cur)[:, 0]):
            raise ValueError("init of edge %d has x = %s, the batch was built with x = %s: the x of an init point cannot change"
                             % (e, a[:, 0].tolist(), np.asarray(cur)[:, 0].tolist()))
        i_lo, i_hi = init_row_span(a)
        if i_lo < 0 or i_hi > frame_M - 1:
            raise ValueError("init of edge %d: an init point lies outside the frame (init rows %d .. %d, M = %d)" % (e, i_lo, i_hi, frame_M))
        if band_rows is not None:
            why = _lib.band_refusal(frame_M, band_rows, band[e], i_lo, i_hi)
            if why is not None:
                raise ValueError("band of edge %d: %s (M = %d, band_rows = %d, r0 = %d, new init rows %d .. %d)"
                                 % (e, why, frame_M, band_rows, band[e], i_lo, i_hi))
        out.append(a)
    return "set", out


def _shift_rows(d, keys, r0, col=None):
    """``d`` with ``r0`` added to the row-valued entries ``keys`` (column ``col`` of 2-D ones)."""
    out = dict(d)
    for k in keys:
        if k not in d or d[k] is None:
            continue
        a = np.array(d[k], copy=True)
        if col is None or a.ndim == 1:
            a = a + r0
        else:
            a[..., col] += r0
        out[k] = a
    return out


class BatchImages(object):
    """What images a batch takes and what its next frames must look like: the one place that knows, and it needs no device.  Built
    once from the image arguments of ``GP_Edge_Tracing_Batch`` (``inits`` in the batch's coordinates, ``transposed`` what
    ``resolve_orientation`` returned); ``resolve_image_source`` decides, here and in ``next_frame``.
    ``batch_kwargs``: the keyword arguments of ``_lib.Batch`` that carry the images (``grads``, ``share_image`` and the library's own
    ``image_of`` -- the edge-to-slot map where there is a slot table -- included); ``trace_shape``: the shape the edges' parameters are
    resolved for; ``band``: (H, r0 list or None), or None without bands; ``polar`` / ``src_shape``: the resolved polar spec (pad
    known) and the frames' own shape, or None; ``edge_frames``: the frame of every edge of a slot table, else None.
    ``n_img`` images of ``frame_shape`` (as they lie in the caller's memory; the polar shape of a polar batch) are what the library
    holds, derived the way it derives them -- one shared image: 1; an image map: its count; a slot table: its slots; else one per edge
    -- and ``n_frames`` raw frames are what makes them: as many, but behind a slot table the frames the constructor got."""

    def __init__(self, inits, grad_imgs=None, grad_device_ptrs=None, grad_shape=None, raw_imgs=None, raw_device_ptrs=None, raw_dtype=None,
                 grad_kernel=None, denoise=None, image_of=None, kernel_of=None, band_rows=None, band_r0=None, polar=None, transposed=False):
        B = n_given = len(inits)
        if image_of is not None:
            image_of = [int(v) for v in np.asarray(image_of).reshape(-1)]
            if len(image_of) != B:
                raise ValueError("image_of has %d entries for %d edges" % (len(image_of), B))
            n_given = max(image_of) + 1
            given = [a for a in (grad_imgs, grad_device_ptrs, raw_imgs, raw_device_ptrs) if a is not None]
            if len(given) == 1 and not (isinstance(given[0], (list, tuple)) or np.ndim(given[0]) == 3):
                raise ValueError("with image_of the images are a list (or stack) of n_img = %d" % n_given)
            if len(given) == 1 and len(given[0]) != n_given:
                raise ValueError("%d images for an image map of n_img = %d" % (len(given[0]), n_given))
            if grad_imgs is not None:
                grad_imgs = list(grad_imgs)
        if kernel_of is not None and len(np.asarray(kernel_of).reshape(-1)) != B:
            raise ValueError("kernel_of has %d entries for %d edges" % (len(np.asarray(kernel_of).reshape(-1)), B))
        src = resolve_image_source(n_given, grad_imgs, grad_device_ptrs, grad_shape, raw_imgs, raw_device_ptrs, raw_dtype, grad_kernel,
                                   denoise, kernel_of=kernel_of, image_of=image_of, band_rows=band_rows, band_r0=band_r0,
                                   inits=None if band_rows is None else list(inits), transposed=transposed, polar=polar)
        raw = src["batch"].get("raw")
        self.transposed = transposed
        self.trace_shape, self.frame_shape = src.get("trace_shape", src["shape"]), src["shape"]
        self.band, self.src_shape, self.edge_frames = src.get("band"), src.get("src_shape"), src.get("edge_frames")
        self.polar = None if polar is None else raw.polar  # (resolved: pad known)
        self.mapped = image_of is not None
        self.share = src["share"] and not self.mapped  # (a map of one image is the shared layout, decided by the library)
        # (what next_frame falls back on; with a slot table the kernels as the table counts them and the kernel of every edge)
        self._dtype, self._denoise, self._kernel_of = raw_dtype, denoise, None
        self.n_img = self.n_frames = 1 if self.share else n_given
        if self.edge_frames is not None:
            self._kernel, self._kernel_of = raw.kernels, check_kernel_of(kernel_of, len(raw.kernels))
            image_of, self.n_img, self.n_frames = src["image_of"], raw.n_slots, len(raw)
        else:
            self._kernel = None if grad_kernel is None else np.array(grad_kernel, dtype=np.float64)
        self.batch_kwargs = dict(src["batch"], share_image=self.share, image_of=image_of, transposed=transposed)
        if self.band is not None:
            self.batch_kwargs["band"] = self.band

    def images_text(self):
        if self._kernel_of is not None:
            return "%d raw frames behind the %d image slots of the batch's slot table" % (self.n_frames, self.n_img)
        if self.mapped:
            return "%d images, the batch's image map has n_img = %d" % (self.n_img, self.n_img)
        return "one shared image" if self.share else "one image per edge, %d" % self.n_img

    def misfit(self, what, n, shape=True):
        """The one refusal of images that do not fit the batch: ``n`` of ``what`` ('frames' / 'images') were given."""
        return ValueError("the new %s do not fit the batch: %d given (%s%s)"
                          % (what, n, self.images_text(), ", %d x %d" % self.frame_shape if shape else ""))

    def frame_polar(self, polar, have_raw):
        """The spec ``set_frame`` unwraps the new frames with: the batch's own, or the one ``polar`` asks for when it keeps the shape and
        the meaning of rows and columns.  ValueError for everything else."""
        if polar is None:
            return self.polar
        if self.polar is None:
            raise ValueError("polar: this batch was not built on polar frames (give polar= to the constructor)")
        if not have_raw:
            raise ValueError("polar needs raw frames (raw_imgs / raw_device_ptrs): gradient images are past that stage")
        if isinstance(polar, dict):
            polar = dict(self.polar.as_dict(), **{k: v for k, v in polar.items() if not (k == "pad" and v is None)})
        new = _lib.polar_spec(polar).resolved(self.polar.pad)
        old = self.polar
        if (new.n_r, new.n_theta, new.pad) != (old.n_r, old.n_theta, old.pad):
            raise ValueError("polar: set_frame cannot change the shape of the polar frames: n_r, n_theta, pad are %d, %d, %d, not %d, %d, %d"
                             % (old.n_r, old.n_theta, old.pad, new.n_r, new.n_theta, new.pad))
        if (new.r0, new.dr, new.theta0) != (old.r0, old.dr, old.theta0):
            raise ValueError("polar: set_frame replaces the centres only: r0, dr, theta0 are %r, %r, %r" % (old.r0, old.dr, old.theta0))
        return new

    def next_frame(self, grad_imgs=None, grad_device_ptrs=None, raw_imgs=None, raw_device_ptrs=None, raw_dtype=None, grad_kernel=None,
                   denoise=None, polar=None):
        """(the keyword arguments of ``Batch.set_images`` that carry the next frame's images, the polar spec to adopt with them), from
        the image arguments of ``set_frame``; kernel(s), slot table, dtype and ``denoise`` are the constructor's where the call does
        not give them.  ValueError for images that do not fit the batch and whatever else ``set_frame`` refuses about them.  Pure:
        nothing on this object changes (``set_frame`` adopts the spec once the images are swapped)."""
        have_raw = raw_imgs is not None or raw_device_ptrs is not None
        new_polar = self.frame_polar(polar, have_raw)
        if denoise not in (None, False) and not have_raw:
            raise ValueError("denoise needs raw frames (raw_imgs / raw_device_ptrs)")
        if have_raw:
            if raw_imgs is not None and self.batch_kwargs["image_of"] is not None and np.ndim(raw_imgs) == 2:
                raw_imgs = [raw_imgs]  # (a 2-D array is ONE frame)
            have = raw_imgs if raw_imgs is not None else _as_list(raw_device_ptrs)
            if not (self.n_frames == 1 and np.ndim(have) == 2) and len(have) != self.n_frames:
                raise self.misfit("frames", len(have))
            src = resolve_image_source(self.n_frames, grad_imgs, grad_device_ptrs,
                                       self.frame_shape if self.polar is None else self.src_shape,  # (device frames: their own shape)
                                       raw_imgs, raw_device_ptrs, self._dtype if raw_dtype is None else raw_dtype,
                                       self._kernel if grad_kernel is None else grad_kernel,
                                       None if denoise is False else (self._denoise if denoise is None else denoise),
                                       kernel_of=self._kernel_of, image_of=self.edge_frames, polar=new_polar)
            raw = src["batch"]["raw"]
            # (whether ONE image is shared was decided at construction: a batch of one edge has one image either way)
            if len(raw) != self.n_frames or src["shape"] != self.frame_shape:
                raise self.misfit("frames", len(raw))
            return dict(raw=raw), new_polar
        if grad_device_ptrs is not None:
            ptrs = _as_list(grad_device_ptrs)
            if len(ptrs) != self.n_img:
                raise self.misfit("images", len(ptrs), shape=False)
            return dict(device_ptrs=ptrs), new_polar
        imgs = list(grad_imgs) if isinstance(grad_imgs, (list, tuple)) else [grad_imgs]
        if len(imgs) != self.n_img or any(np.shape(g) != self.frame_shape for g in imgs):
            raise self.misfit("images", len(imgs))
        return dict(grads=[np.ascontiguousarray(g, dtype=np.float32) for g in imgs]), new_polar  # (no copy of f32 input)


class GP_Edge_Tracing_Batch(object):
    """B independent edges traced together on one GPU (BASELINE config 4's per-GPU share).

    Not in the reference (which traces one edge per object); it is the batched form of the same
    algorithm: every kernel takes the edge index from blockIdx, finished edges are skipped, and
    edge e's result equals what ``GP_Edge_Tracing`` returns for the same arguments.

    ``inits``: list of (n_init, 2) xy arrays; ``grad_imgs``: one (M, N) image shared by all edges
    or a list with one image per edge; ``seeds``: per-edge RNG seed (gpet.py:33,839).
    Remaining keyword arguments are the reference constructor's (gpet.py:22-35), common to all edges.
    """

    def __init__(self, inits, grad_imgs, seeds, kernel_options=(1, 3, 3), noise_y=1, N_samples=500, score_thresh=1,
                 delta_x=20, keep_ratio=0.1, pixel_thresh=5, return_std=False, fix_endpoints=True, *, obs=None,
                 device=0, stream=None, factor_cap=0, z_cols=0, _ctx=None, grad_device_ptrs=None, grad_shape=None,
                 sample_dtype=None, rng=None, raw_imgs=None, grad_kernel=None, raw_device_ptrs=None, raw_dtype=None,
                 denoise=None, image_of=None, history=None, history_cap=64, kernel_of=None, band_rows=None, band_r0=None,
                 init_follow=None, orientation="horizontal", _batch_coords=False, polar=None):
        """``obs``: optional list of per-edge warm-start observation sets (xy), the reference's ``obs`` constructor
        argument (gpet.py:57-61,100,820).  ``grad_device_ptrs`` + ``grad_shape``: the gradient image(s) already live
        on this GPU (e.g. a torch tensor an RCCL broadcast filled): integer device addresses of f32 (M, N) arrays,
        consumed in place instead of ``grad_imgs``.
        ``raw_imgs`` + ``grad_kernel`` (with ``grad_imgs=None``): the frames themselves -- one (M, N) frame for all edges, or a
        list / (B, M, N) stack with one per edge; uint8, uint16, float32 and float64 go to the device as they are, other
        dtypes as float64 -- and the kernel ``comp_grad_img`` would be called with: the gradient images are made on the
        device, all frames in one pass, and the batch equals the one built from ``comp_grad_img``'s outputs bit for bit.
        ``raw_device_ptrs`` + ``raw_dtype`` + ``grad_shape``: the same for frames already on this GPU.  The kernel is
        remembered for ``set_frame``.
        ``denoise=(technique, kwargs)`` (raw frames only): ``gpet_utils.denoise`` of every frame on the device, in the same
        pass, before the kernel is applied; the batch equals the one built from ``gpet_utils.denoise_imgs``' outputs bit for
        bit.  Remembered for ``set_frame`` like the kernel.
        ``image_of``: an image map -- B indices, edge e reads image ``image_of[e]`` -- for frames with several edges on them
        (the layers of a retina, the two walls of a vessel).  ``grad_imgs``, ``grad_device_ptrs``, ``raw_imgs`` and
        ``raw_device_ptrs`` are then ``n_img = max(image_of) + 1`` long instead of B, every index must occur (in any order:
        ``[0, 1, 2, 0, 1, 2]`` is valid), and ``set_frame`` expects ``n_img`` images.  Every image is uploaded, turned into a
        gradient image, denoised and run through the gradient KDE once; the batch equals the one built from the B images
        ``imgs[image_of[e]]`` bit for bit.
        ``grad_kernel=[K0, K1, ...]`` with ``kernel_of`` (B indices): edge e reads its raw frame through
        ``grad_kernel[kernel_of[e]]`` -- the upper wall of a dark lumen is a bright-to-dark edge, the lower wall dark-to-bright,
        on the same frame.  With ``image_of``, that argument keeps meaning "edge e reads raw frame ``image_of[e]``" (the frames
        are ``max(image_of) + 1`` long); without it the frame is shared or per edge as ever.  The image slots are the distinct
        (frame, kernel) pairs (``_lib.derive_slots``); every frame is uploaded, denoised and staged on the device once, however
        many kernels read it, and the batch equals the one built from ``comp_grad_imgs(frames, K[k])``' outputs bit for bit.
        ``set_frame(raw_imgs=...)`` then expects as many frames as the constructor got and reuses kernels and table.
        ``history`` = 'obs', 'curves' or 'full' (default None: off): every loop iteration of every edge leaves a record on the
        device -- the new observation set, the score threshold, the optimal cost and sample index; from 'curves' the optimal
        curve; with 'full' the per-column mean and std of all samples -- read with ``history()`` after ``run_loop`` or
        ``__call__``.  ``history_cap``: records kept per edge; later iterations are counted in ``dropped``, the trace is not
        affected.  No result depends on the level.
        ``band_rows=H`` (with ``band_r0``, one first row per edge; default: placed from the init rows): tracking bands -- the images
        are full frames (raw frames, or full-frame gradient images), and edge e traces rows ``r0 .. r0 + H - 1`` of its full-frame
        gradient image only: bit for bit what a batch without bands gives for the cropped gradient image ``G[r0:r0 + H]`` and the
        init ``init - (0, r0)``, with every row it returns (traces, intervals, ``history``, ``ensemble``, ``results``) raised by
        ``r0`` again.  ``inits`` and ``obs`` are in full-frame rows; presets of ``kernel_options`` that depend on the image height
        see H.  ``band_r0`` (attribute) holds the current table; ``set_frame(band=...)`` moves the bands.
        ``init_follow=dict(window=w, cols=a)``: endpoint tracking -- once the images are made, every init point (x, y) of every edge
        moves, on the device, to the row within ``w`` rows of y whose gradient summed over the columns ``x - a .. x + a`` is largest
        (the rule: csrc/gpet_init_plan.h; ties to the nearest, then the upper row; nothing positive in reach: the point stays; x
        never moves), so rough clicks land on the edge.  On a banded batch the search stays inside the band.  The setting is
        remembered: ``set_frame`` then follows by default.  ``inits`` (attribute) is the current table, a list of (n_init, 2) int64
        xy arrays in full-frame rows; ``reset()`` keeps it.
        ``orientation='vertical'``: the edges run down the frame -- x is a function of y.  The batch is, bit for bit, the horizontal
        batch on the TRANSPOSE of every frame's gradient image with the two coordinates of every point swapped, and whatever it returns
        is swapped back (``swap_xy``): denoising and ``grad_kernel`` are applied to the frames as they lie (a vertical kernel:
        ``kernel_builder(size, vertical_edges=True)``), the transposed image is written on the device in the same pass, and gradient
        images given by the caller are in the frame's layout too.  ``inits``, ``obs`` and ``set_frame(init=[...])`` are (x, y) of the
        frame; the init points of an edge lie in distinct rows.  Traces are (row, column) of the frame with one entry per traced
        ROW; ``history()['obs']`` / ``['optimal_curves']`` are (x, y) of the frame; ``lower`` / ``upper``, the history's ``mean`` and an
        ensemble's ``median``, ``q_lo``, ``q_hi``, ``min``, ``max`` are frame columns indexed by frame row.  Presets of
        ``kernel_options`` see the transposed image: its height is the frame's width, the edge length the row span.  ``band_rows=H``
        is a band of H frame COLUMNS with ``band_r0`` its first column; ``init_follow=dict(window=w, cols=a)`` searches w columns
        left and right of a point, summing over a rows above and below: x moves, y never does.
        ``polar=dict(centre=(cx, cy) | (n_frames, 2) array, n_r=, n_theta=, r0=0.0, dr=1.0, theta0=0.0, pad=None)`` (raw frames only):
        closed contours -- every frame is resampled on the device to (radius x angle) around its centre (``gpet_utils.unwrap_polar_imgs``;
        the rule: csrc/gpet_polar_plan.h) before anything else happens to it, and the batch is, bit for bit, the batch on
        ``unwrap_polar_imgs(frames, **polar)`` given as float64 frames.  ``inits``, ``obs``, traces, intervals, bands, ``history()`` and
        ``ensemble()`` are in polar rows (radius ``r0 + row dr``) and columns (angle index ``(column - pad) mod n_theta``);
        ``gpet_utils.closed_init(row, batch.polar)`` gives the two init points that close the contour, ``gpet_utils.polar_trace_xy`` maps
        a result back to the frame.  ``pad=None``: half the width of the widest kernel.  ``polar`` (attribute) is the resolved spec;
        ``grad_shape`` of ``raw_device_ptrs`` stays the frames' own shape.  ``set_frame`` keeps the spec; ``set_frame(...,
        polar=dict(centre=...))`` replaces the centres.  Refused with gradient images and with ``orientation='vertical'``."""
        self.orientation = orientation
        tr = resolve_orientation(orientation)       # the library holds the transposed gradient images
        self._swap = tr and not _batch_coords       # ... and this object swaps the coordinates of what it takes and returns
        refuse_polar_vertical(polar, tr)  # (before the init points are looked at as those of a vertical edge)
        if self._swap:
            inits = vertical_inits(inits)
            obs = None if obs is None else [swap_xy(np.asarray(o).reshape(-1, 2)) for o in obs]
        B = len(inits)
        self._init_follow = resolve_init_follow(init_follow)
        im = self._images = BatchImages(inits, grad_imgs, grad_device_ptrs, grad_shape, raw_imgs, raw_device_ptrs, raw_dtype, grad_kernel,
                                        denoise, image_of, kernel_of, band_rows, band_r0, polar, transposed=tr)
        self.band_rows, self.band_r0 = (None, None) if im.band is None else im.band
        shapes = [im.trace_shape] * B  # (banded: the parameters are those of the (H, N) crop)
        assert len(seeds) == B
        obs = [np.array([])] * B if obs is None else list(obs)
        inits = list(inits)  # (an ndarray of shape (B, n, 2) makes a fresh view per access: materialise the items once)
        # (edges with the same init points, observations and image shape resolve to the same parameters but for the seed, which
        #  nothing derived depends on: resolved once per distinct triple -- a batch of 1 024 equal edges spent 8 ms here.  The key
        #  is the CONTENT: object identities can be reused by temporaries)
        def content(a):
            a = np.asarray(a)
            return (a.shape, a.dtype.str, a.tobytes())
        self._ps, abi, memo, by_id = [], [], {}, {}
        for e in range(B):
            ik = (id(inits[e]), id(obs[e]))  # (the items are alive in `inits` / `obs`, so these identities are stable here)
            ck = by_id.get(ik)
            if ck is None:
                ck = by_id[ik] = (content(inits[e]), tuple(shapes[e]), content(obs[e]))
            key = ck
            hit = memo.get(key)
            if hit is None:
                pe = resolve_params(inits[e], shapes[e], kernel_options, noise_y, obs[e], N_samples, score_thresh,
                                    delta_x, keep_ratio, pixel_thresh, int(seeds[e]), return_std, fix_endpoints)
                hit = memo[key] = (pe, to_abi_params(pe, factor_cap=factor_cap, z_cols=z_cols))
            else:
                pe = dict(hit[0], seed=int(seeds[e]))
                pe["init"] = hit[0]["init"].copy()
                pe["obs"] = np.array(hit[0]["obs"], copy=True)
            self._ps.append(pe)
            abi.append(hit[1])
        self._ctx = _ctx if _ctx is not None else _lib.Context(device, stream)
        kw = dict(im.batch_kwargs)
        self._batch = _lib.Batch(self._ctx, kw.pop("grads"), abi, [p["init"] for p in self._ps], **kw)
        # (from here on what fits the batch is decided by `im` alone: once, that it counts the images as the library does)
        assert (im.n_img, tuple(im.frame_shape)) == (self._batch.n_img, tuple(self._batch.frame_shape))
        if band_rows is not None:  # (the table as the library placed or took it; observations are kept in band rows from here on)
            self.band_r0 = self._batch.band_r0()
            self._init_span = [init_row_span(p["init"]) for p in self._ps]
            for p, r0 in zip(self._ps, self.band_r0):
                p["obs"] = p["obs"] - np.array([0, int(r0)], dtype=np.int64)
        if self._init_follow is not None:  # (the given points refined on the images just made)
            self._take_inits(self._batch.init_follow(*self._init_follow))
        else:
            self._inits = [np.array(p["init"], dtype=np.int64) for p in self._ps]
        if sample_dtype is not None:
            self._batch.set_sample_dtype(sample_dtype)
        if rng is not None:
            self._batch.set_rng(rng)
        if _lib.history_level(history):
            self._batch.set_history(history, history_cap)
        self._set_obs()
        self.B = B
        self.return_std = return_std
        self.seeds = [int(s) for s in seeds]
        self.timings = {}
        self.last_ensemble = None  # (set_frame(warm_from=...): the ensemble of the frame it left)

    def _take_inits(self, table):
        """The current init points as the library holds them now: ``inits``, every edge's parameters and the span the bands respect."""
        self._inits = [np.array(i, dtype=np.int64) for i in table]
        for p, i in zip(self._ps, self._inits):
            p["init"] = i.astype(p["init"].dtype)
        if self.band_rows is not None:
            self._init_span = [init_row_span(i) for i in self._inits]

    @property
    def inits(self):
        """The current init points, a list of (n_init, 2) int64 xy arrays in the frame's coordinates (full-frame rows; the points of a
        vertical edge ordered by y)."""
        return swap_xy(self._inits) if self._swap else self._inits

    def _set_obs(self):
        for e, p in enumerate(self._ps):
            if p["obs"].shape[0]:
                self._batch.set_obs(e, p["obs"])

    def reset(self):
        """Back to the state right after construction (the warm-start observations included): nothing of the trace the
        object ran before is used by the next one."""
        self._batch.reset()
        self._set_obs()

    @property
    def polar(self):
        """The resolved polar spec the frames are unwrapped by (``set_frame`` may replace its centres), None without ``polar=``."""
        return self._images.polar

    def _keep_obs(self, obs):
        """The warm-start observation sets as ``reset()`` sets them again (the device's own are read back once for this)."""
        for p, o in zip(self._ps, obs):
            p["obs"] = np.asarray(o).reshape(-1, 2).astype(np.int64)

    def set_frame(self, grad_imgs=None, obs=None, seeds=None, grad_device_ptrs=None, next_frame=True, raw_imgs=None,
                  raw_device_ptrs=None, raw_dtype=None, grad_kernel=None, denoise=None, warm_every=None, warm_from=None,
                  group_of=None, tol=2, band=None, init=None, init_follow=None, polar=None):
        """The next frame of an image sequence for the same edges (gpet.py:57-61: the previous trace warm-starts the
        next through ``obs``): new gradient image(s) -- host arrays, or device addresses with ``grad_device_ptrs`` --
        new warm-start observations and, optionally, new seeds.  Geometry, kernel and every other parameter stay, so
        what depends only on them (arena, streams, the prior eigenbasis of the structured loop path) is reused.
        ``next_frame`` (default): the images continue the sequences just traced, so the any-rank (Matern) factor of the
        new trace's first iteration may start from the last trace's rows -- an iterative solve, the same rows to its
        tolerance.  ``next_frame=False``: unrelated images; the trace is what a fresh object would compute, bit for bit.
        ``raw_imgs`` / ``raw_device_ptrs``: the frames themselves, as in the constructor; ``grad_kernel``, ``raw_dtype`` and
        ``denoise`` default to the constructor's (``denoise=None``); ``denoise=False`` takes these frames as they are, without
        denoising, whatever the constructor was given.
        A batch with an image map takes ``n_img`` images.  A call whose images do not fit the batch raises ValueError, a
        ``warm_every`` without a last trace raises GpetError, and both leave the batch as it was; a call that is wrong in both ways
        raises the ValueError.
        ``warm_every=k`` instead of ``obs``: the warm start is made on the device (gpet_batch_warm_start) -- every edge's
        observations from its own last converged fit by the rule of ``sequence.warm_start_obs(trace, x_st, x_en, k, algo_thresh,
        M)`` -- with no trip of the traces through the host; the sets are read back once, so that ``reset()`` restores the same
        warm start.  It needs the trace this object ran last (``__call__`` or ``finish``).
        ``warm_from='medoid'``, ``'best_cost'`` or ``'consensus'`` with ``warm_every`` (and ``group_of``, ``tol`` as ``ensemble``
        takes them): the batch traces seed ensembles, and every edge assigned to a group takes its observations from the group's
        medoid, its member of smallest final cost, or the consensus trace -- edges in no group from their own fit, the edges of a
        group without members none.  The ensemble is reduced and kept on the device BEFORE the images are swapped (its final costs
        are scored on the frame just traced; gpet_batch_ensemble_keep), the warm start is made from it after the swap
        (gpet_batch_warm_start_groups); ``last_ensemble`` is then the list ``ensemble(group_of, tol)`` would have returned for the
        frame just left.  ``warm_from=None`` (default): every edge from its own fit, as above.
        ``band`` (a batch with ``band_rows``): ``'follow'`` -- every band is placed on the device from the trace its edge's warm start
        comes from (its own fit, or its group's source with ``warm_from``; ``_lib.band_place``), after the ensemble is kept and before
        the images are swapped, so a group's members share one band -- or one first row per edge; the default is ``'follow'`` with
        ``warm_every`` and "the bands stay" without.  The warm start then carries every row from the source's old band into the
        edge's new one.  A band that cannot hold its edge's init points raises ValueError and leaves the batch as it was.  ``obs``
        are in full-frame rows.
        ``init``: ``'follow'`` -- after the images are swapped and before the warm start, every init point moves onto the edge of
        the new image by the rule of the constructor's ``init_follow`` (or of ``init_follow=dict(window=w, cols=a)`` given here), on
        the device, starting from where it is now; ``'keep'`` -- the points stay; or one (n_init, 2) xy array per edge in full-frame
        rows, with the x and counts the batch has (on a banded batch only together with an explicit ``band=[r0_e]`` that holds them
        as well as the current points).  Default: ``'follow'`` when the constructor or this call has ``init_follow``, else
        ``'keep'``.  Bands are placed against the points as they are BEFORE this call; the search then stays inside the band.
        Whatever is refused without a device -- images that do not fit, ``denoise`` without raw frames and the ensemble keywords
        included -- raises ValueError before anything is touched: every such check comes before the first device call, so neither the
        kept ensemble nor ``last_ensemble`` has changed when it does.
        A vertical batch takes its frames and gradient images in the frame's layout, ``obs`` and ``init`` as (x, y) of the frame, and
        ``band`` as first frame columns.
        A polar batch unwraps the new frames by the constructor's spec; ``polar=dict(centre=...)`` replaces the centres from this frame
        on (the whole dict may be given again: whatever would change the polar shape -- ``n_r``, ``n_theta``, ``pad`` -- or the radii
        and angles behind the rows and columns -- ``r0``, ``dr``, ``theta0`` -- is refused with ValueError)."""
        # 1. every check that needs no device, in the order they are reported
        if polar is not None:  # (a spec that is refused is refused first, as ever; next_frame takes the checked one as it is)
            polar = self._images.frame_polar(polar, raw_imgs is not None or raw_device_ptrs is not None)
        if warm_every is not None and obs is not None:
            raise ValueError("obs and warm_every are alternatives: the device derives the observations itself")
        if warm_from is not None:
            if obs is not None:
                raise ValueError("obs and warm_from are alternatives: the device derives the observations itself")
            if warm_every is None:
                raise ValueError("warm_from chooses the source of the device's warm start: it needs warm_every")
            _lib.warm_from(warm_from)
            groups = self.group_table(group_of)
            if not float(tol) >= 0.0:
                raise ValueError("tol must be >= 0 pixels, not %r" % (tol,))
        if self._swap:  # (a vertical batch: the caller's points into the batch's coordinates)
            if obs is not None:
                obs = [swap_xy(np.asarray(o).reshape(-1, 2)) for o in obs]
            if init is not None and not isinstance(init, str):
                init = vertical_inits(list(init))
        mode = resolve_frame_band(self.band_rows, band, warm_every, len(self._ps))
        if isinstance(mode, list):
            for e, r0 in enumerate(mode):
                why = _lib.band_refusal(self._batch.frame_M, self.band_rows, r0, *self._init_span[e])
                if why is not None:
                    raise ValueError("band of edge %d: %s (M = %d, band_rows = %d, r0 = %d, init rows %d .. %d)"
                                     % ((e, why, self._batch.frame_M, self.band_rows, r0) + self._init_span[e]))
        imode, ipoints = resolve_frame_init(init, init_follow, self._init_follow, self._inits, self._batch.frame_M, self.band_rows, mode)
        images, new_polar = self._images.next_frame(grad_imgs, grad_device_ptrs, raw_imgs, raw_device_ptrs, raw_dtype, grad_kernel, denoise,
                                                    polar)
        # 2. the device calls
        if warm_every is not None or mode == "follow":
            self._batch.warm_start_ready()  # (refused before the images are swapped: the batch stays on its old frames)
        if warm_from is not None:
            # (before the swap: the final costs that break the medoid's ties and define best_cost are those of the frame just traced)
            self._batch.ensemble_keep(groups, tol)
            keys = ("trace", "median", "q_lo", "q_hi", "min", "max", "agree", "members", "off", "cost", "medoid", "best_cost")
            self.last_ensemble = self._ensemble_rows([{k: d[k] for k in keys} for d in self._batch.ensemble_kept()[0]], groups)
        # (placement sits between the kept ensemble and the swap; the swap reads the placed table on the device)
        if mode == "follow":
            self._batch.band_place(frm=warm_from)
        elif mode is not None:
            self._batch.band_set(mode)
        self._batch.set_images(next_frame=next_frame, **images)
        self._images.polar = new_polar
        # (the init points move between the swap and the warm start, which keeps columns strictly inside the end points only)
        if imode == "follow":
            self._take_inits(self._batch.init_follow(*ipoints))
        elif imode == "set":
            self._batch.set_init(ipoints)
            self._take_inits(ipoints)
        if warm_from is not None:
            self._batch.warm_start_groups(warm_from, warm_every)
        elif warm_every is not None:
            self._batch.warm_start(warm_every)
        if warm_every is not None:
            obs = self._batch.read_obs_all()  # (what reset() sets again)
        else:
            obs = [np.array([])] * self.B if obs is None else list(obs)
        if self.band_rows is not None:
            self.band_r0 = self._batch.band_r0()
            if warm_every is None:  # (a caller's observations are in full-frame rows; the device's own are band rows already)
                obs = [np.asarray(o).reshape(-1, 2).astype(np.int64) - np.array([0, int(r0)], dtype=np.int64)
                       for o, r0 in zip(obs, self.band_r0)]
        self._keep_obs(obs)
        if seeds is not None:
            self.seeds = [int(v) for v in seeds]
            for p, s in zip(self._ps, self.seeds):
                p["seed"] = s
        if warm_every is None:
            self._set_obs()

    def warm_start_from(self, src_of, warm_every):
        """The explicit form of the device's warm start (gpet_batch_warm_start_from), where ``set_frame`` would make it -- after the
        images were swapped: edge e's observations from the last converged fit of edge ``src_of[e]`` (on the same columns), -1 for
        none.  The sets are read back once, so that ``reset()`` restores them.  Returns their sizes."""
        cnt = self._batch.warm_start_from(src_of, warm_every)
        self._keep_obs(self._batch.read_obs_all())
        return cnt

    def run_loop(self, max_iter=1000, chunk=64):
        """The device-resident while-loops of all edges (gpet.py:829-870); returns iterations per edge.

        One library call advances the loop by up to `chunk` iterations and returns as soon as every edge has finished
        (gpet_trace_iterate enqueues the iterations in shrinking groups and checks the `done` flags in between)."""
        b = self._batch
        n_active = self.B
        done_iters = 0
        while n_active > 0:
            n_active = b.iterate(self.seeds, chunk)
            done_iters += chunk
            if done_iters >= max_iter and n_active > 0:
                raise _lib.GpetError(_lib.ERR_ITER_CAP, f"{n_active} edges did not converge in {max_iter} iterations")
        return self._iters()

    def _iters(self):
        return [s.iter for s in self._batch.all_scalars()]

    def final_fits(self, iters):
        fits, self._fit_rounds = device_final_fits(self._batch, self._ps, None, iters)
        return fits

    def finish(self, iters):
        """Converged fits + rounding of the means to pixel indices (gpet.py:874-886) for every edge."""
        fits = self.final_fits(iters)
        out = []
        for p, (mean, std, theta) in zip(self._ps, fits):
            curve = np.concatenate([p["x_grid"][:, None], mean[:, None]], axis=1)
            et = np.rint(curve[:, [1, 0]]).astype(int)
            out.append((et, (mean - 1.96 * std, mean + 1.96 * std)) if self.return_std else et)
        if self.band_rows is not None:  # (band rows -> full-frame rows: one addition of r0)
            for e, r0 in enumerate(self.band_r0):
                if self.return_std:
                    et, (lo, hi) = out[e]
                    out[e] = (et + np.array([int(r0), 0]), (lo + float(r0), hi + float(r0)))
                else:
                    out[e] = out[e] + np.array([int(r0), 0])
        if self._swap:  # (a vertical batch: (row, column) of the transposed image -> of the frame; the interval is frame columns as it is)
            out = [(swap_xy(o[0]), o[1]) if self.return_std else swap_xy(o) for o in out]
        return out

    def _ensemble_rows(self, groups, group_of):
        """The row fields of an ensemble's dicts in full-frame rows: the members of a group share one band."""
        if self.band_rows is None:
            return [swap_record(d, ("trace",)) for d in groups] if self._swap else groups
        out = []
        for g, d in enumerate(groups):
            idx = np.flatnonzero(np.asarray(group_of) == g)
            r0s = {int(self.band_r0[e]) for e in idx}
            if len(r0s) > 1:
                raise ValueError("group %d: its edges lie in different bands (r0 = %s); a group of an ensemble shares one band"
                                 % (g, sorted(r0s)))
            r0 = r0s.pop() if r0s else 0
            d = _shift_rows(d, ("trace",), r0, col=0)
            d = _shift_rows(d, ("median", "q_lo", "q_hi", "min", "max"), float(r0))
            out.append(swap_record(d, ("trace",)) if self._swap else d)
        return out

    def history(self):
        """The iteration history of the current trace (constructor keyword ``history``), one dict per edge as
        ``_lib.decode_history`` returns it; valid after ``run_loop`` or ``__call__``.  ``reset()``, ``set_frame`` and new
        observations empty it.  GpetError (ERR_STATE) when the batch was built without ``history``."""
        hist = self._batch.history()
        if self.band_rows is not None:
            for e, d in enumerate(hist):
                r0 = int(self.band_r0[e])
                d["obs"] = [o + np.array([0, r0], dtype=np.int64) for o in d["obs"]]
                if "optimal_curves" in d:
                    d["optimal_curves"] = [c + np.array([0.0, float(r0)]) for c in d["optimal_curves"]]
                if "mean" in d:
                    d["mean"] = d["mean"] + float(r0)
        if self._swap:
            hist = [swap_record(d, ("obs", "optimal_curves")) for d in hist]
        return hist

    def results(self):
        """What ``finish`` returned for every edge, recomputed on the device from the converged fits it left there
        (gpet_batch_results: the same bits), plus the statistics of each trace: (per-edge results, dict(n_iter, n_obs,
        theta, nlml)).  Valid after ``__call__`` or ``finish``; before a converged fit of the current trace it raises
        GpetError."""
        rec = self._batch.results()
        if self.band_rows is not None:
            rec = dict(rec)
            r0 = np.asarray(self.band_r0, dtype=np.int64)
            tr = np.array(rec["trace"], copy=True)
            tr[:, :, 0] += r0[:, None]
            rec["trace"] = tr
            rec["lower"] = rec["lower"] + r0[:, None].astype(np.float64)
            rec["upper"] = rec["upper"] + r0[:, None].astype(np.float64)
        if self._swap:
            rec = swap_record(rec, ("trace",))
        return results_from_records(rec, self.return_std)

    def default_map_of(self):
        """The map every edge goes on when ``label_maps`` is not told: the raw frame (or image) the edge reads."""
        im = self._images
        if im.edge_frames is not None:
            return list(im.edge_frames)
        if im.mapped:
            return list(im.batch_kwargs["image_of"])
        return [0] * self.B if im.share else list(range(self.B))

    def label_maps(self, map_of=None, extend=False, thickness=False, space=None, out_device_ptrs=None, thick_device_ptr=None):
        """The regions the traced edges bound, as uint8 label maps made on the device from the converged fits where they lie
        (gpet_batch_label_maps / gpet_batch_label_maps_xy; the rules: include/gpet_hip.h "label maps") -- equal to
        ``gpet_utils.label_maps`` of the traces this object returned.  Valid when ``results`` is, raises what it raises; the trace,
        the fits and a kept ensemble are not touched.
        ``map_of``: one map index per edge, -1 for "on no map"; default: the frame (image) the edge reads -- ``image_of``, e with one
        image per edge, 0 with a shared image.  With seed ensembles choose the members yourself, e.g. -1 everywhere but the medoids
        of ``ensemble()``.  An edge the device stopped with an error contributes nothing.
        Returns (n_maps, M, N) uint8 in the frame's shape and orientation -- ``label[f, r, c]`` = edges of map f at or above pixel
        (r, c); a vertical batch: at or left of it; a banded batch: full-frame rows -- and with ``thickness`` also (n_maps, L + 1, N')
        int32, rows (a vertical batch: columns) of label l per column (per row).  ``extend``: columns outside an edge's grid take its
        first / last row instead of not counting.
        ``space`` (a polar batch): ``'polar'`` (default) -- the maps above in polar rows and columns; ``'frame'`` -- (n_maps, Ms, Ns)
        maps on the source frames' shape: the pixels inside the closed outline of every edge of the map (even-odd rule on the
        vertices ``polar_trace_xy`` gives, the seam's second column left out), with the batch's own spec, the centre of map f the
        f-th.  ``space='frame'`` on a batch without ``polar`` raises ValueError.
        ``out_device_ptrs`` (one device address per map; ``thick_device_ptr`` for the thickness): the maps are written there, the
        work is enqueued on the batch's stream, nothing is waited for and None is returned."""
        if space not in (None, "polar", "frame"):
            raise ValueError("space must be None, 'polar' or 'frame', not %r" % (space,))
        if space == "frame" and self.polar is None:
            raise ValueError("space='frame' maps closed contours back to their frames: the batch was not built on polar frames (polar=)")
        if map_of is None:
            map_of = self.default_map_of()
        if space == "frame":
            if extend or thickness:
                raise ValueError("extend and thickness belong to the row maps (space='polar')")
            return self._batch.label_maps_xy(self.polar, self._images.src_shape, map_of, out_device_ptrs=out_device_ptrs)
        return self._batch.label_maps(map_of, extend=extend, transposed=self._images.transposed, thickness=thickness,
                                      out_device_ptrs=out_device_ptrs, thick_device_ptr=thick_device_ptr)

    def final_costs(self):
        """(B,) f64: the scorer's cost of every edge's converged mean curve on its own gradient image -- the reference's
        ``cost_funct(optim_mean_curve)`` (gpet.py:888-890), the algorithm's own figure of merit for a finished trace -- computed on
        the device (gpet_batch_final_costs); +inf for an edge the device stopped with an error.  Valid when ``results`` is, raises
        what it raises; the loop's samples and scores are not touched."""
        return self._batch.final_costs()

    def group_table(self, group_of=None):
        """``group_of`` of ``ensemble`` as the int32 table the library takes; None: one group of all edges, a ValueError if their
        x-grids differ.  Needs no device."""
        if group_of is None:
            grids = {(p["x_st"], p["x_en"]) for p in self._ps}
            if len(grids) > 1:
                raise ValueError("ensemble(group_of=None) makes ONE group of all edges, but their x-grids differ: %s"
                                 % sorted(grids)[:4])
            group_of = np.zeros(self.B, dtype=np.int32)
        return _lib.check_group_table(group_of, self.B)[0]

    def ensemble(self, group_of=None, tol=2):
        """Consensus across the traces of one edge (gpet_batch_ensemble): ``group_of`` one group index per edge, -1 for "in no
        group" (None: one group of all edges); the members of a group are its edges minus those the device stopped with an error.
        Per group and column the order statistics of the members' converged means are taken on the device; returns one dict per
        group: ``trace`` (Lg, 2) int64 yx, the rounded median; ``median``, ``q_lo``, ``q_hi``, ``min``, ``max`` (Lg,);
        ``agree`` (Lg,) members within ``tol`` pixels of the consensus per column; ``members`` (edge indices) with ``off`` (columns
        where the member is more than ``tol`` pixels off the consensus) and ``cost`` (``final_costs``) per member; ``medoid`` (the
        member with the smallest ``off``, then cost, then index -- a real trace, what ``GP_Edge_Tracing`` returns for its seed) and
        ``best_cost`` (the member of smallest cost), both edge indices, -1 in a group without members.  Valid when ``results``
        is, raises what it raises."""
        g = self.group_table(group_of)
        if not float(tol) >= 0.0:
            raise ValueError("tol must be >= 0 pixels, not %r" % (tol,))
        groups, _, _ = self._batch.ensemble(g, tol)
        keys = ("trace", "median", "q_lo", "q_hi", "min", "max", "agree", "members", "off", "cost", "medoid", "best_cost")
        return self._ensemble_rows([{k: d[k] for k in keys} for d in groups], g)

    def __call__(self, max_iter=1000):
        t0 = t.time()
        iters = self.run_loop(max_iter)
        t1 = t.time()
        out = self.finish(iters)
        t2 = t.time()
        self.timings = dict(loop_s=t1 - t0, final_fit_s=t2 - t1, iters=iters)
        return out
