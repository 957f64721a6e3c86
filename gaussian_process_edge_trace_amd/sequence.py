"""Image-sequence tracing (BASELINE config 5): one edge, or the few edges of every frame, followed through the frames of a
sequence.

The reference traces one image per ``GP_Edge_Tracing`` object; a sequence is chained by the user through the
constructor's ``obs`` argument (gp_edge_tracing/gpet.py:57-61, 100, 820): pixels of the previous frame's trace are the
warm-start observations of the next.  With ``algo_thresh`` or more of them the while-loop would not run at all
(gpet.py:829), so the warm start takes every ``warm_every``-th pixel of the previous trace and must stay below it.

A chain is serial by construction (frame t needs trace t-1).  Parallelism comes from independent CHAINS: a sequence
of T frames is cut into C chains of consecutive frames, the first frame of every chain starting cold;
step s of all chains is one batch of C edges on the GPU (``GP_Edge_Tracing_Batch``, one image per edge), and chains
spread over the GPUs of a node like independent edges do (``sharding.trace_sequence_sharded``).

A frame often carries several edges (the layers of a retina, the two walls of a vessel): with E inits step s is one batch of
C x E edges, chain-major, on C images -- the batch's image map says which edge reads which (``image_of``), so a frame is
uploaded and prepared once.  From one step to the next the traces stay on the device: the warm start of every edge is made
there from its own converged fit (``set_frame(..., warm_every=k)``, the rule of ``warm_start_obs`` below).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import split_kernels
from .gpet import (GP_Edge_Tracing_Batch, check_kernel_of, refuse_polar_vertical, resolve_init_follow, resolve_orientation, resolve_params,
                   swap_record, swap_xy, vertical_inits)


def chain_slices(n_frames, n_chains):
    """[lo, hi) frame ranges of ``n_chains`` chains of consecutive frames (lengths differ by at most one)."""
    n_chains = max(1, min(int(n_chains), int(n_frames)))
    base, rem = divmod(int(n_frames), n_chains)
    out, lo = [], 0
    for c in range(n_chains):
        hi = lo + base + (1 if c < rem else 0)
        out.append((lo, hi))
        lo = hi
    return out


def warm_start_obs(edge_trace, x_st, x_en, warm_every, algo_thresh, M=None):
    """Observations (xy int64) for the next frame: every ``warm_every``-th pixel of ``edge_trace`` ((N, 2) yx, as
    ``GP_Edge_Tracing.__call__`` returns it) strictly inside the end points.  Fewer than ``algo_thresh`` of them, or
    the next frame's loop would be skipped (gpet.py:829): a too dense choice is thinned by doubling the stride."""
    et = np.asarray(edge_trace)
    step = max(1, int(warm_every))
    while True:
        sel = et[step:-1:step] if step < et.shape[0] else et[:0]
        sel = sel[(sel[:, 1] > x_st) & (sel[:, 1] < x_en)]
        if M is not None:  # (a rounded posterior mean may leave the image; such a pixel cannot be an observation)
            sel = sel[(sel[:, 0] >= 0) & (sel[:, 0] <= M - 1)]
        if sel.shape[0] < algo_thresh or sel.shape[0] == 0:
            return sel[:, [1, 0]].astype(np.int64)
        step *= 2


def _inits_of(init):
    """(list of E (n_init, 2) arrays, multi): a 2-D array is ONE init (results as for one edge); a list / tuple or a 3-D array
    holds E of them, which may span different columns."""
    if isinstance(init, (list, tuple)):
        inits = [np.asarray(i) for i in init]
        if inits and inits[0].ndim == 1:  # (a nested list of points: one init)
            return [np.asarray(init)], False
        return inits, True
    a = np.asarray(init)
    if a.ndim == 3:
        return [a[k] for k in range(a.shape[0])], True
    return [a], False


def resolve_labels(labels):
    """``labels`` as ``SequenceTracer`` accepts it, decided without a device: None / False (off), True, or a dict with any of
    ``extend``, ``thickness``, ``space`` -> None or dict(extend=, thickness=, space=).  ValueError for anything else."""
    if labels is None or labels is False:
        return None
    out = dict(extend=False, thickness=False, space=None)
    if labels is True:
        return out
    if not isinstance(labels, dict) or not set(labels) <= set(out):
        raise ValueError("labels must be True or dict(extend=, thickness=, space=), not %r" % (labels,))
    out.update(labels)
    if out["space"] not in (None, "polar", "frame"):
        raise ValueError("labels: space must be None, 'polar' or 'frame', not %r" % (out["space"],))
    if out["space"] == "frame" and (out["extend"] or out["thickness"]):
        raise ValueError("labels: extend and thickness belong to the row maps (space='polar')")
    return out


class SequenceTracer(object):
    """Traces ``init`` through ``frames`` (T gradient images of one shape) in ``n_chains`` chains on one GPU.

    ``frames``: sequence of (M, N) gradient images -- or, with ``grad_kernel=K``, of raw frames (uint8, uint16, float32,
    float64 as they are, see ``GP_Edge_Tracing_Batch``) whose gradient images ``comp_grad_img(frame, K)`` are made on the
    device, every step's frames in one pass, at construction and through ``set_frame`` alike -- after
    ``gpet_utils.denoise`` of every frame, on the device in the same pass, with ``denoise=(technique, kwargs)``; ``seeds``: one seed per frame (default: ``seed`` for all, like a
    user re-creating ``GP_Edge_Tracing(..., seed=seed)`` per frame).  Remaining keyword arguments are the reference
    constructor's (gpet.py:22-35).  ``__call__`` returns the list of T results in frame order, each what
    ``GP_Edge_Tracing.__call__`` returns for that frame (trace, or (trace, credible interval) with ``return_std``).

    ``init``: one (n_init, 2) array -- or a list (or 3-D array) of E of them, the E edges of every frame, which may span
    different columns.  Then every entry of the result is a list of E results, ``iterations[t]`` a list of E counts, and
    edge k's results are what ``SequenceTracer(frames, init[k], ...)`` gives: the E edges of a frame share its seed.

    ``grad_kernel=[K_0 .. K_{E-1}]``: one kernel per init, for edges of opposite polarity on the same raw frames (the two walls
    of a vessel) -- or fewer kernels plus ``kernel_of`` with E indices into them.  Every frame is uploaded, denoised and staged
    on the device once, and edge k's results are what ``SequenceTracer(frames, init[k], grad_kernel=K[kernel_of[k]], ...)``
    gives, bit for bit.

    ``ensemble_seeds=[s_0 .. s_{K-1}]``: every frame is traced with K seeds per init -- a step of C chains and E inits is one batch
    of C x E x K edges (``step_tables``), member j of every frame with seed ``s_j`` (``seed`` / ``seeds`` are then refused) -- and
    ALL K members of the next frame start from one source of their group, so a seed that strayed onto a neighbouring edge does
    not hand its trace on: ``warm_from='medoid'`` (default; a real trace), ``'best_cost'`` or ``'consensus'``.  The group is
    reduced and the warm start made on the device (``set_frame(..., warm_from=)``).  Every result is then the dict
    ``trace_ensemble`` returns for that frame and init -- the reduction's arrays (``ensemble_tol`` = its ``tol``) plus ``seeds``,
    ``medoid_seed`` and ``result``, the medoid member's own result -- and ``iterations[t]`` holds the K counts.

    ``band_rows=H``: tracking bands (``GP_Edge_Tracing_Batch``) -- every edge traces inside H rows of its frame.  The first frame of
    every chain is placed from the init rows, every later one follows the trace its warm start comes from
    (``set_frame(..., band='follow')``, on the device); with ``ensemble_seeds`` the K members of a group share the band placed from
    the group's source.  Results are in full-frame rows; presets of ``kernel_options`` that depend on the image height see H.

    ``init_follow=dict(window=w, cols=a)``: endpoint tracking (``GP_Edge_Tracing_Batch``) -- on every frame the init points move onto
    the edge of that frame, on the device, starting from where the frame before it in its chain left them (a chain's first frame:
    from ``init``).  ``inits[t]`` holds the points frame t was traced with -- one (n_init, 2) int64 xy array in the order of ``init``,
    or a list of E of them -- without ``init_follow`` the given ones.  The K members of an ensemble share init and image, hence the
    result; with ``band_rows`` the bands are placed as ever, against the points of the frame before, and the search stays inside.

    ``orientation='vertical'``: the edges run down the frames (``GP_Edge_Tracing_Batch``) -- the sequence is, bit for bit, the
    horizontal one on the transposed gradient images with the coordinates of ``init`` swapped, and every result, ensemble dict and
    ``inits[t]`` comes back in the frame's coordinates.  The frames -- raw or gradient images -- are given as they lie; the transposes
    are made on the device.  ``warm_start_obs`` is applied to the traces of the transposed images.

    ``polar=dict(centre=(cx, cy) | (T, 2) array, n_r=, n_theta=, ...)`` with ``grad_kernel``: closed contours (``GP_Edge_Tracing_Batch``)
    -- every frame is unwrapped to (radius x angle) on the device, around its own centre where ``centre`` has one per frame, and the
    sequence is, bit for bit, the one on ``unwrap_polar_imgs(frames, **polar)``; ``init`` (``closed_init(row, polar)``), results and
    everything else are in polar rows and columns.  ``polar`` (attribute) is the resolved spec.  Not with ``orientation='vertical'``.

    ``labels=True`` or ``dict(extend=, thickness=, space=)``: after every step's trace the label map of every frame -- all E edges of
    the frame on one map, ``GP_Edge_Tracing_Batch.label_maps`` -- is made on the device from that step's fits, before the next
    ``set_frame``: ``labels[t]`` is frame t's (M, N) uint8 map (``space='frame'`` with ``polar``: on the source frame's shape),
    ``thickness[t]`` its (E + 1, N) int32 profiles when asked for.  Not with ``ensemble_seeds`` (ValueError): the ensemble of a step
    is known only after the swap, when the fits' results are no longer valid -- labels from an ensemble's consensus are out of scope."""

    _UNSET = object()

    def __init__(self, frames, init, n_chains=1, warm_every=None, seed=_UNSET, seeds=None, *, device=0, _ctx=None, grad_kernel=None,
                 denoise=None, kernel_of=None, ensemble_seeds=None, ensemble_tol=2, warm_from='medoid', band_rows=None, init_follow=None,
                 orientation="horizontal", polar=None, labels=None, **kw):
        self._labels = resolve_labels(labels)
        if self._labels is not None and ensemble_seeds is not None:
            raise ValueError("labels and ensemble_seeds are alternatives: a step's ensemble is known only after the swap to the next "
                             "frame, when the fits the maps are made from are no longer valid")
        if self._labels is not None and self._labels["space"] == "frame" and polar is None:
            raise ValueError("labels: space='frame' maps closed contours back to their frames: it needs polar")
        if ensemble_seeds is not None:
            if seed is not SequenceTracer._UNSET or seeds is not None:
                raise ValueError("ensemble_seeds are the seeds of every frame's members: seed / seeds are not accepted with them")
            ensemble_seeds = [int(v) for v in np.asarray(ensemble_seeds).reshape(-1)]
            if not ensemble_seeds:
                raise ValueError("ensemble_seeds is empty: an ensemble needs at least one seed")
            if len(ensemble_seeds) > _lib.ENSEMBLE_MAX:
                raise ValueError("%d ensemble_seeds: a group holds at most %d members" % (len(ensemble_seeds), _lib.ENSEMBLE_MAX))
            if not float(ensemble_tol) >= 0.0:
                raise ValueError("ensemble_tol must be >= 0 pixels, not %r" % (ensemble_tol,))
            _lib.warm_from(warm_from)
        if seed is SequenceTracer._UNSET:
            seed = 42
        self.ensemble_seeds, self.ensemble_tol, self.warm_from = ensemble_seeds, ensemble_tol, warm_from
        self.K = 1 if ensemble_seeds is None else len(ensemble_seeds)
        self.frames = frames
        self.T = len(frames)
        self.orientation = orientation
        self._tr = resolve_orientation(orientation)
        refuse_polar_vertical(polar, self._tr)
        self._inits, self.multi = _inits_of(init)
        if not self._inits:
            raise ValueError("no init")
        if self._tr:  # (from here on everything but what is handed back is in the coordinates of the transposed images)
            self._inits = vertical_inits(self._inits)
        self.E = len(self._inits)
        self.init = self._inits[0] if not self.multi else self._inits
        resolve_init_follow(init_follow)  # (refused here, before a frame is looked at)
        self.init_follow = init_follow
        self.inits = [None] * self.T  # the init points every frame was traced with
        self.labels = [None] * self.T     # labels=: the label map of every frame
        self.thickness = [None] * self.T  # labels=dict(thickness=True): its thickness profiles
        self._cur = {}  # (chain, edge of the frame) -> the init points the chain's last frame left, in the order of `init`
        self.kw = dict(kw)
        self.kw.pop("obs", None)
        self.grad_kernel = grad_kernel
        if denoise is not None and grad_kernel is None:
            raise ValueError("denoise needs raw frames, i.e. grad_kernel")
        self.kernel_of = None
        if kernel_of is not None and grad_kernel is None:
            raise ValueError("kernel_of picks the gradient kernel of raw frames, i.e. needs grad_kernel")
        if grad_kernel is not None:
            kernels, multi = split_kernels(grad_kernel)
            if multi or kernel_of is not None:
                if kernel_of is None:
                    if len(kernels) != self.E:
                        raise ValueError("%d kernels in grad_kernel for %d inits: pass one per init, or kernel_of with one index "
                                         "per init" % (len(kernels), self.E))
                    kernel_of = range(self.E)
                kernel_of = [int(v) for v in kernel_of]
                if len(kernel_of) != self.E:
                    raise ValueError("kernel_of has %d entries for %d inits" % (len(kernel_of), self.E))
                check_kernel_of(kernel_of, len(kernels))
                used = sorted(set(kernel_of))  # (kernels no init uses are dropped: the library refuses a kernel no slot reads)
                self.grad_kernel = [kernels[k] for k in used]
                self.kernel_of = [used.index(k) for k in kernel_of]
        self.denoise = denoise
        self.chains = chain_slices(self.T, n_chains)
        self.seeds = [int(seed)] * self.T if seeds is None else [int(v) for v in seeds]
        ctor = {k: v for k, v in self.kw.items() if k in ("kernel_options", "noise_y", "N_samples", "score_thresh", "delta_x",
                                                           "keep_ratio", "pixel_thresh", "return_std", "fix_endpoints")}
        self.band_rows = None if band_rows is None else int(band_rows)
        shape = np.asarray(frames[0]).shape
        # (closed contours: every step's batch unwraps its frames by this spec, around the centres of the step's frames; inits, traces
        #  and everything else are in polar rows and columns)
        self.polar = None
        if polar is not None:
            if grad_kernel is None:
                raise ValueError("polar needs raw frames, i.e. grad_kernel")
            self.polar = _lib.polar_spec(polar).resolved(_lib.polar_default_pad(split_kernels(grad_kernel)[0]))
            if self.polar.centre.shape[0] not in (1, self.T):
                raise ValueError("polar: %d centres for %d frames: one for all frames or one per frame" % (self.polar.centre.shape[0], self.T))
            shape = self.polar.shape
        if self._tr:
            shape = (shape[1], shape[0])
        self._frame_M = int(shape[0])
        if self.band_rows is not None:
            shape = (self.band_rows, shape[1])  # (the parameters are those of the (H, N) crop)
        self._ps = [resolve_params(i, shape, **ctor) for i in self._inits]
        self._p = self._ps[0]
        self.warm_every = int(warm_every) if warm_every else 2 * self._p["delta_x"]
        self.device, self._ctx = device, _ctx
        self.iterations = [0] * self.T
        self._tracer = None

    def _init_of(self, c, k):
        """The init points the next frame of chain ``c`` starts from for edge ``k``: where the chain's last frame left them, else the given ones."""
        return self._cur.get((c, k), self._inits[k])

    def _file_inits(self, active):
        """The step's init points as its batch holds them, filed per frame and carried per (chain, edge) in the order of ``init``."""
        table = self._tracer.inits
        for ci, (c, f) in enumerate(active):
            got = []
            for k in range(self.E):
                mine = np.array(self._inits[k], dtype=np.int64)
                mine[np.argsort(np.asarray(self._inits[k])[:, 0]), 1] = table[(ci * self.E + k) * self.K][:, 1]  # (the batch sorts by x, as resolve_params does)
                if self.init_follow is not None:
                    self._cur[c, k] = mine
                got.append(mine)
            if self._tr:
                got = swap_xy(got)
            self.inits[f] = got if self.multi else got[0]

    def _file_labels(self, active):
        """The label maps of the step just traced, one per frame (map = the chain's frame), filed per frame."""
        E, K = self.E, self.K
        opts = self._labels
        got = self._tracer.label_maps([ci for ci in range(len(active)) for _ in range(E * K)], extend=opts["extend"],
                                      thickness=opts["thickness"], space=opts["space"])
        maps, thick = got if opts["thickness"] else (got, None)
        for ci, (_, f) in enumerate(active):
            self.labels[f] = maps[ci]
            if thick is not None:
                self.thickness[f] = thick[ci]

    def _result_out(self, res):
        """A result of the step's batch as it is handed back: on a vertical sequence with the trace in the frame's coordinates."""
        if not self._tr or res is None:
            return res
        return (swap_xy(res[0]), res[1]) if self._tracer.return_std else swap_xy(res)

    def _place(self, p, trace, init=None):
        """The first row of an edge's band from ``trace`` ((Lg, 2) yx, full-frame rows; None: from the init rows), ``_lib.band_place``;
        ``init``: the edge's current init points (default: the given ones)."""
        rows = p["init"][:, 1] if init is None else np.asarray(init)[:, 1]
        i_lo, i_hi = int(rows.min()), int(rows.max())
        t = rows if trace is None else np.asarray(trace)[:, 0]
        t = t[(t >= 0) & (t <= self._frame_M - 1)]
        if t.size == 0:
            t = rows
        return _lib.band_place(self._frame_M, self.band_rows, int(t.min()), int(t.max()), i_lo, i_hi)

    def _polar_of(self, active):
        """The polar spec of a step's batch: the sequence's own, around the centres of the step's frames where there is one per frame."""
        if self.polar is None or self.polar.centre.shape[0] == 1:
            return self.polar
        return self.polar.with_centre(self.polar.centre[[f for _, f in active]])

    def _frames_of_step(self, s):
        return [lo + s for lo, hi in self.chains if lo + s < hi]

    def step_tables(self, active):
        """The layout of one step's batch, from the frames alone (no device).  ``active``: the step's (chain, frame) pairs.  A dict:
        ``inits`` and ``seeds`` per edge, ``image_of`` and ``kernel_of`` (None where the batch does without), ``group_of`` (None
        without ``ensemble_seeds``).  Edges are chain-major, then init-major, then member-minor: edge ``(ci * E + k) * K + j`` is
        init k of the ci-th active chain's frame with seed ``ensemble_seeds[j]``, group ``ci * E + k`` its K members.  Without
        ``ensemble_seeds`` K is 1 and the E edges of a frame share the frame's seed."""
        E, K = self.E, self.K
        ens = self.ensemble_seeds is not None
        if ens:
            seeds = [sd for _ in active for _ in range(E) for sd in self.ensemble_seeds]
        else:
            seeds = [self.seeds[f] for _, f in active for _ in range(E)]  # (chain-major: the E edges of a frame are adjacent)
        # (several edges per frame: one image per chain, read by its edges; one edge per frame is a batch with one image per edge,
        # as ever)
        image_of = ([ci for ci in range(len(active)) for _ in range(E * K)]
                    if E > 1 or ens or self.kernel_of is not None else None)
        # (chain-major, like the inits: C frames, C x distinct kernels image slots)
        kernel_of = None if self.kernel_of is None else [k for _ in active for k in self.kernel_of for _ in range(K)]
        group_of = np.repeat(np.arange(len(active) * E, dtype=np.int32), K) if ens else None
        return dict(inits=[self._init_of(c, k) for c, _ in active for k in range(E) for _ in range(K)], seeds=seeds, image_of=image_of,
                    kernel_of=kernel_of, group_of=group_of)

    def _source_trace(self, d, res):
        """The trace the members of the next frame start from, on the host (the rebuilt batch): the medoid's or the best-cost
        member's own, or the consensus; None for a group without members."""
        if d["medoid"] < 0:
            return None
        if self.warm_from in ("consensus", _lib.WARM_CONSENSUS):
            return d["trace"]
        r = res[d["medoid"] if self.warm_from in ("medoid", _lib.WARM_MEDOID) else d["best_cost"]]
        return r[0] if self._tracer.return_std else r

    def _close_step(self, pending, ens, results, prev):
        """Files the results of the step traced last: ``pending`` = (active, results per edge, iterations per edge, group table), ``ens`` the
        ensemble of its groups (None without ``ensemble_seeds``)."""
        active, out, iters, _ = pending
        E, K = self.E, self.K
        for ci, (c, f) in enumerate(active):
            if ens is None:
                res = out[ci * E:(ci + 1) * E]
                results[f] = [self._result_out(r) for r in res] if self.multi else self._result_out(res[0])
                self.iterations[f] = list(iters[ci * E:(ci + 1) * E]) if self.multi else iters[ci * E]
                for k in range(E):
                    prev[c, k] = res[k][0] if self._tracer.return_std else res[k]
                continue
            dicts, its = [], []
            for k in range(E):
                g = ci * E + k
                d = dict(ens[g])
                d["seeds"] = [self.ensemble_seeds[e - g * K] for e in d["members"]]
                d["medoid_seed"] = self.ensemble_seeds[d["medoid"] - g * K] if d["medoid"] >= 0 else None
                d["result"] = self._result_out(out[d["medoid"]] if d["medoid"] >= 0 else None)
                prev[c, k] = self._source_trace(d, out)
                dicts.append(swap_record(d, ("trace",)) if self._tr else d)
                its.append(list(iters[g * K:(g + 1) * K]))
            results[f] = dicts if self.multi else dicts[0]
            self.iterations[f] = its if self.multi else its[0]

    def __call__(self, max_iter=1000):
        results = [None] * self.T
        prev = {}  # (chain index, edge of the frame) -> the trace the next frame starts from
        n_steps = max(hi - lo for lo, hi in self.chains)
        E, K = self.E, self.K
        ens = self.ensemble_seeds is not None
        pending = None  # the step traced last, filed once its ensemble is there: set_frame reduces it on its way to the next frame
        for s in range(n_steps):
            active = [(c, lo + s) for c, (lo, hi) in enumerate(self.chains) if lo + s < hi]
            imgs = [np.asarray(self.frames[f]) for _, f in active]
            tab = self.step_tables(active)
            seeds = tab["seeds"]
            if self._tracer is None or len(active) * E * K != self._tracer.B:
                # (first step, or the shorter chains have run out: a smaller batch from here on; the old batch's arena,
                # streams and events are released now, not whenever the garbage collector gets to them.  The new batch's
                # warm start comes from the traces on the host: the converged fits went with the old batch)
                if pending is not None:
                    self._close_step(pending, self._tracer.ensemble(pending[3], self.ensemble_tol) if ens else None, results, prev)
                    pending = None
                obs, r0s = [], []
                for c, f in active:
                    for k, p in enumerate(self._ps):
                        cold = s == 0 or prev[c, k] is None
                        if self.band_rows is not None:  # (placed from the trace the warm start comes from, else from the inits)
                            r0 = self._place(p, None if cold else prev[c, k], self._init_of(c, k))
                            r0s.extend([r0] * K)
                            shift = np.array([r0, 0])
                        o = (np.zeros((0, 2), dtype=np.int64) if cold else
                             warm_start_obs(prev[c, k] if self.band_rows is None else prev[c, k] - shift, p["x_st"], p["x_en"],
                                            self.warm_every, p["algo_thresh"], p["M"]))
                        if self.band_rows is not None:
                            o = o + shift[[1, 0]]  # (the constructor takes observations in full-frame rows)
                        obs.extend([o] * K)
                if self._tracer is not None:
                    self._tracer._batch.close()
                images = dict(grad_imgs=imgs) if self.grad_kernel is None else dict(grad_imgs=None, raw_imgs=imgs,
                                                                                     grad_kernel=self.grad_kernel,
                                                                                     denoise=self.denoise)
                if tab["kernel_of"] is not None:
                    images["kernel_of"] = tab["kernel_of"]
                if self.band_rows is not None:
                    images.update(band_rows=self.band_rows, band_r0=r0s)
                if self.init_follow is not None:  # (remembered by the batch: its set_frame then follows by default)
                    images["init_follow"] = self.init_follow
                if self.polar is not None:
                    images["polar"] = self._polar_of(active)
                self._tracer = GP_Edge_Tracing_Batch(tab["inits"], seeds=seeds, obs=obs, device=self.device, _ctx=self._ctx,
                                                     image_of=tab["image_of"], orientation=self.orientation, _batch_coords=self._tr,
                                                     **images, **self.kw)
                if self._ctx is None:
                    self._ctx = self._tracer._ctx
            else:
                warm = dict(warm_every=self.warm_every)
                if ens:  # (the ensemble of the step before is reduced and kept on the device, then warm-starts every member)
                    warm.update(warm_from=self.warm_from, group_of=tab["group_of"], tol=self.ensemble_tol)
                if self.polar is not None:
                    warm["polar"] = self._polar_of(active)
                if self.grad_kernel is None:
                    self._tracer.set_frame(imgs, None, seeds, **warm)
                else:
                    self._tracer.set_frame(None, None, seeds, raw_imgs=imgs, **warm)
                if ens:
                    self._close_step(pending, self._tracer.last_ensemble, results, prev)
                    pending = None
            self._file_inits(active)
            out = self._tracer(max_iter)
            if self._labels is not None:  # (from this step's fits, before the next set_frame invalidates them)
                self._file_labels(active)
            pending = (active, out, list(self._tracer.timings["iters"]), tab["group_of"])
            if not ens:
                self._close_step(pending, None, results, prev)
                pending = None
        if pending is not None:
            self._close_step(pending, self._tracer.ensemble(pending[3], self.ensemble_tol), results, prev)
        return results


def trace_sequence(frames, init, n_chains=1, warm_every=None, **kw):
    """Convenience wrapper: ``SequenceTracer(frames, init, n_chains, warm_every, **kw)()``."""
    return SequenceTracer(frames, init, n_chains, warm_every, **kw)()
