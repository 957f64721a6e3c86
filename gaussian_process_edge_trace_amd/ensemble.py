"""Seed ensembles: one edge traced with many seeds in one batch, and what to do with the traces.

The tracer is stochastic, and on some images bistable: a seed lands on the edge or on a neighbouring one.  The reference cannot
afford many seeds per edge; a batch traces hundreds in less time than the reference takes for one.  ``trace_ensemble`` runs E inits x K seeds as one batch on
a shared image (edges init-major: edge ``i * K + s`` is init i with seed s; group i = the K traces of init i) and reduces every
group on the device (``GP_Edge_Tracing_Batch.ensemble``): per-column order statistics of the converged means, the consensus
trace, how many members agree with it per column, every member's distance from it and final cost -- and the MEDOID, the member
closest to the consensus, whose own result is returned as ``result``: a trace ``GP_Edge_Tracing(seed=...)`` returns bit for bit,
not a synthetic one.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .gpet import GP_Edge_Tracing_Batch
from .sequence import _inits_of


def ensemble_table(n_inits, seeds):
    """The batch layout of ``trace_ensemble``, init-major: (group_of (E * K,) int32, edge seeds (E * K,), init index per edge).
    ValueError for no seeds, more than ``_lib.ENSEMBLE_MAX`` per init, or no init."""
    seeds = [int(s) for s in np.asarray(seeds).reshape(-1)]
    E, K = int(n_inits), len(seeds)
    if E < 1:
        raise ValueError("trace_ensemble needs at least one init")
    if K < 1:
        raise ValueError("trace_ensemble needs at least one seed")
    if K > _lib.ENSEMBLE_MAX:
        raise ValueError("%d seeds per init: a group holds at most %d members" % (K, _lib.ENSEMBLE_MAX))
    group_of = np.repeat(np.arange(E, dtype=np.int32), K)
    return group_of, seeds * E, group_of.copy()


def trace_ensemble(init, grad_img, seeds, tol=2, **ctor_kwargs):
    """Traces ``init`` on ``grad_img`` once per seed of ``seeds``, all in one batch, and reduces the traces on the device.

    ``init``: one (n_init, 2) xy array, or a list of E of them as in ``trace_sequence`` (the E edges of the image; they may span
    different columns); ``grad_img``: the (M, N) gradient image all of them share -- or None with the raw-frame keywords of
    ``GP_Edge_Tracing_Batch`` (``raw_imgs=frame, grad_kernel=K``, ``denoise=...``); ``seeds``: the K seeds every init is traced
    with; ``tol``: pixels within which a member agrees with the consensus.  Remaining keyword arguments are the batch
    constructor's (the reference's, common to all edges).

    Returns, per init, the dict of ``GP_Edge_Tracing_Batch.ensemble`` (``trace``, ``median``, ``q_lo``, ``q_hi``, ``min``, ``max``,
    ``agree``, ``members``, ``off``, ``cost``, ``medoid``, ``best_cost``; member indices are batch edge indices, init-major) plus
    ``seeds`` (the members' seeds), ``medoid_seed`` and ``result``: the medoid member's own result as ``finish`` returns it (the
    trace, or (trace, credible interval) with ``return_std``) -- None if the device stopped every member.  One dict for one
    init, a list for a list of inits.  ``orientation='vertical'`` (a batch keyword): ``grad_img`` / the raw frame as it lies, ``init``
    and every trace of the dict in the frame's coordinates, as the batch returns them.  ``polar=dict(...)`` (a batch keyword, with
    ``raw_imgs``): a closed contour -- ``init`` (``gpet_utils.closed_init``) and every trace of the dict in polar rows and columns."""
    inits, multi = _inits_of(init)
    if not float(tol) >= 0.0:
        raise ValueError("tol must be >= 0 pixels, not %r" % (tol,))
    for k in ("seeds", "image_of", "obs"):
        if k in ctor_kwargs:
            raise ValueError("trace_ensemble lays the batch out itself: %r is not accepted" % k)
    group_of, edge_seeds, init_of = ensemble_table(len(inits), seeds)
    if grad_img is not None and np.ndim(grad_img) != 2:
        raise ValueError("trace_ensemble takes ONE (M, N) gradient image shared by every trace")
    if "kernel_of" in ctor_kwargs and ctor_kwargs["kernel_of"] is not None:  # (one kernel index per init -> per edge)
        ko = [int(v) for v in np.asarray(ctor_kwargs["kernel_of"]).reshape(-1)]
        if len(ko) != len(inits):
            raise ValueError("kernel_of has %d entries for %d inits" % (len(ko), len(inits)))
        ctor_kwargs = dict(ctor_kwargs, kernel_of=[ko[i] for i in init_of])
    batch = GP_Edge_Tracing_Batch([inits[i] for i in init_of], grad_img, edge_seeds, **ctor_kwargs)
    results = batch()
    out = []
    for d in batch.ensemble(group_of, tol):
        d = dict(d)
        d["seeds"] = [edge_seeds[e] for e in d["members"]]
        d["medoid_seed"] = edge_seeds[d["medoid"]] if d["medoid"] >= 0 else None
        d["result"] = results[d["medoid"]] if d["medoid"] >= 0 else None
        out.append(d)
    return out if multi else out[0]
