"""The definition of the seed-ensemble reduction (include/gpet_hip.h, "seed ensembles") in numpy: the only oracle the GPU tests
of gpet_batch_ensemble compare against.  Everything is a selection from np.sort(kind="stable") along the member axis, one exact
add and halving (np.median's own arithmetic for an even count), np.rint (round half to even) and integer counts."""
import numpy as np


def group_ref(means, x_st, tol, costs, edges):
    """One group.  ``means``: (n, Lg) f64, the members' converged means in member order; ``costs``: (n,) their final costs;
    ``edges``: (n,) their edge indices (ascending).  Returns the dict of GP_Edge_Tracing_Batch.ensemble for the group."""
    means = np.asarray(means, dtype=np.float64)
    n, Lg = means.shape
    edges = np.asarray(edges, dtype=np.int64)
    costs = np.asarray(costs, dtype=np.float64)
    if n == 0:
        z = np.zeros(Lg)
        return dict(trace=np.zeros((Lg, 2), dtype=np.int64), median=z, q_lo=z, q_hi=z, min=z, max=z, agree=np.zeros(Lg, dtype=np.int32),
                    members=edges, off=np.zeros(0, dtype=np.int32), cost=costs, medoid=-1, best_cost=-1)
    s = np.sort(means, axis=0, kind="stable")
    median = (s[(n - 1) // 2] + s[n // 2]) * 0.5
    assert np.array_equal(median, np.median(means, axis=0))
    c = np.rint(median).astype(np.int64)
    dist = np.abs(np.rint(means) - c[None, :])
    agree = (dist <= tol).sum(axis=0).astype(np.int32)
    off = (dist > tol).sum(axis=1).astype(np.int32)
    order = sorted(range(n), key=lambda m: (int(off[m]), float(costs[m]), int(edges[m])))
    by_cost = sorted(range(n), key=lambda m: (float(costs[m]), int(edges[m])))
    trace = np.stack((c, x_st + np.arange(Lg, dtype=np.int64)), axis=-1)
    return dict(trace=trace, median=median, q_lo=s[(n - 1) // 4], q_hi=s[n - 1 - (n - 1) // 4], min=s[0], max=s[n - 1], agree=agree,
                members=edges, off=off, cost=costs, medoid=int(edges[order[0]]), best_cost=int(edges[by_cost[0]]))


def ensemble_ref(means, lens, x_sts, group_of, tol, costs, excluded=()):
    """``means``: per edge its (Lg_e,) mean; ``lens`` / ``x_sts``: per edge; ``group_of``: per edge, -1 = in no group; ``costs``: per
    edge final cost; ``excluded``: edges whose device status is not OK.  Returns (list of group dicts, off per edge (-1: no
    member), cost per edge (+inf: excluded))."""
    group_of = np.asarray(group_of)
    B = len(group_of)
    G = int(group_of.max()) + 1
    excluded = set(int(e) for e in excluded)
    off_all = np.full(B, -1, dtype=np.int32)
    cost_all = np.array([np.inf if e in excluded else float(costs[e]) for e in range(B)])
    out = []
    for g in range(G):
        assigned = [e for e in range(B) if group_of[e] == g]
        mem = [e for e in assigned if e not in excluded]
        Lg, x0 = int(lens[assigned[0]]), int(x_sts[assigned[0]])
        m = np.stack([np.asarray(means[e])[:Lg] for e in mem]) if mem else np.zeros((0, Lg))
        d = group_ref(m, x0, tol, cost_all[mem] if mem else np.zeros(0), np.array(mem, dtype=np.int64))
        off_all[mem] = d["off"]
        out.append(d)
    return out, off_all, cost_all


KEYS_EXACT = ("trace", "median", "q_lo", "q_hi", "min", "max", "agree", "members", "off", "cost")


def assert_group_equal(got, want, what=""):
    for k in KEYS_EXACT:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (what, k, g, w)
    assert (int(got["medoid"]), int(got["best_cost"])) == (int(want["medoid"]), int(want["best_cost"])), (what, got["medoid"], want["medoid"],
                                                                                                         got["best_cost"], want["best_cost"])
