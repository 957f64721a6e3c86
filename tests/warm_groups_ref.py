"""The definition of the group warm start (include/gpet_hip.h, "seed ensembles in sequences") in numpy, built on the definition of the
reduction (tests/ensemble_ref.py) and on the host's warm-start rule (sequence.warm_start_obs): the only oracle the GPU tests of
gpet_batch_warm_start_groups / gpet_batch_warm_start_from compare against."""
import numpy as np

from gaussian_process_edge_trace_amd.sequence import warm_start_obs
from tests.ensemble_ref import ensemble_ref

SRC_NONE, SRC_CONSENSUS = -1, -2
FROM = ("medoid", "best_cost", "consensus")


def trace_of_mean(mean, x_st):
    """The (Lg, 2) int64 yx trace of a converged mean, rounded as finish / gpet_batch_results round it (NaN: INT64_MIN)."""
    mean = np.asarray(mean, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        y = np.rint(mean).astype(np.int64)
    y[~np.isfinite(mean)] = np.iinfo(np.int64).min
    return np.stack((y, x_st + np.arange(mean.shape[0], dtype=np.int64)), axis=-1)


def sources_ref(group_of, groups, frm):
    """src per edge: the edge itself outside any group; -1 for the edges of a group without members; else the group's medoid, its
    member of smallest final cost, or -2 for the consensus.  Assigned edges that are no members get their group's source too."""
    assert frm in FROM
    src = np.empty(len(group_of), dtype=np.int32)
    for e, g in enumerate(np.asarray(group_of).tolist()):
        if g < 0:
            src[e] = e
        elif len(groups[g]["members"]) == 0:
            src[e] = SRC_NONE
        else:
            src[e] = {"medoid": groups[g]["medoid"], "best_cost": groups[g]["best_cost"], "consensus": SRC_CONSENSUS}[frm]
    return src


def obs_from_sources(means, ps, src, group_of, groups, warm_every):
    """Observation set (xy int64) of every edge from its source, with the DESTINATION's bounds (ps[e]: x_st, x_en, algo_thresh, M)."""
    out = []
    for e, p in enumerate(ps):
        s = int(src[e])
        if s == SRC_NONE:
            out.append(np.zeros((0, 2), dtype=np.int64))
            continue
        Lg = p["x_en"] - p["x_st"] + 1
        trace = groups[group_of[e]]["trace"] if s == SRC_CONSENSUS else trace_of_mean(np.asarray(means[s])[:Lg], p["x_st"])
        assert trace.shape == (Lg, 2)
        out.append(warm_start_obs(trace, p["x_st"], p["x_en"], warm_every, p["algo_thresh"], p["M"]))
    return out


def warm_groups_ref(means, ps, group_of, tol, costs, excluded, frm, warm_every):
    """(observation sets per edge, src per edge, the groups of ensemble_ref).  ``means``: per edge its converged mean; ``ps``: per
    edge dict(x_st, x_en, algo_thresh, M); ``costs``: final costs on the images the edges read when the ensemble is kept;
    ``excluded``: edges whose device status is not OK."""
    lens = [p["x_en"] - p["x_st"] + 1 for p in ps]
    groups, _, _ = ensemble_ref(means, lens, [p["x_st"] for p in ps], group_of, tol, costs, excluded)
    src = sources_ref(group_of, groups, frm)
    return obs_from_sources(means, ps, src, np.asarray(group_of), groups, warm_every), src, groups


def first_pass_count(trace, p, warm_every):
    """Pixels the rule keeps at its first stride: ``algo_thresh`` or more (and not zero) means the stride is doubled."""
    step = max(1, int(warm_every))
    sel = trace[step:-1:step] if step < trace.shape[0] else trace[:0]
    sel = sel[(sel[:, 1] > p["x_st"]) & (sel[:, 1] < p["x_en"]) & (sel[:, 0] >= 0) & (sel[:, 0] <= p["M"] - 1)]
    return sel.shape[0]
