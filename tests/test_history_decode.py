"""decode_history (plain numpy, no device) on a byte buffer written by hand in the documented layout (include/gpet_hip.h,
"iteration history"): two edges of different length in one batch-wide padding, one of them past its iter_cap."""
import numpy as np
import pytest

from gaussian_process_edge_trace_amd import _lib


def _build(level):
    """Batch-wide: iter_cap 3, obs_cap 5, len_cap 7.  Edge 0: Lg 7, own obs_cap 5, x_st 10, 3 records kept and 2 dropped (it ran 5
    iterations); edge 1: Lg 4, own obs_cap 3, x_st 2, 2 records."""
    P = _lib.history_plan(level, 3, 5, 7)
    raw = bytearray(2 * P.edge_bytes)
    spec = [dict(Lg=7, n_rec=3, dropped=2, n_iter=5), dict(Lg=4, n_rec=2, dropped=0, n_iter=2)]
    for e, sp in enumerate(spec):
        base = e * P.edge_bytes
        eh = _lib.GpetHistoryEdgeHead.from_buffer(raw, base)
        eh.n_rec, eh.dropped, eh.n_iter, eh.edge_len = sp["n_rec"], sp["dropped"], sp["n_iter"], sp["Lg"]
        for i in range(sp["n_rec"]):
            rb = base + P.off_records + i * P.record_bytes
            h = _lib.GpetHistoryHead.from_buffer(raw, rb)
            h.iter, h.n_obs, h.best_idx, h.rank, h.n_removed = i + 1, 1 + i + e, 100 * e + i, 20 + i, e
            h.score_thresh, h.optimal_cost, h.y_s = 1.0 - 0.25 * i, 0.5 + e + i, 3.0 + e
            obs = np.frombuffer(raw, dtype="<i4", count=10, offset=rb + P.off_obs).reshape(5, 2)
            obs[:h.n_obs] = [[10 * e + k, 50 + i + k] for k in range(h.n_obs)]
            if level >= 2:
                np.frombuffer(raw, dtype="<f8", count=7, offset=rb + P.off_curve)[:sp["Lg"]] = 0.5 * np.arange(sp["Lg"]) + i + 10 * e
            if level >= 3:
                np.frombuffer(raw, dtype="<f8", count=7, offset=rb + P.off_mean)[:sp["Lg"]] = np.arange(sp["Lg"]) - i
                np.frombuffer(raw, dtype="<f8", count=7, offset=rb + P.off_std)[:sp["Lg"]] = 0.125 * (i + 1)
    return P, bytes(raw)


def test_two_edges_of_different_length_one_past_its_cap():
    P, raw = _build(3)
    d0, d1 = _lib.decode_history(raw, P, [7, 4], [5, 3], [10, 2])
    assert (d0["n_iter"], d0["dropped"]) == (3, 2) and (d1["n_iter"], d1["dropped"]) == (2, 0)
    assert d0["dropped"] > 0 and d0["n_iter"] > d1["n_iter"]
    assert [o.shape for o in d0["obs"]] == [(1, 2), (2, 2), (3, 2)] and [o.shape for o in d1["obs"]] == [(2, 2), (3, 2)]
    assert d0["obs"][2].dtype == np.int64 and d0["obs"][2].tolist() == [[0, 52], [1, 53], [2, 54]]
    assert d1["obs"][1].tolist() == [[10, 51], [11, 52], [12, 53]]
    assert d0["score_thresh"].tolist() == [1.0, 0.75, 0.5] and d1["optimal_cost"].tolist() == [1.5, 2.5]
    assert d0["best_idx"].tolist() == [0, 1, 2] and d1["best_idx"].tolist() == [100, 101] and d1["rank"].tolist() == [20, 21]
    assert d1["n_removed"].tolist() == [1, 1] and d1["y_s"].tolist() == [4.0, 4.0] and d0["n_obs"].tolist() == [1, 2, 3]
    assert len(d0["optimal_curves"]) == 3 and d0["optimal_curves"][1].shape == (7, 2) and d1["optimal_curves"][0].shape == (4, 2)
    assert d1["optimal_curves"][1][:, 0].tolist() == [2.0, 3.0, 4.0, 5.0]          # x = the edge's grid
    assert d1["optimal_curves"][1][:, 1].tolist() == [11.0, 11.5, 12.0, 12.5]
    assert d0["optimal_curves"][0][:, 0].tolist() == list(range(10, 17))
    assert d0["mean"].shape == (3, 7) and d1["mean"].shape == (2, 4) and d1["std"].shape == (2, 4)
    assert d0["mean"][2].tolist() == [-2.0, -1.0, 0.0, 1.0, 2.0, 3.0, 4.0] and d1["std"][1].tolist() == [0.25] * 4


def test_levels_leave_out_what_they_do_not_record():
    P1, raw1 = _build(1)
    d = _lib.decode_history(raw1, P1, [7, 4], [5, 3])
    assert "optimal_curves" not in d[0] and "mean" not in d[0] and "std" not in d[0] and d[0]["obs"][1].shape == (2, 2)
    P2, raw2 = _build(2)
    d = _lib.decode_history(raw2, P2, [7, 4], [5, 3])
    assert "mean" not in d[1] and "std" not in d[1] and len(d[1]["optimal_curves"]) == 2
    assert d[1]["optimal_curves"][0][:, 0].tolist() == [0.0, 1.0, 2.0, 3.0]  # no x_sts: the grid index


def test_an_empty_history_and_a_short_buffer():
    P = _lib.history_plan(3, 3, 5, 7)
    d = _lib.decode_history(bytes(2 * P.edge_bytes), P, [7, 4], [5, 3])
    assert [x["n_iter"] for x in d] == [0, 0] and d[0]["obs"] == [] and d[0]["mean"].shape == (0, 7) and d[1]["score_thresh"].shape == (0,)
    with pytest.raises(ValueError):
        _lib.decode_history(bytes(2 * P.edge_bytes - 1), P, [7, 4], [5, 3])
