"""sequence.warm_start_obs against a restatement in plain loops: the function is the oracle of the device warm start
(tests/test_gpu_warm_start.py, tests/test_gpu_fit_injection.py) and was only ever used as the expected value.  The rule
(gpet.py:57-61, 820, 829): candidates are the trace's pixels at the grid indices step, 2 step, ... below the last one, from
step = max(1, warm_every); a candidate is kept when its column lies strictly between the end points and its row in the image;
while algo_thresh or more are kept (and not none) the stride doubles.  No GPU needed."""
import itertools

import numpy as np
import pytest

from gaussian_process_edge_trace_amd.sequence import warm_start_obs

M = 48
X_ST = 17
INT64_MIN = -2 ** 63  # what finish's np.rint(...).astype(int) yields for a NaN or infinite mean
LGS = [1, 2, 3, 64, 65, 129, 256]


def rule_in_loops(trace, x_st, x_en, warm_every, algo_thresh, n_rows):
    """The rule with one Python loop over grid indices per stride: no slicing, no masks.  Returns a list of (x, y)."""
    n = len(trace)
    step = warm_every if warm_every > 1 else 1
    while True:
        kept = []
        k = step
        while k < n - 1:
            y, x = int(trace[k][0]), int(trace[k][1])
            if x > x_st and x < x_en and y >= 0 and y <= n_rows - 1:
                kept.append((x, y))
            k += step
        if len(kept) < algo_thresh or len(kept) == 0:
            return kept
        step *= 2


def rows_of(kind, Lg, rs):
    if kind == "inside":
        y = rs.randint(0, M, Lg).astype(np.int64)
        y[::5] = M - 1  # (the image's last row and its first are inside)
        y[1::5] = 0
        return y
    if kind == "outside":
        return rs.choice(np.array([-1, M, M + 5, -7, INT64_MIN, 2 ** 62], dtype=np.int64), Lg)
    y = rs.randint(-6, M + 6, Lg).astype(np.int64)  # mixed: both sides of both borders, and NaN's INT64_MIN
    y[::7] = INT64_MIN
    y[3::11] = M
    y[4::11] = -1
    return y


def trace_of(kind, Lg, seed):
    rs = np.random.RandomState(seed)
    return np.stack([rows_of(kind, Lg, rs), X_ST + np.arange(Lg, dtype=np.int64)], axis=1)  # yx, as finish returns it


def check(trace, x_st, x_en, warm_every, algo_thresh):
    got = warm_start_obs(trace, x_st, x_en, warm_every, algo_thresh, M)
    want = rule_in_loops(trace, x_st, x_en, warm_every, algo_thresh, M)
    ctx = (len(trace), x_st, x_en, warm_every, algo_thresh)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.ndim == 2 and got.shape[1] == 2, ctx
    assert got.tolist() == [list(p) for p in want], ctx  # xy column order, the same points in the same order
    assert np.all(np.diff(got[:, 0]) > 0), ctx  # ascending x
    assert len(got) < algo_thresh or len(got) == 0, ctx
    return got


@pytest.mark.parametrize("Lg", LGS)
def test_warm_start_obs_equals_the_rule_in_plain_loops(Lg):
    warm = [-5, 0, 1, 2, 3, 64, Lg - 2, Lg - 1, Lg, 2 ** 31 - 1]
    thresh = [-3, 0, 1, 18, 39, 128, Lg]
    n_kept = set()
    for ki, kind in enumerate(["inside", "outside", "mixed"]):
        trace = trace_of(kind, Lg, 100 * Lg + ki)
        for w, a in itertools.product(warm, thresh):
            got = check(trace, X_ST, X_ST + Lg - 1, w, a)
            n_kept.add(len(got))
            if kind == "outside":
                assert len(got) == 0
        # end points narrower than the trace: the column test decides, not only the slice
        for w, a in itertools.product([1, 3], [18, Lg]):
            got = check(trace, X_ST + 3, X_ST + Lg - 6, w, a)
            assert np.all((got[:, 0] > X_ST + 3) & (got[:, 0] < X_ST + Lg - 6))
    if Lg >= 64:
        assert max(n_kept) >= 18  # (the sweep is not all empty sets)


def test_warm_start_obs_hand_worked_cases():
    """Counts worked out by hand from the rule, so that a misreading shared by the function and its restatement shows."""
    Lg = 256
    tr = np.stack([np.full(Lg, 7, dtype=np.int64), np.arange(Lg, dtype=np.int64)], axis=1)
    # 254 inner pixels; strides 1, 2, 4 keep 254, 127, 63 -- all at or above 39 --, stride 8 keeps x = 8, 16, ..., 248: 31
    o = warm_start_obs(tr, 0, Lg - 1, 1, 39, M)
    assert o.dtype == np.int64 and o[:, 0].tolist() == list(range(8, 255, 8)) and o[:, 1].tolist() == [7] * 31
    # a threshold of 128 is first met by the 127 pixels of stride 2; one of 127 needs stride 4
    assert warm_start_obs(tr, 0, Lg - 1, 1, 128, M)[:, 0].tolist() == list(range(2, 255, 2))
    assert warm_start_obs(tr, 0, Lg - 1, 1, 127, M)[:, 0].tolist() == list(range(4, 255, 4))
    # the last pixel of the trace is never a candidate, the one before it is
    assert warm_start_obs(tr, 0, Lg - 1, 127, 39, M)[:, 0].tolist() == [127, 254]
    assert warm_start_obs(tr, 0, Lg - 1, 255, 39, M).shape == (0, 2)
    # a threshold of zero or below cannot be met from below: the stride doubles until nothing is kept
    assert warm_start_obs(tr, 0, Lg - 1, 1, 0, M).shape == (0, 2) and warm_start_obs(tr, 0, Lg - 1, 1, -3, M).shape == (0, 2)
    # rows: 0 and M - 1 are in the image, -1, M and INT64_MIN are not
    tr2 = tr.copy()
    tr2[1:6, 0] = [0, M - 1, -1, M, INT64_MIN]
    assert warm_start_obs(tr2, 0, Lg - 1, 1, 256, M)[:3].tolist() == [[1, 0], [2, M - 1], [6, 7]]
    # without M rows are not tested (the constructor's obs argument has no such test either)
    assert warm_start_obs(tr2, 0, Lg - 1, 1, 256)[:5, 1].tolist() == [0, M - 1, -1, M, INT64_MIN]
