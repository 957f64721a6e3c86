"""What the Python layer of the seed ensembles decides without a device: the group table and the arguments GP_Edge_Tracing_Batch.ensemble
and trace_ensemble refuse (before a library or a GPU is looked for), decode_ensemble on a buffer built by hand from the documented
layout (include/gpet_hip.h, "seed ensembles"), and the init-major batch layout of trace_ensemble."""
import struct

import numpy as np
import pytest

from gaussian_process_edge_trace_amd import _lib, gpet
from gaussian_process_edge_trace_amd import ensemble as ens


def bare_batch(grids):
    """A GP_Edge_Tracing_Batch with just what the argument checks read (no device, no library)."""
    b = object.__new__(gpet.GP_Edge_Tracing_Batch)
    b._ps = [dict(x_st=a, x_en=z) for a, z in grids]
    b.B = len(grids)
    return b


def test_group_table_checks():
    g, n = _lib.check_group_table([0, 1, 0, -1, 1, 0], 6)
    assert g.dtype == np.int32 and g.tolist() == [0, 1, 0, -1, 1, 0] and n == 2
    with pytest.raises(ValueError, match="one group index per edge"):
        _lib.check_group_table([0, 0], 3)
    with pytest.raises(ValueError, match="one group index per edge"):
        _lib.check_group_table([[0, 0]], 2)
    with pytest.raises(ValueError, match="below -1"):
        _lib.check_group_table([0, -2], 2)
    with pytest.raises(ValueError, match="never uses group 1 of 3"):
        _lib.check_group_table([0, 2, 2], 3)
    with pytest.raises(ValueError, match="no edge to a group"):
        _lib.check_group_table([-1, -1], 2)
    with pytest.raises(ValueError, match="integers"):
        _lib.check_group_table([0.0, 1.0], 2)


def test_batch_ensemble_refuses_before_a_device():
    same = bare_batch([(0, 63)] * 4)
    assert same.group_table(None).tolist() == [0, 0, 0, 0]
    assert same.group_table([1, 0, -1, 1]).tolist() == [1, 0, -1, 1]
    mixed = bare_batch([(0, 63), (0, 63), (0, 39)])
    with pytest.raises(ValueError, match="x-grids differ"):
        mixed.group_table(None)
    with pytest.raises(ValueError, match="x-grids differ"):
        mixed.ensemble()
    assert mixed.group_table([0, 0, 1]).tolist() == [0, 0, 1]  # (an explicit table may separate them; the library checks the grids)
    for tol in (-1, float("nan")):
        with pytest.raises(ValueError, match="tol"):
            same.ensemble(tol=tol)
    with pytest.raises(ValueError, match="one group index per edge"):
        same.ensemble(group_of=[0, 0])


def test_trace_ensemble_refuses_before_a_device():
    init = np.array([[0, 10], [63, 12]])
    grad = np.zeros((64, 64), np.float32)
    with pytest.raises(ValueError, match="at least one seed"):
        ens.trace_ensemble(init, grad, [])
    with pytest.raises(ValueError, match="at most 1024"):
        ens.trace_ensemble(init, grad, list(range(1025)))
    with pytest.raises(ValueError, match="tol"):
        ens.trace_ensemble(init, grad, [1, 2], tol=-0.1)
    with pytest.raises(ValueError, match="ONE"):
        ens.trace_ensemble(init, np.zeros((2, 64, 64), np.float32), [1, 2])
    for k in ("image_of", "obs"):
        with pytest.raises(ValueError, match=k):
            ens.trace_ensemble(init, grad, [1, 2], **{k: [0, 0]})
    with pytest.raises(ValueError, match="kernel_of has 1 entries for 2 inits"):
        ens.trace_ensemble([init, init], None, [1, 2], raw_imgs=grad, grad_kernel=[np.ones((3, 3))], kernel_of=[0])


def test_init_major_table_of_two_inits_three_seeds():
    group_of, seeds, init_of = ens.ensemble_table(2, [7, 8, 9])
    assert group_of.dtype == np.int32 and group_of.tolist() == [0, 0, 0, 1, 1, 1]
    assert seeds == [7, 8, 9, 7, 8, 9] and init_of.tolist() == [0, 0, 0, 1, 1, 1]
    assert _lib.check_group_table(group_of, 6)[1] == 2
    with pytest.raises(ValueError):
        ens.ensemble_table(0, [1])


def test_decode_a_buffer_built_by_hand():
    """G = 2 groups over B = 5 edges, len_cap = 6: record = 32 + 96 + 5 * 48 + 24 = 392 bytes, cost at 784, off at 824, 848 in all."""
    G, B, L = 2, 5, 6
    lay = _lib.ensemble_layout(G, B, L)
    assert (lay["record_bytes"], lay["off_cost"], lay["off_off"], lay["total_bytes"]) == (392, 784, 824, 848)
    buf = bytearray(848)
    # group 0: 3 members on 4 points from column 10; group 1: empty, 6 points from column 2
    struct.pack_into("<6id", buf, 0, 3, 4, 10, 3, 0, 0, 1.5)
    struct.pack_into("<8q", buf, 32, 5, 10, 6, 11, 6, 12, 7, 13)
    for i in range(5):  # median, q_lo, q_hi, min, max
        struct.pack_into("<4d", buf, 32 + 96 + 48 * i, *[100.0 * (i + 1) + k for k in range(4)])
    struct.pack_into("<4i", buf, 32 + 96 + 240, 3, 2, 3, 1)
    struct.pack_into("<6id", buf, 392, 0, 6, 2, -1, -1, 0, 1.5)
    struct.pack_into("<5d", buf, 784, 0.5, np.inf, 0.25, 0.75, 0.125)
    struct.pack_into("<5i", buf, 824, 2, -1, -1, 0, 1)
    group_of = [0, 1, -1, 0, 0]
    groups, cost, off = _lib.decode_ensemble(bytes(buf), G, B, L, group_of)
    assert cost.tolist() == [0.5, np.inf, 0.25, 0.75, 0.125] and off.tolist() == [2, -1, -1, 0, 1] and off.dtype == np.int32
    g0, g1 = groups
    assert (g0["n_members"], g0["edge_len"], g0["x_st"], g0["medoid"], g0["best_cost"], g0["tol"]) == (3, 4, 10, 3, 0, 1.5)
    assert g0["trace"].dtype == np.int64 and g0["trace"].tolist() == [[5, 10], [6, 11], [6, 12], [7, 13]]
    for i, k in enumerate(("median", "q_lo", "q_hi", "min", "max")):
        assert g0[k].tolist() == [100.0 * (i + 1) + j for j in range(4)], k
    assert g0["agree"].dtype == np.int32 and g0["agree"].tolist() == [3, 2, 3, 1]
    assert g0["members"].tolist() == [0, 3, 4] and g0["off"].tolist() == [2, 0, 1] and g0["cost"].tolist() == [0.5, 0.75, 0.125]
    assert (g1["n_members"], g1["edge_len"], g1["x_st"], g1["medoid"], g1["best_cost"]) == (0, 6, 2, -1, -1)
    assert g1["trace"].shape == (6, 2) and not g1["trace"].any() and not g1["median"].any() and not g1["agree"].any()
    assert g1["members"].size == 0 and g1["off"].size == 0 and g1["cost"].size == 0
    without = _lib.decode_ensemble(bytes(buf), G, B, L)[0]
    assert "members" not in without[0] and np.array_equal(without[0]["trace"], g0["trace"])
    with pytest.raises(ValueError, match="needs 848 bytes"):
        _lib.decode_ensemble(bytes(buf[:800]), G, B, L)
    with pytest.raises(ValueError, match="group_of has 4 entries"):
        _lib.decode_ensemble(bytes(buf), G, B, L, [0, 1, -1, 0])
