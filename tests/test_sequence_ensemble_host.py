"""Host logic of seed ensembles in sequences (SequenceTracer(..., ensemble_seeds=)): the layout of a step's batch, the seed rule, the
refusals, and that without the new keywords the object lays a step out as it always did.  Needs no device: the tables are made from
the arguments alone (SequenceTracer.step_tables), and nothing here builds a batch."""
import numpy as np
import pytest

from gaussian_process_edge_trace_amd import _lib
from gaussian_process_edge_trace_amd.gpet_utils import kernel_builder
from gaussian_process_edge_trace_amd.sequence import SequenceTracer, trace_sequence

KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 10, 'length_scale': 8}, noise_y=1, N_samples=128, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True)
FRAMES = [np.zeros((64, 64), dtype=np.float32)] * 5
A, B = np.array([[0, 30], [63, 34]]), np.array([[16, 20], [47, 22]])


def same_inits(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


def test_layout_is_chain_major_init_major_member_minor():
    st = SequenceTracer(FRAMES, [A, B], n_chains=2, ensemble_seeds=[11, 12, 13], **KW)
    assert (st.E, st.K, st.chains) == (2, 3, [(0, 3), (3, 5)])
    active = [(0, 1), (1, 4)]  # step 1: frames 1 and 4
    tab = st.step_tables(active)
    assert same_inits(tab["inits"], [A, A, A, B, B, B, A, A, A, B, B, B])
    assert tab["seeds"] == [11, 12, 13] * 4  # member j of every frame and init: ensemble_seeds[j]
    assert tab["image_of"] == [0] * 6 + [1] * 6  # one image per chain's frame, read by its E * K edges
    assert tab["kernel_of"] is None
    assert tab["group_of"].dtype == np.int32 and tab["group_of"].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]
    # edge (ci * E + k) * K + j
    for ci in range(2):
        for k in range(2):
            for j in range(3):
                e = (ci * 2 + k) * 3 + j
                assert tab["group_of"][e] == ci * 2 + k and tab["seeds"][e] == 11 + j and tab["image_of"][e] == ci
    # the shorter chain has run out: one chain's frame, groups 0 .. E - 1
    tab = st.step_tables([(0, 2)])
    assert tab["group_of"].tolist() == [0, 0, 0, 1, 1, 1] and tab["image_of"] == [0] * 6 and tab["seeds"] == [11, 12, 13] * 2


def test_one_init_shares_the_frame_through_the_image_map_too():
    st = SequenceTracer(FRAMES, A, n_chains=2, ensemble_seeds=[5, 6, 7, 8], **KW)
    tab = st.step_tables([(0, 0), (1, 3)])
    assert not st.multi and same_inits(tab["inits"], [A] * 8)
    assert tab["image_of"] == [0, 0, 0, 0, 1, 1, 1, 1] and tab["group_of"].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert tab["seeds"] == [5, 6, 7, 8, 5, 6, 7, 8]


def test_two_kernels_follow_the_inits():
    k0, k1 = kernel_builder((11, 5)), kernel_builder((7, 3))
    frames = [np.zeros((64, 64), dtype=np.uint8)] * 5
    st = SequenceTracer(frames, [A, B], n_chains=2, ensemble_seeds=[1, 2], grad_kernel=[k0, k1], **KW)
    tab = st.step_tables([(0, 0), (1, 3)])
    assert tab["kernel_of"] == [0, 0, 1, 1, 0, 0, 1, 1] and tab["image_of"] == [0, 0, 0, 0, 1, 1, 1, 1]
    st = SequenceTracer(frames, [A, B, A], n_chains=1, ensemble_seeds=[1, 2], grad_kernel=[k0, k1], kernel_of=[1, 0, 1], **KW)
    assert st.step_tables([(0, 0)])["kernel_of"] == [1, 1, 0, 0, 1, 1]


def test_refusals():
    for bad in (dict(seed=3), dict(seeds=[1, 2, 3, 4, 5]), dict(seed=42)):
        with pytest.raises(ValueError, match="seed"):
            SequenceTracer(FRAMES, A, ensemble_seeds=[1, 2], **bad, **KW)
    with pytest.raises(ValueError, match="seed"):
        trace_sequence(FRAMES, A, ensemble_seeds=[1, 2], seed=7, **KW)
    with pytest.raises(ValueError, match="at least one seed"):
        SequenceTracer(FRAMES, A, ensemble_seeds=[], **KW)
    with pytest.raises(ValueError, match="at most %d" % _lib.ENSEMBLE_MAX):
        SequenceTracer(FRAMES, A, ensemble_seeds=list(range(_lib.ENSEMBLE_MAX + 1)), **KW)
    SequenceTracer(FRAMES, A, ensemble_seeds=list(range(_lib.ENSEMBLE_MAX)), **KW)  # (the bound itself is fine)
    with pytest.raises(ValueError, match="warm_from"):
        SequenceTracer(FRAMES, A, ensemble_seeds=[1, 2], warm_from="median", **KW)
    with pytest.raises(ValueError, match="ensemble_tol"):
        SequenceTracer(FRAMES, A, ensemble_seeds=[1, 2], ensemble_tol=-1, **KW)
    for w in ("medoid", "best_cost", "consensus"):
        assert SequenceTracer(FRAMES, A, ensemble_seeds=[1, 2], warm_from=w, ensemble_tol=0, **KW).warm_from == w


def test_without_the_keywords_a_step_is_laid_out_as_ever():
    """The batch arguments of the sequence paths that exist: one seed per FRAME shared by its E edges, an image map only with
    several inits or a kernel table, no groups."""
    seeds = [5, 6, 7, 8, 9]
    active = [(0, 1), (1, 4)]
    one = SequenceTracer(FRAMES, A, n_chains=2, seeds=seeds, **KW)
    tab = one.step_tables(active)
    assert (one.K, one.ensemble_seeds) == (1, None)
    assert same_inits(tab["inits"], [A, A]) and tab["seeds"] == [6, 9]
    assert tab["image_of"] is None and tab["kernel_of"] is None and tab["group_of"] is None
    two = SequenceTracer(FRAMES, [A, B], n_chains=2, seeds=seeds, **KW)
    tab = two.step_tables(active)
    assert same_inits(tab["inits"], [A, B, A, B]) and tab["seeds"] == [6, 6, 9, 9] and tab["image_of"] == [0, 0, 1, 1]
    assert tab["kernel_of"] is None and tab["group_of"] is None
    k0, k1 = kernel_builder((11, 5)), kernel_builder((7, 3))
    multi = SequenceTracer([np.zeros((64, 64), dtype=np.uint8)] * 5, [A, B], n_chains=2, seeds=seeds, grad_kernel=[k0, k1], **KW)
    tab = multi.step_tables(active)
    assert tab["kernel_of"] == [0, 1, 0, 1] and tab["image_of"] == [0, 0, 1, 1] and tab["group_of"] is None
    # the default seed is still 42 for every frame
    assert SequenceTracer(FRAMES, A, **KW).seeds == [42] * 5 and SequenceTracer(FRAMES, A, seed=3, **KW).seeds == [3] * 5
    assert SequenceTracer(FRAMES, A, 1, None, 9, **KW).seeds == [9] * 5  # (seed is still the fifth positional argument)


def test_set_frame_keywords_are_checked_before_the_device_is():
    """warm_from without warm_every, and warm_from with obs, are ValueErrors raised before anything is asked of the batch."""
    from gaussian_process_edge_trace_amd.gpet import GP_Edge_Tracing_Batch
    b = object.__new__(GP_Edge_Tracing_Batch)  # (no constructor: no device; the refusals must not get as far as using one)
    with pytest.raises(ValueError, match="warm_every"):
        b.set_frame([FRAMES[0]], warm_from="medoid")
    with pytest.raises(ValueError, match="alternatives"):
        b.set_frame([FRAMES[0]], obs=[np.zeros((0, 2))], warm_every=5, warm_from="medoid")
    with pytest.raises(ValueError, match="warm_from"):
        b.set_frame([FRAMES[0]], warm_every=5, warm_from="mean")
