"""The curve scorer (csrc/gpet_k_sample_score.inc: k_score_tile + k_score_combine, and the wave-per-curve k_score) on injected
curves: written through GPET_BUF_SAMPLES, scored by gpet_score_curves, every cost compared with the extended-precision
restatement of the reference's cost (tests/curve_cost_exact.py) on the float32 image read back from GPET_BUF_GRAD -- for
float32 samples on the float32-rounded curves.

The inputs are those of tests/test_curve_cost_exact.py (which pins the reference itself against the oracle): thirteen families
of curves -- smooth, on integer rows, on row 0 and row M - 1, outside the image on either side, crossing it, sawteeth, random,
integers and integers nudged by an ulp, a jump at the last point -- on an image with 30 % exact zeros, at edge widths that put
the last Simpson pair on and next to the boundary of a 15-pair tile (Lg = 32 .. 35), at the shortest widths (4, 5), with and
without Cartwright's term (odd / even width), at x_st > 0 and ending at the image's last column, where the slab of the last
tile reaches beyond the image.  S >= 64 takes the tiled form (200: two blocks of 128 curves, the second not full; 1100: nine,
and the rank-counting top-k), S < 64 the wave-per-curve form, whose lane 63 takes its successor from the next chunk on the 65
pairs of Lg = 133.  One batch of three edges of 1, 2 and 3 tiles covers a launch with more tiles than an edge has.
With so few edges launch_score gives every workgroup 128 curves, one pass: the loop over passes -- the prefetch of the next 128
curves, its handover, the re-read of the block's first curve by rows beyond the block -- runs only in the batch of 26 edges at
S = 1100, whose workgroups take 256 curves (two passes; one that is not full in the last block of 76).
Not reached from here: k_score_tail, the fused form that only the device loop launches.  S < 101 is reachable through the C ABI
only (tests/injected_batch.py): the Python constructor turns such a count into 1000.

Tolerance, per curve: rtol = (npair + 32) 2^-53 cond, with npair = (Lg - 2) // 2 pairs and cond the reference's condition
number (sum |term| / |sum term|, at most 32 on these inputs).  Derived, not measured: a term of the line integral carries about
a dozen roundings (interpolation weights and taps, the 1e-3, two segment lengths each from a Newton-corrected rsqrt, the weight's
products), the arc's fewer, then the sum over the pairs in some order, the combination over the tiles and the division.

Measured on an MI355X (largest |cost - reference| / |reference| as a fraction of the bound, over all cases):
k_score_tile + k_score_combine 0.35 (Lg = 4; 0.10 at the other widths), k_score 0.07.  The constant 32 stands.
BUF_BEST_IDX must be the stable argsort of the device's own costs."""
import numpy as np
import pytest

from tests import curve_cost_exact as cx
from tests.injected_batch import make_batch

pytestmark = pytest.mark.gpu

SLACK = 32  # the constant of the bound above


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def check_edge(L, b, e, grad, x_st, Lg, Y, costs, cond, what):
    """Every cost of edge e within the bound, the top-k the stable argsort of the device's costs.  Returns the largest ratio of a
    deviation to its bound."""
    S = Y.shape[0]
    assert cond.max() <= 32.0
    got = b.read(L.BUF_COSTS, e)
    assert got.shape == (S,) and np.all(np.isfinite(got)), (what, got[~np.isfinite(got)][:8])
    npair = (Lg - 2) // 2
    dev = np.array([cx.rel_err(g, c) for g, c in zip(got, costs)])
    bound = (npair + SLACK) * 2.0 ** -53 * cond
    ratio = dev / bound
    w = int(ratio.argmax())
    print("%s: largest deviation %.2e, largest ratio to the bound %.3f (curve %d, %s, cond %.1f)"
          % (what, dev.max(), ratio[w], w, cx.FAMILIES[w % 13], cond[w]))
    assert ratio[w] <= 1.0, (what, w, cx.FAMILIES[w % 13], dev[w], bound[w], cond[w])
    n_keep = b.info(e)["n_keep"]
    assert n_keep == max(1, S // 4)
    order = np.argsort(got, kind="stable")[:n_keep]
    assert np.array_equal(b.read(L.BUF_BEST_IDX, e), order), what
    assert np.array_equal(b.read(L.BUF_BEST_COSTS, e), got[order]), what
    return ratio[w]


@pytest.mark.parametrize("shape,S,dtype", cx.CASES, ids=["M%d-N%d-x%d-Lg%d-S%d-%s" % (sh + (S, dt)) for sh, S, dt in cx.CASES])
def test_costs_of_injected_curves(amd, ctx, shape, S, dtype):
    L = amd._lib
    rows, N, x_st, Lg = shape
    grad, Y, costs, cond = cx.case_reference(shape, S, dtype)
    b = make_batch(amd, ctx, grad, [(x_st, Lg)], S, sample_dtype=dtype)
    try:
        assert (b.info()["Lg"], b.info()["S"]) == (Lg, S)
        assert np.array_equal(b.read(L.BUF_GRAD), grad)  # (min 0 and max 1: the library's normalisation changes nothing)
        b.write(L.BUF_SAMPLES, Y)
        assert np.array_equal(b.read(L.BUF_SAMPLES), Y)
        b.score()
        form = "k_score_tile" if S >= 64 else "k_score"  # (launch_score: an image this low always fits the tile's slab)
        check_edge(L, b, 0, grad, x_st, Lg, Y, costs, cond, "%s %s %s S=%d" % (form, dtype, shape, S))
    finally:
        b.close()


def test_costs_of_three_edges_with_different_tile_counts(amd, ctx):
    L = amd._lib
    grad, edges = cx.batch_reference()
    b = make_batch(amd, ctx, grad, cx.BATCH_SPANS, cx.BATCH_S)
    try:
        assert np.array_equal(b.read(L.BUF_GRAD), grad)
        assert [((Lg - 2) // 2 + 14) // 15 for _, Lg in cx.BATCH_SPANS] == [1, 2, 3]
        for e, (Y, _, _) in enumerate(edges):
            b.write(L.BUF_SAMPLES, Y, e)
        b.score()
        for e, ((x_st, Lg), (Y, costs, cond)) in enumerate(zip(cx.BATCH_SPANS, edges)):
            check_edge(L, b, e, grad, x_st, Lg, Y, costs, cond, "k_score_tile batch edge %d (x_st %d, Lg %d)" % (e, x_st, Lg))
    finally:
        b.close()


def curves_per_workgroup(B, Lg, S):
    """launch_score's choice, restated: 1024, halved down to 128 while the launch has fewer than 256 workgroups."""
    n_tiles = ((Lg - 2) // 2 + 14) // 15
    cpw = 1024
    while cpw > 128 and B * n_tiles * -(-S // cpw) < 256:
        cpw //= 2
    return cpw


def test_costs_with_two_passes_per_workgroup(amd, ctx):
    """26 edges of the first shape at S = 1100: 2 tiles x 5 blocks of 256 curves x 26 = 260 workgroups, two passes of 128 curves
    each (76 curves in the last block: one pass, not full).  Edge e holds the case's curves rotated by 7 e rows, so that no two
    edges hold the same curve in the same row."""
    L = amd._lib
    shape, S, B = cx.SHAPES[0], 1100, 26
    rows, N, x_st, Lg = shape
    assert curves_per_workgroup(B, Lg, S) == 256 and all(curves_per_workgroup(1, sh[3], s) == 128 for sh, s, _ in cx.CASES)
    assert curves_per_workgroup(len(cx.BATCH_SPANS), max(lg for _, lg in cx.BATCH_SPANS), cx.BATCH_S) == 128
    grad, Y, costs, cond = cx.case_reference(shape, S, "f64")
    b = make_batch(amd, ctx, grad, [(x_st, Lg)] * B, S)
    try:
        assert b.B == B and np.array_equal(b.read(L.BUF_GRAD), grad)
        for e in range(B):
            b.write(L.BUF_SAMPLES, np.roll(Y, 7 * e, axis=0), e)
        b.score()
        bound = ((Lg - 2) // 2 + SLACK) * 2.0 ** -53 * cond
        worst = 0.0
        for e in range(B):
            got = np.roll(b.read(L.BUF_COSTS, e), -7 * e)
            assert got.shape == (S,) and np.all(np.isfinite(got)), e
            ratio = np.array([cx.rel_err(g, c) for g, c in zip(got, costs)]) / bound
            w = int(ratio.argmax())
            worst = max(worst, ratio[w])
            assert ratio[w] <= 1.0, (e, w, cx.FAMILIES[w % 13], ratio[w] * bound[w], bound[w], cond[w])
        print("k_score_tile, two passes per workgroup: largest ratio to the bound %.3f" % worst)
    finally:
        b.close()
