"""GPU tests of label maps (gpet_label_maps[_xy], gpet_batch_label_maps[_xy]; k_label_thresholds, k_label_fill, k_label_thick,
k_label_vertices, k_label_fill_xy; gpet_utils.label_maps / outline_label_maps, GP_Edge_Tracing_Batch.label_maps,
SequenceTracer(labels=)).

Both rules are integer or float64 arithmetic without a transcendental function, so everything below is np.array_equal against
tests/label_ref.py.  The shapes cover the 16-byte chunk a lane stores (N = 15, 16, 17), a row end inside a chunk, more than one wave
and more than one workgroup (70 x 130 = 9 100 bytes against 4 096 a workgroup), a row longer than a wave's kilobyte (3 x 1025)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import band_ref, label_ref as R, polar_ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(2, 2), (5, 7), (3, 15), (3, 16), (3, 17), (33, 64), (64, 65), (70, 130), (3, 1025)]
KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 10, 'length_scale': 8}, noise_y=1, N_samples=128, score_thresh=1, delta_x=5,
          keep_ratio=0.1, pixel_thresh=3, fix_endpoints=True)


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


class DeviceBytes(object):
    """``n`` bytes of device memory of the context, filled with ``fill``; ``at(off)`` is an address inside."""

    def __init__(self, ctx, n, fill=0xAB):
        self.ctx, self.n = ctx, int(n)
        d = C.c_void_p()
        ctx.check(ctx.lib.gpet_dev_alloc(ctx.h, self.n, C.byref(d)))
        self.ptr = d.value
        self.upload(np.full(self.n, fill, dtype=np.uint8))

    def upload(self, a):
        a = np.ascontiguousarray(a)
        self.ctx.check(self.ctx.lib.gpet_dev_copy(self.ctx.h, C.c_void_p(self.ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, 0))

    def download(self):
        out = np.empty(self.n, dtype=np.uint8)
        self.ctx.sync()
        self.ctx.check(self.ctx.lib.gpet_dev_copy(self.ctx.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), out.nbytes, 1))
        return out

    def at(self, off):
        return self.ptr + int(off)

    def free(self):
        self.ctx.lib.gpet_dev_free(self.ctx.h, C.c_void_p(self.ptr))


# ---- Rule 1 on injected rows ---------------------------------------------------------------------------------------------------------
def edges_case(seed, M, N, per_map):
    """(x_st, rows, map_of) of two maps: map 0 with ``per_map`` edges that are NOT adjacent in the table -- an edge of map 1 and edges on no
    map lie between them --, map 1 with one edge.  Partial grids, rows from below 0 to above M (-1, 0, M - 1, M, M + 1 for certain), rows
    that cross, NO_ROW here and there."""
    rng = np.random.default_rng(seed)
    map_of = []
    for e in range(per_map):
        map_of.append(0)
        if e == 0:
            map_of.append(1)
        if e % 5 == 1:
            map_of.append(-1)
    if per_map == 1:
        map_of.append(-1)
    x_st, rows = [], []
    for e in range(len(map_of)):
        full = e % 3 == 0
        x0 = 0 if full else int(rng.integers(0, N - 1))
        n = N if full else int(rng.integers(1, N - x0 + 1))
        t = rng.integers(-3, M + 4, size=n).astype(np.int64)  # (independent per column: neighbouring edges cross all the time)
        t[rng.random(n) < 0.08] = R.NO_ROW
        x_st.append(x0)
        rows.append(t)
    special = np.array([-1, 0, M - 1, M, M + 1, R.NO_ROW], dtype=np.int64)
    rows[0][:min(N, 6)] = special[:min(N, 6)]
    return x_st, rows, map_of


@pytest.mark.parametrize("per_map", [1, 3, 32])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_row_maps_on_injected_rows(amd, ctx, shape, per_map):
    M, N = shape
    x_st, rows, map_of = edges_case(1000 * per_map + M + N, M, N, per_map)
    L = R.most_edges(map_of, len(map_of))
    assert L == per_map
    for extend in (False, True):
        want = R.row_maps(shape, x_st, rows, map_of, extend)
        thick_want = R.thick_of(want, L)  # (counting the reference map)
        assert np.array_equal(thick_want.sum(axis=1), np.full((2, N), M))
        for transposed in (False, True):
            got, thick = ctx.label_maps(shape, x_st, rows, map_of, extend=extend, transposed=transposed, thickness=True)
            assert got.dtype == np.uint8 and got.shape == ((2, N, M) if transposed else (2, M, N))
            assert np.array_equal(got, want.transpose(0, 2, 1) if transposed else want), (shape, per_map, extend, transposed)
            assert thick.dtype == np.int32 and np.array_equal(thick, thick_want), (shape, per_map, extend, transposed)
            assert np.array_equal(ctx.label_maps(shape, x_st, rows, map_of, extend=extend, transposed=transposed), got)  # (without thick)
    assert want.max() > 1 or per_map == 1


@pytest.mark.parametrize("shape", [(5, 7), (3, 17), (64, 65), (70, 130)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mis", [0, 3, 13])
def test_row_maps_into_device_memory(amd, ctx, shape, mis):
    """GPET_LABELS_OUT_ON_DEVICE: the maps lie one behind the other ``mis`` bytes past a 256-byte boundary (M N is odd for three of the
    shapes: every map then starts at another offset inside its 16 bytes); not a byte around them is touched."""
    M, N = shape
    x_st, rows, map_of = edges_case(77 + M + mis, M, N, 3)
    L, n_maps, guard = 3, 2, 64
    n_thick = amd._lib.label_thick_count(n_maps, L, N)
    for transposed in (False, True):
        want = R.row_maps(shape, x_st, rows, map_of, True, transposed=transposed)
        buf = DeviceBytes(ctx, 2 * guard + mis + n_maps * M * N)
        tbuf = DeviceBytes(ctx, 4 * n_thick + 2 * guard)
        try:
            ptrs = [buf.at(guard + mis + f * M * N) for f in range(n_maps)]
            assert ctx.label_maps(shape, x_st, rows, map_of, extend=True, transposed=transposed, thickness=True, out_device_ptrs=ptrs,
                                  thick_device_ptr=tbuf.at(guard)) is None
            raw, traw = buf.download(), tbuf.download()
            assert np.all(raw[:guard + mis] == 0xAB) and np.all(raw[guard + mis + n_maps * M * N:] == 0xAB)
            assert np.array_equal(raw[guard + mis:guard + mis + n_maps * M * N].reshape(want.shape), want)
            assert np.all(traw[:guard] == 0xAB) and np.all(traw[guard + 4 * n_thick:] == 0xAB)
            thick = traw[guard:guard + 4 * n_thick].view(np.int32).reshape(n_maps, L + 1, N)
            assert np.array_equal(thick, R.thick_of(R.row_maps(shape, x_st, rows, map_of, True), L))
        finally:
            buf.free()
            tbuf.free()


def test_row_maps_refusals_through_the_c_abi(amd, ctx):
    L = amd._lib
    M, N = 6, 9
    rows = [np.arange(N, dtype=np.int64) % M] * 34
    with pytest.raises(ValueError, match=r"map 0 has more than 32 edges \(33\)"):
        ctx.label_maps((M, N), [0] * 33, rows[:33])
    assert ctx.label_maps((M, N), [0] * 32, rows[:32]).max() == 32
    # straight at the library: the words are label_check's, nothing is launched
    xs, ln, flat = np.zeros(33, np.int32), np.full(33, N, np.int32), np.concatenate(rows[:33])
    out = np.full((1, M, N), 7, dtype=np.uint8)
    ip, op = C.POINTER(C.c_int32), (C.c_void_p * 2)(out.ctypes.data, out.ctypes.data)  # (one entry per map of the widest table below)

    def call(n, map_of, n_maps, M=M, N=N, flags=0, xs=xs, outp=op):
        m = np.ascontiguousarray(map_of, dtype=np.int32)
        return ctx.lib.gpet_label_maps(ctx.h, M, N, n, xs.ctypes.data_as(ip), ln.ctypes.data_as(ip), flat.ctypes.data_as(C.POINTER(C.c_int64)),
                                       m.ctypes.data_as(ip), n_maps, flags, outp, None)

    for args, words in (((33, [0] * 33, 1), "label maps: map 0 has more than 32 edges (33)"),
                        ((3, [0, 2, 0], 2), "label maps: map_of[1] = 2 lies outside [-1, n_maps = 2)"),
                        ((3, [0, -1, 0], 2), "label maps: map 1 has no edge"),
                        ((3, [0, 0, 0], 0), "label maps: n_maps must be at least 1"),
                        ((3, [0, 0, 0], 1, 1, N), "label maps: frames must be at least 2 x 2 pixels"),
                        ((3, [0, 0, 0], 1, M, N - 1), "label maps: the grid of edge 0 lies outside [0, N) (x_st = 0, len = 9, N = 8)"),
                        ((3, [0, 0, 0], 1, M, N, 0, xs, None), "label maps: a null pointer"),
                        ((3, [0, 0, 0], 1, M, N, 8), "label maps: unknown flag bits 0x8")):
        assert call(*args) == L.ERR_BAD_ARG
        assert ctx.lib.gpet_last_error(ctx.h).decode() == words
    assert np.all(out == 7)
    assert call(3, [0, 0, 0], 1) == L.OK and np.array_equal(out, R.row_maps((M, N), [0] * 3, rows[:3]))


# ---- Rule 2 on injected vertices -----------------------------------------------------------------------------------------------------
def star(n, shape, seed, reach):
    """n vertices around the middle of the frame at angles in order, radii up to ``reach`` times the frame's larger half extent."""
    Ms, Ns = shape
    rng = np.random.default_rng(seed)
    th = (np.arange(n) + rng.random(n) * 0.8) * (2.0 * np.pi / n)
    rad = (0.25 + 0.75 * rng.random(n)) * reach * max(Ms, Ns) / 2.0
    return np.stack([Ns / 2.0 - 0.3 + rad * np.cos(th), Ms / 2.0 + 0.2 + rad * np.sin(th)], axis=1)


@pytest.mark.parametrize("n", [4, 5, 64, 65, 720])
@pytest.mark.parametrize("shape", [(9, 9), (33, 64), (70, 130)], ids=lambda s: "%dx%d" % s)
def test_outline_maps_on_injected_vertices(amd, ctx, shape, n):
    inner = star(n, shape, 10 * n + shape[0], 0.6)
    leaving = star(n, shape, 10 * n + shape[1] + 1, 1.6)
    leaving[0], leaving[n // 2] = (shape[1] + 3.5, shape[0] / 2.0), (-4.25, shape[0] / 2.0 - 1.0)  # (leaves the frame on the right and on the left)
    assert leaving[:, 0].min() < 0 and leaving[:, 0].max() > shape[1] - 1
    outlines, map_of = [inner, leaving, inner * 0.5 + np.array([shape[1], shape[0]]) * 0.25], [0, 1, 0]
    want = R.outline_maps(shape, outlines, map_of)
    got = amd.gpet_utils.outline_label_maps(outlines, shape, map_of, ctx=ctx)
    assert got.dtype == np.uint8 and got.shape == (2,) + shape and np.array_equal(got, want)
    assert want[0].max() >= 1 and want[1].max() == 1
    buf = DeviceBytes(ctx, 128 + 5 + 2 * shape[0] * shape[1])
    try:  # (device destinations, 5 bytes past a 16-byte boundary)
        ptrs = [buf.at(64 + 5 + f * shape[0] * shape[1]) for f in range(2)]
        assert ctx.label_maps_xy(shape, outlines, map_of, out_device_ptrs=ptrs) is None
        raw = buf.download()
        assert np.all(raw[:69] == 0xAB) and np.all(raw[69 + want.size:] == 0xAB) and np.array_equal(raw[69:69 + want.size].reshape(want.shape), want)
    finally:
        buf.free()


def test_outline_maps_special_outlines(amd, ctx):
    U = amd.gpet_utils
    shape = (12, 14)
    touching = np.array([[1, 1], [4, 1], [4, 4], [7, 4], [7, 7], [4, 7], [4, 4], [1, 4]], dtype=np.float64)  # two squares that share a vertex
    square = np.array([[2, 3], [11, 3], [11, 9], [2, 9]], dtype=np.float64)  # horizontal segments on pixel rows 3 and 9, vertices on pixels
    bowtie = np.array([[1.5, 1.5], [10.5, 8.5], [10.5, 1.5], [1.5, 8.5]])
    for xy in (touching, square, bowtie, square[::-1]):
        got = U.outline_label_maps(xy, shape, ctx=ctx)
        assert np.array_equal(got, R.outline_maps(shape, [xy])) and got.max() == 1
    sq = U.outline_label_maps(square, shape, ctx=ctx)[0]
    assert sq[3, 2] == 1 and sq[9, 5] == 0 and sq[5, 11] == 0 and sq.sum() == 6 * 9  # (rows 3 .. 8, columns 2 .. 10: the upper and left sides are in)
    # two nested outlines: lumen 2, wall 1, outside 0
    th = 2.0 * np.pi * np.arange(40) / 40
    outer = np.stack([32.3 + 20.0 * np.cos(th), 30.1 + 17.0 * np.sin(th)], axis=1)
    inner = np.stack([32.3 + 9.0 * np.cos(th), 30.1 + 8.0 * np.sin(th)], axis=1)
    nested = U.outline_label_maps([outer, inner], (61, 66), ctx=ctx)
    assert nested.shape == (1, 61, 66) and np.array_equal(nested, R.outline_maps((61, 66), [outer, inner]))
    assert set(np.unique(nested)) == {0, 1, 2} and nested[0, 30, 32] == 2 and nested[0, 30, 48] == 1 and nested[0, 2, 2] == 0
    # a vertex that is not finite takes its outline out, the other one stays
    bad = inner.copy()
    bad[7, 1] = np.inf
    assert np.array_equal(U.outline_label_maps([outer, bad], (61, 66), ctx=ctx), R.outline_maps((61, 66), [outer]))
    for n in (3, 4097):
        with pytest.raises(ValueError, match=r"contour 0 has %d vertices, outside \[4, 4096\]" % n):
            U.outline_label_maps(np.zeros((n, 2)), shape, ctx=ctx)
    big = np.stack([7.0 + 5.0 * np.cos(2 * np.pi * np.arange(4096) / 4096), 6.0 + 4.0 * np.sin(2 * np.pi * np.arange(4096) / 4096)], axis=1)
    assert np.array_equal(U.outline_label_maps(big, shape, ctx=ctx), R.outline_maps(shape, [big]))  # (64 KB of vertices in LDS)


# ---- the batch forms ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def layered(amd):
    """6 uint8 frames of 64 x 65 with two layers 22 rows apart (tests/test_gpu_bands.py's scene), the two inits, the kernel."""
    frames, init_a, init_b, _ = band_ref.layered_frames(64, 65, 6, 165, "uint8", base=14, gap=22, step=4.5)
    return dict(frames=frames, inits=[init_a, init_b], K=amd.gpet_utils.kernel_builder((11, 5)))


def check_batch(amd, ctx, b, traces, shape, transpose=False, L=2):
    """batch.label_maps() against gpet_utils.label_maps of the traces the batch returned, and against the restated rule."""
    map_of = b.default_map_of()
    want = R.trace_maps(traces, shape, map_of, transpose=transpose)
    got, thick = b.label_maps(thickness=True)
    assert got.dtype == np.uint8 and got.shape == (max(map_of) + 1,) + tuple(shape) and np.array_equal(got, want)
    mine, mine_thick = amd.gpet_utils.label_maps(traces, shape, map_of, thickness=True, transpose=transpose, ctx=ctx)
    assert np.array_equal(got, mine) and np.array_equal(thick, mine_thick)
    rows_major = want.transpose(0, 2, 1) if transpose else want
    assert np.array_equal(thick, R.thick_of(rows_major, L))
    assert np.array_equal(b.label_maps(extend=True), R.trace_maps(traces, shape, map_of, extend=True, transpose=transpose))
    return got


def test_batch_with_an_image_map(amd, ctx, layered):
    """2 frames x 2 edges: by default every frame is a map and its two edges the layer boundaries."""
    b = amd.GP_Edge_Tracing_Batch(layered["inits"] * 2, None, [3, 4, 5, 6], raw_imgs=layered["frames"][:2], grad_kernel=layered["K"],
                                  image_of=[0, 0, 1, 1], _ctx=ctx, **KW)
    traces = b()
    assert b.default_map_of() == [0, 0, 1, 1]
    got = check_batch(amd, ctx, b, traces, (64, 65))
    assert set(np.unique(got)) == {0, 1, 2}
    # the caller's own table: edges that are not adjacent on one map, an edge on none
    assert np.array_equal(b.label_maps([1, 0, 1, -1]), R.trace_maps(traces, (64, 65), [1, 0, 1, -1]))
    # into device memory
    buf = DeviceBytes(ctx, 2 * 64 * 65 + 64)
    try:
        assert b.label_maps(out_device_ptrs=[buf.at(7), buf.at(7 + 64 * 65)]) is None
        assert np.array_equal(buf.download()[7:7 + 2 * 64 * 65].reshape(2, 64, 65), got)
    finally:
        buf.free()
    with pytest.raises(ValueError, match="not built on polar frames"):
        b.label_maps(space="frame")
    with pytest.raises(ValueError, match="map 1 has no edge"):
        b.label_maps([0, 0, 2, 2])
    b._batch.close()


def test_banded_batch_gives_full_frame_rows(amd, ctx, layered):
    b = amd.GP_Edge_Tracing_Batch(layered["inits"], None, [5, 6], raw_imgs=layered["frames"][1], grad_kernel=layered["K"], band_rows=32,
                                  band_r0=(7, 13), _ctx=ctx, **KW)
    traces = b()
    assert b._batch.M == 32 and b._batch.frame_M == 64 and b.default_map_of() == [0, 0]
    got = check_batch(amd, ctx, b, traces, (64, 65))
    assert got.shape == (1, 64, 65) and got[0, 63].min() == 2 and got[0, 0].max() == 0
    b._batch.close()


def test_vertical_batch_gives_maps_in_the_frames_orientation(amd, ctx):
    from tests.test_gpu_orientation import FM, FN, vertical_frame
    made = [vertical_frame(amd, 40 + t, "uint8", amplitude=38 + t) for t in range(2)]
    K = amd.gpet_utils.kernel_builder((11, 5), vertical_edges=True)
    b = amd.GP_Edge_Tracing_Batch([made[0][1]] * 4, None, [3, 4, 5, 6], raw_imgs=[m[0] for m in made], grad_kernel=K, image_of=[0, 0, 1, 1],
                                  orientation="vertical", _ctx=ctx, **KW)
    traces = b()
    assert traces[0].shape[0] > 100 and np.array_equal(traces[0][:, 0], traces[0][0, 0] + np.arange(traces[0].shape[0]))  # one entry per frame row
    got = check_batch(amd, ctx, b, traces, (FM, FN), transpose=True)
    assert got.shape == (2, FM, FN) and got[0][:, FN - 1].max() == 2 and got[0][:, 0].max() == 0  # (labels grow to the right)
    b._batch.close()


def disc_bound(R0, a):
    """(area, perimeter) of the outline R(theta) = R0 + a cos 3 theta: the area is (1/2) int R^2 = pi (R0^2 + a^2 / 2) exactly; the
    perimeter int sqrt(R^2 + R'^2) by the midpoint rule on 2^16 points."""
    th = (np.arange(1 << 16) + 0.5) * (2.0 * np.pi / (1 << 16))
    Rt, dR = R0 + a * np.cos(3 * th), -3.0 * a * np.sin(3 * th)
    return np.pi * (R0 * R0 + a * a / 2.0), float(np.sum(np.hypot(Rt, dR)) * (2.0 * np.pi / (1 << 16)))


def test_polar_batch_in_both_spaces(amd, ctx):
    """The polar test disc: space='frame' is Rule 2 on the vertices polar_trace_xy gives.  The area inside lies within the perimeter's
    pixel count of the disc's own: the traced outline runs within about a pixel of R(theta) = 26 + 4 cos 3 theta (the trace's mean radial
    error is below one row), and counting pixel centres misjudges a region by less than the pixels its boundary passes through --
    both are bounded by one pixel per unit of the outline's length, the perimeter derived in disc_bound."""
    U = amd.gpet_utils
    g = np.load(os.path.join(GOLDEN, "polar_disc.npz"))
    pol, kw = json.loads(str(g["polar"])), json.loads(str(g["kw"]))
    assert tuple(g["outer"]) == (26.0, 4.0)
    bt = amd.GP_Edge_Tracing_Batch([g["init"]], None, [int(g["seed"])], raw_imgs=g["frame"], grad_kernel=g["kernel"],
                                   polar=dict(pol, centre=tuple(g["centre"])), _ctx=ctx, **kw)
    trace = bt()[0]
    xy = U.polar_trace_xy(trace, bt.polar)
    assert np.array_equal(xy[0], xy[-1])
    got = bt.label_maps(space="frame")
    assert got.shape == (1, 96, 96) and got.dtype == np.uint8
    assert np.array_equal(got, U.outline_label_maps(xy[:-1], (96, 96), ctx=ctx)) and np.array_equal(got, R.outline_maps((96, 96), [xy[:-1]]))
    area, perimeter = disc_bound(26.0, 4.0)
    print("polar disc: %d pixels inside, area %.1f, perimeter %.1f" % (got.sum(), area, perimeter))
    assert abs(float(got.sum()) - area) <= perimeter
    assert got[0, 48, 47] == 1 and got[0, 2, 2] == 0
    # space=None / 'polar': Rule 1 in polar rows and columns
    polar_maps = bt.label_maps()
    assert polar_maps.shape == (1, 40, 93) and np.array_equal(polar_maps, bt.label_maps(space="polar"))
    assert np.array_equal(polar_maps, R.trace_maps([trace], (40, 93))) and np.array_equal(polar_maps, U.label_maps(trace, (40, 93), ctx=ctx))
    with pytest.raises(ValueError, match="space must be"):
        bt.label_maps(space="screen")
    bt._batch.close()
    # an edge that does not run from seam to seam is no closed contour
    init = np.array([[5, int(g["init"][0, 1])], [60, int(g["init"][0, 1])]])
    part = amd.GP_Edge_Tracing_Batch([init], None, [1], raw_imgs=g["frame"], grad_kernel=g["kernel"], polar=dict(pol, centre=tuple(g["centre"])),
                                     _ctx=ctx, **kw)
    part()
    with pytest.raises(amd._lib.GpetError, match=r"edge 0 does not span the closed contour \(x_st = 5, x_en = 60; pad = 1, pad \+ n_theta = 91\)"):
        part.label_maps(space="frame")
    part._batch.close()


def test_two_nested_contours_of_two_frames(amd, ctx):
    """The batch of tests/test_gpu_polar.py: two frames, the two outlines of a nested lumen each, a centre per frame -- lumen 2, wall 1."""
    U = amd.gpet_utils
    K = U.kernel_builder((5, 3))
    cs = [(47.5, 48.25), (49.0, 46.5)]
    frames = [polar_ref.disc_frame((96, 96), c, seed=31 + i) for i, c in enumerate(cs)]
    pol = dict(centre=cs, n_r=40, n_theta=90)
    inits = [U.closed_init(int(round(polar_ref.outline(0.0, *o))), dict(pol, pad=1)) for _ in range(2) for o in ((14.0, 2.0), (26.0, 4.0))]
    b = amd.GP_Edge_Tracing_Batch(inits, None, [3, 4, 5, 6], raw_imgs=frames, grad_kernel=K, image_of=[0, 0, 1, 1], polar=pol, _ctx=ctx, **KW)
    traces = b()
    got = b.label_maps(space="frame")
    want = np.concatenate([R.outline_maps((96, 96), [U.polar_trace_xy(traces[2 * f + k], b.polar, frame=f)[:-1] for k in range(2)]) for f in range(2)])
    assert got.shape == (2, 96, 96) and np.array_equal(got, want)
    assert all(set(np.unique(m)) == {0, 1, 2} for m in got) and got[0, 48, 47] == 2 and got[1, 46, 49] == 2
    b._batch.close()


# ---- state ------------------------------------------------------------------------------------------------------------------------------
def test_label_maps_are_valid_exactly_when_results_are(amd, ctx, layered):
    L = amd._lib
    b = amd.GP_Edge_Tracing_Batch(layered["inits"], None, [3, 4], raw_imgs=layered["frames"][0], grad_kernel=layered["K"], _ctx=ctx, **KW)
    words = "gpet_batch_label_maps: no converged fit of the current trace"
    with pytest.raises(L.GpetError, match=words):
        b.label_maps()
    iters = b.run_loop()
    with pytest.raises(L.GpetError, match=words) as ei:  # the loop has run, the final fit has not
        b.label_maps()
    assert ei.value.code == L.ERR_BAD_ARG
    traces = b.finish(iters)
    assert np.array_equal(b.label_maps(), R.trace_maps(traces, (64, 65), [0, 0]))
    b.set_frame(raw_imgs=layered["frames"][1], warm_every=10)
    with pytest.raises(L.GpetError, match=words):  # the fits are those of the frame before
        b.label_maps()
    with pytest.raises(L.GpetError):
        b.results()
    b._batch.close()


def test_a_label_map_in_between_changes_nothing(amd, ctx, layered):
    """Two batches through two frames with a device warm start, one of them asked for maps (to the host and into device memory) after
    each trace: traces, result records and the next frame's warm start are the same to the bit."""
    def run(ask):
        b = amd.GP_Edge_Tracing_Batch(layered["inits"], None, [3, 4], raw_imgs=layered["frames"][0], grad_kernel=layered["K"], return_std=True,
                                      _ctx=ctx, **KW)
        out, buf = [], DeviceBytes(ctx, 64 * 65) if ask else None
        for t in range(2):
            if t:
                b.set_frame(raw_imgs=layered["frames"][t], warm_every=10)
            res = b()
            if ask:
                b.label_maps(thickness=True)
                b.label_maps(out_device_ptrs=[buf.at(0)])
            out.append((res, b.results(), b._batch.read_obs_all(), b.final_costs()))
        if buf is not None:
            buf.free()
        b._batch.close()
        return out

    def same(a, b):
        if isinstance(a, dict):
            return sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
        if isinstance(a, (tuple, list)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return np.array_equal(np.asarray(a), np.asarray(b))
    assert same(run(True), run(False))


def test_an_edge_stopped_with_an_error_contributes_nothing(amd, ctx, layered):
    L = amd._lib
    b = amd.GP_Edge_Tracing_Batch(layered["inits"] * 2, None, [3, 4, 5, 6], raw_imgs=layered["frames"][:2], grad_kernel=layered["K"],
                                  image_of=[0, 0, 1, 1], _ctx=ctx, **KW)
    iters = b.run_loop()
    s = b._batch.scalars(1)
    s.status = L.ERR_STATE
    b._batch.write_scalars(s, 1)
    with pytest.raises(L.GpetError):  # (the fits are made for every edge; the call then reports the stopped edge)
        b.finish(iters)
    traces = b.results()[0]
    got, thick = b.label_maps(thickness=True)
    want = R.trace_maps(traces, (64, 65), [0, -1, 1, 1])  # edge 1 counts nowhere: its map has one boundary left
    assert np.array_equal(got, want) and got[0].max() == 1 and got[1].max() == 2
    assert np.array_equal(thick, R.thick_of(want, 2)) and np.all(thick[0, 2] == 0)
    b._batch.close()


# ---- sequences -----------------------------------------------------------------------------------------------------------------------------
def test_sequence_keeps_the_labels_of_every_frame(amd, ctx, layered):
    frames = layered["frames"][:4]
    st = amd.SequenceTracer(frames, layered["inits"], n_chains=2, warm_every=10, seed=5, grad_kernel=layered["K"],
                            labels=dict(thickness=True), _ctx=ctx, **KW)
    results = st()
    assert len(st.labels) == 4 == len(st.thickness)
    for t in range(4):
        want, thick = amd.gpet_utils.label_maps(results[t], (64, 65), thickness=True, ctx=ctx)
        assert st.labels[t].shape == (64, 65) and np.array_equal(st.labels[t], want[0]), t
        assert np.array_equal(st.labels[t], R.trace_maps(results[t], (64, 65))[0])
        assert st.thickness[t].shape == (3, 65) and np.array_equal(st.thickness[t], thick[0])
    plain = amd.SequenceTracer(frames, layered["inits"], n_chains=2, warm_every=10, seed=5, grad_kernel=layered["K"], _ctx=ctx, **KW)
    assert all(np.array_equal(a, b) for ra, rb in zip(results, plain()) for a, b in zip(ra, rb))  # (the maps change no trace)
    assert plain.labels == [None] * 4
    with pytest.raises(ValueError, match="labels and ensemble_seeds are alternatives"):
        amd.SequenceTracer(frames, layered["inits"], n_chains=2, grad_kernel=layered["K"], labels=True, ensemble_seeds=[1, 2], _ctx=ctx, **KW)
