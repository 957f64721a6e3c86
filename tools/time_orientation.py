"""What a vertical batch costs in a frame change, against the horizontal batch on the same frames and against the host route it
replaces: 256 uint8 frames of 500 x 500, one per edge of a 256-edge batch, the (11, 5) kernel.

  python tools/time_orientation.py [--edges 256] [--size 500] [--changes 5] [--out FILE]
      Per case one batch traces nothing; per frame change, wall clock in ms around calls that end with a wait:
        horizontal   set_frame(raw_imgs=frames) on a horizontal batch: upload, convolution (k_conv_relu_batch), in-place normaliser,
                     gradient KDE, reset
        vertical     the same call on an orientation='vertical' batch: the convolution stores transposed (k_conv_tr_batch, the
                     16 x 64 tile of csrc/gpet_transpose_plan.h), everything else is the same code on the N x M images
        host route   what a caller with host frames had to do: comp_grad_imgs home, .transpose(0, 2, 1).copy(), then
                     set_frame(grad_imgs=...) on a horizontal batch of the transposed shape
      medians with min - max over the frame changes, after one change that is not timed.  The same frames on the device
      (raw_device_ptrs) for the first two cases, where the upload is not in the way of the kernels.  Then, from
      gpet_profile_stage (events on the stream, 20 repetitions): k_normalise_f32_batch alone over the batch's 256 images -- one more
      read and write of every pixel, the yardstick the store side is read against: vertical should cost no more than horizontal
      plus that.  Only the 16 x 64 store layout is built; the LDS-staged 64 x 16 layout is not, so there is no second
      column.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KW = dict(kernel_options={'kernel': 'RBF', 'sigma_f': 20, 'length_scale': 40}, noise_y=1, N_samples=500, score_thresh=1, delta_x=10,
          keep_ratio=0.1, pixel_thresh=5, fix_endpoints=True)


class DeviceFrames(object):
    """Frames copied into device memory of the context (gpet_dev_alloc / gpet_dev_copy); ``ptrs`` are their addresses."""

    def __init__(self, ctx, frames):
        self.ctx, self.ptrs = ctx, []
        for f in frames:
            f = np.ascontiguousarray(f)
            d = C.c_void_p()
            ctx.check(ctx.lib.gpet_dev_alloc(ctx.h, f.nbytes, C.byref(d)))
            ctx.check(ctx.lib.gpet_dev_copy(ctx.h, d, f.ctypes.data, f.nbytes, 0))
            self.ptrs.append(d.value)

    def free(self):
        for p in self.ptrs:
            self.ctx.lib.gpet_dev_free(self.ctx.h, C.c_void_p(p))
        self.ptrs = []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--edges", type=int, default=256)
    ap.add_argument("--size", type=int, default=500)
    ap.add_argument("--changes", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gaussian_process_edge_trace_amd as pkg
    L = pkg._lib
    ctx = L.Context(0)
    B, S = a.edges, a.size
    K = pkg.gpet_utils.kernel_builder((11, 5))
    rng = np.random.default_rng(11)
    sets = [rng.integers(0, 256, size=(B, S, S), dtype=np.uint8) for _ in range(2)]  # two sets of frames, alternated
    init_h = np.array([[0, S // 2], [S - 1, S // 2]], dtype=np.int64)
    seeds = list(range(3, 3 + B))
    med = lambda v: "%9.3f (%.3f - %.3f)" % (np.median(v), min(v), max(v))

    def timed(call):
        ctx.sync()
        t0 = time.perf_counter()
        call()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    hb = pkg.GP_Edge_Tracing_Batch([init_h] * B, None, seeds, raw_imgs=sets[0], grad_kernel=K, _ctx=ctx, **KW)
    vb = pkg.GP_Edge_Tracing_Batch([init_h[:, ::-1]] * B, None, seeds, raw_imgs=sets[0], grad_kernel=K, orientation='vertical', _ctx=ctx,
                                   **KW)
    gb = pkg.GP_Edge_Tracing_Batch([init_h] * B, list(pkg.gpet_utils.comp_grad_imgs(sets[0], K, ctx=ctx).transpose(0, 2, 1).copy()), seeds,
                                   _ctx=ctx, **KW)

    def host_route(frames):
        G = pkg.gpet_utils.comp_grad_imgs(frames, K, ctx=ctx)
        gb.set_frame(list(G.transpose(0, 2, 1).copy()), next_frame=False)

    cases = [("horizontal", lambda f: hb.set_frame(raw_imgs=f, next_frame=False)),
             ("vertical", lambda f: vb.set_frame(raw_imgs=f, next_frame=False)),
             ("host route", host_route)]
    times = {name: [] for name, _ in cases}
    for r in range(a.changes + 1):  # (the first change is the warm-up; the cases alternate)
        for name, call in cases:
            ms = timed(lambda: call(sets[(r + 1) % 2]))
            if r:
                times[name].append(ms)
    # the transposed store writes what the horizontal store writes, transposed
    for e in (0, B - 1):
        assert np.array_equal(vb._batch.read(L.BUF_GRAD, e), hb._batch.read(L.BUF_GRAD, e).T)
        assert np.array_equal(vb._batch.read(L.BUF_GRAD, e), gb._batch.read(L.BUF_GRAD, e))
    dev = [DeviceFrames(ctx, s) for s in sets]
    dtimes = {"horizontal": [], "vertical": []}
    for r in range(a.changes + 1):
        for name, bt in (("horizontal", hb), ("vertical", vb)):
            ms = timed(lambda: bt.set_frame(raw_device_ptrs=dev[(r + 1) % 2].ptrs, raw_dtype=np.uint8, next_frame=False))
            if r:
                dtimes[name].append(ms)
    for d in dev:
        d.free()
    norm_h, norm_v = hb._batch.profile_stage(170, 20), vb._batch.profile_stage(170, 20)
    lines = ["set_frame of %d distinct %d x %d uint8 frames on a %d-edge batch, kernel (11, 5), next_frame=False; ms, median (min - max) "
             "over %d frame changes after one that is not timed" % (B, S, S, B, a.changes),
             "host frames (raw_imgs):",
             "  horizontal   %s" % med(times["horizontal"]),
             "  vertical     %s" % med(times["vertical"]),
             "  host route   %s   (comp_grad_imgs home, .transpose(0, 2, 1).copy(), set_frame(grad_imgs=...))" % med(times["host route"]),
             "frames on the device (raw_device_ptrs):",
             "  horizontal   %s" % med(dtimes["horizontal"]),
             "  vertical     %s" % med(dtimes["vertical"]),
             "k_normalise_f32_batch alone over the %d images (gpet_profile_stage 170, 20 repetitions): %.3f ms on the horizontal batch, "
             "%.3f ms on the vertical one" % (B, norm_h, norm_v),
             "vertical - horizontal: %+.3f ms with host frames, %+.3f ms with device frames (medians); the yardstick is +%.3f ms"
             % (np.median(times["vertical"]) - np.median(times["horizontal"]),
                np.median(dtimes["vertical"]) - np.median(dtimes["horizontal"]), norm_h),
             "store layouts built: the 16 x 64 tile (frame columns x frame rows, 256-byte runs) only"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    for bt in (hb, vb, gb):
        bt._batch.close()


if __name__ == "__main__":
    main()
