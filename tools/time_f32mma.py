"""Sample GEMM, scorer and curve KDE of the bench batch at its mid-trace state with f64 samples, f32 storage ("f32") and the GEMM
on the f32 matrix cores ("f32mma"): per-stage times in the order f64, f32, f32mma, f32, f64 at 1 024 and 32 edges (or the counts
given on the command line), then whole GP_Edge_Tracing_Batch.__call__ times of the three modes at the first count.
The output of one run, with the run's conditions, is kept in profiles/r11_f32mma.txt."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gaussian_process_edge_trace_amd as amd
import bench
from bench import synth_image, README_KW
L = amd._lib
ctx = L.Context(0)
counts = [int(a) for a in sys.argv[1:]] or [1024, 32]
N = 500
img, truth = synth_image(N, 3)
init = truth[[0, -1], :][:, [1, 0]]
grad = amd.gpet_utils.comp_grad_img(img, amd.gpet_utils.kernel_builder((11, 5)), ctx=ctx)
ids = dict(bench.KERNEL_IDS_STRUCT); ids.update(bench.KERNEL_IDS_COMMON)
want = [k for k, v in sorted(ids.items()) if any(t in v for t in ("gemm", "score", "kde", "pix", "topk"))]
for E in counts:
    seeds = list(range(1, E + 1))
    print("%d edges, ms per launch of the whole batch (profile_stage, 20 repetitions)" % E, flush=True)
    for dt in ("f64", "f32", "f32mma", "f32", "f64"):
        tr = amd.GP_Edge_Tracing_Batch([init] * E, grad, seeds, **README_KW, _ctx=ctx, sample_dtype=dt)
        tr._batch.iterate(seeds, 7)
        print("%-6s" % dt, "  ".join("%s %.3f" % ("sample_gemm" if k == 130 else ids[k], tr._batch.profile_stage(k, 20)) for k in want), flush=True)
        tr._batch.close()
E = counts[0]
seeds = list(range(1, E + 1))
print("%d edges, whole batch trace (__call__: loop + converged fits), two runs per mode after one warm-up" % E, flush=True)
for dt in ("f64", "f32", "f32mma", "f32mma", "f32", "f64"):
    tr = amd.GP_Edge_Tracing_Batch([init] * E, grad, seeds, **README_KW, _ctx=ctx, sample_dtype=dt)
    tr()
    ts = []
    for rep in range(2):
        tr.reset()
        t0 = time.perf_counter()
        tr()
        ts.append((time.perf_counter() - t0, tr.timings["loop_s"]))
    print("%-6s" % dt, "  ".join("%.3f s = %.0f traces/s (loop %.3f s)" % (s, E / s, ls) for s, ls in ts),
          "iterations %d..%d" % (min(tr.timings["iters"]), max(tr.timings["iters"])), flush=True)
    tr._batch.close()
