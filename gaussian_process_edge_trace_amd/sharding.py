"""Sharding of independent edges over the GPUs of one node.

Edges share no state, so the partition is embarrassingly parallel: rank r traces a contiguous
block of edges; the only exchanges are one broadcast of the shared gradient image from rank 0
(RCCL over xGMI when the backend is "nccl") and one gather of the finished traces.  No
per-iteration collective exists.  The same code runs under "gloo" on CPU tensors (tests).

A tracer may return bare (L_e, 2) traces or ``(trace, (lower, upper))`` tuples (``return_std=True``), and edges may have
different lengths (L_e from each edge's own init).  Uniform bare traces come back as one (n, L, 2) ndarray; anything else
as a list of per-edge results of the tracer's own form, trimmed to L_e, in global order and identical on every rank.
"""
from __future__ import annotations

import numpy as np


def edge_slice(n_edges, world, rank):
    """Contiguous block [lo, hi) of edge indices owned by ``rank`` (sizes differ by at most 1)."""
    base, rem = divmod(int(n_edges), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def broadcast_tensor(arr, shape, dtype, dist, src=0, device="cpu"):
    """Broadcast a numpy array from ``src`` to every rank; returns the torch tensor the collective filled (on
    ``device``: with backend "nccl" that is this rank's GPU, and the tracer consumes it in place through
    ``tensor.data_ptr()`` -- gpet_batch_create2 / GPET_GRAD_ON_DEVICE -- with no trip through host memory)."""
    import torch
    t = torch.empty(tuple(shape), dtype=getattr(torch, np.dtype(dtype).name), device=device)
    if dist.get_rank() == src:
        t.copy_(torch.from_numpy(np.ascontiguousarray(arr, dtype=dtype)))
    dist.broadcast(t, src=src)
    if t.is_cuda:
        # the collective (and rank src's host-to-device copy) only order torch's current stream; the tracer reads the
        # tensor on the library's own HIP stream through data_ptr(): wait here, once, before handing it out
        torch.cuda.current_stream(t.device).synchronize()
    return t


def broadcast_array(arr, shape, dtype, dist, src=0, device="cpu"):
    """Broadcast a numpy array from ``src`` to every rank; returns it as numpy on all ranks."""
    return broadcast_tensor(arr, shape, dtype, dist, src, device).cpu().numpy()


def gather_traces(local, n_edges, edge_len, dist, device="cpu"):
    """All ranks contribute their (n_local, edge_len, 2) int64 traces; every rank gets the
    (n_edges, edge_len, 2) array in global edge order."""
    import torch
    world, rank = dist.get_world_size(), dist.get_rank()
    cap = max(edge_slice(n_edges, world, r)[1] - edge_slice(n_edges, world, r)[0] for r in range(world))
    buf = torch.zeros((cap, edge_len, 2), dtype=torch.int64, device=device)
    loc = np.asarray(local, dtype=np.int64).reshape(-1, edge_len, 2)
    if loc.shape[0]:
        buf[:loc.shape[0]].copy_(torch.from_numpy(loc))
    parts = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(parts, buf)
    out = []
    for r in range(world):
        lo, hi = edge_slice(n_edges, world, r)
        out.append(parts[r][:hi - lo].cpu().numpy())
    return np.concatenate(out, axis=0)


def init_edge_len(init):
    """Points of an edge's x-grid from its init: abs(x_en - x_st) + 1 of the first and last rows."""
    return int(abs(int(init[-1][0]) - int(init[0][0])) + 1)


def _with_ci(result):
    """True for a ``(trace, (lower, upper))`` result (``return_std=True``), False for a bare trace."""
    return isinstance(result, tuple)


def _assemble(results, lens):
    """The single-process return value: uniform bare traces stacked into one ndarray, anything else a list."""
    results = list(results)
    if not any(_with_ci(r) for r in results) and len(set(lens)) <= 1:
        return np.stack(results) if results else np.zeros((0, lens[0] if lens else 0, 2), dtype=np.int64)
    return results


def _agree_with_ci(local, dist, device):
    """Whether the tracer returns intervals: a rank with no edges cannot see it, so the ranks agree (all_reduce MAX)."""
    import torch
    flag = torch.tensor([1 if any(_with_ci(r) for r in local) else 0], dtype=torch.int64, device=device)
    dist.all_reduce(flag, op=dist.ReduceOp.MAX)
    return bool(flag.item())


def gather_results(local, blocks, lens, with_ci, dist, device="cpu"):
    """All ranks contribute the results of their block (``blocks[r]`` = [lo, hi) of rank r, contiguous and in rank order;
    ``lens[u]`` = points of unit u): int64 traces and, ``with_ci``, f64 (lower, upper), each padded to the longest unit
    and the longest block.  Every rank gets the list of results in global order, trimmed to each unit's length."""
    import torch
    world, rank = dist.get_world_size(), dist.get_rank()
    cap = max(hi - lo for lo, hi in blocks)
    L = max(lens) if len(lens) else 0
    lo, hi = blocks[rank]
    if len(local) != hi - lo:
        raise ValueError("tracer returned %d results for a block of %d" % (len(local), hi - lo))
    tr = np.zeros((cap, L, 2), dtype=np.int64)
    ci = np.zeros((cap, 2, L), dtype=np.float64) if with_ci else None
    for i, r in enumerate(local):
        t = np.asarray(r[0] if _with_ci(r) else r)
        if t.shape != (lens[lo + i], 2):
            raise ValueError("result %d has shape %s, its init gives (%d, 2)" % (lo + i, t.shape, lens[lo + i]))
        tr[i, :t.shape[0]] = t
        if with_ci:
            ci[i, 0, :t.shape[0]], ci[i, 1, :t.shape[0]] = r[1][0], r[1][1]
    bufs = [torch.from_numpy(tr).to(device)] + ([torch.from_numpy(ci).to(device)] if with_ci else [])
    parts = []
    for b in bufs:
        p = [torch.empty_like(b) for _ in range(world)]
        dist.all_gather(p, b)
        parts.append([q.cpu().numpy() for q in p])
    out = []
    for r, (a, b) in enumerate(blocks):
        for i in range(b - a):
            n_pts = lens[a + i]
            t = parts[0][r][i, :n_pts]
            out.append((t, (parts[1][r][i, 0, :n_pts], parts[1][r][i, 1, :n_pts])) if with_ci else t)
    return out


def trace_sharded(grad, grad_shape, inits, seeds, tracer, dist=None, device="cpu"):
    """Trace ``len(inits)`` independent edges of one shared gradient image across all ranks.

    ``grad`` is needed on rank 0 only.  ``tracer(grad, inits_block, seeds_block)`` returns the
    list of results of its block -- (L_e, 2) traces, or (trace, (lower, upper)) tuples -- (GP_Edge_Tracing_Batch on a GPU;
    tests pass a CPU callable).  Returns on every rank, in global order, the (n_edges, edge_len, 2) traces when they are
    bare and of one length, else the list of per-edge results (module docstring)."""
    n = len(inits)
    lens = [init_edge_len(i) for i in inits]
    if dist is None or dist.get_world_size() == 1:
        return _assemble(tracer(grad, list(inits), list(seeds)), lens)
    world, rank = dist.get_world_size(), dist.get_rank()
    g = broadcast_tensor(grad, grad_shape, np.float32, dist, 0, device)
    # on a GPU the tracer gets the device tensor itself (it passes data_ptr() to the library); on CPU, numpy
    grad = g if str(g.device).startswith("cuda") else g.numpy()
    lo, hi = edge_slice(n, world, rank)
    local = list(tracer(grad, list(inits[lo:hi]), list(seeds[lo:hi]))) if hi > lo else []
    with_ci = _agree_with_ci(local, dist, device)
    if not with_ci and len(set(lens)) == 1:
        return gather_traces(local, n, lens[0], dist, device)
    return gather_results(local, [edge_slice(n, world, r) for r in range(world)], lens, with_ci, dist, device)


def trace_sharded_cabi(grad, grad_shape, inits, seeds, comm, with_stats=False, **ctor_kwargs):
    """``trace_sharded`` with no torch in the process: the C ABI's own RCCL call sites (``_lib.Comm``: gpet_comm_create,
    gpet_bcast_grad, gpet_gather_traces / gpet_gather_results; include/gpet_hip.h "collectives") -- what a non-Python host
    of the reference would call.  ``grad`` is needed on rank 0 only; the broadcast image is consumed where RCCL put it
    (device pointer -> gpet_batch_create2 / GPET_GRAD_ON_DEVICE).  Returns on every rank, in global order, what
    ``trace_sharded`` returns: the (n_edges, edge_len, 2) traces when they are bare and of one length, else the list of
    per-edge results.  With ``return_std=True`` in ``ctor_kwargs``, edges of different lengths or ``with_stats``, the
    gather moves the result records the device packed from the converged fits (gpet_gather_results); ``with_stats``
    returns (results, dict(n_iter, n_obs, theta, nlml)) with one entry per edge."""
    from .gpet import GP_Edge_Tracing_Batch, results_from_records
    n = len(inits)
    lens = [init_edge_len(i) for i in inits]
    return_std = bool(ctor_kwargs.get("return_std", False))
    ptr = comm.bcast_grad(grad, grad_shape, root=0)
    lo, hi = comm.block(n)
    tr = None
    if hi > lo:
        tr = GP_Edge_Tracing_Batch(list(inits[lo:hi]), None, list(seeds[lo:hi]), grad_device_ptrs=[ptr],
                                   grad_shape=tuple(grad_shape), _ctx=comm.ctx, **ctor_kwargs)
    uniform = len(set(lens)) <= 1
    if uniform and not return_std and not with_stats:
        return comm.gather_traces(tr() if tr is not None else [], n, lens[0] if lens else 0)
    if tr is not None:
        tr.final_fits(tr.run_loop())  # (the records are packed on the device from the converged fits)
    out, stats = results_from_records(comm.gather_results(tr._batch if tr is not None else None, n, max(lens, default=0)),
                                      return_std)
    if uniform and not return_std:
        out = np.stack(out) if out else np.zeros((0, lens[0] if lens else 0, 2), dtype=np.int64)
    return (out, stats) if with_stats else out


def sequence_partition(n_frames, n_chains, world, rank):
    """Frames of an image sequence owned by ``rank``: the sequence is cut into ``n_chains`` chains of consecutive
    frames (``sequence.chain_slices``; the first frame of a chain starts cold, later ones warm-start from the
    previous trace), and whole chains are dealt to the ranks in contiguous blocks like independent edges.
    Returns (first_frame, last_frame_exclusive, number_of_local_chains)."""
    from .sequence import chain_slices
    chains = chain_slices(n_frames, n_chains)
    lo, hi = edge_slice(len(chains), world, rank)
    if hi <= lo:
        return 0, 0, 0
    return chains[lo][0], chains[hi - 1][1], hi - lo


def trace_sequence_sharded(frames, frame_shape, n_frames, init, n_chains, tracer, dist=None, device="cpu"):
    """Trace one edge through ``n_frames`` gradient images in ``n_chains`` chains spread over all ranks
    (BASELINE config 5: 64 frames, 8 chains, 8 GPUs).  ``frames`` ((T, M, N) float32) is needed on rank 0 only and is
    broadcast once; ``tracer(frames_block, first_frame, n_local_chains)`` returns the (edge_len, 2) traces of a
    contiguous block of frames that consists of whole chains (bare traces, or (trace, (lower, upper)) tuples).  Every
    rank gets the (T, edge_len, 2) traces when they are bare, else the list of T per-frame results."""
    edge_len = init_edge_len(init)
    if dist is None or dist.get_world_size() == 1:
        return _assemble(tracer(frames, 0, min(int(n_chains), int(n_frames))), [edge_len] * int(n_frames))
    world, rank = dist.get_world_size(), dist.get_rank()
    t = broadcast_tensor(frames, (n_frames,) + tuple(frame_shape), np.float32, dist, 0, device)
    f0, f1, nc = sequence_partition(n_frames, n_chains, world, rank)
    block = t[f0:f1] if str(t.device).startswith("cuda") else t[f0:f1].numpy()
    local = list(tracer(block, f0, nc)) if nc else []
    with_ci = _agree_with_ci(local, dist, device)
    if not with_ci:
        # gather: frame blocks are contiguous and in rank order, but of different lengths -> pad to the longest
        import torch
        sizes = [sequence_partition(n_frames, n_chains, world, r) for r in range(world)]
        cap = max(b - a for a, b, _ in sizes)
        buf = torch.zeros((cap, edge_len, 2), dtype=torch.int64, device=device)
        loc = np.asarray(local, dtype=np.int64).reshape(-1, edge_len, 2)
        if loc.shape[0]:
            buf[:loc.shape[0]].copy_(torch.from_numpy(loc))
        parts = [torch.empty_like(buf) for _ in range(world)]
        dist.all_gather(parts, buf)
        return np.concatenate([parts[r][:sizes[r][1] - sizes[r][0]].cpu().numpy() for r in range(world)], axis=0)
    blocks = [sequence_partition(n_frames, n_chains, world, r)[:2] for r in range(world)]  # (an idle rank's is empty)
    return gather_results(local, blocks, [edge_len] * int(n_frames), True, dist, device)
