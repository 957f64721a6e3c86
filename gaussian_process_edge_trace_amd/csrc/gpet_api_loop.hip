// C ABI, part 5: the device-resident loop (a8) and the dispatch of its normal generators.
#include "gpet_api_internal.h"
#include "gpet_loop_plan.h"
#include "gpet_zstore_plan.h"

#include <mutex>

// One sequential walk per stream: the register-resident generator (four streams per wave, gpet_rng.hip) when the batch is
// homogeneous and the launch has enough streams to fill the GPU with single waves (2 048 = half of its SIMDs; a wave of
// four streams takes ~2.5 ms against 0.6 ms for a three-wave workgroup per stream, so small launches keep the old kernel),
// else one workgroup per stream (k_mt_normals).  The same numbers either way.
hipError_t launch_normals_seq(gpet_batch* b, hipStream_t st, EdgeDev* edges_l, int B_l, const unsigned int* seeds_l,
                              int add_iter, int iter_abs, int n_ahead, int z_store) {
  const int o = opt(Opt::rng4);
  if (b->bd.rng4 && (o > 0 || (o < 0 && (long long)B_l * n_ahead >= 2048)))
    return launch_normals4(st, edges_l, B_l, seeds_l, add_iter, iter_abs, n_ahead, z_store, b->bd.Lg, b->bd.S, b->bd.z_cols);
  return launch_normals(st, edges_l, B_l, seeds_l, add_iter, iter_abs, n_ahead, z_store);
}

// The normals of `n_ahead` iterations of B_l edges: one workgroup per stream (k_mt_normals), or -- when that leaves
// most of the GPU idle and the streams are long -- every stream cut into chunks that many workgroups generate at once
// (MT19937 jump-ahead, launch_normals_chunked).  The same numbers either way.
int normals_auto(gpet_batch* b, hipStream_t st, EdgeDev* edges_l, int B_l, const unsigned int* seeds_l, int add_iter,
                 int iter_abs, int n_ahead, int z_store, bool allow_chunked) {
  gpet_ctx* c = b->ctx;
  if (b->rng_mode == 1) {  // opt-in Philox mode (gpet_batch_set_rng)
    HIPCHK(c, launch_normals_philox(st, edges_l, B_l, b->bd, seeds_l, add_iter, iter_abs, n_ahead, z_store));
    return GPET_OK;
  }
  const int streams = B_l * n_ahead;
  const int nc = mtj_chunks((long long)b->bd.S * b->bd.Lg);
  const int o = opt(Opt::rng_chunked);  // -1: by launch shape
  const bool force4 = opt(Opt::rng4) > 0 && b->bd.rng4;  // (tests: the register-resident generator on any launch shape)
  // (the chunked form works in the batch's ONE jump workspace: a launch that runs beside another chunked launch of the same batch
  //  -- the tail of a small batch's first normals on the fit stream, Loop::normals_side_deep -- must take the sequential kernel)
  const bool chunked = allow_chunked && !force4 && nc >= 2 && (o > 0 || (o < 0 && streams <= 32 && nc >= 4));
  if (!chunked) {
    HIPCHK(c, launch_normals_seq(b, st, edges_l, B_l, seeds_l, add_iter, iter_abs, n_ahead, z_store));
    return GPET_OK;
  }
  const size_t need = mtj_work_bytes(streams, nc);
  if (need > b->mtj_bytes) {
    if (b->mtj_work) {
      HIPCHK(c, hipDeviceSynchronize());  // (launches that use the old workspace may still be in flight)
      (void)hipFree(b->mtj_work);
      b->mtj_work = nullptr;
      b->mtj_bytes = 0;
    }
    HIPCHK(c, hipMalloc(&b->mtj_work, need));
    b->mtj_bytes = need;
  }
  if (!b->d_mtj_poly) {
    HIPCHK(c, hipMalloc(&b->d_mtj_poly, mtj_poly_bytes()));
    HIPCHK(c, hipMemcpy(b->d_mtj_poly, mtj_poly_host(), mtj_poly_bytes(), hipMemcpyHostToDevice));
  }
  HIPCHK(c, launch_normals_chunked(st, edges_l, B_l, seeds_l, add_iter, iter_abs, n_ahead, z_store, b->mtj_work, nc, b->d_mtj_poly));
  return GPET_OK;
}

// A store that a destroyed batch leaves behind is kept for the next batch of the process (one block per process, the largest seen):
// hipMalloc of a store takes ~30 ms per GiB -- 0.3 s for 1 024 edges -- and hipFree as long again, which a caller that creates,
// traces once and destroys a batch per step would pay every step for a store it never reads twice.  With the block kept, that
// caller pays it once per process.  The block is nobody's while it lies here, so it is given back to the device as soon as an
// arena does not find its room (zstore_pool_drain, batch creation).
namespace {
struct ZPool {
  std::mutex mu;  // also: one store at a time in the process (zstore_create)
  void* mem = nullptr;
  size_t bytes = 0;
  int device = -1;
} z_pool;
}  // namespace

void zstore_pool_drain() {
  std::lock_guard<std::mutex> lock(z_pool.mu);
  if (z_pool.mem) (void)hipFree(z_pool.mem);
  z_pool.mem = nullptr;
  z_pool.bytes = 0;
}

void zstore_release(gpet_batch* b) {  // (gpet_batch_destroy, after its streams were waited for)
  ZStore& z = b->zst;
  if (!z.mem) return;
  std::lock_guard<std::mutex> lock(z_pool.mu);
  if (z_pool.mem && (z_pool.bytes >= z.alloc_bytes || z_pool.device != b->ctx->device)) {
    (void)hipFree(z.mem);
  } else {
    if (z_pool.mem) (void)hipFree(z_pool.mem);
    z_pool.mem = z.mem;
    z_pool.bytes = z.alloc_bytes;
    z_pool.device = b->ctx->device;
  }
  z.mem = nullptr;
  z.iters = 0;
}

namespace {

// The batch's normals store, decided once, by its first gpet_trace_iterate (the trace that fills it is the one that would have
// generated anyway; a batch that is created and never traced pays nothing).  A store the budget refuses, or whose allocation
// fails, is no error: the batch runs on its ring alone (gpet_batch_info: zstore_iters == 0).
int zstore_create(gpet_batch* b) {
  gpet_ctx* c = b->ctx;
  ZStore& z = b->zst;
  z.decided = true;
  size_t slot = 0;
  for (const EdgeDev& E : b->h_edges) slot = std::max(slot, (size_t)8 * (size_t)E.S * (size_t)E.z_cols);
  // (one store at a time in the process: batch objects in flight start their first traces together, each on its own host thread,
  //  and a budget taken from the same reading of the free memory by all of them would be no budget)
  std::lock_guard<std::mutex> lock(z_pool.mu);
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
    (void)hipGetLastError();
    return GPET_OK;
  }
  const bool pooled = z_pool.mem && z_pool.device == c->device;  // (the kept block is this process's own: free for this purpose)
  const int iters = zstore_iters(b->B, (long long)slot, (long long)(fr + (pooled ? z_pool.bytes : 0)), (long long)tot, opt(Opt::normals_store),
                                 opt(Opt::normals_store_iters));
  if (iters < 1) return GPET_OK;
  const size_t bytes = (size_t)iters * (size_t)b->B * slot;
  void* mem = nullptr;
  size_t alloc_bytes = bytes;
  if (pooled && z_pool.bytes >= bytes && z_pool.bytes <= 4 * bytes) {  // (a small batch does not sit on a big batch's block)
    mem = z_pool.mem;
    alloc_bytes = z_pool.bytes;
    z_pool.mem = nullptr;
    z_pool.bytes = 0;
  } else {
    if (pooled && z_pool.bytes < bytes) {  // too small: its room goes into the new block
      (void)hipFree(z_pool.mem);
      z_pool.mem = nullptr;
      z_pool.bytes = 0;
    }
    if (hipMalloc(&mem, bytes) != hipSuccess) {
      (void)hipGetLastError();  // (refused by the device: not this call's error)
      return GPET_OK;
    }
  }
  z.mem = (double*)mem;
  z.iters = iters;
  z.slot_bytes = slot;
  z.bytes = bytes;
  z.alloc_bytes = alloc_bytes;
  z.tags.assign((size_t)b->B * iters, 0);
  for (int e = 0; e < b->B; ++e) {
    b->h_edges[e].Zs = z.mem + (size_t)e * iters * (slot / 8);
    b->h_edges[e].zs_iters = iters;
  }
  // (the loop's launches follow on this stream, or wait for ev_main, recorded on it; the compacted tables are copies of h_edges)
  HIPCHK(c, hipMemcpyAsync(b->d_edges, b->h_edges.data(), sizeof(EdgeDev) * (size_t)b->B, hipMemcpyHostToDevice, c->stream));
  return GPET_OK;
}

int read_active(gpet_batch* b, int* active) {  // the edges' state as of now on the host; *active = edges still running
  int rc = check_device_status(b);
  if (rc) return rc;
  *active = 0;
  for (int e = 0; e < b->B; ++e) *active += b->h_scalars[e].done ? 0 : 1;
  return GPET_OK;
}

// One call of gpet_trace_iterate: the batch, the plan and the tables of the group being enqueued.
struct Loop {
  gpet_batch* const b;
  gpet_ctx* const c;
  const uint32_t* const base_seeds;
  const int ring;
  const LoopPlan plan;  // the options, resolved once: the batch's table is installed for the whole call (GPET_BATCH_SCOPE)
  EdgeDev* edges_l;     // the batch's tables, or the compacted ones
  unsigned int* seeds_l;
  int B_l;
  int first = 0, horizon = 0;  // the group's iterations: first <= cur < horizon
  bool fit_used = false;       // the head of a small batch's normals put a launch on the fit stream (this group)
  bool ring_keep = false;      // ring tags are kept by this call (zring_keep: an inline mode, normals_ring_keep != 0, one ring length)
  bool table_running = false;  // the current table holds only edges the host has seen running (from the call's second group on)
  std::vector<unsigned char> miss_buf;  // per entry of the current table: it belongs to the store launch at hand
  std::vector<int> miss_lo, miss_hi;    // per entry of the current table: the store iterations it misses (zstore_misses)

  // The tables of the edges still running.  Every kernel skips finished edges by itself, but it still starts one workgroup per edge
  // and tile to find that out: 2.2 ms per iteration for 1024 finished edges, and the last iterations of a batch run with a handful
  // of edges left.  (The previous group has completed -- check_device_status synchronised -- so the tables may be overwritten.)
  int compact_active() {
    b->h_edges_act.clear();
    b->h_seeds_act.clear();
    b->h_idx_act.clear();
    for (int e = 0; e < b->B; ++e)
      if (!b->h_scalars[e].done) {
        b->h_edges_act.push_back(b->h_edges[e]);
        b->h_seeds_act.push_back(base_seeds[e]);
        b->h_idx_act.push_back(e);
      }
    B_l = (int)b->h_edges_act.size();
    if (!b->d_edges_act) {
      HIPCHK(c, hipMalloc(&b->d_edges_act, sizeof(EdgeDev) * b->B));
      HIPCHK(c, hipMalloc(&b->d_seeds_act, sizeof(unsigned int) * b->B));
    }
    HIPCHK(c, hipMemcpyAsync(b->d_edges_act, b->h_edges_act.data(), sizeof(EdgeDev) * B_l, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b->d_seeds_act, b->h_seeds_act.data(), sizeof(unsigned int) * B_l, hipMemcpyHostToDevice, c->stream));
    edges_l = b->d_edges_act;
    seeds_l = b->d_seeds_act;
    return GPET_OK;
  }

  const int* idx_l() const { return edges_l == b->d_edges ? nullptr : b->h_idx_act.data(); }  // the current table's edges in the batch
  int zs_l() const {  // the columns the generators store of a row (launch_normals*: z_store of 0 or beyond z_cols means all)
    const int z = loop_z_store(b);
    return z > 0 && z < b->bd.z_cols ? z : b->bd.z_cols;
  }
  // One generator launch on st for `count` edges (tab / seeds: device tables; idx: their indices in the batch, nullptr = all B of
  // them), iterations [from, from + n).  The launch is noted and end_group settles it: a launch into the RING skips an edge whose
  // `done` flag is set when it runs, which the host does not know here; a launch into the store always generates (miss_table),
  // but its slots are tagged only once the group has come back without a device error.
  // A launch into the ring empties the tags of the slots it may overwrite HERE, whatever the mode (a side-stream launch, or one
  // under normals_ring_keep = 0, must not leave a stale tag behind for a later trace of the batch that keeps them); keep: its
  // slots get their tags when it is settled, `certain`: for every stream, else for the iterations the edge went on to run.
  int generate(hipStream_t st, EdgeDev* tab, const unsigned int* seeds, const int* idx, int count, int from, int n, bool allow_chunked,
               bool store, bool keep = false, bool certain = false) {
    ZStore& z = b->zst;
    if (!store && z.ring > 0) zring_clear(z.rtags.data(), z.ring, idx, count, from, n);
    int rc = normals_auto(b, st, tab, count, seeds, 1, from, n, loop_z_store(b), allow_chunked);
    if (rc) return rc;
    z.pending.push_back(ZGenLaunch{from, n, store, idx ? std::vector<int>(idx, idx + count) : std::vector<int>(), keep, certain});
    return GPET_OK;
  }
  // One launch on st per distinct range [miss_lo[i], miss_hi[i]] of the current table's entries (a cold trace, a new seed, an
  // injected slot: one), each through a table of its own that always generates (miss_table); `left` = entries with a miss.
  int generate_misses(hipStream_t st, int left, bool allow_chunked, bool store) {
    for (int i0 = 0; i0 < B_l && left > 0; ++i0) {
      const int lo = miss_lo[i0], hi = miss_hi[i0];
      if (lo > hi) continue;
      int count = 0;
      for (int i = 0; i < B_l; ++i) {
        miss_buf[i] = i >= i0 && miss_lo[i] == lo && miss_hi[i] == hi;
        if (miss_buf[i]) {
          count += 1;
          miss_hi[i] = miss_lo[i] - 1;  // (taken)
        }
      }
      left -= count;
      EdgeDev* tab = nullptr;
      unsigned int* sd = nullptr;
      const int* idx = nullptr;
      int rc = miss_table(st, miss_buf.data(), count, &tab, &sd, &idx);
      if (!rc) rc = generate(st, tab, sd, idx, count, lo, hi - lo + 1, allow_chunked, store, !store, !store);
      if (rc) return rc;
    }
    return GPET_OK;
  }
  // A device table of the current table's entries with miss[i] set, for a launch on st into the store (ZStore: segments of one
  // block).  Its entries read their `done` flag from a record of the store's own that never says so: the generators skip finished
  // edges by themselves, and a stream that was enqueued for a store slot and then skipped would leave a slot the host believes
  // filled -- or, untagged, one that every later trace draws again.  (An edge can only finish AFTER the iterations whose normals
  // were enqueued before it did, so what the extra streams cost is what the look-ahead always cost.)
  int miss_table(hipStream_t st, const unsigned char* miss, int count, EdgeDev** tab, unsigned int** seeds, const int** idx) {
    ZStore& z = b->zst;
    const int* cur = idx_l();
    std::vector<int> want;
    want.reserve((size_t)count);
    for (int i = 0; i < B_l; ++i)
      if (miss[i]) want.push_back(cur ? cur[i] : i);
    if (want != z.last_idx || st != z.last_stream) {  // (the same stream: the segment's copy lies before the launch in stream order)
      if (!z.d_edges) {
        z.cap = (size_t)4 * b->B;
        HIPCHK(c, hipMalloc(&z.d_edges, sizeof(EdgeDev) * z.cap));
        HIPCHK(c, hipMalloc(&z.d_seeds, sizeof(unsigned int) * z.cap));
        HIPCHK(c, hipMalloc(&z.d_running, sizeof(gpet_scalars)));
        HIPCHK(c, hipMemset(z.d_running, 0, sizeof(gpet_scalars)));  // done = 0, force = 0, status = GPET_OK
        z.h_edges.resize(z.cap);
        z.h_seeds.resize(z.cap);
      }
      if (z.used + want.size() > z.cap) {  // (rare: the block is full of segments launches may still read)
        HIPCHK(c, gpet_wait(b->side));
        HIPCHK(c, gpet_wait(b->fit));
        HIPCHK(c, gpet_wait(c->stream));
        z.used = 0;
      }
      z.last_off = z.used;
      z.used += want.size();
      for (size_t i = 0; i < want.size(); ++i) {
        z.h_edges[z.last_off + i] = b->h_edges[want[i]];
        z.h_edges[z.last_off + i].sc = z.d_running;
        z.h_seeds[z.last_off + i] = base_seeds[want[i]];
      }
      HIPCHK(c, hipMemcpyAsync(z.d_edges + z.last_off, &z.h_edges[z.last_off], sizeof(EdgeDev) * want.size(), hipMemcpyHostToDevice, st));
      HIPCHK(c, hipMemcpyAsync(z.d_seeds + z.last_off, &z.h_seeds[z.last_off], sizeof(unsigned int) * want.size(), hipMemcpyHostToDevice, st));
      z.last_idx.swap(want);
      z.last_stream = st;
    }
    *tab = z.d_edges + z.last_off;
    *seeds = z.d_seeds + z.last_off;
    *idx = z.last_idx.data();
    return GPET_OK;
  }
  // The normals of iterations [from, from + n) on st, and their events.  The leading iterations that live in the store are
  // generated only for the edges whose tags miss (no edge: no launch -- a trace repeated with the same seeds).  The rest take the
  // ring.  Where ring tags are kept (the inline modes: st is the loop's own stream) the same holds for them; a table that misses
  // the whole range throughout -- a cold trace -- gets its one launch for the current table as ever.  Elsewhere: that launch, always.
  int normals(hipStream_t st, int from, int n, bool allow_chunked = true) {
    ZStore& z = b->zst;
    const int n_st = zstore_span(from, n, z.iters);
    miss_buf.resize((size_t)B_l);
    miss_lo.resize((size_t)B_l);
    miss_hi.resize((size_t)B_l);
    if (n_st > 0) {
      const int left = zstore_misses(z.tags.data(), z.iters, idx_l(), base_seeds, B_l, from, n_st, b->rng_mode, zs_l(), miss_lo.data(), miss_hi.data());
      int rc = generate_misses(st, left, allow_chunked, true);
      if (rc) return rc;
    }
    if (n > n_st) {
      const int rf = from + n_st, rn = n - n_st;
      const bool keep = ring_keep && st == c->stream && rn <= z.ring;
      int left = B_l;
      bool whole = true;  // every entry misses all of [rf, rf + rn)
      if (keep) {
        left = zring_misses(z.rtags.data(), z.ring, idx_l(), base_seeds, B_l, rf, rn, b->rng_mode, zs_l(), miss_lo.data(), miss_hi.data());
        for (int i = 0; i < B_l && whole; ++i) whole = miss_lo[i] == rf && miss_hi[i] == rf + rn - 1;
      }
      int rc = GPET_OK;
      // (the launch lies before the kernels of iteration `from` on the loop's stream: at a group's first iteration, with a table of
      //  edges the host has just seen running, no entry can have finished when it runs -- every stream is generated)
      if (whole) rc = generate(st, edges_l, seeds_l, idx_l(), B_l, rf, rn, allow_chunked, false, keep, keep && table_running && from == first);
      else rc = generate_misses(st, left, allow_chunked, false);
      if (rc) return rc;
    }
    for (int q = from; q < from + n; ++q) HIPCHK(c, hipEventRecord(b->ev_norm[q % 16], st));
    b->st.norm_issued = from + n;
    return GPET_OK;
  }
  // What the group's generator launches did, now that the host has the edges' state and every stream has been waited for.  Store
  // launches generated every stream: their slots get their tags.  normals_generated counts the streams of iterations the edge
  // went on to RUN -- for a finished edge those below its iteration counter: a ring launch may or may not have skipped the ones
  // after, and a store launch drew them ahead for nothing yet.
  void settle_generated() {
    ZStore& z = b->zst;
    const int mode = b->rng_mode, zs = zs_l();
    for (const ZGenLaunch& g : z.pending) {
      const int count = g.idx.empty() ? b->B : (int)g.idx.size();
      for (int i = 0; i < count; ++i) {
        const int e = g.idx.empty() ? i : g.idx[i];
        const gpet_scalars& s = b->h_scalars[e];
        const int end = s.done ? std::min(g.from + g.n, s.iter) : g.from + g.n;
        if (end > g.from) z.generated += end - g.from;
        if (g.store) z.drawn += g.n;  // (a store launch generates every stream it was enqueued for)
        if (g.store)
          for (int q = g.from; q < g.from + g.n && q < z.iters; ++q) z.tags[(size_t)e * z.iters + q] = zstore_loop_tag(base_seeds[e], q, mode, zs);
        if (g.keep) zring_settle(z.rtags.data(), z.ring, e, base_seeds[e], g.from, g.n, s.done, s.iter, g.certain, mode, zs);
      }
    }
    z.pending.clear();
  }
  int normals_inline_iteration(int cur) { return normals(c->stream, cur, 1); }
  int normals_inline_group(int cur) {  // at the group's first iteration (and again where a group is longer than the ring)
    return b->st.norm_issued > cur ? GPET_OK : normals(c->stream, cur, std::min(horizon - cur, ring - 1));
  }
  // The streams of the next n <= look iterations in ONE launch (blockIdx.x = iteration), side by side, whenever at most refill_at are
  // left.  Their ring slots were last read by the sample GEMMs of iterations <= cur - 1 (outstanding + n <= ring).
  int normals_side_deep(int cur) {
    if (b->st.norm_issued - cur > plan.refill_at) return GPET_OK;
    const int j = b->st.norm_issued, n = std::min(ring - (j - cur), plan.look);
    if (cur - 1 >= first) HIPCHK(c, hipStreamWaitEvent(b->side, b->ev_gemm[(cur - 1) % 16], 0));
    // the head of a trace: chunked, one launch per iteration on the side stream, while the sequential launch of the iterations
    // after them runs beside them on the (idle until the converged fits) fit stream
    const int head = head_iterations(plan, j, cur, B_l, b->rng_mode, n);
    for (int q = j; q < j + head; ++q) {
      int rc = normals(b->side, q, 1);
      if (rc) return rc;
    }
    if (head > 0) HIPCHK(c, hipStreamWaitEvent(b->fit, b->ev_main, 0));  // (the seeds and the edge table are on the device)
    // (later refills run on the side stream BESIDE this tail -- different ring slots, and the tail is the sequential kernel,
    //  which has no workspace; the host waits for the fit stream too at the end of the group)
    if (head > 0) fit_used = true;
    return n > head ? normals(head > 0 ? b->fit : b->side, j + head, n - head, head == 0) : GPET_OK;
  }
  // one launch per iteration, `look` iterations ahead of the loop, never past the horizon of the iterations enqueued together
  int normals_side_shallow(int cur) {
    while (b->st.norm_issued <= cur + plan.look && b->st.norm_issued < horizon) {
      const int j = b->st.norm_issued;
      if (plan.look == 0) {
        if (j - 1 >= first) HIPCHK(c, hipStreamWaitEvent(b->side, b->ev_pix[(j - 1) % 16], 0));
      } else if (j - ring >= first) {
        HIPCHK(c, hipStreamWaitEvent(b->side, b->ev_gemm[(j - ring) % 16], 0));
      }
      int rc = normals(b->side, j, 1);
      if (rc) return rc;
    }
    return GPET_OK;
  }

  // the kernel chain of iteration cur (every kernel skips edges whose `done` flag is set, so edges that finish inside a group cost little)
  int enqueue_iteration(int cur) {
    if (b->structured) {
      HIPCHK(c, launch_struct_iteration(c->stream, edges_l, B_l, b->bd));
    } else {
      HIPCHK(c, launch_fit_predict(c->stream, edges_l, B_l, b->bd, 1));
      HIPCHK(c, launch_factor(c->stream, edges_l, B_l, b->bd, ~0u, edges_l == b->d_edges ? b->h_edges.data() : b->h_edges_act.data()));
    }
    HIPCHK(c, hipStreamWaitEvent(c->stream, b->ev_norm[cur % 16], 0));
    // samples + scores: the GEMM writes all S rows and the scorer reads them back (two fused forms that never wrote the sample
    // matrix were built in rounds 3 and 4, bit-identical, and measured slower: an f64 matrix instruction and f64 vector
    // work do not overlap, DESIGN.md history)
    HIPCHK(c, launch_sample(c->stream, edges_l, B_l, b->bd, b->structured ? b->bd.r0_max : 0));
    HIPCHK(c, hipEventRecord(b->ev_gemm[cur % 16], c->stream));  // ring slot cur % ring may be refilled
    // loop form: the density stays raw and band-limited in HBM; the pixel kernels normalise on the fly
    if (plan.fused_tail) {
      HIPCHK(c, launch_score_kde_fused_tail(c->stream, edges_l, B_l, b->bd));
    } else {
      HIPCHK(c, launch_score(c->stream, edges_l, B_l, b->bd));
      HIPCHK(c, launch_kde(c->stream, edges_l, B_l, b->bd, 0, ~0u, 1));
    }
    HIPCHK(c, launch_pixels(c->stream, edges_l, B_l, b->bd, 1));
    HIPCHK(c, hipEventRecord(b->ev_pix[cur % 16], c->stream));
    // opt-in history: the record of this iteration for the edges that completed it (their counter is now iters_issued + 1)
    if (b->d_hist) HIPCHK(c, launch_history(c->stream, edges_l, B_l, b->hist, b->st.iters_issued + 1));
    state_apply(b->st, StateEvent::iteration_enqueued);
    return GPET_OK;
  }

  // waits for the group (n_it iterations, of `group` planned), reads the edges' state and sizes the next group (*next = 0: stop)
  int end_group(int group, int n_it, int* active, int* next) {
    state_apply(b->st, StateEvent::group_end);
    HIPCHK(c, gpet_wait(b->side));  // (its launches read the compacted tables too)
    if (fit_used) HIPCHK(c, gpet_wait(b->fit));
    fit_used = false;
    int rc = read_active(b, active);
    if (rc) return rc;
    settle_generated();
    table_running = true;  // (the next group's table: all B edges if all are running, else the compacted one)
    EdgeProgress prog[64];  // (next_group looks at the edges of a batch of up to 64 only)
    const int count = b->B <= 64 && *active > 0 ? b->B : 0;
    if (count && (int)b->h_nobs_prev.size() != b->B) b->h_nobs_prev.assign(b->B, 0);
    for (int e = 0; e < count; ++e) {
      prog[e] = {b->h_scalars[e].done, b->h_scalars[e].n_obs, b->h_nobs_prev[e], b->h_edges[e].algo_thresh};
      b->h_nobs_prev[e] = prog[e].n_obs;  // (of finished edges too)
    }
    *next = next_group(b->B, group, n_it, *active, prog, count);
    return GPET_OK;
  }
};

}  // namespace

extern "C" {

int gpet_trace_iterate(gpet_batch* b, const uint32_t* base_seeds, int max_iters, int* n_active) {
  GPET_BATCH_SCOPE(b);
  if (!b || !base_seeds || !n_active || max_iters < 0) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  state_apply(b->st, StateEvent::trace_entry);  // (another trace is under way: d_fin_out belongs to the one before until its own converged fit)
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(b->d_seeds, base_seeds, sizeof(uint32_t) * b->B, hipMemcpyHostToDevice, c->stream));
  b->h_seeds_dev.assign(base_seeds, base_seeds + b->B);
  *n_active = b->B;
  if (max_iters == 0) return read_active(b, n_active);
  LoopPlan plan = resolve_loop_plan(b->B, b->bd.z_ring, opt(Opt::rng_lookahead), opt(Opt::rng_inline), opt(Opt::rng_refill_at),
                                    opt(Opt::rng_head), opt(Opt::loop_fused_tail));
  plan.fused_tail = plan.fused_tail && score_tail_applies(b->bd);
  if (!b->zst.decided) {
    const int rc_z = zstore_create(b);
    if (rc_z) return rc_z;
  }
  b->zst.pending.clear();  // (of a call that ended in an error: its slots stay untagged)
  b->zst.last_idx.clear();
  b->zst.used = 0;         // (every launch of the call before has completed: end_group waited for the three streams)
  if (b->zst.rtags.empty()) {  // ring tags, once per batch: host memory only (edges whose rings differ in length: none)
    bool one = b->bd.z_ring > 0 && b->bd.z_ring <= kZRingMax;
    for (const EdgeDev& E : b->h_edges) one = one && E.z_ring == b->bd.z_ring;
    b->zst.ring = one ? b->bd.z_ring : 0;
    b->zst.rtags.assign((size_t)b->B * (size_t)(one ? b->bd.z_ring : 1), 0);
  }
  Loop l{b, c, base_seeds, b->bd.z_ring, plan, b->d_edges, b->d_seeds, b->B};
  l.ring_keep = zring_keep(opt(Opt::normals_ring_keep), plan.mode == NormalsMode::inline_per_iteration || plan.mode == NormalsMode::inline_per_group,
                           b->zst.ring);
  // Groups of iterations (next_group): after every group the host reads the `done` flags, stops if no edge is left and otherwise
  // enqueues the next group for the edges still running.
  for (int remaining = max_iters, group = 8; remaining > 0 && group > 0;) {
    const int n_it = std::min(group, remaining);
    int rc = *n_active < b->B ? l.compact_active() : GPET_OK;
    if (rc) return rc;
    l.first = b->st.iters_issued;
    l.horizon = l.first + n_it;
    if (b->st.norm_issued < l.first) b->st.norm_issued = l.first;
    HIPCHK(c, hipEventRecord(b->ev_main, c->stream));  // the seeds and the edge table are on the device
    HIPCHK(c, hipStreamWaitEvent(b->side, b->ev_main, 0));
    for (int cur = l.first; cur < l.horizon && !rc; ++cur) {
      switch (plan.mode) {
        case NormalsMode::inline_per_iteration: rc = l.normals_inline_iteration(cur); break;
        case NormalsMode::inline_per_group: rc = l.normals_inline_group(cur); break;
        case NormalsMode::side_deep: rc = l.normals_side_deep(cur); break;
        case NormalsMode::side_shallow: rc = l.normals_side_shallow(cur); break;
      }
      if (!rc) rc = l.enqueue_iteration(cur);
    }
    if (!rc) rc = l.end_group(group, n_it, n_active, &group);
    if (rc) return rc;
    remaining -= n_it;
  }
  return GPET_OK;
}

}  // extern "C"
