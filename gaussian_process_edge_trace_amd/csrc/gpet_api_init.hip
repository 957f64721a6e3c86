// C ABI, endpoint tracking (the rule: gpet_init_plan.h, the kernel: gpet_k_init.inc): the init points of a batch
// follow the edge on the images the batch holds now, are set by the caller, or are read back.
#include "gpet_api_internal.h"

// the host copy of the band tables lags behind the device after gpet_batch_init_follow: (i_lo, i_hi) and the inits come home once
int band_refresh_host(gpet_batch* b) {
  BandState& bs = b->band;
  if (!bs.H || !bs.moved) return GPET_OK;
  gpet_ctx* c = b->ctx;
  const BandTables t = band_tables(b->B, bs.n_init_max);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(&bs.h_tab[t.off_lohi], bs.lohi, sizeof(long long) * (t.count - t.off_lohi), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, gpet_wait(c->stream));
  bs.moved = false;
  return GPET_OK;
}

// legal only while no iteration has run since creation, gpet_batch_reset or an image swap
static int init_state_check(gpet_batch* b, const char* who) {
  if (state_missing(b->st, StateEvent::init_moved))
    return fail(b->ctx, GPET_ERR_STATE, "%s: %d iterations have run since the batch was created, reset or given new images; the init points "
                                         "can move only before the first one", who, b->st.iters_issued);
  return GPET_OK;
}

extern "C" {

int gpet_batch_init_xy(gpet_batch* b, int64_t* out) {
  GPET_BATCH_SCOPE(b);
  if (!b || !out) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  // (a banded batch keeps the points in full-frame rows in a table of the same shape; the arena's are in band rows)
  const long long* src = b->band.H ? b->band.init : b->d_init;
  HIPCHK(c, hipMemcpyAsync(out, src, sizeof(long long) * (size_t)b->B * 2 * (size_t)b->n_init_max, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, gpet_wait(c->stream));
  return GPET_OK;
}

int gpet_batch_init_follow(gpet_batch* b, int window, int cols, int64_t* init_out) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  if (const char* why = init_follow_check(window, cols)) return fail(c, GPET_ERR_BAD_ARG, "%s (window = %d, cols = %d)", why, window, cols);
  const int rc = init_state_check(b, "gpet_batch_init_follow");
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  BandState& bs = b->band;
  if (bs.H) {
    HIPCHK(c, launch_init_follow(c->stream, b->d_edges, b->B, window, cols, b->n_init_max, bs.r0, bs.init, bs.lohi));
    bs.moved = true;
  } else {
    HIPCHK(c, launch_init_follow(c->stream, b->d_edges, b->B, window, cols, b->n_init_max, nullptr, nullptr, nullptr));
  }
  state_apply(b->st, StateEvent::init_moved);
  return init_out ? gpet_batch_init_xy(b, init_out) : GPET_OK;
}

int gpet_batch_set_init(gpet_batch* b, const int64_t* const* init_xy) {
  GPET_BATCH_SCOPE(b);
  if (!b || !init_xy) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  const int rc = init_state_check(b, "gpet_batch_set_init");
  if (rc) return rc;
  const int B = b->B;
  const size_t stride = 2 * (size_t)b->n_init_max;
  BandState& bs = b->band;
  const long long M = bs.H ? bs.M : b->bd.M;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, gpet_wait(c->stream));  // (h_init and h_tab may still be the source of an earlier copy)
  std::vector<long long> r0;
  if (bs.H) {  // (the bands the slots are at: placed on the device, so they come home first)
    r0.resize((size_t)B);
    HIPCHK(c, hipMemcpyAsync(r0.data(), bs.r0, sizeof(long long) * (size_t)B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, gpet_wait(c->stream));
  }
  // every refusal before anything is written
  for (int e = 0; e < B; ++e) {
    if (!init_xy[e]) return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_set_init: the init points of edge %d are a null pointer", e);
    for (int i = 0; i < b->h_edges[e].n_init; ++i) {
      const long long x = init_xy[e][2 * i], y = init_xy[e][2 * i + 1], x_is = b->h_init[(size_t)e * stride + 2 * (size_t)i];
      if (x != x_is)
        return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_set_init: init point %d of edge %d has x = %lld, the batch was created with x = %lld "
                                          "(the x of an init point cannot change)", i, e, x, x_is);
      if (y < 0 || y > M - 1)
        return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_set_init: init point %d of edge %d lies outside the frame (row %lld, M = %lld)", i, e, y, M);
      if (bs.H && (y < r0[(size_t)e] || y > r0[(size_t)e] + bs.H - 1))
        return fail(c, GPET_ERR_BAD_ARG, "gpet_batch_set_init: init point %d of edge %d lies outside its band (row %lld, band rows %lld .. "
                                          "%lld)", i, e, y, r0[(size_t)e], r0[(size_t)e] + bs.H - 1);
    }
  }
  for (int e = 0; e < B; ++e)
    for (int i = 0; i < b->h_edges[e].n_init; ++i)
      b->h_init[(size_t)e * stride + 2 * (size_t)i + 1] = init_xy[e][2 * i + 1] - (bs.H ? r0[(size_t)e] : 0);
  HIPCHK(c, hipMemcpyAsync(b->d_init, b->h_init.data(), sizeof(long long) * b->h_init.size(), hipMemcpyHostToDevice, c->stream));
  if (bs.H) {
    const BandTables t = band_tables(B, bs.n_init_max);
    for (int e = 0; e < B; ++e) {
      long long* full = &bs.h_tab[t.off_init + (size_t)e * stride];
      for (int i = 0; i < b->h_edges[e].n_init; ++i) full[2 * i + 1] = init_xy[e][2 * i + 1];
      long long lo = full[1], hi = full[1];
      for (int i = 1; i < b->h_edges[e].n_init; ++i) {
        lo = std::min(lo, full[2 * i + 1]);
        hi = std::max(hi, full[2 * i + 1]);
      }
      bs.h_tab[t.off_lohi + 2 * (size_t)e] = lo;
      bs.h_tab[t.off_lohi + 2 * (size_t)e + 1] = hi;
    }
    HIPCHK(c, hipMemcpyAsync(bs.lohi, &bs.h_tab[t.off_lohi], sizeof(long long) * (t.count - t.off_lohi), hipMemcpyHostToDevice, c->stream));
    bs.moved = false;  // (every row of both tables has just been written from the host copy)
  }
  state_apply(b->st, StateEvent::init_moved);
  HIPCHK(c, gpet_wait(c->stream));
  return GPET_OK;
}

}  // extern "C"
