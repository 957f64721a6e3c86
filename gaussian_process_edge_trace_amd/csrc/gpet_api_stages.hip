// C ABI, part 3: the per-stage entry points (a2-a7, f1) and gpet_profile_stage.
#include "gpet_api_internal.h"
#include "gpet_zstore_plan.h"

// ---- stages ---------------------------------------------------------------------------
// What the per-stage entry points share once nothing refuses: the stage's launches with every edge made to run it (launch_set_force
// around them), then the event; status: the edges' device status is read back and reported
template <class Launches>
static int forced_stage(gpet_batch* b, StateEvent ev, bool status, Launches launches) {
  gpet_ctx* c = b->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, launch_set_force(c->stream, b->d_edges, b->B, 1));
  const int rc = launches();
  if (rc) return rc;
  HIPCHK(c, launch_set_force(c->stream, b->d_edges, b->B, 0));
  state_apply(b->st, ev);
  return status ? check_device_status(b) : GPET_OK;
}

// The one body of the three pixel-selection entry points, behind their refusals.  kde: the curve KDE first (else the selection
// runs on the density GPET_BUF_KDE holds); raw_band: the form the device loop runs after its scorer (enqueue_iteration) -- the
// density stays raw and band-limited in GPET_BUF_KDE, rows outside a tile's band keep what they held, the pixel kernels normalise
// on the fly
static int select_pixels(gpet_batch* b, StateEvent begin, bool kde, int raw_band) {
  gpet_ctx* c = b->ctx;
  state_apply(b->st, begin);  // (a new observation set: another trace)
  // (k_pix_select advances every active edge's iteration counter)
  return forced_stage(b, StateEvent::iteration_enqueued, true, [&]() -> int {
    if (kde) HIPCHK(c, launch_kde(c->stream, b->d_edges, b->B, b->bd, 0, ~0u, raw_band));
    else HIPCHK(c, launch_pixels_reset(c->stream, b->d_edges, b->B, b->bd));
    HIPCHK(c, launch_pixels(c->stream, b->d_edges, b->B, b->bd, raw_band));
    return GPET_OK;
  });
}

extern "C" {

int gpet_gp_fit_predict(gpet_batch* b, int want_cov) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  return forced_stage(b, StateEvent::stage_fit, true, [&]() -> int {
    HIPCHK(c, launch_fit_predict(c->stream, b->d_edges, b->B, b->bd, want_cov));
    return GPET_OK;
  });
}

int gpet_gp_factor(gpet_batch* b) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  if (state_missing(b->st, StateEvent::stage_factor)) return fail(c, GPET_ERR_STATE, "gpet_gp_factor before gpet_gp_fit_predict");
  return forced_stage(b, StateEvent::stage_factor, true, [&]() -> int {
    HIPCHK(c, launch_factor(c->stream, b->d_edges, b->B, b->bd, ~0u, b->h_edges.data()));
    return GPET_OK;
  });
}

int gpet_gp_normals(gpet_batch* b, const uint32_t* seeds) {
  GPET_BATCH_SCOPE(b);
  if (!b || !seeds) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(b->d_seeds, seeds, sizeof(uint32_t) * b->B, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch_set_force(c->stream, b->d_edges, b->B, 1));
  {
    int rcn = normals_auto(b, c->stream, b->d_edges, b->B, b->d_seeds, 0, -1, 1, 0);
    if (rcn) return rcn;
  }
  b->h_seeds_dev.assign(seeds, seeds + b->B);
  HIPCHK(c, launch_set_force(c->stream, b->d_edges, b->B, 0));
  HIPCHK(c, gpet_wait(c->stream));
  if (b->zst.iters > 0 || b->zst.ring > 0) {
    // the slot z_slot names at every edge's own iteration -- of the store or of the ring -- now holds the stream of the seed the
    // caller named, every column of it: its tag says so (the loop finds it where seed + iteration + 1 is that seed).  An edge in
    // an error state was skipped
    const int rcs = fetch_all_scalars(b);
    if (rcs) return rcs;
    for (int e = 0; e < b->B; ++e) {
      const gpet_scalars& s = b->h_scalars[e];
      if (s.status != GPET_OK) continue;
      if (uint64_t* t = zstore_tag_at(b->zst, e, s.iter)) *t = zstore_tag(seeds[e], b->rng_mode, b->bd.z_cols);
    }
  }
  state_apply(b->st, StateEvent::stage_normals);
  return GPET_OK;
}

int gpet_gp_sample(gpet_batch* b) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  if (state_missing(b->st, StateEvent::stage_sample))
    return fail(c, GPET_ERR_STATE, "gpet_gp_sample needs fit, factor and normals first");
  return forced_stage(b, StateEvent::stage_sample, false, [&]() -> int {
    HIPCHK(c, launch_sample(c->stream, b->d_edges, b->B, b->bd));
    return GPET_OK;
  });
}

int gpet_score_curves(gpet_batch* b) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  if (state_missing(b->st, StateEvent::stage_score)) return fail(c, GPET_ERR_STATE, "gpet_score_curves before samples exist");
  return forced_stage(b, StateEvent::stage_score, false, [&]() -> int {
    HIPCHK(c, launch_score(c->stream, b->d_edges, b->B, b->bd));
    return GPET_OK;
  });
}

int gpet_curve_kde(gpet_batch* b) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  if (state_missing(b->st, StateEvent::stage_kde)) return fail(c, GPET_ERR_STATE, "gpet_curve_kde before gpet_score_curves");
  return forced_stage(b, StateEvent::stage_kde, true, [&]() -> int {
    HIPCHK(c, launch_kde(c->stream, b->d_edges, b->B, b->bd, 0));
    return GPET_OK;
  });
}

int gpet_final_cov(gpet_batch* b) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  for (int e = 0; e < b->B; ++e)
    if (b->h_edges[e].fin_n < 1) return fail(c, GPET_ERR_STATE, "gpet_final_cov before gpet_final_predict_all");
  HIPCHK(c, launch_final_cov(c->stream, b->d_edges, b->B, b->bd));
  HIPCHK(c, gpet_wait(c->stream));
  state_apply(b->st, StateEvent::final_cov);  // (mean in the caller's hands, covariance in GPET_BUF_COV: gpet_gp_factor may follow)
  return GPET_OK;
}

int gpet_select_pixels(gpet_batch* b) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  if (state_missing(b->st, StateEvent::select_pixels)) return fail(c, GPET_ERR_STATE, "gpet_select_pixels before gpet_score_curves");
  return select_pixels(b, StateEvent::select_pixels, true, 0);
}

// gpet_select_pixels in the form the device loop runs after its scorer
int gpet_select_pixels_loop(gpet_batch* b) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  if (state_missing(b->st, StateEvent::select_pixels)) return fail(c, GPET_ERR_STATE, "gpet_select_pixels_loop before gpet_score_curves");
  return select_pixels(b, StateEvent::select_pixels, true, 1);
}

int gpet_select_pixels_only(gpet_batch* b) {
  GPET_BATCH_SCOPE(b);
  if (!b) return GPET_ERR_BAD_ARG;
  return select_pixels(b, StateEvent::select_pixels_only, false, 0);
}

int gpet_profile_stage(gpet_batch* b, int stage, int reps, float* ms_per_rep) {
  GPET_BATCH_SCOPE(b);
  if (!b || !ms_per_rep || reps < 1) return GPET_ERR_BAD_ARG;
  gpet_ctx* c = b->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  // 120-123 on a batch that has left the structured path (gpet_batch_set_obs with an off-grid observation clears b->structured;
  // the edges keep structured = 1 and their basis): k_struct_H / k_structB_build would gather Q0[a * Lg + (x - x_st)] with the
  // off-grid x outside the basis.  Refused before any launch
  if (stage >= 120 && stage <= 123 && !b->structured)
    return fail(c, GPET_ERR_BAD_ARG, "gpet_profile_stage: stage %d needs a structured batch (gpet_batch_info: structured)", stage);
  // 170: the in-place normaliser of the raw-frame path (k_normalise_f32_batch) over the batch's image slots, with the neutral pair
  // (min 0, max 1) in every slot of d_minmax -- (x - 0) / 1 leaves every bit of the images as it is
  float** d_slots = nullptr;
  if (stage == 170) {
    std::vector<float*> slots((size_t)b->n_img);
    for (int g = 0; g < b->n_img; ++g) slots[(size_t)g] = (float*)b->h_edges[b->img_rep[g]].grad;
    b->h_mm0.assign((size_t)2 * b->n_img, 0x80000000u);  // the order key of +0.0f ...
    for (int g = 0; g < b->n_img; ++g) b->h_mm0[2 * (size_t)g + 1] = 0xBF800000u;  // ... and of 1.0f
    HIPCHK(c, hipMalloc(&d_slots, sizeof(float*) * slots.size()));
    hipError_t e = hipMemcpy(d_slots, slots.data(), sizeof(float*) * slots.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(b->d_minmax, b->h_mm0.data(), sizeof(unsigned int) * b->h_mm0.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d_slots);
      HIPCHK(c, e);
    }
  }
  struct SlotGuard {
    float** p;
    ~SlotGuard() {
      if (p) (void)hipFree(p);
    }
  } slot_guard{d_slots};
  bool normals_profiled = false;
  HIPCHK(c, hipEventRecord(c->ev0, c->stream));
  for (int r = 0; r < reps; ++r) {
    switch (stage) {
      case 170: HIPCHK(c, launch_normalise_batch(c->stream, d_slots, b->n_img, (size_t)b->bd.M * b->bd.N, b->d_minmax)); break;
      case 0:
        if (b->structured) HIPCHK(c, launch_struct_iteration(c->stream, b->d_edges, b->B, b->bd, 1u | 2u));
        else HIPCHK(c, launch_fit_predict(c->stream, b->d_edges, b->B, b->bd, 1));
        break;
      case 1:
        if (b->structured) HIPCHK(c, launch_struct_iteration(c->stream, b->d_edges, b->B, b->bd, 4u | 8u));
        else HIPCHK(c, launch_factor(c->stream, b->d_edges, b->B, b->bd, ~0u, b->h_edges.data()));
        break;
      case 120: case 121: case 122: case 123:  // structured path: fit, (U, H, mean), Jacobi, factor rows
        HIPCHK(c, launch_struct_iteration(c->stream, b->d_edges, b->B, b->bd, 1u << (stage - 120))); break;
      case 2:
        if (b->rng_mode == 1) HIPCHK(c, launch_normals_philox(c->stream, b->d_edges, b->B, b->bd, b->d_seeds, 1, -1, b->bd.z_ring, loop_z_store(b)));
        else HIPCHK(c, launch_normals_seq(b, c->stream, b->d_edges, b->B, b->d_seeds, 1, -1, b->bd.z_ring, loop_z_store(b)));
        normals_profiled = true;  // (always generates, into the slots z_slot names: their tags are settled below)
        break;
      case 3: HIPCHK(c, launch_sample(c->stream, b->d_edges, b->B, b->bd, b->structured ? b->bd.r0_max : 0)); break;
      case 4: HIPCHK(c, launch_score(c->stream, b->d_edges, b->B, b->bd)); break;
      case 5: HIPCHK(c, launch_kde(c->stream, b->d_edges, b->B, b->bd, 0, ~0u, 1)); break;  // (the loop form: raw, band only)
      case 6: HIPCHK(c, launch_pixels_reset(c->stream, b->d_edges, b->B, b->bd)); break;  // (reset only: selection mutates the loop state)
      // single kernels: 100+ fit/predict/cov, 110+ pchol/gram/jacobi/rows, 130 gemm, 140+ score/topk, 150+ kde prep/fused/normalise
      case 100: case 101: case 102:
        HIPCHK(c, launch_fit_predict(c->stream, b->d_edges, b->B, b->bd, 1, 1u << (stage - 100))); break;
      case 110: case 111: case 112: case 113:
        HIPCHK(c, launch_factor(c->stream, b->d_edges, b->B, b->bd, 1u << (stage - 110))); break;
      case 130: HIPCHK(c, launch_sample(c->stream, b->d_edges, b->B, b->bd, b->structured ? b->bd.r0_max : 0)); break;
      case 140: case 141: HIPCHK(c, launch_score(c->stream, b->d_edges, b->B, b->bd, 1u << (stage - 140))); break;
      case 150: case 151: HIPCHK(c, launch_kde(c->stream, b->d_edges, b->B, b->bd, 0, 1u << (stage - 150), 1)); break;
      case 152: HIPCHK(c, launch_kde(c->stream, b->d_edges, b->B, b->bd, 0, 4u, 0)); break;  // (stage-API form only)
      // 160: the column scan of the pixel selection, loop form (reads the raw KDE band of stage 151; it only raises
      // per-bin maxima to values they already hold, so repeating it leaves the loop state as it was)
      case 160: HIPCHK(c, launch_pixels(c->stream, b->d_edges, b->B, b->bd, 1, 1u)); break;
      default: return fail(c, GPET_ERR_BAD_ARG, "gpet_profile_stage: unknown stage %d", stage);
    }
  }
  HIPCHK(c, hipEventRecord(c->ev1, c->stream));
  HIPCHK(c, hipEventSynchronize(c->ev1));
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
  *ms_per_rep = ms / (float)reps;
  const int rc_status = check_device_status(b);  // (reads every edge's state)
  if (normals_profiled && (b->zst.iters > 0 || b->zst.ring > 0)) {
    // Stage 2 drew, for every running edge, the z_ring iterations from its own on by the loop's seed rule from the seeds on the
    // device: the store slots among them, and the ring slots of the others (z_ring iterations: z_ring distinct slots at most), hold
    // exactly what the loop would draw there, so they get the loop's tags.  Without a host copy of those seeds, or after an error,
    // the slots it may have written lose theirs.
    const int zsel = loop_z_store(b), zs = zsel > 0 && zsel < b->bd.z_cols ? zsel : b->bd.z_cols;
    const bool known = rc_status == GPET_OK && (int)b->h_seeds_dev.size() == b->B;
    for (int e = 0; e < b->B; ++e) {
      const gpet_scalars& s = b->h_scalars[e];
      if (known && (s.done || s.status != GPET_OK)) continue;  // (skipped by the generators: untouched)
      for (int q = std::max(0, s.iter); q < s.iter + b->bd.z_ring; ++q)
        if (uint64_t* t = zstore_tag_at(b->zst, e, q)) *t = known ? zstore_loop_tag(b->h_seeds_dev[e], q, b->rng_mode, zs) : 0;
    }
  }
  return rc_status;
}

}  // extern "C"
