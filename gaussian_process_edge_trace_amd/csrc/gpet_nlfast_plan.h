// What the fast-mode non-local means stage (a0: gpet_nlmeans_fast_images) decides before anything is launched, as plain data: the
// spec and its validation, the shift table, the padded geometry, how the shifts are cut into groups, a frame's workspace, the
// chunks and the launch geometry of the three kernels (gpet_k_nlfast.inc), which take all of it from here.  No HIP, so the host
// compiler alone builds it (tests/test_nlmeans_fast_plan.py).  The reference: gpet_utils.denoise 'nl' with the library's default
// fast_mode=True = scikit-image 0.18.3's denoise_nl_means(image, patch_size, patch_distance, h, fast_mode=True, sigma) on a 2-D
// single-channel frame.  Python spells the technique 'nl_fast'.
//
// The arithmetic (all f64, no fused multiply-add, IEEE division; sums left to right as written).  s = patch_size (+ 1 if even),
// off = s / 2, d = patch_distance, pad = off + d + 1, var2 = 2 sigma^2, h2s2 = ((h * h) * s) * s.  P is the frame widened to f64 --
// integer frames keep their range -- and padded by pad with numpy's 'reflect' (nlm_mirror); nr = M + 2 pad, nc = N + 2 pad.  W and
// R start at zero over the padded frame.  For t_row = -d .. d (outer) and t_col = 0 .. d (inner), alpha = 0.5 if t_col == 0 and
// t_row != 0, else 1:
//   the integral: I starts at zero; for r = max(1, -t_row) .. min(nr, nr - t_row) - 1 and inside it c likewise with t_col and nc:
//     t = P[r, c] - P[r + t_row, c + t_col]; q = (0 + t * t) - var2; I[r, c] = ((q + I[r-1, c]) + I[r, c-1]) - I[r-1, c-1]
//     (cells outside the ranges stay 0 and ARE read);
//   the weights: for row = max(off, off - t_row) .. min(nr - off, nr - off - t_row) - 1 and inside it col likewise:
//     dd = ((I[row+off, col+off] + I[row-off, col-off]) - I[row-off, col+off]) - I[row+off, col-off]; dist = max(dd, 0) / h2s2;
//     a pair with dist > 5.0 is skipped; else w = alpha * nlm_fexp(-dist) (gpet_nlmeans_plan.h; its argument stays in [-5, 0]) and
//     W[row, col] += w; W[row+t_row, col+t_col] += w; R[row, col] += w * P[row+t_row, col+t_col]; R[row+t_row, col+t_col] += w * P[row, col].
// The result is R / W on the unpadded region; W > 0 always (the shift (0, 0) contributes twice).
//
// How the device follows it bit for bit.
// The integral: cell (r, c) reads (r-1, c), (r, c-1), (r-1, c-1), so the cells of an anti-diagonal are independent and walking the
// diagonals in ascending order gives every cell the operands it had in raster order (the argument of gpet_tvb_plan.h).  The shifts
// of a frame are independent chains.  THE CHOICE HERE: one WAVE per (frame, shift) strip-mines the rows NLF_STRIP at a time; lane l
// holds row r0 + l at column (step - l), I[r, c-1] is its own previous value, I[r-1, c] the previous value of the lane below it
// (one DPP lane shift), I[r-1, c-1] what it received a step earlier; the last row of a strip is read back by the next strip from
// the plane itself, 64 columns at a time.  No workgroup barrier per step; the values of P a step needs do not depend on the
// chain and are loaded a block of steps ahead.  The alternative, 'tvb''s one workgroup per chain with a barrier per diagonal,
// was not built or measured here (profiles/nlmeans_fast_timing.txt has this form's figures).  Every cell of a plane is written, cells outside the
// shift's ranges as 0.  The planes are stored row-major straight from the lanes (a lane's stores walk along its row); staging
// 64-wide tiles through LDS to store whole segments was not built.
// The sums: the scatter above reaches a pixel p in a fixed sequence, which a gather follows: in shift order, and within a shift
// t the term of the pair (p - t, p) ("partner": weight looked up at p - t, adds P[p - t]) before the term of the pair (p, p + t)
// ("own": weight looked up at p, adds P[p + t]) when t_row > 0 or t_row == 0 and t_col > 0, own before partner when t_row < 0,
// own twice for (0, 0).  One thread per OUTPUT pixel carries its W and R through the groups.  For an output pixel both pairs of
// every shift lie inside the weight ranges -- that is what pad = off + d + 1 buys -- so a term is absent only by the cutoff.
#pragma once
#include <math.h>
#include <stddef.h>

#include "gpet_conv_plan.h"     // pixel types, staging
#include "gpet_denoise_plan.h"  // dn_align
#include "gpet_nlmeans_plan.h"  // nlm_patch, nlm_mirror, nlm_fexp, NLM_CUTOFF, NLM_PATCH_MAX, NLM_DIST_MAX

namespace gpet {

// ---- the spec (include/gpet_hip.h: gpet_nlmeans_fast) ---------------------------------------------------------------------------
struct NlfSpec {
  int patch_size = 7;  // as the caller wrote it: an even size means the next odd one
  int patch_distance = 11;
  double h = 0.1, sigma = 0.0;
};

// ---- the shift table --------------------------------------------------------------------------------------------------------------
// shift k = (t_row + d) (d + 1) + t_col: t_row = -d .. d outer, t_col = 0 .. d inner; a "row" of shifts is the d + 1 of one t_row
struct NlfShift {
  int t_row, t_col;
  double alpha;
};
GPET_NLM_HD inline int nlf_row_shifts(int d) { return d + 1; }
GPET_NLM_HD inline int nlf_shift_rows(int d) { return 2 * d + 1; }
GPET_NLM_HD inline int nlf_shifts(int d) { return nlf_shift_rows(d) * nlf_row_shifts(d); }
GPET_NLM_HD inline NlfShift nlf_shift(int d, int k) {
  const int t_row = k / (d + 1) - d, t_col = k % (d + 1);
  return NlfShift{t_row, t_col, (t_col == 0 && t_row != 0) ? 0.5 : 1.0};
}
// along an axis of padded length n, for the shift's component t: first and one-past-last index of the integral's and the weights'
GPET_NLM_HD inline int nlf_integral_lo(int t) { return -t > 1 ? -t : 1; }
GPET_NLM_HD inline int nlf_integral_hi(int n, int t) { return t > 0 ? n - t : n; }
GPET_NLM_HD inline int nlf_weight_lo(int t, int off) { return t < 0 ? off - t : off; }
GPET_NLM_HD inline int nlf_weight_hi(int n, int t, int off) { return t > 0 ? n - off - t : n - off; }
// whether, at a pixel, the partner term of a shift is added before its own term (the per-pixel order of the header comment)
GPET_NLM_HD inline bool nlf_partner_first(int t_row, int t_col) { return t_row > 0 || (t_row == 0 && t_col > 0); }

// ---- geometry, groups, workspace --------------------------------------------------------------------------------------------------
constexpr int NLF_STRIP = 64;     // rows of a strip: the lanes of a wave
constexpr int NLF_THREADS = 256;  // workgroup of the pad and the gather kernel, a thread per cell / output pixel
// a chunk's staging (host frames, host results) and its workspaces together stay inside the budget, as in the other stages
constexpr size_t NLF_CHUNK_BUDGET = (size_t)256 << 20;
constexpr int NLF_CHUNK_MAX = STAGE_GRID_Z_MAX;  // gridDim.z

struct NlfPlan {
  int s, off, d, pad, nr, nc;
  int n_shifts;         // (2 d + 1)(d + 1)
  int rows_per_group;   // whole rows of shifts whose planes a frame's workspace holds at a time; 0: not even one fits the budget
  int n_groups;         // ceil((2 d + 1) / rows_per_group)
  int strips;           // ceil(nr / NLF_STRIP)
  int steps;            // steps of a strip: nc + NLF_STRIP - 1
  size_t plane_doubles;  // nr nc: P and every I
  size_t off_w, off_r, off_i;  // doubles from the frame's workspace to W, R (M N each) and the group's planes; P is at 0
  size_t frame_bytes;   // with rows_per_group rows (with one row if none fits), to 256 bytes
};
inline size_t nlf_frame_bytes_with(size_t plane, size_t px, int d, int rows) {
  return dn_align((plane + 2 * px + (size_t)rows * (size_t)nlf_row_shifts(d) * plane) * sizeof(double));
}
// (s odd, d >= 0, M, N >= 1)
inline NlfPlan nlf_plan(int M, int N, int s, int d, size_t budget = NLF_CHUNK_BUDGET) {
  NlfPlan p{};
  p.s = s;
  p.off = s / 2;
  p.d = d;
  p.pad = p.off + d + 1;
  p.nr = M + 2 * p.pad;
  p.nc = N + 2 * p.pad;
  p.n_shifts = nlf_shifts(d);
  p.strips = (p.nr + NLF_STRIP - 1) / NLF_STRIP;
  p.steps = p.nc + NLF_STRIP - 1;
  p.plane_doubles = (size_t)p.nr * (size_t)p.nc;
  const size_t px = (size_t)M * (size_t)N;
  p.off_w = p.plane_doubles;
  p.off_r = p.off_w + px;
  p.off_i = p.off_r + px;
  int rows = 0;
  while (rows < nlf_shift_rows(d) && nlf_frame_bytes_with(p.plane_doubles, px, d, rows + 1) <= budget) ++rows;
  p.rows_per_group = rows;
  p.n_groups = rows ? (nlf_shift_rows(d) + rows - 1) / rows : 0;
  p.frame_bytes = nlf_frame_bytes_with(p.plane_doubles, px, d, rows ? rows : 1);
  return p;
}
// group g of a plan: its first shift and how many shifts it has
inline int nlf_group_first(const NlfPlan& p, int g) { return g * p.rows_per_group * nlf_row_shifts(p.d); }
inline int nlf_group_count(const NlfPlan& p, int g) {
  const int left = p.n_shifts - nlf_group_first(p, g), full = p.rows_per_group * nlf_row_shifts(p.d);
  return left < full ? left : full;
}
inline StagePlan nlf_chunks(int n_img, size_t staged_bytes_per_img, const NlfPlan& p, size_t budget = NLF_CHUNK_BUDGET) {
  return stage_plan_z(n_img, staged_bytes_per_img + p.frame_bytes, budget);
}

// ---- launch geometry (gridDim.z = frames of the chunk everywhere) ----------------------------------------------------------------
inline unsigned nlf_pad_blocks(const NlfPlan& p) { return (unsigned)((p.plane_doubles + NLF_THREADS - 1) / NLF_THREADS); }
inline unsigned nlf_gather_blocks(int M, int N) { return (unsigned)(((size_t)M * (size_t)N + NLF_THREADS - 1) / NLF_THREADS); }
// the integral kernel: gridDim.x = the group's shifts, one wave of NLF_STRIP lanes each

// ---- validation ------------------------------------------------------------------------------------------------------------------
// nullptr if the spec can run on M x N frames of pixel type pix, else what is wrong with it (the workspace bound apart: nlf_plan's
// rows_per_group == 0, which the entry point reports with the byte counts)
inline const char* nlf_check(const NlfSpec& sp, int pix, int M, int N) {
  if (!pix_bytes(pix)) return "unknown pixel type";
  if (M < 1 || N < 1) return "empty frame";
  if (sp.patch_size < 2) return "patch_size must be at least 2";
  const int s = nlm_patch(sp.patch_size);
  if (s > NLM_PATCH_MAX) return "patches of more than 15 x 15 pixels are not built";
  if (sp.patch_distance < 0) return "patch_distance must not be negative";
  if (sp.patch_distance > NLM_DIST_MAX) return "patch distances above 31 are not built";
  if (!(sp.h > 0.0) || !(sp.h < INFINITY)) return "h must be above 0";
  if (!(sp.sigma >= 0.0) || !(sp.sigma < INFINITY)) return "sigma must not be negative";
  if (s / 2 + sp.patch_distance + 1 > (M < N ? M : N) - 1)
    return "the padding off + patch_distance + 1 must be below the frame's smaller extent (the padding reflects once)";
  return nullptr;
}

}  // namespace gpet
