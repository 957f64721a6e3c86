// What the gradient-image convolution (a1: gpet_grad_image, gpet_grad_images, the raw-frame batch calls) decides before anything
// is launched, as plain data: the taps as the kernels read them, the launch geometry, and how a stack of host frames goes up in
// chunks.  No HIP, so the host compiler alone builds it (tests/test_raw_frames_host.py).
#pragma once
#include <stddef.h>

namespace gpet {

// ---- pixel types of raw frames (include/gpet_hip.h: GPET_PIX_*) ---------------------------------------------------------------
enum { PIX_U8 = 0, PIX_U16 = 1, PIX_F32 = 2, PIX_F64 = 3, PIX_COUNT = 4 };
// bytes of one pixel; 0 for a code that is none of the four
inline int pix_bytes(int pix) { return pix == PIX_U8 ? 1 : pix == PIX_U16 ? 2 : pix == PIX_F32 ? 4 : pix == PIX_F64 ? 8 : 0; }

// ---- taps ---------------------------------------------------------------------------------------------------------------------
// scipy.ndimage.convolve (gpet_utils.py:112) is a correlation with the kernel flipped in both directions ...
inline void conv_flip_taps(const double* kern, int kh, int kw, double* wf) {
  for (int a = 0; a < kh; ++a)
    for (int b = 0; b < kw; ++b) wf[(size_t)a * kw + b] = kern[(size_t)(kh - 1 - a) * kw + (kw - 1 - b)];
}
// ... whose tap (0, 0) lies `conv_origin` pixels before the output pixel: the centre k / 2, one less for an even extent
inline int conv_origin(int k) { return k / 2 - ((k % 2 == 0) ? 1 : 0); }

// ---- launch geometry ----------------------------------------------------------------------------------------------------------
// a workgroup of 64 x 4 threads owns CONV_TILE_X columns x CONV_TILE_Y rows of one image's output; its edge-replicated patch and
// the taps sit in LDS as f64
constexpr int CONV_TILE_X = 64, CONV_TILE_Y = 16;
constexpr size_t CONV_LDS_MAX = 64 * 1024;
inline size_t conv_lds_bytes(int kh, int kw) {
  return ((size_t)kh * kw + (size_t)(CONV_TILE_Y + kh - 1) * (CONV_TILE_X + kw - 1)) * sizeof(double);
}
// (a kernel of hundreds of taps per side is not the reference's use: refused, not tiled differently)
inline bool conv_fits_lds(int kh, int kw) { return kh > 0 && kw > 0 && conv_lds_bytes(kh, kw) <= CONV_LDS_MAX; }
struct ConvGrid {
  int gx, gy;  // workgroups along x and y; gridDim.z = images of the launch
};
inline ConvGrid conv_grid(int M, int N) { return ConvGrid{(N + CONV_TILE_X - 1) / CONV_TILE_X, (M + CONV_TILE_Y - 1) / CONV_TILE_Y}; }

// ---- staging of host frames ---------------------------------------------------------------------------------------------------
// Host frames reach the device in chunks of whole images through a ring of equal staging slots: chunk k is copied into slot
// k % slots and convolved from there, one launch per chunk.  A slot holds as many images as fit the byte budget (at least one).
// Copies and convolutions share the context's one stream, so a chunk's copy cannot overtake the convolution that last read its
// slot, and a second slot buys nothing: 256 frames of 500 x 500 took 8.1 / 12.7 / 18.2 ms (u8 / f32 / f64) with two slots and
// 8.1 / 12.7 / 18.1 ms with one.  The library therefore stages through ONE slot; the depth stays a parameter of the plan.
constexpr size_t STAGE_SLOT_BUDGET = (size_t)64 << 20;  // 256 u8 frames of 500 x 500 are one chunk, 256 f64 frames eight
constexpr int STAGE_RING = 1;
struct StagePlan {
  int per_chunk;      // images of a full chunk
  int n_chunks;
  int slots;          // ring slots in use: min(n_chunks, ring)
  size_t slot_bytes;  // bytes between the slots, a multiple of 256
};
inline StagePlan stage_plan(int n_img, size_t img_bytes, size_t budget = STAGE_SLOT_BUDGET, int ring = STAGE_RING) {
  StagePlan p{0, 0, 0, 0};
  if (n_img <= 0 || img_bytes == 0 || ring <= 0) return p;
  size_t fit = budget / img_bytes;
  if (fit < 1) fit = 1;
  p.per_chunk = fit < (size_t)n_img ? (int)fit : n_img;
  p.n_chunks = (n_img + p.per_chunk - 1) / p.per_chunk;
  p.slots = p.n_chunks < ring ? p.n_chunks : ring;
  p.slot_bytes = ((size_t)p.per_chunk * img_bytes + 255) & ~(size_t)255;
  return p;
}
// the chunks of a stage whose frames keep a workspace each (wavelet, split-Bregman): staging and workspace of a chunk together stay
// inside the budget, and a chunk is one launch along gridDim.z
constexpr int STAGE_GRID_Z_MAX = 65535;
inline StagePlan stage_plan_z(int n_img, size_t bytes_per_img, size_t budget) {
  StagePlan p = stage_plan(n_img, bytes_per_img, budget);
  if (p.per_chunk > STAGE_GRID_Z_MAX) {
    p.per_chunk = STAGE_GRID_Z_MAX;
    p.n_chunks = (n_img + p.per_chunk - 1) / p.per_chunk;
  }
  return p;
}
inline int stage_slot(const StagePlan& p, int k) { return k % p.slots; }
inline int stage_first(const StagePlan& p, int k) { return k * p.per_chunk; }                                // first image of chunk k
inline int stage_count(const StagePlan& p, int k, int n_img) {                                               // images of chunk k
  const int left = n_img - stage_first(p, k);
  return left < p.per_chunk ? left : p.per_chunk;
}

}  // namespace gpet
