// The slot table of a multi-kernel raw-frame source (gpet_grad_images_multi, gpet_batch_create_raw_multi,
// gpet_batch_set_raw_images_multi), decided before anything is launched, as plain data: image slot g is raw frame frame_of[g]
// convolved with kernel kernel_of[g].  Every frame is uploaded, denoised and staged into LDS once, however many kernels read it:
// a workgroup loads the UNION patch of all kernels and evaluates each slot of its frame out of it (k_conv_relu_multi).  No HIP, so
// the host compiler alone builds it (tests/test_multi_kernel_host.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gpet_conv_plan.h"

namespace gpet {

constexpr int CONV_MULTI_MAX_KERN = 8;  // kernels of one table (the reference's users have two: one per polarity)

// ---- validation ---------------------------------------------------------------------------------------------------------------
// nullptr, or why the table is refused (as dn_check does)
inline const char* slot_table_check(int n_frames, int n_kern, int n_img, const int32_t* frame_of, const int32_t* kernel_of) {
  if (n_frames <= 0 || n_kern <= 0 || n_img <= 0 || !frame_of || !kernel_of) return "empty slot table";
  if (n_kern > CONV_MULTI_MAX_KERN) return "more than 8 kernels";
  for (int g = 0; g < n_img; ++g) {
    if (frame_of[g] < 0 || frame_of[g] >= n_frames) return "frame index out of range";
    if (kernel_of[g] < 0 || kernel_of[g] >= n_kern) return "kernel index out of range";
  }
  // (tables are small: slots of a batch, not pixels)
  for (int f = 0; f < n_frames; ++f) {
    bool used = false;
    for (int g = 0; g < n_img && !used; ++g) used = frame_of[g] == f;
    if (!used) return "a frame no slot reads";
  }
  for (int k = 0; k < n_kern; ++k) {
    bool used = false;
    for (int g = 0; g < n_img && !used; ++g) used = kernel_of[g] == k;
    if (!used) return "a kernel no slot reads";
  }
  for (int g = 1; g < n_img; ++g)
    for (int h = 0; h < g; ++h)
      if (frame_of[g] == frame_of[h] && kernel_of[g] == kernel_of[h])
        return "the same (frame, kernel) pair twice (edges that want the same image share a slot through image_of)";
  return nullptr;
}
// one kernel, one slot per frame, in frame order: the single-kernel path, which the multi entry points then take as it is
inline bool slot_table_is_identity(int n_frames, int n_kern, int n_img, const int32_t* frame_of, const int32_t* kernel_of) {
  if (n_kern != 1 || n_img != n_frames) return false;
  for (int g = 0; g < n_img; ++g)
    if (frame_of[g] != g || kernel_of[g] != 0) return false;
  return true;
}

// ---- union patch --------------------------------------------------------------------------------------------------------------
// kernel k's tap (0, 0) lies conv_origin(kh_k) rows above the output pixel and its last tap kh_k - 1 - conv_origin(kh_k) below:
// the patch all kernels can be evaluated from has the largest of each on every side
struct ConvUnion {
  int top, bottom, left, right;
  size_t taps;  // sum of kh_k * kw_k
};
inline ConvUnion conv_union(int n_kern, const int32_t* kh, const int32_t* kw) {
  ConvUnion u{0, 0, 0, 0, 0};
  for (int k = 0; k < n_kern; ++k) {
    const int oy = conv_origin(kh[k]), ox = conv_origin(kw[k]);
    if (oy > u.top) u.top = oy;
    if (kh[k] - 1 - oy > u.bottom) u.bottom = kh[k] - 1 - oy;
    if (ox > u.left) u.left = ox;
    if (kw[k] - 1 - ox > u.right) u.right = kw[k] - 1 - ox;
    u.taps += (size_t)kh[k] * kw[k];
  }
  return u;
}
inline int conv_union_rows(const ConvUnion& u) { return CONV_TILE_Y + u.top + u.bottom; }
inline int conv_union_cols(const ConvUnion& u) { return CONV_TILE_X + u.left + u.right; }
inline size_t conv_union_lds_bytes(const ConvUnion& u) {
  return (u.taps + (size_t)conv_union_rows(u) * conv_union_cols(u)) * sizeof(double);
}
inline bool conv_union_fits_lds(int n_kern, const int32_t* kh, const int32_t* kw) {
  for (int k = 0; k < n_kern; ++k)
    if (kh[k] <= 0 || kw[k] <= 0) return false;
  return conv_union_lds_bytes(conv_union(n_kern, kh, kw)) <= CONV_LDS_MAX;
}

// what the kernel reads of kernel k: its extents, where its tap (0, 0) lies in the union patch relative to the output pixel's
// (row yl, column tx) -- tap (a, b) reads patch row yl + a + dy, column tx + b + dx -- and where its flipped taps start
struct ConvKernDesc {
  int32_t kh, kw, dy, dx, w0;
};
inline void conv_kern_descs(int n_kern, const int32_t* kh, const int32_t* kw, ConvKernDesc* kd) {
  const ConvUnion u = conv_union(n_kern, kh, kw);
  int32_t w0 = 0;
  for (int k = 0; k < n_kern; ++k) {
    kd[k] = ConvKernDesc{kh[k], kw[k], u.top - conv_origin(kh[k]), u.left - conv_origin(kw[k]), w0};
    w0 += kh[k] * kw[k];
  }
}

// ---- slots of each frame ------------------------------------------------------------------------------------------------------
// off[n_frames + 1], list[n_img]: the slots of frame f are list[off[f] .. off[f + 1]), in ascending slot order
inline void frame_slots(int n_frames, int n_img, const int32_t* frame_of, int32_t* off, int32_t* list) {
  for (int f = 0; f <= n_frames; ++f) off[f] = 0;
  for (int g = 0; g < n_img; ++g) ++off[frame_of[g] + 1];
  for (int f = 0; f < n_frames; ++f) off[f + 1] += off[f];
  for (int g = 0; g < n_img; ++g) list[off[frame_of[g]]++] = g;  // (off[f] is now the end of frame f: shift back)
  for (int f = n_frames; f > 0; --f) off[f] = off[f - 1];
  off[0] = 0;
}

}  // namespace gpet
