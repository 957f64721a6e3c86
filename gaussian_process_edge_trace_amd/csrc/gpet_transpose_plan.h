// What a vertical batch (GPET_FRAMES_TRANSPOSED) decides before anything is launched, as plain data: an M x N frame -- M rows of N
// pixels, as it lies in memory -- becomes the N x M image G.T in the batch's own buffers, and pixel (row, col) of the frame's gradient
// image lands at offset col * M + row.  Two ways in:
//   - raw frames: the transposed-store form of the convolution (k_conv_tr_batch / k_conv_tr_multi).  A workgroup of 64 x 4
//     threads owns CONV_T_TILE_X = 16 frame columns x CONV_T_TILE_Y = 64 frame rows; a wave's 64 lanes are 64 consecutive frame
//     ROWS of one frame column, so every store of a wave is one run of 64 floats (256 bytes) of a row of G.T.  The patch lies in
//     LDS column-major -- (16 + kw - 1) columns of (64 + kh - 1) pixels -- so that the 64 lanes of a tap read, one patch row apart,
//     are consecutive doubles; the pitch between the columns is odd, which spreads the strided writes of the patch load over the
//     banks.
//   - gradient images of the caller: a tile kernel (k_transpose_f32), TR_TILE x TR_TILE through LDS with a pitch of TR_TILE + 1,
//     rows of the source read and rows of the destination written by consecutive lanes.
// No HIP, so the host compiler alone builds it (tests/test_transpose_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gpet_conv_multi_plan.h"

namespace gpet {

// ---- the index map ------------------------------------------------------------------------------------------------------------
// pixel (row, col) of an M x N frame in the N x M transposed image
constexpr size_t tr_offset(int row, int col, int M) { return (size_t)col * (size_t)M + (size_t)row; }

// ---- tile transpose of a finished f32 image -----------------------------------------------------------------------------------
constexpr int TR_TILE = 64;              // a workgroup of 64 x 4 threads moves TR_TILE x TR_TILE pixels
constexpr int TR_PITCH = TR_TILE + 1;    // floats between the tile's rows in LDS: a column read walks all banks
constexpr size_t tr_lds_bytes() { return (size_t)TR_TILE * TR_PITCH * sizeof(float); }
struct TrGrid {
  int gx, gy;  // workgroups along the frame's columns and rows; gridDim.z = images of the launch
};
inline TrGrid tr_grid(int M, int N) { return TrGrid{(N + TR_TILE - 1) / TR_TILE, (M + TR_TILE - 1) / TR_TILE}; }

// ---- transposed-store convolution ---------------------------------------------------------------------------------------------
constexpr int CONV_T_TILE_X = 16, CONV_T_TILE_Y = 64;
// doubles between the patch's COLUMNS in LDS for a patch of `rows` rows: the next odd number
constexpr int conv_t_pitch(int rows) { return rows | 1; }
inline int conv_t_rows(int kh) { return CONV_T_TILE_Y + kh - 1; }
inline int conv_t_cols(int kw) { return CONV_T_TILE_X + kw - 1; }
inline size_t conv_t_lds_bytes(int kh, int kw) {
  return ((size_t)kh * kw + (size_t)conv_t_cols(kw) * conv_t_pitch(conv_t_rows(kh))) * sizeof(double);
}
inline bool conv_t_fits_lds(int kh, int kw) { return kh > 0 && kw > 0 && conv_t_lds_bytes(kh, kw) <= CONV_LDS_MAX; }
inline ConvGrid conv_t_grid(int M, int N) {
  return ConvGrid{(N + CONV_T_TILE_X - 1) / CONV_T_TILE_X, (M + CONV_T_TILE_Y - 1) / CONV_T_TILE_Y};
}
// thread (lane, j) of workgroup (bx, by) -- lane 0 .. 63 = threadIdx.x, j = 0 .. 15 the column it is at -- computes this pixel
constexpr int conv_t_row(int by, int lane) { return by * CONV_T_TILE_Y + lane; }
constexpr int conv_t_col(int bx, int j) { return bx * CONV_T_TILE_X + j; }

// the union patch of a slot table (gpet_conv_multi_plan.h) under the transposed tile
inline int conv_union_t_rows(const ConvUnion& u) { return CONV_T_TILE_Y + u.top + u.bottom; }
inline int conv_union_t_cols(const ConvUnion& u) { return CONV_T_TILE_X + u.left + u.right; }
inline size_t conv_union_t_lds_bytes(const ConvUnion& u) {
  return (u.taps + (size_t)conv_union_t_cols(u) * conv_t_pitch(conv_union_t_rows(u))) * sizeof(double);
}
inline bool conv_union_t_fits_lds(int n_kern, const int32_t* kh, const int32_t* kw) {
  for (int k = 0; k < n_kern; ++k)
    if (kh[k] <= 0 || kw[k] <= 0) return false;
  return conv_union_t_lds_bytes(conv_union(n_kern, kh, kw)) <= CONV_LDS_MAX;
}

}  // namespace gpet
