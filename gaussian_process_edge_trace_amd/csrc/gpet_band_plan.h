// Tracking bands: what a banded batch decides before a kernel is launched, as plain data.  No HIP: the host
// compiler alone builds this header (tests/test_band_plan.py compiles it into a shim), and k_band_place calls band_place on the device.
//
// A band is (r0, H): rows r0 .. r0 + H - 1 of an M x N frame, 1 <= H <= M, 0 <= r0 <= M - H.  All edges of a batch share H (the batch's
// image shape is (H, N)); r0 is per edge.  Edge e of a banded batch computes what an unbanded batch computes on rows r0 .. r0 + H - 1
// of the full-frame gradient image with its init rows lowered by r0; every row it reports is in band coordinates on the device and
// raised by r0 where the records are decoded.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GPET_BAND_HD __host__ __device__
#else
#define GPET_BAND_HD
#endif

namespace gpet {

// The refusals of a band, in the order they are checked: nullptr when (r0, H) can hold the init rows i_lo .. i_hi of an M-row frame.
// r0 < 0 with place == true: the band is still to be placed (band_place then keeps the inits inside), so only H is judged.
inline const char* band_check(long long M, long long H, long long r0, long long i_lo, long long i_hi, bool place = false) {
  if (H < 1) return "band_rows must be at least 1";
  if (H > M) return "band_rows exceeds the rows of the frame (H > M)";
  if (i_hi - i_lo + 1 > H) return "the init rows span more rows than the band holds (i_hi - i_lo + 1 > H)";
  if (place) return nullptr;
  if (r0 < 0 || r0 > M - H) return "r0 lies outside [0, M - H]";
  if (i_lo < r0 || i_hi > r0 + H - 1) return "an init point lies outside its band";
  return nullptr;
}

// floor(a / 2) for any sign (C++ division truncates towards zero)
GPET_BAND_HD inline long long band_floor_half(long long a) { return a / 2 - ((a % 2) < 0 ? 1 : 0); }

// The placement rule.  lo / hi: the smallest and largest entry of the source's trace in full-frame rows that is neither NaN nor outside
// [0, M - 1]; i_lo / i_hi: the smallest and largest init row of the destination edge, i_hi - i_lo + 1 <= H (band_check).  All int64,
// floor division:
//   r0 = (lo + hi) // 2 - H // 2;   r0 = min(max(r0, 0), M - H);   r0 = max(min(r0, i_lo), i_hi - H + 1)
// The last line keeps the fixed init rows inside the band, and cannot leave [0, M - H] when the inits lie in the frame.
GPET_BAND_HD inline long long band_place(long long M, long long H, long long lo, long long hi, long long i_lo, long long i_hi) {
  long long r0 = band_floor_half(lo + hi) - band_floor_half(H);
  const long long top = M - H;
  r0 = r0 < 0 ? 0 : r0;
  r0 = r0 > top ? top : r0;
  r0 = r0 < i_lo ? r0 : i_lo;
  const long long need = i_hi - H + 1;
  r0 = r0 > need ? r0 : need;
  return r0;
}

// ---- what a banded batch owns in addition to the arena -----------------------------------------------------------------------------
// the full-frame gradient images: one per distinct (frame, kernel) pair, f32
inline size_t band_image_bytes(int n_pair, int M, int N) { return (size_t)n_pair * (size_t)M * (size_t)N * sizeof(float); }
// the int64 tables, in this order: r0 of the slots [B] | r0 placed for the next swap [B] | r0 of the last converged fits [B] |
// (i_lo, i_hi) [B][2] | the init points in full-frame rows [B][n_init_max][2]
struct BandTables {
  size_t off_r0, off_pend, off_fit, off_lohi, off_init, count;
};
inline BandTables band_tables(int B, int n_init_max) {
  BandTables t;
  t.off_r0 = 0;
  t.off_pend = (size_t)B;
  t.off_fit = 2 * (size_t)B;
  t.off_lohi = 3 * (size_t)B;
  t.off_init = 5 * (size_t)B;
  t.count = 5 * (size_t)B + (size_t)B * 2 * (size_t)n_init_max;
  return t;
}
inline size_t band_table_bytes(int B, int n_init_max) { return band_tables(B, n_init_max).count * sizeof(long long); }

}  // namespace gpet
