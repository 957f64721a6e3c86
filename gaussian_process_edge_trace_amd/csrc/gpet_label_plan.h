// Label maps: the two rules that rasterise traces into uint8 masks, as plain data and plain arithmetic.  No HIP: the
// host compiler alone builds this header (tests/test_label_plan.py compiles it into a shim with -ffp-contract=off), and the kernels of
// gpet_k_label.inc call label_col_index / label_clamp / label_count / label_crossing on the device.  tests/label_ref.py restates both
// rules with numpy.
//
// Rule 1, row maps (M x N).  Contributing edge e has a grid [x_st, x_st + len - 1], int64 rows t_e[k] and a map index map_of[e] in
// [-1, n_maps) (-1: in no map).  Its threshold at frame column c:
//   k            c - x_st inside the grid; with LABELS_EXTEND 0 left of it and len - 1 right of it; else the edge does not count at c
//   T_e[c]       M where the edge does not count or t_e[k] == LABEL_NO_ROW; else min(max(t_e[k], 0), M)
//   label        label[f][r][c] = #{e : map_of[e] = f, r >= T_e[c]}
//   thick        thick[f][l][c] = #{r in [0, M) : label[f][r][c] = l}, int32 [n_maps][L + 1][N], L the most edges on one map
// LABELS_TRANSPOSED stores every map as N x M, out[c][r] = label[r][c]; thick is the same either way.
//
// Rule 2, frame maps of closed outlines (Ms x Ns).  Contour e has n vertices (X_j, Y_j), f64, 4 <= n <= LABEL_VERTS_MAX.  For the pixel
// (px, py), integers taken as doubles, and every j with (xi, yi) = V_j, (xj, yj) = V_{(j + 1) mod n}:
//   straddle     (yi > py) != (yj > py)
//   products     a = (px - xi) * (yj - yi),  b = (xj - xi) * (py - yi): every difference and every product rounded once, no division
//   toggle       yj > yi ? a < b : a > b
// The pixel is inside when the toggles are odd in number; label_xy[f][py][px] counts the contours of map f it is inside.  A contour
// with a vertex that is not finite contributes nothing.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__)
#define GPET_LABEL_HD __host__ __device__
#else
#define GPET_LABEL_HD
#endif
// (no fused multiply-add in the functions the kernel shares with the host, whatever the compiler's default)
#if defined(__clang__)
#define GPET_LABEL_NO_FMA _Pragma("clang fp contract(off)")
#else
#define GPET_LABEL_NO_FMA
#endif

namespace gpet {

constexpr int LABEL_EDGES_MAX = 32;                 // edges (contours) on one map: a label fits a byte with room to spare
constexpr int LABEL_VERTS_MIN = 4;
constexpr int LABEL_VERTS_MAX = 4096;               // 2 * 8 bytes a vertex: 64 KB of LDS
constexpr long long LABEL_NO_ROW = INT64_MIN;       // a row that does not count (what a non-finite mean rounds to)
constexpr long long LABEL_CELLS_MAX = 1LL << 31;    // M * N of one map
constexpr unsigned int LABELS_EXTEND = 1u, LABELS_TRANSPOSED = 2u, LABELS_OUT_ON_DEVICE = 4u;

// ---- the launch shapes ------------------------------------------------------------------------------------------------------------
constexpr int LABEL_THREADS = 256;                  // lanes of a fill workgroup
constexpr int LABEL_CHUNK = 16;                     // bytes a lane stores at once: one global_store_dwordx4
constexpr int LABEL_SPAN = LABEL_THREADS * LABEL_CHUNK;  // flattened map bytes a workgroup covers
constexpr int LABEL_LDS_INTS = 12288;               // thresholds staged at once: 48 KB
constexpr int LABEL_XY_LDS_MAX = 2 * 8 * LABEL_VERTS_MAX + 16;  // the vertices of one contour and a flag behind them

// columns whose thresholds a fill workgroup stages: row-major maps cover min(N, SPAN) columns; transposed ones, whose flattened bytes
// run down a column of M rows, at most SPAN / M + 2
inline int label_stage_cols(int M, int N, bool transposed) {
  if (!transposed) return N < LABEL_SPAN ? N : LABEL_SPAN;
  const long long n = LABEL_SPAN / (long long)M + 2;
  return n < N ? (int)n : N;
}
// edges staged per pass over a workgroup's chunk (at least 1, at most L)
inline int label_stage_edges(int cols, int L) {
  int g = LABEL_LDS_INTS / (cols > 0 ? cols : 1);
  if (g < 1) g = 1;
  return g < L ? g : L;
}
// workgroups that cover `bytes` flattened map bytes starting `mis` bytes past a 16-byte boundary
inline unsigned int label_blocks(long long bytes, int mis) { return (unsigned int)((bytes + mis + LABEL_SPAN - 1) / LABEL_SPAN); }

// int32 elements of thick; 0 when the arguments are out of range
inline long long label_thick_count(long long n_maps, long long L, long long N) {
  if (n_maps < 1 || L < 1 || L > LABEL_EDGES_MAX || N < 1 || N > LABEL_CELLS_MAX) return 0;
  if (n_maps > (1LL << 40) / ((L + 1) * N)) return 0;
  return n_maps * (L + 1) * N;
}

// ---- Rule 1 -----------------------------------------------------------------------------------------------------------------------
// k of column c, or -1 where the edge does not count
GPET_LABEL_HD inline long long label_col_index(long long c, long long x_st, long long len, bool extend) {
  if (c < x_st) return extend ? 0 : -1;
  if (c >= x_st + len) return extend ? len - 1 : -1;
  return c - x_st;
}
// T of a row t
GPET_LABEL_HD inline int label_clamp(long long t, int M) {
  if (t == LABEL_NO_ROW) return M;
  return t < 0 ? 0 : (t > (long long)M ? M : (int)t);
}
GPET_LABEL_HD inline int label_threshold(const long long* rows, long long x_st, long long len, long long c, int M, bool extend) {
  const long long k = label_col_index(c, x_st, len, extend);
  return k < 0 ? M : label_clamp(rows[k], M);
}
// the label of row r from the n thresholds T[0], T[stride], ... of one column
GPET_LABEL_HD inline int label_count(const int* T, int n, size_t stride, int r) {
  int v = 0;
  for (int e = 0; e < n; ++e) v += r >= T[(size_t)e * stride] ? 1 : 0;
  return v;
}

// ---- Rule 2 -----------------------------------------------------------------------------------------------------------------------
GPET_LABEL_HD inline bool label_crossing(double px, double py, double xi, double yi, double xj, double yj) {
  GPET_LABEL_NO_FMA
  if ((yi > py) == (yj > py)) return false;
  const double dx0 = px - xi, dy0 = yj - yi, dx1 = xj - xi, dy1 = py - yi;
  const double a = dx0 * dy0;
  const double b = dx1 * dy1;
  return yj > yi ? a < b : a > b;
}
GPET_LABEL_HD inline bool label_finite(double v) { return fabs(v) < INFINITY; }
// xy: n pairs (x, y).  The host's form; the kernel stages the vertices in LDS and runs the same loop
inline bool label_inside(double px, double py, const double* xy, int n) {
  bool in = false;
  for (int j = 0; j < n; ++j) {
    const int q = j + 1 == n ? 0 : j + 1;
    if (label_crossing(px, py, xy[2 * j], xy[2 * j + 1], xy[2 * q], xy[2 * q + 1])) in = !in;
  }
  return in;
}
// a vertex of a contour traced on polar frames (gpet_polar_plan.h): polar_to_xy's arithmetic at the integer row t, not clamped
GPET_LABEL_HD inline void label_vertex(long long t, double r0, double dr, double cx, double cy, double cos_t, double sin_t, double* x, double* y) {
  GPET_LABEL_NO_FMA
  const double step = (double)t * dr;
  const double rho = r0 + step;
  const double px = rho * cos_t, py = rho * sin_t;
  *x = cx + px;
  *y = cy + py;
}

// ---- the refusals, in the order they are checked: 0, or 1 with the reason in msg ------------------------------------------------------
// what every form shares: the pointers, the frame, n_maps and the map table.  noun: "edge" or "contour".  L_out: the most members on a map
inline int label_check_maps(bool null_arg, long long M, long long N, int n, const int32_t* map_of, int n_maps, const char* noun, int* L_out,
                            char* msg, size_t cap) {
  if (null_arg || !map_of) return snprintf(msg, cap, "label maps: a null pointer"), 1;
  if (M < 2 || N < 2) return snprintf(msg, cap, "label maps: frames must be at least 2 x 2 pixels"), 1;
  if (M > LABEL_CELLS_MAX / N) return snprintf(msg, cap, "label maps: a map exceeds 2^31 pixels (M * N)"), 1;
  if (n_maps < 1) return snprintf(msg, cap, "label maps: n_maps must be at least 1"), 1;
  for (int e = 0; e < n; ++e)
    if (map_of[e] < -1 || map_of[e] >= n_maps)
      return snprintf(msg, cap, "label maps: map_of[%d] = %d lies outside [-1, n_maps = %d)", e, (int)map_of[e], n_maps), 1;
  int L = 0;
  for (int f = 0; f < n_maps; ++f) {
    int cnt = 0;
    for (int e = 0; e < n; ++e) cnt += map_of[e] == f ? 1 : 0;
    if (cnt == 0) return snprintf(msg, cap, "label maps: map %d has no %s", f, noun), 1;
    if (cnt > LABEL_EDGES_MAX) return snprintf(msg, cap, "label maps: map %d has more than 32 %ss (%d)", f, noun, cnt), 1;
    L = cnt > L ? cnt : L;
  }
  if (L_out) *L_out = L;
  return 0;
}
// Rule 1: the grids of all edges
inline int label_check(long long M, long long N, int n_edges, const int32_t* x_st, const int32_t* len, bool rows_null, const int32_t* map_of,
                       int n_maps, bool out_null, int* L_out, char* msg, size_t cap) {
  if (label_check_maps(rows_null || out_null || !x_st || !len, M, N, n_edges, map_of, n_maps, "edge", L_out, msg, cap)) return 1;
  for (int e = 0; e < n_edges; ++e)
    if (len[e] < 1 || x_st[e] < 0 || (long long)x_st[e] + len[e] > N)
      return snprintf(msg, cap, "label maps: the grid of edge %d lies outside [0, N) (x_st = %d, len = %d, N = %lld)", e, (int)x_st[e],
                      (int)len[e], N), 1;
  return 0;
}
// Rule 2: the vertex counts of all contours
inline int label_check_xy(long long Ms, long long Ns, int n_contours, const int32_t* n_vert, bool xy_null, const int32_t* map_of, int n_maps,
                          bool out_null, int* L_out, char* msg, size_t cap) {
  if (label_check_maps(xy_null || out_null || !n_vert, Ms, Ns, n_contours, map_of, n_maps, "contour", L_out, msg, cap)) return 1;
  for (int e = 0; e < n_contours; ++e)
    if (n_vert[e] < LABEL_VERTS_MIN || n_vert[e] > LABEL_VERTS_MAX)
      return snprintf(msg, cap, "label maps: contour %d has %d vertices, outside [4, 4096]", e, (int)n_vert[e]), 1;
  return 0;
}
// Rule 2 from a batch: a contributing edge spans the closed contour of the polar spec, seam to seam
inline int label_check_closed(int e, int x_st, int x_en, int pad, int n_theta, char* msg, size_t cap) {
  if (x_st == pad && x_en == pad + n_theta) return 0;
  return snprintf(msg, cap, "label maps: edge %d does not span the closed contour (x_st = %d, x_en = %d; pad = %d, pad + n_theta = %d)", e, x_st,
                  x_en, pad, pad + n_theta), 1;
}

// The members of every map in the order the kernels read them: used[map_off[f] .. map_off[f + 1]) are the edges of map f, ascending
// (used: room for n entries, map_off: n_maps + 1).  Returns their number.
inline int label_map_table(int n, const int32_t* map_of, int n_maps, int32_t* used, int32_t* map_off) {
  int k = 0;
  for (int f = 0; f < n_maps; ++f) {
    map_off[f] = k;
    for (int e = 0; e < n; ++e)
      if (map_of[e] == f) used[k++] = e;
  }
  map_off[n_maps] = k;
  return k;
}

}  // namespace gpet
