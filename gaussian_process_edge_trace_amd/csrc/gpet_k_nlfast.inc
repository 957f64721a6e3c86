// Part of gpet_kernels.hip (included there, inside namespace gpet): a0: fast-mode non-local means of raw frames, the reference's
// gpet_utils.denoise 'nl' with the library's default fast_mode=True = scikit-image 0.18.3's denoise_nl_means on a 2-D frame.  The
// arithmetic, its order, the shift table, the groups and the workspace: gpet_nlfast_plan.h.
// ---------------------------------------------------------------------------------------
// Image blockIdx.z of a launch is frame img0 + blockIdx.z of the device pointer tables and workspace blockIdx.z of the chunk
// (`stride` doubles apart): P [nr nc] | W [M N] | R [M N] | the planes I of the group's shifts [nr nc each].

// Frame -> P, the frame widened to f64 and padded by `pad` with numpy's 'reflect'.  One thread per cell of the padded frame.
template <typename T>
__global__ void __launch_bounds__(NLF_THREADS) k_nlf_pad(const T* const* __restrict__ src, int img0, double* __restrict__ ws, size_t stride, int M,
                                                         int N, int pad) {
  const int nc = N + 2 * pad;
  const size_t cells = (size_t)(M + 2 * pad) * nc, e = (size_t)blockIdx.x * NLF_THREADS + threadIdx.x;
  if (e >= cells) return;
  const int r = (int)(e / nc), c = (int)(e - (size_t)r * nc);
  const T* __restrict__ img = src[img0 + blockIdx.z];
  ws[(size_t)blockIdx.z * stride + e] = (double)img[(size_t)nlm_mirror(r - pad, M) * N + nlm_mirror(c - pad, N)];
}

// lane `from` (uniform) of x
__device__ inline double nlf_read_lane(double x, int from) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), from), __builtin_amdgcn_readlane(__double2loint(x), from));
}
// x of lane l - 1 (lane 0 keeps its own): two wave-wide DPP shifts, no LDS round trip in the chain
__device__ inline double nlf_from_lane_below(double x) {
  const int hi = __double2hiint(x), lo = __double2loint(x);
  return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, 0x138 /* wave_shr:1 */, 0xf, 0xf, false),
                          __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false));
}

// The integral image of shift shift0 + blockIdx.x into plane blockIdx.x of the frame's workspace: ONE WAVE, rows NLF_STRIP at a
// time.  In step k of a strip lane l is at cell (r0 + l, k - l): `v` is its own previous cell I[r, c-1], `up` = I[r-1, c] the
// previous cell of lane l - 1 (lane 0: the last row of the strip before, read from the plane 64 columns at a time and handed to
// lane 0 out of lane k % 64), `prev_up` = I[r-1, c-1] the `up` of the step before.  A cell outside the shift's ranges is 0, and
// column 0 is outside every range, which is what resets a lane's three values when it enters its row.
// Nothing a step loads depends on the chain: the P values of NLF_AHEAD steps are one block, the block after the running one is
// in flight while it runs, and so is the next piece of the hand-over row.  Every load is unconditional, from an address clamped
// into the shift's range (a lane outside the range discards what it loaded): a load under a lane condition costs a branch and a
// full wait each.
constexpr int NLF_AHEAD = 16;
static_assert(NLF_STRIP == 64 && NLF_STRIP % NLF_AHEAD == 0, "a strip is a wave; the hand-over row is reloaded at whole blocks of steps");
struct NlfBlock {
  double a[NLF_AHEAD], b[NLF_AHEAD];  // P[r, c] and P[r + t_row, c + t_col] of the block's steps
};
__global__ void __launch_bounds__(NLF_STRIP) k_nlf_integral(double* __restrict__ ws, size_t stride, int shift0, int d, int nr, int nc, size_t off_i,
                                                            double var2) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  const NlfShift sh = nlf_shift(d, shift0 + (int)blockIdx.x);
  const int r_lo = nlf_integral_lo(sh.t_row), r_hi = nlf_integral_hi(nr, sh.t_row);
  const int c_lo = nlf_integral_lo(sh.t_col), c_hi = nlf_integral_hi(nc, sh.t_col);
  double* f = ws + (size_t)blockIdx.z * stride;
  const double* P = f;
  double* I = f + off_i + (size_t)blockIdx.x * ((size_t)nr * nc);
  const int steps = nc + NLF_STRIP - 1;
  for (int r0 = 0; r0 < nr; r0 += NLF_STRIP) {
    const int r = r0 + lane;
    const bool row_live = r < nr, row_in = r >= r_lo && r < r_hi;
    const double* Pa = P + (size_t)(row_in ? r : 0) * nc;
    const double* Pb = P + (size_t)(row_in ? r + sh.t_row : 0) * nc + sh.t_col;
    double* Ir = I + (size_t)(row_live ? r : 0) * nc;
    const double* Iup = I + (size_t)(r0 > 0 ? r0 - 1 : 0) * nc;
    double v = 0.0, prev_up = 0.0, up_row = 0.0;
    auto load = [&](int k0, NlfBlock& B) {
#pragma unroll
      for (int j = 0; j < NLF_AHEAD; ++j) {
        int c = k0 + j - lane;
        c = c < c_lo ? c_lo : (c > c_hi - 1 ? c_hi - 1 : c);
        B.a[j] = Pa[c];
        B.b[j] = Pb[c];
      }
    };
    auto load_up = [&](int k0) {  // (r0 is uniform)
      const int c = k0 + lane < nc ? k0 + lane : nc - 1;
      return r0 > 0 ? Iup[c] : 0.0;
    };
    double up_next = load_up(0);
    auto run = [&](int k0, const NlfBlock& B) {
      if ((k0 & (NLF_STRIP - 1)) == 0) {
        up_row = up_next;
        up_next = load_up(k0 + NLF_STRIP);
      }
#pragma unroll
      for (int j = 0; j < NLF_AHEAD; ++j) {
        const int k = k0 + j, c = k - lane;
        const bool in = row_in && c >= c_lo && c < c_hi;
        double up = nlf_from_lane_below(v);
        const double handed = nlf_read_lane(up_row, k & (NLF_STRIP - 1));
        if (lane == 0) up = handed;
        const double t = B.a[j] - B.b[j];
        const double q = (0.0 + t * t) - var2;
        const double cell = ((q + up) + v) - prev_up;
        v = in ? cell : 0.0;
        prev_up = up;
        if (row_live && c >= 0 && c < nc) Ir[c] = v;
      }
    };
    NlfBlock B0, B1;
    load(0, B0);
    for (int k0 = 0; k0 < steps; k0 += 2 * NLF_AHEAD) {  // (steps past the last are no lane's: c >= nc everywhere)
      load(k0 + NLF_AHEAD, B1);
      run(k0, B0);
      load(k0 + 2 * NLF_AHEAD, B0);
      run(k0 + NLF_AHEAD, B1);
    }
    __threadfence();  // the strip's last row is read by other lanes of this wave in the next strip
  }
}

// One pair's term at a pixel: the pair's first pixel is (row, col) of plane I, `val` the value the term adds.
__device__ inline void nlf_term(const double* __restrict__ I, int nc, int row, int col, int off, double h2s2, double alpha, double val, double& W,
                                double& R) {
#pragma clang fp contract(off)
  const double* hi = I + (size_t)(row + off) * nc + col;
  const double* lo = I + (size_t)(row - off) * nc + col;
  const double dd = ((hi[off] + lo[-off]) - lo[off]) - hi[-off];
  const double dist = (dd > 0.0 ? dd : 0.0) / h2s2;
  if (dist > NLM_CUTOFF) return;
  const double w = alpha * nlm_fexp(-dist);
  W = W + w;
  R = R + w * val;
}

// The sums of a group of shifts (shift0 .. shift0 + count - 1, their planes in the workspace), one thread per OUTPUT pixel, in
// the order the scatter reaches the pixel.  W and R come from the workspace (first group: zero) and go back to it; after the last
// group R / W goes to dst[img0 + z] (f64, M x N).
__global__ void __launch_bounds__(NLF_THREADS) k_nlf_gather(double* __restrict__ ws, size_t stride, double* const* __restrict__ dst, int img0, int M,
                                                            int N, int off, int d, int shift0, int count, int last, size_t off_w, size_t off_r,
                                                            size_t off_i, double h2s2) {
#pragma clang fp contract(off)
  const size_t e = (size_t)blockIdx.x * NLF_THREADS + threadIdx.x;
  if (e >= (size_t)M * N) return;
  const int pad = off + d + 1, nr = M + 2 * pad, nc = N + 2 * pad;
  const int pr = pad + (int)(e / N), pc = pad + (int)(e % N);
  double* f = ws + (size_t)blockIdx.z * stride;
  const double* P = f;
  double W = shift0 ? f[off_w + e] : 0.0, R = shift0 ? f[off_r + e] : 0.0;
  for (int q = 0; q < count; ++q) {
    const NlfShift sh = nlf_shift(d, shift0 + q);
    const double* I = f + off_i + (size_t)q * ((size_t)nr * nc);
    const double own = P[(size_t)(pr + sh.t_row) * nc + pc + sh.t_col], partner = P[(size_t)(pr - sh.t_row) * nc + pc - sh.t_col];
    if (nlf_partner_first(sh.t_row, sh.t_col)) {
      nlf_term(I, nc, pr - sh.t_row, pc - sh.t_col, off, h2s2, sh.alpha, partner, W, R);
      nlf_term(I, nc, pr, pc, off, h2s2, sh.alpha, own, W, R);
    } else {  // ((0, 0): the pair is its own partner, the same term twice)
      nlf_term(I, nc, pr, pc, off, h2s2, sh.alpha, own, W, R);
      nlf_term(I, nc, pr - sh.t_row, pc - sh.t_col, off, h2s2, sh.alpha, partner, W, R);
    }
  }
  if (last) {
    dst[img0 + blockIdx.z][e] = R / W;
  } else {
    f[off_w + e] = W;
    f[off_r + e] = R;
  }
}
