// Part of gpet_kernels.hip (included there, inside namespace gpet, in this order): shared device helpers (block sums, the XCD-aware workgroup -> (edge, part) map, correlation functions).
#define WAVE 64

// ---------------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------------

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}

// value of one lane (the same for the whole wave) in every lane: two v_readlane_b32 into scalar registers
__device__ __forceinline__ double wave_bcast(double v, int src_lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, src_lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src_lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Sum over the whole workgroup; result returned to every thread.  sh: >= 16 doubles.
__device__ __forceinline__ double block_sum(double v, double* sh) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < nw; ++i) t += sh[i];
  return t;
}

// Workgroup id -> (edge, part) such that the parts of one edge share an XCD.  The dispatcher deals consecutive workgroup
// ids round the 8 XCDs (cdna_hip_programming.md T1), so with the plain (part, edge) grid the parts of an edge sit on
// different XCDs and each pulls the edge's shared operand -- or the cache lines it shares with its neighbours -- through
// its own L2.  Bijective for any grid size.  Grid: parts along x (and y), edges along the last used dimension.
__device__ __forceinline__ void xcd_edge_part(int nparts, int& edge, int& part) {
  const int nwg = (int)(gridDim.x * gridDim.y * gridDim.z);
  const int bid = (int)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z));
#ifdef GPET_NO_XCD_REMAP  // (A/B builds)
  const int wg = bid;
#else
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
#endif
  edge = wg / nparts;
  part = wg - edge * nparts;
}

// General-nu Matern correlation (sklearn kernels.py Matern.__call__, the Bessel-K branch the reference reaches with
// kernel_options = {'kernel': 'Matern', 'nu': ...}, gpet.py:134):
//   rho(r) = 2^(1-nu) / Gamma(nu) (sqrt(2 nu) r)^nu K_nu(sqrt(2 nu) r)  =  1 / Gamma(nu) int exp(nu s - e^s - q e^-s) ds,
// q = nu r^2 / 2  (substitute u = e^s in the Gamma-mixture-of-Gaussians form of x^nu K_nu(x)).  The integrand decays
// doubly exponentially on both sides, so the trapezoid rule converges geometrically: absolute error <= 4e-14 for
// 0.1 <= nu <= 170 with the step below (~60-600 nodes; ~1e-13 at nu = 500 and ~6e-13 at nu = 1000, where nu s itself
// carries that rounding), pinned against an exact reference by tests/test_gpu_matern_nu.py.  Also d rho / d log(length_scale)
// = 2 q / Gamma(nu) int exp((nu - 1) s - e^s - q e^-s) ds -- analytic, where sklearn differentiates numerically.
// inv_gamma: 1 / Gamma(nu) for nu <= 170; above, it is -lgamma(nu) < 0 instead, folded into the exponent (+ 0.0 at
// nu <= 170: the same arithmetic bit for bit).  Gamma(nu) itself is finite up to nu = 171.62, but the running sum,
// ~Gamma(nu) / h, overflows from nu ~ 170.97 and the peak term exp(nu s - e^s) from nu ~ 171.3.
// r == 0 (a zero distance off a self-kernel's diagonal; callers write the diagonal themselves) is evaluated at eps with
// a zero derivative, as sklearn does: it adds eps to exact zeros, and its forward difference of two equal values is 0.
// 0.01 <= nu <= 1000 (nu_to_code).
__device__ double matern_gen(double nu, double inv_gamma, double r, double* dlogl) {
  const bool at_zero = (r == 0.0);
  if (at_zero) r = 2.220446049250313e-16;  // np.finfo(float).eps
  const double lsh = inv_gamma > 0.0 ? 0.0 : inv_gamma;
  const double scale = inv_gamma > 0.0 ? inv_gamma : 1.0;
  const double q = 0.5 * nu * r * r;
  double h = 0.45 * rsqrt(nu);
  if (h > 0.2) h = 0.2;
  const double s_hi = log(45.0 + 4.0 * nu) + 0.5;
  double lo_a;
  if (dlogl != nullptr && nu > 1.0) lo_a = -40.0 / fmin(nu, fmax(nu - 1.0, 0.25));
  else lo_a = -40.0 / fmin(nu, 1.0);
  double s_lo = lo_a;
  if (q > 0.0) s_lo = fmax(log(q / 45.0), lo_a);
  const int n0 = (int)floor(s_lo / h), n1 = (int)ceil(s_hi / h);
  double sum = 0.0, dsum = 0.0;
  for (int k = n0; k <= n1; ++k) {
    const double sv = (double)k * h;
    const double es = exp(sv);
    const double w = exp(nu * sv - es - q / es + lsh);
    sum += w;
    dsum += w / es;
  }
  if (dlogl != nullptr) *dlogl = at_zero ? 0.0 : 2.0 * q * h * dsum * scale;
  return h * sum * scale;
}

// sklearn kernels.py RBF / Matern on pre-scaled 1-D inputs a = x_i / l, b = x_j / l.
__device__ __forceinline__ double corr_fn(const EdgeDev& E, double a, double b) {
  const double d = a - b;
  const double d2 = d * d;
  if (E.kernel_type == GPET_KERNEL_RBF) return exp(-0.5 * d2);
  const double r = sqrt(d2);
  if (E.nu_code == 0) return exp(-r);
  if (E.nu_code == 1) {
    const double k = r * 1.7320508075688772;  // math.sqrt(3)
    return (1.0 + k) * exp(-k);
  }
  if (E.nu_code == 3) return matern_gen(E.nu_gen, E.inv_gamma_nu, r, nullptr);
  const double k = r * 2.23606797749979;  // math.sqrt(5)
  return (1.0 + k + k * k / 3.0) * exp(-k);
}
// The same for two PIXEL coordinates of the loop (integer lags, constructor length scale): general nu reads the lag
// table built at construction instead of integrating again.
__device__ __forceinline__ double corr_px(const EdgeDev& E, double xi, double xj, double length) {
  if (E.kernel_type == GPET_KERNEL_MATERN && E.nu_code == 3 && E.tab_ok) {
    const double lag = fabs(xi - xj);
    return E.rho_tab[(int)(lag + 0.5)];
  }
  return corr_fn(E, xi / length, xj / length);
}

// A pointer the compiler knows to be GLOBAL memory.  The buffers of an edge are pointers read from its EdgeDev record, which the
// compiler can only treat as generic: every access becomes a FLAT instruction, and a FLAT instruction counts in BOTH wait
// counters (it might be an LDS access), so a wait for an LDS operand (lgkmcnt) can end up waiting for global stores issued
// before it.  Tried on the sample GEMM as the explanation of its store cost: global_store / global_load instead of flat_*
// take 0-5 % (1.92 -> 1.82-1.91 ms per 1 024 edges) -- kept, but not the explanation.
#define GPET_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ GPET_GLOBAL T* as_global(T* p) {
  return (GPET_GLOBAL T*)p;
}
template <typename T>
__device__ __forceinline__ const GPET_GLOBAL T* as_global(const T* p) {
  return (const GPET_GLOBAL T*)p;
}
