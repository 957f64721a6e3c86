/*
 * gpet_hip.h -- C ABI of libgpet_hip.so: the MI355X (gfx950) implementation of the
 * GP posterior-update + posterior-sampling + curve-scoring hot path of
 * gp_edge_tracing.gpet.GP_Edge_Tracing (reference: jaburke166/gaussian_process_edge_trace).
 *
 * The reference is pure Python and has no FFI; each entry point below names the reference
 * interface (file:line under /root/reference) whose arithmetic it replaces.  The Python host
 * (gaussian_process_edge_trace_amd/) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain C, POD only, no exceptions; every call returns a gpet_status (0 = ok);
 *     gpet_last_error(ctx) gives the message of the last failure on that context.
 *   - M rows (y), N columns (x) image; Lg = edge_length = x_en - x_st + 1 grid points;
 *     n = training points (inits + observations); S = posterior samples.
 *   - a "batch" holds B independent edges that are processed together (blockIdx.y = edge).
 *     A single edge is a batch of 1.
 *   - host pointers unless a parameter says "device".  All work is enqueued on the
 *     context's HIP stream; calls that return data to the host synchronise that stream.
 *   - handles are not thread-safe individually; distinct contexts may be used from
 *     distinct host threads.
 */
#ifndef GPET_HIP_H
#define GPET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPET_ABI_VERSION 1

typedef enum gpet_status {
  GPET_OK = 0,
  GPET_ERR_BAD_ARG = 1,
  GPET_ERR_HIP = 2,          /* a HIP runtime call failed (message has the HIP error) */
  GPET_ERR_NOT_PD = 3,       /* Cholesky met a non-positive pivot (sklearn_gpr.py:306-314 LinAlgError) */
  GPET_ERR_ITER_CAP = 4,     /* trace did not converge within the iteration cap */
  GPET_ERR_RANK_CAP = 5,     /* posterior covariance rank exceeded the factor capacity */
  GPET_ERR_UNSUPPORTED = 6,  /* e.g. a Matern nu that is not a positive finite number */
  GPET_ERR_NO_DEVICE = 7,
  GPET_ERR_STATE = 8         /* call sequence error (stage input not produced yet) */
} gpet_status;

typedef enum gpet_kernel_type { GPET_KERNEL_RBF = 0, GPET_KERNEL_MATERN = 1 } gpet_kernel_type;

/* Clamped constructor arguments of GP_Edge_Tracing.__init__ (gpet.py:95-158), resolved by the host. */
typedef struct gpet_params {
  int32_t kernel_type;   /* gpet_kernel_type                  gpet.py:133,142 */
  double nu;             /* Matern smoothness: 0.5 / 1.5 / 2.5 in closed form, any other nu > 0 through the
                          * Bessel form (quadrature; lag table for the loop)      gpet.py:134,143 */
  double sigma_f;        /* amplitude                         gpet.py:131,147 */
  double length_scale;   /*                                   gpet.py:132,151 */
  double noise_y;        /*                                   gpet.py:98 */
  int32_t n_samples;     /* S (already clamped)               gpet.py:99 */
  int32_t n_keep;        /* int(keep_ratio*N_samples) raw     gpet.py:118 */
  int32_t delta_x;       /* clamped                           gpet.py:105 */
  int32_t pixel_thresh;  /* clamped                           gpet.py:103 */
  double score_thresh;   /* clamped initial value             gpet.py:104 */
  int32_t fix_endpoints; /*                                   gpet.py:108,161 */
  int32_t x_st, x_en;    /* from the UNSORTED init            gpet.py:96 */
  int32_t n_init;        /* rows of init                      gpet.py:112 */
  int32_t obs_cap;       /* capacity for observations (>= any obs set passed later) */
  int32_t factor_cap;    /* max rank kept by the eigen-factor sampler (0 = library default) */
  int32_t z_cols;        /* normal columns stored per sample (0 = default: factor_cap; Lg = full stream) */
  double jitter;         /* GPR alpha, 1e-6                    gpet.py:155 */
} gpet_params;

/* Named per-edge device buffers readable/writable through gpet_batch_read/_write (tests, injection). */
typedef enum gpet_buf {
  GPET_BUF_X_TRAIN = 0,   /* f64 [n]        sorted training x             gpet.py:212-223 */
  GPET_BUF_Y_TRAIN = 1,   /* f64 [n]        y/y_s - mean                  sklearn_gpr.py:227 */
  GPET_BUF_CHOL = 2,      /* f64 [n_cap*n_cap] row-major, lower = L       sklearn_gpr.py:307 */
  GPET_BUF_ALPHA = 3,     /* f64 [n]                                       sklearn_gpr.py:316 */
  GPET_BUF_MEAN = 4,      /* f64 [Lg]       posterior mean (scaled units)  sklearn_gpr.py:382-385 */
  GPET_BUF_STD = 5,       /* f64 [Lg]                                      sklearn_gpr.py:414-436 */
  GPET_BUF_COV = 6,       /* f64 [Lg*Lg]                                   sklearn_gpr.py:398-403 */
  GPET_BUF_FACTOR = 7,    /* f64 [rows*Lg]  rows of sqrt(s)*v              numpy mvn via sklearn_gpr.py:464 */
  GPET_BUF_EIGVALS = 8,   /* f64 [factor rows]                             */
  GPET_BUF_NORMALS = 9,   /* f64 [S*z_cols] standard normals, row = sample sklearn_gpr.py:464 */
  GPET_BUF_SAMPLES = 10,  /* f64 [S*Lg]     row = sample, pixel units      gpet.py:260-261 */
  GPET_BUF_COSTS = 11,    /* f64 [S]                                       gpet.py:438-440 */
  GPET_BUF_BEST_IDX = 12, /* i32 [n_keep]                                  gpet.py:443 */
  GPET_BUF_BEST_COSTS = 13, /* f64 [n_keep]                                gpet.py:445 */
  GPET_BUF_SCALARS = 14,  /* gpet_scalars                                  */
  GPET_BUF_OBS = 15,      /* i64 [n_obs*2] xy                              gpet.py:857 */
  GPET_BUF_KDE = 16,      /* f32 [M*N]      normalised curve KDE           gpet.py:648
                           *                (as left by gpet_select_pixels; gpet_trace_iterate keeps the raw density of
                           *                 the band rows only and normalises inside its pixel kernels) */
  GPET_BUF_GRAD_KDE = 17, /* f32 [M*N]      normalised gradient KDE        gpet.py:127 */
  GPET_BUF_GRAD = 18,     /* f32 [M*N]      normalised gradient image      gpet.py:97 */
  GPET_BUF_NOISE_W = 19,  /* f64 [n]        per-point noise weights        gpet.py:209-213 */
  GPET_BUF_FIN_TRAIN = 20,  /* f64 [3][n_cap] converged fit: standardised x | y | noise weights, n = n_init + n_obs used
                             *                (gpet.py:235-238; sklearn_gpr.py:229-234), as gpet_final_fit_all built them */
  GPET_BUF_FIN_PAR = 21,  /* f64 [12]       optimum and transforms: constant, length_scale, noise_level, X_m, X_s, y_m,
                           *                y_s, m2, s2, 0, 0, 0 */
  GPET_BUF_FIN_STARTS = 22, /* f64 [13][3]  theta0 + the 12 restart points of the last gpet_final_fit_all
                             *                (gpet.py:244-245; sklearn_gpr.py:283-288) */
  GPET_BUF_FIN_OUT = 23,  /* f64 [2][Lg]   converged fit's output block: posterior mean in pixels, then std in standardised
                           *                units (gpet.py:266), as gpet_final_fit_all left them -- what gpet_batch_results and
                           *                gpet_batch_warm_start read.  Writable (tests inject fits no scene produces): exactly
                           *                2 * Lg * 8 bytes; a write changes no state flag, so a record or a warm start after it
                           *                reads the written values where the last converged fit allowed one */
  GPET_BUF_KDE_TILES = 24, /* i32 [ceil(N/16) + 1][2]  what the fused curve KDE left beside GPET_BUF_KDE: per 16-column tile the
                           *                first and last image row of its band (written by the loop's form only,
                           *                gpet_select_pixels_loop / gpet_trace_iterate; (M, -1): no band), then the ordered
                           *                keys of the raw density's minimum and maximum as two u32.  Read only (tests) */
  /* What the structured loop path (prior eigenbasis of the pixel grid) keeps.  Read only (tests); gpet_batch_read refuses them
   * with GPET_ERR_BAD_ARG on a batch that is not structured (gpet_batch_info: structured == 0, at creation or after an
   * off-grid observation).  r0 is gpet_batch_info's. */
  GPET_BUF_STRUCT_Q0 = 25,   /* f64 [r0][Lg]  unit eigenvectors of the grid's unit-amplitude correlation matrix, fixed at creation */
  GPET_BUF_STRUCT_LAM0 = 26, /* f64 [r0]      their eigenvalues */
  GPET_BUF_STRUCT_H = 27     /* f64 [r0][r0]  H = amp * diag(lam0) - U^T U of the current observation set, compact (on the device its
                              *                rows have the factor capacity's stride).  Valid after stage 121 of gpet_profile_stage
                              *                and before stage 122 only: the eigen-decomposition's warm start rotates it in place,
                              *                so after stage 122 or a loop iteration its contents are unspecified */
} gpet_buf;

/* Per-edge scalar state kept on the device (GPET_BUF_SCALARS). */
typedef struct gpet_scalars {
  double y_s;          /* std(y)+1                              gpet.py:228 */
  double amp;          /* sigma_f^2 / y_s^2                     gpet.py:230 */
  double y_mean;       /* _y_train_mean                         sklearn_gpr.py:222 */
  double y_std;        /* _y_train_std                          sklearn_gpr.py:223 */
  double score_thresh; /* persists across iterations            gpet.py:595 */
  double lml;          /* diagnostics (Jacobi sweeps of the last factorisation) */
  int32_t n;           /* training points of the last fit */
  int32_t n_obs;       /* current observation count */
  int32_t rank;        /* rows of the factor */
  int32_t status;      /* gpet_status raised on the device */
  int32_t iter;        /* iterations done                       gpet.py:865 */
  int32_t done;        /* n_obs >= algo_thresh                  gpet.py:829 */
  int32_t n_removed;   /* curve points outside the image        gpet.py:498-500 */
  int32_t force;       /* set by the per-stage entry points: run the stage even if `done` */
} gpet_scalars;

typedef struct gpet_ctx gpet_ctx;
typedef struct gpet_batch gpet_batch;

/* ---- context ------------------------------------------------------------------------ */
int gpet_abi_version(void);

/* Process-wide tuning switches (no reference counterpart): ONE table (csrc/gpet_options.hip; INTEGRATION.md section 5
 * lists every name with its default, range and meaning).  An option's initial value is the environment variable
 * GPET_<NAME IN CAPITALS> if set, else the table's default; results never depend on an option except where its
 * description says so (cross-check solvers, opt-in modes).
 * gpet_set_option returns the previous value -- "chosen automatically" (-1) is reported as the option's largest value
 * + 1 -- or -1 for an unknown name; values outside an option's range are clamped.  gpet_get_option stores the current
 * value (-1 = automatic) and returns 0, or GPET_ERR_BAD_ARG for an unknown name.  gpet_option_count / gpet_option_info
 * enumerate the table (any out pointer may be NULL; strings are static). */
int gpet_set_option(const char* name, int value);
int gpet_get_option(const char* name, int* value);
/* A batch keeps its OWN copy of the table, taken when it is created: what a batch does is fixed by the options in force at
 * gpet_batch_create and by these two calls, never by a gpet_set_option another thread makes while it runs (every batch entry
 * point reads the batch's copy).  Same return conventions as gpet_set_option / gpet_get_option. */
int gpet_batch_set_option(gpet_batch* b, const char* name, int value);
int gpet_batch_get_option(const gpet_batch* b, const char* name, int* value);
int gpet_option_count(void);
int gpet_option_info(int index, const char** name, int* value, int* def, int* lo, int* hi, const char** doc);
/* stream: a hipStream_t to enqueue on (e.g. torch.cuda.current_stream().cuda_stream), or NULL
 * to let the library create its own. */
int gpet_ctx_create(int device, void* stream, gpet_ctx** out);
void gpet_ctx_destroy(gpet_ctx* ctx);
const char* gpet_last_error(const gpet_ctx* ctx);
int gpet_sync(gpet_ctx* ctx);
void* gpet_ctx_stream(gpet_ctx* ctx);
/* hipEvent timing on the context's stream (bench.py roofline leg). */
int gpet_timer_start(gpet_ctx* ctx);
int gpet_timer_stop_ms(gpet_ctx* ctx, float* ms);

/* ---- a1: gpet_utils.comp_grad_img + normalise (gpet_utils.py:65-119) ------------------ */
/* img f64 [M*N], kern f64 [kh*kw] (host); out f32 [M*N] (host).  True convolution with
 * clamp-to-edge padding, negatives -> 0, float32 min-max normalisation. */
int gpet_grad_image(gpet_ctx* ctx, const double* img, int M, int N, const double* kern, int kh, int kw,
                    float* out);
/* Raw frames in the pixel type the caller has them in; every type converts to float64 exactly, so a frame means what
 * np.asarray(frame, dtype=np.float64) means to gpet_utils.comp_grad_img (gpet_utils.py:95-119). */
#define GPET_PIX_U8 0
#define GPET_PIX_U16 1
#define GPET_PIX_F32 2
#define GPET_PIX_F64 3
/* raw[] are DEVICE pointers on the context's device (a decoded video frame, a tensor an RCCL broadcast filled): read where
 * they lie, no staging and no copy.  Without the flag raw[] are host pointers; the frames go up in chunks of whole images
 * through a small staging ring the context owns. */
#define GPET_RAW_ON_DEVICE 4u
/* Vertical edges (added without a change of GPET_ABI_VERSION: one flag bit, no new export).  The tracer follows an edge that is a
 * function of the column; an edge that runs down the frame is traced on the TRANSPOSE of the frame's gradient image.  With this flag
 * M, N stay the frame as it lies in memory -- M rows of N pixels -- denoising and the kernel are applied to it as it lies, and what
 * is written is the N x M transpose of its M x N gradient image, bit for bit, made on the device in the same pass.  Accepted by
 * gpet_grad_images, gpet_grad_images_dn, gpet_grad_images_multi (out[g] is then f32 [N*M]), by every gpet_batch_create* that takes
 * flags and in gpet_band_images.flags: the batch's image shape is then (N, M), gpet_params.x_st / x_en count frame ROWS, band->H
 * <= N and band->r0 count frame COLUMNS, and gradient images given by the caller (grad[]) are M x N in frame layout as well.
 * init_xy, observations and everything the batch returns are in the BATCH's coordinates -- x a frame row, y a frame column: a C
 * caller swaps its own points.  The batch remembers its orientation: gpet_batch_set_images and gpet_batch_set_raw_images* take
 * frames in frame layout on such a batch and need not repeat the bit; on a batch created without it a set call that carries the
 * bit is refused with GPET_ERR_BAD_ARG and touches nothing.  Calls without a flags argument (gpet_batch_create, gpet_grad_image,
 * gpet_normalise_f32) are unaffected. */
#define GPET_FRAMES_TRANSPOSED 16u
/* gpet_utils.comp_grad_img (gpet_utils.py:95-119) for n_img frames [M*N] of pixel type pix (GPET_PIX_*) in one batched
 * pass: out[g] f32 [M*N] (host) is bit for bit what gpet_grad_image gives for frame g.  The number of kernel launches does
 * not depend on n_img (one convolution per staging chunk, one normalisation).  flags: GPET_RAW_ON_DEVICE.
 * GPET_ERR_BAD_ARG for an unknown pix, a null frame, or a kernel whose patch exceeds 64 KB of LDS. */
int gpet_grad_images(gpet_ctx* ctx, const void* const* raw, int n_img, int pix, int M, int N, const double* kern, int kh,
                     int kw, unsigned int flags, float* const* out);
/* ---- a0: gpet_utils.denoise in front of a1 (gpet_utils.py:122-158) ---------------------- */
/* The four techniques of the reference's denoise() that are deterministic stencils, on the device, for whole stacks:
 * 'median' / 'minimum' (scipy.ndimage.median_filter / minimum_filter: size, mode), 'gaussian' (scipy.ndimage.gaussian_filter:
 * sigma per axis, truncate, mode; order 0) and 'tvc' (skimage.restoration.denoise_tv_chambolle: weight, eps, n_iter_max).
 * The denoised frame has the reference's dtype: the frame's own pixel type for the three filters (integer frames are
 * quantised after each Gaussian pass, as scipy does), float64 for 'tvc' (u8 / u16 enter through img_as_float; an f32 frame is
 * promoted to f64, where the reference would iterate in f32). */
#define GPET_DN_NONE 0
#define GPET_DN_MEDIAN 1
#define GPET_DN_MINIMUM 2
#define GPET_DN_GAUSSIAN 3
#define GPET_DN_TVC 4
#define GPET_DN_MODE_REFLECT 0 /* d c b a | a b c d | d c b a: scipy's default */
#define GPET_DN_MODE_NEAREST 1 /* a a a a | a b c d | d d d d */
typedef struct gpet_denoise {
  int32_t technique;       /* GPET_DN_* */
  int32_t size_y, size_x;  /* median / minimum: the window, at most 81 pixels (9 x 9) */
  int32_t mode;            /* median / minimum / gaussian: GPET_DN_MODE_* */
  double sigma_y, sigma_x; /* gaussian: both above 0 */
  double truncate;         /* gaussian: radius int(truncate * sigma + 0.5); scipy's default 4.0 */
  double weight;           /* tvc: above 0; skimage's default 0.1 */
  double eps;              /* tvc: stop when |E_prev - E| < eps * E_0; skimage's default 2e-4 */
  int32_t n_iter_max;      /* tvc: at least 1; skimage's default 200 */
} gpet_denoise;
/* denoise() of n_img frames [M*N] of pixel type pix in one batched pass: out[g] (host) receives frame g denoised, in the
 * pixel type described above; n_iter_out (host, [n_img], may be NULL): iterations 'tvc' ran on frame g, 0 for the filters.
 * A filter is one kernel launch per staging chunk (the Gaussian two) however many frames the chunk holds; the number of chunks
 * grows with n_img once frames and workspace fill the 64 MB slot.  flags: GPET_RAW_ON_DEVICE.  GPET_ERR_BAD_ARG for
 * technique NONE or unknown, a window above 81 pixels, sigma <= 0, weight <= 0, an unknown mode, n_iter_max < 1, an unknown
 * pix or a null frame. */
int gpet_denoise_images(gpet_ctx* ctx, const void* const* raw, int n_img, int pix, int M, int N, const gpet_denoise* dn,
                        unsigned int flags, void* const* out, int32_t* n_iter_out);
/* gpet_grad_images of the denoised frames, in one device pass: out[g] is bit for bit gpet_grad_images of what
 * gpet_denoise_images returns for frame g.  dn NULL or technique NONE: gpet_grad_images itself. */
int gpet_grad_images_dn(gpet_ctx* ctx, const void* const* raw, int n_img, int pix, int M, int N, const double* kern, int kh,
                        int kw, const gpet_denoise* dn, unsigned int flags, float* const* out);
/* Several kernels on shared frames: a slot table.  n_frames raw frames, n_kern kernels kern[k] of kh[k] x kw[k] (f64, host; the
 * extents may differ and may be even or odd), n_img image slots: slot g is gpet_grad_images_dn of frame frame_of[g] with kernel
 * kernel_of[g], bit for bit -- the two walls of a vessel are a bright-to-dark and a dark-to-bright edge on the same frame.  Every
 * frame is uploaded, denoised (dn; NULL: not at all) and staged on the device once, however many kernels read it.  out[g]
 * (host, f32 [M*N]): slot g.  GPET_ERR_BAD_ARG, gpet_last_error naming the cause, for an index out of range, a frame or a kernel
 * no slot reads, the same (frame, kernel) pair twice (edges that want the same image share a slot through image_of), more than
 * 8 kernels, kernels whose taps and union patch exceed 64 KB of LDS, and whatever gpet_grad_images_dn refuses.  n_kern = 1 with
 * one slot per frame in frame order (frame_of[g] = g) is gpet_grad_images_dn itself. */
int gpet_grad_images_multi(gpet_ctx* ctx, const void* const* raw, int n_frames, int pix, int M, int N, int n_kern,
                           const double* const* kern, const int32_t* kh, const int32_t* kw, const gpet_denoise* dn, int n_img,
                           const int32_t* frame_of, const int32_t* kernel_of, unsigned int flags, float* const* out);
/* ---- a0: non-local means, gpet_utils.denoise(image, 'nl', kwargs) (gpet_utils.py:133-134) -- */
/* scikit-image 0.18.3's denoise_nl_means(image, patch_size, patch_distance, h, fast_mode=False, sigma) on 2-D single-channel
 * frames, bit for bit: the classic algorithm (Gaussian-weighted patch distances, the 5.0 cutoff at patch-row starts, the
 * integer-trick exponential), in float64, in the library's order of operations (csrc/gpet_nlmeans_plan.h states it).  A stage of
 * its own, not a gpet_denoise technique: milliseconds per frame, one kernel launch per staging chunk.  fast_mode=True (the
 * library's default, another algorithm) is gpet_nlmeans_fast_images below.  The frame is widened to float64 as it is -- u8 / u16 frames keep their
 * range, so h and sigma are in the frame's units -- and the result is float64; an f32 frame gives the library's result on the
 * frame widened to f64 (the library would run in f32).  The weight of a candidate whose final patch distance exceeds 708 is
 * +0.0 (there the library's exponential is undefined): parity is claimed where no final distance exceeds 708. */
typedef struct gpet_nlmeans {
  int32_t patch_size;     /* an even size means the next odd one s; 3 <= s <= 15, s / 2 < min(M, N); skimage's default 7 */
  int32_t patch_distance; /* d: candidates up to d pixels away in each direction, 0 <= d <= 31; skimage's default 11 */
  double h;               /* above 0: cut-off distance in grey levels; skimage's default 0.1 */
  double sigma;           /* not negative: noise standard deviation, 2 sigma^2 is taken off every squared difference */
  const double* taps;     /* host, [s * s]: w[a][b] = exp(-(x_a^2 + x_b^2) / (2 A^2)) / (sum h^2), A = (s - 1) / 4 -- an input,
                           * because numpy's exp and the C library's differ in the last place for some arguments */
} gpet_nlmeans;
/* out[] are DEVICE pointers (f64 [M*N] each) on the context's device: with GPET_RAW_ON_DEVICE too, nothing is waited for -- the
 * stage is enqueued on the context's stream and whatever follows on that stream reads its output */
#define GPET_NLM_OUT_ON_DEVICE 8u
/* Non-local means of n_img frames [M*N] of pixel type pix: out[g] f64 [M*N] receives frame g.  Host frames go up in the staging
 * chunks of the raw-frame calls.  flags: GPET_RAW_ON_DEVICE, GPET_NLM_OUT_ON_DEVICE.  GPET_ERR_BAD_ARG, gpet_last_error naming
 * the cause, for a patch below 3 or above 15, d above 31, a patch radius not below min(M, N), h <= 0, sigma < 0, taps that are
 * not finite, a tile neighbourhood (16 + 2 d + 2 (s / 2) pixels each way, f64) beyond 64 KB of LDS, an unknown pix, a null
 * frame or output. */
int gpet_nlmeans_images(gpet_ctx* ctx, const void* const* raw, int n_img, int pix, int M, int N, const gpet_nlmeans* spec,
                        unsigned int flags, void* const* out);
/* ---- a0: fast-mode non-local means, gpet_utils.denoise(image, 'nl', kwargs) with the library's default fast_mode=True -- */
/* scikit-image 0.18.3's denoise_nl_means(image, patch_size, patch_distance, h, fast_mode=True, sigma) on 2-D single-channel
 * frames, bit for bit: per shift an integral image of squared differences whose serial recurrence is followed in its rounding
 * order, uniform patch weights, the 5.0 cutoff, the integer-trick exponential, and every pixel's sums in the order the library's
 * scatter reaches it; in float64 (csrc/gpet_nlfast_plan.h states the arithmetic).  A stage of its own like gpet_nlmeans_images,
 * with the same two deviations: frames are widened to float64 as they are -- u8 / u16 frames keep their range, so h and sigma are
 * in the frame's units --, an f32 frame gives the library's result on the frame widened to f64, and the result is float64.
 * The frame is padded by s / 2 + d + 1 pixels, reflected once.  A frame's workspace holds the padded frame, two accumulators
 * and the integral images of as many whole rows of shifts (d + 1 shifts of one row offset) as fit 256 MiB. */
typedef struct gpet_nlmeans_fast {
  int32_t patch_size;     /* an even size means the next odd one s; 3 <= s <= 15; skimage's default 7 */
  int32_t patch_distance; /* d: shifts up to d pixels in each direction, 0 <= d <= 31; s / 2 + d + 1 <= min(M, N) - 1; default 11 */
  double h;               /* above 0: cut-off distance in grey levels; skimage's default 0.1 */
  double sigma;           /* not negative: noise standard deviation, 2 sigma^2 is taken off every squared difference */
} gpet_nlmeans_fast;
/* Fast-mode non-local means of n_img frames [M*N] of pixel type pix: out[g] f64 [M*N] receives frame g.  Host frames and host
 * outputs go through the staging slot in chunks.  flags: GPET_RAW_ON_DEVICE, GPET_NLM_OUT_ON_DEVICE (with both, nothing is waited
 * for).  GPET_ERR_BAD_ARG, gpet_last_error naming the cause, for a patch_size below 2 or a patch above 15, d below 0 or above 31,
 * h <= 0, sigma < 0 or non-finite values, a padding s / 2 + d + 1 above min(M, N) - 1, an unknown pix, a null frame or output,
 * and a frame so large that the integral images of one row of shifts do not fit the workspace bound (the message gives the bytes). */
int gpet_nlmeans_fast_images(gpet_ctx* ctx, const void* const* raw, int n_img, int pix, int M, int N, const gpet_nlmeans_fast* spec,
                             unsigned int flags, void* const* out);
/* ---- a0: wavelet denoising, gpet_utils.denoise(image, 'wavelet', kwargs) (gpet_utils.py:137-138) -- */
/* scikit-image 0.18.3's denoise_wavelet(image, sigma, wavelet, mode, wavelet_levels, method, rescale_sigma) on PyWavelets 1.1.1 for
 * 2-D single-channel frames and an ORTHOGONAL wavelet given by its decomposition low-pass filter: a separable DWT with symmetric
 * extension, the noise level from the median of the finest diagonal band, BayesShrink or VisuShrink thresholds, soft or hard
 * shrinkage, the inverse transform.  All arithmetic is float64 in the library's order of operations (csrc/gpet_wavelet_plan.h
 * states it); the result is float64.  A stage of its own like non-local means, about 2 levels + 2 kernel launches per staging
 * chunk.  Two deviations: an f32 frame gives the library's result on the frame widened to f64, and the mean of squares under a
 * BayesShrink threshold is summed in the order the plan header defines, not numpy's -- the two means differ by at most
 * 2 (n - 1) 2^-53 relative for a band of n coefficients, and thresholds can be injected.  u8 / u16 frames enter as x / 255,
 * x / 65535 and their result is clipped to [0, 1], as img_as_float and the library do. */
#define GPET_WV_TAPS_MAX 16
#define GPET_WV_SOFT 0
#define GPET_WV_HARD 1
#define GPET_WV_BAYES 0
#define GPET_WV_VISU 1
typedef struct gpet_wavelet {
  int32_t n_taps;           /* F: taps of dec_lo, even, 2 .. 16 */
  int32_t levels;           /* 0: max(max_level - 3, 1); else 1 .. max_level, the largest L with (F - 1) 2^L <= min(M, N) */
  int32_t mode;             /* GPET_WV_SOFT / GPET_WV_HARD */
  int32_t method;           /* GPET_WV_BAYES / GPET_WV_VISU */
  double dec_lo[16];        /* the wavelet's decomposition low-pass filter (PyWavelets' dec_lo); the other three follow from it */
  double sigma;             /* the noise standard deviation, above 0; NaN: estimated per frame */
  int32_t rescale_sigma;    /* not 0: a given sigma of a u8 / u16 frame is scaled as the frame is (skimage's default) */
  int32_t n_thresholds;     /* entries of thresholds: n_img * levels * 3 */
  double ppf;               /* scipy.stats.norm.ppf(0.75) = 0.6744897501960817: the median is divided by it */
  double c;                 /* VisuShrink: sqrt(2 log(M N)), formed by the caller */
  const double* thresholds; /* host or NULL: thresholds to use instead of the derived ones, [frame][level, finest first][ad, da, dd] */
  double* sigma_out;        /* host or NULL, [n_img]: the noise level of every frame */
  double* thresholds_out;   /* host or NULL, [n_img * levels * 3]: the thresholds used */
  double* mean_sq_out;      /* host or NULL, [n_img * levels * 3]: mean(x x) of every detail band (BayesShrink without injection) */
  double* coeffs_out;       /* host or NULL, [n_img * frame_doubles]: every frame's pyramid, level after level (finest first), the
                             * bands aa, ad, da, dd of a level one after the other, each (n + F - 1) / 2 per axis of the level's
                             * input; aa of every level but the coarsest holds the reconstruction that replaced it */
} gpet_wavelet;
/* out[] are DEVICE pointers (f64 [M*N] each) on the context's device */
#define GPET_WV_OUT_ON_DEVICE 8u
/* Wavelet denoising of n_img frames [M*N] of pixel type pix: out[g] f64 [M*N] receives frame g.  Host frames go up in staging
 * chunks; the coefficient pyramids (about 4/3 of a frame in f64 each) live in workspace the context owns, grown on demand and sized
 * per chunk.  flags: GPET_RAW_ON_DEVICE, GPET_WV_OUT_ON_DEVICE.  The call waits for the stream before it returns: it reads every
 * frame's noise level back.  GPET_ERR_BAD_ARG, gpet_last_error naming the cause, for a filter that is not 2 .. 16 taps (even),
 * levels above max_level, a frame whose smaller extent the filter does not fit, an unknown mode, method or pix, sigma <= 0,
 * thresholds of the wrong count, a null frame or output -- and, after the run, for a frame whose noise level is not a number: a
 * finest diagonal band that is all zero (the library returns NaN there) or, with a given sigma under rescale_sigma, a flat integer
 * frame; the message names the first such frame, and the outputs of that call are not to be used. */
int gpet_wavelet_images(gpet_ctx* ctx, const void* const* raw, int n_img, int pix, int M, int N, const gpet_wavelet* spec,
                        unsigned int flags, void* const* out);
/* ---- a0: split-Bregman total-variation denoising, gpet_utils.denoise(image, 'tvb', kwargs) -- */
/* scikit-image 0.18.3's denoise_tv_bregman(image, weight, max_iter, eps, isotropic) on 2-D single-channel frames: Gauss-Seidel
 * sweeps over u with the split variables dx, dy and the Bregman variables bx, by, until the root mean square change of a sweep is
 * at most eps or max_iter sweeps have run.  All arithmetic is float64 in the library's order of operations
 * (csrc/gpet_tvb_plan.h states it); the result is float64 and is not clipped.  The raster order of a sweep is kept: the cells of
 * an anti-diagonal are independent, one workgroup per frame walks the diagonals, and the frames of a call run side by side.  A
 * stage of its own like non-local means and the wavelet stage.  Two deviations: an f32 frame gives the library's result on the
 * frame widened to f64, and the sum of squared changes under the stopping rule is added in the order the plan header defines,
 * not in raster order -- the two sums of n = M N terms differ by at most 2 (n - 1) 2^-53 relative, so the sweep counts can differ
 * only when a sweep's rmse lies that close to eps; where the counts agree the output is the library's bit for bit.  u8 / u16 frames
 * enter as x / 255, x / 65535 (a product with the rounded reciprocal). */
typedef struct gpet_tvb {
  double weight;     /* above 0: the library's required argument (lam = 2 weight) */
  double eps;        /* not negative; the library's default 1e-3 */
  int32_t max_iter;  /* at least 1; the library's default 100 */
  int32_t isotropic; /* not 0: isotropic TV (the library's default), 0: anisotropic */
} gpet_tvb;
/* out[] are DEVICE pointers (f64 [M*N] each) on the context's device */
#define GPET_TVB_OUT_ON_DEVICE 8u
/* Split-Bregman denoising of n_img frames [M*N] of pixel type pix: out[g] f64 [M*N] receives frame g, n_iter_out[g] (host, or NULL)
 * the sweeps frame g ran.  Host frames go up in staging chunks; every frame's six skewed arrays ((M + 2)(N + 2) doubles each) live in
 * workspace the context owns, grown on demand and sized per chunk.  flags: GPET_RAW_ON_DEVICE, GPET_TVB_OUT_ON_DEVICE; with both and
 * n_iter_out NULL nothing is waited for.  GPET_ERR_BAD_ARG, gpet_last_error naming the cause, for weight <= 0, eps < 0,
 * max_iter < 1, M < 2 or N < 2 (the library raises on a 1-pixel axis), min(M, N) above 768 (a diagonal's hand-over must fit 64 KB
 * of LDS), an unknown pix, a null spec, frame or output. */
int gpet_tvb_images(gpet_ctx* ctx, const void* const* raw, int n_img, int pix, int M, int N, const gpet_tvb* spec, unsigned int flags,
                    void* const* out, int32_t* n_iter_out);
/* ---- polar unwrap: closed contours as horizontal edges (no reference function: csrc/gpet_polar_plan.h defines the rule) -- */
/* A frame resampled to (radius x angle) around a centre: a boundary that closes on itself, r(theta), becomes the edge y(x) the
 * tracer follows.  The result of one frame is ONE f64 frame of n_r rows and W = n_theta + 1 + 2 pad columns:
 *   column c     holds angle index a(c) = (c - pad) mod n_theta (non-negative): columns pad and pad + n_theta are the same ray --
 *                the seam --, the pad columns either side repeat the far end, so filters see periodic data there
 *   position     rho = r0 + i dr;  x = cx + rho cos_t[a];  y = cy + rho sin_t[a]  (x the column, y the row; one multiply and one
 *                add each in f64, not contracted; positive angles run clockwise on the screen)
 *   clamp        x into [0, N - 1], y into [0, M - 1]: a ray that leaves the frame repeats the border pixel
 *   taps         x0 = min(floor(x), N - 2), fx = x - x0; y0, fy likewise
 *   value        top = (1 - fx) p[y0, x0] + fx p[y0, x0 + 1]; bot the same on row y0 + 1; out = (1 - fy) top + fy bot, in this order;
 *                u8 / u16 / f32 pixels widened exactly to f64 first (integer frames keep their range)
 * cos_t / sin_t are cos and sin of theta0 + 2 pi j / n_theta, computed by the CALLER and taken as data: the device evaluates no
 * trigonometric function.  (Added without a change of GPET_ABI_VERSION: the surface only grew.) */
typedef struct gpet_polar {
  const double* cx;    /* centres, columns: n_centres values (host) */
  const double* cy;    /* centres, rows */
  int32_t n_centres;   /* 1: one centre for all frames; else n_img, one per frame */
  int32_t n_r;         /* rows of the result, at least 1 */
  int32_t n_theta;     /* distinct angles, at least 4 */
  int32_t pad;         /* periodic columns added on each side, 0 .. n_theta */
  double r0;           /* radius of row 0, finite, at least 0 */
  double dr;           /* radius step per row, finite, above 0 */
  const double* cos_t; /* [n_theta] (host) */
  const double* sin_t; /* [n_theta] (host) */
} gpet_polar;
/* out[] are DEVICE pointers (f64 [n_r * W] each) on the context's device */
#define GPET_POLAR_OUT_ON_DEVICE 8u
/* The polar unwrap of n_img frames [M*N] of pixel type pix: out[g] f64 [n_r * W] receives frame g.  Host frames and host outputs
 * go through the staging slot in chunks, one launch per chunk.  flags: GPET_RAW_ON_DEVICE, GPET_POLAR_OUT_ON_DEVICE (with both,
 * nothing is waited for).  GPET_ERR_BAD_ARG, gpet_last_error carrying polar_check's words, and nothing launched, for an unknown
 * pix, a frame below 2 x 2, n_r < 1, n_theta < 4, pad outside [0, n_theta], r0 < 0, dr <= 0 or non-finite values, n_r * W above
 * 2^28 (a result's bytes stay within 2^31), n_centres neither 1 nor n_img, a non-finite centre, and null centres, tables, frames
 * or outputs. */
int gpet_polar_images(gpet_ctx* ctx, const void* const* raw, int n_img, int pix, int M, int N, const gpet_polar* spec,
                      unsigned int flags, void* const* out);
/* gpet_utils.normalise(img, (0,1)) for an f32 image (gpet.py:97): out f32 [count] (host). */
int gpet_normalise_f32(gpet_ctx* ctx, const float* img, size_t count, float* out);

/* ---- batch of edges (GP_Edge_Tracing.__init__, gpet.py:95-178) ------------------------- */
/* grad: B pointers (host memory) to f32 [M*N] gradient images as the user passes them; the
 * library re-normalises them (gpet.py:97).  If share_image != 0 only grad[0] is used for all
 * edges.  params: B structs.  init_xy: B pointers to i64 [n_init*2], already sorted by x. */
int gpet_batch_create(gpet_ctx* ctx, int B, int M, int N, const float* const* grad, int share_image,
                      const gpet_params* params, const int64_t* const* init_xy, gpet_batch** out);
/* The same with flags.  GPET_GRAD_ON_DEVICE: grad[] are DEVICE pointers on the context's device (e.g. the data_ptr()
 * of the torch tensor an RCCL broadcast over xGMI has just filled): the images are consumed in place, with
 * no copy through host memory.  init_xy and params stay host pointers. */
#define GPET_GRAD_ON_DEVICE 1u
int gpet_batch_create2(gpet_ctx* ctx, int B, int M, int N, const float* const* grad, int share_image,
                       const gpet_params* params, const int64_t* const* init_xy, unsigned int flags, gpet_batch** out);
/* gpet_batch_create2 with the images given as raw frames and the kh x kw kernel (f64, host) of gpet_utils.comp_grad_img:
 * what a caller of the reference writes as GP_Edge_Tracing(init, comp_grad_img(frame, kern), ...) (gpet_utils.py:95-119,
 * then gpet.py:97,127).  raw: B pointers (one if share_image) to frames [M*N] of pixel type pix, host memory or, with
 * GPET_RAW_ON_DEVICE, device memory.  The gradient images are made on the device, all frames in one pass, straight into
 * the batch's buffers; the batch equals, bit for bit, the one gpet_batch_create2 builds from gpet_grad_image's outputs.
 * GPET_ERR_BAD_ARG as for gpet_grad_images. */
int gpet_batch_create_raw(gpet_ctx* ctx, int B, int M, int N, const void* const* raw, int pix, const double* kern, int kh,
                          int kw, int share_image, const gpet_params* params, const int64_t* const* init_xy,
                          unsigned int flags, gpet_batch** out);
/* gpet_batch_create_raw with the frames denoised first (gpet_denoise): the batch equals, bit for bit, the one
 * gpet_batch_create_raw builds from gpet_denoise_images' outputs.  dn NULL or technique NONE: gpet_batch_create_raw itself. */
int gpet_batch_create_raw_dn(gpet_ctx* ctx, int B, int M, int N, const void* const* raw, int pix, const double* kern, int kh,
                             int kw, const gpet_denoise* dn, int share_image, const gpet_params* params,
                             const int64_t* const* init_xy, unsigned int flags, gpet_batch** out);
/* Batches with an image map: n_img images for B edges, edge e reads image image_of[e] -- a video frame or an OCT slice with
 * several edges on it (the layers of a retina, the two walls of a vessel) is uploaded, turned into a gradient image, denoised
 * and run through the gradient KDE (gpet.py:127) once, not once per edge.  1 <= n_img <= B, 0 <= image_of[e] < n_img, every
 * image read by at least one edge; the edges of an image need not be adjacent ([0,1,2,0,1,2] is valid).  grad: n_img pointers
 * as in gpet_batch_create2 (flags: GPET_GRAD_ON_DEVICE).  The batch equals, bit for bit, the one gpet_batch_create2 builds from
 * the B images grad[image_of[e]]; n_img = 1 is the shared-image batch.  GPET_ERR_BAD_ARG (gpet_last_error names the cause) for
 * a map that breaks one of the rules or a null image. */
int gpet_batch_create_mapped(gpet_ctx* ctx, int B, int M, int N, int n_img, const int32_t* image_of, const float* const* grad,
                             const gpet_params* params, const int64_t* const* init_xy, unsigned int flags, gpet_batch** out);
/* The same with the images given as n_img raw frames (raw, pix, kern as in gpet_batch_create_raw; flags: GPET_RAW_ON_DEVICE),
 * denoised first if dn is not NULL (gpet_batch_create_raw_dn). */
int gpet_batch_create_raw_mapped(gpet_ctx* ctx, int B, int M, int N, int n_img, const int32_t* image_of, const void* const* raw,
                                 int pix, const double* kern, int kh, int kw, const gpet_denoise* dn, const gpet_params* params,
                                 const int64_t* const* init_xy, unsigned int flags, gpet_batch** out);
/* The same with a slot table (gpet_grad_images_multi): the n_img image slots of the map are made of n_frames raw frames and
 * n_kern kernels, slot g of frame frame_of[g] with kernel kernel_of[g]; image_of maps the B edges to slots as ever.  The batch
 * equals, bit for bit, the one gpet_batch_create_mapped builds from gpet_grad_images_multi's outputs; one kernel with one slot per
 * frame in frame order is gpet_batch_create_raw_mapped itself.  GPET_ERR_BAD_ARG as for gpet_grad_images_multi and the map. */
int gpet_batch_create_raw_multi(gpet_ctx* ctx, int B, int M, int N, int n_img, const int32_t* image_of, int n_frames,
                                const void* const* raw, int pix, int n_kern, const double* const* kern, const int32_t* kh,
                                const int32_t* kw, const int32_t* frame_of, const int32_t* kernel_of, const gpet_denoise* dn,
                                const gpet_params* params, const int64_t* const* init_xy, unsigned int flags, gpet_batch** out);
void gpet_batch_destroy(gpet_batch* b);
int gpet_batch_size(const gpet_batch* b);
/* Images the batch holds: 1 if it shares one image, B with one image per edge, n_img with an image map.  That many pointers
 * gpet_batch_set_images, gpet_batch_set_raw_images and gpet_batch_set_raw_images_dn take. */
int gpet_batch_image_count(const gpet_batch* b);
/* out[0..count): Lg, S, n_keep, n_cap, factor_cap, z_cols, factor_rows_cap, n_bins, obs_cap, algo_thresh,
 * structured (1: the loop uses the prior-eigenbasis path), r0 (rank of the grid's correlation matrix), z_ring (slots
 * of pre-generated normals per edge), arena size of the batch in MiB, then the batch's normals store (options normals_store,
 * normals_store_iters; decided by the first gpet_trace_iterate): zstore_iters (iterations held per edge; 0: no store),
 * its size in MiB, normals_generated (the (edge, iteration) streams the loop has generated so far for iterations the edge
 * went on to run; a trace repeated with the same seeds does not move it for the iterations the store holds, nor -- where the
 * generator runs on the loop's own stream, option normals_ring_keep -- for ring iterations whose slots nothing has overwritten
 * since), normals_drawn (the streams the loop's launches into the store generated, exactly: they generate whatever
 * the edge's `done` flag says, look-ahead included); both saturating */
int gpet_batch_info(const gpet_batch* b, int e, int32_t* out, int count);

/* Back to the state right after gpet_batch_create: no observations, initial score threshold,
 * iteration counter 0 (a GP_Edge_Tracing instance is single-use in the reference; benches re-run). */
int gpet_batch_reset(gpet_batch* b);

/* New gradient image(s) for an existing batch of the same geometry and parameters -- the next frame of an image
 * sequence (gpet.py:57-61: a trace warm-starts the next one through `obs`): grad as in gpet_batch_create2
 * (gpet_batch_image_count(b) pointers: one if the batch shares its image, n_img with an image map, else B), re-normalised, gradient KDE recomputed (gpet.py:97,127), then
 * gpet_batch_reset.  The per-edge work that depends only on the geometry and the kernel (the prior eigenbasis of the
 * structured loop path) is kept. */
int gpet_batch_set_images(gpet_batch* b, const float* const* grad, unsigned int flags);
/* flags: GPET_GRAD_ON_DEVICE as above, and GPET_IMAGES_NEXT_FRAME: the new images are the NEXT FRAMES of the sequences
 * the edges have just been traced through (gpet.py:57-61), so the any-rank factor of the new trace's first iteration may
 * start from the last trace's factor rows (an iterative solve: the same rows to its tolerance, 4e-9 relative).  Without the
 * flag -- and after gpet_batch_reset / gpet_batch_set_obs always -- nothing of an earlier trace is used: a trace depends
 * on (image, seed, observations) only, like the reference's single-use object. */
#define GPET_IMAGES_NEXT_FRAME 2u
/* gpet_batch_set_images with raw frames (gpet_utils.py:95-119 for every frame, then gpet.py:97,127; the next frame of a
 * sequence, gpet.py:57-61): raw, pix, kern as in gpet_batch_create_raw; flags: GPET_RAW_ON_DEVICE, GPET_IMAGES_NEXT_FRAME.
 * A call refused with GPET_ERR_BAD_ARG (unknown pix, null frame, oversized kernel) leaves the batch as it was. */
int gpet_batch_set_raw_images(gpet_batch* b, const void* const* raw, int pix, const double* kern, int kh, int kw,
                              unsigned int flags);

/* gpet_batch_set_raw_images with the frames denoised first; dn NULL or technique NONE: gpet_batch_set_raw_images itself.  A
 * call refused with GPET_ERR_BAD_ARG (as gpet_batch_set_raw_images, or a spec gpet_denoise_images refuses) leaves the batch as
 * it was. */
int gpet_batch_set_raw_images_dn(gpet_batch* b, const void* const* raw, int pix, const double* kern, int kh, int kw,
                                 const gpet_denoise* dn, unsigned int flags);

/* gpet_batch_set_raw_images_dn with a slot table (gpet_batch_create_raw_multi): n_frames frames, and a table of
 * gpet_batch_image_count(b) slots.  A call refused with GPET_ERR_BAD_ARG (a bad table, the LDS bound, a null frame, a bad
 * denoising spec) leaves the batch as it was. */
int gpet_batch_set_raw_images_multi(gpet_batch* b, int n_frames, const void* const* raw, int pix, int n_kern,
                                    const double* const* kern, const int32_t* kh, const int32_t* kw, const int32_t* frame_of,
                                    const int32_t* kernel_of, const gpet_denoise* dn, unsigned int flags);

/* set / get the observation set (xy int64) of edge e (gpet.py:100,820,857). */
int gpet_batch_set_obs(gpet_batch* b, int e, const int64_t* obs_xy, int n_obs);
/* The warm start of the next frame of a sequence (gpet.py:57-61) for every edge at once, on the device: edge e's new observation
 * set is derived from its own last converged fit, which gpet_final_fit_all left in device memory -- call it after the images were
 * swapped (gpet_batch_set_images with GPET_IMAGES_NEXT_FRAME), where gpet_batch_set_obs would be called.  The trace is
 * rint(mean) on the edge's x-grid (the rounding of gpet_batch_results); candidates are the grid indices step, 2 step, ...
 * < Lg - 1 with step = max(1, warm_every); a candidate with x_st < x < x_en and 0 <= y <= M - 1 is kept; while algo_thresh or
 * more (and not zero) are kept -- the next trace's loop would not run, gpet.py:829 -- step is doubled.  The kept pixels are the
 * observation set, (x, y) in ascending x.  The batch is then in the state B calls of gpet_batch_set_obs with those sets leave,
 * after ONE wait instead of B.  n_obs_out (host, [B], may be NULL): the sizes of the sets.  GPET_ERR_BAD_ARG (with a message)
 * when the last trace's converged fits are not there: on a fresh batch, and after gpet_batch_set_obs or a warm start without a
 * trace in between. */
int gpet_batch_warm_start(gpet_batch* b, int warm_every, int32_t* n_obs_out);
/* GPET_OK when gpet_batch_warm_start would run now, else its GPET_ERR_BAD_ARG and message, with nothing touched: ask before
 * gpet_batch_set_images, which cannot be undone once the warm start is refused. */
int gpet_batch_warm_start_ready(gpet_batch* b);
int gpet_batch_read(gpet_batch* b, int e, int which, void* dst, size_t bytes);
/* Writable: FACTOR (rows = factor rows; marks the factor as injected so gpet_gp_factor leaves
 * it alone), NORMALS, SAMPLES, COSTS, BEST_IDX, BEST_COSTS (a caller's own choice of best curves for
 * gpet_curve_kde / gpet_select_pixels, gpet.py:622-648), MEAN, COV, KDE, GRAD_KDE, SCALARS. */
int gpet_batch_write(gpet_batch* b, int e, int which, const void* src, size_t bytes, int rows);
int gpet_batch_clear_injected_factor(gpet_batch* b, int e);

/* ---- a2-a5: fit_predict_GP not-converged, deterministic part -------------------------- */
/* gpet.py:209-231 + sklearn_gpr.py:221-227,304-320 (fit) + :381-436 (predict mean/std/cov).
 * want_cov: also materialise the Lg x Lg covariance. */
int gpet_gp_fit_predict(gpet_batch* b, int want_cov);

/* ---- a6: sample_y (sklearn_gpr.py:440-473) --------------------------------------------- */
/* Factor the posterior covariance into rows sqrt(s_k) v_k (k by descending s_k), the object
 * numpy's legacy multivariate_normal builds from LAPACK SVD.  Eigenvector signs follow the
 * library convention: sum_j row[j] / (j + 1) >= 0 (LAPACK's are implementation-defined). */
int gpet_gp_factor(gpet_batch* b);
/* Fill the normals with RandomState(seed[e]).standard_normal((S, Lg)) (first z_cols columns
 * of every row are stored).  seeds: B values. */
int gpet_gp_normals(gpet_batch* b, const uint32_t* seeds);
/* samples[s, :] = y_s * (Z[s, :rows] @ factor + mean)            (gpet.py:260-261) */
int gpet_gp_sample(gpet_batch* b);

/* ---- a7: get_best_curves / cost_funct (gpet.py:371-451) -------------------------------- */
int gpet_score_curves(gpet_batch* b);

/* ---- f1: get_best_pixels (gpet.py:455-662) --------------------------------------------- */
/* kernel_density_estimate(best_curves, costs) alone (gpet.py:455-529): the normalised KDE of the curves
 * GPET_BUF_BEST_IDX / _BEST_COSTS select among GPET_BUF_SAMPLES goes to GPET_BUF_KDE. */
int gpet_curve_kde(gpet_batch* b);
int gpet_select_pixels(gpet_batch* b);
/* gpet_select_pixels by the kernels and in the form gpet_trace_iterate runs after its scorer: same observation set, score
 * threshold and counters, but GPET_BUF_KDE keeps the RAW density, and only inside every 16-column tile's band of rows (the
 * rows of the tile's surviving curve points, +-4); rows outside a band keep what they held.  There so that tests reach the
 * loop's form of the stage on injected inputs. */
int gpet_select_pixels_loop(gpet_batch* b);
/* Pixel scoring / threshold decay / per-bin argmax only (gpet.py:532-618), on whatever curve KDE
 * is currently in GPET_BUF_KDE (tests inject the reference's). */
int gpet_select_pixels_only(gpet_batch* b);

/* ---- a8: the outer loop (gpet.py:829-870) ---------------------------------------------- */
/* Runs up to max_iters iterations of fit->factor->normals->sample->score->pixels for every
 * edge that is not done; seed of iteration k (0-based) of edge e is base_seed[e] + k + 1
 * (gpet.py:839).  The iterations are enqueued in groups (8, 4, then 2 once edges start to finish); after
 * each group the `done` flags are read, the call returns early when no edge is left, and the next group is
 * launched over the edges still running only.  Returns the number of edges still not done in *n_active. */
int gpet_trace_iterate(gpet_batch* b, const uint32_t* base_seeds, int max_iters, int* n_active);

/* ---- iteration history: what __call__(return_lines=True) returns per iteration (gpet.py:840-866), kept on the device --------
 * Opt-in.  With a history enabled, gpet_trace_iterate runs one more kernel per iteration (k_history, after the pixel selection,
 * on the context's stream) that appends ONE record for every edge that completed that iteration, at slot iter - 1 of the edge's
 * region; nothing waits on the host and no sample matrix travels.  With it off (the default) the loop enqueues exactly what it
 * enqueued before, and no result depends on the level either way.
 * Storage: one device allocation of its own, B regions of edge_bytes, in one fixed layout that a host in any language decodes
 * with the numbers of gpet_history_plan:
 *   region = gpet_history_edge_head | record[iter_cap]                              (records at off_records + k * record_bytes)
 *   record = gpet_history_head                                                       the scalars after the iteration
 *          | int32 obs[obs_cap][2]        at off_obs    the new observation set, xy, as the pixel selection left it (gpet.py:857)
 *          | f64 curve[len_cap]           at off_curve  level >= 2: the optimal curve = sample row best_idx (gpet.py:443-449),
 *                                                       widened exactly from f32 under gpet_batch_set_sample_dtype
 *          | f64 mean[len_cap]            at off_mean   level 3: per-column mean of all S samples          (gpet.py:687)
 *          | f64 std[len_cap]             at off_std    level 3: per-column population std (np.std)       (gpet.py:688)
 *   obs_cap / len_cap are the batch's largest observation capacity / widest edge; entries past an edge's own n_obs / edge
 *   length are zero, and so are records past n_rec.  The statistics are two passes in f64 without contraction, rows summed in
 *   a fixed partition and order: edge e's values do not depend on the batch around it.
 * iter_cap: an edge that runs past iter_cap iterations traces on unchanged; its later records are dropped and counted in
 *   `dropped` (nothing is overwritten, no error).
 * Lifetime: the history is the current trace's.  gpet_batch_reset, gpet_batch_set_images (and the raw forms) and
 *   gpet_batch_warm_start empty every edge's region, gpet_batch_set_obs empties edge e's. */
/* (named _plan, not _layout: C keeps typedef names and functions in one name space, and the call below is gpet_history_layout) */
typedef struct gpet_history_plan {
  int32_t level;        /* 1 'obs', 2 'curves', 3 'full' */
  int32_t iter_cap;     /* records per edge */
  int32_t obs_cap;      /* observation pairs per record */
  int32_t len_cap;      /* points per curve / mean / std section */
  int64_t edge_bytes;   /* one edge's region: off_records + iter_cap * record_bytes */
  int64_t record_bytes;
  int64_t off_records;  /* in the region: the first record (= sizeof(gpet_history_edge_head)) */
  int64_t off_obs;      /* in a record: the observation pairs (= sizeof(gpet_history_head)) */
  int64_t off_curve;    /* in a record; 0 below level 2 */
  int64_t off_mean;     /* in a record; 0 below level 3 */
  int64_t off_std;      /* in a record; 0 below level 3 */
} gpet_history_plan;
typedef struct gpet_history_edge_head {  /* one per edge, followed by its records */
  int32_t n_rec;     /* records kept: min(iterations recorded, iter_cap) */
  int32_t dropped;   /* iterations that found no slot left */
  int32_t n_iter;    /* iteration count of the edge at its last record (= n_rec + dropped after a loop) */
  int32_t edge_len;  /* points of this edge's x-grid (0 until the first record) */
} gpet_history_edge_head;
typedef struct gpet_history_head {  /* one per record, followed by its sections */
  int32_t iter;         /* the iteration, 1-based                                     gpet.py:865 */
  int32_t n_obs;        /* observations after it                                      gpet.py:861 */
  int32_t best_idx;     /* index of the optimal curve among the samples (best_idx[0]) gpet.py:443 */
  int32_t rank;         /* rows of the factor the samples were drawn from */
  int32_t n_removed;    /* curve points outside the image                             gpet.py:498-500 */
  int32_t reserved;
  double score_thresh;  /* after the iteration                                        gpet.py:595 */
  double optimal_cost;  /* best_costs[0]                                              gpet.py:449 */
  double y_s;           /* std(y) + 1 of the iteration's fit                          gpet.py:228 */
} gpet_history_head;
/* level 0: off, the storage is freed; 1..3: (re)allocate for iter_cap records per edge, zeroed, and point the edges at it.
 * GPET_ERR_BAD_ARG for another level or iter_cap < 1.  Call between traces, not while a loop is enqueued. */
int gpet_batch_set_history(gpet_batch* b, int level, int iter_cap);
/* the numbers above for this batch; GPET_ERR_STATE when the history is off */
int gpet_history_layout(gpet_batch* b, gpet_history_plan* out);
/* Edge e's region (edge_bytes), or with e = -1 all B regions (B * edge_bytes), into host memory (dst_on_device = 0: complete on
 * return) or device memory (1: enqueued on the context's stream): one copy, one wait.  `bytes` is the room at dst.
 * GPET_ERR_STATE when the history is off, GPET_ERR_BAD_ARG when dst is too small. */
int gpet_batch_history(gpet_batch* b, int e, void* dst, size_t bytes, int dst_on_device);
/* The history kernel once, alone, on whatever the buffers hold now (GPET_BUF_SAMPLES, _BEST_IDX, _BEST_COSTS, _OBS, _SCALARS):
 * every edge whose iteration count is at least 1 gets the record of slot iter - 1 (re)written -- a per-stage entry point like
 * gpet_select_pixels_only, there so that tests can inject inputs no scene produces.  GPET_ERR_STATE when the history is off. */
int gpet_history_record(gpet_batch* b);

/* ---- f2: converged fit (gpet.py:232-248; sklearn_gpr.py:254-295, 475-585) ----------------- */
/* Upload edge e's standardised training set (x, y standardised as gpet.py:235-238 and
 * sklearn_gpr.py:229-234 do; w = per-point noise weights), n <= the batch's training-set capacity (register-tile objective
 * kernels up to 250 points; above, the blocked HBM path: Cholesky, L^-1 and K^-1 tiles on the matrix cores). */
int gpet_final_set_training(gpet_batch* b, int e, const double* xs, const double* ys, const double* w, int n);
/* The same for every edge of the batch in one call: xs/ys/w are [B*stride], n [B]. */
int gpet_final_set_training_all(gpet_batch* b, const double* xs, const double* ys, const double* w, const int32_t* n,
                                int stride);
/* Scalar state of every edge in one copy: dst [B]. */
int gpet_batch_read_scalars_all(gpet_batch* b, gpet_scalars* dst);
/* Observation sets of every edge in one call: dst i64 [B*stride_obs*2] xy, counts [B]. */
int gpet_batch_read_obs_all(gpet_batch* b, int64_t* dst, int32_t* counts, int stride_obs);
/* Posterior of the converged fit at the optimum (gpet.py:262-266) for every edge: par [B*12] =
 * constant, length_scale, noise_level (values, not logs), X_m, X_s, y_m, y_s, m2, s2, 0, 0, 0;
 * mean_out (pixels) and std_out (standardised units, as the reference returns it) are [B*stride]. */
int gpet_final_predict_all(gpet_batch* b, const double* par, double* mean_out, double* std_out, int stride);
/* GaussianProcessRegressor.predict(return_cov=True) (sklearn_gpr.py:398-403) for the fit gpet_final_predict_all has
 * just evaluated: the Lg x Lg posterior covariance on the standardised grid goes to GPET_BUF_COV of every edge. */
int gpet_final_cov(gpet_batch* b);
/* Objective of the reference's L-BFGS-B runs for P problems at once: problem i evaluates
 * -log_marginal_likelihood and its gradient wrt theta_i = log(constant, length_scale, noise_level)
 * on edge edge_of[i]'s training set.  theta [P*3], f_out [P], g_out [P*3] (host).  A non-PD
 * kernel matrix gives f = +inf, g = 0 (sklearn_gpr.py:521-522). */
int gpet_lml_batch(gpet_batch* b, int P, const int32_t* edge_of, const double* theta, double* f_out, double* g_out);

/* The whole converged fit of every edge of the batch on the device (gpet.py:874-876 -> :232-248, 262-266;
 * sklearn_gpr.py:254-295): training sets from the current observation sets, standardised as the reference does;
 * theta0 + 12 restarts from RandomState(seeds[e]).uniform (the caller passes seed + N_iter, gpet.py:874); L-BFGS-B
 * (scipy.optimize.minimize's algorithm and defaults) for all 13 B problems in lock step, one batched objective launch
 * per round; best restart; posterior at the optimum.  mean_out (pixels) and std_out (standardised units, as the
 * reference returns it) are [B*stride]; theta_out (optional) [B*4] = log(constant, length_scale, noise_level) and the
 * minimum of -log marginal likelihood; rounds_out (optional) = objective rounds.  Any number of training points the
 * batch was created for (more than 250: the blocked objective, ~100 launches per round -- a rare, slower path). */
int gpet_final_fit_all(gpet_batch* b, const uint32_t* seeds, double* mean_out, double* std_out, double* theta_out,
                       int stride, int32_t* rounds_out);

/* Random numbers of this batch: 0 = MT19937 + polar method, the stream of numpy's RandomState(seed).standard_normal that
 * sklearn_gpr.py:460-464 draws from (default; every parity statement is made on it); 1 = Philox4x32-10 + Box-Muller, a
 * counter-based generator (normal (s, j) of an iteration is a pure function of seed, s, j): NOT the reference's numbers, an
 * opt-in mode with its own oracle (oracle.philox_standard_normal); the per-iteration seed rule (gpet.py:839) is the same. */
int gpet_batch_set_rng(gpet_batch* b, int mode);

/* Storage type of the posterior samples of this batch: 0 = f64 (default: the reference's sample_y, sklearn_gpr.py:440-473,
 * every parity statement is made on it), 1 = f32 -- BASELINE config 2's "fp32 posterior samples": the sample GEMM rounds
 * each sample to f32 when it stores it, scorer / KDE / pixel kernels widen it again, all arithmetic stays f64; GPET_BUF_SAMPLES
 * is f64 on the interface either way.  Results equal the reference with `y_samples.astype(float32)` inserted after
 * sample_y (oracle mode sample_dtype="f32").  Call between traces, not while a loop is enqueued. */
int gpet_batch_set_sample_dtype(gpet_batch* b, int f32);

/* Arithmetic of the sample GEMM of this batch: GPET_SAMPLE_ARITH_F64 (default: products and sums on the f64 matrix cores, whatever
 * the storage type) or GPET_SAMPLE_ARITH_F32 -- BASELINE config 2's "fp32 posterior samples" as arithmetic, on the f32 matrix
 * cores.  For an edge with factor rows A[k][j], normals Z[s][k], posterior mean mean[j], scale y_s and rank r the result is
 * DEFINED as
 *     z = (float)Z[s][k],  a = (float)A[k][j]             round to nearest even, once each
 *     acc_0 = +0.0f
 *     acc_{k+1} = fmaf(z_k, a_k, acc_k)                   k = 0, 1, ..., r-1 ascending, one accumulator per (s, j)
 *     Y[s][j] = (float)(((double)acc_r + mean[j]) * y_s)  the add and the multiply in f64, each rounded, not contracted
 * bit for bit (f32 subnormals kept; normals and factor rows beyond the rank are not read as values).  F32 also switches the
 * storage to f32, since the two go together; gpet_batch_set_sample_dtype keeps its meaning and in addition sets the arithmetic
 * back to F64, so no batch holds f64 storage with f32 arithmetic.  Any other value: GPET_ERR_BAD_ARG, the batch as it was.  NOT
 * the reference's numbers (there is no oracle mode; tests/f32_chain.py evaluates the definition).  Call between traces, not while
 * a loop is enqueued.  (Added without a change of GPET_ABI_VERSION: the surface only grew.) */
#define GPET_SAMPLE_ARITH_F64 0
#define GPET_SAMPLE_ARITH_F32 1
int gpet_batch_set_sample_arith(gpet_batch* b, int arith);

/* The optimiser alone, for a caller's own training sets (GaussianProcessRegressor.fit with optimizer="fmin_l_bfgs_b",
 * sklearn_gpr.py:254-295, 587-607): L-BFGS-B from n_starts start points per edge (starts [B][n_starts][3], theta = log
 * (constant, length_scale, noise_level)) inside bounds [3][2] = (lo, hi) per component, on the training sets of
 * gpet_final_set_training(_all); theta_out [B*4] = the best start's optimum (first minimum, np.argmin) and its objective
 * value (-log marginal likelihood); it is also left in GPET_BUF_FIN_PAR[0..2] as exp(theta). */
int gpet_final_optimize(gpet_batch* b, int n_starts, const double* starts, const double* bounds, double* theta_out,
                        int32_t* rounds_out);

/* What became of every problem of the last gpet_final_fit_all / gpet_final_optimize of this batch: *n_out = the number of
 * (edge, start) problems P (edge-major, as the starts were given), and, if cap >= P, out[P][10] = the final point x[3], its
 * objective value f, the gradient g[3], the number of iterations, the number of objective evaluations, and the reason for
 * stopping (1: projected gradient <= pgtol at the start point, 2: the same after an iteration, 3: relative reduction of f <=
 * factr * eps, 4: no descent direction, 5: line search failed).  cap = 0 only asks for the count; 0 < cap < P is
 * GPET_ERR_BAD_ARG.  (Added without a change of GPET_ABI_VERSION: the surface only grew.) */
int gpet_final_problems(gpet_batch* b, double* out, int cap, int32_t* n_out);

/* Device time of the LML kernel launches of this batch since the last reset (hipEvents around each launch), the
 * number of objective evaluations and of launches; any of the outputs may be NULL.  (bench.py's roofline leg.) */
int gpet_lml_stats(gpet_batch* b, int reset, double* kernel_ms, int64_t* evaluations, int32_t* launches);

/* ---- collectives: one process per GPU ---------------------------------------------------------------
 * The reference has no multi-GPU path; independent edges (and whole chains of an image sequence) shard over ranks with no
 * collective on a trace's data path: ONE broadcast of the shared gradient image(s) and ONE gather of the finished traces.
 * These are the RCCL call sites for a host that is not Python (the Python package does the same through torch.distributed,
 * sharding.py).  RCCL is bound at run time (dlopen); a world of 1 needs none.
 *   rank 0: gpet_comm_unique_id(id)  -> ship the GPET_COMM_ID_BYTES bytes to every rank by any means (file, socket, MPI)
 *   all:    gpet_comm_create(ctx, id, world, rank, &comm)        (ncclCommInitRank on the context's device)
 *           gpet_comm_block(comm, n_edges, &lo, &hi)             this rank's contiguous block of edges [lo, hi)
 *           gpet_bcast_grad(comm, d_grad, count, root)           in place on DEVICE memory, on the context's stream; hand
 *                                                                d_grad to gpet_batch_create2(..., GPET_GRAD_ON_DEVICE)
 *           gpet_gather_traces(comm, local, n_edges, len, all)   host int64 [n_local][len][2] -> [n_edges][len][2] on every
 *                                                                rank, in global edge order (blocks as gpet_comm_block)
 *           gpet_allgather_i64(comm, local, counts, all)         the same for blocks of counts[r] int64 per rank (sequences)
 *           gpet_gather_results(comm, batch, n_edges, cap, all)  the finished result RECORD of every edge (below) -> host
 *                                                                [n_edges] records on every rank, in global edge order
 * Result records: what GP_Edge_Tracing(..., return_std=True) returns for an edge (gpet.py:874-886, 902-903) plus the trace's
 * statistics, in one fixed layout that a host in any language reads without the library:
 *   record = gpet_result_head | int64 trace[len_cap][2] (yx: rint(mean), x_st + k; gpet.py:885-886)
 *                             | f64 lower[len_cap] | f64 upper[len_cap]  (mean -/+ 1.96 std, gpet.py:876)
 *   entries past the edge's own edge_len are zero; gpet_result_bytes gives the size of one record (48 + 32 len_cap bytes).
 *   gpet_batch_results(batch, len_cap, dst, on_device)   the B records of a batch, contiguous, computed on the device from the
 *       converged fit (k_finish_results, bit for bit what the host computes from gpet_final_fit_all's mean / std): valid only
 *       after gpet_final_fit_all has run on the batch's current trace (GPET_ERR_BAD_ARG before it and after gpet_batch_reset,
 *       gpet_batch_set_images, gpet_batch_set_obs or more loop iterations); len_cap >= the batch's widest edge.  dst is host
 *       memory (on_device = 0: complete on return) or device memory (1: enqueued on the context's stream).
 *   gpet_gather_results: each rank packs its block straight into the communicator's device buffer and ONE all-gather of the
 *       padded blocks runs; batch is NULL on a rank that owns no edges, else its B equals the rank's block and its context is
 *       the communicator's.  A world of one without a communicator is a copy. */
typedef struct gpet_result_head {  /* one per edge, followed by its arrays */
  int32_t edge_len;  /* points of this edge's x-grid                                gpet.py:112 */
  int32_t n_iter;    /* loop iterations                                             gpet.py:865 */
  int32_t n_obs;     /* final observation count                                     gpet.py:861 */
  int32_t status;    /* gpet_status raised on the device for this edge */
  double theta[3];   /* log(constant, length_scale, noise_level) at the optimum     gpet.py:241-248 */
  double nlml;       /* -log marginal likelihood at the optimum */
} gpet_result_head;
typedef struct gpet_comm gpet_comm;
#define GPET_COMM_ID_BYTES 128
int gpet_comm_unique_id(void* id128);
int gpet_comm_create(gpet_ctx* ctx, const void* id128, int world, int rank, gpet_comm** out);
void gpet_comm_destroy(gpet_comm* comm);
int gpet_comm_rank(const gpet_comm* comm);
int gpet_comm_world(const gpet_comm* comm);
int gpet_comm_block(const gpet_comm* comm, int64_t n_units, int64_t* lo, int64_t* hi);
int gpet_bcast_grad(gpet_comm* comm, float* d_grad, size_t count, int root);
/* device memory on the context's device for the broadcast buffer (hosts that do not call the HIP runtime themselves);
 * gpet_dev_copy: host -> device (to_host = 0) or device -> host (1), on the context's stream, complete on return */
int gpet_dev_alloc(gpet_ctx* ctx, size_t bytes, void** out);
int gpet_dev_free(gpet_ctx* ctx, void* ptr);
int gpet_dev_copy(gpet_ctx* ctx, void* dst, const void* src, size_t bytes, int to_host);
int gpet_allgather_i64(gpet_comm* comm, const int64_t* h_local, const int64_t* counts, int64_t* h_all);
int gpet_gather_traces(gpet_comm* comm, const int64_t* h_local, int64_t n_edges, int64_t edge_len, int64_t* h_all);
int gpet_result_bytes(int64_t len_cap, size_t* bytes);
int gpet_batch_results(gpet_batch* b, int64_t len_cap, void* dst, int dst_on_device);
int gpet_gather_results(gpet_comm* comm, gpet_batch* local, int64_t n_edges, int64_t len_cap, void* h_all);

/* ---- seed ensembles: final costs and a per-column consensus over the traces of one edge -------------------------------------
 * The tracer is stochastic; a batch that traces one edge with many seeds holds many converged fits of it.  Two reductions are
 * made where those fits lie (fin_out), both valid exactly when gpet_batch_results is (after gpet_final_fit_all on the current
 * trace; GPET_ERR_BAD_ARG otherwise) and both leaving the loop's state -- samples, costs, best curves, scalars, history --
 * untouched (their scratch is an allocation of its own, made on first use):
 *   gpet_batch_final_costs(batch, dst, on_device)   cost[e], f64 [B]: the scorer's cost of edge e's converged mean curve on its
 *       own gradient image -- cost_funct(optim_mean_curve), gpet.py:888-890 -- bit for bit what gpet_score_curves writes to
 *       costs[s] when that curve stands in row s of edge e's sample matrix in this batch (the same kernels, launched on a
 *       one-row view of the means; with f32 samples the mean is rounded to f32 as a write of the samples rounds it).  An edge
 *       whose gpet_scalars.status is not GPET_OK gets +inf.
 *   gpet_batch_ensemble(batch, G, group_of, tol, len_cap, dst, on_device)   group_of[B]: the group of every edge in [0, G), or -1
 *       for "in no group"; every index in [0, G) occurs; all edges assigned to a group share x_st and x_en; tol >= 0 in pixels;
 *       len_cap >= the batch's widest edge.  The MEMBERS of group g are its edges in ascending order minus those whose status
 *       is not GPET_OK, at most GPET_ENSEMBLE_MAX.  With n members, v_m[k] the converged mean (pixels) of member m at grid index
 *       k, and s[0..n-1] the v_m[k] in ascending order (equal values in member order):
 *         min = s[0], max = s[n-1], q_lo = s[(n-1)/4], q_hi = s[n-1-(n-1)/4], median = (s[(n-1)/2] + s[n/2]) * 0.5
 *         (integer divisions; selections and one exact add and halving: np.sort / np.median along the member axis, bit for bit)
 *         c[k] = (int64) rint(median[k]), round half to even; the consensus trace is (c[k], x_st + k), yx like a result record's
 *         agree[k] = number of members with |rint(v_m[k]) - c[k]| <= tol
 *         off[e]   = number of columns with |rint(v_e[k]) - c[k]| > tol for a member e; -1 for every other edge
 *         medoid   = the member with the smallest off, ties to the smaller final cost, then to the smaller edge index
 *         best_cost = the member with the smallest final cost, ties to the smaller edge index
 *       (both are edge indices; the final costs are those of gpet_batch_final_costs, computed inside the call).  A group without
 *       members has n_members = 0, medoid = best_cost = -1 and zero arrays.  NaN means are not ordered.
 *   dst = G records | f64 cost[B] | int32 off[B] (padded to 8 bytes), gpet_ensemble_bytes(G, B, len_cap) in all;
 *   record = gpet_ensemble_head | int64 trace[len_cap][2] | f64 median | q_lo | q_hi | min | max [len_cap] each
 *                               | int32 agree[len_cap] (padded to 8 bytes); entries past the group's edge_len are zero.
 *   dst is host memory (on_device = 0: complete on return) or device memory (1: enqueued on the context's stream). */
#define GPET_ENSEMBLE_MAX 1024
typedef struct gpet_ensemble_head {  /* one per group, followed by its arrays */
  int32_t n_members; /* members of the group (assigned edges with status GPET_OK) */
  int32_t edge_len;  /* points of the group's x-grid */
  int32_t x_st;      /* its first column */
  int32_t medoid;    /* edge index, -1 without members */
  int32_t best_cost; /* edge index, -1 without members */
  int32_t reserved;
  double tol;        /* the tolerance the counts were made with */
} gpet_ensemble_head;
int gpet_batch_final_costs(gpet_batch* b, double* dst, int dst_on_device);
int gpet_ensemble_bytes(int n_groups, int n_edges, int64_t len_cap, size_t* bytes);
int gpet_batch_ensemble(gpet_batch* b, int n_groups, const int32_t* group_of, double tol, int64_t len_cap, void* dst,
                        int dst_on_device);

/* ---- seed ensembles in sequences: the next frame's warm start from the group's medoid, best member or consensus ---------------
 * In a sequence every frame is traced with K seeds per edge (one group per edge of the frame), and ALL K members of the next frame
 * start from one source of their group -- so a seed that strayed in frame t does not hand its trace on.  Two calls around the swap
 * of the images, because the final costs -- the medoid's tie-break, and what best_cost is -- are scored on the images every edge
 * reads NOW, which the swap replaces, while the observations may only be set after it:
 *   gpet_batch_ensemble_keep(batch, G, group_of, tol)   BEFORE gpet_batch_set_images: the reduction of gpet_batch_ensemble -- same
 *       validity, members, ties and bits -- into an allocation the batch owns, with the table.  The kept ensemble survives
 *       gpet_batch_set_images and its raw forms; a warm start of any kind, gpet_batch_set_obs, gpet_batch_reset and the next
 *       gpet_final_fit_all drop it.
 *   gpet_batch_ensemble_kept(batch, len_cap, dst, on_device)   copies it out in the layout of gpet_batch_ensemble, byte for byte
 *       what that call writes for the same arguments; GPET_ERR_BAD_ARG (with a message) when none is kept.
 *   gpet_batch_warm_start_groups(batch, from, warm_every, n_obs_out, src_out)   AFTER the swap, where gpet_batch_warm_start is
 *       called, with its rule, its end state and its waits (one; the histories are emptied).  from: GPET_WARM_MEDOID, _BEST_COST
 *       or _CONSENSUS.  Every edge ASSIGNED to group g -- one the device stopped with an error included: it is re-seeded from the
 *       group -- gets its observations from g's source: rint of that member's converged mean, or the consensus row c[k] of g's
 *       kept record; its bounds (x_st, x_en, M, algo_thresh) are its own.  An edge with group_of = -1 gets them from its own fit,
 *       exactly as gpet_batch_warm_start; every edge of a group with n_members = 0 gets the empty set.  src_out (host, [B], may be
 *       NULL): the source used -- an edge index (the edge itself outside any group), -1 for none, -2 for the consensus.
 *       GPET_ERR_BAD_ARG (with a message, nothing touched) when gpet_batch_warm_start_ready refuses, or when no ensemble is kept.
 *   gpet_batch_warm_start_from(batch, src_of, warm_every, n_obs_out)   the explicit form: src_of[e] in [0, B), or -1 for the
 *       empty set.  GPET_ERR_BAD_ARG naming the edge when src_of[e] is out of range or e and its source differ in x_st or x_en.
 *       No status is looked at: the caller chose.  With src_of[e] = e it leaves exactly what gpet_batch_warm_start leaves. */
#define GPET_WARM_MEDOID 0
#define GPET_WARM_BEST_COST 1
#define GPET_WARM_CONSENSUS 2
int gpet_batch_ensemble_keep(gpet_batch* b, int n_groups, const int32_t* group_of, double tol);
int gpet_batch_ensemble_kept(gpet_batch* b, int64_t len_cap, void* dst, int dst_on_device);
int gpet_batch_warm_start_groups(gpet_batch* b, int from, int warm_every, int32_t* n_obs_out, int32_t* src_out);
int gpet_batch_warm_start_from(gpet_batch* b, const int32_t* src_of, int warm_every, int32_t* n_obs_out);

/* ---- tracking bands: every edge traces inside a row band that follows it (the rules: csrc/gpet_band_plan.h) ----
 * A band is (r0, H): rows r0 .. r0 + H - 1 of an M x N frame; H is the batch's, r0 per edge.  Edge e of a banded batch gives, bit for
 * bit, what an unbanded batch gives on rows r0 .. r0 + H - 1 of the FULL-FRAME gradient image G (re-normalised over the band, as an
 * unbanded batch re-normalises the image it is given) with init rows lowered by r0.  The batch's image shape is (H, N): every record
 * it returns (results, history, ensembles, observation sets, gpet_batch_read) is in band rows; the caller adds r0.
 *   gpet_batch_create_banded(ctx, B, M, N, band, images, params, init_xy, out)   init_xy in full-frame rows.  band->H; band->r0 [B] or
 *       NULL (every edge placed from its own init rows by band_place); band->n_pair full-frame gradient images, edge e reads image
 *       band->pair_of[e] (every index must occur).  images: the n_pair images as f32 gradient images (grad; GPET_GRAD_ON_DEVICE in
 *       flags) -- taken as they are, G = grad -- or raw frames with a slot table as gpet_batch_create_raw_multi takes it (n_frames
 *       frames, image p = comp_grad_img(frame frame_of[p], kern[kernel_of[p]]) after dn; GPET_RAW_ON_DEVICE), made once per pair into
 *       memory the batch owns.  Refused with GPET_ERR_BAD_ARG and band_check's reason: H > M, r0 outside [0, M - H], init rows that
 *       span more than H rows, an init outside its band.
 *   gpet_batch_set_images and the gpet_batch_set_raw_images* calls take n_pair images on a banded batch (gpet_batch_image_count
 *       returns n_pair), and move every slot to the band placed or set since the last swap -- r0 is read on the device.
 *   gpet_batch_band_place(batch, src_of, from)   BEFORE the swap (after gpet_batch_ensemble_keep): r0 of every edge for the next
 *       frame by band_place from the trace of its source in full-frame rows -- src_of[e] as gpet_batch_warm_start_from takes it (-1:
 *       the band stays); src_of == NULL and from < 0: the edge itself; src_of == NULL and from = GPET_WARM_*: the source of its group
 *       in the kept ensemble, as gpet_batch_warm_start_groups picks it.  One wave per edge, no host wait.  A source without a usable
 *       row, or an edge that is its own source and was stopped with an error, keeps its band.
 *   gpet_batch_band_set(batch, r0)   the explicit table instead; refused (nothing touched) by band_check, naming the edge.
 *   gpet_batch_band_r0(batch, r0_out)   reads the table back: the bands the slots are at (after a swap: the placed ones).
 *   gpet_batch_warm_start, _groups and _from on a banded batch carry every row from the source's band of the last converged fits
 *       into the destination's new band: y = rint(mean_src[k]) + r0_src_old - r0_dst_new, kept when 0 <= y <= H - 1. */
typedef struct gpet_band {
  int32_t H;             /* rows of every band */
  int32_t n_pair;        /* full-frame gradient images */
  const int64_t* r0;     /* [B], or NULL: placed from the init rows */
  const int32_t* pair_of; /* [B] */
} gpet_band;
typedef struct gpet_band_images {
  const float* const* grad; /* [n_pair] f32 gradient images, or NULL and: */
  const void* const* raw;   /* [n_frames] raw frames of pixel type pix */
  int32_t pix;
  int32_t n_frames;
  int32_t n_kern;
  int32_t reserved;
  const double* const* kern; /* [n_kern] kernels of kh[k] x kw[k] */
  const int32_t* kh;
  const int32_t* kw;
  const int32_t* frame_of;   /* [n_pair] */
  const int32_t* kernel_of;  /* [n_pair] */
  const gpet_denoise* dn;    /* may be NULL */
  unsigned int flags;
} gpet_band_images;
int gpet_batch_create_banded(gpet_ctx* c, int B, int M, int N, const gpet_band* band, const gpet_band_images* images,
                             const gpet_params* params, const int64_t* const* init_xy, gpet_batch** out);
int gpet_batch_band_place(gpet_batch* b, const int32_t* src_of, int from);
int gpet_batch_band_set(gpet_batch* b, const int64_t* r0);
int gpet_batch_band_r0(gpet_batch* b, int64_t* r0_out);

/* ---- endpoint tracking: the init points follow the edge from frame to frame (the rule: csrc/gpet_init_plan.h) ----
 * The rule, for the init point (x, y) of an edge that reads the M x N image G (the H x N slot of a banded batch, rows in band
 * coordinates): among the rows r in [max(0, y - window), min(M - 1, y + window)] whose score s(r) = sum of (double)G[r][c] over
 * c = max(0, x - cols) .. min(N - 1, x + cols) is > 0, the one of largest s -- ties: the smallest |r - y|, then the smallest r -- becomes
 * y; none: y stays.  x never changes; every init point of every edge is moved.  0 <= window <= 4096, 0 <= cols <= 64.
 *   gpet_batch_init_follow(batch, window, cols, init_out)   applies the rule to every edge on the images the batch holds now (one wave per
 *       edge, no host wait).  init_out (host, [B][n_init_max][2] xy in full-frame rows, n_init_max the largest n_init of the batch, unused
 *       entries 0; may be NULL): filled after one wait.  On a banded batch the band tables follow (the full-frame init points and the
 *       (i_lo, i_hi) span gpet_batch_band_place clamps against).
 *   gpet_batch_set_init(batch, init_xy)   the caller's init points instead: init_xy[e] holds the batch's n_init points of edge e, xy in
 *       full-frame rows, with the x the batch was created with; rows in [0, M - 1] of the frame and, on a banded batch, inside the edge's
 *       current band.  Anything else: GPET_ERR_BAD_ARG with the reason, checked on the host before anything is written.
 *   gpet_batch_init_xy(batch, out)   the current init points of all edges, [B][n_init_max][2] xy in full-frame rows.
 * The first two are legal only while no iteration has run since creation, gpet_batch_reset or an image swap (else GPET_ERR_STATE,
 * nothing touched).  They change neither the observation sets nor the last converged fits (the warm start after a swap still needs
 * them) nor the next-frame factor state; gpet_batch_reset keeps the current init points.  In a frame change their place is: ensemble
 * keep, band placement (against the old init span), image swap, init follow, warm start.  (Added without a change of
 * GPET_ABI_VERSION: the surface only grew.) */
int gpet_batch_init_follow(gpet_batch* b, int window, int cols, int64_t* init_out);
int gpet_batch_set_init(gpet_batch* b, const int64_t* const* init_xy);
int gpet_batch_init_xy(gpet_batch* b, int64_t* out);

/* ---- label maps: traces rasterised into uint8 masks on the device (the rules: csrc/gpet_label_plan.h) ----------
 * Rule 1, row maps.  A map is M x N uint8.  Contributing edge e has a grid [x_st, x_en] of len = x_en - x_st + 1 columns, int64 rows
 * t_e[k], k = 0 .. len - 1, and a map index map_of[e] in [-1, n_maps); -1: the edge is in no map.  The edges of a map need not be
 * adjacent.  The threshold of edge e at frame column c, in this order:
 *   1. x_st <= c <= x_en: k = c - x_st;
 *   2. else with GPET_LABELS_EXTEND: k = 0 left of the grid, k = len - 1 right of it;
 *   3. else the edge does not count at c: T = M;
 *   4. a row equal to GPET_LABEL_NO_ROW does not count: T = M;
 *   5. else T_e[c] = min(max(t_e[k], 0), M).
 *   label[f][r][c] = #{e : map_of[e] = f, r >= T_e[c]}: for one edge the mask "at or below the trace", for stacked edges the layer index,
 *       and edges that cross need no ordering.
 *   thick[f][l][c] = #{r in [0, M) : label[f][r][c] = l}, int32 [n_maps][L + 1][N], L the largest number of edges on one map: the
 *       thickness profile of layer l; its sum over c is the layer's area.
 * At most GPET_LABEL_EDGES_MAX edges on a map.  GPET_LABELS_TRANSPOSED writes every map as N x M with out[c][r] = label[r][c] (the
 * frame's own orientation for a vertical batch); thick is the same either way.
 * Rule 2, frame maps of closed outlines.  A map is Ms x Ns uint8 in the coordinates of the raw frame.  Contour e has n vertices
 * (X_j, Y_j), f64, 4 <= n <= GPET_LABEL_VERTS_MAX.  For the pixel (px, py), integers taken as doubles, and every j with (xi, yi) = V_j,
 * (xj, yj) = V_((j + 1) mod n):
 *   1. if (yi > py) != (yj > py): a = (px - xi) * (yj - yi), b = (xj - xi) * (py - yi), every product rounded once, no division;
 *   2. the pixel toggles when yj > yi ? a < b : a > b.
 * The pixel is inside when the toggles are odd in number; label_xy[f][py][px] is the number of contours of map f it is inside (two
 * nested outlines: lumen 2, wall 1, outside 0).  A contour with a vertex that is not finite contributes nothing.
 *   gpet_label_maps(ctx, M, N, n_edges, x_st, len, rows, map_of, n_maps, flags, out, thick)   Rule 1 on the caller's rows: rows holds
 *       len[0] + len[1] + ... int64, edge after edge (host).  out: n_maps pointers to M * N bytes; thick (may be NULL):
 *       gpet_label_thick_count elements.
 *   gpet_label_maps_xy(ctx, Ms, Ns, n_contours, n_vert, xy, map_of, n_maps, flags, out)   Rule 2 on the caller's vertices: xy holds
 *       (x, y) pairs, contour after contour (host).
 *   gpet_batch_label_maps(batch, map_of, n_maps, flags, out, thick)   Rule 1 from the batch's converged fits where they lie:
 *       t_e[k] = (int64) rint(mean[k]) as gpet_batch_results rounds it, plus the first row of the band the fit was made in on a banded
 *       batch; a mean that is not finite is GPET_LABEL_NO_ROW, and an edge whose status is not GPET_OK contributes nothing.  The maps
 *       have the batch's full-frame shape (M x N as the batch traces it; a banded batch: full-frame rows).
 *   gpet_batch_label_maps_xy(batch, polar, Ms, Ns, map_of, n_maps, flags, out)   Rule 2 from the converged fits of a batch on polar
 *       frames: polar is the spec the frames were unwrapped with, n_centres 1 or n_maps, the centre of map f is centre f.  Every
 *       contributing edge has x_st = pad and x_en = pad + n_theta (else GPET_ERR_BAD_ARG naming the edge).  Vertex j = 0 .. n_theta - 1
 *       comes from grid index j: rho = r0 + (double)t dr, X = cx + rho cos_t[j], Y = cy + rho sin_t[j], not clamped; the seam's second
 *       column is no vertex, the polygon closes from n_theta - 1 to 0.
 *   gpet_label_thick_count(n_maps, L, N, count)   the int32 elements of thick.
 * flags: GPET_LABELS_EXTEND, GPET_LABELS_TRANSPOSED (Rule 1), GPET_LABELS_OUT_ON_DEVICE: out[] and thick are DEVICE pointers, the work
 * is enqueued on the context's stream and nothing waits; otherwise the call is complete on return.
 * The batch forms are valid exactly when gpet_batch_results is (GPET_ERR_BAD_ARG with a message otherwise); they leave the loop's
 * state, the fits and a kept ensemble untouched, and their scratch is an allocation of its own, made on first use: a batch that never
 * asks for a map holds and enqueues nothing for it.  Refused with GPET_ERR_BAD_ARG, gpet_last_error carrying label_check's words, and
 * nothing launched: a null pointer, n_maps < 1, a map_of entry outside [-1, n_maps), a map with no edge or with more than 32, a grid
 * outside [0, N), M * N above 2^31, a vertex count outside [4, 4096], a frame below 2 x 2.  (Added without a change of
 * GPET_ABI_VERSION: the surface only grew.) */
#define GPET_LABELS_EXTEND 1u
#define GPET_LABELS_TRANSPOSED 2u
#define GPET_LABELS_OUT_ON_DEVICE 4u
#define GPET_LABEL_EDGES_MAX 32
#define GPET_LABEL_VERTS_MAX 4096
#define GPET_LABEL_NO_ROW INT64_MIN
int gpet_label_maps(gpet_ctx* ctx, int M, int N, int n_edges, const int32_t* x_st, const int32_t* len, const int64_t* rows,
                    const int32_t* map_of, int n_maps, unsigned int flags, void* const* out, int32_t* thick);
int gpet_label_maps_xy(gpet_ctx* ctx, int Ms, int Ns, int n_contours, const int32_t* n_vert, const double* xy, const int32_t* map_of,
                       int n_maps, unsigned int flags, void* const* out);
int gpet_batch_label_maps(gpet_batch* b, const int32_t* map_of, int n_maps, unsigned int flags, void* const* out, int32_t* thick);
int gpet_batch_label_maps_xy(gpet_batch* b, const gpet_polar* polar, int Ms, int Ns, const int32_t* map_of, int n_maps,
                             unsigned int flags, void* const* out);
int gpet_label_thick_count(int n_maps, int L, int N, int64_t* count);

/* ---- denoise quality metrics: what the reference's denoise(verbose=True) prints (gpet_utils.py:151-156) ------------------------------ */
/* The four figures of scikit-image 0.18.3 for n_img pairs (a = the frame as given, b = the denoised frame, M x N each, pixel types pix_a
 * and pix_b, which may differ): peak_signal_noise_ratio(a, b), structural_similarity(a, b) in its default form (uniform window),
 * normalized_root_mse(a, b, normalization='min-max') and shannon_entropy(b).  csrc/gpet_metrics_plan.h states the arithmetic:
 *   PSNR, NRMSE  a - b and its square round in the library's working type (f32 unless a or b is f64), the squares are summed in f64;
 *                data_range 0: the library's rule from a's type (255, 65535; floats 1 when min(a) >= 0, else 2 -- a float frame
 *                outside [-1, 1] is refused in the library's words); min(a), max(a) and their difference in the working type.
 *   SSIM         both frames widened to f64; the planes x, y, x x, y y, x y through scipy.ndimage.uniform_filter's running sums (axis 0,
 *                then axis 1, reflect), S in the library's order of operations, no fused multiply-add: the S map is the library's bit
 *                for bit.  data_range 0: 255, 65535, floats 2.  The mean runs over the map cropped by (win_size - 1) / 2.
 *   entropy      the counts of b's distinct values (-0.0 and 0.0 are one) are exact: b's order-preserving keys are sorted in workspace.
 * The deviations are three summation orders -- the squared differences, S over the crop, the entropy terms -- which the plan header
 * defines (metrics_sum); DESIGN.md section 9 gives the bounds that follow.  Frames that hold a NaN have no defined figures.
 * out (host, f64 [n_img][4]): psnr, ssim, nrmse, entropy of every pair.  ssim_maps (NULL, or [n_img] pointers to f64 [M*N]): the S map
 * of every pair.  flags: GPET_RAW_ON_DEVICE (raw_a[] are device pointers), GPET_METRICS_B_ON_DEVICE (raw_b[] are),
 * GPET_METRICS_MAPS_ON_DEVICE (ssim_maps[] are).  The pairs go through workspace the context owns, grown on demand, in chunks of at most
 * 512 MB: six f64 planes per pair and the staged copies of host frames.  The call waits for the stream: it reads the sums back and
 * finishes the figures on the host.  GPET_ERR_BAD_ARG, gpet_last_error carrying metrics_check's words (the library's own where it has
 * some), and nothing launched: a null pointer, no frame, an unknown pixel type, win_size above an extent ("win_size exceeds image
 * extent. ..."), even ("Window size must be odd.") or below 3, a negative K1 or K2, a data_range that is negative or not finite, a
 * frame above 2^26 pixels or whose workspace exceeds the chunk budget, unknown flag bits.  (Added without a change of
 * GPET_ABI_VERSION: the surface only grew.) */
typedef struct gpet_metrics {
  int32_t win_size;               /* odd, 3 .. min(M, N); the library's default 7 */
  int32_t use_sample_covariance;  /* not 0: covariances normalised by NP / (NP - 1) (the library's default) */
  double K1, K2;                  /* the library's defaults 0.01, 0.03 */
  double data_range;              /* above 0: R of PSNR and SSIM; 0: the library's rule from a's pixel type */
} gpet_metrics;
#define GPET_METRICS_B_ON_DEVICE 32u
#define GPET_METRICS_MAPS_ON_DEVICE 64u
int gpet_metrics_images(gpet_ctx* ctx, const void* const* raw_a, int pix_a, const void* const* raw_b, int pix_b, int n_img, int M, int N,
                        const gpet_metrics* spec, unsigned int flags, double* out, double* const* ssim_maps);

/* ---- measurement -------------------------------------------------------------------------- */
/* Enqueue one stage `reps` times between two hipEvents on the context's stream and return the
 * mean milliseconds per repetition.  stage: 0 fit+predict+cov, 1 factor, 2 normals, 3 sample
 * GEMM, 4 scoring+top-k, 5 curve KDE; single kernels: 100 fit, 101 predict, 102 covariance, 110 pivoted
 * Cholesky, 111 Gram, 112 Jacobi, 113 factor rows, 130 sample GEMM, 140 scoring, 141 top-k, 150 KDE prep,
 * 151 fused KDE (5, 150, 151: the loop form -- raw density, band rows only), 152 KDE normalise (stage-API form),
 * 160 column scan of the pixel selection (loop form); 170 the in-place normaliser of the raw-frame path over the batch's image
 * slots (with the neutral pair min 0, max 1: the images keep their bits);
 * structured loop path: 120 fit, 121 U/H/mean, 122 Jacobi, 123 factor rows + sign pass.
 * (bench.py's roofline leg; leaves the loop state as-is.) */
int gpet_profile_stage(gpet_batch* b, int stage, int reps, float* ms_per_rep);

#ifdef __cplusplus
}
#endif
#endif /* GPET_HIP_H */
