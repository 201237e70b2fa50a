/*
 * rti.h -- C ABI of the MI355X-native RTI reflectance fitter (PTM / HSH).
 *
 * Drop-in boundary for the per-pixel reflectance-fit hot path of
 * bara96/Smartphone-based-RTI (reference @ v0).  The reference has no FFI of
 * its own: the path sits behind plain Python calls in analysis.py.  Each entry
 * point below names the reference code it replaces.  The Python package
 * (smartphone-based-rti_amd/rti) binds these symbols with ctypes; INTEGRATION.md
 * shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - Plain pointers and sizes only.  Functions named rti_fit_* / rti_relight*
 *     take DEVICE pointers (hipMalloc'd or torch CUDA tensors) and enqueue
 *     asynchronously on `stream` (a hipStream_t; NULL = default stream).  They
 *     never allocate, free or synchronise, so they can be captured in a
 *     hipGraph.  Functions named rti_design_* / rti_pinv / rti_basis_* are
 *     host-only and take HOST pointers.
 *   - Return value: RTI_OK (0) or an RTI_ERR_* status; rti_last_error()
 *     returns a thread-local message for the most recent failure.
 *   - Reentrant: no global mutable state besides the thread-local message.
 *   - Intensity stacks are LIGHT-MAJOR: I[c][n][p] with pixel p = y*W + x
 *     contiguous inside one light plane (strides in elements; 0 = dense).
 *     The reference stacks pixel-major [y][x][n] (analysis.py:217-219);
 *     rti_fit_shared_pm and the per-pixel "dirs" entry point take that layout.
 */
#ifndef RTI_H
#define RTI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---- */
#define RTI_OK              0
#define RTI_ERR_BAD_ARG     1   /* null pointer, non-positive size, k/N mismatch, N < k */
#define RTI_ERR_UNSUPPORTED 2   /* valid but unsupported combination (dtype/basis/layout) */
#define RTI_ERR_HIP         3   /* HIP runtime error at launch */
#define RTI_ERR_SINGULAR    4   /* singular system (the reference's SciPy Rbf raises LinAlgError) */

/* ---- bases ---- */
#define RTI_BASIS_PTM6  0   /* (lu², lv², lu·lv, lu, lv, 1), analysis.py:285 */
#define RTI_BASIS_HSH16 1   /* hemispherical harmonics l=0..3 (build-defined) */
#define RTI_BASIS_HSH9  2   /* hemispherical harmonics l=0..2 */

/* ---- element types ---- */
#define RTI_F32 0
#define RTI_U8  1
#define RTI_I32 2
#define RTI_F64 3

/* ---- coefficient layouts ---- */
#define RTI_COEF_PIXEL_MAJOR 0  /* coef[c][p][k] */
#define RTI_COEF_PLANAR      1  /* coef[c][k][p] */

/* ---- relight output layouts ---- */
#define RTI_OUT_EVAL_MAJOR  0   /* out[e][p]: one image per light (prepare_images_data order) */
#define RTI_OUT_PIXEL_MAJOR 1   /* out[p][e]: interpolate_intensities order [y][x][ly][lx] */

/* ---- shared-fit kernel selection ---- */
#define RTI_KERNEL_AUTO 0
#define RTI_KERNEL_VALU 1   /* pinv in SGPRs, fp32 FMA stream */
#define RTI_KERNEL_MFMA 2   /* v_mfma_f32_16x16x4_f32, pinv staged in LDS */
#define RTI_KERNEL_TILE 3   /* the same MFMA fed from a double-buffered LDS tile [4·sp lights][256·rc pixels] */
/* OR-able tuning flags (VALU kernel; only NONTEMPORAL applies to the MFMA kernel) */
#define RTI_KERNEL_NONTEMPORAL 0x100  /* non-temporal intensity loads (the stack is read once) */
#define RTI_KERNEL_PINV_LDS    0x200  /* stage pinv in LDS instead of scalar loads */
#define RTI_KERNEL_NT_STORE    0x400  /* non-temporal coefficient stores */
#define RTI_KERNEL_STAGE       0x800  /* pixel-major output transposed through LDS (1 KiB stores) */
#define RTI_KERNEL_ROTATE      0x10000000  /* AUTO PTM-6 fp32: each wave starts its light sweep at its own plane; rti_fit_shared_pm: each wave streams one contiguous run of units (measurement variants) */
#define RTI_KERNEL_ROUNDS      0x40000000  /* AUTO PTM-6 fp32/int32: launch generations as rounds of one launch (rti_fit.hip) */
#define RTI_KERNEL_ONE_LAUNCH  0x20000000  /* AUTO: one launch, no launch generations (measurement variant; rti_fit.hip) */
/* VALU chunks per lane (bits 12-15; 0 = AUTO): a wave reads chunks*1 KiB contiguous per plane */
#define RTI_KERNEL_CHUNKS_SHIFT 12
#define RTI_KERNEL_CHUNKS(n)   ((n) << RTI_KERNEL_CHUNKS_SHIFT)
/* TILE kernel: CHUNKS(rc) sets the tile width (256·rc pixels; 0 = 8, or 4 above N = 512),
 * TILE_PLANES(sp) the light planes each wave loads per step (bits 16-19, 0 = 2) */
#define RTI_KERNEL_TILE_PLANES_SHIFT 16
#define RTI_KERNEL_TILE_PLANES(n)    ((n) << RTI_KERNEL_TILE_PLANES_SHIFT)
/* TILE kernel: tiles in the LDS ring (bits 20-23; 0 = 2): 2 = register-staged double buffer,
 * 3 or 4 = global_load_lds ring with depth-1 steps in flight (fp32 stacks) */
#define RTI_KERNEL_TILE_DEPTH_SHIFT 20
#define RTI_KERNEL_TILE_DEPTH(n)    ((n) << RTI_KERNEL_TILE_DEPTH_SHIFT)
/* TILE kernel, fp32 stacks: waves per workgroup (bits 24-27; 0 = 4).  8 = one light plane per wave
 * and step with the plane loads issued DEPTH − 1 steps ahead in registers (DEPTH 2 or 3) */
#define RTI_KERNEL_TILE_WAVES_SHIFT 24
#define RTI_KERNEL_TILE_WAVES(n)    ((n) << RTI_KERNEL_TILE_WAVES_SHIFT)

typedef void* rti_stream_t; /* hipStream_t */

/* ---- library info ---- */
int         rti_version(void);                 /* 10000*major + 100*minor + patch */
const char* rti_status_string(int status);
const char* rti_last_error(void);
/* Kernel launches issued by this thread's most recent rti_fit_shared / rti_fit_shared_residual call:
 * 1, or more when AUTO issues a large fit as consecutive "launch generations" over pixel ranges
 * (rti_fit.hip).  For timing tools (per-launch figures); the results do not depend on it. */
int rti_last_launch_count(void);
int         rti_basis_terms(int basis);        /* k for a basis, or -1 */
int         rti_device_count(void);            /* hipGetDeviceCount, 0 on failure */

/* ---- host: basis / design matrix / pseudo-inverse ----------------------------------
 * rti_design_matrix replaces the design-row loop of _interpolate_PTM
 * (analysis.py:280-291): A[n][k] in fp64 with PTM monomials formed in fp32 from
 * fp32 (lu, lv), as the reference does.
 * rti_pinv replaces the SVD solve (analysis.py:293-298) for a SHARED light set:
 * pinv[k][n] = V Σ⁻¹ Uᵀ by one-sided Jacobi SVD in fp64.  rcond < 0 keeps the
 * reference's semantics (no threshold: a zero singular value gives inf/NaN);
 * rcond >= 0 zeroes σ <= rcond·σ_max.  Returns RTI_ERR_BAD_ARG when n < k
 * (the reference raises ValueError at analysis.py:298).
 * rti_basis_eval evaluates the basis at E host (lu, lv) pairs (fp64 inputs). */
int rti_design_matrix(int basis, const float* lu, const float* lv, int n, double* A);
int rti_pinv(int basis, const float* lu, const float* lv, int n, double rcond, double* pinv);
int rti_basis_eval(int basis, const double* lu, const double* lv, int E, double* out);
/* rti_gram_inverse: the Gram (pseudo-)inverse ginv[k][k] = (AᵀA)⁺ = V Σ⁻² Vᵀ of the same shared
 * design and SVD as rti_pinv (so pinv = ginv·Aᵀ; rcond as there), the operator with which
 * rti_fit_shared_residual turns Aᵀ I into coefficients (analysis.py:293-298). */
int rti_gram_inverse(int basis, const float* lu, const float* lv, int n, double rcond, double* ginv);
/* rti_lsq_factors: the thin SVD A = U Σ Vᵀ of the same shared design (same Jacobi SVD, rcond as in
 * rti_pinv) split as the reference's solve splits it (analysis.py:295-298: c = uᵀL, w = c/s, a = vᵀw):
 * U[n][k] = the orthonormal left singular vectors, W[k][k] = V Σ⁻¹ (W[i][m] = v_im / σ_m), so that
 * pinv = W·Uᵀ.  A truncated σ_m zeroes column m of both; σ_m = 0 without rcond leaves NaN in
 * column m (0·inf), the reference's division by a zero singular value.  Host fp64. */
int rti_lsq_factors(int basis, const float* lu, const float* lv, int n, double rcond, double* U, double* W);

/* ---- device: shared-direction fit (the north_star hot path) ------------------------
 * Replaces interpolate_intensities' per-pixel loop + _interpolate_PTM's solve
 * (analysis.py:321-363, :293-298) when every pixel sees the same light set:
 *   coef[c][p][i] = Σ_n pinv[i][n] · I[c][n][p]
 * pinv: device fp32 [k][N].  I: device, dtype in_dtype (F32, U8 or I32),
 * element (c,n,p) at c*channel_stride + n*light_stride + p
 * (light_stride 0 = P, channel_stride 0 = N*light_stride).
 * coef: device fp32, layout coef_layout, channel stride coef_channel_stride
 * (0 = P*k).  k must equal rti_basis_terms(basis) for some basis, or any
 * 1 <= k <= 16 with kernel = RTI_KERNEL_MFMA. */
int rti_fit_shared(const float* pinv, int k, int N,
                   const void* I, int in_dtype, int64_t P, int C,
                   int64_t light_stride, int64_t channel_stride,
                   float* coef, int coef_layout, int64_t coef_channel_stride,
                   int kernel, rti_stream_t stream);

/* ---- device: shared-direction fit on PIXEL-major stacks (rti_fit_pm.hip) ---------------
 * The same contraction as rti_fit_shared on the reference's own stack layout: compute_intensities
 * returns (R, R, N) arrays (analysis.py:217-219), pixel p's N intensities contiguous:
 *   coef[c][p][i] = Σ_n pinv[i][n] · I[c*channel_stride + p*pixel_stride + n]
 * (pixel_stride 0 = N, channel_stride 0 = P*pixel_stride).  pinv, coef, coef_layout and
 * coef_channel_stride as rti_fit_shared; in_dtype F32 / I32 / U8.
 * AUTO for k <= 9 (the VALU generations form): launches over a channel's 64-pixel blocks in which every wave
 * streams its units HBM -> a private LDS ring by 1-KiB LDS-DMAs (bounded buffer loads), computes one pixel per
 * lane with packed FMAs and keeps the coefficients in registers until the launch's end (one store burst per
 * wave).  AUTO for k = 16, and with RTI_KERNEL_STAGE for any k: the DIRECT form loads 16-pixel groups straight
 * into VGPRs as v_mfma_f32_16x16x4_f32 operands and writes the coefficients in LDS-staged 1-KiB bursts
 * (non-temporal for AUTO k = 16; N % 4 == 0, N <= 256).  RTI_KERNEL_MFMA: the MFMA stream through the LDS ring
 * for every k; RTI_KERNEL_TILE: a double-buffered block form.  All forms compute the same coefficients.
 * These take F32 / I32 stacks, k in {6, 9, 16}, pixel_stride = N, P·N and channel_stride multiples of 4,
 * I 16-byte aligned, coef 8- (VALU generations) or 16-byte aligned, P·k·4 < 2^31 (all but the VALU
 * generations) and N within the LDS budget (rti_fit_shared_pm_plan); RTI_KERNEL_MFMA / TILE fail with
 * RTI_ERR_UNSUPPORTED outside that, AUTO and RTI_KERNEL_VALU run one lane per pixel instead (any shape, uint8
 * included).  Tuning flags (the only bits accepted besides the selector; anything else is RTI_ERR_BAD_ARG):
 * RTI_KERNEL_TILE_WAVES(W) waves per workgroup (direct form: per CU), RTI_KERNEL_CHUNKS(n) (VALU generations:
 * at least n launches per channel; MFMA stream: n× the smallest unit; block form: 16n-pixel blocks; direct
 * form: n launch generations), RTI_KERNEL_ROTATE (VALU generations and MFMA stream: each wave one contiguous
 * run instead of interleaved units), RTI_KERNEL_NT_STORE (MFMA stream k = 16 and direct form: non-temporal
 * coefficient stores), RTI_KERNEL_STAGE (AUTO: the direct form). */
int rti_fit_shared_pm(const float* pinv, int k, int N, const void* I, int in_dtype, int64_t P, int C,
                      int64_t pixel_stride, int64_t channel_stride,
                      float* coef, int coef_layout, int64_t coef_channel_stride,
                      int kernel, rti_stream_t stream);
/* 0 if rti_fit_shared_pm runs one lane per pixel (the fallback) for this shape and kernel selection, else
 * form·10^8 + size·1000 + W: form RTI_PM_VALU_STREAM (AUTO, k <= 9: the VALU generations form) or
 * RTI_PM_MFMA_STREAM (RTI_KERNEL_MFMA) with size = KiB of LDS ring per wave and W = waves per workgroup,
 * RTI_PM_BLOCK (RTI_KERNEL_TILE, or N too small for a ring) with size = pixels per block, or RTI_PM_DIRECT
 * (AUTO k = 16, AUTO | RTI_KERNEL_STAGE) with size = 16-light steps and W = waves per CU. */
#define RTI_PM_VALU_STREAM 1
#define RTI_PM_MFMA_STREAM 2
#define RTI_PM_BLOCK       3
#define RTI_PM_DIRECT      4
int rti_fit_shared_pm_plan(int k, int N, int in_dtype, int64_t P, int C, int64_t pixel_stride,
                           int64_t channel_stride, int kernel);

/* ---- 8-bit stacks: the shared fit on the int8 matrix cores -------------------------
 * The reference's intensities are the uint8 V channel (FeatureMatcher.py:183-184, analysis.py:219).
 * rti_q8_operator (host) turns an fp64 operator pinv[k][N] (rti_pinv) into the fixed-point form the
 * kernel reads: each row scaled to 27-bit fixed point and split into four int8 digits laid out as
 * v_mfma_i32_16x16x64_i8 A fragments, plus per-row scales and sign-flip corrections (layout:
 * smartphone-based-rti_amd/csrc/rti_q8.h).  op must hold rti_q8_operator_bytes(k, N) bytes; it is copied
 * to the device by the caller (16-byte aligned).  Non-finite pinv entries (an exactly rank-deficient light
 * set without rcond) return RTI_ERR_BAD_ARG: those fits keep the fp32 path and its NaN semantics.
 * rti_fit_shared_q8 = rti_fit_shared for U8 stacks: coef[c][p][i] = Σ_n pinv[i][n]·I[c][n][p] with the
 * digit products summed exactly in int32 and combined in fp64 (|Δc_i| <= 2^-28·max_n|pinv[i][n]|·Σ_n I_n,
 * then one fp32 rounding), k ∈ {6, 9, 16}, N <= rti_fit_shared_q8_max_lights().  P, strides, I, op and
 * coef 16-byte aligned (else RTI_ERR_UNSUPPORTED).  kernel: RTI_KERNEL_ONE_LAUNCH or 0 (AUTO). */
int64_t rti_q8_operator_bytes(int k, int N);
int rti_q8_operator(const double* pinv, int k, int N, void* op);
int rti_fit_shared_q8_max_lights(void);
int rti_fit_shared_q8(const void* op, int k, int N, const uint8_t* I, int64_t P, int C,
                      int64_t light_stride, int64_t channel_stride,
                      float* coef, int coef_layout, int64_t coef_channel_stride,
                      int kernel, rti_stream_t stream);

/* ---- device: shared fit of 8-bit stacks on the fp16 matrix cores (rti_fit_h16.hip) ----
 * The same contraction as rti_fit_shared_q8 with the operator split as w·s = hi + lo in fp16 (s a power
 * of two per row: 22 significant bits) and fp32 accumulation (v_mfma_f32_16x16x32_f16): the accuracy of
 * the fp32 stream, a quarter of the q8 form's accumulator registers per pixel: 1024-pixel tiles with two
 * workgroups per CU for k <= 9 (when both fit in the LDS), else 2048-pixel tiles with one; kernel flags
 * (measurement): RTI_KERNEL_TILE_WAVES(1|2|3) forces the 2048- / 1024-pixel tile / 2048 pixels on 16 waves, RTI_KERNEL_CHUNKS(n) n tiles
 * per workgroup, RTI_KERNEL_TILE_DEPTH(1|4|8) 16-pixel groups per read/MFMA round (all bit-identical).
 * rti_h16_operator builds the operator (rti_h16_operator_bytes(k, N)
 * bytes, device copy 16-byte aligned) from the fp64 pseudo-inverse (non-finite entries -> RTI_ERR_BAD_ARG).
 * Arguments, alignment and layouts as rti_fit_shared_q8; N <= rti_fit_shared_h16_max_lights().
 * op (here and for rti_fit_shared_q8) must be the operator built for the SAME k and N: the kernel copies
 * rti_*_operator_bytes(k, N) bytes of it into LDS and the buffer carries no size the ABI could check
 * (the Python layer checks the tensor's size). */
int64_t rti_h16_operator_bytes(int k, int N);
int rti_h16_operator(const double* pinv, int k, int N, void* op);
int rti_fit_shared_h16_max_lights(void);
int rti_fit_shared_h16(const void* op, int k, int N, const uint8_t* I, int64_t P, int C,
                       int64_t light_stride, int64_t channel_stride,
                       float* coef, int coef_layout, int64_t coef_channel_stride,
                       int kernel, rti_stream_t stream);

/* ---- device: per-pixel residuals of the shared-direction fit -----------------------
 * Fit quality next to rti_fit_shared's coefficients (the reference computes the same
 * least-squares solution, analysis.py:280-298, and never reports its residual):
 *   res[c][p]     = sqrt( Σ_n (I[c][n][p] − Σ_i A[n][i]·coef[c][p][i])² / N )
 *   partial[c][b] = Σ of the squared residuals (before /N) of workgroup b's pixels, fp64
 * A: device fp32 design matrix [N][k] (rti_design_matrix rounded to fp32); k ∈ {6, 9, 16}.
 * I / coef / strides exactly as rti_fit_shared.  res: device fp32 [C][P].
 * partial: NULL, or device fp64 [C][rti_fit_residual_blocks(P)] that the caller zeroes
 * (entries past the launched grid stay 0); its sum over b is channel c's residual energy.
 * A second HBM pass over the stack (4 + 4(k+1)/N bytes per pixel·light). */
int64_t rti_fit_residual_blocks(int64_t P);
int rti_fit_residual(const float* A, int k, int N, const void* I, int in_dtype, int64_t P, int C,
                     int64_t light_stride, int64_t channel_stride, const float* coef, int coef_layout,
                     int64_t coef_channel_stride, float* res, double* partial, rti_stream_t stream);

/* ---- device: shared-direction fit + residuals in ONE pass over the stack ---------------
 * The north_star's fit with per-pixel residuals from wavefront reductions, reading the stack once
 * (analysis.py:280-298 is the solve; its residual is never reported by the reference):
 *   b = Aᵀ I[c][·][p], q = ‖I[c][·][p]‖²      accumulated in fp64 (exact fp32×fp32 products)
 *   coef[c][p] = ginv · b                      (fp32 out, layout coef_layout, as rti_fit_shared)
 *   ss = q − coefᵀ b,  res[c][p] = sqrt(ss/N), partial[c][blk] = Σ_workgroup ss (fp64)
 * A: device fp64 design matrix [N][k] (rti_design_matrix); ginv: device fp64 [k][k]
 * (rti_gram_inverse); k ∈ {6, 9, 16}.  I / strides / coef as rti_fit_shared.  res: NULL or device
 * fp32 [C][P]; partial: NULL or device fp64 [C][rti_fit_shared_residual_blocks(P)] the caller zeroes.
 * kernel: RTI_KERNEL_CHUNKS(n) overrides the chunks per lane (0 = AUTO); other bits ignored.
 * 4 + 4(k+1)/N bytes per pixel·light (one stack read + coefficients + residual map). */
int64_t rti_fit_shared_residual_blocks(int64_t P);
int rti_fit_shared_residual(const double* A, const double* ginv, int k, int N, const void* I, int in_dtype,
                            int64_t P, int C, int64_t light_stride, int64_t channel_stride,
                            float* coef, int coef_layout, int64_t coef_channel_stride,
                            float* res, double* partial, int kernel, rti_stream_t stream);
/* The same one-pass fit with the reference's SVD solve instead of the Gram form (analysis.py:295-298):
 *   y = Uᵀ I[c][·][p], q = ‖I[c][·][p]‖²      (fp64),  coef = W · y,  ss = q − yᵀ y
 * U: device fp64 [N][k], W: device fp64 [k][k] (rti_lsq_factors).  Never forms AᵀA, so coefficients
 * keep cond(A)·1e-16 relative accuracy (the Gram form: cond(A)²·1e-16) — what the reference's SVD
 * returns for ill-conditioned light sets.  Every other argument, the traffic and the speed as
 * rti_fit_shared_residual; this is the form rti.fit_with_residual uses. */
int rti_fit_shared_residual_svd(const double* U, const double* W, int k, int N, const void* I, int in_dtype,
                                int64_t P, int C, int64_t light_stride, int64_t channel_stride,
                                float* coef, int coef_layout, int64_t coef_channel_stride,
                                float* res, double* partial, int kernel, rti_stream_t stream);

/* ---- device: robust shared-direction fit (rti_fit_robust.hip) --------------------------
 * The least squares of analysis.py:280-298 with the samples the model cannot describe left out: an
 * intensity window (clipped highlights at 255, self-shadow at 0 in the reference's 8-bit V channel) and,
 * with iters > 0, Huber-weighted IRLS.  Per channel c and pixel p, with a_n the rows of A and
 * y_n = I[c][n][p] in fp64:
 *   window    win_n = (lo <= y_n <= hi), compared on the input value; m = Σ win_n (±inf = no bound)
 *   solve(w)  G = Σ w_n a_n a_nᵀ, b = Σ w_n a_n y_n in fp64, Cholesky of G; the solve FAILS at a pivot
 *             d_j <= 1e-10·max_i G_ii, else coef = G⁻¹ b
 *   fallback  if m < min_lights or solve(win) fails the pixel uses every light (win_n = 1, m = N,
 *             coef = solve(1)) and *fallback_px is incremented; if that fails too coef and res are NaN
 *             (as rti_fit_perpixel_cam for a singular light set with rcond >= 0)
 *   IRLS      for t = 1..iters: r_n = y_n − a_n·coef, w_n = win_n·(|r_n| <= delta ? 1 : delta/|r_n|)
 *             (delta in intensity units), coef = solve(w); a failed solve keeps the previous coef and
 *             ends that pixel's iteration
 *   coef      fp32, coef_layout / coef_channel_stride as rti_fit_shared
 *   res[c][p]  = sqrt(Σ win_n r_n² / m), r from the final coef; fp32 [C][P], may be NULL
 *   kept[c][p] = m (N on fallback pixels); int32 [C][P], may be NULL
 * A: device fp64 design matrix [N][k] (rti_design_matrix).  I, in_dtype (F32 / U8 / I32), P, C and the
 * strides as rti_fit_shared (light-major).  fallback_px: NULL or a device int the caller zeroes.
 * k ∈ {6, 9}; k = 16 returns RTI_ERR_UNSUPPORTED: one lane owns one pixel, and 136 + 16 fp64
 * accumulators do not fit a lane's registers (splitting a pixel over lanes is future work).
 * RTI_ERR_BAD_ARG: null A / I / coef, N < k, lo > hi or a NaN bound, min_lights outside [k, N], iters
 * outside [0, 16], delta <= 0 with iters > 0, or any kernel bit but RTI_KERNEL_ONE_LAUNCH.
 * Forms (the same arithmetic in the same order): RESIDENT (AUTO when iters > 0 and a tile fits) copies a
 * workgroup's tile [N][TP] of the stack into LDS once and runs the window pass and every IRLS pass from
 * there, so the stack is read from HBM once whatever iters is; TP = the largest of 256 / 128 / 64 pixels
 * with N·TP·sizeof(element) <= 160 KiB.  STREAMING (no tile fits, iters == 0, or kernel =
 * RTI_KERNEL_ONE_LAUNCH, for measurement and tests) reads the stack from global memory in every pass:
 * once for iters == 0, iters + 2 times otherwise.  rti_fit_shared_robust_plan returns 0 for the
 * streaming form, else the resident tile's pixel count TP. */
int rti_fit_shared_robust(const double* A, int k, int N, const void* I, int in_dtype, int64_t P, int C,
                          int64_t light_stride, int64_t channel_stride,
                          float lo, float hi, int min_lights, int iters, float delta,
                          float* coef, int coef_layout, int64_t coef_channel_stride,
                          float* res, int32_t* kept, int* fallback_px, int kernel, rti_stream_t stream);
int rti_fit_shared_robust_plan(int k, int N, int in_dtype, int iters, int kernel);

/* ---- device: photometric stereo (rti_ps.hip) -------------------------------------------
 * Robust Lambertian normals and albedo fitted to the stack itself: I_n = g·l_n per pixel with the
 * samples the model cannot describe (attached shadow, clipped highlight) left out, n = g/|g| and albedo
 * |g|: the normal map of RTIBuilder and Relight.  (rti_ptm_normals and rti_hsh_normals read a normal off a
 * fitted function and inherit what shadows and highlights did to that fit.)
 *
 * rti_ps_design (host): A[n][3] = (lu, lv, lw), lw = sqrt(max(0, 1 − lu² − lv²)) formed in fp64 from the
 * fp32 inputs; a caller with measured lz writes its own third column.  RTI_ERR_BAD_ARG: a null pointer, n < 1.
 *
 * rti_photometric_stereo: per channel c and pixel p the fit is rti_fit_shared_robust's, word for word, at
 * k = 3 (window compared on the input value, solve(w) with the same Cholesky and pivot rule, fallback to
 * every light, Huber IRLS; res, kept and fallback_px, one count per channel-pixel that fell back, as there).
 * It gives g_c in fp64.  Then, in fp64 without contraction, in the written order:
 *   g      = g_0 (C = 1);  g_j = fma(w_2, g_2j, fma(w_1, g_1j, w_0·g_0j)) (C = 3)
 *   s      = sqrt(g_x² + g_y² + g_z²),  n = g/s
 *   albedo_c = g_c·n, an fma chain over x, y, z starting from 0
 *   kind 0  s > 0 and g_z >= 0
 *   kind 1  s > 0 and g_z < 0: the normal is returned as fitted, not clamped
 *   kind 2  s == 0: n = (0, 0, 1), albedo as defined (0 for C = 1)
 *   kind 4  a non-finite component of any g_c: n and every albedo are NaN; res and kept are what the fit
 *           produced                                              (3 is not used: rti_ptm_normals' numbers)
 * and every output is rounded once to fp32.
 * A: device fp64 [N][3].  I, in_dtype (F32 / U8 / I32), P and the strides as rti_fit_shared (light-major);
 * C = 1 (grey) or 3 (RGB: one normal per pixel from all three channels).  w: HOST [3], NULL = 0.299, 0.587,
 * 0.114; read only when C == 3.  normals: device fp32, normal_layout as rti_ptm_normals; albedo: device fp32
 * [C][P]; kind: uint8 [P] or NULL; res: fp32 [C][P] or NULL; kept: int32 [C][P] or NULL; fallback_px: NULL or
 * a device int the caller zeroes.
 * Every argument check answers before any HIP call.  RTI_ERR_BAD_ARG: null A / I / normals / albedo; N < 3;
 * P < 1; lo > hi or a NaN bound; min_lights outside [3, N]; iters outside [0, 16]; delta <= 0 or NaN with
 * iters > 0; a bad normal layout; a non-finite weight; a non-zero light_stride < P; with C = 3 a non-zero
 * channel stride below its dense value; any kernel bit but RTI_KERNEL_ONE_LAUNCH.  RTI_ERR_UNSUPPORTED: C
 * outside {1, 3}; an in_dtype other than F32 / U8 / I32.
 * One launch; one lane owns one pixel with all its channels.  Forms (the same arithmetic in the same order,
 * hence the same bits): STREAMING reads the samples from global memory in every pass (iters == 0: the stack
 * once, the residual energy from q − 2cᵀb + cᵀGc; also when no tile fits, or with RTI_KERNEL_ONE_LAUNCH).
 * RESIDENT (iters > 0) copies a workgroup's tile [C][N][TP] into LDS once, by 16-byte loads when every plane
 * of the tile is 16-byte aligned; TP = the largest of 256 / 128 / 64 with C·N·TP·sizeof(element) <= 160 KiB.
 * rti_photometric_stereo_plan returns TP, or 0 for the streaming form.
 * Not built: pixel-major stacks, fp64 stacks, a chunked (FitAccumulator) form (the window needs the samples),
 * a multi-GPU split.  (Per-pixel light directions: rti_photometric_stereo_near, below.) */
int rti_ps_design(const float* lu, const float* lv, int n, double* A);
int rti_photometric_stereo_plan(int N, int in_dtype, int C, int iters, int kernel);
int rti_photometric_stereo(const double* A, int N, const void* I, int in_dtype, int64_t P, int C,
                           int64_t light_stride, int64_t channel_stride,
                           float lo, float hi, int min_lights, int iters, float delta,
                           const float* w, float* normals, int normal_layout, float* albedo,
                           uint8_t* kind, float* res, int32_t* kept, int* fallback_px,
                           int kernel, rti_stream_t stream);

/* ---- device: near-light photometric stereo (rti_ps_near.hip) ------------------------------
 * rti_photometric_stereo for lights a few image widths from the object (the reference's phone flash): the
 * direction to a light and, by the inverse square of the distance, its strength differ from pixel to pixel, so
 * every pixel has its own design row per light, formed from the light's position and the pixel's, as
 * compute_intensities / rti_light_dirs form cam_n − (x0+x, y0+y, 0).
 *
 * The fit, the tail (normal, albedo, kind 0 / 1 / 2 / 4), the outputs and their layouts, the argument checks
 * and the streaming and LDS-resident forms with their plan rule are rti_photometric_stereo's, word for word;
 * only the row a_n of light n differs.  For pixel p = y·W + x (x the column), in fp64:
 *   pos   = (x0 + x, y0 + y, z_offset + h),  h = height[p] if height is given and that value is finite, else 0
 *   d     = L_n − pos                                    (L_n = lights[n][0..2], one rounding per component)
 *   s     = fma(d_x, d_x, fma(d_y, d_y, d_z·d_z))        (= r²)
 *   y     = 1/√s to within 1 ulp (the fp64 reciprocal-square-root seed and two Newton steps,
 *           y ← fma(y, fma(−(½s·y), y, ½), y))
 *   falloff == 0:  f = s_n·y                 a_n = f·d   (= s_n·d/r: direction only)
 *   falloff == 1:  f = ((s_n·y)·r0²)·(y·y)   a_n = f·d   (= s_n·(r0²/r²)·d/r: inverse square)
 * s_n = lights[n][3] is the light's scale and r0 a reference distance (r0² is rounded once on the host), so a
 * light of scale 1 at distance r0 has strength 1 and the albedo stays in intensity units.  Each component of
 * a_n is within 6·2⁻⁵³ (falloff 0) or 16·2⁻⁵³ (falloff 1: 8 ulps) relative of the expression on the right
 * evaluated exactly from the fp64 d: 3·2⁻⁵³ from s, 2·2⁻⁵³ from y, and one rounding per product.
 * s == 0 (a light on the pixel) or a non-finite light gives y = NaN and a NaN row; the pixel then fails both
 * solves of the fit like any singular system and ends as kind 4 (NaN normal and albedo, kept = N, counted in
 * fallback_px); no branch skips its work.  The rows are formed anew in every pass (window, fallback, each Huber
 * pass, the residual pass) by one device function, so every pass and both forms see the same bits; none is
 * stored.  height_from_normals gives a zero-mean height: z_offset is the gauge and the caller's.
 * lights: device fp64 [N][4] = x, y, z, scale, in the frame of rti_light_dirs' cams (pixel units).  height:
 * device fp32 [H·W] or NULL.  I, in_dtype, C, the strides and every argument from lo on as
 * rti_photometric_stereo, with P = H·W.
 * Every argument check answers before any HIP call.  RTI_ERR_BAD_ARG, besides rti_photometric_stereo's cases
 * (null lights in place of null A): H or W < 1, or H·W >= 2^31; falloff outside {0, 1}; r0 not finite or <= 0
 * with falloff == 1 (it is not read otherwise); a non-finite x0, y0 or z_offset.
 * rti_photometric_stereo_near_plan is rti_photometric_stereo_plan's rule.
 * Not built: anisotropic (cos^μ) sources, perspective cameras, a per-component height gauge, pixel-major or
 * fp64 stacks, a multi-GPU split. */
int rti_photometric_stereo_near_plan(int N, int in_dtype, int C, int iters, int kernel);
int rti_photometric_stereo_near(const double* lights, int N, const void* I, int in_dtype, int H, int W, int C,
                                int64_t light_stride, int64_t channel_stride, double x0, double y0,
                                const float* height, double z_offset, int falloff, double r0,
                                float lo, float hi, int min_lights, int iters, float delta,
                                const float* w, float* normals, int normal_layout, float* albedo,
                                uint8_t* kind, float* res, int32_t* kept, int* fallback_px,
                                int kernel, rti_stream_t stream);

/* ---- device: the shared fit fed in chunks of light planes (rti_fit_accum.hip) -----------
 * rti_fit_shared_residual's per-pixel sums kept in HBM between calls, for stacks that do not fit beside
 * their outputs and for frames that arrive over time (analysis.py produces one intensity plane and one
 * light direction per video frame).  Light n's contribution depends on light n alone, so planes can be
 * fed any number at a time and a fit read out after any of them.
 * state: device fp64, planar: element (c, j, p) at c*state_channel_stride + j*P + p
 * (state_channel_stride 0 = (k+1)*P); planes j < k hold y_j = Σ_n R[n][j]·I[c][n][p], plane k holds
 * q = Σ_n I[c][n][p]².  rti_fit_accum_state_doubles = C*(k+1)*P, the doubles a dense state holds, or -1
 * for k outside {6, 9, 16}, P < 1 or C outside [1, 65535].
 *
 * rti_fit_accumulate adds one chunk of B >= 1 light planes (B = 1: a live frame).
 *   R: device fp64 [B][k], the rows of THIS chunk's lights: rows of the design matrix A
 *      (rti_design_matrix), or rows of U (rti_lsq_factors) when every direction is known in advance.
 *   I: the chunk [C][B][P], light-major, F32 / U8 / I32; element (c, n, p) at
 *      c*channel_stride + n*light_stride + p (light_stride 0 = P, channel_stride 0 = B*light_stride).
 *   Per channel and pixel, for n = 0..B-1 in that order: x = (double)I[c][n][p],
 *      y_j = fma(R[n][j], x, y_j) for each j, q = fma(x, x, q) -- one accumulator per (pixel, j), so the
 *      state after N lights is bit-identical for every split of the N lights into chunks.
 *   init != 0: the state is taken as zero and overwritten (it is not read; the caller need not zero it).
 *   init == 0: the chunk is added to the state.
 *   B*sizeof(element) + 8(k+1) (read; not with init) + 8(k+1) (write) bytes per pixel.
 *
 * rti_fit_accum_solve reads the state, leaves it unchanged (a preview after any chunk; accumulation can
 * go on afterwards) and finishes the fit as rti_fit_shared_residual does:
 *   M: device fp64 [k][k].  orth == 0: M = ginv (rti_gram_inverse) over ALL directions accumulated so
 *      far, the state built from rows of A.  orth != 0: M = W (rti_lsq_factors), the state built from ALL
 *      N rows of U (a prefix of U's rows is not an orthonormal basis: no preview in this form).
 *   c_i = Σ_l M[i][l]·y_l (fma, l ascending from 0.0);  ss = q − Σ_i (orth ? y_i : c_i)·y_i;
 *   ss < 0 -> 0, NaN passes;  res[c][p] = sqrt(ss / n_lights), fp32 [C][P], may be NULL;
 *   coef: fp32, coef_layout / coef_channel_stride as rti_fit_shared.  n_lights: the lights accumulated.
 *   8(k+1) bytes in and 4k + 4 out per pixel.
 *
 * Both: k ∈ {6, 9, 16} and F32 / U8 / I32 input, else RTI_ERR_UNSUPPORTED.  RTI_ERR_BAD_ARG: null
 * R / I / state / M / coef; B, P, C or n_lights < 1; C > 65535; light_stride < P; with C > 1 a channel
 * stride (input, state or coef) below its dense value; a bad coef_layout.  The vector path (16-byte
 * loads) needs P and the strides multiples of 4 and 16-byte aligned bases; anything else runs one pixel
 * per lane with the same arithmetic and bits. */
int64_t rti_fit_accum_state_doubles(int k, int64_t P, int C);
int rti_fit_accumulate(const double* R, int k, int B,
                       const void* I, int in_dtype, int64_t P, int C,
                       int64_t light_stride, int64_t channel_stride,
                       double* state, int64_t state_channel_stride,
                       int init, rti_stream_t stream);
int rti_fit_accum_solve(const double* M, int k, int orth, int64_t n_lights,
                        const double* state, int64_t P, int C, int64_t state_channel_stride,
                        float* coef, int coef_layout, int64_t coef_channel_stride,
                        float* res, rti_stream_t stream);

/* ---- device: per-pixel PTM fit, light vectors generated in-kernel ------------------
 * Fuses compute_intensities' light vectors (analysis.py:221-231) into the
 * per-pixel PTM solve (analysis.py:280-298): for pixel (x, y) of an H×W stack
 * and camera n, l = (cam_n − (x0+x, y0+y, 0)) / ‖·‖ (fp64, rounded to fp32 as
 * the reference stores lx/ly in float32), then the 6×6 normal equations are
 * accumulated and solved in fp64 (Cholesky).  cams: device fp64 [N][3].
 * I: device light-major [N][light_stride] (0 = H*W), dtype F32/U8/I32.
 * coef: device, coef_dtype F32 or F64, layout coef_layout.
 * rcond < 0: reference semantics (exactly singular → NaN coefficients);
 * rcond >= 0: pivots <= rcond²·max_pivot are treated as singular → NaN. */
int rti_fit_perpixel_cam(const double* cams, int N,
                         const void* I, int in_dtype, int H, int W, int64_t light_stride,
                         double x0, double y0, double rcond,
                         void* coef, int coef_dtype, int coef_layout, rti_stream_t stream);

/* ---- device: per-pixel PTM fit from explicit per-pixel light vectors ---------------
 * The exact input of interpolate_intensities (analysis.py:321-363): lu, lv
 * (fp32) and I (F32/U8/I32), each PIXEL-major [P][N] as compute_intensities
 * returns them (analysis.py:217-219).  Same solve and output as above. */
int rti_fit_perpixel_dirs(const float* lu, const float* lv, const void* I, int in_dtype,
                          int N, int64_t P, double rcond,
                          void* coef, int coef_dtype, int coef_layout, rti_stream_t stream);

/* ---- host: light operators for a SHARED light set ---------------------------------
 * A light operator maps the N intensities of a pixel to E outputs: out_e = Σ_n M[e][n] I_n.
 * Both builders return it LIGHT-MAJOR, opT[n][e] (row stride E), fp64, ready for
 * rti_apply_operator after a cast to fp32.
 * rti_rbf_operator: the reference's default interpolator, SciPy Rbf(lu, lv, I,
 *   function='linear') evaluated at (qu_e, qv_e) (analysis.py:249-260):
 *   A_ij = ‖x_i − x_j‖, Φ_ej = ‖q_e − x_j‖, M = Φ A⁻¹ (LU with partial pivoting, fp64).
 *   Returns RTI_ERR_SINGULAR for a singular A (e.g. duplicate light directions), where
 *   SciPy raises LinAlgError.
 * rti_basis_operator: M = B(q) · pinv for PTM/HSH — the fit and the grid evaluation
 *   (analysis.py:293-315) fused into one operator (rcond as in rti_pinv). */
int rti_rbf_operator(const float* lu, const float* lv, int n, const double* qu, const double* qv, int E,
                     double* opT);
int rti_basis_operator(int basis, const float* lu, const float* lv, int n, const double* qu, const double* qv,
                       int E, double rcond, double* opT);

/* ---- device: apply a light operator (MFMA) -------------------------------------------
 * out[c][e][p] = Σ_n opT[n][e] · I[c][n][p]   (v_mfma_f32_16x16x4_f32, fp32 accumulate)
 * opT: device fp32 [N][op_stride] (op_stride >= E).  I as in rti_fit_shared.
 * out: device, out_dtype F32 / F64 / I32 (C truncation, NaN → INT32_MIN) / U8 (clipped),
 * element (c, e, p) at c*out_channel_stride + e*out_row_stride + p (0 = dense).
 * With the RBF operator on the 100×100 grid this is interpolate_intensities +
 * prepare_images_data for the reference's default method in one pass. */
int rti_apply_operator(const float* opT, int E, int N, int64_t op_stride,
                       const void* I, int in_dtype, int64_t P, int C,
                       int64_t light_stride, int64_t channel_stride,
                       void* out, int out_dtype, int64_t out_row_stride, int64_t out_channel_stride,
                       rti_stream_t stream);

/* ---- split-fp16 operator (v_mfma_f32_32x32x16_f16) -----------------------------------
 * The same product as rti_apply_operator at the fp16 MFMA rate: the host splits the fp64
 * operator into two fp16 halves, M·s = hi + lo (s = power of two, max|M·s| < 2^15;
 * inv_scale = 1/s), row-major [E][Kp] with Kp = N rounded up to 16 (16 <= Kp <= 256) and
 * zero padding; the device stages each 128-pixel tile of I as fp16 (a per-tile power-of-two
 * scale for values >= 2^15, plus fp16 remainders when the data is not exact in fp16) and
 * accumulates hi·I + lo·I (+ hi·I_lo) in fp32.  8-bit intensities are exact.
 * Accuracy: operator carried to 22 significant bits, fp32 accumulation (as the fp32 path).
 * op_hi / op_lo: device, 16-byte aligned.  Other arguments as rti_apply_operator. */
int rti_operator_split_f16(const double* opT, int N, int E, int64_t op_stride, int Kp,
                           uint16_t* hi, uint16_t* lo, float* inv_scale);
int rti_apply_operator_f16(const uint16_t* op_hi, const uint16_t* op_lo, int Kp, float inv_scale,
                           int E, int N, const void* I, int in_dtype, int64_t P, int C,
                           int64_t light_stride, int64_t channel_stride,
                           void* out, int out_dtype, int64_t out_row_stride, int64_t out_channel_stride,
                           rti_stream_t stream);

/* ---- device: per-pixel linear RBF (the reference's default, with its own geometry) ---
 * interpolate_intensities (analysis.py:350-363) -> _interpolate_RBF (analysis.py:249-260)
 * for every pixel: nodes x_n = (lu[p][n], lv[p][n]) and values I[p][n], PIXEL-major as
 * compute_intensities returns them; A_ij = ‖x_i − x_j‖, A w = I solved to fp64 accuracy (what
 * SciPy's LU with partial pivoting returns, to rounding: fp64 Gauss-Jordan for N <= 80, an fp32
 * Gauss-Jordan inverse + fp64 iterative refinement to 128 with an fp64 partial-pivoting fallback
 * for ill-conditioned pixels, and a blocked fp64 Cholesky of the bordered system above 128: (r06) left-looking
 * on the fp64 matrix cores to N = 1022 (two pixels per CU to 641), right-looking above),
 * f(q_e) = Σ_n w_n ‖q_e − x_n‖
 * evaluated in fp64 at luv[E][2] (device).
 * out: F64 / F32 / I32 / U8, layout RTI_OUT_PIXEL_MAJOR ([p][e], the reference's
 * [y][x][ly][lx]) or RTI_OUT_EVAL_MAJOR ([e][p], prepare_images_data's [ly][lx][y][x]).
 * status: device int the caller zeroes; set to RTI_ERR_SINGULAR when a pixel's system is
 * singular (that pixel's outputs are NaN), where SciPy raises LinAlgError.  N <= 32768 (RTI_ERR_UNSUPPORTED
 * above): above 1022 the right-looking Cholesky's panels narrow from 16 columns to 1 at N <= 4089 (the panel in
 * LDS), and above 4089 only the 32×32 diagonal block stays in LDS while the panel is solved in place in the slot.
 * Device memory: the call allocates (stream-ordered, hipMallocAsync) and frees a workspace of
 * P·N·(8 + 8) bytes (weights + nodes) plus, for N > 128, one Cholesky slot of ≈ 4·(N+pad)² bytes (L as the matrix
 * cores' 16×4 tiles plus the 64×64 diagonal blocks' factors to N = 1022, then the packed lower triangle) per
 * workgroup on min(P, 2·CUs) workgroups to N = 641, min(P, CUs) above (≈ 0.23 GB at N = 400, 3.3 GB at N = 1800, 6.7 GB at N = 2556, 17 GB at
 * N = 4089 on 256 CUs; above 4089 as many slots as fit in min(48 GiB, 90 % of the device's free memory less the
 * weights and nodes), halved again while the allocation fails, at least one; the environment variable
 * RTI_RBF_GP_WS_BYTES lowers that budget), or, for the fp32 inverses' fallback above N = 138 (reached only
 * with the RTI_RBF_LLT_MIN_N / RTI_RBF_CHOL_OLD measurement switches), 8·N·(N+1) bytes per CU (below: in LDS),
 * plus a P + 1 int list of the fallback's pixels; RTI_ERR_HIP if it cannot. */
int rti_rbf_perpixel(const float* lu, const float* lv, const void* I, int in_dtype, int N, int64_t P,
                     const double* luv, int E, void* out, int out_dtype, int out_layout, int* status,
                     rti_stream_t stream);
/* The same, and fallback_px (NULL, or a device int the caller zeroes) receives the number of pixels the
 * fp32-inverse solvers (81 <= N <= 128) handed to the fp64 partial-pivoting fallback (ill-conditioned:
 * nearly repeated light directions). */
int rti_rbf_perpixel_ex(const float* lu, const float* lv, const void* I, int in_dtype, int N, int64_t P,
                        const double* luv, int E, void* out, int out_dtype, int out_layout, int* status,
                        int* fallback_px, rti_stream_t stream);
/* Cholesky workgroups (= workspace slots) of this thread's most recent rti_rbf_perpixel call (N > 128), 0 for
 * the other solvers.  For tests and timing tools; the results do not depend on it. */
int64_t rti_rbf_last_chol_grid(void);

/* ---- device: light vectors ---------------------------------------------------------
 * The light-vector half of compute_intensities (analysis.py:221-231) for an
 * H×W ROI and N cameras: lu[p][n], lv[p][n] (fp32, pixel-major, p = y*W + x),
 * l = (cam_n − (x0+x, y0+y, 0)) / ‖·‖ in fp64 rounded to fp32. */
int rti_light_dirs(const double* cams, int N, int H, int W, double x0, double y0,
                   float* lu, float* lv, rti_stream_t stream);

/* ---- device: relight evaluator -----------------------------------------------------
 * Replaces _interpolate_PTM's grid evaluation (analysis.py:300-315), the
 * prepare_images_data transpose/truncation (analysis.py:375-411) and the
 * relighting_event lookup + clip (interactive_relighting.py:25-36):
 *   out[e][p] (or out[p][e]) = Σ_i coef[p][i] · b_i(lu_e, lv_e)
 * coef: device, coef_dtype F32 or F64 (arithmetic is done in that type; the
 * F64 PTM path sums the six terms left to right without contraction, exactly
 * as analysis.py:307-312).  luv: device fp64 [E][2] (lu, lv).
 * out_dtype: F32 / F64 value; I32 = C truncation toward zero, NaN/overflow →
 * INT32_MIN (the int32 assignment of analysis.py:407 on x86); U8 = the I32
 * value clipped to [0, 255] (interactive_relighting.py:35-36). */
int rti_relight(const void* coef, int coef_dtype, int basis, int64_t P, int coef_layout,
                const double* luv, int E,
                void* out, int out_dtype, int out_layout, rti_stream_t stream);

/* ---- device: interactive relight frame ----------------------------------------------
 * Replaces relighting_event's per-event image work (interactive_relighting.py:31-38):
 * V = clip(value, 0, 255) (the in-place clip of :35-36), img[:, :, 2] = V (:37), then
 * cv2.cvtColor(img, COLOR_HSV2BGR) (:38) for 8-bit images (OpenCV >= 4.2 HSV2RGB_b,
 * hue range 180, restated in DESIGN.md §4.4).
 *   src_dtype I32: src is the int32 table image [P] the cursor selected
 *     (interpolation_results[int_ly][int_lx]); basis, coef_layout, lu, lv ignored.
 *   src_dtype F32/F64: src is the coefficient map [P][k] / [k][P] (coef_layout) and
 *     value = relight at (lu, lv) truncated to int32 exactly as rti_relight's I32 output.
 * hsv: device uint8 [P][3] (the ROI in HSV, get_ROI(..., hsv=True)); bgr: device uint8
 * [P][3] output, may not alias hsv. */
int rti_relight_frame(const void* src, int src_dtype, int basis, int coef_layout, int64_t P,
                      double lu, double lv, const uint8_t* hsv, uint8_t* bgr, rti_stream_t stream);

/* ---- device: PTM surface normals and enhanced relighting (rti_normals.hip) -------------
 * What a fitted PTM says about the surface, after Malzbender, Gelb and Wolters (2001); the reference
 * stops at the relit value, so these semantics are build-defined.  PTM-6 only:
 *   L(u, v) = a0·u² + a1·v² + a2·u·v + a3·u + a4·v + a5
 * (HSH has no closed-form maximum: any other basis returns RTI_ERR_UNSUPPORTED).
 * All per-pixel arithmetic is fp64 from the F32 / F64 coefficients, every product, sum, quotient and
 * square root rounded (no contraction), products and sums taken left to right as written, and the
 * result rounded once to the output type.  Per pixel:
 *   D = 4·a0·a1 − a2²,  S = a0² + a1² + ½·a2²
 *   a maximum exists when every coefficient is finite, D > 1e-6·S and a0 < 0; then
 *     u0 = (a2·a4 − 2·a1·a3)/D,  v0 = (a2·a3 − 2·a0·a4)/D,  r² = u0² + v0²
 *   kind 0  a maximum with r² <= 1:       n = (u0, v0, sqrt(1 − r²))
 *   kind 1  a maximum outside the disc:   n = (u0, v0, 0)/sqrt(r²), scaled radially onto the edge
 *   kind 2  no maximum:                   g = (a3, a4, max(a5, 0)), n = g/‖g‖, (0, 0, 1) when ‖g‖ = 0
 *                                         (the Lambertian reading of the linear terms)
 *   kind 4  a non-finite coefficient:     n and peak are NaN           (3 is not used)
 *   peak = L(n_x, n_y) with the unrounded fp64 normal, the six terms summed left to right as
 *   rti_relight's F64 path sums them: an albedo proxy.
 * rti_ptm_normals: coef as rti_relight (coef_layout [p][6] or [6][p]); normals: device fp32,
 * normal_layout [p][3] or [3][p]; kind: NULL or device uint8 [P]; peak: NULL or device fp32 [P].
 * 4·6 (or 8·6) bytes in and 12 (+ 1 + 4) out per pixel. */
#define RTI_NORMAL_PIXEL_MAJOR   0   /* normals[p][3] */
#define RTI_NORMAL_PLANAR        1   /* normals[3][p] */
int rti_ptm_normals(const void* coef, int coef_dtype, int basis, int coef_layout, int64_t P,
                    float* normals, int normal_layout,
                    uint8_t* kind /* NULL ok */, float* peak /* NULL ok */, rti_stream_t stream);

/* rti_relight_enhanced: one image out[P] at the light direction (lu, lv), computed from the coefficients
 * alone (the peak is recomputed per pixel, no normal map is read: the 4k + 4 = 28 bytes per pixel of a
 * one-direction rti_relight).  Pixels of kind 4 give NaN in both modes.
 *   RTI_ENHANCE_DIFFUSE_GAIN, gain g >= 0: for pixels with a maximum (kinds 0 and 1), about the
 *   UNPROJECTED stationary point (u0, v0):
 *     a0' = g·a0, a1' = g·a1, a2' = g·a2
 *     a3' = (1−g)·(2·a0·u0 + a2·v0) + a3
 *     a4' = (1−g)·(2·a1·v0 + a2·u0) + a4
 *     a5' = (1−g)·(a0·u0² + a1·v0² + a2·u0·v0) + (a3−a3')·u0 + (a4−a4')·v0 + a5
 *   out = L'(lu, lv): the curvature scaled by g, the location and the height of the peak kept.  Pixels
 *   of kind 2 give the plain L(lu, lv).  kd, ks and spec_exp are not used.
 *   RTI_ENHANCE_SPECULAR: lw = sqrt(max(0, 1 − lu² − lv²)), H = (lu, lv, lw + 1)/‖·‖ (formed once on the
 *   host in fp64), out = kd·L(lu, lv) + ks·max(0, n·H)^spec_exp with n the normal above and spec_exp an
 *   integer in [1, 255] raised by repeated squaring (r = 1, b = x; for each bit of spec_exp from the
 *   lowest: r = r·b if it is set, then b = b·b while higher bits remain).  gain is not used.
 * out_dtype: F32 value; I32 / U8 as rti_relight (C truncation, NaN / overflow -> INT32_MIN; U8 = that
 * clipped to [0, 255]).
 * Both entries: device pointers, stream-ordered, no allocation, no synchronisation.  Every argument
 * check answers before any HIP call.  RTI_ERR_BAD_ARG: null coef / normals / out; P < 1; an unknown
 * coefficient layout, normal layout or mode; non-finite lu, lv, gain, kd or ks; gain < 0; spec_exp
 * outside [1, 255] in specular mode.  RTI_ERR_UNSUPPORTED: a basis other than PTM-6, a coefficient
 * dtype other than F32 / F64, an output dtype other than F32 / I32 / U8.  The vector path (one lane =
 * 4 pixels) needs P % 4 == 0, coef 16-byte aligned and every output aligned to a lane's 4 elements;
 * anything else, and the last partial 256-pixel chunk, runs one pixel per lane with the same arithmetic
 * and bits. */
#define RTI_ENHANCE_DIFFUSE_GAIN 1
#define RTI_ENHANCE_SPECULAR     2
int rti_relight_enhanced(const void* coef, int coef_dtype, int basis, int coef_layout, int64_t P,
                         int mode, double gain, double kd, double ks, int spec_exp,
                         double lu, double lv, void* out, int out_dtype, rti_stream_t stream);

/* ---- device: unsharp masking of k-channel maps, shading from a normal map (rti_unsharp.hip) ----
 * The spatial operator of the classic RTI rendering modes (image, luminance, coefficient and normal unsharp
 * masking); the reference has none, so these semantics are build-defined.  Relighting is
 * linear in the coefficients, so the unsharp-masked coefficient map relights to the unsharp-masked image at
 * every light direction, before any integer conversion.
 * rti_gauss_radius (host): max(1, ceil(3·sigma)), or -1 for sigma not finite or <= 0.
 * rti_gauss_taps (host): taps[0..radius], fp64: e_d = exp(−d²/(2σ²)) for d = 0..radius,
 *   Z = e_0 + 2·Σ_{d>=1} e_d summed with d ascending, taps[d] = e_d/Z.  RTI_ERR_BAD_ARG: null taps, sigma not
 *   finite or <= 0, radius outside [1, RTI_UNSHARP_MAX_RADIUS].
 * rti_map_unsharp: src / dst: device fp32, dense, layout RTI_COEF_PIXEL_MAJOR ([y][x][c]) or RTI_COEF_PLANAR
 *   ([c][y][x]), channels in [1, 16].  radius 0 = rti_gauss_radius(sigma); the effective radius R must lie in
 *   [1, RTI_UNSHARP_MAX_RADIUS].  A pixel is valid (m = 1) when all of its channels are finite.  With
 *   w = taps and all arithmetic in fp64 (fma where written, every other operation rounded, no contraction):
 *     hnum_c[y][x] = Σ_{dx=−R..R ascending; 0<=x+dx<W; m[y][x+dx]} fma(w|dx|, v_c[y][x+dx], ·)
 *     hden[y][x]   = the same sum of w|dx|
 *     num_c[y][x]  = Σ_{dy=−R..R ascending; 0<=y+dy<H} fma(w|dy|, hnum_c[y+dy][x], ·)     den likewise from hden
 *     blur_c = num_c/den;   o_c = v_c + amount·(v_c − blur_c);   dst_c = (float)o_c
 *   A normalised convolution: taps outside the image and invalid pixels are left out of numerator and
 *   denominator alike (no border replication, NaN does not spread); den >= w0² > 0 at every valid pixel.
 *   An invalid pixel's channels are copied to dst unchanged, bit for bit.  amount = −1 is the plain blur,
 *   amount = 0 returns src.  renorm != 0 (channels == 3): a valid pixel writes o/‖o‖ with ‖o‖ in fp64 from
 *   the unrounded o (squares summed left to right), and (0, 0, 1) when ‖o‖ is 0 or not finite.  Every
 *   output's sums have a fixed order: the result does not depend on the tiling, the layout or the load path,
 *   to the bit.  One launch: a workgroup stages its 32×64 tile plus R pixels of halo per side into LDS with
 *   the mask, runs the horizontal pass LDS -> LDS in fp64 and the vertical pass into registers; no
 *   intermediate map goes to HBM.  16- (or 8-) byte loads need W % 4 == 0 and src 16-byte aligned (planar)
 *   or channels % 4 (% 2) == 0 and src 16- (8-) byte aligned (pixel-major); anything else loads one float at
 *   a time with the same arithmetic and bits.
 * rti_shade_normals: one image out[P] from a normal map (normal_layout as rti_ptm_normals) and an optional
 *   albedo map (fp32 [P], NULL = 1) at the light direction (lu, lv): lw = sqrt(max(0, 1 − lu² − lv²)),
 *   l = (lu, lv, lw), H = (lu, lv, lw + 1)/‖·‖, both formed on the host in fp64 exactly as
 *   rti_relight_enhanced forms them;
 *     out = kd·albedo·max(0, n·l) + ks·max(0, n·H)^spec_exp
 *   in fp64 without contraction, products and sums left to right, the power by rti_relight_enhanced's
 *   repeated squaring.  A pixel with a NaN normal component or a NaN albedo gives NaN.  out_dtype F32 / I32 /
 *   U8 converts as rti_relight does.  The vector path (one lane = 4 pixels) needs P % 4 == 0, normals and
 *   albedo 16-byte aligned and out aligned to a lane's 4 elements; anything else runs one pixel per lane
 *   with the same arithmetic and bits.
 * Both device entries: device pointers, stream-ordered, no allocation, no synchronisation; the taps travel as
 * kernel arguments, so the calls can be captured in a hipGraph.  Every argument check answers before any HIP
 * call.  RTI_ERR_BAD_ARG: null src / dst / normals / out; H, W or P < 1; H·W·channels >= 2^31; channels
 * outside [1, 16]; a bad layout; sigma not finite or <= 0; an effective radius outside [1, 32]; amount not
 * finite; renorm with channels != 3; src and dst ranges that overlap; non-finite kd, ks, lu or lv; spec_exp
 * outside [1, 255].  RTI_ERR_UNSUPPORTED: an out_dtype other than F32 / I32 / U8.
 * Not built: halo exchange between the row tiles of a multi-GPU map, fp64 maps, strided maps. */
#define RTI_UNSHARP_MAX_RADIUS 32
int rti_gauss_radius(double sigma);
int rti_gauss_taps(double sigma, int radius, double* taps);
int rti_map_unsharp(const float* src, int channels, int layout, int H, int W,
                    double sigma, int radius, double amount, int renorm,
                    float* dst, rti_stream_t stream);
int rti_shade_normals(const float* normals, int normal_layout, const float* albedo /* NULL = 1 */, int64_t P,
                      double kd, double ks, int spec_exp, double lu, double lv,
                      void* out, int out_dtype, rti_stream_t stream);

/* ---- device: LRGB PTMs, the colour form (rti_lrgb.hip) ------------------------------------------
 * Six luminance coefficients and one RGB colour per pixel, rendered as rgb · L(lu, lv): the form in which
 * Malzbender, Gelb and Wolters (2001) and every PTM viewer hold a colour object, and one of the two
 * uncompressed payloads of the .ptm format.  The reference fits one channel, so these semantics are
 * build-defined.  PTM-6 only: the entries take no basis argument, and the Python layer
 * answers any other basis with NotImplementedError (RTI_ERR_UNSUPPORTED's exception).
 * An LRGB map is fp32 with 9 channels (a0..a5, cR, cG, cB), [p][9] (RTI_COEF_PIXEL_MAJOR) or [9][p]
 * (RTI_COEF_PLANAR); the first six planes of a planar map are a dense PTM-6 map that rti_ptm_normals,
 * rti_relight_enhanced and rti_map_unsharp take as it is.
 * rti_lrgb_from_rgb: coef: device fp32, three PTM-6 maps as rti_fit_shared writes them with C = 3
 *   (coef_layout, coef_channel_stride in elements, 0 = dense = 6·P).  gram: HOST fp64 [6][6], AᵀA of the
 *   shared design; weights: HOST fp64 [3] or NULL = 1.0/3.0 each (not normalised by the library).  Both are
 *   read during the call and travel as kernel arguments, so the call can be captured in a hipGraph.  Per
 *   pixel, in fp64 from the fp32 inputs, no contraction, every product and sum rounded, each expression
 *   left to right as written (x_c = channel c's coefficients, r g b = x_0 x_1 x_2):
 *     a_j = w0·r_j + w1·g_j + w2·b_j                      j = 0..5
 *     t_i = G[i][0]·a_0 + G[i][1]·a_1 + … + G[i][5]·a_5
 *     d   = a_0·t_0 + … + a_5·t_5
 *     s_c = x_c,0·t_0 + … + x_c,5·t_5
 *   any of the 18 inputs not finite: all nine outputs NaN; else d finite and d > 0: chroma_c = s_c/d; else
 *   (a black pixel): chroma = (1, 1, 1).  Written: (float)a_j, (float)chroma_c.  chroma_c is the c that
 *   minimises Σ_n (I_c,n − c·A_n·a)² when coef_c is the least-squares fit of I_c (AᵀI_c = G·coef_c), and
 *   Σ_c w_c·chroma_c = 1 up to rounding whenever d > 0 (Σ_c w_c·s_c = a·t = d).
 *   72 bytes in and 36 out per pixel.
 * rti_relight_lrgb: luv: device fp64 [E][2] as rti_relight's; out[e][p][c], RGB interleaved.  Per pixel and
 *   direction L = the six terms (double)a_i · b_i(lu_e, lv_e) summed as rti_relight's F64 path sums them,
 *   channel c = (double)chroma_c · L converted once: F32 value; I32 / U8 as rti_relight (a NaN gives NaN,
 *   INT32_MIN, 0).  With chroma = 1 the F32 output equals rti_relight's of the fp64 coefficients bit for
 *   bit.  The map is read once for all E directions of a launch (the kernel loops over them): 36 bytes in
 *   and 3·sizeof(out) per direction out per pixel.
 * Both entries: device pointers but gram / weights, stream-ordered, no allocation, no synchronisation.
 * Every argument check answers before any HIP call.  RTI_ERR_BAD_ARG: a null pointer other than weights;
 * P < 1 (or E < 1); a bad layout; a channel stride below its dense value; a non-finite gram entry; a weight
 * that is negative or not finite; weights that are all zero.  RTI_ERR_UNSUPPORTED: an out_dtype other than
 * F32 / I32 / U8.  The vector path (one lane = 4 pixels) needs P % 4 == 0, the maps 16-byte aligned with a
 * channel stride that is a multiple of 4, and out 16-byte (U8: 4-byte) aligned; anything else, and the last
 * partial 256-pixel chunk, runs one pixel per lane with the same arithmetic and bits. */
int rti_lrgb_from_rgb(const float* coef, int coef_layout, int64_t coef_channel_stride, int64_t P,
                      const double* gram, const double* weights /* NULL = 1/3 each */,
                      float* lrgb, int lrgb_layout, rti_stream_t stream);
int rti_relight_lrgb(const float* lrgb, int lrgb_layout, int64_t P, const double* luv, int E,
                     void* out, int out_dtype, rti_stream_t stream);

/* ---- device: 8-bit LRGB PTMs, the .ptm payload (rti_lrgb8.hip) ----------------------------------
 * A quantised LRGB map ("LRGB8") is the two blocks of a PTM_FORMAT_LRGB payload and its header values:
 *   coef8:   uint8 [p][6], the bytes a0..a5 of every pixel;   rgb8: uint8 [p][3];
 *   qparams: device fp64 [13]: scale[0..5], bias[0..5] (integral values), s (the chroma scale).
 * Rows top first, as every map of the project (a file stores them bottom first: the flip is the host's).
 * The arithmetic is that of rti/io.py (write_ptm, _ptm_quantise, read_ptm), in fp64
 * from the fp32 map, no contraction, each expression left to right as written.
 * rti_lrgb_qparams_workspace: bytes of device scratch rti_lrgb_qparams needs for P pixels (0 for P < 1);
 *   monotone in P and at most 39936.
 * rti_lrgb_qparams: lrgb: an fp32 LRGB map, [p][9] or [9][p] (lrgb_layout).  One pass finds, over the finite
 *   values, cmax = the largest of the three chroma planes and lo_j, hi_j of luminance plane j; then
 *     s       = cmax if there is a finite chroma value and cmax > 0, else 1
 *     LO_j    = (double)lo_j·s, HI_j = (double)hi_j·s
 *     scale_j = (HI_j − LO_j)/255.0 if plane j has a finite value and HI_j > LO_j, else 1
 *     bias_j  = clip(rint(−LO_j/scale_j), 0, 255) if plane j has a finite value, else 0
 *   (min and max are order-independent, so the result does not depend on the reduction tree; no atomics).
 *   workspace: 4-byte aligned, need not be initialised: the entry reads only what it wrote.  Two launches.
 *   36 bytes in per pixel.
 * rti_lrgb_quantise: per pixel, x = (double)a_j·s, raw_j = clip(rint(x/scale_j + bias_j), 0, 255), a NaN a_j
 *   writes bias_j, ±inf saturates; colour byte c = clip(rint(255.0·(double)chroma_c/s), 0, 255), a NaN writes
 *   0.  36 bytes in and 9 out per pixel.
 * rti_relight_lrgb8: reads scale and bias of qparams (not s).  Per pixel
 *     a_j = (float)(((double)raw_j − bias_j)·scale_j),  chroma_c = (float)((double)byte_c/255.0)
 *   -- the fp32 map read_ptm builds -- and then L, the three channels, their conversion and out[e][p][c] exactly
 *   as rti_relight_lrgb, so the image equals rti_relight_lrgb's of that map bit for bit.  The 9 bytes are read
 *   once for all E directions: 9 bytes in and 3·sizeof(out) per direction out per pixel.
 * All: device pointers, stream-ordered, no allocation, no synchronisation, capturable in a hipGraph.  Every
 * argument check answers before any HIP call.  RTI_ERR_BAD_ARG: a null pointer; P < 1 (or E < 1); a bad
 * layout; a misaligned workspace (4) or qparams (8).  RTI_ERR_UNSUPPORTED: an out_dtype other than F32 / I32 /
 * U8.  The vector path (one lane = 4 pixels, the byte blocks as whole dwords) needs P % 4 == 0, the fp32 map
 * 16-byte aligned, coef8 4-byte (rti_relight_lrgb8: 8-byte) and rgb8 4-byte aligned, and out aligned as
 * rti_relight_lrgb requires; anything else, and the last partial 256-pixel chunk, runs one pixel per lane with
 * the same arithmetic and bits. */
int64_t rti_lrgb_qparams_workspace(int64_t P);
int rti_lrgb_qparams(const float* lrgb, int lrgb_layout, int64_t P, void* workspace, double* qparams,
                     rti_stream_t stream);
int rti_lrgb_quantise(const float* lrgb, int lrgb_layout, int64_t P, const double* qparams,
                      uint8_t* coef8, uint8_t* rgb8, rti_stream_t stream);
int rti_relight_lrgb8(const uint8_t* coef8, const uint8_t* rgb8, int64_t P, const double* qparams,
                      const double* luv, int E, void* out, int out_dtype, rti_stream_t stream);

/* ---- device: 8-bit RGB HSH maps, the .rti payload (rti_hsh8.hip) ---------------------------------
 * A quantised RGB HSH map ("HSH8") is the payload of an HSH .rti file and its header values:
 *   coef8:   uint8 [p][3][k]: pixel, then channel (R, G, B), then term;
 *   qparams: device fp32 [2k]: scale[0..k-1], then bias[0..k-1], shared by the three channels and equal to
 *            the file header's values bit for bit.
 * k = 9 (RTI_BASIS_HSH9) or 16 (RTI_BASIS_HSH16); term j is column j of rti_basis_eval.  Rows top first, as
 * every map of the project.  The arithmetic is build-defined.  Every operation below is
 * rounded, nothing is contracted, each expression is evaluated left to right as written:
 *   step_j = scale_j / 255.0f               one correctly rounded fp32 division per term, formed once per
 *                                           workgroup, never per pixel
 *   c_j    = (float)raw_j * step_j + bias_j  the fp32 map read_rti builds: a byte -> fp32 conversion, an fp32
 *                                           multiply and an fp32 add, no FMA
 * rti_hsh_qparams_workspace: bytes of device scratch rti_hsh_qparams needs for k terms and P pixels; 0 for
 *   P < 1 or a k other than 9 / 16; monotone in P and at most 768·2k·4 (98304 for k = 16).
 * rti_hsh_qparams: coef: device fp32, three HSH maps as rti_fit_shared writes them with C = 3: [c][p][k]
 *   (RTI_COEF_PIXEL_MAJOR) or [c][k][p] (RTI_COEF_PLANAR), coef_channel_stride in elements, 0 = dense = k·P.
 *   One pass finds lo_j and hi_j, the smallest and largest finite value of term j in the three channels
 *   (exact fp32 values; min and max are order-independent, so the result does not depend on the reduction
 *   tree; no atomics); then
 *     bias_j  = lo_j (a zero of either sign is written as +0) if term j has a finite value, else 0
 *     scale_j = hi_j − lo_j in fp32 if term j has a finite value and that difference is finite and > 0, else 1
 *   workspace: 4-byte aligned, need not be initialised: the entry reads only what it wrote.  Two launches.
 *   12k bytes in per pixel.
 * rti_hsh_quantise: raw = clip(rint(((double)x − (double)bias_j) / (double)step_j), 0, 255); a NaN writes 0,
 *   ±inf saturates.  fp64: the quantiser runs once per object.  12k bytes in and 3k out per pixel.
 * rti_relight_hsh8: per pixel, channel and direction, rti_relight's F32 path applied to c_0..c_{k-1}: the
 *   same basis_eval<float> of ((float)lu, (float)lv), the same chain of k fused multiply-adds, converted once
 *   (F32; I32 / U8 as rti_relight).  out[e][p][c], RGB interleaved like rti_relight_lrgb's.  The image equals
 *   rti_relight's of the dequantised map of channel c bit for bit.  The bytes are read once for all E
 *   directions of a launch: 3k bytes in and 3·sizeof(out) per direction out per pixel.
 * All: device pointers, stream-ordered, no allocation, no synchronisation, capturable in a hipGraph.  Every
 * argument check answers before any HIP call.  RTI_ERR_BAD_ARG: a null pointer; P < 1 (or E < 1); a bad
 * layout; a channel stride below dense; a misaligned workspace or qparams (4 bytes).  RTI_ERR_UNSUPPORTED: a
 * basis other than HSH-9 / HSH-16; an out_dtype other than F32 / I32 / U8.
 * Every kernel runs one pixel per lane, 64 consecutive pixels per wave.  The fast paths move a full wave's
 * contiguous run as whole 16-byte (output images: 4-byte) pieces through LDS and need:
 *   the fp32 maps, pixel-major:  coef 16-byte aligned and a channel stride that is a multiple of 4
 *                                (planar maps are read per lane, coalesced as they are);
 *   coef8 (read or written):     16-byte aligned;
 *   out:                         4-byte aligned, and for U8 also P % 4 == 0.
 * Anything else, and the last partial wave of any launch, loads and stores per lane through the same
 * per-pixel arithmetic and gives the same bits. */
int64_t rti_hsh_qparams_workspace(int k, int64_t P);
int rti_hsh_qparams(const float* coef, int basis, int coef_layout, int64_t coef_channel_stride, int64_t P,
                    void* workspace, float* qparams, rti_stream_t stream);
int rti_hsh_quantise(const float* coef, int basis, int coef_layout, int64_t coef_channel_stride, int64_t P,
                     const float* qparams, uint8_t* coef8, rti_stream_t stream);
int rti_relight_hsh8(const uint8_t* coef8, int basis, int64_t P, const float* qparams,
                     const double* luv, int E, void* out, int out_dtype, rti_stream_t stream);

/* ---- device: HSH surface normals, a peak-direction search (rti_hsh_normals.hip) -------------------
 * What a fitted HSH map says about the surface: the light direction at which the fitted function peaks, the
 * analogue of rti_ptm_normals for a basis without a closed-form maximum.  It is found by evaluating the function
 * on a grid of directions and one parabolic step; the semantics are build-defined.  Every
 * expression below is evaluated left to right as written, every operation rounded, nothing contracted except
 * the fused multiply-adds named.
 *   luminance map   one map (C = 1): l_j = c_j.  Three maps (C = 3): l_j = (wR·r_j + wG·g_j) + wB·b_j in fp32,
 *                   two products and two sums.  w: three fp32 weights on the HOST, NULL = (0.299f, 0.587f,
 *                   0.114f).  For the 8-bit map r_j, g_j, b_j are the dequantised c_j = (float)raw_j·step_j +
 *                   bias_j of rti_hsh8.hip above.
 *   grid            G = grid in [4, 16].  The points are the integer pairs (i, j), −G <= i, j <= G, with
 *                   i² + j² <= G² (this integer test is the mask), numbered e = 0..E−1 with j ascending, then
 *                   i ascending; point e lies at (u, v) = ((double)i/(double)G, (double)j/(double)G).
 *   value           V_e = rti_relight's F32 value of the luminance map at (u, v), bit for bit: the same
 *                   basis_eval<float> of ((float)u, (float)v) and the same chain acc = l_0·b_0,
 *                   acc = fmaf(l_j, b_j, acc) for j = 1..k−1.
 *   peak            e* = the point with the largest V, the smallest e among equals; V0 = V_e*.
 *   refinement      in fp64 from the fp32 values.  Along u, with Vm, Vp the values at (i−1, j) and (i+1, j): if
 *                   both points lie inside the mask and d = (Vm − 2·V0) + Vp < 0, then
 *                   δu = min(max(0.5·(Vm − Vp)/d, −0.5), 0.5), otherwise δu = 0; δv likewise along j.
 *                   u0 = ((double)i + δu)/(double)G, v0 likewise, r² = u0·u0 + v0·v0.
 *   kind 0  r² <= 1:                     n = (u0, v0, sqrt(1 − r²))
 *   kind 1  r² > 1:                      n = (u0/sqrt(r²), v0/sqrt(r²), 0)
 *   kind 2  the largest and the smallest V of the grid are equal (a flat function, e.g. an all-zero pixel):
 *                                        n = (0, 0, 1)
 *   kind 4  an l_j that is not finite:   n and peak are NaN              (3 is not used: rti_ptm_normals' numbers)
 *   peak = V0, the fp32 grid maximum (an albedo proxy, as the PTM peak is); normals are rounded once to fp32.
 * rti_peak_grid_points: E for a grid, or -1 outside [4, 16] (49 at G = 4, 317 at G = 10, 797 at G = 16).
 * rti_peak_table_bytes: the size of the table of (basis, grid); 0 for a basis other than HSH-9 / HSH-16 or a grid
 *   outside [4, 16].
 * rti_peak_table: fills `table` (device, 16-byte aligned, rti_peak_table_bytes long) with the basis values of the
 *   E grid points, formed by the device basis_eval<float> that rti_relight runs.  The buffer is opaque; one table
 *   serves any number of maps of that (basis, grid).  One launch.
 * rti_hsh_normals: coef: device fp32, C = 1 or 3 maps as rti_fit_shared writes them: [c][p][k]
 *   (RTI_COEF_PIXEL_MAJOR) or [c][k][p] (RTI_COEF_PLANAR), coef_channel_stride in elements, 0 = dense = k·P (one
 *   map never uses it).  4·C·k bytes in and 12 (+ 1 + 4) out per pixel; P·E·k fused multiply-adds.
 * rti_hsh8_normals: coef8 / qparams as rti_relight_hsh8 takes them.  3k bytes in per pixel.
 * Both: normals: device fp32, normal_layout [p][3] or [3][p]; kind: NULL or device uint8 [P]; peak: NULL or
 *   device fp32 [P], as rti_ptm_normals.  The result of rti_hsh8_normals equals rti_hsh_normals' of the
 *   dequantised maps bit for bit.
 * All: device pointers, stream-ordered, no allocation, no synchronisation, capturable in a hipGraph; one launch.
 * Every argument check answers before any HIP call.  RTI_ERR_BAD_ARG: a null pointer (kind, peak and w may be
 * null); P < 1; C other than 1 or 3; a channel stride below dense (C = 3); a bad coefficient or normal layout; a
 * grid outside [4, 16]; a non-finite weight; a table off 16 bytes or qparams off 4.  RTI_ERR_UNSUPPORTED: a basis
 * other than HSH-9 / HSH-16 (PTM-6 has rti_ptm_normals).
 * A lane owns two pixels, a wave two runs of 64 consecutive pixels.  The fast loads move a full run as whole
 * 16-byte pieces through LDS and need: pixel-major fp32 maps 16-byte aligned with (C = 3) a channel stride that is
 * a multiple of 4; coef8 16-byte aligned.  Planar maps are read per lane, coalesced as they are.  Anything else,
 * and the last partial run, loads and stores per lane through the same per-pixel arithmetic and gives the same
 * bits. */
int     rti_peak_grid_points(int grid);
int64_t rti_peak_table_bytes(int basis, int grid);
int     rti_peak_table(int basis, int grid, void* table, rti_stream_t stream);
int     rti_hsh_normals(const float* coef, int basis, int coef_layout, int C, int64_t coef_channel_stride,
                        int64_t P, const float* w /* NULL ok */, int grid, const void* table,
                        float* normals, int normal_layout, uint8_t* kind /* NULL ok */, float* peak /* NULL ok */,
                        rti_stream_t stream);
int     rti_hsh8_normals(const uint8_t* coef8, int basis, int64_t P, const float* qparams, const float* w /* NULL ok */,
                         int grid, const void* table,
                         float* normals, int normal_layout, uint8_t* kind /* NULL ok */, float* peak /* NULL ok */,
                         rti_stream_t stream);

/* ---- device: 8-bit RGB PTMs, the PTM_FORMAT_RGB payload (rti_rgb8.hip) ---------------------------
 * A quantised RGB PTM ("RGB8") is the three coefficient blocks of a PTM_FORMAT_RGB payload and its header values:
 *   coef8:   uint8 [3][p][6]: block R, then G, then B, each the bytes a0..a5 of every pixel (18 bytes per pixel);
 *   qparams: device fp64 [12]: scale[0..5], bias[0..5] (integral values), shared by the three channels as the file
 *            header shares them.
 * Rows top first, as every map of the project (a file stores them bottom first: the flip is the host's).  The
 * arithmetic is that of rti/io.py (write_ptm(format="rgb"), _ptm_quantise, read_ptm): fp64 from the
 * fp32 inputs unless an fp32 operation is named, no contraction, each expression left to right as written.
 * rti_rgb8_qparams_workspace: bytes of device scratch rti_rgb8_qparams needs for P pixels (0 for P < 1); monotone
 *   in P and at most 36864 (12 floats for each of at most 768 workgroups).
 * rti_rgb8_qparams: coef: device fp32, three PTM-6 maps as rti_fit_shared writes them with C = 3: [c][p][6]
 *   (RTI_COEF_PIXEL_MAJOR) or [c][6][p] (RTI_COEF_PLANAR), coef_channel_stride in elements, 0 = dense = 6·P.  One
 *   pass finds lo_j and hi_j, the smallest and largest finite value of coefficient plane j over the three channels
 *   (exact fp32 values; min and max are order-independent, so the result does not depend on the reduction tree; no
 *   atomics); then
 *     scale_j = ((double)hi_j − (double)lo_j)/255.0 if plane j has a finite value and hi_j > lo_j, else 1
 *     bias_j  = clip(rint(−(double)lo_j/scale_j), 0, 255) if plane j has a finite value, else 0
 *   workspace: 4-byte aligned, need not be initialised: the entry reads only what it wrote.  Two launches.
 *   72 bytes in per pixel.
 * rti_rgb8_quantise: raw = clip(rint((double)x/scale_j + bias_j), 0, 255); a NaN writes bias_j, ±inf saturates.
 *   72 bytes in and 18 out per pixel.
 * rti_relight_rgb8: a_cj = (float)(((double)raw_cj − bias_j)·scale_j), the fp32 map read_ptm builds.  (A workgroup
 *   forms the 256 possible values of each plane once, in exactly this arithmetic, and a pixel looks its 18 up: the
 *   same fp32 values.)  Then per channel and direction rti_relight's F32 path: the same basis_eval<float> of
 *   ((float)lu, (float)lv) and the same chain acc = a_0·b_0, acc = fmaf(a_j, b_j, acc) for j = 1..5, converted once
 *   (F32; I32 / U8 as rti_relight).  out[e][p][c], RGB interleaved like rti_relight_lrgb's and rti_relight_hsh8's.
 *   Channel c of the image equals rti_relight's of dequantised map c bit for bit.  A NaN coefficient was stored as
 *   bias_j and renders as a finite 0 term: that is what the format does.  The bytes are read once for all E
 *   directions of a launch (the kernel loops over them): 18 bytes in and 3·sizeof(out) per direction out per pixel.
 * rti_rgb8_normals: luminance in fp32 on the dequantised values, l_j = (wR·r_j + wG·g_j) + wB·b_j: two products and
 *   two sums, each rounded, no FMA.  w: three fp32 weights on the HOST, NULL = (0.299f, 0.587f, 0.114f), as
 *   rti_hsh_normals takes them.  Then rti_ptm_normals' per-pixel function on the F32 coefficients l_0..l_5 (fp64
 *   from the fp32 values; kinds 0 / 1 / 2 / 4; peak): normals, kind and peak equal rti_ptm_normals' of that fp32
 *   luminance map bit for bit.  The 18 dequantised values of a pixel are finite whenever qparams is, so kind 4
 *   occurs only if the weighted sum itself overflows fp32: a map made by rti_rgb8_quantise or read from a file,
 *   with weights of ordinary size, never gives it.  normals: device fp32, normal_layout [p][3] or [3][p]; kind:
 *   NULL or device uint8 [P]; peak: NULL or device fp32 [P].  One launch; 18 bytes in and 12 (+ 1 + 4) out per
 *   pixel.
 * All: device pointers except w, stream-ordered, no allocation, no synchronisation, capturable in a hipGraph.
 * Every argument check answers before any HIP call.  RTI_ERR_BAD_ARG: a null pointer (kind, peak and w may be null);
 * P < 1 (or E < 1); a bad coefficient or normal layout; a channel stride below dense; a non-finite weight; a
 * workspace off 4 bytes; qparams off 8 bytes.  RTI_ERR_UNSUPPORTED: an out_dtype other than F32 / I32 / U8.
 * The vector path (one lane = 4 pixels; a lane's 24 bytes of a block as three 8-byte loads or six dword stores)
 * needs P % 4 == 0 (the three blocks are then 24·(P/4) bytes apart, so one alignment covers them), the fp32 maps
 * 16-byte aligned with a channel stride that is a multiple of 4, coef8 8-byte aligned, out aligned as
 * rti_relight_lrgb requires (16 bytes; U8: 4) and normals / kind / peak as rti_ptm_normals requires (16 / 4 / 16);
 * anything else, and the last partial 256-pixel chunk, runs one pixel per lane with the same arithmetic and bits.
 * Not built: planar or strided coef8.  (Diffuse gain and specular rendering from the bytes:
 * rti_relight_rgb8_enhanced, below; the fp32 maps themselves in one pass: rti_relight_rgb, below.) */
int64_t rti_rgb8_qparams_workspace(int64_t P);
int rti_rgb8_qparams(const float* coef, int coef_layout, int64_t coef_channel_stride, int64_t P,
                     void* workspace, double* qparams, rti_stream_t stream);
int rti_rgb8_quantise(const float* coef, int coef_layout, int64_t coef_channel_stride, int64_t P,
                      const double* qparams, uint8_t* coef8, rti_stream_t stream);
int rti_relight_rgb8(const uint8_t* coef8, int64_t P, const double* qparams,
                     const double* luv, int E, void* out, int out_dtype, rti_stream_t stream);
int rti_rgb8_normals(const uint8_t* coef8, int64_t P, const double* qparams, const float* w /* HOST, NULL ok */,
                     float* normals, int normal_layout, uint8_t* kind /* NULL ok */, float* peak /* NULL ok */,
                     rti_stream_t stream);

/* ---- device: diffuse gain and specular rendering of the colour forms (rti_enhance_px.h) ----------
 * rti_relight_enhanced's two modes for an fp32 LRGB map, the 9-byte LRGB payload and the 18-byte RGB payload: one
 * launch, one image out[p][3] (RGB interleaved like rti_relight_lrgb's) at the light direction (lu, lv).  mode, gain,
 * kd, ks, spec_exp, lu, lv and out_dtype are rti_relight_enhanced's; lrgb and lrgb_layout rti_relight_lrgb's; coef8,
 * rgb8 and qparams rti_relight_lrgb8's and rti_relight_rgb8's; w rti_rgb8_normals'.  The half vector H is formed once
 * on the host and everything travels as kernel arguments.
 * All per-pixel arithmetic is fp64 without contraction, each expression left to right as written, converted once
 * (F32; I32 / U8 as rti_relight).  With l a LUMINANCE coefficient vector (fp64 from fp32), (u0, v0), the kind and the
 * normal n those rti_ptm_normals states for l, and for any coefficient vector a:
 *   G(a) = L'(lu, lv) with a' the diffuse gain transform of a about l's (u0, v0) (the formulas of
 *          rti_relight_enhanced with a's coefficients and l's stationary point; a itself where l has no maximum).
 *          The transform keeps the value and the gradient of a at (u0, v0) and scales its second derivatives by g
 *          for ANY point, so every channel keeps its colour at the luminance's peak: no fringes.
 *   D(a) = L(lu, lv) of a, the six terms summed as rti_relight's F64 path sums them
 *   S    = max(0, n·H)^spec_exp, n·H = n_x·H_x + n_y·H_y + n_z·H_z, the power by repeated squaring
 * A pixel whose l is not finite (kind 4) is NaN in its three channels, in both modes.
 * rti_relight_lrgb_enhanced: l = a0..a5 of the pixel.
 *   diffuse gain: channel c = (double)chroma_c · G(l)
 *   specular:     channel c = kd · ((double)chroma_c · D(l)) + ks · S      (a white highlight on the coloured term)
 *   A NaN chroma gives NaN in its channel.  With chroma = 1 every F32 channel equals rti_relight_enhanced's output
 *   for the luminance planes bit for bit.  36 bytes in and 3·sizeof(out) out per pixel.
 * rti_relight_lrgb8_enhanced: a_j = (float)(((double)raw_j − bias_j)·scale_j), chroma_c = (float)((double)byte_c/255.0)
 *   as rti_relight_lrgb8 states them, then the LRGB function: the image equals rti_relight_lrgb_enhanced's of the
 *   dequantised map bit for bit.  (A workgroup forms the 256 possible values of each plane and of the chroma once,
 *   in exactly this arithmetic, and a pixel looks its 9 up.)  9 bytes in per pixel.
 * rti_relight_rgb8_enhanced: a_cj as rti_relight_rgb8 states them; l_j = (wR·r_j + wG·g_j) + wB·b_j in fp32 as
 *   rti_rgb8_normals forms it (w: three fp32 weights on the HOST, NULL = (0.299f, 0.587f, 0.114f)).
 *   diffuse gain: channel c = G(a_c)
 *   specular:     channel c = kd · D(a_c) + ks · S
 *   With weights (1,0,0), (0,1,0) or (0,0,1) the channel whose weight is 1 equals rti_relight_enhanced's output for
 *   that dequantised fp32 map bit for bit.  18 bytes in per pixel.
 * All: device pointers except w, stream-ordered, no allocation, no synchronisation, capturable in a hipGraph.
 * Every argument check answers before any HIP call.  RTI_ERR_BAD_ARG: a null pointer (w may be null); P < 1; a bad
 * layout or mode; non-finite lu, lv, gain, kd, ks or weight; gain < 0; spec_exp outside [1, 255] in specular mode;
 * qparams off 8 bytes.  RTI_ERR_UNSUPPORTED: an out_dtype other than F32 / I32 / U8.
 * The vector path (one lane = 4 pixels) applies under the conditions of the plain relight of each form
 * (rti_relight_lrgb, rti_relight_lrgb8, rti_relight_rgb8); anything else, and the last partial 256-pixel chunk, runs
 * one pixel per lane with the same arithmetic and bits.
 * Not built: E > 1 directions per launch, a multi-GPU wrapper, planar RGB output, HSH8 enhanced rendering,
 * rti_relight_lrgb8 itself in the table form.  (Three fp32 RGB maps: rti_relight_rgb_enhanced, below.) */
int rti_relight_lrgb_enhanced(const float* lrgb, int lrgb_layout, int64_t P,
                              int mode, double gain, double kd, double ks, int spec_exp, double lu, double lv,
                              void* out, int out_dtype, rti_stream_t stream);
int rti_relight_lrgb8_enhanced(const uint8_t* coef8, const uint8_t* rgb8, int64_t P, const double* qparams,
                               int mode, double gain, double kd, double ks, int spec_exp, double lu, double lv,
                               void* out, int out_dtype, rti_stream_t stream);
int rti_relight_rgb8_enhanced(const uint8_t* coef8, int64_t P, const double* qparams,
                              const float* w /* HOST, NULL ok */,
                              int mode, double gain, double kd, double ks, int spec_exp, double lu, double lv,
                              void* out, int out_dtype, rti_stream_t stream);

/* ---- device: three fp32 RGB maps rendered in one pass (rti_rgb.hip) -------------------------------
 * What rti_fit_shared writes for a colour stack (C = 3), rendered without a detour through 8 bits or LRGB:
 *   coef: device fp32, three maps of k terms: [c][p][k] (RTI_COEF_PIXEL_MAJOR) or [c][k][p] (RTI_COEF_PLANAR),
 *         coef_channel_stride in elements, 0 = dense = k·P.  Every offset is formed in 64 bits.
 * Outputs are RGB interleaved like rti_relight_rgb8's.
 * rti_relight_rgb: PTM-6, HSH-9 and HSH-16.  out[e][p][c]; luv: device fp64 [E][2].  Per channel and direction
 *   rti_relight's F32 path: the same basis_eval<float> of ((float)lu, (float)lv) and the same chain acc = a_0·b_0,
 *   acc = fmaf(a_j, b_j, acc) for j = 1..k−1, converted once (F32; I32 / U8 as rti_relight).  Channel c of the image
 *   equals rti_relight's of map c bit for bit.  The maps are read once for all E directions of a launch (the kernel
 *   loops over them): 12k bytes in and 3·sizeof(out) per direction out per pixel.
 * rti_relight_rgb_enhanced: PTM-6 only.  rti_relight_rgb8_enhanced's definition above with a_cj the fp32 map values
 *   instead of dequantised bytes: l_j = (wR·r_j + wG·g_j) + wB·b_j in fp32, two products and two sums, no FMA (w:
 *   three fp32 weights on the HOST, NULL = (0.299f, 0.587f, 0.114f)); the peak, the kind and the normal are those of
 *   l; diffuse gain: channel c = G(a_c); specular: channel c = kd · D(a_c) + ks · S; kind 4 gives NaN in three
 *   channels.  out[p][c].  The half vector is formed once on the host and everything travels as kernel arguments.
 *   With weights (1,0,0), (0,1,0) or (0,0,1) the channel whose weight is 1 equals rti_relight_enhanced's output for
 *   that map bit for bit; for maps that are dequantised bytes the image equals rti_relight_rgb8_enhanced's.  72 bytes
 *   in and 3·sizeof(out) out per pixel.
 * rti_rgb_normals: PTM-6 only.  rti_rgb8_normals on the fp32 maps: the same fp32 luminance, then rti_ptm_normals'
 *   per-pixel function: normals, kind and peak equal rti_ptm_normals' of that fp32 luminance map bit for bit.  A
 *   non-finite input value reaches kind 4 here (the bytes of an 8-bit map cannot hold one).  normals: device fp32,
 *   normal_layout [p][3] or [3][p]; kind: NULL or device uint8 [P]; peak: NULL or device fp32 [P].  72 bytes in and
 *   12 (+ 1 + 4) out per pixel.
 * All: device pointers except w, stream-ordered, no allocation, no synchronisation, capturable in a hipGraph; one
 * launch.  Every argument check answers before any HIP call.  RTI_ERR_BAD_ARG: a null pointer (w, kind and peak may
 * be null); P < 1 (or E < 1); an unknown basis (as rti_relight answers it); a bad coefficient or normal layout or
 * mode; a channel stride below dense (a negative one included); non-finite lu, lv, gain, kd, ks or weight; gain < 0;
 * spec_exp outside [1, 255] in specular mode.  RTI_ERR_UNSUPPORTED: an out_dtype other than F32 / I32 / U8.
 * PTM-6: the vector path (one lane = 4 pixels, a wave 256, a workgroup 1024; pixel-major rows as coalesced 16-byte
 * loads through LDS, planar planes as 16-byte loads) needs P % 4 == 0, coef 16-byte aligned with a channel stride
 * that is a multiple of 4, and out aligned as rti_relight_rgb8 requires (16 bytes; U8: 4) or normals / kind / peak as
 * rti_rgb8_normals requires (16 / 4 / 16); anything else, and the last partial 256-pixel chunk, runs one pixel per
 * lane with the same arithmetic and bits.
 * HSH-9 / HSH-16: a lane owns one pixel, a wave 64 and a workgroup 256, as rti_relight_hsh8 (three channels of four
 * pixels do not fit a lane's registers).  A full wave of a pixel-major map loads its 64 rows as 16-byte pieces
 * through LDS if coef is 16-byte aligned with a channel stride that is a multiple of 4, and stores its 192 output
 * elements as whole dwords if out is 4-byte aligned (U8: and P % 4 == 0); anything else loads and stores per lane,
 * with the same bits.  The basis rows of up to 64 directions at a time are kept in LDS.
 * Not built: fp64 RGB maps, planar RGB output, a multi-GPU wrapper.  (Several directions per launch of an enhanced
 * rendering, and diffuse gain for HSH maps: rti_relight_hsh_specular and rti_relight_hsh_gain, below.) */
int rti_relight_rgb(const float* coef, int basis, int coef_layout, int64_t coef_channel_stride, int64_t P,
                    const double* luv, int E, void* out, int out_dtype, rti_stream_t stream);
int rti_relight_rgb_enhanced(const float* coef, int coef_layout, int64_t coef_channel_stride, int64_t P,
                             const float* w /* HOST, NULL ok */,
                             int mode, double gain, double kd, double ks, int spec_exp, double lu, double lv,
                             void* out, int out_dtype, rti_stream_t stream);
int rti_rgb_normals(const float* coef, int coef_layout, int64_t coef_channel_stride, int64_t P,
                    const float* w /* HOST, NULL ok */, float* normals, int normal_layout,
                    uint8_t* kind /* NULL ok */, float* peak /* NULL ok */, rti_stream_t stream);

/* ---- device: specular enhancement of HSH maps under a normal map (rti_hsh_specular.hip) -----------
 * The specular mode of rti_relight_enhanced for the bases without a closed-form peak.  An HSH normal is a search
 * (rti_hsh_normals, once per object), so these entries read a normal map (rti_hsh_normals / rti_hsh8_normals, optionally
 * sharpened by rti_map_unsharp) instead of recomputing the normal per frame; the semantics are build-defined.  Per
 * pixel p, channel c and direction e, every operation rounded, each expression left to right as written:
 *   V_c  = rti_relight's F32 value of channel c's coefficients at (lu_e, lv_e), bit for bit: the same
 *          basis_eval<float> of ((float)lu, (float)lv) and the same chain acc = c_0·b_0, acc = fmaf(c_j, b_j, acc) for
 *          j = 1..k−1; for the 8-bit map c_j = (float)raw_j·step_j + bias_j as rti_relight_hsh8 states it
 *   h    = n_x·hx + n_y·hy + n_z·hz           fp64 from the fp32 normal; H = (hx, hy, hz) = (lu, lv, lw + 1)/‖·‖ with
 *                                             lw = sqrt(max(0, 1 − lu² − lv²)), formed on the HOST in fp64 exactly as
 *                                             rti_shade_normals forms it
 *   S    = ks · max(0, h)^spec_exp            rti_relight_enhanced's repeated squaring
 *   v_c  = kd·(double)V_c + S                 fp64, no contraction
 *   out  = NaN if n_x, n_y or n_z is NaN, else v_c; converted once (F32; I32 / U8 as rti_relight)
 * The highlight is white: one S for the three channels.  A NaN normal (kind 4 of the normal entries) gives a NaN
 * pixel whatever ks is; a non-finite coefficient propagates through V_c as in rti_relight.  There is no albedo
 * argument: the diffuse term is the HSH value itself.  With kd = 1, ks = 0 and finite normals the F32 image equals
 * rti_relight's (rti_relight_rgb's, rti_relight_hsh8's) as values (a −0 becomes +0); with kd = 0, finite coefficients
 * and C = 1 it equals rti_shade_normals(kd = 0) bit for bit.
 * rti_relight_hsh_specular: coef: device fp32, C = 1 or 3 maps as rti_hsh_normals takes them: [c][p][k]
 *   (RTI_COEF_PIXEL_MAJOR) or [c][k][p] (RTI_COEF_PLANAR), coef_channel_stride in elements, 0 = dense = k·P (one map
 *   never uses it).  out[e][p] for C = 1, out[e][p][c] (RGB interleaved) for C = 3.  4·C·k + 12 bytes in and
 *   C·sizeof(out) per direction out per pixel.
 * rti_relight_hsh8_specular: coef8 / qparams as rti_relight_hsh8 takes them; out[e][p][c].  The image equals
 *   rti_relight_hsh_specular's of the dequantised maps bit for bit.  3k + 12 bytes in and 3·sizeof(out) per
 *   direction out per pixel.
 * Both: normals: device fp32, normal_layout [p][3] or [3][p].  luv: [E][2] fp64 on the HOST, 1 <= E <=
 *   RTI_SPECULAR_MAX_DIRS -- unlike rti_relight_hsh8's device luv: the entry forms each direction's
 *   {lu, lv, hx, hy, hz} in fp64 and all of them travel as one kernel argument (16 × 40 bytes), so a call allocates
 *   and copies nothing and can be captured in a hipGraph (the directions are then part of the capture).  One launch;
 *   the coefficients or bytes and the normal are read once for all E directions.  Device pointers otherwise,
 *   stream-ordered, no synchronisation.
 * Every argument check answers before any HIP call.  RTI_ERR_BAD_ARG: a null pointer; P < 1; E outside
 * [1, RTI_SPECULAR_MAX_DIRS]; C other than 1 or 3; a channel stride below dense (C = 3); a bad coefficient or normal
 * layout; non-finite kd, ks or luv value; spec_exp outside [1, 255]; qparams off 4 bytes.  RTI_ERR_UNSUPPORTED: a basis
 * other than HSH-9 / HSH-16 (PTM-6 has rti_relight_rgb_enhanced); an out_dtype other than F32 / I32 / U8.
 * One pixel per lane, 64 consecutive pixels per wave, as rti_relight_hsh8.  The fast paths move a full wave's
 * contiguous run as whole 16-byte (output images: 4-byte) pieces through LDS and need:
 *   the fp32 maps, pixel-major:  coef 16-byte aligned and (C = 3) a channel stride that is a multiple of 4
 *                                (planar maps are read per lane, coalesced as they are);
 *   coef8:                       16-byte aligned;
 *   normals, pixel-major:        16-byte aligned (planar normals are read per lane);
 *   out:                         4-byte aligned, and for U8 also P % 4 == 0.
 * Anything else, and the last partial wave of any launch, loads and stores per lane through the same per-pixel
 * function and gives the same bits.
 * Not built: planar RGB output, a multi-GPU wrapper.  (Diffuse gain for HSH maps: rti_relight_hsh_gain, below.) */
#define RTI_SPECULAR_MAX_DIRS 16
int rti_relight_hsh_specular(const float* coef, int basis, int coef_layout, int C, int64_t coef_channel_stride,
                             int64_t P, const float* normals, int normal_layout,
                             double kd, double ks, int spec_exp, const double* luv /* HOST [E][2] */, int E,
                             void* out, int out_dtype, rti_stream_t stream);
int rti_relight_hsh8_specular(const uint8_t* coef8, int basis, int64_t P, const float* qparams,
                              const float* normals, int normal_layout,
                              double kd, double ks, int spec_exp, const double* luv /* HOST [E][2] */, int E,
                              void* out, int out_dtype, rti_stream_t stream);

/* ---- device: diffuse gain for HSH maps under a normal map (rti_hsh_gain.hip) ------------------------
 * The diffuse-gain mode of rti_relight_enhanced for the bases without a closed-form peak.  For a PTM whose gradient
 * vanishes at its peak l0, Malzbender's transform of the six coefficients is, identically,
 *   L'(l) = L(l) + (g − 1)·(L(l) − L(l0)):
 * it keeps the peak's value and direction and multiplies the fall-off away from the peak by g.  The expression names
 * no curvature, so it carries over to any basis once a peak direction is known; for an HSH map that is the normal map
 * rti_hsh_normals / rti_hsh8_normals produce once per object (optionally sharpened by rti_map_unsharp), which these
 * entries read as rti_relight_hsh_specular does; the semantics are build-defined.  Per pixel p, channel c and
 * direction e, every operation rounded, each expression left to right as written, nothing contracted except the fmaf
 * chain named:
 *   V_c = rti_relight's F32 value of channel c's coefficients at (lu_e, lv_e), bit for bit (as rti_relight_hsh_specular
 *         states it; for the 8-bit map c_j = (float)raw_j·step_j + bias_j as rti_relight_hsh8 states it)
 *   A_c = the same F32 value at the pixel's own direction (n_x, n_y), the fp32 normal components as they are:
 *         basis_eval<float>(n_x, n_y), acc = c_0·b_0, acc = fmaf(c_j, b_j, acc) for j = 1..k−1.  That is
 *         rti_relight(coef_c, (double)n_x, (double)n_y) at that pixel, bit for bit.
 *   d   = (double)V_c − (double)A_c
 *   v_c = (double)V_c + gm1·d            fp64, no contraction; gm1 = gain − 1 formed on the HOST in fp64
 *   out = NaN if n_x, n_y or n_z is NaN, else v_c; converted once (F32; I32 / U8 as rti_relight)
 * The normal is not checked for unit length and n_z is read only for the NaN test (the basis clamps a direction
 * outside the unit disc as it does a light's).  A non-finite coefficient propagates through V and A as the arithmetic
 * gives.  gain is any finite double; zero and negative values are allowed.  Hence: gain = 1 under finite normals and
 * finite coefficients is the plain relight exactly (gm1 = 0); gain = 0 gives A_c for every direction (to fp64
 * rounding); a light direction equal to a pixel's (n_x, n_y) gives A_c at that pixel for every gain.
 * rti_relight_hsh_gain: coef, basis, coef_layout, C, coef_channel_stride, P, normals, normal_layout, luv, E, out and
 *   out_dtype exactly as rti_relight_hsh_specular takes them: C = 1 or 3 maps, out[e][p] or out[e][p][c], luv [E][2]
 *   fp64 on the HOST with 1 <= E <= RTI_SPECULAR_MAX_DIRS (the directions travel as one kernel argument, 16 × 16
 *   bytes).  4·C·k + 12 bytes in and C·sizeof(out) per direction out per pixel.
 * rti_relight_hsh8_gain: coef8 / qparams as rti_relight_hsh8 takes them, the rest as above; out[e][p][c].  The image
 *   equals rti_relight_hsh_gain's of the dequantised maps bit for bit.  3k + 12 bytes in and 3·sizeof(out) per
 *   direction out per pixel.
 * Both: one launch, no allocation, no copy, no synchronisation, capturable in a hipGraph (the directions and the gain
 *   are then part of the capture).  The coefficients or bytes and the normal are read once for all E directions; the
 *   basis at the normal (three fp32 square roots and two divisions) and the C anchors are formed once per pixel and
 *   launch, not per direction.
 * Every argument check answers before any HIP call.  RTI_ERR_BAD_ARG: the cases of rti_relight_hsh_specular (a null
 * pointer; P < 1; E outside [1, RTI_SPECULAR_MAX_DIRS]; C other than 1 or 3; a channel stride below dense (C = 3); a
 * bad coefficient or normal layout; a non-finite luv value; qparams off 4 bytes) and a non-finite gain.
 * RTI_ERR_UNSUPPORTED: a basis other than HSH-9 / HSH-16 (PTM-6 has rti_relight_enhanced and its RGB forms); an
 * out_dtype other than F32 / I32 / U8.
 * Lane map, fast paths and their alignment rules: rti_relight_hsh_specular's, above.  Anything they cannot serve, and
 * the last partial wave of any launch, loads and stores per lane through the same per-pixel functions and gives the
 * same bits.
 * Not built: planar RGB output, a gain combined with a highlight, fp64 maps, a multi-GPU wrapper. */
int rti_relight_hsh_gain(const float* coef, int basis, int coef_layout, int C, int64_t coef_channel_stride,
                         int64_t P, const float* normals, int normal_layout, double gain,
                         const double* luv /* HOST [E][2] */, int E, void* out, int out_dtype, rti_stream_t stream);
int rti_relight_hsh8_gain(const uint8_t* coef8, int basis, int64_t P, const float* qparams,
                          const float* normals, int normal_layout, double gain,
                          const double* luv /* HOST [E][2] */, int E, void* out, int out_dtype, rti_stream_t stream);

/* ---- device: surface height from a normal map, masked Poisson integration (rti_height.hip) -----------------------
 * The reference has no integrator; the semantics are build-defined.
 * Input: normals, fp32, dense, H x W, [y][x][3] (RTI_NORMAL_PIXEL_MAJOR) or [3][y][x] (RTI_NORMAL_PLANAR).  x is the
 *   column index and y the row index.  The height z satisfies dz/dx = -n_x/n_z and dz/dy = -n_y/n_z; flip_y != 0
 *   negates the y-gradient, for maps whose y component points up the image.
 * Validity: a pixel is valid when its three components are finite and n_z >= nz_min, nz_min in (0, 1]; the kind-4 NaN
 *   pixels and the kind-1 edge normals with n_z = 0 of the normal entries fall out this way.  A valid pixel with no
 *   valid 4-neighbour carries no height information and is invalid too.
 * Gradients, per valid pixel, in fp64 from the fp32 components, each quotient rounded once:
 *     p = -((double)n_x/(double)n_z),   q = -((double)n_y/(double)n_z), or +(...) under flip_y
 * The problem: the least-squares surface over the graph of valid pixels with an edge between valid 4-neighbours,
 *     minimise  sum over edges (z_j - z_i - g_ij)^2
 *   with g_ij = (p_i + p_j)/2 for a horizontal edge (i left of j) and (q_i + q_j)/2 for a vertical one (i above j):
 *   the midpoint functional, exact for quadratic surfaces.  No boundary condition: holes and irregular outlines are
 *   natural boundaries.  Normal equations A z = b: A the graph Laplacian, b_i = sum over the neighbours j of -g_ij with
 *   the edge oriented from i, summed in the order left, right, up, down in fp64 with no contraction.
 * Gauge: the null space is one constant per connected component.  The entry subtracts the mean of z over ALL valid
 *   pixels (one fixed-order fp64 reduction at the end); separate components float independently of each other.
 * Output: height fp32 [H][W], NaN at invalid pixels; valid (NULL ok) uint8 [H][W], 1 / 0.
 * Solver: preconditioned conjugate gradients in fp64 on the device from z = 0, or from z0 (NULL ok; fp32 [H][W], read
 *   only at valid pixels, where it must be finite; it may be the height array itself).  It stops when
 *   |r|_2 <= rtol*|b|_2 or after max_iters iterations (0 returns the start with its residual); |b|_2 = 0 returns z = 0
 *   with 0 iterations and no division.  Not converging is not an error: RTI_OK and stats[1] = -1.
 *   precond = RTI_HEIGHT_JACOBI: the diagonal (the valid degree).  RTI_HEIGHT_MULTIGRID: one symmetric V-cycle of
 *   unsmoothed 2x2 aggregation multigrid in fp64: level l+1 is ceil(H_l/2) x ceil(W_l/2), a coarse cell exists when
 *   any child does, its edges carry the summed fine weights crossing between the two cells (the Galerkin operator),
 *   restriction sums the children's residuals, prolongation copies the coarse correction times 2 (over-correction),
 *   2 + 2 sweeps of weighted Jacobi (0.8) from a zero guess, levels stop at max(H_l, W_l) <= 4 where 8 sweeps run and
 *   no exact solve (the operator is singular); cells of degree 0 on any level keep a zero correction.  The
 *   preconditioner is one fixed, symmetric, linear operator throughout a solve.
 *   Dot products are two-stage fixed-order reductions (no atomics), so one call gives the same bits run to run; the
 *   PCG scalars stay in device memory.  No kernel waits on another workgroup.
 * Synchronisation: the host reads |r|^2 back through the workspace every check_every iterations, in [1, 1024], and
 *   once after set-up and once at the end, and SYNCHRONISES stream each time: the entry is not capturable in a
 *   hipGraph.  The host overshoots by at most check_every - 1 iterations.  No allocation.
 * workspace: device, 256-byte aligned, the bytes the size query returns (0 on bad arguments; a function of H*W and
 *   precond alone, monotone in H*W); it need not be initialised.  The level count query answers -1 on bad sizes.
 * stats (HOST [6], NULL ok): iterations run; the iteration at which the criterion was first met on the device (0 = the
 *   start met it), or -1; the final recursive |r|/|b|; the true |b - A z|/|b| recomputed once at the end; the count
 *   of valid pixels; |b|_2.  With |b|_2 = 0: 0, 0, 0, 0, the count, 0.
 * Every argument check answers before any HIP call.  RTI_ERR_BAD_ARG: null normals, workspace or height; H or W < 1;
 *   H*W >= 2^31; a bad layout or precond; nz_min outside (0, 1]; rtol not finite or < 0; max_iters outside
 *   [0, 100000]; check_every outside [1, 1024]; workspace off 256 bytes; height overlapping normals.
 * Not built: per-edge confidence weights, robust (L1 / total-variation) integration for depth discontinuities,
 *   perspective cameras, a per-component gauge, a multi-GPU wrapper, an entry that takes gradients, mesh export. */
#define RTI_HEIGHT_MULTIGRID 0
#define RTI_HEIGHT_JACOBI    1
int    rti_height_levels(int H, int W);
size_t rti_height_workspace_bytes(int H, int W, int precond);
int    rti_height_from_normals(const float* normals, int normal_layout, int H, int W,
                               double nz_min, int flip_y, const float* z0 /* NULL ok */,
                               double rtol, int max_iters, int check_every, int precond,
                               void* workspace, float* height, uint8_t* valid /* NULL ok */,
                               double* stats /* HOST [6], NULL ok */, rti_stream_t stream);

/* ---- device: multi-light detail enhancement (rti_multilight.hip) ----------------------------------
 * RTIViewer's static / dynamic multi-light mode (Palma, Corsini, Cignoni, Scopigno, Mudge 2010): for every small tile
 * of the image the light, out of E candidates near the user's light, that shows the tile's relief best (local
 * sharpness plus brightness); the per-tile choice smoothed into a light field; the image relit with a light direction
 * per pixel.  The reference has none of it; the semantics are build-defined.  Every expression below is evaluated left
 * to right as written, every operation rounded, nothing contracted except the fused multiply-adds named.
 * Common to the three entries: the image is H x W with pixel p = y·W + x and H·W < 2^31.  Maps: device fp32, C = 1 or 3
 * maps as rti_fit_shared writes them, [c][p][k] (RTI_COEF_PIXEL_MAJOR) or [c][k][p] (RTI_COEF_PLANAR),
 * coef_channel_stride in elements, 0 = dense = k·P (one map never uses it); basis PTM-6, HSH-9 or HSH-16.  The tile
 * edge T is 8, 16 or 32; tile (ty, tx) covers the rows [ty·T, min((ty+1)·T, H)) and the columns likewise;
 * Ty = ceil(H/T), Tx = ceil(W/T); tile arrays are [Ty][Tx] row-major.
 * rti_light_scores (the search; one launch, one workgroup per tile, the maps read once, 16·E bytes out per tile):
 *   luminance map   C = 1: l_j = c_j.  C = 3: l_j = (wR·r_j + wG·g_j) + wB·b_j in fp32 as rti_hsh_normals forms it; w:
 *                   three fp32 weights on the HOST, NULL = (0.299f, 0.587f, 0.114f).
 *   candidates      luv: fp64 [E][2] on the HOST, 1 <= E <= RTI_LIGHT_MAX_CANDIDATES, every value finite (they travel
 *                   as one kernel argument, 64 × 16 bytes).
 *   usable          a pixel all k of whose l_j are finite; this does not depend on the candidate.
 *   value           V_e(x, y) = rti_relight's F32 value of the luminance map at candidate e, bit for bit: the same
 *                   basis_eval<float> of ((float)lu_e, (float)lv_e) and the same chain acc = l_0·b_0,
 *                   acc = fmaf(l_j, b_j, acc) for j = 1..k−1.
 *   S_e             the fp64 sum of d·d over every pair of usable pixels inside the tile that are horizontal or vertical
 *                   neighbours, d = (double)V_e(second) − (double)V_e(first) (exact); n_S = the number of pairs.  No
 *                   pixel outside the tile is read: pairs across a tile edge do not count.
 *   B_e             the fp64 sum of (double)V_e over the tile's n_P usable pixels.
 *   scores          device fp64 [Ty][Tx][E][2], 8-byte aligned: sharp_e = S_e/(double)n_S, or 0 if n_S = 0;
 *                   bright_e = B_e/(double)n_P, or 0 if n_P = 0.
 *   count           NULL or device int32 [Ty][Tx]: n_P.
 *   The order of the two sums is the kernel's own (per lane, then over the wave, then over the waves, each fixed): a
 *   call gives the same bits run to run, and sharp_e lies within (n_S + 2)·2^-53 (relative) of the exact quotient,
 *   bright_e within (n_P + 1)·2^-53·mean|V_e|.  No floating-point atomics.
 * rti_light_field (the choice and its smoothing; 1 + smooth launches of a thread per tile):
 *   scores, count   as rti_light_scores wrote them (count is required); luv, E: the same candidates.
 *   per tile, fp64  Smax = the largest sharp_e and Bmax the largest bright_e over e, each raised from 0 with `>` (a NaN
 *                   never raises it).  s_e = sharp_e/Smax if Smax > 0, else 0; b_e = bright_e/Bmax if Bmax > 0, else 0;
 *                   score_e = ws·s_e + wb·b_e: two products, one sum.  ws, wb: finite and >= 0.
 *   choice          the e with the largest score_e, the smallest e among equals; a NaN score never wins.  −1 if count
 *                   is 0 or every score is NaN: such a tile takes the main light (lu0, lv0), finite; any other tile
 *                   takes (lu_e, lv_e) of its choice, in fp64.
 *   smoothing       smooth in [0, 8] passes of the 3x3 binomial (1 2 1)x(1 2 1) over the tile grid, per component:
 *                   acc = 0, wsum = 0; for dy = −1..1 (outer), dx = −1..1 (inner), tiles outside the grid skipped:
 *                   acc = acc + wt·f, wsum = wsum + wt with wt = (2 − |dy|)·(2 − |dx|); the result is acc/wsum.
 *                   Intermediates stay fp64 in the workspace.
 *   field           device fp32 [Ty][Tx][2], rounded once from the last pass (or from the choice when smooth = 0).
 *   choice          NULL or device int32 [Ty][Tx].
 *   workspace       device, 8-byte aligned, workspace_bytes >= rti_light_field_workspace_bytes(Ty, Tx) = 32·Ty·Tx (0 on
 *                   bad sizes); it need not be initialised.
 * rti_relight_field (a light per pixel; one launch, a pixel per lane):
 *   light_form RTI_LIGHT_TILES   light: device fp32 [Ty][Tx][2] for tile edge T.  Per pixel (x, y) in fp64:
 *                   fx = ((double)x − (double)(T − 1)/2)/(double)T clamped to [0, Tx − 1]; i0 = floor(fx),
 *                   i1 = min(i0 + 1, Tx − 1), a = fx − i0; fy, j0, j1, b likewise along y with Ty.  Per component:
 *                   top = f[j0][i0] + a·(f[j0][i1] − f[j0][i0]), bottom likewise on row j1,
 *                   l = top + b·(bottom − top).  The light is ((float)lu, (float)lv).
 *   light_form RTI_LIGHT_PIXELS  light: device fp32 [H·W][2], used as it is; T is not read.  The entry for any other
 *                   source of per-pixel light directions, e.g. a near-light correction.
 *   value           per channel c: rti_relight's F32 value of that channel's own coefficients at the pixel's light,
 *                   bit for bit: basis_eval<float>(lu, lv) on the device, acc = c_0·b_0, acc = fmaf(c_j, b_j, acc);
 *                   that is rti_relight(coef_c, (double)lu, (double)lv) at that pixel.  A light with a non-finite
 *                   component gives NaN instead.  Converted once: F32, or I32 / U8 as rti_relight (NaN gives INT32_MIN
 *                   and 0).
 *   out             [p] for C = 1, [p][c] for C = 3.  4·C·k + 8 bytes (PIXELS) in and C·sizeof(out) out per pixel.
 *   Lane map, fast paths and alignment rules of the maps and the output: rti_relight_hsh_specular's for one direction;
 *   anything they cannot serve, and the last partial wave, loads and stores per lane and gives the same bits.
 * All: device pointers, stream-ordered, no allocation, no synchronisation, capturable in a hipGraph (the candidates,
 * weights and main light are then part of the capture).  Every argument check answers before any HIP call.
 * RTI_ERR_BAD_ARG: a null pointer (w, count of rti_light_scores and choice may be null); H or W < 1 or H·W >= 2^31; Ty or
 * Tx < 1; a tile edge other than 8, 16, 32; E outside [1, RTI_LIGHT_MAX_CANDIDATES]; a non-finite candidate, weight or
 * main light; ws or wb negative or not finite; smooth outside [0, 8]; C other than 1 or 3; a bad coefficient layout or
 * light form; a channel stride below dense (C = 3); scores or workspace off 8 bytes, light off 4; a workspace too
 * small.  RTI_ERR_UNSUPPORTED: an unknown basis; an out_dtype other than F32 / I32 / U8.
 * Not built: the 8-bit and LRGB forms, a multi-GPU wrapper, the enhanced modes (diffuse gain, specular) under a light
 * field, overlapping tiles, fp64 maps. */
#define RTI_LIGHT_MAX_CANDIDATES 64
#define RTI_LIGHT_TILES  0   /* light[Ty][Tx][2], bilinear between the tile centres */
#define RTI_LIGHT_PIXELS 1   /* light[H*W][2] */
int    rti_light_scores(const float* coef, int basis, int coef_layout, int C, int64_t coef_channel_stride,
                        int H, int W, int T, const float* w /* HOST, NULL ok */,
                        const double* luv /* HOST [E][2] */, int E,
                        double* scores, int32_t* count /* NULL ok */, rti_stream_t stream);
size_t rti_light_field_workspace_bytes(int Ty, int Tx);
int    rti_light_field(const double* scores, const int32_t* count, int Ty, int Tx,
                       const double* luv /* HOST [E][2] */, int E, double ws, double wb, double lu0, double lv0,
                       int smooth, void* workspace, size_t workspace_bytes,
                       float* field, int32_t* choice /* NULL ok */, rti_stream_t stream);
int    rti_relight_field(const float* coef, int basis, int coef_layout, int C, int64_t coef_channel_stride,
                         int H, int W, const float* light, int light_form, int T,
                         void* out, int out_dtype, rti_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* RTI_H */
