// rti_fit_robust.hip -- robust shared-direction fit: intensity window + Huber IRLS (gfx950).
//
// The plain least squares of analysis.py:280-298 treats every one of a pixel's N samples alike.  On the
// 8-bit V channel of a metal surface (FeatureMatcher.py:183-184, analysis.py:219) many of them are clipped
// at 255 (specular highlight) or sit at 0 (self-shadow); the PTM/HSH model cannot describe those.  Here each
// pixel drops the samples outside [lo, hi] and, optionally, reweights the rest by Huber's function of their
// residuals.  Per channel and pixel, with A the shared fp64 design [N][k] and y_n the pixel's samples:
//
//   window    win_n = lo <= y_n <= hi, m = Σ win_n
//   solve(w)  G = Σ w_n a_n a_nᵀ, b = Σ w_n a_n y_n (fp64), Cholesky G = L Lᵀ; fails at a pivot
//             d_j <= 1e-10·max_i G_ii, else coef = G⁻¹ b
//   fallback  m < min_lights or solve(win) failed: win = 1, m = N, coef = solve(1) (NaN if that fails too);
//             the pixel is counted in *fallback_px
//   IRLS      iters times: r_n = y_n − a_n·coef, w_n = win_n·min(1, delta/|r_n|), coef = solve(w); a failed
//             solve keeps the previous coef and ends the pixel's iteration
//   outputs   coef (fp32), res = sqrt(Σ win_n r_n² / m), kept = m
//
// The weights depend on the pixel's own residuals, so there is no shared operator: every pass accumulates a
// k×k Gram per pixel.  One lane owns one pixel; the rows of A are wave-uniform (scalar loads) and the fp64
// state is k(k+1)/2 + k accumulators (54 VGPRs at k = 6, 108 at k = 9), factored in registers like
// rti_perpixel.hip's ne_solve.
//
// Two forms run the same arithmetic in the same order:
//   resident   a workgroup of TP lanes copies its tile [N][TP] of the stack, in the input dtype, into LDS once
//              (16-byte loads when the planes are 16-byte aligned) and every pass reads the samples from there:
//              one stack read from HBM whatever iters is.  TP = the largest of 256 / 128 / 64 pixels whose tile
//              fits the CU's 160 KiB (rti_fit_shared_robust_plan); the kernel stages nothing else.
//   streaming  every pass reads the samples from global memory (no tile fits, iters == 0, or forced).
// With iters == 0 the residual energy comes from the same pass as the solve, Σ w r² = q − 2 cᵀb + cᵀG c with
// q = Σ w y² (fp64: the cancellation leaves ~1e-9 of q), so that fit reads the stack once; with iters > 0 a last
// pass forms the residuals of the final coefficients explicitly.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rti_internal.h"
#include "rti_robust_px.h"
#include "rti_stack.h"

namespace rti {
namespace {

using namespace robust_px;  // the per-pixel fit, shared with rti_ps.hip

// TP lanes per workgroup, one pixel each.  RESIDENT: the tile [N][TP] is copied into LDS first (vec: by 16-byte
// loads; the host passes vec only when every plane of every tile is 16-byte aligned) and the passes read it from
// there.  A lane past P reads pixel P − 1 and stores nothing.
template <int K, typename T, int TP, bool RESIDENT, bool ITER, int LAYOUT>
__global__ void __launch_bounds__(TP)
fit_robust_k(const double* __restrict__ A, int N, const T* __restrict__ I, int64_t P, int64_t lstride, int64_t cstride,
             double lo, double hi, int min_lights, int iters, double delta, float* __restrict__ coef, int64_t ocstride,
             float* __restrict__ res, int32_t* __restrict__ kept, int* __restrict__ fallback_px, int vec) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rb_lds[];
  const int t = threadIdx.x;
  const int64_t tile0 = (int64_t)blockIdx.x * TP;
  const int64_t p = tile0 + t;
  const bool live = p < P;
  const int64_t pr = live ? p : P - 1;
  const T* __restrict__ src = I + (int64_t)blockIdx.y * cstride;

  RbSamples<T> y_of;
  if constexpr (RESIDENT) {
    rb_stage_tile<T, TP>(rb_lds, src, N, lstride, tile0, P, vec);
    __syncthreads();
    y_of.p = reinterpret_cast<const T*>(rb_lds) + t;
    y_of.step = TP;
  } else {
    y_of.p = src + pr;
    y_of.step = lstride;
  }

  double c[K];
  const RbOut o = rb_pixel<K, ITER>(RbSharedRows<K>{A}, N, y_of, lo, hi, min_lights, iters, delta, c);

  if (live) {
    float* __restrict__ dst = coef + (int64_t)blockIdx.y * ocstride;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      if constexpr (LAYOUT == RTI_COEF_PLANAR)
        dst[(int64_t)i * P + p] = (float)c[i];
      else
        dst[p * K + i] = (float)c[i];
    }
    if (res) res[(int64_t)blockIdx.y * P + p] = (float)sqrt(o.ss / (double)o.m);
    if (kept) kept[(int64_t)blockIdx.y * P + p] = o.m;
  }
  if (fallback_px) {  // one atomic per wave that has any
    const unsigned long long fb = __ballot(live && o.fell);
    if (fb != 0 && (t & 63) == 0) atomicAdd(fallback_px, __popcll(fb));
  }
}

struct RbArgs {
  const double* A;
  StackView in;
  double lo, hi;
  int min_lights, iters;
  double delta;
  CoefView out;
  float* res;
  int32_t* kept;
  int* fallback_px;
  int tp;  // resident tile pixels, 0 = streaming
  int vec;
  hipStream_t s;
};

template <int K, typename T, int TP, bool RESIDENT, bool ITER, int LAYOUT>
int launch_rb(const RbArgs& a) {
  auto kern = fit_robust_k<K, T, TP, RESIDENT, ITER, LAYOUT>;
  const StackView& in = a.in;
  const size_t lds = RESIDENT ? (size_t)in.N * TP * sizeof(T) : 0;
  if (lds > 64 * 1024 && reserve_lds(reinterpret_cast<const void*>(kern), lds) != hipSuccess)
    return fail(RTI_ERR_HIP, "rti_fit_shared_robust: cannot reserve %zu bytes of LDS", lds);
  const dim3 grid(grid_1d(in.P, TP), in.C);
  hipLaunchKernelGGL(kern, grid, dim3(TP), lds, a.s, a.A, in.N, static_cast<const T*>(in.I), in.P, in.lstride, in.cstride,
                     a.lo, a.hi, a.min_lights, a.iters, a.delta, a.out.coef, a.out.ocstride, a.res, a.kept, a.fallback_px,
                     a.vec);
  return check_launch("rti_fit_shared_robust");
}

template <int K, typename T, int LAYOUT>
int launch_rb_form(const RbArgs& a) {
  // the resident form runs only with iters > 0 (rti_fit_shared_robust_plan)
  switch (a.tp) {
    case 256: return launch_rb<K, T, 256, true, true, LAYOUT>(a);
    case 128: return launch_rb<K, T, 128, true, true, LAYOUT>(a);
    case 64: return launch_rb<K, T, 64, true, true, LAYOUT>(a);
    default:
      return a.iters > 0 ? launch_rb<K, T, 256, false, true, LAYOUT>(a) : launch_rb<K, T, 256, false, false, LAYOUT>(a);
  }
}

template <int K, typename T>
int launch_rb_l(const RbArgs& a) {
  return a.out.layout == RTI_COEF_PLANAR ? launch_rb_form<K, T, RTI_COEF_PLANAR>(a)
                                     : launch_rb_form<K, T, RTI_COEF_PIXEL_MAJOR>(a);
}

template <typename T>
int launch_rb_k(const RbArgs& a) {
  return a.out.k == 6 ? launch_rb_l<6, T>(a) : launch_rb_l<9, T>(a);
}

}  // namespace
}  // namespace rti

using namespace rti;

extern "C" int rti_fit_shared_robust_plan(int k, int N, int in_dtype, int iters, int kernel) {
  if ((k != 6 && k != 9) || N < k || iters <= 0 || (kernel & RTI_KERNEL_ONE_LAUNCH)) return 0;
  if (in_dtype != RTI_F32 && in_dtype != RTI_U8 && in_dtype != RTI_I32) return 0;
  return rb_tile_pixels(N, in_dtype);
}

extern "C" int rti_fit_shared_robust(const double* A, int k, int N, const void* I, int in_dtype, int64_t P, int C,
                                     int64_t light_stride, int64_t channel_stride, float lo, float hi,
                                     int min_lights, int iters, float delta, float* coef, int coef_layout,
                                     int64_t coef_channel_stride, float* res, int32_t* kept, int* fallback_px,
                                     int kernel, rti_stream_t stream) {
  if (!kernel_bits_ok(kernel, RTI_KERNEL_AUTO, RTI_KERNEL_ONE_LAUNCH))
    return fail(RTI_ERR_BAD_ARG, "rti_fit_shared_robust: unknown kernel bits 0x%x", kernel);
  const char* const E = "rti_fit_shared_robust";
  if (int st = check_pointers(E, {A, I, coef})) return st;
  if (int st = check_extents(E, "N/P/C", N, P, C)) return st;
  if (k == 16) return fail(RTI_ERR_UNSUPPORTED, "%s: k=16 (its 136 + 16 fp64 accumulators do not fit one lane)", E);
  if (k != 6 && k != 9) return fail(RTI_ERR_UNSUPPORTED, "%s: k=%d (supported: 6, 9)", E, k);
  if (int st = check_in_dtype(E, in_dtype)) return st;
  if (int st = check_lights(E, N, k)) return st;
  if (!(lo <= hi)) return fail(RTI_ERR_BAD_ARG, "%s: window needs lo <= hi, neither NaN", E);
  if (min_lights < k || min_lights > N)
    return fail(RTI_ERR_BAD_ARG, "%s: min_lights=%d outside [k=%d, N=%d]", E, min_lights, k, N);
  if (iters < 0 || iters > 16) return fail(RTI_ERR_BAD_ARG, "%s: iters=%d outside [0, 16]", E, iters);
  if (iters > 0 && !(delta > 0.0f)) return fail(RTI_ERR_BAD_ARG, "%s: delta must be > 0", E);
  if (int st = check_coef_layout(E, coef_layout)) return st;
  RbArgs a{A, stack_view(I, in_dtype, N, P, C, light_stride, channel_stride), (double)lo, (double)hi, min_lights, iters,
           (double)delta, coef_view(coef, coef_layout, k, P, coef_channel_stride), res, kept, fallback_px};
  if (int st = check_stack_strides(E, a.in)) return st;
  if (int st = check_coef_stride(E, a.out, P, C)) return st;
  a.tp = rti_fit_shared_robust_plan(k, N, in_dtype, iters, kernel);
  // 16-byte tile loads, a rule of this kernel's own: strides in bytes, no condition on P
  const int64_t es = (int64_t)a.in.es;
  a.vec = aligned_to(I, 16) && a.in.lstride * es % 16 == 0 && a.in.cstride * es % 16 == 0;
  a.s = (hipStream_t)stream;
  note_launches(1);
  switch (in_dtype) {  // not with_in_dtype: its order of instantiation would reorder this file's kernels
    case RTI_F32: return launch_rb_k<float>(a);
    case RTI_U8: return launch_rb_k<uint8_t>(a);
    default: return launch_rb_k<int32_t>(a);
  }
}
