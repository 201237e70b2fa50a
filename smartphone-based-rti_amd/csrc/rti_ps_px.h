// rti_ps_px.h -- the photometric-stereo kernel shared by rti_ps.hip (one light direction per light) and
// rti_ps_near.hip (a light position per light, a row per pixel): the fit of rti_robust_px.h per channel, the tail
// (normal, albedos, kind), the outputs and the two forms.  The two entries differ only in the light source SRC, a
// kernel argument whose rows(p) returns the row source of pixel p for rb_pixel.
//
// Two forms run the same arithmetic in the same order, so they give the same bits:
//   streaming  every pass reads the samples from global memory (iters == 0: one read of the stack, the residual
//              energy from q − 2cᵀb + cᵀGc; also when no tile fits, or forced with RTI_KERNEL_ONE_LAUNCH)
//   resident   a workgroup of TP lanes copies its tile [C][N][TP] of the stack, in the input dtype, into LDS once
//              and every pass reads from there.  TP = the largest of 256 / 128 / 64 with C·N·TP·sizeof(element)
//              <= 160 KiB (ps_plan).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rti_dispatch.h"
#include "rti_internal.h"
#include "rti_robust_px.h"
#include "rti_stack.h"

namespace rti {
namespace ps_px {

using namespace robust_px;

// ---- light sources ------------------------------------------------------------------------------------------------

// rti_photometric_stereo: the design A [N][3], the same rows for every pixel
struct PsFarSrc {
  const double* __restrict__ A;
  __device__ __forceinline__ RbSharedRows<3> rows(int64_t) const { return {A}; }
};

// The near-light row of include/rti.h (rti_photometric_stereo_near), formed anew at every use: with p the pixel's
// position and L, sc the light's,
//   d = L − p,  s = fma(d_x, d_x, fma(d_y, d_y, d_z·d_z)),  y ≈ 1/√s (the fp64 rsq seed and two Newton steps,
//   y ← fma(y, fma(−(½s)·y, y, ½), y): within 1 ulp, tools/probe/rsq_probe.hip),
//   f = sc·y;  with fall-off f = (f·r0²)·(y·y);  a_j = f·d_j.
// s = 0 gives y = NaN (0·inf in the first step) and s = inf gives y = NaN (inf·0), so a light on the pixel or a
// non-finite light leaves a NaN row for the fit's own failure path.  The light is wave-uniform (scalar loads); p is
// lane-private.
struct PsNearRows {
  const double* __restrict__ L;  // [N][4]: x, y, z, scale
  double px, py, pz, r02;
  int falloff;
  __device__ __forceinline__ void operator()(int n, double (&a)[3]) const {
#pragma clang fp contract(off)
    const double* Ln = L + (int64_t)n * 4;
    const double dx = Ln[0] - px, dy = Ln[1] - py, dz = Ln[2] - pz;
    const double s = fma(dx, dx, fma(dy, dy, dz * dz));
    double y = __builtin_amdgcn_rsq(s);
    const double h = 0.5 * s;
    y = fma(y, fma(-(h * y), y, 0.5), y);
    y = fma(y, fma(-(h * y), y, 0.5), y);
    double f = Ln[3] * y;
    if (falloff) f = (f * r02) * (y * y);  // wave-uniform
    a[0] = f * dx;
    a[1] = f * dy;
    a[2] = f * dz;
  }
};

// rti_photometric_stereo_near: pixel p = y·W + x sits at (x0 + x, y0 + y, z_offset + h), h = height[p] where that
// is given and finite, else 0
struct PsNearSrc {
  const double* __restrict__ L;
  const float* __restrict__ height;
  double x0, y0, z_offset, r02;
  int W, falloff;
  __device__ __forceinline__ PsNearRows rows(int64_t p) const {
#pragma clang fp contract(off)
    const uint32_t q = (uint32_t)p;  // H·W < 2^31
    const uint32_t yi = q / (uint32_t)W, xi = q - yi * (uint32_t)W;
    float h = 0.0f;
    if (height) {
      h = height[p];
      h = isfinite(h) ? h : 0.0f;
    }
    return {L, x0 + (double)xi, y0 + (double)yi, z_offset + (double)h, r02, falloff};
  }
};

// ---- the tail -----------------------------------------------------------------------------------------------------

struct PsPixel {
  double n[3], albedo[3];
  int kind;
};

// g_c [C][3] -> normal, albedos and kind, in the order include/rti.h writes them
template <int C>
__device__ __forceinline__ PsPixel ps_tail(const double (&gc)[C][3], const double (&w)[3]) {
#pragma clang fp contract(off)
  PsPixel o;
  bool finite = true;
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int j = 0; j < 3; ++j) finite = finite && isfinite(gc[c][j]);
  double g[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if constexpr (C == 1)
      g[j] = gc[0][j];
    else
      g[j] = fma(w[2], gc[2][j], fma(w[1], gc[1][j], w[0] * gc[0][j]));
  }
  const double s = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
  if (!finite) {
    o.kind = 4;
#pragma unroll
    for (int j = 0; j < 3; ++j) o.n[j] = o.albedo[j] = __builtin_nan("");
    return o;
  }
  if (s > 0.0) {
    o.kind = g[2] >= 0.0 ? 0 : 1;
#pragma unroll
    for (int j = 0; j < 3; ++j) o.n[j] = g[j] / s;
  } else {  // s == 0 (a finite g leaves no NaN)
    o.kind = 2;
    o.n[0] = 0.0, o.n[1] = 0.0, o.n[2] = 1.0;
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    double a = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) a = fma(gc[c][j], o.n[j], a);
    o.albedo[c] = a;
  }
  return o;
}

// ---- the kernel ---------------------------------------------------------------------------------------------------

// TP lanes per workgroup, one pixel with its C channels each.  RESIDENT: the tile [C][N][TP] is copied into LDS
// first and the passes read it from there.  A lane past P reads pixel P − 1 and stores nothing.
template <typename SRC, typename T, int C, int TP, bool RESIDENT, bool ITER, int NL>
__global__ void __launch_bounds__(TP)
ps_k(const SRC src, int N, const T* __restrict__ I, int64_t P, int64_t lstride, int64_t cstride, double lo, double hi,
     int min_lights, int iters, double delta, double w0, double w1, double w2, float* __restrict__ normals,
     float* __restrict__ albedo, uint8_t* __restrict__ kind, float* __restrict__ res, int32_t* __restrict__ kept,
     int* __restrict__ fallback_px, int vec) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ps_lds[];
  const int t = threadIdx.x;
  const int64_t tile0 = (int64_t)blockIdx.x * TP;
  const int64_t p = tile0 + t;
  const bool live = p < P;
  const int64_t pr = live ? p : P - 1;

  if constexpr (RESIDENT) {
#pragma unroll
    for (int c = 0; c < C; ++c)
      rb_stage_tile<T, TP>(ps_lds + (size_t)c * N * TP * sizeof(T), I + (int64_t)c * cstride, N, lstride, tile0, P, vec);
    __syncthreads();
  }

  const auto row_of = src.rows(pr);
  double gc[C][3];
  int fell = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    RbSamples<T> y_of;
    if constexpr (RESIDENT) {
      y_of.p = reinterpret_cast<const T*>(ps_lds) + c * N * TP + t;
      y_of.step = TP;
    } else {
      y_of.p = I + (int64_t)c * cstride + pr;
      y_of.step = lstride;
    }
    const RbOut o = rb_pixel<3, ITER>(row_of, N, y_of, lo, hi, min_lights, iters, delta, gc[c]);
    if (live) {
      if (res) res[(int64_t)c * P + p] = (float)sqrt(o.ss / (double)o.m);
      if (kept) kept[(int64_t)c * P + p] = o.m;
    }
    if (fallback_px) fell += __popcll(__ballot(live && o.fell));  // wave-uniform
  }

  const double w[3] = {w0, w1, w2};
  const PsPixel o = ps_tail<C>(gc, w);
  if (live) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if constexpr (NL == RTI_NORMAL_PLANAR)
        normals[(int64_t)j * P + p] = (float)o.n[j];
      else
        normals[p * 3 + j] = (float)o.n[j];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) albedo[(int64_t)c * P + p] = (float)o.albedo[c];
    if (kind) kind[p] = (uint8_t)o.kind;
  }
  if (fallback_px && fell != 0 && (t & 63) == 0) atomicAdd(fallback_px, fell);  // one atomic per wave that has any
}

// ---- host: the checks and the dispatch both entries share ------------------------------------------------------------

template <typename SRC>
struct PsArgs {
  const char* entry;
  SRC src;
  StackView in;
  double lo, hi;
  int min_lights, iters;
  double delta;
  double w[3];
  float *normals, *albedo;
  int nl;
  uint8_t* kind;
  float* res;
  int32_t* kept;
  int* fallback_px;
  int tp;  // resident tile pixels, 0 = streaming
  int vec;
  hipStream_t s;
};

// the resident tile's pixels, 0 = the streaming form
inline int ps_plan(int N, int in_dtype, int C, int iters, int kernel) {
  if (N < 3 || (C != 1 && C != 3) || iters <= 0 || (kernel & RTI_KERNEL_ONE_LAUNCH)) return 0;
  if (in_dtype != RTI_F32 && in_dtype != RTI_U8 && in_dtype != RTI_I32) return 0;
  return rb_tile_pixels((int64_t)C * N, in_dtype);
}

template <typename SRC, typename T, int C, int TP, bool RESIDENT, bool ITER, int NL>
int launch_ps(const PsArgs<SRC>& a) {
  auto kern = ps_k<SRC, T, C, TP, RESIDENT, ITER, NL>;
  const StackView& in = a.in;
  const size_t lds = RESIDENT ? (size_t)C * in.N * TP * sizeof(T) : 0;
  if (lds > 64 * 1024 && reserve_lds(reinterpret_cast<const void*>(kern), lds) != hipSuccess)
    return fail(RTI_ERR_HIP, "%s: cannot reserve %zu bytes of LDS", a.entry, lds);
  hipLaunchKernelGGL(kern, dim3(grid_1d(in.P, TP)), dim3(TP), lds, a.s, a.src, in.N, static_cast<const T*>(in.I), in.P,
                     in.lstride, in.cstride, a.lo, a.hi, a.min_lights, a.iters, a.delta, a.w[0], a.w[1], a.w[2],
                     a.normals, a.albedo, a.kind, a.res, a.kept, a.fallback_px, a.vec);
  return check_launch(a.entry);
}

template <typename SRC, typename T, int C, int NL>
int launch_ps_form(const PsArgs<SRC>& a) {
  // the resident form runs only with iters > 0 (ps_plan)
  switch (a.tp) {
    case 256: return launch_ps<SRC, T, C, 256, true, true, NL>(a);
    case 128: return launch_ps<SRC, T, C, 128, true, true, NL>(a);
    case 64: return launch_ps<SRC, T, C, 64, true, true, NL>(a);
    default:
      return a.iters > 0 ? launch_ps<SRC, T, C, 256, false, true, NL>(a) : launch_ps<SRC, T, C, 256, false, false, NL>(a);
  }
}

template <typename SRC, typename T>
int launch_ps_c(const PsArgs<SRC>& a) {
  int st = RTI_OK;
  with_normal_layout(a.nl, [&](auto nl) {
    constexpr int NL = decltype(nl)::value;
    st = a.in.C == 3 ? launch_ps_form<SRC, T, 3, NL>(a) : launch_ps_form<SRC, T, 1, NL>(a);
  });
  return st;
}

// Everything both entries check and set after their own light arguments, in the order include/rti.h lists it for
// rti_photometric_stereo, then the launch.  `lights`: the entry's light array (A or the positions).
template <typename SRC>
int ps_run(const char* E, const SRC& src, const void* lights, int N, const void* I, int in_dtype, int64_t P, int C,
           int64_t light_stride, int64_t channel_stride, float lo, float hi, int min_lights, int iters, float delta,
           const float* w, float* normals, int normal_layout, float* albedo, uint8_t* kind, float* res, int32_t* kept,
           int* fallback_px, int kernel, rti_stream_t stream) {
  if (!kernel_bits_ok(kernel, RTI_KERNEL_AUTO, RTI_KERNEL_ONE_LAUNCH))
    return fail(RTI_ERR_BAD_ARG, "%s: unknown kernel bits 0x%x", E, kernel);
  if (int st = check_pointers(E, {lights, I, normals, albedo})) return st;
  if (N < 3 || P < 1) return fail(RTI_ERR_BAD_ARG, "%s: N=%d < 3 or P < 1", E, N);
  if (C != 1 && C != 3) return fail(RTI_ERR_UNSUPPORTED, "%s: C=%d (supported: 1, 3)", E, C);
  if (int st = check_in_dtype(E, in_dtype)) return st;
  if (!(lo <= hi)) return fail(RTI_ERR_BAD_ARG, "%s: window needs lo <= hi, neither NaN", E);
  if (min_lights < 3 || min_lights > N)
    return fail(RTI_ERR_BAD_ARG, "%s: min_lights=%d outside [3, N=%d]", E, min_lights, N);
  if (iters < 0 || iters > 16) return fail(RTI_ERR_BAD_ARG, "%s: iters=%d outside [0, 16]", E, iters);
  if (iters > 0 && !(delta > 0.0f)) return fail(RTI_ERR_BAD_ARG, "%s: delta must be > 0", E);
  if (int st = check_normal_layout(E, normal_layout)) return st;
  PsArgs<SRC> a{E, src, stack_view(I, in_dtype, N, P, C, light_stride, channel_stride), (double)lo, (double)hi,
                min_lights, iters, (double)delta};
  const float wdef[3] = {0.299f, 0.587f, 0.114f};
  for (int c = 0; c < 3; ++c) {
    a.w[c] = (double)(C == 3 && w ? w[c] : wdef[c]);  // read only when C == 3
    if (!std::isfinite(a.w[c])) return fail(RTI_ERR_BAD_ARG, "%s: non-finite weight", E);
  }
  if (int st = check_stack_strides(E, a.in)) return st;
  a.normals = normals, a.albedo = albedo, a.nl = normal_layout;
  a.kind = kind, a.res = res, a.kept = kept, a.fallback_px = fallback_px;
  a.tp = ps_plan(N, in_dtype, C, iters, kernel);
  // 16-byte tile loads: every plane of every tile starts on a 16-byte boundary (strides in bytes, any P)
  const int64_t es = (int64_t)a.in.es;
  a.vec = aligned_to(I, 16) && a.in.lstride * es % 16 == 0 && (C == 1 || a.in.cstride * es % 16 == 0);
  a.s = (hipStream_t)stream;
  note_launches(1);
  switch (in_dtype) {
    case RTI_F32: return launch_ps_c<SRC, float>(a);
    case RTI_U8: return launch_ps_c<SRC, uint8_t>(a);
    default: return launch_ps_c<SRC, int32_t>(a);
  }
}

}  // namespace ps_px
}  // namespace rti
