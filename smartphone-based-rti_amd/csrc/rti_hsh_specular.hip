// rti_hsh_specular.hip -- specular enhancement of HSH maps under a normal map (gfx950).
//
//     rti_relight_hsh_specular    one or three fp32 HSH maps + a normal map -> E images
//     rti_relight_hsh8_specular   the bytes of an .rti file + a normal map  -> E interleaved RGB images
//
// An HSH map has no closed-form peak (rti_hsh_normals searches for it, once per object), so these entries read a
// normal map instead of recomputing the normal per frame as rti_relight_enhanced does.  Per pixel, channel and
// direction the value is include/rti.h's: V = rti_relight's F32 value (hsh_px::dot_k of the basis row that
// hsh_eval<float> forms), S = ks·powi(max(0, n·H), spec_exp) in fp64, kd·V + S in fp64 without contraction,
// converted once.  The half vectors are formed on the host (light_frame) and travel with the directions as one
// kernel argument, so a call copies and allocates nothing.
//
// Lane map: rti_hsh8.hip's.  One pixel per lane, a wave owns 64 consecutive pixels, a workgroup 256.  A full wave
// moves its contiguous run of bytes, of a pixel-major channel's rows and of pixel-major normals (64 x 12 B) as
// whole 16-byte pieces through its LDS slab, and its output elements leave through the slab as whole dwords.
// Planar maps and normals are read per lane, coalesced as they are.  Anything the pieces cannot serve (a pointer
// off its alignment, uint8 output with P % 4 != 0, the last partial wave) loads and stores per lane; every path
// runs specular_value, so the bits do not depend on it.  The coefficients or bytes and the normal are read once
// for all E directions; the E basis rows are formed once per workgroup in LDS.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rti_basis.h"
#include "rti_convert.h"
#include "rti_dispatch.h"
#include "rti_hsh_render_px.h"
#include "rti_shade.h"
#include "rti_stack.h"

namespace rti {
namespace {

using namespace hsh_render;  // the chain, the slab runs, the basis rows, the normal and the output rows

// a direction and its half vector, formed on the host in fp64 (light_frame)
struct Dir {
  double lu, lv;
  double hx, hy, hz;
};
struct Dirs {
  Dir d[MAXE];
};
struct Spec {
  double kd, ks;
  int e;
};

// ---- the per-pixel function ------------------------------------------------------------------------------------
// C channels of one pixel at one direction: b its basis row, n the pixel's normal.  The highlight is white: one S
// for the C channels.  A NaN normal component gives NaN whatever ks is.
template <int K, int C, typename TO>
__device__ __forceinline__ void specular_value(const float (&c)[C][K], const float* __restrict__ b,
                                               const float (&n)[3], const Dir& d, const Spec& q, TO (&o)[C]) {
#pragma clang fp contract(off)
  const double nx = (double)n[0], ny = (double)n[1], nz = (double)n[2];
  const double h = nx * d.hx + ny * d.hy + nz * d.hz;
  const double S = q.ks * powi(h > 0.0 ? h : 0.0, q.e);
  const bool bad = nx != nx || ny != ny || nz != nz;
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    const double v = q.kd * (double)dot_k<K>(c[ch], b) + S;
    o[ch] = cvt_out<TO>(bad ? (double)NAN : v);
  }
}

// ---- kernels ------------------------------------------------------------------------------------------------------
// Both: wave w of workgroup g owns pixels [(4g + w)·64, + 64).  vin / vn / vout: the coefficient run, the normal run
// and the output rows may move as whole pieces (the entry's alignment checks).

template <int K, typename TO>
__global__ void __launch_bounds__(256)
relight_hsh8_specular_k(const uint8_t* __restrict__ coef8, int64_t P, int vin, const float* __restrict__ qparams,
                        const float* __restrict__ normals, int nl, int vn, int vout, Spec q, Dirs dirs, int E,
                        TO* __restrict__ out) {
  constexpr int NB = 3 * K, NW = (NB + 3) / 4;
  constexpr int SLAB = render_slab(run_v4<NB>());
  __shared__ u32x4 slabs[4 * SLAB];
  __shared__ float btab[MAXE * K];
  __shared__ float qs[2 * K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32x4* slab = slabs + wave * SLAB;
  load_steps<K>(qparams, qs);
  fill_basis<K>(dirs, E, btab);
  __syncthreads();
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 64;
  if (wave_px >= P) return;  // wave-uniform; no workgroup barrier below
  const int64_t p = wave_px + lane;
  const bool live = p < P, full = wave_px + 64 <= P;  // full: wave-uniform
  uint32_t w[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) w[i] = 0;
  if (vin && full) {
    run_in<NB>(coef8 + wave_px * NB, lane, slab);
    lane_words<NB>(slab, lane, w);
  } else if (live) {
#pragma unroll
    for (int i = 0; i < NB; ++i) w[i >> 2] |= (uint32_t)coef8[p * NB + i] << (8 * (i & 3));
  }
  float c[3][K];
  dequantise_px<K>(w, qs, c);
  float n[3];
  load_normal(normals, nl, vn && full, P, wave_px, lane, live, slab, n);
  render<3, TO>(E, P, wave_px, lane, live, vout && full, slab, out,
                [&](int e, TO (&o)[3]) { specular_value<K, 3, TO>(c, btab + e * K, n, dirs.d[e], q, o); });
}

template <int K, int C, int CL, typename TO>
__global__ void __launch_bounds__(256)
relight_hsh_specular_k(const float* __restrict__ coef, int64_t cs, int64_t P, int vin,
                       const float* __restrict__ normals, int nl, int vn, int vout, Spec q, Dirs dirs, int E,
                       TO* __restrict__ out) {
  constexpr int SLAB = render_slab(CL == RTI_COEF_PIXEL_MAJOR ? run_v4<4 * K>() : 0);
  __shared__ u32x4 slabs[4 * SLAB];
  __shared__ float btab[MAXE * K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32x4* slab = slabs + wave * SLAB;
  fill_basis<K>(dirs, E, btab);
  __syncthreads();
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 64;
  if (wave_px >= P) return;  // wave-uniform; no workgroup barrier below
  const int64_t p = wave_px + lane;
  const bool live = p < P, full = wave_px + 64 <= P;  // full: wave-uniform
  float c[C][K];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    const float* map = coef + ch * cs;
    if (CL == RTI_COEF_PIXEL_MAJOR && vin && full) {  // wave-uniform: the wave's 64 rows of the channel are one run
      run_in<4 * K>(map + wave_px * K, lane, slab);
      uint32_t w[K];
      lane_words<4 * K>(slab, lane, w);
#pragma unroll
      for (int j = 0; j < K; ++j) c[ch][j] = __uint_as_float(w[j]);
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j)
        c[ch][j] = !live ? 0.f : CL == RTI_COEF_PLANAR ? map[(int64_t)j * P + p] : map[p * K + j];
    }
  }
  float n[3];
  load_normal(normals, nl, vn && full, P, wave_px, lane, live, slab, n);
  render<C, TO>(E, P, wave_px, lane, live, vout && full, slab, out,
               [&](int e, TO (&o)[C]) { specular_value<K, C, TO>(c, btab + e * K, n, dirs.d[e], q, o); });
}

// ---- launchers and checks -----------------------------------------------------------------------------------------

// what a launch takes besides its coefficients
struct Frame {
  int64_t P;
  const float* normals;
  int nl, vn, vout;
  Spec q;
  Dirs dirs;
  int E;
  void* out;
  hipStream_t s;
};

template <int K>
void launch8(const uint8_t* coef8, int vin, const float* qparams, const Frame& a, int out_dtype) {
  with_out(out_dtype, [&](auto t) {
    using TO = decltype(t);
    hipLaunchKernelGGL((relight_hsh8_specular_k<K, TO>), dim3(grid_1d(a.P, CHUNK)), dim3(256), 0, a.s, coef8, a.P, vin,
                       qparams, a.normals, a.nl, a.vn, a.vout, a.q, a.dirs, a.E, static_cast<TO*>(a.out));
  });
}

template <int K, int C, int CL>
void launch_t(const float* coef, int64_t cs, int vin, const Frame& a, int out_dtype) {
  with_out(out_dtype, [&](auto t) {
    using TO = decltype(t);
    hipLaunchKernelGGL((relight_hsh_specular_k<K, C, CL, TO>), dim3(grid_1d(a.P, CHUNK)), dim3(256), 0, a.s, coef, cs,
                       a.P, vin, a.normals, a.nl, a.vn, a.vout, a.q, a.dirs, a.E, static_cast<TO*>(a.out));
  });
}

template <int K, int C>
void launch_cl(const float* coef, int layout, int64_t cs, int vin, const Frame& a, int out_dtype) {
  if (layout == RTI_COEF_PLANAR)
    launch_t<K, C, RTI_COEF_PLANAR>(coef, cs, vin, a, out_dtype);
  else
    launch_t<K, C, RTI_COEF_PIXEL_MAJOR>(coef, cs, vin, a, out_dtype);
}

template <int K>
void launch_c(const float* coef, int C, int layout, int64_t cs, int vin, const Frame& a, int out_dtype) {
  if (C == 1)
    launch_cl<K, 1>(coef, layout, cs, vin, a, out_dtype);
  else
    launch_cl<K, 3>(coef, layout, cs, vin, a, out_dtype);
}

// the checks the two entries share after their coefficients, in the order include/rti.h lists the arguments (E
// before the values of luv it counts); fills everything of `a` but the stream
int check_frame(const char* entry, int64_t P, const float* normals, int normal_layout, double kd, double ks,
                int spec_exp, const double* luv, int E, void* out, int out_dtype, Frame& a) {
  if (int st = check_normal_layout(entry, normal_layout)) return st;
  if (!std::isfinite(kd) || !std::isfinite(ks)) return fail(RTI_ERR_BAD_ARG, "%s: non-finite kd or ks", entry);
  if (spec_exp < 1 || spec_exp > 255)
    return fail(RTI_ERR_BAD_ARG, "%s: spec_exp %d outside [1, 255]", entry, spec_exp);
  if (E < 1 || E > MAXE) return fail(RTI_ERR_BAD_ARG, "%s: E = %d outside [1, %d]", entry, E, MAXE);
  for (int i = 0; i < 2 * E; ++i)
    if (!std::isfinite(luv[i])) return fail(RTI_ERR_BAD_ARG, "%s: non-finite light direction", entry);
  if (int st = check_out_dtype(entry, out_dtype)) return st;
  a.P = P;
  a.normals = normals;
  a.nl = normal_layout;
  a.vn = normals_staged(normals, normal_layout);
  a.vout = rows_as_dwords(out, out_dtype, P);
  a.q = Spec{kd, ks, spec_exp};
  for (int i = 0; i < E; ++i) {
    const LightFrame f = light_frame(luv[2 * i], luv[2 * i + 1]);
    a.dirs.d[i] = Dir{f.lu, f.lv, f.hx, f.hy, f.hz};
  }
  a.E = E;
  a.out = out;
  return RTI_OK;
}

}  // namespace
}  // namespace rti

using namespace rti;

extern "C" int rti_relight_hsh_specular(const float* coef, int basis, int coef_layout, int C,
                                        int64_t coef_channel_stride, int64_t P, const float* normals,
                                        int normal_layout, double kd, double ks, int spec_exp, const double* luv,
                                        int E_, void* out, int out_dtype, rti_stream_t stream) {
  const char* const E = "rti_relight_hsh_specular";
  if (int st = check_pointers(E, {coef, normals, luv, out})) return st;
  if (!hsh_basis(basis))
    return fail(RTI_ERR_UNSUPPORTED, "%s: basis %d (HSH-9 and HSH-16 only; PTM-6 has rti_relight_rgb_enhanced)", E, basis);
  if (int st = check_coef_layout(E, coef_layout)) return st;
  if (C != 1 && C != 3) return fail(RTI_ERR_BAD_ARG, "%s: C = %d (one map or three)", E, C);
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  const int k = basis_terms(basis);
  if (int st = check_coef_stride(E, coef_view(coef, coef_layout, k, P, coef_channel_stride), P, C)) return st;
  Frame a{};  // directions past E stay zero
  if (int st = check_frame(E, P, normals, normal_layout, kd, ks, spec_exp, luv, E_, out, out_dtype, a)) return st;
  a.s = (hipStream_t)stream;
  const int64_t cs = coef_channel_stride ? coef_channel_stride : P * k;
  const int vin = maps_staged(coef, coef_layout, C, cs);
  note_launches(1);
  if (k == 9)
    launch_c<9>(coef, C, coef_layout, cs, vin, a, out_dtype);
  else
    launch_c<16>(coef, C, coef_layout, cs, vin, a, out_dtype);
  return check_launch(E);
}

extern "C" int rti_relight_hsh8_specular(const uint8_t* coef8, int basis, int64_t P, const float* qparams,
                                         const float* normals, int normal_layout, double kd, double ks,
                                         int spec_exp, const double* luv, int E_, void* out, int out_dtype,
                                         rti_stream_t stream) {
  const char* const E = "rti_relight_hsh8_specular";
  if (int st = check_pointers(E, {coef8, qparams, normals, luv, out})) return st;
  if (!hsh_basis(basis))
    return fail(RTI_ERR_UNSUPPORTED, "%s: basis %d (HSH-9 and HSH-16 only; PTM-6 has rti_relight_rgb8_enhanced)", E, basis);
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  if (!aligned_to(qparams, 4)) return fail(RTI_ERR_BAD_ARG, "%s: qparams must be 4-byte aligned", E);
  Frame a{};  // directions past E stay zero
  if (int st = check_frame(E, P, normals, normal_layout, kd, ks, spec_exp, luv, E_, out, out_dtype, a)) return st;
  a.s = (hipStream_t)stream;
  const int vin = aligned_to(coef8, 16) ? 1 : 0;
  note_launches(1);
  if (basis == RTI_BASIS_HSH9)
    launch8<9>(coef8, vin, qparams, a, out_dtype);
  else
    launch8<16>(coef8, vin, qparams, a, out_dtype);
  return check_launch(E);
}
