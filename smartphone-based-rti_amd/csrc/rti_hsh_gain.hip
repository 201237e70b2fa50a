// rti_hsh_gain.hip -- diffuse gain for HSH maps under a normal map (gfx950).
//
//     rti_relight_hsh_gain    one or three fp32 HSH maps + a normal map -> E images
//     rti_relight_hsh8_gain   the bytes of an .rti file + a normal map  -> E interleaved RGB images
//
// Diffuse gain keeps a pixel's value at its peak direction and multiplies the fall-off away from it by g:
// L'(l) = L(l) + (g − 1)·(L(l) − L(l0)).  For a PTM that is Malzbender's transform of the six coefficients; in this
// form it names no curvature, so it holds for any basis once the peak direction l0 is known, and for an HSH map that
// is the normal map these entries read (rti_hsh_normals, once per object), as rti_relight_hsh_specular does.  Per
// pixel and channel the value is include/rti.h's: V = rti_relight's F32 value at the light, A = the same F32 value at
// the pixel's own (n_x, n_y) -- hsh_eval<float> at a per-pixel direction, once per pixel and launch -- and
// V + gm1·(V − A) in fp64 without contraction, converted once.
//
// Lane map, staging and output rows: rti_hsh_specular.hip's (rti_hsh_render_px.h).  One pixel per lane; the
// coefficients or bytes and the normal are read once for all E directions, the C anchors are formed once, the E basis
// rows of the lights once per workgroup in LDS.  Every path runs anchors and gain_value, so the bits do not depend
// on it.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rti_basis.h"
#include "rti_convert.h"
#include "rti_dispatch.h"
#include "rti_hsh_render_px.h"
#include "rti_stack.h"

namespace rti {
namespace {

using namespace hsh_render;  // the chain, the slab runs, the basis rows, the normal and the output rows

struct Dir {
  double lu, lv;
};
struct Dirs {
  Dir d[MAXE];
};

// ---- the per-pixel functions -------------------------------------------------------------------------------------
// A_c: rti_relight's F32 value of each channel at the pixel's own direction (n_x, n_y), the fp32 components as they
// are (hsh_eval clamps outside the disc).  Three square roots and two divisions per pixel and launch.
template <int K, int C>
__device__ __forceinline__ void anchors(const float (&c)[C][K], const float (&n)[3], float (&A)[C]) {
  float b[K];
  hsh_eval<float>(n[0], n[1], K, b);  // basis_eval<float>'s HSH branch
#pragma unroll
  for (int ch = 0; ch < C; ++ch) A[ch] = dot_k<K>(c[ch], b);
}

// C channels of one pixel at one direction: b the light's basis row.  A NaN normal component gives NaN.
template <int K, int C, typename TO>
__device__ __forceinline__ void gain_value(const float (&c)[C][K], const float* __restrict__ b, const float (&A)[C],
                                           bool bad, double gm1, TO (&o)[C]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    const double V = (double)dot_k<K>(c[ch], b);
    const double d = V - (double)A[ch];
    const double v = V + gm1 * d;
    o[ch] = cvt_out<TO>(bad ? (double)NAN : v);
  }
}

// the anchors, then the wave's 64 pixels at every direction
template <int K, int C, typename TO>
__device__ __forceinline__ void render_gain(const float (&c)[C][K], const float (&n)[3], const float* __restrict__ btab,
                                            int E, double gm1, int64_t P, int64_t wave_px, int lane, bool live,
                                            bool vout, u32x4* __restrict__ slab, TO* __restrict__ out) {
  float A[C];
  anchors<K, C>(c, n, A);
  const bool bad = n[0] != n[0] || n[1] != n[1] || n[2] != n[2];
  render<C, TO>(E, P, wave_px, lane, live, vout, slab, out,
                [&](int e, TO (&o)[C]) { gain_value<K, C, TO>(c, btab + e * K, A, bad, gm1, o); });
}

// ---- kernels ------------------------------------------------------------------------------------------------------
// Both: wave w of workgroup g owns pixels [(4g + w)·64, + 64).  vin / vn / vout: the coefficient run, the normal run
// and the output rows may move as whole pieces (the entry's alignment checks).

template <int K, typename TO>
__global__ void __launch_bounds__(256)
relight_hsh8_gain_k(const uint8_t* __restrict__ coef8, int64_t P, int vin, const float* __restrict__ qparams,
                    const float* __restrict__ normals, int nl, int vn, int vout, double gm1, Dirs dirs, int E,
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
  render_gain<K, 3, TO>(c, n, btab, E, gm1, P, wave_px, lane, live, vout && full, slab, out);
}

template <int K, int C, int CL, typename TO>
__global__ void __launch_bounds__(256)
relight_hsh_gain_k(const float* __restrict__ coef, int64_t cs, int64_t P, int vin, const float* __restrict__ normals,
                   int nl, int vn, int vout, double gm1, Dirs dirs, int E, TO* __restrict__ out) {
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
  render_gain<K, C, TO>(c, n, btab, E, gm1, P, wave_px, lane, live, vout && full, slab, out);
}

// ---- launchers and checks -----------------------------------------------------------------------------------------

// what a launch takes besides its coefficients
struct Frame {
  int64_t P;
  const float* normals;
  int nl, vn, vout;
  double gm1;
  Dirs dirs;
  int E;
  void* out;
  hipStream_t s;
};

template <int K>
void launch8(const uint8_t* coef8, int vin, const float* qparams, const Frame& a, int out_dtype) {
  with_out(out_dtype, [&](auto t) {
    using TO = decltype(t);
    hipLaunchKernelGGL((relight_hsh8_gain_k<K, TO>), dim3(grid_1d(a.P, CHUNK)), dim3(256), 0, a.s, coef8, a.P, vin,
                       qparams, a.normals, a.nl, a.vn, a.vout, a.gm1, a.dirs, a.E, static_cast<TO*>(a.out));
  });
}

template <int K, int C, int CL>
void launch_t(const float* coef, int64_t cs, int vin, const Frame& a, int out_dtype) {
  with_out(out_dtype, [&](auto t) {
    using TO = decltype(t);
    hipLaunchKernelGGL((relight_hsh_gain_k<K, C, CL, TO>), dim3(grid_1d(a.P, CHUNK)), dim3(256), 0, a.s, coef, cs, a.P,
                       vin, a.normals, a.nl, a.vn, a.vout, a.gm1, a.dirs, a.E, static_cast<TO*>(a.out));
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
int check_frame(const char* entry, int64_t P, const float* normals, int normal_layout, double gain, const double* luv,
                int E, void* out, int out_dtype, Frame& a) {
  if (int st = check_normal_layout(entry, normal_layout)) return st;
  if (!std::isfinite(gain)) return fail(RTI_ERR_BAD_ARG, "%s: non-finite gain", entry);
  if (E < 1 || E > MAXE) return fail(RTI_ERR_BAD_ARG, "%s: E = %d outside [1, %d]", entry, E, MAXE);
  for (int i = 0; i < 2 * E; ++i)
    if (!std::isfinite(luv[i])) return fail(RTI_ERR_BAD_ARG, "%s: non-finite light direction", entry);
  if (int st = check_out_dtype(entry, out_dtype)) return st;
  a.P = P;
  a.normals = normals;
  a.nl = normal_layout;
  a.vn = normals_staged(normals, normal_layout);
  a.vout = rows_as_dwords(out, out_dtype, P);
  a.gm1 = gain - 1.0;
  for (int i = 0; i < E; ++i) a.dirs.d[i] = Dir{luv[2 * i], luv[2 * i + 1]};
  a.E = E;
  a.out = out;
  return RTI_OK;
}

}  // namespace
}  // namespace rti

using namespace rti;

extern "C" int rti_relight_hsh_gain(const float* coef, int basis, int coef_layout, int C, int64_t coef_channel_stride,
                                    int64_t P, const float* normals, int normal_layout, double gain, const double* luv,
                                    int E_, void* out, int out_dtype, rti_stream_t stream) {
  const char* const E = "rti_relight_hsh_gain";
  if (int st = check_pointers(E, {coef, normals, luv, out})) return st;
  if (!hsh_basis(basis))
    return fail(RTI_ERR_UNSUPPORTED, "%s: basis %d (HSH-9 and HSH-16 only; PTM-6 has rti_relight_rgb_enhanced)", E, basis);
  if (int st = check_coef_layout(E, coef_layout)) return st;
  if (C != 1 && C != 3) return fail(RTI_ERR_BAD_ARG, "%s: C = %d (one map or three)", E, C);
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  const int k = basis_terms(basis);
  if (int st = check_coef_stride(E, coef_view(coef, coef_layout, k, P, coef_channel_stride), P, C)) return st;
  Frame a{};  // directions past E stay zero
  if (int st = check_frame(E, P, normals, normal_layout, gain, luv, E_, out, out_dtype, a)) return st;
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

extern "C" int rti_relight_hsh8_gain(const uint8_t* coef8, int basis, int64_t P, const float* qparams,
                                     const float* normals, int normal_layout, double gain, const double* luv, int E_,
                                     void* out, int out_dtype, rti_stream_t stream) {
  const char* const E = "rti_relight_hsh8_gain";
  if (int st = check_pointers(E, {coef8, qparams, normals, luv, out})) return st;
  if (!hsh_basis(basis))
    return fail(RTI_ERR_UNSUPPORTED, "%s: basis %d (HSH-9 and HSH-16 only; PTM-6 has rti_relight_rgb8_enhanced)", E, basis);
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  if (!aligned_to(qparams, 4)) return fail(RTI_ERR_BAD_ARG, "%s: qparams must be 4-byte aligned", E);
  Frame a{};  // directions past E stay zero
  if (int st = check_frame(E, P, normals, normal_layout, gain, luv, E_, out, out_dtype, a)) return st;
  a.s = (hipStream_t)stream;
  const int vin = aligned_to(coef8, 16) ? 1 : 0;
  note_launches(1);
  if (basis == RTI_BASIS_HSH9)
    launch8<9>(coef8, vin, qparams, a, out_dtype);
  else
    launch8<16>(coef8, vin, qparams, a, out_dtype);
  return check_launch(E);
}
