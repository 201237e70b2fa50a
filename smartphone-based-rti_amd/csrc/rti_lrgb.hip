// rti_lrgb.hip -- LRGB PTMs (gfx950): the colour form of Malzbender, Gelb and Wolters (2001) and of every PTM
// viewer.  Six luminance coefficients and one RGB colour per pixel, rendered as rgb · L(lu, lv).
//
// The reference fits one channel (V of HSV); these semantics are build-defined and stated in include/rti.h and
// DESIGN.md §4.7.  PTM-6 only.
//
//     rti_lrgb_from_rgb   three PTM-6 maps (rti_fit_shared with C = 3) + the design's Gram matrix -> one LRGB map
//     rti_relight_lrgb    one LRGB map -> E interleaved RGB images
//     rti_relight_lrgb_enhanced   one LRGB map -> one diffuse gain or specular RGB image
//
// The least-squares colour needs no second pass over the stack: with G = AᵀA, a = Σ_c w_c·coef_c and the fitted
// luminance A_n·a at light n, the c that minimises Σ_n (I_c,n − c·A_n·a)² is (aᵀG·coef_c)/(aᵀG·a), because
// AᵀI_c = G·coef_c for a least-squares coef_c.  G and the weights travel as kernel arguments.
//
// Every per-pixel quantity is computed in fp64 from the fp32 maps with FP contraction off and rounded once to the
// output type.  Both kernels are streams with rti_relight's lane map: a lane owns 4 consecutive pixels, a wave
// 256, a block 1024.  Pixel-major rows (24 B of coefficients, 36 B of LRGB per pixel) come in as coalesced 1-KiB
// non-temporal wave loads parked in the wave's LDS slab (relight_eval_major's staging); planar maps as 16-byte
// loads per plane.  Pixel-major LRGB rows (144 B per lane) and fp32 / int32 RGB pixels (48 B per lane) leave
// through the same slab so that each store instruction writes one contiguous KiB; uint8 RGB is three dword stores
// per lane, as relight_frame_k's.  rti_relight_lrgb reads its map once and loops over the E directions inside the
// kernel (the PTM basis of a direction is three products, formed per wave from two uniform loads).
//
// A launch whose P is no multiple of 4 or whose pointers are not aligned for the vector accesses, and the last
// partial wave of any launch, take one pixel per lane (a wave still covers its 256 pixels, 64 at a time) through
// the same per-pixel functions, so the bits do not depend on the path.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "rti_basis.h"
#include "rti_convert.h"
#include "rti_dispatch.h"
#include "rti_enhance_px.h"
#include "rti_lane4.h"
#include "rti_lrgb_px.h"

namespace rti {
namespace {

using namespace lrgb_px;  // K, NL, dot6, rgb_of, shared with rti_lrgb8.hip
using namespace lane4;    // the wave loads, the staged row store and the RGB sink

// ---- per-pixel arithmetic (fp64, no contraction; tests/lrgb_ref.py restates it line by line) ------------------

struct Colour {
  double G[K][K];  // AᵀA of the shared design
  double w[3];     // channel weights of the luminance
};

// one pixel's three coefficient vectors -> (a0..a5, cR, cG, cB)
__device__ __forceinline__ void lrgb_of(const float (&xr)[K], const float (&xg)[K], const float (&xb)[K],
                                        const Colour& q, float (&o)[NL]) {
#pragma clang fp contract(off)
  double x[3][K];
  bool finite = true;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    x[0][i] = (double)xr[i];
    x[1][i] = (double)xg[i];
    x[2][i] = (double)xb[i];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < K; ++i) finite = finite && fabs(x[c][i]) <= DBL_MAX;  // false for NaN
  double a[K], t[K];
#pragma unroll
  for (int j = 0; j < K; ++j) a[j] = q.w[0] * x[0][j] + q.w[1] * x[1][j] + q.w[2] * x[2][j];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    double acc = q.G[i][0] * a[0];
#pragma unroll
    for (int j = 1; j < K; ++j) acc = acc + q.G[i][j] * a[j];
    t[i] = acc;
  }
  double d = a[0] * t[0];
#pragma unroll
  for (int i = 1; i < K; ++i) d = d + a[i] * t[i];
  const bool lit = d <= DBL_MAX && d > 0.0;  // false for NaN, inf and a black pixel
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double s = x[c][0] * t[0];
#pragma unroll
    for (int i = 1; i < K; ++i) s = s + x[c][i] * t[i];
    const double chroma = lit ? s / d : 1.0;
    o[K + c] = finite ? (float)chroma : NAN;
  }
#pragma unroll
  for (int j = 0; j < K; ++j) o[j] = finite ? (float)a[j] : NAN;
}

// dot6, rgb_of (the relight's per-pixel arithmetic): rti_lrgb_px.h

// ---- kernels ------------------------------------------------------------------------------------------------------
// Both: a wave owns pixels [wave_px, wave_px + 256).  vec != 0 (P % 4 == 0, every pointer aligned for its vector
// access) and the whole chunk inside the image: lane l owns pixels wave_px + 4l .. + 3.  Otherwise lane l takes
// pixels wave_px + 64j + l, j = 0..3, one at a time.

template <int CL, int OL>
__global__ void __launch_bounds__(256)
lrgb_from_rgb_k(const float* __restrict__ coef, int64_t cstride, int64_t P, int vec, Colour q,
                float* __restrict__ lrgb) {
  constexpr int SLAB = slab_v4(CL == RTI_COEF_PIXEL_MAJOR ? K : 0, OL == RTI_COEF_PIXEL_MAJOR ? NL : 0);
  __shared__ floatx4 slabs[4 * SLAB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 256;
  if (wave_px >= P) return;
  floatx4* slab = slabs + wave * SLAB;
  if (vec && wave_px + 256 <= P) {  // wave-uniform
    float x[3][4][K];
#pragma unroll
    for (int c = 0; c < 3; ++c) load_wave<K, CL>(coef + c * cstride, P, wave_px, lane, slab, x[c]);
    float o[4][NL];
#pragma unroll
    for (int v = 0; v < 4; ++v) lrgb_of(x[0][v], x[1][v], x[2][v], q, o[v]);
    if constexpr (OL == RTI_COEF_PIXEL_MAJOR) {
      store_rows_staged<NL>(lrgb + wave_px * NL, lane, slab, o);
    } else {
      const int64_t p0 = wave_px + 4 * lane;
#pragma unroll
      for (int i = 0; i < NL; ++i)
        *reinterpret_cast<floatx4*>(lrgb + (int64_t)i * P + p0) = floatx4{o[0][i], o[1][i], o[2][i], o[3][i]};
    }
    return;
  }
  for (int j = 0; j < 4; ++j) {
    const int64_t p = wave_px + 64 * j + lane;
    if (p >= P) break;
    float x[3][K], o[NL];
#pragma unroll
    for (int c = 0; c < 3; ++c) load_pixel<K, CL>(coef + c * cstride, P, p, x[c]);
    lrgb_of(x[0], x[1], x[2], q, o);
#pragma unroll
    for (int i = 0; i < NL; ++i) lrgb[OL == RTI_COEF_PLANAR ? (int64_t)i * P + p : p * NL + i] = o[i];
  }
}

template <int CL, typename TO>
__global__ void __launch_bounds__(256)
relight_lrgb_k(const float* __restrict__ lrgb, int64_t P, int vec, const double* __restrict__ luv, int E,
               TO* __restrict__ out) {
  constexpr int SLAB = slab_v4(CL == RTI_COEF_PIXEL_MAJOR ? NL : 0, rgb_staged<TO>() ? 3 : 0);
  __shared__ floatx4 slabs[4 * SLAB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 256;
  if (wave_px >= P) return;
  floatx4* slab = slabs + wave * SLAB;
  if (vec && wave_px + 256 <= P) {  // wave-uniform
    float m[4][NL];
    load_wave<NL, CL>(lrgb, P, wave_px, lane, slab, m);
    for (int e = 0; e < E; ++e) {
      double b[K];
      ptm_eval<double>(luv[2 * e], luv[2 * e + 1], b);
      TO o[4][3];
#pragma unroll
      for (int v = 0; v < 4; ++v) rgb_of<TO>(m[v], b, o[v]);
      TO* rows = out + ((int64_t)e * P + wave_px) * 3;
      if constexpr (rgb_staged<TO>()) {
        store_rows_staged<3, TO>(rows, lane, slab, o);
      } else {  // uint8: a lane's 12 bytes as three dwords, packed here: with store_rgb4 the pixel-major uint8
                // instantiation missed the A/B bound by 0.05 us (profiles/lane4_ab.json), so this body stays
        uint32_t* o4 = reinterpret_cast<uint32_t*>(rows + 12 * lane);
        const uint8_t* f = &o[0][0];
#pragma unroll
        for (int w = 0; w < 3; ++w)
          o4[w] = (uint32_t)f[4 * w] | ((uint32_t)f[4 * w + 1] << 8) | ((uint32_t)f[4 * w + 2] << 16) |
                  ((uint32_t)f[4 * w + 3] << 24);
      }
    }
    return;
  }
  for (int j = 0; j < 4; ++j) {
    const int64_t p = wave_px + 64 * j + lane;
    if (p >= P) break;
    float m[NL];
    load_pixel<NL, CL>(lrgb, P, p, m);
    for (int e = 0; e < E; ++e) {
      double b[K];
      ptm_eval<double>(luv[2 * e], luv[2 * e + 1], b);
      TO o[3];
      rgb_of<TO>(m, b, o);
      TO* px = out + ((int64_t)e * P + p) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) px[c] = o[c];
    }
  }
}

// rti_relight_lrgb's kernel with one direction and the enhanced luminance in place of the plain one
// (enhance_px::lrgb_enhanced)
template <int CL, typename TO, int MODE>
__global__ void __launch_bounds__(256)
relight_lrgb_enhanced_k(const float* __restrict__ lrgb, int64_t P, int vec, enhance_px::Enhance q,
                        TO* __restrict__ out) {
  constexpr int SLAB = slab_v4(CL == RTI_COEF_PIXEL_MAJOR ? NL : 0, rgb_staged<TO>() ? 3 : 0);
  __shared__ floatx4 slabs[4 * SLAB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 256;
  if (wave_px >= P) return;
  floatx4* slab = slabs + wave * SLAB;
  if (vec && wave_px + 256 <= P) {  // wave-uniform
    float m[4][NL];
    load_wave<NL, CL>(lrgb, P, wave_px, lane, slab, m);
    TO o[4][3];
#pragma unroll
    for (int v = 0; v < 4; ++v) enhance_px::lrgb_enhanced<MODE, TO>(m[v], q, o[v]);
    store_rgb4<TO>(out + wave_px * 3, lane, slab, o);
    return;
  }
  for (int j = 0; j < 4; ++j) {
    const int64_t p = wave_px + 64 * j + lane;
    if (p >= P) break;
    float m[NL];
    load_pixel<NL, CL>(lrgb, P, p, m);
    TO o[3];
    enhance_px::lrgb_enhanced<MODE, TO>(m, q, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[p * 3 + c] = o[c];
  }
}

int check_lrgb_layout(const char* entry, int layout) {
  if (layout != RTI_COEF_PIXEL_MAJOR && layout != RTI_COEF_PLANAR)
    return fail(RTI_ERR_BAD_ARG, "%s: lrgb layout %d", entry, layout);
  return RTI_OK;
}

}  // namespace
}  // namespace rti

using namespace rti;

extern "C" int rti_lrgb_from_rgb(const float* coef, int coef_layout, int64_t coef_channel_stride, int64_t P,
                                 const double* gram, const double* weights, float* lrgb, int lrgb_layout,
                                 rti_stream_t stream) {
  const char* const E = "rti_lrgb_from_rgb";
  if (int st = check_pointers(E, {coef, gram, lrgb})) return st;
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  if (int st = check_coef_layout(E, coef_layout)) return st;
  if (int st = check_lrgb_layout(E, lrgb_layout)) return st;
  const CoefSource src = coef_view(coef, coef_layout, K, P, coef_channel_stride);
  if (int st = check_coef_stride(E, src, P, 3)) return st;
  Colour q;
  for (int i = 0; i < K * K; ++i) {
    if (!std::isfinite(gram[i])) return fail(RTI_ERR_BAD_ARG, "%s: non-finite gram entry %d", E, i);
    q.G[i / K][i % K] = gram[i];
  }
  double wsum = 0.0;
  for (int c = 0; c < 3; ++c) {
    const double w = weights ? weights[c] : 1.0 / 3.0;
    if (!std::isfinite(w) || w < 0.0) return fail(RTI_ERR_BAD_ARG, "%s: weight %d is negative or not finite", E, c);
    q.w[c] = w;
    wsum += w;
  }
  if (!(wsum > 0.0)) return fail(RTI_ERR_BAD_ARG, "%s: the weights are all zero", E);
  const int vec = P % 4 == 0 && coef_vec_ok_any_c(src) && aligned_to(lrgb, 16) ? 1 : 0;
  with_layout(coef_layout, [&](auto cl) {
    with_layout(lrgb_layout, [&](auto ol) {
      launch(lrgb_from_rgb_k<decltype(cl)::value, decltype(ol)::value>, P, (hipStream_t)stream, coef, src.ocstride, P,
             vec, q, lrgb);
    });
  });
  return check_launch(E);
}

extern "C" int rti_relight_lrgb(const float* lrgb, int lrgb_layout, int64_t P, const double* luv, int E_, void* out,
                                int out_dtype, rti_stream_t stream) {
  const char* const E = "rti_relight_lrgb";
  if (int st = check_pointers(E, {lrgb, luv, out})) return st;
  if (P < 1 || E_ < 1) return fail(RTI_ERR_BAD_ARG, "%s: P and E must be positive", E);
  if (int st = check_lrgb_layout(E, lrgb_layout)) return st;
  if (int st = check_out_dtype(E, out_dtype)) return st;
  const int vec = P % 4 == 0 && aligned_to(lrgb, 16) && rgb_out_vec(out, out_dtype) ? 1 : 0;
  with_layout(lrgb_layout, [&](auto cl) {
    with_out(out_dtype, [&](auto t) {
      launch(relight_lrgb_k<decltype(cl)::value, decltype(t)>, P, (hipStream_t)stream, lrgb, P, vec, luv, E_, out);
    });
  });
  return check_launch(E);
}

extern "C" int rti_relight_lrgb_enhanced(const float* lrgb, int lrgb_layout, int64_t P, int mode, double gain,
                                         double kd, double ks, int spec_exp, double lu, double lv, void* out,
                                         int out_dtype, rti_stream_t stream) {
  const char* const E = "rti_relight_lrgb_enhanced";
  if (int st = check_pointers(E, {lrgb, out})) return st;
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  if (int st = check_lrgb_layout(E, lrgb_layout)) return st;
  if (int st = enhance_px::check_enhance(E, mode, gain, kd, ks, spec_exp, lu, lv)) return st;
  if (int st = check_out_dtype(E, out_dtype)) return st;
  const int vec = P % 4 == 0 && aligned_to(lrgb, 16) && rgb_out_vec(out, out_dtype) ? 1 : 0;
  const enhance_px::Enhance q = enhance_px::enhance_args(gain, kd, ks, spec_exp, lu, lv);
  note_launches(1);
  with_layout(lrgb_layout, [&](auto cl) {
    enhance_px::with_mode_out(mode, out_dtype, [&](auto m, auto t) {
      launch(relight_lrgb_enhanced_k<decltype(cl)::value, decltype(t), decltype(m)::value>, P, (hipStream_t)stream,
             lrgb, P, vec, q, out);
    });
  });
  return check_launch(E);
}
