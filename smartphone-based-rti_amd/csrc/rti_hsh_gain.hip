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
// Kernels, lane map, staging, output rows, launchers and the checks of the shared arguments: rti_hsh_render_px.h's,
// instantiated with the policy below as rti_hsh_specular.hip does with its own.  One pixel per lane; the
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

using namespace hsh_render;  // the chain, the kernel pair of a policy, Frame, check_frame and the launchers

struct Dir {
  double lu, lv;
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

// ---- the policy of rti_hsh_render_px.h's kernels, and its check ------------------------------------------------------

struct Gain {
  double gm1;  // g − 1
  struct Dirs {
    Dir d[MAXE];
  };
  static Dir dir(double lu, double lv) { return Dir{lu, lv}; }
  template <int C>
  struct Px {
    float A[C];
    bool bad;
  };
  template <int K, int C>
  __device__ __forceinline__ Px<C> prepare(const float (&c)[C][K], const float (&n)[3]) const {
    Px<C> px;
    anchors<K, C>(c, n, px.A);
    px.bad = n[0] != n[0] || n[1] != n[1] || n[2] != n[2];
    return px;
  }
  template <int K, int C, typename TO>
  __device__ __forceinline__ void value(const float (&c)[C][K], const float* __restrict__ b, const float (&)[3],
                                        const Px<C>& px, const Dir&, TO (&o)[C]) const {
    gain_value<K, C, TO>(c, b, px.A, px.bad, gm1, o);
  }
};

int check_gain(const char* entry, double gain) {
  if (!std::isfinite(gain)) return fail(RTI_ERR_BAD_ARG, "%s: non-finite gain", entry);
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
  Frame<Gain> a;
  if (int st = check_frame(E, P, normals, normal_layout, [&] { return check_gain(E, gain); }, Gain{gain - 1.0}, luv, E_,
                           out, out_dtype, stream, a))
    return st;
  note_launches(1);
  launch(k, coef, C, coef_layout, coef_channel_stride ? coef_channel_stride : P * k, a);
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
  Frame<Gain> a;
  if (int st = check_frame(E, P, normals, normal_layout, [&] { return check_gain(E, gain); }, Gain{gain - 1.0}, luv, E_,
                           out, out_dtype, stream, a))
    return st;
  note_launches(1);
  launch8(basis_terms(basis), coef8, qparams, a);
  return check_launch(E);
}
