// rti_enhance_px.h -- the enhanced renderings' per-pixel functions (Malzbender, Gelb, Wolters 2001: diffuse gain,
// specular enhancement), shared by the translation units that render them: rti_normals.hip (one grey PTM-6 map,
// rti_relight_enhanced) and the colour forms of DESIGN.md §4.12 (rti_lrgb.hip, rti_lrgb8.hip, rti_rgb8.hip).  The
// semantics are include/rti.h's; tests/normals_ref.py and tests/enhance_rgb_ref.py restate them line by line.
// Everything is __forceinline__ device code or a small host helper; moving the grey functions here changed no
// instruction of rti_normals.hip's kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "rti_convert.h"
#include "rti_dispatch.h"
#include "rti_internal.h"
#include "rti_ptm_px.h"
#include "rti_shade.h"

namespace rti {
namespace enhance_px {

// ---- per-pixel arithmetic (fp64, no contraction; ptm_value, ptm_peak and ptm_normal: rti_ptm_px.h) ------------

// diffuse gain g: the curvature of a scaled by g about the unprojected stationary point k, whose location and
// height stay; pixels without a maximum keep their coefficients.  k need not be a's own peak: the transform keeps
// the value and the gradient of a at (k.u0, k.v0) for any point, which is how a colour channel is rendered under
// its luminance's peak.
__device__ __forceinline__ double diffuse_gain_value(const double (&a)[ptm_px::K], const ptm_px::Peak& k, double g,
                                                     double lu, double lv) {
#pragma clang fp contract(off)
  constexpr int K = ptm_px::K;
  const double h = 1.0 - g, u0 = k.u0, v0 = k.v0;
  double b[K];
  b[0] = g * a[0];
  b[1] = g * a[1];
  b[2] = g * a[2];
  b[3] = h * (2.0 * a[0] * u0 + a[2] * v0) + a[3];
  b[4] = h * (2.0 * a[1] * v0 + a[2] * u0) + a[4];
  b[5] = h * (a[0] * (u0 * u0) + a[1] * (v0 * v0) + a[2] * u0 * v0) + (a[3] - b[3]) * u0 + (a[4] - b[4]) * v0 + a[5];
#pragma unroll
  for (int i = 0; i < K; ++i) b[i] = k.has_max ? b[i] : a[i];
  return k.finite ? ptm_px::ptm_value(b, lu, lv) : (double)NAN;
}

struct Enhance {
  double gain, kd, ks;
  int e;
  double lu, lv;
  double hx, hy, hz;  // the half vector between the light and the viewer (0, 0, 1), unit length
};

// the highlight of a pixel whose coefficients a peak at k: max(0, n·H)^e
__device__ __forceinline__ double highlight(const double (&a)[ptm_px::K], const ptm_px::Peak& k, const Enhance& q) {
#pragma clang fp contract(off)
  double n[3];
  ptm_px::ptm_normal(a, k, n);
  const double c = n[0] * q.hx + n[1] * q.hy + n[2] * q.hz;
  return powi(c > 0.0 ? c : 0.0, q.e);
}

template <int MODE>
__device__ __forceinline__ double enhanced_value(const double (&a)[ptm_px::K], const Enhance& q) {
#pragma clang fp contract(off)
  const ptm_px::Peak k = ptm_px::ptm_peak(a);
  if constexpr (MODE == RTI_ENHANCE_DIFFUSE_GAIN) {
    return diffuse_gain_value(a, k, q.gain, q.lu, q.lv);
  } else {
    const double v = q.kd * ptm_px::ptm_value(a, q.lu, q.lv) + q.ks * highlight(a, k, q);
    return k.finite ? v : (double)NAN;
  }
}

// ---- the colour forms ---------------------------------------------------------------------------
// Both take the peak and the normal from a luminance vector l and write one RGB pixel, converted once.  A pixel
// whose l is not finite is NaN in its three channels.

// LRGB: the enhanced luminance under the pixel's chroma; the highlight is white.  With chroma 1 a channel is
// enhanced_value of l.
template <int MODE, typename TO>
__device__ __forceinline__ void lrgb_enhanced(const float (&m)[ptm_px::K + 3], const Enhance& q, TO (&o)[3]) {
#pragma clang fp contract(off)
  constexpr int K = ptm_px::K;
  double l[K];
#pragma unroll
  for (int i = 0; i < K; ++i) l[i] = (double)m[i];
  const ptm_px::Peak k = ptm_px::ptm_peak(l);
  if constexpr (MODE == RTI_ENHANCE_DIFFUSE_GAIN) {
    const double G = diffuse_gain_value(l, k, q.gain, q.lu, q.lv);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = cvt_out<TO>((double)m[K + c] * G);
  } else {
    const double D = ptm_px::ptm_value(l, q.lu, q.lv);
    const double S = q.ks * highlight(l, k, q);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v = q.kd * ((double)m[K + c] * D) + S;
      o[c] = cvt_out<TO>(k.finite ? v : (double)NAN);
    }
  }
}

// RGB: every channel's own coefficients under the luminance's peak (no fringes: the three channels move their
// curvature about one point) and the luminance's white highlight.  Where l equals a channel, that channel is
// enhanced_value of it.
template <int MODE, typename TO>
__device__ __forceinline__ void rgb_enhanced(const float (&c)[3][ptm_px::K], const float (&lum)[ptm_px::K],
                                             const Enhance& q, TO (&o)[3]) {
#pragma clang fp contract(off)
  constexpr int K = ptm_px::K;
  double l[K];
#pragma unroll
  for (int i = 0; i < K; ++i) l[i] = (double)lum[i];
  const ptm_px::Peak k = ptm_px::ptm_peak(l);
  double S = 0.0;
  if constexpr (MODE == RTI_ENHANCE_SPECULAR) S = q.ks * highlight(l, k, q);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    double a[K];
#pragma unroll
    for (int i = 0; i < K; ++i) a[i] = (double)c[ch][i];
    if constexpr (MODE == RTI_ENHANCE_DIFFUSE_GAIN) {
      o[ch] = cvt_out<TO>(diffuse_gain_value(a, k, q.gain, q.lu, q.lv));
    } else {
      const double v = q.kd * ptm_px::ptm_value(a, q.lu, q.lv) + S;
      o[ch] = cvt_out<TO>(k.finite ? v : (double)NAN);
    }
  }
}

// ---- the argument contract of the enhanced entries (host) --------------------------------------------------------

// mode, light, gain, kd, ks and spec_exp, in the order include/rti.h lists them
inline int check_enhance(const char* entry, int mode, double gain, double kd, double ks, int spec_exp, double lu,
                         double lv) {
  if (mode != RTI_ENHANCE_DIFFUSE_GAIN && mode != RTI_ENHANCE_SPECULAR)
    return fail(RTI_ERR_BAD_ARG, "%s: mode %d", entry, mode);
  if (!std::isfinite(lu) || !std::isfinite(lv)) return fail(RTI_ERR_BAD_ARG, "%s: non-finite light direction", entry);
  if (!std::isfinite(gain) || !std::isfinite(kd) || !std::isfinite(ks))
    return fail(RTI_ERR_BAD_ARG, "%s: non-finite gain, kd or ks", entry);
  if (gain < 0.0) return fail(RTI_ERR_BAD_ARG, "%s: gain %g < 0", entry, gain);
  if (mode == RTI_ENHANCE_SPECULAR && (spec_exp < 1 || spec_exp > 255))
    return fail(RTI_ERR_BAD_ARG, "%s: spec_exp %d outside [1, 255]", entry, spec_exp);
  return RTI_OK;
}

// the kernel argument: the half vector is wave-uniform, so light_frame forms it here
inline Enhance enhance_args(double gain, double kd, double ks, int spec_exp, double lu, double lv) {
  const LightFrame f = light_frame(lu, lv);
  return Enhance{gain, kd, ks, spec_exp, lu, lv, f.hx, f.hy, f.hz};
}

// f(mode tag, TO{}) for a checked mode and out_dtype: f is a generic lambda that launches the kernel instantiated
// on decltype of its arguments
template <typename F>
inline void with_mode_out(int mode, int out_dtype, F&& f) {
  auto out = [&](auto m) { with_out(out_dtype, [&](auto t) { f(m, t); }); };
  if (mode == RTI_ENHANCE_SPECULAR)
    out(Tag<RTI_ENHANCE_SPECULAR>{});
  else
    out(Tag<RTI_ENHANCE_DIFFUSE_GAIN>{});
}

}  // namespace enhance_px
}  // namespace rti
