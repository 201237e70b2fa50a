// rti_ptm_px.h -- rti_ptm_normals' per-pixel function, shared by the translation units that compute PTM normals
// (rti_normals.hip from fp32 / fp64 coefficient maps, rti_rgb8.hip from the 18 bytes of an 8-bit RGB PTM): the
// stationary point of the biquadratic, the normal and its kind, the peak value.  The semantics are include/rti.h's
// (DESIGN.md §4.5); tests/normals_ref.py restates them line by line.  Everything is __forceinline__ device code;
// moving it here changed no instruction of rti_normals.hip's kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

namespace rti {
namespace ptm_px {

constexpr int K = 6;  // PTM-6

// ---- per-pixel arithmetic (fp64, no contraction; tests/normals_ref.py restates it line by line) --------------

// L(u, v), the six terms summed left to right as rti_relight's fp64 path does
__device__ __forceinline__ double ptm_value(const double (&a)[K], double u, double v) {
#pragma clang fp contract(off)
  double acc = a[0] * (u * u);
  acc = acc + a[1] * (v * v);
  acc = acc + a[2] * (u * v);
  acc = acc + a[3] * u;
  acc = acc + a[4] * v;
  return acc + a[5];
}

struct Peak {
  double u0, v0, r2;  // the stationary point and its squared radius (meaningful with has_max)
  bool finite;        // every coefficient is finite
  bool has_max;       // finite, D > 1e-6·S and a0 < 0
};

__device__ __forceinline__ Peak ptm_peak(const double (&a)[K]) {
#pragma clang fp contract(off)
  Peak k;
  k.finite = true;
#pragma unroll
  for (int i = 0; i < K; ++i) k.finite = k.finite && fabs(a[i]) <= DBL_MAX;  // false for NaN
  const double a22 = a[2] * a[2];
  const double D = 4.0 * a[0] * a[1] - a22;
  const double S = a[0] * a[0] + a[1] * a[1] + 0.5 * a22;
  k.has_max = k.finite && D > 1e-6 * S && a[0] < 0.0;
  k.u0 = (a[2] * a[4] - 2.0 * a[1] * a[3]) / D;
  k.v0 = (a[2] * a[3] - 2.0 * a[0] * a[4]) / D;
  k.r2 = k.u0 * k.u0 + k.v0 * k.v0;
  return k;
}

// the normal and the pixel's kind: 0 interior maximum, 1 maximum outside the unit disc (scaled radially onto
// its edge), 2 no maximum (the Lambertian reading of the linear terms), 4 non-finite (NaN)
__device__ __forceinline__ int ptm_normal(const double (&a)[K], const Peak& k, double (&n)[3]) {
#pragma clang fp contract(off)
  const bool inside = k.has_max && k.r2 <= 1.0;
  const bool outside = k.has_max && !inside;
  const double g2 = a[5] > 0.0 ? a[5] : 0.0;
  const double gg = a[3] * a[3] + a[4] * a[4] + g2 * g2;
  const double s = sqrt(inside ? 1.0 - k.r2 : outside ? k.r2 : gg);
  const bool flat = !k.has_max && s == 0.0;  // ‖g‖ = 0 -> (0, 0, 1)
  const double nx = k.has_max ? k.u0 : a[3];
  const double ny = k.has_max ? k.v0 : a[4];
  const double nz = inside ? s : outside ? 0.0 : g2;
  const double den = (inside || flat) ? 1.0 : s;
  n[0] = (flat ? 0.0 : nx) / den;
  n[1] = (flat ? 0.0 : ny) / den;
  n[2] = (flat ? 1.0 : nz) / den;
  if (!k.finite) n[0] = n[1] = n[2] = NAN;
  return !k.finite ? 4 : inside ? 0 : outside ? 1 : 2;
}

// ---- what rti_ptm_normals writes for a pixel ------------------------------------------------------------------

struct NormalOut {
  float n[3];
  float peak;
  uint8_t kind;
};

__device__ __forceinline__ NormalOut normal_of(const double (&a)[K], bool want_peak) {
  double n[3];
  const int kind = ptm_normal(a, ptm_peak(a), n);
  NormalOut o;
  o.n[0] = (float)n[0];
  o.n[1] = (float)n[1];
  o.n[2] = (float)n[2];
  o.kind = (uint8_t)kind;
  o.peak = want_peak ? (float)(kind == 4 ? (double)NAN : ptm_value(a, n[0], n[1])) : 0.f;
  return o;
}

}  // namespace ptm_px
}  // namespace rti
