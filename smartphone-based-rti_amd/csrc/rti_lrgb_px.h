// rti_lrgb_px.h -- what the LRGB translation units share (rti_lrgb.hip, rti_lrgb8.hip): the per-pixel relight
// arithmetic.  The lane map, the loads and the stores around it are rti_lane4.h's.  Everything is __forceinline__
// device code; moving it here changed no instruction of rti_lrgb.hip's kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rti_convert.h"
#include "rti_internal.h"

namespace rti {
namespace lrgb_px {

constexpr int K = 6;   // PTM-6
constexpr int NL = 9;  // floats of an LRGB pixel: a0..a5, cR, cG, cB

// ---- per-pixel arithmetic (fp64, no contraction; tests/lrgb_ref.py restates it line by line) ------------------

// rti_relight's dot_k<6>(double): the six products summed left to right, every one rounded
__device__ __forceinline__ double dot6(const double (&c)[K], const double (&b)[K]) {
#pragma clang fp contract(off)
  double acc = c[0] * b[0];
#pragma unroll
  for (int k = 1; k < K; ++k) acc = acc + c[k] * b[k];
  return acc;
}

// one LRGB pixel at the basis row b -> its three channels, converted once
template <typename TO>
__device__ __forceinline__ void rgb_of(const float (&m)[NL], const double (&b)[K], TO (&o)[3]) {
#pragma clang fp contract(off)
  double a[K];
#pragma unroll
  for (int i = 0; i < K; ++i) a[i] = (double)m[i];
  const double L = dot6(a, b);
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = cvt_out<TO>((double)m[K + c] * L);
}

}  // namespace lrgb_px
}  // namespace rti
