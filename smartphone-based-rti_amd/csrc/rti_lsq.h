// rti_lsq.h -- device helpers shared by the fp64 fits and the residual stream (rti_fitres.hip, rti_fit_accum.hip,
// rti_residual.hip): the non-temporal lane load and the wavefront sum.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rti_internal.h"

namespace rti {

// VEC consecutive T as one non-temporal load, widened to D (D = T: as loaded, for a caller that converts itself)
template <typename D, typename T, int VEC>
__device__ __forceinline__ void load_nt(const T* __restrict__ p, D (&x)[VEC]) {
  if constexpr (VEC == 1) {
    x[0] = (D)__builtin_nontemporal_load(p);
  } else {
    typedef T vec_t __attribute__((ext_vector_type(VEC)));
    const vec_t v = __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(p));
#pragma unroll
    for (int i = 0; i < VEC; ++i) x[i] = (D)v[i];
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

}  // namespace rti
