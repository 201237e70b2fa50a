// rti_rgb_px.h -- what the RGB PTM translation units share (rti_rgb8.hip from the 18 bytes of an 8-bit RGB PTM,
// rti_rgb.hip from three fp32 maps): the fp32 luminance of a pixel's three channels, rti_ptm_normals' function of
// it, and the luminance weights of the C entries.  Everything is __forceinline__ device code or a small host
// helper; moving it here changed no instruction of rti_rgb8.hip's kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "rti_internal.h"
#include "rti_ptm_px.h"

namespace rti {
namespace rgb_px {

constexpr int K = ptm_px::K;  // PTM-6

// three channels of a pixel -> the fp32 luminance map: two products and two sums, each rounded
__device__ __forceinline__ void luminance(const float (&c)[3][K], float wr, float wg, float wb, float (&l)[K]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const float rg = wr * c[0][j] + wg * c[1][j];
    l[j] = rg + wb * c[2][j];
  }
}

struct Weights {
  float r, g, b;
};

// three channels of a pixel -> what rti_ptm_normals writes for its fp32 luminance coefficients
__device__ __forceinline__ ptm_px::NormalOut normal_px(const float (&c)[3][K], const Weights& w, bool want_peak) {
  float l[K];
  luminance(c, w.r, w.g, w.b, l);
  double a[K];
#pragma unroll
  for (int j = 0; j < K; ++j) a[j] = (double)l[j];
  return ptm_px::normal_of(a, want_peak);
}

// the HOST argument w of the C entries: NULL means (0.299f, 0.587f, 0.114f)
inline int host_weights(const char* entry, const float* w, Weights& wt) {
  wt = Weights{w ? w[0] : 0.299f, w ? w[1] : 0.587f, w ? w[2] : 0.114f};
  if (!std::isfinite(wt.r) || !std::isfinite(wt.g) || !std::isfinite(wt.b))
    return fail(RTI_ERR_BAD_ARG, "%s: non-finite weight", entry);
  return RTI_OK;
}

}  // namespace rgb_px
}  // namespace rti
