// rti_shade.h -- what the shading entries share (rti_relight_enhanced's specular mode, rti_shade_normals):
// the integer power and the light and half vectors of a direction (lu, lv), as include/rti.h states them.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace rti {

// x^e, 1 <= e <= 255, by repeated squaring (e is wave-uniform); no pow
__device__ __forceinline__ double powi(double x, int e) {
#pragma clang fp contract(off)
  double r = 1.0, b = x;
  for (;;) {
    if (e & 1) r = r * b;
    e >>= 1;
    if (!e) return r;
    b = b * b;
  }
}

// the light (lu, lv, lw), lw = sqrt(max(0, 1 − lu² − lv²)), and the unit half vector between it and the viewer
// (0, 0, 1): wave-uniform, so formed once on the host in fp64
struct LightFrame {
  double lu, lv, lw;
  double hx, hy, hz;
};

inline LightFrame light_frame(double lu, double lv) {
  const double lw2 = 1.0 - lu * lu - lv * lv;
  const double lw = lw2 > 0.0 ? std::sqrt(lw2) : 0.0;
  const double hz = lw + 1.0;
  const double hn = std::sqrt(lu * lu + lv * lv + hz * hz);
  return {lu, lv, lw, lu / hn, lv / hn, hz / hn};
}

}  // namespace rti
