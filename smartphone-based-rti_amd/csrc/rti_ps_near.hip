// rti_ps_near.hip -- near-light photometric stereo: a light position per light, a design row per pixel (gfx950).
//
// rti_photometric_stereo takes one direction and one strength per light for the whole image.  A phone flash a few
// image widths from the object is neither: the direction to it and, by the inverse square of the distance, its
// strength change from pixel to pixel.  Here every lane forms the row of its own pixel from the light's position
// (wave-uniform, scalar loads) and the pixel's (lane-private: x and y from the linear index, z from a height map),
// anew in every pass of the fit: N·3 doubles per pixel fit neither a lane's registers nor the LDS tile, and the row
// costs less than reading it back would (ps_px::PsNearRows: three subtractions, the squared norm, the fp64 rsq seed
// with two Newton steps, and the scalings).
//
// The fit, the tail, the outputs, the forms and their plan rule are rti_photometric_stereo's: one kernel template
// (rti_ps_px.h) with the light source as its argument.
#include <cmath>
#include <cstdint>

#include "rti_ps_px.h"

using namespace rti;

extern "C" int rti_photometric_stereo_near_plan(int N, int in_dtype, int C, int iters, int kernel) {
  return ps_px::ps_plan(N, in_dtype, C, iters, kernel);
}

extern "C" int rti_photometric_stereo_near(const double* lights, int N, const void* I, int in_dtype, int H, int W, int C,
                                           int64_t light_stride, int64_t channel_stride, double x0, double y0,
                                           const float* height, double z_offset, int falloff, double r0, float lo,
                                           float hi, int min_lights, int iters, float delta, const float* w,
                                           float* normals, int normal_layout, float* albedo, uint8_t* kind, float* res,
                                           int32_t* kept, int* fallback_px, int kernel, rti_stream_t stream) {
  const char* const E = "rti_photometric_stereo_near";
  if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31))
    return fail(RTI_ERR_BAD_ARG, "%s: H=%d or W=%d < 1, or H*W >= 2^31", E, H, W);
  if (falloff != 0 && falloff != 1) return fail(RTI_ERR_BAD_ARG, "%s: falloff=%d outside {0, 1}", E, falloff);
  if (falloff == 1 && !(std::isfinite(r0) && r0 > 0.0)) return fail(RTI_ERR_BAD_ARG, "%s: r0 must be finite and > 0", E);
  if (!std::isfinite(x0) || !std::isfinite(y0) || !std::isfinite(z_offset))
    return fail(RTI_ERR_BAD_ARG, "%s: non-finite x0, y0 or z_offset", E);
  const ps_px::PsNearSrc src{lights, height, x0, y0, z_offset, falloff ? r0 * r0 : 1.0, W, falloff};
  return ps_px::ps_run(E, src, lights, N, I, in_dtype, (int64_t)H * W, C, light_stride, channel_stride, lo, hi,
                       min_lights, iters, delta, w, normals, normal_layout, albedo, kind, res, kept, fallback_px, kernel,
                       stream);
}
