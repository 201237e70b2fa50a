// rti_ps.hip -- photometric stereo: robust Lambertian normals and albedo straight from the stack (gfx950).
//
// The Lambertian model I_n = g·l_n fitted per pixel to the samples themselves, with the samples it cannot describe
// (attached shadow, clipped highlight) left out: n = g/‖g‖ is the surface normal and ‖g‖ the albedo.  This is the
// normal map RTI users know from RTIBuilder and Relight; rti_ptm_normals and rti_hsh_normals read theirs off a
// fitted function instead and inherit what shadows and highlights did to that fit.
//
// Per channel and pixel the fit is rti_fit_shared_robust's at k = 3 on the design (lu, lv, lw): the templates of
// rti_robust_px.h as they stand (window, Cholesky with the pivot rule, fallback to every light, Huber IRLS), which
// leave g_c in fp64.  One lane owns one pixel with all its C channels, one channel after the other, so the shared
// normal of an RGB pixel needs no second launch: g = Σ w_c g_c, n = g/‖g‖, albedo_c = g_c·n (ps_tail, fp64
// without contraction), rounded once to fp32.  The rows of A are wave-uniform.
//
// The kernel, its two forms (streaming and LDS-resident, the same bits) and the argument checks are rti_ps_px.h's,
// shared with rti_ps_near.hip; this file supplies the shared design as the light source.
#include <cmath>
#include <cstdint>

#include "rti_ps_px.h"

using namespace rti;

extern "C" int rti_ps_design(const float* lu, const float* lv, int n, double* A) {
  if (!lu || !lv || !A || n <= 0) return fail(RTI_ERR_BAD_ARG, "rti_ps_design: null pointer or n <= 0");
  for (int i = 0; i < n; ++i) {
    const double u = lu[i], v = lv[i];  // the squares of fp32 values are exact in fp64
    A[3 * i] = u;
    A[3 * i + 1] = v;
    A[3 * i + 2] = std::sqrt(std::fmax(0.0, 1.0 - u * u - v * v));
  }
  return RTI_OK;
}

extern "C" int rti_photometric_stereo_plan(int N, int in_dtype, int C, int iters, int kernel) {
  return ps_px::ps_plan(N, in_dtype, C, iters, kernel);
}

extern "C" int rti_photometric_stereo(const double* A, int N, const void* I, int in_dtype, int64_t P, int C,
                                      int64_t light_stride, int64_t channel_stride, float lo, float hi,
                                      int min_lights, int iters, float delta, const float* w, float* normals,
                                      int normal_layout, float* albedo, uint8_t* kind, float* res, int32_t* kept,
                                      int* fallback_px, int kernel, rti_stream_t stream) {
  return ps_px::ps_run("rti_photometric_stereo", ps_px::PsFarSrc{A}, A, N, I, in_dtype, P, C, light_stride,
                       channel_stride, lo, hi, min_lights, iters, delta, w, normals, normal_layout, albedo, kind, res,
                       kept, fallback_px, kernel, stream);
}
