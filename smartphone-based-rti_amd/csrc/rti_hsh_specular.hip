// rti_hsh_specular.hip -- specular enhancement of HSH maps under a normal map (gfx950).
//
//     rti_relight_hsh_specular    one or three fp32 HSH maps + a normal map -> E images
//     rti_relight_hsh8_specular   the bytes of an .rti file + a normal map  -> E interleaved RGB images
//
// An HSH map has no closed-form peak (rti_hsh_normals searches for it, once per object), so these entries read a
// normal map instead of recomputing the normal per frame as rti_relight_enhanced does.  Per pixel, channel and
// direction the value is include/rti.h's: V = rti_relight's F32 value (hsh_px::dot_k of the basis row that
// hsh_eval<float> forms), S = ks·powi(max(0, n·H), spec_exp) in fp64, kd·V + S in fp64 without contraction,
// converted once.  The half vectors are formed on the host (light_frame) and travel with the directions as one
// kernel argument, so a call copies and allocates nothing.
//
// The kernels, their launchers and the checks of the shared arguments are rti_hsh_render_px.h's, instantiated with
// the policy below; rti_hsh_gain.hip is the other one.
// Lane map: rti_hsh8.hip's.  One pixel per lane, a wave owns 64 consecutive pixels, a workgroup 256.  A full wave
// moves its contiguous run of bytes, of a pixel-major channel's rows and of pixel-major normals (64 x 12 B) as
// whole 16-byte pieces through its LDS slab, and its output elements leave through the slab as whole dwords.
// Planar maps and normals are read per lane, coalesced as they are.  Anything the pieces cannot serve (a pointer
// off its alignment, uint8 output with P % 4 != 0, the last partial wave) loads and stores per lane; every path
// runs specular_value, so the bits do not depend on it.  The coefficients or bytes and the normal are read once
// for all E directions; the E basis rows are formed once per workgroup in LDS.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rti_basis.h"
#include "rti_convert.h"
#include "rti_dispatch.h"
#include "rti_hsh_render_px.h"
#include "rti_shade.h"
#include "rti_stack.h"

namespace rti {
namespace {

using namespace hsh_render;  // the chain, the kernel pair of a policy, Frame, check_frame and the launchers

// a direction and its half vector, formed on the host in fp64 (light_frame)
struct Dir {
  double lu, lv;
  double hx, hy, hz;
};
struct Spec {
  double kd, ks;
  int e;
};

// ---- the per-pixel function ------------------------------------------------------------------------------------
// C channels of one pixel at one direction: b its basis row, n the pixel's normal.  The highlight is white: one S
// for the C channels.  A NaN normal component gives NaN whatever ks is.
template <int K, int C, typename TO>
__device__ __forceinline__ void specular_value(const float (&c)[C][K], const float* __restrict__ b,
                                               const float (&n)[3], const Dir& d, const Spec& q, TO (&o)[C]) {
#pragma clang fp contract(off)
  const double nx = (double)n[0], ny = (double)n[1], nz = (double)n[2];
  const double h = nx * d.hx + ny * d.hy + nz * d.hz;
  const double S = q.ks * powi(h > 0.0 ? h : 0.0, q.e);
  const bool bad = nx != nx || ny != ny || nz != nz;
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    const double v = q.kd * (double)dot_k<K>(c[ch], b) + S;
    o[ch] = cvt_out<TO>(bad ? (double)NAN : v);
  }
}

// ---- the policy of rti_hsh_render_px.h's kernels, and its checks -----------------------------------------------------

struct Specular {
  Spec q;
  struct Dirs {
    Dir d[MAXE];
  };
  static Dir dir(double lu, double lv) {
    const LightFrame f = light_frame(lu, lv);
    return Dir{f.lu, f.lv, f.hx, f.hy, f.hz};
  }
  struct Px {};  // nothing per pixel: the highlight depends on the direction
  template <int K, int C>
  __device__ __forceinline__ Px prepare(const float (&)[C][K], const float (&)[3]) const { return {}; }
  template <int K, int C, typename TO>
  __device__ __forceinline__ void value(const float (&c)[C][K], const float* __restrict__ b, const float (&n)[3],
                                        const Px&, const Dir& d, TO (&o)[C]) const {
    specular_value<K, C, TO>(c, b, n, d, q, o);
  }
};

int check_spec(const char* entry, double kd, double ks, int spec_exp) {
  if (!std::isfinite(kd) || !std::isfinite(ks)) return fail(RTI_ERR_BAD_ARG, "%s: non-finite kd or ks", entry);
  if (spec_exp < 1 || spec_exp > 255)
    return fail(RTI_ERR_BAD_ARG, "%s: spec_exp %d outside [1, 255]", entry, spec_exp);
  return RTI_OK;
}

}  // namespace
}  // namespace rti

using namespace rti;

extern "C" int rti_relight_hsh_specular(const float* coef, int basis, int coef_layout, int C,
                                        int64_t coef_channel_stride, int64_t P, const float* normals,
                                        int normal_layout, double kd, double ks, int spec_exp, const double* luv,
                                        int E_, void* out, int out_dtype, rti_stream_t stream) {
  const char* const E = "rti_relight_hsh_specular";
  if (int st = check_pointers(E, {coef, normals, luv, out})) return st;
  if (!hsh_basis(basis))
    return fail(RTI_ERR_UNSUPPORTED, "%s: basis %d (HSH-9 and HSH-16 only; PTM-6 has rti_relight_rgb_enhanced)", E, basis);
  if (int st = check_coef_layout(E, coef_layout)) return st;
  if (C != 1 && C != 3) return fail(RTI_ERR_BAD_ARG, "%s: C = %d (one map or three)", E, C);
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  const int k = basis_terms(basis);
  if (int st = check_coef_stride(E, coef_view(coef, coef_layout, k, P, coef_channel_stride), P, C)) return st;
  Frame<Specular> a;
  if (int st = check_frame(E, P, normals, normal_layout, [&] { return check_spec(E, kd, ks, spec_exp); },
                           Specular{Spec{kd, ks, spec_exp}}, luv, E_, out, out_dtype, stream, a))
    return st;
  note_launches(1);
  launch(k, coef, C, coef_layout, coef_channel_stride ? coef_channel_stride : P * k, a);
  return check_launch(E);
}

extern "C" int rti_relight_hsh8_specular(const uint8_t* coef8, int basis, int64_t P, const float* qparams,
                                         const float* normals, int normal_layout, double kd, double ks,
                                         int spec_exp, const double* luv, int E_, void* out, int out_dtype,
                                         rti_stream_t stream) {
  const char* const E = "rti_relight_hsh8_specular";
  if (int st = check_pointers(E, {coef8, qparams, normals, luv, out})) return st;
  if (!hsh_basis(basis))
    return fail(RTI_ERR_UNSUPPORTED, "%s: basis %d (HSH-9 and HSH-16 only; PTM-6 has rti_relight_rgb8_enhanced)", E, basis);
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  if (!aligned_to(qparams, 4)) return fail(RTI_ERR_BAD_ARG, "%s: qparams must be 4-byte aligned", E);
  Frame<Specular> a;
  if (int st = check_frame(E, P, normals, normal_layout, [&] { return check_spec(E, kd, ks, spec_exp); },
                           Specular{Spec{kd, ks, spec_exp}}, luv, E_, out, out_dtype, stream, a))
    return st;
  note_launches(1);
  launch8(basis_terms(basis), coef8, qparams, a);
  return check_launch(E);
}
