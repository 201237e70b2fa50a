// rti_normals.hip -- what a fitted PTM says about the surface (gfx950): per-pixel normals and the
// enhanced renderings built on them (Malzbender, Gelb, Wolters 2001: diffuse gain, specular enhancement).
//
// The reference stops at the relit value (analysis.py:300-315, interactive_relighting.py:25-38); these
// semantics are build-defined and stated in include/rti.h and DESIGN.md §4.5.  PTM-6 only: the biquadratic
//     L(u, v) = a0·u² + a1·v² + a2·u·v + a3·u + a4·v + a5
// has a closed-form stationary point, HSH has none.
//
//     rti_ptm_normals        coefficients -> normal [3], kind, peak value
//     rti_relight_enhanced   coefficients -> one image at (lu, lv): diffuse gain or specular enhancement
//
// Every per-pixel quantity is computed in fp64 from the fp32 / fp64 coefficients with FP contraction off and
// rounded once to the output type: D = 4·a0·a1 − a2² cancels badly in fp32.  The branches (interior maximum,
// maximum outside the disc, no maximum, non-finite) are selects: a wave sees every kind.  The one square root
// and the three divisions of the normal are shared by the kinds (x/1 is exact), so a pixel costs five fp64
// divisions and one square root whatever its kind.
//
// Both kernels are streams with rti_relight's lane map: a lane owns 4 consecutive pixels, a wave 256, a block
// 1024.  Pixel-major coefficient rows come in as coalesced 1-KiB wave loads parked in the wave's LDS slab
// (relight_eval_major's staging); planar maps as 16-byte loads per plane.  Pixel-major normals (12 B per
// pixel) leave through the same slab so that each store instruction writes one contiguous KiB (the VM_STAGE
// idea of rti_fit.hip).  rti_relight_enhanced reads no normal map: it recomputes the peak from the
// coefficients and moves the 4k + 4 = 28 B per pixel of a one-direction rti_relight.
//
// A launch whose P is no multiple of 4 or whose pointers are not aligned for the vector accesses, and the
// last partial wave of any launch, take one pixel per lane (a wave still covers its 256 pixels, 64 at a
// time) through the same per-pixel functions, so the bits do not depend on the path.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "rti_convert.h"
#include "rti_dispatch.h"
#include "rti_enhance_px.h"
#include "rti_lane4.h"
#include "rti_ptm_px.h"
#include "rti_stack.h"

namespace rti {
namespace {

using namespace ptm_px;      // K = 6 and rti_ptm_normals' per-pixel function, shared with rti_rgb8.hip
using namespace enhance_px;  // rti_relight_enhanced's, shared with the colour forms
typedef double doublex2 __attribute__((ext_vector_type(2)));

using lane4::wave_lds_sync;

// ---- per-pixel arithmetic: ptm_value, ptm_peak and ptm_normal in rti_ptm_px.h; diffuse_gain_value, Enhance and
// enhanced_value in rti_enhance_px.h, shared with the colour forms

// ---- coefficient loads ------------------------------------------------------------------------------------------

// LDS per wave in 16-byte units: the coefficient staging slab and / or the pixel-major normals' 3 KiB
template <typename TC, int CL, bool STAGE_OUT>
constexpr int slab_v4() {
  const int in = CL == RTI_COEF_PIXEL_MAJOR ? 64 * K * (int)sizeof(TC) / 4 : 0;
  const int out = STAGE_OUT ? 64 * 3 : 0;
  return in > out ? in : (out > 0 ? out : 1);
}

// Pixel-major coefficient rows through LDS: relight_eval_major's load_coef_staged (rti_relight.hip), restated.
// It is a copy because bench.py hashes rti_relight.hip and rti_convert.h to decide whether
// profiles/traffic.json is stale, so neither file can grow a shared header's include.  The wave reads its 256
// pixels' rows as PIECES coalesced 1-KiB non-temporal loads (lane l, piece j: bytes 16·(64·j + l) of the
// chunk), parks them in its slab and reads back its own 4 pixels' rows.
template <typename TC>
__device__ __forceinline__ void load_rows_staged(const TC* __restrict__ coef, int64_t wave_px, int lane,
                                                 floatx4* __restrict__ slab, double (&a)[4][K]) {
  constexpr int PIECES = K * (int)sizeof(TC) / 4;  // 16-B pieces per lane: 6 (fp32) or 12 (fp64)
  const floatx4* g = reinterpret_cast<const floatx4*>(coef + wave_px * K);
  floatx4 t[PIECES];
#pragma unroll
  for (int j = 0; j < PIECES; ++j) t[j] = __builtin_nontemporal_load(g + j * 64 + lane);
#pragma unroll
  for (int j = 0; j < PIECES; ++j) slab[j * 64 + lane] = t[j];
  wave_lds_sync();
  union {
    floatx4 v[PIECES];
    TC c[4][K];
  } u;
#pragma unroll
  for (int j = 0; j < PIECES; ++j) u.v[j] = slab[lane * PIECES + j];
#pragma unroll
  for (int v = 0; v < 4; ++v)
#pragma unroll
    for (int i = 0; i < K; ++i) a[v][i] = (double)u.c[v][i];
}

// planar maps: a lane's 4 pixels of one plane are 16 (fp32) or 32 (fp64) contiguous bytes
template <typename TC>
__device__ __forceinline__ void load_planes(const TC* __restrict__ coef, int64_t P, int64_t p0, double (&a)[4][K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const TC* src = coef + (int64_t)i * P + p0;
    if constexpr (std::is_same<TC, float>::value) {
      const floatx4 t = __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(src));
#pragma unroll
      for (int v = 0; v < 4; ++v) a[v][i] = (double)t[v];
    } else {
      const doublex2 lo = __builtin_nontemporal_load(reinterpret_cast<const doublex2*>(src));
      const doublex2 hi = __builtin_nontemporal_load(reinterpret_cast<const doublex2*>(src) + 1);
      a[0][i] = lo[0];
      a[1][i] = lo[1];
      a[2][i] = hi[0];
      a[3][i] = hi[1];
    }
  }
}

template <typename TC, int CL>
__device__ __forceinline__ void load_wave(const TC* __restrict__ coef, int64_t P, int64_t wave_px, int lane,
                                          floatx4* __restrict__ slab, double (&a)[4][K]) {
  if constexpr (CL == RTI_COEF_PIXEL_MAJOR)
    load_rows_staged<TC>(coef, wave_px, lane, slab, a);
  else
    load_planes<TC>(coef, P, wave_px + 4 * lane, a);
}

template <typename TC, int CL>
__device__ __forceinline__ void load_pixel(const TC* __restrict__ coef, int64_t P, int64_t p, double (&a)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) a[i] = (double)(CL == RTI_COEF_PLANAR ? coef[(int64_t)i * P + p] : coef[p * K + i]);
}

// ---- kernels --------------------------------------------------------------------------------------------------
// Both: a wave owns pixels [wave_px, wave_px + 256).  vec != 0 (P % 4 == 0, every pointer aligned for its vector
// access) and the whole chunk inside the image: lane l owns pixels wave_px + 4l .. + 3.  Otherwise lane l takes
// pixels wave_px + 64j + l, j = 0..3, one at a time.

template <typename TC, int CL, int NL>
__global__ void __launch_bounds__(256)
ptm_normals_k(const TC* __restrict__ coef, int64_t P, int vec, float* __restrict__ normals, uint8_t* __restrict__ kind,
              float* __restrict__ peak) {
  constexpr bool STAGE_OUT = NL == RTI_NORMAL_PIXEL_MAJOR;
  constexpr int SLAB = slab_v4<TC, CL, STAGE_OUT>();
  __shared__ floatx4 slabs[4 * SLAB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 256;
  if (wave_px >= P) return;
  floatx4* slab = slabs + wave * SLAB;
  if (vec && wave_px + 256 <= P) {  // wave-uniform
    const int64_t p0 = wave_px + 4 * lane;
    double a[4][K];
    load_wave<TC, CL>(coef, P, wave_px, lane, slab, a);
    NormalOut o[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) o[v] = normal_of(a[v], peak != nullptr);
    if (kind)
      *reinterpret_cast<uint32_t*>(kind + p0) = (uint32_t)o[0].kind | ((uint32_t)o[1].kind << 8) |
                                                ((uint32_t)o[2].kind << 16) | ((uint32_t)o[3].kind << 24);
    if (peak) *reinterpret_cast<floatx4*>(peak + p0) = floatx4{o[0].peak, o[1].peak, o[2].peak, o[3].peak};
    if constexpr (STAGE_OUT) {
      // a lane's 48 B would be three stores strided 48 B across the wave: the wave's 3 KiB go through its slab
      // (every lane has read its coefficient rows back by now) and leave as three contiguous 1-KiB stores
      wave_lds_sync();
      slab[lane * 3 + 0] = floatx4{o[0].n[0], o[0].n[1], o[0].n[2], o[1].n[0]};
      slab[lane * 3 + 1] = floatx4{o[1].n[1], o[1].n[2], o[2].n[0], o[2].n[1]};
      slab[lane * 3 + 2] = floatx4{o[2].n[2], o[3].n[0], o[3].n[1], o[3].n[2]};
      wave_lds_sync();
      floatx4* g = reinterpret_cast<floatx4*>(normals + wave_px * 3);
#pragma unroll
      for (int j = 0; j < 3; ++j) g[j * 64 + lane] = slab[j * 64 + lane];
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i)
        *reinterpret_cast<floatx4*>(normals + (int64_t)i * P + p0) = floatx4{o[0].n[i], o[1].n[i], o[2].n[i], o[3].n[i]};
    }
    return;
  }
  for (int j = 0; j < 4; ++j) {
    const int64_t p = wave_px + 64 * j + lane;
    if (p >= P) break;
    double a[K];
    load_pixel<TC, CL>(coef, P, p, a);
    const NormalOut o = normal_of(a, peak != nullptr);
#pragma unroll
    for (int i = 0; i < 3; ++i) normals[NL == RTI_NORMAL_PLANAR ? (int64_t)i * P + p : p * 3 + i] = o.n[i];
    if (kind) kind[p] = o.kind;
    if (peak) peak[p] = o.peak;
  }
}

template <typename TC, int CL, typename TO, int MODE>
__global__ void __launch_bounds__(256)
relight_enhanced_k(const TC* __restrict__ coef, int64_t P, int vec, Enhance q, TO* __restrict__ out) {
  constexpr int SLAB = slab_v4<TC, CL, false>();
  __shared__ floatx4 slabs[4 * SLAB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 256;
  if (wave_px >= P) return;
  if (vec && wave_px + 256 <= P) {  // wave-uniform
    double a[4][K];
    load_wave<TC, CL>(coef, P, wave_px, lane, slabs + wave * SLAB, a);
    typedef TO vec_t __attribute__((ext_vector_type(4)));
    vec_t o;
#pragma unroll
    for (int v = 0; v < 4; ++v) o[v] = cvt_out<TO>(enhanced_value<MODE>(a[v], q));
    *reinterpret_cast<vec_t*>(out + wave_px + 4 * lane) = o;
    return;
  }
  for (int j = 0; j < 4; ++j) {
    const int64_t p = wave_px + 64 * j + lane;
    if (p >= P) break;
    double a[K];
    load_pixel<TC, CL>(coef, P, p, a);
    out[p] = cvt_out<TO>(enhanced_value<MODE>(a, q));
  }
}

// ---- checks --------------------------------------------------------------------------------------------------

// the checks the two entries share, in the order include/rti.h documents them
int check_ptm_map(const char* entry, int64_t P, int coef_layout) {
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", entry);
  return check_coef_layout(entry, coef_layout);
}

int check_ptm_types(const char* entry, int basis, int coef_dtype) {
  if (basis != RTI_BASIS_PTM6)
    return fail(RTI_ERR_UNSUPPORTED, "%s: basis %d (PTM-6 only: HSH has no closed-form maximum)", entry, basis);
  if (coef_dtype != RTI_F32 && coef_dtype != RTI_F64) return fail(RTI_ERR_UNSUPPORTED, "%s: coef dtype %d", entry, coef_dtype);
  return RTI_OK;
}

}  // namespace
}  // namespace rti

using namespace rti;

extern "C" int rti_ptm_normals(const void* coef, int coef_dtype, int basis, int coef_layout, int64_t P, float* normals,
                               int normal_layout, uint8_t* kind, float* peak, rti_stream_t stream) {
  const char* const E = "rti_ptm_normals";
  if (int st = check_pointers(E, {coef, normals})) return st;
  if (int st = check_ptm_map(E, P, coef_layout)) return st;
  if (int st = check_normal_layout(E, normal_layout)) return st;
  if (int st = check_ptm_types(E, basis, coef_dtype)) return st;
  const int vec = P % 4 == 0 && aligned_to(coef, 16) && normals_out_vec(normals, kind, peak) ? 1 : 0;
  with_coef_dtype(coef_dtype, [&](auto c) {
    with_layout(coef_layout, [&](auto cl) {
      with_normal_layout(normal_layout, [&](auto nl) {
        lane4::launch(ptm_normals_k<decltype(c), decltype(cl)::value, decltype(nl)::value>, P, (hipStream_t)stream, coef,
                      P, vec, normals, kind, peak);
      });
    });
  });
  return check_launch(E);
}

extern "C" int rti_relight_enhanced(const void* coef, int coef_dtype, int basis, int coef_layout, int64_t P, int mode,
                                    double gain, double kd, double ks, int spec_exp, double lu, double lv, void* out,
                                    int out_dtype, rti_stream_t stream) {
  const char* const E = "rti_relight_enhanced";
  if (int st = check_pointers(E, {coef, out})) return st;
  if (int st = check_ptm_map(E, P, coef_layout)) return st;
  if (int st = check_enhance(E, mode, gain, kd, ks, spec_exp, lu, lv)) return st;
  if (int st = check_ptm_types(E, basis, coef_dtype)) return st;
  if (int st = check_out_dtype(E, out_dtype)) return st;
  const int vec = P % 4 == 0 && aligned_to(coef, 16) && rgb_out_vec(out, out_dtype) ? 1 : 0;
  const Enhance q = enhance_args(gain, kd, ks, spec_exp, lu, lv);
  with_coef_dtype(coef_dtype, [&](auto c) {
    with_layout(coef_layout, [&](auto cl) {
      with_mode_out(mode, out_dtype, [&](auto m, auto t) {
        lane4::launch(relight_enhanced_k<decltype(c), decltype(cl)::value, decltype(t), decltype(m)::value>, P,
                      (hipStream_t)stream, coef, P, vec, q, out);
      });
    });
  });
  return check_launch(E);
}
