// rti_rgb.hip -- three fp32 RGB maps rendered in one pass (gfx950): what rti_fit_shared writes for a colour stack
// (C = 3), read once per launch.
//
//     rti_relight_rgb            PTM-6 / HSH-9 / HSH-16 maps -> E interleaved RGB images
//     rti_relight_rgb_enhanced   PTM-6 maps -> one diffuse gain or specular RGB image (DESIGN.md §4.12's RGB form)
//     rti_rgb_normals            PTM-6 maps -> rti_ptm_normals of their fp32 luminance map
//
// The arithmetic is the existing entries': a channel of an image is rti_relight's F32 path (basis_eval<float>, the
// FMA chain of dot_k, cvt_out), the luminance is rti_rgb8_normals' (rti_rgb_px.h), the normals are
// ptm_px::normal_of and the enhanced modes enhance_px::rgb_enhanced, so every output equals the entry it replaces
// three launches of, or the rti_rgb8 entry of the same coefficient values, bit for bit.
//
// The PTM-6 kernels keep rti_relight's lane map (a lane owns 4 consecutive pixels, a wave 256, a block 1024) and
// rti_lane4.h's loads: a full 256-pixel chunk of a pixel-major map reaches registers through 6 coalesced 1-KiB
// loads and the wave's LDS slab, one channel after the other through the same slab with wave-level fences only; a
// planar map is read as 16-byte loads.  Three 4-byte output rows leave through the slab as whole 1-KiB stores,
// uint8 rows as the lane's three dwords.  A launch whose P is no multiple of 4 or whose pointers or channel stride
// are not aligned for the vector accesses, and the last partial chunk of any launch, take one pixel per lane
// through the same per-pixel functions.
//
// HSH-9 / HSH-16: 3 channels x 4 pixels x k values do not fit a lane (192 at k = 16), so a lane owns one pixel
// (48 values at k = 16), a wave 64 and a block 256, as rti_hsh8.hip's kernels do, with the basis rows of up to 64
// directions in LDS.  A full wave of a pixel-major map stages its 64 rows of a channel through the slab; the
// wave's 192 output elements leave as whole dwords.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rti_basis.h"
#include "rti_convert.h"
#include "rti_dispatch.h"
#include "rti_enhance_px.h"
#include "rti_hsh_px.h"
#include "rti_lane4.h"
#include "rti_ptm_px.h"
#include "rti_quant8.h"
#include "rti_rgb_px.h"
#include "rti_stack.h"

namespace rti {
namespace {

using namespace lane4;  // the wave loads of fp32 maps and the sinks
using rgb_px::K;        // PTM-6
using hsh_px::dot_k;      // rti_relight's fp32 chain
using rgb_px::luminance;
using rgb_px::normal_px;
using rgb_px::Weights;

constexpr int ECH = 64;  // directions per basis table of the HSH kernel

// ---- PTM-6: a lane owns 4 pixels ---------------------------------------------------------------------------------

// LDS per wave: a channel's 256 rows in (pixel-major), three 4-byte rows per pixel out
template <int CL>
constexpr int ptm_slab(bool stage_out) {
  return slab_v4(CL == RTI_COEF_PIXEL_MAJOR ? K : 0, stage_out ? 3 : 0);
}

// the wave's 256 pixels of the three channels, one after the other through the same slab
template <int CL>
__device__ __forceinline__ void load_wave3(const float* __restrict__ coef, int64_t cs, int64_t P, int64_t wave_px,
                                           int lane, floatx4* __restrict__ slab, float (&a)[3][4][K]) {
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) load_wave<K, CL>(coef + ch * cs, P, wave_px, lane, slab, a[ch]);
}

template <int CL>
__device__ __forceinline__ void load_pixel3(const float* __restrict__ coef, int64_t cs, int64_t P, int64_t p,
                                            float (&c)[3][K]) {
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) load_pixel<K, CL>(coef + ch * cs, P, p, c[ch]);
}

// pixel v of a lane's four, its three channels together
__device__ __forceinline__ void pixel_of(const float (&a)[3][4][K], int v, float (&c)[3][K]) {
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
#pragma unroll
    for (int j = 0; j < K; ++j) c[ch][j] = a[ch][v][j];
}

template <typename TO, int CL>
__global__ void __launch_bounds__(256)
relight_rgb_ptm_k(const float* __restrict__ coef, int64_t cs, int64_t P, int vec, const double* __restrict__ luv,
                  int E, TO* __restrict__ out) {
  constexpr int SLAB = ptm_slab<CL>(sizeof(TO) == 4);
  __shared__ floatx4 slabs[4 * SLAB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 256;
  if (wave_px >= P) return;
  floatx4* slab = slabs + wave * SLAB;
  if (vec && wave_px + 256 <= P) {  // wave-uniform
    float a[3][4][K];
    load_wave3<CL>(coef, cs, P, wave_px, lane, slab, a);
    for (int e = 0; e < E; ++e) {
      float b[K];
      ptm_eval<float>((float)luv[2 * e], (float)luv[2 * e + 1], b);  // basis_eval<float>'s PTM-6 branch
      TO o[4][3];
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[v][ch] = cvt_out<TO>(dot_k<K>(a[ch][v], b));
      store_rgb4<TO>(out + ((int64_t)e * P + wave_px) * 3, lane, slab, o);
    }
    return;
  }
  for (int j = 0; j < 4; ++j) {
    const int64_t p = wave_px + 64 * j + lane;
    if (p >= P) break;
    float c[3][K];
    load_pixel3<CL>(coef, cs, P, p, c);
    for (int e = 0; e < E; ++e) {
      float b[K];
      ptm_eval<float>((float)luv[2 * e], (float)luv[2 * e + 1], b);
      TO* px = out + ((int64_t)e * P + p) * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) px[ch] = cvt_out<TO>(dot_k<K>(c[ch], b));
    }
  }
}

// every channel enhanced under the luminance's peak (enhance_px::rgb_enhanced)
template <typename TO, int MODE, int CL>
__global__ void __launch_bounds__(256)
relight_rgb_enhanced_k(const float* __restrict__ coef, int64_t cs, int64_t P, int vec, Weights w,
                       enhance_px::Enhance q, TO* __restrict__ out) {
  constexpr int SLAB = ptm_slab<CL>(sizeof(TO) == 4);
  __shared__ floatx4 slabs[4 * SLAB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 256;
  if (wave_px >= P) return;
  floatx4* slab = slabs + wave * SLAB;
  if (vec && wave_px + 256 <= P) {  // wave-uniform
    float a[3][4][K];
    load_wave3<CL>(coef, cs, P, wave_px, lane, slab, a);
    TO o[4][3];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      float c[3][K], l[K];
      pixel_of(a, v, c);
      luminance(c, w.r, w.g, w.b, l);
      enhance_px::rgb_enhanced<MODE, TO>(c, l, q, o[v]);
    }
    store_rgb4<TO>(out + wave_px * 3, lane, slab, o);
    return;
  }
  for (int j = 0; j < 4; ++j) {
    const int64_t p = wave_px + 64 * j + lane;
    if (p >= P) break;
    float c[3][K], l[K];
    load_pixel3<CL>(coef, cs, P, p, c);
    luminance(c, w.r, w.g, w.b, l);
    TO o[3];
    enhance_px::rgb_enhanced<MODE, TO>(c, l, q, o);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[p * 3 + ch] = o[ch];
  }
}

template <int NL, int CL>
__global__ void __launch_bounds__(256)
rgb_normals_k(const float* __restrict__ coef, int64_t cs, int64_t P, int vec, Weights w, float* __restrict__ normals,
              uint8_t* __restrict__ kind, float* __restrict__ peak) {
  constexpr bool STAGE_OUT = NL == RTI_NORMAL_PIXEL_MAJOR;
  constexpr int SLAB = ptm_slab<CL>(STAGE_OUT);
  __shared__ floatx4 slabs[4 * SLAB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 256;
  if (wave_px >= P) return;
  floatx4* slab = slabs + wave * SLAB;
  if (vec && wave_px + 256 <= P) {  // wave-uniform
    const int64_t p0 = wave_px + 4 * lane;
    float a[3][4][K];
    load_wave3<CL>(coef, cs, P, wave_px, lane, slab, a);
    ptm_px::NormalOut o[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      float c[3][K];
      pixel_of(a, v, c);
      o[v] = normal_px(c, w, peak != nullptr);
    }
    if (kind)
      *reinterpret_cast<uint32_t*>(kind + p0) = (uint32_t)o[0].kind | ((uint32_t)o[1].kind << 8) |
                                                ((uint32_t)o[2].kind << 16) | ((uint32_t)o[3].kind << 24);
    if (peak) *reinterpret_cast<floatx4*>(peak + p0) = floatx4{o[0].peak, o[1].peak, o[2].peak, o[3].peak};
    if constexpr (STAGE_OUT) {
      float n[4][3];
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int i = 0; i < 3; ++i) n[v][i] = o[v].n[i];
      store_rows_staged<3, float>(normals + wave_px * 3, lane, slab, n);
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
    float c[3][K];
    load_pixel3<CL>(coef, cs, P, p, c);
    const ptm_px::NormalOut o = normal_px(c, w, peak != nullptr);
#pragma unroll
    for (int i = 0; i < 3; ++i) normals[NL == RTI_NORMAL_PLANAR ? (int64_t)i * P + p : p * 3 + i] = o.n[i];
    if (kind) kind[p] = o.kind;
    if (peak) peak[p] = o.peak;
  }
}

// ---- HSH-9 / HSH-16: a lane owns one pixel ---------------------------------------------------------------------

// 16-byte pieces of a wave's 64 rows of KH floats (144 at k = 9, 256 at k = 16); 64·KH·4 is a multiple of 16
template <int KH>
constexpr int hsh_run_v4() { return 64 * KH / 4; }

// the wave's 64 rows of a pixel-major channel through its slab: coalesced 16-byte loads, then the lane's own row
template <int KH>
__device__ __forceinline__ void load_rows64(const float* __restrict__ rows, int lane, floatx4* __restrict__ slab,
                                            float (&c)[KH]) {
  constexpr int NV = hsh_run_v4<KH>(), PIECES = (NV + 63) / 64;
  const floatx4* g = reinterpret_cast<const floatx4*>(rows);
  floatx4 t[PIECES];
#pragma unroll
  for (int j = 0; j < PIECES; ++j)
    if (j * 64 + lane < NV) t[j] = __builtin_nontemporal_load(g + j * 64 + lane);
#pragma unroll
  for (int j = 0; j < PIECES; ++j)
    if (j * 64 + lane < NV) slab[j * 64 + lane] = t[j];
  wave_lds_sync();
  const float* s = reinterpret_cast<const float*>(slab) + lane * KH;
#pragma unroll
  for (int i = 0; i < KH; ++i) c[i] = s[i];
  wave_lds_sync();  // every lane has its row: the slab may be written again
}

template <int KH, typename TO, int CL>
__global__ void __launch_bounds__(256)
relight_rgb_hsh_k(const float* __restrict__ coef, int64_t cs, int64_t P, int vin, int vout,
                  const double* __restrict__ luv, int E, TO* __restrict__ out) {
  constexpr int SLAB = CL == RTI_COEF_PIXEL_MAJOR ? hsh_run_v4<KH>() : 48;  // rows in; 64 rows of 3 dwords out
  __shared__ floatx4 slabs[4 * SLAB];
  __shared__ float btab[ECH * KH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  floatx4* slab = slabs + wave * SLAB;
  // every lane stays to the end: the basis tables are filled by the whole workgroup
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 64;
  const int64_t p = wave_px + lane;
  const bool live = p < P, full = wave_px + 64 <= P;  // full: wave-uniform
  float c[3][KH];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float* map = coef + ch * cs;
    if (CL == RTI_COEF_PIXEL_MAJOR && vin && full) {  // wave-uniform
      load_rows64<KH>(map + wave_px * KH, lane, slab, c[ch]);
    } else if (live) {
      load_pixel<KH, CL>(map, P, p, c[ch]);
    } else {
#pragma unroll
      for (int i = 0; i < KH; ++i) c[ch][i] = 0.f;
    }
  }

  for (int e0 = 0; e0 < E; e0 += ECH) {
    const int ne = min(ECH, E - e0);
    if (e0) __syncthreads();  // the previous table has been read
    for (int i = threadIdx.x; i < ne; i += 256) {
      float b[KH];
      hsh_eval<float>((float)luv[2 * (e0 + i)], (float)luv[2 * (e0 + i) + 1], KH, b);  // basis_eval<float>'s HSH branch
#pragma unroll
      for (int k = 0; k < KH; ++k) btab[i * KH + k] = b[k];
    }
    __syncthreads();
    for (int e = 0; e < ne; ++e) {
      const float* b = btab + e * KH;
      TO o[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) o[ch] = cvt_out<TO>(dot_k<KH>(c[ch], b));
      TO* rows = out + ((int64_t)(e0 + e) * P + wave_px) * 3;
      if (vout && full) {  // wave-uniform: the wave's 192 elements as whole dwords
        uint32_t* d = reinterpret_cast<uint32_t*>(rows);
        const uint32_t* s = reinterpret_cast<const uint32_t*>(slab);
        if constexpr (sizeof(TO) == 4) {
          uint32_t* sw = reinterpret_cast<uint32_t*>(slab) + 3 * lane;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) sw[ch] = __builtin_bit_cast(uint32_t, o[ch]);
          wave_lds_sync();
#pragma unroll
          for (int j = 0; j < 3; ++j) d[j * 64 + lane] = s[j * 64 + lane];
        } else {
          uint8_t* sb = reinterpret_cast<uint8_t*>(slab) + 3 * lane;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) sb[ch] = o[ch];
          wave_lds_sync();
          if (lane < 48) d[lane] = s[lane];
        }
        wave_lds_sync();  // the slab may be written again
      } else if (live) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) rows[3 * lane + ch] = o[ch];
      }
    }
  }
}

// ---- launchers --------------------------------------------------------------------------------------------------

struct Maps {
  const float* coef;
  int layout;
  int64_t cs, P;
  hipStream_t s;
};

template <int KH, typename TO, int CL>
void launch_hsh(const Maps& m, int vin, int vout, const double* luv, int E, void* out) {
  hipLaunchKernelGGL((relight_rgb_hsh_k<KH, TO, CL>), dim3(grid_1d(m.P, 256)), dim3(256), 0, m.s, m.coef, m.cs, m.P,
                     vin, vout, luv, E, static_cast<TO*>(out));
}

}  // namespace
}  // namespace rti

using namespace rti;

extern "C" int rti_relight_rgb(const float* coef, int basis, int coef_layout, int64_t coef_channel_stride, int64_t P,
                               const double* luv, int E_, void* out, int out_dtype, rti_stream_t stream) {
  const char* const E = "rti_relight_rgb";
  if (int st = check_pointers(E, {coef, luv, out})) return st;
  if (P < 1 || E_ < 1) return fail(RTI_ERR_BAD_ARG, "%s: P and E must be positive", E);
  const int k = basis_terms(basis);
  if (k < 0) return fail(RTI_ERR_BAD_ARG, "%s: unknown basis %d", E, basis);
  if (int st = check_rgb_maps(E, k, coef_layout, coef_channel_stride, P)) return st;
  if (int st = check_out_dtype(E, out_dtype)) return st;
  const Maps m{coef, coef_layout, coef_channel_stride ? coef_channel_stride : P * k, P, (hipStream_t)stream};
  note_launches(1);
  if (k == K) {
    const int vec = maps_vec(coef, m.cs, P) && rgb_out_vec(out, out_dtype) ? 1 : 0;
    with_layout(coef_layout, [&](auto l) {
      with_out(out_dtype, [&](auto t) {
        launch(relight_rgb_ptm_k<decltype(t), decltype(l)::value>, P, m.s, coef, m.cs, P, vec, luv, E_, out);
      });
    });
  } else {
    // a wave's 64 rows as 16-byte pieces; its 192 output elements as dwords (direction e's rows start 3·P·e
    // elements into out)
    const int vin = aligned_to(coef, 16) && m.cs % 4 == 0 ? 1 : 0;
    const int vout = aligned_to(out, 4) && (out_dtype != RTI_U8 || P % 4 == 0) ? 1 : 0;
    with_layout(coef_layout, [&](auto l) {
      with_out(out_dtype, [&](auto t) {
        using TO = decltype(t);
        if (k == 9)
          launch_hsh<9, TO, decltype(l)::value>(m, vin, vout, luv, E_, out);
        else
          launch_hsh<16, TO, decltype(l)::value>(m, vin, vout, luv, E_, out);
      });
    });
  }
  return check_launch(E);
}

extern "C" int rti_relight_rgb_enhanced(const float* coef, int coef_layout, int64_t coef_channel_stride, int64_t P,
                                        const float* w, int mode, double gain, double kd, double ks, int spec_exp,
                                        double lu, double lv, void* out, int out_dtype, rti_stream_t stream) {
  const char* const E = "rti_relight_rgb_enhanced";
  if (int st = check_pointers(E, {coef, out})) return st;
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  if (int st = check_rgb_maps(E, K, coef_layout, coef_channel_stride, P)) return st;
  if (int st = enhance_px::check_enhance(E, mode, gain, kd, ks, spec_exp, lu, lv)) return st;
  Weights wt;
  if (int st = rgb_px::host_weights(E, w, wt)) return st;
  if (int st = check_out_dtype(E, out_dtype)) return st;
  const int64_t cs = coef_channel_stride ? coef_channel_stride : P * K;
  const int vec = maps_vec(coef, cs, P) && rgb_out_vec(out, out_dtype) ? 1 : 0;
  const enhance_px::Enhance q = enhance_px::enhance_args(gain, kd, ks, spec_exp, lu, lv);
  note_launches(1);
  with_layout(coef_layout, [&](auto l) {
    enhance_px::with_mode_out(mode, out_dtype, [&](auto m, auto t) {
      launch(relight_rgb_enhanced_k<decltype(t), decltype(m)::value, decltype(l)::value>, P, (hipStream_t)stream, coef,
             cs, P, vec, wt, q, out);
    });
  });
  return check_launch(E);
}

extern "C" int rti_rgb_normals(const float* coef, int coef_layout, int64_t coef_channel_stride, int64_t P,
                               const float* w, float* normals, int normal_layout, uint8_t* kind, float* peak,
                               rti_stream_t stream) {
  const char* const E = "rti_rgb_normals";
  if (int st = check_pointers(E, {coef, normals})) return st;
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  if (int st = check_rgb_maps(E, K, coef_layout, coef_channel_stride, P)) return st;
  if (int st = check_normal_layout(E, normal_layout)) return st;
  Weights wt;
  if (int st = rgb_px::host_weights(E, w, wt)) return st;
  const int64_t cs = coef_channel_stride ? coef_channel_stride : P * K;
  const int vec = maps_vec(coef, cs, P) && normals_out_vec(normals, kind, peak) ? 1 : 0;
  note_launches(1);
  with_layout(coef_layout, [&](auto l) {
    with_normal_layout(normal_layout, [&](auto nl) {
      launch(rgb_normals_k<decltype(nl)::value, decltype(l)::value>, P, (hipStream_t)stream, coef, cs, P, vec, wt,
             normals, kind, peak);
    });
  });
  return check_launch(E);
}
