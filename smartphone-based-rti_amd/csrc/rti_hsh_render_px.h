// rti_hsh_render_px.h -- the renderers of HSH maps with one pixel per lane.  rti_hsh8.hip takes the
// store of a direction's rows (store_dir) and rows_as_dwords.  rti_hsh_specular.hip and rti_hsh_gain.hip (§4.14, §4.15)
// take everything: the E basis rows in LDS, a lane's normal, the loop over the directions, and the kernel pair, Frame,
// launchers and checks of a renderer under a normal map, which they instantiate with a per-pixel policy.
// rti_hsh8.hip's lane map: one pixel per lane, 64 consecutive pixels per wave, 256 per workgroup.  Everything on the
// device but the kernels is __forceinline__.
//
// A policy is a struct of the launch's scalar parameters (a kernel argument as it is) with
//     Dirs                                  the E directions as a kernel argument: d[e].lu, d[e].lv and what else
//                                           value() reads of a direction, formed on the host by
//     static dir(lu, lv)
//     prepare<K, C>(c, n)                   what a pixel keeps for all directions
//     value<K, C, TO>(c, b, n, px, d, o)    the pixel's C elements at direction d with basis row b
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rti_basis.h"
#include "rti_dispatch.h"
#include "rti_hsh_px.h"

namespace rti {
namespace hsh_render {

using namespace hsh_px;  // the chain, the slab runs and the two sources

constexpr int CHUNK = 256;  // pixels of a workgroup
constexpr int MAXE = RTI_SPECULAR_MAX_DIRS;

// LDS per wave in 16-byte pieces: the coefficient run in, 64 normals in (48 pieces), at most 64 rows of 3 dwords out
constexpr int render_slab(int coef_run) { return slab_v4(coef_run, run_v4<12>()); }

// the E basis rows, by the first E threads of the workgroup; the caller synchronises.  DIRS: d[e].lu, d[e].lv in fp64
template <int K, typename DIRS>
__device__ __forceinline__ void fill_basis(const DIRS& dirs, int E, float* __restrict__ btab) {
  if ((int)threadIdx.x < E) {
    float b[K];
    hsh_eval<float>((float)dirs.d[threadIdx.x].lu, (float)dirs.d[threadIdx.x].lv, K, b);  // basis_eval<float>'s HSH branch
#pragma unroll
    for (int k = 0; k < K; ++k) btab[threadIdx.x * K + k] = b[k];
  }
}

// the normal of pixel wave_px + lane.  staged (wave-uniform; pixel-major, a full wave, normals 16-byte aligned):
// the wave's 64 normals are one run of 768 bytes.
__device__ __forceinline__ void load_normal(const float* __restrict__ normals, int nl, bool staged, int64_t P,
                                            int64_t wave_px, int lane, bool live, u32x4* __restrict__ slab,
                                            float (&n)[3]) {
  if (staged) {
    run_in<12>(normals + wave_px * 3, lane, slab);
    uint32_t w[3];
    lane_words<12>(slab, lane, w);
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = __uint_as_float(w[i]);
    return;
  }
  const int64_t p = wave_px + lane;
#pragma unroll
  for (int i = 0; i < 3; ++i) n[i] = !live ? 0.f : nl == RTI_NORMAL_PLANAR ? normals[(int64_t)i * P + p] : normals[p * 3 + i];
}

// the wave's 64 pixels of one direction: rows[lane][ch] = o[ch].  vout (wave-uniform; a full wave, the alignment of
// rows_as_dwords): the wave's 64·C elements leave as whole dwords, through the slab unless a lane's element is one.
template <int C, typename TO>
__device__ __forceinline__ void store_dir(const TO (&o)[C], TO* rows, int lane, bool live, bool vout, u32x4* slab) {
  constexpr int ND = 64 * C * (int)sizeof(TO) / 4;  // dwords of a wave and direction: 192, 64, 48 or 16
  if (vout && !(C == 1 && sizeof(TO) == 4)) {
    uint32_t* d = reinterpret_cast<uint32_t*>(rows);
    const uint32_t* s = reinterpret_cast<const uint32_t*>(slab);
    if constexpr (sizeof(TO) == 4) {
      uint32_t* sw = reinterpret_cast<uint32_t*>(slab) + C * lane;
#pragma unroll
      for (int ch = 0; ch < C; ++ch) sw[ch] = __builtin_bit_cast(uint32_t, o[ch]);
    } else {
      uint8_t* sb = reinterpret_cast<uint8_t*>(slab) + C * lane;
#pragma unroll
      for (int ch = 0; ch < C; ++ch) sb[ch] = o[ch];
    }
    wave_lds_sync();
#pragma unroll
    for (int j = 0; j < (ND + 63) / 64; ++j)
      if (j * 64 + lane < ND) d[j * 64 + lane] = s[j * 64 + lane];
    wave_lds_sync();  // the slab may be written again
  } else if (live) {
#pragma unroll
    for (int ch = 0; ch < C; ++ch) rows[C * lane + ch] = o[ch];
  }
}

// the wave's 64 pixels at every direction: out[e][p][ch], value(e, o) giving the lane's C elements of direction e
template <int C, typename TO, typename V>
__device__ __forceinline__ void render(int E, int64_t P, int64_t wave_px, int lane, bool live, bool vout,
                                       u32x4* __restrict__ slab, TO* __restrict__ out, V&& value) {
  for (int e = 0; e < E; ++e) {
    TO o[C];
    value(e, o);
    store_dir<C, TO>(o, out + ((int64_t)e * P + wave_px) * C, lane, live, vout, slab);
  }
}

// ---- a renderer under a normal map: the kernel pair of a policy ------------------------------------------------------
// Both: wave w of workgroup g owns pixels [(4g + w)·64, + 64).  vin / vn / vout: the coefficient run, the normal run
// and the output rows may move as whole pieces (the entry's alignment checks).  The coefficients or bytes and the
// normal are read once for all E directions; every path runs the policy's prepare and value, so the bits do not
// depend on it.

template <int K, int C, typename TO, typename Policy>
__device__ __forceinline__ void render_policy(const Policy& pol, const typename Policy::Dirs& dirs, const float (&c)[C][K],
                                              const float (&n)[3], const float* __restrict__ btab, int E, int64_t P,
                                              int64_t wave_px, int lane, bool live, bool vout, u32x4* __restrict__ slab,
                                              TO* __restrict__ out) {
  const auto px = pol.template prepare<K, C>(c, n);
  render<C, TO>(E, P, wave_px, lane, live, vout, slab, out, [&](int e, TO (&o)[C]) {
    pol.template value<K, C, TO>(c, btab + e * K, n, px, dirs.d[e], o);
  });
}

template <int K, typename TO, typename Policy>
__global__ void __launch_bounds__(256)
relight_hsh8_policy_k(const uint8_t* __restrict__ coef8, int64_t P, int vin, const float* __restrict__ qparams,
                      const float* __restrict__ normals, int nl, int vn, int vout, Policy pol,
                      typename Policy::Dirs dirs, int E, TO* __restrict__ out) {
  constexpr int SLAB = render_slab(run_v4<3 * K>());
  __shared__ u32x4 slabs[4 * SLAB];
  __shared__ float btab[MAXE * K];
  __shared__ float qs[2 * K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32x4* slab = slabs + wave * SLAB;
  load_steps<K>(qparams, qs);
  fill_basis<K>(dirs, E, btab);
  __syncthreads();
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 64;
  if (wave_px >= P) return;  // wave-uniform; no workgroup barrier below
  const bool live = wave_px + lane < P, full = wave_px + 64 <= P;  // full: wave-uniform
  float c[3][K];
  load_px8<K>(coef8, wave_px, lane, live, vin && full, slab, qs, c);
  float n[3];
  load_normal(normals, nl, vn && full, P, wave_px, lane, live, slab, n);
  render_policy<K, 3, TO>(pol, dirs, c, n, btab, E, P, wave_px, lane, live, vout && full, slab, out);
}

template <int K, int C, int CL, typename TO, typename Policy>
__global__ void __launch_bounds__(256)
relight_hsh_policy_k(const float* __restrict__ coef, int64_t cs, int64_t P, int vin, const float* __restrict__ normals,
                     int nl, int vn, int vout, Policy pol, typename Policy::Dirs dirs, int E, TO* __restrict__ out) {
  constexpr int SLAB = render_slab(CL == RTI_COEF_PIXEL_MAJOR ? run_v4<4 * K>() : 0);
  __shared__ u32x4 slabs[4 * SLAB];
  __shared__ float btab[MAXE * K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32x4* slab = slabs + wave * SLAB;
  fill_basis<K>(dirs, E, btab);
  __syncthreads();
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 64;
  if (wave_px >= P) return;  // wave-uniform; no workgroup barrier below
  const bool live = wave_px + lane < P, full = wave_px + 64 <= P;  // full: wave-uniform
  // hsh_px::load_px<K, C, CL> with dead lanes 0, written out: as a call it costs two K = 16, C = 3 instantiations a
  // wave of occupancy
  float c[C][K];
  const int64_t p = wave_px + lane;
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    const float* map = coef + ch * cs;
    if (CL == RTI_COEF_PIXEL_MAJOR && vin && full) {  // wave-uniform: the wave's 64 rows of the channel are one run
      run_in<4 * K>(map + wave_px * K, lane, slab);
      uint32_t w[K];
      lane_words<4 * K>(slab, lane, w);
#pragma unroll
      for (int j = 0; j < K; ++j) c[ch][j] = __uint_as_float(w[j]);
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j)
        c[ch][j] = !live ? 0.f : CL == RTI_COEF_PLANAR ? map[(int64_t)j * P + p] : map[p * K + j];
    }
  }
  float n[3];
  load_normal(normals, nl, vn && full, P, wave_px, lane, live, slab, n);
  render_policy<K, C, TO>(pol, dirs, c, n, btab, E, P, wave_px, lane, live, vout && full, slab, out);
}

// ---- host ---------------------------------------------------------------------------------------------------------

inline int normals_staged(const float* normals, int normal_layout) {
  return normal_layout == RTI_NORMAL_PIXEL_MAJOR && aligned_to(normals, 16) ? 1 : 0;
}
// a wave's 64·C output elements as dwords: direction e's rows start C·P·e elements into out
inline int rows_as_dwords(const void* out, int out_dtype, int64_t P) {
  return aligned_to(out, 4) && (out_dtype != RTI_U8 || P % 4 == 0) ? 1 : 0;
}

// what a launch takes besides its coefficients
template <typename Policy>
struct Frame {
  int64_t P;
  const float* normals;
  int nl, vn, vout;
  Policy pol;
  typename Policy::Dirs dirs;
  int E;
  void* out;
  int out_dtype;
  hipStream_t s;
};

// the checks a policy's two entries share after their coefficients, in the order include/rti.h lists the arguments:
// check_params() is the policy's own, between the normal layout and E (E before the values of luv it counts).  Fills
// `a`; directions past E stay zero.
template <typename Policy, typename Check>
int check_frame(const char* entry, int64_t P, const float* normals, int normal_layout, Check&& check_params,
                const Policy& pol, const double* luv, int E, void* out, int out_dtype, rti_stream_t stream,
                Frame<Policy>& a) {
  if (int st = check_normal_layout(entry, normal_layout)) return st;
  if (int st = check_params()) return st;
  if (E < 1 || E > MAXE) return fail(RTI_ERR_BAD_ARG, "%s: E = %d outside [1, %d]", entry, E, MAXE);
  for (int i = 0; i < 2 * E; ++i)
    if (!std::isfinite(luv[i])) return fail(RTI_ERR_BAD_ARG, "%s: non-finite light direction", entry);
  if (int st = check_out_dtype(entry, out_dtype)) return st;
  a = Frame<Policy>{P, normals, normal_layout, normals_staged(normals, normal_layout), rows_as_dwords(out, out_dtype, P),
                    pol, {}, E, out, out_dtype, (hipStream_t)stream};
  for (int i = 0; i < E; ++i) a.dirs.d[i] = Policy::dir(luv[2 * i], luv[2 * i + 1]);
  return RTI_OK;
}

template <typename Policy>
void launch8(int k, const uint8_t* coef8, const float* qparams, const Frame<Policy>& a) {
  const int vin = aligned_to(coef8, 16) ? 1 : 0;
  with_hsh_terms(k, [&](auto kt) {
    with_out(a.out_dtype, [&](auto t) {
      using TO = decltype(t);
      hipLaunchKernelGGL((relight_hsh8_policy_k<decltype(kt)::value, TO, Policy>), dim3(grid_1d(a.P, CHUNK)), dim3(256), 0,
                         a.s, coef8, a.P, vin, qparams, a.normals, a.nl, a.vn, a.vout, a.pol, a.dirs, a.E,
                         static_cast<TO*>(a.out));
    });
  });
}

template <typename Policy>
void launch(int k, const float* coef, int C, int layout, int64_t cs, const Frame<Policy>& a) {
  const int vin = maps_staged(coef, layout, C, cs);
  with_hsh_terms(k, [&](auto kt) {
    with_channels(C, [&](auto ct) {
      with_layout(layout, [&](auto l) {
        with_out(a.out_dtype, [&](auto t) {
          using TO = decltype(t);
          hipLaunchKernelGGL((relight_hsh_policy_k<decltype(kt)::value, decltype(ct)::value, decltype(l)::value, TO, Policy>),
                             dim3(grid_1d(a.P, CHUNK)), dim3(256), 0, a.s, coef, cs, a.P, vin, a.normals, a.nl, a.vn,
                             a.vout, a.pol, a.dirs, a.E, static_cast<TO*>(a.out));
        });
      });
    });
  });
}

}  // namespace hsh_render
}  // namespace rti
