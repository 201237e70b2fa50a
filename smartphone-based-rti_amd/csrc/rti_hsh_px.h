// rti_hsh_px.h -- what the kernels with one HSH pixel per lane share (rti_hsh8.hip, rti_hsh_normals.hip, and through
// rti_hsh_render_px.h rti_hsh_specular.hip and rti_hsh_gain.hip): rti_relight's fp32 chain, a wave's run of 64 rows
// through its LDS slab, and the two sources of a lane's pixel, the 8-bit payload and the fp32 maps (DESIGN.md §4.9,
// §4.18).  The device code is __forceinline__, with 64 consecutive pixels per wave.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rti_internal.h"
#include "rti_wave_lds.h"

namespace rti {
namespace hsh_px {

using lds::wave_lds_sync;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

inline bool hsh_basis(int basis) { return basis == RTI_BASIS_HSH9 || basis == RTI_BASIS_HSH16; }

// rti_relight.hip's dot_k for fp32: fused multiply-adds in term order.  A copy, as rti_lane4.h's loads are:
// bench.py hashes rti_relight.hip to decide whether profiles/traffic.json is stale.
template <int K>
__device__ __forceinline__ float dot_k(const float (&c)[K], const float* b) {
  float acc = c[0] * b[0];
#pragma unroll
  for (int k = 1; k < K; ++k) acc = fmaf(c[k], b[k], acc);
  return acc;
}

// ---- a wave's run of 64 rows of ROWB bytes through its slab ---------------------------------------------------
// 64·ROWB is a multiple of 16 for every ROWB; the run's base must be 16-byte aligned.  The slab is only ever
// accessed as uint32_t / u32x4 / bytes, with a wave-level release / acquire between its phases.

template <int ROWB>
constexpr int run_v4() { return 64 * ROWB / 16; }
// + one piece: k = 9's realigning read (lane_words) takes one dword past the run
constexpr int slab_v4(int a, int b) { return (a > b ? a : b) + 1; }

template <int ROWB>
__device__ __forceinline__ void run_in(const void* __restrict__ g, int lane, u32x4* __restrict__ slab) {
  constexpr int NV = run_v4<ROWB>(), PIECES = (NV + 63) / 64;
  const u32x4* g4 = static_cast<const u32x4*>(g);
  u32x4 t[PIECES];
#pragma unroll
  for (int j = 0; j < PIECES; ++j)
    if (j * 64 + lane < NV) t[j] = __builtin_nontemporal_load(g4 + j * 64 + lane);
#pragma unroll
  for (int j = 0; j < PIECES; ++j)
    if (j * 64 + lane < NV) slab[j * 64 + lane] = t[j];
  wave_lds_sync();
}

template <int ROWB>
__device__ __forceinline__ void run_out(void* __restrict__ g, int lane, const u32x4* __restrict__ slab) {
  constexpr int NV = run_v4<ROWB>(), PIECES = (NV + 63) / 64;
  wave_lds_sync();
  u32x4* g4 = static_cast<u32x4*>(g);
#pragma unroll
  for (int j = 0; j < PIECES; ++j)
    if (j * 64 + lane < NV) g4[j * 64 + lane] = slab[j * 64 + lane];
  wave_lds_sync();  // the slab may be written again
}

// the lane's row of NB bytes out of the slab as (NB + 3) / 4 dwords, byte i of the row in byte i % 4 of word i / 4
template <int NB>
__device__ __forceinline__ void lane_words(const u32x4* __restrict__ slab, int lane, uint32_t (&w)[(NB + 3) / 4]) {
  constexpr int NW = (NB + 3) / 4;
  if constexpr (NB % 16 == 0) {
#pragma unroll
    for (int j = 0; j < NB / 16; ++j) {
      const u32x4 t = slab[lane * (NB / 16) + j];
#pragma unroll
      for (int i = 0; i < 4; ++i) w[4 * j + i] = t[i];
    }
  } else {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(slab);
    const int o = NB * lane, d0 = o >> 2, sh = 8 * (o & 3);
    uint32_t d[NW + 1];
#pragma unroll
    for (int i = 0; i <= NW; ++i) d[i] = s[d0 + i];
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = (uint32_t)((((uint64_t)d[i + 1] << 32) | d[i]) >> sh);
  }
  wave_lds_sync();  // every lane has its row: the slab may be written again
}

// the lane's row of NB bytes (packed as lane_words returns them) into the slab
template <int NB>
__device__ __forceinline__ void put_lane_words(u32x4* __restrict__ slab, int lane, const uint32_t (&w)[(NB + 3) / 4]) {
  if constexpr (NB % 16 == 0) {
#pragma unroll
    for (int j = 0; j < NB / 16; ++j) {
      u32x4 t;
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] = w[4 * j + i];
      slab[lane * (NB / 16) + j] = t;
    }
  } else {
    uint8_t* s = reinterpret_cast<uint8_t*>(slab) + NB * lane;
#pragma unroll
    for (int i = 0; i < NB; ++i) s[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  }
}

// ---- dequantisation of an 8-bit pixel ------------------------------------------------------------------------------

// step[0..K-1] = scale_j / 255.0f (one correctly rounded fp32 division per term and workgroup), bias[0..K-1];
// the caller synchronises the workgroup
template <int K>
__device__ __forceinline__ void load_steps(const float* __restrict__ qparams, float* __restrict__ qs) {
#pragma clang fp contract(off)
  if (threadIdx.x < K) {
    qs[threadIdx.x] = qparams[threadIdx.x] / 255.0f;
    qs[K + threadIdx.x] = qparams[K + threadIdx.x];
  }
}

// 3K bytes -> the fp32 coefficients read_rti builds from them: a multiply and an add, each rounded
template <int K>
__device__ __forceinline__ void dequantise_px(const uint32_t (&w)[(3 * K + 3) / 4], const float* __restrict__ qs,
                                              float (&c)[3][K]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const float step = qs[j], bias = qs[K + j];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int i = ch * K + j;
      const float raw = (float)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
      const float t = raw * step;
      c[ch][j] = t + bias;
    }
  }
}

// ---- the two sources of a lane's pixel --------------------------------------------------------------------------
// Pixel run_px + lane of a run of 64.  staged is wave-uniform: a full run whose rows may move as 16-byte pieces (the
// entry's alignment checks).  Otherwise a live lane loads its own values.

// c[ch][j] of the 8-bit payload [p][ch][j]; qs: load_steps'.  A lane past the image dequantises zero bytes.
template <int K>
__device__ __forceinline__ void load_px8(const uint8_t* __restrict__ coef8, int64_t run_px, int lane, bool live,
                                         bool staged, u32x4* __restrict__ slab, const float* __restrict__ qs,
                                         float (&c)[3][K]) {
  constexpr int NB = 3 * K, NW = (NB + 3) / 4;
  uint32_t w[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) w[i] = 0;
  if (staged) {
    run_in<NB>(coef8 + run_px * NB, lane, slab);
    lane_words<NB>(slab, lane, w);
  } else if (live) {
    const int64_t p = run_px + lane;
#pragma unroll
    for (int i = 0; i < NB; ++i) w[i >> 2] |= (uint32_t)coef8[p * NB + i] << (8 * (i & 3));
  }
  dequantise_px<K>(w, qs, c);
}

// c[ch][j] of C fp32 maps cs elements apart in layout CL: a pixel-major channel's 64 rows are one run when staged,
// planar maps are coalesced as they are.  A lane past the image gets `dead`.
template <int K, int C, int CL>
__device__ __forceinline__ void load_px(const float* coef, int64_t cs, int64_t P, int64_t run_px, int lane, bool live,
                                        bool staged, float dead, u32x4* slab, float (&c)[C][K]) {
  const int64_t p = run_px + lane;
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    const float* map = coef + ch * cs;
    if (CL == RTI_COEF_PIXEL_MAJOR && staged) {
      run_in<4 * K>(map + run_px * K, lane, slab);
      uint32_t w[K];
      lane_words<4 * K>(slab, lane, w);
#pragma unroll
      for (int j = 0; j < K; ++j) c[ch][j] = __uint_as_float(w[j]);
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j)
        c[ch][j] = !live ? dead : CL == RTI_COEF_PLANAR ? map[(int64_t)j * P + p] : map[p * K + j];
    }
  }
}

// host: staged may hold for fp32 maps, every run of every channel read starts on a 16-byte boundary
inline int maps_staged(const float* coef, int coef_layout, int C, int64_t cs) {
  return coef_layout == RTI_COEF_PIXEL_MAJOR && aligned_to(coef, 16) && (C == 1 || cs % 4 == 0) ? 1 : 0;
}

}  // namespace hsh_px
}  // namespace rti
