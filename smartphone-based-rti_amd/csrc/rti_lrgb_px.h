// rti_lrgb_px.h -- what the LRGB translation units share (rti_lrgb.hip, rti_lrgb8.hip): the per-pixel relight
// arithmetic and the wave-level loads and stores of rti_relight's lane map (a lane owns 4 consecutive pixels, a
// wave 256, a block 1024).  Everything is __forceinline__ device code; moving it here changed no instruction of
// rti_lrgb.hip's kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rti_convert.h"
#include "rti_internal.h"

namespace rti {
namespace lrgb_px {

constexpr int K = 6;   // PTM-6
constexpr int NL = 9;  // floats of an LRGB pixel: a0..a5, cR, cG, cB

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- per-pixel arithmetic (fp64, no contraction; tests/lrgb_ref.py restates it line by line) ------------------

// rti_relight's dot_k<6>(double): the six products summed left to right, every one rounded
__device__ __forceinline__ double dot6(const double (&c)[K], const double (&b)[K]) {
#pragma clang fp contract(off)
  double acc = c[0] * b[0];
#pragma unroll
  for (int k = 1; k < K; ++k) acc = acc + c[k] * b[k];
  return acc;
}

// one LRGB pixel at the basis row b -> its three channels, converted once
template <typename TO>
__device__ __forceinline__ void rgb_of(const float (&m)[NL], const double (&b)[K], TO (&o)[3]) {
#pragma clang fp contract(off)
  double a[K];
#pragma unroll
  for (int i = 0; i < K; ++i) a[i] = (double)m[i];
  const double L = dot6(a, b);
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = cvt_out<TO>((double)m[K + c] * L);
}

// ---- loads and stores --------------------------------------------------------------------------------------------

// LDS per wave in 16-byte units: rows of `in` floats per pixel staged in, rows of `out` 4-byte elements staged out
constexpr int slab_v4(int in, int out) {
  const int n = in > out ? in : out;
  return n > 0 ? 64 * n : 1;
}

// Pixel-major rows of NF floats through LDS: relight_eval_major's load_coef_staged (rti_relight.hip), restated
// for fp32 rows of any length.  It is a copy because bench.py hashes rti_relight.hip to decide whether
// profiles/traffic.json is stale.  The wave reads its 256 pixels' rows as NF coalesced 1-KiB non-temporal loads
// (lane l, piece j: bytes 16·(64·j + l) of the chunk), parks them in its slab and reads back its own 4 rows.
template <int NF>
__device__ __forceinline__ void load_rows_staged(const float* __restrict__ rows, int lane, floatx4* __restrict__ slab,
                                                 float (&r)[4][NF]) {
  const floatx4* g = reinterpret_cast<const floatx4*>(rows);
  floatx4 t[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) t[j] = __builtin_nontemporal_load(g + j * 64 + lane);
#pragma unroll
  for (int j = 0; j < NF; ++j) slab[j * 64 + lane] = t[j];
  wave_lds_sync();
  union {
    floatx4 v[NF];
    float c[4][NF];
  } u;
#pragma unroll
  for (int j = 0; j < NF; ++j) u.v[j] = slab[lane * NF + j];
#pragma unroll
  for (int v = 0; v < 4; ++v)
#pragma unroll
    for (int i = 0; i < NF; ++i) r[v][i] = u.c[v][i];
  wave_lds_sync();  // every lane has its rows: the slab may be written again
}

// the wave's 256 rows of NF 4-byte elements out through its slab: NF contiguous 1-KiB stores
template <int NF, typename T>
__device__ __forceinline__ void store_rows_staged(T* __restrict__ rows, int lane, floatx4* __restrict__ slab,
                                                  const T (&r)[4][NF]) {
  static_assert(sizeof(T) == 4, "rows of 4-byte elements");
  union {
    floatx4 v[NF];
    T c[4][NF];
  } u;
#pragma unroll
  for (int v = 0; v < 4; ++v)
#pragma unroll
    for (int i = 0; i < NF; ++i) u.c[v][i] = r[v][i];
#pragma unroll
  for (int j = 0; j < NF; ++j) slab[lane * NF + j] = u.v[j];
  wave_lds_sync();
  floatx4* g = reinterpret_cast<floatx4*>(rows);
#pragma unroll
  for (int j = 0; j < NF; ++j) g[j * 64 + lane] = slab[j * 64 + lane];
  wave_lds_sync();  // the slab may be written again
}

// a wave's 256 pixels of an NF-channel fp32 map, lane l getting pixels wave_px + 4l .. + 3
template <int NF, int CL>
__device__ __forceinline__ void load_wave(const float* __restrict__ map, int64_t P, int64_t wave_px, int lane,
                                          floatx4* __restrict__ slab, float (&r)[4][NF]) {
  if constexpr (CL == RTI_COEF_PIXEL_MAJOR) {
    load_rows_staged<NF>(map + wave_px * NF, lane, slab, r);
  } else {
#pragma unroll
    for (int i = 0; i < NF; ++i) {
      const floatx4 t =
          __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(map + (int64_t)i * P + wave_px + 4 * lane));
#pragma unroll
      for (int v = 0; v < 4; ++v) r[v][i] = t[v];
    }
  }
}

template <int NF, int CL>
__device__ __forceinline__ void load_pixel(const float* __restrict__ map, int64_t P, int64_t p, float (&r)[NF]) {
#pragma unroll
  for (int i = 0; i < NF; ++i) r[i] = CL == RTI_COEF_PLANAR ? map[(int64_t)i * P + p] : map[p * NF + i];
}

}  // namespace lrgb_px
}  // namespace rti
