// rti_lane4.h -- what the kernels on rti_relight's lane map share: a lane owns 4 consecutive
// pixels, a wave 256, a block 1024.  A kernel is a source (how a wave's pixels reach registers), a per-pixel
// function (rti_*_px.h) and a sink (how they leave); the sources and sinks are here, once.  Everything on the device
// is __forceinline__; moving it here changed no operation of the kernels.
//
// A wave owns pixels [wave_px, wave_px + 256).  vec != 0 (P % 4 == 0 and every pointer aligned for its vector
// access: the entry decides) and the whole chunk inside the image: lane l owns pixels wave_px + 4l .. + 3 and uses
// the four-pixel forms below (load_wave, load_bytes4, store_rgb4).  Otherwise lane l takes pixels
// wave_px + 64j + l, j = 0..3, one at a time (load_pixel, load_bytes1) through the same per-pixel
// function, so a wave still covers its 256 pixels and the bits do not depend on the path.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <utility>

#include "rti_internal.h"
#include "rti_ptm_px.h"
#include "rti_quant8.h"
#include "rti_wave_lds.h"

namespace rti {
namespace lane4 {

// ---- launch -----------------------------------------------------------------------------------------------------

// a launch argument as the kernel's parameter type A: a void pointer (an entry's `void* out`, `const void* coef`)
// becomes the kernel's typed pointer; everything else converts implicitly, as in a direct launch
template <typename A, typename B>
inline A launch_arg(B&& b) {
  using V = std::remove_cv_t<std::remove_pointer_t<std::decay_t<B>>>;
  if constexpr (std::is_pointer_v<A> && std::is_pointer_v<std::decay_t<B>> && std::is_void_v<V>)
    return static_cast<A>(b);
  else
    return std::forward<B>(b);
}

// the lane map's launch: kern<<<ceil(P / 1024), 256, 0, s>>>(args...)
template <typename... A, typename... B>
inline void launch(void (*kern)(A...), int64_t P, hipStream_t s, B&&... args) {
  hipLaunchKernelGGL(kern, dim3(grid_1d(P, 1024)), dim3(256), 0, s, launch_arg<A>(std::forward<B>(args))...);
}

// ---- fp32 maps in and out ------------------------------------------------------------------------------------------

using lds::wave_lds_sync;

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

// ---- the RGB sink ------------------------------------------------------------------------------------------------

// whether a kernel that writes RGB rows of TO stages them (its slab then holds 3 elements per pixel)
template <typename TO>
constexpr bool rgb_staged() { return sizeof(TO) == 4; }

// the lane's four RGB pixels into the wave's 256 rows: fp32 / int32 as three whole 1-KiB stores through the slab,
// uint8 as the lane's 12 bytes in three dwords
template <typename TO>
__device__ __forceinline__ void store_rgb4(TO* __restrict__ rows, int lane, floatx4* __restrict__ slab,
                                           const TO (&o)[4][3]) {
  if constexpr (rgb_staged<TO>())
    store_rows_staged<3, TO>(rows, lane, slab, o);
  else
    quant8::store_dwords<12>(rows + 12 * lane, &o[0][0]);
}

// ---- the byte sources: 8-bit PTM-6 payloads ----------------------------------------------

constexpr int CB = ptm_px::K;  // coefficient bytes of a pixel (and channel): PTM-6
using quant8::u32x2;

// four pixels of an 8-bit RGB PTM: three blocks of 6 bytes per pixel.  A lane's 24 bytes of a block are three
// 8-byte loads.
struct Rgb8Px {
  union {
    u32x2 v[3];
    uint8_t b[4][CB];
  } c[3];
};

__device__ __forceinline__ void load_bytes4(const uint8_t* __restrict__ coef8, int64_t P, int64_t p0, Rgb8Px& r) {
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const u32x2* s = reinterpret_cast<const u32x2*>(coef8 + ((int64_t)ch * P + p0) * CB);
#pragma unroll
    for (int w = 0; w < 3; ++w) r.c[ch].v[w] = s[w];
  }
}

__device__ __forceinline__ void load_bytes1(const uint8_t* __restrict__ coef8, int64_t P, int64_t p,
                                            uint8_t (&b)[3][CB]) {
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
#pragma unroll
    for (int j = 0; j < CB; ++j) b[ch][j] = coef8[((int64_t)ch * P + p) * CB + j];
}

// four pixels of an 8-bit LRGB PTM: 6 coefficient bytes and 3 colour bytes per pixel.  A lane's 24 + 12 bytes are three 8-byte and
// three 4-byte loads, issued in turn.
struct Lrgb8Px {
  union {
    u32x2 v[3];
    uint8_t b[4][CB];
  } cb;
  union {
    uint32_t v[3];
    uint8_t b[4][3];
  } rb;
};

__device__ __forceinline__ void load_bytes4(const uint8_t* __restrict__ coef8, const uint8_t* __restrict__ rgb8,
                                            int64_t p0, Lrgb8Px& r) {
  const u32x2* c2 = reinterpret_cast<const u32x2*>(coef8 + p0 * CB);
  const uint32_t* r4 = reinterpret_cast<const uint32_t*>(rgb8 + p0 * 3);
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    r.cb.v[w] = c2[w];
    r.rb.v[w] = r4[w];
  }
}

__device__ __forceinline__ void load_bytes1(const uint8_t* __restrict__ coef8, const uint8_t* __restrict__ rgb8,
                                            int64_t p, uint8_t (&cb)[CB], uint8_t (&rb)[3]) {
#pragma unroll
  for (int i = 0; i < CB; ++i) cb[i] = coef8[p * CB + i];
#pragma unroll
  for (int c = 0; c < 3; ++c) rb[c] = rgb8[p * 3 + c];
}

// Dequantisation is not per-pixel arithmetic: a byte of plane j can only become one of 256 fp32 values, so a
// workgroup fills NTAB 256-entry fp32 tables in LDS and a pixel costs one LDS read per byte and no fp64 operation.
// tab[j][t] = (float)(((double)t − bias_j)·scale_j), j < 6, the fp32 value read_ptm gives byte t of plane j; a
// seventh table is the chroma's t / 255.  Each of the workgroup's 256 lanes forms entry t = threadIdx.x of every
// table in fp64 and rounds it once; the caller synchronises the workgroup.
constexpr int TAB = 256;

template <int NTAB>
__device__ __forceinline__ void fill_tables(const double* __restrict__ qparams, float* __restrict__ tab) {
#pragma clang fp contract(off)
  static_assert(NTAB == CB || NTAB == CB + 1, "six coefficient tables, and the chroma's");
  const double t = (double)threadIdx.x;
#pragma unroll
  for (int j = 0; j < CB; ++j) tab[j * TAB + threadIdx.x] = (float)((t - qparams[CB + j]) * qparams[j]);
  if constexpr (NTAB > CB) tab[CB * TAB + threadIdx.x] = (float)(t / 255.0);
}

}  // namespace lane4
}  // namespace rti
