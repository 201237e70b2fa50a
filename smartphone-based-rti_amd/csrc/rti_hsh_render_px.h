// rti_hsh_render_px.h -- what the renderers of HSH maps under a normal map share (rti_hsh_specular.hip,
// rti_hsh_gain.hip): the E basis rows in LDS, a lane's normal, the loop over the directions
// with its output rows, and the alignment rules of the staged paths.  rti_hsh8.hip's lane map: one pixel per
// lane, 64 consecutive pixels per wave, 256 per workgroup.  Everything on the device is __forceinline__; moving it
// here out of rti_hsh_specular.hip changed no operation of its kernels, only the order of some instructions and the
// registers they use (one instantiation takes one more VGPR, none changes its occupancy).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rti_basis.h"
#include "rti_hsh_px.h"

namespace rti {
namespace hsh_render {

using namespace hsh_px;  // the chain, the slab runs and the dequantisation

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

// the wave's 64 pixels at every direction: out[e][p][ch], value(e, o) giving the lane's C elements of direction e.
// vout (wave-uniform; a full wave, the alignment of rows_as_dwords): the wave's 64·C elements of a direction leave
// as whole dwords, through the slab unless a lane's element is one.
template <int C, typename TO, typename V>
__device__ __forceinline__ void render(int E, int64_t P, int64_t wave_px, int lane, bool live, bool vout,
                                       u32x4* __restrict__ slab, TO* __restrict__ out, V&& value) {
  constexpr int ND = 64 * C * (int)sizeof(TO) / 4;  // dwords of a wave and direction: 192, 64, 48 or 16
  for (int e = 0; e < E; ++e) {
    TO o[C];
    value(e, o);
    TO* rows = out + ((int64_t)e * P + wave_px) * C;
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
}

// ---- host: which launches may move whole pieces -------------------------------------------------------------------

// pixel-major rows as 16-byte pieces: every wave's run of every channel read starts on a 16-byte boundary
inline int maps_staged(const float* coef, int coef_layout, int C, int64_t cs) {
  return coef_layout == RTI_COEF_PIXEL_MAJOR && aligned_to(coef, 16) && (C == 1 || cs % 4 == 0) ? 1 : 0;
}
inline int normals_staged(const float* normals, int normal_layout) {
  return normal_layout == RTI_NORMAL_PIXEL_MAJOR && aligned_to(normals, 16) ? 1 : 0;
}
// a wave's 64·C output elements as dwords: direction e's rows start C·P·e elements into out
inline int rows_as_dwords(const void* out, int out_dtype, int64_t P) {
  return aligned_to(out, 4) && (out_dtype != RTI_U8 || P % 4 == 0) ? 1 : 0;
}

}  // namespace hsh_render
}  // namespace rti
