// rti_hsh8.hip -- 8-bit RGB HSH maps (gfx950): the payload of an .rti file on the device.
//
//     rti_hsh_qparams    one pass over three fp32 HSH maps -> the file's k scales and k biases
//     rti_hsh_quantise   the maps + those 2k floats -> 3k bytes per pixel, [p][c][k]
//     rti_relight_hsh8   the bytes + scales and biases -> E interleaved RGB images
//
// The arithmetic is include/rti.h's: step_j = scale_j / 255.0f once per workgroup, a coefficient is
// (float)raw·step_j + bias_j in two rounded fp32 operations, and an image is rti_relight's F32 path of those
// coefficients (the same basis_eval<float>, the same FMA chain, cvt_out), so it equals rti_relight's of the map
// read_rti builds bit for bit.  Only the quantiser uses fp64; nothing per pixel divides.
//
// Lane map: one pixel per lane, a wave owns 64 consecutive pixels, a workgroup 256.  A wave's bytes are one
// contiguous run of 64·3k bytes (1728 or 3072) that starts on a 16-byte boundary whenever coef8 does, so a full
// wave moves it as whole 16-byte pieces through its LDS slab (rti_relight.hip's load_coef_staged, for rows that
// are not dword-aligned): a lane then takes its 3k bytes out of the slab as dwords, realigned with a funnel
// shift for k = 9.  fp32 rows of the pixel-major maps and the output rows go through the slab the same way.
// Anything the pieces cannot serve (a pointer off its alignment, the last partial wave) loads and stores per
// lane, through the same per-pixel functions.  The two sources of a pixel are rti_hsh_px.h's, the store of a
// direction's rows rti_hsh_render_px.h's.
//
// The extremes pass is rti_quant8.h's, with a partial of 2k floats: the k minima and the k maxima over the three
// channels.  A zero minimum is stored as +0, so the bias does not depend on the order of the reduction either.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "rti_basis.h"
#include "rti_convert.h"
#include "rti_dispatch.h"
#include "rti_hsh_render_px.h"
#include "rti_quant8.h"
#include "rti_stack.h"

namespace rti {
namespace {

using namespace hsh_px;  // the chain, the slab runs and the two sources of a pixel
using namespace quant8;

constexpr int ECH = 64;     // directions per basis table in LDS (rti_relight's)
constexpr int CHUNK = 256;  // pixels of a workgroup

// ---- extremes ----------------------------------------------------------------------------------------------------
// q[j], q[K + j]: min and max of the finite values of term j in the three channels.

template <int K, int CL>
__global__ void __launch_bounds__(256)
hsh_extremes_k(const float* __restrict__ coef, int64_t cs, int64_t P, int vin, float* __restrict__ partial) {
  constexpr int SLAB = slab_v4(CL == RTI_COEF_PIXEL_MAJOR ? run_v4<4 * K>() : 0, 0);
  __shared__ u32x4 slabs[4 * SLAB];
  __shared__ float part[4][2 * K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float q[2 * K];
  ext_init<K>(q);
  const int64_t chunks = (P + CHUNK - 1) / CHUNK;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t wave_px = (c * 4 + wave) * 64;
    if (wave_px >= P) continue;  // wave-uniform
    float x[3][K];
    // a lane past the image gets NaNs, which the extremes skip
    load_px<K, 3, CL>(coef, cs, P, wave_px, lane, wave_px + lane < P, vin && wave_px + 64 <= P, NAN,
                      slabs + wave * SLAB, x);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
      for (int j = 0; j < K; ++j) ext_update(q[j], q[K + j], x[ch][j]);
  }
  const float r = ext_block_fold<K>(q, part);
  if (threadIdx.x < 2 * K) partial[(int64_t)blockIdx.x * (2 * K) + threadIdx.x] = r;
}

// n partials -> qparams; one workgroup
template <int K>
__global__ void __launch_bounds__(256)
hsh_qparams_k(const float* __restrict__ partial, int n, float* __restrict__ qparams) {
#pragma clang fp contract(off)
  __shared__ float part[4][2 * K];
  __shared__ float fin[2 * K];
  fold_partials<K>(partial, n, part, fin);
  if (threadIdx.x < K) {
    const int j = threadIdx.x;
    const float lo = fin[j], hi = fin[K + j];
    const bool has = lo <= hi;  // the term has a finite value
    const float d = hi - lo;
    qparams[j] = has && d > 0.0f && d <= FLT_MAX ? d : 1.0f;
    qparams[K + j] = has ? lo + 0.0f : 0.0f;  // -0.0 -> +0.0: min(-0, +0) depends on the order
  }
}

// ---- per-pixel quantisation (load_steps and dequantise_px: rti_hsh_px.h) ----------------------------------------

// three fp32 maps of a pixel -> its 3K bytes, [c][j], packed as lane_words packs them
template <int K>
__device__ __forceinline__ void quantise_px(const float (&x)[3][K], const float* __restrict__ qs,
                                            uint32_t (&w)[(3 * K + 3) / 4]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < (3 * K + 3) / 4; ++i) w[i] = 0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const double step = (double)qs[j], bias = (double)qs[K + j];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int i = c * K + j;
      w[i >> 2] |= byte_of(((double)x[c][j] - bias) / step) << (8 * (i & 3));
    }
  }
}

// ---- kernels ------------------------------------------------------------------------------------------------------
// Both: wave w of workgroup g owns pixels [(4g + w)·64, + 64).

template <int K, int CL>
__global__ void __launch_bounds__(256)
hsh_quantise_k(const float* __restrict__ coef, int64_t cs, int64_t P, int vin, int vout,
               const float* __restrict__ qparams, uint8_t* __restrict__ coef8) {
  constexpr int NB = 3 * K, NW = (NB + 3) / 4;
  constexpr int SLAB = slab_v4(CL == RTI_COEF_PIXEL_MAJOR ? run_v4<4 * K>() : 0, run_v4<NB>());
  __shared__ u32x4 slabs[4 * SLAB];
  __shared__ float qs[2 * K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32x4* slab = slabs + wave * SLAB;
  load_steps<K>(qparams, qs);
  __syncthreads();
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 64;
  if (wave_px >= P) return;  // wave-uniform; no workgroup barrier below
  const int64_t p = wave_px + lane;
  const bool live = p < P, full = wave_px + 64 <= P;
  float x[3][K];
  load_px<K, 3, CL>(coef, cs, P, wave_px, lane, live, vin && full, NAN, slab, x);
  uint32_t w[NW];
  quantise_px<K>(x, qs, w);
  if (vout && full) {  // wave-uniform
    put_lane_words<NB>(slab, lane, w);
    run_out<NB>(coef8 + wave_px * NB, lane, slab);
  } else if (live) {
#pragma unroll
    for (int i = 0; i < NB; ++i) coef8[p * NB + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  }
}

template <int K, typename TO>
__global__ void __launch_bounds__(256)
relight_hsh8_k(const uint8_t* __restrict__ coef8, int64_t P, int vin, int vout,
               const float* __restrict__ qparams, const double* __restrict__ luv, int E, TO* __restrict__ out) {
  constexpr int SLAB = slab_v4(run_v4<3 * K>(), run_v4<12>());  // bytes in; 64 rows of 3 elements of <= 4 bytes out
  __shared__ u32x4 slabs[4 * SLAB];
  __shared__ float btab[ECH * K];
  __shared__ float qs[2 * K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32x4* slab = slabs + wave * SLAB;
  load_steps<K>(qparams, qs);
  __syncthreads();
  // every lane stays to the end: the basis tables are filled by the whole workgroup
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 64;
  const bool live = wave_px + lane < P, full = wave_px + 64 <= P;  // full: wave-uniform
  float c[3][K];
  load_px8<K>(coef8, wave_px, lane, live, vin && full, slab, qs, c);

  for (int e0 = 0; e0 < E; e0 += ECH) {
    const int ne = min(ECH, E - e0);
    if (e0) __syncthreads();  // the previous table has been read
    for (int i = threadIdx.x; i < ne; i += 256) {
      float b[K];
      hsh_eval<float>((float)luv[2 * (e0 + i)], (float)luv[2 * (e0 + i) + 1], K, b);  // basis_eval<float>'s HSH branch
#pragma unroll
      for (int k = 0; k < K; ++k) btab[i * K + k] = b[k];
    }
    __syncthreads();
    for (int e = 0; e < ne; ++e) {
      const float* b = btab + e * K;
      TO o[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) o[ch] = cvt_out<TO>(dot_k<K>(c[ch], b));
      hsh_render::store_dir<3, TO>(o, out + ((int64_t)(e0 + e) * P + wave_px) * 3, lane, live, vout && full, slab);
    }
  }
}

// the checks rti_hsh_qparams and rti_hsh_quantise share, in the order include/rti.h lists them
int check_hsh_maps(const char* entry, int basis, int layout, int64_t stride, int64_t P) {
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", entry);
  if (!hsh_basis(basis)) return fail(RTI_ERR_UNSUPPORTED, "%s: basis %d (HSH-9 and HSH-16 only)", entry, basis);
  return check_rgb_maps(entry, basis_terms(basis), layout, stride, P);
}

}  // namespace
}  // namespace rti

using namespace rti;

extern "C" int64_t rti_hsh_qparams_workspace(int k, int64_t P) {
  return P < 1 || (k != 9 && k != 16) ? 0 : qparams_blocks(P, CHUNK) * 2 * k * (int64_t)sizeof(float);
}

extern "C" int rti_hsh_qparams(const float* coef, int basis, int coef_layout, int64_t coef_channel_stride, int64_t P,
                               void* workspace, float* qparams, rti_stream_t stream) {
  const char* const E = "rti_hsh_qparams";
  if (int st = check_pointers(E, {coef, workspace, qparams})) return st;
  if (int st = check_hsh_maps(E, basis, coef_layout, coef_channel_stride, P)) return st;
  if (!aligned_to(workspace, 4) || !aligned_to(qparams, 4))
    return fail(RTI_ERR_BAD_ARG, "%s: workspace and qparams must be 4-byte aligned", E);
  const int k = basis_terms(basis);
  const int64_t cs = coef_channel_stride ? coef_channel_stride : P * k;
  const int blocks = (int)qparams_blocks(P, CHUNK);
  float* partial = static_cast<float*>(workspace);
  const int vin = maps_staged(coef, coef_layout, 3, cs);
  const hipStream_t s = (hipStream_t)stream;
  note_launches(2);
  with_hsh_terms(k, [&](auto kt) {
    with_layout(coef_layout, [&](auto l) {
      hipLaunchKernelGGL((hsh_extremes_k<decltype(kt)::value, decltype(l)::value>), dim3(blocks), dim3(256), 0, s, coef,
                         cs, P, vin, partial);
    });
  });
  if (int st = check_launch(E)) return st;
  with_hsh_terms(k, [&](auto kt) {
    hipLaunchKernelGGL(hsh_qparams_k<decltype(kt)::value>, dim3(1), dim3(256), 0, s, partial, blocks, qparams);
  });
  return check_launch(E);
}

extern "C" int rti_hsh_quantise(const float* coef, int basis, int coef_layout, int64_t coef_channel_stride, int64_t P,
                                const float* qparams, uint8_t* coef8, rti_stream_t stream) {
  const char* const E = "rti_hsh_quantise";
  if (int st = check_pointers(E, {coef, qparams, coef8})) return st;
  if (int st = check_hsh_maps(E, basis, coef_layout, coef_channel_stride, P)) return st;
  if (!aligned_to(qparams, 4)) return fail(RTI_ERR_BAD_ARG, "%s: qparams must be 4-byte aligned", E);
  const int k = basis_terms(basis);
  const int64_t cs = coef_channel_stride ? coef_channel_stride : P * k;
  const int vin = maps_staged(coef, coef_layout, 3, cs), vout = aligned_to(coef8, 16) ? 1 : 0;
  note_launches(1);
  with_hsh_terms(k, [&](auto kt) {
    with_layout(coef_layout, [&](auto l) {
      hipLaunchKernelGGL((hsh_quantise_k<decltype(kt)::value, decltype(l)::value>), dim3(grid_1d(P, CHUNK)), dim3(256), 0,
                         (hipStream_t)stream, coef, cs, P, vin, vout, qparams, coef8);
    });
  });
  return check_launch(E);
}

extern "C" int rti_relight_hsh8(const uint8_t* coef8, int basis, int64_t P, const float* qparams, const double* luv,
                                int E_, void* out, int out_dtype, rti_stream_t stream) {
  const char* const E = "rti_relight_hsh8";
  if (int st = check_pointers(E, {coef8, qparams, luv, out})) return st;
  if (P < 1 || E_ < 1) return fail(RTI_ERR_BAD_ARG, "%s: P and E must be positive", E);
  if (!hsh_basis(basis)) return fail(RTI_ERR_UNSUPPORTED, "%s: basis %d (HSH-9 and HSH-16 only)", E, basis);
  if (int st = check_out_dtype(E, out_dtype)) return st;
  if (!aligned_to(qparams, 4)) return fail(RTI_ERR_BAD_ARG, "%s: qparams must be 4-byte aligned", E);
  const int vin = aligned_to(coef8, 16) ? 1 : 0;
  const int vout = hsh_render::rows_as_dwords(out, out_dtype, P);
  note_launches(1);
  with_hsh_terms(basis_terms(basis), [&](auto kt) {
    with_out(out_dtype, [&](auto t) {
      using TO = decltype(t);
      hipLaunchKernelGGL((relight_hsh8_k<decltype(kt)::value, TO>), dim3(grid_1d(P, CHUNK)), dim3(256), 0,
                         (hipStream_t)stream, coef8, P, vin, vout, qparams, luv, E_, static_cast<TO*>(out));
    });
  });
  return check_launch(E);
}
