// rti_lrgb8.hip -- 8-bit LRGB PTMs (gfx950): the payload of a PTM_FORMAT_LRGB file on the device.
//
//     rti_lrgb_qparams    one pass over an fp32 LRGB map -> the file's six scales, six biases and the chroma scale s
//     rti_lrgb_quantise   the map + those 13 doubles -> 6 coefficient bytes and 3 colour bytes per pixel
//     rti_relight_lrgb8   the 9 bytes + scales and biases -> E interleaved RGB images
//     rti_relight_lrgb8_enhanced   the 9 bytes -> one diffuse gain or specular RGB image
//
// The arithmetic is rti/io.py's (write_ptm, _ptm_quantise, read_ptm), in fp64 from the fp32 map with FP contraction
// off, so the bytes equal the host's and an image rendered from the bytes equals rti_relight_lrgb's of the fp32 map
// read_ptm would build: the dequantised values are rounded through fp32 on purpose and then go through the same
// dot6 / rgb_of (rti_lrgb_px.h).
//
// All kernels keep rti_relight's lane map (a lane owns 4 consecutive pixels, a wave 256, a block 1024) and
// rti_lrgb.hip's loads of the fp32 map.  The extremes pass is rti_quant8.h's, with a partial of 13 floats: the six
// minima, the six maxima and the chroma max.  The byte blocks are read and written as whole dwords per lane
// (24 B + 12 B).
//
// A launch whose P is no multiple of 4 or whose pointers are not aligned for the vector accesses, and the last
// partial wave of any launch, take one pixel per lane through the same per-pixel functions.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "rti_basis.h"
#include "rti_convert.h"
#include "rti_dispatch.h"
#include "rti_enhance_px.h"
#include "rti_lane4.h"
#include "rti_lrgb_px.h"
#include "rti_quant8.h"

namespace rti {
namespace {

using namespace lrgb_px;
using namespace lane4;  // the wave loads of the fp32 map, the byte sources, the tables and the RGB sink
using namespace quant8;

constexpr int NQ = 2 * K + 1;  // a partial: lo[6], hi[6], the chroma max; qparams: scale[6], bias[6], s

// ---- extremes ----------------------------------------------------------------------------------------------------
// q[j], q[6 + j]: min and max of the finite values of plane j; q[12]: max of the finite chroma values.

__device__ __forceinline__ void ext_pixel(float (&q)[NQ], const float (&m)[NL]) {
#pragma unroll
  for (int j = 0; j < K; ++j) ext_update(q[j], q[K + j], m[j]);
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (is_finite(m[K + c])) q[2 * K] = fmaxf(q[2 * K], m[K + c]);
}

template <int CL>
__global__ void __launch_bounds__(256)
lrgb_extremes_k(const float* __restrict__ lrgb, int64_t P, int vec, float* __restrict__ partial) {
  constexpr int SLAB = slab_v4(CL == RTI_COEF_PIXEL_MAJOR ? NL : 0, 0);
  __shared__ floatx4 slabs[4 * SLAB];
  __shared__ float part[4][NQ];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  floatx4* slab = slabs + wave * SLAB;
  float q[NQ];
  ext_init<K>(q);
  const int64_t chunks = (P + 1023) / 1024;
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t wave_px = (c * 4 + wave) * 256;
    if (wave_px >= P) continue;       // wave-uniform
    if (vec && wave_px + 256 <= P) {  // wave-uniform
      float m[4][NL];
      load_wave<NL, CL>(lrgb, P, wave_px, lane, slab, m);
#pragma unroll
      for (int v = 0; v < 4; ++v) ext_pixel(q, m[v]);
    } else {
      for (int j = 0; j < 4; ++j) {
        const int64_t p = wave_px + 64 * j + lane;
        if (p >= P) break;
        float m[NL];
        load_pixel<NL, CL>(lrgb, P, p, m);
        ext_pixel(q, m);
      }
    }
  }
  const float r = ext_block_fold<K>(q, part);
  if (threadIdx.x < NQ) partial[(int64_t)blockIdx.x * NQ + threadIdx.x] = r;
}

// n partials -> qparams; one workgroup
__global__ void __launch_bounds__(256)
lrgb_qparams_k(const float* __restrict__ partial, int n, double* __restrict__ qparams) {
  __shared__ float part[4][NQ];
  __shared__ float fin[NQ];
  fold_partials<K>(partial, n, part, fin);
  const double s = fin[2 * K] > 0.0f ? (double)fin[2 * K] : 1.0;
  if (threadIdx.x == 0) qparams[2 * K] = s;
  if (threadIdx.x < K) {
    const int j = threadIdx.x;
    ptm_scale_bias(fin[j], fin[K + j], s, qparams[j], qparams[K + j]);
  }
}

// ---- per-pixel quantisation and dequantisation (fp64, no contraction) -------------------------------------------

// one fp32 LRGB pixel -> its 6 coefficient bytes and 3 colour bytes (rti/io.py: _ptm_quantise, write_ptm)
__device__ __forceinline__ void quantise_px(const float (&m)[NL], const QParams<K>& q, double s, uint8_t (&cb)[K],
                                            uint8_t (&rb)[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const double a = (double)m[j];
    cb[j] = coef_byte(a, a * s, q.scale[j], q.bias[j]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) rb[c] = (uint8_t)byte_of(255.0 * (double)m[K + c] / s);
}

// 9 bytes -> the fp32 LRGB pixel read_ptm builds from them
__device__ __forceinline__ void dequantise_px(const uint8_t (&cb)[K], const uint8_t (&rb)[3], const QParams<K>& q,
                                              float (&m)[NL]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < K; ++j) m[j] = (float)(((double)cb[j] - q.bias[j]) * q.scale[j]);
#pragma unroll
  for (int c = 0; c < 3; ++c) m[K + c] = (float)((double)rb[c] / 255.0);
}

// ---- kernels ------------------------------------------------------------------------------------------------------
// Both: a wave owns pixels [wave_px, wave_px + 256), as rti_lrgb.hip's kernels.

template <int CL>
__global__ void __launch_bounds__(256)
lrgb_quantise_k(const float* __restrict__ lrgb, int64_t P, int vec, const double* __restrict__ qparams,
                uint8_t* __restrict__ coef8, uint8_t* __restrict__ rgb8) {
  constexpr int SLAB = slab_v4(CL == RTI_COEF_PIXEL_MAJOR ? NL : 0, 0);
  __shared__ floatx4 slabs[4 * SLAB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 256;
  if (wave_px >= P) return;
  const QParams<K> q = load_qparams<K>(qparams);
  const double s = qparams[2 * K];
  if (vec && wave_px + 256 <= P) {  // wave-uniform
    float m[4][NL];
    load_wave<NL, CL>(lrgb, P, wave_px, lane, slabs + wave * SLAB, m);
    uint8_t cb[4][K], rb[4][3];
#pragma unroll
    for (int v = 0; v < 4; ++v) quantise_px(m[v], q, s, cb[v], rb[v]);
    const int64_t p0 = wave_px + 4 * lane;
    store_dwords<4 * K>(coef8 + p0 * K, &cb[0][0]);
    store_dwords<12>(rgb8 + p0 * 3, &rb[0][0]);
    return;
  }
  for (int j = 0; j < 4; ++j) {
    const int64_t p = wave_px + 64 * j + lane;
    if (p >= P) break;
    float m[NL];
    load_pixel<NL, CL>(lrgb, P, p, m);
    uint8_t cb[K], rb[3];
    quantise_px(m, q, s, cb, rb);
#pragma unroll
    for (int i = 0; i < K; ++i) coef8[p * K + i] = cb[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb8[p * 3 + c] = rb[c];
  }
}

template <typename TO>
__global__ void __launch_bounds__(256)
relight_lrgb8_k(const uint8_t* __restrict__ coef8, const uint8_t* __restrict__ rgb8, int64_t P, int vec,
                const double* __restrict__ qparams, const double* __restrict__ luv, int E, TO* __restrict__ out) {
  constexpr int SLAB = slab_v4(0, rgb_staged<TO>() ? 3 : 0);
  __shared__ floatx4 slabs[4 * SLAB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 256;
  if (wave_px >= P) return;
  floatx4* slab = slabs + wave * SLAB;
  const QParams<K> q = load_qparams<K>(qparams);  // s is not used: the colour bytes are chroma·255
  if (vec && wave_px + 256 <= P) {                // wave-uniform
    const int64_t p0 = wave_px + 4 * lane;
    Lrgb8Px r;
    load_bytes4(coef8, rgb8, p0, r);
    float m[4][NL];
#pragma unroll
    for (int v = 0; v < 4; ++v) dequantise_px(r.cb.b[v], r.rb.b[v], q, m[v]);
    for (int e = 0; e < E; ++e) {
      double b[K];
      ptm_eval<double>(luv[2 * e], luv[2 * e + 1], b);
      TO o[4][3];
#pragma unroll
      for (int v = 0; v < 4; ++v) rgb_of<TO>(m[v], b, o[v]);
      TO* rows = out + ((int64_t)e * P + wave_px) * 3;
      store_rgb4<TO>(rows, lane, slab, o);
    }
    return;
  }
  for (int j = 0; j < 4; ++j) {
    const int64_t p = wave_px + 64 * j + lane;
    if (p >= P) break;
    uint8_t cb[K], rb[3];
    load_bytes1(coef8, rgb8, p, cb, rb);
    float m[NL];
    dequantise_px(cb, rb, q, m);
    for (int e = 0; e < E; ++e) {
      double b[K];
      ptm_eval<double>(luv[2 * e], luv[2 * e + 1], b);
      TO o[3];
      rgb_of<TO>(m, b, o);
      TO* px = out + ((int64_t)e * P + p) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) px[c] = o[c];
    }
  }
}

// ---- enhanced rendering from the bytes ---------------------------------------------------------
// A byte can only become one of 256 fp32 values, so the workgroup fills seven 256-entry tables in LDS (7 KiB; lane t
// forms entry t of each in fp64 and rounds it once: rti_lane4.h's fill_tables<7>, the seventh the chroma's byte / 255) and a
// pixel costs 9 LDS reads instead of six fp64 products and three fp64 divisions.  The tables hold the very values
// dequantise_px gives, so the image is rti_relight_lrgb_enhanced's of the dequantised map bit for bit.

__device__ __forceinline__ void lookup_px(const uint8_t (&cb)[K], const uint8_t (&rb)[3], const float* __restrict__ tab,
                                          float (&m)[NL]) {
#pragma unroll
  for (int j = 0; j < K; ++j) m[j] = tab[j * TAB + cb[j]];
#pragma unroll
  for (int c = 0; c < 3; ++c) m[K + c] = tab[K * TAB + rb[c]];
}

template <typename TO, int MODE>
__global__ void __launch_bounds__(256)
relight_lrgb8_enhanced_k(const uint8_t* __restrict__ coef8, const uint8_t* __restrict__ rgb8, int64_t P, int vec,
                         const double* __restrict__ qparams, enhance_px::Enhance q, TO* __restrict__ out) {
  constexpr int SLAB = slab_v4(0, rgb_staged<TO>() ? 3 : 0);
  __shared__ floatx4 slabs[4 * SLAB];
  __shared__ float tab[(K + 1) * TAB];
  fill_tables<K + 1>(qparams, tab);
  __syncthreads();  // the one workgroup barrier: waves may leave below
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 256;
  if (wave_px >= P) return;
  floatx4* slab = slabs + wave * SLAB;
  if (vec && wave_px + 256 <= P) {  // wave-uniform
    const int64_t p0 = wave_px + 4 * lane;
    Lrgb8Px r;
    load_bytes4(coef8, rgb8, p0, r);
    TO o[4][3];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      float m[NL];
      lookup_px(r.cb.b[v], r.rb.b[v], tab, m);
      enhance_px::lrgb_enhanced<MODE, TO>(m, q, o[v]);
    }
    TO* rows = out + wave_px * 3;
    store_rgb4<TO>(rows, lane, slab, o);
    return;
  }
  for (int j = 0; j < 4; ++j) {
    const int64_t p = wave_px + 64 * j + lane;
    if (p >= P) break;
    uint8_t cb[K], rb[3];
    load_bytes1(coef8, rgb8, p, cb, rb);
    float m[NL];
    lookup_px(cb, rb, tab, m);
    TO o[3];
    enhance_px::lrgb_enhanced<MODE, TO>(m, q, o);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[p * 3 + c] = o[c];
  }
}

int check_lrgb_layout(const char* entry, int layout) {
  if (layout != RTI_COEF_PIXEL_MAJOR && layout != RTI_COEF_PLANAR)
    return fail(RTI_ERR_BAD_ARG, "%s: lrgb layout %d", entry, layout);
  return RTI_OK;
}

}  // namespace
}  // namespace rti

using namespace rti;

extern "C" int64_t rti_lrgb_qparams_workspace(int64_t P) {
  return P < 1 ? 0 : qparams_blocks(P, 1024) * NQ * (int64_t)sizeof(float);
}

extern "C" int rti_lrgb_qparams(const float* lrgb, int lrgb_layout, int64_t P, void* workspace, double* qparams,
                                rti_stream_t stream) {
  const char* const E = "rti_lrgb_qparams";
  if (int st = check_pointers(E, {lrgb, workspace, qparams})) return st;
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  if (int st = check_lrgb_layout(E, lrgb_layout)) return st;
  if (!aligned_to(workspace, 4) || !aligned_to(qparams, 8))
    return fail(RTI_ERR_BAD_ARG, "%s: workspace must be 4-byte and qparams 8-byte aligned", E);
  const int blocks = (int)qparams_blocks(P, 1024);
  const int vec = P % 4 == 0 && aligned_to(lrgb, 16) ? 1 : 0;
  float* partial = static_cast<float*>(workspace);
  note_launches(2);
  with_layout(lrgb_layout, [&](auto cl) {
    hipLaunchKernelGGL((lrgb_extremes_k<decltype(cl)::value>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, lrgb, P,
                       vec, partial);
  });
  if (int st = check_launch(E)) return st;
  hipLaunchKernelGGL(lrgb_qparams_k, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, blocks, qparams);
  return check_launch(E);
}

extern "C" int rti_lrgb_quantise(const float* lrgb, int lrgb_layout, int64_t P, const double* qparams, uint8_t* coef8,
                                 uint8_t* rgb8, rti_stream_t stream) {
  const char* const E = "rti_lrgb_quantise";
  if (int st = check_pointers(E, {lrgb, qparams, coef8, rgb8})) return st;
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  if (int st = check_lrgb_layout(E, lrgb_layout)) return st;
  if (int st = check_qparams_aligned(E, qparams)) return st;
  const int vec = P % 4 == 0 && aligned_to(lrgb, 16) && aligned_to(coef8, 4) && aligned_to(rgb8, 4) ? 1 : 0;
  note_launches(1);
  with_layout(lrgb_layout, [&](auto cl) {
    launch(lrgb_quantise_k<decltype(cl)::value>, P, (hipStream_t)stream, lrgb, P, vec, qparams, coef8, rgb8);
  });
  return check_launch(E);
}

extern "C" int rti_relight_lrgb8(const uint8_t* coef8, const uint8_t* rgb8, int64_t P, const double* qparams,
                                 const double* luv, int E_, void* out, int out_dtype, rti_stream_t stream) {
  const char* const E = "rti_relight_lrgb8";
  if (int st = check_pointers(E, {coef8, rgb8, qparams, luv, out})) return st;
  if (P < 1 || E_ < 1) return fail(RTI_ERR_BAD_ARG, "%s: P and E must be positive", E);
  if (int st = check_out_dtype(E, out_dtype)) return st;
  if (int st = check_qparams_aligned(E, qparams)) return st;
  const int vec = P % 4 == 0 && aligned_to(coef8, 8) && aligned_to(rgb8, 4) && rgb_out_vec(out, out_dtype) ? 1 : 0;
  note_launches(1);
  with_out(out_dtype, [&](auto t) {
    launch(relight_lrgb8_k<decltype(t)>, P, (hipStream_t)stream, coef8, rgb8, P, vec, qparams, luv, E_, out);
  });
  return check_launch(E);
}

extern "C" int rti_relight_lrgb8_enhanced(const uint8_t* coef8, const uint8_t* rgb8, int64_t P, const double* qparams,
                                          int mode, double gain, double kd, double ks, int spec_exp, double lu,
                                          double lv, void* out, int out_dtype, rti_stream_t stream) {
  const char* const E = "rti_relight_lrgb8_enhanced";
  if (int st = check_pointers(E, {coef8, rgb8, qparams, out})) return st;
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  if (int st = enhance_px::check_enhance(E, mode, gain, kd, ks, spec_exp, lu, lv)) return st;
  if (int st = check_out_dtype(E, out_dtype)) return st;
  if (int st = check_qparams_aligned(E, qparams)) return st;
  const int vec = P % 4 == 0 && aligned_to(coef8, 8) && aligned_to(rgb8, 4) && rgb_out_vec(out, out_dtype) ? 1 : 0;
  const enhance_px::Enhance q = enhance_px::enhance_args(gain, kd, ks, spec_exp, lu, lv);
  note_launches(1);
  enhance_px::with_mode_out(mode, out_dtype, [&](auto m, auto t) {
    launch(relight_lrgb8_enhanced_k<decltype(t), decltype(m)::value>, P, (hipStream_t)stream, coef8, rgb8, P, vec,
           qparams, q, out);
  });
  return check_launch(E);
}
