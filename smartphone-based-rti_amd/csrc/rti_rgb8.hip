// rti_rgb8.hip -- 8-bit RGB PTMs (gfx950): the payload of a PTM_FORMAT_RGB file on the device.
//
//     rti_rgb8_qparams    one pass over three fp32 PTM-6 maps -> the file's six scales and six biases
//     rti_rgb8_quantise   the maps + those 12 doubles -> three blocks of 6 bytes per pixel, R then G then B
//     rti_relight_rgb8    the 18 bytes + scales and biases -> E interleaved RGB images
//     rti_rgb8_normals    the 18 bytes -> rti_ptm_normals of their fp32 luminance map
//     rti_relight_rgb8_enhanced   the 18 bytes -> one diffuse gain or specular RGB image
//
// The quantiser's arithmetic is rti/io.py's (write_ptm(format="rgb"), _ptm_quantise), in fp64 from the fp32 maps with
// FP contraction off, so the bytes equal the host's.  A dequantised coefficient is the fp32 value read_ptm builds,
// (float)(((double)raw − bias_j)·scale_j); the image is rti_relight's F32 path of those values (the same
// basis_eval<float>, the same FMA chain, cvt_out) and the normals are rti_ptm_normals' per-pixel function
// (rti_ptm_px.h) of their fp32 luminance, so both equal what the fp32 entries give for the dequantised maps bit for
// bit.
//
// Dequantisation is not per-pixel arithmetic: a byte of plane j can only become one of 256 fp32 values, so every
// workgroup of the two reading kernels first fills six 256-entry fp32 tables in LDS (6 KiB; each of its 256 lanes
// forms entry t = threadIdx.x of the six tables in fp64 and rounds it once) and a pixel then costs 18 LDS reads and
// no fp64 operation.  The table holds the very (float) values the expression gives, so nothing downstream can tell.
//
// All kernels keep rti_relight's lane map (a lane owns 4 consecutive pixels, a wave 256, a block 1024) and
// rti_lane4.h's loads of the fp32 maps.  A lane's 24 bytes of a channel block are contiguous: they are read as
// three 8-byte loads per block and written as six dwords.  The extremes pass is rti_quant8.h's, with a partial of 12
// floats: the six minima and the six maxima over the three channels.
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
#include "rti_hsh_px.h"
#include "rti_lane4.h"
#include "rti_ptm_px.h"
#include "rti_quant8.h"
#include "rti_rgb_px.h"
#include "rti_stack.h"

namespace rti {
namespace {

using namespace lane4;  // the wave loads of fp32 maps, the byte source, the tables and the sinks
using rgb_px::K;        // PTM-6
using hsh_px::dot_k;      // rti_relight's fp32 chain
using namespace quant8;
using rgb_px::luminance;  // the fp32 luminance, its normal and the weights: shared with rti_rgb.hip
using rgb_px::normal_px;
using rgb_px::Weights;

constexpr int NQ = 2 * K;  // a partial: lo[6], hi[6]; qparams: scale[6], bias[6]

// ---- extremes ----------------------------------------------------------------------------------------------------
// q[j], q[6 + j]: min and max of the finite values of plane j in the three channels.

__device__ __forceinline__ void ext_pixel(float (&q)[NQ], const float (&m)[K]) {
#pragma unroll
  for (int j = 0; j < K; ++j) ext_update(q[j], q[K + j], m[j]);
}

template <int CL>
__global__ void __launch_bounds__(256)
rgb_extremes_k(const float* __restrict__ coef, int64_t cs, int64_t P, int vec, float* __restrict__ partial) {
  constexpr int SLAB = slab_v4(CL == RTI_COEF_PIXEL_MAJOR ? K : 0, 0);
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
#pragma unroll 1
      for (int ch = 0; ch < 3; ++ch) {
        float m[4][K];
        load_wave<K, CL>(coef + ch * cs, P, wave_px, lane, slab, m);
#pragma unroll
        for (int v = 0; v < 4; ++v) ext_pixel(q, m[v]);
      }
    } else {
      for (int j = 0; j < 4; ++j) {
        const int64_t p = wave_px + 64 * j + lane;
        if (p >= P) break;
#pragma unroll 1
        for (int ch = 0; ch < 3; ++ch) {
          float m[K];
          load_pixel<K, CL>(coef + ch * cs, P, p, m);
          ext_pixel(q, m);
        }
      }
    }
  }
  const float r = ext_block_fold<K>(q, part);
  if (threadIdx.x < NQ) partial[(int64_t)blockIdx.x * NQ + threadIdx.x] = r;
}

// n partials -> qparams; one workgroup
__global__ void __launch_bounds__(256)
rgb_qparams_k(const float* __restrict__ partial, int n, double* __restrict__ qparams) {
  __shared__ float part[4][NQ];
  __shared__ float fin[NQ];
  fold_partials<K>(partial, n, part, fin);
  if (threadIdx.x < K) {
    const int j = threadIdx.x;
    ptm_scale_bias(fin[j], fin[K + j], 1.0, qparams[j], qparams[K + j]);
  }
}

// ---- per-pixel quantisation (fp64, no contraction) ---------------------------------------------------------------

// six fp32 coefficients of one channel of a pixel -> their bytes (rti/io.py: _ptm_quantise)
__device__ __forceinline__ void quantise_px(const float (&m)[K], const QParams<K>& q, uint8_t (&cb)[K]) {
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const double x = (double)m[j];
    cb[j] = coef_byte(x, x, q.scale[j], q.bias[j]);
  }
}

// ---- dequantisation: six 256-entry tables per workgroup (rti_lane4.h: fill_tables<6>, Rgb8Px, load_bytes) -------

__device__ __forceinline__ void dequantise_px(const uint8_t (&b)[K], const float* __restrict__ tab, float (&a)[K]) {
#pragma unroll
  for (int j = 0; j < K; ++j) a[j] = tab[j * TAB + b[j]];
}

// ---- kernels ------------------------------------------------------------------------------------------------------
// All: a wave owns pixels [wave_px, wave_px + 256), as rti_lrgb8.hip's kernels.

template <int CL>
__global__ void __launch_bounds__(256)
rgb_quantise_k(const float* __restrict__ coef, int64_t cs, int64_t P, int vec, const double* __restrict__ qparams,
               uint8_t* __restrict__ coef8) {
  constexpr int SLAB = slab_v4(CL == RTI_COEF_PIXEL_MAJOR ? K : 0, 0);
  __shared__ floatx4 slabs[4 * SLAB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 256;
  if (wave_px >= P) return;
  const QParams<K> q = load_qparams<K>(qparams);
  if (vec && wave_px + 256 <= P) {  // wave-uniform
    const int64_t p0 = wave_px + 4 * lane;
#pragma unroll 1
    for (int ch = 0; ch < 3; ++ch) {
      float m[4][K];
      load_wave<K, CL>(coef + ch * cs, P, wave_px, lane, slabs + wave * SLAB, m);
      uint8_t cb[4][K];
#pragma unroll
      for (int v = 0; v < 4; ++v) quantise_px(m[v], q, cb[v]);
      store_dwords<4 * K>(coef8 + ((int64_t)ch * P + p0) * K, &cb[0][0]);
    }
    return;
  }
  for (int j = 0; j < 4; ++j) {
    const int64_t p = wave_px + 64 * j + lane;
    if (p >= P) break;
#pragma unroll 1
    for (int ch = 0; ch < 3; ++ch) {
      float m[K];
      load_pixel<K, CL>(coef + ch * cs, P, p, m);
      uint8_t cb[K];
      quantise_px(m, q, cb);
#pragma unroll
      for (int i = 0; i < K; ++i) coef8[((int64_t)ch * P + p) * K + i] = cb[i];
    }
  }
}

// one pixel's three channels at the basis row b, converted once: rti_relight's F32 path per channel
template <typename TO>
__device__ __forceinline__ void rgb_px(const float (&a)[3][K], const float (&b)[K], TO (&o)[3]) {
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) o[ch] = cvt_out<TO>(dot_k<K>(a[ch], b));
}

template <typename TO>
__global__ void __launch_bounds__(256)
relight_rgb8_k(const uint8_t* __restrict__ coef8, int64_t P, int vec, const double* __restrict__ qparams,
               const double* __restrict__ luv, int E, TO* __restrict__ out) {
  constexpr int SLAB = slab_v4(0, rgb_staged<TO>() ? 3 : 0);
  __shared__ floatx4 slabs[4 * SLAB];
  __shared__ float tab[K * TAB];
  fill_tables<K>(qparams, tab);
  __syncthreads();  // the one workgroup barrier: waves may leave below
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 256;
  if (wave_px >= P) return;
  floatx4* slab = slabs + wave * SLAB;
  if (vec && wave_px + 256 <= P) {  // wave-uniform
    Rgb8Px r;
    load_bytes4(coef8, P, wave_px + 4 * lane, r);
    float a[4][3][K];
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) dequantise_px(r.c[ch].b[v], tab, a[v][ch]);
    for (int e = 0; e < E; ++e) {
      float b[K];
      ptm_eval<float>((float)luv[2 * e], (float)luv[2 * e + 1], b);  // basis_eval<float>'s PTM-6 branch
      TO o[4][3];
#pragma unroll
      for (int v = 0; v < 4; ++v) rgb_px<TO>(a[v], b, o[v]);
      TO* rows = out + ((int64_t)e * P + wave_px) * 3;
      store_rgb4<TO>(rows, lane, slab, o);
    }
    return;
  }
  for (int j = 0; j < 4; ++j) {
    const int64_t p = wave_px + 64 * j + lane;
    if (p >= P) break;
    uint8_t cb[3][K];
    load_bytes1(coef8, P, p, cb);
    float a[3][K];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) dequantise_px(cb[ch], tab, a[ch]);
    for (int e = 0; e < E; ++e) {
      float b[K];
      ptm_eval<float>((float)luv[2 * e], (float)luv[2 * e + 1], b);
      TO o[3];
      rgb_px<TO>(a, b, o);
      TO* px = out + ((int64_t)e * P + p) * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) px[ch] = o[ch];
    }
  }
}

template <int NL>
__global__ void __launch_bounds__(256)
rgb8_normals_k(const uint8_t* __restrict__ coef8, int64_t P, int vec, const double* __restrict__ qparams, Weights w,
               float* __restrict__ normals, uint8_t* __restrict__ kind, float* __restrict__ peak) {
  constexpr bool STAGE_OUT = NL == RTI_NORMAL_PIXEL_MAJOR;
  constexpr int SLAB = slab_v4(0, STAGE_OUT ? 3 : 0);
  __shared__ floatx4 slabs[4 * SLAB];
  __shared__ float tab[K * TAB];
  fill_tables<K>(qparams, tab);
  __syncthreads();  // the one workgroup barrier: waves may leave below
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 256;
  if (wave_px >= P) return;
  floatx4* slab = slabs + wave * SLAB;
  if (vec && wave_px + 256 <= P) {  // wave-uniform
    const int64_t p0 = wave_px + 4 * lane;
    Rgb8Px r;
    load_bytes4(coef8, P, p0, r);
    ptm_px::NormalOut o[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      float c[3][K];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) dequantise_px(r.c[ch].b[v], tab, c[ch]);
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
    uint8_t cb[3][K];
    load_bytes1(coef8, P, p, cb);
    float c[3][K];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) dequantise_px(cb[ch], tab, c[ch]);
    const ptm_px::NormalOut o = normal_px(c, w, peak != nullptr);
#pragma unroll
    for (int i = 0; i < 3; ++i) normals[NL == RTI_NORMAL_PLANAR ? (int64_t)i * P + p : p * 3 + i] = o.n[i];
    if (kind) kind[p] = o.kind;
    if (peak) peak[p] = o.peak;
  }
}

// rti_relight_rgb8's loads and tables, rti_rgb8_normals' luminance, and every channel enhanced under the
// luminance's peak (enhance_px::rgb_enhanced)
template <typename TO, int MODE>
__global__ void __launch_bounds__(256)
relight_rgb8_enhanced_k(const uint8_t* __restrict__ coef8, int64_t P, int vec, const double* __restrict__ qparams,
                        Weights w, enhance_px::Enhance q, TO* __restrict__ out) {
  constexpr int SLAB = slab_v4(0, rgb_staged<TO>() ? 3 : 0);
  __shared__ floatx4 slabs[4 * SLAB];
  __shared__ float tab[K * TAB];
  fill_tables<K>(qparams, tab);
  __syncthreads();  // the one workgroup barrier: waves may leave below
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 256;
  if (wave_px >= P) return;
  floatx4* slab = slabs + wave * SLAB;
  if (vec && wave_px + 256 <= P) {  // wave-uniform
    Rgb8Px r;
    load_bytes4(coef8, P, wave_px + 4 * lane, r);
    TO o[4][3];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      float c[3][K], l[K];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) dequantise_px(r.c[ch].b[v], tab, c[ch]);
      luminance(c, w.r, w.g, w.b, l);
      enhance_px::rgb_enhanced<MODE, TO>(c, l, q, o[v]);
    }
    TO* rows = out + wave_px * 3;
    store_rgb4<TO>(rows, lane, slab, o);
    return;
  }
  for (int j = 0; j < 4; ++j) {
    const int64_t p = wave_px + 64 * j + lane;
    if (p >= P) break;
    uint8_t cb[3][K];
    load_bytes1(coef8, P, p, cb);
    float c[3][K], l[K];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) dequantise_px(cb[ch], tab, c[ch]);
    luminance(c, w.r, w.g, w.b, l);
    TO o[3];
    enhance_px::rgb_enhanced<MODE, TO>(c, l, q, o);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[p * 3 + ch] = o[ch];
  }
}

}  // namespace
}  // namespace rti

using namespace rti;

extern "C" int64_t rti_rgb8_qparams_workspace(int64_t P) {
  return P < 1 ? 0 : qparams_blocks(P, 1024) * NQ * (int64_t)sizeof(float);
}

extern "C" int rti_rgb8_qparams(const float* coef, int coef_layout, int64_t coef_channel_stride, int64_t P,
                                void* workspace, double* qparams, rti_stream_t stream) {
  const char* const E = "rti_rgb8_qparams";
  if (int st = check_pointers(E, {coef, workspace, qparams})) return st;
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  if (int st = check_rgb_maps(E, K, coef_layout, coef_channel_stride, P)) return st;
  if (!aligned_to(workspace, 4) || !aligned_to(qparams, 8))
    return fail(RTI_ERR_BAD_ARG, "%s: workspace must be 4-byte and qparams 8-byte aligned", E);
  const int64_t cs = coef_channel_stride ? coef_channel_stride : P * K;
  const int blocks = (int)qparams_blocks(P, 1024);
  const int vec = maps_vec(coef, cs, P) ? 1 : 0;
  float* partial = static_cast<float*>(workspace);
  note_launches(2);
  with_layout(coef_layout, [&](auto cl) {
    hipLaunchKernelGGL((rgb_extremes_k<decltype(cl)::value>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, coef, cs,
                       P, vec, partial);
  });
  if (int st = check_launch(E)) return st;
  hipLaunchKernelGGL(rgb_qparams_k, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, blocks, qparams);
  return check_launch(E);
}

extern "C" int rti_rgb8_quantise(const float* coef, int coef_layout, int64_t coef_channel_stride, int64_t P,
                                 const double* qparams, uint8_t* coef8, rti_stream_t stream) {
  const char* const E = "rti_rgb8_quantise";
  if (int st = check_pointers(E, {coef, qparams, coef8})) return st;
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  if (int st = check_rgb_maps(E, K, coef_layout, coef_channel_stride, P)) return st;
  if (int st = check_qparams_aligned(E, qparams)) return st;
  const int64_t cs = coef_channel_stride ? coef_channel_stride : P * K;
  const int vec = maps_vec(coef, cs, P) && aligned_to(coef8, 8) ? 1 : 0;
  note_launches(1);
  with_layout(coef_layout, [&](auto cl) {
    launch(rgb_quantise_k<decltype(cl)::value>, P, (hipStream_t)stream, coef, cs, P, vec, qparams, coef8);
  });
  return check_launch(E);
}

extern "C" int rti_relight_rgb8(const uint8_t* coef8, int64_t P, const double* qparams, const double* luv, int E_,
                                void* out, int out_dtype, rti_stream_t stream) {
  const char* const E = "rti_relight_rgb8";
  if (int st = check_pointers(E, {coef8, qparams, luv, out})) return st;
  if (P < 1 || E_ < 1) return fail(RTI_ERR_BAD_ARG, "%s: P and E must be positive", E);
  if (int st = check_out_dtype(E, out_dtype)) return st;
  if (int st = check_qparams_aligned(E, qparams)) return st;
  const int vec = P % 4 == 0 && aligned_to(coef8, 8) && rgb_out_vec(out, out_dtype) ? 1 : 0;
  note_launches(1);
  with_out(out_dtype, [&](auto t) {
    launch(relight_rgb8_k<decltype(t)>, P, (hipStream_t)stream, coef8, P, vec, qparams, luv, E_, out);
  });
  return check_launch(E);
}

extern "C" int rti_rgb8_normals(const uint8_t* coef8, int64_t P, const double* qparams, const float* w,
                                float* normals, int normal_layout, uint8_t* kind, float* peak, rti_stream_t stream) {
  const char* const E = "rti_rgb8_normals";
  if (int st = check_pointers(E, {coef8, qparams, normals})) return st;
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  if (int st = check_normal_layout(E, normal_layout)) return st;
  Weights wt;
  if (int st = rgb_px::host_weights(E, w, wt)) return st;
  if (int st = check_qparams_aligned(E, qparams)) return st;
  const int vec = P % 4 == 0 && aligned_to(coef8, 8) && normals_out_vec(normals, kind, peak) ? 1 : 0;
  note_launches(1);
  with_normal_layout(normal_layout, [&](auto nl) {
    launch(rgb8_normals_k<decltype(nl)::value>, P, (hipStream_t)stream, coef8, P, vec, qparams, wt, normals, kind, peak);
  });
  return check_launch(E);
}

extern "C" int rti_relight_rgb8_enhanced(const uint8_t* coef8, int64_t P, const double* qparams, const float* w,
                                         int mode, double gain, double kd, double ks, int spec_exp, double lu,
                                         double lv, void* out, int out_dtype, rti_stream_t stream) {
  const char* const E = "rti_relight_rgb8_enhanced";
  if (int st = check_pointers(E, {coef8, qparams, out})) return st;
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  if (int st = enhance_px::check_enhance(E, mode, gain, kd, ks, spec_exp, lu, lv)) return st;
  Weights wt;
  if (int st = rgb_px::host_weights(E, w, wt)) return st;
  if (int st = check_out_dtype(E, out_dtype)) return st;
  if (int st = check_qparams_aligned(E, qparams)) return st;
  const int vec = P % 4 == 0 && aligned_to(coef8, 8) && rgb_out_vec(out, out_dtype) ? 1 : 0;
  const enhance_px::Enhance q = enhance_px::enhance_args(gain, kd, ks, spec_exp, lu, lv);
  note_launches(1);
  enhance_px::with_mode_out(mode, out_dtype, [&](auto m, auto t) {
    launch(relight_rgb8_enhanced_k<decltype(t), decltype(m)::value>, P, (hipStream_t)stream, coef8, P, vec, qparams,
           wt, q, out);
  });
  return check_launch(E);
}
