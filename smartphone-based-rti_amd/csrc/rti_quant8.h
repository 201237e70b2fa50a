// rti_quant8.h -- what the 8-bit quantisers share (rti_lrgb8.hip, rti_hsh8.hip, rti_rgb8.hip): the extremes pass
// behind every *_qparams entry, the byte rounding, and the header arithmetic of a .ptm file (DESIGN.md §4.8, §4.9,
// §4.11).  Everything is __forceinline__ device code or a small host helper.  The kernels keep their own lane maps,
// loads, dequantisation and launchers: nothing here knows which format calls it.
//
// The extremes pass.  A partial is NQ floats: entries [0, NMIN) are minima, entries [NMIN, NQ) maxima, of finite
// values only (an entry without one keeps +inf or -inf).  Min and max are order-independent, so the reduction tree
// does not show in the result: a lane folds its pixels into a partial, a wave folds its lanes with shuffles, a
// workgroup its waves through LDS (ext_block_fold), and every workgroup of a grid of at most QP_MAX_BLOCKS, each
// striding over chunks of pixels, writes its partial to the workspace; a one-workgroup tail folds those
// (fold_partials) and forms the qparams.  No atomics, and no workspace word is read that this call did not write.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

namespace rti {
namespace quant8 {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int QP_MAX_BLOCKS = 768;  // the extremes' grid: 3 workgroups per CU of 256, each striding over chunks

// workgroups of the extremes' grid for P pixels, `chunk` pixels per workgroup and stride
inline int64_t qparams_blocks(int64_t P, int chunk) {
  const int64_t chunks = (P + chunk - 1) / chunk;
  return chunks < QP_MAX_BLOCKS ? chunks : QP_MAX_BLOCKS;
}

// ---- extremes ----------------------------------------------------------------------------------------------------

template <int NMIN, int NQ>
__device__ __forceinline__ void ext_init(float (&q)[NQ]) {
#pragma unroll
  for (int i = 0; i < NQ; ++i) q[i] = i < NMIN ? INFINITY : -INFINITY;
}

template <int NMIN>
__device__ __forceinline__ float ext_fold(int i, float a, float b) { return i < NMIN ? fminf(a, b) : fmaxf(a, b); }

__device__ __forceinline__ bool is_finite(float x) { return fabsf(x) <= FLT_MAX; }  // false for NaN

// a value into the min and max of its plane, if it is finite
__device__ __forceinline__ void ext_update(float& lo, float& hi, float x) {
  if (is_finite(x)) {
    lo = fminf(lo, x);
    hi = fmaxf(hi, x);
  }
}

// the workgroup's 256 lanes -> thread i < NQ returns value i
template <int NMIN, int NQ>
__device__ __forceinline__ float ext_block_fold(float (&q)[NQ], float (*part)[NQ]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) q[i] = ext_fold<NMIN>(i, q[i], __shfl_xor(q[i], m, 64));
    if (lane == 0) part[wave][i] = q[i];
  }
  __syncthreads();
  const int i = threadIdx.x < NQ ? threadIdx.x : 0;
  return ext_fold<NMIN>(i, ext_fold<NMIN>(i, part[0][i], part[1][i]), ext_fold<NMIN>(i, part[2][i], part[3][i]));
}

// the tail's first half: n partials -> fin[0 .. NQ), which every thread of the one workgroup may read on return
template <int NMIN, int NQ>
__device__ __forceinline__ void fold_partials(const float* __restrict__ partial, int n, float (*part)[NQ],
                                              float (&fin)[NQ]) {
  float q[NQ];
  ext_init<NMIN>(q);
  for (int b = threadIdx.x; b < n; b += 256)
#pragma unroll
    for (int i = 0; i < NQ; ++i) q[i] = ext_fold<NMIN>(i, q[i], partial[(int64_t)b * NQ + i]);
  const float r = ext_block_fold<NMIN>(q, part);
  if (threadIdx.x < NQ) fin[threadIdx.x] = r;
  __syncthreads();
}

// ---- bytes ---------------------------------------------------------------------------------------------------------

// rint(t) clipped to a byte; NaN -> 0
__device__ __forceinline__ uint32_t byte_of(double t) {
  const double r = rint(t);
  return (uint32_t)(int)(r > 0.0 ? (r < 255.0 ? r : 255.0) : 0.0);
}

// NB bytes (a multiple of 4) of a lane as dwords
template <int NB>
__device__ __forceinline__ void store_dwords(uint8_t* __restrict__ dst, const uint8_t* f) {
  uint32_t* o4 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
  for (int w = 0; w < NB / 4; ++w)
    o4[w] = (uint32_t)f[4 * w] | ((uint32_t)f[4 * w + 1] << 8) | ((uint32_t)f[4 * w + 2] << 16) |
            ((uint32_t)f[4 * w + 3] << 24);
}

// ---- the .ptm header (rti/io.py: _ptm_quantise; fp64, no contraction) ---------------------------------------------

// extremes lo, hi of a plane (lo > hi: it has no finite value), stored as coefficient·s -> its scale and bias
__device__ __forceinline__ void ptm_scale_bias(float lo, float hi, double s, double& scale, double& bias) {
#pragma clang fp contract(off)
  const bool has = lo <= hi;
  const double LO = (double)lo * s, HI = (double)hi * s;
  const double sc = has && HI > LO ? (HI - LO) / 255.0 : 1.0;
  double bi = 0.0;
  if (has) {
    const double b = rint(-LO / sc);
    bi = b > 0.0 ? (b < 255.0 ? b : 255.0) : 0.0;  // -0.0 -> 0.0
  }
  scale = sc;
  bias = bi;
}

// the K scales and K biases at the head of a PTM's qparams
template <int K>
struct QParams {
  double scale[K], bias[K];
};

template <int K>
__device__ __forceinline__ QParams<K> load_qparams(const double* __restrict__ qparams) {
  QParams<K> q;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    q.scale[j] = qparams[j];
    q.bias[j] = qparams[K + j];
  }
  return q;
}

// the byte of coefficient a, stored as x (a itself, or a·s); a NaN coefficient takes the bias, which reads back as 0
__device__ __forceinline__ uint8_t coef_byte(double a, double x, double scale, double bias) {
#pragma clang fp contract(off)
  return a != a ? (uint8_t)(int)bias : (uint8_t)byte_of(x / scale + bias);
}

}  // namespace quant8
}  // namespace rti
