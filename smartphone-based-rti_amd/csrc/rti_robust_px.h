// rti_robust_px.h -- the per-pixel robust fit shared by rti_fit_robust.hip (k = 6, 9: coefficients), rti_ps.hip and
// rti_ps_near.hip (k = 3: photometric stereo): intensity window, Cholesky solve with the 1e-10·max diag G pivot rule,
// fallback to every light, Huber IRLS (include/rti.h states the semantics).  One lane owns one pixel and the fp64
// state is k(k+1)/2 + k + 1 accumulators, factored in registers like rti_perpixel.hip's ne_solve.  Every file runs
// these templates as they stand, so a fit at a k has one arithmetic.
//
// The design row of light n comes from a row source R: a functor `void operator()(int n, double (&a)[K]) const`
// called once per sample in every pass.  RbSharedRows reads the wave-uniform row A[n] (scalar loads, the values
// stay in SGPR pairs); rti_ps_px.h's near-light source forms a lane-private row from the light and the pixel.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rti_internal.h"

namespace rti {
namespace robust_px {

typedef uint32_t uintx4 __attribute__((ext_vector_type(4)));

constexpr int64_t RB_LDS_BYTES = 160 * 1024;  // LDS of one CU
constexpr double RB_PIVOT_TOL = 1e-10;        // a pivot <= RB_PIVOT_TOL·max diag G fails the solve

inline int rb_elem_size(int in_dtype) { return in_dtype == RTI_U8 ? 1 : 4; }

template <int K>
__host__ __device__ constexpr int rb_tri(int i, int j) {  // packed lower triangle, i >= j
  return i * (i + 1) / 2 + j;
}

template <int K>
struct RbSys {
  double g[K * (K + 1) / 2], b[K], q;
  int m;
};

// The samples of one pixel: lane-private address, `step` elements between lights (LDS tile or global plane).
template <typename T>
struct RbSamples {
  const T* p;
  int64_t step;
  __device__ __forceinline__ double operator()(int n) const { return (double)p[(int64_t)n * step]; }
};

// The shared design: row n of A [N][K], the same for every lane.
template <int K>
struct RbSharedRows {
  const double* __restrict__ A;
  __device__ __forceinline__ void operator()(int n, double (&a)[K]) const {
    const double* An = A + (int64_t)n * K;  // wave-uniform row -> SGPR pairs
#pragma unroll
    for (int i = 0; i < K; ++i) a[i] = An[i];
  }
};

enum { RB_W_WINDOW = 0, RB_W_ALL = 1, RB_W_HUBER = 2 };

// sample weight: the window (or 1 for every light on a fallback pixel) times Huber's weight of the residual
template <int K, int MODE>
__device__ __forceinline__ double rb_weight(const double (&An)[K], double y, double lo, double hi, bool all,
                                            const double (&c)[K], double delta) {
  const double win = (all || (y >= lo && y <= hi)) ? 1.0 : 0.0;
  if constexpr (MODE == RB_W_ALL) return 1.0;
  if constexpr (MODE == RB_W_WINDOW) return win;
  double r = y;
#pragma unroll
  for (int i = 0; i < K; ++i) r = fma(-An[i], c[i], r);
  const double ar = fabs(r);
  return win * (ar <= delta ? 1.0 : delta / ar);
}

// one pass over the pixel's N samples: G, b, q and the count of samples in the window
template <int K, int MODE, bool NEED_Q, typename R, typename S>
__device__ __forceinline__ void rb_accumulate(const R& row_of, int N, const S& y_of, double lo, double hi, bool all,
                                              const double (&c)[K], double delta, RbSys<K>& s) {
#pragma unroll
  for (int i = 0; i < K * (K + 1) / 2; ++i) s.g[i] = 0.0;
#pragma unroll
  for (int i = 0; i < K; ++i) s.b[i] = 0.0;
  s.q = 0.0;
  int m = 0;
#pragma unroll 2
  for (int n = 0; n < N; ++n) {
    double An[K];
    row_of(n, An);
    const double y = y_of(n);
    const double w = rb_weight<K, MODE>(An, y, lo, hi, all, c, delta);
    if constexpr (MODE == RB_W_WINDOW) m += w != 0.0 ? 1 : 0;
    const double wy = w * y;
    if constexpr (NEED_Q) s.q = fma(wy, y, s.q);
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const double wa = w * An[i];
#pragma unroll
      for (int j = 0; j <= i; ++j) s.g[rb_tri<K>(i, j)] = fma(wa, An[j], s.g[rb_tri<K>(i, j)]);
      s.b[i] = fma(An[i], wy, s.b[i]);
    }
  }
  s.m = MODE == RB_W_WINDOW ? m : N;
}

// Cholesky solve of G c = b in registers (the idiom of rti_perpixel.hip's ne_solve).  Returns false, leaving c
// untouched, when a pivot is not above RB_PIVOT_TOL·max diag G (NaN included).
template <int K>
__device__ __forceinline__ bool rb_solve(const RbSys<K>& s, double (&c)[K]) {
  double L[K * (K + 1) / 2];
  double dmax = 0.0;
#pragma unroll
  for (int i = 0; i < K; ++i) dmax = fmax(dmax, s.g[rb_tri<K>(i, i)]);
  const double thr = RB_PIVOT_TOL * dmax;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    double d = s.g[rb_tri<K>(j, j)];
#pragma unroll
    for (int p = 0; p < j; ++p) d = fma(-L[rb_tri<K>(j, p)], L[rb_tri<K>(j, p)], d);
    ok = ok && (d > thr);
    const double ljj = sqrt(d > 0.0 ? d : 1.0);
    const double inv = 1.0 / ljj;
    L[rb_tri<K>(j, j)] = inv;  // the diagonal is kept inverted
#pragma unroll
    for (int i = j + 1; i < K; ++i) {
      double t = s.g[rb_tri<K>(i, j)];
#pragma unroll
      for (int p = 0; p < j; ++p) t = fma(-L[rb_tri<K>(i, p)], L[rb_tri<K>(j, p)], t);
      L[rb_tri<K>(i, j)] = t * inv;
    }
  }
  double z[K], x[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    double t = s.b[i];
#pragma unroll
    for (int p = 0; p < i; ++p) t = fma(-L[rb_tri<K>(i, p)], z[p], t);
    z[i] = t * L[rb_tri<K>(i, i)];
  }
#pragma unroll
  for (int i = K - 1; i >= 0; --i) {
    double t = z[i];
#pragma unroll
    for (int p = i + 1; p < K; ++p) t = fma(-L[rb_tri<K>(p, i)], x[p], t);
    x[i] = t * L[rb_tri<K>(i, i)];
  }
  if (ok) {
#pragma unroll
    for (int i = 0; i < K; ++i) c[i] = x[i];
  }
  return ok;
}

struct RbOut {
  double ss;  // Σ win r²
  int m;
  bool fell;
};

// The whole fit of one pixel from its samples (either form).  ITER: iters > 0.
template <int K, bool ITER, typename R, typename S>
__device__ __forceinline__ RbOut rb_pixel(const R& row_of, int N, const S& y_of, double lo, double hi, int min_lights,
                                          int iters, double delta, double (&c)[K]) {
  RbSys<K> s;
#pragma unroll
  for (int i = 0; i < K; ++i) c[i] = __builtin_nan("");
  rb_accumulate<K, RB_W_WINDOW, !ITER>(row_of, N, y_of, lo, hi, false, c, delta, s);
  RbOut o;
  o.m = s.m;
  bool ok = s.m >= min_lights && rb_solve<K>(s, c);
  o.fell = !ok;
  if (!ok) {  // every light; a second failure leaves the NaN
    rb_accumulate<K, RB_W_ALL, !ITER>(row_of, N, y_of, lo, hi, true, c, delta, s);
    o.m = N;
    ok = rb_solve<K>(s, c);
  }
  if constexpr (!ITER) {
    // Σ w r² = q − 2 cᵀb + cᵀG c with this pass's own G, b, q (w ∈ {0, 1})
    double e = s.q;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      double gc = 0.0;
#pragma unroll
      for (int j = 0; j < K; ++j) gc = fma(s.g[i >= j ? rb_tri<K>(i, j) : rb_tri<K>(j, i)], c[j], gc);
      e = fma(c[i], gc - 2.0 * s.b[i], e);
    }
    o.ss = e < 0.0 ? 0.0 : e;  // rounding can leave an exact fit below zero; NaN passes
  } else {
    for (int t = 0; t < iters && ok; ++t) {
      rb_accumulate<K, RB_W_HUBER, false>(row_of, N, y_of, lo, hi, o.fell, c, delta, s);
      ok = rb_solve<K>(s, c);  // a failed solve keeps the previous coefficients and stops
    }
    double e = 0.0;
#pragma unroll 2
    for (int n = 0; n < N; ++n) {
      double An[K];
      row_of(n, An);
      const double y = y_of(n);
      double r = y;
#pragma unroll
      for (int i = 0; i < K; ++i) r = fma(-An[i], c[i], r);
      const bool in = o.fell || (y >= lo && y <= hi);
      e = fma(in ? r : 0.0, r, e);
    }
    o.ss = e;
  }
  return o;
}

// The largest tile of 256 / 128 / 64 pixels whose `planes` planes of the input dtype fit the CU's LDS, 0 if none.
inline int rb_tile_pixels(int64_t planes, int in_dtype) {
  for (int tp : {256, 128, 64})
    if (planes * tp * rb_elem_size(in_dtype) <= RB_LDS_BYTES) return tp;
  return 0;
}

// Copies a workgroup's tile [N][TP] of one channel's planes (src: pixel 0 of its first plane, lstride elements
// between planes) to `lds`; the caller synchronises.  vec: 16-byte loads (the host passes it only when every
// plane of every tile is 16-byte aligned), taken by full tiles.  A lane past P copies pixel P − 1.
template <typename T, int TP>
__device__ __forceinline__ void rb_stage_tile(unsigned char* lds, const T* __restrict__ src, int N, int64_t lstride,
                                              int64_t tile0, int64_t P, int vec) {
  const int t = threadIdx.x;
  if (vec && tile0 + TP <= P) {  // workgroup-uniform
    constexpr int VR = TP * (int)sizeof(T) / 16;  // 16-byte vectors per plane row
    constexpr int EV = 16 / (int)sizeof(T);       // elements per vector
    uintx4* tv = reinterpret_cast<uintx4*>(lds);
    const int total = N * VR;
#pragma unroll 4
    for (int idx = t; idx < total; idx += TP) {
      const int n = idx / VR, v = idx - n * VR;
      tv[idx] = __builtin_nontemporal_load(reinterpret_cast<const uintx4*>(src + (int64_t)n * lstride + tile0 + v * EV));
    }
  } else {
    T* tile = reinterpret_cast<T*>(lds);
    const int64_t p = tile0 + t;
    const int64_t pr = p < P ? p : P - 1;
#pragma unroll 4
    for (int n = 0; n < N; ++n) tile[n * TP + t] = __builtin_nontemporal_load(src + (int64_t)n * lstride + pr);
  }
}

}  // namespace robust_px
}  // namespace rti
