// rti_unsharp.hip -- the project's spatial operator (gfx950): unsharp masking of k-channel maps by a fused
// separable Gaussian, and shading from a given normal map.
//
//     rti_gauss_radius / rti_gauss_taps   host: the taps the kernel convolves with
//     rti_map_unsharp                     map -> map + amount·(map − blur), optionally renormalised (normal maps)
//     rti_shade_normals                   normal map (+ albedo) -> one image at (lu, lv)
//
// The reference has no spatial operator; the semantics are build-defined and stated in include/rti.h and
// DESIGN.md §4.6.  The blur is a NORMALISED convolution: a pixel with a non-finite channel (the NaN pixels of
// rti_fit_shared_robust and of rti_ptm_normals' kind 4) and every tap outside the image are left out of the
// numerator and of the denominator, so NaN does not spread and no border is replicated.
//
// map_unsharp_k does both passes in one launch.  A workgroup of 256 threads owns a 32×64 output tile:
//   mask    the tile plus R rows / R4 = ⌈R/4⌉·4 columns of halo: every channel of every staged pixel is read once
//           (16- or 8-byte loads on the vector path) and the pixel's validity kept as a byte in LDS
//   then per "plane" -- first the mask itself as 1.0 / 0.0 (its blur is the denominator), then each channel:
//     stage   the plane's fp32 values into LDS, invalid and outside pixels as 0 (fma(w, 0, acc) = acc: leaving
//             a term out and adding its zero are the same bits)
//     H pass  LDS -> LDS in fp64: a thread owns 8 consecutive outputs of one staged row
//     V pass  LDS -> registers: a thread owns 8 consecutive rows of one output column; then blur = num/den,
//             the unsharp step and the store (an invalid pixel copies its source bits)
// The map is read from HBM about once (the per-channel staging re-reads a tile's pixels from L2) and written
// once; no intermediate goes to global memory.  Both passes run conv8: the 8 outputs of a thread share each
// source value (one LDS read per 8 fp64 FMAs) and take their taps from a register window that slides 8 taps
// per unrolled group, every output summing its 2R + 1 terms in ascending order whatever the tile.  LDS at
// R = 32: 96×65 doubles + 96×129 floats + 96×129 bytes = 109 KiB of the CU's 160 (reserve_lds above 64 KiB).
// Lanes of the H pass walk down a column of the odd-pitched value tile and lanes of the V pass along a row of
// the fp64 intermediate: both conflict-free.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "rti_convert.h"
#include "rti_dispatch.h"
#include "rti_lane4.h"
#include "rti_shade.h"

namespace rti {
namespace {

constexpr int TH = 32, TW = 64;  // output tile
constexpr int NB = 8;            // outputs per thread and pass
constexpr int THREADS = 256;
constexpr int PH = TW + 1;       // pitch of the fp64 intermediate (odd: lanes one row apart never share a bank)
constexpr int MAXR = RTI_UNSHARP_MAX_RADIUS;

struct Taps {
  double w[MAXR + 1];
};

// the staged region and its LDS footprint for radius R
struct Tile {
  int R, R4;   // halo rows, halo columns (R rounded up to 4: staged chunks of 4 pixels stay 16-byte aligned)
  int NR, NC;  // staged rows, staged columns
  int PV;      // pitch of the value and mask tiles (odd)
};
__host__ __device__ inline Tile tile_of(int R) {
  Tile t;
  t.R = R;
  t.R4 = (R + 3) & ~3;
  t.NR = TH + 2 * R;
  t.NC = TW + 2 * t.R4;
  t.PV = t.NC | 1;
  return t;
}
__host__ __device__ inline size_t hnum_bytes(const Tile& t) { return (size_t)t.NR * PH * sizeof(double); }
__host__ __device__ inline size_t vals_bytes(const Tile& t) { return (size_t)t.NR * t.PV * sizeof(float); }
inline size_t lds_bytes(const Tile& t) { return hnum_bytes(t) + vals_bytes(t) + (size_t)t.NR * t.PV; }

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= FLT_MAX; }  // false for NaN

// i / n for 0 <= i < 2^16, 1 <= n <= 2^10, inv = 1.0f / n: the float quotient is off by at most one
__device__ __forceinline__ int div_small(int i, int n, float inv) {
  int q = (int)((float)i * inv);
  const int r = i - q * n;
  q += r >= n ? 1 : (r < 0 ? -1 : 0);
  return q;
}

// acc[j] = Σ_{t = 0..2R ascending} fma(w|t − R|, read(j + t), acc[j]) for j = 0..7: the 8 outputs share the
// sources s = j + t in [0, 8 + 2R).  win holds the taps of t = 8g − 7 .. 8g + 7, so output j takes source
// 8g + i with win[7 + i − j], a compile-time index.  Groups in which some (i, j) has no term test each pair.
template <typename Read>
__device__ __forceinline__ void conv8(const Taps& tp, int R, Read read, double (&acc)[NB]) {
  const int n = NB + 2 * R;
  double win[2 * NB - 1];
#pragma unroll
  for (int i = 0; i < 2 * NB - 1; ++i) win[i] = 0.0;
  for (int g0 = 0; g0 < n; g0 += NB) {
#pragma unroll
    for (int i = 0; i < NB - 1; ++i) win[i] = win[i + NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int d = g0 + i - R;
      const int a = d < 0 ? -d : d;
      const double w = tp.w[a < MAXR ? a : MAXR];
      win[NB - 1 + i] = a <= R ? w : 0.0;
    }
    if (g0 > 0 && g0 + NB - 1 <= 2 * R) {  // 1 <= t <= 2R for every pair
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const double v = read(g0 + i);
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[j] = __builtin_fma(win[NB - 1 + i - j], v, acc[j]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int s = g0 + i;
        if (s < n) {
          const double v = read(s);
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            const int t = s - j;
            if (t >= 0 && t <= 2 * R) acc[j] = __builtin_fma(win[NB - 1 + i - j], v, acc[j]);
          }
        }
      }
    }
  }
}

template <int LAYOUT>
__device__ __forceinline__ int64_t elem(int c, int y, int x, int C, int H, int W) {
  return LAYOUT == RTI_COEF_PLANAR ? ((int64_t)c * H + y) * W + x : ((int64_t)y * W + x) * C + c;
}

struct UnsharpLds {
  double* hnum;
  float* vals;
  uint8_t* msk;
};

// the validity of every staged pixel: inside the image and all channels finite.  vec: planar 4 = float4 along
// x; pixel-major 4 / 2 = float4 / float2 along a pixel's channels; 1 = one float at a time.
template <int LAYOUT>
__device__ __forceinline__ void stage_mask(const float* __restrict__ src, int C, int H, int W, int vec, const Tile& t,
                                           int y0, int x0, uint8_t* __restrict__ msk) {
  if (LAYOUT == RTI_COEF_PLANAR && vec == 4) {
    const int nq = t.NC / 4;
    const float inv = 1.0f / (float)nq;
#pragma unroll 2
    for (int i = threadIdx.x; i < t.NR * nq; i += THREADS) {
      const int r = div_small(i, nq, inv), q = i - r * nq;
      const int y = y0 - t.R + r, x = x0 - t.R4 + 4 * q;
      // W % 4 == 0 and x % 4 == 0: the chunk is inside or outside.  An outside chunk loads the map's first chunk
      // instead (no branch around the loads, so the compiler keeps several in flight) and is then marked invalid.
      const bool in = y >= 0 && y < H && x >= 0 && x < W;
      bool ok[4] = {in, in, in, in};
      for (int c = 0; c < C; ++c) {
        const floatx4 v = *reinterpret_cast<const floatx4*>(src + elem<LAYOUT>(c, in ? y : 0, in ? x : 0, C, H, W));
#pragma unroll
        for (int e = 0; e < 4; ++e) ok[e] = ok[e] && finite_f(v[e]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) msk[r * t.PV + 4 * q + e] = ok[e] ? 1 : 0;
    }
    return;
  }
  const float inv = 1.0f / (float)t.NC;
#pragma unroll 2
  for (int i = threadIdx.x; i < t.NR * t.NC; i += THREADS) {
    const int r = div_small(i, t.NC, inv), j = i - r * t.NC;
    int y = y0 - t.R + r, x = x0 - t.R4 + j;
    bool ok = y >= 0 && y < H && x >= 0 && x < W;
    // an outside pixel reads the map's first pixel (no branch around the loads, so the compiler keeps several in
    // flight) and stays invalid
    if (!ok) y = x = 0;
    if (LAYOUT == RTI_COEF_PIXEL_MAJOR && vec == 4) {
      const floatx4* p = reinterpret_cast<const floatx4*>(src + elem<LAYOUT>(0, y, x, C, H, W));
      for (int c = 0; c < C / 4; ++c) {
        const floatx4 v = p[c];
        ok = ok && finite_f(v[0]) && finite_f(v[1]) && finite_f(v[2]) && finite_f(v[3]);
      }
    } else if (LAYOUT == RTI_COEF_PIXEL_MAJOR && vec == 2) {
      const floatx2* p = reinterpret_cast<const floatx2*>(src + elem<LAYOUT>(0, y, x, C, H, W));
      for (int c = 0; c < C / 2; ++c) {
        const floatx2 v = p[c];
        ok = ok && finite_f(v[0]) && finite_f(v[1]);
      }
    } else {
      for (int c = 0; c < C; ++c) ok = ok && finite_f(src[elem<LAYOUT>(c, y, x, C, H, W)]);
    }
    msk[r * t.PV + j] = ok ? 1 : 0;
  }
}

// one plane into the value tile: c < 0 the mask as 1.0 / 0.0, else channel c with invalid pixels as 0
template <int LAYOUT>
__device__ __forceinline__ void stage_plane(const float* __restrict__ src, int c, int C, int H, int W, int vec,
                                            const Tile& t, int y0, int x0, const UnsharpLds& s) {
  if (LAYOUT == RTI_COEF_PLANAR && vec == 4 && c >= 0) {
    const int nq = t.NC / 4;
    const float inv = 1.0f / (float)nq;
#pragma unroll 4
    for (int i = threadIdx.x; i < t.NR * nq; i += THREADS) {
      const int r = div_small(i, nq, inv), q = i - r * nq;
      const int o = r * t.PV + 4 * q;
      const bool m0 = s.msk[o], m1 = s.msk[o + 1], m2 = s.msk[o + 2], m3 = s.msk[o + 3];
      // a set byte means the whole chunk lies inside the image; any other chunk loads the map's first chunk instead
      // (no branch around the load, so the compiler keeps the unrolled loads in flight together) and stages zeros
      const bool in = m0 || m1 || m2 || m3;
      const floatx4 v = *reinterpret_cast<const floatx4*>(
          src + elem<LAYOUT>(c, in ? y0 - t.R + r : 0, in ? x0 - t.R4 + 4 * q : 0, C, H, W));
      s.vals[o] = m0 ? v[0] : 0.f;
      s.vals[o + 1] = m1 ? v[1] : 0.f;
      s.vals[o + 2] = m2 ? v[2] : 0.f;
      s.vals[o + 3] = m3 ? v[3] : 0.f;
    }
    return;
  }
  const float inv = 1.0f / (float)t.NC;
  if (c < 0) {
    for (int i = threadIdx.x; i < t.NR * t.NC; i += THREADS) {
      const int r = div_small(i, t.NC, inv), o = r * t.PV + i - r * t.NC;
      s.vals[o] = s.msk[o] ? 1.f : 0.f;
    }
    return;
  }
#pragma unroll 4
  for (int i = threadIdx.x; i < t.NR * t.NC; i += THREADS) {
    const int r = div_small(i, t.NC, inv), j = i - r * t.NC;
    const int o = r * t.PV + j;
    const bool m = s.msk[o];  // an invalid or outside pixel loads the map's first element instead and stages 0
    const float v = src[elem<LAYOUT>(c, m ? y0 - t.R + r : 0, m ? x0 - t.R4 + j : 0, C, H, W)];
    s.vals[o] = m ? v : 0.f;
  }
}

// stage -> H pass -> V pass of one plane; acc: this thread's 8 vertical sums (column x, rows yb·8 ..)
template <int LAYOUT>
__device__ __forceinline__ void blur_plane(const float* __restrict__ src, int c, int C, int H, int W, int vec,
                                           const Tile& t, int y0, int x0, const Taps& tp, const UnsharpLds& s,
                                           double (&acc)[NB]) {
  __syncthreads();  // the previous plane's reads of the value tile and of the intermediate are done
  stage_plane<LAYOUT>(src, c, C, H, W, vec, t, y0, x0, s);
  __syncthreads();
  // H pass: task = (staged row r, block xb of 8 output columns); consecutive lanes take consecutive rows
  const float inv = 1.0f / (float)t.NR;
  for (int i = threadIdx.x; i < t.NR * (TW / NB); i += THREADS) {
    const int xb = div_small(i, t.NR, inv), r = i - xb * t.NR;
    const float* row = s.vals + r * t.PV + xb * NB + (t.R4 - t.R);
    double h[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) h[j] = 0.0;
    conv8(tp, t.R, [&](int k) { return (double)row[k]; }, h);
#pragma unroll
    for (int j = 0; j < NB; ++j) s.hnum[r * PH + xb * NB + j] = h[j];
  }
  __syncthreads();
  // V pass: thread = (column x, block yb of 8 output rows); a wave reads 64 consecutive doubles
  const int x = threadIdx.x & (TW - 1), yb = threadIdx.x / TW;
  const double* col = s.hnum + yb * NB * PH + x;
#pragma unroll
  for (int j = 0; j < NB; ++j) acc[j] = 0.0;
  conv8(tp, t.R, [&](int k) { return col[k * PH]; }, acc);
}

__device__ __forceinline__ double unsharp_value(double v, double num, double den, double amount) {
#pragma clang fp contract(off)
  const double blur = num / den;
  return v + amount * (v - blur);
}

template <int LAYOUT, bool RENORM>
__global__ void __launch_bounds__(THREADS)
map_unsharp_k(const float* __restrict__ src, float* __restrict__ dst, int C, int H, int W, int R, Taps tp, double amount,
              int vec, int tiles_x) {
  extern __shared__ __attribute__((aligned(16))) unsigned char us_lds[];
  const Tile t = tile_of(R);
  UnsharpLds s;
  s.hnum = reinterpret_cast<double*>(us_lds);
  s.vals = reinterpret_cast<float*>(us_lds + hnum_bytes(t));
  s.msk = us_lds + hnum_bytes(t) + vals_bytes(t);
  const int ty = blockIdx.x / tiles_x;  // a 1-D grid: a tall map has more tile rows than a grid's y extent
  const int x0 = (blockIdx.x - ty * tiles_x) * TW, y0 = ty * TH;
  stage_mask<LAYOUT>(src, C, H, W, vec, t, y0, x0, s.msk);

  double den[NB];
  blur_plane<LAYOUT>(src, -1, C, H, W, vec, t, y0, x0, tp, s, den);

  // this thread's 8 output pixels: column x, rows y0 + yb·8 + j; their place in the staged tiles
  const int xl = threadIdx.x & (TW - 1), yb = threadIdx.x / TW;
  const int x = x0 + xl;
  const int centre = (yb * NB + t.R) * t.PV + xl + t.R4;
  if constexpr (RENORM) {
    double o[3][NB];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double num[NB];
      blur_plane<LAYOUT>(src, c, C, H, W, vec, t, y0, x0, tp, s, num);
#pragma unroll
      for (int j = 0; j < NB; ++j) o[c][j] = unsharp_value((double)s.vals[centre + j * t.PV], num[j], den[j], amount);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
#pragma clang fp contract(off)
      const int y = y0 + yb * NB + j;
      if (y >= H || x >= W) continue;
      if (s.msk[centre + j * t.PV]) {
        const double nrm = sqrt(o[0][j] * o[0][j] + o[1][j] * o[1][j] + o[2][j] * o[2][j]);
        const bool unit = !(nrm > 0.0 && nrm <= DBL_MAX);  // ‖o‖ = 0 or not finite -> (0, 0, 1)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          dst[elem<LAYOUT>(c, y, x, 3, H, W)] = unit ? (c == 2 ? 1.f : 0.f) : (float)(o[c][j] / nrm);
      } else {
        for (int c = 0; c < 3; ++c) {
          const int64_t e = elem<LAYOUT>(c, y, x, 3, H, W);
          reinterpret_cast<uint32_t*>(dst)[e] = reinterpret_cast<const uint32_t*>(src)[e];
        }
      }
    }
  } else {
    for (int c = 0; c < C; ++c) {
      double num[NB];
      blur_plane<LAYOUT>(src, c, C, H, W, vec, t, y0, x0, tp, s, num);
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int y = y0 + yb * NB + j;
        if (y >= H || x >= W) continue;
        const int64_t e = elem<LAYOUT>(c, y, x, C, H, W);
        if (s.msk[centre + j * t.PV])
          dst[e] = (float)unsharp_value((double)s.vals[centre + j * t.PV], num[j], den[j], amount);
        else
          reinterpret_cast<uint32_t*>(dst)[e] = reinterpret_cast<const uint32_t*>(src)[e];
      }
    }
  }
}

template <int LAYOUT, bool RENORM>
int launch_unsharp(const float* src, float* dst, int C, int H, int W, int R, const Taps& tp, double amount, int vec,
                   hipStream_t s) {
  auto kern = map_unsharp_k<LAYOUT, RENORM>;
  const size_t lds = lds_bytes(tile_of(R));
  if (lds > 64 * 1024 && reserve_lds(reinterpret_cast<const void*>(kern), lds) != hipSuccess)
    return fail(RTI_ERR_HIP, "rti_map_unsharp: cannot reserve %zu bytes of LDS", lds);
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;  // tiles_x·tiles_y < 2^31 as H·W is
  hipLaunchKernelGGL(kern, dim3((unsigned)(tiles_x * tiles_y)), dim3(THREADS), lds, s, src, dst, C, H, W, R, tp, amount,
                     vec, tiles_x);
  return check_launch("rti_map_unsharp");
}

// ---- shading from a normal map ----------------------------------------------------------------------------------

struct Shade {
  double kd, ks;
  int e;
  double lx, ly, lz;  // the light
  double hx, hy, hz;  // the half vector between the light and the viewer (0, 0, 1), unit length
};

__device__ __forceinline__ double shade_value(double nx, double ny, double nz, double alb, const Shade& q) {
#pragma clang fp contract(off)
  const double d = nx * q.lx + ny * q.ly + nz * q.lz;
  const double h = nx * q.hx + ny * q.hy + nz * q.hz;
  const double v = q.kd * alb * (d > 0.0 ? d : 0.0) + q.ks * powi(h > 0.0 ? h : 0.0, q.e);
  return (nx != nx || ny != ny || nz != nz || alb != alb) ? (double)NAN : v;
}

// rti_relight_enhanced's lane map: a wave owns pixels [wave_px, wave_px + 256).  vec != 0 and the whole chunk
// inside the map: lane l owns pixels wave_px + 4l .. + 3 (16-byte loads and stores); otherwise lane l takes
// pixels wave_px + 64j + l, j = 0..3, one at a time.
template <int NL, typename TO>
__global__ void __launch_bounds__(256)
shade_normals_k(const float* __restrict__ normals, const float* __restrict__ albedo, int64_t P, int vec, Shade q,
                TO* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 256;
  if (wave_px >= P) return;
  if (vec && wave_px + 256 <= P) {  // wave-uniform
    const int64_t p0 = wave_px + 4 * lane;
    float n[3][4];
    if constexpr (NL == RTI_NORMAL_PLANAR) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const floatx4 v = *reinterpret_cast<const floatx4*>(normals + (int64_t)i * P + p0);
#pragma unroll
        for (int e = 0; e < 4; ++e) n[i][e] = v[e];
      }
    } else {
      union {
        floatx4 v[3];
        float f[4][3];
      } u;
#pragma unroll
      for (int i = 0; i < 3; ++i) u.v[i] = reinterpret_cast<const floatx4*>(normals + p0 * 3)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < 3; ++i) n[i][e] = u.f[e][i];
    }
    floatx4 a = {1.f, 1.f, 1.f, 1.f};
    if (albedo) a = *reinterpret_cast<const floatx4*>(albedo + p0);
    typedef TO vec_t __attribute__((ext_vector_type(4)));
    vec_t o;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      o[e] = cvt_out<TO>(shade_value((double)n[0][e], (double)n[1][e], (double)n[2][e], (double)a[e], q));
    *reinterpret_cast<vec_t*>(out + p0) = o;
    return;
  }
  for (int j = 0; j < 4; ++j) {
    const int64_t p = wave_px + 64 * j + lane;
    if (p >= P) break;
    double n[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = (double)normals[NL == RTI_NORMAL_PLANAR ? (int64_t)i * P + p : p * 3 + i];
    out[p] = cvt_out<TO>(shade_value(n[0], n[1], n[2], albedo ? (double)albedo[p] : 1.0, q));
  }
}

bool sigma_ok(double sigma) { return std::isfinite(sigma) && sigma > 0.0; }

}  // namespace
}  // namespace rti

using namespace rti;

extern "C" int rti_gauss_radius(double sigma) {
  if (!sigma_ok(sigma)) return -1;
  const double r = std::ceil(3.0 * sigma);
  return r < 1.0 ? 1 : (r > 1073741824.0 ? 1073741824 : (int)r);
}

extern "C" int rti_gauss_taps(double sigma, int radius, double* taps) {
  const char* const E = "rti_gauss_taps";
  if (!taps) return fail(RTI_ERR_BAD_ARG, "%s: null pointer", E);
  if (!sigma_ok(sigma)) return fail(RTI_ERR_BAD_ARG, "%s: sigma %g must be finite and positive", E, sigma);
  if (radius < 1 || radius > MAXR) return fail(RTI_ERR_BAD_ARG, "%s: radius %d outside [1, %d]", E, radius, MAXR);
  for (int d = 0; d <= radius; ++d) taps[d] = std::exp(-(double)(d * d) / (2.0 * sigma * sigma));
  double z = taps[0];
  double tail = 0.0;
  for (int d = 1; d <= radius; ++d) tail += taps[d];
  z += 2.0 * tail;
  for (int d = 0; d <= radius; ++d) taps[d] /= z;
  return RTI_OK;
}

extern "C" int rti_map_unsharp(const float* src, int channels, int layout, int H, int W, double sigma, int radius,
                               double amount, int renorm, float* dst, rti_stream_t stream) {
  const char* const E = "rti_map_unsharp";
  if (int st = check_pointers(E, {src, dst})) return st;
  if (H < 1 || W < 1) return fail(RTI_ERR_BAD_ARG, "%s: H and W must be positive", E);
  if (channels < 1 || channels > 16) return fail(RTI_ERR_BAD_ARG, "%s: channels %d outside [1, 16]", E, channels);
  if ((int64_t)H * W >= ((int64_t)1 << 31) || (int64_t)H * W * channels >= ((int64_t)1 << 31))
    return fail(RTI_ERR_BAD_ARG, "%s: H*W*channels must be below 2^31", E);
  if (int st = check_coef_layout(E, layout)) return st;
  if (!sigma_ok(sigma)) return fail(RTI_ERR_BAD_ARG, "%s: sigma %g must be finite and positive", E, sigma);
  const int R = radius ? radius : rti_gauss_radius(sigma);
  if (!radius && R > MAXR)
    return fail(RTI_ERR_BAD_ARG, "%s: the default radius ceil(3*sigma) = %d exceeds %d; pass a radius in [1, %d]", E, R,
                MAXR, MAXR);
  if (R < 1 || R > MAXR) return fail(RTI_ERR_BAD_ARG, "%s: radius %d outside [1, %d]", E, R, MAXR);
  if (!std::isfinite(amount)) return fail(RTI_ERR_BAD_ARG, "%s: non-finite amount", E);
  if (renorm && channels != 3) return fail(RTI_ERR_BAD_ARG, "%s: renorm needs 3 channels, got %d", E, channels);
  const uintptr_t bytes = (uintptr_t)((int64_t)H * W * channels) * sizeof(float);
  const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
  if (s0 < d0 + bytes && d0 < s0 + bytes) return fail(RTI_ERR_BAD_ARG, "%s: src and dst overlap", E);
  Taps tp;
  for (int d = 0; d <= MAXR; ++d) tp.w[d] = 0.0;
  if (int st = rti_gauss_taps(sigma, R, tp.w)) return st;
  int vec = 1;
  if (layout == RTI_COEF_PLANAR)
    vec = W % 4 == 0 && aligned_to(src, 16) ? 4 : 1;
  else if (channels % 4 == 0 && aligned_to(src, 16))
    vec = 4;
  else if (channels % 2 == 0 && aligned_to(src, 8))
    vec = 2;
  hipStream_t s = (hipStream_t)stream;
  if (layout == RTI_COEF_PLANAR)
    return renorm ? launch_unsharp<RTI_COEF_PLANAR, true>(src, dst, channels, H, W, R, tp, amount, vec, s)
                  : launch_unsharp<RTI_COEF_PLANAR, false>(src, dst, channels, H, W, R, tp, amount, vec, s);
  return renorm ? launch_unsharp<RTI_COEF_PIXEL_MAJOR, true>(src, dst, channels, H, W, R, tp, amount, vec, s)
                : launch_unsharp<RTI_COEF_PIXEL_MAJOR, false>(src, dst, channels, H, W, R, tp, amount, vec, s);
}

extern "C" int rti_shade_normals(const float* normals, int normal_layout, const float* albedo, int64_t P, double kd,
                                 double ks, int spec_exp, double lu, double lv, void* out, int out_dtype,
                                 rti_stream_t stream) {
  const char* const E = "rti_shade_normals";
  if (int st = check_pointers(E, {normals, out})) return st;
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  if (int st = check_normal_layout(E, normal_layout)) return st;
  if (!std::isfinite(lu) || !std::isfinite(lv)) return fail(RTI_ERR_BAD_ARG, "%s: non-finite light direction", E);
  if (!std::isfinite(kd) || !std::isfinite(ks)) return fail(RTI_ERR_BAD_ARG, "%s: non-finite kd or ks", E);
  if (spec_exp < 1 || spec_exp > 255) return fail(RTI_ERR_BAD_ARG, "%s: spec_exp %d outside [1, 255]", E, spec_exp);
  if (int st = check_out_dtype(E, out_dtype)) return st;
  const LightFrame f = light_frame(lu, lv);
  const int vec =
      P % 4 == 0 && aligned_to(normals, 16) && (!albedo || aligned_to(albedo, 16)) && rgb_out_vec(out, out_dtype);
  const Shade q{kd, ks, spec_exp, f.lu, f.lv, f.lw, f.hx, f.hy, f.hz};
  with_normal_layout(normal_layout, [&](auto nl) {
    with_out(out_dtype, [&](auto t) {
      lane4::launch(shade_normals_k<decltype(nl)::value, decltype(t)>, P, (hipStream_t)stream, normals, albedo, P, vec,
                    q, out);
    });
  });
  return check_launch(E);
}
