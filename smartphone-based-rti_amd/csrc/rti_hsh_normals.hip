// rti_hsh_normals.hip -- what a fitted HSH map says about the surface (gfx950): the light direction at which each
// pixel's fitted function peaks, found by a search over a grid of directions.
//
//     rti_peak_table     the basis values of the E grid points of (basis, grid), once per object or session
//     rti_hsh_normals    one or three fp32 HSH maps -> normal [3], kind, peak value
//     rti_hsh8_normals   the 8-bit RGB map of rti_hsh8.hip -> the same
//
// The semantics are include/rti.h's.  A grid value is rti_relight's F32 value of the luminance map at that
// direction bit for bit: the table holds what the same device hsh_eval<float> returns for ((float)u, (float)v),
// and the chain is rti_relight's dot_k (l_0·b_0, then fused multiply-adds in term order).  That fixes the
// summation order, so this is a VALU kernel: the matrix cores sum in another order.  It is the one kernel of the
// viewer side that arithmetic bounds: P·E·k fused multiply-adds against 4k (or 3k bytes) + 17 bytes per pixel.
//
// Lane map: a workgroup of 256 lanes owns 512 consecutive pixels, wave w the two runs of 64 that start at
// 128·w and 128·w + 64, lane l pixel l of both.  A lane keeps the 2k luminance coefficients of its two pixels in
// registers.  The workgroup copies the table into LDS once; in the sweep every lane of a wave reads the same k
// values of a grid point (a broadcast read, which still costs the LDS its cycles: §4.10) and feeds them to both
// pixels' chains, so the LDS moves half the bytes per multiply-add that one pixel per lane would.  A lane keeps
// a running maximum, minimum and the index of the maximum; after the sweep it evaluates the four neighbours'
// chains again from the table at its own indices -- the same values and the same chain, hence the same bits --
// and refines in fp64.  No grid value is ever written to memory.
//
// The LDS region of the table first serves as the waves' staging slabs: pixel-major fp32 rows and the bytes of a
// full run come in as whole 16-byte pieces (rti_hsh_px.h), a workgroup barrier ends that phase, and the table is
// copied over it.  A pointer off its alignment, a channel stride that is no multiple of 4 and the last partial
// run load per lane; planar maps are coalesced as they are.  Every path ends in the same registers and the same
// per-pixel arithmetic, so the bits do not depend on it.  Pixel-major normals (12 B per pixel) leave through a
// slab of their own as three contiguous 256-byte stores per run (rti_normals.hip's idea).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "rti_basis.h"
#include "rti_dispatch.h"
#include "rti_hsh_px.h"
#include "rti_stack.h"

namespace rti {
namespace {

using namespace hsh_px;

constexpr int GRID_MIN = 4, GRID_MAX = 16;
constexpr int ROWS_MAX = 2 * GRID_MAX + 1;
constexpr int NPX = 2;             // pixels per lane
constexpr int CHUNK = 256 * NPX;   // pixels of a workgroup
constexpr int OUT_V4 = 64 * 3 / 4; // a run's normals in 16-byte units

// half width of row j: the largest w with w² + j² <= G² (integers; |j| <= G)
__host__ __device__ inline int row_half_width(int G, int j) {
  int w = 0;
  while ((w + 1) * (w + 1) + j * j <= G * G) ++w;
  return w;
}

inline int grid_points(int G) {
  if (G < GRID_MIN || G > GRID_MAX) return -1;
  int n = 0;
  for (int j = -G; j <= G; ++j) n += 2 * row_half_width(G, j) + 1;
  return n;
}

// the table: E rows of k floats, padded with zeros to whole 16-byte pieces
__host__ __device__ inline int64_t table_v4(int k, int E) { return ((int64_t)E * k + 3) / 4; }

// ---- rti_peak_table ---------------------------------------------------------------------------------------------

template <int K>
__global__ void __launch_bounds__(256) peak_table_k(int G, int E, float* __restrict__ table) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) {
    if (e == E)  // the pad of the last 16-byte piece
      for (int i = E * K; i < (int)table_v4(K, E) * 4; ++i) table[i] = 0.0f;
    return;
  }
  int j = -G, start = 0;
  for (;; ++j) {
    const int n = 2 * row_half_width(G, j) + 1;
    if (e < start + n) break;
    start += n;
  }
  const int i = e - start - row_half_width(G, j);
  const double u = (double)i / (double)G, v = (double)j / (double)G;
  float b[K];
  hsh_eval<float>((float)u, (float)v, K, b);  // basis_eval<float>'s HSH branch, as rti_relight runs it
#pragma unroll
  for (int t = 0; t < K; ++t) table[(int64_t)e * K + t] = b[t];
}

// ---- per-pixel arithmetic (tests/hsh_normals_ref.py restates it line by line) ---------------------------------

// three maps -> the luminance map: two products and two sums, each rounded
template <int K>
__device__ __forceinline__ void luminance(const float (&c)[3][K], float wr, float wg, float wb, float (&l)[K]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const float rg = wr * c[0][j] + wg * c[1][j];
    l[j] = rg + wb * c[2][j];
  }
}

// the parabolic step along one axis: vm and vp are the neighbours' values, has: both lie inside the mask
__device__ __forceinline__ double parabolic_step(bool has, float vm, float v0, float vp) {
#pragma clang fp contract(off)
  const double m = (double)vm, z = (double)v0, p = (double)vp;
  const double d = (m - 2.0 * z) + p;
  double t = 0.5 * (m - p) / d;
  t = t < -0.5 ? -0.5 : t;
  t = t > 0.5 ? 0.5 : t;
  return has && d < 0.0 ? t : 0.0;
}

struct NormalOut {
  float n[3];
  float peak;
  uint8_t kind;
};

// i, j: the peak's grid point; du, dv: its parabolic steps; flat: max V == min V; finite: every l_j is finite
__device__ __forceinline__ NormalOut normal_of(int G, int i, int j, double du, double dv, float v0, bool flat,
                                               bool finite) {
#pragma clang fp contract(off)
  const double u0 = ((double)i + du) / (double)G, w0 = ((double)j + dv) / (double)G;
  const double r2 = u0 * u0 + w0 * w0;
  const bool inside = r2 <= 1.0;
  const double s = sqrt(inside ? 1.0 - r2 : r2);
  NormalOut o;
  o.n[0] = (float)(inside ? u0 : u0 / s);
  o.n[1] = (float)(inside ? w0 : w0 / s);
  o.n[2] = (float)(inside ? s : 0.0);
  o.kind = inside ? 0 : 1;
  o.peak = v0;
  if (flat) {
    o.n[0] = o.n[1] = 0.0f;
    o.n[2] = 1.0f;
    o.kind = 2;
  }
  if (!finite) {
    o.n[0] = o.n[1] = o.n[2] = o.peak = NAN;
    o.kind = 4;
  }
  return o;
}

// ---- the grid in LDS ----------------------------------------------------------------------------------------------

struct Grid {
  int G, E;
  const float* tab;  // [E][K]
  const int* start;  // [2G + 1]: the index of row j's first point, j = -G..G
  const int* half;   // [2G + 1]: its half width
};

// the index of grid point (i, j), or -1 outside the mask
__device__ __forceinline__ int point_index(const Grid& g, int i, int j) {
  if (j < -g.G || j > g.G) return -1;
  const int w = g.half[j + g.G];
  return i < -w || i > w ? -1 : g.start[j + g.G] + i + w;
}

template <int K>
__device__ __forceinline__ float value_at(const Grid& g, const float (&l)[K], int e, float fallback) {
  return e < 0 ? fallback : dot_k<K>(l, g.tab + e * K);
}

// the sweep over the E points for the lane's NPX pixels, then each pixel's refinement
template <int K>
__device__ __forceinline__ void search(const Grid& g, const float (&l)[NPX][K], NormalOut (&o)[NPX]) {
  float vmax[NPX], vmin[NPX];
  int best[NPX];
#pragma unroll
  for (int s = 0; s < NPX; ++s) {
    vmax[s] = -INFINITY;
    vmin[s] = INFINITY;
    best[s] = 0;
  }
  for (int e = 0; e < g.E; ++e) {
    float b[K];
#pragma unroll
    for (int t = 0; t < K; ++t) b[t] = g.tab[e * K + t];  // wave-uniform
#pragma unroll
    for (int s = 0; s < NPX; ++s) {
      const float v = dot_k<K>(l[s], b);
      const bool up = v > vmax[s];  // strict: ties stay with the smallest e
      vmax[s] = up ? v : vmax[s];
      best[s] = up ? e : best[s];
      vmin[s] = v < vmin[s] ? v : vmin[s];
    }
  }
#pragma unroll
  for (int s = 0; s < NPX; ++s) {
    bool finite = true;
#pragma unroll
    for (int t = 0; t < K; ++t) finite = finite && fabsf(l[s][t]) <= FLT_MAX;  // false for NaN
    int row = 0;
    for (int r = 1; r <= 2 * g.G; ++r) row = g.start[r] <= best[s] ? r : row;
    const int j = row - g.G, i = best[s] - g.start[row] - g.half[row];
    const float v0 = vmax[s];
    const int em = point_index(g, i - 1, j), ep = point_index(g, i + 1, j);
    const int fm = point_index(g, i, j - 1), fp = point_index(g, i, j + 1);
    const double du = parabolic_step(em >= 0 && ep >= 0, value_at<K>(g, l[s], em, v0), v0, value_at<K>(g, l[s], ep, v0));
    const double dv = parabolic_step(fm >= 0 && fp >= 0, value_at<K>(g, l[s], fm, v0), v0, value_at<K>(g, l[s], fp, v0));
    o[s] = normal_of(g.G, i, j, du, dv, v0, vmax[s] == vmin[s], finite);
  }
}

// ---- the kernel ---------------------------------------------------------------------------------------------------

struct Source {
  const float* coef;       // fp32 maps, or
  const uint8_t* coef8;    // the bytes [p][3][K] and
  const float* qparams;    // their 2K header floats
  int64_t cs;              // channel stride of the fp32 maps in elements
  int vin;                 // the 16-byte pieces may be used
  float w[3];
};

struct Sink {
  float* normals;
  uint8_t* kind;
  float* peak;
};

// LDS in 16-byte units: the table, over the four waves' staging slabs
inline int64_t lds_v4(int k, int E, int in_slab_v4) {
  const int64_t t = table_v4(k, E), s = 4 * (int64_t)in_slab_v4;
  return (t > s ? t : s) + 4 * OUT_V4;
}

// C: 1 or 3 fp32 maps in layout CL, or 0 for the 8-bit map; NL: the normals' layout
template <int K, int C, int CL, int NL>
__global__ void __launch_bounds__(256)
hsh_normals_k(Source src, int64_t P, int G, int E, const u32x4* __restrict__ table, Sink dst) {
  constexpr int IN_SLAB = C == 0 ? slab_v4(run_v4<3 * K>(), 0) : CL == RTI_COEF_PIXEL_MAJOR ? slab_v4(run_v4<4 * K>(), 0) : 0;
  extern __shared__ u32x4 lds[];  // [max(table, 4·IN_SLAB)] then [4][OUT_V4]
  __shared__ int row_start[ROWS_MAX], row_half[ROWS_MAX];
  __shared__ float qs[2 * K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tv4 = table_v4(K, E);
  const int64_t in_v4 = tv4 > 4 * IN_SLAB ? tv4 : 4 * IN_SLAB;
  u32x4* in_slab = lds + wave * IN_SLAB;
  u32x4* out_slab = lds + in_v4 + wave * OUT_V4;

  if constexpr (C == 0) load_steps<K>(src.qparams, qs);
  if (threadIdx.x <= 2 * G) row_half[threadIdx.x] = row_half_width(G, (int)threadIdx.x - G);
  __syncthreads();
  if (threadIdx.x <= 2 * G) {
    int n = 0;
    for (int r = 0; r < (int)threadIdx.x; ++r) n += 2 * row_half[r] + 1;
    row_start[threadIdx.x] = n;
  }

  // every lane stays to the end: the workgroup fills the table together
  const int64_t wave_px = (int64_t)blockIdx.x * CHUNK + wave * (64 * NPX);
  // the two sources are rti_hsh_px.h's load_px8 and load_px written out: as calls they move the occupancy of 11 of the
  // 20 instantiations of this kernel, the one that arithmetic bounds
  float l[NPX][K];
#pragma unroll
  for (int s = 0; s < NPX; ++s) {
    const int64_t run_px = wave_px + 64 * s, p = run_px + lane;
    const bool live = p < P, full = run_px + 64 <= P;  // full: wave-uniform
    if constexpr (C == 0) {
      constexpr int NB = 3 * K, NW = (NB + 3) / 4;
      uint32_t w[NW];
#pragma unroll
      for (int i = 0; i < NW; ++i) w[i] = 0;
      if (src.vin && full) {
        run_in<NB>(src.coef8 + run_px * NB, lane, in_slab);
        lane_words<NB>(in_slab, lane, w);
      } else if (live) {
#pragma unroll
        for (int i = 0; i < NB; ++i) w[i >> 2] |= (uint32_t)src.coef8[p * NB + i] << (8 * (i & 3));
      }
      float c[3][K];
      dequantise_px<K>(w, qs, c);
      luminance<K>(c, src.w[0], src.w[1], src.w[2], l[s]);
    } else {
      float c[C][K];
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        const float* map = src.coef + ch * src.cs;
        bool staged = false;
        if constexpr (CL == RTI_COEF_PIXEL_MAJOR) {
          if (src.vin && full) {  // wave-uniform
            run_in<4 * K>(map + run_px * K, lane, in_slab);
            uint32_t w[K];
            lane_words<4 * K>(in_slab, lane, w);
#pragma unroll
            for (int j = 0; j < K; ++j) c[ch][j] = __uint_as_float(w[j]);
            staged = true;
          }
        }
        if (!staged) {
#pragma unroll
          for (int j = 0; j < K; ++j)
            c[ch][j] = !live ? 0.0f : CL == RTI_COEF_PLANAR ? map[(int64_t)j * P + p] : map[p * K + j];
        }
      }
      if constexpr (C == 3) {
        luminance<K>(c, src.w[0], src.w[1], src.w[2], l[s]);
      } else {
#pragma unroll
        for (int j = 0; j < K; ++j) l[s][j] = c[0][j];
      }
    }
  }

  __syncthreads();  // the slabs have been read (and row_start is written): the table goes over them
  for (int64_t i = threadIdx.x; i < tv4; i += 256) lds[i] = table[i];
  __syncthreads();

  const Grid g{G, E, reinterpret_cast<const float*>(lds), row_start, row_half};
  NormalOut o[NPX];
  search<K>(g, l, o);

#pragma unroll
  for (int s = 0; s < NPX; ++s) {
    const int64_t run_px = wave_px + 64 * s, p = run_px + lane;
    if (run_px >= P) break;  // wave-uniform; no workgroup barrier below
    const bool live = p < P, full = run_px + 64 <= P;
    if (live) {
      if (dst.kind) dst.kind[p] = o[s].kind;
      if (dst.peak) dst.peak[p] = o[s].peak;
    }
    if constexpr (NL == RTI_NORMAL_PLANAR) {
      if (live) {
#pragma unroll
        for (int i = 0; i < 3; ++i) dst.normals[(int64_t)i * P + p] = o[s].n[i];
      }
    } else if (full) {  // the run's 192 floats as three contiguous 256-byte stores
      float* sw = reinterpret_cast<float*>(out_slab);
#pragma unroll
      for (int i = 0; i < 3; ++i) sw[3 * lane + i] = o[s].n[i];
      wave_lds_sync();
      float* rows = dst.normals + run_px * 3;
#pragma unroll
      for (int i = 0; i < 3; ++i) rows[i * 64 + lane] = sw[i * 64 + lane];
      wave_lds_sync();  // the slab may be written again
    } else if (live) {
#pragma unroll
      for (int i = 0; i < 3; ++i) dst.normals[p * 3 + i] = o[s].n[i];
    }
  }
}

// ---- launchers ----------------------------------------------------------------------------------------------------

struct Launch {
  Source src;
  int64_t P;
  int G, E;
  const void* table;
  Sink dst;
  hipStream_t s;
};

// C = 0: the 8-bit map
template <int K, int C, int CL>
void launch(const Launch& a, int nl) {
  constexpr int IN_SLAB = C == 0 ? slab_v4(run_v4<3 * K>(), 0) : CL == RTI_COEF_PIXEL_MAJOR ? slab_v4(run_v4<4 * K>(), 0) : 0;
  const size_t lds_bytes = (size_t)lds_v4(K, a.E, IN_SLAB) * 16;  // at most 51008 + 3072 bytes: under the 64 KiB default
  with_normal_layout(nl, [&](auto n) {
    hipLaunchKernelGGL((hsh_normals_k<K, C, CL, decltype(n)::value>), dim3(grid_1d(a.P, CHUNK)), dim3(256), lds_bytes, a.s,
                       a.src, a.P, a.G, a.E, static_cast<const u32x4*>(a.table), a.dst);
  });
}

// ---- checks -------------------------------------------------------------------------------------------------------

int check_basis_grid(const char* entry, int basis, int grid) {
  if (!hsh_basis(basis)) return fail(RTI_ERR_UNSUPPORTED, "%s: basis %d (HSH-9 and HSH-16 only)", entry, basis);
  if (grid < GRID_MIN || grid > GRID_MAX)
    return fail(RTI_ERR_BAD_ARG, "%s: grid %d outside [%d, %d]", entry, grid, GRID_MIN, GRID_MAX);
  return RTI_OK;
}

// what the two map entries share after their own map checks; fills the weights
int check_search(const char* entry, int basis, int normal_layout, int grid, const float* w, const void* table,
                 float (&weights)[3]) {
  if (int st = check_normal_layout(entry, normal_layout)) return st;
  if (int st = check_basis_grid(entry, basis, grid)) return st;
  weights[0] = w ? w[0] : 0.299f;
  weights[1] = w ? w[1] : 0.587f;
  weights[2] = w ? w[2] : 0.114f;
  for (float x : weights)
    if (!std::isfinite(x)) return fail(RTI_ERR_BAD_ARG, "%s: non-finite weight", entry);
  if (!aligned_to(table, 16)) return fail(RTI_ERR_BAD_ARG, "%s: table must be 16-byte aligned", entry);
  return RTI_OK;
}

}  // namespace
}  // namespace rti

using namespace rti;

extern "C" int rti_peak_grid_points(int grid) { return grid_points(grid); }

extern "C" int64_t rti_peak_table_bytes(int basis, int grid) {
  const int E = grid_points(grid);
  return !hsh_basis(basis) || E < 0 ? 0 : table_v4(basis_terms(basis), E) * 16;
}

extern "C" int rti_peak_table(int basis, int grid, void* table, rti_stream_t stream) {
  const char* const E = "rti_peak_table";
  if (int st = check_pointers(E, {table})) return st;
  if (int st = check_basis_grid(E, basis, grid)) return st;
  if (!aligned_to(table, 16)) return fail(RTI_ERR_BAD_ARG, "%s: table must be 16-byte aligned", E);
  const int n = grid_points(grid);
  const dim3 blocks(grid_1d(n + 1, 256));  // + 1: the thread that zeroes the pad
  note_launches(1);
  if (basis == RTI_BASIS_HSH9)
    hipLaunchKernelGGL(peak_table_k<9>, blocks, dim3(256), 0, (hipStream_t)stream, grid, n, static_cast<float*>(table));
  else
    hipLaunchKernelGGL(peak_table_k<16>, blocks, dim3(256), 0, (hipStream_t)stream, grid, n, static_cast<float*>(table));
  return check_launch(E);
}

extern "C" int rti_hsh_normals(const float* coef, int basis, int coef_layout, int C, int64_t coef_channel_stride,
                               int64_t P, const float* w, int grid, const void* table, float* normals,
                               int normal_layout, uint8_t* kind, float* peak, rti_stream_t stream) {
  const char* const E = "rti_hsh_normals";
  if (int st = check_pointers(E, {coef, table, normals})) return st;
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  if (C != 1 && C != 3) return fail(RTI_ERR_BAD_ARG, "%s: C = %d (one map or three)", E, C);
  if (int st = check_coef_layout(E, coef_layout)) return st;
  float weights[3];
  if (int st = check_search(E, basis, normal_layout, grid, w, table, weights)) return st;
  const int k = basis_terms(basis);
  if (int st = check_coef_stride(E, coef_view(coef, coef_layout, k, P, coef_channel_stride), P, C)) return st;
  const int64_t cs = coef_channel_stride ? coef_channel_stride : P * k;
  const int vin = maps_staged(coef, coef_layout, C, cs);
  const Launch a{Source{coef, nullptr, nullptr, cs, vin, {weights[0], weights[1], weights[2]}}, P, grid,
                 grid_points(grid), table, Sink{normals, kind, peak}, (hipStream_t)stream};
  note_launches(1);
  with_hsh_terms(k, [&](auto kt) {
    with_channels(C, [&](auto ct) {
      with_layout(coef_layout, [&](auto l) {
        launch<decltype(kt)::value, decltype(ct)::value, decltype(l)::value>(a, normal_layout);
      });
    });
  });
  return check_launch(E);
}

extern "C" int rti_hsh8_normals(const uint8_t* coef8, int basis, int64_t P, const float* qparams, const float* w,
                                int grid, const void* table, float* normals, int normal_layout, uint8_t* kind,
                                float* peak, rti_stream_t stream) {
  const char* const E = "rti_hsh8_normals";
  if (int st = check_pointers(E, {coef8, qparams, table, normals})) return st;
  if (P < 1) return fail(RTI_ERR_BAD_ARG, "%s: P must be positive", E);
  float weights[3];
  if (int st = check_search(E, basis, normal_layout, grid, w, table, weights)) return st;
  if (!aligned_to(qparams, 4)) return fail(RTI_ERR_BAD_ARG, "%s: qparams must be 4-byte aligned", E);
  const Launch a{Source{nullptr, coef8, qparams, 0, aligned_to(coef8, 16) ? 1 : 0, {weights[0], weights[1], weights[2]}},
                 P, grid, grid_points(grid), table, Sink{normals, kind, peak}, (hipStream_t)stream};
  note_launches(1);
  with_hsh_terms(basis_terms(basis),
                 [&](auto kt) { launch<decltype(kt)::value, 0, RTI_COEF_PIXEL_MAJOR>(a, normal_layout); });
  return check_launch(E);
}
