// rti_multilight.hip -- multi-light detail enhancement (gfx950): for every tile of the image the
// candidate light that shows its relief best, the choices smoothed into a light field, and a relight with a light
// direction per pixel.
//
//     rti_light_scores    one or three fp32 maps + E candidate lights -> per tile and candidate: sharpness, brightness
//     rti_light_field     the scores -> the winning candidate per tile, smoothed over the tile grid: field [Ty][Tx][2]
//     rti_relight_field   the maps under a light per pixel: bilinear from a tile field, or given per pixel
//
// The semantics are include/rti.h's.  A candidate's value at a pixel is rti_relight's F32 value of the luminance map
// bit for bit (rti_hsh_normals.hip's argument: the same basis_eval<float>, the same chain), so the search is a VALU
// kernel with the arithmetic of rti_hsh_normals: P·E·k fused multiply-adds against the maps read once.  No candidate
// frame is ever written to memory.
//
// rti_light_scores, lane map: one workgroup per tile.  T = 8 is one wave with a pixel per lane, T = 16 four waves with
// a pixel per lane, T = 32 four waves with four pixels per lane (pixel i of the tile, row-major, belongs to lane
// i % NT as its pixel i / NT).  A lane keeps the luminance coefficients of its pixels in registers; the E basis rows
// sit in LDS (a broadcast read per term).  Per candidate every lane writes its values to one of two LDS planes of T·T
// floats, one barrier, then reads its right and its lower neighbour from that plane: the second plane lets the next
// candidate's writes start before every lane has read this one's (two barriers apart, see the loop).  The squared
// differences and the values are summed in fp64 per lane, reduced over the wave by shuffles in a fixed order and
// joined over the waves in wave order after the loop: no atomics on floating point, so a call gives the same bits
// run to run.  Which pixels are usable and which pairs exist does not depend on the candidate: a mask in LDS, formed
// once; the two counts are integer atomics on LDS.
//
// rti_light_field is a thread per tile: the choice, then `smooth` passes of the 3x3 binomial between the two fp64
// halves of the workspace, the last pass (or the choice itself when smooth = 0) rounding to fp32 once.
//
// rti_relight_field is rti_hsh_render_px.h's lane map (a pixel per lane, 64 consecutive pixels per wave) with its
// loads and its store: the basis row is evaluated per pixel at the pixel's own light, as rti_hsh_gain.hip evaluates it
// at the pixel's normal.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "rti_basis.h"
#include "rti_convert.h"
#include "rti_dispatch.h"
#include "rti_hsh_render_px.h"
#include "rti_stack.h"

namespace rti {
namespace {

using namespace hsh_render;  // the chain, a wave's runs through its slab, load_px, store_dir and their predicates

constexpr int MAXC = RTI_LIGHT_MAX_CANDIDATES;
constexpr int MAX_SMOOTH = 8;

struct Cand {
  double lu, lv;
};
struct Cands {  // a kernel argument: 64 × 16 bytes
  Cand d[MAXC];
};

// basis_eval<float> with the terms known at compile time
template <int K>
__device__ __forceinline__ void basis_row(float lu, float lv, float (&b)[K]) {
  if constexpr (K == 6)
    ptm_eval<float>(lu, lv, b);
  else
    hsh_eval<float>(lu, lv, K, b);
}

// three maps -> the luminance map: two products and two sums, each rounded (rti_hsh_normals.hip's)
template <int K>
__device__ __forceinline__ void luminance(const float (&c)[3][K], float wr, float wg, float wb, float (&l)[K]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const float rg = wr * c[0][j] + wg * c[1][j];
    l[j] = rg + wb * c[2][j];
  }
}

// f(Tag<K>) for the three bases (after the entry's check of the basis)
template <typename F>
inline void with_terms(int k, F&& f) {
  if (k == 6)
    f(Tag<6>{});
  else
    with_hsh_terms(k, f);
}

// f(Tag<T>) for the three tile edges (after check_tile)
template <typename F>
inline void with_tile(int T, F&& f) {
  if (T == 8)
    f(Tag<8>{});
  else if (T == 16)
    f(Tag<16>{});
  else
    f(Tag<32>{});
}

// ---- rti_light_scores ---------------------------------------------------------------------------------------------

struct Weights {
  float r, g, b;
};

// the sum over the wave's lanes in a fixed order; every lane gets it
__device__ __forceinline__ double wave_sum(double v) {
#pragma clang fp contract(off)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
  return v;
}

template <int K, int C, int CL, int T>
__global__ void __launch_bounds__(T == 8 ? 64 : 256)
light_scores_k(const float* __restrict__ coef, int64_t cs, int H, int W, int Tx, Weights w, Cands cands, int E,
               double* __restrict__ scores, int32_t* __restrict__ count) {
  constexpr int NT = T == 8 ? 64 : 256;  // lanes of the workgroup
  constexpr int NPX = T * T / NT;        // pixels of a lane
  constexpr int NW = NT / 64;
  __shared__ float btab[MAXC * K];
  __shared__ float vplane[2][T * T];
  __shared__ uint8_t usable[T * T];
  __shared__ double part[MAXC][NW][2];
  __shared__ int n_px, n_pairs;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = blockIdx.x / Tx, tx = blockIdx.x % Tx;
  const int64_t P = (int64_t)H * W;

  if (tid < E) {
    float b[K];
    basis_row<K>((float)cands.d[tid].lu, (float)cands.d[tid].lv, b);
#pragma unroll
    for (int j = 0; j < K; ++j) btab[tid * K + j] = b[j];
  }
  if (tid == 0) n_px = n_pairs = 0;

  // the lane's pixels: their luminance coefficients, and whether all of them are finite
  float l[NPX][K];
  bool ok[NPX];
#pragma unroll
  for (int s = 0; s < NPX; ++s) {
    const int i = s * NT + tid, y = ty * T + i / T, x = tx * T + i % T;
    const bool live = y < H && x < W;
    const int64_t p = (int64_t)y * W + x;
    float c[C][K];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      const float* map = coef + ch * cs;
#pragma unroll
      for (int j = 0; j < K; ++j)
        c[ch][j] = !live ? 0.0f : CL == RTI_COEF_PLANAR ? map[(int64_t)j * P + p] : map[p * K + j];
    }
    if constexpr (C == 3) {
      luminance<K>(c, w.r, w.g, w.b, l[s]);
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j) l[s][j] = c[0][j];
    }
    bool finite = live;
#pragma unroll
    for (int j = 0; j < K; ++j) finite = finite && fabsf(l[s][j]) <= FLT_MAX;  // false for NaN
    ok[s] = finite;
    usable[i] = finite ? 1 : 0;
  }
  __syncthreads();  // btab, usable and the two counters are written

  // the pairs of a pixel: with its right and with its lower neighbour inside the tile
  bool right[NPX], down[NPX];
  int mine = 0, pairs = 0;
#pragma unroll
  for (int s = 0; s < NPX; ++s) {
    const int i = s * NT + tid, row = i / T, col = i % T;
    right[s] = ok[s] && col + 1 < T && usable[i + 1];
    down[s] = ok[s] && row + 1 < T && usable[i + T];
    mine += ok[s] ? 1 : 0;
    pairs += (right[s] ? 1 : 0) + (down[s] ? 1 : 0);
  }
  if (mine) atomicAdd(&n_px, mine);  // integers: any order gives the same sum
  if (pairs) atomicAdd(&n_pairs, pairs);

  for (int e = 0; e < E; ++e) {
    // Plane e & 1.  A lane that writes it for candidate e + 2 has passed the barrier of candidate e + 1, which every
    // lane reaches only after its reads of candidate e.
    float* plane = vplane[e & 1];
    float v[NPX];
#pragma unroll
    for (int s = 0; s < NPX; ++s) {
      v[s] = dot_k<K>(l[s], btab + e * K);
      plane[s * NT + tid] = v[s];
    }
    __syncthreads();
    double S = 0.0, B = 0.0;
    {
#pragma clang fp contract(off)
#pragma unroll
      for (int s = 0; s < NPX; ++s) {
        const int i = s * NT + tid;
        const double here = (double)v[s];
        if (right[s]) {
          const double d = (double)plane[i + 1] - here;
          S = S + d * d;
        }
        if (down[s]) {
          const double d = (double)plane[i + T] - here;
          S = S + d * d;
        }
        if (ok[s]) B = B + here;
      }
    }
    S = wave_sum(S);
    B = wave_sum(B);
    if (lane == 0) {
      part[e][wave][0] = S;
      part[e][wave][1] = B;
    }
  }
  __syncthreads();  // part and the two counters are complete

  const int nP = n_px, nS = n_pairs;
  if (tid < E) {
#pragma clang fp contract(off)
    double S = part[tid][0][0], B = part[tid][0][1];
#pragma unroll
    for (int wv = 1; wv < NW; ++wv) {
      S = S + part[tid][wv][0];
      B = B + part[tid][wv][1];
    }
    double* o = scores + ((int64_t)blockIdx.x * E + tid) * 2;
    o[0] = nS ? S / (double)nS : 0.0;
    o[1] = nP ? B / (double)nP : 0.0;
  }
  if (tid == 0 && count) count[blockIdx.x] = nP;
}

// ---- rti_light_field ------------------------------------------------------------------------------------------------

// a tile's light: fp64 into the workspace, or rounded once into the field
__device__ __forceinline__ void put_light(double lu, double lv, int64_t t, double* __restrict__ dst64,
                                          float* __restrict__ field) {
  if (dst64) {
    dst64[2 * t] = lu;
    dst64[2 * t + 1] = lv;
  } else {
    field[2 * t] = (float)lu;
    field[2 * t + 1] = (float)lv;
  }
}

__global__ void __launch_bounds__(256)
light_choice_k(const double* __restrict__ scores, const int32_t* __restrict__ count, int64_t tiles, Cands cands, int E,
               double ws, double wb, double lu0, double lv0, double* __restrict__ dst64, float* __restrict__ field,
               int32_t* __restrict__ choice) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= tiles) return;
  const double* sc = scores + t * E * 2;
  double smax = 0.0, bmax = 0.0;  // a NaN never raises either
  for (int e = 0; e < E; ++e) {
    smax = sc[2 * e] > smax ? sc[2 * e] : smax;
    bmax = sc[2 * e + 1] > bmax ? sc[2 * e + 1] : bmax;
  }
  int best = -1;
  double top = 0.0;
  if (count[t] != 0) {
    for (int e = 0; e < E; ++e) {
      const double sn = smax > 0.0 ? sc[2 * e] / smax : 0.0;
      const double bn = bmax > 0.0 ? sc[2 * e + 1] / bmax : 0.0;
      const double a = ws * sn, b = wb * bn;
      const double score = a + b;
      if (score == score && (best < 0 || score > top)) {  // strict: ties stay with the smallest e
        best = e;
        top = score;
      }
    }
  }
  if (choice) choice[t] = best;
  put_light(best < 0 ? lu0 : cands.d[best].lu, best < 0 ? lv0 : cands.d[best].lv, t, dst64, field);
}

__global__ void __launch_bounds__(256)
light_smooth_k(const double* __restrict__ src, int Ty, int Tx, double* __restrict__ dst64, float* __restrict__ field) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)Ty * Tx) return;
  const int ty = (int)(t / Tx), tx = (int)(t % Tx);
  double au = 0.0, av = 0.0, wsum = 0.0;
  for (int dy = -1; dy <= 1; ++dy) {
    for (int dx = -1; dx <= 1; ++dx) {
      const int y = ty + dy, x = tx + dx;
      if (y < 0 || y >= Ty || x < 0 || x >= Tx) continue;
      const double wt = (double)((2 - (dy < 0 ? -dy : dy)) * (2 - (dx < 0 ? -dx : dx)));  // 1, 2 or 4
      const double* f = src + ((int64_t)y * Tx + x) * 2;
      const double pu = wt * f[0], pv = wt * f[1];
      au = au + pu;
      av = av + pv;
      wsum = wsum + wt;
    }
  }
  put_light(au / wsum, av / wsum, t, dst64, field);
}

// ---- rti_relight_field ----------------------------------------------------------------------------------------------

// the tile field at pixel (x, y), bilinear between the tile centres in fp64
__device__ __forceinline__ void field_at(const float* __restrict__ f, int Ty, int Tx, int T, int x, int y, double& lu,
                                         double& lv) {
#pragma clang fp contract(off)
  const double half = (double)(T - 1) / 2.0, edge = (double)T;
  double fx = ((double)x - half) / edge, fy = ((double)y - half) / edge;
  fx = fx < 0.0 ? 0.0 : fx;
  fx = fx > (double)(Tx - 1) ? (double)(Tx - 1) : fx;
  fy = fy < 0.0 ? 0.0 : fy;
  fy = fy > (double)(Ty - 1) ? (double)(Ty - 1) : fy;
  const int i0 = (int)floor(fx), j0 = (int)floor(fy);
  const int i1 = i0 + 1 < Tx ? i0 + 1 : Tx - 1, j1 = j0 + 1 < Ty ? j0 + 1 : Ty - 1;
  const double a = fx - (double)i0, b = fy - (double)j0;
  const float* f00 = f + ((int64_t)j0 * Tx + i0) * 2;
  const float* f10 = f + ((int64_t)j0 * Tx + i1) * 2;
  const float* f01 = f + ((int64_t)j1 * Tx + i0) * 2;
  const float* f11 = f + ((int64_t)j1 * Tx + i1) * 2;
  double r[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const double v00 = (double)f00[c], v10 = (double)f10[c], v01 = (double)f01[c], v11 = (double)f11[c];
    const double top = v00 + a * (v10 - v00);
    const double bottom = v01 + a * (v11 - v01);
    r[c] = top + b * (bottom - top);
  }
  lu = r[0];
  lv = r[1];
}

struct FieldArgs {
  const float* light;
  int form, Ty, Tx, T, W;
};

template <int K, int C, int CL, typename TO>
__global__ void __launch_bounds__(256)
relight_field_k(const float* __restrict__ coef, int64_t cs, int64_t P, int vin, int vout, FieldArgs fa,
                TO* __restrict__ out) {
  constexpr int SLAB = render_slab(CL == RTI_COEF_PIXEL_MAJOR ? run_v4<4 * K>() : 0);
  __shared__ u32x4 slabs[4 * SLAB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32x4* slab = slabs + wave * SLAB;
  const int64_t wave_px = ((int64_t)blockIdx.x * 4 + wave) * 64;
  if (wave_px >= P) return;  // wave-uniform; no workgroup barrier in this kernel
  const bool live = wave_px + lane < P, full = wave_px + 64 <= P;  // full: wave-uniform
  const int64_t p = live ? wave_px + lane : P - 1;  // a lane past the image computes the last pixel and stores nothing
  float c[C][K];
  load_px<K, C, CL>(coef, cs, P, wave_px, lane, live, vin && full, 0.0f, slab, c);

  float lu, lv;
  if (fa.form == RTI_LIGHT_PIXELS) {
    lu = fa.light[2 * p];
    lv = fa.light[2 * p + 1];
  } else {
    double du, dv;
    field_at(fa.light, fa.Ty, fa.Tx, fa.T, (int)(p % fa.W), (int)(p / fa.W), du, dv);
    lu = (float)du;
    lv = (float)dv;
  }
  const bool bad = !(fabsf(lu) <= FLT_MAX && fabsf(lv) <= FLT_MAX);
  float b[K];
  basis_row<K>(lu, lv, b);
  TO o[C];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) o[ch] = cvt_out<TO>(bad ? NAN : dot_k<K>(c[ch], b));
  store_dir<C, TO>(o, out + wave_px * C, lane, live, vout && full, slab);
}

// ---- checks ---------------------------------------------------------------------------------------------------------

int check_basis(const char* entry, int basis) {
  if (basis_terms(basis) < 0) return fail(RTI_ERR_UNSUPPORTED, "%s: basis %d (PTM-6, HSH-9 and HSH-16)", entry, basis);
  return RTI_OK;
}

int check_image(const char* entry, int H, int W) {
  if (H < 1 || W < 1) return fail(RTI_ERR_BAD_ARG, "%s: H and W must be positive", entry);
  if ((int64_t)H * W >= ((int64_t)1 << 31)) return fail(RTI_ERR_BAD_ARG, "%s: H*W must be below 2^31", entry);
  return RTI_OK;
}

int check_tile(const char* entry, int T) {
  if (T != 8 && T != 16 && T != 32) return fail(RTI_ERR_BAD_ARG, "%s: tile edge %d (8, 16 or 32)", entry, T);
  return RTI_OK;
}

// the maps of the two entries that read them, in the order include/rti.h lists the arguments
int check_maps(const char* entry, int basis, int coef_layout, int C, int64_t coef_channel_stride, int H, int W) {
  if (int st = check_basis(entry, basis)) return st;
  if (int st = check_coef_layout(entry, coef_layout)) return st;
  if (C != 1 && C != 3) return fail(RTI_ERR_BAD_ARG, "%s: C = %d (one map or three)", entry, C);
  if (int st = check_image(entry, H, W)) return st;
  const int64_t P = (int64_t)H * W;
  return check_coef_stride(entry, coef_view(static_cast<const float*>(nullptr), coef_layout, basis_terms(basis), P,
                                            coef_channel_stride), P, C);
}

// E and the values of luv it counts; fills `c`, candidates past E stay zero
int check_candidates(const char* entry, const double* luv, int E, Cands& c) {
  if (E < 1 || E > MAXC) return fail(RTI_ERR_BAD_ARG, "%s: E = %d outside [1, %d]", entry, E, MAXC);
  for (int i = 0; i < 2 * E; ++i)
    if (!std::isfinite(luv[i])) return fail(RTI_ERR_BAD_ARG, "%s: non-finite candidate direction", entry);
  c = Cands{};
  for (int i = 0; i < E; ++i) c.d[i] = Cand{luv[2 * i], luv[2 * i + 1]};
  return RTI_OK;
}

int64_t field_workspace_bytes(int Ty, int Tx) {
  if (Ty < 1 || Tx < 1 || (int64_t)Ty * Tx >= ((int64_t)1 << 31)) return 0;
  return (int64_t)Ty * Tx * 2 * 2 * (int64_t)sizeof(double);  // two fp64 fields
}

}  // namespace
}  // namespace rti

using namespace rti;

extern "C" int rti_light_scores(const float* coef, int basis, int coef_layout, int C, int64_t coef_channel_stride,
                                int H, int W, int T, const float* w, const double* luv, int E_, double* scores,
                                int32_t* count, rti_stream_t stream) {
  const char* const E = "rti_light_scores";
  if (int st = check_pointers(E, {coef, luv, scores})) return st;
  if (int st = check_maps(E, basis, coef_layout, C, coef_channel_stride, H, W)) return st;
  if (int st = check_tile(E, T)) return st;
  const Weights wt{w ? w[0] : 0.299f, w ? w[1] : 0.587f, w ? w[2] : 0.114f};
  if (!std::isfinite(wt.r) || !std::isfinite(wt.g) || !std::isfinite(wt.b))
    return fail(RTI_ERR_BAD_ARG, "%s: non-finite weight", E);
  Cands cands;
  if (int st = check_candidates(E, luv, E_, cands)) return st;
  if (!aligned_to(scores, 8)) return fail(RTI_ERR_BAD_ARG, "%s: scores must be 8-byte aligned", E);
  const int k = basis_terms(basis);
  const int64_t cs = coef_channel_stride ? coef_channel_stride : (int64_t)H * W * k;
  const int Ty = (H + T - 1) / T, Tx = (W + T - 1) / T;
  note_launches(1);
  with_terms(k, [&](auto kt) {
    with_channels(C, [&](auto ct) {
      with_layout(coef_layout, [&](auto l) {
        with_tile(T, [&](auto t) {
          constexpr int TT = decltype(t)::value;
          hipLaunchKernelGGL((light_scores_k<decltype(kt)::value, decltype(ct)::value, decltype(l)::value, TT>),
                             dim3((unsigned)((int64_t)Ty * Tx)), dim3(TT == 8 ? 64 : 256), 0, (hipStream_t)stream, coef,
                             cs, H, W, Tx, wt, cands, E_, scores, count);
        });
      });
    });
  });
  return check_launch(E);
}

extern "C" size_t rti_light_field_workspace_bytes(int Ty, int Tx) { return (size_t)field_workspace_bytes(Ty, Tx); }

extern "C" int rti_light_field(const double* scores, const int32_t* count, int Ty, int Tx, const double* luv, int E_,
                               double ws, double wb, double lu0, double lv0, int smooth, void* workspace,
                               size_t workspace_bytes, float* field, int32_t* choice, rti_stream_t stream) {
  const char* const E = "rti_light_field";
  if (int st = check_pointers(E, {scores, count, luv, workspace, field})) return st;
  const int64_t need = field_workspace_bytes(Ty, Tx);
  if (need == 0) return fail(RTI_ERR_BAD_ARG, "%s: Ty and Tx must be positive with Ty*Tx below 2^31", E);
  Cands cands;
  if (int st = check_candidates(E, luv, E_, cands)) return st;
  if (!std::isfinite(ws) || !std::isfinite(wb) || ws < 0.0 || wb < 0.0)
    return fail(RTI_ERR_BAD_ARG, "%s: ws and wb must be finite and not negative", E);
  if (!std::isfinite(lu0) || !std::isfinite(lv0)) return fail(RTI_ERR_BAD_ARG, "%s: non-finite main light", E);
  if (smooth < 0 || smooth > MAX_SMOOTH) return fail(RTI_ERR_BAD_ARG, "%s: smooth = %d outside [0, %d]", E, smooth, MAX_SMOOTH);
  if (!aligned_to(workspace, 8) || !aligned_to(scores, 8))
    return fail(RTI_ERR_BAD_ARG, "%s: scores and workspace must be 8-byte aligned", E);
  if ((int64_t)workspace_bytes < need)
    return fail(RTI_ERR_BAD_ARG, "%s: workspace of %lld bytes, %lld needed", E, (long long)workspace_bytes, (long long)need);
  const int64_t tiles = (int64_t)Ty * Tx;
  double* half[2] = {static_cast<double*>(workspace), static_cast<double*>(workspace) + 2 * tiles};
  const dim3 blocks(grid_1d(tiles, 256));
  hipStream_t s = (hipStream_t)stream;
  note_launches(1 + smooth);
  hipLaunchKernelGGL(light_choice_k, blocks, dim3(256), 0, s, scores, count, tiles, cands, E_, ws, wb, lu0, lv0,
                     smooth ? half[0] : nullptr, field, choice);
  for (int i = 0; i < smooth; ++i)
    hipLaunchKernelGGL(light_smooth_k, blocks, dim3(256), 0, s, half[i & 1], Ty, Tx,
                       i + 1 < smooth ? half[(i + 1) & 1] : nullptr, field);
  return check_launch(E);
}

extern "C" int rti_relight_field(const float* coef, int basis, int coef_layout, int C, int64_t coef_channel_stride,
                                 int H, int W, const float* light, int light_form, int T, void* out, int out_dtype,
                                 rti_stream_t stream) {
  const char* const E = "rti_relight_field";
  if (int st = check_pointers(E, {coef, light, out})) return st;
  if (int st = check_maps(E, basis, coef_layout, C, coef_channel_stride, H, W)) return st;
  if (light_form != RTI_LIGHT_TILES && light_form != RTI_LIGHT_PIXELS)
    return fail(RTI_ERR_BAD_ARG, "%s: light form %d", E, light_form);
  if (light_form == RTI_LIGHT_TILES)
    if (int st = check_tile(E, T)) return st;
  if (int st = check_out_dtype(E, out_dtype)) return st;
  if (!aligned_to(light, 4)) return fail(RTI_ERR_BAD_ARG, "%s: light must be 4-byte aligned", E);
  const int k = basis_terms(basis);
  const int64_t P = (int64_t)H * W, cs = coef_channel_stride ? coef_channel_stride : P * k;
  const int tiled = light_form == RTI_LIGHT_TILES;
  const FieldArgs fa{light, light_form, tiled ? (H + T - 1) / T : 0, tiled ? (W + T - 1) / T : 0, tiled ? T : 0, W};
  const int vin = maps_staged(coef, coef_layout, C, cs), vout = rows_as_dwords(out, out_dtype, P);
  note_launches(1);
  with_terms(k, [&](auto kt) {
    with_channels(C, [&](auto ct) {
      with_layout(coef_layout, [&](auto l) {
        with_out(out_dtype, [&](auto t) {
          using TO = decltype(t);
          hipLaunchKernelGGL((relight_field_k<decltype(kt)::value, decltype(ct)::value, decltype(l)::value, TO>),
                             dim3(grid_1d(P, CHUNK)), dim3(256), 0, (hipStream_t)stream, coef, cs, P, vin, vout, fa,
                             static_cast<TO*>(out));
        });
      });
    });
  });
  return check_launch(E);
}
