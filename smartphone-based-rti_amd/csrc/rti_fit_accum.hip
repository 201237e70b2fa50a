// rti_fit_accum.hip -- the shared-direction fit fed in chunks of light planes (gfx950).
//
// rti_fit_shared_residual (rti_fitres.hip) keeps, per pixel, y = Rᵀ I (k fp64 sums; R = the design rows A, or
// the orthonormal U of its thin SVD) and q = ‖I‖², and forms coefficients and the residual only at its very
// end.  Light n's contribution to y and q depends on light n alone, so here that state lives in HBM between
// calls:
//
//     rti_fit_accumulate    state[c][j][p] (+)= Σ_{n in chunk} R[n][j]·I[c][n][p]   (j < k),
//                           state[c][k][p] (+)= Σ_{n in chunk} I[c][n][p]²
//     rti_fit_accum_solve   coef = M·y,  ss = q − coefᵀy (or q − yᵀy),  res = sqrt(ss / n_lights)
//
// for stacks that do not fit in HBM beside their outputs and for frames that arrive over time (a preview fit
// after any chunk).  Every (pixel, j) sum is one chain of explicit fma calls in light order, so the state
// after N lights has the same bits however the N lights were split into chunks.
//
// Both kernels are streams.  Accumulate moves B·sizeof(element) + 8(k+1) (read, not with init) + 8(k+1)
// (write) bytes per pixel, solve 8(k+1) in and 4k + 4 out.  Lane map as fit_shared_residual_k: a wave owns
// consecutive pixels, a lane VEC of them; on the vector path a light plane is one 16-byte (fp32 / int32)
// non-temporal load per lane and a state plane two; R's row and M are wave-uniform (scalar loads).  The state
// is 2(k+1) VGPRs per pixel: 56 / 80 / 136 per lane at k = 6 / 9 / 16 with four pixels per lane, which leaves
// 8 / 4 / 2 light planes in flight per lane without spilling.  The fp64 planes are 16-byte aligned only when
// P is even and the base is; anything else takes one pixel per lane.  A lane past the image does nothing:
// neither kernel has a wave-wide step that needs it, so there is no stand-in pixel whose state could be hurt.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rti_lsq.h"
#include "rti_stack.h"

namespace rti {
namespace {

typedef double doublex2 __attribute__((ext_vector_type(2)));
constexpr int FA_THREADS = 256;

// VEC consecutive doubles of a state plane (VEC even: 16-byte loads / stores)
template <int VEC>
__device__ __forceinline__ void load_state(const double* __restrict__ p, double (&y)[VEC]) {
  if constexpr (VEC == 1) {
    y[0] = *p;
  } else {
#pragma unroll
    for (int i = 0; i < VEC; i += 2) {
      const doublex2 v = *reinterpret_cast<const doublex2*>(p + i);
      y[i] = v[0];
      y[i + 1] = v[1];
    }
  }
}

template <int VEC>
__device__ __forceinline__ void store_state(double* __restrict__ p, const double (&y)[VEC]) {
  if constexpr (VEC == 1) {
    *p = y[0];
  } else {
#pragma unroll
    for (int i = 0; i < VEC; i += 2) *reinterpret_cast<doublex2*>(p + i) = doublex2{y[i], y[i + 1]};
  }
}

// one light plane into a lane's state: x = (double)I, y_j = fma(R[n][j], x, y_j), q = fma(x, x, q)
template <int K, int VEC, typename T>
__device__ __forceinline__ void add_plane(const double* __restrict__ Rn, const T (&x)[VEC], double (&y)[K + 1][VEC]) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const double xd = (double)x[v];
#pragma unroll
    for (int j = 0; j < K; ++j) y[j][v] = fma(Rn[j], xd, y[j][v]);
    y[K][v] = fma(xd, xd, y[K][v]);
  }
}

template <int K, int VEC, int U, typename T, bool INIT>
__global__ void __launch_bounds__(FA_THREADS)
fit_accumulate_k(const double* __restrict__ R, int B, const T* __restrict__ I, int64_t P, int64_t lstride, int64_t cstride,
                 double* __restrict__ state, int64_t scstride) {
  const int64_t p0 = ((int64_t)blockIdx.x * FA_THREADS + threadIdx.x) * VEC;
  if (p0 >= P) return;  // VEC > 1 only with P % VEC == 0: a lane's pixels are all inside or all outside
  const T* __restrict__ src = I + (int64_t)blockIdx.y * cstride + p0;
  double* __restrict__ st = state + (int64_t)blockIdx.y * scstride + p0;
  double y[K + 1][VEC];
#pragma unroll
  for (int j = 0; j <= K; ++j) {
    if constexpr (INIT) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) y[j][v] = 0.0;
    } else {
      load_state<VEC>(st + (int64_t)j * P, y[j]);
    }
  }
  int n = 0;
  for (; n + U <= B; n += U) {  // U plane loads in flight per lane
    T x[U][VEC];
#pragma unroll
    for (int u = 0; u < U; ++u) load_nt<T>(src + (int64_t)(n + u) * lstride, x[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) add_plane<K, VEC, T>(R + (int64_t)(n + u) * K, x[u], y);  // wave-uniform row -> SGPRs
  }
  for (; n < B; ++n) {  // the last B % U planes; the whole chunk for a live frame (B = 1)
    T x[VEC];
    load_nt<T>(src + (int64_t)n * lstride, x);
    add_plane<K, VEC, T>(R + (int64_t)n * K, x, y);
  }
#pragma unroll
  for (int j = 0; j <= K; ++j) store_state<VEC>(st + (int64_t)j * P, y[j]);
}

// pixel-major coefficient rows leave through LDS as whole 1 KiB rows per store instruction (as fitres_body)
template <int K, int VEC, int LAYOUT>
constexpr bool fa_stage() { return LAYOUT == RTI_COEF_PIXEL_MAJOR && VEC == 4 && K <= 9; }

template <int K, int VEC, int LAYOUT>
__global__ void __launch_bounds__(FA_THREADS)
fit_accum_solve_k(const double* __restrict__ M, int orth, int64_t n_lights, const double* __restrict__ state, int64_t P,
                  int64_t scstride, float* __restrict__ coef, int64_t ocstride, float* __restrict__ res) {
  constexpr int F = VEC * K;
  __shared__ __attribute__((aligned(16))) float lds[fa_stage<K, VEC, LAYOUT>() ? FA_THREADS * F : 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wave_base = ((int64_t)blockIdx.x * (FA_THREADS / 64) + wave) * (64 * VEC);
  const int64_t p0 = wave_base + (int64_t)lane * VEC;
  const bool full = wave_base + 64 * VEC <= P;  // wave-uniform
  if (p0 >= P) return;                          // never in a full wave
  const double* __restrict__ st = state + (int64_t)blockIdx.y * scstride + p0;
  float* __restrict__ dst = coef + (int64_t)blockIdx.y * ocstride;
  double y[K + 1][VEC];
#pragma unroll
  for (int j = 0; j <= K; ++j) load_state<VEC>(st + (int64_t)j * P, y[j]);

  // the tail of fitres_body (rti_fitres.hip), restated: c_i = Σ_l M[i][l]·y_l, ss = q − Σ_i (orth ? y_i : c_i)·y_i;
  // tests/test_gpu_accum.py::test_same_bits_as_one_pass_fit holds the two copies to the same bits
  const double invN = 1.0 / (double)n_lights;
  float o[F], r[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    double s = y[K][v];
#pragma unroll
    for (int i = 0; i < K; ++i) {
      double ci = 0.0;
#pragma unroll
      for (int l = 0; l < K; ++l) ci = fma(M[i * K + l], y[l][v], ci);
      s = fma(orth ? -y[i][v] : -ci, y[i][v], s);
      o[v * K + i] = (float)ci;
    }
    s = s < 0.0 ? 0.0 : s;  // rounding can leave an exact fit a few ulps below zero; NaN passes
    r[v] = (float)sqrt(s * invN);
  }
  if (res) {
    float* __restrict__ rc = res + (int64_t)blockIdx.y * P + p0;
    if constexpr (VEC == 4)
      *reinterpret_cast<floatx4*>(rc) = floatx4{r[0], r[1], r[2], r[3]};
    else if constexpr (VEC == 2)
      *reinterpret_cast<floatx2*>(rc) = floatx2{r[0], r[1]};
    else
      rc[0] = r[0];
  }
  if constexpr (LAYOUT == RTI_COEF_PLANAR) {
#pragma unroll
    for (int i = 0; i < K; ++i) {
      float* __restrict__ d = dst + (int64_t)i * P + p0;
      if constexpr (VEC == 4)
        *reinterpret_cast<floatx4*>(d) = floatx4{o[i], o[K + i], o[2 * K + i], o[3 * K + i]};
      else if constexpr (VEC == 2)
        *reinterpret_cast<floatx2*>(d) = floatx2{o[i], o[K + i]};
      else
        d[0] = o[i];
    }
  } else {
    if constexpr (fa_stage<K, VEC, LAYOUT>()) {
      if (full) {  // the whole wave is here: its 64·VEC rows are 64·F contiguous floats
        float* lds_wave = lds + wave * 64 * F;
#pragma unroll
        for (int i = 0; i < F; i += 4)
          *reinterpret_cast<floatx4*>(lds_wave + lane * F + i) = floatx4{o[i], o[i + 1], o[i + 2], o[i + 3]};
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float* wdst = dst + wave_base * K;
#pragma unroll
        for (int j = 0; j < F / 4; ++j)
          *reinterpret_cast<floatx4*>(wdst + j * 256 + lane * 4) =
              *reinterpret_cast<const floatx4*>(lds_wave + j * 256 + lane * 4);
        return;
      }
    }
    float* __restrict__ d = dst + p0 * K;
    if constexpr (F % 4 == 0 && VEC > 1) {  // F contiguous floats per lane, 16-byte aligned (p0 % VEC == 0)
#pragma unroll
      for (int i = 0; i < F; i += 4) *reinterpret_cast<floatx4*>(d + i) = floatx4{o[i], o[i + 1], o[i + 2], o[i + 3]};
    } else {
#pragma unroll
      for (int i = 0; i < F; ++i) d[i] = o[i];
    }
  }
}

struct AccArgs {
  const double* R;
  StackView in;  // the chunk: N = its B planes
  double* state;
  int64_t scstride;
  bool init;
  hipStream_t s;
};

template <int K, int VEC, int U, typename T>
int launch_acc_t(const AccArgs& a) {
  const StackView& in = a.in;
  const dim3 grid(grid_1d(in.P, FA_THREADS * VEC), in.C);
  if (a.init)
    hipLaunchKernelGGL((fit_accumulate_k<K, VEC, U, T, true>), grid, dim3(FA_THREADS), 0, a.s, a.R, in.N,
                       static_cast<const T*>(in.I), in.P, in.lstride, in.cstride, a.state, a.scstride);
  else
    hipLaunchKernelGGL((fit_accumulate_k<K, VEC, U, T, false>), grid, dim3(FA_THREADS), 0, a.s, a.R, in.N,
                       static_cast<const T*>(in.I), in.P, in.lstride, in.cstride, a.state, a.scstride);
  return check_launch("rti_fit_accumulate");
}

template <int K, typename T>
int launch_acc_v(const AccArgs& a, bool vec4) {
  // plane loads in flight per lane, beside 2(k+1) state VGPRs per pixel (resource usage: DESIGN.md §4.1h)
  constexpr int U = K <= 6 ? 8 : K <= 9 ? 4 : 2;
  return vec4 ? launch_acc_t<K, 4, U, T>(a) : launch_acc_t<K, 1, 8, T>(a);
}

template <typename T>
int launch_acc_k(int k, const AccArgs& a, bool vec4) {
  switch (k) {
    case 6: return launch_acc_v<6, T>(a, vec4);
    case 9: return launch_acc_v<9, T>(a, vec4);
    default: return launch_acc_v<16, T>(a, vec4);
  }
}

struct SolveArgs {
  const double* M;
  int orth;
  int64_t n_lights;
  const double* state;
  int64_t P, scstride;
  int C;
  CoefView out;
  float* res;
  hipStream_t s;
};

template <int K, int VEC, int LAYOUT>
int launch_solve_t(const SolveArgs& a) {
  const dim3 grid(grid_1d(a.P, FA_THREADS * VEC), a.C);
  hipLaunchKernelGGL((fit_accum_solve_k<K, VEC, LAYOUT>), grid, dim3(FA_THREADS), 0, a.s, a.M, a.orth, a.n_lights, a.state,
                     a.P, a.scstride, a.out.coef, a.out.ocstride, a.res);
  return check_launch("rti_fit_accum_solve");
}

template <int K, int LAYOUT>
int launch_solve_v(const SolveArgs& a, int vec) {
  // pixels per lane: 4 for PTM-6 / HSH-9 (56 / 80 state VGPRs), 2 for HSH-16 (68, and 32 coefficients)
  if (vec == 1) return launch_solve_t<K, 1, LAYOUT>(a);
  return launch_solve_t<K, (K <= 9 ? 4 : 2), LAYOUT>(a);
}

template <int LAYOUT>
int launch_solve_k(int k, const SolveArgs& a, int vec) {
  switch (k) {
    case 6: return launch_solve_v<6, LAYOUT>(a, vec);
    case 9: return launch_solve_v<9, LAYOUT>(a, vec);
    default: return launch_solve_v<16, LAYOUT>(a, vec);
  }
}

bool accum_k_ok(int k) { return k == 6 || k == 9 || k == 16; }

}  // namespace
}  // namespace rti

using namespace rti;

extern "C" int64_t rti_fit_accum_state_doubles(int k, int64_t P, int C) {
  if (!accum_k_ok(k) || P < 1 || C < 1 || C > 65535) return -1;
  return (int64_t)C * (k + 1) * P;
}

extern "C" int rti_fit_accumulate(const double* R, int k, int B, const void* I, int in_dtype, int64_t P, int C,
                                  int64_t light_stride, int64_t channel_stride, double* state,
                                  int64_t state_channel_stride, int init, rti_stream_t stream) {
  const char* const E = "rti_fit_accumulate";
  if (int st = check_pointers(E, {R, I, state})) return st;
  if (int st = check_extents(E, "B/P/C", B, P, C)) return st;
  if (!accum_k_ok(k)) return fail(RTI_ERR_UNSUPPORTED, "%s: k=%d (supported: 6, 9, 16)", E, k);
  if (int st = check_in_dtype(E, in_dtype)) return st;
  const int64_t scstride = state_channel_stride ? state_channel_stride : (int64_t)(k + 1) * P;
  const AccArgs a{R, stack_view(I, in_dtype, B, P, C, light_stride, channel_stride), state, scstride, init != 0,
                  (hipStream_t)stream};
  if (int st = check_stack_strides(E, a.in)) return st;
  if (C > 1 && scstride < (int64_t)(k + 1) * P) return fail(RTI_ERR_BAD_ARG, "%s: state_channel_stride", E);
  const bool vec4 = stack_vec_ok_used(a.in, 4) && aligned_to(state, 16) && (C == 1 || scstride % 2 == 0);
  return with_in_dtype(in_dtype, [&](auto t) { return launch_acc_k<decltype(t)>(k, a, vec4); });
}

extern "C" int rti_fit_accum_solve(const double* M, int k, int orth, int64_t n_lights, const double* state, int64_t P,
                                   int C, int64_t state_channel_stride, float* coef, int coef_layout,
                                   int64_t coef_channel_stride, float* res, rti_stream_t stream) {
  const char* const E = "rti_fit_accum_solve";
  if (int st = check_pointers(E, {M, state, coef})) return st;
  if (int st = check_extents(E, "n_lights/P/C", n_lights, P, C)) return st;
  if (!accum_k_ok(k)) return fail(RTI_ERR_UNSUPPORTED, "%s: k=%d (supported: 6, 9, 16)", E, k);
  if (int st = check_coef_layout(E, coef_layout)) return st;
  const int64_t scstride = state_channel_stride ? state_channel_stride : (int64_t)(k + 1) * P;
  const SolveArgs a{M, orth ? 1 : 0, n_lights, state, P, scstride, C, coef_view(coef, coef_layout, k, P, coef_channel_stride),
                    res, (hipStream_t)stream};
  if (C > 1 && scstride < (int64_t)(k + 1) * P) return fail(RTI_ERR_BAD_ARG, "%s: state_channel_stride", E);
  if (int st = check_coef_stride(E, a.out, P, C)) return st;
  const bool vec = P % 4 == 0 && aligned_to(state, 16) && (C == 1 || scstride % 2 == 0) && coef_vec_ok_used(a.out, C) &&
                   (!res || aligned_to(res, 16));
  return coef_layout == RTI_COEF_PLANAR ? launch_solve_k<RTI_COEF_PLANAR>(k, a, vec ? 4 : 1)
                                        : launch_solve_k<RTI_COEF_PIXEL_MAJOR>(k, a, vec ? 4 : 1);
}
