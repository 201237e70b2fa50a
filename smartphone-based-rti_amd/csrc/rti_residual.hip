// rti_residual.hip -- per-pixel fit residuals of the shared-direction fit on gfx950.
//
// The reference never reports how well _interpolate_PTM's least-squares solution
// (analysis.py:280-298) explains a pixel's N samples; the north_star asks for the
// per-pixel residual next to the coefficients.  For a shared light set the design
// matrix A[N][k] is the same for every pixel, so
//     ss[c][p]  = Σ_n (I[c][n][p] − Σ_i A[n][i] · coef[c][p][i])²
//     res[c][p] = sqrt(ss / N)                       (RMS residual, intensity units)
//     partial[c][b] = Σ_{p in workgroup b} ss[c][p]  (fp64, one per workgroup)
// The single-pass identity ‖I‖² − cᵀAᵀA c cancels catastrophically in fp32 (‖I‖² ≈ 4e6
// against residual energies of a few hundred at N=100), so this is a second stream
// over the intensity stack, HBM-bound like the fit: 4 + 4(k+1)/N bytes per pixel·light.
//
// One lane owns VEC adjacent pixels: their k coefficients are loaded once, then every
// light plane is one 16-B load; A's row n is wave-uniform (scalar loads into SGPRs).
// The per-workgroup sum is a wavefront reduction (DPP/shuffle, fp64) plus one LDS
// exchange between the 4 waves, written by lane 0 with a plain vector store: no atomics,
// so the partial sums are deterministic.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rti_lsq.h"
#include "rti_stack.h"

namespace rti {
namespace {

constexpr int RES_THREADS = 256;

// Wide lanes (as the fit): a wave owns NC·64·VEC consecutive pixels and
// lane l's chunk j is the VEC pixels at wave_base + j·64·VEC + VEC·l, so the wave's NC loads
// of one light plane cover NC KiB contiguous (VEC = 4, fp32).
template <int K, int VEC, int NC, typename T>
__global__ __launch_bounds__(RES_THREADS) void fit_residual_k(const float* __restrict__ A, int N,
                                                             const T* __restrict__ I, int64_t P,
                                                             int64_t lstride, int64_t cstride,
                                                             const float* __restrict__ coef, int layout,
                                                             int64_t ocstride, float* __restrict__ res,
                                                             double* __restrict__ partial, int64_t pstride) {
  const int c = blockIdx.y;
  const int64_t wave = ((int64_t)blockIdx.x * RES_THREADS + threadIdx.x) >> 6;
  const int64_t base = wave * (NC * 64 * VEC) + (threadIdx.x & 63) * VEC;
  const T* Ic = I + c * cstride;
  const float* cc = coef + c * ocstride;
  double mine = 0.0;
  bool live[NC];
  float a[NC][VEC][K];
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int64_t p0 = base + j * 64 * VEC;
    live[j] = p0 < P;
    if (!live[j]) continue;
    if (layout == RTI_COEF_PIXEL_MAJOR) {
#pragma unroll
      for (int v = 0; v < VEC; ++v)
#pragma unroll
        for (int i = 0; i < K; ++i) a[j][v][i] = cc[(p0 + v) * K + i];
    } else {
#pragma unroll
      for (int i = 0; i < K; ++i) {
        float x[VEC];
        load_nt<float>(cc + i * P + p0, x);
#pragma unroll
        for (int v = 0; v < VEC; ++v) a[j][v][i] = x[v];
      }
    }
  }
  float ss[NC][VEC] = {};
  for (int n = 0; n < N; ++n) {
    float x[NC][VEC];
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (live[j]) load_nt<float>(Ic + n * lstride + base + j * 64 * VEC, x[j]);
    const float* An = A + (int64_t)n * K;  // wave-uniform row
#pragma unroll
    for (int j = 0; j < NC; ++j) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        float pred = 0.f;
#pragma unroll
        for (int i = 0; i < K; ++i) pred = fmaf(An[i], a[j][v][i], pred);
        const float r = x[j][v] - pred;
        ss[j][v] = fmaf(r, r, ss[j][v]);
      }
    }
  }
  const float invN = 1.0f / (float)N;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    if (!live[j]) continue;
    float out[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      out[v] = sqrtf(ss[j][v] * invN);
      mine += (double)ss[j][v];
    }
    float* rc = res + c * P + base + j * 64 * VEC;
    if constexpr (VEC == 4) {
      *reinterpret_cast<float4*>(rc) = make_float4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
      for (int v = 0; v < VEC; ++v) rc[v] = out[v];
    }
  }
  if (partial) {
    __shared__ double wsum[RES_THREADS / 64];
    const double w = wave_sum(mine);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
#pragma unroll
      for (int i = 0; i < RES_THREADS / 64; ++i) t += wsum[i];
      partial[(int64_t)c * pstride + blockIdx.x] = t;
    }
  }
}

struct ResArgs {
  const float* A;
  StackView in;
  CoefSource coef;  // read here
  float* res;
  double* partial;
  hipStream_t s;
};

template <int K, int VEC, int NC, typename T>
int launch_res(const ResArgs& a) {
  const StackView& in = a.in;
  const dim3 grid(grid_1d(in.P, RES_THREADS * VEC * NC), in.C);
  hipLaunchKernelGGL((fit_residual_k<K, VEC, NC, T>), grid, dim3(RES_THREADS), 0, a.s, a.A, in.N,
                     static_cast<const T*>(in.I), in.P, in.lstride, in.cstride, a.coef.coef, a.coef.layout, a.coef.ocstride,
                     a.res, a.partial, (int64_t)grid_1d(in.P, RES_THREADS));
  return check_launch("rti_fit_residual");
}

// Chunks per lane, measured at 4K x 100 (profiles/r01_residual_c3_nc_sweep.log): PTM-6
// NC = 1 / 2 / 4 / 8 -> 0.522 / 0.520 / 0.505 / 0.578 ms (8 chunks = 256 VGPRs, 1 wave/SIMD,
// cannot hide the coefficient loads).  HSH-9/16 keep one chunk (wide lanes not measured).
// The wide form needs enough waves to cover the chip (1024 SIMDs, 2 waves each at 4 chunks);
// the cutoff is the fit's heuristic (rti_fit.hip AUTO: >= 2000 waves), not a residual sweep.
constexpr int64_t kResWideMinWaves = 2000;

template <int K, typename T>
int launch_res_v(const ResArgs& a, bool vec4) {
  if (!vec4) return launch_res<K, 1, 1, T>(a);
  if constexpr (K == 6) {
    constexpr int NC = 4;
    if (a.in.P * a.in.C / (64 * 4 * NC) >= kResWideMinWaves) return launch_res<K, 4, NC, T>(a);
  }
  return launch_res<K, 4, 1, T>(a);
}

template <typename T>
int launch_res_k(const ResArgs& a, bool vec4) {
  switch (a.coef.k) {
    case 6: return launch_res_v<6, T>(a, vec4);
    case 9: return launch_res_v<9, T>(a, vec4);
    case 16: return launch_res_v<16, T>(a, vec4);
    default: return fail(RTI_ERR_UNSUPPORTED, "rti_fit_residual: k=%d (supported: 6, 9, 16)", a.coef.k);
  }
}

}  // namespace
}  // namespace rti

using namespace rti;

extern "C" int64_t rti_fit_residual_blocks(int64_t P) {
  if (P <= 0) return 0;
  // per-channel stride of `partial`: the VEC = 1 grid, so it bounds either launch; entries
  // past the launched grid are not written (the caller zeroes the buffer)
  return (int64_t)grid_1d(P, RES_THREADS);
}

extern "C" int rti_fit_residual(const float* A, int k, int N, const void* I, int in_dtype, int64_t P, int C,
                                int64_t light_stride, int64_t channel_stride, const float* coef, int coef_layout,
                                int64_t coef_channel_stride, float* res, double* partial, rti_stream_t stream) {
  const char* const E = "rti_fit_residual";
  if (int st = check_pointers(E, {A, I, coef, res})) return st;
  if (int st = check_extents(E, "N/P/C", N, P, C)) return st;
  if (int st = check_lights(E, N, k)) return st;
  if (int st = check_in_dtype(E, in_dtype)) return st;
  if (int st = check_coef_layout(E, coef_layout)) return st;
  const ResArgs a{A, stack_view(I, in_dtype, N, P, C, light_stride, channel_stride),
                  coef_view(coef, coef_layout, k, P, coef_channel_stride), res, partial,
                  (hipStream_t)stream};
  if (int st = check_stack_strides(E, a.in)) return st;
  if (int st = check_coef_stride(E, a.coef, P, C)) return st;
  const bool vec4 = stack_vec_ok_any_c(a.in, 4) && aligned_to(res, 16) && coef_vec_ok_any_c(a.coef);
  return with_in_dtype(in_dtype, [&](auto t) { return launch_res_k<decltype(t)>(a, vec4); });
}
