// rti_height.hip -- surface height from a normal map (gfx950): masked Poisson integration by preconditioned
// conjugate gradients.  The project's first global solve.
//
//     rti_height_levels            host: grids of the aggregation hierarchy
//     rti_height_workspace_bytes   host: device scratch of a solve
//     rti_height_from_normals      normal map -> height [H][W] (+ valid, stats)
//
// The semantics are build-defined and stated in include/rti.h and DESIGN.md §4.19: the least-squares surface over
// the graph of valid pixels, A z = b with A that graph's Laplacian, gauged to zero mean.
//
// Every grid of the hierarchy is three int32 arrays: wR[i] the weight of the edge to the right neighbour, wD[i] to
// the one below, deg[i] the sum of the four.  On the pixel grid the weights are 0 / 1; a coarse edge carries the sum
// of the fine weights crossing between its two 2×2 aggregates (the Galerkin operator of piecewise-constant
// aggregation), so one integer kernel builds each level.  A cell of degree 0 (an invalid pixel, an empty aggregate,
// an aggregate that swallowed a whole component) has no row: every vector is 0 there and stays 0, so the kernels
// run over the dense grid, the dot products need no mask, and an edge of weight 0 is never loaded across.
//
// All stencil kernels index a grid linearly (i ± 1, i ± W) and take their neighbours from L1 / L2: a row of doubles
// at 4K is 30 KiB, so the rows above and below a workgroup's run are resident.  An LDS tile with a halo is not
// built.  Reductions are two-stage and fixed-order: a workgroup owns a contiguous run of `chunk`
// cells, its threads sum their cells in ascending order, an LDS tree joins them and the partial goes to slot
// blockIdx.x; reduce_k, one workgroup, sums the slots (thread t the slots t, t + 256, ... in order, then the same
// tree) and forms the PCG scalar that depends on it in device memory, where the next kernel reads it.  No atomics,
// no kernel waits on another workgroup.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rti_dispatch.h"
#include "rti_stack.h"

namespace rti {
namespace {

constexpr int THREADS = 256;
constexpr int MAX_PARTIALS = 8192;
constexpr int MAX_LEVELS = 32;
constexpr double OMEGA = 0.8;      // weighted Jacobi
constexpr double OVER = 2.0;       // over-correction of the piecewise-constant prolongation
constexpr int COARSEST_SWEEPS = 8;
constexpr int COARSEST_MAX = 4;    // levels stop when max(H_l, W_l) <= 4

// device scalars (doubles) at the head of the workspace
enum { S_BB, S_RR, S_RHO, S_PQ, S_ALPHA, S_BETA, S_NVALID, S_TRUE_RR, S_ZSUM, S_MET, S_COUNT = 32 };

// what reduce_k does with the sum(s)
enum { RED_SETUP, RED_RR0, RED_PQ, RED_RR, RED_RHO_FIRST, RED_RHO, RED_TRUE, RED_ZSUM };

struct Grid {
  int h, w;
  int64_t n;
  int *wR, *wD, *deg;
  double *f, *xa, *xb;  // V-cycle right-hand side, result, scratch
};

inline int levels_of(int H, int W) {
  int L = 1;
  while ((H > W ? H : W) > COARSEST_MAX) {
    H = (H + 1) / 2;
    W = (W + 1) / 2;
    ++L;
  }
  return L;
}

inline bool dims_ok(int H, int W) { return H >= 1 && W >= 1 && (int64_t)H * W < ((int64_t)1 << 31); }

// cells a workgroup owns in the reductions: a multiple of 256, at most MAX_PARTIALS workgroups
inline int64_t chunk_of(int64_t P) {
  int64_t c = (P + MAX_PARTIALS - 1) / MAX_PARTIALS;
  c = (c + THREADS - 1) / THREADS * THREADS;
  return c < 2048 ? 2048 : c;
}
inline int blocks_of(int64_t P) { return (int)((P + chunk_of(P) - 1) / chunk_of(P)); }

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// Σ_{l>=1} n_l <= P + levels (n_{l+1} = ⌈h/2⌉⌈w/2⌉ <= ⌈n_l/2⌉), so the coarse arrays are sized from P alone and
// the workspace is monotone in H·W whatever the aspect
inline int64_t coarse_cells(int64_t P) { return P + MAX_LEVELS; }

struct Layout {
  size_t scalars, part0, part1, vec[6], w0[3], cw[3], cf[3], total;
};
inline Layout layout_of(int64_t P, int precond) {
  Layout o;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at += up256(bytes);
    return here;
  };
  o.scalars = take(S_COUNT * sizeof(double));
  o.part0 = take(MAX_PARTIALS * sizeof(double));
  o.part1 = take(MAX_PARTIALS * sizeof(double));
  for (int i = 0; i < 6; ++i) o.vec[i] = take((size_t)P * sizeof(double));
  for (int i = 0; i < 3; ++i) o.w0[i] = take((size_t)P * sizeof(int));
  for (int i = 0; i < 3; ++i) o.cw[i] = o.cf[i] = 0;
  if (precond == RTI_HEIGHT_MULTIGRID) {
    for (int i = 0; i < 3; ++i) o.cw[i] = take((size_t)coarse_cells(P) * sizeof(int));
    for (int i = 0; i < 3; ++i) o.cf[i] = take((size_t)coarse_cells(P) * sizeof(double));
  }
  o.total = at;
  return o;
}

// ---- device helpers ----------------------------------------------------------------------------------------------

// the sum of v over the workgroup in a fixed tree, valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* sh) {
  const int t = threadIdx.x;
  __syncthreads();  // sh may still be read from the previous sum
  sh[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (t < s) sh[t] += sh[t + s];
    __syncthreads();
  }
  return sh[0];
}

// (A x)_i on a grid of n cells, width w: deg·x_i − Σ weight·x_j in the order left, right, up, down
__device__ __forceinline__ double lap_at(const int* __restrict__ wR, const int* __restrict__ wD,
                                         const int* __restrict__ deg, const double* __restrict__ x, int64_t i,
                                         int64_t n, int w) {
  double acc = (double)deg[i] * x[i];
  if (i > 0) {
    const int e = wR[i - 1];
    if (e) acc -= (double)e * x[i - 1];
  }
  {
    const int e = wR[i];
    if (e) acc -= (double)e * x[i + 1];  // wR is 0 in the last column: i + 1 < n here
  }
  if (i >= w) {
    const int e = wD[i - w];
    if (e) acc -= (double)e * x[i - w];
  }
  {
    const int e = wD[i];
    if (e) acc -= (double)e * x[i + w];  // wD is 0 in the last row
  }
  return acc;
}

__device__ __forceinline__ double inv_deg(int d) { return d > 0 ? 1.0 / (double)d : 0.0; }

template <int NL>
__device__ __forceinline__ void load_normal(const float* __restrict__ nrm, int64_t i, int64_t P, float& nx, float& ny,
                                            float& nz) {
  if constexpr (NL == RTI_NORMAL_PLANAR) {
    nx = nrm[i];
    ny = nrm[P + i];
    nz = nrm[2 * P + i];
  } else {
    nx = nrm[3 * i];
    ny = nrm[3 * i + 1];
    nz = nrm[3 * i + 2];
  }
}

// a pixel's raw validity and its gradients p = −n_x/n_z, q = ∓n_y/n_z (fp64, each quotient rounded once)
template <int NL>
__device__ __forceinline__ bool gradient_at(const float* __restrict__ nrm, int64_t i, int64_t P, double nz_min,
                                            int flip_y, double& p, double& q) {
  float nx, ny, nz;
  load_normal<NL>(nrm, i, P, nx, ny, nz);
  const bool ok = isfinite(nx) && isfinite(ny) && isfinite(nz) && (double)nz >= nz_min;
  p = q = 0.0;
  if (ok) {
    const double px = (double)nx / (double)nz, qy = (double)ny / (double)nz;
    p = -px;
    q = flip_y ? qy : -qy;
  }
  return ok;
}

// ---- set-up: mask, gradients, b, degree, weights and the start in one pass over the normals --------------------

template <int NL>
__global__ void __launch_bounds__(THREADS)
height_setup_k(const float* __restrict__ nrm, int H, int W, double nz_min, int flip_y, const float* __restrict__ z0,
               int64_t chunk, int* __restrict__ wR, int* __restrict__ wD, int* __restrict__ deg,
               double* __restrict__ b, double* __restrict__ z, double* __restrict__ part_bb,
               double* __restrict__ part_nv) {
#pragma clang fp contract(off)
  __shared__ double sh[THREADS];
  const int64_t P = (int64_t)H * W;
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < P ? lo + chunk : P;
  double bb = 0.0, nv = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) {
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    double p, q, pj, qj;
    int eR = 0, eD = 0, d = 0;
    double bi = 0.0;
    if (gradient_at<NL>(nrm, i, P, nz_min, flip_y, p, q)) {
      // −g_ij with the edge oriented from i: the left and upper neighbours add, the right and lower subtract
      if (x > 0 && gradient_at<NL>(nrm, i - 1, P, nz_min, flip_y, pj, qj)) {
        bi += 0.5 * (p + pj);
        ++d;
      }
      if (x + 1 < W && gradient_at<NL>(nrm, i + 1, P, nz_min, flip_y, pj, qj)) {
        bi -= 0.5 * (p + pj);
        eR = 1;
        ++d;
      }
      if (y > 0 && gradient_at<NL>(nrm, i - W, P, nz_min, flip_y, pj, qj)) {
        bi += 0.5 * (q + qj);
        ++d;
      }
      if (y + 1 < H && gradient_at<NL>(nrm, i + W, P, nz_min, flip_y, pj, qj)) {
        bi -= 0.5 * (q + qj);
        eD = 1;
        ++d;
      }
    }
    wR[i] = eR;
    wD[i] = eD;
    deg[i] = d;
    b[i] = bi;
    z[i] = (d > 0 && z0) ? (double)z0[i] : 0.0;
    bb += bi * bi;
    nv += d > 0 ? 1.0 : 0.0;
  }
  const double sbb = block_sum(bb, sh);
  const double snv = block_sum(nv, sh);
  if (threadIdx.x == 0) {
    part_bb[blockIdx.x] = sbb;
    part_nv[blockIdx.x] = snv;
  }
}

// ---- the PCG vector kernels -------------------------------------------------------------------------------------

// r = b − A z (WRITE) and the partials of ‖b − A z‖²
template <bool WRITE>
__global__ void __launch_bounds__(THREADS)
height_residual_k(const int* __restrict__ wR, const int* __restrict__ wD, const int* __restrict__ deg,
                  const double* __restrict__ b, const double* __restrict__ z, int64_t n, int w, int64_t chunk,
                  double* __restrict__ r, double* __restrict__ part) {
  __shared__ double sh[THREADS];
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) {
    const double v = deg[i] > 0 ? b[i] - lap_at(wR, wD, deg, z, i, n, w) : 0.0;
    if constexpr (WRITE) r[i] = v;
    acc += v * v;
  }
  const double s = block_sum(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// q = A p and the partials of p·q
__global__ void __launch_bounds__(THREADS)
height_apply_k(const int* __restrict__ wR, const int* __restrict__ wD, const int* __restrict__ deg,
               const double* __restrict__ p, int64_t n, int w, int64_t chunk, double* __restrict__ q,
               double* __restrict__ part) {
  __shared__ double sh[THREADS];
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) {
    const double v = deg[i] > 0 ? lap_at(wR, wD, deg, p, i, n, w) : 0.0;
    q[i] = v;
    acc += p[i] * v;
  }
  const double s = block_sum(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// z += α p, r −= α q and the partials of r·r; α from device memory
__global__ void __launch_bounds__(THREADS)
height_update_k(const double* __restrict__ sc, const double* __restrict__ p, const double* __restrict__ q, int64_t n,
                int64_t chunk, double* __restrict__ z, double* __restrict__ r, double* __restrict__ part) {
  __shared__ double sh[THREADS];
  const double alpha = sc[S_ALPHA];
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) {
    z[i] += alpha * p[i];
    const double v = r[i] - alpha * q[i];
    r[i] = v;
    acc += v * v;
  }
  const double s = block_sum(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// the Jacobi preconditioner s = r/deg with the partials of r·s (JACOBI), or those partials alone of a given s
template <bool JACOBI>
__global__ void __launch_bounds__(THREADS)
height_dot_k(const int* __restrict__ deg, const double* __restrict__ r, int64_t n, int64_t chunk,
             double* __restrict__ s, double* __restrict__ part) {
  __shared__ double sh[THREADS];
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) {
    double v;
    if constexpr (JACOBI) {
      v = r[i] * inv_deg(deg[i]);
      s[i] = v;
    } else {
      v = s[i];
    }
    acc += r[i] * v;
  }
  const double t = block_sum(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// p = s (first) or p = s + β p; β from device memory
__global__ void __launch_bounds__(THREADS)
height_direction_k(const double* __restrict__ sc, const double* __restrict__ s, int64_t n, int first,
                   double* __restrict__ p) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  p[i] = first ? s[i] : s[i] + sc[S_BETA] * p[i];
}

// the second stage of every reduction and the scalar that follows from it
__global__ void __launch_bounds__(THREADS)
height_reduce_k(const double* __restrict__ part0, const double* __restrict__ part1, int nparts, int mode, double rtol,
                int iter, double* __restrict__ sc) {
  __shared__ double sh[THREADS];
  double a = 0.0, c = 0.0;
  for (int j = threadIdx.x; j < nparts; j += THREADS) {
    a += part0[j];
    if (mode == RED_SETUP) c += part1[j];
  }
  const double sum = block_sum(a, sh);
  const double sum1 = mode == RED_SETUP ? block_sum(c, sh) : 0.0;
  if (threadIdx.x != 0) return;
  switch (mode) {
    case RED_SETUP:
      sc[S_BB] = sum;
      sc[S_NVALID] = sum1;
      sc[S_MET] = -1.0;
      sc[S_RR] = sc[S_RHO] = sc[S_PQ] = sc[S_ALPHA] = sc[S_BETA] = sc[S_TRUE_RR] = sc[S_ZSUM] = 0.0;
      break;
    case RED_RR0:
    case RED_RR:
      sc[S_RR] = sum;
      if (sc[S_MET] < 0.0 && sqrt(sum) <= rtol * sqrt(sc[S_BB])) sc[S_MET] = (double)iter;
      break;
    case RED_PQ:
      sc[S_PQ] = sum;
      sc[S_ALPHA] = sum > 0.0 ? sc[S_RHO] / sum : 0.0;  // p = 0 (an exact solution): the step is 0, not 0/0
      break;
    case RED_RHO_FIRST:
      sc[S_RHO] = sum;
      sc[S_BETA] = 0.0;
      break;
    case RED_RHO: {
      const double old = sc[S_RHO];
      sc[S_BETA] = old > 0.0 ? sum / old : 0.0;
      sc[S_RHO] = sum;
      break;
    }
    case RED_TRUE:
      sc[S_TRUE_RR] = sum;
      break;
    case RED_ZSUM:
      sc[S_ZSUM] = sum;
      break;
  }
}

// the partials of Σ z (z is 0 at invalid pixels)
__global__ void __launch_bounds__(THREADS)
height_zsum_k(const double* __restrict__ z, int64_t n, int64_t chunk, double* __restrict__ part) {
  __shared__ double sh[THREADS];
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  double acc = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) acc += z[i];
  const double s = block_sum(acc, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// height = (float)(z − mean) at valid pixels, NaN elsewhere; the mean over the valid pixels
__global__ void __launch_bounds__(THREADS)
height_finish_k(const double* __restrict__ sc, const int* __restrict__ deg, const double* __restrict__ z, int64_t n,
                float* __restrict__ height, uint8_t* __restrict__ valid) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  const double nv = sc[S_NVALID];
  const double mean = nv > 0.0 ? sc[S_ZSUM] / nv : 0.0;
  const bool ok = deg[i] > 0;
  height[i] = ok ? (float)(z[i] - mean) : __builtin_nanf("");
  if (valid) valid[i] = ok ? 1 : 0;
}

// ---- the aggregation hierarchy and its V-cycle -------------------------------------------------------------------

// level l + 1 from level l: a coarse edge sums the fine weights that cross between the two aggregates
__global__ void __launch_bounds__(THREADS)
height_coarsen_k(const int* __restrict__ fR, const int* __restrict__ fD, int fh, int fw, int ch, int cw,
                 int* __restrict__ cR, int* __restrict__ cD, int* __restrict__ cdeg) {
  const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (c >= (int64_t)ch * cw) return;
  const int Y = (int)(c / cw), X = (int)(c - (int64_t)Y * cw);
  const int y0 = 2 * Y, x0 = 2 * X;
  const bool row1 = y0 + 1 < fh, col1 = x0 + 1 < fw;
  const int xr = col1 ? x0 + 1 : x0, yd = row1 ? y0 + 1 : y0;  // the aggregate's last column and row
  int l = 0, r = 0, u = 0, d = 0;
  for (int y = y0; y <= yd; ++y) {
    r += fR[(int64_t)y * fw + xr];
    if (x0 > 0) l += fR[(int64_t)y * fw + x0 - 1];
  }
  for (int x = x0; x <= xr; ++x) {
    d += fD[(int64_t)yd * fw + x];
    if (y0 > 0) u += fD[(int64_t)(y0 - 1) * fw + x];
  }
  cR[c] = r;
  cD[c] = d;
  cdeg[c] = l + r + u + d;
}

// two weighted-Jacobi sweeps from a zero guess: x1 = ω f/deg, x2 = x1 + ω (f − A x1)/deg, x1 formed on the fly
__global__ void __launch_bounds__(THREADS)
height_presmooth_k(const int* __restrict__ wR, const int* __restrict__ wD, const int* __restrict__ deg,
                   const double* __restrict__ f, int64_t n, int w, double* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  const int d = deg[i];
  if (d == 0) {
    x[i] = 0.0;
    return;
  }
  const double id = inv_deg(d);
  const double x1 = OMEGA * f[i] * id;
  double acc = (double)d * x1;
  if (i > 0) {
    const int e = wR[i - 1];
    if (e) acc -= (double)e * (OMEGA * f[i - 1] * inv_deg(deg[i - 1]));
  }
  {
    const int e = wR[i];
    if (e) acc -= (double)e * (OMEGA * f[i + 1] * inv_deg(deg[i + 1]));
  }
  if (i >= w) {
    const int e = wD[i - w];
    if (e) acc -= (double)e * (OMEGA * f[i - w] * inv_deg(deg[i - w]));
  }
  {
    const int e = wD[i];
    if (e) acc -= (double)e * (OMEGA * f[i + w] * inv_deg(deg[i + w]));
  }
  x[i] = x1 + OMEGA * (f[i] - acc) * id;
}

// one weighted-Jacobi sweep xout = xin + ω (f − A xin)/deg
__global__ void __launch_bounds__(THREADS)
height_sweep_k(const int* __restrict__ wR, const int* __restrict__ wD, const int* __restrict__ deg,
               const double* __restrict__ f, const double* __restrict__ xin, int64_t n, int w,
               double* __restrict__ xout) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  const int d = deg[i];
  xout[i] = d > 0 ? xin[i] + OMEGA * (f[i] - lap_at(wR, wD, deg, xin, i, n, w)) * inv_deg(d) : 0.0;
}

// the coarse right-hand side: the residuals f − A x of an aggregate's children (those with a row), summed in the
// order (0,0), (0,1), (1,0), (1,1)
__global__ void __launch_bounds__(THREADS)
height_restrict_k(const int* __restrict__ wR, const int* __restrict__ wD, const int* __restrict__ deg,
                  const double* __restrict__ f, const double* __restrict__ x, int fh, int fw, int ch, int cw,
                  double* __restrict__ fc) {
  const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (c >= (int64_t)ch * cw) return;
  const int Y = (int)(c / cw), X = (int)(c - (int64_t)Y * cw);
  const int64_t n = (int64_t)fh * fw;
  double acc = 0.0;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int y = 2 * Y + dy, xx = 2 * X + dx;
      if (y >= fh || xx >= fw) continue;
      const int64_t i = (int64_t)y * fw + xx;
      if (deg[i] > 0) acc += f[i] - lap_at(wR, wD, deg, x, i, n, fw);
    }
  fc[c] = acc;
}

// x += 2·e[parent] at the cells that have a row
__global__ void __launch_bounds__(THREADS)
height_prolong_k(const int* __restrict__ deg, const double* __restrict__ e, int fh, int fw, int cw,
                 double* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= (int64_t)fh * fw) return;
  if (deg[i] == 0) return;
  const int y = (int)(i / fw), xx = (int)(i - (int64_t)y * fw);
  x[i] += OVER * e[(int64_t)(y >> 1) * cw + (xx >> 1)];
}

// the last grid (at most 4×4 cells, one wave): 8 sweeps from zero in LDS; its operator is singular, so no solve
__global__ void __launch_bounds__(64)
height_coarsest_k(const int* __restrict__ wR, const int* __restrict__ wD, const int* __restrict__ deg,
                  const double* __restrict__ f, int n, int w, double* __restrict__ x) {
  __shared__ double xs[2][COARSEST_MAX * COARSEST_MAX];
  const int i = threadIdx.x;
  const bool on = i < n;
  int d = 0, eL = 0, eR = 0, eU = 0, eD = 0;
  double fi = 0.0;
  if (on) {
    d = deg[i];
    fi = f[i];
    eL = i > 0 ? wR[i - 1] : 0;
    eR = wR[i];
    eU = i >= w ? wD[i - w] : 0;
    eD = wD[i];
    xs[0][i] = 0.0;
  }
  __syncthreads();
  const double id = inv_deg(d);
  for (int s = 0; s < COARSEST_SWEEPS; ++s) {
    const double* cur = xs[s & 1];
    if (on) {
      double acc = (double)d * cur[i];
      if (eL) acc -= (double)eL * cur[i - 1];
      if (eR) acc -= (double)eR * cur[i + 1];
      if (eU) acc -= (double)eU * cur[i - w];
      if (eD) acc -= (double)eD * cur[i + w];
      xs[(s + 1) & 1][i] = d > 0 ? cur[i] + OMEGA * (fi - acc) * id : 0.0;
    }
    __syncthreads();
  }
  if (on) x[i] = xs[COARSEST_SWEEPS & 1][i];
}

inline dim3 grid_of(int64_t n) { return dim3(grid_1d(n, THREADS)); }

// one V-cycle: g[0].xa = M⁻¹ g[0].f.  Launches counted in `launches`.
void vcycle(const Grid* g, int L, hipStream_t s, int& launches) {
  for (int l = 0; l + 1 < L; ++l) {
    const Grid& a = g[l];
    const Grid& c = g[l + 1];
    hipLaunchKernelGGL(height_presmooth_k, grid_of(a.n), dim3(THREADS), 0, s, a.wR, a.wD, a.deg, a.f, a.n, a.w, a.xa);
    hipLaunchKernelGGL(height_restrict_k, grid_of(c.n), dim3(THREADS), 0, s, a.wR, a.wD, a.deg, a.f, a.xa, a.h, a.w,
                       c.h, c.w, c.f);
    launches += 2;
  }
  const Grid& last = g[L - 1];
  hipLaunchKernelGGL(height_coarsest_k, dim3(1), dim3(64), 0, s, last.wR, last.wD, last.deg, last.f, (int)last.n,
                     last.w, last.xa);
  ++launches;
  for (int l = L - 2; l >= 0; --l) {
    const Grid& a = g[l];
    const Grid& c = g[l + 1];
    hipLaunchKernelGGL(height_prolong_k, grid_of(a.n), dim3(THREADS), 0, s, a.deg, c.xa, a.h, a.w, c.w, a.xa);
    hipLaunchKernelGGL(height_sweep_k, grid_of(a.n), dim3(THREADS), 0, s, a.wR, a.wD, a.deg, a.f, a.xa, a.n, a.w,
                       a.xb);
    hipLaunchKernelGGL(height_sweep_k, grid_of(a.n), dim3(THREADS), 0, s, a.wR, a.wD, a.deg, a.f, a.xb, a.n, a.w,
                       a.xa);
    launches += 3;
  }
}

}  // namespace
}  // namespace rti

using namespace rti;

extern "C" int rti_height_levels(int H, int W) { return dims_ok(H, W) ? levels_of(H, W) : -1; }

extern "C" size_t rti_height_workspace_bytes(int H, int W, int precond) {
  if (!dims_ok(H, W) || (precond != RTI_HEIGHT_MULTIGRID && precond != RTI_HEIGHT_JACOBI)) return 0;
  return layout_of((int64_t)H * W, precond).total;
}

extern "C" int rti_height_from_normals(const float* normals, int normal_layout, int H, int W, double nz_min,
                                       int flip_y, const float* z0, double rtol, int max_iters, int check_every,
                                       int precond, void* workspace, float* height, uint8_t* valid, double* stats,
                                       rti_stream_t stream) {
  const char* const E = "rti_height_from_normals";
  if (int st = check_pointers(E, {normals, workspace, height})) return st;
  if (H < 1 || W < 1) return fail(RTI_ERR_BAD_ARG, "%s: H and W must be positive", E);
  if ((int64_t)H * W >= ((int64_t)1 << 31)) return fail(RTI_ERR_BAD_ARG, "%s: H*W must be below 2^31", E);
  if (int st = check_normal_layout(E, normal_layout)) return st;
  if (precond != RTI_HEIGHT_MULTIGRID && precond != RTI_HEIGHT_JACOBI)
    return fail(RTI_ERR_BAD_ARG, "%s: preconditioner %d", E, precond);
  if (!(nz_min > 0.0 && nz_min <= 1.0)) return fail(RTI_ERR_BAD_ARG, "%s: nz_min %g outside (0, 1]", E, nz_min);
  if (!std::isfinite(rtol) || rtol < 0.0) return fail(RTI_ERR_BAD_ARG, "%s: rtol %g must be finite and >= 0", E, rtol);
  if (max_iters < 0 || max_iters > 100000)
    return fail(RTI_ERR_BAD_ARG, "%s: max_iters %d outside [0, 100000]", E, max_iters);
  if (check_every < 1 || check_every > 1024)
    return fail(RTI_ERR_BAD_ARG, "%s: check_every %d outside [1, 1024]", E, check_every);
  if (!aligned_to(workspace, 256)) return fail(RTI_ERR_BAD_ARG, "%s: workspace must be 256-byte aligned", E);
  const int64_t P = (int64_t)H * W;
  {
    const uintptr_t n0 = (uintptr_t)normals, n1 = n0 + (uintptr_t)P * 3 * sizeof(float);
    const uintptr_t h0 = (uintptr_t)height, h1 = h0 + (uintptr_t)P * sizeof(float);
    if (n0 < h1 && h0 < n1) return fail(RTI_ERR_BAD_ARG, "%s: height overlaps normals", E);
  }

  hipStream_t s = (hipStream_t)stream;
  const Layout lay = layout_of(P, precond);
  char* const ws = static_cast<char*>(workspace);
  double* const sc = reinterpret_cast<double*>(ws + lay.scalars);
  double* const part0 = reinterpret_cast<double*>(ws + lay.part0);
  double* const part1 = reinterpret_cast<double*>(ws + lay.part1);
  double* vec[6];
  for (int i = 0; i < 6; ++i) vec[i] = reinterpret_cast<double*>(ws + lay.vec[i]);
  double *const z = vec[0], *const r = vec[1], *const p = vec[2], *const q = vec[3], *const sv = vec[4],
               *const b = vec[5];
  const int L = precond == RTI_HEIGHT_MULTIGRID ? levels_of(H, W) : 1;
  Grid g[MAX_LEVELS];
  g[0] = Grid{H, W, P, reinterpret_cast<int*>(ws + lay.w0[0]), reinterpret_cast<int*>(ws + lay.w0[1]),
              reinterpret_cast<int*>(ws + lay.w0[2]), r, sv, q};  // the V-cycle reads r, writes s, borrows q
  {
    int64_t at = 0;  // cells of the coarse arrays taken so far (at most coarse_cells(P) in all)
    for (int l = 1; l < L; ++l) {
      Grid& c = g[l];
      c.h = (g[l - 1].h + 1) / 2;
      c.w = (g[l - 1].w + 1) / 2;
      c.n = (int64_t)c.h * c.w;
      c.wR = reinterpret_cast<int*>(ws + lay.cw[0]) + at;
      c.wD = reinterpret_cast<int*>(ws + lay.cw[1]) + at;
      c.deg = reinterpret_cast<int*>(ws + lay.cw[2]) + at;
      c.f = reinterpret_cast<double*>(ws + lay.cf[0]) + at;
      c.xa = reinterpret_cast<double*>(ws + lay.cf[1]) + at;
      c.xb = reinterpret_cast<double*>(ws + lay.cf[2]) + at;
      at += c.n;
    }
  }
  const int64_t chunk = chunk_of(P);
  const int nb = blocks_of(P);
  const dim3 rgrid((unsigned)nb), block(THREADS);
  int launches = 0;
  auto reduce = [&](int mode, int iter) {
    hipLaunchKernelGGL(height_reduce_k, dim3(1), block, 0, s, part0, part1, nb, mode, rtol, iter, sc);
    ++launches;
  };
  double host[S_COUNT];
  auto read_scalars = [&]() -> hipError_t {
    hipError_t e = hipMemcpyAsync(host, sc, sizeof(host), hipMemcpyDeviceToHost, s);
    return e != hipSuccess ? e : hipStreamSynchronize(s);
  };
  auto hip_fail = [&](hipError_t e) { return fail(RTI_ERR_HIP, "%s: %s", E, hipGetErrorString(e)); };

  with_normal_layout(normal_layout, [&](auto nl) {
    hipLaunchKernelGGL(height_setup_k<decltype(nl)::value>, rgrid, block, 0, s, normals, H, W, nz_min, flip_y, z0,
                       chunk, g[0].wR, g[0].wD, g[0].deg, b, z, part0, part1);
  });
  reduce(RED_SETUP, 0);
  hipLaunchKernelGGL(height_residual_k<true>, rgrid, block, 0, s, g[0].wR, g[0].wD, g[0].deg, b, z, P, W, chunk, r,
                     part0);
  reduce(RED_RR0, 0);
  launches += 2;
  for (int l = 1; l < L; ++l) {
    hipLaunchKernelGGL(height_coarsen_k, grid_of(g[l].n), block, 0, s, g[l - 1].wR, g[l - 1].wD, g[l - 1].h,
                       g[l - 1].w, g[l].h, g[l].w, g[l].wR, g[l].wD, g[l].deg);
    ++launches;
  }
  if (int st = check_launch(E)) return st;
  if (hipError_t e = read_scalars()) return hip_fail(e);

  auto precondition = [&](int mode) {  // s = M⁻¹ r and ρ = r·s
    if (precond == RTI_HEIGHT_JACOBI) {
      hipLaunchKernelGGL(height_dot_k<true>, rgrid, block, 0, s, g[0].deg, r, P, chunk, sv, part0);
    } else {
      vcycle(g, L, s, launches);
      hipLaunchKernelGGL(height_dot_k<false>, rgrid, block, 0, s, g[0].deg, r, P, chunk, sv, part0);
    }
    ++launches;
    reduce(mode, 0);
  };

  int iters = 0;
  const bool trivial = !(host[S_BB] > 0.0);  // b = 0 (a flat map, no valid pixel): z = 0, nothing to divide
  if (trivial && z0) {
    hipError_t e = hipMemsetAsync(z, 0, (size_t)P * sizeof(double), s);
    if (e != hipSuccess) return hip_fail(e);
  }
  if (!trivial && host[S_MET] < 0.0 && max_iters > 0) {
    precondition(RED_RHO_FIRST);
    hipLaunchKernelGGL(height_direction_k, grid_of(P), block, 0, s, sc, sv, P, 1, p);
    ++launches;
    while (iters < max_iters) {
      ++iters;
      hipLaunchKernelGGL(height_apply_k, rgrid, block, 0, s, g[0].wR, g[0].wD, g[0].deg, p, P, W, chunk, q, part0);
      reduce(RED_PQ, iters);
      hipLaunchKernelGGL(height_update_k, rgrid, block, 0, s, sc, p, q, P, chunk, z, r, part0);
      reduce(RED_RR, iters);
      launches += 2;
      if (iters % check_every == 0 || iters == max_iters) {
        if (int st = check_launch(E)) return st;
        if (hipError_t e = read_scalars()) return hip_fail(e);
        if (host[S_MET] >= 0.0) break;
      }
      if (iters == max_iters) break;
      precondition(RED_RHO);
      hipLaunchKernelGGL(height_direction_k, grid_of(P), block, 0, s, sc, sv, P, 0, p);
      ++launches;
    }
  }

  if (!trivial) {
    hipLaunchKernelGGL(height_residual_k<false>, rgrid, block, 0, s, g[0].wR, g[0].wD, g[0].deg, b, z, P, W, chunk,
                       (double*)nullptr, part0);
    reduce(RED_TRUE, 0);
    ++launches;
  }
  hipLaunchKernelGGL(height_zsum_k, rgrid, block, 0, s, z, P, chunk, part0);
  reduce(RED_ZSUM, 0);
  hipLaunchKernelGGL(height_finish_k, grid_of(P), block, 0, s, sc, g[0].deg, z, P, height, valid);
  launches += 2;
  note_launches(launches);
  if (int st = check_launch(E)) return st;
  if (hipError_t e = read_scalars()) return hip_fail(e);
  if (stats) {
    const double nb2 = std::sqrt(host[S_BB]);
    stats[0] = (double)iters;
    stats[1] = trivial ? 0.0 : host[S_MET];
    stats[2] = trivial ? 0.0 : std::sqrt(host[S_RR]) / nb2;
    stats[3] = trivial ? 0.0 : std::sqrt(host[S_TRUE_RR]) / nb2;
    stats[4] = host[S_NVALID];
    stats[5] = nb2;
  }
  return RTI_OK;
}
