// Rayleigh-quotient minimisation (MGCMTSolver.py:17-57) on 3-D levels: the algorithm of kernels_rq.hip — two passes over
// the data per step, the 2 x 2 pencil solved on the device by the same one-workgroup scalar kernels, the same state
// words and partial-sum layout (rq_common.h), so the sums are added in a fixed order and the results are deterministic.
//
// A 3-D level is n^3 points, idx = z n^2 + y n + x, with A and M as K3Op (kernels_3d.hip).  Three forms:
//   - flat: one thread per point (grid-strided over at most kFlatBlocks workgroups), any A and M — the 27-point Galerkin
//     levels of a V-cycle, a mass operator, the cube well's fine level;
//   - marching: the constant 7-point fine level with M = I and n a multiple of 64 (the scaled Laplacian of a box).  A
//     workgroup owns a 64 x 4 tile of x-y columns and marches a chunk of z-planes with the planes z-1, z, z+1 of both
//     vectors in registers (the k3m_sweep pattern); the x-y neighbours are the neighbouring threads' loads of the same
//     plane (L1 / L2 hits).  Pass 1 reads x, g, p_old, forms p = -g + beta p_old on the fly and writes p; pass 2 reads
//     x, p, forms x + delta p on the fly and writes x', g': 32 B per point and pass.  Same arithmetic per point as the
//     flat form (same terms, same order); only the order of the partial sums differs;
//   - small: a level of at most 16^3 points, the whole call in ONE workgroup launch (k_rq_small of kernels_rq.hip): the
//     coarse levels of a vcycle_rqmg, which are otherwise pure launch latency.
#include <cstdint>
#include <cstdlib>

#include "mgcmt_internal.h"
#include "rq_common.h"

namespace mgcmt {

namespace {

constexpr int kTileX = 64, kTileY = 4;  // marching: x-y tile of a workgroup (kRqThreads = 256 threads)
constexpr int kFlatBlocks = 4096;       // partial sums per result: what the scalar kernels and the plan's scratch hold
constexpr int kRq3SmallMax = 4096;      // 16^3: four points per thread of the single workgroup

// (Op v)(z, y, x) with v = cu u + cw w formed on the fly (u alone when w == nullptr); identity: v(z, y, x).  Out-of-grid
// neighbours are zero (Dirichlet) and are never read.
__device__ __forceinline__ double apply3_point(const K3Op& op, int identity, const double* __restrict__ u, const double* __restrict__ w, double cu, double cw,
                                               long z, long y, long x) {
  const long n = op.n, n2 = n * n;
  const long c = z * n2 + y * n + x;
  auto val = [&](long off) { return w ? cu * u[off] + cw * w[off] : cu * u[off]; };
  if (identity) return val(c);
  const bool zm = z > 0, zp = z + 1 < n, ym = y > 0, yp = y + 1 < n, xm = x > 0, xp = x + 1 < n;
  if (op.seven) {
    double acc = op.c0 * val(c);
    if (xm) acc += op.cxm * val(c - 1);
    if (xp) acc += op.cxp * val(c + 1);
    if (ym) acc += op.cym * val(c - n);
    if (yp) acc += op.cyp * val(c + n);
    if (zm) acc += op.czm * val(c - n2);
    if (zp) acc += op.czp * val(c + n2);
    return acc;
  }
  // general: the 27 values once, then a(dz, dy, dx) = sum_m X_m[dz](z) Y_m[dy](y) Z_m[dx](x) term by term
  const bool in[3][3] = {{zm, true, zp}, {ym, true, yp}, {xm, true, xp}};
  double v[3][3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b)
      for (int e = 0; e < 3; ++e)
        v[a][b][e] = (in[0][a] && in[1][b] && in[2][e]) ? val(c + (a - 1) * n2 + (b - 1) * n + (e - 1)) : 0.0;
  double acc = 0.0;
  for (int m = 0; m < op.nterms; ++m) {
    double fz[3], fy[3], fx[3];
    for (int t = 0; t < 3; ++t) {
      fz[t] = op.X[m][t * n + z];
      fy[t] = op.Y[m][t * n + y];
      fx[t] = op.Z[m][t * n + x];
    }
    double pa = 0.0;
    for (int a = 0; a < 3; ++a) {
      double pb = 0.0;
      for (int b = 0; b < 3; ++b) pb += fy[b] * (fx[0] * v[a][b][0] + fx[1] * v[a][b][1] + fx[2] * v[a][b][2]);
      pa += fz[a] * pb;
    }
    acc += pa;
  }
  return acc;
}

// ---- flat: one thread per point ------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kRqThreads) k_rq3_pass1(K3Op A, K3Op Mo, int m_identity, const double* __restrict__ x, const double* __restrict__ gv,
                                                         const double* __restrict__ pold, double* __restrict__ pnew, const double* __restrict__ state,
                                                         int init, double* __restrict__ partials, int nblocks) {
  __shared__ double s_part[kRqSums][kRqThreads / 64];
  const long n = A.n, n2 = n * n, N = n2 * n;
  const double beta = init ? 0.0 : state[kBeta];
  const double* po = init >= 2 ? nullptr : pold;  // the first step takes p = -g (MGCMTSolver.py:29-30): p_old is not read
  const double cg = init == 3 ? 1.0 : -1.0;        // (init 3: the direction is gv itself, mgcmt_rq_line_step)
  double acc[kRqSums];
#pragma unroll
  for (int q = 0; q < kRqSums; ++q) acc[q] = 0.0;
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < N; k += (long)gridDim.x * blockDim.x) {
    const long z = k / n2, y = (k / n) % n, xx = k % n;
    const double xc = x[k], pc = init == 1 ? 0.0 : (po ? cg * gv[k] + beta * po[k] : cg * gv[k]);
    const double ax = apply3_point(A, 0, x, nullptr, 1.0, 0.0, z, y, xx), mx = apply3_point(Mo, m_identity, x, nullptr, 1.0, 0.0, z, y, xx);
    const double ap = init == 1 ? 0.0 : apply3_point(A, 0, gv, po, cg, beta, z, y, xx);
    const double mp = init == 1 ? 0.0 : apply3_point(Mo, m_identity, gv, po, cg, beta, z, y, xx);
    acc[kS_xAx] += xc * ax;
    acc[kS_xAp] += xc * ap;
    acc[kS_pAx] += pc * ax;
    acc[kS_pAp] += pc * ap;
    acc[kS_xMx] += xc * mx;
    acc[kS_xMp] += xc * mp;
    acc[kS_pMx] += pc * mx;
    acc[kS_pMp] += pc * mp;
    if (init == 0 || init == 2) pnew[k] = pc;
  }
  block_partials<kRqSums>(acc, s_part, partials, nblocks, (int)blockIdx.x);
}

__global__ void __launch_bounds__(kRqThreads) k_rq3_pass2(K3Op A, K3Op Mo, int m_identity, const double* __restrict__ x, const double* __restrict__ p,
                                                         double* __restrict__ xnew, double* __restrict__ gout, const double* __restrict__ state, int init,
                                                         double* __restrict__ partials, int nblocks) {
  __shared__ double s_part[3][kRqThreads / 64];
  const long n = A.n, n2 = n * n, N = n2 * n;
  const double delta = state[kDelta], rho = state[kRhoLin];
  const double* pp = init == 1 ? nullptr : p;
  double acc[3] = {0.0, 0.0, 0.0};
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < N; k += (long)gridDim.x * blockDim.x) {
    const long z = k / n2, y = (k / n) % n, xx = k % n;
    const double xc = pp ? 1.0 * x[k] + delta * pp[k] : 1.0 * x[k];
    const double ax = apply3_point(A, 0, x, pp, 1.0, delta, z, y, xx), mx = apply3_point(Mo, m_identity, x, pp, 1.0, delta, z, y, xx);
    const double gg = 2.0 * (ax - rho * mx);
    if (init != 1) xnew[k] = xc;  // (the initial pair: x' = x stays where it is)
    gout[k] = gg;
    acc[0] += xc * ax;
    acc[1] += xc * mx;
    acc[2] += gg * gg;
  }
  block_partials<3>(acc, s_part, partials, nblocks, (int)blockIdx.x);
}

// <g, M g> without storing M g: result 3 of pass 2's partial sums (the flat pass 2's grid)
__global__ void __launch_bounds__(kRqThreads) k_rq3_gmg(K3Op Mo, const double* __restrict__ gv, double* __restrict__ partials, int nblocks) {
  __shared__ double s_part[1][kRqThreads / 64];
  const long n = Mo.n, n2 = n * n, N = n2 * n;
  double acc[1] = {0.0};
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < N; k += (long)gridDim.x * blockDim.x) {
    const long z = k / n2, y = (k / n) % n, xx = k % n;
    acc[0] += gv[k] * apply3_point(Mo, 0, gv, nullptr, 1.0, 0.0, z, y, xx);
  }
  block_partials<1>(acc, s_part, partials + 3L * nblocks, nblocks, (int)blockIdx.x);
}

// ---- marching: constant 7-point A, M = I ------------------------------------------------------------------------------

// 7-point A at (z, y, x) of column `col`: the plane's x-y neighbours through `val`, the z neighbours from registers; the
// terms in the order of apply3_point
template <class V>
__device__ __forceinline__ double apply7(const K3Op& A, V val, long c, double vc, double vzm, double vzp, bool xm, bool xp, bool ym, bool yp, bool zm,
                                         bool zp) {
  const long n = A.n;
  double acc = A.c0 * vc;
  if (xm) acc += A.cxm * val(c - 1);
  if (xp) acc += A.cxp * val(c + 1);
  if (ym) acc += A.cym * val(c - n);
  if (yp) acc += A.cyp * val(c + n);
  if (zm) acc += A.czm * vzm;
  if (zp) acc += A.czp * vzp;
  return acc;
}

__global__ void __launch_bounds__(kRqThreads) k_rq3m_pass1(K3Op A, const double* __restrict__ x, const double* __restrict__ gv, const double* __restrict__ pold,
                                                          double* __restrict__ pnew, const double* __restrict__ state, int init, int chunk,
                                                          double* __restrict__ partials, int nblocks) {
  __shared__ double s_part[kRqSums][kRqThreads / 64];
  const long n = A.n, n2 = n * n;
  const long xi = (long)blockIdx.x * kTileX + (threadIdx.x & 63);
  const long yi = (long)blockIdx.y * kTileY + (threadIdx.x >> 6);
  const long z0 = (long)blockIdx.z * chunk;
  const double beta = init ? 0.0 : state[kBeta];
  const double* po = init >= 2 ? nullptr : pold;
  const double cg = init == 3 ? 1.0 : -1.0;
  const bool xm = xi > 0, xp = xi + 1 < n, ym = yi > 0, yp = yi + 1 < n;
  const long col = yi * n + xi;
  auto X = [&](long off) { return 1.0 * x[off]; };
  auto P = [&](long off) { return init == 1 ? 0.0 : (po ? cg * gv[off] + beta * po[off] : cg * gv[off]); };
  double acc[kRqSums];
#pragma unroll
  for (int q = 0; q < kRqSums; ++q) acc[q] = 0.0;
  double xm_ = z0 > 0 ? X((z0 - 1) * n2 + col) : 0.0, xc_ = X(z0 * n2 + col);
  double pm_ = z0 > 0 ? P((z0 - 1) * n2 + col) : 0.0, pc_ = P(z0 * n2 + col);
  for (int t = 0; t < chunk; ++t) {
    const long z = z0 + t, c = z * n2 + col;
    const bool zm = z > 0, zp = z + 1 < n;
    const double xp_ = zp ? X(c + n2) : 0.0, pp_ = zp ? P(c + n2) : 0.0;
    const double ax = apply7(A, X, c, xc_, xm_, xp_, xm, xp, ym, yp, zm, zp);
    const double ap = init == 1 ? 0.0 : apply7(A, P, c, pc_, pm_, pp_, xm, xp, ym, yp, zm, zp);
    const double mx = xc_, mp = pc_;
    acc[kS_xAx] += xc_ * ax;
    acc[kS_xAp] += xc_ * ap;
    acc[kS_pAx] += pc_ * ax;
    acc[kS_pAp] += pc_ * ap;
    acc[kS_xMx] += xc_ * mx;
    acc[kS_xMp] += xc_ * mp;
    acc[kS_pMx] += pc_ * mx;
    acc[kS_pMp] += pc_ * mp;
    if (init == 0 || init == 2) pnew[c] = pc_;
    xm_ = xc_;
    xc_ = xp_;
    pm_ = pc_;
    pc_ = pp_;
  }
  block_partials<kRqSums>(acc, s_part, partials, nblocks, (int)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)));
}

__global__ void __launch_bounds__(kRqThreads) k_rq3m_pass2(K3Op A, const double* __restrict__ x, const double* __restrict__ p, double* __restrict__ xnew,
                                                          double* __restrict__ gout, const double* __restrict__ state, int init, int chunk,
                                                          double* __restrict__ partials, int nblocks) {
  __shared__ double s_part[3][kRqThreads / 64];
  const long n = A.n, n2 = n * n;
  const long xi = (long)blockIdx.x * kTileX + (threadIdx.x & 63);
  const long yi = (long)blockIdx.y * kTileY + (threadIdx.x >> 6);
  const long z0 = (long)blockIdx.z * chunk;
  const double delta = state[kDelta], rho = state[kRhoLin];
  const double* pp = init == 1 ? nullptr : p;
  const bool xm = xi > 0, xp = xi + 1 < n, ym = yi > 0, yp = yi + 1 < n;
  const long col = yi * n + xi;
  auto X = [&](long off) { return pp ? 1.0 * x[off] + delta * pp[off] : 1.0 * x[off]; };
  double acc[3] = {0.0, 0.0, 0.0};
  double vm = z0 > 0 ? X((z0 - 1) * n2 + col) : 0.0, vc = X(z0 * n2 + col);
  for (int t = 0; t < chunk; ++t) {
    const long z = z0 + t, c = z * n2 + col;
    const bool zm = z > 0, zp = z + 1 < n;
    const double vp = zp ? X(c + n2) : 0.0;
    const double ax = apply7(A, X, c, vc, vm, vp, xm, xp, ym, yp, zm, zp);
    const double mx = vc;
    const double gg = 2.0 * (ax - rho * mx);
    if (init != 1) xnew[c] = vc;
    gout[c] = gg;
    acc[0] += vc * ax;
    acc[1] += vc * mx;
    acc[2] += gg * gg;
    vm = vc;
    vc = vp;
  }
  block_partials<3>(acc, s_part, partials, nblocks, (int)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)));
}

// ---- small: the whole call in one workgroup -----------------------------------------------------------------------------
// k_rq_small (kernels_rq.hip) with the 3-D operators: vectors updated in place in global memory, sums reduced in LDS, the
// scalars by thread 0 into an LDS copy of the state block, block barriers where the passes have kernel boundaries.
__global__ void __launch_bounds__(kRqSmallThreads) k_rq3_small(K3Op A, K3Op Mo, int m_identity, double* x, double* p, double* gv, double* state, int nu,
                                                             int robust) {
  __shared__ double s_part[kRqSums][kRqSmallThreads / 64];
  __shared__ double s_sum[kRqSums];
  __shared__ double s_state[kRqStateWords];
  const long n = A.n, n2 = n * n, N = n2 * n;
  if (threadIdx.x < kRqStateWords) s_state[threadIdx.x] = state[threadIdx.x];
  __syncthreads();
  for (int it = -1; it < nu; ++it) {  // (uniform trip counts: every thread reaches every barrier)
    const int init = it < 0 ? 1 : (it == 0 ? 2 : 0);
    if (init != 1) {
      const double beta = init == 2 ? 0.0 : s_state[kBeta];
      for (long k = threadIdx.x; k < N; k += kRqSmallThreads) p[k] = init == 2 ? -gv[k] : -gv[k] + beta * p[k];
      __syncthreads();
    }
    double acc[kRqSums];
#pragma unroll
    for (int q = 0; q < kRqSums; ++q) acc[q] = 0.0;
    for (long k = threadIdx.x; k < N; k += kRqSmallThreads) {
      const long z = k / n2, y = (k / n) % n, xx = k % n;
      const double xc = x[k], pc = init == 1 ? 0.0 : p[k];
      const double ax = apply3_point(A, 0, x, nullptr, 1.0, 0.0, z, y, xx), mx = apply3_point(Mo, m_identity, x, nullptr, 1.0, 0.0, z, y, xx);
      const double ap = init == 1 ? 0.0 : apply3_point(A, 0, p, nullptr, 1.0, 0.0, z, y, xx);
      const double mp = init == 1 ? 0.0 : apply3_point(Mo, m_identity, p, nullptr, 1.0, 0.0, z, y, xx);
      acc[kS_xAx] += xc * ax;
      acc[kS_xAp] += xc * ap;
      acc[kS_pAx] += pc * ax;
      acc[kS_pAp] += pc * ap;
      acc[kS_xMx] += xc * mx;
      acc[kS_xMp] += xc * mp;
      acc[kS_pMx] += pc * mx;
      acc[kS_pMp] += pc * mp;
    }
    small_reduce<kRqSums>(acc, s_part, s_sum);
    if (threadIdx.x == 0) rq_step_scalars(s_sum, s_state, init, robust);
    __syncthreads();
    if (init != 1) {
      const double delta = s_state[kDelta];
      for (long k = threadIdx.x; k < N; k += kRqSmallThreads) x[k] = x[k] + delta * p[k];
      __syncthreads();
    }
    const double rho = s_state[kRhoLin];
    double acc2[4] = {0.0, 0.0, 0.0, 0.0};
    for (long k = threadIdx.x; k < N; k += kRqSmallThreads) {
      const long z = k / n2, y = (k / n) % n, xx = k % n;
      const double xc = x[k];
      const double ax = apply3_point(A, 0, x, nullptr, 1.0, 0.0, z, y, xx), mx = apply3_point(Mo, m_identity, x, nullptr, 1.0, 0.0, z, y, xx);
      const double gg = 2.0 * (ax - rho * mx);
      gv[k] = gg;
      acc2[0] += xc * ax;
      acc2[1] += xc * mx;
      acc2[2] += gg * gg;
    }
    if (!m_identity) {
      __syncthreads();
      for (long k = threadIdx.x; k < N; k += kRqSmallThreads) {
        const long z = k / n2, y = (k / n) % n, xx = k % n;
        acc2[3] += gv[k] * apply3_point(Mo, 0, gv, nullptr, 1.0, 0.0, z, y, xx);
      }
    }
    small_reduce<4>(acc2, s_part, s_sum);
    if (threadIdx.x == 0) rq_gradient_scalars(s_sum, s_sum[3], s_state, m_identity ? 1 : 0, init);
    __syncthreads();
  }
  if (threadIdx.x < kRqStateWords) state[threadIdx.x] = s_state[threadIdx.x];
}

// flat launch geometry: one thread per point, at most kFlatBlocks workgroups
int flat_blocks(const K3Op& A) {
  const long N = A.n * A.n * A.n;
  const long b = (N + kRqThreads - 1) / kRqThreads;
  return (int)(b < kFlatBlocks ? b : kFlatBlocks);
}

// marching launch geometry: z-planes per chunk — 32, longer where the partial sums would overflow, shorter where the level
// would not fill the chip (a march is one dependent load per plane)
dim3 march_grid(const K3Op& A, int* chunk) {
  const long n = A.n, xy = (n / kTileX) * (n / kTileY);
  long c = 32 < n ? 32 : n;
  while (xy * (n / c) > kFlatBlocks && c < n) c *= 2;
  while (c > 4 && xy * (n / c) < 2048) c /= 2;
  *chunk = (int)c;
  return dim3((unsigned)(n / kTileX), (unsigned)(n / kTileY), (unsigned)(n / c));
}

}  // namespace

// the marching passes take the level: constant 7-point A, M = I, n a multiple of 64 (MGCMT_RQ_MARCH=0: the flat form,
// read per call so tests can compare both in one process)
bool rq3_marching(const K3Op& A, int m_identity) {
  const char* e = getenv("MGCMT_RQ_MARCH");
  if (e && e[0] == '0') return false;
  return A.seven && m_identity && A.n >= kTileX && A.n % kTileX == 0;
}

void launch_rq3_pass1(hipStream_t s, const K3Op& A, const K3Op& Mo, int m_identity, const double* x, const double* gv, const double* pold, double* pnew,
                      double* state, int init, int robust, double* partials) {
  int nblocks;
  if (rq3_marching(A, m_identity)) {
    int chunk;
    const dim3 grid = march_grid(A, &chunk);
    nblocks = (int)(grid.x * grid.y * grid.z);
    hipLaunchKernelGGL(k_rq3m_pass1, grid, dim3(kRqThreads), 0, s, A, x, gv, pold, pnew, state, init, chunk, partials, nblocks);
  } else {
    nblocks = flat_blocks(A);
    hipLaunchKernelGGL(k_rq3_pass1, dim3((unsigned)nblocks), dim3(kRqThreads), 0, s, A, Mo, m_identity, x, gv, pold, pnew, state, init, partials, nblocks);
  }
  launch_rq_scalars1(s, partials, nblocks, state, init, robust);
}

int launch_rq3_pass2(hipStream_t s, const K3Op& A, const K3Op& Mo, int m_identity, const double* x, const double* p, double* xnew, double* gout, double* state,
                     int init, double* partials) {
  int nblocks;
  if (rq3_marching(A, m_identity)) {
    int chunk;
    const dim3 grid = march_grid(A, &chunk);
    nblocks = (int)(grid.x * grid.y * grid.z);
    hipLaunchKernelGGL(k_rq3m_pass2, grid, dim3(kRqThreads), 0, s, A, x, p, xnew, gout, state, init, chunk, partials, nblocks);
  } else {
    nblocks = flat_blocks(A);
    hipLaunchKernelGGL(k_rq3_pass2, dim3((unsigned)nblocks), dim3(kRqThreads), 0, s, A, Mo, m_identity, x, p, xnew, gout, state, init, partials, nblocks);
  }
  return nblocks;
}

bool launch_rq3_gmg(hipStream_t s, const K3Op& Mo, const double* gv, double* partials, int nblocks) {
  if (flat_blocks(Mo) != nblocks) return false;  // (pass 2 marched: M is the identity there, <g, g> is already result 2)
  hipLaunchKernelGGL(k_rq3_gmg, dim3((unsigned)nblocks), dim3(kRqThreads), 0, s, Mo, gv, partials, nblocks);
  return true;
}

bool launch_rq3_small(hipStream_t s, const K3Op& A, const K3Op& Mo, int m_identity, double* x, double* p, double* gv, double* state, int nu, int robust) {
  if (A.n * A.n * A.n > kRq3SmallMax) return false;
  hipLaunchKernelGGL(k_rq3_small, dim3(1), dim3(kRqSmallThreads), 0, s, A, Mo, m_identity, x, p, gv, state, nu, robust);
  return true;
}

}  // namespace mgcmt
