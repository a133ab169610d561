// Shared by the Rayleigh-quotient kernels (kernels_rq.hip: 1-D and 2-D levels, kernels_rq3d.hip: 3-D levels): the state
// words, the per-block partial sums, and the scalars of a step computed by one thread (the 2 x 2 pencil after pass 1,
// rho and beta after pass 2).  One copy of the arithmetic, so both dimensions take the same scalars from the same sums.
#pragma once

#include "mgcmt_internal.h"

namespace mgcmt {

namespace {

// state words (doubles in device memory, one block per plan)
enum {
  kS_xAx = 0, kS_xAp, kS_pAx, kS_pAp, kS_xMx, kS_xMp, kS_pMx, kS_pMp,  // pass 1
  kDelta = 8, kRho, kBeta, kGMGprev, kGMG, kStop, kXAXn, kXMXn, kGG, kRhoLin,
  kRqStateWords = 32
};

constexpr int kRqThreads = 256;
constexpr int kRqSums = 8;

// per block: nq partial sums into partials[q * nblocks + block] (fixed order: deterministic)
template <int NQ>
__device__ __forceinline__ void block_partials(const double* acc, double (*s_part)[kRqThreads / 64], double* __restrict__ partials, int nblocks, int block) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    double t = acc[q];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) t += __shfl_down(t, d);
    if (lane == 0) s_part[q][wave] = t;
  }
  __syncthreads();
  if ((int)threadIdx.x < NQ) {
    double t = 0.0;
    const int nw = blockDim.x >> 6;
    for (int k = 0; k < nw; ++k) t += s_part[threadIdx.x][k];
    partials[(long)threadIdx.x * nblocks + block] = t;
  }
}

// after pass 1: the 2 x 2 pencil R y = lambda RM y (MGCMTSolver.py:33-49), delta = y1 / y0 of the smaller eigenvalue
// (:49-50), and rho of x + delta p by bilinearity (what pass 2 needs before it has formed x').  init: delta = 0.
// robust (the repaired variants, solver.py): a degenerate pencil ends the minimisation on this level (delta = 0 from
// here on) instead of producing infinities.
// (one thread) the step's scalars from the eight sums s
__device__ void rq_step_scalars(const double* s, double* __restrict__ state, int init, int robust) {
  for (int q = 0; q < kRqSums; ++q) state[q] = s[q];
  const double r00 = s[kS_xAx], r01 = s[kS_xAp], r10 = s[kS_pAx], r11 = s[kS_pAp];
  const double m00 = s[kS_xMx], m01 = s[kS_xMp], m10 = s[kS_pMx], m11 = s[kS_pMp];
  if (init == 1) {
    state[kDelta] = 0.0;
    state[kRhoLin] = r00 / m00;
    state[kStop] = 0.0;
    return;
  }
  double delta = 0.0;
  bool stop = state[kStop] != 0.0;
  if (!stop && robust) {
    const double ms01 = 0.5 * (m01 + m10);
    const double scale = fabs(m00) > 1e-300 ? fabs(m00) : 1e-300;
    auto fin = [](double v) { return fabs(v) <= 1.7e308; };  // (false for NaN and the infinities)
    const bool finite = fin(r00) && fin(r01) && fin(r10) && fin(r11) && fin(m00) && fin(ms01) && fin(m11);
    if (!finite || m11 <= 1e-28 * scale || (m00 * m11 - ms01 * ms01) <= 1e-14 * m00 * m11) stop = true;
  }
  if (!stop) {
    // det(R - l RM) = a l^2 + b l + c; the smaller root (a > 0 for a definite RM), stable form
    const double a = m00 * m11 - m01 * m10;
    const double b = -(r00 * m11 + m00 * r11) + (r01 * m10 + m01 * r10);
    const double c = r00 * r11 - r01 * r10;
    double disc = b * b - 4.0 * a * c;
    if (disc < 0.0) disc = 0.0;
    const double q = -0.5 * (b + (b >= 0.0 ? sqrt(disc) : -sqrt(disc)));
    const double l1 = q / a, l2 = q != 0.0 ? c / q : l1;
    const double lam = l1 < l2 ? l1 : l2;  // (np.argmin of the two eigenvalues, :49)
    // eigenvector from the row (p, .): delta = y1 / y0 = -(r10 - l m10) / (r11 - l m11).  That row, not (x, .): its
    // numerator is p . (A x - l M x), a product with the gradient, where the other row's r00 - l m00 cancels two numbers
    // of the size of <x, A x> down to rounding noise once x has converged (a 2-point level after one step) — and p may be
    // of ANY size, so the rows cannot be compared by magnitude.  The row (x, .) only when the pencil leaves no choice.
    const double n2 = r10 - lam * m10, d2 = r11 - lam * m11;
    delta = -n2 / d2;
    if (!(fabs(delta) <= 1.7e308)) delta = -(r00 - lam * m00) / (r01 - lam * m01);
    // p = 0 (a gradient that came out as exact zeros: x is an eigenvector to the last bit, as on a 2-point level after one
    // step): the minimiser over span{x} is x — where the reference's eig would return NaNs, nothing is updated
    if (!(fabs(delta) <= 1.7e308)) delta = 0.0;
    if (robust && !(fabs(delta) < 1e300)) {  // y0 = 0: the minimiser is p itself — the reference's ratio is infinite
      stop = true;
      delta = 0.0;
    }
  }
  state[kStop] = stop ? 1.0 : 0.0;
  state[kDelta] = delta;
  const double rl = (r00 + delta * (r01 + r10) + delta * delta * r11) / (m00 + delta * (m01 + m10) + delta * delta * m11);
  state[kRhoLin] = fabs(rl) <= 1.7e308 ? rl : r00 / m00;
}

// after pass 2 (and, with M != I, after <g, M g> has been put into state[kGMG] by a dot product): rho (:53), beta (:31)
// (one thread) rho and the next step's beta from <x',Ax'>, <x',Mx'>, <g',g'> (s[0..2]) and <g',Mg'> (gmg_in unless M = I)
__device__ void rq_gradient_scalars(const double* s, double gmg_in, double* __restrict__ state, int m_identity, int init) {
  state[kXAXn] = s[0];
  state[kXMXn] = s[1];
  state[kGG] = s[2];
  state[kRho] = s[0] / s[1];
  const double gmg = m_identity == 1 ? s[2] : gmg_in;
  // the first step takes p = -g (:29-30): beta = 0; afterwards <g,Mg> / <g_old,Mg_old>
  const double prev = state[kGMGprev];
  state[kBeta] = (init == 1 || !(prev != 0.0)) ? 0.0 : gmg / prev;  // (a previous gradient of exact zeros: restart from -g)
  state[kGMGprev] = gmg;
  state[kGMG] = gmg;
}

constexpr int kRqSmallThreads = 1024;
constexpr int kRqSmallMax = kRqSmallThreads;

template <int NQ>
__device__ __forceinline__ void small_reduce(const double* acc, double (*s_part)[kRqSmallThreads / 64], double* s_sum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    double t = acc[q];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) t += __shfl_down(t, d);
    if (lane == 0) s_part[q][wave] = t;
  }
  __syncthreads();
  if ((int)threadIdx.x < NQ) {
    double t = 0.0;
    for (int k = 0; k < kRqSmallThreads / 64; ++k) t += s_part[threadIdx.x][k];
    s_sum[threadIdx.x] = t;
  }
  __syncthreads();
}

}  // namespace

}  // namespace mgcmt
