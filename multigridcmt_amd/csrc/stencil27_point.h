// One point of a 3-D level whose per-point part is 27 planes (K3Op::point == kPointPlanes): the Galerkin levels of every 3-D
// plan with a per-point part, and level 0 of mgcmt_plan_create3d_stencil.  The flat kernels of kernels_3d_point.hip and the
// kernels of kernels_3d_stencil.hip compute every point with THESE functions from the same values — the 27 neighbours (zeros
// outside the grid) and the point's 27 coefficients —, so a sweep gives the same bits in either form.  (The library is built
// with -ffp-contract=off: a product and a sum fuse only where fma is written.)
//   general: any Kronecker terms plus the planes — the terms summed as eval3 sums them (kernels_3d.hip), then the planes as
//            three partial sums per z-offset, a division by a_ii - mu in the relaxation.
//   seven:   a constant 7-point Kronecker part plus the planes (level 0 of a stencil plan: K3Op::seven; no level of any other
//            plan has this form, a coarsened 7-point part being a 27-point Kronecker sum) — no factor loads; explicit fma in
//            the fixed neighbour order (a, b, c) = (0,0,0), (0,0,1), ..., (2,2,2), plane 9 a + 3 b + c, the centre first as
//            (c0 - mu + G[1,1,1]) v; the six axis neighbours take their plane plus the constant; fast_reciprocal of
//            c0 - mu + G[1,1,1] once in the relaxation.
#pragma once
#include "fused_kernel.h"
#include "mgcmt_internal.h"

namespace mgcmt {
namespace p27 {

struct Eval {
  double av;  // ((A - mu I) w) at the point
  double dg;  // a_ii - mu
};

// the 27 neighbours of (z, y, x), zeros outside the grid; w(zz, yy, xx): the vector at an in-grid point
template <class W>
__device__ __forceinline__ void neighbours(W&& w, long n, long z, long y, long x, double (&wn)[3][3][3]) {
  const bool zm = z > 0, zp = z + 1 < n, ym = y > 0, yp = y + 1 < n, xm = x > 0, xp = x + 1 < n;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const bool in = (a != 0 || zm) && (a != 2 || zp) && (b != 0 || ym) && (b != 2 || yp) && (c != 0 || xm) && (c != 2 || xp);
        wn[a][b][c] = in ? w(z + a - 1, y + b - 1, x + c - 1) : 0.0;
      }
}

// the point's 27 coefficients (coalesced: a thread reads its own point's)
__device__ __forceinline__ void coefficients(const K3Op& op, long idx, double (&g)[27]) {
  const double* __restrict__ p = op.pg + idx;
  const long pl = op.pplane;
#pragma unroll
  for (int j = 0; j < 27; ++j) g[j] = p[j * pl];
}

// Kronecker part: a(dz, dy, dx) = sum_m X_m[dz](z) Y_m[dy](y) Z_m[dx](x), summed as eval3 does; acc and diag are added to
__device__ __forceinline__ void kronecker(const K3Op& op, long z, long y, long x, const double (&wn)[3][3][3], double& acc, double& diag) {
  const long n = op.n;
  for (int m = 0; m < op.nterms; ++m) {
    double fz[3], fy[3], fx[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      fz[t] = op.X[m][t * n + z];
      fy[t] = op.Y[m][t * n + y];
      fx[t] = op.Z[m][t * n + x];
    }
    diag += fz[1] * fy[1] * fx[1];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double pa = 0.0;
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        double pb = fx[0] * wn[a][b][0];
        pb += fx[1] * wn[a][b][1];
        pb += fx[2] * wn[a][b][2];
        pa += fy[b] * pb;
      }
      acc += fz[a] * pa;
    }
  }
}

__device__ __forceinline__ Eval general(const K3Op& op, long z, long y, long x, const double (&wn)[3][3][3], const double (&g)[27], double mu) {
  double acc = 0.0, diag = 0.0;
  kronecker(op, z, y, x, wn, acc, diag);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double pa = 0.0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      double pb = g[9 * a + 3 * b] * wn[a][b][0];
      pb += g[9 * a + 3 * b + 1] * wn[a][b][1];
      pb += g[9 * a + 3 * b + 2] * wn[a][b][2];
      pa += pb;
    }
    acc += pa;
  }
  diag += g[13];
  // acc holds the unshifted sum, centre included
  Eval r;
  r.dg = diag - mu;
  r.av = acc - mu * wn[1][1][1];
  return r;
}

__device__ __forceinline__ Eval seven(const K3Op& op, const double (&wn)[3][3][3], const double (&g)[27], double mu) {
  Eval r;
  r.dg = (op.c0 - mu) + g[13];
  double acc = r.dg * wn[1][1][1];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int j = 9 * a + 3 * b + c;
        if (j == 13) continue;
        double cf = g[j];
        if (j == 4) cf = op.czm + g[j];
        if (j == 22) cf = op.czp + g[j];
        if (j == 10) cf = op.cym + g[j];
        if (j == 16) cf = op.cyp + g[j];
        if (j == 12) cf = op.cxm + g[j];
        if (j == 14) cf = op.cxp + g[j];
        acc = fma(cf, wn[a][b][c], acc);
      }
  r.av = acc;
  return r;
}

// the point of either form, from values
__device__ __forceinline__ Eval point(const K3Op& op, long z, long y, long x, const double (&wn)[3][3][3], const double (&g)[27], double mu) {
  return op.seven ? seven(op, wn, g, mu) : general(op, z, y, x, wn, g, mu);
}

// ... with the neighbours and the coefficients loaded here
template <class W>
__device__ __forceinline__ Eval point(const K3Op& op, W&& w, long z, long y, long x, double mu) {
  double wn[3][3][3], g[27];
  neighbours(w, op.n, z, y, x, wn);
  coefficients(op, (z * op.n + y) * op.n + x, g);
  return point(op, z, y, x, wn, g, mu);
}

// v + omega (f - (A - mu I) v) / (a_ii - mu)
__device__ __forceinline__ double relax(const K3Op& op, double omega, double f, const Eval& e, double vc) {
  if (op.seven) return fma(omega * (f - e.av), fused::fast_reciprocal(e.dg), vc);
  return vc + omega * (f - e.av) / e.dg;
}

}  // namespace p27
}  // namespace mgcmt
