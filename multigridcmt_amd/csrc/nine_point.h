// One point of (A - mu I) for a 9-point operator with per-point coefficients (KOp::point == kPointPlanes): the Kronecker part plus nine
// planes G, the coefficient of v(i + a - 1, j + b - 1) in row (i, j) being G[3 a + b](i, j) — the Galerkin levels of every plan
// with a per-point part, and level 0 of mgcmt_plan_create_nine (H = -div(W grad) + V with a 2 x 2 inverse-mass tensor W).
//
// The functions take VALUES — the centre, the eight neighbours, the nine coefficients — so the flat kernels
// (kernels_pointwise.hip, one thread per point, values from global memory) and the tile kernels (kernels_nine_tile.hip, values
// from LDS) call them with the same numbers and a sweep gives the same bits in either form.  A neighbour outside the grid
// enters as value 0; G is zero towards it.  Two forms of the Kronecker part:
//   five     constant 5-point (c0, cn, cw): explicit fma, one fixed order (west, east, north, south, then the corners north-west,
//            north-east, south-west, south-east), the reciprocal of the fused policies — level 0 of mgcmt_plan_create_nine
//   general  any Kronecker terms: the expressions and the order the Galerkin levels have always been evaluated with
#pragma once

#include "fused_kernel.h"
#include "mgcmt_internal.h"

namespace mgcmt {
namespace nine {

// v at the eight neighbours of a point, rows north to south
struct Nb {
  double nw, n, ne, w, e, sw, s, se;
};

// neighbour sum, shifted diagonal and its reciprocal
struct Pt {
  double off, dg, inv;
};

// the point's nine coefficients: g[3 a + b] = G[3 a + b](i, j), p = pg + i * pld + j
__device__ __forceinline__ void load9(double (&g)[9], const double* __restrict__ p, long plane) {
#pragma unroll
  for (int a = 0; a < 9; ++a) g[a] = p[a * plane];
}

// constant 5-point Kronecker part; d0 = c0 - mu
__device__ __forceinline__ Pt five(double cn, double cw, double d0, const Nb& v, const double (&g)[9]) {
  double t = (cw + g[3]) * v.w;
  t = fma(cw + g[5], v.e, t);
  t = fma(cn + g[1], v.n, t);
  t = fma(cn + g[7], v.s, t);
  t = fma(g[0], v.nw, t);
  t = fma(g[2], v.ne, t);
  t = fma(g[6], v.sw, t);
  t = fma(g[8], v.se, t);
  Pt p;
  p.off = t;
  p.dg = d0 + g[4];
  p.inv = fused::fast_reciprocal(p.dg);
  return p;
}

// the Kronecker terms of row (i, j): off += the neighbours' part, diag += the diagonal entry
__device__ __forceinline__ void kron_terms(const KOp& op, long i, long j, const Nb& v, double& off, double& diag) {
  for (int m = 0; m < op.nterms; ++m) {
    const double* X = op.X[m] + i;
    const double* Y = op.Y[m] + j;
    const double xl = X[0], xd = X[op.ldx], xu = X[2 * op.ldx];
    const double yl = Y[0], yd = Y[op.ldy], yu = Y[2 * op.ldy];
    const double rn = yl * v.nw + yd * v.n + yu * v.ne;
    const double rc = yl * v.w + yu * v.e;
    const double rs = yl * v.sw + yd * v.s + yu * v.se;
    off += xl * rn + xd * rc + xu * rs;
    diag += xd * yd;
  }
}

// the nine planes' part of the row
__device__ __forceinline__ void plane_terms(const double (&g)[9], const Nb& v, double& off, double& diag) {
  const double rn = g[0] * v.nw + g[1] * v.n + g[2] * v.ne;
  const double rc = g[3] * v.w + g[5] * v.e;
  const double rs = g[6] * v.sw + g[7] * v.s + g[8] * v.se;
  off += rn + rc + rs;
  diag += g[4];
}

// any Kronecker terms plus the nine planes
__device__ __forceinline__ Pt general(const KOp& op, long i, long j, double mu, const Nb& v, const double (&g)[9]) {
  double off = 0.0, diag = 0.0;
  kron_terms(op, i, j, v, off, diag);
  plane_terms(g, v, off, diag);
  Pt p;
  p.off = off;
  p.dg = diag - mu;
  p.inv = 1.0 / p.dg;
  return p;
}

// f - (A - mu I) v at the point
__device__ __forceinline__ double residual(double f, const Pt& p, double vc) { return f - fma(p.dg, vc, p.off); }

// the point's new value under weighted Jacobi / one colour of the multicolour sweep
__device__ __forceinline__ double relaxed(double omega, double f, const Pt& p, double vc) { return fma(omega, (f - fma(p.dg, vc, p.off)) * p.inv, vc); }

}  // namespace nine
}  // namespace mgcmt
