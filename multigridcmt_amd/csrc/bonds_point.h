// One point of (A - mu I) for a 5-point operator with per-point bond coefficients (KOp::point == kPointBonds,
// mgcmt_plan_create_bonds): the constant 5-point Kronecker part (c0, cn, cw) plus a diagonal D and the bonds E (towards
// the east neighbour) and S (towards the south neighbour) — H = -div(w grad) + V with a position-dependent inverse mass w.
//   east  coefficient  cw + E(i, j)        west   cw + E(i, j - 1)
//   south coefficient  cn + S(i, j)        north  cn + S(i - 1, j)
//   diagonal           (c0 - mu) + D(i, j)
// The flat kernels (kernels_pointwise.hip, one thread per point) and the marching kernels (kernels_bonds.hip) both call
// these functions with the same values, so a sweep gives the same bits in either form: explicit fma, one fixed order
// (west, east, north, south), the reciprocal of the fused policies (fused::fast_reciprocal).  A neighbour outside the grid
// enters as value 0 with bond 0.
#pragma once

#include "fused_kernel.h"

namespace mgcmt {
namespace bonds {

// sum over the four neighbours of a_kj v_j
__device__ __forceinline__ double neighbour_sum(double cw, double cn, double ew, double ee, double sn, double ss, double vw, double ve, double vn,
                                                double vs) {
  double t = (cw + ew) * vw;
  t = fma(cw + ee, ve, t);
  t = fma(cn + sn, vn, t);
  t = fma(cn + ss, vs, t);
  return t;
}

// d0 = c0 - mu
__device__ __forceinline__ double diagonal(double d0, double d) { return d0 + d; }

// (A - mu I) v at the point
__device__ __forceinline__ double applied(double dg, double vc, double off) { return fma(dg, vc, off); }

// f - (A - mu I) v at the point
__device__ __forceinline__ double residual(double f, double dg, double vc, double off) { return f - fma(dg, vc, off); }

// the point's new value under weighted Jacobi / one colour of the multicolour sweep
__device__ __forceinline__ double relaxed(double omega, double f, double dg, double vc, double off) {
  return fma(omega, (f - fma(dg, vc, off)) * fused::fast_reciprocal(dg), vc);
}

}  // namespace bonds
}  // namespace mgcmt
