// One point of a 3-D fine level with a per-point part: a constant 7-point Kronecker part plus a diagonal D (K3Op::point ==
// kPointDiag, mgcmt_plan_create3d_pot) or plus the planes D, Bx, By, Bz (kPointBonds, mgcmt_plan_create3d_bonds).  The flat and
// the marching kernels of kernels_3d_point.hip compute every point of both kinds with THESE functions from the same values —
// the same sums, the same fma order (z-, z+, y-, y+, x-, x+), the same reciprocal of c0 + D - mu — so their sweeps give the
// same bits.  A neighbour outside the grid is passed as zero, and so is the bond towards it.
#pragma once
#include "fused_kernel.h"
#include "mgcmt_internal.h"

namespace mgcmt {
namespace p7 {

// the six off-diagonal entries of the point's row
struct Coef {
  double zm, zp, ym, yp, xm, xp;
};

// a diagonal alone: the operator's constants as they are (not constant + 0.0, which would turn a -0.0 into +0.0)
__device__ __forceinline__ Coef coef(const K3Op& op) { return Coef{op.czm, op.czp, op.cym, op.cyp, op.cxm, op.cxp}; }

// with bonds: bzm = Bz(z-1, y, x), bzp = Bz(z, y, x), and so on
__device__ __forceinline__ Coef coef(const K3Op& op, double bzm, double bzp, double bym, double byp, double bxm, double bxp) {
  Coef c;
  c.zm = op.czm + bzm;
  c.zp = op.czp + bzp;
  c.ym = op.cym + bym;
  c.yp = op.cyp + byp;
  c.xm = op.cxm + bxm;
  c.xp = op.cxp + bxp;
  return c;
}

__device__ __forceinline__ double dg(const K3Op& op, double d, double mu) { return (op.c0 - mu) + d; }

// ((A - mu I) v) at the point
__device__ __forceinline__ double av(const Coef& c, double dgv, double vc, double vzm, double vzp, double vym, double vyp, double vxm,
                                     double vxp) {
  double acc = dgv * vc;
  acc = fma(c.zm, vzm, acc);
  acc = fma(c.zp, vzp, acc);
  acc = fma(c.ym, vym, acc);
  acc = fma(c.yp, vyp, acc);
  acc = fma(c.xm, vxm, acc);
  acc = fma(c.xp, vxp, acc);
  return acc;
}

// v + omega (f - (A - mu I) v) / (c0 + D - mu)
__device__ __forceinline__ double relax(double omega, double f, double avv, double dgv, double vc) {
  return fma(omega * (f - avv), fused::fast_reciprocal(dgv), vc);
}

}  // namespace p7
}  // namespace mgcmt
