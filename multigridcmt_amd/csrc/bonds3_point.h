// One point of a 3-D level with per-point bonds (K3Op::point == 3, mgcmt_plan_create3d_bonds): a constant 7-point Kronecker
// part plus the planes D, Bx, By, Bz.  The flat kernels (kernels_3d_point.hip) and the marching kernels
// (kernels_3d_bonds.hip) compute every point with THESE functions from the same values — the same sums, the same fma order
// (p7_av's: z-, z+, y-, y+, x-, x+), the same reciprocal of c0 + D - mu — so their sweeps give the same bits.
// A bond towards a point outside the grid is passed as zero, and so is that point's value.
#pragma once
#include "fused_kernel.h"
#include "mgcmt_internal.h"

namespace mgcmt {
namespace b7 {

struct Coef {
  double zm, zp, ym, yp, xm, xp;
};

// the six off-diagonal entries of the point's row: bzm = Bz(z-1, y, x), bzp = Bz(z, y, x), and so on
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

}  // namespace b7
}  // namespace mgcmt
