// The level operator at one point, as the one-launch-per-operation kernels evaluate it (kernels_stencil.hip and, with a
// per-point part on top, kernels_pointwise.hip): one definition, so both families keep one expression order.
#pragma once

#include "mgcmt_internal.h"

namespace mgcmt {

struct Point {
  double off;   // sum over the 8 (or 4, or 2) neighbours of a_kj v_j
  double diag;  // a_kk without the shift
};

// Neighbour sum and diagonal of the Kronecker part of the level operator at (i, j) of vector `v`.
__device__ __forceinline__ Point eval_point(const KOp& op, const double* __restrict__ v, long nc, long i, long j) {
  const double* c = v + i * nc + j;
  const bool hw = j > 0, he = j + 1 < nc;
  Point r;
  if (op.five_point) {
    const double w = hw ? c[-1] : 0.0, e = he ? c[1] : 0.0;
    double acc = op.cw * (w + e);
    if (op.cn != 0.0) acc += op.cn * (c[-nc] + c[nc]);
    r.off = acc;
    r.diag = op.c0;
    return r;
  }
  const double n = c[-nc], s = c[nc];
  const double w = hw ? c[-1] : 0.0, e = he ? c[1] : 0.0;
  const double nw = hw ? c[-nc - 1] : 0.0, ne = he ? c[-nc + 1] : 0.0;
  const double sw = hw ? c[nc - 1] : 0.0, se = he ? c[nc + 1] : 0.0;
  double off = 0.0, diag = 0.0;
  for (int m = 0; m < op.nterms; ++m) {
    const double* X = op.X[m] + i;
    const double* Y = op.Y[m] + j;
    const double xl = X[0], xd = X[op.ldx], xu = X[2 * op.ldx];
    const double yl = Y[0], yd = Y[op.ldy], yu = Y[2 * op.ldy];
    const double rn = yl * nw + yd * n + yu * ne;
    const double rc = yl * w + yu * e;
    const double rs = yl * sw + yd * s + yu * se;
    off += xl * rn + xd * rc + xu * rs;
    diag += xd * yd;
  }
  r.off = off;
  r.diag = diag;
  return r;
}

}  // namespace mgcmt
