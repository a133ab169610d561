// Instantiations of the two-level fused passes (fused2_kernel.h): a constant 5-point level with weighted Jacobi and
// its Galerkin coarsening (Op9c) below it, 2 sweeps per leg on level l+1, 2 post-smoothing sweeps on level l.
#include "fused2_kernel.h"

namespace mgcmt {

void launch_fused2(hipStream_t s, int up, int nf, int zero_in, const KOp& op0, const KOp& op1, long nr, long nc, long cnr, long cnc,
                   long c2nc, KVec v, KVec f, KVec vout, KVec f1, KVec c2, const double* shifts, double omega, int k, long rows_override,
                   double* fcarry) {
  using namespace fused;
  Fused2Args a{};
  a.fine.c0 = op0.c0;
  a.fine.cn = op0.cn;
  a.fine.cw = op0.cw;
  a.fine.shifts = shifts;
  a.fine.omega = omega;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) a.coarse.c9[i][j] = op1.c9[i][j];
    a.coarse.c9row[i] = op1.c9row[i];
    a.coarse.c9col[i] = op1.c9col[i];
  }
  a.coarse.c9corner = op1.c9corner;
  a.coarse.last_row = cnr - 1;
  a.coarse.shifts = shifts;
  a.coarse.omega = omega;
  a.v = v.p;
  a.f = f.p;
  a.vout = vout.p;
  a.f1 = f1.p;
  a.c2 = c2.p;
  a.s0 = v.stride;
  a.s1 = f1.stride;
  a.s2 = c2.stride;
  a.nr = (int)nr;
  a.nc = (int)nc;
  a.cnr = (int)cnr;
  a.cnc = (int)cnc;
  a.c2nc = (int)c2nc;
  a.fcarry = fcarry;
  if (fcarry) {
    // (cycle.hip asks for a carrying pass only as an up pass on a nonzero iterate)
    if (nf == 1) launch_two<true, 1, false, true>(s, a, k, rows_override);
    else launch_two<true, 2, false, true>(s, a, k, rows_override);
  } else if (up) {
    if (nf == 1) zero_in ? launch_two<true, 1, true>(s, a, k, rows_override) : launch_two<true, 1, false>(s, a, k, rows_override);
    else zero_in ? launch_two<true, 2, true>(s, a, k, rows_override) : launch_two<true, 2, false>(s, a, k, rows_override);
  } else {
    if (nf == 1) zero_in ? launch_two<false, 1, true>(s, a, k, rows_override) : launch_two<false, 1, false>(s, a, k, rows_override);
    else zero_in ? launch_two<false, 2, true>(s, a, k, rows_override) : launch_two<false, 2, false>(s, a, k, rows_override);
  }
}

}  // namespace mgcmt
