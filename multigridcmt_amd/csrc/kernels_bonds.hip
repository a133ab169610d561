// Marching kernels of the fine level of a plan with per-point bonds (KOp::point == kPointBonds, mgcmt_plan_create_bonds), fp64, gfx950:
// H = -div(w grad) + V, a symmetric 5-point operator whose off-diagonals vary from point to point.
//
// The mapping is k_apply_march's (kernels_stencil.hip): a thread owns two adjacent columns, so every access to v, f and
// the planes D, E, S is a 16-byte one, and walks down a chunk of rows with v's rows above / at / below in registers.  S of
// the row above is carried from the previous step, so every bond is read from memory once; E(i, j - 1) of the left
// neighbour is one more 8-byte load that L1 serves, like the lateral v.  No LDS, no scratch.  The point itself is
// evaluated by bonds_point.h's functions, which the flat kernels (kernels_pointwise.hip, eval_five_bonds) call with the
// same values: a sweep gives the same bits in either form.
//
//   k_bm_apply              dst = (A - mu I) src                                      40 B per point
//   k_bm_wjacobi            one weighted-Jacobi sweep, out of place                   48 B per point (v, f, D, E, S in; v' out)
//   k_bm_parity             one red-black parity stage, in place                      36 B per point (the other parity's f, D stay)
//   k_bm_residual_restrict  F[l+1] = R (f - (A - mu I) v), V[l+1] = 0, one pass       42 B per fine point
//
// Rows -1 and nr of the vectors and of the planes are halo rows of zeros (whole grids only), columns are predicated.
#include <cstdint>

#include "bonds_point.h"
#include "mgcmt_internal.h"

namespace mgcmt {

namespace {

#ifndef MGCMT_BONDS_ROWS
#define MGCMT_BONDS_ROWS 32
#endif
constexpr int kBondRows = MGCMT_BONDS_ROWS;      // fine rows per chunk of a sweep (even)
constexpr int kBondCoarseRows = kBondRows / 2;   // coarse rows per chunk of the residual + restriction pass
constexpr long kBondMinCols = 128;

__device__ __forceinline__ double2 ld2(const double* p) { return *reinterpret_cast<const double2*>(p); }
__device__ __forceinline__ void st2(double* p, double a, double b) { *reinterpret_cast<double2*>(p) = make_double2(a, b); }

// The thread's columns j, j + 1 of the three planes and the scalars of the Kronecker part.
struct BondLevel {
  const double* __restrict__ D;
  const double* __restrict__ E;
  const double* __restrict__ S;
  long pld;
  double cn, cw, d0;
  __device__ __forceinline__ BondLevel(const KOp& op, double mu)
      : D(op.pg), E(op.pg + op.pplane), S(op.pg + 2 * op.pplane), pld(op.pld), cn(op.cn), cw(op.cw), d0(op.c0 - mu) {}
};

// Neighbour sums and diagonals of the thread's two points of one row: n, c, s = v's rows above / at / below at columns
// j, j + 1; w, e = v(i, j - 1), v(i, j + 2) (zero outside the grid); ew = E(i, j - 1) (zero outside); ee, dd = E, D of the
// row; sn, ss = S of the row above and of the row.
struct PairOp {
  double offa, dga, offb, dgb;
};
__device__ __forceinline__ PairOp eval_pair(const BondLevel& L, double2 n, double2 c, double2 s, double w, double e, double ew, double2 ee,
                                            double2 dd, double2 sn, double2 ss) {
  PairOp p;
  p.offa = bonds::neighbour_sum(L.cw, L.cn, ew, ee.x, sn.x, ss.x, w, c.y, n.x, s.x);
  p.offb = bonds::neighbour_sum(L.cw, L.cn, ee.x, ee.y, sn.y, ss.y, c.x, e, n.y, s.y);
  p.dga = bonds::diagonal(L.d0, dd.x);
  p.dgb = bonds::diagonal(L.d0, dd.y);
  return p;
}

// dst = (A - mu I) src
__global__ void __launch_bounds__(256) k_bm_apply(KGrid g, KOp op, KVec src, KVec dst, const double* __restrict__ shifts) {
  const long j = 2 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= g.nc) return;
  const int q = blockIdx.z;
  const long nc = g.nc;
  const long i0 = (long)blockIdx.y * kBondRows;
  const long i1 = i0 + kBondRows < g.nr ? i0 + kBondRows : g.nr;
  const BondLevel L(op, shifts ? shifts[q] : 0.0);
  const double* __restrict__ v = src.p + q * src.stride;
  double* __restrict__ out = dst.p + q * dst.stride;
  const bool hw = j > 0, he = j + 2 < nc;
  const long jw = hw ? j - 1 : j, je = he ? j + 2 : j + 1;  // (clamped: the value is discarded)
  double2 n = ld2(v + (i0 - 1) * nc + j), c = ld2(v + i0 * nc + j);
  double w = hw ? v[i0 * nc + jw] : 0.0, e = he ? v[i0 * nc + je] : 0.0;
  double2 sn = ld2(L.S + (i0 - 1) * L.pld + j);
#pragma unroll 2
  for (long i = i0; i < i1; ++i) {
    const double2 sr = ld2(v + (i + 1) * nc + j);
    const double wn = v[(i + 1) * nc + jw], en = v[(i + 1) * nc + je];
    const double2 dd = ld2(L.D + i * L.pld + j), ee = ld2(L.E + i * L.pld + j), ss = ld2(L.S + i * L.pld + j);
    const double ew = hw ? L.E[i * L.pld + jw] : 0.0;
    const PairOp p = eval_pair(L, n, c, sr, w, e, ew, ee, dd, sn, ss);
    st2(out + i * nc + j, bonds::applied(p.dga, c.x, p.offa), bonds::applied(p.dgb, c.y, p.offb));
    n = c;
    c = sr;
    w = hw ? wn : 0.0;
    e = he ? en : 0.0;
    sn = ss;
  }
}

// weighted Jacobi, out of place:  v' = v + w (f - (A - mu I) v) / d     (MGCMTSolver.py:193-206)
__global__ void __launch_bounds__(256) k_bm_wjacobi(KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* __restrict__ shifts, double omega) {
  const long j = 2 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= g.nc) return;
  const int q = blockIdx.z;
  const long nc = g.nc;
  const long i0 = (long)blockIdx.y * kBondRows;
  const long i1 = i0 + kBondRows < g.nr ? i0 + kBondRows : g.nr;
  const BondLevel L(op, shifts[q]);
  const double* __restrict__ v = vin.p + q * vin.stride;
  const double* __restrict__ fp = f.p + q * f.stride;
  double* __restrict__ out = vout.p + q * vout.stride;
  const bool hw = j > 0, he = j + 2 < nc;
  const long jw = hw ? j - 1 : j, je = he ? j + 2 : j + 1;
  double2 n = ld2(v + (i0 - 1) * nc + j), c = ld2(v + i0 * nc + j);
  double w = hw ? v[i0 * nc + jw] : 0.0, e = he ? v[i0 * nc + je] : 0.0;
  double2 sn = ld2(L.S + (i0 - 1) * L.pld + j);
#pragma unroll 2
  for (long i = i0; i < i1; ++i) {
    const double2 sr = ld2(v + (i + 1) * nc + j);
    const double wn = v[(i + 1) * nc + jw], en = v[(i + 1) * nc + je];
    const double2 fr = ld2(fp + i * nc + j);
    const double2 dd = ld2(L.D + i * L.pld + j), ee = ld2(L.E + i * L.pld + j), ss = ld2(L.S + i * L.pld + j);
    const double ew = hw ? L.E[i * L.pld + jw] : 0.0;
    const PairOp p = eval_pair(L, n, c, sr, w, e, ew, ee, dd, sn, ss);
    st2(out + i * nc + j, bonds::relaxed(omega, fr.x, p.dga, c.x, p.offa), bonds::relaxed(omega, fr.y, p.dgb, c.y, p.offb));
    n = c;
    c = sr;
    w = hw ? wn : 0.0;
    e = he ? en : 0.0;
    sn = ss;
  }
}

// One parity stage of the multicolour sweep, in place: the points with (i + j) % 2 == parity.  A 5-point operator does
// not couple the points of one parity, so the stage reads only values it does not write, and parity 1 followed by parity
// 0 gives the bits of the four colour launches (0,1), (1,0), (0,0), (1,1).  Of the thread's two columns one is the row's
// point of the stage — the first in rows with i % 2 == parity (a wave-uniform choice); f and D are read at that point only.
__global__ void __launch_bounds__(256) k_bm_parity(KGrid g, KOp op, KVec vv, KVec f, const double* __restrict__ shifts, double omega, int parity) {
  const long j = 2 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= g.nc) return;
  const int q = blockIdx.z;
  const long nc = g.nc;
  const long i0 = (long)blockIdx.y * kBondRows;
  const long i1 = i0 + kBondRows < g.nr ? i0 + kBondRows : g.nr;
  const BondLevel L(op, shifts[q]);
  double* v = vv.p + q * vv.stride;
  const double* __restrict__ fp = f.p + q * f.stride;
  const bool hw = j > 0, he = j + 2 < nc;
  const long jw = hw ? j - 1 : j, je = he ? j + 2 : j + 1;
  double2 n = ld2(v + (i0 - 1) * nc + j), c = ld2(v + i0 * nc + j);
  double2 sn = ld2(L.S + (i0 - 1) * L.pld + j);
#pragma unroll 2
  for (long i = i0; i < i1; ++i) {
    const double2 sr = ld2(v + (i + 1) * nc + j);
    const double2 ee = ld2(L.E + i * L.pld + j), ss = ld2(L.S + i * L.pld + j);
    if ((((int)i ^ parity) & 1) == 0) {  // column j
      const double w = hw ? v[i * nc + jw] : 0.0, ew = hw ? L.E[i * L.pld + jw] : 0.0;
      const double off = bonds::neighbour_sum(L.cw, L.cn, ew, ee.x, sn.x, ss.x, w, c.y, n.x, sr.x);
      const double dg = bonds::diagonal(L.d0, L.D[i * L.pld + j]);
      c.x = bonds::relaxed(omega, fp[i * nc + j], dg, c.x, off);
      v[i * nc + j] = c.x;
    } else {  // column j + 1
      const double e = he ? v[i * nc + je] : 0.0;
      const double off = bonds::neighbour_sum(L.cw, L.cn, ee.x, ee.y, sn.y, ss.y, c.x, e, n.y, sr.y);
      const double dg = bonds::diagonal(L.d0, L.D[i * L.pld + j + 1]);
      c.y = bonds::relaxed(omega, fp[i * nc + j + 1], dg, c.y, off);
      v[i * nc + j + 1] = c.y;
    }
    n = c;
    c = sr;
    sn = ss;
  }
}

// Residual and full-weighting restriction in one pass: fc(I, J) = sum over fine rows 2I .. 2I + 2 and columns 2J .. 2J + 2
// of (1/4, 1/2, 1/4) (x) (1/4, 1/2, 1/4) times r = f - (A - mu I) v, in k_restrict's order (kernels_stencil.hip) — the bits
// of k_pw_residual followed by k_restrict; the fine residual is not stored.  A thread owns coarse column J, fine columns
// 2J, 2J + 1; the residual of column 2J + 2 comes from the next lane (__shfl_down).  The last lane of a wave only supplies
// it: a wave produces 63 coarse columns, and waves overlap by that one lane.  Row 2I + 2 of a chunk's last coarse row is
// evaluated again by the next chunk; beyond the grid (2I + 2 == nr) it is zero.  No thread leaves before the shuffles.
__global__ void __launch_bounds__(256) k_bm_residual_restrict(KGrid g, KOp op, KVec vv, KVec f, KVec fc, KVec vc, const double* __restrict__ shifts) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long nc = g.nc, cnc = g.nc / 2, cnr = g.nr / 2;
  const long J = ((long)blockIdx.x * (blockDim.x >> 6) + wave) * 63 + lane;
  const bool live = J < cnc, writes = live && lane < 63;
  const long j = live ? 2 * J : 0;
  const int q = blockIdx.z;
  const long I0 = (long)blockIdx.y * kBondCoarseRows;
  const long I1 = I0 + kBondCoarseRows < cnr ? I0 + kBondCoarseRows : cnr;
  const BondLevel L(op, shifts[q]);
  const double* __restrict__ v = vv.p + q * vv.stride;
  const double* __restrict__ fp = f.p + q * f.stride;
  const bool hw = j > 0, he = j + 2 < nc;
  const long jw = hw ? j - 1 : j, je = he ? j + 2 : j + 1;
  double2 n = make_double2(0.0, 0.0), c = n, sn = n;
  double w = 0.0, e = 0.0;
  if (live) {
    const long i = 2 * I0;
    n = ld2(v + (i - 1) * nc + j);
    c = ld2(v + i * nc + j);
    w = hw ? v[i * nc + jw] : 0.0;
    e = he ? v[i * nc + je] : 0.0;
    sn = ld2(L.S + (i - 1) * L.pld + j);
  }
  // the residual of fine row i restricted along the row, at coarse column J; moves the row window on to row i + 1
  auto restricted_row = [&](long i) -> double {
    double ra = 0.0, rb = 0.0;
    if (live) {
      const double2 sr = ld2(v + (i + 1) * nc + j);
      const double wn = v[(i + 1) * nc + jw], en = v[(i + 1) * nc + je];
      const double2 fr = ld2(fp + i * nc + j);
      const double2 dd = ld2(L.D + i * L.pld + j), ee = ld2(L.E + i * L.pld + j), ss = ld2(L.S + i * L.pld + j);
      const double ew = hw ? L.E[i * L.pld + jw] : 0.0;
      const PairOp p = eval_pair(L, n, c, sr, w, e, ew, ee, dd, sn, ss);
      ra = bonds::residual(fr.x, p.dga, c.x, p.offa);
      rb = bonds::residual(fr.y, p.dgb, c.y, p.offb);
      n = c;
      c = sr;
      w = hw ? wn : 0.0;
      e = he ? en : 0.0;
      sn = ss;
    }
    const double rc = __shfl_down(ra, 1);
    return 0.25 * ra + 0.5 * rb + (he ? 0.25 * rc : 0.0);
  };
  double top = restricted_row(2 * I0);
  for (long I = I0; I < I1; ++I) {
    const double mid = restricted_row(2 * I + 1);
    const double bot = 2 * I + 2 < g.nr ? restricted_row(2 * I + 2) : 0.0;
    if (writes) {
      fc.p[q * fc.stride + I * cnc + J] = 0.25 * top + 0.5 * mid + 0.25 * bot;
      if (vc.p) vc.p[q * vc.stride + I * cnc + J] = 0.0;
    }
    top = bot;
  }
}

inline bool aligned16(const KVec& a) { return (((uintptr_t)a.p) & 15) == 0 && (a.stride & 1) == 0; }

inline dim3 sweep_block(long nc) { return dim3(nc >= 512 ? 256 : 64, 1, 1); }

inline dim3 sweep_grid(const KGrid& g, dim3 b, int k) {
  return dim3((unsigned)((g.nc / 2 + b.x - 1) / b.x), (unsigned)((g.nr + kBondRows - 1) / kBondRows), (unsigned)k);
}

}  // namespace

bool bonds_marching(const KGrid& g, const KOp& op) {
  return op.point == kPointBonds && op.pmarch && op.five_point && g.coarsen_rows && g.nc >= kBondMinCols && (g.nc & 1) == 0 && g.nr >= 2 && (g.nr & 1) == 0 &&
         (((uintptr_t)op.pg) & 15) == 0 && (op.pld & 1) == 0 && (op.pplane & 1) == 0;
}

// KOp::pmarch: bit 0 = the parity stages and residual + restriction march, bit 1 = the Jacobi sweep and the applied operator
// march too (hierarchy.hip, build_point_part: what MGCMT_BONDS_MARCH selects and why)
bool launch_bonds_apply(hipStream_t s, KGrid g, KOp op, KVec src, KVec dst, const double* shifts, int k) {
  if (!(op.pmarch & 2) || !bonds_marching(g, op) || !aligned16(src) || !aligned16(dst)) return false;
  const dim3 b = sweep_block(g.nc);
  hipLaunchKernelGGL(k_bm_apply, sweep_grid(g, b, k), b, 0, s, g, op, src, dst, shifts);
  return true;
}

bool launch_bonds_wjacobi(hipStream_t s, KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k) {
  if (!(op.pmarch & 2) || !bonds_marching(g, op) || !aligned16(vin) || !aligned16(f) || !aligned16(vout)) return false;
  const dim3 b = sweep_block(g.nc);
  hipLaunchKernelGGL(k_bm_wjacobi, sweep_grid(g, b, k), b, 0, s, g, op, vin, f, vout, shifts, omega);
  return true;
}

bool launch_bonds_parity(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, const double* shifts, double omega, int parity, int k) {
  if (!(op.pmarch & 1) || !bonds_marching(g, op) || !aligned16(v) || !aligned16(f)) return false;
  const dim3 b = sweep_block(g.nc);
  hipLaunchKernelGGL(k_bm_parity, sweep_grid(g, b, k), b, 0, s, g, op, v, f, shifts, omega, parity);
  return true;
}

bool launch_bonds_residual_restrict(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, KVec fc, KVec vc, const double* shifts, int k) {
  if (!(op.pmarch & 1) || !bonds_marching(g, op) || !aligned16(v) || !aligned16(f)) return false;
  const dim3 b = sweep_block(g.nc);
  const long per_block = 63 * (long)(b.x / 64), cnc = g.nc / 2, cnr = g.nr / 2;
  const dim3 grid((unsigned)((cnc + per_block - 1) / per_block), (unsigned)((cnr + kBondCoarseRows - 1) / kBondCoarseRows), (unsigned)k);
  hipLaunchKernelGGL(k_bm_residual_restrict, grid, b, 0, s, g, op, v, f, fc, vc, shifts);
  return true;
}

}  // namespace mgcmt
