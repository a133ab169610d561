// Operators with a per-point part, fp64, gfx950: H = -c Laplacian + V(x, y) with an arbitrary potential V.
//
// The Kronecker part of such an operator (the scaled Laplacian and whatever of V is separable) keeps its factors and
// their Galerkin hierarchy; the rest of V is data per point.  On the fine level it is a diagonal D; under the reference's
// transfers R = R1 (x) R1, P = P1 (x) P1 (MGCMTStencilMaker.py:27-78) the Galerkin product R D P (MGCMTSolver.py:318) is a
// symmetric 9-point stencil with variable coefficients, and R G P of such a stencil is one again.  Storage: nine planes
// per coarse level (KOp::pg, one coefficient per neighbour and point: 72 bytes per coarse point, 24 per fine point summed
// over all coarse levels), read coalesced — a thread reads its own point's nine coefficients.
//
// This file holds the Galerkin product of the per-point part (k_pw_coarsen, one thread per coarse point) and the
// one-launch-per-operation kernels of such levels: apply, weighted Jacobi, one colour stage, residual — kernels_stencil.hip's
// with the per-point part evaluated beside the Kronecker terms — and the per-point entries of the coarsest level's band
// matrix.  They run the variable 9-point levels of a cycle and are the A/B reference (MGCMT_OPT_FUSED = 0) of the fused
// pass of the fine level (Op5P, fused_kernel.h), whose bits they reproduce.  Restriction and prolongation do not see the operator.
#include "bonds_point.h"
#include "fused_kernel.h"
#include "mgcmt_internal.h"
#include "nine_point.h"

namespace mgcmt {

namespace {

// The operator at (i, j) of vector `v` for (A - mu I): neighbour sum, shifted diagonal and its reciprocal.
// Rows -1 and nr are halo rows — zeros: plans with a per-point part are whole grids (mgcmt_plan_create_pot refuses row
// strips), so the halo rows are the Dirichlet ghosts and a coefficient that multiplies one is an exact zero.  Columns
// outside the grid are predicated, and G is zero towards them.
struct PointOp {
  double off, dg, inv;
};

// Fine level: constant 5-point Kronecker part plus the diagonal D.  The expressions are the fused policy's (Op5P,
// fused_kernel.h) — explicit fma, the same order, the same reciprocal — so a fused pass and these kernels give the same bits.
__device__ __forceinline__ PointOp eval_five_diag(const KOp& op, const double* __restrict__ v, long nc, long i, long j, double mu) {
  const double* c = v + i * nc + j;
  const double w = j > 0 ? c[-1] : 0.0, e = j + 1 < nc ? c[1] : 0.0;
  PointOp r;
  r.off = fma(op.cn, c[-nc] + c[nc], op.cw * (w + e));
  r.dg = (op.c0 - mu) + op.pg[i * op.pld + j];
  r.inv = fused::fast_reciprocal(r.dg);
  return r;
}

// Fine level of a plan with per-point bonds (point == kPointBonds): constant 5-point Kronecker part plus the planes D, E, S.  The
// expressions are bonds_point.h's, which the marching kernels (kernels_bonds.hip) share: the same bits in either form.
// Row -1 of the plane S is a halo row of zeros; column -1 is predicated.
__device__ __forceinline__ PointOp eval_five_bonds(const KOp& op, const double* __restrict__ v, long nc, long i, long j, double mu) {
  const double* c = v + i * nc + j;
  const bool hw = j > 0, he = j + 1 < nc;
  const double w = hw ? c[-1] : 0.0, e = he ? c[1] : 0.0;
  const double* __restrict__ g = op.pg + i * op.pld + j;
  const double* __restrict__ ge = g + op.pplane;
  const double* __restrict__ gs = g + 2 * op.pplane;
  PointOp r;
  r.off = bonds::neighbour_sum(op.cw, op.cn, hw ? ge[-1] : 0.0, ge[0], gs[-op.pld], gs[0], w, e, c[-nc], c[nc]);
  r.dg = bonds::diagonal(op.c0 - mu, g[0]);
  r.inv = fused::fast_reciprocal(r.dg);
  return r;
}

// The values at the eight neighbours of (i, j): rows -1 / nr are the halo rows, columns outside the grid enter as zeros.
__device__ __forceinline__ nine::Nb neighbours(const double* __restrict__ c, long nc, long j) {
  const bool hw = j > 0, he = j + 1 < nc;
  nine::Nb v;
  v.n = c[-nc];
  v.s = c[nc];
  v.w = hw ? c[-1] : 0.0;
  v.e = he ? c[1] : 0.0;
  v.nw = hw ? c[-nc - 1] : 0.0;
  v.ne = he ? c[-nc + 1] : 0.0;
  v.sw = hw ? c[nc - 1] : 0.0;
  v.se = he ? c[nc + 1] : 0.0;
  return v;
}

// Fine level of a plan with a per-point 9-point stencil (mgcmt_plan_create_nine; point == kPointPlanes): constant 5-point Kronecker part
// plus the nine planes.  The expressions are nine_point.h's, which the tile kernels (kernels_nine_tile.hip) share: the same
// bits in either form.
__device__ __forceinline__ PointOp eval_five_nine(const KOp& op, const double* __restrict__ v, long nc, long i, long j, double mu) {
  const nine::Nb nb = neighbours(v + i * nc + j, nc, j);
  double g[9];
  nine::load9(g, op.pg + i * op.pld + j, op.pplane);
  const nine::Pt p = nine::five(op.cn, op.cw, op.c0 - mu, nb, g);
  PointOp r;
  r.off = p.off;
  r.dg = p.dg;
  r.inv = p.inv;
  return r;
}

// Any other level: the Kronecker terms and the per-point part (nine planes of G, or D, or D with the bonds E, S)
// evaluated from ONE set of neighbour registers, rows north to south (nine_point.h: the tile kernels evaluate a nine-plane
// level with the same functions).
__device__ __forceinline__ PointOp eval_general(const KOp& op, const double* __restrict__ v, long nc, long i, long j, double mu) {
  const nine::Nb nb = neighbours(v + i * nc + j, nc, j);
  double off = 0.0, diag = 0.0;
  nine::kron_terms(op, i, j, nb, off, diag);
  const double* __restrict__ g = op.pg + i * op.pld + j;
  if (op.point == kPointDiag) {
    diag += g[0];
  } else if (op.point == kPointBonds) {
    const double* __restrict__ ge = g + op.pplane;
    const double* __restrict__ gs = g + 2 * op.pplane;
    off += bonds::neighbour_sum(0.0, 0.0, j > 0 ? ge[-1] : 0.0, ge[0], gs[-op.pld], gs[0], nb.w, nb.e, nb.n, nb.s);
    diag += g[0];
  } else {
    double g9[9];
    nine::load9(g9, g, op.pplane);
    nine::plane_terms(g9, nb, off, diag);
  }
  PointOp r;
  r.off = off;
  r.dg = diag - mu;
  r.inv = 1.0 / r.dg;
  return r;
}

__device__ __forceinline__ PointOp eval_point_pw(const KOp& op, const double* __restrict__ v, long nc, long i, long j, double mu) {
  if (op.point == kPointBonds && op.five_point) return eval_five_bonds(op, v, nc, i, j, mu);
  if (op.point == kPointPlanes && op.five_point) return eval_five_nine(op, v, nc, i, j, mu);
  return (op.point == kPointDiag && op.five_point) ? eval_five_diag(op, v, nc, i, j, mu) : eval_general(op, v, nc, i, j, mu);
}

// dst = (A - mu I) src
__global__ void k_pw_apply(KGrid g, KOp op, KVec src, KVec dst, const double* __restrict__ shifts) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long i = (long)blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= g.nr || j >= g.nc) return;
  const int q = blockIdx.z;
  const double mu = shifts ? shifts[q] : 0.0;
  const double* v = src.p + q * src.stride;
  const PointOp p = eval_point_pw(op, v, g.nc, i, j, mu);
  dst.p[q * dst.stride + i * g.nc + j] = fma(p.dg, v[i * g.nc + j], p.off);
}

// weighted Jacobi, out of place:  v' = v + w (f - (A - mu I) v) / d     (MGCMTSolver.py:193-206)
__global__ void k_pw_wjacobi(KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* __restrict__ shifts, double omega) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long i = (long)blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= g.nr || j >= g.nc) return;
  const int q = blockIdx.z;
  const double* v = vin.p + q * vin.stride;
  const PointOp p = eval_point_pw(op, v, g.nc, i, j, shifts[q]);
  const double vc = v[i * g.nc + j];
  vout.p[q * vout.stride + i * g.nc + j] = fma(omega, (f.p[q * f.stride + i * g.nc + j] - fma(p.dg, vc, p.off)) * p.inv, vc);
}

// one colour (ca, cb) = (i%2, j%2) of the multicolour Gauss-Seidel / SOR sweep, in place
__global__ void k_pw_mc_colour(KGrid g, KOp op, KVec vv, KVec f, const double* __restrict__ shifts, double omega, int ca, int cb) {
  const long j = 2 * ((long)blockIdx.x * blockDim.x + threadIdx.x) + cb;
  const long i = 2 * ((long)blockIdx.y * blockDim.y + threadIdx.y) + ca;
  if (i >= g.nr || j >= g.nc) return;
  const int q = blockIdx.z;
  double* v = vv.p + q * vv.stride;
  const PointOp p = eval_point_pw(op, v, g.nc, i, j, shifts[q]);
  const double vc = v[i * g.nc + j];
  v[i * g.nc + j] = fma(omega, (f.p[q * f.stride + i * g.nc + j] - fma(p.dg, vc, p.off)) * p.inv, vc);
}

// r = f - (A - mu I) v                                                   (MGCMTSolver.py:315)
__global__ void k_pw_residual(KGrid g, KOp op, KVec vv, KVec f, KVec r, const double* __restrict__ shifts) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long i = (long)blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= g.nr || j >= g.nc) return;
  const int q = blockIdx.z;
  const double* v = vv.p + q * vv.stride;
  const PointOp p = eval_point_pw(op, v, g.nc, i, j, shifts[q]);
  r.p[q * r.stride + i * g.nc + j] = f.p[q * f.stride + i * g.nc + j] - fma(p.dg, v[i * g.nc + j], p.off);
}

// the per-point entries of row r of the coarsest level's band matrix, added to what k_band_assemble wrote
__global__ void k_pw_band_add(KGrid g, KOp op, KBand b) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= b.n) return;
  const int q = blockIdx.y;
  double* ab = b.ab + q * b.ab_stride;
  const long nc = g.nc;
  const long i = r / nc, j = r % nc;
  const double* gp = op.pg + i * op.pld + j;
  if (op.point == kPointDiag) {
    ab[r * b.width + b.kl] += gp[0];
    return;
  }
  if (op.point == kPointBonds) {  // a single-level plan: the diagonal and the four bonds of the row
    const double* ge = gp + op.pplane;
    const double* gs = gp + 2 * op.pplane;
    ab[r * b.width + b.kl] += gp[0];
    if (j > 0) ab[r * b.width + b.kl - 1] += ge[-1];
    if (j + 1 < nc) ab[r * b.width + b.kl + 1] += ge[0];
    if (i > 0) ab[r * b.width + b.kl - nc] += gs[-op.pld];
    if (i + 1 < g.nr) ab[r * b.width + b.kl + nc] += gs[0];
    return;
  }
  for (int di = -1; di <= 1; ++di) {
    const long ii = i + di;
    if (ii < 0 || ii >= g.nr) continue;
    for (int dj = -1; dj <= 1; ++dj) {
      const long jj = j + dj;
      if (jj < 0 || jj >= nc) continue;
      ab[r * b.width + (ii * nc + jj - r + b.kl)] += gp[(3 * (di + 1) + (dj + 1)) * op.pplane];
    }
  }
}

// coarse = R G P for the per-point part G of a fnr x fnc level (fp == 9: nine planes; fp == 1: a diagonal; fp == 3: the
// planes D, E, S of a level with bonds — west = E(i, j - 1), north = S(i - 1, j), no corner entries), one thread per
// coarse point (I, J) and all nine of its coefficients.  R1 puts (1/4, 1/2, 1/4) on fine 2I .. 2I + 2 and P1 = 2 R1^T; the
// last coarse row / column has no fine point 2I + 2 (the one-sided end of MGCMTStencilMaker.py:27-78), which the range
// checks below are.  Fixed summation order: the result does not depend on the launch geometry.
__global__ void k_pw_coarsen(long fnr, long fnc, const double* __restrict__ fine, int fp, long fld, long fplane, double* __restrict__ coarse,
                             long cld, long cplane) {
  const long J = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long I = (long)blockIdx.y * blockDim.y + threadIdx.y;
  const long cnr = fnr / 2, cnc = fnc / 2;
  if (I >= cnr || J >= cnc) return;
  const double rw[3] = {0.25, 0.5, 0.25};
  const double pw[3] = {0.5, 1.0, 0.5};
  double out[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  for (int t = 0; t < 3; ++t) {
    const long i = 2 * I + t;
    if (i >= fnr) continue;
    for (int s = 0; s < 3; ++s) {
      const long j = 2 * J + s;
      if (j >= fnc) continue;
      const double r = rw[t] * rw[s];
      for (int a = 0; a < 3; ++a) {
        const long ip = i + a - 1;
        if (ip < 0 || ip >= fnr || (fp == 1 && a != 1)) continue;
        for (int b = 0; b < 3; ++b) {
          const long jp = j + b - 1;
          if (jp < 0 || jp >= fnc || (fp == 1 && b != 1) || (fp == 3 && a != 1 && b != 1)) continue;
          double fv;
          if (fp == 1) fv = fine[i * fld + j];
          else if (fp == 9) fv = fine[(3 * a + b) * fplane + i * fld + j];
          else if (a == 1) fv = b == 1 ? fine[i * fld + j] : fine[fplane + i * fld + (b == 2 ? j : j - 1)];
          else fv = fine[2 * fplane + (a == 2 ? i : i - 1) * fld + j];
          const double gv = r * fv;
          for (int A = 0; A < 3; ++A) {
            const long Ip = I + A - 1, oi = ip - 2 * Ip;
            if (Ip < 0 || Ip >= cnr || oi < 0 || oi > 2) continue;
            for (int B = 0; B < 3; ++B) {
              const long Jp = J + B - 1, oj = jp - 2 * Jp;
              if (Jp < 0 || Jp >= cnc || oj < 0 || oj > 2) continue;
              out[A][B] += gv * (pw[oi] * pw[oj]);
            }
          }
        }
      }
    }
  }
  for (int A = 0; A < 3; ++A)
    for (int B = 0; B < 3; ++B) coarse[(3 * A + B) * cplane + I * cld + J] = out[A][B];
}

inline dim3 grid2d(long nc, long nr, int k, dim3 b) {
  return dim3((unsigned)((nc + b.x - 1) / b.x), (unsigned)((nr + b.y - 1) / b.y), (unsigned)k);
}

}  // namespace

void launch_point_apply(hipStream_t s, KGrid g, KOp op, KVec src, KVec dst, const double* shifts, int k) {
  if (launch_bonds_apply(s, g, op, src, dst, shifts, k)) return;  // the marching form of a level with bonds
  const dim3 b(64, 4, 1);
  hipLaunchKernelGGL(k_pw_apply, grid2d(g.nc, g.nr, k, b), b, 0, s, g, op, src, dst, shifts);
}

void launch_point_wjacobi(hipStream_t s, KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k) {
  if (launch_bonds_wjacobi(s, g, op, vin, f, vout, shifts, omega, k)) return;
  if (launch_nine_wjacobi(s, g, op, vin, f, vout, shifts, omega, 1, k)) return;  // the tile form of a nine-plane level
  const dim3 b(64, 4, 1);
  hipLaunchKernelGGL(k_pw_wjacobi, grid2d(g.nc, g.nr, k, b), b, 0, s, g, op, vin, f, vout, shifts, omega);
}

void launch_point_mc_colour(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, const double* shifts, double omega, int ca, int cb, int k) {
  const long rows = (g.nr - ca + 1) / 2, cols = (g.nc - cb + 1) / 2;
  if (rows <= 0 || cols <= 0) return;
  const dim3 b(64, 4, 1);
  hipLaunchKernelGGL(k_pw_mc_colour, grid2d(cols, rows, k, b), b, 0, s, g, op, v, f, shifts, omega, ca, cb);
}

void launch_point_residual(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, KVec r, const double* shifts, int k) {
  const dim3 b(64, 4, 1);
  hipLaunchKernelGGL(k_pw_residual, grid2d(g.nc, g.nr, k, b), b, 0, s, g, op, v, f, r, shifts);
}

bool launch_point_wjacobi_pair(hipStream_t s, KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k) {
  return launch_nine_wjacobi(s, g, op, vin, f, vout, shifts, omega, 2, k);
}

bool launch_point_mc_sweep(hipStream_t s, KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k) {
  return launch_nine_colour(s, g, op, vin, f, vout, shifts, omega, k);
}

bool launch_point_residual_restrict(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, KVec fc, KVec vc, const double* shifts, int k) {
  if (op.point == kPointBonds) return launch_bonds_residual_restrict(s, g, op, v, f, fc, vc, shifts, k);
  return launch_nine_residual_restrict(s, g, op, v, f, fc, vc, shifts, k);
}

void launch_point_band_add(hipStream_t s, KGrid g, KOp op, const KBand& b, int k) {
  hipLaunchKernelGGL(k_pw_band_add, dim3((unsigned)((b.n + 255) / 256), (unsigned)k), dim3(256), 0, s, g, op, b);
}

void launch_point_coarsen(hipStream_t s, long fnr, long fnc, const double* fine, int fine_planes, long fld, long fplane, double* coarse, long cld,
                          long cplane) {
  const dim3 b(64, 4, 1);
  hipLaunchKernelGGL(k_pw_coarsen, grid2d(fnc / 2, fnr / 2, 1, b), b, 0, s, fnr, fnc, fine, fine_planes, fld, fplane, coarse, cld, cplane);
}

}  // namespace mgcmt
