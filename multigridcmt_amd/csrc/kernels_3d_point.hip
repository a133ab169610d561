// 3-D operators with a per-point part, fp64, gfx950: H = -c Laplacian + V(x, y, z) with an arbitrary potential V, or
// H = -div(w grad) + V with a position-dependent inverse effective mass w.
//
// As in 2-D (kernels_pointwise.hip) the Kronecker part keeps its factors and their Galerkin hierarchy and the rest is data per
// point.  On the fine level that is a diagonal D (K3Op::point == kPointDiag, mgcmt_plan_create3d_pot: one vector, 8 B per point,
// read at the index of the right-hand side) or the four planes D, Bx, By, Bz, pplane apart (kPointBonds,
// mgcmt_plan_create3d_bonds: Bx / By / Bz are added to the two entries between a point and its neighbour at x + 1 / y + 1 / z + 1).
// Under R = R1 (x) R1 (x) R1, P = P1 (x) P1 (x) P1 either becomes a 27-point stencil with variable coefficients on every level
// below — 27 planes per level (kPointPlanes; K3Op::pg; a thread reads its own point's coefficients, coalesced): 216 B per coarse
// point, 27/7 of a fine vector summed over all coarse levels (about 4 GiB at 512^3).
//
// This file holds
//   - the Galerkin product of the per-point part (k3p_coarsen, one thread per coarse point and all 27 of its coefficients;
//     the diagonal, the four planes of a level with bonds or 27 planes as its source);
//   - flat kernels, one thread per point, for any such level: apply, weighted Jacobi, one colour stage, residual + full
//     weighting, prolongation + correction + first Jacobi sweep, the per-point entries of the coarsest level's band matrix.
//     They evaluate the Kronecker part with eval3's expressions (kernels_3d.hip) and the planes from the same neighbour registers;
//   - marching kernels for the fine level — constant 7-point Kronecker part plus D, or plus D and bonds; 7/8 of all points —:
//     kernels_3d.hip's 64 x 4 tile and 32-plane chunks with the planes z-1, z, z+1 of the thread's column in registers, no LDS,
//     no halo planes (all three directions are predicated), templated on whether the level has bonds.
// The flat and the marching form of the fine level compute every point with ONE set of inline functions (seven_point.h: the
// same fma order, the same reciprocal of c0 + D - mu), so their sweeps give the same bits.  Which passes march is
// point3_marching (K3Op::pmarch, hierarchy.hip); MGCMT_3D_POINT_MARCH=0 selects the flat form.
// A level of 27 planes — the Galerkin levels, and level 0 of mgcmt_plan_create3d_stencil, whose Kronecker part is a constant
// 7-point operator — computes a point with stencil27_point.h's functions; its colour stages and its residual + restriction
// have a second form in kernels_3d_stencil.hip (stencil3_tiled), which the launchers below try first.
#include "kernels_3d_common.h"
#include "mgcmt_internal.h"
#include "seven_point.h"
#include "stencil27_point.h"

namespace mgcmt {

namespace {

using namespace k3;

// the fine level's own form: a constant 7-point Kronecker part plus a per-point row (seven_point.h)
__host__ __device__ __forceinline__ bool seven_point_row(const K3Op& op) {
  return op.seven && (op.point == kPointDiag || op.point == kPointBonds);
}

// ---- any level with a per-point part, one point -------------------------------------------------------------------
struct PEval {
  double av;  // ((A - mu I) w) at the point
  double dg;  // a_ii - mu
};

// w(zz, yy, xx): the vector at an in-grid point (a load, or v + P e formed on the fly)
template <class W>
__device__ __forceinline__ PEval eval3p(const K3Op& op, W&& w, long z, long y, long x, double mu) {
  const long n = op.n, n2 = n * n;
  const long idx = z * n2 + y * n + x;
  const bool zm = z > 0, zp = z + 1 < n, ym = y > 0, yp = y + 1 < n, xm = x > 0, xp = x + 1 < n;
  PEval r;
  // the fine level's own forms, constant 7-point part + D and the same + bonds (seven_point.h): neighbours outside the grid are
  // passed as zeros, a bond towards outside is a predicated zero.  (Two branches that differ in the coefficient source only: as
  // one branch every red-black cycle measured 2 % slower at 256^3, see profiles/r11_fold_3d_point_bonds.md)
  if (op.point == kPointDiag && op.seven) {
    r.dg = p7::dg(op, op.pg[idx], mu);
    r.av = p7::av(p7::coef(op), r.dg, w(z, y, x), zm ? w(z - 1, y, x) : 0.0, zp ? w(z + 1, y, x) : 0.0, ym ? w(z, y - 1, x) : 0.0,
                  yp ? w(z, y + 1, x) : 0.0, xm ? w(z, y, x - 1) : 0.0, xp ? w(z, y, x + 1) : 0.0);
    return r;
  }
  if (op.point == kPointBonds && op.seven) {
    const double* __restrict__ g = op.pg + idx;
    const long pl = op.pplane;
    const p7::Coef c = p7::coef(op, zm ? g[3 * pl - n2] : 0.0, g[3 * pl], ym ? g[2 * pl - n] : 0.0, g[2 * pl], xm ? g[pl - 1] : 0.0, g[pl]);
    r.dg = p7::dg(op, g[0], mu);
    r.av = p7::av(c, r.dg, w(z, y, x), zm ? w(z - 1, y, x) : 0.0, zp ? w(z + 1, y, x) : 0.0, ym ? w(z, y - 1, x) : 0.0,
                  yp ? w(z, y + 1, x) : 0.0, xm ? w(z, y, x - 1) : 0.0, xp ? w(z, y, x + 1) : 0.0);
    return r;
  }
  // 27 planes, on a constant 7-point part or on general terms (stencil27_point.h)
  if (op.point == kPointPlanes) {
    const p27::Eval e = p27::point(op, w, z, y, x, mu);
    r.av = e.av;
    r.dg = e.dg;
    return r;
  }
  // the 27 neighbours once, zeros outside the grid
  double wn[3][3][3];
  p27::neighbours(w, n, z, y, x, wn);
  // Kronecker part: a(dz, dy, dx) = sum_m X_m[dz](z) Y_m[dy](y) Z_m[dx](x), summed as eval3 does
  double acc = 0.0, diag = 0.0;
  p27::kronecker(op, z, y, x, wn, acc, diag);
  const double* __restrict__ g = op.pg + idx;
  if (op.point == kPointDiag) {  // a diagonal on top of general terms
    acc += g[0] * wn[1][1][1];
    diag += g[0];
  } else if (op.point == kPointBonds) {  // a diagonal and bonds on top of general terms: the six neighbour products and the centre
    const long pl = op.pplane;
    double pa = g[0] * wn[1][1][1];
    pa += (zm ? g[3 * pl - n2] : 0.0) * wn[0][1][1];
    pa += g[3 * pl] * wn[2][1][1];
    pa += (ym ? g[2 * pl - n] : 0.0) * wn[1][0][1];
    pa += g[2 * pl] * wn[1][2][1];
    pa += (xm ? g[pl - 1] : 0.0) * wn[1][1][0];
    pa += g[pl] * wn[1][1][2];
    acc += pa;
    diag += g[0];
  }
  // acc holds the unshifted sum, centre included
  r.dg = diag - mu;
  r.av = acc - mu * wn[1][1][1];
  return r;
}

__device__ __forceinline__ double relax3p(const K3Op& op, const PEval& e, double omega, double f, double vc) {
  if (seven_point_row(op)) return p7::relax(omega, f, e.av, e.dg, vc);
  if (op.point == kPointPlanes) return p27::relax(op, omega, f, p27::Eval{e.av, e.dg}, vc);
  return vc + omega * (f - e.av) / e.dg;
}

struct Load {
  const double* v;
  long n;
  __device__ __forceinline__ double operator()(long z, long y, long x) const { return v[(z * n + y) * n + x]; }
};

struct LoadProlonged {  // v + P e
  const double* v;
  const double* e;
  long n;
  __device__ __forceinline__ double operator()(long z, long y, long x) const { return v[(z * n + y) * n + x] + prolong_at(e, n / 2, z, y, x); }
};

// ---- flat kernels --------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kFlatThreads) k3p_apply(K3Op op, KVec src, KVec dst, const double* __restrict__ shifts) {
  const long n = op.n, N = n * n * n;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int q = blockIdx.y;
  const long z = i / (n * n), y = (i / n) % n, x = i % n;
  const PEval e = eval3p(op, Load{src.p + q * src.stride, n}, z, y, x, shifts[q]);
  dst.p[q * dst.stride + i] = e.av;
}

__global__ void __launch_bounds__(kFlatThreads) k3p_wjacobi(K3Op op, KVec vin, KVec f, KVec vout, const double* __restrict__ shifts,
                                                           double omega) {
  const long n = op.n, N = n * n * n;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int q = blockIdx.y;
  const double* v = vin.p + q * vin.stride;
  const long z = i / (n * n), y = (i / n) % n, x = i % n;
  const PEval e = eval3p(op, Load{v, n}, z, y, x, shifts[q]);
  vout.p[q * vout.stride + i] = relax3p(op, e, omega, f.p[q * f.stride + i], v[i]);
}

// one colour of the multicolour sweep, in place (k3_colour's conventions: cz < 0 selects the parity class cy)
__global__ void __launch_bounds__(kFlatThreads) k3p_colour(K3Op op, KVec vv, KVec f, const double* __restrict__ shifts, double omega,
                                                          int cz, int cy, int cx) {
  const long n = op.n, N = n * n * n;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const long z = i / (n * n), y = (i / n) % n, x = i % n;
  if (cz < 0) {
    if (((x + y + z) & 1) != cy) return;
  } else if ((z & 1) != cz || (y & 1) != cy || (x & 1) != cx) {
    return;
  }
  const int q = blockIdx.y;
  double* v = vv.p + q * vv.stride;
  const PEval e = eval3p(op, Load{v, n}, z, y, x, shifts[q]);
  v[i] = relax3p(op, e, omega, f.p[q * f.stride + i], v[i]);
}

// fc <- R (f - (A - mu I) v), vc <- 0: one thread per coarse point (k3_restrict's weights and summation order)
__global__ void __launch_bounds__(kFlatThreads) k3p_residual_restrict(K3Op op, KVec v, KVec f, KVec fc, KVec vc,
                                                                     const double* __restrict__ shifts) {
  const long n = op.n, nc = n / 2, Nc = nc * nc * nc;
  const long I = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (I >= Nc) return;
  const int q = blockIdx.y;
  const double* vq = v.p + q * v.stride;
  const double* fq = f.p + q * f.stride;
  const double mu = shifts[q];
  const long Z = I / (nc * nc), Y = (I / nc) % nc, X = I % nc;
  double acc = 0.0;
  for (int a = 0; a < 3; ++a) {
    const long z = 2 * Z + a;
    if (z >= n) continue;
    double pa = 0.0;
    for (int b = 0; b < 3; ++b) {
      const long y = 2 * Y + b;
      if (y >= n) continue;
      double pb = 0.0;
      for (int c = 0; c < 3; ++c) {
        const long x = 2 * X + c;
        if (x >= n) continue;
        const PEval e = eval3p(op, Load{vq, n}, z, y, x, mu);
        pb += (c == 1 ? 0.5 : 0.25) * (fq[(z * n + y) * n + x] - e.av);
      }
      pa += (b == 1 ? 0.5 : 0.25) * pb;
    }
    acc += (a == 1 ? 0.5 : 0.25) * pa;
  }
  fc.p[q * fc.stride + I] = acc;
  vc.p[q * vc.stride + I] = 0.0;
}

// prolongation + correction fused with one weighted-Jacobi sweep: w = v + P e formed on the fly, only vout written
__global__ void __launch_bounds__(kFlatThreads) k3p_prolong_jacobi(K3Op op, KVec e, KVec vin, KVec f, KVec vout,
                                                                  const double* __restrict__ shifts, double omega) {
  const long n = op.n, N = n * n * n;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int q = blockIdx.y;
  const long z = i / (n * n), y = (i / n) % n, x = i % n;
  const LoadProlonged w{vin.p + q * vin.stride, e.p + q * e.stride, n};
  const PEval ev = eval3p(op, w, z, y, x, shifts[q]);
  vout.p[q * vout.stride + i] = relax3p(op, ev, omega, f.p[q * f.stride + i], w(z, y, x));
}

// the per-point entries of row r of the coarsest level's band matrix, added to what k3_band_assemble wrote
__global__ void k3p_band_add(K3Op op, KBand b) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= b.n) return;
  const int q = blockIdx.y;
  double* ab = b.ab + q * b.ab_stride;
  const long n = op.n, n2 = n * n;
  const long z = r / n2, y = (r / n) % n, x = r % n;
  if (op.point == kPointDiag) {
    ab[r * b.width + b.kl] += op.pg[r];
    return;
  }
  if (op.point == kPointBonds) {  // D and the six bonds (a plan whose fine level is also its coarsest)
    const long pl = op.pplane;
    double* row = ab + r * b.width + b.kl;
    row[0] += op.pg[r];
    if (x > 0) row[-1] += op.pg[pl + r - 1];
    if (x + 1 < n) row[1] += op.pg[pl + r];
    if (y > 0) row[-n] += op.pg[2 * pl + r - n];
    if (y + 1 < n) row[n] += op.pg[2 * pl + r];
    if (z > 0) row[-n2] += op.pg[3 * pl + r - n2];
    if (z + 1 < n) row[n2] += op.pg[3 * pl + r];
    return;
  }
  for (int a = -1; a <= 1; ++a)
    for (int bb = -1; bb <= 1; ++bb)
      for (int c = -1; c <= 1; ++c) {
        const long zz = z + a, yy = y + bb, xx = x + c;
        if (zz < 0 || zz >= n || yy < 0 || yy >= n || xx < 0 || xx >= n) continue;
        const long col = zz * n2 + yy * n + xx;
        ab[r * b.width + (col - r + b.kl)] += op.pg[(9 * (a + 1) + 3 * (bb + 1) + (c + 1)) * op.pplane + r];
      }
}

// ---- Galerkin product of the per-point part ---------------------------------------------------------------------------
// the weights of P1 that take coarse I - 1, I, I + 1 to fine point ip (P1 = 2 R1^T puts 1/2, 1, 1/2 on fine 2J .. 2J + 2);
// zero where the coarse point does not exist or does not reach ip
__device__ __forceinline__ void prolong_weights(long ip, long I, long cn, double* w) {
#pragma unroll
  for (int A = 0; A < 3; ++A) {
    const long Ip = I + A - 1, o = ip - 2 * Ip;
    w[A] = (Ip >= 0 && Ip < cn && o >= 0 && o <= 2) ? (o == 1 ? 1.0 : 0.5) : 0.0;
  }
}

// coarse = R G P for the per-point part G of a level of fn^3 points (fp == 27: 27 planes; fp == 1: a diagonal; fp == 4: the
// planes D, Bx, By, Bz of a level with bonds — the centre from D, the six axis neighbours from the bond the two points share), one thread
// per coarse point (Z, Y, X) and all 27 of its coefficients.  R1 puts (1/4, 1/2, 1/4) on fine 2I .. 2I + 2; the last coarse
// plane / row / column has no fine point 2I + 2 (the one-sided end of the reference's transfers), which the range checks
// are.  Fixed summation order: the result does not depend on the launch geometry.  Every weight is a power of two, so only
// the accumulation rounds.
__global__ void __launch_bounds__(kFlatThreads) k3p_coarsen(long fn, const double* __restrict__ fine, int fp, long fplane,
                                                           double* __restrict__ coarse, long cplane) {
  const long cn = fn / 2, Nc = cn * cn * cn;
  const long I = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (I >= Nc) return;
  const long Z = I / (cn * cn), Y = (I / cn) % cn, X = I % cn;
  double out[27];
#pragma unroll
  for (int j = 0; j < 27; ++j) out[j] = 0.0;
  for (int t = 0; t < 3; ++t) {
    const long z = 2 * Z + t;
    if (z >= fn) continue;
    for (int s = 0; s < 3; ++s) {
      const long y = 2 * Y + s;
      if (y >= fn) continue;
      for (int u = 0; u < 3; ++u) {
        const long x = 2 * X + u;
        if (x >= fn) continue;
        const double r = (t == 1 ? 0.5 : 0.25) * (s == 1 ? 0.5 : 0.25) * (u == 1 ? 0.5 : 0.25);
        const long fi = (z * fn + y) * fn + x;
        for (int a = 0; a < 3; ++a) {
          const long zp = z + a - 1;
          if (zp < 0 || zp >= fn || (fp == 1 && a != 1)) continue;
          double wz[3];
          prolong_weights(zp, Z, cn, wz);
          for (int b = 0; b < 3; ++b) {
            const long yp = y + b - 1;
            if (yp < 0 || yp >= fn || (fp == 1 && b != 1) || (fp == 4 && a != 1 && b != 1)) continue;
            double wy[3];
            prolong_weights(yp, Y, cn, wy);
            for (int c = 0; c < 3; ++c) {
              const long xp = x + c - 1;
              if (xp < 0 || xp >= fn || (fp == 1 && c != 1) || (fp == 4 && (a != 1 || b != 1) && c != 1)) continue;
              double wx[3];
              prolong_weights(xp, X, cn, wx);
              double gf;
              if (fp == 1)
                gf = fine[fi];
              else if (fp == 4)  // the bond lies with the lower of the two points
                gf = a != 1   ? fine[3 * fplane + (a == 0 ? fi - fn * fn : fi)]
                     : b != 1 ? fine[2 * fplane + (b == 0 ? fi - fn : fi)]
                     : c != 1 ? fine[fplane + (c == 0 ? fi - 1 : fi)]
                              : fine[fi];
              else
                gf = fine[(9 * a + 3 * b + c) * fplane + fi];
              const double gv = r * gf;
#pragma unroll
              for (int A = 0; A < 3; ++A) {
                if (wz[A] == 0.0) continue;
#pragma unroll
                for (int B = 0; B < 3; ++B) {
                  if (wy[B] == 0.0) continue;
#pragma unroll
                  for (int C = 0; C < 3; ++C)
                    if (wx[C] != 0.0) out[9 * A + 3 * B + C] += gv * (wz[A] * wy[B] * wx[C]);
                }
              }
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 27; ++j) coarse[j * cplane + I] = out[j];
}

// ---- marching kernels: constant 7-point part + per-point row, n a multiple of 64 ---------------------------------------
// k3m_sweep's geometry (kernels_3d.hip) with D as a fourth stream, read once per updated point at the address of f.  BONDS:
// Bx, By, Bz are three more streams read there; Bx(x-1) and By(y-1) are one more 8-byte load each from the same or the
// neighbouring row's cache line; Bz(z-1) is carried from the previous plane step where every plane is updated (the Jacobi and
// the prolongation pass: a predicated load of its own at a chunk's first plane) and a load of its own in a parity stage, which
// updates every other point.  A bond towards a point outside the grid is a predicated zero.
// stage 0: weighted Jacobi vin -> vout; stage 1: the parity class (x + y + z) % 2 == par of the red-black sweep, in place
// (exact on a 7-point operator with any coefficients: same-parity points do not couple)
template <bool BONDS, int STAGE>
__global__ void __launch_bounds__(kTileX* kTileY) k3pm_sweep(K3Op op, KVec vin, KVec f, KVec vout, const double* __restrict__ shifts,
                                                           double omega, int par, int nchunks) {
  const long n = op.n, n2 = n * n;
  const long x = (long)blockIdx.x * kTileX + threadIdx.x;
  const long y = (long)blockIdx.y * kTileY + threadIdx.y;
  const int q = blockIdx.z / nchunks;
  const long z0 = (long)(blockIdx.z % nchunks) * kChunkZ;
  const double* v = vin.p + q * vin.stride;
  const double* fq = f.p + q * f.stride;
  const double* __restrict__ dq = op.pg;
  const double* __restrict__ bxq = op.pg + op.pplane;  // (the three bond streams: read only where BONDS)
  const double* __restrict__ byq = op.pg + 2 * op.pplane;
  const double* __restrict__ bzq = op.pg + 3 * op.pplane;
  double* out = vout.p + q * vout.stride;
  const double mu = shifts[q];
  const bool xm = x > 0, xp = x + 1 < n, ym = y > 0, yp = y + 1 < n;
  const long col = y * n + x;
  double vm = z0 > 0 ? v[(z0 - 1) * n2 + col] : 0.0;
  double vc = v[z0 * n2 + col];
  double bzm = 0.0;  // Bz(z-1) of the column
  if constexpr (BONDS && STAGE == 0) bzm = z0 > 0 ? bzq[(z0 - 1) * n2 + col] : 0.0;
  for (int t = 0; t < kChunkZ; ++t) {
    const long z = z0 + t;
    const long i = z * n2 + col;
    const double vp = z + 1 < n ? v[i + n2] : 0.0;
    if (STAGE == 0 || (((x + y + z) & 1) == par)) {
      const double* c = v + i;
      p7::Coef cf;
      if constexpr (BONDS) {
        const double bzp = bzq[i];
        if (STAGE != 0) bzm = z > 0 ? bzq[i - n2] : 0.0;
        cf = p7::coef(op, bzm, bzp, ym ? byq[i - n] : 0.0, byq[i], xm ? bxq[i - 1] : 0.0, bxq[i]);
        if (STAGE == 0) bzm = bzp;
      } else {
        cf = p7::coef(op);
      }
      const double dg = p7::dg(op, dq[i], mu);
      const double av = p7::av(cf, dg, vc, vm, vp, ym ? c[-n] : 0.0, yp ? c[n] : 0.0, xm ? c[-1] : 0.0, xp ? c[1] : 0.0);
      out[i] = p7::relax(omega, fq[i], av, dg, vc);
    }
    vm = vc;
    vc = vp;
  }
}

// residual + restriction, marching: a thread owns one coarse x-y column (X, Y) of a chunk of coarse planes and keeps the
// x-y weighted residual of the fine plane 2Z + 2 (shared with the next coarse plane) in a register.  k3m_residual_restrict's
// structure: v's planes are NOT held in registers here — every plane's nine residuals are re-formed from (cached) loads, the
// bonds among them
template <bool BONDS>
__global__ void __launch_bounds__(kTileX* kTileY) k3pm_residual_restrict(K3Op op, KVec v, KVec f, KVec fc, KVec vc,
                                                                       const double* __restrict__ shifts, int nchunks) {
  const long n = op.n, n2 = n * n, nc = n / 2, nc2 = nc * nc;
  const long X = (long)blockIdx.x * kTileX + threadIdx.x;
  const long Y = (long)blockIdx.y * kTileY + threadIdx.y;
  if (X >= nc || Y >= nc) return;
  const int q = blockIdx.z / nchunks;
  const long Z0 = (long)(blockIdx.z % nchunks) * (kChunkZ / 2);
  const double* vq = v.p + q * v.stride;
  const double* fq = f.p + q * f.stride;
  const double* __restrict__ dq = op.pg;
  const long pl = op.pplane;
  const double mu = shifts[q];
  // x-y full weighting of the residual on fine plane z
  auto plane = [&](long z) {
    double pa = 0.0;
    for (int b = 0; b < 3; ++b) {
      const long y = 2 * Y + b;
      if (y >= n) continue;
      double pb = 0.0;
      for (int c = 0; c < 3; ++c) {
        const long x = 2 * X + c;
        if (x >= n) continue;
        const long i = z * n2 + y * n + x;
        const double* p = vq + i;
        const double* g = dq + i;
        p7::Coef cf;
        if constexpr (BONDS)
          cf = p7::coef(op, z > 0 ? g[3 * pl - n2] : 0.0, g[3 * pl], y > 0 ? g[2 * pl - n] : 0.0, g[2 * pl], x > 0 ? g[pl - 1] : 0.0, g[pl]);
        else
          cf = p7::coef(op);
        const double dg = p7::dg(op, g[0], mu);
        const double av = p7::av(cf, dg, p[0], z > 0 ? p[-n2] : 0.0, z + 1 < n ? p[n2] : 0.0, y > 0 ? p[-n] : 0.0, y + 1 < n ? p[n] : 0.0,
                                 x > 0 ? p[-1] : 0.0, x + 1 < n ? p[1] : 0.0);
        pb += (c == 1 ? 0.5 : 0.25) * (fq[i] - av);
      }
      pa += (b == 1 ? 0.5 : 0.25) * pb;
    }
    return pa;
  };
  double lo = plane(2 * Z0);
  for (int t = 0; t < kChunkZ / 2; ++t) {
    const long Z = Z0 + t;
    const double mid = plane(2 * Z + 1);
    const double hi = 2 * Z + 2 < n ? plane(2 * Z + 2) : 0.0;
    fc.p[q * fc.stride + Z * nc2 + Y * nc + X] = 0.25 * lo + 0.5 * mid + 0.25 * hi;
    vc.p[q * vc.stride + Z * nc2 + Y * nc + X] = 0.0;
    lo = hi;
  }
}

// prolongation + correction + one weighted-Jacobi sweep, marching: w = v + P e of the planes z-1, z, z+1 of the thread's
// column in registers
template <bool BONDS>
__global__ void __launch_bounds__(kTileX* kTileY) k3pm_prolong_jacobi(K3Op op, KVec e, KVec vin, KVec f, KVec vout,
                                                                    const double* __restrict__ shifts, double omega, int nchunks) {
  const long n = op.n, n2 = n * n;
  const long x = (long)blockIdx.x * kTileX + threadIdx.x;
  const long y = (long)blockIdx.y * kTileY + threadIdx.y;
  const int q = blockIdx.z / nchunks;
  const long z0 = (long)(blockIdx.z % nchunks) * kChunkZ;
  const LoadProlonged w{vin.p + q * vin.stride, e.p + q * e.stride, n};
  const double* fq = f.p + q * f.stride;
  const double* __restrict__ dq = op.pg;
  const double* __restrict__ bxq = op.pg + op.pplane;  // (the three bond streams: read only where BONDS)
  const double* __restrict__ byq = op.pg + 2 * op.pplane;
  const double* __restrict__ bzq = op.pg + 3 * op.pplane;
  double* out = vout.p + q * vout.stride;
  const double mu = shifts[q];
  const bool xm = x > 0, xp = x + 1 < n, ym = y > 0, yp = y + 1 < n;
  const long col = y * n + x;
  double wm = z0 > 0 ? w(z0 - 1, y, x) : 0.0;
  double wc = w(z0, y, x);
  double bzm = 0.0;  // Bz(z-1) of the column
  if constexpr (BONDS) bzm = z0 > 0 ? bzq[(z0 - 1) * n2 + col] : 0.0;
  for (int t = 0; t < kChunkZ; ++t) {
    const long z = z0 + t;
    const long i = z * n2 + col;
    const double wp = z + 1 < n ? w(z + 1, y, x) : 0.0;
    p7::Coef cf;
    if constexpr (BONDS) {
      const double bzp = bzq[i];
      cf = p7::coef(op, bzm, bzp, ym ? byq[i - n] : 0.0, byq[i], xm ? bxq[i - 1] : 0.0, bxq[i]);
      bzm = bzp;
    } else {
      cf = p7::coef(op);
    }
    const double dg = p7::dg(op, dq[i], mu);
    const double av = p7::av(cf, dg, wc, wm, wp, ym ? w(z, y - 1, x) : 0.0, yp ? w(z, y + 1, x) : 0.0, xm ? w(z, y, x - 1) : 0.0,
                             xp ? w(z, y, x + 1) : 0.0);
    out[i] = p7::relax(omega, fq[i], av, dg, wc);
    wm = wc;
    wc = wp;
  }
}

dim3 march_grid(const K3Op& op, int k) {
  return dim3((unsigned)(op.n / kTileX), (unsigned)(op.n / kTileY), (unsigned)(op.n / kChunkZ * k));
}

}  // namespace

int point3_marching(const K3Op& op) { return seven_point_row(op) && op.n >= kTileX && op.n % kTileX == 0 ? op.pmarch : 0; }

void launch3p_apply(hipStream_t s, const K3Op& op, KVec src, KVec dst, const double* shifts, int k) {
  hipLaunchKernelGGL(k3p_apply, flat_grid(op.n * op.n * op.n, k), dim3(kFlatThreads), 0, s, op, src, dst, shifts);
}

void launch3p_wjacobi(hipStream_t s, const K3Op& op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k) {
  if (point3_marching(op) & kMarch3Jacobi) {
    const auto kern = op.point == kPointBonds ? k3pm_sweep<true, 0> : k3pm_sweep<false, 0>;
    hipLaunchKernelGGL(kern, march_grid(op, k), dim3(kTileX, kTileY), 0, s, op, vin, f, vout, shifts, omega, 0, (int)(op.n / kChunkZ));
    return;
  }
  hipLaunchKernelGGL(k3p_wjacobi, flat_grid(op.n * op.n * op.n, k), dim3(kFlatThreads), 0, s, op, vin, f, vout, shifts, omega);
}

void launch3p_mc_sweep(hipStream_t s, const K3Op& op, KVec v, KVec f, const double* shifts, double omega, int k) {
  // the order of launch3_mc_sweep: odd coordinate sum first
  static const int order[8][3] = {{0, 0, 1}, {0, 1, 0}, {1, 0, 0}, {1, 1, 1}, {0, 0, 0}, {0, 1, 1}, {1, 0, 1}, {1, 1, 0}};
  if (seven_point_row(op)) {  // a 7-point operator with any coefficients does not couple points of one parity: two stages
    const auto kern = op.point == kPointBonds ? k3pm_sweep<true, 1> : k3pm_sweep<false, 1>;
    for (int par = 1; par >= 0; --par) {
      if (point3_marching(op) & kMarch3Parity)
        hipLaunchKernelGGL(kern, march_grid(op, k), dim3(kTileX, kTileY), 0, s, op, v, f, v, shifts, omega, par, (int)(op.n / kChunkZ));
      else
        hipLaunchKernelGGL(k3p_colour, flat_grid(op.n * op.n * op.n, k), dim3(kFlatThreads), 0, s, op, v, f, shifts, omega, -1, par, 0);
    }
    return;
  }
  for (int c = 0; c < 8; ++c) {
    if (launch3n_colour(s, op, v, f, shifts, omega, order[c][0], order[c][1], order[c][2], k)) continue;  // (a 27-plane level's own stage)
    hipLaunchKernelGGL(k3p_colour, flat_grid(op.n * op.n * op.n, k), dim3(kFlatThreads), 0, s, op, v, f, shifts, omega, order[c][0], order[c][1],
                       order[c][2]);
  }
}

void launch3p_residual_restrict(hipStream_t s, const K3Op& op, KVec v, KVec f, KVec fc, KVec vc, const double* shifts, int k) {
  const long nc = op.n / 2;
  if (point3_marching(op) & kMarch3Residual) {
    const int nch = (int)(op.n / kChunkZ);
    const auto kern = op.point == kPointBonds ? k3pm_residual_restrict<true> : k3pm_residual_restrict<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((nc + kTileX - 1) / kTileX), (unsigned)((nc + kTileY - 1) / kTileY), (unsigned)(nch * k)),
                       dim3(kTileX, kTileY), 0, s, op, v, f, fc, vc, shifts, nch);
    return;
  }
  if (launch3n_residual_restrict(s, op, v, f, fc, vc, shifts, k)) return;  // (a 27-plane level's own pass)
  hipLaunchKernelGGL(k3p_residual_restrict, flat_grid(nc * nc * nc, k), dim3(kFlatThreads), 0, s, op, v, f, fc, vc, shifts);
}

void launch3p_prolong_jacobi(hipStream_t s, const K3Op& op, KVec e, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k) {
  if (point3_marching(op) & kMarch3Prolong) {
    const auto kern = op.point == kPointBonds ? k3pm_prolong_jacobi<true> : k3pm_prolong_jacobi<false>;
    hipLaunchKernelGGL(kern, march_grid(op, k), dim3(kTileX, kTileY), 0, s, op, e, vin, f, vout, shifts, omega, (int)(op.n / kChunkZ));
    return;
  }
  hipLaunchKernelGGL(k3p_prolong_jacobi, flat_grid(op.n * op.n * op.n, k), dim3(kFlatThreads), 0, s, op, e, vin, f, vout, shifts, omega);
}

void launch3p_band_add(hipStream_t s, const K3Op& op, const KBand& b, int k) {
  hipLaunchKernelGGL(k3p_band_add, dim3((unsigned)((b.n + 127) / 128), (unsigned)k, 1), dim3(128), 0, s, op, b);
}

void launch3p_coarsen(hipStream_t s, long fn, const double* fine, int fine_planes, long fplane, double* coarse, long cplane) {
  const long cn = fn / 2;
  hipLaunchKernelGGL(k3p_coarsen, flat_grid(cn * cn * cn, 1), dim3(kFlatThreads), 0, s, fn, fine, fine_planes, fplane, coarse, cplane);
}

}  // namespace mgcmt
