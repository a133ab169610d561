// The fine level of a 3-D plan with per-point bonds as a plane march, fp64, gfx950: H = -div(w grad) + V on g^3 points with a
// position-dependent inverse effective mass w (mgcmt_plan_create3d_bonds; K3Op::point == 3).
//
// The level is a constant 7-point Kronecker part plus four planes of g^3 numbers, pplane apart: D on the diagonal, Bx / By / Bz
// added to the two entries between a point and its neighbour at x + 1 / y + 1 / z + 1.  The geometry is kernels_3d_point.hip's
// (64 x 4 tile, 32-plane chunks, v's planes z-1, z, z+1 of the thread's column in registers, no LDS); D, Bx, By, Bz are
// streams read at the index of the right-hand side, Bx(x-1) and By(y-1) one more 8-byte load each from the same or the
// neighbouring row's cache line, Bz(z-1) carried from the previous plane step where every plane is updated (the Jacobi and
// the prolongation pass) and a load of its own in a parity stage, which updates every other point.  No halo planes: all three
// directions are predicated, a bond towards a point outside the grid is a predicated zero.
//
// Every point goes through bonds3_point.h, as in the flat kernels (eval3p / relax3p of kernels_3d_point.hip): the sweeps of
// both forms give the same bits.  The residual + restriction keeps k3pm_residual_restrict's structure and summation order.
// Which passes march is K3Op::pmarch (hierarchy.hip); a launcher returns false — nothing launched — where its pass stays flat.
#include "bonds3_point.h"
#include "kernels_3d_common.h"
#include "mgcmt_internal.h"

namespace mgcmt {

namespace {

using namespace k3;

struct LoadProlonged {  // v + P e
  const double* v;
  const double* e;
  long n;
  __device__ __forceinline__ double operator()(long z, long y, long x) const { return v[(z * n + y) * n + x] + prolong_at(e, n / 2, z, y, x); }
};

// stage 0: weighted Jacobi vin -> vout; stage 1: the parity class (x + y + z) % 2 == par of the red-black sweep, in place
template <int STAGE>
__global__ void __launch_bounds__(kTileX* kTileY) k3bm_sweep(K3Op op, KVec vin, KVec f, KVec vout, const double* __restrict__ shifts,
                                                           double omega, int par, int nchunks) {
  const long n = op.n, n2 = n * n;
  const long x = (long)blockIdx.x * kTileX + threadIdx.x;
  const long y = (long)blockIdx.y * kTileY + threadIdx.y;
  const int q = blockIdx.z / nchunks;
  const long z0 = (long)(blockIdx.z % nchunks) * kChunkZ;
  const double* v = vin.p + q * vin.stride;
  const double* fq = f.p + q * f.stride;
  const double* __restrict__ dq = op.pg;
  const double* __restrict__ bxq = op.pg + op.pplane;
  const double* __restrict__ byq = op.pg + 2 * op.pplane;
  const double* __restrict__ bzq = op.pg + 3 * op.pplane;
  double* out = vout.p + q * vout.stride;
  const double mu = shifts[q];
  const bool xm = x > 0, xp = x + 1 < n, ym = y > 0, yp = y + 1 < n;
  const long col = y * n + x;
  double vm = z0 > 0 ? v[(z0 - 1) * n2 + col] : 0.0;
  double vc = v[z0 * n2 + col];
  double bzm = (STAGE == 0 && z0 > 0) ? bzq[(z0 - 1) * n2 + col] : 0.0;  // (a chunk's first plane: a load of its own)
  for (int t = 0; t < kChunkZ; ++t) {
    const long z = z0 + t;
    const long i = z * n2 + col;
    const double vp = z + 1 < n ? v[i + n2] : 0.0;
    if (STAGE == 0 || (((x + y + z) & 1) == par)) {
      const double* c = v + i;
      const double bzp = bzq[i];
      if (STAGE != 0) bzm = z > 0 ? bzq[i - n2] : 0.0;
      const b7::Coef cf = b7::coef(op, bzm, bzp, ym ? byq[i - n] : 0.0, byq[i], xm ? bxq[i - 1] : 0.0, bxq[i]);
      const double dg = b7::dg(op, dq[i], mu);
      const double av = b7::av(cf, dg, vc, vm, vp, ym ? c[-n] : 0.0, yp ? c[n] : 0.0, xm ? c[-1] : 0.0, xp ? c[1] : 0.0);
      out[i] = b7::relax(omega, fq[i], av, dg, vc);
      if (STAGE == 0) bzm = bzp;
    }
    vm = vc;
    vc = vp;
  }
}

// residual + restriction: a thread owns one coarse x-y column (X, Y) of a chunk of coarse planes and keeps the x-y weighted
// residual of the fine plane 2Z + 2 (shared with the next coarse plane) in a register; every plane's nine residuals are
// re-formed from (cached) loads, the bonds among them
__global__ void __launch_bounds__(kTileX* kTileY) k3bm_residual_restrict(K3Op op, KVec v, KVec f, KVec fc, KVec vc,
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
        const b7::Coef cf = b7::coef(op, z > 0 ? g[3 * pl - n2] : 0.0, g[3 * pl], y > 0 ? g[2 * pl - n] : 0.0, g[2 * pl],
                                     x > 0 ? g[pl - 1] : 0.0, g[pl]);
        const double dg = b7::dg(op, g[0], mu);
        const double av = b7::av(cf, dg, p[0], z > 0 ? p[-n2] : 0.0, z + 1 < n ? p[n2] : 0.0, y > 0 ? p[-n] : 0.0, y + 1 < n ? p[n] : 0.0,
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

// prolongation + correction + one weighted-Jacobi sweep: w = v + P e of the planes z-1, z, z+1 of the thread's column in registers
__global__ void __launch_bounds__(kTileX* kTileY) k3bm_prolong_jacobi(K3Op op, KVec e, KVec vin, KVec f, KVec vout,
                                                                    const double* __restrict__ shifts, double omega, int nchunks) {
  const long n = op.n, n2 = n * n;
  const long x = (long)blockIdx.x * kTileX + threadIdx.x;
  const long y = (long)blockIdx.y * kTileY + threadIdx.y;
  const int q = blockIdx.z / nchunks;
  const long z0 = (long)(blockIdx.z % nchunks) * kChunkZ;
  const LoadProlonged w{vin.p + q * vin.stride, e.p + q * e.stride, n};
  const double* fq = f.p + q * f.stride;
  const double* __restrict__ dq = op.pg;
  const double* __restrict__ bxq = op.pg + op.pplane;
  const double* __restrict__ byq = op.pg + 2 * op.pplane;
  const double* __restrict__ bzq = op.pg + 3 * op.pplane;
  double* out = vout.p + q * vout.stride;
  const double mu = shifts[q];
  const bool xm = x > 0, xp = x + 1 < n, ym = y > 0, yp = y + 1 < n;
  const long col = y * n + x;
  double wm = z0 > 0 ? w(z0 - 1, y, x) : 0.0;
  double wc = w(z0, y, x);
  double bzm = z0 > 0 ? bzq[(z0 - 1) * n2 + col] : 0.0;
  for (int t = 0; t < kChunkZ; ++t) {
    const long z = z0 + t;
    const long i = z * n2 + col;
    const double wp = z + 1 < n ? w(z + 1, y, x) : 0.0;
    const double bzp = bzq[i];
    const b7::Coef cf = b7::coef(op, bzm, bzp, ym ? byq[i - n] : 0.0, byq[i], xm ? bxq[i - 1] : 0.0, bxq[i]);
    const double dg = b7::dg(op, dq[i], mu);
    const double av = b7::av(cf, dg, wc, wm, wp, ym ? w(z, y - 1, x) : 0.0, yp ? w(z, y + 1, x) : 0.0, xm ? w(z, y, x - 1) : 0.0,
                             xp ? w(z, y, x + 1) : 0.0);
    out[i] = b7::relax(omega, fq[i], av, dg, wc);
    wm = wc;
    wc = wp;
    bzm = bzp;
  }
}

dim3 march_grid(const K3Op& op, int k) {
  return dim3((unsigned)(op.n / kTileX), (unsigned)(op.n / kTileY), (unsigned)(op.n / kChunkZ * k));
}

}  // namespace

int bonds3_marching(const K3Op& op) {
  return op.point == 3 && op.seven && op.n >= kTileX && op.n % kTileX == 0 ? op.pmarch : 0;
}

bool launch3b_wjacobi(hipStream_t s, const K3Op& op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k) {
  if (!(bonds3_marching(op) & kBonds3Jacobi)) return false;
  hipLaunchKernelGGL(k3bm_sweep<0>, march_grid(op, k), dim3(kTileX, kTileY), 0, s, op, vin, f, vout, shifts, omega, 0, (int)(op.n / kChunkZ));
  return true;
}

bool launch3b_parity(hipStream_t s, const K3Op& op, KVec v, KVec f, const double* shifts, double omega, int par, int k) {
  if (!(bonds3_marching(op) & kBonds3Parity)) return false;
  hipLaunchKernelGGL(k3bm_sweep<1>, march_grid(op, k), dim3(kTileX, kTileY), 0, s, op, v, f, v, shifts, omega, par, (int)(op.n / kChunkZ));
  return true;
}

bool launch3b_residual_restrict(hipStream_t s, const K3Op& op, KVec v, KVec f, KVec fc, KVec vc, const double* shifts, int k) {
  if (!(bonds3_marching(op) & kBonds3Residual)) return false;
  const long nc = op.n / 2;
  const int nch = (int)(op.n / kChunkZ);
  hipLaunchKernelGGL(k3bm_residual_restrict, dim3((unsigned)((nc + kTileX - 1) / kTileX), (unsigned)((nc + kTileY - 1) / kTileY), (unsigned)(nch * k)),
                     dim3(kTileX, kTileY), 0, s, op, v, f, fc, vc, shifts, nch);
  return true;
}

bool launch3b_prolong_jacobi(hipStream_t s, const K3Op& op, KVec e, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k) {
  if (!(bonds3_marching(op) & kBonds3Prolong)) return false;
  hipLaunchKernelGGL(k3bm_prolong_jacobi, march_grid(op, k), dim3(kTileX, kTileY), 0, s, op, e, vin, f, vout, shifts, omega, (int)(op.n / kChunkZ));
  return true;
}

}  // namespace mgcmt
