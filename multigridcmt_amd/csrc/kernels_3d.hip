// Three-dimensional levels: operator apply, weighted Jacobi, multicolour Gauss-Seidel stages, the fused
// residual + full-weighting restriction and the fused trilinear prolongation + correction + first sweep, and the
// coarsest level's band assembly.  fp64, gfx950.
//
// A 3-D level is g x g x g points, index idx = z*g^2 + y*g + x (x fastest: kron(A, kron(B, C)) ordering), stored as
// g z-planes of g^2 points with one zero halo plane above and below (see plan_internal.h).  Every kernel predicates
// all three directions, so the halo planes are never read.  The operator is A = sum_m X_m (x) Y_m (x) Z_m with
// tridiagonal factors over z, y and x (K3Op); the shift mu of (A - mu I) is read per vector from `shifts`.
//
// Two forms:
//   - flat kernels, one thread per point (or per coarse point), any operator: the general three-term path computes
//     the 27 coefficients from the factors, the constant 7-point path (the fine level of a Laplacian) from seven scalars;
//   - marching kernels for the constant 7-point fine level (the hot path): a workgroup owns a 64 x 4 tile of x-y
//     columns and marches a chunk of z-planes, each thread keeping its column's planes z-1, z, z+1 in registers, so that
//     every plane of v is read from HBM once per pass (plus the two halo planes of each chunk); the x-y neighbours are
//     the neighbouring threads' centre loads of the same plane (L1 / L2 hits).
// A level with a per-point part (K3Op::point) is kernels_3d_point.hip's: the launchers below hand over.
#include <cstdint>

#include "kernels_3d_common.h"
#include "mgcmt_internal.h"

namespace mgcmt {

namespace {

using namespace k3;

struct Coef3 {
  double sum;   // sum_j a_ij v_j over the stencil (centre included, unshifted)
  double diag;  // a_ii (unshifted)
};

// (A v)_i and a_ii at (z, y, x); out-of-grid neighbours are zero (Dirichlet)
__device__ __forceinline__ Coef3 eval3(const K3Op& op, const double* __restrict__ v, long z, long y, long x) {
  const long n = op.n, n2 = n * n;
  const double* c = v + z * n2 + y * n + x;
  const bool zm = z > 0, zp = z + 1 < n, ym = y > 0, yp = y + 1 < n, xm = x > 0, xp = x + 1 < n;
  Coef3 r;
  if (op.seven) {
    double acc = op.c0 * c[0];
    if (xm) acc += op.cxm * c[-1];
    if (xp) acc += op.cxp * c[1];
    if (ym) acc += op.cym * c[-n];
    if (yp) acc += op.cyp * c[n];
    if (zm) acc += op.czm * c[-n2];
    if (zp) acc += op.czp * c[n2];
    r.sum = acc;
    r.diag = op.c0;
    return r;
  }
  // general: a(dz, dy, dx) = sum_m X_m[dz](z) Y_m[dy](y) Z_m[dx](x)
  double acc = 0.0, diag = 0.0;
  for (int m = 0; m < op.nterms; ++m) {
    double fz[3], fy[3], fx[3];
    for (int t = 0; t < 3; ++t) {
      fz[t] = op.X[m][t * n + z];
      fy[t] = op.Y[m][t * n + y];
      fx[t] = op.Z[m][t * n + x];
    }
    if (!zm) fz[0] = 0.0;
    if (!zp) fz[2] = 0.0;
    if (!ym) fy[0] = 0.0;
    if (!yp) fy[2] = 0.0;
    if (!xm) fx[0] = 0.0;
    if (!xp) fx[2] = 0.0;
    diag += fz[1] * fy[1] * fx[1];
    for (int a = 0; a < 3; ++a) {
      if (fz[a] == 0.0) continue;
      double pa = 0.0;
      for (int b = 0; b < 3; ++b) {
        if (fy[b] == 0.0) continue;
        const double* row = c + (a - 1) * n2 + (b - 1) * n;
        double pb = 0.0;
        if (fx[0] != 0.0) pb += fx[0] * row[-1];
        pb += fx[1] * row[0];
        if (fx[2] != 0.0) pb += fx[2] * row[1];
        pa += fy[b] * pb;
      }
      acc += fz[a] * pa;
    }
  }
  r.sum = acc;
  r.diag = diag;
  return r;
}

__global__ void __launch_bounds__(kFlatThreads) k3_apply(K3Op op, KVec src, KVec dst, const double* __restrict__ shifts) {
  const long n = op.n, N = n * n * n;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int q = blockIdx.y;
  const double* v = src.p + q * src.stride;
  const long z = i / (n * n), y = (i / n) % n, x = i % n;
  const Coef3 c = eval3(op, v, z, y, x);
  dst.p[q * dst.stride + i] = c.sum - shifts[q] * v[i];
}

__global__ void __launch_bounds__(kFlatThreads) k3_wjacobi(K3Op op, KVec vin, KVec f, KVec vout, const double* __restrict__ shifts,
                                                          double omega) {
  const long n = op.n, N = n * n * n;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int q = blockIdx.y;
  const double* v = vin.p + q * vin.stride;
  const long z = i / (n * n), y = (i / n) % n, x = i % n;
  const Coef3 c = eval3(op, v, z, y, x);
  const double mu = shifts[q];
  const double r = f.p[q * f.stride + i] - (c.sum - mu * v[i]);
  vout.p[q * vout.stride + i] = v[i] + omega * r / (c.diag - mu);
}

// one colour of the multicolour sweep, in place: colour (z%2, y%2, x%2) == (cz, cy, cx); cz < 0: the parity class
// (x + y + z) % 2 == cy (the four odd or four even colours at once — exact on a 7-point operator, whose same-parity
// points do not couple)
__global__ void __launch_bounds__(kFlatThreads) k3_colour(K3Op op, KVec vv, KVec f, const double* __restrict__ shifts, double omega,
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
  const Coef3 c = eval3(op, v, z, y, x);
  const double mu = shifts[q];
  const double r = f.p[q * f.stride + i] - (c.sum - mu * v[i]);
  v[i] = v[i] + omega * r / (c.diag - mu);
}

// full weighting (1/4, 1/2, 1/4 per axis on fine 2I .. 2I+2) of r = f - (A - mu) v (residual != 0) or of src,
// one thread per coarse point; zero_coarse: the coarse iterate vc is set to zero alongside
__global__ void __launch_bounds__(kFlatThreads) k3_restrict(K3Op op, int residual, KVec v, KVec f, KVec fc, KVec vc, int zero_coarse,
                                                           const double* __restrict__ shifts) {
  const long n = op.n, nc = n / 2, Nc = nc * nc * nc;
  const long I = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (I >= Nc) return;
  const int q = blockIdx.y;
  const double* vq = v.p + q * v.stride;
  const double* fq = residual ? f.p + q * f.stride : nullptr;
  const double mu = residual ? shifts[q] : 0.0;
  const long Z = I / (nc * nc), Y = (I / nc) % nc, X = I % nc;
  const double w[3] = {0.25, 0.5, 0.25};
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
        const long i = (z * n + y) * n + x;
        double r;
        if (residual) {
          const Coef3 e = eval3(op, vq, z, y, x);
          r = fq[i] - (e.sum - mu * vq[i]);
        } else {
          r = vq[i];
        }
        pb += w[c] * r;
      }
      pa += w[b] * pb;
    }
    acc += w[a] * pa;
  }
  fc.p[q * fc.stride + I] = acc;
  if (zero_coarse) vc.p[q * vc.stride + I] = 0.0;
}

// mode 0: dst = P e; 1: dst += P e
__global__ void __launch_bounds__(kFlatThreads) k3_prolong(long n, KVec e, KVec dst, int accumulate) {
  const long N = n * n * n;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int q = blockIdx.y;
  const long z = i / (n * n), y = (i / n) % n, x = i % n;
  const double p = prolong_at(e.p + q * e.stride, n / 2, z, y, x);
  double* d = dst.p + q * dst.stride;
  d[i] = accumulate ? d[i] + p : p;
}

// prolongation + correction fused with one weighted-Jacobi sweep: w = v + P e (at the point and its stencil
// neighbours, formed on the fly), vout = w + omega (f - (A - mu) w) / (a_ii - mu).  Nothing but vout is written.
__global__ void __launch_bounds__(kFlatThreads) k3_prolong_jacobi(K3Op op, KVec e, KVec vin, KVec f, KVec vout,
                                                                 const double* __restrict__ shifts, double omega) {
  const long n = op.n, n2 = n * n, N = n2 * n, nc = n / 2;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int q = blockIdx.y;
  const double* eq = e.p + q * e.stride;
  const double* v = vin.p + q * vin.stride;
  const long z = i / n2, y = (i / n) % n, x = i % n;
  const double mu = shifts[q];
  auto w = [&](long zz, long yy, long xx) { return v[(zz * n + yy) * n + xx] + prolong_at(eq, nc, zz, yy, xx); };
  const double wc = w(z, y, x);
  double sum, diag;
  if (op.seven) {
    sum = op.c0 * wc;
    if (x > 0) sum += op.cxm * w(z, y, x - 1);
    if (x + 1 < n) sum += op.cxp * w(z, y, x + 1);
    if (y > 0) sum += op.cym * w(z, y - 1, x);
    if (y + 1 < n) sum += op.cyp * w(z, y + 1, x);
    if (z > 0) sum += op.czm * w(z - 1, y, x);
    if (z + 1 < n) sum += op.czp * w(z + 1, y, x);
    diag = op.c0;
  } else {
    sum = 0.0;
    diag = 0.0;
    for (int m = 0; m < op.nterms; ++m) {
      double fz[3], fy[3], fx[3];
      for (int t = 0; t < 3; ++t) {
        fz[t] = op.X[m][t * n + z];
        fy[t] = op.Y[m][t * n + y];
        fx[t] = op.Z[m][t * n + x];
      }
      diag += fz[1] * fy[1] * fx[1];
    }
    double wn[27];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b)
        for (int c = 0; c < 3; ++c) {
          const long zz = z + a - 1, yy = y + b - 1, xx = x + c - 1;
          wn[(a * 3 + b) * 3 + c] = (zz < 0 || zz >= n || yy < 0 || yy >= n || xx < 0 || xx >= n) ? 0.0 : w(zz, yy, xx);
        }
    for (int m = 0; m < op.nterms; ++m) {
      double fz[3], fy[3], fx[3];
      for (int t = 0; t < 3; ++t) {
        fz[t] = op.X[m][t * n + z];
        fy[t] = op.Y[m][t * n + y];
        fx[t] = op.Z[m][t * n + x];
      }
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
          double pb = 0.0;
          for (int c = 0; c < 3; ++c) pb += fx[c] * wn[(a * 3 + b) * 3 + c];
          sum += fz[a] * fy[b] * pb;
        }
    }
  }
  const double r = f.p[q * f.stride + i] - (sum - mu * wc);
  vout.p[q * vout.stride + i] = wc + omega * r / (diag - mu);
}

// ---- marching kernels: constant 7-point operator, n a multiple of 64 --------------------------------------------
// stage 0: weighted Jacobi vin -> vout; stage 1: the parity class (x + y + z) % 2 == par of the red-black sweep, in
// place (vout == vin; the planes z +- 1 a thread keeps are of the other parity, never updated by this launch)
template <int STAGE>
__global__ void __launch_bounds__(kTileX* kTileY) k3m_sweep(K3Op op, KVec vin, KVec f, KVec vout, const double* __restrict__ shifts,
                                                          double omega, int par, int nchunks) {
  const long n = op.n, n2 = n * n;
  const long x = (long)blockIdx.x * kTileX + threadIdx.x;
  const long y = (long)blockIdx.y * kTileY + threadIdx.y;
  const int q = blockIdx.z / nchunks;
  const long z0 = (long)(blockIdx.z % nchunks) * kChunkZ;
  const double* v = vin.p + q * vin.stride;
  const double* fq = f.p + q * f.stride;
  double* out = vout.p + q * vout.stride;
  const double mu = shifts[q];
  const double inv = omega / (op.c0 - mu);
  const bool xm = x > 0, xp = x + 1 < n, ym = y > 0, yp = y + 1 < n;
  const long col = y * n + x;
  double vm = z0 > 0 ? v[(z0 - 1) * n2 + col] : 0.0;
  double vc = v[z0 * n2 + col];
  for (int t = 0; t < kChunkZ; ++t) {
    const long z = z0 + t;
    const double vp = z + 1 < n ? v[(z + 1) * n2 + col] : 0.0;
    if (STAGE == 0 || (((x + y + z) & 1) == par)) {
      const double* c = v + z * n2 + col;
      double acc = (op.c0 - mu) * vc + op.czm * vm + op.czp * vp;
      if (xm) acc += op.cxm * c[-1];
      if (xp) acc += op.cxp * c[1];
      if (ym) acc += op.cym * c[-n];
      if (yp) acc += op.cyp * c[n];
      out[z * n2 + col] = vc + inv * (fq[z * n2 + col] - acc);
    }
    vm = vc;
    vc = vp;
  }
}

// residual + restriction on a constant 7-point level, marching: a thread owns one coarse x-y column (X, Y) of a chunk of
// coarse planes and keeps the residuals of the fine planes 2Z+2 (shared with the next coarse plane) in registers
__global__ void __launch_bounds__(kTileX* kTileY) k3m_residual_restrict(K3Op op, KVec v, KVec f, KVec fc, KVec vc, const double* __restrict__ shifts,
                                                                      int nchunks) {
  const long n = op.n, n2 = n * n, nc = n / 2, nc2 = nc * nc;
  const long X = (long)blockIdx.x * kTileX + threadIdx.x;
  const long Y = (long)blockIdx.y * kTileY + threadIdx.y;
  if (X >= nc || Y >= nc) return;
  const int q = blockIdx.z / nchunks;
  const long Z0 = (long)(blockIdx.z % nchunks) * (kChunkZ / 2);
  const double* vq = v.p + q * v.stride;
  const double* fq = f.p + q * f.stride;
  const double mu = shifts[q];
  const double w[3] = {0.25, 0.5, 0.25};
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
        const double* p = vq + z * n2 + y * n + x;
        double acc = (op.c0 - mu) * p[0];
        if (x > 0) acc += op.cxm * p[-1];
        if (x + 1 < n) acc += op.cxp * p[1];
        if (y > 0) acc += op.cym * p[-n];
        if (y + 1 < n) acc += op.cyp * p[n];
        if (z > 0) acc += op.czm * p[-n2];
        if (z + 1 < n) acc += op.czp * p[n2];
        pb += w[c] * (fq[z * n2 + y * n + x] - acc);
      }
      pa += w[b] * pb;
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

// prolongation + correction + one weighted-Jacobi sweep on a constant 7-point level, marching: w = v + P e of the
// planes z-1, z, z+1 of the thread's column in registers
__global__ void __launch_bounds__(kTileX* kTileY) k3m_prolong_jacobi(K3Op op, KVec e, KVec vin, KVec f, KVec vout, const double* __restrict__ shifts,
                                                                   double omega, int nchunks) {
  const long n = op.n, n2 = n * n, nc = n / 2;
  const long x = (long)blockIdx.x * kTileX + threadIdx.x;
  const long y = (long)blockIdx.y * kTileY + threadIdx.y;
  const int q = blockIdx.z / nchunks;
  const long z0 = (long)(blockIdx.z % nchunks) * kChunkZ;
  const double* eq = e.p + q * e.stride;
  const double* v = vin.p + q * vin.stride;
  const double* fq = f.p + q * f.stride;
  double* out = vout.p + q * vout.stride;
  const double mu = shifts[q];
  const double inv = omega / (op.c0 - mu);
  const bool xm = x > 0, xp = x + 1 < n, ym = y > 0, yp = y + 1 < n;
  const long col = y * n + x;
  auto w = [&](long zz, long yy, long xx) { return v[zz * n2 + yy * n + xx] + prolong_at(eq, nc, zz, yy, xx); };
  double wm = z0 > 0 ? w(z0 - 1, y, x) : 0.0;
  double wc = w(z0, y, x);
  for (int t = 0; t < kChunkZ; ++t) {
    const long z = z0 + t;
    const double wp = z + 1 < n ? w(z + 1, y, x) : 0.0;
    double acc = (op.c0 - mu) * wc + op.czm * wm + op.czp * wp;
    if (xm) acc += op.cxm * w(z, y, x - 1);
    if (xp) acc += op.cxp * w(z, y, x + 1);
    if (ym) acc += op.cym * w(z, y - 1, x);
    if (yp) acc += op.cyp * w(z, y + 1, x);
    out[z * n2 + col] = wc + inv * (fq[z * n2 + col] - acc);
    wm = wc;
    wc = wp;
  }
}

bool marching(const K3Op& op) { return op.seven && op.n >= kTileX && op.n % kTileX == 0; }

__global__ void k3_band_assemble(K3Op op, const double* __restrict__ shifts, KBand b) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= b.n) return;
  const int q = blockIdx.y;
  double* ab = b.ab + q * b.ab_stride;
  const long n = op.n, n2 = n * n;
  const long z = r / n2, y = (r / n) % n, x = r % n;
  for (int w = 0; w < b.width; ++w) ab[r * b.width + w] = 0.0;
  for (int a = -1; a <= 1; ++a)
    for (int bb = -1; bb <= 1; ++bb)
      for (int c = -1; c <= 1; ++c) {
        const long zz = z + a, yy = y + bb, xx = x + c;
        if (zz < 0 || zz >= n || yy < 0 || yy >= n || xx < 0 || xx >= n) continue;
        double v = 0.0;
        if (op.seven) {
          const int nzero = (a != 0) + (bb != 0) + (c != 0);
          if (nzero == 0) v = op.c0;
          else if (nzero == 1) v = a < 0 ? op.czm : a > 0 ? op.czp : bb < 0 ? op.cym : bb > 0 ? op.cyp : c < 0 ? op.cxm : op.cxp;
        } else {
          for (int m = 0; m < op.nterms; ++m) v += op.X[m][(a + 1) * n + z] * op.Y[m][(bb + 1) * n + y] * op.Z[m][(c + 1) * n + x];
        }
        if (a == 0 && bb == 0 && c == 0) v -= shifts[q];
        const long col = zz * n2 + yy * n + xx;
        ab[r * b.width + (col - r + b.kl)] = v;
      }
}

}  // namespace

void launch3_apply(hipStream_t s, const K3Op& op, KVec src, KVec dst, const double* shifts, int k) {
  if (op.point) return launch3p_apply(s, op, src, dst, shifts, k);
  hipLaunchKernelGGL(k3_apply, flat_grid(op.n * op.n * op.n, k), dim3(kFlatThreads), 0, s, op, src, dst, shifts);
}

void launch3_wjacobi(hipStream_t s, const K3Op& op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k) {
  if (op.point) return launch3p_wjacobi(s, op, vin, f, vout, shifts, omega, k);
  if (marching(op)) {
    const int nch = (int)(op.n / kChunkZ);
    hipLaunchKernelGGL(k3m_sweep<0>, dim3((unsigned)(op.n / kTileX), (unsigned)(op.n / kTileY), (unsigned)(nch * k)), dim3(kTileX, kTileY), 0, s,
                       op, vin, f, vout, shifts, omega, 0, nch);
    return;
  }
  hipLaunchKernelGGL(k3_wjacobi, flat_grid(op.n * op.n * op.n, k), dim3(kFlatThreads), 0, s, op, vin, f, vout, shifts, omega);
}

void launch3_mc_sweep(hipStream_t s, const K3Op& op, KVec v, KVec f, const double* shifts, double omega, int k) {
  if (op.point) return launch3p_mc_sweep(s, op, v, f, shifts, omega, k);
  // odd coordinate sum first: (0,0,1), (0,1,0), (1,0,0), (1,1,1), then (0,0,0), (0,1,1), (1,0,1), (1,1,0)
  static const int order[8][3] = {{0, 0, 1}, {0, 1, 0}, {1, 0, 0}, {1, 1, 1}, {0, 0, 0}, {0, 1, 1}, {1, 0, 1}, {1, 1, 0}};
  if (op.seven) {  // the four odd colours do not couple on a 7-point operator, nor the four even ones: two stages
    for (int par = 1; par >= 0; --par) {
      if (marching(op)) {
        const int nch = (int)(op.n / kChunkZ);
        hipLaunchKernelGGL(k3m_sweep<1>, dim3((unsigned)(op.n / kTileX), (unsigned)(op.n / kTileY), (unsigned)(nch * k)), dim3(kTileX, kTileY), 0,
                           s, op, v, f, v, shifts, omega, par, nch);
      } else {
        hipLaunchKernelGGL(k3_colour, flat_grid(op.n * op.n * op.n, k), dim3(kFlatThreads), 0, s, op, v, f, shifts, omega, -1, par, 0);
      }
    }
    return;
  }
  for (int c = 0; c < 8; ++c)
    hipLaunchKernelGGL(k3_colour, flat_grid(op.n * op.n * op.n, k), dim3(kFlatThreads), 0, s, op, v, f, shifts, omega, order[c][0], order[c][1],
                       order[c][2]);
}

void launch3_residual_restrict(hipStream_t s, const K3Op& op, KVec v, KVec f, KVec fc, KVec vc, const double* shifts, int k) {
  if (op.point) return launch3p_residual_restrict(s, op, v, f, fc, vc, shifts, k);
  const long nc = op.n / 2;
  if (marching(op)) {
    const int nch = (int)(op.n / kChunkZ);
    hipLaunchKernelGGL(k3m_residual_restrict, dim3((unsigned)((nc + kTileX - 1) / kTileX), (unsigned)((nc + kTileY - 1) / kTileY), (unsigned)(nch * k)),
                       dim3(kTileX, kTileY), 0, s, op, v, f, fc, vc, shifts, nch);
    return;
  }
  hipLaunchKernelGGL(k3_restrict, flat_grid(nc * nc * nc, k), dim3(kFlatThreads), 0, s, op, 1, v, f, fc, vc, 1, shifts);
}

void launch3_restrict(hipStream_t s, const K3Op& fine, KVec src, KVec dst, int k) {
  const long nc = fine.n / 2;
  hipLaunchKernelGGL(k3_restrict, flat_grid(nc * nc * nc, k), dim3(kFlatThreads), 0, s, fine, 0, src, src, dst, dst, 0, (const double*)nullptr);
}

void launch3_prolong(hipStream_t s, long n, KVec e, KVec dst, int accumulate, int k) {
  hipLaunchKernelGGL(k3_prolong, flat_grid(n * n * n, k), dim3(kFlatThreads), 0, s, n, e, dst, accumulate);
}

void launch3_prolong_jacobi(hipStream_t s, const K3Op& op, KVec e, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k) {
  if (op.point) return launch3p_prolong_jacobi(s, op, e, vin, f, vout, shifts, omega, k);
  if (marching(op)) {
    const int nch = (int)(op.n / kChunkZ);
    hipLaunchKernelGGL(k3m_prolong_jacobi, dim3((unsigned)(op.n / kTileX), (unsigned)(op.n / kTileY), (unsigned)(nch * k)), dim3(kTileX, kTileY), 0, s,
                       op, e, vin, f, vout, shifts, omega, nch);
    return;
  }
  hipLaunchKernelGGL(k3_prolong_jacobi, flat_grid(op.n * op.n * op.n, k), dim3(kFlatThreads), 0, s, op, e, vin, f, vout, shifts, omega);
}

void launch3_band_assemble(hipStream_t s, const K3Op& op, const double* shifts, KBand b, int k) {
  hipLaunchKernelGGL(k3_band_assemble, dim3((unsigned)((b.n + 127) / 128), (unsigned)k, 1), dim3(128), 0, s, op, shifts, b);
  if (op.point) launch3p_band_add(s, op, b, k);  // the per-point entries, on top of the Kronecker part's
}

}  // namespace mgcmt
