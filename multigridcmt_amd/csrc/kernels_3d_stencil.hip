// 27-plane levels of a 3-D plan (K3Op::point == kPointPlanes), fp64, gfx950: the two passes whose flat form
// (kernels_3d_point.hip, one thread per point) leaves most of its traffic unused.  Level 0 of mgcmt_plan_create3d_stencil is
// such a level with a constant 7-point Kronecker part (7/8 of all points of the plan); the Galerkin levels of every plan with
// a per-point part are such levels with general terms.  Both kernels serve both forms: a point is computed by
// stencil27_point.h's p27::point from the same values as in the flat kernels, so each pass gives the bits of its flat form.
//   k3n_colour: one stage (cz, cy, cx) of the eight-colour sweep, in place, launched on the n^3 / 8 points of its colour only
//     (the flat stage launches n^3 threads and retires 7/8 of them).  Exact in place: points of one colour are two apart on
//     every axis and a 27-point stencil does not couple them.  A thread owns one point; consecutive threads own consecutive
//     points of the colour along x, so a wave reads its coefficients and f at stride 2.
//   k3n_residual_restrict: fc <- R (f - (A - mu I) v), vc <- 0 with every fine residual evaluated ONCE (the flat kernel forms
//     the 27 fine residuals of every coarse point: each fine residual 27/8 times).  A workgroup of 16 x 16 threads owns a
//     16 x 16 tile of coarse (Y, X) columns and marches a chunk of 8 coarse planes.  Per coarse plane Z the residuals of the
//     fine planes 2Z + 1 and 2Z + 2 on the tile's 33 x 33 window go to LDS, one evaluation per fine point, the coefficients
//     read once; full weighting then reads LDS with k3p_residual_restrict's weights and summation order (pb over c, pa over b,
//     then 1/4 lo + 1/2 mid + 1/4 hi).  The x-y weighted plane 2Z + 2 is carried to the next coarse plane in a register: the
//     weights are powers of two, so the carried sum has the bits of the re-formed one.  The last coarse plane / row / column is
//     one-sided as in the reference's transfers.  Points outside the grid are predicated, every thread reaches every barrier,
//     nothing passes between workgroups (out of place: v and f are read, fc and vc written).
// Which levels take them is stencil3_tiled (K3Op::pmarch, decided at plan creation: hierarchy.hip, MGCMT_3D_STENCIL_TILE).
#include "kernels_3d_common.h"
#include "mgcmt_internal.h"
#include "stencil27_point.h"

namespace mgcmt {

namespace {

using namespace k3;

constexpr int kRTX = 16, kRTY = 16;  // coarse columns per workgroup: two tiles along x and y at 64^3
constexpr int kRCZ = 8;              // coarse planes per chunk
constexpr int kRW = 2 * kRTX + 1, kRH = 2 * kRTY + 1;  // the fine window of a tile

struct Load {
  const double* v;
  long n;
  __device__ __forceinline__ double operator()(long z, long y, long x) const { return v[(z * n + y) * n + x]; }
};

__global__ void __launch_bounds__(kFlatThreads) k3n_colour(K3Op op, KVec vv, KVec f, const double* __restrict__ shifts, double omega, int cz,
                                                          int cy, int cx) {
  const long n = op.n, h = n / 2, H = h * h * h;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= H) return;
  const long z = 2 * (i / (h * h)) + cz, y = 2 * ((i / h) % h) + cy, x = 2 * (i % h) + cx;
  const long idx = (z * n + y) * n + x;
  const int q = blockIdx.y;
  double* v = vv.p + q * vv.stride;
  const p27::Eval e = p27::point(op, Load{v, n}, z, y, x, shifts[q]);
  v[idx] = p27::relax(op, omega, f.p[q * f.stride + idx], e, v[idx]);
}

__global__ void __launch_bounds__(kRTX* kRTY) k3n_residual_restrict(K3Op op, KVec v, KVec f, KVec fc, KVec vc, const double* __restrict__ shifts,
                                                                  int nchunks) {
  __shared__ double lds_mid[kRH * kRW];
  __shared__ double lds_hi[kRH * kRW];
  const long n = op.n, nc = n / 2, nc2 = nc * nc;
  const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * kRTX + tx;
  const long X0 = (long)blockIdx.x * kRTX, Y0 = (long)blockIdx.y * kRTY;
  const long X = X0 + tx, Y = Y0 + ty;  // (nc is a multiple of the tile: every thread owns a coarse column)
  const int q = blockIdx.z / nchunks;
  const long Z0 = (long)(blockIdx.z % nchunks) * kRCZ;
  const double* vq = v.p + q * v.stride;
  const double* fq = f.p + q * f.stride;
  const double mu = shifts[q];
  // the residuals of fine plane z on the tile's window, one evaluation per point (zeros outside the grid: never read)
  auto fill = [&](double* buf, long z) {
    for (int i = tid; i < kRH * kRW; i += kRTX * kRTY) {
      const long y = 2 * Y0 + i / kRW, x = 2 * X0 + i % kRW;
      double r = 0.0;
      if (y < n && x < n) {
        const p27::Eval e = p27::point(op, Load{vq, n}, z, y, x, mu);
        r = fq[(z * n + y) * n + x] - e.av;
      }
      buf[i] = r;
    }
  };
  // x-y full weighting of a plane of residuals at the thread's coarse column
  auto weigh = [&](const double* buf) {
    double pa = 0.0;
    for (int b = 0; b < 3; ++b) {
      if (2 * Y + b >= n) continue;
      double pb = 0.0;
      for (int c = 0; c < 3; ++c) {
        if (2 * X + c >= n) continue;
        pb += (c == 1 ? 0.5 : 0.25) * buf[(2 * ty + b) * kRW + 2 * tx + c];
      }
      pa += (b == 1 ? 0.5 : 0.25) * pb;
    }
    return pa;
  };
  fill(lds_hi, 2 * Z0);
  __syncthreads();
  double lo = weigh(lds_hi);
  __syncthreads();
  for (int t = 0; t < kRCZ; ++t) {
    const long Z = Z0 + t;
    const bool has_hi = 2 * Z + 2 < n;  // (the same for every thread of the workgroup)
    fill(lds_mid, 2 * Z + 1);
    if (has_hi) fill(lds_hi, 2 * Z + 2);
    __syncthreads();
    const double mid = weigh(lds_mid);
    const double hi = has_hi ? weigh(lds_hi) : 0.0;
    double acc = 0.0;
    acc += 0.25 * lo;
    acc += 0.5 * mid;
    if (has_hi) acc += 0.25 * hi;
    fc.p[q * fc.stride + Z * nc2 + Y * nc + X] = acc;
    vc.p[q * vc.stride + Z * nc2 + Y * nc + X] = 0.0;
    lo = hi;
    __syncthreads();
  }
}

}  // namespace

int stencil3_tiled(const K3Op& op) {
  return op.point == kPointPlanes && op.n >= 64 && op.n % 64 == 0 ? op.pmarch & (kStencil3Colour | kStencil3Residual) : 0;
}

bool launch3n_colour(hipStream_t s, const K3Op& op, KVec v, KVec f, const double* shifts, double omega, int cz, int cy, int cx, int k) {
  if (!(stencil3_tiled(op) & kStencil3Colour)) return false;
  const long h = op.n / 2;
  hipLaunchKernelGGL(k3n_colour, flat_grid(h * h * h, k), dim3(kFlatThreads), 0, s, op, v, f, shifts, omega, cz, cy, cx);
  return true;
}

bool launch3n_residual_restrict(hipStream_t s, const K3Op& op, KVec v, KVec f, KVec fc, KVec vc, const double* shifts, int k) {
  if (!(stencil3_tiled(op) & kStencil3Residual)) return false;
  const long nc = op.n / 2;  // a multiple of 32: whole tiles, whole chunks
  const int nch = (int)(nc / kRCZ);
  hipLaunchKernelGGL(k3n_residual_restrict, dim3((unsigned)(nc / kRTX), (unsigned)(nc / kRTY), (unsigned)(nch * k)), dim3(kRTX, kRTY), 0, s, op, v,
                     f, fc, vc, shifts, nch);
  return true;
}

}  // namespace mgcmt
