// Tile kernels of a nine-plane level (KOp::point == kPointPlanes), fp64, gfx950: level 0 of mgcmt_plan_create_nine — H = -div(W grad) + V
// with a position-dependent 2 x 2 inverse-mass tensor W, a symmetric 9-point operator with per-point coefficients — and, with
// MGCMT_NINE_TILE=2, the Galerkin levels of any plan with a per-point part.
//
// The flat kernels of such a level (kernels_pointwise.hip) are one launch per operation: a four-colour sweep is four launches,
// each touching every cache line of the nine planes to use a quarter of it.  Here one workgroup of 256 threads owns a
// kTileRows x kTileCols output tile: it stages v on the tile plus H rings in LDS (points outside the grid are zeros — the
// Dirichlet ghosts, never updated), runs every stage there between barriers — stage k inside the window shrunk by k rings, so
// that what it reads has been through the stages before it — and stores the tile.  The thread that updates a point reads f and
// the point's nine coefficients straight from global memory.  Every pass is out of place (vin -> vout; the caller exchanges the
// two), so a tile never sees a neighbour's writes and nothing passes between workgroups.  A point is evaluated by
// nine_point.h's functions, which the flat kernels call with the same values: a sweep gives the same bits in either form.
//
//   k_n9_colour              one four-colour sweep (0,1), (1,0), (0,0), (1,1): H = 4
//   k_n9_jacobi<., NS>       NS = 1 or 2 weighted-Jacobi sweeps: H = NS, two LDS windows when NS = 2
//   k_n9_residual_restrict   the residual of a (2 kCoarseRows + 1) x (2 kCoarseCols + 1) window into LDS, full weighting out of
//                            it in k_restrict's order (kernels_stencil.hip): F[l+1] = R (f - (A - mu I) v), V[l+1] = 0
//
// Compulsory traffic of a colour sweep or a Jacobi pair: v, f, the nine planes in, v' out = 96 B per point; the halo is read
// (TR + 2H)(TC + 2H) / (TR TC) times over: 1.41 (colour), 1.20 (Jacobi pair), for v, and for f and the planes stage by stage.
#include <cstdint>

#include "mgcmt_internal.h"
#include "nine_point.h"

namespace mgcmt {

namespace {

#ifndef MGCMT_NINE_TILE_ROWS
#define MGCMT_NINE_TILE_ROWS 32
#endif
#ifndef MGCMT_NINE_TILE_COLS
#define MGCMT_NINE_TILE_COLS 64
#endif
constexpr int kTileRows = MGCMT_NINE_TILE_ROWS, kTileCols = MGCMT_NINE_TILE_COLS;  // both even
constexpr int kCoarseRows = kTileRows / 2, kCoarseCols = kTileCols / 2;            // coarse tile of the residual + restriction pass
constexpr int kTileThreads = 256;
constexpr long kNineMinCols = 128;

// A window of WR x WC points in LDS whose point (0, 0) is grid point (i0, j0).
template <int WR, int WC>
struct Window {
  double* t;
  long i0, j0;
  __device__ __forceinline__ double& at(int r, int c) const { return t[r * WC + c]; }
  // v on the whole window; zeros outside the grid
  __device__ __forceinline__ void stage_in(const double* __restrict__ v, long nr, long nc) const {
    for (int idx = threadIdx.x; idx < WR * WC; idx += kTileThreads) {
      const int r = idx / WC, c = idx % WC;
      const long i = i0 + r, j = j0 + c;
      t[idx] = (i >= 0 && i < nr && j >= 0 && j < nc) ? v[i * nc + j] : 0.0;
    }
  }
  // the values around window point (r, c), 1 <= r < WR - 1, 1 <= c < WC - 1
  __device__ __forceinline__ nine::Nb neighbours(int r, int c) const {
    const double* p = t + r * WC + c;
    nine::Nb v;
    v.nw = p[-WC - 1];
    v.n = p[-WC];
    v.ne = p[-WC + 1];
    v.w = p[-1];
    v.e = p[1];
    v.sw = p[WC - 1];
    v.s = p[WC];
    v.se = p[WC + 1];
    return v;
  }
};

// grid point (i, j), inside the grid, from the values around it
template <bool FIVE>
__device__ __forceinline__ nine::Pt eval(const KOp& op, long i, long j, double mu, const nine::Nb& nb) {
  double g[9];
  nine::load9(g, op.pg + i * op.pld + j, op.pplane);
  if (FIVE) return nine::five(op.cn, op.cw, op.c0 - mu, nb, g);
  return nine::general(op, i, j, mu, nb, g);
}

// Stage K (1 ..) of a colour sweep in the window: the points of colour (CA, CB) = (i % 2, j % 2) inside the window shrunk
// by K rings, in place.  The window's origin is even in both directions, so a window index has its grid index's parity.
template <bool FIVE, int WR, int WC, int K, int CA, int CB>
__device__ __forceinline__ void colour_stage(const Window<WR, WC>& w, const KOp& op, const double* __restrict__ fp, long nr, long nc, double mu,
                                             double omega) {
  constexpr int r0 = K + ((K ^ CA) & 1), c0 = K + ((K ^ CB) & 1);
  constexpr int rows = (WR - K - r0 + 1) / 2, cols = (WC - K - c0 + 1) / 2;
#pragma unroll 2
  for (int idx = threadIdx.x; idx < rows * cols; idx += kTileThreads) {
    const int r = r0 + 2 * (idx / cols), c = c0 + 2 * (idx % cols);
    const long i = w.i0 + r, j = w.j0 + c;
    const bool in = i >= 0 && i < nr && j >= 0 && j < nc;
    const long ii = in ? i : 0, jj = in ? j : 0;  // (outside the grid: point (0, 0) is read and the result dropped — loads without a branch)
    const nine::Pt p = eval<FIVE>(op, ii, jj, mu, w.neighbours(r, c));
    const double vc = w.at(r, c);
    const double vn = nine::relaxed(omega, fp[ii * nc + jj], p, vc);
    if (in) w.at(r, c) = vn;
  }
}

// one whole four-colour sweep, vin -> vout
template <bool FIVE>
__global__ void __launch_bounds__(kTileThreads) k_n9_colour(KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* __restrict__ shifts, double omega) {
  constexpr int H = 4, WR = kTileRows + 2 * H, WC = kTileCols + 2 * H;
  __shared__ double lds[WR * WC];
  const int q = blockIdx.z;
  const long nr = g.nr, nc = g.nc;
  const long ti = (long)blockIdx.y * kTileRows, tj = (long)blockIdx.x * kTileCols;
  const double mu = shifts[q];
  const double* __restrict__ fp = f.p + q * f.stride;
  const Window<WR, WC> w{lds, ti - H, tj - H};
  w.stage_in(vin.p + q * vin.stride, nr, nc);
  __syncthreads();
  colour_stage<FIVE, WR, WC, 1, 0, 1>(w, op, fp, nr, nc, mu, omega);
  __syncthreads();
  colour_stage<FIVE, WR, WC, 2, 1, 0>(w, op, fp, nr, nc, mu, omega);
  __syncthreads();
  colour_stage<FIVE, WR, WC, 3, 0, 0>(w, op, fp, nr, nc, mu, omega);
  __syncthreads();
  colour_stage<FIVE, WR, WC, 4, 1, 1>(w, op, fp, nr, nc, mu, omega);
  __syncthreads();
  double* __restrict__ out = vout.p + q * vout.stride;
  for (int idx = threadIdx.x; idx < kTileRows * kTileCols; idx += kTileThreads) {
    const int r = idx / kTileCols, c = idx % kTileCols;
    const long i = ti + r, j = tj + c;
    if (i < nr && j < nc) out[i * nc + j] = w.at(r + H, c + H);
  }
}

// NS weighted-Jacobi sweeps, vin -> vout: v' = v + w (f - (A - mu I) v) / d     (MGCMTSolver.py:193-206)
template <bool FIVE, int NS>
__global__ void __launch_bounds__(kTileThreads) k_n9_jacobi(KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* __restrict__ shifts, double omega) {
  constexpr int H = NS, WR = kTileRows + 2 * H, WC = kTileCols + 2 * H;
  __shared__ double lds_a[WR * WC];
  __shared__ double lds_b[NS == 2 ? WR * WC : 1];
  const int q = blockIdx.z;
  const long nr = g.nr, nc = g.nc;
  const long ti = (long)blockIdx.y * kTileRows, tj = (long)blockIdx.x * kTileCols;
  const double mu = shifts[q];
  const double* __restrict__ fp = f.p + q * f.stride;
  const Window<WR, WC> a{lds_a, ti - H, tj - H};
  a.stage_in(vin.p + q * vin.stride, nr, nc);
  __syncthreads();
  const Window<WR, WC> b{NS == 2 ? lds_b : lds_a, ti - H, tj - H};
  if (NS == 2) {
    // the first sweep on the window shrunk by one ring, a -> b; a point outside the grid stays the zero it is
    constexpr int rows = WR - 2, cols = WC - 2;
#pragma unroll 4
    for (int idx = threadIdx.x; idx < rows * cols; idx += kTileThreads) {
      const int r = 1 + idx / cols, c = 1 + idx % cols;
      const long i = a.i0 + r, j = a.j0 + c;
      const bool in = i >= 0 && i < nr && j >= 0 && j < nc;
      const long ii = in ? i : 0, jj = in ? j : 0;  // (outside the grid: point (0, 0) is read and the result dropped)
      const nine::Pt p = eval<FIVE>(op, ii, jj, mu, a.neighbours(r, c));
      const double val = nine::relaxed(omega, fp[ii * nc + jj], p, a.at(r, c));
      b.at(r, c) = in ? val : 0.0;
    }
    __syncthreads();
  }
  double* __restrict__ out = vout.p + q * vout.stride;
#pragma unroll 4
  for (int idx = threadIdx.x; idx < kTileRows * kTileCols; idx += kTileThreads) {
    const int r = H + idx / kTileCols, c = H + idx % kTileCols;
    const long i = b.i0 + r, j = b.j0 + c;
    const bool in = i < nr && j < nc;
    const long ii = in ? i : 0, jj = in ? j : 0;
    const nine::Pt p = eval<FIVE>(op, ii, jj, mu, b.neighbours(r, c));
    const double val = nine::relaxed(omega, fp[ii * nc + jj], p, b.at(r, c));
    if (in) out[i * nc + j] = val;
  }
}

// fc(I, J) = sum over fine rows 2I .. 2I + 2 and columns 2J .. 2J + 2 of (1/4, 1/2, 1/4) (x) (1/4, 1/2, 1/4) times
// r = f - (A - mu I) v, in k_restrict's order — the bits of k_pw_residual followed by k_restrict.  The residual of fine row nr
// (below the last coarse row: the reference's one-sided end) is the zero k_restrict reads from the halo row; column nc is
// left out as it leaves it out.
template <bool FIVE>
__global__ void __launch_bounds__(kTileThreads) k_n9_residual_restrict(KGrid g, KOp op, KVec vv, KVec f, KVec fc, KVec vc, const double* __restrict__ shifts) {
  constexpr int RR = 2 * kCoarseRows + 1, RC = 2 * kCoarseCols + 1, WR = RR + 2, WC = RC + 2;
  __shared__ double lds_v[WR * WC];
  __shared__ double lds_r[RR * RC];
  const int q = blockIdx.z;
  const long nr = g.nr, nc = g.nc, cnr = nr / 2, cnc = nc / 2;
  const long I0 = (long)blockIdx.y * kCoarseRows, J0 = (long)blockIdx.x * kCoarseCols;
  const double mu = shifts[q];
  const double* __restrict__ fp = f.p + q * f.stride;
  const Window<WR, WC> w{lds_v, 2 * I0 - 1, 2 * J0 - 1};
  w.stage_in(vv.p + q * vv.stride, nr, nc);
  __syncthreads();
#pragma unroll 4
  for (int idx = threadIdx.x; idx < RR * RC; idx += kTileThreads) {
    const int r = idx / RC, c = idx % RC;
    const long i = 2 * I0 + r, j = 2 * J0 + c;
    const bool in = i < nr && j < nc;
    const long ii = in ? i : 0, jj = in ? j : 0;  // (outside the grid: point (0, 0) is read and the result dropped)
    const nine::Pt p = eval<FIVE>(op, ii, jj, mu, w.neighbours(r + 1, c + 1));
    const double val = nine::residual(fp[ii * nc + jj], p, w.at(r + 1, c + 1));
    lds_r[idx] = in ? val : 0.0;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < kCoarseRows * kCoarseCols; idx += kTileThreads) {
    const int li = idx / kCoarseCols, lj = idx % kCoarseCols;
    const long I = I0 + li, J = J0 + lj;
    if (I >= cnr || J >= cnc) continue;
    const bool h2 = 2 * J + 2 < nc;
    const double* a = lds_r + (2 * li) * RC + 2 * lj;
    const double* b = a + RC;
    const double* c = b + RC;
    const double ra = 0.25 * a[0] + 0.5 * a[1] + (h2 ? 0.25 * a[2] : 0.0);
    const double rb = 0.25 * b[0] + 0.5 * b[1] + (h2 ? 0.25 * b[2] : 0.0);
    const double rcw = 0.25 * c[0] + 0.5 * c[1] + (h2 ? 0.25 * c[2] : 0.0);
    fc.p[q * fc.stride + I * cnc + J] = 0.25 * ra + 0.5 * rb + 0.25 * rcw;
    if (vc.p) vc.p[q * vc.stride + I * cnc + J] = 0.0;
  }
}

inline dim3 tile_grid(long nr, long nc, int tr, int tc, int k) { return dim3((unsigned)((nc + tc - 1) / tc), (unsigned)((nr + tr - 1) / tr), (unsigned)k); }

}  // namespace

int nine_tiled(const KGrid& g, const KOp& op) {
  if (op.point != kPointPlanes || !g.coarsen_rows || g.nc < kNineMinCols || g.nr < 2) return 0;
  return op.pmarch & (kNineColour | kNineJacobi | kNineResidual);
}

bool launch_nine_wjacobi(hipStream_t s, KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int nsweep, int k) {
  if (!(nine_tiled(g, op) & kNineJacobi) || (nsweep != 1 && nsweep != 2)) return false;
  const dim3 grid = tile_grid(g.nr, g.nc, kTileRows, kTileCols, k), b(kTileThreads, 1, 1);
  if (op.five_point) {
    if (nsweep == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_n9_jacobi<true, 1>), grid, b, 0, s, g, op, vin, f, vout, shifts, omega);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_n9_jacobi<true, 2>), grid, b, 0, s, g, op, vin, f, vout, shifts, omega);
  } else {
    if (nsweep == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_n9_jacobi<false, 1>), grid, b, 0, s, g, op, vin, f, vout, shifts, omega);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_n9_jacobi<false, 2>), grid, b, 0, s, g, op, vin, f, vout, shifts, omega);
  }
  return true;
}

bool launch_nine_colour(hipStream_t s, KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k) {
  if (!(nine_tiled(g, op) & kNineColour)) return false;
  const dim3 grid = tile_grid(g.nr, g.nc, kTileRows, kTileCols, k), b(kTileThreads, 1, 1);
  if (op.five_point) hipLaunchKernelGGL(k_n9_colour<true>, grid, b, 0, s, g, op, vin, f, vout, shifts, omega);
  else hipLaunchKernelGGL(k_n9_colour<false>, grid, b, 0, s, g, op, vin, f, vout, shifts, omega);
  return true;
}

bool launch_nine_residual_restrict(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, KVec fc, KVec vc, const double* shifts, int k) {
  if (!(nine_tiled(g, op) & kNineResidual) || (g.nr & 1) || (g.nc & 1)) return false;
  const dim3 grid = tile_grid(g.nr / 2, g.nc / 2, kCoarseRows, kCoarseCols, k), b(kTileThreads, 1, 1);
  if (op.five_point) hipLaunchKernelGGL(k_n9_residual_restrict<true>, grid, b, 0, s, g, op, v, f, fc, vc, shifts);
  else hipLaunchKernelGGL(k_n9_residual_restrict<false>, grid, b, 0, s, g, op, v, f, fc, vc, shifts);
  return true;
}

}  // namespace mgcmt
