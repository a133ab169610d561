// V-cycle-preconditioned conjugate gradients for (A - mu I) x = f: the vector passes and the scalar kernels between them
// (the driver is pcg_host.hip; the preconditioner is mgcmt_vcycle, the operator the level's own apply kernel).
//
// One iteration is  z = cycle(r);  rho = <z, r>, sigma = <z, q>;  beta;  p <- z + beta p;  q <- (A - mu I) p;  <p, q>;  alpha;
// x += alpha p, r -= alpha q, <r, r>;  ||r|| into the history, the stop word.  Every scalar stays in a block of device state
// words (mgcmt_internal.h, kPcg*): nothing here synchronises with the host.  Reductions are per-block partial sums in a fixed
// order (block_partials of rq_common.h), added by the one workgroup of the scalar kernel that follows the pass, again in a
// fixed order: the same bits from run to run.  The library is built with -ffp-contract=off; the multiply-adds of the
// direction and update passes are explicit fma() calls, the same in the device and the emulation build.
//
// The passes work on the contiguous interior of a level vector — n doubles — and know nothing of its shape.  Level vectors are
// 16-byte aligned and hold an even number of points, so the passes use 16-byte accesses (VEC2); anything else takes the
// 8-byte form of the same arithmetic.
//
// Once the stop word is set (convergence, or a rho / <p, q> that is zero or not finite) every kernel of an iteration returns
// before it writes: x, p, r, the scalars and the history stay those of the iteration that set it, however many iterations
// the host has queued behind it.
//
// Columns.  Every kernel works on k independent systems at once (mgcmt_pcg_begin_k; the single solve is k = 1): the column is
// a grid dimension — y of the flat passes, z of the marching pass, x of the one-workgroup scalar kernels —, a workgroup works
// on exactly one column, and the vectors, the state words, the history and the partial sums of column c are those of column 0
// moved by c strides (PcgCols, mgcmt_internal.h).  The stop test is per column, the first thing a workgroup does and uniform
// over it (the reductions have barriers): a frozen column's workgroups return while the others go on.  Per column the number of
// workgroups and the order of every sum are those of k = 1, so a column carries the bits of the same system solved alone.  A
// column that sets its stop word also adds one to the block's count of stopped columns (an atomic: nothing else passes between
// workgroups of a launch), which is all the host reads to decide whether to queue more.
#include <initializer_list>

#include "rq_common.h"

namespace mgcmt {

namespace {

constexpr int kPcgThreads = kRqThreads;

__device__ __forceinline__ bool pcg_finite(double v) { return fabs(v) <= 1.7e308; }  // (false for NaN and the infinities)

// the element type of a pass: two points per access, or one
template <bool VEC2>
struct PcgElem {
  typedef double type;
};
template <>
struct PcgElem<true> {
  typedef double2 type;
};

__device__ __forceinline__ double pcg_prod(double a, double b) { return a * b; }
__device__ __forceinline__ double pcg_prod(double2 a, double2 b) { return a.x * b.x + a.y * b.y; }
__device__ __forceinline__ double pcg_fma(double s, double a, double b) { return fma(s, a, b); }
__device__ __forceinline__ double2 pcg_fma(double s, double2 a, double2 b) { return make_double2(fma(s, a.x, b.x), fma(s, a.y, b.y)); }
__device__ __forceinline__ double pcg_sub(double a, double b) { return a - b; }
__device__ __forceinline__ double2 pcg_sub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ void pcg_zero(double& a) { a = 0.0; }
__device__ __forceinline__ void pcg_zero(double2& a) { a = make_double2(0.0, 0.0); }

// the sums of NQ results' partial sums, by one workgroup, into s_tot[0..NQ) (fixed order)
template <int NQ>
__device__ __forceinline__ void pcg_totals(const double* __restrict__ partials, int nblocks, double (*s_part)[kPcgThreads / 64], double* s_tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    double t = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kPcgThreads) t += partials[(long)q * nblocks + i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) t += __shfl_down(t, d);
    if (lane == 0) s_part[q][wave] = t;
  }
  __syncthreads();
  if ((int)threadIdx.x < NQ) {
    double t = 0.0;
    for (int k = 0; k < kPcgThreads / 64; ++k) t += s_part[threadIdx.x][k];
    s_tot[threadIdx.x] = t;
  }
  __syncthreads();
}

// the column's stop word and status (1 converged, 2 breakdown); set once per solve, so the count of stopped columns gets one
__device__ __forceinline__ void pcg_stop(double* __restrict__ state, unsigned* stopped, double status) {
  state[kPcgStop] = 1.0;
  state[kPcgStatus] = status;
  atomicAdd(stopped, 1u);
}
__device__ __forceinline__ void pcg_break(double* __restrict__ state, unsigned* stopped) { pcg_stop(state, stopped, 2.0); }

// column `col` of a block: its state words, history, partial sums
__device__ __forceinline__ double* pcg_col_state(const PcgCols& c, int col) { return c.state + (long)col * kPcgStateWords; }
__device__ __forceinline__ double* pcg_col_history(const PcgCols& c, int col) { return c.history + (long)col * MGCMT_RQ_HISTORY; }
__device__ __forceinline__ double* pcg_col_partials(const PcgCols& c, int col) { return c.partials + (long)col * kPcgColPartials; }

// ---- begin: r = f - (A - mu I) x0 in place, ||f||^2 and ||r_0||^2 ----------------------------------------------------------
template <bool VEC2>
__global__ void __launch_bounds__(kPcgThreads) k_pcg_begin(long n, double* __restrict__ r_, const double* __restrict__ q_, double* __restrict__ x_,
                                                           PcgCols cols) {
  typedef typename PcgElem<VEC2>::type E;
  __shared__ double s_part[kPcgSums][kPcgThreads / 64];
  const int col = blockIdx.y;
  double* partials = pcg_col_partials(cols, col);
  E* r = (E*)(r_ + col * cols.stride);
  const E* q = q_ ? (const E*)(q_ + col * cols.stride) : nullptr;
  E* x = x_ ? (E*)(x_ + col * cols.stride) : nullptr;
  double acc[kPcgSums] = {0.0, 0.0};
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    E rv = r[i];
    acc[0] += pcg_prod(rv, rv);
    if (q) {
      rv = pcg_sub(rv, q[i]);
      r[i] = rv;
    } else {
      E zero;
      pcg_zero(zero);
      x[i] = zero;
    }
    acc[1] += pcg_prod(rv, rv);
  }
  block_partials<kPcgSums>(acc, s_part, partials, gridDim.x, blockIdx.x);
}

__global__ void __launch_bounds__(kPcgThreads) k_pcg_begin_scalars(PcgCols cols, int nblocks, double rtol, int flexible) {
  __shared__ double s_part[kPcgSums][kPcgThreads / 64];
  __shared__ double s_tot[kPcgSums];
  const int col = blockIdx.x;
  const double* partials = pcg_col_partials(cols, col);
  double* state = pcg_col_state(cols, col);
  double* history = pcg_col_history(cols, col);
  pcg_totals<kPcgSums>(partials, nblocks, s_part, s_tot);
  for (int i = threadIdx.x; i < MGCMT_RQ_HISTORY; i += kPcgThreads) history[i] = 0.0;
  if (threadIdx.x != 0) return;
  for (int w = 0; w < kPcgStateWords; ++w) state[w] = 0.0;
  const double ff = s_tot[0], rr = s_tot[1];
  const double fnorm = sqrt(ff), rnorm = sqrt(rr);
  state[kPcgRR] = rr;
  state[kPcgFnorm] = fnorm;
  state[kPcgR0norm] = rnorm;
  state[kPcgRtol] = rtol;
  state[kPcgFlexible] = flexible ? 1.0 : 0.0;
  if (!pcg_finite(ff) || !pcg_finite(rr)) {
    pcg_break(state, cols.stopped);
  } else if (rnorm <= rtol * fnorm) {  // the start vector already solves the system (f = 0 included)
    pcg_stop(state, cols.stopped, 1.0);
  }
}

// ---- dots: rho = <z, r>, sigma = <z, q> (q: the previous iteration's (A - mu I) p; not read on the first) -------------------
template <bool VEC2>
__global__ void __launch_bounds__(kPcgThreads) k_pcg_dots(long n, const double* __restrict__ z_, const double* __restrict__ r_,
                                                          const double* __restrict__ q_, PcgCols cols) {
  const int col = blockIdx.y;
  const double* state = pcg_col_state(cols, col);
  if (state[kPcgStop] != 0.0) return;
  typedef typename PcgElem<VEC2>::type E;
  __shared__ double s_part[kPcgSums][kPcgThreads / 64];
  double* partials = pcg_col_partials(cols, col);
  const E* z = (const E*)(z_ + col * cols.stride);
  const E* r = (const E*)(r_ + col * cols.stride);
  const E* q = (const E*)(q_ + col * cols.stride);
  const bool first = state[kPcgIter] == 0.0;
  double acc[kPcgSums] = {0.0, 0.0};
  if (first) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) acc[0] += pcg_prod(z[i], r[i]);
  } else {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
      const E zv = z[i];
      acc[0] += pcg_prod(zv, r[i]);
      acc[1] += pcg_prod(zv, q[i]);
    }
  }
  block_partials<kPcgSums>(acc, s_part, partials, gridDim.x, blockIdx.x);
}

// beta: rho / rho_old, or the flexible form -alpha_old sigma / rho_old — Polak-Ribiere's <z, r - r_old> / rho_old with
// r - r_old = -alpha_old q, which needs no copy of r_old and equals the first form when the preconditioner is symmetric
__global__ void __launch_bounds__(kPcgThreads) k_pcg_beta(PcgCols cols, int nblocks) {
  const int col = blockIdx.x;
  double* state = pcg_col_state(cols, col);
  if (state[kPcgStop] != 0.0) return;
  const double* partials = pcg_col_partials(cols, col);
  __shared__ double s_part[kPcgSums][kPcgThreads / 64];
  __shared__ double s_tot[kPcgSums];
  pcg_totals<kPcgSums>(partials, nblocks, s_part, s_tot);
  if (threadIdx.x != 0) return;
  const double rho = s_tot[0], sigma = s_tot[1];
  const bool first = state[kPcgIter] == 0.0;
  if (!pcg_finite(rho) || rho == 0.0 || !pcg_finite(sigma)) {
    pcg_break(state, cols.stopped);
    return;
  }
  const double rho_old = state[kPcgRho];
  double beta = 0.0;
  if (!first) beta = state[kPcgFlexible] != 0.0 ? -(state[kPcgAlpha] * sigma) / rho_old : rho / rho_old;
  if (!pcg_finite(beta)) {
    pcg_break(state, cols.stopped);
    return;
  }
  if (rho < 0.0) state[kPcgIndefinite] = 1.0;
  state[kPcgRhoOld] = rho_old;
  state[kPcgRho] = rho;
  state[kPcgSigma] = sigma;
  state[kPcgBeta] = beta;
}

// ---- direction: p <- z + beta p (the first iteration: p <- z, p not read) ---------------------------------------------------
template <bool VEC2>
__global__ void __launch_bounds__(kPcgThreads) k_pcg_direction(long n, const double* __restrict__ z_, double* __restrict__ p_, PcgCols cols) {
  const int col = blockIdx.y;
  const double* state = pcg_col_state(cols, col);
  if (state[kPcgStop] != 0.0) return;
  typedef typename PcgElem<VEC2>::type E;
  const E* z = (const E*)(z_ + col * cols.stride);
  E* p = (E*)(p_ + col * cols.stride);
  const double beta = state[kPcgBeta];
  if (state[kPcgIter] == 0.0) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = z[i];
  } else {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = pcg_fma(beta, p[i], z[i]);
  }
}

// ---- curvature: <p, q> -----------------------------------------------------------------------------------------------------------
template <bool VEC2>
__global__ void __launch_bounds__(kPcgThreads) k_pcg_curvature(long n, const double* __restrict__ p_, const double* __restrict__ q_,
                                                               PcgCols cols) {
  const int col = blockIdx.y;
  const double* state = pcg_col_state(cols, col);
  if (state[kPcgStop] != 0.0) return;
  typedef typename PcgElem<VEC2>::type E;
  __shared__ double s_part[1][kPcgThreads / 64];
  double* partials = pcg_col_partials(cols, col);
  const E* p = (const E*)(p_ + col * cols.stride);
  const E* q = (const E*)(q_ + col * cols.stride);
  double acc[1] = {0.0};
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) acc[0] += pcg_prod(p[i], q[i]);
  block_partials<1>(acc, s_part, partials, gridDim.x, blockIdx.x);
}

__global__ void __launch_bounds__(kPcgThreads) k_pcg_alpha(PcgCols cols, int nblocks) {
  const int col = blockIdx.x;
  double* state = pcg_col_state(cols, col);
  if (state[kPcgStop] != 0.0) return;
  const double* partials = pcg_col_partials(cols, col);
  __shared__ double s_part[1][kPcgThreads / 64];
  __shared__ double s_tot[1];
  pcg_totals<1>(partials, nblocks, s_part, s_tot);
  if (threadIdx.x != 0) return;
  const double pq = s_tot[0];
  const double alpha = state[kPcgRho] / pq;
  if (!pcg_finite(pq) || pq == 0.0 || !pcg_finite(alpha)) {
    pcg_break(state, cols.stopped);
    return;
  }
  if (pq < 0.0) state[kPcgIndefinite] = 1.0;  // (conjugate gradients go on: the shifted systems next to an eigenvalue converge)
  state[kPcgPq] = pq;
  state[kPcgAlpha] = alpha;
}

// ---- update: x += alpha p, r -= alpha q, <r, r> -----------------------------------------------------------------------------
template <bool VEC2>
__global__ void __launch_bounds__(kPcgThreads) k_pcg_update(long n, double* __restrict__ x_, const double* __restrict__ p_,
                                                            double* __restrict__ r_, const double* __restrict__ q_, PcgCols cols) {
  const int col = blockIdx.y;
  const double* state = pcg_col_state(cols, col);
  if (state[kPcgStop] != 0.0) return;
  typedef typename PcgElem<VEC2>::type E;
  __shared__ double s_part[1][kPcgThreads / 64];
  double* partials = pcg_col_partials(cols, col);
  E* x = (E*)(x_ + col * cols.stride);
  const E* p = (const E*)(p_ + col * cols.stride);
  E* r = (E*)(r_ + col * cols.stride);
  const E* q = (const E*)(q_ + col * cols.stride);
  const double alpha = state[kPcgAlpha];
  double acc[1] = {0.0};
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    x[i] = pcg_fma(alpha, p[i], x[i]);
    const E rv = pcg_fma(-alpha, q[i], r[i]);
    r[i] = rv;
    acc[0] += pcg_prod(rv, rv);
  }
  block_partials<1>(acc, s_part, partials, gridDim.x, blockIdx.x);
}

__global__ void __launch_bounds__(kPcgThreads) k_pcg_norm(PcgCols cols, int nblocks) {
  const int col = blockIdx.x;
  double* state = pcg_col_state(cols, col);
  if (state[kPcgStop] != 0.0) return;
  const double* partials = pcg_col_partials(cols, col);
  double* history = pcg_col_history(cols, col);
  __shared__ double s_part[1][kPcgThreads / 64];
  __shared__ double s_tot[1];
  pcg_totals<1>(partials, nblocks, s_part, s_tot);
  if (threadIdx.x != 0) return;
  const double rr = s_tot[0];
  const double rnorm = sqrt(rr);
  const long it = (long)state[kPcgIter];
  if (it < MGCMT_RQ_HISTORY) history[it] = rnorm;
  state[kPcgIter] = (double)(it + 1);
  state[kPcgRR] = rr;
  if (!pcg_finite(rr)) {
    pcg_break(state, cols.stopped);
  } else if (rnorm <= state[kPcgRtol] * state[kPcgFnorm]) {
    pcg_stop(state, cols.stopped, 1.0);
  }
}

// ---- the marching direction pass: p2 <- z + beta p, q <- (A - mu I) p2, <p2, q> in one launch --------------------------------
// On the 2-D levels k_ritz_march covers (kernels_stencil.hip: a constant 5-point operator, ND = 0, or one with a product
// potential of ND diagonal terms).  The mapping is k_apply_march's: a thread owns two adjacent columns (16-byte accesses) and
// walks down `rows` rows with the new direction's rows above / at / below in registers — formed on the fly from z and the OLD
// p, which is why the new one goes to another vector: the thread to the left and the chunk above still read the old values
// (one overlap row above and below a chunk, one column either side of a thread's pair).  The row's factors dX[m][i] are
// wave-uniform loads.  32 bytes per point (z, p read; p2, q written) instead of the 64 of direction + application + curvature.
// The expressions are k_pcg_direction's and k_apply_march's term by term: p2 and q are theirs bit for bit; the partial sums
// of <p2, q> are per column group and row chunk, added in a fixed order.
template <int ND>
__global__ void __launch_bounds__(256) k_pcg_march(KGrid g, KOp op, const double* __restrict__ z, const double* __restrict__ p,
                                                  double* __restrict__ p2, double* __restrict__ qout, const double* __restrict__ shifts, int rows,
                                                  PcgCols cols, int nblocks) {
  const int col = blockIdx.z;  // its own shift, beta and first flag: a column on its first iteration and one on its fifth share a launch
  const double* state = pcg_col_state(cols, col);
  if (state[kPcgStop] != 0.0) return;
  __shared__ double s_part[1][kPcgThreads / 64];
  double* partials = pcg_col_partials(cols, col);
  z += col * cols.stride;
  p += col * cols.stride;
  p2 += col * cols.stride;
  qout += col * cols.stride;
  const long j = 2 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  const long nc = g.nc;
  const long i0 = (long)blockIdx.y * rows;
  const long i1 = i0 + rows < g.nr ? i0 + rows : g.nr;
  const bool first = state[kPcgIter] == 0.0;  // p <- z: the old p is not read
  const double beta = state[kPcgBeta];
  double acc[1] = {0.0};
  if (j < nc) {
    const bool hw = j > 0, he = j + 2 < nc;
    const long jw = hw ? j - 1 : j, je = he ? j + 2 : j + 1;  // (clamped: the value is discarded)
    const double cn = op.cn, cw = op.cw, d0 = op.c0 - shifts[col];
    double qa[ND > 0 ? ND : 1], qb[ND > 0 ? ND : 1];
#pragma unroll
    for (int m = 0; m < ND; ++m) {
      qa[m] = op.dY[m][j];
      qb[m] = op.dY[m][j + 1];
    }
    // the new direction at two adjacent points / at one point of row i (rows -1 and nr are halo rows: zeros in z and in p)
    auto dir2 = [&](long i) {
      const double2 zv = *reinterpret_cast<const double2*>(z + i * nc + j);
      if (first) return zv;
      const double2 pv = *reinterpret_cast<const double2*>(p + i * nc + j);
      return make_double2(fma(beta, pv.x, zv.x), fma(beta, pv.y, zv.y));
    };
    auto dir1 = [&](long i, long jj) { return first ? z[i * nc + jj] : fma(beta, p[i * nc + jj], z[i * nc + jj]); };
    double2 n = dir2(i0 - 1), c = dir2(i0);
    double w = hw ? dir1(i0, jw) : 0.0, e = he ? dir1(i0, je) : 0.0;
#pragma unroll 2
    for (long i = i0; i < i1; ++i) {
      const double2 sr = dir2(i + 1);
      const double wn = dir1(i + 1, jw), en = dir1(i + 1, je);
      double da = d0, db = d0;
#pragma unroll
      for (int m = 0; m < ND; ++m) {
        const double pm = op.dX[m][i];
        da += pm * qa[m];
        db += pm * qb[m];
      }
      double acc_a = cw * (w + c.y), acc_b = cw * (c.x + e);
      acc_a += cn * (n.x + sr.x);
      acc_b += cn * (n.y + sr.y);
      const double ha = acc_a + da * c.x, hb = acc_b + db * c.y;
      *reinterpret_cast<double2*>(p2 + i * nc + j) = c;
      *reinterpret_cast<double2*>(qout + i * nc + j) = make_double2(ha, hb);
      acc[0] += c.x * ha + c.y * hb;
      n = c;
      c = sr;
      w = hw ? wn : 0.0;
      e = he ? en : 0.0;
    }
  }
  block_partials<1>(acc, s_part, partials, nblocks, (int)(blockIdx.y * gridDim.x + blockIdx.x));
}

// 16-byte accesses when every vector allows them (k columns: every column's start, `stride` doubles apart)
bool pcg_vec2(long n, const PcgCols& c, std::initializer_list<const void*> ptrs) {
  if (n & 1) return false;
  if (c.k > 1 && (c.stride & 1)) return false;
  for (const void* p : ptrs)
    if (p && ((uintptr_t)p & 15)) return false;
  return true;
}

// workgroups of a pass over m elements of ONE column: eight per thread, at most kPcgMaxBlocks (never a function of the
// column count: a column's partial sums, and with them its bits, are those of the single solve)
int pcg_blocks(long m) {
  long b = (m + (long)kPcgThreads * 8 - 1) / ((long)kPcgThreads * 8);
  if (b > kPcgMaxBlocks) b = kPcgMaxBlocks;
  return b < 1 ? 1 : (int)b;
}

}  // namespace

// Launch geometry: a flat pass is (pcg_blocks, k) workgroups of 256 threads, the scalar kernel behind it k workgroups.

void launch_pcg_begin(hipStream_t s, long n, double* r, const double* q, double* x, const PcgCols& c, double rtol, int flexible) {
  const bool v2 = pcg_vec2(n, c, {r, q, x});
  const long m = v2 ? n / 2 : n;
  const int nb = pcg_blocks(m);
  if (v2) hipLaunchKernelGGL(k_pcg_begin<true>, dim3(nb, c.k), dim3(kPcgThreads), 0, s, m, r, q, x, c);
  else hipLaunchKernelGGL(k_pcg_begin<false>, dim3(nb, c.k), dim3(kPcgThreads), 0, s, m, r, q, x, c);
  hipLaunchKernelGGL(k_pcg_begin_scalars, dim3(c.k), dim3(kPcgThreads), 0, s, c, nb, rtol, flexible);
}

void launch_pcg_dots(hipStream_t s, long n, const double* z, const double* r, const double* q, const PcgCols& c) {
  const bool v2 = pcg_vec2(n, c, {z, r, q});
  const long m = v2 ? n / 2 : n;
  const int nb = pcg_blocks(m);
  if (v2) hipLaunchKernelGGL(k_pcg_dots<true>, dim3(nb, c.k), dim3(kPcgThreads), 0, s, m, z, r, q, c);
  else hipLaunchKernelGGL(k_pcg_dots<false>, dim3(nb, c.k), dim3(kPcgThreads), 0, s, m, z, r, q, c);
  hipLaunchKernelGGL(k_pcg_beta, dim3(c.k), dim3(kPcgThreads), 0, s, c, nb);
}

void launch_pcg_direction(hipStream_t s, long n, const double* z, double* p, const PcgCols& c) {
  const bool v2 = pcg_vec2(n, c, {z, p});
  const long m = v2 ? n / 2 : n;
  const int nb = pcg_blocks(m);
  if (v2) hipLaunchKernelGGL(k_pcg_direction<true>, dim3(nb, c.k), dim3(kPcgThreads), 0, s, m, z, p, c);
  else hipLaunchKernelGGL(k_pcg_direction<false>, dim3(nb, c.k), dim3(kPcgThreads), 0, s, m, z, p, c);
}

void launch_pcg_curvature(hipStream_t s, long n, const double* p, const double* q, const PcgCols& c) {
  const bool v2 = pcg_vec2(n, c, {p, q});
  const long m = v2 ? n / 2 : n;
  const int nb = pcg_blocks(m);
  if (v2) hipLaunchKernelGGL(k_pcg_curvature<true>, dim3(nb, c.k), dim3(kPcgThreads), 0, s, m, p, q, c);
  else hipLaunchKernelGGL(k_pcg_curvature<false>, dim3(nb, c.k), dim3(kPcgThreads), 0, s, m, p, q, c);
  hipLaunchKernelGGL(k_pcg_alpha, dim3(c.k), dim3(kPcgThreads), 0, s, c, nb);
}

bool launch_pcg_march(hipStream_t s, KGrid g, KOp op, const double* z, const double* p, double* p2, double* q, const double* shifts, const PcgCols& c) {
  if (op.point) return false;
  const bool aligned = (((uintptr_t)z | (uintptr_t)p | (uintptr_t)p2 | (uintptr_t)q) & 15) == 0 && (c.k == 1 || (c.stride & 1) == 0);
  // (the levels launch_ritz_pair and the marching launch_apply take)
  if (!(g.coarsen_rows && g.nr >= 2 && g.nc >= 2 && (g.nc & 1) == 0 && aligned && ((op.five_point && op.cn != 0.0) || (op.five_diag && op.ndiag <= 2))))
    return false;
  const dim3 b(g.nc >= 512 ? 256 : 64, 1, 1);
  const unsigned gx = (unsigned)((g.nc / 2 + b.x - 1) / b.x);
  long rows = 32;  // row chunks as short as the partial sums allow, not shorter than an application's
  while ((long)gx * ((g.nr + rows - 1) / rows) > kPcgPartialCap) rows *= 2;
  const dim3 grid(gx, (unsigned)((g.nr + rows - 1) / rows), (unsigned)c.k);  // z: the column
  const int nblocks = (int)(grid.x * grid.y);
  if (op.five_point) hipLaunchKernelGGL(k_pcg_march<0>, grid, b, 0, s, g, op, z, p, p2, q, shifts, (int)rows, c, nblocks);
  else if (op.ndiag == 1) hipLaunchKernelGGL(k_pcg_march<1>, grid, b, 0, s, g, op, z, p, p2, q, shifts, (int)rows, c, nblocks);
  else hipLaunchKernelGGL(k_pcg_march<2>, grid, b, 0, s, g, op, z, p, p2, q, shifts, (int)rows, c, nblocks);
  hipLaunchKernelGGL(k_pcg_alpha, dim3(c.k), dim3(kPcgThreads), 0, s, c, nblocks);
  return true;
}

void launch_pcg_update(hipStream_t s, long n, double* x, const double* p, double* r, const double* q, const PcgCols& c) {
  const bool v2 = pcg_vec2(n, c, {x, p, r, q});
  const long m = v2 ? n / 2 : n;
  const int nb = pcg_blocks(m);
  if (v2) hipLaunchKernelGGL(k_pcg_update<true>, dim3(nb, c.k), dim3(kPcgThreads), 0, s, m, x, p, r, q, c);
  else hipLaunchKernelGGL(k_pcg_update<false>, dim3(nb, c.k), dim3(kPcgThreads), 0, s, m, x, p, r, q, c);
  hipLaunchKernelGGL(k_pcg_norm, dim3(c.k), dim3(kPcgThreads), 0, s, c, nb);
}

}  // namespace mgcmt
