// Wide block operations of the blocked Rayleigh-Ritz eigen-solver (drivers.block_eigensolve with more than four states;
// DESIGN.md par. 4.11b): the pencil H = S^T AS, G = S^T MS of up to 48 trial vectors in ONE pass over them, accumulated on
// the matrix cores (v_mfma_f64_16x16x4_f64), and the tall-skinny product OUT = IN C with up to 48 inputs and 16 outputs.
//
// Pencil.  The contracted index of S^T AS is the grid point, so a 16 x 16 tile of H is a chain of 16x16x4 products over runs
// of four points: A[i][k] = S_(16 I + i)(p + k), B[k][j] = AS_(16 J + j)(p + k).  Lane l of a wave holds A[l & 15][l >> 4] and
// B[l >> 4][l & 15]: the vector index is l & 15 and the point index l >> 4 in BOTH operands, so one register of S serves
// as A (of H and of G) and, when M = I, as B of G.  A sum over points has no prescribed order: each of the four K lane
// groups streams its own run of kRun = 4 contiguous points per block step (two 16-byte loads per lane and vector; the four
// groups of a wave cover 128 contiguous bytes of every vector), and the S and AS operands of one product see the same
// point.  m is padded to whole tiles with zero operands; vectors the call did not name are never read.
// Deterministic: a fixed point -> (block, wave, lane, trip) map, waves summed 0..3 through LDS, blocks summed 0..nb-1 by
// k_pencil_final.
#include <cstring>

#include "mgcmt_internal.h"

namespace mgcmt {
namespace {

constexpr int kWideThreads = 256, kWideWaves = kWideThreads / 64;
constexpr int kRun = 4;                                // points per lane and block step
constexpr int kStepPoints = kWideWaves * 4 * kRun;     // points per block step: 64
constexpr int kPencilMaxBlocks = 512;
constexpr int kTile = 16, kTileWords = kTile * kTile;

// D += A B on one 16 x 16 x 4 tile; c[r] is D[(lane >> 4) + 4 r][lane & 15].  The host-side build (the CPU emulation of
// the tests, and the host pass of hipcc, which never runs it) has no matrix cores: the same lane <-> element maps on wave
// shuffles, the four products of an entry summed k = 0..3.
__device__ __forceinline__ void mfma_f64_16x16x4(double a, double b, double (&c)[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef double v4d __attribute__((ext_vector_type(4)));
  v4d cv = {c[0], c[1], c[2], c[3]};
  cv = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, cv, 0, 0, 0);
  c[0] = cv[0];
  c[1] = cv[1];
  c[2] = cv[2];
  c[3] = cv[3];
#else
  const int lane = threadIdx.x & 63;
  double bk[4];
  for (int k = 0; k < 4; ++k) bk[k] = __shfl(b, (lane & 15) + 16 * k);  // B[k][col]
  for (int r = 0; r < 4; ++r) {
    const int row = (lane >> 4) + 4 * r;
    for (int k = 0; k < 4; ++k) c[r] = fma(__shfl(a, row + 16 * k), bk[k], c[r]);  // A[row][k]
  }
#endif
}

// x[q] = v[p + q] for the points below n, zero beyond them and for a padding lane (v == nullptr); v is 16-byte aligned
// and p a multiple of kRun (the launcher refuses anything else)
__device__ __forceinline__ void load_run(const double* v, long p, long n, double (&x)[kRun]) {
  if (v != nullptr && p + kRun <= n) {
    const double2 a = reinterpret_cast<const double2*>(v + p)[0], b = reinterpret_cast<const double2*>(v + p)[1];
    x[0] = a.x;
    x[1] = a.y;
    x[2] = b.x;
    x[3] = b.y;
  } else {
#pragma unroll
    for (int q = 0; q < kRun; ++q) x[q] = (v != nullptr && p + q < n) ? v[p + q] : 0.0;
  }
}

struct PencilArgs {
  const double* s[kBlockWideMax];
  const double* as[kBlockWideMax];
  const double* ms[kBlockWideMax];  // (MASS only)
};

// tiles of one launch, in the order of the partial sums: H (I, J) row-major, then G (I, J) row-major — all of them with a
// mass operator, the upper triangle J >= I without (G = S^T S is symmetric to the last bit; the host mirrors it)
__host__ __device__ constexpr int pencil_tiles(int t, bool mass) { return t * t + (mass ? t * t : t * (t + 1) / 2); }

// T: tiles per side (m <= 16 T)
template <int T, bool MASS>
__global__ void __launch_bounds__(kWideThreads) k_block_pencil(long n, PencilArgs g, int m, double* __restrict__ partials) {
  __shared__ double s_red[kWideWaves - 1][kTileWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, kg = lane >> 4;
  const double *ps[T], *pa[T], *pm[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int v = kTile * t + col;
    ps[t] = v < m ? g.s[v] : nullptr;
    pa[t] = v < m ? g.as[v] : nullptr;
    pm[t] = (MASS && v < m) ? g.ms[v] : nullptr;
  }
  double acc_h[T][T][4], acc_g[T][T][4];
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int j = 0; j < T; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc_h[i][j][r] = acc_g[i][j][r] = 0.0;

  const long nsteps = (n + kStepPoints - 1) / kStepPoints;
  const long lane_off = (long)(wave * 4 + kg) * kRun;
  double xs[T][kRun], xa[T][kRun], xm[T][kRun], ys[T][kRun], ya[T][kRun], ym[T][kRun];
  long step = blockIdx.x;  // (every wave of a block takes the same trips: the emulation's shuffles need whole workgroups)
  if (step < nsteps) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      load_run(ps[t], step * kStepPoints + lane_off, n, xs[t]);
      load_run(pa[t], step * kStepPoints + lane_off, n, xa[t]);
      if (MASS) load_run(pm[t], step * kStepPoints + lane_off, n, xm[t]);
    }
  }
  for (; step < nsteps; step += gridDim.x) {
    const long next = step + gridDim.x;
    if (next < nsteps) {  // the next step's operands are in flight while this step's products run
#pragma unroll
      for (int t = 0; t < T; ++t) {
        load_run(ps[t], next * kStepPoints + lane_off, n, ys[t]);
        load_run(pa[t], next * kStepPoints + lane_off, n, ya[t]);
        if (MASS) load_run(pm[t], next * kStepPoints + lane_off, n, ym[t]);
      }
    }
#pragma unroll
    for (int q = 0; q < kRun; ++q)
#pragma unroll
      for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) {
          mfma_f64_16x16x4(xs[i][q], xa[j][q], acc_h[i][j]);
          if (MASS) mfma_f64_16x16x4(xs[i][q], xm[j][q], acc_g[i][j]);
          else if (j >= i) mfma_f64_16x16x4(xs[i][q], xs[j][q], acc_g[i][j]);
        }
    if (next < nsteps) {
#pragma unroll
      for (int t = 0; t < T; ++t)
#pragma unroll
        for (int q = 0; q < kRun; ++q) {
          xs[t][q] = ys[t][q];
          xa[t][q] = ya[t][q];
          if (MASS) xm[t][q] = ym[t][q];
        }
    }
  }

  // waves 1..3 hand their tile to wave 0 through LDS, one tile at a time; wave 0 adds them in wave order and stores the
  // block's partial tile row-major: partials[(tile * gridDim.x + block) * 256 + row * 16 + col]
  int tile = 0;
#pragma unroll
  for (int which = 0; which < 2; ++which)
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
      for (int j = 0; j < T; ++j) {
        if (which == 1 && !MASS && j < i) continue;
        const double(&acc)[4] = which == 0 ? acc_h[i][j] : acc_g[i][j];
        if (wave > 0) {
#pragma unroll
          for (int r = 0; r < 4; ++r) s_red[wave - 1][r * 64 + lane] = acc[r];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double tot = acc[r];
            for (int w = 0; w < kWideWaves - 1; ++w) tot += s_red[w][r * 64 + lane];
            partials[((long)tile * gridDim.x + blockIdx.x) * kTileWords + (kg + 4 * r) * kTile + col] = tot;
          }
        }
        __syncthreads();
        ++tile;
      }
}

// out[tile * 256 + e] = sum over blocks b = 0..nb-1, in that order, of partials[(tile * nb + b) * 256 + e]
__global__ void __launch_bounds__(kTileWords) k_pencil_final(int nb, const double* __restrict__ partials, double* __restrict__ out) {
  const double* src = partials + (long)blockIdx.x * nb * kTileWords + threadIdx.x;
  double tot = 0.0;
  for (int b = 0; b < nb; ++b) tot += src[(long)b * kTileWords];
  out[(long)blockIdx.x * kTileWords + threadIdx.x] = tot;
}

// The table of a wide combine in device memory (48 x 16 coefficients do not fit the kernel arguments): kWideCoefWords
// coefficients c[t][j] (rows of 16, zero beyond nout), then the input and the output pointers.  Filled stream-ordered by
// k_wide_stage from chunks that travel as kernel arguments, so nothing depends on the lifetime of host memory.
constexpr int kWideCoefWords = kBlockWideMax * kBlockWideOut;
constexpr int kStageWords = 416;  // (half the table: 3.3 KB of kernel arguments)
struct StageArgs {
  unsigned long long w[kStageWords];
};
__global__ void __launch_bounds__(kWideThreads) k_wide_stage(unsigned long long* __restrict__ table, int offset, int count, StageArgs a) {
  for (int t = threadIdx.x; t < count; t += blockDim.x) table[offset + t] = a.w[t];
}

// OUT_j = sum_t c[t][j] IN_t on the vector ALUs (about 3 flop per byte moved: far below what they sustain per byte of
// HBM traffic, and a thread that owns its points keeps "all inputs of a point are read before any output of it is
// written" true by construction, so an output may be one of the inputs).  The coefficients and pointers are wave-uniform:
// they come through the scalar cache.  Two points per thread and 16-byte accesses (n even, every vector 16-byte aligned:
// the launcher refuses anything else).
__global__ void __launch_bounds__(kWideThreads) k_block_combine_wide(long n2, const unsigned long long* __restrict__ table, int nin, int nout) {
  const double* __restrict__ coef = reinterpret_cast<const double*>(table);
  const double* const* in = reinterpret_cast<const double* const*>(table + kWideCoefWords);
  double* const* out = reinterpret_cast<double* const*>(table + kWideCoefWords + kBlockWideMax);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long)gridDim.x * blockDim.x) {
    double2 acc[kBlockWideOut];
#pragma unroll
    for (int j = 0; j < kBlockWideOut; ++j) acc[j] = make_double2(0.0, 0.0);
#pragma unroll 4
    for (int t = 0; t < nin; ++t) {
      const double* c = coef + t * kBlockWideOut;
      const double2 x = reinterpret_cast<const double2*>(in[t])[i];
#pragma unroll
      for (int j = 0; j < kBlockWideOut; ++j) {
        acc[j].x = fma(c[j], x.x, acc[j].x);
        acc[j].y = fma(c[j], x.y, acc[j].y);
      }
    }
#pragma unroll
    for (int j = 0; j < kBlockWideOut; ++j)
      if (j < nout) reinterpret_cast<double2*>(out[j])[i] = acc[j];
  }
}

// Deflation W_j <- W_j - sum_i <Q_i, W_j> Q_i against up to 64 locked vectors Q (drivers.deflated_eigensolve; DESIGN.md
// par. 4.21) in two launches.  The 64 + 16 pointers travel as kernel arguments (640 bytes): no table is staged.
struct DeflateArgs {
  const double* q[kBlockLockedMax];
  double* w[kBlockWideOut];
};

// Pass 1: C = Q^T W, TQ x 1 tiles of the pencil's products — A[i][k] = Q_(16 I + i)(p + k), B[k][j] = W_j(p + k) — with the
// pencil's lane <-> element map, runs, prefetch, trips and sums.  The partial tile of block b and tile I is
// partials[(I * gridDim.x + b) * 256 + row * 16 + col]; k_pencil_final leaves C row-major, 16 columns per Q.
template <int TQ>
__global__ void __launch_bounds__(kWideThreads) k_block_cross(long n, DeflateArgs g, int nq, int k, double* __restrict__ partials) {
  __shared__ double s_red[kWideWaves - 1][kTileWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, kg = lane >> 4;
  const double *pq[TQ], *pw = col < k ? g.w[col] : nullptr;
#pragma unroll
  for (int t = 0; t < TQ; ++t) pq[t] = kTile * t + col < nq ? g.q[kTile * t + col] : nullptr;
  double acc[TQ][4];
#pragma unroll
  for (int t = 0; t < TQ; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[t][r] = 0.0;

  const long nsteps = (n + kStepPoints - 1) / kStepPoints;
  const long lane_off = (long)(wave * 4 + kg) * kRun;
  double xq[TQ][kRun], xw[kRun], yq[TQ][kRun], yw[kRun];
  long step = blockIdx.x;  // (every wave of a block takes the same trips: the emulation's shuffles need whole workgroups)
  if (step < nsteps) {
#pragma unroll
    for (int t = 0; t < TQ; ++t) load_run(pq[t], step * kStepPoints + lane_off, n, xq[t]);
    load_run(pw, step * kStepPoints + lane_off, n, xw);
  }
  for (; step < nsteps; step += gridDim.x) {
    const long next = step + gridDim.x;
    if (next < nsteps) {  // the next step's operands are in flight while this step's products run
#pragma unroll
      for (int t = 0; t < TQ; ++t) load_run(pq[t], next * kStepPoints + lane_off, n, yq[t]);
      load_run(pw, next * kStepPoints + lane_off, n, yw);
    }
#pragma unroll
    for (int q = 0; q < kRun; ++q)
#pragma unroll
      for (int t = 0; t < TQ; ++t) mfma_f64_16x16x4(xq[t][q], xw[q], acc[t]);
    if (next < nsteps) {
#pragma unroll
      for (int q = 0; q < kRun; ++q) {
#pragma unroll
        for (int t = 0; t < TQ; ++t) xq[t][q] = yq[t][q];
        xw[q] = yw[q];
      }
    }
  }

  // waves 1..3 hand their tile to wave 0 through LDS, one tile at a time; wave 0 adds them in wave order
#pragma unroll
  for (int t = 0; t < TQ; ++t) {
    if (wave > 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) s_red[wave - 1][r * 64 + lane] = acc[t][r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double tot = acc[t][r];
        for (int w = 0; w < kWideWaves - 1; ++w) tot += s_red[w][r * 64 + lane];
        partials[((long)t * gridDim.x + blockIdx.x) * kTileWords + (kg + 4 * r) * kTile + col] = tot;
      }
    }
    __syncthreads();
  }
}

// Pass 2: W_j <- W_j - sum_i c[i][j] Q_i on the vector ALUs, as k_block_combine_wide: a thread owns two points, the
// accumulators start as W_j, the coefficient rows c[i][0..15] (the summed tiles of pass 1, zero beyond k) and the pointers are
// wave-uniform and come through the scalar cache.  Columns j >= k are neither read nor stored.
__global__ void __launch_bounds__(kWideThreads) k_block_deflate(long n2, DeflateArgs g, int nq, int k, const double* __restrict__ coef) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long)gridDim.x * blockDim.x) {
    double2 acc[kBlockWideOut];
#pragma unroll
    for (int j = 0; j < kBlockWideOut; ++j) acc[j] = j < k ? reinterpret_cast<const double2*>(g.w[j])[i] : make_double2(0.0, 0.0);
#pragma unroll 4
    for (int t = 0; t < nq; ++t) {
      const double* c = coef + t * kBlockWideOut;
      const double2 x = reinterpret_cast<const double2*>(g.q[t])[i];
#pragma unroll
      for (int j = 0; j < kBlockWideOut; ++j) {
        acc[j].x = fma(-c[j], x.x, acc[j].x);
        acc[j].y = fma(-c[j], x.y, acc[j].y);
      }
    }
#pragma unroll
    for (int j = 0; j < kBlockWideOut; ++j)
      if (j < k) reinterpret_cast<double2*>(g.w[j])[i] = acc[j];
  }
}

// The density of up to 64 weighted vectors, dst(r) = sum_t w_t x_t(r)^2 (mgcmt_block_density; DESIGN.md par. 4.23), in one
// launch shaped as k_block_deflate: a thread owns two points (16-byte accesses) in a grid-stride loop, the 64 pointers, the 64
// weights and dst travel as kernel arguments (1032 bytes) and are wave-uniform, the t loop is unrolled by four so that four
// vector loads are in flight.  Plain stores, no LDS, no atomics, nothing handed from one workgroup to another.  The arithmetic
// of a point is fixed:
//     acc = 0;  for t = 0 .. nq - 1 ascending:  acc = fma(w_t * x_t, x_t, acc)
// (one rounding in the product w_t * x_t, one in the fused multiply-add), so the result is the same bits from call to call
// and whatever the grid.  Vectors t >= nq are never read.
struct DensityArgs {
  const double* x[kBlockLockedMax];
  double w[kBlockLockedMax];
  double* dst;
};

__global__ void __launch_bounds__(kWideThreads) k_block_density(long n2, DensityArgs g, int nq) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long)gridDim.x * blockDim.x) {
    double2 acc = make_double2(0.0, 0.0);
#pragma unroll 4
    for (int t = 0; t < nq; ++t) {
      const double w = g.w[t];
      const double2 x = reinterpret_cast<const double2*>(g.x[t])[i];
      acc.x = fma(w * x.x, x.x, acc.x);
      acc.y = fma(w * x.y, x.y, acc.y);
    }
    reinterpret_cast<double2*>(g.dst)[i] = acc;
  }
}

// One Cholesky-QR step W <- W T on k <= 16 vectors (mgcmt_block_orthonormalize; DESIGN.md par. 4.22) in three launches.
struct OrthArgs {
  double* w[kBlockWideOut];
};

// Launch 1: G = W^T W, one tile of the pencil's products with ONE operand register per vector serving as A and as B (the
// pencil's G when M = I): W is read once.  Lane <-> element map, runs, prefetch, trips and sums of k_block_pencil; the partial
// tile of block b is partials[b * 256 + row * 16 + col].
__global__ void __launch_bounds__(kWideThreads) k_block_gram16(long n, OrthArgs g, int k, double* __restrict__ partials) {
  __shared__ double s_red[kWideWaves - 1][kTileWords];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, kg = lane >> 4;
  const double* pw = col < k ? g.w[col] : nullptr;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const long nsteps = (n + kStepPoints - 1) / kStepPoints;
  const long lane_off = (long)(wave * 4 + kg) * kRun;
  double xw[kRun], yw[kRun];
  long step = blockIdx.x;  // (every wave of a block takes the same trips: the emulation's shuffles need whole workgroups)
  if (step < nsteps) load_run(pw, step * kStepPoints + lane_off, n, xw);
  for (; step < nsteps; step += gridDim.x) {
    const long next = step + gridDim.x;
    if (next < nsteps) load_run(pw, next * kStepPoints + lane_off, n, yw);  // in flight while this step's products run
#pragma unroll
    for (int q = 0; q < kRun; ++q) mfma_f64_16x16x4(xw[q], xw[q], acc);
    if (next < nsteps) {
#pragma unroll
      for (int q = 0; q < kRun; ++q) xw[q] = yw[q];
    }
  }
  // waves 1..3 hand their tile to wave 0 through LDS; wave 0 adds them in wave order
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) s_red[wave - 1][r * 64 + lane] = acc[r];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double tot = acc[r];
      for (int w = 0; w < kWideWaves - 1; ++w) tot += s_red[w][r * 64 + lane];
      partials[(long)blockIdx.x * kTileWords + (kg + 4 * r) * kTile + col] = tot;
    }
  }
}

// Launch 2, one workgroup, a thread per entry of the tile: the blocks' partial tiles summed 0..nb-1, G symmetrised and
// scaled to a unit diagonal (d_j = G_jj^(-1/2); a column whose G_jj is zero or not finite is dropped), the right-looking
// Cholesky factorisation D G D = R^T R in LDS in column order without pivoting — a column whose pivot is <= drop_tol is
// dropped: its row and column leave the factorisation —, R inverted by back substitution (a thread per column), and
// T = D R^-1 stored as the coefficient rows k_block_transform reads (table[i * 16 + j], zero beyond k and in the row and
// the column of a dropped vector) next to the mask of dropped columns.
__global__ void __launch_bounds__(kTileWords) k_orth_factor(int nb, int k, double drop_tol, const double* __restrict__ partials, double* __restrict__ table,
                                                            unsigned* __restrict__ mask_out) {
  __shared__ double S[kTile][kTile];  // G, then the scaled matrix, overwritten by R (upper triangle)
  __shared__ double C[kTile][kTile];  // R^-1
  __shared__ double d[kTile];
  __shared__ int alive[kTile];
  const int ti = threadIdx.x / kTile, tj = threadIdx.x % kTile;
  {
    const double* src = partials + threadIdx.x;
    double tot = 0.0;
    for (int b = 0; b < nb; ++b) tot += src[(long)b * kTileWords];
    S[ti][tj] = tot;
  }
  __syncthreads();
  if ((int)threadIdx.x < kTile) {
    const int j = threadIdx.x;
    const double gj = S[j][j];
    const bool fine = j < k && gj > 0.0 && gj <= 1.7e308;
    alive[j] = fine ? 1 : 0;
    d[j] = fine ? 1.0 / sqrt(gj) : 0.0;
  }
  __syncthreads();
  const double sym = 0.5 * (S[ti][tj] + S[tj][ti]);
  const bool both = alive[ti] && alive[tj];
  __syncthreads();
  S[ti][tj] = both ? (ti == tj ? 1.0 : sym * d[ti] * d[tj]) : 0.0;
  C[ti][tj] = 0.0;
  __syncthreads();
  for (int t = 0; t < k; ++t) {
    if (!alive[t]) continue;  // (every thread reads the same words: uniform)
    const double piv = S[t][t];
    __syncthreads();
    if (!(piv > drop_tol)) {
      if (ti == t || tj == t) S[ti][tj] = 0.0;
      if (threadIdx.x == 0) alive[t] = 0;
      __syncthreads();
      continue;
    }
    const double r = sqrt(piv);
    if (ti == t && tj >= t) S[t][tj] = tj == t ? r : S[t][tj] / r;
    __syncthreads();
    if (ti > t && tj >= ti) S[ti][tj] -= S[t][ti] * S[t][tj];
    __syncthreads();
  }
  if ((int)threadIdx.x < k && alive[threadIdx.x]) {  // column j of C = R^-1 over the vectors that stayed
    const int j = threadIdx.x;
    C[j][j] = 1.0 / S[j][j];
    for (int i = j - 1; i >= 0; --i) {
      if (!alive[i]) continue;
      double sum = 0.0;
      for (int t = i + 1; t <= j; ++t) sum += S[i][t] * C[t][j];
      C[i][j] = -sum / S[i][i];
    }
  }
  __syncthreads();
  table[ti * kTile + tj] = d[ti] * C[ti][tj];
  if (threadIdx.x == 0) {
    unsigned m = 0;
    for (int j = 0; j < k; ++j) m |= alive[j] ? 0u : 1u << j;
    mask_out[0] = m;
  }
}

// Launch 3: OUT_j = sum_(i <= j) T_ij W_i in place on the vector ALUs, as k_block_deflate: a thread owns two points (16-byte
// accesses), loads its k values and forms the k outputs over the unrolled triangle; the coefficient rows and the mask are
// wave-uniform reads.  A dropped vector is not read and is stored as exact zeros; columns j >= k are neither read nor stored.
__global__ void __launch_bounds__(kWideThreads) k_block_transform(long n2, OrthArgs g, int k, const double* __restrict__ coef,
                                                                  const unsigned* __restrict__ mask) {
  const unsigned dropped = mask[0];
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long)gridDim.x * blockDim.x) {
    double2 x[kBlockWideOut];
#pragma unroll
    for (int t = 0; t < kBlockWideOut; ++t)
      x[t] = (t < k && !((dropped >> t) & 1u)) ? reinterpret_cast<const double2*>(g.w[t])[i] : make_double2(0.0, 0.0);
    // output j needs the inputs i <= j only: from the last column down, each output takes its input's registers
#pragma unroll
    for (int j = kBlockWideOut - 1; j >= 0; --j) {
      if (j < k) {  // (wave-uniform)
        double2 a = make_double2(coef[j * kBlockWideOut + j] * x[j].x, coef[j * kBlockWideOut + j] * x[j].y);
#pragma unroll
        for (int t = 0; t < j; ++t) {
          a.x = fma(coef[t * kBlockWideOut + j], x[t].x, a.x);
          a.y = fma(coef[t * kBlockWideOut + j], x[t].y, a.y);
        }
        x[j] = ((dropped >> j) & 1u) ? make_double2(0.0, 0.0) : a;
      }
    }
#pragma unroll
    for (int j = 0; j < kBlockWideOut; ++j)
      if (j < k) reinterpret_cast<double2*>(g.w[j])[i] = x[j];
  }
}

}  // namespace

int block_pencil_blocks(long n) {
  long b = (n + kStepPoints - 1) / kStepPoints;
  if (b > kPencilMaxBlocks) b = kPencilMaxBlocks;
  if (b < 1) b = 1;
  return (int)b;
}

int block_pencil_tiles(int m, bool mass) { return pencil_tiles((m + kTile - 1) / kTile, mass); }

long block_wide_table_words() { return kWideCoefWords + kBlockWideMax + kBlockWideOut; }

// out (device) = the tiles of H then G, 256 numbers each, row-major inside a tile, in the order of pencil_tiles;
// `partials` holds block_pencil_tiles(m, ms != nullptr) * block_pencil_blocks(n) * 256 doubles.  false (nothing launched): a
// vector is not 16-byte aligned — no level of a plan has such vectors
bool launch_block_pencil(hipStream_t s, long n, int m, const double* const* sv, const double* const* as, const double* const* ms, double* partials,
                         double* out) {
  PencilArgs g{};
  uintptr_t bits = 0;
  for (int t = 0; t < kBlockWideMax; ++t) {
    g.s[t] = sv[t < m ? t : 0];
    g.as[t] = as[t < m ? t : 0];
    g.ms[t] = ms ? ms[t < m ? t : 0] : nullptr;
    if (t < m) bits |= (reinterpret_cast<uintptr_t>(sv[t]) | reinterpret_cast<uintptr_t>(as[t]) | (ms ? reinterpret_cast<uintptr_t>(ms[t]) : 0)) & 15;
  }
  if (bits != 0) return false;
  const int blocks = block_pencil_blocks(n), tiles = (m + kTile - 1) / kTile;
  const dim3 grid(blocks), block(kWideThreads);
  if (ms) {
    if (tiles == 1) hipLaunchKernelGGL((k_block_pencil<1, true>), grid, block, 0, s, n, g, m, partials);
    else if (tiles == 2) hipLaunchKernelGGL((k_block_pencil<2, true>), grid, block, 0, s, n, g, m, partials);
    else hipLaunchKernelGGL((k_block_pencil<3, true>), grid, block, 0, s, n, g, m, partials);
  } else {
    if (tiles == 1) hipLaunchKernelGGL((k_block_pencil<1, false>), grid, block, 0, s, n, g, m, partials);
    else if (tiles == 2) hipLaunchKernelGGL((k_block_pencil<2, false>), grid, block, 0, s, n, g, m, partials);
    else hipLaunchKernelGGL((k_block_pencil<3, false>), grid, block, 0, s, n, g, m, partials);
  }
  hipLaunchKernelGGL(k_pencil_final, dim3(pencil_tiles(tiles, ms != nullptr)), dim3(kTileWords), 0, s, blocks, partials, out);
  return true;
}

// out_j = sum_t c[t * nout + j] in_t; `table`: block_wide_table_words() words of device memory.  false (nothing launched): n is
// odd or a vector is not 16-byte aligned — no level of a plan has such vectors
bool launch_block_combine_wide(hipStream_t s, long n, const double* const* in, int nin, double* const* out, int nout, const double* c,
                               unsigned long long* table) {
  const int words = (int)block_wide_table_words();
  unsigned long long host[kWideCoefWords + kBlockWideMax + kBlockWideOut];
  uintptr_t bits = (uintptr_t)(n & 1);
  for (int t = 0; t < kBlockWideMax; ++t) {
    for (int j = 0; j < kBlockWideOut; ++j) {
      const double v = (t < nin && j < nout) ? c[t * nout + j] : 0.0;
      memcpy(&host[t * kBlockWideOut + j], &v, sizeof(double));
    }
    host[kWideCoefWords + t] = reinterpret_cast<uintptr_t>(in[t < nin ? t : 0]);
    if (t < nin) bits |= reinterpret_cast<uintptr_t>(in[t]) & 15;
  }
  for (int j = 0; j < kBlockWideOut; ++j) {
    host[kWideCoefWords + kBlockWideMax + j] = reinterpret_cast<uintptr_t>(out[j < nout ? j : 0]);
    if (j < nout) bits |= reinterpret_cast<uintptr_t>(out[j]) & 15;
  }
  if (bits != 0) return false;
  for (int off = 0; off < words; off += kStageWords) {
    StageArgs a{};
    const int count = words - off < kStageWords ? words - off : kStageWords;
    memcpy(a.w, host + off, sizeof(unsigned long long) * count);
    hipLaunchKernelGGL(k_wide_stage, dim3(1), dim3(kWideThreads), 0, s, table, off, count, a);
  }
  const long n2 = n / 2;
  long blocks = (n2 + kWideThreads - 1) / kWideThreads;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_block_combine_wide, dim3((unsigned)blocks), dim3(kWideThreads), 0, s, n2, table, nin, nout);
  return true;
}

// w_j <- w_j - sum_i <q_i, w_j> q_i for nq <= 64 vectors q and k <= 16 distinct vectors w, none of them a q.  `partials` holds
// ceil(nq / 16) * block_pencil_blocks(n) * 256 doubles; `out` (ceil(nq / 16) * 256 doubles) is left holding the coefficients
// <q_i, w_j> at out[i * 16 + j].  false (nothing launched): n is odd or a vector is not 16-byte aligned
bool launch_block_deflate(hipStream_t s, long n, int nq, const double* const* q, int k, double* const* w, double* partials, double* out) {
  DeflateArgs g{};
  uintptr_t bits = (uintptr_t)(n & 1);
  for (int t = 0; t < kBlockLockedMax; ++t) {
    g.q[t] = q[t < nq ? t : 0];
    if (t < nq) bits |= reinterpret_cast<uintptr_t>(q[t]) & 15;
  }
  for (int j = 0; j < kBlockWideOut; ++j) {
    g.w[j] = w[j < k ? j : 0];
    if (j < k) bits |= reinterpret_cast<uintptr_t>(w[j]) & 15;
  }
  if (bits != 0) return false;
  const int nb = block_pencil_blocks(n), tiles = (nq + kTile - 1) / kTile;
  const dim3 grid(nb), block(kWideThreads);
  if (tiles == 1) hipLaunchKernelGGL((k_block_cross<1>), grid, block, 0, s, n, g, nq, k, partials);
  else if (tiles == 2) hipLaunchKernelGGL((k_block_cross<2>), grid, block, 0, s, n, g, nq, k, partials);
  else if (tiles == 3) hipLaunchKernelGGL((k_block_cross<3>), grid, block, 0, s, n, g, nq, k, partials);
  else hipLaunchKernelGGL((k_block_cross<4>), grid, block, 0, s, n, g, nq, k, partials);
  hipLaunchKernelGGL(k_pencil_final, dim3(tiles), dim3(kTileWords), 0, s, nb, partials, out);
  const long n2 = n / 2;
  long blocks = (n2 + kWideThreads - 1) / kWideThreads;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_block_deflate, dim3((unsigned)blocks), dim3(kWideThreads), 0, s, n2, g, nq, k, out);
  return true;
}

// dst = sum_t w[t] x_t^2 for nq <= 64 vectors x, none of them dst; w: host numbers, copied into the launch.  max_blocks > 0:
// the grid's upper limit in place of 4096 (tests: a small grid takes several trips at a small size; the result does not depend
// on it).  false (nothing launched): n is odd or a vector is not 16-byte aligned
bool launch_block_density(hipStream_t s, long n, int nq, const double* const* x, const double* w, double* dst, int max_blocks) {
  DensityArgs g{};
  uintptr_t bits = (uintptr_t)(n & 1) | (reinterpret_cast<uintptr_t>(dst) & 15);
  for (int t = 0; t < kBlockLockedMax; ++t) {
    g.x[t] = x[t < nq ? t : 0];
    g.w[t] = t < nq ? w[t] : 0.0;
    if (t < nq) bits |= reinterpret_cast<uintptr_t>(x[t]) & 15;
  }
  g.dst = dst;
  if (bits != 0) return false;
  const long n2 = n / 2, cap = max_blocks > 0 ? max_blocks : 4096;
  long blocks = (n2 + kWideThreads - 1) / kWideThreads;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_block_density, dim3((unsigned)blocks), dim3(kWideThreads), 0, s, n2, g, nq);
  return true;
}

// launch_block_deflate with companions: aw_j <- aw_j - sum_i <b_i, w_j> ab_i with the coefficients of the w (ab == aw ==
// nullptr: the w only).  Pass 2 is k_block_deflate once per pair on the same coefficient table.
bool launch_block_project(hipStream_t s, long n, int nb, const double* const* b, const double* const* ab, int k, double* const* w, double* const* aw,
                          double* partials, double* out) {
  DeflateArgs g{}, ga{};
  uintptr_t bits = (uintptr_t)(n & 1);
  for (int t = 0; t < kBlockLockedMax; ++t) {
    g.q[t] = b[t < nb ? t : 0];
    if (ab) ga.q[t] = ab[t < nb ? t : 0];
    if (t < nb) bits |= (reinterpret_cast<uintptr_t>(b[t]) | (ab ? reinterpret_cast<uintptr_t>(ab[t]) : 0)) & 15;
  }
  for (int j = 0; j < kBlockWideOut; ++j) {
    g.w[j] = w[j < k ? j : 0];
    if (aw) ga.w[j] = aw[j < k ? j : 0];
    if (j < k) bits |= (reinterpret_cast<uintptr_t>(w[j]) | (aw ? reinterpret_cast<uintptr_t>(aw[j]) : 0)) & 15;
  }
  if (bits != 0) return false;
  const int blocks1 = block_pencil_blocks(n), tiles = (nb + kTile - 1) / kTile;
  const dim3 grid(blocks1), block(kWideThreads);
  if (tiles == 1) hipLaunchKernelGGL((k_block_cross<1>), grid, block, 0, s, n, g, nb, k, partials);
  else if (tiles == 2) hipLaunchKernelGGL((k_block_cross<2>), grid, block, 0, s, n, g, nb, k, partials);
  else if (tiles == 3) hipLaunchKernelGGL((k_block_cross<3>), grid, block, 0, s, n, g, nb, k, partials);
  else hipLaunchKernelGGL((k_block_cross<4>), grid, block, 0, s, n, g, nb, k, partials);
  hipLaunchKernelGGL(k_pencil_final, dim3(tiles), dim3(kTileWords), 0, s, blocks1, partials, out);
  const long n2 = n / 2;
  long blocks = (n2 + kWideThreads - 1) / kWideThreads;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_block_deflate, dim3((unsigned)blocks), dim3(kWideThreads), 0, s, n2, g, nb, k, out);
  if (ab) hipLaunchKernelGGL(k_block_deflate, dim3((unsigned)blocks), dim3(kWideThreads), 0, s, n2, ga, nb, k, out);
  return true;
}

// One Cholesky-QR step w <- w T, aw <- aw T (aw == nullptr: the w only) on k <= 16 distinct vectors: `partials` holds
// block_pencil_blocks(n) * 256 doubles, `table` (256 doubles) is left holding T row-major in rows of 16, `mask` the dropped
// columns.  false (nothing launched): n is odd or a vector is not 16-byte aligned
bool launch_block_orthonormalize(hipStream_t s, long n, int k, double* const* w, double* const* aw, double drop_tol, double* partials, double* table,
                                 unsigned* mask) {
  OrthArgs g{}, ga{};
  uintptr_t bits = (uintptr_t)(n & 1);
  for (int j = 0; j < kBlockWideOut; ++j) {
    g.w[j] = w[j < k ? j : 0];
    if (aw) ga.w[j] = aw[j < k ? j : 0];
    if (j < k) bits |= (reinterpret_cast<uintptr_t>(w[j]) | (aw ? reinterpret_cast<uintptr_t>(aw[j]) : 0)) & 15;
  }
  if (bits != 0) return false;
  const int nb = block_pencil_blocks(n);
  hipLaunchKernelGGL(k_block_gram16, dim3(nb), dim3(kWideThreads), 0, s, n, g, k, partials);
  hipLaunchKernelGGL(k_orth_factor, dim3(1), dim3(kTileWords), 0, s, nb, k, drop_tol, partials, table, mask);
  const long n2 = n / 2;
  long blocks = (n2 + kWideThreads - 1) / kWideThreads;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_block_transform, dim3((unsigned)blocks), dim3(kWideThreads), 0, s, n2, g, k, table, mask);
  if (aw) hipLaunchKernelGGL(k_block_transform, dim3((unsigned)blocks), dim3(kWideThreads), 0, s, n2, ga, k, table, mask);
  return true;
}

}  // namespace mgcmt
