// Anderson (Pulay) mixing of the potential in drivers.schroedinger_poisson (DESIGN.md par. 4.24): the two per-point operations
// of a step, shaped as k_block_density / k_block_deflate (kernels_blockwide.hip).  A thread owns two points (16-byte loads and
// stores) in a grid-stride loop over a bounded grid of 256-thread workgroups; the pointer lists and the coefficients travel as
// kernel arguments and are wave-uniform; plain stores, no atomics, nothing handed from one workgroup to another inside a launch;
// every multiply-add is an explicit fma in a fixed order.
#include "mgcmt_internal.h"

namespace mgcmt {

namespace {

constexpr int kMixThreads = 256, kMixWaves = kMixThreads / 64;
constexpr int kMixSums = kMixMax + 1;       // <r, r>, <out, out> and up to kMixMax - 1 products <r, r_j>
constexpr int kMixMaxSlices = 2048;         // slices of the residual pass (its partial sums), whatever the launched grid
constexpr int kMixCombineBlocks = 2048;     // the default grid limit of the combine pass

struct MixResidualArgs {
  const double* out;
  const double* in;
  double* r;
  const double* prev[kMixMax - 1];
};

struct MixCombineArgs {
  const double* x[kMixMax];
  const double* r[kMixMax];
  double alpha[kMixMax];
  double beta;
  double* dst;
};

__device__ __forceinline__ double mix_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
  return v;  // valid on lane 0
}

// r = out - in and the partial sums of <r, r>, <out, out> and <r, prev_j>, j < nprev, in ONE pass: out, in and the nprev earlier
// residuals are read once, r is written once.  The n2 double2 elements are dealt to `slices` slices — slice v holds the
// elements v * 256 + thread + m * slices * 256, m = 0, 1, ... — and partials[q * slices + v] is the sum of result q over slice
// v: a thread's own chain in ascending m (x then y of an element, each one fma), the 64-lane shuffle tree, the four waves in
// turn.  The slices are a function of n2 alone (mix_slices); the launched grid only decides which workgroup takes which
// slices (v = blockIdx.x, blockIdx.x + gridDim.x, ...), so every partial sum and with it every result is the same bits
// whatever the grid.  Result order: 0 = <r, r>, 1 = <out, out>, 2 + j = <r, prev_j>.  prev_j, j >= nprev, is never read.
__global__ void __launch_bounds__(kMixThreads) k_mix_residual(long n2, MixResidualArgs g, int nprev, int slices, double* __restrict__ partials) {
  __shared__ double s_part[kMixWaves][kMixSums];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int v = blockIdx.x; v < slices; v += gridDim.x) {
    double acc[kMixSums];
#pragma unroll
    for (int t = 0; t < kMixSums; ++t) acc[t] = 0.0;
    for (long i = (long)v * kMixThreads + threadIdx.x; i < n2; i += (long)slices * kMixThreads) {
      const double2 o = reinterpret_cast<const double2*>(g.out)[i];
      const double2 x = reinterpret_cast<const double2*>(g.in)[i];
      double2 pv[kMixMax - 1];
#pragma unroll
      for (int j = 0; j < kMixMax - 1; ++j)
        pv[j] = j < nprev ? reinterpret_cast<const double2*>(g.prev[j])[i] : make_double2(0.0, 0.0);
      const double2 r = make_double2(o.x - x.x, o.y - x.y);
      reinterpret_cast<double2*>(g.r)[i] = r;
      acc[0] = fma(r.y, r.y, fma(r.x, r.x, acc[0]));
      acc[1] = fma(o.y, o.y, fma(o.x, o.x, acc[1]));
#pragma unroll
      for (int j = 0; j < kMixMax - 1; ++j)
        if (j < nprev) acc[2 + j] = fma(r.y, pv[j].y, fma(r.x, pv[j].x, acc[2 + j]));
    }
#pragma unroll
    for (int t = 0; t < kMixSums; ++t) {
      const double tot = mix_wave_sum(acc[t]);
      if (lane == 0) s_part[wave][t] = tot;
    }
    __syncthreads();
    if ((int)threadIdx.x < nprev + 2) {
      double tot = 0.0;
      for (int w = 0; w < kMixWaves; ++w) tot += s_part[w][threadIdx.x];
      partials[(long)threadIdx.x * slices + v] = tot;
    }
    __syncthreads();  // (s_part is written again in the workgroup's next slice)
  }
}

// out[q] = sum of partials[q * slices .. (q + 1) * slices), q < nq, by ONE workgroup: thread t adds the partials t, t + 256, ...
// in ascending order, then the shuffle tree and the four waves in turn (k_dot_final's order, kernels_blas.hip)
__global__ void __launch_bounds__(kMixThreads) k_mix_final(int nq, int slices, const double* __restrict__ partials, double* __restrict__ out) {
  __shared__ double s_part[kMixWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int q = 0; q < nq; ++q) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < slices; i += kMixThreads) acc += partials[(long)q * slices + i];
    const double tot = mix_wave_sum(acc);
    if (lane == 0) s_part[wave] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int w = 0; w < kMixWaves; ++w) t += s_part[w];
      out[q] = t;
    }
    __syncthreads();
  }
}

// dst = sum_(i < p) alpha_i (x_i + beta r_i) in one pass over the 2p vectors.  The arithmetic of a point is fixed:
//     acc = 0;  for i = 0 .. p - 1 ascending:  acc = fma(alpha_i, fma(beta, r_i, x_i), acc)
// Every element is read before the thread that owns it stores it and no other thread touches it, so dst may be one of the
// inputs as far as the kernel goes (the entry allows x_0, the pair that is about to be dropped).  Vectors i >= p are never read.
__global__ void __launch_bounds__(kMixThreads) k_mix_combine(long n2, MixCombineArgs g, int p) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long)gridDim.x * blockDim.x) {
    double2 acc = make_double2(0.0, 0.0);
#pragma unroll 3
    for (int t = 0; t < p; ++t) {
      const double2 x = reinterpret_cast<const double2*>(g.x[t])[i];
      const double2 r = reinterpret_cast<const double2*>(g.r[t])[i];
      const double a = g.alpha[t];
      acc.x = fma(a, fma(g.beta, r.x, x.x), acc.x);
      acc.y = fma(a, fma(g.beta, r.y, x.y), acc.y);
    }
    reinterpret_cast<double2*>(g.dst)[i] = acc;
  }
}

}  // namespace

// the slices of the residual pass over n points: one per 256 double2 elements, at most 2048
int mix_slices(long n) {
  long s = (n / 2 + kMixThreads - 1) / kMixThreads;
  if (s > kMixMaxSlices) s = kMixMaxSlices;
  if (s < 1) s = 1;
  return (int)s;
}

// r = out - in; results[0] = <r, r>, results[1] = <out, out>, results[2 + j] = <r, prev_j>, j < nprev <= kMixMax - 1 (device
// memory; partials: kMixSums * mix_slices(n) doubles).  max_blocks > 0: the grid's upper limit in place of one workgroup per
// slice (tests: several slices per workgroup at a small size; the results do not depend on it).  false (nothing launched): n
// is odd or a vector is not 16-byte aligned
bool launch_mix_residual(hipStream_t s, long n, const double* out, const double* in, double* r, int nprev, const double* const* prev, double* partials,
                         double* results, int max_blocks) {
  MixResidualArgs g{};
  g.out = out;
  g.in = in;
  g.r = r;
  uintptr_t bits = (uintptr_t)(n & 1) | ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(r)) & 15);
  for (int j = 0; j < kMixMax - 1; ++j) {
    g.prev[j] = j < nprev ? prev[j] : out;
    if (j < nprev) bits |= reinterpret_cast<uintptr_t>(prev[j]) & 15;
  }
  if (bits != 0) return false;
  const int slices = mix_slices(n);
  int blocks = slices;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
  hipLaunchKernelGGL(k_mix_residual, dim3((unsigned)blocks), dim3(kMixThreads), 0, s, n / 2, g, nprev, slices, partials);
  hipLaunchKernelGGL(k_mix_final, dim3(1), dim3(kMixThreads), 0, s, nprev + 2, slices, partials, results);
  return true;
}

// dst = sum_(i < p) alpha[i] (x_i + beta r_i), p <= kMixMax; alpha, beta: host numbers, copied into the launch.  max_blocks as
// above (default limit: 2048 workgroups).  false (nothing launched): n is odd or a vector is not 16-byte aligned
bool launch_mix_combine(hipStream_t s, long n, int p, const double* const* x, const double* const* r, const double* alpha, double beta, double* dst,
                        int max_blocks) {
  MixCombineArgs g{};
  uintptr_t bits = (uintptr_t)(n & 1) | (reinterpret_cast<uintptr_t>(dst) & 15);
  for (int t = 0; t < kMixMax; ++t) {
    g.x[t] = x[t < p ? t : 0];
    g.r[t] = r[t < p ? t : 0];
    g.alpha[t] = t < p ? alpha[t] : 0.0;
    if (t < p) bits |= (reinterpret_cast<uintptr_t>(x[t]) | reinterpret_cast<uintptr_t>(r[t])) & 15;
  }
  g.beta = beta;
  g.dst = dst;
  if (bits != 0) return false;
  const long n2 = n / 2, cap = max_blocks > 0 ? max_blocks : kMixCombineBlocks;
  long blocks = (n2 + kMixThreads - 1) / kMixThreads;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_mix_combine, dim3((unsigned)blocks), dim3(kMixThreads), 0, s, n2, g, p);
  return true;
}

}  // namespace mgcmt
