// What the 3-D kernel files share (kernels_3d.hip, kernels_3d_point.hip): the launch geometry and the trilinear interpolation.
#pragma once
#include "mgcmt_internal.h"

namespace mgcmt {
namespace k3 {

constexpr int kFlatThreads = 256;
constexpr int kTileX = 64, kTileY = 4, kChunkZ = 32;  // marching kernels: x-y tile per workgroup, z-planes per chunk

// (P e)(z, y, x) of the trilinear interpolation P = S (x) S (x) S: fine 2J+1 takes coarse J with weight 1, fine 2J takes
// coarse J-1 and J with weight 1/2 each (where they exist)
__device__ __forceinline__ double prolong_at(const double* __restrict__ e, long nc, long z, long y, long x) {
  long jz[2], jy[2], jx[2];
  double wz[2], wy[2], wx[2];
  int nz = 0, ny = 0, nx = 0;
  auto split = [nc](long i, long* j, double* w, int& cnt) {
    if (i & 1) {
      j[0] = i >> 1;
      w[0] = 1.0;
      cnt = 1;
      return;
    }
    cnt = 0;
    const long h = i >> 1;
    if (h - 1 >= 0) {
      j[cnt] = h - 1;
      w[cnt++] = 0.5;
    }
    if (h < nc) {
      j[cnt] = h;
      w[cnt++] = 0.5;
    }
  };
  split(z, jz, wz, nz);
  split(y, jy, wy, ny);
  split(x, jx, wx, nx);
  double acc = 0.0;
  for (int a = 0; a < nz; ++a) {
    double pa = 0.0;
    for (int b = 0; b < ny; ++b) {
      const double* row = e + (jz[a] * nc + jy[b]) * nc;
      double pb = 0.0;
      for (int c = 0; c < nx; ++c) pb += wx[c] * row[jx[c]];
      pa += wy[b] * pb;
    }
    acc += wz[a] * pa;
  }
  return acc;
}

inline dim3 flat_grid(long points, int k) { return dim3((unsigned)((points + kFlatThreads - 1) / kFlatThreads), (unsigned)k, 1); }

}  // namespace k3
}  // namespace mgcmt
