// The level hierarchy of a plan: the host Galerkin factors of every level, their upload (with the classification of
// the operator the kernels branch on), plan creation for 1, 2 and 3 axes, destruction and the entries that describe levels.
// A per-point part (a diagonal, bonds or a stencil; 2-D or 3-D) has ONE description here: PointPart (what a creator hands
// over), point_planes (how many planes a level holds), build_point_part (every level's planes), create_point (the checks all
// six creators share, with check_bonds / check_stencil) and point_of (what the entries that describe levels read).
// Host code only.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "plan_internal.h"

using namespace mgcmt;

namespace {

bool is_pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

// Galerkin product of one factor: R1 * T * P1 with R1 = full weighting (1/4,1/2,1/4 on fine
// 2I..2I+2) and P1 = 2 R1^T (MGCMTStencilMaker.py:27-78, MGCMTSolver.py:318).  Stays tridiagonal.
Tri galerkin(const Tri& f) {
  static const double rw[3] = {0.25, 0.5, 0.25};
  static const double pw[3] = {0.5, 1.0, 0.5};
  Tri c;
  c.n = f.n / 2;
  c.a.assign(3 * c.n, 0.0);
  for (int64_t I = 0; I < c.n; ++I) {
    for (int dJ = -1; dJ <= 1; ++dJ) {
      const int64_t J = I + dJ;
      if (J < 0 || J >= c.n) continue;
      double acc = 0.0;
      for (int t = 0; t < 3; ++t) {
        const int64_t a = 2 * I + t;
        if (a >= f.n) continue;
        for (int s = -1; s <= 1; ++s) {
          const int64_t b = a + s;
          if (b < 0 || b >= f.n) continue;
          const int64_t o = b - 2 * J;
          if (o < 0 || o > 2) continue;
          acc += rw[t] * f.at(a, b) * pw[o];
        }
      }
      c.a[(dJ + 1) * c.n + I] = acc;
    }
  }
  return c;
}

Tri identity_tri(int64_t n) {
  Tri t;
  t.n = n;
  t.a.assign(3 * n, 0.0);
  for (int64_t i = 0; i < n; ++i) t.a[n + i] = 1.0;
  return t;
}

// n doubles on the device, freed with the operator (d->owned)
int upload_array(DevOp* d, const double* src, size_t n, const double** dst) {
  double* q = nullptr;
  MG_HIP(hipMalloc((void**)&q, n * sizeof(double)));
  d->owned.push_back(q);
  MG_HIP(hipMemcpy(q, src, n * sizeof(double), hipMemcpyHostToDevice));
  *dst = q;
  return MGCMT_OK;
}

int upload_op(const HostOp& h, const Level& L, int dim, DevOp* d) {
  KOp& k = d->k;
  k = KOp{};
  k.nterms = h.nterms;
  k.ldx = L.nr + 2 * L.halo;
  k.ldy = L.gc;
  for (int m = 0; m < h.nterms; ++m) {
    std::vector<double> xs(3 * k.ldx, 0.0);
    for (int part = 0; part < 3; ++part)
      for (int64_t i = -L.halo; i < L.nr + L.halo; ++i) {
        const int64_t gi = L.r0 + i;
        if (gi >= 0 && gi < L.gr) xs[part * k.ldx + (i + L.halo)] = h.X[m].a[part * L.gr + gi];
      }
    const double* dx = nullptr;
    MG_TRY(upload_array(d, xs.data(), xs.size(), &dx));
    MG_TRY(upload_array(d, h.Y[m].a.data(), 3 * L.gc, &k.Y[m]));
    k.X[m] = dx + L.halo;
  }
  if (dim == 1 && h.nterms > 0) {
    // 1-D: X_m is 1 x 1, so the operator is ONE tridiagonal, sum_m x_m Y_m — folded here for the fused 1-D passes
    const int64_t n = L.gc;
    std::vector<double> t(3 * n, 0.0);
    for (int m = 0; m < h.nterms; ++m) {
      const double x = h.X[m].di(0);
      for (int64_t i = 0; i < 3 * n; ++i) t[i] += x * h.Y[m].a[i];
    }
    MG_TRY(upload_array(d, t.data(), t.size(), &k.tri));
    k.one_d = 1;
    bool constant = n >= 3;
    for (int64_t i = 0; constant && i < n; ++i) {
      if (i > 0 && t[i] != t[1]) constant = false;                          // lower (entry 0 is outside the matrix)
      if (i + 1 < n && (t[n + i] != t[n] || t[2 * n + i] != t[2 * n])) constant = false;  // diagonal but the last, upper (the last entry is outside)
    }
    if (constant) {
      k.tri_const = 1;
      k.t_lo = t[1];
      k.t_di = t[n];
      k.t_up = t[2 * n];
      k.t_last = t[2 * n - 1];
    }
  }
  // constant-coefficient 5-point (2-D) / 3-point (1-D) detection: every factor Toeplitz and the
  // corner coefficients zero -> the kernels take three scalars instead of the factor arrays
  auto toeplitz = [](const Tri& t, double* lo, double* di, double* up) {
    *di = t.di(0);
    *lo = t.n > 1 ? t.lo(1) : 0.0;
    *up = t.n > 1 ? t.up(0) : 0.0;
    for (int64_t i = 0; i < t.n; ++i) {
      if (t.di(i) != *di) return false;
      if (i > 0 && t.lo(i) != *lo) return false;
      if (i + 1 < t.n && t.up(i) != *up) return false;
    }
    return true;
  };
  double c[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  bool all = h.nterms > 0;
  for (int m = 0; m < h.nterms && all; ++m) {
    double x[3], y[3];
    if (!toeplitz(h.X[m], &x[0], &x[1], &x[2]) || !toeplitz(h.Y[m], &y[0], &y[1], &y[2])) {
      all = false;
      break;
    }
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) c[a][b] += x[a] * y[b];
  }
  if (all && c[0][0] == 0 && c[0][2] == 0 && c[2][0] == 0 && c[2][2] == 0 && c[0][1] == c[2][1] && c[1][0] == c[1][2] &&
      (dim == 2 || c[0][1] == 0)) {
    k.five_point = 1;
    k.c0 = c[1][1];
    k.cn = c[0][1];
    k.cw = c[1][0];
  }
  // constant 5-point part plus ONE product potential on the diagonal: the Toeplitz terms form a 5-point operator,
  // the remaining term has diagonal factors only
  if (!k.five_point && dim == 2 && h.nterms >= 2) {
    auto diagonal_only = [](const Tri& t) {
      for (int64_t i = 0; i < t.n; ++i)
        if ((i > 0 && t.lo(i) != 0.0) || (i + 1 < t.n && t.up(i) != 0.0)) return false;
      return true;
    };
    double c5[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    int nd = 0, dm[2] = {0, 0};
    bool ok = true;
    for (int m = 0; m < h.nterms && ok; ++m) {
      double x[3], y[3];
      if (toeplitz(h.X[m], &x[0], &x[1], &x[2]) && toeplitz(h.Y[m], &y[0], &y[1], &y[2])) {
        for (int a = 0; a < 3; ++a)
          for (int b = 0; b < 3; ++b) c5[a][b] += x[a] * y[b];
      } else if (diagonal_only(h.X[m]) && diagonal_only(h.Y[m]) && nd < 1) {
        dm[nd++] = m;
      } else {
        ok = false;
      }
    }
    if (ok && nd == 1 && c5[0][0] == 0 && c5[0][2] == 0 && c5[2][0] == 0 && c5[2][2] == 0 && c5[0][1] == c5[2][1] && c5[1][0] == c5[1][2]) {
      k.five_diag = 1;
      k.ndiag = nd;
      k.c0 = c5[1][1];
      k.cn = c5[0][1];
      k.cw = c5[1][0];
      for (int t = 0; t < nd; ++t) {
        k.dX[t] = k.X[dm[t]] + k.ldx;  // the diagonal row of the factor arrays ([lower | diag | upper])
        k.dY[t] = k.Y[dm[t]] + k.ldy;
      }
    }
  }
  // Galerkin levels of a constant operator: Toeplitz factors whose last diagonal entry differs
  if (!k.five_point && !k.five_diag && dim == 2 && h.nterms > 0) {
    auto toeplitz_but_last = [](const Tri& t, double* lo, double* di, double* up, double* last) {
      if (t.n < 3) return false;
      *di = t.di(0);
      *lo = t.lo(1);
      *up = t.up(0);
      *last = t.di(t.n - 1);
      for (int64_t i = 0; i < t.n; ++i) {
        if (i + 1 < t.n && t.di(i) != *di) return false;
        if (i > 0 && t.lo(i) != *lo) return false;
        if (i + 1 < t.n && t.up(i) != *up) return false;
      }
      return true;
    };
    bool ok = true;
    double c9[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, crow[3] = {0, 0, 0}, ccol[3] = {0, 0, 0}, corner = 0;
    int nconst = 0, nvar = 0, var_term = -1;
    for (int m = 0; m < h.nterms && ok; ++m) {
      double x[3], y[3], xl, yl;
      if (!(toeplitz_but_last(h.X[m], &x[0], &x[1], &x[2], &xl) && toeplitz_but_last(h.Y[m], &y[0], &y[1], &y[2], &yl))) {
        // a term with variable factors: one of them may ride on top of the constant part (nine_var)
        ++nvar;
        var_term = m;
        ok = nvar <= 1;
        continue;
      }
      ++nconst;
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) c9[a][b] += x[a] * y[b];
      for (int b = 0; b < 3; ++b) crow[b] += xl * y[b];   // last row: X's diagonal entry is the modified one
      for (int a = 0; a < 3; ++a) ccol[a] += x[a] * yl;   // last column: Y's diagonal entry is the modified one
      corner += xl * yl;
      crow[1] += 0.0;
    }
    if (ok && nconst >= 1) {
      // on the last row the centre coefficient of the last column is the corner; crow[1] is the centre elsewhere
      if (nvar == 0) {
        k.nine_const = 1;
      } else {
        k.nine_var = 1;
        k.vX = k.X[var_term];
        k.vY = k.Y[var_term];
      }
      for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) k.c9[a][b] = c9[a][b];
        k.c9row[a] = crow[a];
        k.c9col[a] = ccol[a];
      }
      k.c9corner = corner;
    }
  }
  return MGCMT_OK;
}

// a 3-D level's factors on the device, and the constant 7-point form where every factor is Toeplitz and the summed
// stencil has no entry off the three axes
int upload_op3(const HostOp& h, int64_t n, DevOp* d) {
  K3Op& k = d->k3;
  k = K3Op{};
  k.nterms = h.nterms;
  k.n = (long)n;
  for (int m = 0; m < h.nterms; ++m) {
    MG_TRY(upload_array(d, h.X[m].a.data(), h.X[m].a.size(), &k.X[m]));
    MG_TRY(upload_array(d, h.Y[m].a.data(), h.Y[m].a.size(), &k.Y[m]));
    MG_TRY(upload_array(d, h.Z[m].a.data(), h.Z[m].a.size(), &k.Z[m]));
  }
  auto toeplitz = [](const Tri& t, double* f) {
    f[1] = t.di(0);
    f[0] = t.n > 1 ? t.lo(1) : 0.0;
    f[2] = t.n > 1 ? t.up(0) : 0.0;
    for (int64_t i = 0; i < t.n; ++i) {
      if (t.di(i) != f[1]) return false;
      if (i > 0 && t.lo(i) != f[0]) return false;
      if (i + 1 < t.n && t.up(i) != f[2]) return false;
    }
    return true;
  };
  double c[3][3][3] = {};
  bool all = h.nterms > 0 && n >= 2;
  for (int m = 0; m < h.nterms && all; ++m) {
    double fz[3], fy[3], fx[3];
    if (!toeplitz(h.X[m], fz) || !toeplitz(h.Y[m], fy) || !toeplitz(h.Z[m], fx)) {
      all = false;
      break;
    }
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b)
        for (int e = 0; e < 3; ++e) c[a][b][e] += fz[a] * fy[b] * fx[e];
  }
  for (int a = 0; a < 3 && all; ++a)
    for (int b = 0; b < 3; ++b)
      for (int e = 0; e < 3; ++e)
        if ((a != 1) + (b != 1) + (e != 1) >= 2 && c[a][b][e] != 0.0) all = false;
  if (all) {
    k.seven = 1;
    k.c0 = c[1][1][1];
    k.czm = c[0][1][1];
    k.czp = c[2][1][1];
    k.cym = c[1][0][1];
    k.cyp = c[1][2][1];
    k.cxm = c[1][1][0];
    k.cxp = c[1][1][2];
  }
  return MGCMT_OK;
}

// The per-point part of A as a creator hands it over (host arrays).  kPointDiag: planes = {D}; kPointBonds: {D, b_0, ..,
// b_dim-1}, the bond plane of axis a counted from the fastest index — 2-D: E (towards (i, j + 1)), S (towards (i + 1, j));
// 3-D: Bx, By, Bz —; kPointPlanes: {G}, the 3^dim planes of a 9- / 27-point stencil one behind the other.  g^dim numbers a plane.
struct PointPart {
  int kind = kPointNone;
  const double* planes[4] = {nullptr, nullptr, nullptr, nullptr};
};

// how many planes a level of a dim-axis plan with this kind of per-point part holds
int point_planes(int dim, int kind) { return kind == kPointDiag ? 1 : kind == kPointBonds ? dim + 1 : dim == 3 ? 27 : 9; }

// What a creator asks for.  fac / m_fac: the factor arrays of A / M per axis as HostOp holds them — {X, Y, Z}, i.e.
// 3-D: {z, y, x}; 2-D: {rows, columns}; 1-D: {none, the vector} (X is the 1 x 1 identity there) — nterms blocks of 3 g each
struct PlanSpec {
  int dim, nvec, device;
  int64_t g, lowest;
  int nterms, m_nterms;
  const double* fac[3];
  const double* m_fac[3];
  int64_t row_begin, row_end;  // a 2-D plan's rows of level 0, (0, 0) = all; ignored otherwise
  int strip_levels;
  PointPart point{};  // 2-D and 3-D (create_point)
};

PlanSpec spec_of(const mgcmt_plan_desc& d) {
  return PlanSpec{d.dim, d.nvec, d.device, d.g, d.lowest, d.nterms, d.m_nterms, {d.xfac, d.yfac, nullptr}, {d.m_xfac, d.m_yfac, nullptr},
                  d.row_begin, d.row_end, d.strip_levels};
}

PlanSpec spec_of(const mgcmt_plan3d_desc& d) {
  return PlanSpec{3, d.nvec, d.device, d.g, d.lowest, d.nterms, 0, {d.zfac, d.yfac, d.xfac}, {nullptr, nullptr, nullptr}, 0, 0, 0};
}

// the per-point part of level l as the kernels see it, whichever of KOp / K3Op holds it
struct PointView {
  int kind;
  const double* pg;
  long pplane;
};

PointView point_of(const mgcmt_plan* p, int l) {
  const DevOp& d = p->levels[l].dA;
  return p->dim == 3 ? PointView{d.k3.point, d.k3.pg, d.k3.pplane} : PointView{d.k.point, d.k.pg, d.k.pplane};
}

// The per-point part of A on every level (2-D: kernels_pointwise.hip, 3-D: kernels_3d_point.hip).  Level 0 holds the
// caller's planes (PointPart), pplane apart, and KOp::point / K3Op::point = their kind; every level below holds the 3^dim
// planes of the Galerkin product R (.) P of the level above (kPointPlanes), formed on the device, one launch per level — the
// same launch whatever the kind above, so a stencil's level 1 is formed from level 0 as level 2 is from level 1.  The Kronecker
// part's operators (upload_op / upload_op3) are in place; this adds the pointers to them.
// Layout of level 0: a 2-D diagonal or D, E, S sit in the level's padded row layout each (zero halo rows, pg at the interior:
// the marching kernels read S(-1, j) as an exact zero); 2-D stencil planes and everything in 3-D (the kernels predicate all
// directions) are g^dim numbers a plane, at the index of the right-hand side.
int build_point_part(mgcmt_plan* p, const PointPart& pt) {
  const bool three = p->dim == 3;
  // Which levels of planes take the tile kernels (pmarch; 2-D: kernels_nine_tile.hip, nine_tiled adds the size rule, MGCMT_NINE_TILE;
  // 3-D: kernels_3d_stencil.hip, stencil3_tiled adds it, MGCMT_3D_STENCIL_TILE).  Unset or "1": level 0 of a plan with a stencil,
  // the passes in tile_all (2-D: each measured faster than its flat form at 4096^2; 3-D: those that measured no slower than
  // 1.03 x their flat form at 256^3: DESIGN par. 4.18); "0": none (A/B tests); "2": the Galerkin levels of every plan with a
  // per-point part as well (measurements; not the default: existing plans run the launches they always ran).
  const char* t = getenv(three ? "MGCMT_3D_STENCIL_TILE" : "MGCMT_NINE_TILE");
  const int tile_mode = !t || !t[0] ? 1 : t[0] == '0' ? 0 : t[0] == '2' ? 2 : 1;
  const int tile_all = three ? kStencil3Colour | kStencil3Residual : kNineColour | kNineJacobi | kNineResidual;
  // Which passes of a fine level with a diagonal or bonds march (pmarch).  3-D (point3_marching adds the size rule): all of them,
  // MGCMT_3D_POINT_MARCH = "0": none (A/B tests).  2-D, bonds only (kernels_bonds.hip; MGCMT_BONDS_MARCH): unset, those that
  // measured faster than their flat form at 8192^2 — the parity stages and residual + restriction (bit 0); the weighted-Jacobi
  // sweep and the applied operator measured level with it and stay flat; "1": every pass (bit 1 as well); "0": none.
  const char* e = getenv(three ? "MGCMT_3D_POINT_MARCH" : "MGCMT_BONDS_MARCH");
  int march = three ? kMarch3Jacobi | kMarch3Parity | kMarch3Residual | kMarch3Prolong : pt.kind != kPointBonds ? 0 : !e || !e[0] ? 1 : 3;
  if (e && e[0] == '0') march = 0;
  auto set = [&](Level& L, int kind, int pmarch, const double* pg, size_t pplane) {
    auto fill = [&](auto& k) {  // (KOp and K3Op name these alike)
      k.point = kind;
      k.pmarch = pmarch;
      k.pg = pg;
      k.pplane = (long)pplane;
    };
    if (three) {
      fill(L.dA.k3);
    } else {
      fill(L.dA.k);
      L.dA.k.pld = L.gc;
    }
  };
  for (size_t l = 0; l < p->levels.size(); ++l) {
    Level& L = p->levels[l];
    const size_t N = (size_t)L.nr * L.gc;
    double* q = nullptr;
    if (l == 0) {
      const int np = point_planes(p->dim, pt.kind);
      const bool padded = !three && pt.kind != kPointPlanes;
      const size_t first = padded ? (size_t)L.halo * L.gc : 0, plane = N + 2 * first;
      MG_HIP(hipMalloc((void**)&q, np * plane * sizeof(double)));
      L.dA.owned.push_back(q);
      if (padded) MG_HIP(hipMemset(q, 0, np * plane * sizeof(double)));
      if (pt.kind == kPointPlanes) MG_HIP(hipMemcpy(q, pt.planes[0], np * N * sizeof(double), hipMemcpyHostToDevice));
      else
        for (int a = 0; a < np; ++a) MG_HIP(hipMemcpy(q + a * plane + first, pt.planes[a], N * sizeof(double), hipMemcpyHostToDevice));
      set(L, pt.kind, pt.kind == kPointPlanes ? (tile_mode >= 1 ? tile_all : 0) : march, q + first, pt.kind == kPointDiag ? 0 : plane);
      continue;
    }
    const Level& F = p->levels[l - 1];
    const PointView f = point_of(p, (int)l - 1);
    MG_HIP(hipMalloc((void**)&q, point_planes(p->dim, kPointPlanes) * N * sizeof(double)));
    L.dA.owned.push_back(q);
    if (three) launch3p_coarsen(nullptr, F.dA.k3.n, f.pg, point_planes(3, f.kind), f.pplane, q, (long)N);
    else launch_point_coarsen(nullptr, F.nr, F.gc, f.pg, point_planes(2, f.kind), F.gc, f.pplane, q, L.gc, L.nr * L.gc);
    MG_TRY(post_launch());
    set(L, kPointPlanes, tile_mode == 2 ? tile_all : 0, q, N);
  }
  MG_HIP(hipDeviceSynchronize());
  p->has_point = true;
  return MGCMT_OK;
}

// the seven pieces of device scratch every plan starts with
hipError_t alloc_scratch(mgcmt_plan* p) {
  hipError_t e = hipMalloc((void**)&p->d_shifts, sizeof(double) * kMaxVec);
  if (e == hipSuccess) e = hipMalloc((void**)&p->d_zero, sizeof(double) * kMaxVec);
  if (e == hipSuccess) e = hipMalloc((void**)&p->d_partials, sizeof(double) * (kMaxVec + 1) * 1024 * 2);
  if (e == hipSuccess) e = hipMalloc((void**)&p->d_mgs, sizeof(double) * mgs_block_words());
  if (e == hipSuccess) e = hipMalloc((void**)&p->d_scalars, sizeof(double) * 4 * kMaxVec);
  if (e == hipSuccess) e = hipMemset(p->d_shifts, 0, sizeof(double) * kMaxVec);
  if (e == hipSuccess) e = hipMemset(p->d_zero, 0, sizeof(double) * kMaxVec);
  return e;
}

// A plan of 1, 2 or 3 axes: level l has g >> l points per axis.  1-D: one "row" of g >> l; 2-D: (g >> l)^2 as rows
// (a strip of them on the first strip_levels levels); 3-D: g >> l z-planes of (g >> l)^2 points, one zero halo plane
// above and below.  The creators have checked what is theirs alone (dim, the mass terms, the direct solve's limit in 3-D).
int build_plan(const PlanSpec& d, mgcmt_plan** out) {
  if (!is_pow2(d.g) || !is_pow2(d.lowest) || d.lowest > d.g) return fail(MGCMT_ERR_INVALID, "g and lowest must be powers of two with lowest <= g");
  if (d.g < 2) return fail(MGCMT_ERR_INVALID, "Length of start vector is not a power of 2");
  if (d.lowest < 2) return fail(MGCMT_ERR_INVALID, "lowest must be at least 2");
  if (d.nterms < 1 || d.nterms > kMaxTerms) return fail(MGCMT_ERR_INVALID, "nterms out of range");
  const int first_axis = d.dim == 1 ? 1 : 0, naxes = d.dim == 3 ? 3 : 2;
  for (int a = first_axis; a < naxes; ++a)
    if (!d.fac[a]) return fail(MGCMT_ERR_INVALID, "missing factor arrays");
  if (d.nvec < 1 || d.nvec > kMaxStoreVec) return fail(MGCMT_ERR_INVALID, "nvec out of range (1..80)");
  const int64_t rows = d.dim == 1 ? 1 : d.g;
  int64_t rb = d.row_begin, re = d.row_end;
  if (d.dim != 2 || (rb == 0 && re == 0)) {
    rb = 0;
    re = rows;
  }
  if (rb < 0 || re > rows || rb >= re) return fail(MGCMT_ERR_INVALID, "bad row range");
  MG_HIP(hipSetDevice(d.device));

  mgcmt_plan* p = new mgcmt_plan();
  p->dim = d.dim;
  p->nvec = d.nvec;
  p->device = d.device;
  p->g = d.g;
  p->lowest = d.lowest;
  p->has_mass = d.m_nterms > 0;
  p->h_shifts.assign(kMaxVec, 0.0);
  const char* mb = getenv("MGCMT_MGS_BLOCK_MIN");  // points per column from which Gram-Schmidt takes its two-pass form (tests, tuning)
  if (mb && atol(mb) > 1) p->mgs_block_min = atol(mb);
  const char* db = getenv("MGCMT_DENSITY_BLOCKS");  // the grid limit of mgcmt_block_density (tests: several trips at a small size)
  if (db && atol(db) >= 1 && atol(db) <= 4096) p->density_max_blocks = (int)atol(db);
  const char* xb = getenv("MGCMT_MIX_BLOCKS");  // the grid limit of mgcmt_mix_residual / mgcmt_mix_combine (tests, as above)
  if (xb && atol(xb) >= 1 && atol(xb) <= 2048) p->mix_max_blocks = (int)atol(xb);
  if (d.dim != 3) {
    const char* e = getenv("MGCMT_TAIL_DENSE");  // "0": the tail as the LDS-resident launch by default (the host-only test build:
    p->use_tail_dense = !(e && e[0] == '0');     // emulating the 1024 workgroups that form the matrix takes minutes)
  }

  int nlev = 1;
  for (int64_t s = d.g; s > d.lowest; s >>= 1) ++nlev;
  const bool whole = rb == 0 && re == rows;
  int strip_levels = whole ? 0 : (d.strip_levels > 0 ? d.strip_levels : nlev);
  if (strip_levels > nlev) strip_levels = nlev;
  if (!whole) {
    const int64_t align = (int64_t)1 << (strip_levels - 1);
    if (rb % align || re % align) {
      delete p;
      return fail(MGCMT_ERR_INVALID, "strip bounds must be multiples of 2^(strip_levels-1)");
    }
  }

  p->levels.resize(nlev);
  for (int l = 0; l < nlev; ++l) {
    Level& L = p->levels[l];
    const int64_t n = d.g >> l;
    L.gr = d.dim == 1 ? 1 : n;
    L.gc = d.dim == 3 ? n * n : n;
    L.r0 = l < strip_levels ? rb >> l : 0;
    L.nr = l < strip_levels ? (re - rb) >> l : L.gr;
    L.halo = d.dim == 2 ? kHalo : 1;
    L.stride = ((L.nr + 2 * L.halo) * L.gc + 31) / 32 * 32;
    // level 0 holds the caller's factors; below it R A P (and R M P) with P = P1 (x) ... (x) P1: each factor coarsened
    // on its own (galerkin), a Kronecker sum stays one
    auto build = [&](HostOp& h, const HostOp* finer, int nterms, const double* const* src) {
      h.nterms = nterms;
      std::vector<Tri>* mine[3] = {&h.X, &h.Y, &h.Z};
      for (int a = 0; a < naxes; ++a) {
        const std::vector<Tri>* above = !finer ? nullptr : a == 0 ? &finer->X : a == 1 ? &finer->Y : &finer->Z;
        mine[a]->resize(nterms);
        for (int m = 0; m < nterms; ++m) {
          Tri& t = (*mine[a])[m];
          if (a < first_axis) {
            t = identity_tri(1);
          } else if (l == 0) {
            t.n = d.g;
            t.a.assign(src[a] + (size_t)m * 3 * d.g, src[a] + (size_t)(m + 1) * 3 * d.g);
          } else {
            t = galerkin((*above)[m]);
          }
        }
      }
    };
    build(L.hA, l ? &p->levels[l - 1].hA : nullptr, d.nterms, d.fac);
    if (p->has_mass) build(L.hM, l ? &p->levels[l - 1].hM : nullptr, d.m_nterms, d.m_fac);
    int rc = d.dim == 3 ? upload_op3(L.hA, n, &L.dA) : upload_op(L.hA, L, d.dim, &L.dA);
    if (rc == MGCMT_OK && p->has_mass) rc = d.dim == 3 ? upload_op3(L.hM, n, &L.dM) : upload_op(L.hM, L, d.dim, &L.dM);
    if (rc != MGCMT_OK) {
      mgcmt_plan_destroy(p);
      return rc;
    }
  }
  if (d.point.kind != kPointNone) {
    const int rc = build_point_part(p, d.point);
    if (rc != MGCMT_OK) {
      mgcmt_plan_destroy(p);
      return rc;
    }
  }
  const hipError_t e = alloc_scratch(p);
  if (e != hipSuccess) {
    mgcmt_plan_destroy(p);
    return fail(MGCMT_ERR_HIP, std::string("plan scratch allocation: ") + hipGetErrorString(e));
  }
  *out = p;
  return MGCMT_OK;
}

// a stencil's 3^dim planes of g^dim numbers (plane index: the offsets + 1 as base-3 digits, slowest axis first): coefficients
// towards points outside the grid are zero and the stencil is symmetric
int check_stencil(int dim, int64_t g, const double* G) {
  if (g < 1) return MGCMT_OK;  // (build_plan refuses it)
  const int np = point_planes(dim, kPointPlanes);
  int64_t N = 1;
  for (int a = 0; a < dim; ++a) N *= g;
  for (int t = 0; t < np; ++t) {
    int o[3] = {0, 0, 0};  // the plane's offset per axis, slowest first; off: the same as a distance in the plane
    int64_t off = 0, w = 1;
    for (int a = dim - 1, r = t; a >= 0; --a, r /= 3, w *= g) off += (o[a] = r % 3 - 1) * w;
    const double* P = G + t * N;
    const double* T = G + (np - 1 - t) * N;  // the plane of the opposite offset
    int64_t c[3] = {0, 0, 0};  // the slow coordinates of the line of g points at `row`
    for (int64_t row = 0; row < N; row += g) {
      bool in = true;
      for (int a = 0; a < dim - 1; ++a) in = in && c[a] + o[a] >= 0 && c[a] + o[a] < g;
      for (int64_t x = 0; x < g; ++x) {
        if (!in || x + o[dim - 1] < 0 || x + o[dim - 1] >= g) {
          if (P[row + x] != 0.0) return fail(MGCMT_ERR_INVALID, "point stencil: a coefficient towards a point outside the grid must be zero");
        } else if (P[row + x] != T[row + x + off]) {
          return fail(MGCMT_ERR_INVALID, dim == 3 ? "point stencil is not symmetric: the coefficient of p' in the row of p must equal that of p in the row of p'"
                                                  : "point stencil is not symmetric: the coefficient of (i', j') in row (i, j) must equal that of (i, j) in row (i', j')");
        }
      }
      for (int a = dim - 2; a >= 0 && ++c[a] == g; --a) c[a] = 0;
    }
  }
  return MGCMT_OK;
}

// bonds[a] (axis a counted from the fastest index) is zero where the index along its axis is g - 1: no bond leaves the grid
int check_bonds(int dim, int64_t g, const double* const* bonds) {
  if (g < 1) return MGCMT_OK;  // (build_plan refuses it)
  int64_t N = 1, s = 1;  // s: the distance between neighbours along axis a
  for (int a = 0; a < dim; ++a) N *= g;
  for (int a = 0; a < dim; ++a, s *= g)
    for (int64_t hi = 0; hi < N; hi += s * g)
      for (int64_t lo = 0; lo < s; ++lo)
        if (bonds[a][hi + (g - 1) * s + lo] != 0.0)
          return fail(MGCMT_ERR_INVALID,
                      dim == 3 ? "bonds towards points outside the grid (bx at x = g - 1, by at y = g - 1, bz at z = g - 1) must be zero"
                               : "bonds towards points outside the grid (the last column of east, the last row of south) must be zero");
  return MGCMT_OK;
}

// A plan with a per-point part, for all six creators: a whole 2-D or 3-D grid without a mass operator.  Desc: mgcmt_plan_desc
// (dim = 2) or mgcmt_plan3d_desc (dim = 3).
template <class Desc>
int create_point(int dim, const Desc* d, const PointPart& pt, mgcmt_plan** out) {
  static const char* const null_msg[] = {"", "null point diagonal", "null point stencil", "null point diagonal or bond array"};  // by kind
  static const char* const part[] = {"", "a point diagonal", "a point stencil", "a point diagonal with bonds"};
  static const char* const plan_with[] = {"", "a plan with a point diagonal", "a plan with a point diagonal (a point stencil)", "a plan with a point diagonal"};
  if (!d || !out) return fail(MGCMT_ERR_INVALID, "null argument");
  *out = nullptr;
  for (int a = 0; a < (pt.kind == kPointPlanes ? 1 : point_planes(dim, pt.kind)); ++a)
    if (!pt.planes[a]) return fail(MGCMT_ERR_INVALID, null_msg[pt.kind]);
  PlanSpec spec = spec_of(*d);
  if (spec.dim != dim) return fail(MGCMT_ERR_INVALID, std::string(part[pt.kind]) + " needs a 2-D plan (dim = 2)");  // (a 3-D desc has no dim to get wrong)
  if (dim == 3 && spec.lowest > 16) return fail(MGCMT_ERR_INVALID, "lowest must be at most 16 on a 3-D plan (the coarsest level is solved directly)");
  if (spec.m_nterms != 0)
    return fail(MGCMT_ERR_UNSUPPORTED, std::string(plan_with[pt.kind]) + " takes no mass operator (the Rayleigh-quotient entries do not run on it)");
  if (!((spec.row_begin == 0 && spec.row_end == 0) || (spec.row_begin == 0 && spec.row_end == spec.g)))
    return fail(MGCMT_ERR_UNSUPPORTED, std::string(plan_with[pt.kind]) + " is a whole grid (no row strips)");
  if (pt.kind == kPointBonds) MG_TRY(check_bonds(dim, spec.g, pt.planes + 1));
  if (pt.kind == kPointPlanes) MG_TRY(check_stencil(dim, spec.g, pt.planes[0]));
  spec.row_begin = spec.row_end = 0;
  spec.strip_levels = 0;
  spec.point = pt;
  return build_plan(spec, out);
}

}  // namespace

extern "C" {

int mgcmt_plan_create(const mgcmt_plan_desc* d, mgcmt_plan** out) {
  if (!d || !out) return fail(MGCMT_ERR_INVALID, "null argument");
  *out = nullptr;
  if (d->dim != 1 && d->dim != 2) return fail(MGCMT_ERR_INVALID, "dim must be 1 or 2");
  if (d->m_nterms < 0 || d->m_nterms > kMaxTerms) return fail(MGCMT_ERR_INVALID, "nterms out of range");
  return build_plan(spec_of(*d), out);
}

int mgcmt_plan_create_pot(const mgcmt_plan_desc* d, const double* point_diag, mgcmt_plan** out) {
  return create_point(2, d, PointPart{kPointDiag, {point_diag}}, out);
}

int mgcmt_plan_create_bonds(const mgcmt_plan_desc* d, const double* point_diag, const double* east, const double* south, mgcmt_plan** out) {
  return create_point(2, d, PointPart{kPointBonds, {point_diag, east, south}}, out);
}

int mgcmt_plan_create_nine(const mgcmt_plan_desc* d, const double* stencil, mgcmt_plan** out) {
  return create_point(2, d, PointPart{kPointPlanes, {stencil}}, out);
}

int mgcmt_plan_level_tiled(const mgcmt_plan* p, int l, int* tiled) {
  MG_TRY(check_level(p, l));
  if (!tiled) return fail(MGCMT_ERR_INVALID, "null argument");
  *tiled = p->dim == 2 && nine_tiled(p->kgrid(l), p->levels[l].dA.k) ? 1 : 0;
  return MGCMT_OK;
}

int mgcmt_plan_get_point_stencil(const mgcmt_plan* p, int l, double* out, int64_t capacity) {
  MG_TRY(check_level(p, l));
  if (!p->has_point) return fail(MGCMT_ERR_INVALID, "plan has no point diagonal");
  const PointView v = point_of(p, l);
  const int np = point_planes(p->dim, v.kind);
  const int64_t N = p->levels[l].nr * p->levels[l].gc;
  if (!out || capacity < np * N) return fail(MGCMT_ERR_INVALID, "point stencil buffer too small");
  // the interior of every plane (2-D level 0 of a diagonal or bonds: the rows between the halo rows, which are contiguous)
  for (int a = 0; a < np; ++a) MG_HIP(hipMemcpy(out + a * N, v.pg + a * v.pplane, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
  return MGCMT_OK;
}

int mgcmt_plan_set_point_diagonal(mgcmt_plan* p, int nterms, const double* coeffs, const int* slots, const int* vecs, void* stream) {
  entry_drops_carry(p);
  if (!p) return fail(MGCMT_ERR_INVALID, "null plan");
  if (!p->has_point) return fail(MGCMT_ERR_INVALID, "plan has no point diagonal");
  if (!coeffs || !slots || !vecs || nterms < 1 || nterms > 4) return fail(MGCMT_ERR_INVALID, "set_point_diagonal: 1..4 terms, non-null arguments");
  const double* v[4];
  for (int t = 0; t < nterms; ++t) {
    MG_TRY(check_vec(p, 0, slots[t], vecs[t]));
    MG_TRY(ensure_slot(p, 0, slots[t]));
    v[t] = p->kvec(0, slots[t], vecs[t]).p;
  }
  hipStream_t s = S(stream);
  // Level 0: the diagonal, plane D of {D, bonds} or the centre plane of a stencil — in each layout of build_point_part the
  // interior of that plane is nr * gc contiguous numbers at pg (+ centre * pplane), as the interior of a level vector is: the
  // halo rows of a padded 2-D plane lie outside it and stay exact zeros
  const PointView top = point_of(p, 0);
  const int centre = top.kind == kPointPlanes ? (point_planes(p->dim, kPointPlanes) - 1) / 2 : 0;
  launch_lincomb(s, p->interior(0), v, coeffs, nterms, const_cast<double*>(top.pg) + centre * top.pplane);
  MG_TRY(post_launch());
  // the levels below: the launches of build_point_part, in its order, into the planes it allocated
  for (size_t l = 1; l < p->levels.size(); ++l) {
    const Level &F = p->levels[l - 1], &L = p->levels[l];
    const PointView f = point_of(p, (int)l - 1);
    double* q = const_cast<double*>(point_of(p, (int)l).pg);
    const size_t N = (size_t)L.nr * L.gc;
    if (p->dim == 3) launch3p_coarsen(s, F.dA.k3.n, f.pg, point_planes(3, f.kind), f.pplane, q, (long)N);
    else launch_point_coarsen(s, F.nr, F.gc, f.pg, point_planes(2, f.kind), F.gc, f.pplane, q, L.gc, L.nr * L.gc);
    MG_TRY(post_launch());
  }
  // What is derived from the planes: the band factorisation and explicit inverse of a coarse solve (factor_coarse compares
  // this count, also in front of a graph replay).  The tail's matrix is not: a plan with a per-point part runs no tail.  Cached
  // cycle graphs hold the planes' addresses, which have not changed: they stay.
  ++p->point_version;
  return MGCMT_OK;
}

static int create3d(const mgcmt_plan3d_desc* d, int32_t m_nterms, const double* m_zfac, const double* m_yfac, const double* m_xfac,
                    mgcmt_plan** out) {
  if (!d || !out) return fail(MGCMT_ERR_INVALID, "null argument");
  *out = nullptr;
  if (d->lowest > 16) return fail(MGCMT_ERR_INVALID, "lowest must be at most 16 on a 3-D plan (the coarsest level is solved directly)");
  if (m_nterms < 0 || m_nterms > kMaxTerms) return fail(MGCMT_ERR_INVALID, "mass nterms out of range");
  if (m_nterms > 0 && (!m_xfac || !m_yfac || !m_zfac)) return fail(MGCMT_ERR_INVALID, "missing mass factor arrays");
  PlanSpec spec = spec_of(*d);
  spec.m_nterms = m_nterms;
  spec.m_fac[0] = m_zfac;
  spec.m_fac[1] = m_yfac;
  spec.m_fac[2] = m_xfac;
  return build_plan(spec, out);
}

int mgcmt_plan_create3d(const mgcmt_plan3d_desc* d, mgcmt_plan** out) { return create3d(d, 0, nullptr, nullptr, nullptr, out); }

int mgcmt_plan_create3d_pot(const mgcmt_plan3d_desc* d, const double* point_diag, mgcmt_plan** out) {
  return create_point(3, d, PointPart{kPointDiag, {point_diag}}, out);
}

int mgcmt_plan_create3d_bonds(const mgcmt_plan3d_desc* d, const double* point_diag, const double* bx, const double* by, const double* bz,
                              mgcmt_plan** out) {
  return create_point(3, d, PointPart{kPointBonds, {point_diag, bx, by, bz}}, out);
}

int mgcmt_plan_create3d_stencil(const mgcmt_plan3d_desc* d, const double* stencil, mgcmt_plan** out) {
  return create_point(3, d, PointPart{kPointPlanes, {stencil}}, out);
}

int mgcmt_plan3d_level_path(const mgcmt_plan* p, int l, int* kind, int* marching) {
  MG_TRY(check_level(p, l));
  if (p->dim != 3) return fail(MGCMT_ERR_INVALID, "mgcmt_plan3d_level_path needs a 3-D plan");
  const K3Op& k = p->levels[l].dA.k3;
  int path = 0, march = 0;  // (kinds: include/mgcmt_hip.h)
  switch (k.point) {
    case kPointNone:
      path = k.seven ? 1 : 0;
      march = k.seven && k.n >= 64 && k.n % 64 == 0;  // the constant level's own kernels (kernels_3d.hip)
      break;
    case kPointDiag:
      path = k.seven ? 2 : 4;
      march = point3_marching(k) != 0;
      break;
    case kPointPlanes:
      path = k.seven ? 7 : 3;
      march = stencil3_tiled(k) != 0;  // (kernels_3d_stencil.hip)
      break;
    case kPointBonds:
      path = k.seven ? 5 : 6;
      march = point3_marching(k) != 0;
      break;
  }
  if (kind) *kind = path;
  if (marching) *marching = march;
  return MGCMT_OK;
}

int mgcmt_plan_create3d_mass(const mgcmt_plan3d_desc* d, int32_t m_nterms, const double* m_zfac, const double* m_yfac, const double* m_xfac,
                             mgcmt_plan** out) {
  if (m_nterms < 1 || m_nterms > kMaxTerms) return fail(MGCMT_ERR_INVALID, "mass nterms out of range (1..4)");
  return create3d(d, m_nterms, m_zfac, m_yfac, m_xfac, out);
}

int mgcmt_plan_destroy(mgcmt_plan* p) {
  entry_drops_carry(p);
  if (!p) return MGCMT_OK;
  comm_release(p);
  for (Level& L : p->levels) {
    for (int s = 0; s < 4; ++s)
      if (L.base[s]) (void)hipFree(L.base[s]);
    for (double* q : L.dA.owned) (void)hipFree(q);
    for (double* q : L.dM.owned) (void)hipFree(q);
    if (L.band.b.ab) (void)hipFree(L.band.b.ab);
    if (L.band.b.piv) (void)hipFree(L.band.b.piv);
    if (L.band.inv) (void)hipFree(L.band.inv);
  }
  for (auto& g : p->graphs)
    if (g.second.exec) (void)hipGraphExecDestroy(g.second.exec);
  if (p->capture_stream) (void)hipStreamDestroy(p->capture_stream);
  if (p->d_rq) (void)hipFree(p->d_rq);
  if (p->d_wide_partials) (void)hipFree(p->d_wide_partials);
  if (p->d_wide_out) (void)hipFree(p->d_wide_out);
  if (p->d_wide_table) (void)hipFree(p->d_wide_table);
  if (p->d_orth_mask) (void)hipFree(p->d_orth_mask);
  if (p->d_rqstate) (void)hipFree(p->d_rqstate);
  if (p->d_rqhistory) (void)hipFree(p->d_rqhistory);
  if (p->d_mgs) (void)hipFree(p->d_mgs);
  if (p->d_pcg_block) (void)hipFree(p->d_pcg_block);
  if (p->tailmat.mt) (void)hipFree(p->tailmat.mt);
  if (p->lex_carry) (void)hipFree(p->lex_carry);
  if (p->lex_sync) (void)hipFree(p->lex_sync);
  if (p->d_shifts) (void)hipFree(p->d_shifts);
  if (p->d_zero) (void)hipFree(p->d_zero);
  if (p->d_partials) (void)hipFree(p->d_partials);
  if (p->d_scalars) (void)hipFree(p->d_scalars);
  delete p;
  return MGCMT_OK;
}

int mgcmt_plan_num_levels(const mgcmt_plan* p, int* levels) {
  if (!p || !levels) return fail(MGCMT_ERR_INVALID, "null argument");
  *levels = (int)p->levels.size();
  return MGCMT_OK;
}

int mgcmt_plan_level_shape(const mgcmt_plan* p, int l, int64_t* rows, int64_t* cols, int64_t* row_begin) {
  MG_TRY(check_level(p, l));
  if (rows) *rows = p->levels[l].nr;
  if (cols) *cols = p->levels[l].gc;
  if (row_begin) *row_begin = p->levels[l].r0;
  return MGCMT_OK;
}

int mgcmt_plan_get_factors(const mgcmt_plan* p, int op, int l, int which, double* out, int64_t capacity) {
  MG_TRY(check_level(p, l));
  const HostOp& h = op == MGCMT_OP_M ? p->levels[l].hM : p->levels[l].hA;
  if (op == MGCMT_OP_M && !p->has_mass) return fail(MGCMT_ERR_INVALID, "plan has no mass operator");
  if (p->dim == 3 && (which < 0 || which > 2)) return fail(MGCMT_ERR_INVALID, "which must be 0 (z), 1 (y) or 2 (x) on a 3-D plan");
  const std::vector<Tri>& f = which == 0 ? h.X : (which == 2 && p->dim == 3) ? h.Z : h.Y;
  int64_t need = 0;
  for (const Tri& t : f) need += (int64_t)t.a.size();
  if (!out || capacity < need) return fail(MGCMT_ERR_INVALID, "factor buffer too small");
  int64_t o = 0;
  for (const Tri& t : f) {
    memcpy(out + o, t.a.data(), t.a.size() * sizeof(double));
    o += (int64_t)t.a.size();
  }
  return MGCMT_OK;
}

int mgcmt_plan_level_halo(const mgcmt_plan* p, int l, int* halo_rows, int* exchanged) {
  MG_TRY(check_level(p, l));
  if (halo_rows) *halo_rows = p->levels[l].halo;
  if (exchanged) *exchanged = p->dim == 3 ? 0 : exchanged_rows(p, l);  // (a 3-D plan is never sharded)
  return MGCMT_OK;
}

int mgcmt_level_operator_kind(const mgcmt_plan* p, int l, int* kind) {
  MG_TRY(mgcmt::unsupported_3d(p, "mgcmt_level_operator_kind"));
  MG_TRY(check_level(p, l));
  if (!kind) return fail(MGCMT_ERR_INVALID, "null output");
  const KOp& k = p->levels[l].dA.k;
  if (k.point) {
    *kind = k.point == kPointDiag ? MGCMT_OPK_POINT_DIAG : k.point == kPointBonds ? MGCMT_OPK_POINT_BONDS : MGCMT_OPK_NINE_POINT;
    return MGCMT_OK;
  }
  *kind = k.five_point ? MGCMT_OPK_FIVE_POINT : k.five_diag ? MGCMT_OPK_FIVE_DIAG : k.nine_const ? MGCMT_OPK_NINE_CONST : k.nine_var ? MGCMT_OPK_NINE_VAR : MGCMT_OPK_GENERAL;
  return MGCMT_OK;
}

}  // extern "C"
