// Two-level fused passes: level l (constant 5-point, weighted Jacobi) and level l+1 (its Galerkin coarsening, Op9c)
// marched by the same wave in one launch.  The level-1 passes of the V-cycle are latency-bound (waves waiting 50-60 %
// of their cycles) and re-read from HBM what the fine passes have just written (F[l+1]) or are about to read (V[l+1]);
// here level l+1's stages run a fixed number of rows behind (down) or ahead of (up) the fine stages instead:
//
//   down:  fine  NF sweeps from V (not stored) -> residual -> restriction, storing F[l+1]
//          l+1   2 sweeps from zero (not stored)       -> residual -> restriction, storing F[l+2]
//   up:    l+1   2 sweeps from zero (the down pass's, recomputed) -> += P V[l+2] -> 2 sweeps    (v1, in registers)
//          fine  NF sweeps from V (the down pass's, recomputed)    -> += P v1     -> 2 sweeps, storing V'
//
// V[l+1] is never written (an up pass leaves it as scratch).  Arithmetic is that of k_fused (fused_kernel.h) stage
// by stage — the same policies, the same fma()s, the same zeros for ghosts — so the results are bit-identical to the
// four single-level passes they replace.
//
// Mapping: as k_fused, a wave64 per 128-column window, two fine columns per lane, 16-byte fine accesses, DPP lane
// shifts, no LDS, no barriers.  Level l+1 has ONE column per lane (coarse column jc = ja / 2); window origins are
// multiples of 4, so that coarse column parity is lane parity and level-l+2 columns sit on even lanes.  Halo (per
// side): down 6 lanes = 12 fine columns (104 of 128 kept), up 8 lanes = 16 columns (96 kept: whole cache lines of V').
// Rows: the march starts on a multiple of 4 and a loop body is 12 fine steps = 6 coarse steps, so every row parity,
// coarse row parity and rotating-window slot is known at compile time.
#pragma once
#include "fused_kernel.h"

namespace mgcmt {

namespace fused {

struct Fused2Args {
  FusedArgs fine, coarse;  // operator data of the two levels (policy init); fine.omega / shifts serve both
  const double* v;         // fine V (read unless ZERO_IN)
  const double* f;         // fine F
  double* vout;            // fine V' (up)
  double* f1;              // F[l+1]: written (down) / read (up)
  double* fcarry;          // carrying up pass: the next cycle's F[l+1], written (never F[l+1] itself: other waves read it)
  double* c2;              // F[l+2] written (down) / V[l+2] read (up)
  long s0, s1, s2;         // vector strides of the three levels
  int nr, nc, cnr, cnc, c2nc;
  int rows_per_chunk, n_row_chunks, n_col_groups, xcd_balanced;
};

template <bool UP>
struct Fused2Shape {
  static constexpr int H = UP ? 8 : 6;          // halo lanes per side
  static constexpr int wout = 128 - 4 * H;      // fine columns a wave stores / owns
  static constexpr int B = 12;                  // fine steps per loop body
};

// UP = false: NF = fine sweeps of the down pass.  UP = true: NF = fine sweeps recomputed in front of the correction
// (the fine post-smoothing is 2 sweeps; level l+1 smooths 2 sweeps per leg).
//
// CARRY (up only): the pass goes on, behind the stage that stores row rs of V', with the fine part of the NEXT cycle's
// down pass on the rows it holds in registers — NF sweeps (not stored), the residual, the restriction — and stores that
// cycle's F[l+1] through a.fcarry.  The stages are the down branch's (eval_a / eval_b, racc, the store predicate), their
// input is the row just stored instead of a loaded one, so the values are the bits the next down pass would write.
//   columns: V' is good 12 fine columns inside the window (above); a sweep and the residual reach one column further
//   each, the restriction of the last owned coarse column reads the residual of the next lane's first column: NF + 1
//   more columns on the left, NF + 2 on the right — within the 16 of H = 8 for NF <= 2.
//   rows: the residual of row r_begin (the first that a coarse row of the chunk takes) needs V' from row
//   r_begin - 1 - NF on: the march starts 4 rows earlier; the residual of row r_end is the last, NF + 2 steps behind
//   the last stored row of V'.
template <bool UP, int NF, bool ZERO_IN, bool CARRY = false>
__global__ void __launch_bounds__(64) k_fused2(Fused2Args a) {
  using Shape = Fused2Shape<UP>;
  constexpr int H = Shape::H, WOUT = Shape::wout, B = Shape::B;
  static_assert(!CARRY || (UP && !ZERO_IN), "only an up pass on a nonzero iterate carries");
  static_assert(!CARRY || 12 + NF + 2 <= 2 * H, "the carried stages must stay inside the halo");
  constexpr int SF = UP ? NF + 2 : NF;     // fine smoothing stages
  constexpr int EF = UP ? 0 : 1;           // fine residual stage (down)
  constexpr int TF = CARRY ? NF + 1 : 0;   // carried stages behind the store of V': NF sweeps and the residual
  constexpr int SR = UP ? (CARRY ? SF + NF : -1) : SF;  // index of the residual stage (-1: none)
  constexpr int SC = UP ? 4 : 2;           // coarse smoothing stages
  constexpr int PC = UP ? 0 : (NF + 1) & 1;  // parity of the fine steps that carry a coarse step
  constexpr int CROW = UP ? 4 : -2;        // coarse input row of a coarse step = base / 2 + U + CROW
  // rows per prefetch batch: the up pass's seven stage windows leave room for two (three: 256 + registers, 1 wave/SIMD)
  // (the carrying pass with NF = 2 is over 256 registers and runs 1 wave / SIMD either way; 3, 4 and 6 rows per batch
  // measured no faster there than 2: profiles/r20_carry.md)
  constexpr int D = UP ? 2 : kDepth;
  constexpr int NS = 2;
  static_assert(B % D == 0 && (B / D) % NS == 0, "the loop body must hold whole rotations of the prefetch sets");
  static_assert(B % 4 == 0, "coarse row parities must repeat with the body");

  const int b = blockIdx.x;
  const int xcd = b & 7, seq = b >> 3;
  int group, chunk;
  if (a.xcd_balanced) {
    const long total = (long)a.n_col_groups * a.n_row_chunks;
    const long lo = xcd * total / 8, hi = (xcd + 1) * total / 8;
    if (lo + seq >= hi) return;
    const int item = (int)(lo + seq);
    chunk = item / a.n_col_groups;
    group = item - chunk * a.n_col_groups;
  } else {
    const int per_xcd = (a.n_col_groups + 7) >> 3;
    group = xcd * per_xcd + seq % per_xcd;
    chunk = seq / per_xcd;
    if (seq % per_xcd + xcd * per_xcd >= a.n_col_groups || chunk >= a.n_row_chunks) return;
  }
  if (group >= a.n_col_groups) return;
  const int lane = threadIdx.x & 63;
  const int lane_up = (lane > 0 ? lane - 1 : 0) << 2, lane_dn = (lane < 63 ? lane + 1 : 63) << 2;
  (void)lane_up;
  (void)lane_dn;
  const int nr = a.nr, nc = a.nc, cnr = a.cnr, cnc = a.cnc, c2nc = a.c2nc;
  const int strip = group;
  if (strip * WOUT >= nc) return;  // wave-uniform
  const int q = blockIdx.y;

  // fine columns ja, ja + 1; coarse column jc (one per lane); level-l+2 column j2 (of the even lanes)
  const int ja = strip * WOUT - 2 * H + 2 * lane;
  const int jc = ja >> 1, j2 = jc >> 1;
  const bool col_in = ja >= 0 && ja < nc;
  const bool ccol_in = jc >= 0 && jc < cnc;
  const bool c2col_in = j2 >= 0 && j2 < c2nc;
  const bool own = lane >= H && lane < 64 - H;  // the lanes whose columns this wave stores
  const double lanemask = col_in ? 1.0 : 0.0, cmask = ccol_in ? 1.0 : 0.0, c2mask = c2col_in ? 1.0 : 0.0;
  const double omega = col_in ? a.fine.omega : 0.0;
  const double comega = ccol_in ? a.fine.omega : 0.0;
  const bool jodd = (lane & 1) != 0;  // coarse column parity (window origins are multiples of 4)

  const double* __restrict__ vin = a.v + q * a.s0;
  const double* __restrict__ fin = a.f + q * a.s0;
  double* __restrict__ vout = a.vout + q * a.s0;
  double* __restrict__ f1 = a.f1 + q * a.s1;
  double* __restrict__ c2 = a.c2 + q * a.s2;
  double* __restrict__ fres = CARRY ? a.fcarry + q * a.s1 : f1;  // where the restricted fine residual goes

  const int r_begin = chunk * a.rows_per_chunk;  // (a multiple of 4)
  const int r_end = r_begin + a.rows_per_chunk < nr ? r_begin + a.rows_per_chunk : nr;
  const int crow_b = r_begin >> 1, crow_e = r_end >> 1;  // coarse rows of the chunk
  // first fine step: down — F[l+1] rows from crow_b - 2 on feed level l+1's stages, they need fine rows from r_begin - 7;
  // up — v1 rows from crow_b - 2 on, i.e. F[l+1] rows from crow_b - 6 on, loaded 4 coarse rows ahead of the fine stream
  const int rstart = UP ? (CARRY ? r_begin - 24 : r_begin - 20) : r_begin - 8;
  // one past the last step: down — the last level-l+2 row (coarse row crow_e + 3 in); up — the last V' row (carrying:
  // the residual of row r_end)
  const int rstop = UP ? (CARRY ? r_end + SF + NF + 2 : r_end + SF) : r_end + 10 + NF;

  const int ja_ld = ja < 0 ? 0 : (ja > nc - 2 ? nc - 2 : ja);
  const int jc_ld = jc < 0 ? 0 : (jc > cnc - 1 ? cnc - 1 : jc);
  const int j2_ld = j2 < 0 ? 0 : (j2 > c2nc - 1 ? c2nc - 1 : j2);

  Op5 op;
  op.init(a.fine, q, ja, nc);
  Op9c cop;
  cop.init(a.coarse, q, jc - 1, cnc);  // the lane's column is the policy's COL 1 (the per-lane last-column terms)

  struct Row {
    double2 v, f;
    double cf, ce;  // up: F[l+1] and V[l+2] of the coarse row loaded with this fine row
  };
  Row sets[NS][D];
  int frow = rstart;
  auto fetch = [&](auto pos, Row& r) __attribute__((always_inline)) {
    constexpr int T = decltype(pos)::value;
    const int t = frow < nr - 1 ? frow : nr - 1;
    const int frl = t > 0 ? t : 0;
    const long fbase = (long)frl * nc;
    if (ZERO_IN) r.v = make_double2(0.0, 0.0);
    else r.v = load2(vin + fbase + ja_ld);
    r.f = load2_stream(fin + fbase + ja_ld);
    r.cf = r.ce = 0.0;
    if (UP && ((T - PC) & 1) == 0) {
      const int ic = (frow >> 1) + CROW;
      const int it = ic < cnr - 1 ? ic : cnr - 1;
      const int icl = it > 0 ? it : 0;
      r.cf = f1[(long)icl * cnc + jc_ld];
      r.ce = c2[(long)(icl >> 1) * c2nc + j2_ld];
    }
    ++frow;
  };
  static_for<0, D>([&](auto u) __attribute__((always_inline)) {
    constexpr int U = decltype(u)::value;
    fetch(StepIndex<U>{}, sets[0][U]);
  });

  // fine stage windows (w[s]: input of stage s + 1; w[SF]: the residual stage's), rotating as in k_fused
  constexpr int NW = SF + EF + TF;
  static_assert(NW < B, "the right-hand side ring must hold the lag of the last stage");
  double wa[NW][3], wb[NW][3];
#pragma unroll
  for (int s = 0; s < NW; ++s)
#pragma unroll
    for (int r = 0; r < 3; ++r) wa[s][r] = wb[s][r] = 0.0;
  double fa[B], fb[B];  // fine right-hand side of row (row - k): slot modn(T - k, B)
#pragma unroll
  for (int s = 0; s < B; ++s) fa[s] = fb[s] = 0.0;
  double er[B], el[B];  // up: v1 of fine row (row - k) and of the lane to the left, slot modn(T - k, B)
#pragma unroll
  for (int s = 0; s < B; ++s) er[s] = el[s] = 0.0;
  // coarse stage windows cw[s] (input of stage s + 1, s >= 1; the first stage's input is zero) with the lateral
  // neighbours; cfr: coarse right-hand side ring, cer / cel: V[l+2] values of coarse rows (slot modn(U - k, 6))
  constexpr int CB = B / 2;
  constexpr int NCW = UP ? SC - 1 : SC;  // windows of stages 1 .. SC - 1 (+ the residual stage's)
  double cw[NCW][3], cl[NCW][3], cr[NCW][3];
#pragma unroll
  for (int s = 0; s < NCW; ++s)
#pragma unroll
    for (int r = 0; r < 3; ++r) cw[s][r] = cl[s][r] = cr[s][r] = 0.0;
  double cfr[CB], cer[CB], cel[CB];
#pragma unroll
  for (int s = 0; s < CB; ++s) cfr[s] = cer[s] = cel[s] = 0.0;
  double v1c = 0.0;     // up: the newest v1 value (coarse row row / 2)
  double racc = 0.0;    // running restriction sums: fine -> F[l+1], coarse -> F[l+2]
  double racc2 = 0.0;
  unsigned okbits = 0, cokbits = 0;  // bit k: fine row (row - k) / coarse row (input - k) inside the grid

  // one coarse step at coarse position U: the coarse input row ic (down: its right-hand side just restricted)
  auto coarse_step = [&](auto upos, auto chk, const int ic, const double fin1, const double e2) __attribute__((always_inline)) {
    constexpr int U = decltype(upos)::value;
    constexpr bool CHK = decltype(chk)::value;
    const bool cok = CHK ? (ic >= 0 && ic < cnr) : true;
    if (CHK) cokbits = (cokbits << 1) | (cok ? 1u : 0u);
    cfr[modn(U, CB)] = fin1;
    if (UP) {
      cer[modn(U, CB)] = e2 * (cok ? c2mask : 0.0);
      cel[modn(U, CB)] = MGCMT_FETCH_LEFT(lane_up, cer[modn(U, CB)]);
    }
    double o = 0.0;  // output of the previous stage
#pragma unroll
    for (int s = 0; s <= SC; ++s) {
      if (s == SC && UP) break;
      const int rs = ic - (s + 1);
      const int sn = mod3(U - s), sa = mod3(U - s + 1), sc = mod3(U - s + 2);
      const int w = s - 1;  // window of stage s (s >= 1)
      if (s >= 1) {
        cw[w][sn] = o;
        cl[w][sn] = MGCMT_FETCH_LEFT(lane_up, o);
        cr[w][sn] = MGCMT_FETCH_RIGHT(lane_dn, o);
      }
      const double cc = s >= 1 ? cw[w][sc] : 0.0;
      const double fv = cfr[modn(U - (s + 1), CB)];
      const bool in = !CHK || ((cokbits >> (s + 1)) & 1u) != 0;
      auto eval = [&](double& off, double& dg, double& inv) __attribute__((always_inline)) {
        if (s >= 1) {
          const double n[3] = {cl[w][sa], cw[w][sa], cr[w][sa]}, c[3] = {cl[w][sc], cc, cr[w][sc]}, so[3] = {cl[w][sn], cw[w][sn], cr[w][sn]};
          cop.template eval<1>(n, c, so, off, dg, inv);
          if (CHK && cop.special_row(rs)) cop.template fix_special<1>(c, off, dg, inv);
        } else {
          const double z[3] = {0.0, 0.0, 0.0};
          cop.template eval<1>(z, z, z, off, dg, inv);
          if (CHK && cop.special_row(rs)) cop.template fix_special<1>(z, off, dg, inv);
        }
      };
      if (s < SC) {
        double nv = cc;
        if (in) {
          double off, dg, inv;
          eval(off, dg, inv);
          nv = fma(comega, (fv - fma(dg, cc, off)) * inv, cc);
        }
        if (UP && s == 1) {
          // += P V[l+2] on row rs (the recomputed pre-smoothing ends here): even coarse column takes the mean of
          // level-l+2 columns j2 - 1 and j2, an even row the mean of level-l+2 rows
          const double e_cur = cer[modn(U - 2, CB)], e_prev = cer[modn(U - 3, CB)];
          double ca = 0.5 * (cel[modn(U - 2, CB)] + e_cur), cb2 = e_cur;
          if (((U - 2 + CROW) & 1) == 0) {
            ca = 0.5 * (0.5 * (cel[modn(U - 3, CB)] + e_prev) + ca);
            cb2 = 0.5 * (e_prev + cb2);
          }
          const double m = in ? cmask : 0.0;
          nv = fma(m, jodd ? cb2 : ca, nv);
        }
        o = nv;
        if (UP && s == SC - 1) v1c = o;
      } else {
        // coarse residual of row rs and its restriction to level l+2 (on the even lanes)
        double r = 0.0;
        if (in) {
          double off, dg, inv;
          eval(off, dg, inv);
          r = cmask * (fv - fma(dg, cc, off));
        }
        const double r1 = MGCMT_FETCH_RIGHT(lane_dn, r);
        const double r2 = MGCMT_FETCH_RIGHT(lane_dn, r1);
        const double h = 0.25 * r + 0.5 * r1 + 0.25 * r2;
        if (((U - (s + 1) + CROW) & 1) == 0) {
          const int I2 = (rs >> 1) - 1;
          if (own && !jodd && c2col_in && (!CHK || (2 * I2 >= crow_b && 2 * I2 < crow_e))) c2[(long)I2 * c2nc + j2] = racc2 + 0.25 * h;
          racc2 = 0.25 * h;
        } else {
          racc2 += 0.5 * h;
        }
      }
    }
  };

  auto step = [&](auto pos, auto chk, const int row, const Row& in) __attribute__((always_inline)) {
    constexpr int T = decltype(pos)::value;
    constexpr bool CHK = decltype(chk)::value;
    constexpr bool CSTEP = ((T - PC) & 1) == 0;
    constexpr int U = (T - PC) / 2;  // coarse position (CSTEP)
    const bool rok = CHK ? (row >= 0 && row < nr) : true;
    if (CHK) okbits = (okbits << 1) | (rok ? 1u : 0u);
    if constexpr (UP && CSTEP) coarse_step(StepIndex<U>{}, chk, (row >> 1) + CROW, in.cf, in.ce);
    double ina = 0.0, inb = 0.0;
    if (!ZERO_IN) {
      const double m = rok ? lanemask : 0.0;
      ina = in.v.x * m;
      inb = in.v.y * m;
    }
    if (UP) {
      er[T] = v1c * (rok ? cmask : 0.0);
      el[T] = MGCMT_FETCH_LEFT(lane_up, er[T]);
    }
    auto correct = [&](int lag, double& va, double& vb) __attribute__((always_inline)) {
      const double e_cur = er[modn(T - lag, B)], e_prev = er[modn(T - lag - 1, B)];
      double ca = 0.5 * (el[modn(T - lag, B)] + e_cur), cb = e_cur;
      if (((T - lag) & 1) == 0) {
        ca = 0.5 * (0.5 * (el[modn(T - lag - 1, B)] + e_prev) + ca);
        cb = 0.5 * (e_prev + cb);
      }
      const double m = (!CHK || ((okbits >> lag) & 1u)) ? lanemask : 0.0;
      va = fma(m, ca, va);
      vb = fma(m, cb, vb);
    };
    fa[T] = in.f.x;
    fb[T] = in.f.y;
    double oa = ina, ob = inb;
#pragma unroll
    for (int s = 0; s < NW; ++s) {
      const int sn = mod3(T - s), sa = mod3(T - s + 1), sc = mod3(T - s + 2);
      wa[s][sn] = oa;
      wb[s][sn] = ob;
      const int rs = row - (s + 1);
      const double ca = wa[s][sc], cb = wb[s][sc];
      const double fva = fa[modn(T - (s + 1), B)], fvb = fb[modn(T - (s + 1), B)];
      auto eval_a = [&](double& off, double& dg, double& inv) __attribute__((always_inline)) {
        const double left = MGCMT_FETCH_LEFT(lane_up, cb);
        const double n[3] = {0.0, wa[s][sa], 0.0}, c[3] = {left, ca, cb}, so[3] = {0.0, wa[s][sn], 0.0};
        op.template eval<0>(n, c, so, off, dg, inv);
      };
      auto eval_b = [&](double& off, double& dg, double& inv) __attribute__((always_inline)) {
        const double right = MGCMT_FETCH_RIGHT(lane_dn, ca);
        const double n[3] = {0.0, wb[s][sa], 0.0}, c[3] = {ca, cb, right}, so[3] = {0.0, wb[s][sn], 0.0};
        op.template eval<1>(n, c, so, off, dg, inv);
      };
      const bool in_grid = !CHK || ((okbits >> (s + 1)) & 1u) != 0;
      if (s != SR) {
        double na = ca, nb = cb;
        if (in_grid) {
          double off, dg, inv;
          eval_a(off, dg, inv);
          na = fma(omega, (fva - fma(dg, ca, off)) * inv, ca);
          eval_b(off, dg, inv);
          nb = fma(omega, (fvb - fma(dg, cb, off)) * inv, cb);
        }
        oa = na;
        ob = nb;
        if (UP && s == NF - 1) correct(s + 1, oa, ob);
        if (UP && s == SF - 1) {
          if (own && col_in && (!CHK || (rs >= r_begin && rs < r_end))) store2_stream(vout + (long)rs * nc + ja, oa, ob);
        }
      } else {
        // fine residual of row rs and its restriction; a finished coarse row feeds level l+1's stages
        double ra = 0.0, rb = 0.0;
        if (in_grid) {
          double offa, offb, dga, dgb, inva, invb;
          eval_a(offa, dga, inva);
          eval_b(offb, dgb, invb);
          ra = lanemask * (fva - fma(dga, ca, offa));
          rb = lanemask * (fvb - fma(dgb, cb, offb));
        }
        const double rnext = MGCMT_FETCH_RIGHT(lane_dn, ra);
        const double h = 0.25 * ra + 0.5 * rb + 0.25 * rnext;
        if (((T - (s + 1)) & 1) == 0) {
          const int I = (rs >> 1) - 1;
          const double v1 = racc + 0.25 * h;
          if (own && ccol_in && (!CHK || (I >= crow_b && I < crow_e))) fres[(long)I * cnc + jc] = v1;
          racc = 0.25 * h;
          if constexpr (!UP && CSTEP) coarse_step(StepIndex<U>{}, chk, I, v1, 0.0);
        } else {
          racc += 0.5 * h;
        }
      }
    }
  };

  auto body = [&](auto chk, const int base) __attribute__((always_inline)) {
    static_for<0, B / D>([&](auto g) __attribute__((always_inline)) {
      constexpr int G = decltype(g)::value;
      Row* cur = sets[G % NS];
      Row* nxt = sets[(G + 1) % NS];
      static_for<0, D>([&](auto u) __attribute__((always_inline)) {
        constexpr int U = decltype(u)::value;
        fetch(StepIndex<((G + 1) * D + U) % B>{}, nxt[U]);
      });
      static_for<0, D>([&](auto u) __attribute__((always_inline)) {
        constexpr int U = decltype(u)::value;
        step(StepIndex<G * D + U>{}, chk, base + G * D + U, cur[U]);
      });
    });
  };
  // Bodies whose every row is inside both grids, off level l+1's last row, and whose every store lies inside the
  // chunk run without row tests (see k_fused)
  // (carrying: the first coarse row stored without a test is row crow_b, restricted from the residual of row r_begin + 2)
  const int fast_lo = UP ? (CARRY ? r_begin + SF + NF + 3 : r_begin + 4) : r_begin + 14;
  // (carrying: fast_last does not grow with the tail's lag — the last row of V' stored without a test, r_end - 1 at step
  // r_end - 1 + SF, bounds it as before; the carried coarse rows of such a body lie NF + 1 steps further back, below crow_e)
  int fast_last = UP ? (r_end - 12 + SF < nr - 20 ? r_end - 12 + SF : nr - 20) : (r_end - 8 < nr - 12 ? r_end - 8 : nr - 12);
  int base = rstart;
#pragma nounroll
  for (int phase = 0; phase < 2; ++phase) {
    int stop = rstop;
    if (phase == 0) {
      stop = fast_lo > rstart ? rstart + ((fast_lo - rstart + B - 1) / B) * B : rstart;
      if (stop > rstop) stop = rstop;
    }
#pragma nounroll
    for (; base < stop; base += B) body(Checked<true>{}, base);
    if (phase == 0) {
#pragma nounroll
      for (; base <= fast_last; base += B) {
        body(Checked<false>{}, base);
        okbits = ~0u;
        cokbits = ~0u;
      }
    }
  }
}

template <bool UP, int NF, bool ZERO_IN, bool CARRY = false>
void launch_two(hipStream_t s, Fused2Args a, int k, long rows_override) {
  using Shape = Fused2Shape<UP>;
  const long groups = (a.nc + Shape::wout - 1) / Shape::wout;
  const long groups8 = (groups + 7) / 8 * 8;
  a.n_col_groups = (int)groups;
  static int resident_blocks = 0;
  if (resident_blocks == 0) {
    int per_cu = 0, dev = 0;
    hipDeviceProp_t prop;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_fused2<UP, NF, ZERO_IN, CARRY>, 64, 0) != hipSuccess ||
        hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess || per_cu < 1)
      resident_blocks = 768;
    else
      resident_blocks = per_cu * prop.multiProcessorCount;
  }
  const long nrows = a.nr;
  long rows = rows_override;
  if (rows <= 0) {
    long chunks = (long)(MGCMT_FUSED_FILL * resident_blocks) / (groups * k);
    if (chunks < 1) chunks = 1;
    rows = (nrows + chunks - 1) / chunks;
  }
  rows = (rows + 3) & ~3L;  // chunks start on multiples of 4: whole coarse row pairs
  if (rows < 4) rows = 4;
  if (rows > nrows) rows = (nrows + 3) & ~3L;
  a.rows_per_chunk = (int)rows;
  a.n_row_chunks = (int)((nrows + rows - 1) / rows);
  a.xcd_balanced = (groups8 * 100 > groups * (100 + MGCMT_FUSED_XCD_IMBALANCE) && groups < MGCMT_FUSED_XCD_MAXGROUPS) ? 1 : 0;
  const unsigned blocks = (unsigned)(groups8 * a.n_row_chunks);
  hipLaunchKernelGGL((k_fused2<UP, NF, ZERO_IN, CARRY>), dim3(blocks, (unsigned)k), dim3(64), 0, s, a);
}

}  // namespace fused

}  // namespace mgcmt
