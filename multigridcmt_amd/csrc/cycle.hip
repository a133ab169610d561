// The single-GPU cycle: smoothers, the legs of a V-cycle as fused passes, two-level passes and single launches, the
// cycle's tail, the 3-D legs, Gram-Schmidt between the levels, the HIP-graph cache that replays whole launch sequences,
// and the C-ABI entries of the cycle and its pieces.  Residual + restriction is chosen in one place (residual_to_coarse) and
// the coarsest level is (re)factored in one (factor_coarse).  Host code only; every kernel it enqueues is in kernels_*.hip.
#include <cstdio>
#include <string>
#include <vector>

#include "plan_internal.h"

using namespace mgcmt;

namespace mgcmt {
// one fused pass V -> T (then swapped) on a level the fused kernels cover
int fused_pass(mgcmt_plan* p, int l, int kind, int nsweep, double omega, int mode, int k, hipStream_t s, int npre, long out_lo,
               long out_hi, bool swap, long out_lo2, long out_hi2) {
  Level& L = p->levels[l];
  KVec coarse{nullptr, 0};
  long cnc = 0;
  if ((mode & 3) != 0) {
    coarse = p->kvec(l + 1, (mode & 3) == 1 ? MGCMT_SLOT_V : MGCMT_SLOT_F);
    cnc = p->levels[l + 1].gc;
  }
  // rows beyond a strip that hold the neighbours' data (the passes read no further: exchanged_rows)
  const long hx = exchanged_rows(p, l);
  const long row_lo = L.r0 == 0 ? 0 : -hx;
  const long row_hi = L.r0 + L.nr == L.gr ? L.nr : L.nr + hx;
  launch_fused(s, p->kgrid(l), L.dA.k, p->kvec(l, MGCMT_SLOT_V), p->kvec(l, MGCMT_SLOT_F), p->kvec(l, MGCMT_SLOT_T), coarse, cnc,
               p->d_shifts, omega, kind == MGCMT_GS_MC ? 1 : 0, nsweep, mode, npre, row_lo, row_hi, L.gr - 1 - L.r0, k, p->fused_rows,
               out_lo, out_hi, out_lo2, out_hi2);
  if (swap && !(mode & 8)) std::swap(L.base[MGCMT_SLOT_V], L.base[MGCMT_SLOT_T]);  // a no-store pass leaves V as it was
  return MGCMT_OK;
}

bool fused_level(const mgcmt_plan* p, int l, int kind) {
  return p->use_fused && (kind == MGCMT_WJACOBI || kind == MGCMT_GS_MC) && fused_supported(p->kgrid(l), p->levels[l].dA.k);
}

int pass_sweeps(const mgcmt_plan* p, int l, int kind, int left) {
  const int cap = fused_max_sweeps(p->levels[l].dA.k, kind == MGCMT_GS_MC ? 1 : 0);
  return left < cap ? left : cap;
}

int exchanged_rows(const mgcmt_plan* p, int l) {
  const Level& L = p->levels[l];
  const KOp& k = L.dA.k;
  const int want = (k.five_point || k.five_diag) ? 8 : 10;
  return want < L.halo ? want : L.halo;
}
}  // namespace mgcmt

namespace {

// nsweeps generalised lexicographic sweeps on vector slot `slot` (right-hand side: slot `fslot`), each followed by
// slot += gamma * fslot: the wave pipeline where it covers the level (sweeps chained in one launch, the update inside
// the sweep), the one-workgroup kernel otherwise
int lex_sweep(mgcmt_plan* p, int l, int slot, double alpha, double beta, double wU, double wL, int k, hipStream_t s, int nsweeps = 1,
              double gamma = 0.0, int fslot = MGCMT_SLOT_F) {
  auto update = [&]() {
    if (gamma != 0.0)
      for (int q = 0; q < k; ++q) launch_axpy(s, p->interior(l), gamma, p->kvec(l, fslot, q).p, p->kvec(l, slot, q).p);
  };
  const KGrid g = p->kgrid(l);
  const KOp& op = p->levels[l].dA.k;
  if (p->use_lex_wave && p->levels[l].nr == p->levels[l].gr && lex_wave_supported(g, op)) {
    const bool band = p->use_lex_wave == 2;
    const size_t blocks = (size_t)lex_wave_blocks(g);
    const size_t need_scan = (size_t)lex_wave_carry(g, p->nvec, nsweeps), need_band = (size_t)p->nvec * lex_band_count(g) * lex_band_stride(g);
    const size_t need_carry = band ? need_band : need_scan, need_sync = 2 + 4 * (size_t)p->nvec * blocks;  // (2 words used; the rest is the diagnostic build's per-block record)
    if (need_carry > p->lex_carry_doubles || need_sync > p->lex_sync_words) {
      // cached cycle graphs hold the old scratch pointers in their memset / kernel nodes: they go before the buffers do
      // (a graph replayed after this point would write through freed memory)
      p->graphs_invalidate();
      MG_HIP(hipStreamSynchronize(s));
      if (p->lex_carry) (void)hipFree(p->lex_carry);
      if (p->lex_sync) (void)hipFree(p->lex_sync);
      p->lex_carry = nullptr;
      p->lex_sync = nullptr;
      p->lex_carry_doubles = p->lex_sync_words = 0;
      if (hipMalloc((void**)&p->lex_carry, need_carry * sizeof(double)) != hipSuccess ||
          hipMalloc((void**)&p->lex_sync, need_sync * sizeof(unsigned)) != hipSuccess)
        return fail(MGCMT_ERR_NOMEM, "scratch of the lexicographic wave pipeline");
      MG_HIP(hipMemset(p->lex_sync, 0, need_sync * sizeof(unsigned)));
      p->lex_carry_doubles = need_carry;
      p->lex_sync_words = need_sync;
    }
    if (band) {
      for (int it = 0; it < nsweeps; ++it) {
        launch_lex_band(s, g, op, p->kvec(l, slot), p->kvec(l, fslot), p->d_shifts, alpha, beta, wU, wL, k, p->lex_carry, p->lex_sync);
        update();
      }
    } else if (p->lex_chain) {
      launch_lex_wave(s, g, op, p->kvec(l, slot), p->kvec(l, fslot), p->d_shifts, alpha, beta, wU, wL, k, p->lex_carry, p->lex_sync, nsweeps, gamma);
    } else {
      for (int it = 0; it < nsweeps; ++it)
        launch_lex_wave(s, g, op, p->kvec(l, slot), p->kvec(l, fslot), p->d_shifts, alpha, beta, wU, wL, k, p->lex_carry, p->lex_sync, 1, gamma);
    }
    p->lex_wave_used = true;
    return MGCMT_OK;
  }
  for (int it = 0; it < nsweeps; ++it) {
    launch_lex_sweep(s, g, op, p->kvec(l, slot), p->kvec(l, fslot), p->d_shifts, alpha, beta, wU, wL, k);
    update();
  }
  return MGCMT_OK;
}

}  // namespace

// a synchronising call looks at the error word of the wave pipeline (a block that gave up waiting)
int mgcmt::lex_wave_check(mgcmt_plan* p) {
  if (!p->lex_wave_used || !p->lex_sync) return MGCMT_OK;
  p->lex_wave_used = false;
  unsigned err = 0;
  MG_HIP(hipMemcpy(&err, p->lex_sync + 1, sizeof(unsigned), hipMemcpyDeviceToHost));
  if (err != 0) {
    MG_HIP(hipMemset(p->lex_sync + 1, 0, sizeof(unsigned)));  // reported: the next sweeps start clean
    return fail(MGCMT_ERR_HIP, "lexicographic wave pipeline: a block timed out waiting for its neighbour");
  }
  return MGCMT_OK;
}

namespace {
int smooth3(mgcmt_plan* p, int l, int kind, int nu, double omega, int k, hipStream_t s);
}

int mgcmt::smooth_impl(mgcmt_plan* p, int l, int kind, int nu, double omega, int k, hipStream_t s) {
  if (p->dim == 3) return smooth3(p, l, kind, nu, omega, k, s);
  MG_TRY(unsupported_point_smoother(p, kind));
  Level& L = p->levels[l];
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_V));
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_F));
  const KGrid g = p->kgrid(l);
  const KOp& op = L.dA.k;
  if (nu <= 0) return MGCMT_OK;  // (a V(0,nu2) cycle: nothing to launch — the chained lexicographic sweeps size their scratch by nu)
  if (fused_level(p, l, kind)) {
    MG_TRY(ensure_slot(p, l, MGCMT_SLOT_T));
    for (int left = nu; left > 0;) {
      const int n = pass_sweeps(p, l, kind, left);
      MG_TRY(fused_pass(p, l, kind, n, omega, 0, k, s));
      left -= n;
    }
    return post_launch();
  }
  switch (kind) {
    case MGCMT_WJACOBI: {
      MG_TRY(ensure_slot(p, l, MGCMT_SLOT_T));
      for (int it = 0; it < nu; ++it) {
        // a level whose kernels take two sweeps in one launch (the tile form of a nine-plane level): pairs, then the odd one
        if (it + 1 < nu && op.point &&
            launch_point_wjacobi_pair(s, g, op, p->kvec(l, MGCMT_SLOT_V), p->kvec(l, MGCMT_SLOT_F), p->kvec(l, MGCMT_SLOT_T), p->d_shifts, omega, k)) {
          std::swap(L.base[MGCMT_SLOT_V], L.base[MGCMT_SLOT_T]);
          ++it;
          continue;
        }
        launch_wjacobi(s, g, op, p->kvec(l, MGCMT_SLOT_V), p->kvec(l, MGCMT_SLOT_F), p->kvec(l, MGCMT_SLOT_T), p->d_shifts, omega, k);
        std::swap(L.base[MGCMT_SLOT_V], L.base[MGCMT_SLOT_T]);
      }
      break;
    }
    case MGCMT_GS_MC: {
      static const int order[4][2] = {{0, 1}, {1, 0}, {0, 0}, {1, 1}};
      if (op.point == kPointPlanes && nine_tiled(g, op)) MG_TRY(ensure_slot(p, l, MGCMT_SLOT_T));  // (the tile form is out of place)
      for (int it = 0; it < nu; ++it) {
        // a level whose kernels take the whole four-colour sweep in one launch, out of place (the tile form of a nine-plane level)
        if (op.point == kPointPlanes &&
            launch_point_mc_sweep(s, g, op, p->kvec(l, MGCMT_SLOT_V), p->kvec(l, MGCMT_SLOT_F), p->kvec(l, MGCMT_SLOT_T), p->d_shifts, omega, k)) {
          std::swap(L.base[MGCMT_SLOT_V], L.base[MGCMT_SLOT_T]);
          continue;
        }
        // a level with bonds on the marching kernels: the colours (0,1), (1,0) are one parity stage, (0,0), (1,1) the other
        if (launch_bonds_parity(s, g, op, p->kvec(l, MGCMT_SLOT_V), p->kvec(l, MGCMT_SLOT_F), p->d_shifts, omega, 1, k)) {
          launch_bonds_parity(s, g, op, p->kvec(l, MGCMT_SLOT_V), p->kvec(l, MGCMT_SLOT_F), p->d_shifts, omega, 0, k);
          continue;
        }
        for (int c = 0; c < 4; ++c)
          launch_mc_colour(s, g, op, p->kvec(l, MGCMT_SLOT_V), p->kvec(l, MGCMT_SLOT_F), p->d_shifts, omega, order[c][0], order[c][1], k);
      }
      break;
    }
    case MGCMT_GS_LEX:
    case MGCMT_SOR_LEX: {
      if (kind == MGCMT_GS_LEX || omega == 1.0) {
        MG_TRY(lex_sweep(p, l, MGCMT_SLOT_V, 0.0, 1.0, 1.0, 1.0, k, s, nu));  // (nu sweeps, chained in one launch where the wave pipeline covers the level)
      } else {
        // reference SOR (MGCMTSolver.py:229-246): v <- (D-wL)^-1((1-w)D + wU) v + w (D-L)^-1 f.
        // T <- (D-L)^-1 f once, then per sweep the homogeneous recurrence followed by v += w T.
        MG_TRY(ensure_slot(p, l, MGCMT_SLOT_T));
        for (int q = 0; q < k; ++q) launch_fill(s, p->kvec(l, MGCMT_SLOT_T, q).p, p->interior(l), 0.0);
        MG_TRY(lex_sweep(p, l, MGCMT_SLOT_T, 0.0, 1.0, 0.0, 1.0, k, s));
        // (beta = 0: the sweeps do not read their right-hand side — T rides in its place and is added as it is stored)
        MG_TRY(lex_sweep(p, l, MGCMT_SLOT_V, 1.0 - omega, 0.0, omega, omega, k, s, nu, omega, MGCMT_SLOT_T));
      }
      break;
    }
    default:
      return fail(MGCMT_ERR_INVALID, "unknown smoother kind");
  }
  return post_launch();
}

namespace {

// level l and the one below halve exactly, as the one-pass residual + restriction of a level with bonds or nine planes assumes
bool bonds_restrict_ok(const mgcmt_plan* p, int l) {
  const Level &F = p->levels[l], &C = p->levels[l + 1];
  return p->dim == 2 && (F.dA.k.point == kPointPlanes || F.dA.k.point == kPointBonds) && C.nr * 2 == F.nr && C.gc * 2 == F.gc;
}

// F[l+1] <- R (F[l] - (A - mu) V[l]) and, with clear_coarse, V[l+1] <- 0; the slots V, F, T of level l and V, F of level l + 1
// are in place.  One pass that stores no fine residual where the level has one — a 3-D level; a 2-D level with bonds or planes
// whose kernels take it — otherwise the residual into T and its restriction.
int residual_to_coarse(mgcmt_plan* p, int l, int k, bool clear_coarse, hipStream_t s) {
  const KVec v = p->kvec(l, MGCMT_SLOT_V), f = p->kvec(l, MGCMT_SLOT_F), fc = p->kvec(l + 1, MGCMT_SLOT_F);
  const KVec vc = clear_coarse ? p->kvec(l + 1, MGCMT_SLOT_V) : KVec{nullptr, 0};
  if (p->dim == 3) {
    launch3_residual_restrict(s, p->levels[l].dA.k3, v, f, fc, vc, p->d_shifts, k);
    return post_launch();
  }
  if (bonds_restrict_ok(p, l) && launch_point_residual_restrict(s, p->kgrid(l), p->levels[l].dA.k, v, f, fc, vc, p->d_shifts, k)) return post_launch();
  launch_residual(s, p->kgrid(l), p->levels[l].dA.k, v, f, p->kvec(l, MGCMT_SLOT_T), p->d_shifts, k);
  launch_restrict(s, p->kgrid(l), p->kgrid(l + 1), p->kvec(l, MGCMT_SLOT_T), fc, k);
  if (clear_coarse)
    for (int q = 0; q < k; ++q) launch_fill(s, p->kvec(l + 1, MGCMT_SLOT_V, q).p, p->interior(l + 1), 0.0);
  return post_launch();
}

int residual_restrict_impl(mgcmt_plan* p, int l, int k, hipStream_t s) {
  if (l + 1 >= (int)p->levels.size()) return fail(MGCMT_ERR_INVALID, "no coarser level");
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_V));
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_F));
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_T));
  MG_TRY(ensure_slot(p, l + 1, MGCMT_SLOT_V));
  MG_TRY(ensure_slot(p, l + 1, MGCMT_SLOT_F));
  return residual_to_coarse(p, l, k, true, s);
}

int prolong_correct_impl(mgcmt_plan* p, int l, int k, hipStream_t s) {
  if (l + 1 >= (int)p->levels.size()) return fail(MGCMT_ERR_INVALID, "no coarser level");
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_V));
  MG_TRY(ensure_slot(p, l + 1, MGCMT_SLOT_V));
  if (p->dim == 3) launch3_prolong(s, p->levels[l].gr, p->kvec(l + 1, MGCMT_SLOT_V), p->kvec(l, MGCMT_SLOT_V), 1, k);
  else launch_prolong(s, p->kgrid(l), p->kgrid(l + 1), p->kvec(l + 1, MGCMT_SLOT_V), p->kvec(l, MGCMT_SLOT_V), 1, k);
  return post_launch();
}

// The coarsest-level matrix (the per-point entries ride in the assembly) for the current shifts, factored and, where the
// explicit inverse is kept, inverted; nothing to do while the first k shifts are those of the last time and the per-point
// planes are the ones that were assembled (mgcmt_plan_set_point_diagonal counts its calls).  The band storage exists.
int factor_coarse(mgcmt_plan* p, int l, int k, hipStream_t s) {
  Level& L = p->levels[l];
  BandState& B = L.band;
  bool same = B.valid && B.k >= k && B.point_version == p->point_version;
  if (same)
    for (int q = 0; q < k; ++q) same = same && B.shifts[q] == p->h_shifts[q];
  if (same) return MGCMT_OK;
  if (p->dim == 3) launch3_band_assemble(s, L.dA.k3, p->d_shifts, B.b, k);
  else launch_band_assemble(s, p->kgrid(l), L.dA.k, p->d_shifts, B.b, k);
  launch_band_factor(s, B.b, k);
  if (B.inv) launch_band_invert(s, B.b, B.inv, (long)B.b.n * B.b.n, k);
  B.valid = true;
  B.k = k;
  B.point_version = p->point_version;
  B.shifts.assign(p->h_shifts.begin(), p->h_shifts.begin() + k);
  return post_launch();
}

// the factorisation (and, for at most 1024 unknowns, the explicit inverse) of the coarsest-level matrix for the current
// shifts: allocated on first use, redone when the shifts change
int ensure_coarse_ready(mgcmt_plan* p, int l, int k, hipStream_t s) {
  Level& L = p->levels[l];
  if (L.nr != L.gr) return fail(MGCMT_ERR_UNSUPPORTED, "direct solve on a row strip");
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_V));
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_F));
  BandState& B = L.band;
  const long n = (long)L.nr * L.gc;
  const int kl = p->dim == 3 ? (int)(L.gc + L.gr + 1) : L.nr == 1 ? 1 : (int)L.gc + 1;
  if (p->dim == 3 && kl > 273) return fail(MGCMT_ERR_UNSUPPORTED, "lowest_level too large for the direct solve (3-D: at most 16)");
  if (p->dim != 3 && kl > 129) return fail(MGCMT_ERR_UNSUPPORTED, "lowest_level too large for the direct solve (2-D: at most 128)");
  if (!B.b.ab) {
    B.b.n = n;
    B.b.kl = kl;
    B.b.width = 3 * kl + 1;
    B.b.ab_stride = n * B.b.width;
    B.b.piv_stride = n;
    const int cols = p->nvec < kMaxVec ? p->nvec : kMaxVec;  // (a solve batches at most kMaxVec columns: check_k)
    MG_HIP(hipMalloc((void**)&B.b.ab, sizeof(double) * B.b.ab_stride * cols));
    MG_HIP(hipMalloc((void**)&B.b.piv, sizeof(int) * B.b.piv_stride * cols));
    if (n <= 1024) MG_HIP(hipMalloc((void**)&B.inv, sizeof(double) * n * n * cols));
  }
  MG_TRY(factor_coarse(p, l, k, s));
  return post_launch();
}

int coarse_solve_impl(mgcmt_plan* p, int l, int k, hipStream_t s) {
  MG_TRY(ensure_coarse_ready(p, l, k, s));
  Level& L = p->levels[l];
  BandState& B = L.band;
  const long n = (long)L.nr * L.gc;
  if (B.inv) launch_dense_solve(s, n, B.inv, n * n, p->kvec(l, MGCMT_SLOT_F), p->kvec(l, MGCMT_SLOT_V), k);
  else launch_band_solve(s, B.b, p->kvec(l, MGCMT_SLOT_F), p->kvec(l, MGCMT_SLOT_V), k);
  return post_launch();
}

// pre-smoothing + residual + restriction (MGCMTSolver.py:313-316); one pass less on fused levels
// zero_in: V[l] is known to be zero (and has not been cleared); true below the level the cycle starts on
// recompute (may be null): out — how many of the pre-smoothing sweeps were NOT stored (the residual was restricted
// from them on the fly) and must be recomputed by up_leg from the untouched V; still_zero: V is still "zero, uncleared"
int down_leg(mgcmt_plan* p, int l, int kind, int nu, double omega, int k, bool zero_in, hipStream_t s, int* recompute = nullptr,
             bool* still_zero = nullptr, int nu_up = 0) {
  if (recompute) *recompute = 0;
  if (still_zero) *still_zero = false;
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_V));
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_F));
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_T));
  MG_TRY(ensure_slot(p, l + 1, MGCMT_SLOT_V));
  MG_TRY(ensure_slot(p, l + 1, MGCMT_SLOT_F));
  // a fused first pass takes "V is zero" as a flag; the one-launch-per-operation path needs V cleared
  if (zero_in && !(nu >= 1 && fused_level(p, l, kind)))
    for (int q = 0; q < k; ++q) launch_fill(s, p->kvec(l, MGCMT_SLOT_V, q).p, p->interior(l), 0.0);
  if (nu >= 1 && fused_level(p, l, kind)) {
    int left = nu, zi = zero_in ? 4 : 0;
    while (left > pass_sweeps(p, l, kind, left)) {
      const int n = pass_sweeps(p, l, kind, left);
      MG_TRY(fused_pass(p, l, kind, n, omega, zi, k, s));
      zi = 0;
      left -= n;
    }
    const int rmax = fused_max_recompute(p->levels[l].dA.k, kind == MGCMT_GS_MC ? 1 : 0, pass_sweeps(p, l, kind, nu_up));
    // worth it where the level is bandwidth-bound; on small levels the longer pipeline of the up-leg pass costs more
    // latency than the saved traffic is worth (measured: 1024^2 cycle 0.148 -> 0.179 ms with it)
    // (the same threshold serves the 9-point Galerkin levels: measured at 16384^2, recompute off on them costs 0.26 ms
    // per cycle, thresholds of 2^20 and 2^18 points are within noise of / slower than 2^22)
    const bool big = p->force_recompute || p->interior(l) >= (1L << 22);
    if (recompute && p->use_recompute && big && left <= rmax) {
      MG_TRY(fused_pass(p, l, kind, left, omega, 2 | 8 | zi, k, s));
      *recompute = left;
      if (still_zero) *still_zero = zi != 0;
    } else {
      MG_TRY(fused_pass(p, l, kind, left, omega, 2 | zi, k, s));
    }
    return post_launch();
  }
  MG_TRY(smooth_impl(p, l, kind, nu, omega, k, s));
  // (V[l+1] is cleared by the level below, which starts from "zero, uncleared")
  return residual_to_coarse(p, l, k, false, s);
}

// prolongation + correction + post-smoothing (MGCMTSolver.py:323-326)
int up_leg(mgcmt_plan* p, int l, int kind, int nu, double omega, int k, hipStream_t s, int recompute = 0, bool still_zero = false) {
  if (nu >= 1 && fused_level(p, l, kind)) {
    MG_TRY(ensure_slot(p, l, MGCMT_SLOT_V));
    MG_TRY(ensure_slot(p, l, MGCMT_SLOT_F));
    MG_TRY(ensure_slot(p, l, MGCMT_SLOT_T));
    MG_TRY(ensure_slot(p, l + 1, MGCMT_SLOT_V));
    int left = nu;
    const int first = pass_sweeps(p, l, kind, left);
    MG_TRY(fused_pass(p, l, kind, first, omega, 1 | (still_zero ? 4 : 0), k, s, recompute));
    left -= first;
    while (left > 0) {
      const int n = pass_sweeps(p, l, kind, left);
      MG_TRY(fused_pass(p, l, kind, n, omega, 0, k, s));
      left -= n;
    }
    return post_launch();
  }
  MG_TRY(prolong_correct_impl(p, l, k, s));
  return smooth_impl(p, l, kind, nu, omega, k, s);
}

// ---- two-level passes (fused2_kernel.h) ---------------------------------------------------------

// sweeps of the last down-leg pass of a fused level smoothed nu times (the passes before it take pass_sweeps each)
int last_pass_sweeps(const mgcmt_plan* p, int l, int kind, int nu) {
  int left = nu;
  while (left > pass_sweeps(p, l, kind, left)) left -= pass_sweeps(p, l, kind, left);
  return left;
}

// Level l and l+1 run as ONE down-leg and ONE up-leg launch: a constant 5-point level with weighted Jacobi, its
// nine_const Galerkin coarsening below, both whole (no strip), level l+1 above the tail / coarse solve, 2 sweeps per
// leg on level l+1, at least 2 post-sweeps on level l, and level l's last down pass a no-store (recompute) pass.  No
// Gram-Schmidt (level l+1's would run between the two up passes).  Otherwise the cycle runs today's passes.
bool two_level_ok(const mgcmt_plan* p, int l, int bottom, int kind, int nu, int nu_up, int nu_coarse, int gram_schmidt) {
  if (p->two_level == 0 || gram_schmidt || kind != MGCMT_WJACOBI || p->comm || p->dim != 2) return false;
  if (l + 1 >= bottom || nu < 1 || nu_up < 2 || nu_coarse != 2) return false;
  if (!fused_level(p, l, kind) || !fused_level(p, l + 1, kind)) return false;
  const Level &L0 = p->levels[l], &L1 = p->levels[l + 1], &L2 = p->levels[l + 2];
  if (!L0.dA.k.five_point || L0.dA.k.one_d || !L1.dA.k.nine_const || L0.dA.k.point || L1.dA.k.point) return false;
  for (const Level* L : {&L0, &L1, &L2})
    if (L->nr != L->gr || L->r0 != 0) return false;
  if (L1.gr * 2 != L0.gr || L1.gc * 2 != L0.gc || L2.gr * 2 != L1.gr || L2.gc * 2 != L1.gc) return false;
  const int nf = last_pass_sweeps(p, l, kind, nu);
  if (!p->use_recompute || nf > fused_max_recompute(L0.dA.k, 0, pass_sweeps(p, l, kind, nu_up))) return false;
  // 1: where the fine level is bandwidth-bound (the recompute threshold); 2: on every eligible level (tests)
  return p->two_level == 2 || p->interior(l) >= (1L << 22);
}

// carry (an up pass on a nonzero iterate only): the pass also leaves the next cycle's F[l+1] in T[l+1]
int two_level_launch(mgcmt_plan* p, int l, int up, int nf, bool zero_in, double omega, int k, hipStream_t s, bool carry = false) {
  const Level &L0 = p->levels[l], &L1 = p->levels[l + 1], &L2 = p->levels[l + 2];
  launch_fused2(s, up, nf, zero_in ? 1 : 0, L0.dA.k, L1.dA.k, L0.gr, L0.gc, L1.gr, L1.gc, L2.gc, p->kvec(l, MGCMT_SLOT_V),
                p->kvec(l, MGCMT_SLOT_F), p->kvec(l, MGCMT_SLOT_T), p->kvec(l + 1, MGCMT_SLOT_F),
                p->kvec(l + 2, up ? MGCMT_SLOT_V : MGCMT_SLOT_F), p->d_shifts, omega, k, p->fused_rows,
                carry ? p->kvec(l + 1, MGCMT_SLOT_T).p : nullptr);
  return post_launch();
}

// down legs of levels l and l+1: level l's passes but the last, then the two-level pass (F[l+1], F[l+2] written, V[l]
// and V[l+1] not).  nf: out — level l's sweeps the up pass recomputes; still_zero: out — V[l] is still "zero, uncleared"
int two_level_down(mgcmt_plan* p, int l, int kind, int nu, double omega, int k, bool zero_in, hipStream_t s, int* nf, bool* still_zero) {
  for (int m = l; m <= l + 2; ++m) {
    MG_TRY(ensure_slot(p, m, MGCMT_SLOT_V));
    MG_TRY(ensure_slot(p, m, MGCMT_SLOT_F));
    MG_TRY(ensure_slot(p, m, MGCMT_SLOT_T));
  }
  int left = nu, zi = zero_in ? 4 : 0;
  while (left > pass_sweeps(p, l, kind, left)) {
    const int n = pass_sweeps(p, l, kind, left);
    MG_TRY(fused_pass(p, l, kind, n, omega, zi, k, s));
    zi = 0;
    left -= n;
  }
  MG_TRY(two_level_launch(p, l, 0, left, zi != 0, omega, k, s));
  *nf = left;
  *still_zero = zi != 0;
  return MGCMT_OK;
}

// up legs of levels l+1 and l: the two-level pass (V[l] -> V', level l+1's correction and smoothing in registers),
// then level l's remaining post-smoothing passes
int two_level_up(mgcmt_plan* p, int l, int kind, int nu, double omega, int k, hipStream_t s, int nf, bool still_zero, bool carry = false) {
  MG_TRY(two_level_launch(p, l, 1, nf, still_zero, omega, k, s, carry));
  std::swap(p->levels[l].base[MGCMT_SLOT_V], p->levels[l].base[MGCMT_SLOT_T]);
  for (int left = nu - 2; left > 0;) {
    const int n = pass_sweeps(p, l, kind, left);
    MG_TRY(fused_pass(p, l, kind, n, omega, 0, k, s));
    left -= n;
  }
  return post_launch();
}

// The down legs of levels l and l+1 when T[l+1] holds the right-hand side that the last cycle's up pass carried: it
// becomes F[l+1] (the two roles swap, as V and T do behind a pass), the fine level has nothing left to do, and level
// l+1 runs its own down pass alone — nu_coarse = 2 sweeps from zero, not stored, residual, restriction to F[l+2] —, which
// is what the two-level down pass computes behind the fine stages.
int carried_down(mgcmt_plan* p, int l, int kind, double omega, int k, hipStream_t s) {
  for (int m = l; m <= l + 2; ++m) {
    MG_TRY(ensure_slot(p, m, MGCMT_SLOT_V));
    MG_TRY(ensure_slot(p, m, MGCMT_SLOT_F));
    MG_TRY(ensure_slot(p, m, MGCMT_SLOT_T));
  }
  std::swap(p->levels[l + 1].base[MGCMT_SLOT_F], p->levels[l + 1].base[MGCMT_SLOT_T]);
  MG_TRY(fused_pass(p, l + 1, kind, 2, omega, 2 | 4 | 8, k, s));
  return post_launch();
}

// ---- Gram-Schmidt -------------------------------------------------------------------------------

}  // namespace

int mgcmt::gramschmidt_impl(mgcmt_plan* p, int l, int slot, int k, int modified, hipStream_t s) {
  MG_TRY(ensure_slot(p, l, slot));
  const long n = p->interior(l);
  const long stride = p->levels[l].stride;
  double* a0 = p->kvec(l, slot, 0).p;
  double* sc = p->d_scalars;
  if (modified) {
    // MGCMTProcessor.py:44-50: q_i = a_i/|a_i|; a_j -= (<a_j,q_i>/<q_i,q_i>) q_i for j > i.
    // One launch per column (k_mgs_step): it projects column i out of all later ones, normalises it and leaves the
    // inner products the next column needs; the first set comes from one batched dot launch.
    if (mgs_small_fits(n)) {
      launch_mgs_small(s, n, a0, stride, k);  // short columns: everything in one workgroup
      return post_launch();
    }
    // Long columns: first the blocked form — Gram matrix, its factor, Q = A R^-1: 3 k vector streams instead of k^2 + k —
    // which leaves a gate word up where its rounding errors (cond^2 eps) would show; the column-by-column launches
    // behind it return at once when the gate is down (MGCMT_OPT_MGS_BLOCK = 0: column by column only)
    const double* gate = nullptr;
    // (on every level the one-workgroup kernel does not take — measured with the blocked form only from 2^20 points on: a
    // 1024^2 cycle of 10 columns 1.32 ms against 1.10, a 4096^2 cycle 6.21 against 6.26: the gated launches cost less than
    // the column steps of the middle levels)
    if (p->use_mgs_block && k >= 2 && k <= mgs_block_max() && n >= p->mgs_block_min) {
      launch_mgs_blocked(s, n, a0, stride, k, p->d_partials, p->d_mgs);
      gate = p->d_mgs + mgs_block_gate_word();
    }
    double* pa = p->d_partials;
    double* pb = p->d_partials + (long)(kMaxVec + 1) * 1024;
    launch_dot_partials(s, n, a0, a0, stride, k, pa, gate);  // <a_0, a_t>, t = 0..k-1
    for (int i = 0; i < k; ++i) {
      launch_mgs_step(s, n, pa, a0 + i * stride, stride, k - 1 - i, pb, 0, gate);
      std::swap(pa, pb);
    }
    (void)sc;
  } else {
    // MGCMTProcessor.py:34-42: u_j = a_j - sum_{i<j} (<a_j,u_i>/<u_i,u_i>) u_i with the ORIGINAL a_j in every
    // inner product, then all columns normalised
    for (int j = 1; j < k; ++j) {
      double* aj = a0 + j * stride;
      launch_dots(s, n, aj, a0, stride, j, p->d_partials, sc);                  // <a_j, u_i>, i < j
      for (int i = 0; i < j; ++i) launch_dots(s, n, a0 + i * stride, a0 + i * stride, 0, 1, p->d_partials + kMaxVec * 1024, sc + kMaxVec + i);
      for (int i = 0; i < j; ++i) launch_axpy_dev(s, n, sc + i, sc + kMaxVec + i, -1.0, a0 + i * stride, aj);
    }
    for (int i = 0; i < k; ++i) {
      double* ai = a0 + i * stride;
      launch_dots(s, n, ai, ai, 0, 1, p->d_partials, sc);
      launch_scale_dev(s, n, sc, 1, ai);
    }
  }
  return post_launch();
}

namespace {

// (re)factor the coarsest-level matrix when the shifts changed; no-op otherwise
int ensure_coarse_factor(mgcmt_plan* p, int l, int k, hipStream_t s) {
  if (!p->levels[l].band.b.ab) return MGCMT_OK;  // first use: coarse_solve_impl allocates and factors
  return factor_coarse(p, l, k, s);
}

// First level of the cycle's tail: the levels of at most 32 x 32 points below the level the cycle starts on run as
// ONE launch (kernels_tail.hip).  -1: no tail (1-D, strips, lexicographic smoothers, Gram-Schmidt between the levels,
// a coarsest grid too large for the explicit inverse, or nothing to gain).
int tail_level(const mgcmt_plan* p, int level, int kind, int nu_coarse, int gram_schmidt) {
  const int last = (int)p->levels.size() - 1;
  if (!p->use_tail || !p->use_fused || p->dim != 2 || gram_schmidt || nu_coarse < 1) return -1;
  if (p->has_point) return -1;  // the tail's kernels know Kronecker terms only: per-level launches down to the coarse solve
  if (kind != MGCMT_WJACOBI && kind != MGCMT_GS_MC) return -1;
  const Level& C = p->levels[last];
  if (C.nr != C.gr || (long)C.nr * C.gc > 1024) return -1;
  for (int l = level + 1; l < last; ++l) {
    const Level& L = p->levels[l];
    if (L.nr != L.gr || L.gr != L.gc) continue;
    if (tail_fits(L.gr, last - l + 1, L.dA.k.nterms)) return l;
  }
  return -1;
}

TailArgs tail_args(mgcmt_plan* p, int lt, int kind, int nu, double omega) {
  const int last = (int)p->levels.size() - 1;
  TailArgs a{};
  a.g0 = (int)p->levels[lt].gr;
  a.nlev = last - lt + 1;
  a.nterms = p->levels[lt].dA.k.nterms;
  for (int l = lt; l <= last; ++l) {
    const KOp& op = p->levels[l].dA.k;
    for (int m = 0; m < op.nterms; ++m) {
      a.X[l - lt][m] = op.X[m];
      a.Y[l - lt][m] = op.Y[m];
    }
    a.ldx[l - lt] = op.ldx;
    a.ldy[l - lt] = op.ldy;
  }
  a.f_in = p->kvec(lt, MGCMT_SLOT_F).p;
  a.v_out = p->kvec(lt, MGCMT_SLOT_V).p;
  a.vstride = p->kvec(lt, MGCMT_SLOT_V).stride;
  const long n = (long)p->levels[last].nr * p->levels[last].gc;
  a.inv = p->levels[last].band.inv;
  a.inv_stride = n * n;
  a.shifts = p->d_shifts;
  a.omega = omega;
  a.kind = kind;
  a.nu = nu;
  return a;
}

// The tail's matrix per vector for the current shifts (allocated on first use, redone when the shifts or the cycle's
// parameters change — like the coarsest level's factorisation, and like it never inside a graph capture: mgcmt_vcycle
// calls this eagerly before a capture or a replay).
int ensure_tail_matrix(mgcmt_plan* p, int lt, int kind, int nu, double omega, int k, hipStream_t s) {
  mgcmt_plan::TailMatrix& T = p->tailmat;
  const long n = (long)p->levels[lt].gr * p->levels[lt].gc;
  bool same = T.valid && T.lt == lt && T.kind == kind && T.nu == nu && T.omega == omega && T.k >= k && T.n == n;
  if (same)
    for (int q = 0; q < k; ++q) same = same && T.shifts[q] == p->h_shifts[q];
  if (same) return MGCMT_OK;
  const int last = (int)p->levels.size() - 1;
  MG_TRY(ensure_coarse_ready(p, last, k, s));
  if (T.capacity < k || T.n != n) {
    if (T.mt) {
      MG_HIP(hipStreamSynchronize(s));
      (void)hipFree(T.mt);
      T.mt = nullptr;
      p->graphs_invalidate();  // (cached graphs point at the old matrices)
    }
    MG_HIP(hipMalloc((void**)&T.mt, sizeof(double) * n * n * k));
    T.capacity = k;
  }
  const TailArgs a = tail_args(p, lt, kind, nu, omega);
  for (int q = 0; q < k; ++q) launch_tail_matrix(s, a, q, T.mt + (long)q * n * n);
  T.n = n;
  T.lt = lt;
  T.kind = kind;
  T.nu = nu;
  T.omega = omega;
  T.k = k;
  T.shifts.assign(p->h_shifts.begin(), p->h_shifts.begin() + k);
  T.valid = true;
  return post_launch();
}

bool tail_dense(const mgcmt_plan* p, int lt) { return p->use_tail_dense && lt > 0 && tail_dense_fits(p->levels[lt].gr); }

int run_tail(mgcmt_plan* p, int lt, int kind, int nu, double omega, int k, hipStream_t s) {
  const int last = (int)p->levels.size() - 1;
  MG_TRY(ensure_coarse_ready(p, last, k, s));
  MG_TRY(ensure_slot(p, lt, MGCMT_SLOT_V));
  MG_TRY(ensure_slot(p, lt, MGCMT_SLOT_F));
  if (tail_dense(p, lt)) {
    MG_TRY(ensure_tail_matrix(p, lt, kind, nu, omega, k, s));
    const long n = p->tailmat.n;
    launch_tail_dense(s, p->levels[lt].gr, p->tailmat.mt, n * n, p->kvec(lt, MGCMT_SLOT_F).p, p->kvec(lt, MGCMT_SLOT_V).p,
                      p->kvec(lt, MGCMT_SLOT_V).stride, k);
    return post_launch();
  }
  launch_tail(s, tail_args(p, lt, kind, nu, omega), k);
  return post_launch();
}

// what a cycle's tail needs ready outside a graph (the matrix of the dense form), for the cycle's parameters
int ensure_tail_for_cycle(mgcmt_plan* p, int level, int nu_coarse, int kind, double omega, int k, int cycle_flags, hipStream_t s) {
  const int lt = tail_level(p, level, kind, nu_coarse, cycle_flags & MGCMT_CYCLE_GRAM_SCHMIDT);
  if (lt > 0 && tail_dense(p, lt)) return ensure_tail_matrix(p, lt, kind, nu_coarse, omega, k, s);
  return MGCMT_OK;
}

// ---- 3-D levels (kernels_3d.hip) -----------------------------------------------------------------

int check_kind3(int kind) {
  if (kind == MGCMT_GS_LEX || kind == MGCMT_SOR_LEX)
    return fail(MGCMT_ERR_UNSUPPORTED, "lexicographic smoothers are not available on 3-D levels (MGCMT_WJACOBI and MGCMT_GS_MC are)");
  if (kind != MGCMT_WJACOBI && kind != MGCMT_GS_MC) return fail(MGCMT_ERR_INVALID, "unknown smoother kind");
  return MGCMT_OK;
}

int smooth3(mgcmt_plan* p, int l, int kind, int nu, double omega, int k, hipStream_t s) {
  Level& L = p->levels[l];
  MG_TRY(check_kind3(kind));
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_V));
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_F));
  if (kind == MGCMT_WJACOBI) {
    MG_TRY(ensure_slot(p, l, MGCMT_SLOT_T));
    for (int it = 0; it < nu; ++it) {
      launch3_wjacobi(s, L.dA.k3, p->kvec(l, MGCMT_SLOT_V), p->kvec(l, MGCMT_SLOT_F), p->kvec(l, MGCMT_SLOT_T), p->d_shifts, omega, k);
      std::swap(L.base[MGCMT_SLOT_V], L.base[MGCMT_SLOT_T]);
    }
  } else {
    for (int it = 0; it < nu; ++it) launch3_mc_sweep(s, L.dA.k3, p->kvec(l, MGCMT_SLOT_V), p->kvec(l, MGCMT_SLOT_F), p->d_shifts, omega, k);
  }
  return post_launch();
}

// prolongation + correction + post-smoothing; with weighted Jacobi the correction rides in the first sweep's pass
int up_leg3(mgcmt_plan* p, int l, int kind, int nu, double omega, int k, hipStream_t s) {
  if (kind == MGCMT_WJACOBI && nu >= 1) {
    Level& L = p->levels[l];
    MG_TRY(ensure_slot(p, l, MGCMT_SLOT_V));
    MG_TRY(ensure_slot(p, l, MGCMT_SLOT_F));
    MG_TRY(ensure_slot(p, l, MGCMT_SLOT_T));
    MG_TRY(ensure_slot(p, l + 1, MGCMT_SLOT_V));
    launch3_prolong_jacobi(s, L.dA.k3, p->kvec(l + 1, MGCMT_SLOT_V), p->kvec(l, MGCMT_SLOT_V), p->kvec(l, MGCMT_SLOT_F), p->kvec(l, MGCMT_SLOT_T),
                           p->d_shifts, omega, k);
    std::swap(L.base[MGCMT_SLOT_V], L.base[MGCMT_SLOT_T]);
    MG_TRY(post_launch());
    return smooth3(p, l, kind, nu - 1, omega, k, s);
  }
  MG_TRY(prolong_correct_impl(p, l, k, s));
  return smooth3(p, l, kind, nu, omega, k, s);
}

// the 3-D V-cycle: per level nu sweeps, one residual + restriction pass (the coarse iterate zero-started), the direct
// solve on the coarsest level, then prolongation + correction + sweeps (+ modified Gram-Schmidt of the k columns)
int vcycle3_body(mgcmt_plan* p, int level, int nu1, int nu2, int nu_coarse, int kind, double omega, int k, int cycle_flags, hipStream_t s) {
  MG_TRY(check_kind3(kind));
  const int last = (int)p->levels.size() - 1;
  if (cycle_flags & MGCMT_CYCLE_ZERO_START) {
    MG_TRY(ensure_slot(p, level, MGCMT_SLOT_V));
    for (int q = 0; q < k; ++q) launch_fill(s, p->kvec(level, MGCMT_SLOT_V, q).p, p->interior(level), 0.0);
  }
  for (int l = level; l < last; ++l) {
    MG_TRY(smooth3(p, l, kind, l == level ? nu1 : nu_coarse, omega, k, s));
    MG_TRY(residual_restrict_impl(p, l, k, s));
  }
  MG_TRY(coarse_solve_impl(p, last, k, s));
  for (int l = last - 1; l >= level; --l) {
    MG_TRY(up_leg3(p, l, kind, l == level ? nu2 : nu_coarse, omega, k, s));
    if (cycle_flags & MGCMT_CYCLE_GRAM_SCHMIDT) MG_TRY(gramschmidt_impl(p, l, MGCMT_SLOT_V, k, 1, s));
  }
  return MGCMT_OK;
}

// carry_mode: kCarryProduce — the cycle's last launch, the two-level up pass of `level`, carries the next cycle's
// F[level+1] (carry_eligible holds); kCarryConsume — the last cycle did, for these parameters
enum { kCarryProduce = 1, kCarryConsume = 2 };
int vcycle_body(mgcmt_plan* p, int level, int nu1, int nu2, int nu_coarse, int kind, double omega, int k, int cycle_flags,
                hipStream_t s, int carry_mode = 0) {
  if (p->dim == 3) return vcycle3_body(p, level, nu1, nu2, nu_coarse, kind, omega, k, cycle_flags, s);
  const int gram_schmidt = cycle_flags & MGCMT_CYCLE_GRAM_SCHMIDT;
  // MGCMT_CYCLE_ZERO_START: the caller vouches that the iterate on `level` is zero — the first pass takes that as a
  // flag (V is neither cleared nor read; where no fused pass runs, down_leg clears it)
  const bool zero_start = (cycle_flags & MGCMT_CYCLE_ZERO_START) != 0;
  const int last = (int)p->levels.size() - 1;
  const int lt = tail_level(p, level, kind, nu_coarse, gram_schmidt);
  const int bottom = lt > 0 ? lt : last;  // the levels level .. bottom-1 run as fused passes / single launches
  std::vector<int> recompute(last + 1, 0);
  std::vector<char> still_zero(last + 1, 0);
  std::vector<char> paired(last + 1, 0);  // level l and l + 1 run as two-level passes
  for (int l = level; l < bottom; ++l) {
    const int nu_up = l == level ? nu2 : nu_coarse;
    bool sz = false;
    if (l == level && (carry_mode & kCarryConsume)) {
      MG_TRY(carried_down(p, l, kind, omega, k, s));
      recompute[l] = nu1;  // what the skipped down pass would have left: nu1 sweeps to recompute, V not zero
      paired[l] = 1;
      ++l;
      continue;
    }
    if (two_level_ok(p, l, bottom, kind, l == level ? nu1 : nu_coarse, nu_up, nu_coarse, gram_schmidt)) {
      MG_TRY(two_level_down(p, l, kind, l == level ? nu1 : nu_coarse, omega, k, l > level || zero_start, s, &recompute[l], &sz));
      still_zero[l] = sz;
      paired[l] = 1;
      ++l;  // level l + 1's down leg ran inside that launch
      continue;
    }
    // the up-leg can only recompute the unstored sweeps if it runs a fused pass itself (>= 1 post-smoothing sweep)
    MG_TRY(down_leg(p, l, kind, l == level ? nu1 : nu_coarse, omega, k, l > level || zero_start, s, nu_up >= 1 ? &recompute[l] : nullptr, &sz, nu_up));
    still_zero[l] = sz;
  }
  if (lt > 0) MG_TRY(run_tail(p, lt, kind, nu_coarse, omega, k, s));
  else MG_TRY(coarse_solve_impl(p, last, k, s));
  for (int l = bottom - 1; l >= level; --l) {
    if (l > level && paired[l - 1]) continue;  // runs inside level l - 1's up pass
    if (paired[l]) {
      MG_TRY(two_level_up(p, l, kind, l == level ? nu2 : nu_coarse, omega, k, s, recompute[l], still_zero[l] != 0,
                          l == level && (carry_mode & kCarryProduce)));
      continue;
    }
    MG_TRY(up_leg(p, l, kind, l == level ? nu2 : nu_coarse, omega, k, s, recompute[l], still_zero[l] != 0));
    if (gram_schmidt) MG_TRY(gramschmidt_impl(p, l, MGCMT_SLOT_V, k, 1, s));
  }
  return MGCMT_OK;
}

// May a cycle with these parameters end in a carrying up pass (and the next one start from what it carried)?  The pair
// (level, level + 1) runs as two-level passes, the up pass is the cycle's last launch (nu2 == 2), the down leg is the
// single no-store launch (so the up pass recomputes nu1 <= 2 sweeps), no Gram-Schmidt, and the iterate is not flagged
// zero: a caller that does starts a new problem with every call, one that cycles on a nonzero iterate is iterating.
bool carry_eligible(const mgcmt_plan* p, int level, int nu1, int nu2, int nu_coarse, int kind, int cycle_flags) {
  if (p->carry_opt == 0 || p->carry.disabled || p->dim != 2 || cycle_flags != 0 || nu2 != 2 || nu1 < 1 || nu1 > 2) return false;
  const int last = (int)p->levels.size() - 1;
  const int lt = tail_level(p, level, kind, nu_coarse, 0);
  const int bottom = lt > 0 ? lt : last;
  if (level >= bottom || !two_level_ok(p, level, bottom, kind, nu1, nu2, nu_coarse, 0)) return false;
  if (last_pass_sweeps(p, level, kind, nu1) != nu1) return false;
  return p->carry_opt == 2 || p->interior(level) >= (1L << 22);
}

}  // namespace

int mgcmt::graph_run(mgcmt_plan* p, const std::string& params, const std::string& key, bool swaps_buffers, const std::function<int()>& prepare,
                     const std::function<int(hipStream_t)>& body, hipStream_t s) {
  auto hit = p->graphs.find(key);
  if (hit != p->graphs.end()) {
    if (prepare) MG_TRY(prepare());
    MG_HIP(hipGraphLaunch(hit->second.exec, s));
    // a replayed cycle runs the wave pipeline too: the next synchronising call must look at its error word
    if (hit->second.lex_wave) p->lex_wave_used = true;
    size_t i = 0;
    if (swaps_buffers)
      for (Level& L : p->levels) {
        L.base[MGCMT_SLOT_V] = hit->second.post_state[i++];
        L.base[MGCMT_SLOT_T] = hit->second.post_state[i++];
        L.base[MGCMT_SLOT_F] = hit->second.post_state[i++];
      }
    return MGCMT_OK;
  }
  // the first call with these parameters runs eagerly: it allocates, factors and queries occupancies
  if (p->cycle_seen[params]++ == 0) return body(s);
  if (prepare) MG_TRY(prepare());
  if ((!p->capture_stream && hipStreamCreate(&p->capture_stream) != hipSuccess) ||
      hipStreamBeginCapture(p->capture_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    if (swaps_buffers) p->use_graph = false;
    (void)hipGetLastError();
    return body(s);
  }
  const bool lex_before = p->lex_wave_used;
  p->lex_wave_used = false;
  const int rc = body(p->capture_stream);
  mgcmt_plan::CycleGraph cg;
  cg.lex_wave = p->lex_wave_used;  // the captured body launches a wave-pipeline sweep
  p->lex_wave_used = lex_before || cg.lex_wave;
  hipGraph_t graph = nullptr;
  const hipError_t end = hipStreamEndCapture(p->capture_stream, &graph);
  // Nothing was executed during the capture.  A body that advanced the plan's buffer roles cannot run again: graphs go
  // off and the call fails.  Any other body keeps no host-side state: it runs for real.
  auto lost = [&](const char* msg) {
    if (swaps_buffers) {
      p->use_graph = false;
      return fail(MGCMT_ERR_HIP, msg);
    }
    (void)hipGetLastError();
    return body(s);
  };
  if (rc != MGCMT_OK || end != hipSuccess || !graph) {
    if (graph) (void)hipGraphDestroy(graph);
    if (rc == MGCMT_OK) return lost("graph capture of the V-cycle failed");
    if (swaps_buffers) p->use_graph = false;
    else (void)hipGetLastError();
    return rc;
  }
  const hipError_t inst = hipGraphInstantiate(&cg.exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (inst != hipSuccess) return lost("hipGraphInstantiate failed");
  if (swaps_buffers)
    for (const Level& L : p->levels) {
      cg.post_state.push_back(L.base[MGCMT_SLOT_V]);
      cg.post_state.push_back(L.base[MGCMT_SLOT_T]);
      cg.post_state.push_back(L.base[MGCMT_SLOT_F]);
    }
  MG_HIP(hipGraphLaunch(cg.exec, s));
  p->graphs[key] = cg;
  return MGCMT_OK;
}

extern "C" {

int mgcmt_smooth(mgcmt_plan* p, int l, int kind, int nu, double omega, int k, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_level(p, l));
  MG_TRY(check_k(p, k));
  if (nu < 0) return fail(MGCMT_ERR_INVALID, "nu must be >= 0");
  return smooth_impl(p, l, kind, nu, omega, k, S(stream));
}

int mgcmt_residual_restrict(mgcmt_plan* p, int l, int k, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_level(p, l));
  MG_TRY(check_k(p, k));
  return residual_restrict_impl(p, l, k, S(stream));
}

int mgcmt_prolong_correct(mgcmt_plan* p, int l, int k, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_level(p, l));
  MG_TRY(check_k(p, k));
  return prolong_correct_impl(p, l, k, S(stream));
}

int mgcmt_coarse_solve(mgcmt_plan* p, int l, int k, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_level(p, l));
  MG_TRY(check_k(p, k));
  return coarse_solve_impl(p, l, k, S(stream));
}

int mgcmt_vcycle(mgcmt_plan* p, int level, int nu1, int nu2, int nu_coarse, int kind, double omega, int k, int cycle_flags,
                 void* stream) {
  // (no entry_drops_carry: this entry decides itself what becomes of a carried right-hand side)
  MG_TRY(check_level(p, level));
  MG_TRY(check_k(p, k));
  char buf[160];
  snprintf(buf, sizeof(buf), "%d/%d/%d/%d/%d/%.17g/%d/%d", level, nu1, nu2, nu_coarse, kind, omega, k, cycle_flags);
  const std::string params(buf);
  // The carry: used if the last cycle left one for exactly these parameters and nothing has touched the plan since
  // (any entry that could have dropped it), produced if this cycle may and the caller has not let two in a row go unused
  // — until a cycle again follows one of its own kind.
  mgcmt_plan::Carry& C = p->carry;
  const bool consume = C.valid && C.level == level && C.nu1 == nu1 && C.nu2 == nu2 && C.nu_coarse == nu_coarse && C.kind == kind &&
                       C.omega == omega && C.k == k && C.flags == cycle_flags &&
                       carry_eligible(p, level, nu1, nu2, nu_coarse, kind, cycle_flags);  // (still: nothing that changes it keeps a carry)
  const bool follows_its_kind = C.prev == params;
  p->carry_drop();
  if (consume || follows_its_kind) C.unused_drops = 0;
  if (nu1 < 0 || nu2 < 0 || nu_coarse < 0) return fail(MGCMT_ERR_INVALID, "sweep counts must be >= 0");
  if (cycle_flags & ~(MGCMT_CYCLE_GRAM_SCHMIDT | MGCMT_CYCLE_ZERO_START)) return fail(MGCMT_ERR_INVALID, "unknown cycle flag");
  MG_TRY(unsupported_point_smoother(p, kind));
  const bool produce = C.unused_drops < 2 && carry_eligible(p, level, nu1, nu2, nu_coarse, kind, cycle_flags);
  const int carry_mode = (produce ? kCarryProduce : 0) | (consume ? kCarryConsume : 0);
  hipStream_t s = S(stream);
  auto body = [&](hipStream_t on) { return vcycle_body(p, level, nu1, nu2, nu_coarse, kind, omega, k, cycle_flags, on, carry_mode); };
  auto done = [&](int rc) {
    if (rc != MGCMT_OK) return rc;
    C.prev = params;
    C.level = level, C.nu1 = nu1, C.nu2 = nu2, C.nu_coarse = nu_coarse, C.kind = kind, C.k = k, C.flags = cycle_flags;
    C.omega = omega;
    C.valid = produce;
    return rc;
  };
  if (!p->use_graph) return done(body(s));

  // HIP-graph replay: the launch sequence is fixed by the parameters, by what the cycle does about a carry and by which
  // buffer of every level currently is V, T and F (`params` stays free of the carry: the cycles of one run share the
  // eager first call)
  snprintf(buf, sizeof(buf), "/c%d", carry_mode);
  std::string key = params + buf;
  for (const Level& L : p->levels) {
    snprintf(buf, sizeof(buf), "|%p,%p,%p", (void*)L.base[MGCMT_SLOT_V], (void*)L.base[MGCMT_SLOT_T], (void*)L.base[MGCMT_SLOT_F]);
    key += buf;
  }
  // the coarsest-level factorisation (and the tail's matrix) depend on the shift VALUES and on the per-point planes; redo them
  // eagerly when either changed (factor_coarse compares the shifts and the plan's point_version)
  auto prepare = [&]() {
    MG_TRY(ensure_coarse_factor(p, (int)p->levels.size() - 1, k, s));
    return ensure_tail_for_cycle(p, level, nu_coarse, kind, omega, k, cycle_flags, s);
  };
  return done(graph_run(p, params, key, /*swaps_buffers=*/true, prepare, body, s));
}

int mgcmt_twogrid(mgcmt_plan* p, int level, int nu1, int nu2, int kind, double omega, int k, void* stream) {
  entry_drops_carry(p);
  MG_TRY(mgcmt::unsupported_3d(p, "mgcmt_twogrid"));
  MG_TRY(mgcmt::unsupported_point(p, "mgcmt_twogrid"));
  MG_TRY(check_level(p, level));
  MG_TRY(check_k(p, k));
  if (level + 1 >= (int)p->levels.size()) return fail(MGCMT_ERR_INVALID, "twogrid needs a coarser level");
  hipStream_t s = S(stream);
  int recompute = 0;
  MG_TRY(down_leg(p, level, kind, nu1, omega, k, false, s, nu2 >= 1 ? &recompute : nullptr, nullptr, nu2));
  MG_TRY(coarse_solve_impl(p, level + 1, k, s));
  MG_TRY(up_leg(p, level, kind, nu2, omega, k, s, recompute));
  return MGCMT_OK;
}

}  // extern "C"
