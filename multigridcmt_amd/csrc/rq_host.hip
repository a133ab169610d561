// The Rayleigh-quotient drivers: Ritz pair and residual of given vectors, rqmin (the device-resident minimisation),
// one line step along a caller's direction, and the Rayleigh-quotient multigrid cycle.  Host code only; the passes are in
// kernels_rq.hip (1-D / 2-D levels) and kernels_rq3d.hip (3-D levels).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "plan_internal.h"

using namespace mgcmt;

extern "C" {

int mgcmt_ritz_pair(mgcmt_plan* p, int l, int xs, int xv, int ws, int wv, int ss, int sv, double* out5, void* stream) {
  entry_drops_carry(p);
  MG_TRY(mgcmt::unsupported_3d(p, "mgcmt_ritz_pair"));
  MG_TRY(mgcmt::unsupported_point(p, "mgcmt_ritz_pair"));
  MG_TRY(check_vec(p, l, xs, xv));
  MG_TRY(check_vec(p, l, ws, wv));
  MG_TRY(check_vec(p, l, ss, sv));
  if (!out5) return fail(MGCMT_ERR_INVALID, "null output");
  if ((ss == xs && sv == xv) || (ss == ws && sv == wv)) return fail(MGCMT_ERR_INVALID, "ritz_pair: the scratch vector must differ from x and w");
  MG_TRY(ensure_slot(p, l, xs));
  MG_TRY(ensure_slot(p, l, ws));
  hipStream_t s = S(stream);
  const double* x = p->kvec(l, xs, xv).p;
  const double* w = p->kvec(l, ws, wv).p;
  if (launch_ritz_pair(s, p->kgrid(l), p->levels[l].dA.k, x, w, p->d_partials, p->d_scalars)) {
    MG_TRY(post_launch());
    MG_HIP(hipMemcpyAsync(out5, p->d_scalars, sizeof(double) * 5, hipMemcpyDeviceToHost, s));
    MG_HIP(hipStreamSynchronize(s));
    return MGCMT_OK;
  }
  MG_TRY(ensure_slot(p, l, ss));
  launch_apply(s, p->kgrid(l), p->levels[l].dA.k, p->kvec(l, ws, wv), p->kvec(l, ss, sv), p->d_zero, 1);
  const double* v[kGramMaxVectors] = {x, w, p->kvec(l, ss, sv).p};
  launch_gram(s, p->interior(l), v, 3, p->d_partials, p->d_scalars);
  MG_TRY(post_launch());
  constexpr int kPairs = kGramMaxVectors * (kGramMaxVectors + 1) / 2;
  double packed[kPairs];
  MG_HIP(hipMemcpyAsync(packed, p->d_scalars, sizeof(packed), hipMemcpyDeviceToHost, s));
  MG_HIP(hipStreamSynchronize(s));
  // packed order: (0,0),(0,1),...,(0,5),(1,1),(1,2),...
  out5[0] = packed[0];
  out5[1] = packed[1];
  out5[2] = packed[kGramMaxVectors];
  out5[3] = packed[2];
  out5[4] = packed[kGramMaxVectors + 1];
  return MGCMT_OK;
}

int mgcmt_rayleigh_residual(mgcmt_plan* p, int l, int slot, int k, double* rq_out, double* res_out, void* stream) {
  entry_drops_carry(p);
  MG_TRY(mgcmt::unsupported_3d(p, "mgcmt_rayleigh_residual"));
  MG_TRY(mgcmt::unsupported_point(p, "mgcmt_rayleigh_residual"));
  MG_TRY(check_vec(p, l, slot, 0));
  MG_TRY(check_k(p, k));
  if (slot == MGCMT_SLOT_W) return fail(MGCMT_ERR_INVALID, "rayleigh_residual uses slot W as its scratch");
  if (!rq_out && !res_out) return fail(MGCMT_ERR_INVALID, "null outputs");
  MG_TRY(ensure_slot(p, l, slot));
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_W));
  constexpr int kPairs = kGramMaxVectors * (kGramMaxVectors + 1) / 2;
  if (!p->d_rq) MG_HIP(hipMalloc((void**)&p->d_rq, sizeof(double) * kPairs * kMaxVec));
  hipStream_t s = S(stream);
  // W_q = (A - mu_q I) v_q for all columns in one launch, then per column <v,v>, <v,r>, <r,r> in one pass each; the
  // host sees all of them after ONE synchronisation
  launch_apply(s, p->kgrid(l), p->levels[l].dA.k, p->kvec(l, slot), p->kvec(l, MGCMT_SLOT_W), p->d_shifts, k);
  for (int q = 0; q < k; ++q) {
    const double* v[kGramMaxVectors] = {p->kvec(l, slot, q).p, p->kvec(l, MGCMT_SLOT_W, q).p};
    launch_gram(s, p->interior(l), v, 2, p->d_partials, p->d_rq + (long)q * kPairs);
  }
  MG_TRY(post_launch());
  std::vector<double> packed((size_t)kPairs * k);
  MG_HIP(hipMemcpyAsync(packed.data(), p->d_rq, sizeof(double) * kPairs * k, hipMemcpyDeviceToHost, s));
  MG_HIP(hipStreamSynchronize(s));
  for (int q = 0; q < k; ++q) {
    const double vv = packed[(size_t)q * kPairs + 0], vr = packed[(size_t)q * kPairs + 1], rr = packed[(size_t)q * kPairs + kGramMaxVectors];
    if (rq_out) rq_out[q] = p->h_shifts[q] + vr / vv;
    if (res_out) res_out[q] = std::sqrt(rr);
  }
  return MGCMT_OK;
}

// rqmin (MGCMTSolver.py:17-57) on `level`, entirely on the device: two passes over the data per step (kernels_rq.hip), the
// 2 x 2 pencil solved by one workgroup, no host round trip; the start vector is vecs[0] of `slot`, which also receives
// the result; vecs[1..5]: five more vectors of the slot as work space (x and p are ping-ponged; g; one for M g).
static int rqmin_check(mgcmt_plan* p, int l, int slot, const int* vecs, int nu) {
  MG_TRY(check_level(p, l));
  if (!vecs || nu < 0) return fail(MGCMT_ERR_INVALID, "rqmin: null vector list or negative step count");
  for (int a = 0; a < 6; ++a) {
    MG_TRY(check_vec(p, l, slot, vecs[a]));
    for (int b = 0; b < a; ++b)
      if (vecs[a] == vecs[b]) return fail(MGCMT_ERR_INVALID, "rqmin: the six vectors must be distinct");
  }
  MG_TRY(ensure_slot(p, l, slot));
  if (!p->d_rqstate) {
    MG_HIP(hipMalloc((void**)&p->d_rqstate, sizeof(double) * rq_state_words()));
    MG_HIP(hipMemset(p->d_rqstate, 0, sizeof(double) * rq_state_words()));
  }
  return MGCMT_OK;
}

// M: the plan's mass operator; none, or one whose factors are identities, is the identity (no application at all)
static bool mass_is_identity(const mgcmt_plan* p, int l) {
  if (!p->has_mass) return true;
  const Level& L = p->levels[l];
  auto is_identity = [](const Tri& t) {
    for (int64_t i = 0; i < t.n; ++i)
      if (t.di(i) != 1.0 || (i > 0 && t.lo(i) != 0.0) || (i + 1 < t.n && t.up(i) != 0.0)) return false;
    return true;
  };
  return L.hM.nterms == 1 && is_identity(L.hM.X[0]) && is_identity(L.hM.Y[0]) && (p->dim != 3 || is_identity(L.hM.Z[0]));
}

// One loop for every dimension.  3-D levels (kernels_rq3d.hip) take the same sequence of passes and scalar kernels with
// the same state words; there <g, M g> always is result 3 of pass 2's partial sums (with M != I pass 2 takes the flat form,
// whose grid the product's kernel shares)
static int rqmin_impl(mgcmt_plan* p, int l, int slot, const int* vecs, int nu, int robust, hipStream_t s) {
  const Level& L = p->levels[l];
  const int mid = mass_is_identity(p, l) ? 1 : 0;
  double* x = p->kvec(l, slot, vecs[0]).p;
  double* xalt = p->kvec(l, slot, vecs[1]).p;
  double* pv = p->kvec(l, slot, vecs[2]).p;
  double* palt = p->kvec(l, slot, vecs[3]).p;
  double* gv = p->kvec(l, slot, vecs[4]).p;
  double* tmp = p->kvec(l, slot, vecs[5]).p;
  double* st = p->d_rqstate;
  double* part = p->d_partials;
  double* part_dot = p->d_partials + 40000;  // (d_partials holds 67584 doubles: 8 x 4096 for the passes, 1024 for the dot)
  const long n = p->interior(l);
  double* x0 = x;
  // the launchers of the level's dimension
  const bool d3 = p->dim == 3;
  const KGrid g = p->kgrid(l);
  const KOp& A = L.dA.k;
  const KOp& Mo = p->has_mass ? L.dM.k : A;  // (not read when M is the identity)
  const K3Op& A3 = L.dA.k3;
  const K3Op& M3 = L.dM.k3;  // (3-D Rayleigh-quotient plans always carry M)
  auto small = [&]() {
    return d3 ? launch_rq3_small(s, A3, M3, mid, x, pv, gv, st, nu, robust) : launch_rq_small(s, g, A, Mo, mid, x, pv, gv, st, nu, robust);
  };
  auto pass1 = [&](int init) {
    if (d3) launch_rq3_pass1(s, A3, M3, mid, x, gv, pv, palt, st, init, robust, part);
    else launch_rq_pass1(s, g, A, Mo, mid, x, gv, pv, palt, st, init, robust, part);
  };
  auto pass2 = [&](int init) {
    return d3 ? launch_rq3_pass2(s, A3, M3, mid, x, pv, xalt, gv, st, init, part) : launch_rq_pass2(s, g, A, Mo, mid, x, pv, xalt, gv, st, init, part);
  };
  // <g, M g> as one more march over g (nothing stored) where the level takes the march
  auto gmg = [&](int nb) { return d3 ? launch_rq3_gmg(s, M3, gv, part, nb) : launch_rq_gmg(s, g, Mo, gv, part, nb); };
  // a level of a few thousand points: the whole call in one launch (MGCMT_RQ_SMALL=0: the passes, for A/B measurements)
  const char* small_env = getenv("MGCMT_RQ_SMALL");  // (read per call: the tests compare both forms in one process)
  const bool small_ok = !(small_env && small_env[0] == '0');
  if (small_ok && small()) return post_launch();
  for (int it = -1; it < nu; ++it) {
    const int init = it < 0 ? 1 : (it == 0 ? 2 : 0);
    pass1(init);
    if (init != 1) std::swap(pv, palt);
    const int nb = pass2(init);
    if (init != 1) std::swap(x, xalt);  // (the initial pair leaves x where it is)
    int mflag = mid;
    if (!mid) {
      if (gmg(nb)) {
        mflag = 2;
      } else if (d3) {
        return fail(MGCMT_ERR_INVALID, "rqmin: no <g, M g> form for this 3-D level");
      } else {  // 1-D / 2-D levels without the march: application + dot product
        launch_apply(s, g, Mo, KVec{gv, 0}, KVec{tmp, 0}, p->d_zero, 1);
        launch_dots(s, n, gv, tmp, 0, 1, part_dot, st + rq_word_gmg());
      }
    }
    launch_rq_scalars2(s, part, nb, st, mflag, init);
  }
  MG_TRY(post_launch());
  if (x != x0) MG_HIP(hipMemcpyAsync(x0, x, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
  return MGCMT_OK;
}

static int rq_result(mgcmt_plan* p, double* rho_out, hipStream_t s) {
  if (!rho_out) return MGCMT_OK;
  MG_HIP(hipMemcpyAsync(rho_out, p->d_rqstate + rq_word_rho(), sizeof(double), hipMemcpyDeviceToHost, s));
  MG_HIP(hipStreamSynchronize(s));
  return MGCMT_OK;
}

int mgcmt_rqmin(mgcmt_plan* p, int l, int slot, const int* vecs, int nu, int robust, double* rho_out, void* stream) {
  entry_drops_carry(p);
  MG_TRY(mgcmt::unsupported_3d_massless(p, "mgcmt_rqmin"));
  MG_TRY(mgcmt::unsupported_point(p, "mgcmt_rqmin"));
  MG_TRY(rqmin_check(p, l, slot, vecs, nu));
  MG_TRY(rqmin_impl(p, l, slot, vecs, nu, robust, S(stream)));
  return rq_result(p, rho_out, S(stream));
}

// One line minimisation of the Rayleigh quotient along a direction the CALLER supplies (see mgcmt_hip.h): the passes of
// rqmin with p = w read as it is and not stored, then x' = x + delta w and its gradient.
int mgcmt_rq_line_step(mgcmt_plan* p, int l, const int* xv, const int* wv, const int* xoutv, const int* gv, const int* tmpv, int robust, int record,
                       void* stream) {
  entry_drops_carry(p);
  MG_TRY(mgcmt::unsupported_3d_massless(p, "mgcmt_rq_line_step"));
  MG_TRY(mgcmt::unsupported_point(p, "mgcmt_rq_line_step"));
  MG_TRY(check_level(p, l));
  if (!xv || !gv) return fail(MGCMT_ERR_INVALID, "rq_line_step: x and g are required");
  if (wv && !xoutv) return fail(MGCMT_ERR_INVALID, "rq_line_step: a step needs a vector for x + delta w");
  const int* all[5] = {xv, wv, xoutv, gv, tmpv};
  for (int a = 0; a < 5; ++a) {
    if (!all[a]) continue;
    MG_TRY(check_vec(p, l, all[a][0], all[a][1]));
    MG_TRY(ensure_slot(p, l, all[a][0]));
    for (int b = 0; b < a; ++b)
      if (all[b] && all[a][0] == all[b][0] && all[a][1] == all[b][1]) return fail(MGCMT_ERR_INVALID, "rq_line_step: the vectors must be distinct");
  }
  if (record >= MGCMT_RQ_HISTORY) return fail(MGCMT_ERR_INVALID, "rq_line_step: history index out of range");
  if (!p->d_rqstate) {
    MG_HIP(hipMalloc((void**)&p->d_rqstate, sizeof(double) * rq_state_words()));
    MG_HIP(hipMemset(p->d_rqstate, 0, sizeof(double) * rq_state_words()));
  }
  if (record >= 0 && !p->d_rqhistory) MG_HIP(hipMalloc((void**)&p->d_rqhistory, sizeof(double) * MGCMT_RQ_HISTORY));
  hipStream_t s = S(stream);
  const Level& L = p->levels[l];
  const KOp& A = L.dA.k;
  const bool m_identity = mass_is_identity(p, l);
  if (!m_identity && !tmpv) return fail(MGCMT_ERR_INVALID, "rq_line_step: with a mass operator a work vector (for M g) is required");
  const KOp& Mo = p->has_mass ? L.dM.k : A;
  const KGrid g = p->kgrid(l);
  const double* x = p->kvec(l, xv[0], xv[1]).p;
  const double* w = wv ? p->kvec(l, wv[0], wv[1]).p : nullptr;
  double* xout = xoutv ? p->kvec(l, xoutv[0], xoutv[1]).p : nullptr;
  double* gout = p->kvec(l, gv[0], gv[1]).p;
  double* st = p->d_rqstate;
  double* part = p->d_partials;
  // without a direction: the initial pair of rqmin (rho and g of x); with one: pass 1 reads p = w (init 3), pass 2 is a step's
  const int init1 = w ? 3 : 1, init2 = w ? 0 : 1;
  if (p->dim == 3) {
    const K3Op& A3 = L.dA.k3;
    const K3Op& M3 = L.dM.k3;
    const int mid = m_identity ? 1 : 0;
    launch_rq3_pass1(s, A3, M3, mid, x, w, nullptr, nullptr, st, init1, robust, part);
    const int nb = launch_rq3_pass2(s, A3, M3, mid, x, w, xout, gout, st, init2, part);
    if (!m_identity && !launch_rq3_gmg(s, M3, gout, part, nb)) return fail(MGCMT_ERR_INVALID, "rq_line_step: no <g, M g> form for this 3-D level");
    launch_rq_scalars2(s, part, nb, st, m_identity ? 1 : 2, init2);
    MG_TRY(post_launch());
    if (record >= 0) MG_HIP(hipMemcpyAsync(p->d_rqhistory + record, st + rq_word_rho(), sizeof(double), hipMemcpyDeviceToDevice, s));
    return MGCMT_OK;
  }
  launch_rq_pass1(s, g, A, Mo, m_identity ? 1 : 0, x, w, nullptr, nullptr, st, init1, robust, part);
  const int nb = launch_rq_pass2(s, g, A, Mo, m_identity ? 1 : 0, x, w, xout, gout, st, init2, part);
  int mflag = m_identity ? 1 : 0;
  if (!m_identity) {
    if (launch_rq_gmg(s, g, Mo, gout, part, nb)) {
      mflag = 2;
    } else {
      double* tmp = p->kvec(l, tmpv[0], tmpv[1]).p;
      launch_apply(s, g, Mo, KVec{gout, 0}, KVec{tmp, 0}, p->d_zero, 1);
      launch_dots(s, p->interior(l), gout, tmp, 0, 1, p->d_partials + 40000, st + rq_word_gmg());
    }
  }
  launch_rq_scalars2(s, part, nb, st, mflag, init2);
  MG_TRY(post_launch());
  if (record >= 0) MG_HIP(hipMemcpyAsync(p->d_rqhistory + record, st + rq_word_rho(), sizeof(double), hipMemcpyDeviceToDevice, s));
  return MGCMT_OK;
}

int mgcmt_rq_history(mgcmt_plan* p, int first, int count, double* out, void* stream) {
  entry_drops_carry(p);
  MG_TRY(mgcmt::unsupported_3d_massless(p, "mgcmt_rq_history"));
  if (!p || !out || first < 0 || count < 0 || first + count > MGCMT_RQ_HISTORY) return fail(MGCMT_ERR_INVALID, "rq_history: bad range");
  if (count == 0) return MGCMT_OK;
  if (!p->d_rqhistory) return fail(MGCMT_ERR_INVALID, "rq_history: nothing recorded");
  MG_HIP(hipMemcpyAsync(out, p->d_rqhistory + first, sizeof(double) * count, hipMemcpyDeviceToHost, S(stream)));
  MG_HIP(hipStreamSynchronize(S(stream)));
  return MGCMT_OK;
}

// vcycle_rqmg (MGCMTSolver.py:99-122): rqmin, the ITERATE restricted (:113), the recursion on the Galerkin pair (R A P,
// R M P) of the next level, the interpolated coarse iterate added (:116-118), rqmin again — down to the plan's coarsest
// level, which only minimises.  One stream-ordered launch sequence without a host round trip, replayed as a HIP graph
// from its second call (the levels below 512^2 are pure launch latency: seven launches per step).
static int rqmg_body(mgcmt_plan* p, int l, int slot, const int* vecs, int nu1, int nu2, int robust, hipStream_t s) {
  const int last = (int)p->levels.size() - 1;
  MG_TRY(rqmin_impl(p, l, slot, vecs, nu1, robust, s));
  if (l == last) return MGCMT_OK;
  if (p->dim == 3) launch3_restrict(s, p->levels[l].dA.k3, p->kvec(l, slot, vecs[0]), p->kvec(l + 1, slot, vecs[0]), 1);
  else launch_restrict(s, p->kgrid(l), p->kgrid(l + 1), p->kvec(l, slot, vecs[0]), p->kvec(l + 1, slot, vecs[0]), 1);
  MG_TRY(rqmg_body(p, l + 1, slot, vecs, nu1, nu2, robust, s));
  if (p->dim == 3) launch3_prolong(s, p->levels[l].gr, p->kvec(l + 1, slot, vecs[0]), p->kvec(l, slot, vecs[0]), 1, 1);
  else launch_prolong(s, p->kgrid(l), p->kgrid(l + 1), p->kvec(l + 1, slot, vecs[0]), p->kvec(l, slot, vecs[0]), 1, 1);
  MG_TRY(post_launch());
  return rqmin_impl(p, l, slot, vecs, nu2, robust, s);
}

int mgcmt_vcycle_rqmg(mgcmt_plan* p, int slot, const int* vecs, int nu1, int nu2, int robust, double* rho_out, void* stream) {
  entry_drops_carry(p);
  MG_TRY(mgcmt::unsupported_3d_massless(p, "mgcmt_vcycle_rqmg"));
  MG_TRY(mgcmt::unsupported_point(p, "mgcmt_vcycle_rqmg"));
  if (!p) return fail(MGCMT_ERR_INVALID, "null plan");
  if (nu1 < 0 || nu2 < 0) return fail(MGCMT_ERR_INVALID, "step counts must be >= 0");
  for (int l = 0; l < (int)p->levels.size(); ++l) MG_TRY(rqmin_check(p, l, slot, vecs, nu1));
  hipStream_t s = S(stream);
  auto body = [&](hipStream_t on) { return rqmg_body(p, 0, slot, vecs, nu1, nu2, robust, on); };
  if (!p->use_graph) {
    MG_TRY(body(s));
    return rq_result(p, rho_out, s);
  }
  char buf[200];
  snprintf(buf, sizeof(buf), "rqmg/%d/%d/%d/%d/%d,%d,%d,%d,%d,%d", nu1, nu2, robust, slot, vecs[0], vecs[1], vecs[2], vecs[3], vecs[4], vecs[5]);
  const std::string params(buf);
  std::string key = params;
  for (const Level& L : p->levels) {
    snprintf(buf, sizeof(buf), "|%p", (void*)L.base[slot]);
    key += buf;
  }
  // the body swaps no buffers and keeps no host-side state: keyed on the base of `slot` alone, no post state, nothing to
  // prepare; a capture or instantiation that fails clears the HIP error and runs eagerly (use_graph stays as it is)
  MG_TRY(graph_run(p, params, key, /*swaps_buffers=*/false, nullptr, body, s));
  return rq_result(p, rho_out, s);
}

}  // extern "C"
