// Solve (A - mu I) x = f to a tolerance: conjugate gradients preconditioned by one V-cycle per iteration, queued on the
// stream without a host round trip.  Host code only; the passes and the scalar kernels are in kernels_pcg.hip, the
// preconditioner is mgcmt_vcycle (its own HIP-graph replay included) and the operator the level's apply kernel.
//
// Layout, fixed by what a cycle leaves alone (mgcmt_hip.h, mgcmt_vcycle): r lives in F[0] column 0 — the cycle's right-hand
// side, which it does not touch —, z is V[0] column 0, the cycle's result, and x, p, q are columns of slot W, which no cycle
// writes.  mu is the plan's shift 0, the one the cycle uses for column 0.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "plan_internal.h"

using namespace mgcmt;

namespace {

int pcg_plan_check(mgcmt_plan* p, const char* what) {
  if (!p) return fail(MGCMT_ERR_INVALID, "null plan");
  if (p->comm || p->levels[0].nr != p->levels[0].gr || p->levels[0].r0 != 0)
    return fail(MGCMT_ERR_UNSUPPORTED, std::string(what) + ": not available on a sharded plan (a row strip)");
  if (p->nvec < 4) return fail(MGCMT_ERR_INVALID, std::string(what) + ": the plan must store at least 4 vectors per slot (x, p, q, p2 in slot W)");
  return MGCMT_OK;
}

// q <- (A - mu I) src on level 0 with the shift of column 0, whatever column of W src is; k > 1: the k columns from src to
// the k columns from dst, column c with the shift of column c
void pcg_apply(mgcmt_plan* p, KVec src, KVec dst, hipStream_t s, int k = 1) {
  if (p->dim == 3) launch3_apply(s, p->levels[0].dA.k3, src, dst, p->d_shifts, k);
  else launch_apply(s, p->kgrid(0), p->levels[0].dA.k, src, dst, p->d_shifts, k);
}

// the marching direction pass (launch_pcg_march): the plan's option where it was set, else the environment variable
// MGCMT_PCG_MARCH (read per call: the tests compare both forms in one process), else kPcgMarchDefault — on: at 8192^2 an
// iteration with it measured 2.26 ms against 2.50 ms with the generic passes (medians of five alternating runs, profiles/r13_pcg.md)
constexpr int kPcgMarchDefault = 1;
bool pcg_march_selected(const mgcmt_plan* p) {
  if (p->pcg_march >= 0) return p->pcg_march != 0;
  const char* env = getenv("MGCMT_PCG_MARCH");
  if (env && env[0]) return env[0] != '0';
  return kPcgMarchDefault != 0;
}

}  // namespace

extern "C" {

int mgcmt_pcg_begin(mgcmt_plan* p, const int* vecs, double rtol, int flags, void* stream) {
  MG_TRY(pcg_plan_check(p, "mgcmt_pcg_begin"));
  if (!vecs) return fail(MGCMT_ERR_INVALID, "pcg_begin: null vector list");
  if (flags & ~(MGCMT_PCG_ZERO_START | MGCMT_PCG_FLEXIBLE)) return fail(MGCMT_ERR_INVALID, "pcg_begin: unknown flag");
  if (!(rtol >= 0.0) || !(rtol < 1.7e308)) return fail(MGCMT_ERR_INVALID, "pcg_begin: rtol must be a finite number >= 0");
  for (int a = 0; a < 4; ++a) {
    MG_TRY(check_vec(p, 0, MGCMT_SLOT_W, vecs[a]));
    for (int b = 0; b < a; ++b)
      if (vecs[a] == vecs[b]) return fail(MGCMT_ERR_INVALID, "pcg_begin: the four vectors (x, p, q, p2) must be distinct");
  }
  MG_TRY(ensure_slot(p, 0, MGCMT_SLOT_V));
  MG_TRY(ensure_slot(p, 0, MGCMT_SLOT_F));
  MG_TRY(ensure_slot(p, 0, MGCMT_SLOT_W));
  // (not cleared: the begin kernels write every state word and the whole history, each pass the partial sums its scalar kernel reads)
  if (!p->d_pcg) MG_HIP(hipMalloc((void**)&p->d_pcg, sizeof(double) * pcg_block_doubles()));
  hipStream_t s = S(stream);
  const long n = p->interior(0);
  const KVec x = p->kvec(0, MGCMT_SLOT_W, vecs[0]), q = p->kvec(0, MGCMT_SLOT_W, vecs[2]);
  double* r = p->kvec(0, MGCMT_SLOT_F, 0).p;
  const int flexible = (flags & MGCMT_PCG_FLEXIBLE) ? 1 : 0;
  if (flags & MGCMT_PCG_ZERO_START) {
    launch_pcg_begin(s, n, r, nullptr, x.p, pcg_cols_single(p->d_pcg), rtol, flexible);
  } else {
    pcg_apply(p, x, q, s);
    launch_pcg_begin(s, n, r, q.p, nullptr, pcg_cols_single(p->d_pcg), rtol, flexible);
  }
  MG_TRY(post_launch());
  for (int a = 0; a < 4; ++a) p->pcg_vecs[a] = vecs[a];
  p->pcgk = 0;  // (a batched solve on this plan is over: the two kinds share F, V and W)
  return MGCMT_OK;
}

int mgcmt_pcg_iterate(mgcmt_plan* p, int iterations, int nu1, int nu2, int nu_coarse, int kind, double omega, void* stream) {
  MG_TRY(pcg_plan_check(p, "mgcmt_pcg_iterate"));
  if (iterations < 0) return fail(MGCMT_ERR_INVALID, "pcg_iterate: negative iteration count");
  if (!p->d_pcg || p->pcg_vecs[0] < 0) return fail(MGCMT_ERR_INVALID, "pcg_iterate: no mgcmt_pcg_begin on this plan");
  hipStream_t s = S(stream);
  const long n = p->interior(0);
  const KVec x = p->kvec(0, MGCMT_SLOT_W, p->pcg_vecs[0]), q = p->kvec(0, MGCMT_SLOT_W, p->pcg_vecs[2]);
  double* r = p->kvec(0, MGCMT_SLOT_F, 0).p;
  const bool march = p->dim == 2 && pcg_march_selected(p);
  const PcgCols cols = pcg_cols_single(p->d_pcg);
  for (int it = 0; it < iterations; ++it) {
    // z = one cycle of r from a zero start; a smoother kind the plan's cycle refuses is the cycle's error
    MG_TRY(mgcmt_vcycle(p, 0, nu1, nu2, nu_coarse, kind, omega, 1, MGCMT_CYCLE_ZERO_START, stream));
    const double* z = p->kvec(0, MGCMT_SLOT_V, 0).p;  // (the cycle exchanges the roles of V and T: the address is the one after it)
    KVec pv = p->kvec(0, MGCMT_SLOT_W, p->pcg_vecs[1]);
    const KVec p2 = p->kvec(0, MGCMT_SLOT_W, p->pcg_vecs[3]);
    launch_pcg_dots(s, n, z, r, q.p, cols);
    if (march && launch_pcg_march(s, p->kgrid(0), p->levels[0].dA.k, z, pv.p, p2.p, q.p, p->d_shifts, cols)) {
      std::swap(p->pcg_vecs[1], p->pcg_vecs[3]);  // the new direction went to the spare vector: the two exchange their roles
      pv = p2;
    } else {
      launch_pcg_direction(s, n, z, pv.p, cols);
      pcg_apply(p, pv, q, s);
      launch_pcg_curvature(s, n, pv.p, q.p, cols);
    }
    launch_pcg_update(s, n, x.p, pv.p, r, q.p, cols);
    MG_TRY(post_launch());
  }
  return MGCMT_OK;
}

int mgcmt_pcg_status(mgcmt_plan* p, int* iterations_done, int* status, double* fnorm, double* history, int capacity, void* stream) {
  MG_TRY(pcg_plan_check(p, "mgcmt_pcg_status"));
  if (capacity < 0 || (capacity > 0 && !history)) return fail(MGCMT_ERR_INVALID, "pcg_status: bad history buffer");
  if (!p->d_pcg || p->pcg_vecs[0] < 0) return fail(MGCMT_ERR_INVALID, "pcg_status: no mgcmt_pcg_begin on this plan");
  if (capacity > MGCMT_RQ_HISTORY) capacity = MGCMT_RQ_HISTORY;
  // the history follows the state words in the plan's block: one copy, one synchronisation
  std::vector<double> host((size_t)kPcgStateWords + capacity);
  MG_HIP(hipMemcpyAsync(host.data(), p->d_pcg, sizeof(double) * host.size(), hipMemcpyDeviceToHost, S(stream)));
  MG_HIP(hipStreamSynchronize(S(stream)));
  MG_TRY(lex_wave_check(p));
  if (iterations_done) *iterations_done = (int)host[kPcgIter];
  if (status) *status = (int)host[kPcgStatus] | (host[kPcgIndefinite] != 0.0 ? MGCMT_PCG_INDEFINITE : 0);
  if (fnorm) *fnorm = host[kPcgFnorm];
  for (int i = 0; i < capacity; ++i) history[i] = host[(size_t)kPcgStateWords + i];
  return MGCMT_OK;
}

// ---- k systems at once: column c is (A - mu_c I) x_c = f_c, mu_c the plan's shift c ------------------------------------------
// The same iteration on k columns: one k-column cycle (zero start, no Gram-Schmidt: the columns are independent systems), then
// the passes with the column as a grid dimension.  r_c is F[0] column c, z_c is V[0] column c, and x, p, q, p2 are four ranges of
// k consecutive columns of slot W.  A column that has stopped is frozen by its own stop word; the cycle and the application
// know nothing of it and still run on all k columns (on scratch: z and q of a frozen column are never read again), so an
// iteration costs k columns until the last column stops.

int mgcmt_pcg_begin_k(mgcmt_plan* p, int k, const int* vecs, double rtol, int flags, void* stream) {
  MG_TRY(pcg_plan_check(p, "mgcmt_pcg_begin_k"));
  if (k < 1 || k > kPcgMaxColumns) return fail(MGCMT_ERR_INVALID, "pcg_begin_k: k must be in 1..16");
  if (!vecs) return fail(MGCMT_ERR_INVALID, "pcg_begin_k: null vector list");
  if (flags & ~(MGCMT_PCG_ZERO_START | MGCMT_PCG_FLEXIBLE)) return fail(MGCMT_ERR_INVALID, "pcg_begin_k: unknown flag");
  if (!(rtol >= 0.0) || !(rtol < 1.7e308)) return fail(MGCMT_ERR_INVALID, "pcg_begin_k: rtol must be a finite number >= 0");
  for (int a = 0; a < 4; ++a) {
    if (vecs[a] < 0 || (long)vecs[a] + k > p->nvec)
      return fail(MGCMT_ERR_INVALID, "pcg_begin_k: a range of k columns leaves the plan's vectors (x, p, q, p2 take 4 k columns of slot W)");
    for (int b = 0; b < a; ++b)
      if (std::abs(vecs[a] - vecs[b]) < k) return fail(MGCMT_ERR_INVALID, "pcg_begin_k: the four column ranges (x, p, q, p2) must not overlap");
  }
  MG_TRY(ensure_slot(p, 0, MGCMT_SLOT_V));
  MG_TRY(ensure_slot(p, 0, MGCMT_SLOT_F));
  MG_TRY(ensure_slot(p, 0, MGCMT_SLOT_W));
  hipStream_t s = S(stream);
  if (k > p->pcgk_cap) {  // (hipFree waits for the work that may still use the block)
    if (p->d_pcgk) MG_HIP(hipFree(p->d_pcgk));
    p->d_pcgk = nullptr;
    p->pcgk_cap = p->pcgk = 0;
    MG_HIP(hipMalloc((void**)&p->d_pcgk, sizeof(double) * pcg_block_k_doubles(k)));
    p->pcgk_cap = k;
  }
  // (otherwise not cleared, as the single block: the begin kernels write every state word and the whole history of the k columns)
  MG_HIP(hipMemsetAsync(p->d_pcgk, 0, sizeof(double) * kPcgHeadWords, s));  // no column has stopped
  const long n = p->interior(0);
  const KVec x = p->kvec(0, MGCMT_SLOT_W, vecs[0]), q = p->kvec(0, MGCMT_SLOT_W, vecs[2]);
  double* r = p->kvec(0, MGCMT_SLOT_F, 0).p;
  const PcgCols cols = pcg_cols_k(p->d_pcgk, p->pcgk_cap, k, x.stride);
  const int flexible = (flags & MGCMT_PCG_FLEXIBLE) ? 1 : 0;
  if (flags & MGCMT_PCG_ZERO_START) {
    launch_pcg_begin(s, n, r, nullptr, x.p, cols, rtol, flexible);
  } else {
    pcg_apply(p, x, q, s, k);
    launch_pcg_begin(s, n, r, q.p, nullptr, cols, rtol, flexible);
  }
  MG_TRY(post_launch());
  for (int a = 0; a < 4; ++a) p->pcgk_vecs[a] = vecs[a];
  p->pcgk = k;
  p->pcg_vecs[0] = -1;  // (a single solve on this plan is over: the two kinds share F, V and W)
  return MGCMT_OK;
}

int mgcmt_pcg_iterate_k(mgcmt_plan* p, int iterations, int nu1, int nu2, int nu_coarse, int kind, double omega, void* stream) {
  MG_TRY(pcg_plan_check(p, "mgcmt_pcg_iterate_k"));
  if (iterations < 0) return fail(MGCMT_ERR_INVALID, "pcg_iterate_k: negative iteration count");
  if (!p->d_pcgk || p->pcgk < 1) return fail(MGCMT_ERR_INVALID, "pcg_iterate_k: no mgcmt_pcg_begin_k on this plan");
  hipStream_t s = S(stream);
  const int k = p->pcgk;
  const long n = p->interior(0);
  const KVec x = p->kvec(0, MGCMT_SLOT_W, p->pcgk_vecs[0]), q = p->kvec(0, MGCMT_SLOT_W, p->pcgk_vecs[2]);
  double* r = p->kvec(0, MGCMT_SLOT_F, 0).p;
  const bool march = p->dim == 2 && pcg_march_selected(p);
  const PcgCols cols = pcg_cols_k(p->d_pcgk, p->pcgk_cap, k, x.stride);
  for (int it = 0; it < iterations; ++it) {
    MG_TRY(mgcmt_vcycle(p, 0, nu1, nu2, nu_coarse, kind, omega, k, MGCMT_CYCLE_ZERO_START, stream));
    const double* z = p->kvec(0, MGCMT_SLOT_V, 0).p;  // (the address after the cycle, as in mgcmt_pcg_iterate)
    KVec pv = p->kvec(0, MGCMT_SLOT_W, p->pcgk_vecs[1]);
    const KVec p2 = p->kvec(0, MGCMT_SLOT_W, p->pcgk_vecs[3]);
    launch_pcg_dots(s, n, z, r, q.p, cols);
    if (march && launch_pcg_march(s, p->kgrid(0), p->levels[0].dA.k, z, pv.p, p2.p, q.p, p->d_shifts, cols)) {
      // every column's new direction went to the spare range — a frozen column's did not, and is not read again —: the ranges
      // exchange their roles for all columns at once
      std::swap(p->pcgk_vecs[1], p->pcgk_vecs[3]);
      pv = p2;
    } else {
      launch_pcg_direction(s, n, z, pv.p, cols);
      pcg_apply(p, pv, q, s, k);
      launch_pcg_curvature(s, n, pv.p, q.p, cols);
    }
    launch_pcg_update(s, n, x.p, pv.p, r, q.p, cols);
    MG_TRY(post_launch());
  }
  return MGCMT_OK;
}

int mgcmt_pcg_status_k(mgcmt_plan* p, int* running, int* iterations_done, int* status, double* fnorm, double* history, int capacity, void* stream) {
  MG_TRY(pcg_plan_check(p, "mgcmt_pcg_status_k"));
  if (capacity < 0 || (capacity > 0 && !history)) return fail(MGCMT_ERR_INVALID, "pcg_status_k: bad history buffer");
  if (!p->d_pcgk || p->pcgk < 1) return fail(MGCMT_ERR_INVALID, "pcg_status_k: no mgcmt_pcg_begin_k on this plan");
  const int k = p->pcgk;
  const int keep = capacity > MGCMT_RQ_HISTORY ? MGCMT_RQ_HISTORY : capacity;
  // the head, the states and — when asked for — the histories of the k columns are contiguous: one copy, one synchronisation
  const size_t words = (size_t)kPcgHeadWords + (size_t)p->pcgk_cap * kPcgStateWords + (keep > 0 ? (size_t)k * MGCMT_RQ_HISTORY : 0);
  std::vector<double> host(words);
  MG_HIP(hipMemcpyAsync(host.data(), p->d_pcgk, sizeof(double) * words, hipMemcpyDeviceToHost, S(stream)));
  MG_HIP(hipStreamSynchronize(S(stream)));
  MG_TRY(lex_wave_check(p));
  unsigned stopped = 0;
  memcpy(&stopped, host.data(), sizeof(stopped));
  if (running) *running = k - (int)stopped;
  const double* st = host.data() + kPcgHeadWords;
  const double* hist = st + (size_t)p->pcgk_cap * kPcgStateWords;
  for (int c = 0; c < k; ++c, st += kPcgStateWords) {
    if (iterations_done) iterations_done[c] = (int)st[kPcgIter];
    if (status) status[c] = (int)st[kPcgStatus] | (st[kPcgIndefinite] != 0.0 ? MGCMT_PCG_INDEFINITE : 0);
    if (fnorm) fnorm[c] = st[kPcgFnorm];
    for (int i = 0; i < keep; ++i) history[(size_t)c * capacity + i] = hist[(size_t)c * MGCMT_RQ_HISTORY + i];
    for (int i = keep; i < capacity; ++i) history[(size_t)c * capacity + i] = 0.0;
  }
  return MGCMT_OK;
}

// Timing for scripts/bench_pcg.py: average milliseconds of `reps` launches of ONE pass of an iteration, with the scalar kernel
// that follows it, between two HIP events (one untimed launch first), on the vectors of the solve in progress
int mgcmt_pcg_time_pass(mgcmt_plan* p, int pass, int reps, double* ms_out, void* stream) {
  MG_TRY(pcg_plan_check(p, "mgcmt_pcg_time_pass"));
  if (!ms_out || reps < 1 || pass < 0 || pass > MGCMT_PCG_PASS_MARCH) return fail(MGCMT_ERR_INVALID, "pcg_time_pass: bad arguments");
  const bool batched = p->d_pcgk && p->pcgk > 0;  // the solve in progress: a batched one times the passes on its k columns
  if (!batched && (!p->d_pcg || p->pcg_vecs[0] < 0)) return fail(MGCMT_ERR_INVALID, "pcg_time_pass: no mgcmt_pcg_begin on this plan");
  hipStream_t s = S(stream);
  const long n = p->interior(0);
  const int* v = batched ? p->pcgk_vecs : p->pcg_vecs;
  const KVec x = p->kvec(0, MGCMT_SLOT_W, v[0]), pv = p->kvec(0, MGCMT_SLOT_W, v[1]), q = p->kvec(0, MGCMT_SLOT_W, v[2]);
  const KVec p2 = p->kvec(0, MGCMT_SLOT_W, v[3]);
  double* r = p->kvec(0, MGCMT_SLOT_F, 0).p;
  const double* z = p->kvec(0, MGCMT_SLOT_V, 0).p;
  const PcgCols cols = batched ? pcg_cols_k(p->d_pcgk, p->pcgk_cap, p->pcgk, x.stride) : pcg_cols_single(p->d_pcg);
  bool covered = true;
  auto once = [&]() {
    switch (pass) {
      case MGCMT_PCG_PASS_DOTS: launch_pcg_dots(s, n, z, r, q.p, cols); break;
      case MGCMT_PCG_PASS_DIRECTION: launch_pcg_direction(s, n, z, pv.p, cols); break;
      case MGCMT_PCG_PASS_CURVATURE: launch_pcg_curvature(s, n, pv.p, q.p, cols); break;
      case MGCMT_PCG_PASS_UPDATE: launch_pcg_update(s, n, x.p, pv.p, r, q.p, cols); break;
      default: covered = p->dim == 2 && launch_pcg_march(s, p->kgrid(0), p->levels[0].dA.k, z, pv.p, p2.p, q.p, p->d_shifts, cols);
    }
  };
  once();
  if (!covered) return fail(MGCMT_ERR_UNSUPPORTED, "pcg_time_pass: the marching direction pass does not cover level 0 of this plan");
  MG_TRY(post_launch());
  hipEvent_t a, b;
  MG_HIP(hipEventCreate(&a));
  MG_HIP(hipEventCreate(&b));
  MG_HIP(hipEventRecord(a, s));
  for (int i = 0; i < reps; ++i) once();
  MG_HIP(hipEventRecord(b, s));
  MG_HIP(hipEventSynchronize(b));
  float ms = 0.f;
  MG_HIP(hipEventElapsedTime(&ms, a, b));
  *ms_out = (double)ms / reps;
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return post_launch();
}

}  // extern "C"
