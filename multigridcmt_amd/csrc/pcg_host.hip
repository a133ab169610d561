// Solve (A - mu_c I) x_c = f_c for k columns to a tolerance: conjugate gradients preconditioned by one V-cycle per iteration,
// queued on the stream without a host round trip.  Host code only; the passes and the scalar kernels are in kernels_pcg.hip,
// the preconditioner is mgcmt_vcycle (its own HIP-graph replay included) and the operator the level's apply kernel.
//
// Layout, fixed by what a cycle leaves alone (mgcmt_hip.h, mgcmt_vcycle): r_c lives in F[0] column c — the cycle's right-hand
// side, which it does not touch —, z_c is V[0] column c, the cycle's result, and x, p, q, p2 are four ranges of k consecutive
// columns of slot W, which no cycle writes.  mu_c is the plan's shift c, the one the cycle uses for column c.
//
// One driver: begin, iterate, status and time_pass below work on k columns and on the plan's one block of device state.  The
// single entries (mgcmt_pcg_begin / _iterate / _status) are that driver with k = 1; the plan records which kind of entry began
// the solve in progress, and the other kind's iterate / status refuse it.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "plan_internal.h"

using namespace mgcmt;

namespace {

typedef mgcmt_plan::PcgKind PcgKind;

// the name, in front of every message, of the entry of `kind` that was called: base, or base_k
std::string pcg_who(const char* base, PcgKind kind) { return std::string(base) + (kind == mgcmt_plan::kPcgBatched ? "_k" : ""); }

int pcg_plan_check(mgcmt_plan* p, const std::string& who) {
  if (!p) return fail(MGCMT_ERR_INVALID, "null plan");
  if (p->comm || p->levels[0].nr != p->levels[0].gr || p->levels[0].r0 != 0)
    return fail(MGCMT_ERR_UNSUPPORTED, "mgcmt_" + who + ": not available on a sharded plan (a row strip)");
  if (p->nvec < 4) return fail(MGCMT_ERR_INVALID, "mgcmt_" + who + ": the plan must store at least 4 vectors per slot (x, p, q, p2 in slot W)");
  return MGCMT_OK;
}

// the columns of the solve in progress, as the kernels take them
PcgCols pcg_cols_of(const mgcmt_plan* p) { return pcg_cols(p->d_pcg_block, p->pcg_cap, p->pcg_k, p->kvec(0, MGCMT_SLOT_W, p->pcg_w[0]).stride); }

// the k columns from dst <- (A - mu_c I) the k columns from src on level 0, column c with the shift of column c
void pcg_apply(mgcmt_plan* p, KVec src, KVec dst, hipStream_t s, int k) {
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

// vecs: the first columns of the four ranges of k columns of slot W.  k = 1: any four distinct columns, in any order
int pcg_begin(mgcmt_plan* p, PcgKind kind, int k, const int* vecs, double rtol, int flags, void* stream) {
  const std::string w = pcg_who("pcg_begin", kind);
  MG_TRY(pcg_plan_check(p, w));
  if (k < 1 || k > kPcgMaxColumns) return fail(MGCMT_ERR_INVALID, w + ": k must be in 1..16");
  if (!vecs) return fail(MGCMT_ERR_INVALID, w + ": null vector list");
  if (flags & ~(MGCMT_PCG_ZERO_START | MGCMT_PCG_FLEXIBLE)) return fail(MGCMT_ERR_INVALID, w + ": unknown flag");
  if (!(rtol >= 0.0) || !(rtol < 1.7e308)) return fail(MGCMT_ERR_INVALID, w + ": rtol must be a finite number >= 0");
  for (int a = 0; a < 4; ++a) {
    if (vecs[a] < 0 || (long)vecs[a] + k > p->nvec)
      return fail(MGCMT_ERR_INVALID, w + ": a range of k columns leaves the plan's vectors (x, p, q, p2 take 4 k columns of slot W)");
    for (int b = 0; b < a; ++b)
      if (std::abs(vecs[a] - vecs[b]) < k) return fail(MGCMT_ERR_INVALID, w + ": the four column ranges (x, p, q, p2) must not overlap");
  }
  MG_TRY(ensure_slot(p, 0, MGCMT_SLOT_V));
  MG_TRY(ensure_slot(p, 0, MGCMT_SLOT_F));
  MG_TRY(ensure_slot(p, 0, MGCMT_SLOT_W));
  hipStream_t s = S(stream);
  if (k > p->pcg_cap) {  // (hipFree waits for the work that may still use the block)
    if (p->d_pcg_block) MG_HIP(hipFree(p->d_pcg_block));
    p->d_pcg_block = nullptr;
    p->pcg_cap = 0;
    p->pcg_kind = mgcmt_plan::kPcgNone;
    MG_HIP(hipMalloc((void**)&p->d_pcg_block, sizeof(double) * pcg_block_doubles(k)));
    p->pcg_cap = k;
  }
  // (otherwise not cleared: the begin kernels write every state word and the whole history of the k columns, each pass the
  // partial sums its scalar kernel reads)
  MG_HIP(hipMemsetAsync(p->d_pcg_block, 0, sizeof(double) * kPcgHeadWords, s));  // no column has stopped
  const long n = p->interior(0);
  const KVec x = p->kvec(0, MGCMT_SLOT_W, vecs[0]), q = p->kvec(0, MGCMT_SLOT_W, vecs[2]);
  double* r = p->kvec(0, MGCMT_SLOT_F, 0).p;
  const PcgCols cols = pcg_cols(p->d_pcg_block, p->pcg_cap, k, x.stride);
  const int flexible = (flags & MGCMT_PCG_FLEXIBLE) ? 1 : 0;
  if (flags & MGCMT_PCG_ZERO_START) {
    launch_pcg_begin(s, n, r, nullptr, x.p, cols, rtol, flexible);
  } else {
    pcg_apply(p, x, q, s, k);
    launch_pcg_begin(s, n, r, q.p, nullptr, cols, rtol, flexible);
  }
  MG_TRY(post_launch());
  for (int a = 0; a < 4; ++a) p->pcg_w[a] = vecs[a];
  p->pcg_k = k;
  p->pcg_kind = kind;  // (a solve of the other kind on this plan is over: the two share F, V, W and the block)
  return MGCMT_OK;
}

// One iteration: one k-column cycle (zero start, no Gram-Schmidt: the columns are independent systems), then the passes with
// the column as a grid dimension.  A column that has stopped is frozen by its own stop word; the cycle and the application
// know nothing of it and still run on all k columns (on scratch: z and q of a frozen column are never read again), so an
// iteration costs k columns until the last column stops.
int pcg_iterate(mgcmt_plan* p, PcgKind kind, int iterations, int nu1, int nu2, int nu_coarse, int smoother, double omega, void* stream) {
  const std::string w = pcg_who("pcg_iterate", kind);
  MG_TRY(pcg_plan_check(p, w));
  if (iterations < 0) return fail(MGCMT_ERR_INVALID, w + ": negative iteration count");
  if (p->pcg_kind != kind) return fail(MGCMT_ERR_INVALID, w + ": no mgcmt_" + pcg_who("pcg_begin", kind) + " on this plan");
  hipStream_t s = S(stream);
  const int k = p->pcg_k;
  const long n = p->interior(0);
  const KVec x = p->kvec(0, MGCMT_SLOT_W, p->pcg_w[0]), q = p->kvec(0, MGCMT_SLOT_W, p->pcg_w[2]);
  double* r = p->kvec(0, MGCMT_SLOT_F, 0).p;
  const bool march = p->dim == 2 && pcg_march_selected(p);
  const PcgCols cols = pcg_cols_of(p);
  for (int it = 0; it < iterations; ++it) {
    // z = one cycle of r from a zero start; a smoother kind the plan's cycle refuses is the cycle's error
    MG_TRY(mgcmt_vcycle(p, 0, nu1, nu2, nu_coarse, smoother, omega, k, MGCMT_CYCLE_ZERO_START, stream));
    const double* z = p->kvec(0, MGCMT_SLOT_V, 0).p;  // (the cycle exchanges the roles of V and T: the address is the one after it)
    KVec pv = p->kvec(0, MGCMT_SLOT_W, p->pcg_w[1]);
    const KVec p2 = p->kvec(0, MGCMT_SLOT_W, p->pcg_w[3]);
    launch_pcg_dots(s, n, z, r, q.p, cols);
    if (march && launch_pcg_march(s, p->kgrid(0), p->levels[0].dA.k, z, pv.p, p2.p, q.p, p->d_shifts, cols)) {
      // every column's new direction went to the spare range — a frozen column's did not, and is not read again —: the ranges
      // exchange their roles for all columns at once
      std::swap(p->pcg_w[1], p->pcg_w[3]);
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

// The outputs are per column (any may be null); history: k rows of `capacity` numbers.  The head, the states and — when asked
// for — the histories of the k columns are contiguous: one copy, one synchronisation; without a history the copy ends behind
// the k states.
int pcg_status(mgcmt_plan* p, PcgKind kind, int* running, int* iterations_done, int* status, double* fnorm, double* history, int capacity, void* stream) {
  const std::string w = pcg_who("pcg_status", kind);
  MG_TRY(pcg_plan_check(p, w));
  if (capacity < 0 || (capacity > 0 && !history)) return fail(MGCMT_ERR_INVALID, w + ": bad history buffer");
  if (p->pcg_kind != kind) return fail(MGCMT_ERR_INVALID, w + ": no mgcmt_" + pcg_who("pcg_begin", kind) + " on this plan");
  const int k = p->pcg_k;
  const int keep = capacity > MGCMT_RQ_HISTORY ? MGCMT_RQ_HISTORY : capacity;
  const size_t words = (size_t)kPcgHeadWords + (keep > 0 ? (size_t)p->pcg_cap * kPcgStateWords + (size_t)k * MGCMT_RQ_HISTORY : (size_t)k * kPcgStateWords);
  std::vector<double> host(words);
  MG_HIP(hipMemcpyAsync(host.data(), p->d_pcg_block, sizeof(double) * words, hipMemcpyDeviceToHost, S(stream)));
  MG_HIP(hipStreamSynchronize(S(stream)));
  MG_TRY(lex_wave_check(p));
  unsigned stopped = 0;
  memcpy(&stopped, host.data(), sizeof(stopped));
  if (running) *running = k - (int)stopped;
  const double* st = host.data() + kPcgHeadWords;
  const double* hist = st + (size_t)p->pcg_cap * kPcgStateWords;
  for (int c = 0; c < k; ++c, st += kPcgStateWords) {
    if (iterations_done) iterations_done[c] = (int)st[kPcgIter];
    if (status) status[c] = (int)st[kPcgStatus] | (st[kPcgIndefinite] != 0.0 ? MGCMT_PCG_INDEFINITE : 0);
    if (fnorm) fnorm[c] = st[kPcgFnorm];
    for (int i = 0; i < keep; ++i) history[(size_t)c * capacity + i] = hist[(size_t)c * MGCMT_RQ_HISTORY + i];
    for (int i = keep; i < capacity; ++i) history[(size_t)c * capacity + i] = 0.0;
  }
  return MGCMT_OK;
}

}  // namespace

extern "C" {

// The six entries: argument handling around the driver.  The single ones pass k = 1 and take column 0 into their scalar outputs
int mgcmt_pcg_begin(mgcmt_plan* p, const int* vecs, double rtol, int flags, void* stream) {
  entry_drops_carry(p);
  return pcg_begin(p, mgcmt_plan::kPcgSingle, 1, vecs, rtol, flags, stream);
}
int mgcmt_pcg_begin_k(mgcmt_plan* p, int k, const int* vecs, double rtol, int flags, void* stream) {
  entry_drops_carry(p);
  return pcg_begin(p, mgcmt_plan::kPcgBatched, k, vecs, rtol, flags, stream);
}
int mgcmt_pcg_iterate(mgcmt_plan* p, int iterations, int nu1, int nu2, int nu_coarse, int kind, double omega, void* stream) {
  entry_drops_carry(p);
  return pcg_iterate(p, mgcmt_plan::kPcgSingle, iterations, nu1, nu2, nu_coarse, kind, omega, stream);
}
int mgcmt_pcg_iterate_k(mgcmt_plan* p, int iterations, int nu1, int nu2, int nu_coarse, int kind, double omega, void* stream) {
  entry_drops_carry(p);
  return pcg_iterate(p, mgcmt_plan::kPcgBatched, iterations, nu1, nu2, nu_coarse, kind, omega, stream);
}
int mgcmt_pcg_status(mgcmt_plan* p, int* iterations_done, int* status, double* fnorm, double* history, int capacity, void* stream) {
  entry_drops_carry(p);
  if (capacity > MGCMT_RQ_HISTORY) capacity = MGCMT_RQ_HISTORY;  // (one row: what lies behind the history stays the caller's, not cleared)
  return pcg_status(p, mgcmt_plan::kPcgSingle, nullptr, iterations_done, status, fnorm, history, capacity, stream);
}
int mgcmt_pcg_status_k(mgcmt_plan* p, int* running, int* iterations_done, int* status, double* fnorm, double* history, int capacity, void* stream) {
  entry_drops_carry(p);
  return pcg_status(p, mgcmt_plan::kPcgBatched, running, iterations_done, status, fnorm, history, capacity, stream);
}

// Timing for scripts/bench_pcg.py: average milliseconds of `reps` launches of ONE pass of an iteration, with the scalar kernel
// that follows it, between two HIP events (one untimed launch first), on the vectors and the columns of the solve in progress
int mgcmt_pcg_time_pass(mgcmt_plan* p, int pass, int reps, double* ms_out, void* stream) {
  entry_drops_carry(p);
  MG_TRY(pcg_plan_check(p, "pcg_time_pass"));
  if (!ms_out || reps < 1 || pass < 0 || pass > MGCMT_PCG_PASS_MARCH) return fail(MGCMT_ERR_INVALID, "pcg_time_pass: bad arguments");
  if (p->pcg_kind == mgcmt_plan::kPcgNone) return fail(MGCMT_ERR_INVALID, "pcg_time_pass: no mgcmt_pcg_begin on this plan");
  hipStream_t s = S(stream);
  const long n = p->interior(0);
  const int* v = p->pcg_w;
  const KVec x = p->kvec(0, MGCMT_SLOT_W, v[0]), pv = p->kvec(0, MGCMT_SLOT_W, v[1]), q = p->kvec(0, MGCMT_SLOT_W, v[2]);
  const KVec p2 = p->kvec(0, MGCMT_SLOT_W, v[3]);
  double* r = p->kvec(0, MGCMT_SLOT_F, 0).p;
  const double* z = p->kvec(0, MGCMT_SLOT_V, 0).p;
  const PcgCols cols = pcg_cols_of(p);
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
