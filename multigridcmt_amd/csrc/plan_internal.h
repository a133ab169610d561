// Host-side types of libmgcmt_hip.so and what its host files share: hierarchy.hip (Galerkin hierarchy, plan creation),
// cycle.hip (single-GPU cycle, HIP-graph cache), rq_host.hip (Rayleigh-quotient drivers), pcg_host.hip (the solve to a
// tolerance), plan.hip (checks, vector
// storage, the rest of the C-ABI) and sharded.hip (communicator, sharded cycle).  Not part of the ABI.
#pragma once
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "mgcmt_internal.h"

namespace mgcmt {

// tridiagonal factor on the host: lo, di, up concatenated, length 3n
struct Tri {
  int64_t n = 0;
  std::vector<double> a;
  double lo(int64_t i) const { return a[i]; }
  double di(int64_t i) const { return a[n + i]; }
  double up(int64_t i) const { return a[2 * n + i]; }
  double at(int64_t r, int64_t c) const {
    if (c == r - 1) return lo(r);
    if (c == r) return di(r);
    if (c == r + 1) return up(r);
    return 0.0;
  }
};

struct HostOp {
  int nterms = 0;
  std::vector<Tri> X, Y;  // per term
  std::vector<Tri> Z;     // 3-D levels: X over z, Y over y, Z over x
};

struct DevOp {
  KOp k{};
  K3Op k3{};  // 3-D levels
  std::vector<double*> owned;
};

struct BandState {
  KBand b{};
  double* inv = nullptr;  // explicit inverse per vector when the coarsest level has at most 1024 unknowns
  bool valid = false;
  int k = 0;
  std::vector<double> shifts;
  unsigned long point_version = 0;  // mgcmt_plan::point_version of the planes that were assembled
};

struct Level {
  int64_t gr = 1, gc = 1;  // global rows / cols
  int64_t r0 = 0, nr = 1;  // local strip
  int64_t stride = 0;      // elements between vectors (halo rows included)
  int halo = kHalo;        // halo rows above and below every vector: kHalo on 2-D levels, 1 on 1-D levels (a "row" is the whole vector)
  double* base[4] = {nullptr, nullptr, nullptr, nullptr};  // allocation start per slot
  HostOp hA, hM;
  DevOp dA, dM;
  BandState band;
  KGrid grid() const { return KGrid{(long)nr, (long)gc, 0}; }
};

struct ShardComm;  // sharded.hip

}  // namespace mgcmt

struct mgcmt_plan {
  int dim = 1;  // 3: a 3-D plan (mgcmt_plan_create3d): level l is (g >> l)^3 points as g >> l z-planes (nr = gr) of (g >> l)^2
                // points (gc), one zero halo plane above and below every vector
  int nvec = 1;
  int device = 0;
  int64_t g = 0, lowest = 0;
  std::vector<mgcmt::Level> levels;
  double* d_shifts = nullptr;   // [kMaxVec] current shifts
  double* d_zero = nullptr;     // [kMaxVec] zeros (apply without shift)
  double* d_partials = nullptr; // reduction scratch
  double* d_scalars = nullptr;  // [4*kMaxVec] reduction results
  // wide block operations (kernels_blockwide.hip), allocated on first use: per-workgroup partial tiles of the pencil, its
  // summed tiles, and the coefficient / pointer table of the wide combine
  double* d_wide_partials = nullptr;
  size_t wide_partials_doubles = 0;
  double* d_wide_out = nullptr;
  unsigned long long* d_wide_table = nullptr;
  unsigned* d_orth_mask = nullptr;  // the dropped columns of mgcmt_block_orthonormalize (its T lives in d_wide_out)
  double* d_rq = nullptr;       // Gram results of mgcmt_rayleigh_residual, one block per column
  double* d_rqstate = nullptr;  // scalars of the device-resident Rayleigh-quotient minimisation (kernels_rq.hip)
  double* d_mgs = nullptr;  // the blocked Gram-Schmidt's R^-1 and gate word (kernels_blas.hip)
  bool use_mgs_block = true;
  long mgs_block_min = 0;  // points per column from which a single plan takes the blocked form (0: wherever the one-workgroup kernel does not apply)
  double* d_rqhistory = nullptr;  // Rayleigh quotients recorded by mgcmt_rq_line_step (MGCMT_RQ_HISTORY numbers)
  // preconditioned conjugate gradients (pcg_host.hip): the head, the state words, the residual histories and the partial sums
  // of pcg_cap columns in one block (pcg_block_doubles(pcg_cap), grown when a begin asks for more columns); the solve in
  // progress: which entry began it (mgcmt_pcg_begin or mgcmt_pcg_begin_k: the other kind's iterate / status refuse it), its
  // columns and the first columns of its four ranges of slot W (x, p, q, p2)
  enum PcgKind { kPcgNone, kPcgSingle, kPcgBatched };
  double* d_pcg_block = nullptr;
  int pcg_cap = 0, pcg_k = 0;
  PcgKind pcg_kind = kPcgNone;
  int pcg_w[4] = {-1, -1, -1, -1};
  int pcg_march = -1;  // MGCMT_OPT_PCG_MARCH: 1 / 0 = the marching direction pass on / off, -1 = not set (MGCMT_PCG_MARCH, else the default)
  std::vector<double> h_shifts;
  bool has_mass = false;
  bool has_point = false;  // A carries a per-point part — a diagonal, bonds or a stencil, 2-D or 3-D: all six creators go through create_point / build_point_part (hierarchy.hip) —: KOp::point / K3Op::point on every level
  // how often mgcmt_plan_set_point_diagonal has replaced the per-point diagonal: what is derived from the planes (BandState)
  // remembers the count it was formed at and is formed again when the plan has moved on
  unsigned long point_version = 0;
  int density_max_blocks = 0;  // the grid limit of mgcmt_block_density, 0 = the default (MGCMT_DENSITY_BLOCKS, read at creation: tests)
  int mix_max_blocks = 0;      // the grid limit of mgcmt_mix_residual / mgcmt_mix_combine, 0 = the default (MGCMT_MIX_BLOCKS, read at creation: tests)
  bool use_fused = true;
  bool use_tail = true;   // levels of at most 32 x 32 points as one launch (kernels_tail.hip)
  bool use_tail_dense = true;  // ... and that launch as ONE dense product with the tail's matrix (formed once per shift set)
  struct TailMatrix {
    double* mt = nullptr;   // [k][n * n]
    int capacity = 0;       // vectors allocated
    long n = 0;
    int lt = -1, kind = -1, nu = -1, k = 0;
    double omega = 0.0;
    std::vector<double> shifts;
    bool valid = false;
  } tailmat;
  bool use_recompute = true;  // down-leg passes skip storing V', up-leg passes recompute it (fused_kernel.h)
  int two_level = 1;  // pair a 5-point level with its Galerkin level below in one down and one up launch: 1 from 2^22 points, 2 always, 0 never
  bool force_recompute = false;  // ... on every fused level, not only the bandwidth-bound ones (tests)
  // The carried right-hand side (cycle.hip: mgcmt_vcycle; fused2_kernel.h: CARRY).  A cycle whose last launch is the
  // two-level up pass has that pass go on with the fine part of the NEXT cycle's down pass and leaves what it would write
  // to F[level+1] in T[level+1]; an identical next cycle swaps the two roles and skips the pass.  The carry holds while
  // nothing it was computed from has changed: V[level] and F[level] (columns < k), T[level+1], the shifts, the options.
  // Every entry that takes a non-const plan drops it in its first statement (entry_drops_carry below); the exceptions
  // keep it with a CarryKeep.  mgcmt_vec_ptr, whose handle is const by the ABI, changes this state as well (it turns
  // carrying off): the one const entry that does.
  int carry_opt = 1;  // MGCMT_OPT_CARRY: 0 never, 1 on fine levels of >= 2^22 points, 2 wherever eligible (tests)
  struct Carry {
    bool valid = false;     // T[level+1] holds the next cycle's F[level+1]
    bool disabled = false;  // mgcmt_vec_ptr handed out a raw address: nothing can be vouched for any more
    int level = 0, nu1 = 0, nu2 = 0, nu_coarse = 0, kind = 0, k = 0, flags = 0;  // the last cycle's parameters (k = 0: none yet)
    double omega = 0.0;
    int unused_drops = 0;  // carries dropped unused in a row: from two on, none is produced ...
    std::string prev;      // ... until a cycle follows a cycle of the same parameters (those of the last cycle, "" once
                           // another entry has touched the plan)
  } carry;
  void carry_drop() {
    if (carry.valid) ++carry.unused_drops;
    carry.valid = false;
    carry.prev.clear();
  }
  // HIP-graph replay of whole cycles (mgcmt_vcycle): the launch sequence of a cycle is fixed by its
  // parameters and by which of the two buffers of every level currently is "V", so it is captured once per
  // such state and replayed; small grids are launch-latency-bound otherwise.
  bool use_graph = true;
  long fused_rows = 0;            // tuning: rows per wave chunk of the fused passes, 0 = automatic
  mgcmt::ShardComm* comm = nullptr;  // communicator of a sharded plan (sharded.hip), owned
  int use_lex_wave = 1;           // lexicographic sweeps on the whole chip where the level is covered: 1 = skewed column blocks with a scan per row (kernels_lexwave.hip), 2 = row bands swept as a wavefront (kernels_lexband.hip); 0 = one workgroup
  double* lex_carry = nullptr;    // its scratch (grown on demand)
  unsigned* lex_sync = nullptr;
  size_t lex_carry_doubles = 0, lex_sync_words = 0;
  bool lex_chain = true;          // consecutive Gauss-Seidel sweeps of a smoothing step run chained in one launch (kernels_lexwave.hip)
  bool lex_wave_used = false;     // the error word of lex_sync has not been looked at since the last sweep
  hipStream_t capture_stream = nullptr;
  struct CycleGraph {
    hipGraphExec_t exec = nullptr;
    std::vector<double*> post_state;  // base pointers of slots V, T and F of every level after the cycle
    bool lex_wave = false;            // the captured body runs the lexicographic wave pipeline (its error word must be checked after a replay)
  };
  std::map<std::string, CycleGraph> graphs;
  std::map<std::string, int> cycle_seen;
  void graphs_invalidate() {  // a captured launch sequence is only valid for the options it was captured under
    for (auto& g : graphs)
      if (g.second.exec) (void)hipGraphExecDestroy(g.second.exec);
    graphs.clear();
    cycle_seen.clear();
    carry_drop();
  }

  mgcmt::KGrid kgrid(int l) const {
    using namespace mgcmt;
    KGrid kg = levels[l].grid();
    kg.coarsen_rows = dim == 2 ? 1 : 0;
    return kg;
  }
  mgcmt::KVec kvec(int l, int slot, int vec = 0) const {
    using namespace mgcmt;
    const Level& L = levels[l];
    return KVec{L.base[slot] + (long)L.halo * L.gc + (long)vec * L.stride, (long)L.stride};
  }
  long interior(int l) const { return (long)levels[l].nr * levels[l].gc; }
};


namespace mgcmt {
// ---- plan.hip ----
int fail(int code, const std::string& msg);
// MGCMT_ERR_UNSUPPORTED (with a message naming `what`) on a 3-D plan: the entries of the 1-D / 2-D path that have no
// 3-D form; MGCMT_OK otherwise (a null plan included: the entry's own checks report it)
int unsupported_3d(const mgcmt_plan* p, const char* what);
int unsupported_3d_massless(const mgcmt_plan* p, const char* what);  // ... on a 3-D plan without a mass operator
// MGCMT_ERR_UNSUPPORTED (naming the point diagonal and `what`) on a plan with a per-point part: the entries whose kernels
// know Kronecker terms only; ..._smoother: the same for the lexicographic smoother kinds, MGCMT_OK for the others
int unsupported_point(const mgcmt_plan* p, const char* what);
int unsupported_point_smoother(const mgcmt_plan* p, int kind);
int check_level(const mgcmt_plan* p, int l);
int check_vec(const mgcmt_plan* p, int l, int slot, int vec);
int check_k(const mgcmt_plan* p, int k);
// The prologue of every exported entry that takes a non-const plan, i.e. may change what a carried right-hand side was
// computed from (mgcmt_plan::carry): the first statement of the entry, once per such plan argument
// (tests/test_carry_prologue.py reads the sources for it).  The exceptions are mgcmt_vcycle, which decides itself what
// becomes of the carry, and the entries that provably leave those vectors alone and declare a CarryKeep instead: the carry
// is dropped there as well, and it and its back-off state are put back when the entry returns, unless writes() found the
// destination to be one of the vectors the carry depends on.
inline void entry_drops_carry(mgcmt_plan* p) {
  if (p) p->carry_drop();
}
struct CarryKeep {
  mgcmt_plan* p;
  mgcmt_plan::Carry saved;
  bool keep = true;
  explicit CarryKeep(mgcmt_plan* plan) : p(plan) {
    if (p) {
      saved = p->carry;
      p->carry_drop();
    }
  }
  // the entry writes vector (l, slot, vec): the carry goes if it depends on it (and with or without a carry, the
  // next cycle no longer follows the last one)
  void writes(int l, int slot, int vec) {
    if (p && vec < saved.k &&
        ((l == saved.level && (slot == MGCMT_SLOT_V || slot == MGCMT_SLOT_F)) || (l == saved.level + 1 && slot == MGCMT_SLOT_T)))
      keep = false;
  }
  ~CarryKeep() {
    if (p && keep) {
      const bool disabled = p->carry.disabled;
      p->carry = saved;
      p->carry.disabled = disabled;
    }
  }
};
inline hipStream_t S(void* s) { return (hipStream_t)s; }
int ensure_slot(mgcmt_plan* p, int l, int slot);
int post_launch();
// ---- cycle.hip ----
bool fused_level(const mgcmt_plan* p, int l, int kind);
int pass_sweeps(const mgcmt_plan* p, int l, int kind, int left);
// halo rows of level l that a sharded cycle exchanges and its passes read (<= the level's halo): 8 behind a 5-point
// operator (at most eight stages per pass), 10 behind a 9-point one (two four-colour sweeps + the restriction: nine)
int exchanged_rows(const mgcmt_plan* p, int l);
// one fused pass V -> T (then swapped); [out_lo, out_hi) = the rows produced (default: the whole strip), swap = false
// leaves the buffer roles alone (the caller issues the other row ranges of the same pass and swaps once)
int fused_pass(mgcmt_plan* p, int l, int kind, int nsweep, double omega, int mode, int k, hipStream_t s, int npre = 0,
               long out_lo = 0, long out_hi = -1, bool swap = true, long out_lo2 = 0, long out_hi2 = 0);
int smooth_impl(mgcmt_plan* p, int l, int kind, int nu, double omega, int k, hipStream_t s);
int gramschmidt_impl(mgcmt_plan* p, int l, int slot, int k, int modified, hipStream_t s);
int lex_wave_check(mgcmt_plan* p);  // a synchronising call looks at the error word of the wave pipeline
// The plan's HIP-graph cache: `body` (a stream-ordered launch sequence fixed by `params` and by the buffer bases in
// `key`) runs eagerly the first time `params` is seen, is captured, launched and stored under `key` the second time, and
// is replayed on every later call with an equal key.  `prepare` (may be empty) is what a replay or a capture relies on
// but must not contain; it runs eagerly before either.  swaps_buffers: the body exchanges the V / T bases of levels, so
// they are recorded after the capture and restored after a replay, a capture that fails cannot be run again (an error)
// and any failure turns the plan's graphs off; without it a failure clears the HIP error and the body runs eagerly.
int graph_run(mgcmt_plan* p, const std::string& params, const std::string& key, bool swaps_buffers, const std::function<int()>& prepare,
              const std::function<int(hipStream_t)>& body, hipStream_t s);
// ---- sharded.hip, transfer.hip ----
void comm_release(mgcmt_plan* p);  // frees p->comm
// a whole vector between caller memory and the device through the pinned ring; completed on return
int transfer(int device, bool upload, void* dev, void* host, size_t bytes, hipStream_t stream);
}  // namespace mgcmt

#define MG_HIP(expr)                                                                                    \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess)                                                                               \
      return mgcmt::fail(MGCMT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));             \
  } while (0)

#define MG_TRY(expr)          \
  do {                        \
    int rc_ = (expr);         \
    if (rc_ != MGCMT_OK) return rc_; \
  } while (0)
