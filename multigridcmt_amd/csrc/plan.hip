// What every other host file of libmgcmt_hip.so leans on (error text, argument checks, level vector storage) and the
// C-ABI that is neither hierarchy (hierarchy.hip), cycle (cycle.hip) nor Rayleigh quotient (rq_host.hip): vector
// transfer / fill / copy, the BLAS-like entries, plan options, the probes and timers.
// Host code only; every kernel it enqueues is in kernels_*.hip.
#include <cmath>
#include <cstdio>
#include <string>

#include "plan_internal.h"

using namespace mgcmt;

namespace {
thread_local std::string g_last_error;
}

namespace mgcmt {
int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

int unsupported_3d(const mgcmt_plan* p, const char* what) {
  if (p && p->dim == 3) return fail(MGCMT_ERR_UNSUPPORTED, std::string(what) + " is not available on a 3-D plan");
  return MGCMT_OK;
}

// the Rayleigh-quotient entries run on a 3-D plan that carries a mass operator (mgcmt_plan_create3d_mass): without one the
// coarse levels would minimise with I where the reference has R I P, so callers pass M = I explicitly
int unsupported_3d_massless(const mgcmt_plan* p, const char* what) {
  if (p && p->dim == 3 && !p->has_mass)
    return fail(MGCMT_ERR_UNSUPPORTED, std::string(what) + " is not available on a 3-D plan without a mass operator (mgcmt_plan_create3d_mass)");
  return MGCMT_OK;
}

int unsupported_point(const mgcmt_plan* p, const char* what) {
  if (p && p->has_point) return fail(MGCMT_ERR_UNSUPPORTED, std::string(what) + " is not available on a plan with a point diagonal");
  return MGCMT_OK;
}

int unsupported_point_smoother(const mgcmt_plan* p, int kind) {
  if (p && p->has_point && (kind == MGCMT_GS_LEX || kind == MGCMT_SOR_LEX))
    return fail(MGCMT_ERR_UNSUPPORTED,
                "lexicographic smoothers are not available on a plan with a point diagonal (MGCMT_WJACOBI and MGCMT_GS_MC are)");
  return MGCMT_OK;
}

int ensure_slot(mgcmt_plan* p, int l, int slot) {
  Level& L = p->levels[l];
  if (L.base[slot]) return MGCMT_OK;
  const size_t bytes = (size_t)L.stride * p->nvec * sizeof(double);
  hipError_t e = hipMalloc((void**)&L.base[slot], bytes);
  if (e != hipSuccess) return fail(MGCMT_ERR_NOMEM, std::string("hipMalloc of a level vector failed: ") + hipGetErrorString(e));
  MG_HIP(hipMemset(L.base[slot], 0, bytes));
  return MGCMT_OK;
}

int check_level(const mgcmt_plan* p, int l) {
  if (!p) return fail(MGCMT_ERR_INVALID, "null plan");
  if (l < 0 || l >= (int)p->levels.size()) return fail(MGCMT_ERR_INVALID, "level out of range");
  return MGCMT_OK;
}

int check_vec(const mgcmt_plan* p, int l, int slot, int vec) {
  MG_TRY(check_level(p, l));
  if (slot < 0 || slot > 3) return fail(MGCMT_ERR_INVALID, "slot out of range");
  if (vec < 0 || vec >= p->nvec) return fail(MGCMT_ERR_INVALID, "vector index out of range");
  return MGCMT_OK;
}

int check_k(const mgcmt_plan* p, int k) {
  if (k < 1 || k > p->nvec) return fail(MGCMT_ERR_INVALID, "k must be in 1..nvec");
  // (a plan may store more vectors than one launch batches: the shifts, the reduction results and the kernels' static arrays hold kMaxVec)
  if (k > kMaxVec) return fail(MGCMT_ERR_INVALID, "k must be at most 32: a plan stores up to 80 vectors per slot, an entry batches 32 columns");
  return MGCMT_OK;
}

int post_launch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MGCMT_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  return MGCMT_OK;
}
}  // namespace mgcmt

extern "C" {

const char* mgcmt_last_error(void) { return g_last_error.c_str(); }

int mgcmt_abi_version(void) { return MGCMT_ABI_VERSION; }

int mgcmt_device_count(int* count) {
  if (!count) return fail(MGCMT_ERR_INVALID, "null count");
  MG_HIP(hipGetDeviceCount(count));
  return MGCMT_OK;
}

int mgcmt_device_name(int device, char* buf, int buflen) {
  if (!buf || buflen <= 0) return fail(MGCMT_ERR_INVALID, "bad buffer");
  hipDeviceProp_t prop;
  MG_HIP(hipGetDeviceProperties(&prop, device));
  snprintf(buf, buflen, "%s (%s, %d CUs)", prop.name[0] ? prop.name : "AMD Instinct", prop.gcnArchName, prop.multiProcessorCount);
  return MGCMT_OK;
}

int mgcmt_vec_ptr(const mgcmt_plan* p, int l, int slot, int vec, void** device_ptr) {
  MG_TRY(check_vec(p, l, slot, vec));
  if (!device_ptr) return fail(MGCMT_ERR_INVALID, "null pointer");
  // a raw address can be written with no further call: no carried right-hand side can be vouched for from here on
  const_cast<mgcmt_plan*>(p)->carry_drop();
  const_cast<mgcmt_plan*>(p)->carry.disabled = true;
  MG_TRY(ensure_slot(const_cast<mgcmt_plan*>(p), l, slot));
  *device_ptr = p->kvec(l, slot, vec).p;
  return MGCMT_OK;
}

int mgcmt_set_shifts(mgcmt_plan* p, const double* shifts, int k, void* stream) {
  entry_drops_carry(p);
  if (!p || !shifts) return fail(MGCMT_ERR_INVALID, "null argument");
  MG_TRY(check_k(p, k));
  for (int q = 0; q < k; ++q) p->h_shifts[q] = shifts[q];
  // the host array may be reused immediately by the caller: stage through the plan's own copy
  MG_HIP(hipMemcpyAsync(p->d_shifts, p->h_shifts.data(), sizeof(double) * k, hipMemcpyHostToDevice, S(stream)));
  MG_HIP(hipStreamSynchronize(S(stream)));
  return MGCMT_OK;
}

int mgcmt_upload(mgcmt_plan* p, int l, int slot, int vec, const double* host, int64_t count, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_vec(p, l, slot, vec));
  if (!host || count != p->interior(l)) return fail(MGCMT_ERR_INVALID, "upload: count must equal rows*cols of the level");
  MG_TRY(ensure_slot(p, l, slot));
  return transfer(p->device, true, p->kvec(l, slot, vec).p, const_cast<double*>(host), sizeof(double) * count, S(stream));
}

int mgcmt_download(mgcmt_plan* p, int l, int slot, int vec, double* host, int64_t count, void* stream) {
  CarryKeep keep(p);  // a reader
  MG_TRY(check_vec(p, l, slot, vec));
  if (!host || count != p->interior(l)) return fail(MGCMT_ERR_INVALID, "download: count must equal rows*cols of the level");
  MG_TRY(ensure_slot(p, l, slot));
  MG_TRY(transfer(p->device, false, p->kvec(l, slot, vec).p, host, sizeof(double) * count, S(stream)));
  return lex_wave_check(p);
}

int mgcmt_fill(mgcmt_plan* p, int l, int slot, int vec, double value, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_vec(p, l, slot, vec));
  MG_TRY(ensure_slot(p, l, slot));
  launch_fill(S(stream), p->kvec(l, slot, vec).p, p->interior(l), value);
  return post_launch();
}

int mgcmt_zero(mgcmt_plan* p, int l, int slot, int vec, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_vec(p, l, slot, vec));
  MG_TRY(ensure_slot(p, l, slot));
  const Level& L = p->levels[l];
  MG_HIP(hipMemsetAsync(p->kvec(l, slot, vec).p - (long)L.halo * L.gc, 0, sizeof(double) * (size_t)(L.nr + 2 * L.halo) * L.gc, S(stream)));
  return MGCMT_OK;
}

int mgcmt_copy(mgcmt_plan* p, int l, int src_slot, int src_vec, int dst_slot, int dst_vec, void* stream) {
  CarryKeep keep(p);
  keep.writes(l, dst_slot, dst_vec);
  MG_TRY(check_vec(p, l, src_slot, src_vec));
  MG_TRY(check_vec(p, l, dst_slot, dst_vec));
  MG_TRY(ensure_slot(p, l, src_slot));
  MG_TRY(ensure_slot(p, l, dst_slot));
  MG_HIP(hipMemcpyAsync(p->kvec(l, dst_slot, dst_vec).p, p->kvec(l, src_slot, src_vec).p, sizeof(double) * p->interior(l),
                        hipMemcpyDeviceToDevice, S(stream)));
  return MGCMT_OK;
}

int mgcmt_copy_across(mgcmt_plan* src, int l, int src_slot, int src_vec, mgcmt_plan* dst, int dst_slot, int dst_vec, void* stream) {
  entry_drops_carry(src);
  entry_drops_carry(dst);
  MG_TRY(check_vec(src, l, src_slot, src_vec));
  MG_TRY(check_vec(dst, l, dst_slot, dst_vec));
  if (src->dim != dst->dim) return fail(MGCMT_ERR_INVALID, "copy_across: the plans differ in dimension");
  if (src->device != dst->device) return fail(MGCMT_ERR_INVALID, "copy_across: the plans live on different devices");
  // the interior of a level vector is nr * gc contiguous numbers behind the halo: equal rows and columns, both whole grids
  const Level &A = src->levels[l], &B = dst->levels[l];
  if (A.nr != B.nr || A.gc != B.gc || A.gr != B.gr || A.r0 != B.r0 || A.nr != A.gr)
    return fail(MGCMT_ERR_INVALID, "copy_across: the level's shape differs between the plans (or one of them is a row strip)");
  MG_TRY(ensure_slot(src, l, src_slot));
  MG_TRY(ensure_slot(dst, l, dst_slot));
  const double* from = src->kvec(l, src_slot, src_vec).p;
  double* to = dst->kvec(l, dst_slot, dst_vec).p;
  if (from == to) return fail(MGCMT_ERR_INVALID, "copy_across: source and destination are the same vector");
  MG_HIP(hipMemcpyAsync(to, from, sizeof(double) * src->interior(l), hipMemcpyDeviceToDevice, S(stream)));
  return MGCMT_OK;
}

int mgcmt_sync(void* stream) {
  MG_HIP(hipStreamSynchronize(S(stream)));
  return MGCMT_OK;
}

int mgcmt_apply(mgcmt_plan* p, int op, int l, int src_slot, int src_vec, int dst_slot, int dst_vec, int with_shift, void* stream) {
  CarryKeep keep(p);
  keep.writes(l, dst_slot, dst_vec);
  MG_TRY(check_vec(p, l, src_slot, src_vec));
  MG_TRY(check_vec(p, l, dst_slot, dst_vec));
  if (src_slot == dst_slot && src_vec == dst_vec) return fail(MGCMT_ERR_INVALID, "apply cannot run in place");
  if (op == MGCMT_OP_M && !p->has_mass) return fail(MGCMT_ERR_INVALID, "plan has no mass operator");
  // (the shift of column src_vec: the plan holds kMaxVec of them however many vectors it stores)
  if (with_shift && src_vec >= kMaxVec) return fail(MGCMT_ERR_INVALID, "apply with_shift: only columns 0..31 have a shift");
  MG_TRY(ensure_slot(p, l, src_slot));
  MG_TRY(ensure_slot(p, l, dst_slot));
  const KOp& k = op == MGCMT_OP_M ? p->levels[l].dM.k : p->levels[l].dA.k;
  const double* sh = with_shift ? p->d_shifts + src_vec : p->d_zero;
  if (p->dim == 3) {
    const K3Op& k3 = op == MGCMT_OP_M ? p->levels[l].dM.k3 : p->levels[l].dA.k3;
    launch3_apply(S(stream), k3, p->kvec(l, src_slot, src_vec), p->kvec(l, dst_slot, dst_vec), sh, 1);
    return post_launch();
  }
  launch_apply(S(stream), p->kgrid(l), k, p->kvec(l, src_slot, src_vec), p->kvec(l, dst_slot, dst_vec), sh, 1);
  return post_launch();
}

int mgcmt_restrict(mgcmt_plan* p, int l, int src_slot, int src_vec, int dst_slot, int dst_vec, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_vec(p, l, src_slot, src_vec));
  MG_TRY(check_vec(p, l + 1, dst_slot, dst_vec));
  MG_TRY(ensure_slot(p, l, src_slot));
  MG_TRY(ensure_slot(p, l + 1, dst_slot));
  if (p->dim == 3) {
    launch3_restrict(S(stream), p->levels[l].dA.k3, p->kvec(l, src_slot, src_vec), p->kvec(l + 1, dst_slot, dst_vec), 1);
    return post_launch();
  }
  launch_restrict(S(stream), p->kgrid(l), p->kgrid(l + 1), p->kvec(l, src_slot, src_vec), p->kvec(l + 1, dst_slot, dst_vec), 1);
  return post_launch();
}

int mgcmt_prolong(mgcmt_plan* p, int l, int src_slot, int src_vec, int dst_slot, int dst_vec, int accumulate, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_vec(p, l + 1, src_slot, src_vec));
  MG_TRY(check_vec(p, l, dst_slot, dst_vec));
  MG_TRY(ensure_slot(p, l + 1, src_slot));
  MG_TRY(ensure_slot(p, l, dst_slot));
  if (p->dim == 3) {
    launch3_prolong(S(stream), p->levels[l].gr, p->kvec(l + 1, src_slot, src_vec), p->kvec(l, dst_slot, dst_vec), accumulate, 1);
    return post_launch();
  }
  launch_prolong(S(stream), p->kgrid(l), p->kgrid(l + 1), p->kvec(l + 1, src_slot, src_vec), p->kvec(l, dst_slot, dst_vec), accumulate, 1);
  return post_launch();
}

int mgcmt_dot(mgcmt_plan* p, int l, int slot_a, int vec_a, int slot_b, int vec_b, double* host_out, void* stream) {
  CarryKeep keep(p);  // a reader
  MG_TRY(check_vec(p, l, slot_a, vec_a));
  MG_TRY(check_vec(p, l, slot_b, vec_b));
  if (!host_out) return fail(MGCMT_ERR_INVALID, "null output");
  MG_TRY(ensure_slot(p, l, slot_a));
  MG_TRY(ensure_slot(p, l, slot_b));
  launch_dots(S(stream), p->interior(l), p->kvec(l, slot_a, vec_a).p, p->kvec(l, slot_b, vec_b).p, 0, 1, p->d_partials, p->d_scalars);
  MG_TRY(post_launch());
  MG_HIP(hipMemcpyAsync(host_out, p->d_scalars, sizeof(double), hipMemcpyDeviceToHost, S(stream)));
  MG_HIP(hipStreamSynchronize(S(stream)));
  return MGCMT_OK;
}

int mgcmt_gram(mgcmt_plan* p, int l, int nv, const int* slots, const int* vecs, double* host_out, void* stream) {
  CarryKeep keep(p);  // a reader
  MG_TRY(check_level(p, l));
  if (!slots || !vecs || !host_out || nv < 1 || nv > kGramMaxVectors) return fail(MGCMT_ERR_INVALID, "gram: 1..6 vectors, non-null arguments");
  const double* v[kGramMaxVectors];
  for (int a = 0; a < nv; ++a) {
    MG_TRY(check_vec(p, l, slots[a], vecs[a]));
    MG_TRY(ensure_slot(p, l, slots[a]));
    v[a] = p->kvec(l, slots[a], vecs[a]).p;
  }
  constexpr int kPairs = kGramMaxVectors * (kGramMaxVectors + 1) / 2;
  launch_gram(S(stream), p->interior(l), v, nv, p->d_partials, p->d_scalars);
  MG_TRY(post_launch());
  double packed[kPairs];
  MG_HIP(hipMemcpyAsync(packed, p->d_scalars, sizeof(packed), hipMemcpyDeviceToHost, S(stream)));
  MG_HIP(hipStreamSynchronize(S(stream)));
  int t = 0;
  for (int a = 0; a < kGramMaxVectors; ++a)
    for (int b = a; b < kGramMaxVectors; ++b, ++t)
      if (b < nv) host_out[a * nv + b] = host_out[b * nv + a] = packed[t];
  return MGCMT_OK;
}

int mgcmt_lincomb(mgcmt_plan* p, int l, int nterms, const double* coeffs, const int* slots, const int* vecs, int dst_slot, int dst_vec,
                  void* stream) {
  CarryKeep keep(p);
  keep.writes(l, dst_slot, dst_vec);
  MG_TRY(check_level(p, l));
  if (!coeffs || !slots || !vecs || nterms < 1 || nterms > 4) return fail(MGCMT_ERR_INVALID, "lincomb: 1..4 terms, non-null arguments");
  MG_TRY(check_vec(p, l, dst_slot, dst_vec));
  MG_TRY(ensure_slot(p, l, dst_slot));
  const double* v[4];
  for (int t = 0; t < nterms; ++t) {
    MG_TRY(check_vec(p, l, slots[t], vecs[t]));
    MG_TRY(ensure_slot(p, l, slots[t]));
    v[t] = p->kvec(l, slots[t], vecs[t]).p;
  }
  launch_lincomb(S(stream), p->interior(l), v, coeffs, nterms, p->kvec(l, dst_slot, dst_vec).p);
  return post_launch();
}

int mgcmt_block_gram(mgcmt_plan* p, int l, int na, const int* a_slots, const int* a_vecs, int nb, const int* b_slots, const int* b_vecs,
                     double* host_out, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_level(p, l));
  if (!a_slots || !a_vecs || !b_slots || !b_vecs || !host_out || na < 1 || na > kBlockMaxA || nb < 1 || nb > kBlockMaxB)
    return fail(MGCMT_ERR_INVALID, "block_gram: 1..12 by 1..4 vectors, non-null arguments");
  const double *a[kBlockMaxA], *b[kBlockMaxB];
  for (int t = 0; t < na; ++t) {
    MG_TRY(check_vec(p, l, a_slots[t], a_vecs[t]));
    MG_TRY(ensure_slot(p, l, a_slots[t]));
    a[t] = p->kvec(l, a_slots[t], a_vecs[t]).p;
  }
  for (int t = 0; t < nb; ++t) {
    MG_TRY(check_vec(p, l, b_slots[t], b_vecs[t]));
    MG_TRY(ensure_slot(p, l, b_slots[t]));
    b[t] = p->kvec(l, b_slots[t], b_vecs[t]).p;
  }
  launch_block_gram(S(stream), p->interior(l), a, na, b, nb, p->d_partials, p->d_scalars);
  MG_TRY(post_launch());
  double packed[kBlockMaxA * kBlockMaxB];
  MG_HIP(hipMemcpyAsync(packed, p->d_scalars, sizeof(packed), hipMemcpyDeviceToHost, S(stream)));
  MG_HIP(hipStreamSynchronize(S(stream)));
  for (int i = 0; i < na; ++i)
    for (int j = 0; j < nb; ++j) host_out[i * nb + j] = packed[i * kBlockMaxB + j];
  return MGCMT_OK;
}

int mgcmt_block_combine(mgcmt_plan* p, int l, int nin, const int* in_slots, const int* in_vecs, int nout, const int* out_slots,
                        const int* out_vecs, const double* coeffs, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_level(p, l));
  if (!in_slots || !in_vecs || !out_slots || !out_vecs || !coeffs || nin < 1 || nin > kBlockMaxA || nout < 1 || nout > kBlockMaxB)
    return fail(MGCMT_ERR_INVALID, "block_combine: 1..12 inputs, 1..4 outputs, non-null arguments");
  const double* in[kBlockMaxA];
  double* out[kBlockMaxB];
  for (int t = 0; t < nin; ++t) {
    MG_TRY(check_vec(p, l, in_slots[t], in_vecs[t]));
    MG_TRY(ensure_slot(p, l, in_slots[t]));
    in[t] = p->kvec(l, in_slots[t], in_vecs[t]).p;
  }
  for (int j = 0; j < nout; ++j) {
    MG_TRY(check_vec(p, l, out_slots[j], out_vecs[j]));
    MG_TRY(ensure_slot(p, l, out_slots[j]));
    out[j] = p->kvec(l, out_slots[j], out_vecs[j]).p;
    for (int i = 0; i < j; ++i)
      if (out[i] == out[j]) return fail(MGCMT_ERR_INVALID, "block_combine: an output vector named twice");
  }
  launch_block_combine(S(stream), p->interior(l), in, nin, out, nout, coeffs);
  return post_launch();
}

// (slot, vec) pairs of a wide block entry -> device pointers
static int wide_vectors(mgcmt_plan* p, int l, int count, const int* slots, const int* vecs, double** out) {
  for (int t = 0; t < count; ++t) {
    MG_TRY(check_vec(p, l, slots[t], vecs[t]));
    MG_TRY(ensure_slot(p, l, slots[t]));
    out[t] = p->kvec(l, slots[t], vecs[t]).p;
  }
  return MGCMT_OK;
}

// the scratch of the entries that sum tiles: room for `need` doubles of per-workgroup partial tiles, and the summed tiles
static int wide_scratch(mgcmt_plan* p, size_t need, hipStream_t stream) {
  if (need > p->wide_partials_doubles) {
    MG_HIP(hipStreamSynchronize(stream));  // (an earlier pencil on this stream may still read the old buffer)
    if (p->d_wide_partials) (void)hipFree(p->d_wide_partials);
    p->d_wide_partials = nullptr;
    p->wide_partials_doubles = 0;
    MG_HIP(hipMalloc((void**)&p->d_wide_partials, sizeof(double) * need));
    p->wide_partials_doubles = need;
  }
  constexpr int kMaxTiles = 2 * 3 * 3;  // (the pencil of 48 vectors with a mass operator; a deflation sums four)
  if (!p->d_wide_out) MG_HIP(hipMalloc((void**)&p->d_wide_out, sizeof(double) * kMaxTiles * 256));
  return MGCMT_OK;
}

int mgcmt_block_pencil(mgcmt_plan* p, int l, int m, const int* s_slots, const int* s_vecs, const int* as_slots, const int* as_vecs,
                       const int* ms_slots, const int* ms_vecs, double* h_out, double* g_out, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_level(p, l));
  if (!s_slots || !s_vecs || !as_slots || !as_vecs || !h_out || !g_out || (ms_slots == nullptr) != (ms_vecs == nullptr) || m < 1 || m > kBlockWideMax)
    return fail(MGCMT_ERR_INVALID, "block_pencil: 1..48 vectors, non-null arguments (ms_slots and ms_vecs both null: M = I)");
  const bool mass = ms_slots != nullptr;
  double *sv[kBlockWideMax], *as[kBlockWideMax], *ms[kBlockWideMax];
  MG_TRY(wide_vectors(p, l, m, s_slots, s_vecs, sv));
  MG_TRY(wide_vectors(p, l, m, as_slots, as_vecs, as));
  if (mass) MG_TRY(wide_vectors(p, l, m, ms_slots, ms_vecs, ms));
  const long n = p->interior(l);
  const int tiles = block_pencil_tiles(m, mass), side = (m + 15) / 16;
  MG_TRY(wide_scratch(p, (size_t)tiles * block_pencil_blocks(n) * 256, S(stream)));
  if (!launch_block_pencil(S(stream), n, m, sv, as, mass ? ms : nullptr, p->d_wide_partials, p->d_wide_out))
    return fail(MGCMT_ERR_INVALID, "block_pencil: a vector is not 16-byte aligned");
  MG_TRY(post_launch());
  std::vector<double> packed((size_t)tiles * 256);
  MG_HIP(hipMemcpyAsync(packed.data(), p->d_wide_out, sizeof(double) * packed.size(), hipMemcpyDeviceToHost, S(stream)));
  MG_HIP(hipStreamSynchronize(S(stream)));
  // tiles of H (I, J) row-major, then of G: all of them with a mass operator, the upper triangle J >= I (mirrored here) without
  const double* t = packed.data();
  for (int which = 0; which < 2; ++which) {
    double* out = which == 0 ? h_out : g_out;
    for (int I = 0; I < side; ++I)
      for (int J = 0; J < side; ++J) {
        if (which == 1 && !mass && J < I) continue;
        for (int r = 0; r < 16 && 16 * I + r < m; ++r)
          for (int c = 0; c < 16 && 16 * J + c < m; ++c) {
            out[(16 * I + r) * m + 16 * J + c] = t[r * 16 + c];
            if (which == 1 && !mass && J > I) out[(16 * J + c) * m + 16 * I + r] = t[r * 16 + c];
          }
        t += 256;
      }
  }
  return MGCMT_OK;
}

int mgcmt_block_combine_wide(mgcmt_plan* p, int l, int nin, const int* in_slots, const int* in_vecs, int nout, const int* out_slots,
                             const int* out_vecs, const double* coeffs, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_level(p, l));
  if (!in_slots || !in_vecs || !out_slots || !out_vecs || !coeffs || nin < 1 || nin > kBlockWideMax || nout < 1 || nout > kBlockWideOut)
    return fail(MGCMT_ERR_INVALID, "block_combine_wide: 1..48 inputs, 1..16 outputs, non-null arguments");
  double *in[kBlockWideMax], *out[kBlockWideOut];
  MG_TRY(wide_vectors(p, l, nin, in_slots, in_vecs, in));
  MG_TRY(wide_vectors(p, l, nout, out_slots, out_vecs, out));
  for (int j = 0; j < nout; ++j)
    for (int i = 0; i < j; ++i)
      if (out[i] == out[j]) return fail(MGCMT_ERR_INVALID, "block_combine_wide: an output vector named twice");
  if (!p->d_wide_table) MG_HIP(hipMalloc((void**)&p->d_wide_table, sizeof(unsigned long long) * block_wide_table_words()));
  if (!launch_block_combine_wide(S(stream), p->interior(l), in, nin, out, nout, coeffs, p->d_wide_table))
    return fail(MGCMT_ERR_INVALID, "block_combine_wide: an odd number of points or a vector that is not 16-byte aligned");
  return post_launch();
}

int mgcmt_block_deflate(mgcmt_plan* p, int l, int nq, const int* q_slots, const int* q_vecs, int k, const int* w_slots, const int* w_vecs,
                        double* coeffs_out, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_level(p, l));
  if (nq < 1 || nq > kBlockLockedMax || k < 1 || k > kBlockWideOut)
    return fail(MGCMT_ERR_INVALID, "block_deflate: 1..64 vectors Q, 1..16 vectors W");
  if (!q_slots || !q_vecs || !w_slots || !w_vecs) return fail(MGCMT_ERR_INVALID, "block_deflate: non-null vector lists");
  double *q[kBlockLockedMax], *w[kBlockWideOut];
  MG_TRY(wide_vectors(p, l, nq, q_slots, q_vecs, q));
  MG_TRY(wide_vectors(p, l, k, w_slots, w_vecs, w));
  for (int j = 0; j < k; ++j) {
    for (int i = 0; i < j; ++i)
      if (w[i] == w[j]) return fail(MGCMT_ERR_INVALID, "block_deflate: a vector W named twice");
    for (int i = 0; i < nq; ++i)
      if (q[i] == w[j]) return fail(MGCMT_ERR_INVALID, "block_deflate: a vector W that is also a Q");
  }
  const long n = p->interior(l);
  const int tiles = (nq + 15) / 16;
  MG_TRY(wide_scratch(p, (size_t)tiles * block_pencil_blocks(n) * 256, S(stream)));
  if (!launch_block_deflate(S(stream), n, nq, q, k, w, p->d_wide_partials, p->d_wide_out))
    return fail(MGCMT_ERR_INVALID, "block_deflate: an odd number of points or a vector that is not 16-byte aligned");
  MG_TRY(post_launch());
  if (coeffs_out) {
    std::vector<double> packed((size_t)nq * kBlockWideOut);
    MG_HIP(hipMemcpyAsync(packed.data(), p->d_wide_out, sizeof(double) * packed.size(), hipMemcpyDeviceToHost, S(stream)));
    MG_HIP(hipStreamSynchronize(S(stream)));
    for (int i = 0; i < nq; ++i)
      for (int j = 0; j < k; ++j) coeffs_out[i * k + j] = packed[(size_t)i * kBlockWideOut + j];
  }
  return MGCMT_OK;
}

int mgcmt_block_density(mgcmt_plan* p, int l, int nq, const int* x_slots, const int* x_vecs, const double* weights, int dst_slot, int dst_vec,
                        void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_level(p, l));
  if (nq < 1 || nq > kBlockLockedMax) return fail(MGCMT_ERR_INVALID, "block_density: 1..64 vectors X");
  if (!x_slots || !x_vecs || !weights) return fail(MGCMT_ERR_INVALID, "block_density: non-null vector lists and weights");
  double* x[kBlockLockedMax];
  MG_TRY(wide_vectors(p, l, nq, x_slots, x_vecs, x));
  MG_TRY(check_vec(p, l, dst_slot, dst_vec));
  MG_TRY(ensure_slot(p, l, dst_slot));
  double* dst = p->kvec(l, dst_slot, dst_vec).p;
  for (int t = 0; t < nq; ++t) {
    if (x[t] == dst) return fail(MGCMT_ERR_INVALID, "block_density: the destination is also an X");
    if (!std::isfinite(weights[t])) return fail(MGCMT_ERR_INVALID, "block_density: a weight that is not finite");
  }
  if (!launch_block_density(S(stream), p->interior(l), nq, x, weights, dst, p->density_max_blocks))
    return fail(MGCMT_ERR_INVALID, "block_density: an odd number of points or a vector that is not 16-byte aligned");
  return post_launch();
}

int mgcmt_mix_residual(mgcmt_plan* p, int l, int out_slot, int out_vec, int in_slot, int in_vec, int r_slot, int r_vec, int nprev,
                       const int* prev_slots, const int* prev_vecs, double* host_out, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_level(p, l));
  if (nprev < 0 || nprev > kMixMax - 1) return fail(MGCMT_ERR_INVALID, "mix_residual: 0..8 earlier residuals");
  if ((nprev > 0 && (!prev_slots || !prev_vecs)) || !host_out) return fail(MGCMT_ERR_INVALID, "mix_residual: non-null vector lists and output");
  const int io_slots[3] = {out_slot, in_slot, r_slot}, io_vecs[3] = {out_vec, in_vec, r_vec};
  double *io[3], *prev[kMixMax];
  MG_TRY(wide_vectors(p, l, 3, io_slots, io_vecs, io));
  MG_TRY(wide_vectors(p, l, nprev, prev_slots, prev_vecs, prev));
  bool aliased = io[2] == io[0] || io[2] == io[1];
  for (int j = 0; j < nprev; ++j) aliased = aliased || prev[j] == io[2];
  if (aliased) return fail(MGCMT_ERR_INVALID, "mix_residual: the destination r is also a vector that is read");
  if (!launch_mix_residual(S(stream), p->interior(l), io[0], io[1], io[2], nprev, prev, p->d_partials, p->d_scalars, p->mix_max_blocks))
    return fail(MGCMT_ERR_INVALID, "mix_residual: an odd number of points or a vector that is not 16-byte aligned");
  MG_TRY(post_launch());
  double packed[kMixMax + 1];  // the kernel's order: <r, r>, <out, out>, <r, prev_j>
  MG_HIP(hipMemcpyAsync(packed, p->d_scalars, sizeof(double) * (nprev + 2), hipMemcpyDeviceToHost, S(stream)));
  MG_HIP(hipStreamSynchronize(S(stream)));
  for (int j = 0; j < nprev; ++j) host_out[j] = packed[2 + j];
  host_out[nprev] = packed[0];
  host_out[nprev + 1] = packed[1];
  return MGCMT_OK;
}

int mgcmt_mix_combine(mgcmt_plan* p, int l, int np, const int* x_slots, const int* x_vecs, const int* r_slots, const int* r_vecs,
                      const double* alpha, double beta, int dst_slot, int dst_vec, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_level(p, l));
  if (np < 1 || np > kMixMax) return fail(MGCMT_ERR_INVALID, "mix_combine: 1..9 pairs (x, r)");
  if (!x_slots || !x_vecs || !r_slots || !r_vecs || !alpha) return fail(MGCMT_ERR_INVALID, "mix_combine: non-null vector lists and coefficients");
  double *x[kMixMax], *r[kMixMax];
  MG_TRY(wide_vectors(p, l, np, x_slots, x_vecs, x));
  MG_TRY(wide_vectors(p, l, np, r_slots, r_vecs, r));
  MG_TRY(check_vec(p, l, dst_slot, dst_vec));
  MG_TRY(ensure_slot(p, l, dst_slot));
  double* dst = p->kvec(l, dst_slot, dst_vec).p;
  if (!std::isfinite(beta)) return fail(MGCMT_ERR_INVALID, "mix_combine: a coefficient that is not finite");
  for (int i = 0; i < np; ++i) {
    if (!std::isfinite(alpha[i])) return fail(MGCMT_ERR_INVALID, "mix_combine: a coefficient that is not finite");
    if ((i > 0 && x[i] == dst) || r[i] == dst)
      return fail(MGCMT_ERR_INVALID, "mix_combine: the destination is also an input other than the oldest x");
  }
  if (!launch_mix_combine(S(stream), p->interior(l), np, x, r, alpha, beta, dst, p->mix_max_blocks))
    return fail(MGCMT_ERR_INVALID, "mix_combine: an odd number of points or a vector that is not 16-byte aligned");
  return post_launch();
}

int mgcmt_block_project(mgcmt_plan* p, int l, int nb, const int* b_slots, const int* b_vecs, const int* ab_slots, const int* ab_vecs, int k,
                        const int* w_slots, const int* w_vecs, const int* aw_slots, const int* aw_vecs, double* coeffs_out, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_level(p, l));
  if (nb < 1 || nb > kBlockLockedMax || k < 1 || k > kBlockWideOut)
    return fail(MGCMT_ERR_INVALID, "block_project: 1..64 vectors B, 1..16 vectors W");
  if (!b_slots || !b_vecs || !w_slots || !w_vecs) return fail(MGCMT_ERR_INVALID, "block_project: non-null vector lists");
  const bool companions = ab_slots != nullptr;
  if ((ab_vecs != nullptr) != companions || (aw_slots != nullptr) != companions || (aw_vecs != nullptr) != companions)
    return fail(MGCMT_ERR_INVALID, "block_project: the companion lists AB and AW are given all four or not at all");
  double *b[kBlockLockedMax], *ab[kBlockLockedMax], *w[kBlockWideOut], *aw[kBlockWideOut];
  MG_TRY(wide_vectors(p, l, nb, b_slots, b_vecs, b));
  MG_TRY(wide_vectors(p, l, k, w_slots, w_vecs, w));
  if (companions) {
    MG_TRY(wide_vectors(p, l, nb, ab_slots, ab_vecs, ab));
    MG_TRY(wide_vectors(p, l, k, aw_slots, aw_vecs, aw));
  }
  for (int j = 0; j < k; ++j) {
    for (int i = 0; i < j; ++i)
      if (w[i] == w[j]) return fail(MGCMT_ERR_INVALID, "block_project: a vector W named twice");
    for (int i = 0; i < nb; ++i)
      if (b[i] == w[j] || (companions && ab[i] == w[j])) return fail(MGCMT_ERR_INVALID, "block_project: a vector W that is also a B or an AB");
  }
  for (int j = 0; companions && j < k; ++j) {
    for (int i = 0; i < j; ++i)
      if (aw[i] == aw[j]) return fail(MGCMT_ERR_INVALID, "block_project: a vector AW named twice");
    for (int i = 0; i < k; ++i)
      if (aw[j] == w[i]) return fail(MGCMT_ERR_INVALID, "block_project: a vector AW that is also a B, an AB or a W");
    for (int i = 0; i < nb; ++i)
      if (aw[j] == b[i] || aw[j] == ab[i]) return fail(MGCMT_ERR_INVALID, "block_project: a vector AW that is also a B, an AB or a W");
  }
  const long n = p->interior(l);
  const int tiles = (nb + 15) / 16;
  MG_TRY(wide_scratch(p, (size_t)tiles * block_pencil_blocks(n) * 256, S(stream)));
  if (!launch_block_project(S(stream), n, nb, b, companions ? ab : nullptr, k, w, companions ? aw : nullptr, p->d_wide_partials, p->d_wide_out))
    return fail(MGCMT_ERR_INVALID, "block_project: an odd number of points or a vector that is not 16-byte aligned");
  MG_TRY(post_launch());
  if (coeffs_out) {
    std::vector<double> packed((size_t)nb * kBlockWideOut);
    MG_HIP(hipMemcpyAsync(packed.data(), p->d_wide_out, sizeof(double) * packed.size(), hipMemcpyDeviceToHost, S(stream)));
    MG_HIP(hipStreamSynchronize(S(stream)));
    for (int i = 0; i < nb; ++i)
      for (int j = 0; j < k; ++j) coeffs_out[i * k + j] = packed[(size_t)i * kBlockWideOut + j];
  }
  return MGCMT_OK;
}

int mgcmt_block_orthonormalize(mgcmt_plan* p, int l, int k, const int* w_slots, const int* w_vecs, const int* aw_slots, const int* aw_vecs,
                               double drop_tol, double* t_out, unsigned* dropped_out, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_level(p, l));
  if (k < 1 || k > kBlockWideOut) return fail(MGCMT_ERR_INVALID, "block_orthonormalize: 1..16 vectors W");
  if (!w_slots || !w_vecs) return fail(MGCMT_ERR_INVALID, "block_orthonormalize: non-null vector lists");
  if ((aw_slots != nullptr) != (aw_vecs != nullptr))
    return fail(MGCMT_ERR_INVALID, "block_orthonormalize: the companion lists are given both or not at all");
  if (!(drop_tol > 0.0 && drop_tol < 1.0)) return fail(MGCMT_ERR_INVALID, "block_orthonormalize: drop_tol lies in (0, 1)");
  const bool companions = aw_slots != nullptr;
  double *w[kBlockWideOut], *aw[kBlockWideOut];
  MG_TRY(wide_vectors(p, l, k, w_slots, w_vecs, w));
  if (companions) MG_TRY(wide_vectors(p, l, k, aw_slots, aw_vecs, aw));
  for (int j = 0; j < k; ++j) {
    for (int i = 0; i < j; ++i)
      if (w[i] == w[j]) return fail(MGCMT_ERR_INVALID, "block_orthonormalize: a vector W named twice");
    for (int i = 0; companions && i < j; ++i)
      if (aw[i] == aw[j]) return fail(MGCMT_ERR_INVALID, "block_orthonormalize: a vector AW named twice");
    for (int i = 0; companions && i < k; ++i)
      if (aw[j] == w[i]) return fail(MGCMT_ERR_INVALID, "block_orthonormalize: a vector AW that is also a W");
  }
  const long n = p->interior(l);
  MG_TRY(wide_scratch(p, (size_t)block_pencil_blocks(n) * 256, S(stream)));
  if (!p->d_orth_mask) MG_HIP(hipMalloc((void**)&p->d_orth_mask, sizeof(unsigned)));
  if (!launch_block_orthonormalize(S(stream), n, k, w, companions ? aw : nullptr, drop_tol, p->d_wide_partials, p->d_wide_out, p->d_orth_mask))
    return fail(MGCMT_ERR_INVALID, "block_orthonormalize: an odd number of points or a vector that is not 16-byte aligned");
  MG_TRY(post_launch());
  if (t_out) {
    double packed[kBlockWideOut * kBlockWideOut];
    MG_HIP(hipMemcpyAsync(packed, p->d_wide_out, sizeof(packed), hipMemcpyDeviceToHost, S(stream)));
    MG_HIP(hipStreamSynchronize(S(stream)));
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < k; ++j) t_out[i * k + j] = packed[i * kBlockWideOut + j];
  }
  if (dropped_out) {
    MG_HIP(hipMemcpyAsync(dropped_out, p->d_orth_mask, sizeof(unsigned), hipMemcpyDeviceToHost, S(stream)));
    MG_HIP(hipStreamSynchronize(S(stream)));
  }
  return MGCMT_OK;
}

int mgcmt_axpy(mgcmt_plan* p, int l, double alpha, int x_slot, int x_vec, int y_slot, int y_vec, void* stream) {
  CarryKeep keep(p);
  keep.writes(l, y_slot, y_vec);
  MG_TRY(check_vec(p, l, x_slot, x_vec));
  MG_TRY(check_vec(p, l, y_slot, y_vec));
  MG_TRY(ensure_slot(p, l, x_slot));
  MG_TRY(ensure_slot(p, l, y_slot));
  launch_axpy(S(stream), p->interior(l), alpha, p->kvec(l, x_slot, x_vec).p, p->kvec(l, y_slot, y_vec).p);
  return post_launch();
}

int mgcmt_scale(mgcmt_plan* p, int l, double alpha, int slot, int vec, void* stream) {
  CarryKeep keep(p);
  keep.writes(l, slot, vec);
  MG_TRY(check_vec(p, l, slot, vec));
  MG_TRY(ensure_slot(p, l, slot));
  launch_scale(S(stream), p->interior(l), alpha, p->kvec(l, slot, vec).p);
  return post_launch();
}

int mgcmt_gramschmidt(mgcmt_plan* p, int l, int slot, int k, int modified, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_vec(p, l, slot, 0));
  MG_TRY(check_k(p, k));
  return gramschmidt_impl(p, l, slot, k, modified, S(stream));
}

int mgcmt_normalize(mgcmt_plan* p, int l, int slot, int k, void* stream) {
  entry_drops_carry(p);
  MG_TRY(check_vec(p, l, slot, 0));
  MG_TRY(check_k(p, k));
  MG_TRY(ensure_slot(p, l, slot));
  for (int i = 0; i < k; ++i) {
    double* a = p->kvec(l, slot, i).p;
    launch_dot_partials(S(stream), p->interior(l), a, a, 0, 1, p->d_partials);
    launch_scale_by_norm(S(stream), p->interior(l), p->d_partials, a);
  }
  return post_launch();
}

static int fused_pass_checked(mgcmt_plan* p, int l, int kind, int nsweep, double omega, int mode, int k, hipStream_t s, int reps) {
  MG_TRY(check_level(p, l));
  MG_TRY(check_k(p, k));
  if (!fused_level(p, l, kind)) return fail(MGCMT_ERR_UNSUPPORTED, "level / smoother not covered by the fused kernels");
  const int transfer = mode & 3, npre = (mode >> 4) & 3;
  if (nsweep < 1 || nsweep > pass_sweeps(p, l, kind, nsweep) || mode < 0 || mode > 63 || transfer == 3 || ((mode & 8) && transfer != 2) ||
      (npre && transfer != 1) || npre > fused_max_recompute(p->levels[l].dA.k, kind == MGCMT_GS_MC ? 1 : 0, nsweep) ||
      (transfer == 1 && (mode & 4) && !npre))
    return fail(MGCMT_ERR_INVALID, "bad nsweep or mode");
  if ((mode & 3) != 0 && l + 1 >= (int)p->levels.size()) return fail(MGCMT_ERR_INVALID, "no coarser level");
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_V));
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_F));
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_T));
  if ((mode & 3) != 0) {
    MG_TRY(ensure_slot(p, l + 1, MGCMT_SLOT_V));
    MG_TRY(ensure_slot(p, l + 1, MGCMT_SLOT_F));
  }
  for (int r = 0; r < reps; ++r) MG_TRY(fused_pass(p, l, kind, nsweep, omega, mode & 15, k, s, npre));
  return post_launch();
}

int mgcmt_fused_pass(mgcmt_plan* p, int l, int kind, int nsweep, double omega, int mode, int k, void* stream) {
  entry_drops_carry(p);
  MG_TRY(mgcmt::unsupported_3d(p, "mgcmt_fused_pass"));
  return fused_pass_checked(p, l, kind, nsweep, omega, mode, k, S(stream), 1);
}

int mgcmt_time_fused_pass(mgcmt_plan* p, int l, int kind, int nsweep, double omega, int mode, int reps, double* ms_out, void* stream) {
  entry_drops_carry(p);
  MG_TRY(mgcmt::unsupported_3d(p, "mgcmt_time_fused_pass"));
  if (!ms_out || reps < 1) return fail(MGCMT_ERR_INVALID, "bad arguments");
  MG_TRY(fused_pass_checked(p, l, kind, nsweep, omega, mode, 1, S(stream), 1));  // (allocations, occupancy query: untimed)
  hipEvent_t a, b;
  MG_HIP(hipEventCreate(&a));
  MG_HIP(hipEventCreate(&b));
  MG_HIP(hipEventRecord(a, S(stream)));
  const int rc = fused_pass_checked(p, l, kind, nsweep, omega, mode, 1, S(stream), reps);
  MG_HIP(hipEventRecord(b, S(stream)));
  MG_HIP(hipEventSynchronize(b));
  float ms = 0.f;
  MG_HIP(hipEventElapsedTime(&ms, a, b));
  *ms_out = (double)ms / reps;
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return rc;
}

int mgcmt_fused_max_sweeps(const mgcmt_plan* p, int l, int kind, int* max_sweeps) {
  MG_TRY(mgcmt::unsupported_3d(p, "mgcmt_fused_max_sweeps"));
  MG_TRY(check_level(p, l));
  if (!max_sweeps) return fail(MGCMT_ERR_INVALID, "null output");
  *max_sweeps = fused_level(p, l, kind) ? pass_sweeps(p, l, kind, 1 << 20) : 0;
  return MGCMT_OK;
}

int mgcmt_fused_max_recompute(const mgcmt_plan* p, int l, int kind, int nsweep, int* max_recompute) {
  MG_TRY(mgcmt::unsupported_3d(p, "mgcmt_fused_max_recompute"));
  MG_TRY(check_level(p, l));
  if (!max_recompute) return fail(MGCMT_ERR_INVALID, "null output");
  *max_recompute = fused_level(p, l, kind) ? fused_max_recompute(p->levels[l].dA.k, kind == MGCMT_GS_MC ? 1 : 0, nsweep) : 0;
  return MGCMT_OK;
}

int mgcmt_plan_set_option(mgcmt_plan* p, int option, int value) {
  entry_drops_carry(p);
  if (!p) return fail(MGCMT_ERR_INVALID, "null plan");
  p->carry_drop();  // (a carried right-hand side belongs to the options it was computed under)
  if (option == MGCMT_OPT_CARRY) {
    p->carry_opt = value < 0 ? 0 : (value > 2 ? 2 : (int)value);
    p->graphs_invalidate();
    return MGCMT_OK;
  }
  if (option == MGCMT_OPT_FUSED) {
    p->use_fused = value != 0;
    p->graphs_invalidate();
    return MGCMT_OK;
  }
  if (option == MGCMT_OPT_RECOMPUTE) {
    p->use_recompute = value != 0;
    p->force_recompute = value == 2;
    p->graphs_invalidate();
    return MGCMT_OK;
  }
  if (option == MGCMT_OPT_TWO_LEVEL) {
    p->two_level = value < 0 ? 0 : (value > 2 ? 2 : (int)value);
    p->graphs_invalidate();
    return MGCMT_OK;
  }
  if (option == MGCMT_OPT_PCG_MARCH) {
    p->pcg_march = value < 0 ? -1 : (value != 0 ? 1 : 0);
    return MGCMT_OK;
  }
  if (option == MGCMT_OPT_GRAPH) {
    p->use_graph = value != 0;
    return MGCMT_OK;
  }
  if (option == MGCMT_OPT_LEX_WAVE) {
    p->use_lex_wave = value < 0 ? 0 : (value > 2 ? 2 : (int)value);
    p->graphs_invalidate();
    return MGCMT_OK;
  }
  if (option == MGCMT_OPT_LEX_CHAIN) {
    p->lex_chain = value != 0;
    p->graphs_invalidate();
    return MGCMT_OK;
  }
  if (option == MGCMT_OPT_TAIL) {
    p->use_tail = value != 0;
    p->use_tail_dense = value != 2;  // 1 (default): the tail as one dense product; 2: as the LDS-resident launch of ~45 phases
    p->graphs_invalidate();
    return MGCMT_OK;
  }
  if (option == MGCMT_OPT_MGS_BLOCK) {
    p->use_mgs_block = value != 0;
    p->mgs_block_min = value > 1 ? (long)value : 0;  // (a value > 1: the blocked form from that many points on — tuning)
    p->graphs_invalidate();
    return MGCMT_OK;
  }
  if (option == MGCMT_OPT_FUSED_ROWS) {
    p->fused_rows = value;
    p->graphs_invalidate();
    return MGCMT_OK;
  }
  return fail(MGCMT_ERR_INVALID, "unknown option");
}

int mgcmt_carry_pending(const mgcmt_plan* p, int* pending) {
  if (!p || !pending) return fail(MGCMT_ERR_INVALID, "null argument");
  *pending = p->carry.valid ? 1 : 0;
  return MGCMT_OK;
}

int mgcmt_lex_wave_stats(mgcmt_plan* p, uint32_t* out, int64_t capacity) {
  entry_drops_carry(p);
  MG_TRY(mgcmt::unsupported_3d(p, "mgcmt_lex_wave_stats"));
  if (!p || !out) return fail(MGCMT_ERR_INVALID, "null argument");
  if (!p->lex_sync) return fail(MGCMT_ERR_INVALID, "no lexicographic wave sweep has run on this plan");
  const int64_t n = capacity < (int64_t)p->lex_sync_words ? capacity : (int64_t)p->lex_sync_words;
  MG_HIP(hipDeviceSynchronize());
  MG_HIP(hipMemcpy(out, p->lex_sync, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
  return MGCMT_OK;
}

int mgcmt_time_smoother(mgcmt_plan* p, int l, int kind, int nu, double omega, int reps, double* ms_out, void* stream) {
  entry_drops_carry(p);
  MG_TRY(mgcmt::unsupported_3d(p, "mgcmt_time_smoother"));
  MG_TRY(check_level(p, l));
  if (!ms_out || reps < 1) return fail(MGCMT_ERR_INVALID, "bad arguments");
  MG_TRY(unsupported_point_smoother(p, kind));
  hipEvent_t a, b;
  MG_HIP(hipEventCreate(&a));
  MG_HIP(hipEventCreate(&b));
  MG_HIP(hipEventRecord(a, S(stream)));
  for (int r = 0; r < reps; ++r) MG_TRY(smooth_impl(p, l, kind, nu, omega, 1, S(stream)));
  MG_HIP(hipEventRecord(b, S(stream)));
  MG_HIP(hipEventSynchronize(b));
  float ms = 0.f;
  MG_HIP(hipEventElapsedTime(&ms, a, b));
  *ms_out = (double)ms;
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return MGCMT_OK;
}

int mgcmt_bandwidth_probe(mgcmt_plan* p, int l, int kind, int blocks, int reps, double* ms_out, void* stream) {
  entry_drops_carry(p);
  MG_TRY(mgcmt::unsupported_3d(p, "mgcmt_bandwidth_probe"));
  MG_TRY(check_level(p, l));
  if (!ms_out || reps < 1 || blocks < 1 || kind < 0 || (kind > 17 && (kind < 20 || kind > 23))) return fail(MGCMT_ERR_INVALID, "bad arguments");
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_V));
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_F));
  MG_TRY(ensure_slot(p, l, MGCMT_SLOT_T));
  const long n = p->interior(l) & ~1L;
  hipEvent_t a, b;
  MG_HIP(hipEventCreate(&a));
  MG_HIP(hipEventCreate(&b));
  auto go = [&]() {
    if (kind >= 20) launch_probe_issue(S(stream), kind - 20, 20000, blocks, p->kvec(l, MGCMT_SLOT_T).p);  // 64 x 20000 instructions per wave
    else if (kind <= 2) launch_probe(S(stream), kind, n, p->kvec(l, MGCMT_SLOT_V).p, p->kvec(l, MGCMT_SLOT_F).p, p->kvec(l, MGCMT_SLOT_T).p, blocks);
    else  // marching pattern: `blocks` = rows per chunk
      // (kind - 3) % 3: one read stream / two read streams / two reads + one write; (kind - 3) / 3: columns a wave
      // writes out of the 128 it reads: 128 (no overlap), 124 (unaligned), 112 (the fused kernels' geometry), 96
      launch_probe_march(S(stream), p->levels[l].nr, p->levels[l].gc, blocks, (kind - 3) % 3 == 0 ? 1 : 2, (kind - 3) % 3 == 2 ? 1 : 0,
                         (kind - 3) / 3 == 0 ? 128 : ((kind - 3) / 3 == 1 ? 124 : ((kind - 3) / 3 == 2 ? 112 : ((kind - 3) / 3 == 3 ? 96 : 120))), p->kvec(l, MGCMT_SLOT_V).p,
                         p->kvec(l, MGCMT_SLOT_F).p, p->kvec(l, MGCMT_SLOT_T).p);
  };
  go();
  MG_HIP(hipEventRecord(a, S(stream)));
  for (int r = 0; r < reps; ++r) go();
  MG_HIP(hipEventRecord(b, S(stream)));
  MG_HIP(hipEventSynchronize(b));
  float ms = 0.f;
  MG_HIP(hipEventElapsedTime(&ms, a, b));
  *ms_out = (double)ms / reps;
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return post_launch();
}

}  // extern "C"
