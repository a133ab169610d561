// Internal declarations shared by the kernel files and the plan/driver of libmgcmt_hip.so.
// Not part of the ABI (the ABI is include/mgcmt_hip.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mgcmt_hip.h"

namespace mgcmt {

constexpr int kHalo = MGCMT_HALO_ROWS;
constexpr int kMaxTerms = MGCMT_MAX_TERMS;
constexpr int kMaxVec = 32;  // upper bound on simultaneous vectors of one launch
constexpr int kMaxStoreVec = MGCMT_MAX_STORE_VEC;  // ... and on the vectors a plan keeps per slot (only the block entries see those beyond kMaxVec)

// KOp::point / K3Op::point: the kind of per-point part a level has on top of its Kronecker terms (the layouts: see the structs)
constexpr int kPointNone = 0, kPointDiag = 1, kPointPlanes = 2, kPointBonds = 3;

// Operator of one level as the kernels see it:  A = sum_m X_m (x) Y_m  (shift applied separately).
// X[m] / Y[m] point at element 0 of the `lower` array; `diag` is at +ldx, `upper` at +2*ldx.
// Row factors are stored with the level's halo count of entries before element 0 and after element nr-1 (the local
// strip's halo rows; zero outside the global grid), column factors span the whole row.
struct KOp {
  int nterms;
  int five_point;  // 1: c0/cn/cw below are valid (constant 5-point / 3-point operator)
  const double* X[kMaxTerms];
  const double* Y[kMaxTerms];
  long ldx, ldy;
  double c0, cn, cw;  // centre, row-neighbour, column-neighbour coefficient (five_point only)
  // nine_const: every factor is Toeplitz except its last diagonal entry (Galerkin levels of a constant
  // operator): interior coefficients c9[di+1][dj+1], own-row coefficients on the last row, centre-column
  // coefficients on the last column, and the corner's diagonal
  int nine_const;
  double c9[3][3], c9row[3], c9col[3], c9corner;
  // nine_var: some terms are Toeplitz-but-last (their sum is c9 / c9row / c9col / c9corner as above), ONE term has
  // arbitrary tridiagonal factors vX, vY ([lower | diag | upper], leading dimensions ldx / ldy) — the Galerkin levels of
  // a constant operator plus a product potential (square well, PotWellSolver.py:150-153 carried to 2-D)
  int nine_var;
  const double* vX;
  const double* vY;
  // five_diag: a constant 5-point part (c0/cn/cw) plus ndiag (1 or 2) terms whose factors are both diagonal — a
  // product potential p(i) q(j) on top of a scaled Laplacian (square well): dX[m][row], dY[m][col] are the diagonals
  int five_diag, ndiag;
  const double* dX[2];
  const double* dY[2];
  // 1-D levels: all terms folded into ONE tridiagonal  T = sum_m x_m Y_m  (X_m is 1 x 1): tri = [lower | diag | upper], n
  // numbers each; tri_const: Toeplitz except for its last diagonal entry (the Laplacian and its Galerkin coarsenings)
  int one_d, tri_const;
  const double* tri;
  double t_lo, t_di, t_up, t_last;
  // point: a per-point part on top of the Kronecker terms above (mgcmt_plan_create_pot; 2-D, whole grids).  1: a diagonal
  // D(i, j) = pg[i * pld + j] (the fine level, stored in the level's padded row layout); 2: a 9-point stencil G (the
  // Galerkin levels R D P): the coefficient of v(i + a - 1, j + b - 1) in row (i, j) is pg[(3 a + b) * pplane + i * pld + j],
  // zero towards points outside the grid.  3: a diagonal and bonds (mgcmt_plan_create_bonds; the fine level): three planes
  // in the level's padded row layout, pplane apart — D(i, j) = pg[i * pld + j], E(i, j) = pg[pplane + ...] added to the
  // entry between (i, j) and (i, j + 1), S(i, j) = pg[2 * pplane + ...] to the one between (i, j) and (i + 1, j); the
  // halo rows of every plane are zero, so S(-1, j) reads an exact zero; E(i, nc - 1) = S(nr - 1, j) = 0.  pmarch: which
  // passes of such a level take the marching kernels where its size allows — bit 0 the parity stages and residual +
  // restriction, bit 1 the Jacobi sweep and the applied operator (MGCMT_BONDS_MARCH, read at plan creation: hierarchy.hip).
  // The flags above describe the Kronecker part alone.  Level 0 of mgcmt_plan_create_nine is a point == 2 level too (the
  // caller's nine planes); on a point == 2 level pmarch is the set of passes (kNine* below) that take the tile kernels of
  // kernels_nine_tile.hip where the level's size allows (MGCMT_NINE_TILE, read at plan creation: hierarchy.hip).
  int point, pmarch;
  const double* pg;
  long pld, pplane;
};

// Operator of a 3-D level (kernels_3d.hip):  A = sum_m X_m (x) Y_m (x) Z_m  over z, y, x (shift applied separately).
// X[m] / Y[m] / Z[m] point at [lower | diag | upper] of n entries each (no halo).  seven: constant 7-point operator
// (centre c0, one coefficient per direction and side) — the fine level of a scaled / shifted Laplacian.
struct K3Op {
  int nterms;
  long n;  // points per axis
  const double* X[kMaxTerms];
  const double* Y[kMaxTerms];
  const double* Z[kMaxTerms];
  int seven;
  double c0, czm, czp, cym, cyp, cxm, cxp;
  // point: a per-point part on top of the Kronecker terms above (mgcmt_plan_create3d_pot; kernels_3d_point.hip).  1: a
  // diagonal D(z, y, x) = pg[idx] (the fine level, g^3 numbers at the index of the right-hand side); 2: a 27-point stencil G
  // (the Galerkin levels R D P): the coefficient of v(z + a - 1, y + b - 1, x + c - 1) in row idx is
  // pg[(9 a + 3 b + c) * pplane + idx], zero towards points outside the grid.  The flags above describe the Kronecker part
  // alone.  3: a diagonal and bonds (mgcmt_plan_create3d_bonds; the fine level): four planes of g^3 numbers, pplane apart, no
  // halo — D = pg[idx], Bx = pg[pplane + idx] added to the two entries between (z, y, x) and (z, y, x + 1),
  // By = pg[2 pplane + idx] towards (z, y + 1, x), Bz = pg[3 pplane + idx] towards (z + 1, y, x);
  // Bx(x = n - 1) = By(y = n - 1) = Bz(z = n - 1) = 0, a bond read at x - 1 < 0 etc. is a predicated zero.
  // pmarch: the set of passes (kMarch3*) of a fine level, 1 or 3, that take the marching kernels where the level's Kronecker
  // part and size allow (point3_marching; MGCMT_3D_POINT_MARCH, read at plan creation: hierarchy.hip).  Level 0 of
  // mgcmt_plan_create3d_stencil is a point == 2 level too (the caller's 27 planes); on a point == 2 level pmarch is the set of
  // passes (kStencil3* below) that take the kernels of kernels_3d_stencil.hip where the level's size allows
  // (stencil3_tiled; MGCMT_3D_STENCIL_TILE, read at plan creation: hierarchy.hip).
  int point, pmarch;
  const double* pg;
  long pplane;
};

// A batch of vectors on one level: interior pointer of vector 0, elements between vectors.
struct KVec {
  double* p;
  long stride;
};

struct KGrid {
  long nr, nc;       // local rows (strip), columns
  int coarsen_rows;  // 1 for 2-D (rows are coarsened too), 0 for 1-D
};

// ---- kernel launchers (kernels_*.hip) --------------------------------------------------------
// All take the number of vectors k (grid z) and a device pointer to the k shifts.

void launch_apply(hipStream_t s, KGrid g, KOp op, KVec src, KVec dst, const double* shifts, int k);
// <x,x>, <x,w>, <w,w>, <x,A w>, <w,A w> in one pass over x and w (nothing stored): true when the level's operator is
// covered (2-D 5-point, with or without a product potential); out[0..4] on the device, partials: 5 * 8192 doubles
bool launch_ritz_pair(hipStream_t s, KGrid g, KOp op, const double* x, const double* w, double* partials, double* out);
void launch_final_sums(hipStream_t s, int nq, int nblocks, const double* partials, double* out);
void launch_wjacobi(hipStream_t s, KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k);
void launch_mc_colour(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, const double* shifts, double omega, int ca, int cb, int k);
void launch_residual(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, KVec r, const double* shifts, int k);
void launch_restrict(hipStream_t s, KGrid fine, KGrid coarse, KVec r, KVec rc, int k);
void launch_prolong(hipStream_t s, KGrid fine, KGrid coarse, KVec e, KVec v, int accumulate, int k);
// the same four for an operator with a per-point part (op.point; kernels_pointwise.hip) — the launchers above hand over —,
// its entries added into the assembled band matrix of the coarsest level, and the Galerkin product of the per-point part:
// coarse <- R G P for the nine planes (fine_planes = 9) or the diagonal (fine_planes = 1) of a fnr x fnc level, with the
// transfers of launch_restrict / launch_prolong; the coarse level always has nine planes
void launch_point_apply(hipStream_t s, KGrid g, KOp op, KVec src, KVec dst, const double* shifts, int k);
void launch_point_wjacobi(hipStream_t s, KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k);
void launch_point_mc_colour(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, const double* shifts, double omega, int ca, int cb, int k);
void launch_point_residual(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, KVec r, const double* shifts, int k);
struct KBand;
void launch_point_band_add(hipStream_t s, KGrid g, KOp op, const KBand& b, int k);
void launch_point_coarsen(hipStream_t s, long fnr, long fnc, const double* fine, int fine_planes, long fld, long fplane, double* coarse, long cld,
                          long cplane);
// a level with per-point bonds (op.point == kPointBonds) as a row march (kernels_bonds.hip; bonds_marching: a constant 5-point
// Kronecker part, at least 128 columns, even sizes, marching not switched off).  Every launcher returns false — nothing
// launched — where the level or the vectors' alignment rule the march out; the flat kernels above take the level then.
// parity: 1 = the colours (0,1), (1,0) of the multicolour order, 0 = (0,0), (1,1) — two launches are one sweep.
// launch_bonds_residual_restrict: fc <- R (f - (A - mu) v) in one pass (the fine residual is not stored); vc.p != null: vc <- 0.
bool bonds_marching(const KGrid& g, const KOp& op);
bool launch_bonds_apply(hipStream_t s, KGrid g, KOp op, KVec src, KVec dst, const double* shifts, int k);
bool launch_bonds_wjacobi(hipStream_t s, KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k);
bool launch_bonds_parity(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, const double* shifts, double omega, int parity, int k);
bool launch_bonds_residual_restrict(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, KVec fc, KVec vc, const double* shifts, int k);
// a nine-plane level (op.point == kPointPlanes) on the tile kernels (kernels_nine_tile.hip): a workgroup stages v on its tile plus the
// stages' rings in LDS, runs every stage there and stores the tile — out of place, vin -> vout, nothing between workgroups.
// nine_tiled: the passes (kNine* bits of op.pmarch) that tile on this level — at least 128 columns, rows coarsened — or 0; a
// launcher returns false, nothing launched, where its pass stays flat.  launch_nine_wjacobi: nsweep = 1 or 2 weighted-Jacobi
// sweeps in one launch; launch_nine_colour: one whole four-colour sweep (0,1), (1,0), (0,0), (1,1);
// launch_nine_residual_restrict: fc <- R (f - (A - mu) v) in one pass (even sizes; the fine residual is not stored), vc.p != null:
// vc <- 0.  The launch_point_* forms are what the cycle calls: they pick the level's own kernels (bonds or nine planes).
constexpr int kNineColour = 1, kNineJacobi = 2, kNineResidual = 4;
int nine_tiled(const KGrid& g, const KOp& op);
bool launch_nine_wjacobi(hipStream_t s, KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int nsweep, int k);
bool launch_nine_colour(hipStream_t s, KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k);
bool launch_nine_residual_restrict(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, KVec fc, KVec vc, const double* shifts, int k);
bool launch_point_wjacobi_pair(hipStream_t s, KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k);
bool launch_point_mc_sweep(hipStream_t s, KGrid g, KOp op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k);
bool launch_point_residual_restrict(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, KVec fc, KVec vc, const double* shifts, int k);
// generalised lexicographic sweep (in place):
//   v_k <- (alpha d_k v_k + beta f_k - wU sum_{j>k} a_kj v_j - wL sum_{j<k} a_kj v_j^new) / d_k
void launch_lex_sweep(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, const double* shifts, double alpha, double beta,
                      double wU, double wL, int k);

// the same sweep as a pipeline of waves over the whole chip (kernels_lexwave.hip; constant-coefficient operators on
// grids of at least 16 x 16 points).  carry: k * lex_wave_blocks(g) * g.nr * 4 eight-byte granules; sync: 2 words; sync[1]
// != 0 after the sweep: a block gave up waiting (reported by the next synchronising call)
bool lex_wave_supported(const KGrid& g, const KOp& op);
long lex_wave_blocks(const KGrid& g);
long lex_wave_carry(const KGrid& g, int k, int nsweeps);  // granules of `carry` for k vectors and nsweeps chained sweeps
void launch_lex_wave(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, const double* shifts, double alpha, double beta, double wU,
                     double wL, int k, double* carry, unsigned* sync, int nsweeps, double gamma);
// ... and as a wavefront over bands of 63 rows (kernels_lexband.hip; same operators and grids).  carry: k *
// lex_band_count(g) * lex_band_stride(g) eight-byte granules; sync as above
long lex_band_count(const KGrid& g);
long lex_band_stride(const KGrid& g);
void launch_lex_band(hipStream_t s, KGrid g, KOp op, KVec v, KVec f, const double* shifts, double alpha, double beta, double wU,
                     double wL, int k, double* carry, unsigned* sync);

// fused row-streaming passes (fused_kernel.h, kernels_fused*.hip): vin -> vout with nsweep sweeps of weighted
// Jacobi or multicolour Gauss-Seidel.  mode & 3: 0 plain, 1 prolong+correct first (coarse = correction), 2
// residual+restrict last (coarse = right-hand side); mode & 4: vin is zero; mode & 8: vout is not written (mode 2);
// npre: pre-smoothing sweeps recomputed in front of the correction (mode 1)
bool fused_supported(const KGrid& g, const KOp& op);
// the 1-D form (kernels_fused1d.hip): a wave takes a window of 128 points through every stage in registers
bool fused1d_supported(const KGrid& g, const KOp& op);
int fused1d_max_sweeps(int multicolour);
int fused1d_max_recompute(int multicolour, int nsweep);
void launch_fused1d(hipStream_t s, KGrid g, KOp op, KVec vin, KVec f, KVec vout, KVec coarse, long coarse_nc, const double* shifts,
                    double omega, int multicolour, int nsweep, int mode, int npre, int k);
int fused_max_sweeps(const KOp& op, int multicolour);
int fused_max_recompute(const KOp& op, int multicolour, int nsweep);
// rows_override: rows per wave chunk (0 = automatic); [out_lo, out_hi): the local rows this launch produces (even
// bounds; the whole strip is 0 .. g.nr) — a sharded pass runs its boundary rows first so that their exchange overlaps
void launch_fused(hipStream_t s, KGrid g, KOp op, KVec vin, KVec f, KVec vout, KVec coarse, long coarse_nc, const double* shifts,
                  double omega, int multicolour, int nsweep, int mode, int npre, long row_lo, long row_hi, long last_row, int k,
                  long rows_override = 0, long out_lo = 0, long out_hi = -1, long out_lo2 = 0, long out_hi2 = 0);

// two-level fused passes (fused2_kernel.h, kernels_fused2_op5.hip): a constant 5-point level (op0, nr x nc, weighted
// Jacobi) and its Galerkin coarsening (op1, nine_const, cnr x cnc) in one launch; level l+2 has c2nc columns.
// up = 0: nf sweeps from v (zero_in: v is zero) -> residual -> F[l+1] (f1) -> 2 sweeps of level l+1 from zero ->
// residual -> F[l+2] (c2).  up = 1: level l+1 recomputes its 2 pre-sweeps from zero, adds P V[l+2] (c2), 2 sweeps;
// level l recomputes nf pre-sweeps from v, adds P of that, 2 sweeps -> vout.  V[l+1] is neither read nor written.
// fcarry (up = 1, zero_in = 0 only; null: none): the carrying up pass — behind vout it runs nf sweeps, the residual and
// the restriction on the rows it holds, and writes what the next cycle's down pass would write to F[l+1] to fcarry
// (same layout as f1, a different buffer: f1 is read by the same launch).
void launch_fused2(hipStream_t s, int up, int nf, int zero_in, const KOp& op0, const KOp& op1, long nr, long nc, long cnr, long cnc,
                   long c2nc, KVec v, KVec f, KVec vout, KVec f1, KVec c2, const double* shifts, double omega, int k, long rows_override,
                   double* fcarry = nullptr);

// vector algebra; scalar results / inputs live in device memory so nothing syncs with the host
void launch_fill(hipStream_t s, double* p, long n, double value);
// y += (alpha_scale * alpha_dev[0] / (den_dev ? den_dev[0] : 1)) * x ;  x /= (use_sqrt ? sqrt(s_dev[0]) : s_dev[0])
void launch_axpy_dev(hipStream_t s, long n, const double* alpha_dev, const double* den_dev, double alpha_scale, const double* x, double* y);
void launch_scale_dev(hipStream_t s, long n, const double* s_dev, int use_sqrt, double* x);
void launch_axpy(hipStream_t s, long n, double alpha, const double* x, double* y);
void launch_scale(hipStream_t s, long n, double alpha, double* x);
// streaming probes: kind 0 copy (a -> out), 1 triad (a + s b -> out), 2 read-only (a)
void launch_probe(hipStream_t s, int kind, long n, const double* a, const double* b, double* out, int blocks);
// the fused kernels' access pattern alone (128-column windows marching down `rows` rows): kind 3 read 1 stream,
// 4 read 2 streams, 5 read 2 + write 1; 6/7/8: the same with overlapping unaligned windows (124 of 128 columns kept)
void launch_probe_march(hipStream_t s, long nr, long nc, long rows, int nstreams, int do_write, int wout, const double* a, const double* b, double* out);
// out[q] = <x, y_q> for q < nq (y_q = y + q*ystride), deterministic two-pass reduction; `partials`
// holds at least nq * reduce_blocks(n) doubles
int reduce_blocks(long n);
void launch_dots(hipStream_t s, long n, const double* x, const double* y, long ystride, int nq, double* partials, double* out);
// Gram-Schmidt building blocks that consume the first reduction pass directly (no separate final pass / no scalar
// round trip): x /= sqrt(sum partials);  a_j -= (<q,a_j>/<q,q>) q for nj columns in one launch
void launch_dot_partials(hipStream_t s, long n, const double* x, const double* y, long ystride, int nq, double* partials, const double* gate = nullptr);
void launch_scale_by_norm(hipStream_t s, long n, const double* partials, double* x);
void launch_project_out(hipStream_t s, long n, const double* partials, const double* q, double* a_first, long astride, int nj);
constexpr int kGramMaxVectors = 6;
constexpr int kBlockMaxA = 12, kBlockMaxB = 4;  // block operations: up to 12 x 4 vectors (three blocks of four trial vectors)
void launch_probe_issue(hipStream_t s, int what, int iters, int blocks, double* sink);  // kinds 20..23 of mgcmt_bandwidth_probe
void launch_block_gram(hipStream_t s, long n, const double* const* a, int na, const double* const* b, int nb, double* partials, double* out);
void launch_block_combine(hipStream_t s, long n, const double* const* in, int nin, double* const* out, int nout, const double* c);
// wide block operations (kernels_blockwide.hip): the pencil of up to 48 vectors on the matrix cores, OUT = IN C for 48 -> 16
constexpr int kBlockWideMax = MGCMT_BLOCK_WIDE_MAX, kBlockWideOut = MGCMT_BLOCK_WIDE_OUT;
int block_pencil_blocks(long n);
int block_pencil_tiles(int m, bool mass);
long block_wide_table_words();
bool launch_block_pencil(hipStream_t s, long n, int m, const double* const* sv, const double* const* as, const double* const* ms, double* partials,
                         double* out);
bool launch_block_combine_wide(hipStream_t s, long n, const double* const* in, int nin, double* const* out, int nout, const double* c,
                               unsigned long long* table);
constexpr int kBlockLockedMax = MGCMT_BLOCK_LOCKED_MAX;  // vectors a block is deflated against (mgcmt_block_deflate)
bool launch_block_deflate(hipStream_t s, long n, int nq, const double* const* q, int k, double* const* w, double* partials, double* out);
// dst = sum_t w[t] x_t^2, nq <= kBlockLockedMax (mgcmt_block_density); max_blocks > 0: the grid's limit in place of the default
bool launch_block_density(hipStream_t s, long n, int nq, const double* const* x, const double* w, double* dst, int max_blocks);
// Anderson mixing (kernels_mix.hip; mgcmt_mix_residual, mgcmt_mix_combine): up to kMixMax pairs (x_i, r_i)
constexpr int kMixMax = MGCMT_MIX_MAX;
int mix_slices(long n);  // partial sums per result of the residual pass (partials: (kMixMax + 1) * mix_slices(n) doubles)
bool launch_mix_residual(hipStream_t s, long n, const double* out, const double* in, double* r, int nprev, const double* const* prev, double* partials,
                         double* results, int max_blocks);
bool launch_mix_combine(hipStream_t s, long n, int p, const double* const* x, const double* const* r, const double* alpha, double beta, double* dst,
                        int max_blocks);
// the same with companions (mgcmt_block_project), and one Cholesky-QR step on k <= 16 vectors (mgcmt_block_orthonormalize)
bool launch_block_project(hipStream_t s, long n, int nb, const double* const* b, const double* const* ab, int k, double* const* w, double* const* aw,
                          double* partials, double* out);
bool launch_block_orthonormalize(hipStream_t s, long n, int k, double* const* w, double* const* aw, double drop_tol, double* partials, double* table,
                                 unsigned* mask);
void launch_gram(hipStream_t s, long n, const double* const* v, int nv, double* partials, double* out);
void launch_lincomb(hipStream_t s, long n, const double* const* v, const double* c, int nt, double* dst);
bool mgs_small_fits(long n);

// Rayleigh-quotient minimisation as two passes per step (kernels_rq.hip); state: rq_state_words() doubles on the device,
// partials: at least 8 * 4096 doubles.  init: 1 = the initial pair (p = 0: rho and g of the start vector), 2 = the first
// step (p = -g, p_old not read), 0 = a step.  launch_rq_pass1 ends with the step's scalars (delta, rho of x + delta p);
// launch_rq_pass2 returns the number of partial sums per result for launch_rq_scalars2 (rho, beta), which the caller
// runs after <g, M g> is in state[rq_word_gmg()] when M is not the identity.
int rq_state_words();
int rq_word_rho();
int rq_word_gmg();
void launch_rq_pass1(hipStream_t s, KGrid g, KOp A, KOp Mo, int m_identity, const double* x, const double* gv, const double* pold, double* pnew,
                     double* state, int init, int robust, double* partials);
int launch_rq_pass2(hipStream_t s, KGrid g, KOp A, KOp Mo, int m_identity, const double* x, const double* p, double* xnew, double* gout, double* state,
                    int init, double* partials);
bool launch_rq_gmg(hipStream_t s, KGrid g, KOp Mo, const double* gv, double* partials, int nblocks);
// the whole rqmin call (initial pair + nu steps) in one single-workgroup launch where the level is small enough; false: not taken
bool launch_rq_small(hipStream_t s, KGrid g, KOp A, KOp Mo, int m_identity, double* x, double* p, double* gv, double* state, int nu, int robust);
// m_identity: 1 = M is the identity, 0 = <g, M g> is in state[rq_word_gmg()], 2 = it is result 3 of the partial sums (launch_rq_gmg)
// the scalars of pass 1 alone (the kernel launch_rq_pass1 ends with), behind the 3-D passes
void launch_rq_scalars1(hipStream_t s, const double* partials, int nblocks, double* state, int init, int robust);
void launch_rq_scalars2(hipStream_t s, const double* partials, int nblocks, double* state, int m_identity, int init);

// the levels of at most 32 x 32 points of a V-cycle in one launch (kernels_tail.hip)
constexpr int kTailMaxLevels = 6;
struct TailArgs {
  int g0, nlev, nterms;       // entry grid (g0 x g0), number of levels, Kronecker terms per level
  const double* X[kTailMaxLevels][kMaxTerms];
  const double* Y[kTailMaxLevels][kMaxTerms];
  long ldx[kTailMaxLevels], ldy[kTailMaxLevels];
  const double* f_in;         // entry level right-hand side (vector 0), vstride between vectors
  double* v_out;              // entry level result
  long vstride;
  const double* inv;          // explicit inverse of the coarsest (A - mu I), one n x n block per vector
  long inv_stride;
  const double* shifts;
  double omega;
  int kind, nu;               // smoother and sweeps (pre and post) on every tail level
  int unit_rhs, unit_q;       // launch_tail_matrix: block b runs on the unit vector e_b with vector unit_q's shift and inverse
};
bool tail_fits(long g0, int nlev, int nterms);
void launch_tail(hipStream_t s, const TailArgs& a, int k);
// The tail is linear in its right-hand side for fixed (shift, smoother, nu, omega): its matrix, formed once per shift set
// by running the tail on the unit vectors, turns the ~45 barrier-separated phases into one dense product.
bool tail_dense_fits(long g0);
void launch_tail_matrix(hipStream_t s, TailArgs a, int q, double* mt);
void launch_tail_dense(hipStream_t s, long g0, const double* mt, long mt_stride, const double* f_in, double* v_out, long vstride, int k);
void launch_mgs_small(hipStream_t s, long n, double* a0, long stride, int k);
// nb_in: partial sums per result in partials_in (0 = reduce_blocks(n), what the previous step left; 1 = already summed)
void launch_mgs_step(hipStream_t s, long n, const double* partials_in, double* u, long stride, int m, double* partials_out, int nb_in = 0,
                     const double* gate = nullptr);
// modified Gram-Schmidt of up to mgs_block_max() long columns in two passes over the data (Gram matrix, its factor, Q = A R^-1),
// with a gate word (cf[mgs_block_gate_word()]: 0 = done) for the column-by-column launches behind it: kernels_blas.hip
int mgs_block_max();
int mgs_block_words();
int mgs_block_gate_word();
void launch_mgs_blocked(hipStream_t s, long n, double* a0, long stride, int k, double* partials, double* cf);
// its three launches one by one (a sharded plan all-reduces the Gram matrix between the first two): per-block partial sums
// (returns the number of blocks), the factor from `nblocks` partial sums per entry, Q = A R^-1
int launch_mgs_gram(hipStream_t s, long n, const double* a0, long stride, int k, double* partials);
void launch_mgs_factor(hipStream_t s, const double* partials, int nblocks, int k, double* cf);
void launch_mgs_apply(hipStream_t s, long n, double* a0, long stride, int k, const double* cf);

// banded LU of (A - mu I) on the coarsest level and its solves (one workgroup per vector)
struct KBand {
  long n;        // unknowns
  int kl;        // half bandwidth
  int width;     // stored entries per row: 3*kl + 1
  double* ab;    // [k][n][width]
  int* piv;      // [k][n]
  long ab_stride, piv_stride;
};
void launch_band_assemble(hipStream_t s, KGrid g, KOp op, const double* shifts, KBand b, int k);
void launch_band_factor(hipStream_t s, KBand b, int k);
void launch_band_solve(hipStream_t s, KBand b, KVec rhs, KVec x, int k);
// explicit inverse (n <= 1024 unknowns) and the dense solve x = inv * rhs that replaces the substitutions
void launch_band_invert(hipStream_t s, KBand b, double* inv, long inv_stride, int k);
void launch_dense_solve(hipStream_t s, long n, const double* inv, long inv_stride, KVec rhs, KVec x, int k);

// 3-D levels (kernels_3d.hip): g^3 points, idx = z g^2 + y g + x; vectors as for the flat kernels (interior pointer, stride)
void launch3_apply(hipStream_t s, const K3Op& op, KVec src, KVec dst, const double* shifts, int k);
void launch3_wjacobi(hipStream_t s, const K3Op& op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k);
// one multicolour sweep in place: colours (z%2, y%2, x%2) in the order (0,0,1), (0,1,0), (1,0,0), (1,1,1), (0,0,0), (0,1,1),
// (1,0,1), (1,1,0) (two parity stages on a 7-point operator, which is the same sweep)
void launch3_mc_sweep(hipStream_t s, const K3Op& op, KVec v, KVec f, const double* shifts, double omega, int k);
// fc <- R (f - (A - mu) v), vc <- 0 (one pass; the fine residual is not stored)
void launch3_residual_restrict(hipStream_t s, const K3Op& op, KVec v, KVec f, KVec fc, KVec vc, const double* shifts, int k);
void launch3_restrict(hipStream_t s, const K3Op& fine, KVec src, KVec dst, int k);
void launch3_prolong(hipStream_t s, long n, KVec e, KVec dst, int accumulate, int k);
// vout <- one weighted-Jacobi sweep from w = vin + P e (w is not stored)
void launch3_prolong_jacobi(hipStream_t s, const K3Op& op, KVec e, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k);
void launch3_band_assemble(hipStream_t s, const K3Op& op, const double* shifts, KBand b, int k);
// the same for a level with a per-point part (op.point; kernels_3d_point.hip) — the launchers above hand over —: flat
// kernels for the 27-plane Galerkin levels, flat and marching ones for the constant 7-point fine level with a diagonal or with bonds; the
// per-point entries added into the assembled band matrix of the coarsest level; and the Galerkin product of the per-point
// part: coarse <- R G P for the 27 planes (fine_planes = 27), the diagonal (fine_planes = 1) or the planes D, Bx, By, Bz
// (fine_planes = 4) of a level of fn^3 points
// point3_marching: the passes (kMarch3* bits of op.pmarch) that march on this level — a constant 7-point Kronecker part with
// a diagonal or with bonds, n a multiple of 64 — or 0; the other passes, and apply, run the flat kernels.
constexpr int kMarch3Jacobi = 1, kMarch3Parity = 2, kMarch3Residual = 4, kMarch3Prolong = 8;
int point3_marching(const K3Op& op);
void launch3p_apply(hipStream_t s, const K3Op& op, KVec src, KVec dst, const double* shifts, int k);
void launch3p_wjacobi(hipStream_t s, const K3Op& op, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k);
void launch3p_mc_sweep(hipStream_t s, const K3Op& op, KVec v, KVec f, const double* shifts, double omega, int k);
void launch3p_residual_restrict(hipStream_t s, const K3Op& op, KVec v, KVec f, KVec fc, KVec vc, const double* shifts, int k);
void launch3p_prolong_jacobi(hipStream_t s, const K3Op& op, KVec e, KVec vin, KVec f, KVec vout, const double* shifts, double omega, int k);
void launch3p_band_add(hipStream_t s, const K3Op& op, const KBand& b, int k);
void launch3p_coarsen(hipStream_t s, long fn, const double* fine, int fine_planes, long fplane, double* coarse, long cplane);
// a 27-plane level (op.point == kPointPlanes) on the kernels of kernels_3d_stencil.hip.  stencil3_tiled: the passes (kStencil3*
// bits of op.pmarch) that take them on this level — n a multiple of 64 — or 0; a launcher returns false, nothing launched, where
// its pass stays flat.  launch3n_colour: one stage (cz, cy, cx) of the eight-colour sweep in place, launched on the n^3 / 8
// points of its colour only; launch3n_residual_restrict: fc <- R (f - (A - mu) v), vc <- 0, a workgroup per tile of coarse
// columns and chunk of coarse planes, every fine residual formed once (LDS).  Both give the bits of their flat form.
constexpr int kStencil3Colour = 16, kStencil3Residual = 32;
int stencil3_tiled(const K3Op& op);
bool launch3n_colour(hipStream_t s, const K3Op& op, KVec v, KVec f, const double* shifts, double omega, int cz, int cy, int cx, int k);
bool launch3n_residual_restrict(hipStream_t s, const K3Op& op, KVec v, KVec f, KVec fc, KVec vc, const double* shifts, int k);

// Rayleigh-quotient passes on 3-D levels (kernels_rq3d.hip), the protocol of launch_rq_pass1 / launch_rq_pass2 /
// launch_rq_scalars2 and the same state words: pass 1 ends with the step's scalars; pass 2 returns the number of partial
// sums per result; with M != I, launch_rq3_gmg puts <g, M g> into result 3 of them (then m_identity = 2 for
// launch_rq_scalars2).  launch_rq3_small: the whole call in one launch on levels of at most 16^3 points (false: not taken).
bool rq3_marching(const K3Op& A, int m_identity);
void launch_rq3_pass1(hipStream_t s, const K3Op& A, const K3Op& Mo, int m_identity, const double* x, const double* gv, const double* pold, double* pnew,
                      double* state, int init, int robust, double* partials);
int launch_rq3_pass2(hipStream_t s, const K3Op& A, const K3Op& Mo, int m_identity, const double* x, const double* p, double* xnew, double* gout, double* state,
                     int init, double* partials);
bool launch_rq3_gmg(hipStream_t s, const K3Op& Mo, const double* gv, double* partials, int nblocks);
bool launch_rq3_small(hipStream_t s, const K3Op& A, const K3Op& Mo, int m_identity, double* x, double* p, double* gv, double* state, int nu, int robust);

// V-cycle-preconditioned conjugate gradients (kernels_pcg.hip; the driver is pcg_host.hip).  One device block per plan; per
// column it holds kPcgStateWords state words, MGCMT_RQ_HISTORY residual norms, kPcgSums * kPcgPartialCap partial sums.  Every pass works on
// the contiguous interior of a level vector (n doubles), so one set serves 1-D, 2-D and 3-D levels.  Every kernel but the
// two of launch_pcg_begin reads the stop word first and returns without writing once it is set.
enum {
  kPcgRho = 0,   // <z, r> of the current iteration
  kPcgRhoOld,    // ... of the previous one
  kPcgSigma,     // <z, q_old>
  kPcgBeta,
  kPcgAlpha,
  kPcgPq,        // <p, q>
  kPcgRR,        // <r, r>
  kPcgFnorm,     // ||f||
  kPcgR0norm,    // ||r_0||
  kPcgRtol,
  kPcgFlexible,  // 1: beta = -alpha_old sigma / rho_old
  kPcgStop,      // != 0: frozen
  kPcgStatus,    // 0 running, 1 converged, 2 breakdown
  kPcgIndefinite,  // 1 once a rho or <p, q> was negative
  kPcgIter,      // iterations done
  kPcgStateWords = 32
};
constexpr int kPcgSums = 2;
constexpr int kPcgMaxBlocks = 2048;    // workgroups of a flat pass
constexpr int kPcgPartialCap = 8192;   // partial sums per result the block holds (the marching pass: one per column group and row chunk)
constexpr int kPcgMaxColumns = 16;     // systems of one batched solve (mgcmt_pcg_begin_k)
constexpr long kPcgColPartials = (long)kPcgSums * kPcgPartialCap;  // partial sums of one column
constexpr int kPcgHeadWords = 32;      // in front of the block; its first 4 bytes: the count of columns whose stop word is set
// The k columns of a solve, as the kernels see them: column c has the state words state + c * kPcgStateWords, the history
// history + c * MGCMT_RQ_HISTORY, the partial sums partials + c * kPcgColPartials, and its vectors are column 0's moved by
// c * stride doubles.  stopped: the count of stopped columns, kept by the kernels that set a stop word (an atomic add each).
// The plan's one block, with room for `cap` columns, is [head | cap states | cap histories | cap x partials]: the head, the
// states and the histories of the first columns are one contiguous copy for the status calls.  The single solve is k = 1 on
// the same block, whatever its capacity.
struct PcgCols {
  double* state;
  double* history;
  double* partials;
  unsigned* stopped;
  long stride;
  int k;
};
inline long pcg_column_doubles() { return kPcgStateWords + MGCMT_RQ_HISTORY + kPcgColPartials; }
inline long pcg_block_doubles(int cap) { return kPcgHeadWords + (long)cap * pcg_column_doubles(); }
inline PcgCols pcg_cols(double* block, int cap, int k, long stride) {
  double* state = block + kPcgHeadWords;
  double* history = state + (long)cap * kPcgStateWords;
  return PcgCols{state, history, history + (long)cap * MGCMT_RQ_HISTORY, (unsigned*)block, stride, k};
}
// Every launch below covers the c.k columns: the vector arguments are column 0's.
// r <- r - q (q = (A - mu I) x0; q == nullptr: the start vector is zero, x <- 0 and r stays f), ||f|| and ||r_0|| from the same
// pass, the state and the history cleared
void launch_pcg_begin(hipStream_t s, long n, double* r, const double* q, double* x, const PcgCols& c, double rtol, int flexible);
void launch_pcg_dots(hipStream_t s, long n, const double* z, const double* r, const double* q, const PcgCols& c);        // rho, sigma; then beta
void launch_pcg_direction(hipStream_t s, long n, const double* z, double* p, const PcgCols& c);                          // p <- z + beta p
void launch_pcg_curvature(hipStream_t s, long n, const double* p, const double* q, const PcgCols& c);                    // <p, q>; then alpha
void launch_pcg_update(hipStream_t s, long n, double* x, const double* p, double* r, const double* q, const PcgCols& c); // x, r, <r, r>; then the norm, the history, the stop word
// direction, application and curvature in ONE march on the 2-D levels launch_ritz_pair covers (a 5-point operator, with or
// without a product potential): p2 <- z + beta p, q <- (A - mu I) p2 and <p2, q>, then alpha; p and p2 are distinct (neighbouring
// threads read the old p).  The bits of launch_pcg_direction + launch_apply; only the order of the partial sums of <p, q> differs.
// Column c takes shifts[c].  false: the level is not covered, nothing was launched
bool launch_pcg_march(hipStream_t s, KGrid g, KOp op, const double* z, const double* p, double* p2, double* q, const double* shifts, const PcgCols& c);

}  // namespace mgcmt
