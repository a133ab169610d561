/*
 * mgcmt_hip.h — C-ABI of libmgcmt_hip.so: the MI355X (gfx950) multigrid V-cycle hot path of
 * AndyMN/MultigridCMT behind plain pointers and sizes.
 *
 * The reference is pure Python (no FFI of its own); the boundary it offers is the class API of
 * MGCMTSolver / MGCMTStencilMaker / MGCMTProcessor.  Each entry point below names the reference
 * function(s) it replaces (paths relative to the reference root).  The Python classes in
 * multigridcmt_amd/ bind these with ctypes (see INTEGRATION.md for the binding a maintainer of
 * the reference would add).
 *
 * Conventions
 *   - every function returns 0 on success, a negative mgcmt_status otherwise; the message of the
 *     last failure on the calling thread is mgcmt_last_error().  No C++ exception crosses the ABI.
 *   - host buffers are C-contiguous IEEE fp64; the library never keeps a host pointer after return.
 *   - a plan belongs to one GPU and is not thread-safe; all work of a call is enqueued on the
 *     `stream` argument (a hipStream_t passed as void*, NULL = the default stream).
 *   - grids: a 2-D level is rows x cols with vector index k = i*cols + j (the reference's
 *     kronsum/kron ordering, MGCMTStencilMaker.py:23-24,53); a 1-D level is 1 x n.
 *   - operators are sums of Kronecker products of tridiagonal factors,
 *         A = sum_m X_m (x) Y_m  - shift * I,
 *     X_m over rows, Y_m over columns, each factor given as three arrays (lower, diagonal, upper).
 *     laplacian(n,"1d") is one term (X = [1], Y = tridiag(1,-2,1)/h^2, MGCMTStencilMaker.py:17-21);
 *     laplacian(n,"2d") = I(x)L + L(x)I is two (MGCMTStencilMaker.py:23-24).  Galerkin coarse
 *     operators R*A*P (MGCMTSolver.py:318) keep this form with X_m <- R1 X_m P1, Y_m <- R1 Y_m P1,
 *     which the library computes at plan creation.
 *   - 3-D grids (mgcmt_plan_create3d, ABI 7): a level is g x g x g points with index idx = z*g^2 + y*g + x (x fastest,
 *     the ordering of kron(A, kron(B, C))), stored as g z-planes of g^2 points with one zero halo plane above and below
 *     every vector.  The operator is  A = sum_m X_m (x) Y_m (x) Z_m - shift * I  with tridiagonal factors over z, y
 *     and x; laplacian(n,"3d") = kronsum(kronsum(L, L), L) is three terms (L(x)I(x)I, I(x)L(x)I, I(x)I(x)L).  With
 *     P = P1 (x) P1 (x) P1 (trilinear interpolation, interpolation(c, f, "3d") = kron(S, kron(S, S))) and
 *     R = (1/8) P^T = R1 (x) R1 (x) R1 (full weighting), every Galerkin level keeps three-factor terms (27-point
 *     stencils).  Multicolour Gauss-Seidel uses the colours (z%2, y%2, x%2) in the order (0,0,1), (0,1,0), (1,0,0),
 *     (1,1,1), (0,0,0), (0,1,1), (1,0,1), (1,1,0): odd coordinate sum first, i.e. red-black on the 7-point fine level.
 *     On a 3-D plan mgcmt_plan_level_shape reports rows = z-planes (g_l) and cols = points per plane (g_l^2), and
 *     mgcmt_plan_get_factors takes which = 0 (z), 1 (y) or 2 (x).  Weighted Jacobi and multicolour Gauss-Seidel are the
 *     3-D smoothers.  A 3-D plan created with a mass operator (mgcmt_plan_create3d_mass) also runs the Rayleigh-quotient
 *     entries (mgcmt_rqmin, mgcmt_rq_line_step, mgcmt_rq_history, mgcmt_vcycle_rqmg) on the Galerkin pairs
 *     (R A P, R M P); on a 3-D plan without one they return MGCMT_ERR_UNSUPPORTED (pass M = I explicitly: the coarse
 *     levels then minimise with R I P, as the reference does).  The entries with no 3-D form (lexicographic smoothers,
 *     twogrid, ritz_pair, rayleigh_residual, sharding, fused-pass and timing entries) return MGCMT_ERR_UNSUPPORTED on
 *     a 3-D plan.
 *     A 3-D operator may carry an arbitrary diagonal on top of its Kronecker terms (mgcmt_plan_create3d_pot), and per-point
 *     bonds as well: any symmetric 7-point matrix (mgcmt_plan_create3d_bonds), or a per-point 27-point stencil: any symmetric
 *     matrix on the 3 x 3 x 3 neighbourhood (mgcmt_plan_create3d_stencil).
 */
#ifndef MGCMT_HIP_H
#define MGCMT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGCMT_ABI_VERSION 7
#define MGCMT_MAX_TERMS 4
#define MGCMT_MAX_STORE_VEC 80   /* vectors a plan may keep per slot (nvec); an entry that takes a column count k batches at most 32, and
                                    only columns 0..31 have a shift (mgcmt_apply with_shift) */
#define MGCMT_BLOCK_WIDE_MAX 48  /* vectors of mgcmt_block_pencil, inputs of mgcmt_block_combine_wide */
#define MGCMT_BLOCK_WIDE_OUT 16  /* outputs of mgcmt_block_combine_wide */
#define MGCMT_BLOCK_LOCKED_MAX 64 /* vectors Q of mgcmt_block_deflate */
#define MGCMT_MIX_MAX 9 /* pairs (x_i, r_i) of mgcmt_mix_residual / mgcmt_mix_combine: Anderson mixing of depth <= 8 */
#define MGCMT_HALO_ROWS 16 /* rows of halo kept above and below every vector of a 2-D level (a 1-D level keeps one: its
                              "row" is the whole vector); how many of them a sharded cycle fills: mgcmt_plan_level_halo */

typedef enum mgcmt_status {
  MGCMT_OK = 0,
  MGCMT_ERR_INVALID = -1,   /* bad argument (sizes not powers of two, level out of range, ...) */
  MGCMT_ERR_HIP = -2,       /* a HIP runtime call failed */
  MGCMT_ERR_NOMEM = -3,
  MGCMT_ERR_UNSUPPORTED = -4
} mgcmt_status;

/* smoother kinds; MGCMTSolver.py:182-246 and the (commented-out) gseidelrb :248-279 */
typedef enum mgcmt_smoother {
  MGCMT_WJACOBI = 0,   /* wjacobi  :182-208  v <- v + w D^-1 (f - A v)                              */
  MGCMT_GS_LEX = 1,    /* gseidel  :210-227  forward lexicographic Gauss-Seidel (index order)        */
  MGCMT_SOR_LEX = 2,   /* sor      :229-246  incl. its (D-L)^-1 right-hand-side term (:241)          */
  MGCMT_GS_MC = 3      /* multicolour GS/SOR: 1-D odd/even, 2-D colours (i%2,j%2) in the order
                          (0,1),(1,0),(0,0),(1,1) = red-black on a 5-point operator                 */
} mgcmt_smoother;

/* vector slots of a level.
 * What an entry writes (checked call by call in tests/test_memory_contract.py): the vectors its comment names as results,
 * for the columns q < k it is given, and the scratch named here — nothing else.  Columns q >= k, the halo rows above and
 * below every vector (exact zeros on a whole-grid plan, always) and the padding between columns are never written.
 * Scratch: slot T of a level belongs to mgcmt_smooth, mgcmt_fused_pass, mgcmt_vcycle and mgcmt_twogrid on the levels they
 * run on (columns q < k; they write the new iterate there and exchange the roles of V and T, so the address behind
 * mgcmt_vec_ptr changes and T holds an older iterate afterwards) and to mgcmt_residual_restrict (the fine residual);
 * slot W belongs to mgcmt_rayleigh_residual (columns q < k) and to no other entry; mgcmt_ritz_pair may write the scratch
 * vector it is given.
 * Left bit for bit: slot F of the level a cycle or mgcmt_twogrid starts on (the coarser levels' F and V are its
 * workspace); slot W in every entry but mgcmt_rayleigh_residual, unless the caller names a vector of W as a result; every
 * vector that an entry takes as an input only (mgcmt_apply, mgcmt_gram, mgcmt_block_gram, mgcmt_lincomb, ...). */
typedef enum mgcmt_slot { MGCMT_SLOT_V = 0, MGCMT_SLOT_F = 1, MGCMT_SLOT_T = 2, MGCMT_SLOT_W = 3 } mgcmt_slot;

/* which operator of the plan: A, or the mass operator M of rqmin (MGCMTSolver.py:17-57) */
typedef enum mgcmt_opsel { MGCMT_OP_A = 0, MGCMT_OP_M = 1 } mgcmt_opsel;

typedef struct mgcmt_plan mgcmt_plan;

typedef struct mgcmt_plan_desc {
  int32_t dim;          /* 1 or 2 */
  int32_t nterms;       /* Kronecker terms of A (1-D: 1) */
  int64_t g;            /* fine grid size per direction (power of two) */
  int64_t lowest;       /* grid size at which the direct solve happens (vcycle's lowest_level) */
  const double* xfac;   /* [nterms][3][g] row factors (lower, diag, upper); NULL for dim == 1 */
  const double* yfac;   /* [nterms][3][g] column factors */
  int32_t m_nterms;     /* Kronecker terms of the mass operator M, 0 = none */
  const double* m_xfac; /* as xfac, for M */
  const double* m_yfac;
  int32_t nvec;         /* number of simultaneous vectors (columns of vcycle_matrix), >= 1 */
  int32_t device;       /* HIP device ordinal */
  int64_t row_begin;    /* rows [row_begin,row_end) of the fine level owned by this plan ...        */
  int64_t row_end;      /* ... (0,g) on one GPU; multiples of 2^(strip_levels-1) when sharded       */
  int32_t strip_levels; /* how many of the finest levels are row strips; the rest are whole grids   */
  int32_t reserved;
} mgcmt_plan_desc;

const char* mgcmt_last_error(void);
int mgcmt_abi_version(void);
int mgcmt_device_count(int* count);
int mgcmt_device_name(int device, char* buf, int buflen);

/* hierarchy: levels, Galerkin factors (R*A*P, MGCMTSolver.py:318), vector storage */
int mgcmt_plan_create(const mgcmt_plan_desc* desc, mgcmt_plan** out);
int mgcmt_plan_destroy(mgcmt_plan* plan);

/* A 3-D plan (see "3-D grids" above): one operator sum_m zfac_m (x) yfac_m (x) xfac_m on g^3 points, levels
 * g^3 -> (g/2)^3 -> ... -> lowest^3 (lowest <= 16: (A - mu I) of the coarsest level is factored directly).  The
 * plan is used through the same entries as a 2-D one (mgcmt_vcycle, mgcmt_smooth, mgcmt_apply, ...). */
typedef struct mgcmt_plan3d_desc {
  int32_t nterms;       /* Kronecker terms of A, 1 .. MGCMT_MAX_TERMS */
  int32_t nvec;         /* number of simultaneous vectors, >= 1 */
  int64_t g;            /* fine grid size per direction (power of two) */
  int64_t lowest;       /* grid size of the direct solve (power of two, 2 .. 16) */
  const double* zfac;   /* [nterms][3][g] factors over z (slowest index): lower, diag, upper */
  const double* yfac;   /* [nterms][3][g] factors over y */
  const double* xfac;   /* [nterms][3][g] factors over x (fastest index) */
  int32_t device;       /* HIP device ordinal */
  int32_t reserved;
} mgcmt_plan3d_desc;
int mgcmt_plan_create3d(const mgcmt_plan3d_desc* desc, mgcmt_plan** out);
/* A 3-D plan with a mass operator M = sum_m m_zfac_m (x) m_yfac_m (x) m_xfac_m (1 .. MGCMT_MAX_TERMS terms, the factor
 * layout of desc's), coarsened per axis like A; M with one identity term is never applied.  The Rayleigh-quotient
 * entries need one on a 3-D plan. */
int mgcmt_plan_create3d_mass(const mgcmt_plan3d_desc* desc, int32_t m_nterms, const double* m_zfac, const double* m_yfac, const double* m_xfac,
                             mgcmt_plan** out);
/* A 2-D plan whose operator carries an arbitrary diagonal on top of its Kronecker terms:
 *     A = sum_m X_m (x) Y_m + diag(point_diag)  - shift * I,
 * point_diag = g x g numbers on the host, index [i * g + j] = grid point (i, j): H = -c Laplacian + V(x, y) with any
 * potential V (the Kronecker terms carry the Laplacian and whatever of V is separable, point_diag the rest).  Under the
 * reference's transfers the Galerkin levels R A P (MGCMTSolver.py:318) are the Kronecker part's usual levels plus a 9-point
 * stencil with per-point coefficients, R diag(point_diag) P, formed on the device at creation.  desc as for
 * mgcmt_plan_create with dim = 2, no mass operator and no row strip.  Such a plan runs mgcmt_vcycle (HIP-graph replay,
 * Gram-Schmidt, per-column shifts and MGCMT_CYCLE_ZERO_START included), mgcmt_smooth, mgcmt_apply, the transfers, the
 * coarse solve and the vector algebra with MGCMT_WJACOBI and MGCMT_GS_MC: the fine level on the fused row-streaming
 * pass (policy Op5P; mgcmt_fused_pass and mgcmt_time_fused_pass take level 0 of such a plan), the Galerkin levels as
 * one launch per operation (csrc/kernels_pointwise.hip), both with the same bits as MGCMT_OPT_FUSED = 0.  The entries
 * that know Kronecker terms only return MGCMT_ERR_UNSUPPORTED with a message that names the point diagonal: the
 * lexicographic smoother kinds, mgcmt_twogrid,
 * mgcmt_rqmin / mgcmt_rq_line_step / mgcmt_vcycle_rqmg, mgcmt_ritz_pair, mgcmt_rayleigh_residual, mgcmt_comm_init /
 * mgcmt_comm_init_external and mgcmt_sharded_vcycle. */
int mgcmt_plan_create_pot(const mgcmt_plan_desc* desc, const double* point_diag, mgcmt_plan** out);
/* A 2-D plan whose operator carries per-point bonds as well: a symmetric 5-point matrix with ANY coefficients,
 *     A = sum_m X_m (x) Y_m + diag(point_diag) + B(east, south)  - shift * I,
 * east[i * g + j] is added to the two entries between the points (i, j) and (i, j + 1), south[i * g + j] to those between
 * (i, j) and (i + 1, j) (g x g numbers each, on the host): H = -div(w grad) + V with a position-dependent inverse effective
 * mass w(x, y) (BenDaniel-Duke), the Kronecker terms carrying a reference mass and the bonds the deviations.  The last
 * column of east and the last row of south point outside the grid and must be zero (MGCMT_ERR_INVALID otherwise).  desc and
 * the refusals are mgcmt_plan_create_pot's (dim = 2, no mass operator, no row strip; the entries listed there return
 * MGCMT_ERR_UNSUPPORTED on such a plan too).  The Galerkin levels are the same nine planes per level as for a point diagonal.
 * Level 0 (MGCMT_OPK_POINT_BONDS) keeps three planes D, E, S and runs kernels of its own (csrc/kernels_bonds.hip): where its
 * Kronecker part is a constant 5-point operator and it has at least 128 columns, a row march with 16-byte accesses —
 * the red-black sweep as two parity stages and residual + restriction in one pass —, otherwise one thread per point
 * (csrc/kernels_pointwise.hip), as for the weighted-Jacobi sweep and mgcmt_apply, whose marching forms measured level with
 * the flat ones.  The environment variable MGCMT_BONDS_MARCH, read at creation, overrides that: 1 = every pass marches, 0 =
 * none does.  Both forms give the same bits.  The fused row-streaming passes do not take such a level (mgcmt_fused_max_sweeps: 0).
 * mgcmt_plan_get_point_stencil(level 0) returns the three planes D, E, S, rows x cols numbers each. */
int mgcmt_plan_create_bonds(const mgcmt_plan_desc* desc, const double* point_diag, const double* east, const double* south, mgcmt_plan** out);
/* A 2-D plan whose operator carries a per-point 9-point stencil on top of its Kronecker terms: any symmetric 9-point matrix,
 *     A = sum_m X_m (x) Y_m + G  - shift * I,
 * stencil = nine planes of g x g numbers on the host, plane 3 a + b, index [i * g + j] = the coefficient of
 * v(i + a - 1, j + b - 1) in row (i, j) (the centre plane is a point diagonal): H = -div(W grad) + V with a position-dependent
 * symmetric 2 x 2 inverse-mass tensor W, whose mixed derivative puts entries on the four corner neighbours.  A non-zero
 * coefficient towards a point outside the grid, and a stencil that is not symmetric — plane 3 a + b at (i, j) must equal plane
 * 3 (2 - a) + (2 - b) at (i + a - 1, j + b - 1) —, give MGCMT_ERR_INVALID.  desc and the refusals are mgcmt_plan_create_pot's
 * (dim = 2, no mass operator, no row strip; the entries listed there return MGCMT_ERR_UNSUPPORTED on such a plan too).
 * Level 0 (MGCMT_OPK_NINE_POINT) has the layout of the Galerkin levels of every plan with a per-point part — nine planes, 72 B
 * per point — and the levels below are formed from it as they are formed from one another.  The fused row-streaming passes
 * (mgcmt_fused_max_sweeps: 0), the tail, the two-level passes and the lexicographic pipelines do not take such a plan.
 * Where level 0 has at least 128 columns it runs the tile kernels of csrc/kernels_nine_tile.hip (a whole four-colour sweep, two
 * weighted-Jacobi sweeps, residual + restriction: one launch each, staged through LDS), otherwise one thread per point
 * (csrc/kernels_pointwise.hip); both forms give the same bits per sweep.  The environment variable MGCMT_NINE_TILE, read at
 * creation: 0 = flat everywhere; 2 = additionally every nine-plane Galerkin level of at least 128 columns of ANY plan with a
 * per-point part takes the tile kernels (for measurements; not the default).
 * mgcmt_plan_get_point_stencil(level 0) returns the nine planes. */
int mgcmt_plan_create_nine(const mgcmt_plan_desc* desc, const double* stencil, mgcmt_plan** out);
/* *tiled = 1 when `level` runs the tile kernels of csrc/kernels_nine_tile.hip (decided at creation, see above), else 0 */
int mgcmt_plan_level_tiled(const mgcmt_plan* plan, int level, int* tiled);
/* host copy of the per-point part of `level` of such a plan: level 0 rows x cols numbers (point_diag); a level below nine
 * planes of rows x cols, plane 3 a + b = the coefficient of v(i + a - 1, j + b - 1) in row (i, j), zero towards points
 * outside the grid.  The level's matrix is the one assembled from mgcmt_plan_get_factors plus these. */
/* A 3-D plan whose operator carries an arbitrary diagonal on top of its Kronecker terms:
 *     A = sum_m X_m (x) Y_m (x) Z_m + diag(point_diag)  - shift * I,
 * point_diag = g^3 numbers on the host, index [z * g^2 + y * g + x]: H = -c Laplacian + V(x, y, z) with any potential V (a
 * spherical well, a lens, coupled dots, disorder).  desc as for mgcmt_plan_create3d; there is no mass operator, so the
 * Rayleigh-quotient entries keep returning their "no mass operator" refusal on such a plan.  The Galerkin levels are the
 * Kronecker part's usual levels plus a 27-point stencil with per-point coefficients, R diag(point_diag) P, formed on the
 * device at creation.  Storage: the diagonal is one level-0 vector (8 B per point); every level below holds 27 planes, summed
 * over the levels 27/7 (about 3.9) fine vectors — about 4 GiB at 512^3.  Such a plan runs what any 3-D plan runs
 * (mgcmt_vcycle with HIP-graph replay, Gram-Schmidt, per-column shifts and MGCMT_CYCLE_ZERO_START; mgcmt_smooth with
 * MGCMT_WJACOBI and MGCMT_GS_MC; mgcmt_apply, the transfers, the coarse solve, the vector algebra): a fine level whose
 * Kronecker part is a constant 7-point operator on marching kernels with the diagonal as a fourth stream (grid sizes that
 * are multiples of 64; the environment variable MGCMT_3D_POINT_MARCH=0, read at creation, selects the flat kernels, which
 * give the same bits per sweep), the levels below as one launch per operation (csrc/kernels_3d_point.hip).
 * mgcmt_plan_get_point_stencil on such a plan: level 0 g^3 numbers; a level below 27 planes of g_l^3, plane 9 a + 3 b + c = the
 * coefficient of v(z + a - 1, y + b - 1, x + c - 1) in row (z, y, x), exactly zero towards points outside the grid. */
int mgcmt_plan_create3d_pot(const mgcmt_plan3d_desc* desc, const double* point_diag, mgcmt_plan** out);
/* A 3-D plan whose operator carries per-point bonds as well: a symmetric 7-point matrix with ANY coefficients,
 *     A = sum_m X_m (x) Y_m (x) Z_m + diag(point_diag) + B(bx, by, bz)  - shift * I,
 * g^3 numbers each on the host, index [z * g^2 + y * g + x]: bx is added to the two entries between the points (z, y, x) and
 * (z, y, x + 1), by to those between (z, y, x) and (z, y + 1, x), bz to those between (z, y, x) and (z + 1, y, x) —
 * H = -div(w grad) + V with a position-dependent inverse effective mass w(x, y, z) (BenDaniel-Duke: a GaAs dot or lens in an
 * AlGaAs barrier), the Kronecker terms carrying a reference mass and the bonds the deviations.  bx at x = g - 1, by at
 * y = g - 1 and bz at z = g - 1 point outside the grid and must be zero (MGCMT_ERR_INVALID otherwise).  desc, what runs and
 * the refusals are mgcmt_plan_create3d_pot's.  The Galerkin levels are the same 27 planes per level as for a point diagonal.
 * Level 0 keeps four planes D, Bx, By, Bz (32 B per point, about 4 GiB at 512^3) and runs the point-diagonal level's kernels
 * with the bonds as three more streams (csrc/kernels_3d_point.hip): where its Kronecker part is a constant 7-point operator and
 * g is a multiple of 64 the marching kernels k3pm_*<BONDS = true>, otherwise — and with MGCMT_3D_POINT_MARCH=0 — the flat
 * ones, one thread per point; both forms give the same bits per sweep.  mgcmt_apply runs flat.
 * mgcmt_plan_get_point_stencil(level 0) returns the four planes D, Bx, By, Bz, g^3 numbers each. */
int mgcmt_plan_create3d_bonds(const mgcmt_plan3d_desc* desc, const double* point_diag, const double* bx, const double* by, const double* bz,
                              mgcmt_plan** out);
/* A 3-D plan whose operator carries a per-point 27-point stencil on top of its Kronecker terms: any symmetric matrix on the
 * 3 x 3 x 3 neighbourhood,
 *     A = sum_m X_m (x) Y_m (x) Z_m + G(stencil)  - shift * I,
 * stencil = 27 planes of g^3 numbers on the host, plane 9 a + 3 b + c, index [z * g^2 + y * g + x]: the coefficient of
 * v(z + a - 1, y + b - 1, x + c - 1) in row (z, y, x) — H = -div(W grad) + V with a position-dependent symmetric 3 x 3
 * inverse-mass tensor W(x, y, z) (a rotated L- or X-valley ellipsoid, strain, a principal axis that turns across an interface),
 * the Kronecker terms carrying reference masses and the planes the deviations, the mixed derivatives on the twelve edge
 * neighbours.  The centre plane (13) is the diagonal.  A non-zero coefficient towards a point outside the grid and a stencil
 * that is not symmetric as a matrix (plane (a, b, c) at a point against plane (2 - a, 2 - b, 2 - c) at its neighbour) return
 * MGCMT_ERR_INVALID.  desc, what runs and the other refusals are mgcmt_plan_create3d_pot's.  Level 0 is stored in the layout
 * of the Galerkin levels below it (216 B per point: about 3.6 GiB at 256^3, 29 GiB at 512^3), which are formed from it as
 * level 2 is formed from level 1.  A level 0 whose Kronecker part is a constant 7-point operator computes a point with
 * csrc/stencil27_point.h's p27::seven (no factor loads).  Where g is a multiple of 64 the passes of level 0 that measured
 * faster than their flat form take the kernels of csrc/kernels_3d_stencil.hip — one stage of the eight-colour sweep launched
 * on its own points only (k3n_colour), residual + restriction with every fine residual formed once through LDS
 * (k3n_residual_restrict) —, each giving the bits of its flat form.  The environment variable MGCMT_3D_STENCIL_TILE, read at
 * creation: 0 = flat kernels everywhere, 1 = every such pass on level 0, 2 = those on the 27-plane Galerkin levels of that
 * size of any 3-D plan with a per-point part as well (measurements).
 * mgcmt_plan_get_point_stencil(level 0) returns the 27 planes. */
int mgcmt_plan_create3d_stencil(const mgcmt_plan3d_desc* desc, const double* stencil, mgcmt_plan** out);
/* Which kernels `level` of a 3-D plan runs on.  kind: 0 general Kronecker terms, 1 constant 7-point, 2 constant 7-point plus a
 * point diagonal, 3 Kronecker terms plus 27 planes, 4 general Kronecker terms plus a point diagonal (a fine level whose
 * factors are not Toeplitz: flat kernels), 5 constant 7-point plus a point diagonal and bonds, 6 general Kronecker terms
 * plus a point diagonal and bonds (flat kernels), 7 constant 7-point plus 27 planes (level 0 of mgcmt_plan_create3d_stencil);
 * marching: whether the level's smoothing and transfer passes take the marching kernels (1) or the flat ones (0) — on a level
 * of kind 3 or 7: whether any of its passes takes the kernels of csrc/kernels_3d_stencil.hip.  Either output may be NULL.
 * (mgcmt_level_operator_kind describes 1-D / 2-D plans.) */
int mgcmt_plan3d_level_path(const mgcmt_plan* plan, int level, int* kind, int* marching);
int mgcmt_plan_get_point_stencil(const mgcmt_plan* plan, int level, double* out, int64_t capacity);
int mgcmt_plan_num_levels(const mgcmt_plan* plan, int* levels);
int mgcmt_plan_level_shape(const mgcmt_plan* plan, int level, int64_t* rows, int64_t* cols, int64_t* row_begin);
/* host copy of a level's factors, [nterms][3][n] with n = global rows (which=0) or cols (which=1) */
int mgcmt_plan_get_factors(const mgcmt_plan* plan, int op, int level, int which, double* out, int64_t capacity);
/* device address of the interior (row 0, col 0) of vector `vec` in `slot` of `level`; rows -halo..-1 and
 * rows..rows+halo-1 are addressable halo rows (halo: mgcmt_plan_level_halo).  The address can be written with no
 * further call into the library, so from the first mgcmt_vec_ptr on a plan no cycle of that plan carries a right-hand
 * side to the next (MGCMT_OPT_CARRY), for the rest of the plan's life. */
int mgcmt_vec_ptr(const mgcmt_plan* plan, int level, int slot, int vec, void** device_ptr);
/* halo_rows: rows kept above and below every vector of `level` (MGCMT_HALO_ROWS on 2-D levels, 1 on 1-D levels);
 * exchanged_rows: how many of them — the ones next to the strip — a sharded cycle fills with the neighbours' rows and its
 * passes read: 8 on levels with a 5-point operator, 10 on the 9-point (Galerkin) levels, whose two four-colour sweeps plus
 * restriction reach nine rows beyond a strip.  Either output may be NULL. */
int mgcmt_plan_level_halo(const mgcmt_plan* plan, int level, int* halo_rows, int* exchanged_rows);

/* shift(s) mu of (A - mu I): vcycle's shift= (MGCMTSolver.py:287-288), vcycle_matrix's shifts= (:385-388) */
int mgcmt_set_shifts(mgcmt_plan* plan, const double* shifts, int k, void* stream);

int mgcmt_upload(mgcmt_plan* plan, int level, int slot, int vec, const double* host, int64_t count, void* stream);
int mgcmt_download(mgcmt_plan* plan, int level, int slot, int vec, double* host, int64_t count, void* stream);
int mgcmt_fill(mgcmt_plan* plan, int level, int slot, int vec, double value, void* stream);
/* vector := 0 including its halo rows (a sharded cycle restarts the coarse iterate without an exchange) */
int mgcmt_zero(mgcmt_plan* plan, int level, int slot, int vec, void* stream);
int mgcmt_copy(mgcmt_plan* plan, int level, int src_slot, int src_vec, int dst_slot, int dst_vec, void* stream);
int mgcmt_sync(void* stream);

/* Page-locked host memory for the host side of mgcmt_upload / mgcmt_download (and mgcmt_csr_upload / _download).
 * A transfer to or from pageable memory is staged through a ring of pinned chunks by several host threads
 * (csrc/transfer.hip); one whose host pointer lies in a buffer of mgcmt_host_alloc — or in any other memory the HIP
 * runtime knows as page-locked — is a single DMA.  The reference returns fresh arrays from every call
 * (MGCMTSolver.py:326 `return v`); the drop-in classes return theirs in recycled buffers of this allocator
 * (multigridcmt_amd/hostmem.py), so a result that is fed back as the next call's v0 never touches pageable memory. */
int mgcmt_host_alloc(int64_t bytes, void** host_ptr);
int mgcmt_host_free(void* host_ptr);

/* smoothers on V,F of `level` for vectors 0..k-1 (MGCMTSolver.py:182-246); slot T of the level is scratch */
int mgcmt_smooth(mgcmt_plan* plan, int level, int kind, int nu, double omega, int k, void* stream);
/* F[level+1] <- R (F - (A - mu I) V), V[level+1] <- 0   (MGCMTSolver.py:315-316); T[level] is scratch (the residual) */
int mgcmt_residual_restrict(mgcmt_plan* plan, int level, int k, void* stream);
/* V[level] <- V[level] + P V[level+1]                    (MGCMTSolver.py:323-324) */
int mgcmt_prolong_correct(mgcmt_plan* plan, int level, int k, void* stream);
/* V[last] <- (A_last - mu I)^-1 F[last]                  (spsolve, MGCMTSolver.py:305-308) */
int mgcmt_coarse_solve(mgcmt_plan* plan, int level, int k, void* stream);
/* one V-cycle from `level` down: vcycle (:281-329) for k == 1, vcycle_matrix (:375-436, incl. the
 * Gram-Schmidt at every non-coarsest level, :434) with MGCMT_CYCLE_GRAM_SCHMIDT in cycle_flags.  nu_coarse is the
 * sweep count on the levels below `level` (the reference does not forward nu1/nu2, so 4: :320,:426).
 * MGCMT_CYCLE_ZERO_START: the caller vouches that V[level] is zero, the way the reference's eigen-drivers start every
 * cycle (1DPotMatrixVcycle.py:70, v0 = zeros): the first pass then neither reads nor needs V cleared (ABI 4; the
 * argument was the 0 / 1 Gram-Schmidt switch before, which keeps its meaning). */
#define MGCMT_CYCLE_GRAM_SCHMIDT 1
#define MGCMT_CYCLE_ZERO_START 2
/* State after a cycle: V[level] holds the new iterate and F[l] of every coarser fused level the restricted residual;
 * the iterates V[l] of the coarser levels are scratch (a level run inside a two-level pass, MGCMT_OPT_TWO_LEVEL, is
 * never written).  A caller that wants a coarse iterate sets MGCMT_OPT_TWO_LEVEL to 0.  Slots V, F and T of the coarser
 * levels and slot T of `level` are the cycle's scratch (columns q < k); F[level] and every slot W are not touched.
 * A carried right-hand side (MGCMT_OPT_CARRY): where the cycle's last launch is the two-level up pass of `level`, the
 * iterate is not flagged zero and there is no Gram-Schmidt, that pass also computes what the NEXT cycle's down pass would
 * write to F[level+1] and leaves it in T[level+1] (scratch by the above; F[level+1] keeps this cycle's restricted
 * residual).  A next mgcmt_vcycle with the same arguments exchanges the two buffers' roles and skips the fine down pass:
 * the same bits.  Anything else that may change V[level], F[level], T[level+1], the shifts or the options drops the
 * carry: every entry that takes a non-const plan, except this one, the readers (mgcmt_dot, mgcmt_gram, mgcmt_download)
 * and mgcmt_apply / _axpy / _copy / _lincomb / _scale into another vector.  mgcmt_vec_ptr turns carrying off for good. */
int mgcmt_vcycle(mgcmt_plan* plan, int level, int nu1, int nu2, int nu_coarse, int kind, double omega, int k,
                 int cycle_flags, void* stream);
/* twogrid (:331-371): exact solve of (R A P - mu I) on level+1; scratch: T[level] and V, F, T of level+1 */
int mgcmt_twogrid(mgcmt_plan* plan, int level, int nu1, int nu2, int kind, double omega, int k, void* stream);

/* dst <- (Op - with_shift*mu I) src        (sparse `*` / .dot, e.g. MGCMTSolver.py:19,315) */
int mgcmt_apply(mgcmt_plan* plan, int op, int level, int src_slot, int src_vec, int dst_slot, int dst_vec,
                int with_shift, void* stream);
/* coarse <- R fine  /  fine <- P coarse    (restriction_matrix * k, MGCMTSolver.py:113,116) */
int mgcmt_restrict(mgcmt_plan* plan, int level, int src_slot, int src_vec, int dst_slot, int dst_vec, void* stream);
int mgcmt_prolong(mgcmt_plan* plan, int level, int src_slot, int src_vec, int dst_slot, int dst_vec, int accumulate,
                  void* stream);

/* vector algebra (MGCMTProcessor.py:10-73; np.dot / np.linalg.norm call sites of MGCMTSolver.py) */
int mgcmt_dot(mgcmt_plan* plan, int level, int slot_a, int vec_a, int slot_b, int vec_b, double* host_out, void* stream);
int mgcmt_axpy(mgcmt_plan* plan, int level, double alpha, int x_slot, int x_vec, int y_slot, int y_vec, void* stream);
/* all inner products <v_a, v_b> of nv <= 6 vectors (slots[a], vecs[a]) in ONE pass over the data; host_out is the
 * symmetric nv x nv Gram matrix, row-major.  The Rayleigh-Ritz steps of rqmin (MGCMTSolver.py:44-50: the entries of
 * its 2x2 matrices R and RM) and of the eigen-drivers need such sets; synchronises like mgcmt_dot. */
int mgcmt_gram(mgcmt_plan* plan, int level, int nv, const int* slots, const int* vecs, double* host_out, void* stream);
/* For the columns q < k of `slot`: rq_out[q] = <v_q, A v_q> / <v_q, v_q> and res_out[q] = ||(A - mu_q I) v_q||_2 with the
 * plan's current shifts mu — the two numbers the reference's eigen-drivers print per column and iteration
 * (2DPotMatrixVcycle.py:100-105: np.dot(v, hamiltonian.dot(v)) and np.linalg.norm(shifted_matrix.dot(v))).  One
 * k-column operator application (into slot W) and one reduction pass per column; ONE synchronisation for all of them.
 * Either output may be NULL. */
int mgcmt_rayleigh_residual(mgcmt_plan* plan, int level, int slot, int k, double* rq_out, double* res_out, void* stream);
/* The inner products of the 2 x 2 Rayleigh-Ritz problem on span{x, w} (rqmin's pencil, MGCMTSolver.py:44-50, when <x, A x>
 * is known from the previous step): out5 = <x,x>, <x,w>, <w,w>, <x,A w>, <w,A w> with the UNSHIFTED operator of `level`.
 * On 2-D levels with a 5-point operator (with or without a product potential) ONE pass reads x and w once and stores
 * nothing; elsewhere A w goes to the scratch vector (mgcmt_apply) and one mgcmt_gram pass follows.  The scratch vector must
 * differ from x and w.  Synchronises. */
int mgcmt_ritz_pair(mgcmt_plan* plan, int level, int x_slot, int x_vec, int w_slot, int w_vec, int scratch_slot, int scratch_vec,
                    double* out5, void* stream);
/* rqmin (MGCMTSolver.py:17-57): nu steps of Rayleigh-quotient minimisation on `level` for the plan's pair (A, M) (M = I
 * without a mass operator), entirely on the device — per step TWO passes over the data (p = -g + beta p_old formed on the
 * fly, A and M applied to x and p in registers, the eight inner products of the 2 x 2 pencil of :33-46; then x + delta p, its
 * gradient g = 2 (A x - rho M x) and the next step's inner products), the pencil solved in closed form by one workgroup,
 * no host round trip.  vecs[0] of `slot` holds the start vector and receives the result; vecs[1..5] are five more, distinct
 * vectors of the slot used as work space.  robust != 0: a degenerate pencil ends the minimisation instead of producing
 * infinities (the repaired variants).  rho_out (may be NULL: nothing synchronises then): the Rayleigh quotient of the
 * result (:53). */
int mgcmt_rqmin(mgcmt_plan* plan, int level, int slot, const int* vecs, int nu, int robust, double* rho_out, void* stream);
/* One line minimisation of the Rayleigh quotient of the plan's pair (A, M) on `level` along a direction the caller
 * supplies: the 2 x 2 problem of rqmin (MGCMTSolver.py:33-50) on span{x, w} — x_out = x + delta w — followed by
 * g = 2 (A x_out - rho M x_out) (:52-54), both on the device, the state words of mgcmt_rqmin reused; no host round trip.
 * With w the preconditioned residual (a V-cycle applied to g) this is the iteration of the 2-D square-well driver.
 * Vectors are {slot, vec} pairs, all distinct: x (read), w (read; NULL: only rho and g of x are computed, x_out unused),
 * x_out, g, and, with a non-identity mass operator, a work vector (NULL otherwise).  record >= 0: the Rayleigh quotient
 * of x_out is also stored as number `record` (< MGCMT_RQ_HISTORY) of the plan's device-side history, read back — with
 * the only synchronisation — by mgcmt_rq_history. */
#define MGCMT_RQ_HISTORY 4096
int mgcmt_rq_line_step(mgcmt_plan* plan, int level, const int* x, const int* w, const int* x_out, const int* g, const int* work, int robust,
                       int record, void* stream);
int mgcmt_rq_history(mgcmt_plan* plan, int first, int count, double* out, void* stream);
/* vcycle_rqmg (MGCMTSolver.py:99-122) from the finest level: rqmin with nu1 steps, the iterate restricted (:113), the same on
 * the Galerkin pair (R A P, R M P) of every coarser level of the plan (the coarsest one only minimises), the interpolated
 * coarse iterates added on the way up (:116-118) and nu2 more steps per level; vectors as for mgcmt_rqmin, on every level.
 * One launch sequence without a host round trip, replayed as a HIP graph from its second call. */
int mgcmt_vcycle_rqmg(mgcmt_plan* plan, int slot, const int* vecs, int nu1, int nu2, int robust, double* rho_out, void* stream);
/* Solve (A - mu I) x = f to a tolerance on level 0 of a whole-grid plan: conjugate gradients preconditioned by one V-cycle per
 * iteration (an addition: every cycle entry of the reference runs a fixed number of cycles).  mu is the plan's shift 0, the one
 * a cycle uses for column 0.  Layout: the residual r lives in F[0] column 0 (the cycle's right-hand side, which a cycle leaves
 * alone), the preconditioned residual z is V[0] column 0 (the cycle's result), and x, p, q and a spare p2 are four distinct
 * columns vecs[0..3] of slot W on level 0; the plan stores at least 4 vectors.  All scalars (rho, alpha, beta, the norms, the
 * iteration count, the stop word) and the history of ||r_k|| (MGCMT_RQ_HISTORY numbers) stay on the device.
 *   mgcmt_pcg_begin: the caller has put f into F[0] column 0 and — unless MGCMT_PCG_ZERO_START — x_0 into x.  Forms
 *     r = f - (A - mu I) x_0 in place (zero start: no operator application, x <- 0), records ||f|| and ||r_0||, clears the state
 *     and the history.  MGCMT_PCG_FLEXIBLE: beta = -alpha_old <z, q_old> / rho_old (Polak-Ribiere with r - r_old = -alpha q: no
 *     extra vector; equal to rho / rho_old for a symmetric preconditioner such as the weighted-Jacobi cycle, and the right
 *     form for the multicolour cycle, which is not symmetric) instead of beta = rho / rho_old.
 *   mgcmt_pcg_iterate: queues `iterations` iterations without synchronising.  One iteration: z = one mgcmt_vcycle of r
 *     (MGCMT_CYCLE_ZERO_START, k = 1; nu1, nu2, nu_coarse, kind, omega are the cycle's); rho = <z, r> and sigma = <z, q> in one
 *     pass; beta; p <- z + beta p; q <- (A - mu I) p; <p, q>; alpha = rho / <p, q>; x += alpha p, r -= alpha q and <r, r> in one pass;
 *     ||r|| into the history, and the stop word set when ||r|| <= rtol ||f|| (converged) or when rho or <p, q> is zero or not
 *     finite (breakdown).  Once the stop word is set the passes and scalar kernels of every later iteration return without
 *     writing (the cycle and the operator application still run, on scratch): x is the iterate of the first iteration that
 *     met the tolerance however many were queued.  A negative rho or <p, q> does not stop the iteration — the shifted systems
 *     next to an eigenvalue are indefinite and converge — and sets MGCMT_PCG_INDEFINITE in the status.  Reductions add
 *     per-block partial sums in a fixed order: results are bit-reproducible.  A smoother kind the plan's cycle refuses is the
 *     cycle's error.  Writes: x, p, q of slot W, F[0] column 0, and what mgcmt_vcycle writes; with the marching direction pass
 *     (MGCMT_OPT_PCG_MARCH) also p2: the direction of iteration k is in p for even k and in p2 for odd k (k = 1 the first).
 *   mgcmt_pcg_status: the only synchronising call.  iterations_done: iterations completed since the begin; status:
 *     MGCMT_PCG_RUNNING, _CONVERGED or _BREAKDOWN, plus MGCMT_PCG_INDEFINITE; fnorm: ||f||; history[k] = ||r_{k+1}|| for
 *     k < min(capacity, MGCMT_RQ_HISTORY).  Any output may be NULL.
 * The three entries are mgcmt_pcg_*_k below with k = 1, on the same device state, with scalar outputs.
 * MGCMT_ERR_UNSUPPORTED on a sharded plan, MGCMT_ERR_INVALID on a plan with fewer than 4 vectors or vecs that are not distinct.
 * The general sparse plans (mgcmt_csr_*) have no such entry. */
#define MGCMT_PCG_ZERO_START 1
#define MGCMT_PCG_FLEXIBLE 2
#define MGCMT_PCG_RUNNING 0
#define MGCMT_PCG_CONVERGED 1
#define MGCMT_PCG_BREAKDOWN 2
#define MGCMT_PCG_INDEFINITE 0x100
int mgcmt_pcg_begin(mgcmt_plan* plan, const int* vecs, double rtol, int flags, void* stream);
int mgcmt_pcg_iterate(mgcmt_plan* plan, int iterations, int nu1, int nu2, int nu_coarse, int kind, double omega, void* stream);
int mgcmt_pcg_status(mgcmt_plan* plan, int* iterations_done, int* status, double* fnorm, double* history, int capacity, void* stream);
/* The same solve for k systems at once, (A - mu_c I) x_c = f_c for c = 0 .. k - 1, 1 <= k <= MGCMT_PCG_MAX_COLUMNS: the shape of
 * a shift-and-invert step on k columns, one shift per column, each next to its own eigenvalue.  mu_c is the plan's shift c.  The
 * columns are independent systems (no Gram-Schmidt) that share every launch: the column is a grid dimension of every kernel.
 * Layout: r_c lives in F[0] column c, z_c is V[0] column c, and vecs[0..3] are the FIRST columns of four ranges of k consecutive
 * columns of slot W on level 0 — x, p, q and the spare p2; column c uses vecs[a] + c.  The ranges must not overlap and must lie
 * within the plan's vectors: nvec >= 4 k (k = 16: nvec = 64 <= MGCMT_MAX_STORE_VEC).  One rtol and one beta form for all columns.
 *   mgcmt_pcg_begin_k: as mgcmt_pcg_begin, per column.  A column whose f is zero, or whose start vector already meets the
 *     tolerance, sets its own stop word here.  The state (k blocks of scalars, k histories, k sets of partial sums) is one device
 *     allocation per plan, made by the first begin of either kind and grown when a later one has more columns.
 *   mgcmt_pcg_iterate_k: queues `iterations` iterations without synchronising.  One iteration: ONE mgcmt_vcycle on k columns
 *     (zero start, no Gram-Schmidt), then the passes and scalar kernels of mgcmt_pcg_iterate with k times the workgroups, the
 *     marching direction pass where mgcmt_pcg_iterate takes it (same gate, same option).  Columns freeze independently: once a
 *     column's stop word is set (converged or breakdown) every pass and scalar kernel returns for that column before it writes,
 *     and the other columns go on.  The cycle and the operator application do not know of the stop words: they still run for
 *     frozen columns, on scratch (z_c and q_c, which nothing reads again) — an iteration costs k columns until the LAST column
 *     stops.  Per column the workgroup count and the order of every sum are those of the single solve and do not depend on k:
 *     where the k-column cycle gives each column the bits of its own k = 1 cycle, column c carries the bits of mgcmt_pcg_* run
 *     alone on (f_c, mu_c).  Writes: the ranges x, p, q (with the marching pass also p2), F[0] columns 0 .. k - 1, and what a
 *     k-column mgcmt_vcycle writes.
 *   mgcmt_pcg_status_k: one copy, one synchronisation.  running: the number of columns without a stop word (kept on the device
 *     as a count of stopped columns, so the host reads one word to decide whether to queue more); iterations_done[k], status[k],
 *     fnorm[k] as in mgcmt_pcg_status, per column; history: k rows of `capacity` numbers.  Any output may be NULL.
 * A batched begin ends a single solve on the same plan and the reverse (they share F, V, W and the state): the other kind's
 * iterate / status then returns MGCMT_ERR_INVALID, as before any begin — after mgcmt_pcg_begin_k with k = 1 as well.  MGCMT_ERR_UNSUPPORTED on a sharded plan; MGCMT_ERR_INVALID for k
 * out of range and for column ranges that overlap or leave the plan's vectors.  mgcmt_pcg_time_pass after a batched begin times
 * the pass on the k columns. */
#define MGCMT_PCG_MAX_COLUMNS 16
int mgcmt_pcg_begin_k(mgcmt_plan* plan, int k, const int* vecs, double rtol, int flags, void* stream);
int mgcmt_pcg_iterate_k(mgcmt_plan* plan, int iterations, int nu1, int nu2, int nu_coarse, int kind, double omega, void* stream);
int mgcmt_pcg_status_k(mgcmt_plan* plan, int* running, int* iterations_done, int* status, double* fnorm, double* history, int capacity,
                       void* stream);
/* timing for scripts/bench_pcg.py: average milliseconds of `reps` launches of ONE pass of an iteration together with the scalar
 * kernel that follows it (one untimed launch first), between two HIP events on `stream`, on the vectors of the solve in progress
 * (after a mgcmt_pcg_begin and at least one iteration; the solve's vectors and scalars are scratch afterwards, and a stop word
 * that is set makes every launch return at once).  MGCMT_PCG_PASS_MARCH on a level the marching pass does not cover:
 * MGCMT_ERR_UNSUPPORTED. */
#define MGCMT_PCG_PASS_DOTS 0      /* rho, sigma: 24 B per point */
#define MGCMT_PCG_PASS_DIRECTION 1 /* p <- z + beta p: 24 B */
#define MGCMT_PCG_PASS_CURVATURE 2 /* <p, q>: 16 B */
#define MGCMT_PCG_PASS_UPDATE 3    /* x, r, <r, r>: 48 B */
#define MGCMT_PCG_PASS_MARCH 4     /* direction + application + curvature in one march: 32 B */
int mgcmt_pcg_time_pass(mgcmt_plan* plan, int pass, int reps, double* ms_out, void* stream);
/* dst = sum_t coeffs[t] * (slots[t], vecs[t]), 1 <= nterms <= 4; dst may be one of the inputs (the updates
 * x <- x + delta p, MGCMTSolver.py:52, and the residual A x - rho M x, :22-23, in one pass each) */
int mgcmt_lincomb(mgcmt_plan* plan, int level, int nterms, const double* coeffs, const int* slots, const int* vecs, int dst_slot,
                  int dst_vec, void* stream);
int mgcmt_scale(mgcmt_plan* plan, int level, double alpha, int slot, int vec, void* stream);
/* Block operations of the blocked Rayleigh-Ritz eigen-solver (the 2-vector problem of rqmin, MGCMTSolver.py:44-50, carried
 * to blocks of trial vectors; SURVEY par. 8(f)4).  block_gram: out[i * nb + j] = <A_i, B_j> for na <= 12 and nb <= 4
 * vectors in one pass, synchronises.  block_combine: OUT_j = sum_i coeffs[i * nout + j] IN_i for nin <= 12 inputs and
 * nout <= 4 distinct outputs, every input read once; an output may be one of the inputs. */
int mgcmt_block_gram(mgcmt_plan* plan, int level, int na, const int* a_slots, const int* a_vecs, int nb, const int* b_slots,
                     const int* b_vecs, double* out, void* stream);
int mgcmt_block_combine(mgcmt_plan* plan, int level, int nin, const int* in_slots, const int* in_vecs, int nout, const int* out_slots,
                        const int* out_vecs, const double* coeffs, void* stream);
/* The same for wide blocks (up to 16 states: S = [X, W, P] of 48 vectors).  block_pencil: h_out = S^T AS and g_out = S^T MS
 * (ms_slots = ms_vecs = NULL: M = I, g_out = S^T S) as full m x m row-major host matrices, 1 <= m <= MGCMT_BLOCK_WIDE_MAX, every
 * named vector read once in one pass on the matrix cores; bit-reproducible from call to call; synchronises.  S and AS (and MS)
 * are independent lists: nothing is assumed symmetric.  block_combine_wide: OUT_j = sum_i coeffs[i * nout + j] IN_i for
 * nin <= MGCMT_BLOCK_WIDE_MAX inputs and nout <= MGCMT_BLOCK_WIDE_OUT distinct outputs, every input read once; an output may
 * be one of the inputs; stream-ordered (coeffs may be reused on return).  Both entries work through scratch of the plan's
 * own (partial tiles, the coefficient table), as the reductions do: the wide entries of one plan run on one stream at a time.
 * Level vectors are 16-byte aligned and hold an even number of points; anything else is MGCMT_ERR_INVALID. */
int mgcmt_block_pencil(mgcmt_plan* plan, int level, int m, const int* s_slots, const int* s_vecs, const int* as_slots, const int* as_vecs,
                       const int* ms_slots, const int* ms_vecs, double* h_out, double* g_out, void* stream);
int mgcmt_block_combine_wide(mgcmt_plan* plan, int level, int nin, const int* in_slots, const int* in_vecs, int nout, const int* out_slots,
                             const int* out_vecs, const double* coeffs, void* stream);
/* W_j <- W_j - sum_i <Q_i, W_j> Q_i   for 1 <= nq <= 64 vectors Q and 1 <= k <= MGCMT_BLOCK_WIDE_OUT distinct vectors W,
 * none of them a Q.  Two stream-ordered passes; the coefficients stay on the device.  coeffs_out (may be NULL): the nq x k
 * coefficients row-major; non-NULL synchronises.  Bit-reproducible from call to call.  Scratch and stream rule: those of
 * the wide entries.  Writes the k vectors W and nothing else. */
int mgcmt_block_deflate(mgcmt_plan* plan, int level, int nq, const int* q_slots, const int* q_vecs, int k,
                        const int* w_slots, const int* w_vecs, double* coeffs_out, void* stream);
/* mgcmt_block_deflate with companions that take the same coefficients:
 *     W_j  <- W_j  - sum_i <B_i, W_j> B_i
 *     AW_j <- AW_j - sum_i <B_i, W_j> AB_i
 * for 1 <= nb <= MGCMT_BLOCK_LOCKED_MAX vectors B and 1 <= k <= MGCMT_BLOCK_WIDE_OUT distinct vectors W (with B orthonormal
 * and AB = A B, AW = A W on entry, AW = A W on return).  ab_slots, ab_vecs, aw_slots and aw_vecs all NULL: W only; given in
 * part: MGCMT_ERR_INVALID, as are a W or an AW named twice, a W that is a B or an AB, an AW that is a B, an AB or a W.  Pass 1
 * is the one of mgcmt_block_deflate, pass 2 runs once per pair on the same coefficients, which stay on the device; coeffs_out,
 * reproducibility, scratch and stream rule as there.  Writes the k vectors W and the k vectors AW and nothing else. */
int mgcmt_block_project(mgcmt_plan* plan, int level, int nb, const int* b_slots, const int* b_vecs, const int* ab_slots, const int* ab_vecs,
                        int k, const int* w_slots, const int* w_vecs, const int* aw_slots, const int* aw_vecs, double* coeffs_out, void* stream);
/* One Cholesky-QR step on 1 <= k <= MGCMT_BLOCK_WIDE_OUT distinct vectors W:  W <- W T  and (aw_slots, aw_vecs not NULL)
 * AW <- AW T, with T upper triangular, its diagonal positive, T^T (W^T W) T = I.  Three stream-ordered launches: G = W^T W on
 * the matrix cores (W read once); one workgroup that scales G to a unit diagonal (d_j = G_jj^(-1/2)), factors D G D = R^T R
 * (Cholesky in column order, no pivoting) and forms T = D R^-1; the in-place product (a second launch for AW).  A column
 * whose G_jj is zero or not finite, or whose pivot of the scaled matrix is <= drop_tol (0 < drop_tol < 1, else
 * MGCMT_ERR_INVALID), is DROPPED: its row and column leave the factorisation, its row and column of T are zero, and it comes
 * back as exact zeros in W and in AW.  t_out (may be NULL): T, k x k row-major; dropped_out (may be NULL): bit j set when
 * column j was dropped; either one synchronises, with both NULL nothing does.  Applied twice to vectors with
 * cond(W)^2 u O(nk) < 1 it leaves them orthonormal to working accuracy.  Bit-reproducible from call to call.  Scratch and
 * stream rule: those of the wide entries.  Refused as there: null lists, k out of range, a W or an AW named twice, an AW that
 * is also a W, one companion list without the other.  Writes the k vectors W and the k vectors AW and nothing else. */
int mgcmt_block_orthonormalize(mgcmt_plan* plan, int level, int k, const int* w_slots, const int* w_vecs, const int* aw_slots,
                               const int* aw_vecs, double drop_tol, double* t_out, unsigned* dropped_out, void* stream);
/* dst(r) = sum_(t < nq) weights[t] x_t(r)^2   for 1 <= nq <= MGCMT_BLOCK_LOCKED_MAX vectors x of `level` (the charge density of
 * nq states with their occupations; drivers.schroedinger_poisson).  One stream-ordered pass, nothing synchronises: every named
 * vector is read once and dst written once, 8 (nq + 1) bytes per point.  weights: nq host numbers, copied on entry.  The
 * arithmetic is fixed — acc = 0; for t ascending: acc = fma(weights[t] * x_t, x_t, acc) —, so the result is bit-reproducible
 * from call to call and does not depend on the launch's grid.  MGCMT_ERR_INVALID: null lists, nq out of range, a vector outside
 * the plan, dst one of the x, a weight that is not finite, an odd number of points or a vector that is not 16-byte aligned
 * (the rule of the wide entries).  Writes dst and nothing else. */
int mgcmt_block_density(mgcmt_plan* plan, int level, int nq, const int* x_slots, const int* x_vecs, const double* weights, int dst_slot,
                        int dst_vec, void* stream);
/* Anderson (Pulay) mixing, the residual of a step (drivers.schroedinger_poisson with mixing_history > 0):
 *     r = out - in   written to (r_slot, r_vec),   and, from the same pass,
 *     host_out[j] = <r, prev_j> for j < nprev in the order given, host_out[nprev] = <r, r>, host_out[nprev + 1] = <out, out>
 * for 0 <= nprev <= MGCMT_MIX_MAX - 1 earlier residuals of `level`.  out, in and every prev_j are read once, r is written
 * once: 8 (nprev + 3) bytes per point.  Per-slice partial sums (the slices depend on the point count alone, not on the
 * launch's grid), then one workgroup that adds them in a fixed order: r and every sum are bit-reproducible from call to call
 * and do not depend on the grid.  Synchronises `stream` as mgcmt_dot does (nprev + 2 numbers cross to the host).
 * MGCMT_ERR_INVALID: null lists (prev_slots / prev_vecs may be NULL only with nprev == 0) or a null host_out, nprev out of
 * range, a vector outside the plan, r one of the vectors read, an odd number of points or a vector that is not 16-byte
 * aligned (the rule of the wide entries).  Writes r and nothing else. */
int mgcmt_mix_residual(mgcmt_plan* plan, int level, int out_slot, int out_vec, int in_slot, int in_vec, int r_slot, int r_vec, int nprev,
                       const int* prev_slots, const int* prev_vecs, double* host_out, void* stream);
/* Anderson mixing, the new iterate:  dst = sum_(i < p) alpha[i] (x_i + beta r_i)  for 1 <= p <= MGCMT_MIX_MAX pairs of vectors
 * of `level`, in one stream-ordered pass over the 2p vectors (8 (2p + 1) bytes per point); nothing synchronises.  alpha (p host
 * numbers) and beta are copied on entry.  The arithmetic is fixed — acc = 0; for i ascending:
 * acc = fma(alpha[i], fma(beta, r_i, x_i), acc) —, so the result is bit-reproducible and does not depend on the grid.  dst may
 * be x_0 (the oldest pair's x, which a ring of pairs is about to drop) and no other input.  MGCMT_ERR_INVALID: null lists, p out
 * of range, a vector outside the plan, an alpha or beta that is not finite, dst one of the other inputs, an odd number of points
 * or a vector that is not 16-byte aligned.  Writes dst and nothing else. */
int mgcmt_mix_combine(mgcmt_plan* plan, int level, int p, const int* x_slots, const int* x_vecs, const int* r_slots, const int* r_vecs,
                      const double* alpha, double beta, int dst_slot, int dst_vec, void* stream);
/* A new per-point diagonal for a plan that has a per-point part (any of the six creators of such plans):
 *     D = sum_(t < nterms) coeffs[t] * (slots[t], vecs[t]),   1 <= nterms <= 4, level-0 vectors of this plan,
 * with the arithmetic of mgcmt_lincomb, written to level 0 — the diagonal of mgcmt_plan_create_pot / create3d_pot, plane D of
 * the creators with bonds (the bonds stay), the centre plane of a stencil (plane 4 of 9, 13 of 27; the others stay) — and the
 * planes of every level below formed again by the launches creation used, in its order and with its arguments: the hierarchy
 * then holds the bits a plan created from that diagonal holds.  Stream-ordered on `stream`; nothing is allocated and the host
 * is not synchronised.  What is derived from the planes follows: the factorisation (and explicit inverse) of a coarse solve
 * is redone before its next use, also in front of a replayed cycle graph; the graphs themselves hold pointers to the planes,
 * which do not move, and are kept.  MGCMT_ERR_INVALID: a plan without a per-point part, null lists, nterms out of range, a
 * vector outside the plan. */
int mgcmt_plan_set_point_diagonal(mgcmt_plan* plan, int nterms, const double* coeffs, const int* slots, const int* vecs, void* stream);
/* (dst_slot, dst_vec) of `dst` <- (src_slot, src_vec) of `src` on `level`: one device-to-device copy of the level vector's
 * interior between two plans on the same device, of the same dimension, whose level has the same rows and columns (whole
 * grids).  Stream-ordered.  Anything else — and src == dst naming the same vector — is MGCMT_ERR_INVALID. */
int mgcmt_copy_across(mgcmt_plan* src, int level, int src_slot, int src_vec, mgcmt_plan* dst, int dst_slot, int dst_vec, void* stream);
/* in-place Gram-Schmidt of vectors 0..k-1 of `slot`: modified != 0 -> MGS (:44-50), else CGS (:34-42) */
int mgcmt_gramschmidt(mgcmt_plan* plan, int level, int slot, int k, int modified, void* stream);
/* columns scaled to unit 2-norm (normalize, :52-63) */
int mgcmt_normalize(mgcmt_plan* plan, int level, int slot, int k, void* stream);

/* Building blocks of a sharded cycle (multigridcmt_amd/distributed.py exchanges halo rows between them).
 * mgcmt_fused_pass: ONE fused row-streaming pass on `level`, V <- nsweep sweeps of `kind` (MGCMT_WJACOBI or
 * MGCMT_GS_MC) applied to V, optionally preceded by V += P V[level+1] (mode 1, MGCMTSolver.py:323-324) or
 * followed by F[level+1] <- R (F - (A - mu I) V) (mode 2, :315); adding 4 to mode 0 or 2 declares the incoming V
 * to be zero (it is then neither read nor required to have been cleared, :316); adding 8 to mode 2 suppresses the
 * store of the smoothed V ("recompute instead of store": a later mode-1 pass with (npre << 4) added re-runs those
 * npre sweeps from the untouched V before it adds the correction — also with 4 when that V is the zero iterate).
 * The pass reads the exchanged halo rows (mgcmt_plan_level_halo) of V
 * and F (and of V[level+1] in mode 1) around a strip.  mgcmt_fused_max_sweeps: sweeps one pass can take on that
 * level (0 = the level is not covered by the fused kernels). */
int mgcmt_fused_pass(mgcmt_plan* plan, int level, int kind, int nsweep, double omega, int mode, int k, void* stream);
int mgcmt_fused_max_sweeps(const mgcmt_plan* plan, int level, int kind, int* max_sweeps);
/* how many pre-smoothing sweeps a mode-1 pass with `nsweep` post-smoothing sweeps can recompute on that level */
int mgcmt_fused_max_recompute(const mgcmt_plan* plan, int level, int kind, int nsweep, int* max_recompute);
/* How the library recognised the operator of `level` (which decides the kernels the level runs on): MGCMT_OPK_GENERAL
 * (Kronecker terms with variable factors), MGCMT_OPK_FIVE_POINT (constant 5-point / 3-point: the scaled, shifted
 * Laplacian of MGCMTStencilMaker.py:15-25), MGCMT_OPK_FIVE_DIAG (the same plus a product potential on the diagonal),
 * MGCMT_OPK_NINE_CONST (Galerkin coarsenings R*A*P, MGCMTSolver.py:318, of a constant operator), MGCMT_OPK_NINE_VAR
 * (the same plus one term with variable factors: the coarsened product potential).  On a plan with a point diagonal
 * (mgcmt_plan_create_pot): MGCMT_OPK_POINT_DIAG (level 0: the Kronecker terms, a 5-point operator, plus a per-point diagonal)
 * and MGCMT_OPK_NINE_POINT (the Galerkin levels: a 9-point stencil with a per-point part). */
#define MGCMT_OPK_GENERAL 0
#define MGCMT_OPK_FIVE_POINT 1
#define MGCMT_OPK_FIVE_DIAG 2
#define MGCMT_OPK_NINE_CONST 3
#define MGCMT_OPK_NINE_VAR 4
#define MGCMT_OPK_POINT_DIAG 5
#define MGCMT_OPK_NINE_POINT 6
#define MGCMT_OPK_POINT_BONDS 7 /* level 0 of mgcmt_plan_create_bonds: the Kronecker terms plus a per-point diagonal and bonds */
int mgcmt_level_operator_kind(const mgcmt_plan* plan, int level, int* kind);

/* ---- multi-GPU: row strips with neighbour halo exchange --------------------------------------------
 * A strip plan (mgcmt_plan_desc.row_begin/row_end/strip_levels) gets a communicator; every exchange below is then
 * enqueued by the library itself.  mgcmt_comm_init: RCCL (ncclSend/ncclRecv groups and ncclAllGather on HIP streams,
 * no host synchronisation inside a cycle; librccl is loaded on first use).  Rank 0 obtains the 128-byte id with
 * mgcmt_comm_unique_id and the host program distributes it (any channel).  mgcmt_comm_init_external: the host
 * program supplies the transport as callbacks (gloo, MPI, staging through host memory ...); the library synchronises
 * its stream before each call, `ptr`s are device addresses of this plan, counts are in doubles, a callback returns 0 on
 * success and must have completed the transfer when it returns. */
#define MGCMT_UNIQUE_ID_BYTES 128
typedef struct mgcmt_p2p_op {
  void* ptr;
  int64_t count;
  int32_t peer;
  int32_t is_send;
} mgcmt_p2p_op;
typedef int (*mgcmt_p2p_fn)(void* user, int nops, const mgcmt_p2p_op* ops);                  /* one batch, all at once */
typedef int (*mgcmt_allgather_fn)(void* user, const void* send, void* recv, int64_t count);  /* recv = nranks * count */
typedef int (*mgcmt_allreduce_fn)(void* user, double* host_inout, int n);                    /* sum over ranks */
int mgcmt_comm_unique_id(void* id_out /* MGCMT_UNIQUE_ID_BYTES */);
int mgcmt_comm_init(mgcmt_plan* plan, int rank, int nranks, const void* unique_id);
int mgcmt_comm_init_external(mgcmt_plan* plan, int rank, int nranks, mgcmt_p2p_fn p2p, mgcmt_allgather_fn allgather,
                             mgcmt_allreduce_fn allreduce, void* user);
int mgcmt_comm_destroy(mgcmt_plan* plan);
typedef enum mgcmt_comm_option {
  MGCMT_COMM_OPT_OVERLAP = 0, /* default 1 (RCCL): the exchange of a pass's boundary rows runs on a second stream beside
                                 the launch that produces the interior rows */
  MGCMT_COMM_OPT_SPLIT = 1,   /* default 1: boundary rows are produced by their own launches first on strips of >= 2^22 points (where the
                                 exchange they take off the critical path outweighs two more launches); 2: on every strip; 0: never */
  MGCMT_COMM_OPT_SELF_RING = 2, /* default 0; 1 on a ONE-rank communicator: the rank acts as its own upper and lower neighbour in
                                 every exchange of a cycle: the split launches, the transport and the stream overlap run
                                 for real on one GPU (on a whole-grid plan the rows it receives are never read) */
  MGCMT_COMM_OPT_EMULATE_OF = 3 /* default 0; N > 1 on a ONE-rank communicator in self-ring mode whose plan is the strip of
                                 some rank R of an N-rank job: the cycle then does that rank's work — strip passes, the
                                 exchanges (with itself), a gather of N strips' worth of data, the redundant coarse
                                 sub-cycle — so that one GPU can time one rank's share (bench.py --emulate-rank).  The halo
                                 rows hold the rank's own rows, so the numbers are not the N-rank job's */
} mgcmt_comm_option;
int mgcmt_comm_set_option(mgcmt_plan* plan, int option, int value);
/* halo rows (the exchanged ones, mgcmt_plan_level_halo) of the slots in slot_mask (bit s = slot s) on strip level `level` <-
 * the chain neighbours' boundary rows, one batch; vectors 0..k-1 with k in bits 16-23 of slot_mask (0 = vector 0 only).
 * Adding 0x100 on a ONE-rank communicator treats the strip as a ring (it is its own upper and lower neighbour): a
 * self-test of the transport. */
int mgcmt_halo_exchange(mgcmt_plan* plan, int level, int slot_mask, void* stream);
/* strips of vectors 0..k-1 of (level, slot) of all ranks -> the whole-grid finest level of `coarse` (dst_slot) on every rank */
int mgcmt_gather_coarse(mgcmt_plan* plan, int level, int slot, mgcmt_plan* coarse, int dst_slot, int k, void* stream);
/* host_inout[0..n) <- sum over ranks (norms, inner products: the np.dot / np.linalg.norm call sites); synchronises */
int mgcmt_allreduce_sum(mgcmt_plan* plan, double* host_inout, int n, void* stream);
/* one V(nu1,nu2) cycle (MGCMTSolver.py:281-329) of the sharded hierarchy on vectors 0..k-1 (each with its own shift):
 * `plan` holds the finest levels as row strips, `coarse` the first whole-grid level and everything below it on every
 * rank.  flags: the caller vouches that the halo rows of the fine level's V (nothing but mgcmt_sharded_vcycle wrote V since
 * the previous cycle) / F (since the previous cycle with the same right-hand side) are still the neighbours' rows, which
 * saves their exchange; MGCMT_SHARDED_GRAM_SCHMIDT: vcycle_matrix (:375-436) — modified Gram-Schmidt of the k columns on
 * every non-coarsest level on the way up (:434), on strip levels with ONE all-reduce of the column's coefficients per
 * column (SURVEY par. 8e). */
#define MGCMT_SHARDED_V_HALO_VALID 1
#define MGCMT_SHARDED_F_HALO_VALID 2
#define MGCMT_SHARDED_GRAM_SCHMIDT 4
int mgcmt_sharded_vcycle(mgcmt_plan* plan, mgcmt_plan* coarse, int nu1, int nu2, int nu_coarse, int kind, double omega, int k,
                         int flags, void* stream);

/* ---- general sparse, complex128 operators -------------------------------------------------------
 * The k.p Hamiltonians of ThesisProblem.py:38-40,80,101 / PotWellSolver.py:54-233: an arbitrary square CSR matrix of
 * complex numbers (values = interleaved re, im), cycled as ONE 1-D grid of its full length with the reference's 1-D
 * transfer operators (MGCMTStencilMaker.py:27-78).  The plan builds the Galerkin hierarchy R*A*P (MGCMTSolver.py:318)
 * on the device; vectors are complex (interleaved), slots V, F, T as for mgcmt_plan.  n and lowest are powers of two,
 * lowest <= 64 (the coarsest level is solved by a dense LU with row pivoting, :305-308).  Rows need not be sorted, and
 * stored duplicates of an entry are summed (as scipy treats them): level 0's nnz is the merged count. */
typedef struct mgcmt_csr_plan mgcmt_csr_plan;
int mgcmt_csr_plan_create(int device, int64_t n, int64_t lowest, const int64_t* indptr, const int32_t* indices, const double* values,
                          mgcmt_csr_plan** out);
int mgcmt_csr_plan_destroy(mgcmt_csr_plan* plan);
int mgcmt_csr_num_levels(const mgcmt_csr_plan* plan, int* levels);
/* rows, entries and the chunk length of the lexicographic sweeps (rows solved together as a first-order recurrence) */
int mgcmt_csr_level_info(const mgcmt_csr_plan* plan, int level, int64_t* n, int64_t* nnz, int32_t* lex_chunk_rows);
/* host copy of a level's matrix (indptr[n+1], indices[nnz], values[2*nnz]): what R*A*P gave on the device */
int mgcmt_csr_get_matrix(const mgcmt_csr_plan* plan, int level, int64_t* indptr, int32_t* indices, double* values);
int mgcmt_csr_upload(mgcmt_csr_plan* plan, int level, int slot, const double* re_im, int64_t count, void* stream);
int mgcmt_csr_download(mgcmt_csr_plan* plan, int level, int slot, double* re_im, int64_t count, void* stream);
/* dst <- (A_level - shift I) src */
int mgcmt_csr_apply(mgcmt_csr_plan* plan, int level, int src_slot, int dst_slot, double shift, void* stream);
/* nu sweeps of MGCMT_WJACOBI / MGCMT_GS_LEX / MGCMT_SOR_LEX on V, F of `level` for (A_level - shift I) */
int mgcmt_csr_smooth(mgcmt_csr_plan* plan, int level, int kind, int nu, double omega, double shift, void* stream);
/* one V-cycle (MGCMTSolver.py:281-329) from level 0; nu_coarse: sweeps below the top level (the reference: 4, :320) */
int mgcmt_csr_vcycle(mgcmt_csr_plan* plan, int nu1, int nu2, int nu_coarse, int kind, double omega, double shift, void* stream);

/* plan options: MGCMT_OPT_FUSED (default 1) selects the fused row-streaming kernels on large constant-
 * coefficient levels; 0 forces the one-launch-per-operation kernels everywhere (A/B checks) */
typedef enum mgcmt_option {
  MGCMT_OPT_FUSED = 0,
  MGCMT_OPT_FUSED_ROWS = 1, /* tuning: rows per wave chunk of this plan's fused passes, 0 = auto */
  MGCMT_OPT_RECOMPUTE = 3,  /* default 1: on levels of >= 2^22 points down-leg passes do not store the pre-smoothed iterate and
                               up-leg passes recompute it; 2: on every fused level; 0: never */
  MGCMT_OPT_GRAPH = 2,      /* default 1: mgcmt_vcycle replays its launch sequence as a HIP graph from the second call on */
  MGCMT_OPT_LEX_WAVE = 5,   /* lexicographic Gauss-Seidel / SOR sweeps of constant-coefficient 2-D levels of >= 16 x 16 points run as a
                               pipeline of waves over the whole chip: 2 = bands of 63 rows swept as a wavefront
                               (kernels_lexband.hip), 1 = skewed blocks of 64 columns with a scan per row (kernels_lexwave.hip);
                               0: one workgroup per vector everywhere */
  MGCMT_OPT_LEX_CHAIN = 6,  /* default 1: the nu Gauss-Seidel sweeps of a smoothing step run chained in ONE launch of the scan pipeline
                               (sweep s + 1 follows sweep s a few rows behind); 0: one launch per sweep.  Same arithmetic, same bits */
  MGCMT_OPT_MGS_BLOCK = 7,  /* default 1: modified Gram-Schmidt of 2..12 columns too long for one workgroup (a value > 1: of at least
                               that many points) as two passes over the data (Gram matrix,
                               its Cholesky factor R, Q = A R^-1 — what MGCMTProcessor.py:44-50 computes in exact arithmetic),
                               with the column-by-column kernels taking over on the device where the columns' condition
                               number would let the difference (cond^2 eps) show; 0: column by column always */
  MGCMT_OPT_TWO_LEVEL = 8,  /* default 1: on constant 5-point levels of >= 2^22 points smoothed by weighted Jacobi, the level and its
                               Galerkin level below run as ONE down-leg and ONE up-leg launch (fused2_kernel.h; 2 sweeps per leg
                               on the level below, a no-store last down pass on the level itself, no Gram-Schmidt, no strips):
                               the same arithmetic, the same bits; 2: on every eligible level; 0: never */
  MGCMT_OPT_PCG_MARCH = 9,  /* mgcmt_pcg_iterate on 2-D plans whose level 0 mgcmt_ritz_pair handles in one march (a 5-point operator, with or
                               without a product potential): 1 = direction, operator application and <p, q> as ONE marching launch
                               (32 bytes per point instead of 64; the new direction goes to the spare vector p2, which exchanges its
                               role with p every iteration), 0 = the generic passes; both give the same p and q bit for bit.  Not set
                               (or a negative value): the environment variable MGCMT_PCG_MARCH, read per call, else 1 (the faster
                               iteration at 8192^2) */
  MGCMT_OPT_CARRY = 10,     /* default 1: on fine levels of >= 2^22 points a V(nu1 <= 2, 2) weighted-Jacobi cycle on a nonzero iterate
                               whose top pair runs as two-level passes ends in an up pass that carries the next cycle's F[level+1]
                               (see mgcmt_vcycle); after two carries in a row that the caller let go unused, none is produced until a
                               cycle again follows one with the same arguments; 2: wherever eligible; 0: never.  The same bits */
  MGCMT_OPT_TAIL = 4        /* default 1: the 2-D levels of at most 32 x 32 points below a cycle's top level, coarse solve
                               included, run as ONE launch (needs MGCMT_OPT_FUSED; not with Gram-Schmidt): a dense product
                               with the tail's matrix — the sub-cycle is linear in its right-hand side for fixed shift,
                               smoother and sweep counts; the matrix is formed once per shift set by running the tail on
                               the unit vectors —; 2: the LDS-resident launch of ~45 barrier-separated phases itself (the
                               dense form's arithmetic in another summation order); 0: one launch per pass */
} mgcmt_option;
int mgcmt_plan_set_option(mgcmt_plan* plan, int option, int value);
/* pending = 1 while T[level+1] holds a right-hand side that the last mgcmt_vcycle carried for its successor, else 0 */
int mgcmt_carry_pending(const mgcmt_plan* plan, int* pending);

/* timing of the dominant kernel for bench.py: runs `reps` fine-level smoother sweeps between two
 * HIP events on `stream` and returns the elapsed milliseconds */
int mgcmt_time_smoother(mgcmt_plan* plan, int level, int kind, int nu, double omega, int reps, double* ms_out,
                        void* stream);

/* the same for ONE fused pass of the cycle's timed region (mode as mgcmt_fused_pass: e.g. 2|8 = the fine level's
 * restrict-without-store down pass, 1|(npre<<4) = its recompute + correct + post-smooth up pass): average milliseconds
 * of `reps` launches between two HIP events on `stream` (one untimed launch first) */
int mgcmt_time_fused_pass(mgcmt_plan* plan, int level, int kind, int nsweep, double omega, int mode, int reps, double* ms_out,
                          void* stream);

/* diagnostics of the last lexicographic wave-pipeline sweep (kernels_lexwave.hip): out[0] = blocks started, out[1] = error
 * word (a block timed out), and — only in a build with -DMGCMT_LEXWAVE_DEBUG — per block four words {ticks of the 100 MHz
 * clock spent in the block, rows, slow-path entries, start tick}. */
int mgcmt_lex_wave_stats(mgcmt_plan* plan, uint32_t* out, int64_t capacity);

/* empirical HBM ceilings for bench.py: streams the plan's level-`level` vectors (slots V, F -> T) with a
 * plain grid-stride kernel; kind 0 copy (16 B/point), 1 triad (24 B/point), 2 read-only (8 B/point); kinds 3/4/5 use
 * the fused kernels' access pattern instead (128-column windows marching down `blocks` rows): read 1 stream (8 B),
 * read 2 (16 B), read 2 + write 1 (24 B); kinds 6/7/8 the same with overlapping, unaligned windows (124 of 128 kept),
 * 9/10/11 with the fused kernels' own geometry (112 of 128 kept: line-aligned stores, loads straddling half lines),
 * 12/13/14 with 96 of 128 kept (everything line-aligned), 15/16/17 with 120 of 128 (64-byte-aligned); kinds 20..23 are
 * issue-rate probes — `blocks` workgroups of ONE wave each run 20000 trips of 64 instructions: a chain of dependent double
 * FMAs (20), eight independent chains (21), dependent 32-bit vector adds (22), dependent scalar adds (23); returns the
 * average milliseconds per launch */
int mgcmt_bandwidth_probe(mgcmt_plan* plan, int level, int kind, int blocks, int reps, double* ms_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGCMT_HIP_H */
