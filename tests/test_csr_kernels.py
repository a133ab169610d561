"""Kernel-level tests of the general sparse path (csrc/csr.hip behind multigridcmt_amd/general.py): every kernel against
the extended-precision restatement of tests/csr_reference.py, on matrices whose structure selects every chunk length of
the lexicographic scan (2, 4, ..., 1024; one, two and four chunks of 1024 rows), on the end conditions of the transfers,
on the Galerkin product level by level up to its 96-entry row limit, on a dense solve that has to pivot, and on whole
cycles whose coarse levels provably matter.

Tolerance.  For every case ``e_oracle`` is the distance of the sequential fp64 oracle (oracle/sparse_ref.py's RefSolver
where it has the operation, a float64 run of csr_reference where it has not) from the extended reference on the same
inputs; the kernel has to stay within max(4 e_oracle, 8 eps): the scan rounds in another order than the sequential
recurrence (log2(chunk) compositions in place of one multiply-add per row) and the GPU contracts to FMA where the host
does not, but a kernel with a wrong term is off by orders, not by a factor.  The floor covers an oracle that happens to be
exact.  Tests that compare two runs of the same kernels (duplicates, pointer swap, reuse) are exact.  Every check prints
its figures ("RATIO group backend kernel oracle") before it asserts.
"""
import ctypes
import functools
from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

import numpy as np
import pytest
import scipy.sparse as sp

import csr_reference as cr
from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, _lib
from multigridcmt_amd._lib import GS_LEX, GS_MC, SLOT_F, SLOT_T, SLOT_V, SOR_LEX, WJACOBI, MgcmtError
from oracle.sparse_ref import RefSolver, RefStencilMaker

EPS = cr.EPS
KIND = {"wj": WJACOBI, "gs": GS_LEX, "sor": SOR_LEX}


def _check(group, backend, got, ref, oracle, err=cr.rel_err, what=""):
    e_kernel, e_oracle = err(got, ref), err(oracle, ref)
    print("RATIO %s %s %.3e %.3e %s" % (group, backend, e_kernel, e_oracle, what))
    assert np.all(np.isfinite(np.asarray(got))), what
    assert e_kernel <= max(4.0 * e_oracle, 8.0 * EPS), "%s %s: kernel %.3e, oracle %.3e" % (group, what, e_kernel, e_oracle)


# ---- matrix families --------------------------------------------------------------------------------------------------

def _cnoise(rng, m, scale, real=False):
    re = rng.standard_normal(m)
    im = rng.standard_normal(m)
    return scale * re if real else scale * (re + 1j * im)


def _tridiagonal(n, d, lo, up):
    k = np.arange(n)
    rows = np.concatenate([k, k[1:], k[:-1]])
    cols = np.concatenate([k, k[:-1], k[1:]])
    return sp.csr_matrix((np.concatenate([d, lo, up]), (rows, cols)), shape=(n, n))


def family_T(n, seed=1, real=False):
    """Complex, non-Hermitian, weakly dominant tridiagonal: off-diagonals -1 + e with |e| <~ 0.1, diagonal 2 + d with
    d = -(e_lower + e_upper), so that interior rows sum to zero: a diffusion operator with varying complex coefficients and
    Dirichlet ends.  Laplacian-like (smallest eigenvalues of order 1 / n^2), so coarse levels matter — independent noise on
    the diagonal would localise the lowest modes and lift them to where the smoothers alone reach them.  One scan chunk
    of 1024 rows."""
    rng = np.random.RandomState(seed)
    lo, up = -1.0 + _cnoise(rng, n - 1, 0.04, real), -1.0 + _cnoise(rng, n - 1, 0.04, real)
    d = np.full(n, 2.0, dtype=lo.dtype)
    d[1:] -= lo + 1.0
    d[:-1] -= up + 1.0
    return _tridiagonal(n, d, lo, up)


def family_B(b, seed=2, real=False):
    """Four diagonal blocks of family T and size b; neighbouring blocks coupled by a diagonal plus one off-diagonal (the
    k.p shape): level 0 sweeps in chunks of b rows."""
    rng = np.random.RandomState(seed)
    n = 4 * b
    A = sp.lil_matrix(sp.block_diag([family_T(b, seed + 10 * (i + 1), real) for i in range(4)]), dtype=float if real else complex)
    for blk in range(3):
        for i in range(b):
            r, c = blk * b + i, (blk + 1) * b + i
            A[r, c] = _cnoise(rng, 1, 0.15, real)[0]
            A[c, r] = _cnoise(rng, 1, 0.15, real)[0]
            if i + 1 < b:
                A[r, c + 1] = _cnoise(rng, 1, 0.1, real)[0]
                A[c + 1, r] = _cnoise(rng, 1, 0.1, real)[0]
    return sp.csr_matrix(A)


def family_U(n, seed=3, real=False):
    """Family T plus ~40 symmetric couplings at random distances and one at distance 2 inside an aligned group of four rows
    (7, 5): no chunk structure.  The chunk analysis then gives 2, its smallest result: inside an aligned pair of rows the
    only strictly-lower entry is k-1, so every matrix admits chunk 2 and chunk 1 cannot occur."""
    rng = np.random.RandomState(seed)
    A = sp.lil_matrix(family_T(n, seed + 1, real))
    for _ in range(40):
        i, j = rng.randint(0, n, 2)
        if abs(i - j) > 1:
            A[i, j] = A[j, i] = _cnoise(rng, 1, 0.05, real)[0]
    A[7, 5] = A[5, 7] = _cnoise(rng, 1, 0.05, real)[0]
    return sp.csr_matrix(A)


N_SHIFT = 0.7


def family_N(n, seed=4):
    """Family T with six stretches of 20-40 rows whose sub-diagonal is doubled: with the shift N_SHIFT (inside the
    spectrum) |a_{k,k-1}| > |a_kk - mu| there, so the sweep's multiplier q = -a_{k,k-1} / (a_kk - mu) exceeds 1 in modulus
    (about 1.5) over each stretch and is about 0.77 elsewhere."""
    rng = np.random.RandomState(seed)
    A = sp.lil_matrix(family_T(n, seed + 1))
    starts = np.linspace(60, n - 100, 6).astype(int)
    for s, length in zip(starts, (20, 25, 30, 35, 40, 28)):
        for k in range(s, s + length):
            A[k, k - 1] = 2.0 * A[k, k - 1]
    return sp.csr_matrix(A)


def _rand_vec(n, seed):
    rng = np.random.RandomState(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def _plan(A, lowest):
    from multigridcmt_amd.general import CsrPlan
    return CsrPlan(A, lowest)


# ---- smoothers and operator application at level 0 ------------------------------------------------------------------------

def _smoother_cases():
    cases = []
    for n in (1, 2, 3, 64, 65, 100, 1024, 1025, 2048, 4096):
        cases.append(pytest.param("T", n, 1024, id="T-%d" % n))
    for b in (2, 4, 8, 16, 32, 64, 128, 256, 512):
        cases.append(pytest.param("B", b, b, id="B-%d" % b))
    cases.append(pytest.param("U", 256, 2, id="U-256"))
    cases.append(pytest.param("N", 2048, 1024, id="N-2048"))
    return cases


@functools.lru_cache(maxsize=None)
def _family(name, size):
    A = {"T": family_T, "B": family_B, "U": family_U, "N": family_N}[name](size)
    A.sort_indices()
    return A


@pytest.mark.parametrize("name,size,chunk", _smoother_cases())
def test_apply_and_smoothers_at_level_0(backend, name, size, chunk):
    """apply (mode 0), weighted Jacobi with nu in {0, 1, 3} (odd counts leave the result in the swapped buffer), Gauss-
    Seidel with nu in {1, 3} and SOR with omega in {1.0, 1.2, 0.8}, at shift 0 and at a shift inside the spectrum, on a
    single-level plan whose chunk length is asserted first: chunks 2, 4, ..., 1024 (2 is the smallest the analysis gives), and 1, 2 (1025, 2048) and 4 (4096)
    chunks of 1024 rows, sizes that are no power of two, n below the chunk."""
    A = _family(name, size)
    n = A.shape[0]
    group = "smooth-" + name
    plan = _plan(A, n)
    try:
        assert plan.num_levels == 1 and plan.level_info(0) == (n, A.nnz, chunk)
        Ar = cr.from_scipy(A)
        ref = RefSolver()
        v0, f = _rand_vec(n, 11), _rand_vec(n, 12)
        v0r, fr = cr.vector(v0), cr.vector(f)
        for mu in (0.0, N_SHIFT if name == "N" else 0.5):
            As = (A - mu * sp.eye(n)).tocsr()
            tag = "%s-%d mu=%g " % (name, size, mu)
            plan.upload(0, SLOT_V, v0)
            plan.apply(0, SLOT_V, SLOT_T, shift=mu)
            _check(group, backend, plan.download(0, SLOT_T), cr.apply(Ar, v0r, mu),
                   cr.array(cr.apply(cr.from_scipy(A, "f64"), cr.vector(v0, "f64"), mu), "f64"), what=tag + "apply")
            assert np.array_equal(plan.download(0, SLOT_V), v0)                     # the source is left alone

            def run(kind, nu, omega=1.0):
                plan.upload(0, SLOT_V, v0)
                plan.upload(0, SLOT_F, f)
                plan.smooth(0, kind, nu, omega=omega, shift=mu)
                assert np.array_equal(plan.download(0, SLOT_F), f)
                return plan.download(0, SLOT_V)

            assert np.array_equal(run(WJACOBI, 0, 2.0 / 3.0), v0)
            for nu in (1, 3):
                _check(group, backend, run(WJACOBI, nu, 2.0 / 3.0), cr.wjacobi(Ar, v0r, fr, mu, 2.0 / 3.0, nu),
                       ref.wjacobi(v0, f, As, nu=nu), what=tag + "wjacobi nu=%d" % nu)
            for nu in (1, 3):
                _check(group, backend, run(GS_LEX, nu), cr.gseidel(Ar, v0r, fr, mu, nu), ref.gseidel(v0, f, As, nu=nu),
                       what=tag + "gseidel nu=%d" % nu)
            for omega in (1.0, 1.2, 0.8):
                _check(group, backend, run(SOR_LEX, 2, omega), cr.sor(Ar, v0r, fr, mu, omega, 2), ref.sor(v0, f, As, nu=2, omega=omega),
                       what=tag + "sor omega=%g" % omega)
    finally:
        plan.close()


def test_jacobi_pointer_swap_is_exact(backend):
    """Three sweeps in one call equal three calls of one sweep, bit for bit, and a following apply reads the swapped buffer."""
    A = _family("B", 8)
    n = A.shape[0]
    v0, f = _rand_vec(n, 21), _rand_vec(n, 22)
    plan = _plan(A, n)
    try:
        plan.upload(0, SLOT_V, v0)
        plan.upload(0, SLOT_F, f)
        plan.smooth(0, WJACOBI, 3, omega=0.6, shift=0.3)
        three = plan.download(0, SLOT_V)
        plan.upload(0, SLOT_V, v0)
        for _ in range(3):
            plan.smooth(0, WJACOBI, 1, omega=0.6, shift=0.3)
        assert np.array_equal(plan.download(0, SLOT_V), three)
        assert not np.array_equal(three, v0)
    finally:
        plan.close()


@pytest.mark.parametrize("name,size,lowest", [("T", 64, 32), ("T", 4096, 64), ("B", 64, 64), ("B", 512, 64), ("U", 256, 16), ("N", 2048, 64)])
def test_residual_through_a_cycle_without_sweeps(backend, name, size, lowest):
    """vcycle with nu1 = nu2 = nu_coarse = 0 leaves f - (A - mu I) v of level 0 in its slot T."""
    A = _family(name, size)
    n = A.shape[0]
    v0, f = _rand_vec(n, 31), _rand_vec(n, 32)
    plan = _plan(A, lowest)
    try:
        for mu in (0.0, 0.5):
            plan.upload(0, SLOT_V, v0)
            plan.upload(0, SLOT_F, f)
            plan.vcycle(0, 0, GS_LEX, nu_coarse=0, shift=mu)
            _check("residual", backend, plan.download(0, SLOT_T), cr.residual(cr.from_scipy(A), cr.vector(v0), cr.vector(f), mu),
                   cr.array(cr.residual(cr.from_scipy(A, "f64"), cr.vector(v0, "f64"), cr.vector(f, "f64"), mu), "f64"),
                   what="%s-%d mu=%g" % (name, size, mu))
    finally:
        plan.close()


# ---- transfers --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [4, 8, 128])
def test_transfers_and_their_end_conditions(backend, n):
    """vcycle(0, 0, nu_coarse=0) on a two-level plan from a zero start is exactly P (R A P - mu)^-1 R f.  Right-hand sides
    that are zero except at index n-1, n-2, 0 or 1 expose the end conditions of restriction and interpolation; compared
    elementwise (max |d| over max |ref|)."""
    A = _family("T", n)
    levels = cr.hierarchy(cr.from_scipy(A), n // 2)
    ref, rsm = RefSolver(), RefStencilMaker()
    rhs = []
    for at in (n - 1, n - 2, 0, 1):
        e = np.zeros(n, dtype=complex)
        e[at] = 0.7 - 1.3j
        rhs.append(("delta@%d" % at, e))
    rhs.append(("random", _rand_vec(n, 41)))
    plan = _plan(A, n // 2)
    try:
        assert plan.num_levels == 2
        for mu in (0.0, 0.5):
            for label, f in rhs:
                plan.upload(0, SLOT_V, np.zeros(n, dtype=complex))
                plan.upload(0, SLOT_F, f)
                plan.vcycle(0, 0, WJACOBI, nu_coarse=0, shift=mu)
                want = cr.vcycle(levels, cr.vector(np.zeros(n)), cr.vector(f), mu, 0, 0, 0)
                oracle = ref.vcycle(np.zeros(n, dtype=complex), f, A, rsm, nu1=0, nu2=0, shift=mu, lowest_level=n // 2)
                _check("transfer", backend, plan.download(0, SLOT_V), want, oracle, err=cr.max_err, what="n=%d mu=%g %s" % (n, mu, label))
    finally:
        plan.close()


# ---- Galerkin product -------------------------------------------------------------------------------------------------

def _random_pattern(n=256, per_row=20, seed=5):
    rng = np.random.RandomState(seed)
    rows = np.repeat(np.arange(n), per_row)
    cols = rng.randint(0, n, n * per_row)
    A = sp.coo_matrix((_cnoise(rng, n * per_row, 1.0), (rows, cols)), shape=(n, n)).tocsr()     # (tocsr sums what collides)
    return A + 8.0 * sp.eye(n, format="csr")


def _check_hierarchy(backend, A, lowest, what):
    levels = cr.hierarchy(cr.from_scipy(A), lowest)
    oracle = cr.hierarchy(cr.from_scipy(A, "f64"), lowest)
    plan = _plan(A, lowest)
    try:
        assert plan.num_levels == len(levels)
        for l, (L, O) in enumerate(zip(levels, oracle)):
            C = plan.matrix(l)
            n, nnz, chunk = plan.level_info(l)
            assert (n, nnz) == (L.n, L.nnz), "%s level %d" % (what, l)
            # the structural pattern of R A P, entries that cancel to zero kept; columns sorted within a row
            assert np.array_equal(C.indptr, L.indptr) and np.array_equal(C.indices, L.indices), "%s level %d" % (what, l)
            for k in range(n):
                assert np.all(np.diff(C.indices[C.indptr[k]:C.indptr[k + 1]]) > 0)
            _check("galerkin", backend, C.data, cr.array(L.data), cr.array(O.data, "f64"), what="%s level %d" % (what, l))
            _check("galerkin", backend, C.data, cr.array(L.data), cr.array(O.data, "f64"), err=cr.max_err, what="%s level %d (max)" % (what, l))
    finally:
        plan.close()


@pytest.mark.parametrize("what", ["T-2048", "B-64", "U-256", "random"])
def test_galerkin_product_on_every_level(backend, what):
    """plan.matrix(l) on every level against the dictionary-of-rows triple product: the same sparsity pattern as the
    structural product (the kernel KEEPS an entry whose value cancels to zero: pinned), sorted columns, values."""
    if what == "T-2048":
        _check_hierarchy(backend, _family("T", 2048), 2, what)
    elif what == "B-64":
        _check_hierarchy(backend, _family("B", 64), 4, what)
    elif what == "U-256":
        _check_hierarchy(backend, _family("U", 256), 16, what)
    else:
        _check_hierarchy(backend, _random_pattern(), 16, what)


def test_galerkin_product_keeps_cancelled_entries(backend):
    """tridiag(1, 0, -1): the coarse diagonal cancels to an exact zero and is stored."""
    n = 16
    A = _tridiagonal(n, np.zeros(n, dtype=complex), np.ones(n - 1, dtype=complex), -np.ones(n - 1, dtype=complex))
    plan = _plan(A, 8)
    try:
        C = plan.matrix(1)
        L = cr.rap(cr.from_scipy(A))
        assert np.array_equal(C.indptr, L.indptr) and np.array_equal(C.indices, L.indices)
        stored_zeros = [k for k in range(8) if k in C.indices[C.indptr[k]:C.indptr[k + 1]] and C[k, k] == 0]
        assert stored_zeros
        assert cr.max_err(C.data, cr.array(L.data)) <= 8 * EPS
    finally:
        plan.close()


def _wide_row_matrix(width):
    """Family T at n = 256 plus entries in fine row 101 at odd columns, so that coarse row 50 has exactly ``width`` entries
    (its three fine rows 100, 101, 102 reach the coarse columns 49, 50, 51 through the tridiagonal part)."""
    n = 256
    A = sp.lil_matrix(family_T(n, 6))
    rng = np.random.RandomState(7)
    extra = [J for J in range(n // 2) if J not in (49, 50, 51)][:width - 3]
    for J in extra:
        A[101, 2 * J + 1] = _cnoise(rng, 1, 0.01)[0]
    return sp.csr_matrix(A)


def test_galerkin_row_limit(backend):
    """A coarse row of exactly 96 entries builds and matches; one of 97 is refused with a message that names the limit,
    and the library goes on working."""
    A = _wide_row_matrix(96)
    L = cr.rap(cr.from_scipy(A))
    assert max(L.indptr[k + 1] - L.indptr[k] for k in range(L.n)) == 96 and L.indptr[51] - L.indptr[50] == 96
    _check_hierarchy(backend, A, 64, "row of 96")
    A97 = _wide_row_matrix(97)
    L97 = cr.rap(cr.from_scipy(A97))
    assert L97.indptr[51] - L97.indptr[50] == 97
    with pytest.raises(MgcmtError, match="more than 96 entries"):
        _plan(A97, 64)
    _check_hierarchy(backend, _family("T", 8), 4, "after the refusal")


# ---- coarsest level: dense solve ----------------------------------------------------------------------------------------

def _dense_matrices(n):
    rng = np.random.RandomState(100 + n)
    out = [("random", rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)), 0.0)]
    if n >= 2:
        Z = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        np.fill_diagonal(Z, 0.0)
        out.append(("zero diagonal", Z, 0.0))
        P = 0.05 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) + 2.0 * np.eye(n)
        P[:, 0] *= 0.01
        P[n - 1, 0] = 3.0 - 1.0j                                             # column 0: the pivot is the last row
        out.append(("pivot in the last row", P, 0.0))
    H = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    H = H + H.conj().T
    out.append(("hermitian indefinite", H, 0.37))
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 17, 63, 64])
def test_dense_solve_with_pivoting(backend, n):
    """vcycle on a single-level plan is the dense solve of (A - mu I) x = f: random dense complex matrices, a zero diagonal
    (every column has to pivot; n >= 2, at n = 1 such a matrix is singular), a pivot in the last row (n >= 2), a Hermitian
    indefinite matrix with a shift — against the pivoted extended-precision elimination."""
    f = _rand_vec(n, 51)
    for label, M, mu in _dense_matrices(n):
        A = sp.csr_matrix(M)
        plan = _plan(A, n)
        try:
            plan.upload(0, SLOT_V, _rand_vec(n, 52))
            plan.upload(0, SLOT_F, f)
            plan.vcycle(2, 2, GS_LEX, shift=mu)
            want = cr.dense_solve(cr.from_scipy(A), cr.vector(f), mu)
            oracle = cr.array(cr.dense_solve(cr.from_scipy(A, "f64"), cr.vector(f, "f64"), mu), "f64")
            _check("dense", backend, plan.download(0, SLOT_V), want, oracle, what="n=%d %s" % (n, label))
        finally:
            plan.close()


def test_dense_solve_refuses_65_unknowns(backend):
    A = _family("T", 65)
    plan = _plan(A, 65)
    try:
        plan.upload(0, SLOT_F, _rand_vec(65, 53))
        with pytest.raises(MgcmtError, match="at most 64 unknowns"):
            plan.vcycle(1, 1, GS_LEX)
        plan.smooth(0, GS_LEX, 1)                                            # the plan is still usable
    finally:
        plan.close()


# ---- whole cycles -----------------------------------------------------------------------------------------------------

SMOOTHERS = {"wj": ("wj", 2.0 / 3.0), "gs": ("gs",), "sor": ("sor", 1.2)}
# (smoother, (nu1, nu2), nu_coarse, shift between the first two eigenvalues?, non-zero start?): a covering set, not the
# full product (96 cycles per backend would take minutes of reference time) — each smoother runs with both sweep patterns,
# both coarse counts and both shifts; the non-zero start with weighted Jacobi and SOR
CYCLE_OPTIONS = [
    ("wj", (2, 2), 4, False, False), ("gs", (2, 2), 4, True, False), ("sor", (2, 2), 4, False, True),
    ("wj", (1, 3), 1, True, True), ("gs", (1, 3), 1, False, False), ("sor", (1, 3), 1, True, False),
]
CYCLE_CASES = [("T", 2048, 2), ("T", 2048, 32), ("T", 2048, 64), ("B", 128, 32), ("U", 256, 16)]


@functools.lru_cache(maxsize=None)
def _between_first_two_eigenvalues(name, size):
    from scipy.sparse.linalg import eigs
    A = _family(name, size)
    w = eigs(sp.csc_matrix(A), k=2, sigma=0.0, which="LM", return_eigenvectors=False, v0=np.ones(A.shape[0]))
    w = np.sort(w.real)
    assert w[1] - w[0] > 1e-6 * abs(w[1])
    return float(0.5 * (w[0] + w[1]))


@functools.lru_cache(maxsize=None)
def _levels(name, size, lowest, prec="ld"):
    return cr.hierarchy(cr.from_scipy(_family(name, size), prec), lowest)


@functools.lru_cache(maxsize=None)
def _reference_cycle(name, size, lowest, opt, coarse=True):
    """(inputs, extended reference) of one cycle case; shared by the backends and by the non-vacuity condition."""
    smo, (nu1, nu2), nuc, shifted, nonzero = CYCLE_OPTIONS[opt]
    n = _family(name, size).shape[0]
    mu = _between_first_two_eigenvalues(name, size) if shifted else 0.0
    f = _rand_vec(n, 61)
    v0 = _rand_vec(n, 62) if nonzero else np.zeros(n, dtype=complex)
    x = cr.vcycle(_levels(name, size, lowest), cr.vector(v0), cr.vector(f), mu, nu1, nu2, nuc, SMOOTHERS[smo], coarse_correction=coarse)
    x = cr.array(x)
    x.setflags(write=False)
    return v0, f, mu, x


def _oracle_cycle(name, size, lowest, opt, v0, f, mu):
    smo, (nu1, nu2), nuc, _, _ = CYCLE_OPTIONS[opt]
    if nuc != 4:        # RefSolver runs V(4,4) below the top level and nothing else: the float64 run of the restatement
        return cr.array(cr.vcycle(_levels(name, size, lowest, "f64"), cr.vector(v0, "f64"), cr.vector(f, "f64"), mu, nu1, nu2, nuc,
                                  SMOOTHERS[smo]), "f64")
    ref = RefSolver()
    fn = {"wj": ref.wjacobi, "gs": ref.gseidel, "sor": lambda v, f, A, nu=4: ref.sor(v, f, A, nu=nu, omega=1.2)}[smo]
    return ref.vcycle(v0, f, _family(name, size), RefStencilMaker(), nu1=nu1, nu2=nu2, smoother=fn, shift=mu, lowest_level=lowest)


@pytest.mark.parametrize("opt", range(len(CYCLE_OPTIONS)))
@pytest.mark.parametrize("name,size,lowest", CYCLE_CASES)
def test_whole_cycle(backend, name, size, lowest, opt):
    """One V-cycle against the extended reference, and again on the same plan (the same bits).  Non-vacuity, asserted on
    the reference alone: the cycle with its coarse correction replaced by zero differs from the cycle by more than 1e-3."""
    smo, (nu1, nu2), nuc, _, _ = CYCLE_OPTIONS[opt]
    v0, f, mu, want = _reference_cycle(name, size, lowest, opt)
    without = _reference_cycle(name, size, lowest, opt, coarse=False)[3]
    assert cr.rel_err(without, want) > 1e-3
    A = _family(name, size)
    plan = _plan(A, lowest)
    try:
        runs = []
        for _ in range(2):
            plan.upload(0, SLOT_V, v0)
            plan.upload(0, SLOT_F, f)
            plan.vcycle(nu1, nu2, KIND[smo], omega=SMOOTHERS[smo][-1] if smo != "gs" else 1.0, nu_coarse=nuc, shift=mu)
            runs.append(plan.download(0, SLOT_V))
        assert np.array_equal(runs[0], runs[1])
        _check("cycle-" + name, backend, runs[0], want, _oracle_cycle(name, size, lowest, opt, v0, f, mu),
               what="%s-%d lowest=%d %s V(%d,%d) nu_coarse=%d mu=%.3g" % (name, size, lowest, smo, nu1, nu2, nuc, mu))
    finally:
        plan.close()


@pytest.mark.parametrize("opt", range(len(CYCLE_OPTIONS)))
def test_the_levels_below_64_matter(opt):
    """Non-vacuity of the lowest_level cases, on the reference alone: the cycles of family T with lowest 2 and lowest 64
    differ by more than 1e-3, so a cycle with broken levels below 64 unknowns cannot pass test_whole_cycle."""
    deep, shallow = _reference_cycle("T", 2048, 2, opt)[3], _reference_cycle("T", 2048, 64, opt)[3]
    assert cr.rel_err(deep, shallow) > 1e-3


# ---- through the drop-in class ----------------------------------------------------------------------------------------

def _pair(op, A, v, f, mu=0.0, nu=2, omega=1.2, lowest=8):
    """(extended reference, fp64 oracle) of a smoother ("wj", "gs", "sor") or of a V(2,2) Gauss-Seidel cycle ("cycle")."""
    L, rv, rf = cr.from_scipy(A), cr.vector(v), cr.vector(f)
    ref = RefSolver()
    As = (sp.csr_matrix(A) - mu * sp.eye(A.shape[0])).tocsr()
    if op == "wj":
        return cr.wjacobi(L, rv, rf, mu, 2.0 / 3.0, nu), ref.wjacobi(v, f, As, nu=nu)
    if op == "gs":
        return cr.gseidel(L, rv, rf, mu, nu), ref.gseidel(v, f, As, nu=nu)
    if op == "sor":
        return cr.sor(L, rv, rf, mu, omega, nu), ref.sor(v, f, As, nu=nu, omega=omega)
    return (cr.vcycle(cr.hierarchy(L, lowest), rv, rf, mu, 2, 2, 4, ("gs",)),
            ref.vcycle(v, f, A, RefStencilMaker(), nu1=2, nu2=2, smoother=ref.gseidel, shift=mu, lowest_level=lowest))


def _assert_general(A):
    from multigridcmt_amd.operators import UnrecognisedOperator, recognise
    with pytest.raises(UnrecognisedOperator):
        recognise(A, "1d")


def test_drop_in_class_dtypes_and_shapes(backend):
    """Real in gives real out; a complex v0, f or A gives complex out; (n, 1) from the smoothers and from a cycle whose grid
    already is the lowest level; values against the reference."""
    solver, sm = MGCMTSolver(), MGCMTStencilMaker()
    n = 64
    Ar, Ac = family_U(n, 8, real=True), _family("B", 16)
    _assert_general(Ar)
    _assert_general(Ac)
    rng = np.random.RandomState(71)
    vr, fr = rng.standard_normal(n), rng.standard_normal(n)
    vc, fc = _rand_vec(n, 72), _rand_vec(n, 73)
    for A, v, f, is_complex in ((Ar, vr, fr, False), (Ar, vc, fr, True), (Ar, vr, fc, True), (Ac, vr, fr, True)):
        for op, fn in (("wj", solver.wjacobi), ("gs", solver.gseidel), ("sor", functools.partial(solver.sor, omega=1.2))):
            x = fn(v.copy(), f.copy(), A, nu=3)
            assert x.shape == (n, 1) and np.iscomplexobj(x) == is_complex
            _check("drop-in", backend, x, *_pair(op, A, v, f, nu=3), what=op)
        x = solver.vcycle(v.copy(), f.copy(), A, sm, nu1=2, nu2=2, shift=0.1, lowest_level=8, smoother=solver.gseidel)
        assert x.shape == (n,) and np.iscomplexobj(x) == is_complex
        _check("drop-in", backend, x, *_pair("cycle", A, v, f, mu=0.1), what="vcycle")
        x = solver.vcycle(v.copy(), f.copy(), A, sm, shift=0.1, lowest_level=n, smoother=solver.gseidel)
        assert x.shape == (n, 1) and np.iscomplexobj(x) == is_complex
        _check("drop-in", backend, x, cr.dense_solve(cr.from_scipy(A), cr.vector(f), 0.1),
               cr.array(cr.dense_solve(cr.from_scipy(A, "f64"), cr.vector(f, "f64"), 0.1), "f64"), what="lowest = n")


def test_drop_in_class_refusals(backend):
    solver, sm = MGCMTSolver(), MGCMTStencilMaker()
    A = _family("T", 64)
    v, f = np.zeros(64, dtype=complex), _rand_vec(64, 74)
    with pytest.raises(NotImplementedError, match="complex shift"):
        solver.vcycle(v.copy(), f.copy(), A, sm, shift=0.1 + 0.2j, lowest_level=8, smoother=solver.gseidel)
    with pytest.raises(NotImplementedError, match="wjacobi / gseidel / sor"):
        solver.vcycle(v.copy(), f.copy(), A, sm, lowest_level=8, smoother=lambda v0, f, A, nu=4: v0)
    assert solver.vcycle(v.copy(), f.copy(), A, sm, lowest_level=8, smoother=solver.gseidel).shape == (64,)


def test_drop_in_class_sees_a_matrix_mutated_in_place(backend):
    """The plan cache is keyed by content: A.data *= 2 between two calls gives the new operator's result."""
    solver, sm = MGCMTSolver(), MGCMTStencilMaker()
    A = family_T(64, 9)
    f = _rand_vec(64, 75)
    zero = np.zeros(64, dtype=complex)
    first = solver.vcycle(zero.copy(), f.copy(), A, sm, nu1=2, nu2=2, lowest_level=8, smoother=solver.gseidel)
    A.data *= 2
    second = solver.vcycle(zero.copy(), f.copy(), A, sm, nu1=2, nu2=2, lowest_level=8, smoother=solver.gseidel)
    want, oracle = _pair("cycle", A, zero, f)
    _check("drop-in", backend, second, want, oracle, what="cycle after A.data *= 2")
    assert cr.rel_err(first, want) > 0.1
    A.data *= 2
    _check("drop-in", backend, solver.gseidel(zero.copy(), f.copy(), A, nu=1), *_pair("gs", A, zero, f, nu=1), what="gseidel after A.data *= 2")


# ---- duplicate entries ------------------------------------------------------------------------------------------------

def _with_duplicates(A):
    """The same operator with three stored duplicates (a diagonal, a sub-diagonal and a far entry split in two), built as
    raw CSR arrays so that nothing sums them on the way, and its summed form."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    split = {(5, 5), (9, 8), (20, 3)}
    rng = np.random.RandomState(81)
    indptr, indices, data = [0], [], []
    for k in range(n):
        row = []
        for e in range(A.indptr[k], A.indptr[k + 1]):
            j, a = int(A.indices[e]), A.data[e]
            if (k, j) in split:
                part = a * (0.3 + 0.2 * rng.standard_normal()) + 0.5
                row += [(j, part), (j, a - part)]
                split.discard((k, j))
            else:
                row.append((j, a))
        row = [row[i] for i in rng.permutation(len(row))]               # unsorted rows too
        indices += [j for j, _ in row]
        data += [a for _, a in row]
        indptr.append(len(indices))
    assert not split
    D = sp.csr_matrix((np.array(data), np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int32)), shape=(n, n))
    assert D.nnz == A.nnz + 3
    S = D.copy()
    S.sum_duplicates()
    assert S.nnz == A.nnz
    return D, S


def _duplicate_base():
    A = sp.lil_matrix(family_T(64, 10))
    A[20, 3] = 0.4 - 0.3j
    return sp.csr_matrix(A)


def test_duplicates_through_the_drop_in_class(backend):
    """A matrix with stored duplicates gives the results of its summed form, bit for bit, through all three smoothers and
    a cycle, agrees with the reference (which sums them), and is not modified."""
    solver, sm = MGCMTSolver(), MGCMTStencilMaker()
    D, S = _with_duplicates(_duplicate_base())
    keep = (D.data.copy(), D.indices.copy(), D.indptr.copy())
    n = D.shape[0]
    v, f = _rand_vec(n, 82), _rand_vec(n, 83)
    assert cr.from_scipy(D).nnz == S.nnz                                     # (the reference sums them as well)
    calls = [(lambda A: solver.wjacobi(v.copy(), f.copy(), A, nu=2), _pair("wj", D, v, f)),
             (lambda A: solver.gseidel(v.copy(), f.copy(), A, nu=2), _pair("gs", D, v, f)),
             (lambda A: solver.sor(v.copy(), f.copy(), A, nu=2, omega=1.2), _pair("sor", D, v, f)),
             (lambda A: solver.vcycle(v.copy(), f.copy(), A, sm, nu1=2, nu2=2, shift=0.2, lowest_level=8, smoother=solver.gseidel),
              _pair("cycle", D, v, f, mu=0.2))]
    for call, (want, oracle) in calls:
        got = call(D)
        assert np.array_equal(got, call(S))
        _check("duplicates", backend, got, want, oracle)
    assert all(np.array_equal(a, b) for a, b in zip(keep, (D.data, D.indices, D.indptr)))
    from multigridcmt_amd.general import CsrPlan
    plan = CsrPlan(D, 8)
    try:
        assert plan.level_info(0)[1] == S.nnz
    finally:
        plan.close()
    assert all(np.array_equal(a, b) for a, b in zip(keep, (D.data, D.indices, D.indptr)))


# ---- the C-ABI, directly ------------------------------------------------------------------------------------------------

ERR_INVALID, ERR_UNSUPPORTED = -1, -4


def _c_create(n, lowest, indptr, indices, data):
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    values = np.ascontiguousarray(np.asarray(data, dtype=np.complex128)).view(np.float64)
    h = c_void_p()
    rc = _lib.lib().mgcmt_csr_plan_create(0, n, lowest, indptr.ctypes.data_as(POINTER(c_int64)), indices.ctypes.data_as(POINTER(c_int32)),
                                          _lib.as_dp(values), ctypes.byref(h))
    return rc, h


def _last_error():
    return (_lib.lib().mgcmt_last_error() or b"").decode()


def test_c_entry_sorts_and_merges_rows(backend):
    """mgcmt_csr_plan_create with unsorted, duplicated rows: level 0 comes back sorted and merged with the merged count, and
    smoothers and a cycle give the bits of the plan created from the summed form."""
    D, S = _with_duplicates(_duplicate_base())
    S.sort_indices()
    n = D.shape[0]
    v, f = _rand_vec(n, 84), _rand_vec(n, 85)
    lib = _lib.lib()
    outs = []
    for M in (D, S):
        rc, h = _c_create(n, 8, M.indptr, M.indices, M.data)
        assert rc == 0, _last_error()
        try:
            nn, nnz, chunk = c_int64(0), c_int64(0), c_int32(0)
            assert lib.mgcmt_csr_level_info(h, 0, ctypes.byref(nn), ctypes.byref(nnz), ctypes.byref(chunk)) == 0
            assert (nn.value, nnz.value, chunk.value) == (n, S.nnz, 16)          # (the far entry (20, 3) lies before the 16 rows of its chunk)
            indptr, indices, values = np.zeros(n + 1, dtype=np.int64), np.zeros(nnz.value, dtype=np.int32), np.zeros(2 * nnz.value)
            assert lib.mgcmt_csr_get_matrix(h, 0, indptr.ctypes.data_as(POINTER(c_int64)), indices.ctypes.data_as(POINTER(c_int32)),
                                            _lib.as_dp(values)) == 0
            assert np.array_equal(indptr, S.indptr) and np.array_equal(indices, S.indices)
            assert np.array_equal(values.view(np.complex128), S.data)
            res = []
            for kind, omega in ((WJACOBI, 0.6), (GS_LEX, 1.0), (SOR_LEX, 1.2), (None, 1.0)):
                for slot, x in ((SLOT_V, v), (SLOT_F, f)):
                    x = np.ascontiguousarray(x)
                    assert lib.mgcmt_csr_upload(h, 0, slot, _lib.as_dp(x.view(np.float64)), n, None) == 0
                if kind is None:
                    assert lib.mgcmt_csr_vcycle(h, 2, 2, 4, GS_LEX, c_double(1.0), c_double(0.2), None) == 0
                else:
                    assert lib.mgcmt_csr_smooth(h, 0, kind, 2, c_double(omega), c_double(0.2), None) == 0
                out = np.empty(n, dtype=np.complex128)
                assert lib.mgcmt_csr_download(h, 0, SLOT_V, _lib.as_dp(out.view(np.float64)), n, None) == 0
                res.append(out)
            outs.append(res)
        finally:
            lib.mgcmt_csr_plan_destroy(h)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    _check("duplicates", backend, outs[0][1], *_pair("gs", D, v, f, mu=0.2), what="C entry, gseidel")
    _check("duplicates", backend, outs[0][3], *_pair("cycle", D, v, f, mu=0.2), what="C entry, cycle")


def test_c_entry_refusals(backend):
    """Every refusal returns its documented code, sets mgcmt_last_error and leaves the library and the plan usable.  All of
    them are host-side argument checks that return before any kernel launch (read in csrc/csr.hip: the creation checks run
    before the first device allocation of a level; upload / download / apply / smooth / vcycle check before they enqueue;
    an unsupported smoother kind is refused by smooth() before its first launch, and in a cycle at level 0, before anything
    of the cycle has been launched)."""
    lib = _lib.lib()
    A = _family("T", 16)
    n = 16
    ip, ix, da = A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data

    def refused(code, text, n_, lowest, indptr, indices, data=da):
        rc, h = _c_create(n_, lowest, indptr, indices, data)
        assert rc == code and not h.value, (rc, text)
        assert text in _last_error(), _last_error()

    bad = ip.copy()
    bad[0] = 1
    refused(ERR_INVALID, "indptr[0] must be 0", n, 4, bad, ix)
    bad = ip.copy()
    bad[5] = bad[4] - 1
    refused(ERR_INVALID, "non-decreasing", n, 4, bad, ix)
    for col in (-1, n):
        bad = ix.copy()
        bad[7] = col
        refused(ERR_INVALID, "column index out of range", n, 4, ip, bad)
    A12 = family_T(12, 1)
    refused(ERR_INVALID, "powers of two", 12, 4, A12.indptr, A12.indices, A12.data)
    A256 = family_T(256, 1)
    refused(ERR_UNSUPPORTED, "at most 64 unknowns", 256, 128, A256.indptr, A256.indices, A256.data)

    rc, h = _c_create(n, 4, ip, ix, da)
    assert rc == 0, _last_error()
    try:
        v, f = _rand_vec(n, 91), _rand_vec(n, 92)
        buf = np.zeros(2 * n)

        def valid():
            """a following valid call works and gives what it gave before"""
            for slot, x in ((SLOT_V, v), (SLOT_F, f)):
                assert lib.mgcmt_csr_upload(h, 0, slot, _lib.as_dp(np.ascontiguousarray(x).view(np.float64)), n, None) == 0
            assert lib.mgcmt_csr_vcycle(h, 1, 1, 2, GS_LEX, c_double(1.0), c_double(0.0), None) == 0
            out = np.empty(n, dtype=np.complex128)
            assert lib.mgcmt_csr_download(h, 0, SLOT_V, _lib.as_dp(out.view(np.float64)), n, None) == 0
            return out

        first = valid()
        calls = [
            ("bad slot or count", ERR_INVALID, lambda: lib.mgcmt_csr_upload(h, 0, 3, _lib.as_dp(buf), n, None)),
            ("bad slot or count", ERR_INVALID, lambda: lib.mgcmt_csr_upload(h, 0, -1, _lib.as_dp(buf), n, None)),
            ("bad slot or count", ERR_INVALID, lambda: lib.mgcmt_csr_download(h, 0, 3, _lib.as_dp(buf), n, None)),
            ("bad slot or count", ERR_INVALID, lambda: lib.mgcmt_csr_upload(h, 0, SLOT_V, _lib.as_dp(buf), n - 1, None)),
            ("bad slot or count", ERR_INVALID, lambda: lib.mgcmt_csr_download(h, 0, SLOT_V, _lib.as_dp(buf), n + 1, None)),
            ("bad slot or count", ERR_INVALID, lambda: lib.mgcmt_csr_upload(h, 1, SLOT_V, _lib.as_dp(buf), n, None)),
            ("apply: bad slots", ERR_INVALID, lambda: lib.mgcmt_csr_apply(h, 0, SLOT_V, SLOT_V, c_double(0.0), None)),
            ("apply: bad slots", ERR_INVALID, lambda: lib.mgcmt_csr_apply(h, 0, SLOT_V, 3, c_double(0.0), None)),
            ("nu must be >= 0", ERR_INVALID, lambda: lib.mgcmt_csr_smooth(h, 0, GS_LEX, -1, c_double(1.0), c_double(0.0), None)),
            ("sweep counts must be >= 0", ERR_INVALID, lambda: lib.mgcmt_csr_vcycle(h, 1, -1, 4, GS_LEX, c_double(1.0), c_double(0.0), None)),
            ("sweep counts must be >= 0", ERR_INVALID, lambda: lib.mgcmt_csr_vcycle(h, 1, 1, -4, GS_LEX, c_double(1.0), c_double(0.0), None)),
            ("level out of range", ERR_INVALID, lambda: lib.mgcmt_csr_smooth(h, 3, GS_LEX, 1, c_double(1.0), c_double(0.0), None)),
            ("level out of range", ERR_INVALID, lambda: lib.mgcmt_csr_apply(h, -1, SLOT_V, SLOT_T, c_double(0.0), None)),
            ("level out of range", ERR_INVALID, lambda: lib.mgcmt_csr_level_info(h, 3, None, None, None)),
            ("take wjacobi, gseidel and sor", ERR_UNSUPPORTED, lambda: lib.mgcmt_csr_smooth(h, 0, GS_MC, 1, c_double(1.0), c_double(0.0), None)),
            ("take wjacobi, gseidel and sor", ERR_UNSUPPORTED, lambda: lib.mgcmt_csr_vcycle(h, 1, 1, 2, GS_MC, c_double(1.0), c_double(0.0), None)),
            ("take wjacobi, gseidel and sor", ERR_UNSUPPORTED, lambda: lib.mgcmt_csr_smooth(h, 0, 17, 1, c_double(1.0), c_double(0.0), None)),
        ]
        for text, code, call in calls:
            assert call() == code, text
            assert text in _last_error(), (text, _last_error())
            assert np.array_equal(valid(), first), text
    finally:
        lib.mgcmt_csr_plan_destroy(h)
