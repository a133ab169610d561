"""Extended-precision restatement of the general sparse path (csrc/csr.hip), for tests/test_csr_kernels.py.

Plain row loops over CSR arrays (indptr, indices, data) in np.longdouble / np.clongdouble, everything sequential and
in index order: (A - mu I) x and the residual, weighted Jacobi, the generalised lexicographic sweep documented at
k_csr_lex with its parameters (alpha, beta, wU, wL) — Gauss-Seidel and the reference's SOR with its (D-L)^-1
right-hand side follow from it —, 1-D full weighting and linear interpolation with their end conditions, R A P as a
dictionary-of-rows triple product, Gaussian elimination with partial pivoting, and the V-cycle assembled from those
pieces (V(nu1, nu2) on top, V(nu_coarse, nu_coarse) below, zero start on the coarse levels).

Independent of oracle/sparse_ref.py and of the code under test: no scipy arithmetic, no dense n x n matrix except in the
elimination (at most 64 unknowns there).  ``prec="f64"`` runs the same statements in float64 / complex128: the
sequential fp64 oracle for operations oracle/sparse_ref.py does not have.  Stored duplicates of an entry are summed, as
scipy treats them.
"""
import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not an extended-precision type on this platform"

EPS = float(np.finfo(np.float64).eps)
_TYPES = {"ld": (np.longdouble, np.clongdouble), "f64": (np.float64, np.complex128)}


class Csr:
    """Canonical CSR (columns sorted, duplicates summed) with data held as a list of scalars of the working type."""

    def __init__(self, n, indptr, indices, data, prec):
        self.n, self.indptr, self.indices, self.data, self.prec = n, indptr, indices, data, prec
        self.R, self.C = _TYPES[prec]

    def row(self, k):
        s, e = self.indptr[k], self.indptr[k + 1]
        return self.indices[s:e], self.data[s:e]

    @property
    def nnz(self):
        return self.indptr[-1]


def _from_rows(n, rows, prec):
    indptr, indices, data = [0], [], []
    for row in rows:
        for j in sorted(row):
            indices.append(j)
            data.append(row[j])
        indptr.append(len(indices))
    return Csr(n, indptr, indices, data, prec)


def from_arrays(n, indptr, indices, data, prec="ld"):
    """CSR arrays as a caller may hand them over (unsorted rows, duplicates) in canonical form."""
    C = _TYPES[prec][1]
    rows = []
    for k in range(n):
        row = {}
        for e in range(int(indptr[k]), int(indptr[k + 1])):
            j = int(indices[e])
            row[j] = row[j] + C(data[e]) if j in row else C(data[e])
        rows.append(row)
    return _from_rows(n, rows, prec)


def from_scipy(A, prec="ld"):
    A = A.tocsr()
    return from_arrays(A.shape[0], A.indptr, A.indices, A.data, prec)


def vector(x, prec="ld"):
    C = _TYPES[prec][1]
    return [C(v) for v in np.asarray(x).reshape(-1)]


def array(x, prec="ld"):
    return np.array(x, dtype=_TYPES[prec][1])


def rel_err(got, ref):
    """conftest.rel_err carried out in extended precision (the reference is not rounded to float64 first)."""
    got = np.asarray(got).reshape(-1).astype(np.clongdouble)
    ref = np.asarray(ref).reshape(-1).astype(np.clongdouble)
    num = np.sqrt(np.sum(np.abs(got - ref) ** 2))
    den = np.sqrt(np.sum(np.abs(ref) ** 2))
    return float(num / max(den, np.longdouble(1e-300)))


def max_err(got, ref):
    """Elementwise: max |got - ref| over max |ref|."""
    got = np.asarray(got).reshape(-1).astype(np.clongdouble)
    ref = np.asarray(ref).reshape(-1).astype(np.clongdouble)
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), np.longdouble(1e-300)))


# ---- operator application ---------------------------------------------------------------------------------------------

def apply(A, x, mu=0.0):
    """(A - mu I) x."""
    mu = A.R(mu)
    out = []
    for k in range(A.n):
        cols, vals = A.row(k)
        acc = A.C(0)
        for j, a in zip(cols, vals):
            acc = acc + a * x[j]
        out.append(acc - mu * x[k])
    return out


def residual(A, x, f, mu=0.0):
    """f - (A - mu I) x."""
    return [fk - ak for fk, ak in zip(f, apply(A, x, mu))]


def _diagonal(A, mu):
    d = []
    for k in range(A.n):
        cols, vals = A.row(k)
        dk = A.C(0)
        for j, a in zip(cols, vals):
            if j == k:
                dk = dk + a
        d.append(dk - mu)
    return d


def wjacobi(A, x, f, mu=0.0, omega=2.0 / 3.0, nu=1):
    """x <- x + omega (f - (A - mu I) x) / (a_kk - mu), nu times."""
    mu, omega = A.R(mu), A.R(omega)
    d = _diagonal(A, mu)
    x = list(x)
    for _ in range(nu):
        r = residual(A, x, f, mu)
        x = [xk + omega * (rk / dk) for xk, rk, dk in zip(x, r, d)]
    return x


# ---- the generalised lexicographic sweep ------------------------------------------------------------------------------

def lex_sweep(A, x, f, mu, alpha, beta, wU, wL):
    """x_k <- (alpha d_k x_k + beta f_k - wU sum_{j>k} a_kj x_j - wL sum_{j<k} a_kj x_j^new) / d_k, d_k = a_kk - mu,
    for k = 0, 1, ... in this order."""
    mu, alpha, beta, wU, wL = (A.R(v) for v in (mu, alpha, beta, wU, wL))
    x = list(x)
    for k in range(A.n):
        cols, vals = A.row(k)
        d, lower, upper = A.C(0) - mu, A.C(0), A.C(0)
        for j, a in zip(cols, vals):
            if j == k:
                d = d + a
            elif j > k:
                upper = upper + a * x[j]
            else:
                lower = lower + a * x[j]
        x[k] = (alpha * (d * x[k]) + beta * f[k] - wU * upper - wL * lower) / d
    return x


def gseidel(A, x, f, mu=0.0, nu=1):
    for _ in range(nu):
        x = lex_sweep(A, x, f, mu, 0.0, 1.0, 1.0, 1.0)
    return list(x)


def sor(A, x, f, mu=0.0, omega=1.0, nu=1):
    """x <- (D - wL)^-1 ((1 - w) D + wU) x + w (D - L)^-1 f: the right-hand side goes through (D - L), not (D - wL)."""
    g = lex_sweep(A, [A.C(0)] * A.n, f, mu, 0.0, 1.0, 0.0, 1.0)
    w = A.R(omega)
    x = list(x)
    for _ in range(nu):
        x = lex_sweep(A, x, f, mu, 1.0 - omega, 0.0, omega, omega)
        x = [xk + w * gk for xk, gk in zip(x, g)]
    return x


def smooth(A, x, f, mu, smoother, nu):
    """smoother: ("wj", omega) | ("gs",) | ("sor", omega)."""
    if smoother[0] == "wj":
        return wjacobi(A, x, f, mu, smoother[1], nu)
    if smoother[0] == "gs":
        return gseidel(A, x, f, mu, nu)
    if smoother[0] == "sor":
        return sor(A, x, f, mu, smoother[1], nu)
    raise ValueError(smoother)


# ---- transfers --------------------------------------------------------------------------------------------------------

def restrict(r):
    """coarse_I = r_{2I}/4 + r_{2I+1}/2 + r_{2I+2}/4, with r = 0 past the end."""
    n = len(r)
    zero = r[0] - r[0]
    quarter, half = type(r[0])(0.25), type(r[0])(0.5)
    return [quarter * r[2 * i] + half * r[2 * i + 1] + quarter * (r[2 * i + 2] if 2 * i + 2 < n else zero) for i in range(n // 2)]


def prolong(e, n):
    """(P e)_k: odd k takes e_{(k-1)/2}; even k takes (e_{k/2-1} + e_{k/2}) / 2 with e_{-1} = 0."""
    zero = e[0] - e[0]
    half = type(e[0])(0.5)
    out = []
    for k in range(n):
        if k % 2:
            out.append(e[(k - 1) // 2])
        else:
            out.append(half * ((e[k // 2 - 1] if k >= 2 else zero) + e[k // 2]))
    return out


def rap(A):
    """R A P with the transfers above, row by row; an entry that is structurally there is kept even when its value
    cancels to zero."""
    nc = A.n // 2
    half = A.R(0.5)
    weights = (A.R(0.25), A.R(0.5), A.R(0.25))
    rows = []
    for i in range(nc):
        row = {}

        def add(j, v):
            if 0 <= j < nc:
                row[j] = row[j] + v if j in row else v

        for t in range(3):
            a = 2 * i + t
            if a >= A.n:
                continue
            cols, vals = A.row(a)
            for b, v in zip(cols, vals):
                v = weights[t] * v
                if b % 2:
                    add((b - 1) // 2, v)
                else:
                    add(b // 2, half * v)
                    add(b // 2 - 1, half * v)
        rows.append(row)
    return _from_rows(nc, rows, A.prec)


def hierarchy(A, lowest):
    levels = [A]
    while levels[-1].n > lowest:
        levels.append(rap(levels[-1]))
    return levels


# ---- coarsest level ---------------------------------------------------------------------------------------------------

def dense_solve(A, f, mu=0.0):
    """(A - mu I) x = f by Gaussian elimination with partial pivoting (largest modulus in the column, the first of equals)."""
    n = A.n
    assert n <= 64
    mu = A.R(mu)
    m = [[A.C(0)] * n for _ in range(n)]
    for k in range(n):
        cols, vals = A.row(k)
        for j, a in zip(cols, vals):
            m[k][j] = m[k][j] + a
        m[k][k] = m[k][k] - mu
    b = list(f)
    for c in range(n):
        best, bestv = c, abs(m[c][c])
        for r in range(c + 1, n):
            if abs(m[r][c]) > bestv:
                best, bestv = r, abs(m[r][c])
        if best != c:
            m[c], m[best] = m[best], m[c]
            b[c], b[best] = b[best], b[c]
        for r in range(c + 1, n):
            l = m[r][c] / m[c][c]
            for j in range(c + 1, n):
                m[r][j] = m[r][j] - l * m[c][j]
            b[r] = b[r] - l * b[c]
    for r in range(n - 1, -1, -1):
        acc = b[r]
        for j in range(r + 1, n):
            acc = acc - m[r][j] * b[j]
        b[r] = acc / m[r][r]
    return b


# ---- the V-cycle ------------------------------------------------------------------------------------------------------

def vcycle(levels, v0, f, mu=0.0, nu1=4, nu2=4, nu_coarse=4, smoother=("wj", 2.0 / 3.0), coarse_correction=True):
    """One V-cycle for (A - mu I) v = f on ``hierarchy(A, lowest)``.  ``coarse_correction=False`` replaces the
    correction that comes up from level 1 by zero (what a cycle with useless coarse levels would compute)."""
    last = len(levels) - 1
    C = levels[0].C
    if last == 0:
        return dense_solve(levels[0], f, mu)
    vs, fs = [list(v0)], [list(f)]
    for l in range(last):
        A = levels[l]
        if l > 0:
            vs.append([C(0)] * A.n)
        vs[l] = smooth(A, vs[l], fs[l], mu, smoother, nu1 if l == 0 else nu_coarse)
        fs.append(restrict(residual(A, vs[l], fs[l], mu)))
        if l == 0 and not coarse_correction:
            return smooth(A, vs[0], fs[0], mu, smoother, nu2)
    vs.append(dense_solve(levels[last], fs[last], mu))
    for l in range(last - 1, -1, -1):
        A = levels[l]
        e = prolong(vs[l + 1], A.n)
        vs[l] = [vk + ek for vk, ek in zip(vs[l], e)]
        vs[l] = smooth(A, vs[l], fs[l], mu, smoother, nu2 if l == 0 else nu_coarse)
    return vs[0]
