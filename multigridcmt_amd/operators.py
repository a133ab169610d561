"""Structured description of the operators the reference hands to its solver.

The reference passes ``scipy.sparse`` matrices built by ``MGCMTStencilMaker.laplacian``
(MGCMTStencilMaker.py:15-25), usually pre-scaled — ``(-1 / np.pi ** 2) * laplacian``
(1DPotMatrixVcycle.py:16, 2DPotMatrixVcycle.py:27) — and sometimes pre-shifted (``A - mu*I`` handed to
a smoother, MGCMTSolver.py:313).  The kernels are matrix-free: they need the operator as a sum of
Kronecker products of tridiagonal factors,  A = sum_m X_m (x) Y_m  (rows (x) columns).  This module
recovers that form from a sparse matrix by an O(nnz) structural check (``recognise``) and offers a
matrix-free operator object (``StructuredOperator``) for grids too large to assemble.
"""
import hashlib
import math

import numpy as np
import scipy.sparse as sp


def tri_identity(n):
    t = np.zeros((3, n))
    t[1] = 1.0
    return t


def tri_laplacian(n):
    """MGCMTStencilMaker.py:17-21 — tridiag(1,-2,1) * (1/h**2), h = 1./n (same float expression)."""
    h = 1. / n
    s = 1 / h ** 2
    t = np.zeros((3, n))
    t[0, 1:] = 1.0 * s
    t[1] = -2.0 * s
    t[2, :-1] = 1.0 * s
    return t


def tri_to_sparse(t):
    n = t.shape[1]
    return sp.diags([t[0, 1:], t[1], t[2, :-1]], [-1, 0, 1], shape=(n, n), format="csr")


class StructuredOperator:
    """A = sum_m X_m (x) Y_m on a g x g grid (dimension "2d") or a single tridiagonal (``"1d"``).

    Behaves like the sparse matrix it stands for where the reference's callers need it: scalar
    ``*`` and ``/``, unary minus, ``.shape``, ``.diagonal()``, ``.tocsr()``/``.toarray()`` (small
    sizes), and ``A.dot(x)`` / ``A * x`` / ``A @ x`` which run the HIP apply kernel.

    ``point_diagonal`` (2-D and 3-D): a (g, g) array added to the diagonal, index [i, j] = row-major point i*g + j — an
    arbitrary potential V(x, y) on top of the Kronecker terms (``potential_operator``, ``recognise_potential``); in 3-D a
    (g, g, g) array, index [z, y, x] = point z*g^2 + y*g + x.

    ``point_bonds`` (2-D only): a pair (E, S) of (g, g) arrays — E[i, j] is added to the two matrix entries between the
    points (i, j) and (i, j + 1), S[i, j] to those between (i, j) and (i + 1, j), on top of the Kronecker terms: a symmetric
    5-point operator with ANY coefficients, e.g. -div(w grad) + V with a position-dependent inverse effective mass w
    (``variable_mass_operator``, ``recognise_five_point``).  E[:, g-1] and S[g-1, :] point outside the grid and must be zero.
    An operator with bonds always has a ``point_diagonal`` (zeros if none was given).

    3-D: a triple (Bx, By, Bz) of (g, g, g) arrays, index [z, y, x] — Bx[z, y, x] is added to the two entries between
    (z, y, x) and (z, y, x + 1), By towards (z, y + 1, x), Bz towards (z + 1, y, x): a symmetric 7-point operator with any
    coefficients (``variable_mass_operator(..., dimension="3d")``, ``recognise_seven_point``).  Bx[:, :, g-1], By[:, g-1, :]
    and Bz[g-1, :, :] point outside the grid and must be zero.

    ``point_stencil`` (2-D only, instead of ``point_diagonal`` / ``point_bonds``, both of which it carries: its centre plane is
    the diagonal): a (3, 3, g, g) array G — G[a, b][i, j] is the coefficient of v(i + a - 1, j + b - 1) in row (i, j), added to
    the Kronecker terms: a symmetric 9-point operator with ANY coefficients, e.g. -div(W grad) + V with a position-dependent
    2 x 2 inverse-mass tensor W (``tensor_mass_operator``, ``recognise_nine_point``).  Coefficients towards points outside the
    grid must be zero and G[a, b][i, j] == G[2 - a, 2 - b][i + a - 1, j + b - 1] (``Plan.point_stencil`` returns this shape
    for the levels below 0).

    3-D: a (3, 3, 3, g, g, g) array G — G[a, b, c][z, y, x] is the coefficient of v(z + a - 1, y + b - 1, x + c - 1) in row
    (z, y, x): a symmetric 27-point operator with any coefficients, e.g. -div(W grad) + V with a symmetric 3 x 3 inverse-mass
    tensor W(x, y, z) (``tensor_mass_operator(..., dimension="3d")``, ``recognise_27_point``).  The same rules: zero towards points
    outside the grid, G[a, b, c][z, y, x] == G[2 - a, 2 - b, 2 - c][z + a - 1, y + b - 1, x + c - 1].
    """

    def __init__(self, dimension, g, terms, point_diagonal=None, point_bonds=None, point_stencil=None):
        self.dimension = dimension
        self.g = int(g)
        self.point_diagonal = None
        self.point_bonds = None
        self.point_stencil = None
        if point_stencil is not None:
            if dimension not in ("2d", "3d"):
                raise ValueError("point_stencil is a property of 2-D and 3-D operators")
            if point_diagonal is not None or point_bonds is not None:
                raise ValueError("point_stencil carries the diagonal (its centre plane) and the bonds: give it instead of point_diagonal / point_bonds")
            G = np.array(point_stencil, dtype=np.float64, order="C")
            if dimension == "3d":
                if G.size != 27 * self.g ** 3:
                    raise ValueError("point_stencil of a 3-D operator must hold 3 x 3 x 3 x g^3 = 27 x %d^3 values, not %r" % (self.g, G.shape))
                G = G.reshape(3, 3, 3, self.g, self.g, self.g)
            else:
                if G.size != 9 * self.g * self.g:
                    raise ValueError("point_stencil must hold 3 x 3 x g x g = 9 x %d x %d values, not %r" % (self.g, self.g, G.shape))
                G = G.reshape(3, 3, self.g, self.g)
            _check_point_stencil(G)
            self.point_stencil = G
        if point_bonds is not None and dimension == "3d":
            if len(point_bonds) != 3:
                raise ValueError("point_bonds of a 3-D operator is a triple (Bx, By, Bz) of g x g x g arrays")
            bonds = []
            for name, b in zip(("Bx", "By", "Bz"), point_bonds):
                b = np.array(b, dtype=np.float64, order="C")
                if b.size != self.g ** 3:
                    raise ValueError("point_bonds %s must hold g^3 = %d^3 values, not %r" % (name, self.g, b.shape))
                bonds.append(b.reshape(self.g, self.g, self.g))
            if bonds[0][:, :, -1].any() or bonds[1][:, -1, :].any() or bonds[2][-1, :, :].any():
                raise ValueError("point_bonds: Bx[:, :, g-1], By[:, g-1, :] and Bz[g-1, :, :] are bonds towards points outside the grid "
                                 "and must be zero")
            self.point_bonds = tuple(bonds)
            if point_diagonal is None:
                point_diagonal = np.zeros((self.g, self.g, self.g))
        elif point_bonds is not None:
            if dimension != "2d":
                raise ValueError("point_bonds is a property of 2-D and 3-D operators")
            if len(point_bonds) != 2:
                raise ValueError("point_bonds is a pair (E, S) of g x g arrays")
            bonds = []
            for name, b in zip(("E", "S"), point_bonds):
                b = np.array(b, dtype=np.float64, order="C")
                if b.size != self.g * self.g:
                    raise ValueError("point_bonds %s must hold g x g = %d x %d values, not %r" % (name, self.g, self.g, b.shape))
                bonds.append(b.reshape(self.g, self.g))
            if bonds[0][:, -1].any() or bonds[1][-1, :].any():
                raise ValueError("point_bonds: E[:, g-1] and S[g-1, :] are bonds towards points outside the grid and must be zero")
            self.point_bonds = tuple(bonds)
            if point_diagonal is None:
                point_diagonal = np.zeros((self.g, self.g))
        if point_diagonal is not None:
            if dimension not in ("2d", "3d"):
                raise ValueError("point_diagonal is a property of 2-D and 3-D operators")
            pd = np.ascontiguousarray(point_diagonal, dtype=np.float64)
            if dimension == "3d":
                if pd.size != self.g ** 3:
                    raise ValueError("point_diagonal must hold g^3 = %d^3 values, not %r" % (self.g, pd.shape))
                self.point_diagonal = pd.reshape(self.g, self.g, self.g)
            else:
                if pd.size != self.g * self.g:
                    raise ValueError("point_diagonal must hold g x g = %d x %d values, not %r" % (self.g, self.g, pd.shape))
                self.point_diagonal = pd.reshape(self.g, self.g)
        if dimension == "3d":
            # (X, Y, Z) per term: A = sum_m X_m (x) Y_m (x) Z_m over z, y, x (idx = z g^2 + y g + x)
            self.terms = [tuple(np.ascontiguousarray(a, dtype=np.float64) for a in t) for t in terms]
            if any(len(t) != 3 for t in self.terms):
                raise ValueError("3-D terms are (X, Y, Z) triples")
            self.shape = (self.g ** 3, self.g ** 3)
            self._fingerprint = None
            return
        self.terms = [(None if x is None else np.ascontiguousarray(x, dtype=np.float64),
                       np.ascontiguousarray(y, dtype=np.float64)) for x, y in terms]
        n = self.g if dimension == "1d" else self.g * self.g
        self.shape = (n, n)
        self._fingerprint = None

    # -- the per-point part as a plan keeps it -----------------------------------------------------
    def point_part(self):
        """(kind, arrays): (None, ()) without a per-point part; ("diag", (D,)); ("bonds", (D, b_0, ..)) with the bonds of axis a
        counted from the fastest index — 2-D: E, S; 3-D: Bx, By, Bz —; ("planes", (G,)) for a point stencil.  The order of
        the arrays is the order of the planes on level 0 of a plan (``Plan.point_stencil(0)``)."""
        if self.point_stencil is not None:
            return "planes", (self.point_stencil,)
        if self.point_bonds is not None:
            return "bonds", (self.point_diagonal,) + self.point_bonds
        if self.point_diagonal is not None:
            return "diag", (self.point_diagonal,)
        return None, ()

    @staticmethod
    def point_keywords(kind, planes):
        """The constructor's keywords for a per-point part of `kind` whose planes come as ``Plan.point_stencil(0)`` returns
        them (the inverse of point_part)."""
        if kind == "planes":
            return {"point_stencil": planes}
        if kind == "bonds":
            return {"point_diagonal": planes[0], "point_bonds": tuple(planes[1:])}
        return {"point_diagonal": planes} if kind == "diag" else {}

    # -- algebra with scalars ---------------------------------------------------------------------
    def _scaled(self, c):
        c = float(c)
        if self.dimension == "1d":
            return StructuredOperator("1d", self.g, [(None, y * c) for _, y in self.terms])
        if self.dimension == "3d":
            return StructuredOperator("3d", self.g, [(x, y, z * c) for x, y, z in self.terms],
                                      point_diagonal=None if self.point_diagonal is None else self.point_diagonal * c,
                                      point_bonds=None if self.point_bonds is None else tuple(b * c for b in self.point_bonds),
                                      point_stencil=None if self.point_stencil is None else self.point_stencil * c)
        return StructuredOperator("2d", self.g, [(x, y * c) for x, y in self.terms],
                                  point_diagonal=None if self.point_diagonal is None else self.point_diagonal * c,
                                  point_bonds=None if self.point_bonds is None else tuple(b * c for b in self.point_bonds),
                                  point_stencil=None if self.point_stencil is None else self.point_stencil * c)

    def __mul__(self, other):
        if np.isscalar(other):
            return self._scaled(other)
        return self.dot(other)

    def __rmul__(self, other):
        if np.isscalar(other):
            return self._scaled(other)
        return NotImplemented

    def __truediv__(self, other):
        return self._scaled(1.0 / other)

    def __neg__(self):
        return self._scaled(-1.0)

    def __matmul__(self, other):
        return self.dot(other)

    def shifted(self, mu):
        """A - mu*I as a structured operator (the shift folded into the first term's diagonal)."""
        if self.dimension == "3d":
            i = tri_identity(self.g)
            terms = [tuple(a.copy() for a in t) for t in self.terms] + [(i, i.copy(), i * (-float(mu)))]
            return StructuredOperator("3d", self.g, terms, point_diagonal=self.point_diagonal, point_bonds=self.point_bonds,
                                      point_stencil=self.point_stencil)
        terms = [(None if x is None else x.copy(), y.copy()) for x, y in self.terms]
        if self.dimension == "1d":
            terms[0][1][1] -= mu
        else:
            terms.append((tri_identity(self.g), tri_identity(self.g) * (-float(mu))))
        return StructuredOperator(self.dimension, self.g, terms, point_diagonal=self.point_diagonal, point_bonds=self.point_bonds,
                                  point_stencil=self.point_stencil)

    # -- views ----------------------------------------------------------------------------------
    def diagonal(self):
        if self.dimension == "1d":
            return sum(y[1] for _, y in self.terms)
        if self.dimension == "3d":
            d = sum(np.kron(x[1], np.kron(y[1], z[1])) for x, y, z in self.terms)
            if self.point_stencil is not None:
                d = d + self.point_stencil[1, 1, 1].reshape(-1)
            return d if self.point_diagonal is None else d + self.point_diagonal.reshape(-1)
        d = sum(np.outer(x[1], y[1]) for x, y in self.terms)
        if self.point_stencil is not None:
            d = d + self.point_stencil[1, 1]
        return (d if self.point_diagonal is None else d + self.point_diagonal).reshape(-1)

    def tocsr(self):
        if self.shape[0] > (1 << 22):
            raise MemoryError("refusing to assemble a %d x %d sparse matrix" % self.shape)
        if self.dimension == "1d":
            return sum(tri_to_sparse(y) for _, y in self.terms).tocsr()
        if self.dimension == "3d":
            A = sum(sp.kron(tri_to_sparse(x), sp.kron(tri_to_sparse(y), tri_to_sparse(z), format="csr"), format="csr")
                    for x, y, z in self.terms).tocsr()
            if self.point_diagonal is not None:
                A = (A + sp.diags(self.point_diagonal.reshape(-1), 0, format="csr")).tocsr()
            if self.point_bonds is not None:
                A = (A + _bonds3_to_sparse(*self.point_bonds)).tocsr()
            if self.point_stencil is not None:
                A = (A + planes_to_csr(self.point_stencil)).tocsr()
            return A
        A = sum(sp.kron(tri_to_sparse(x), tri_to_sparse(y), format="csr") for x, y in self.terms).tocsr()
        if self.point_diagonal is not None:
            A = (A + sp.diags(self.point_diagonal.reshape(-1), 0, format="csr")).tocsr()
        if self.point_bonds is not None:
            A = (A + _bonds_to_sparse(*self.point_bonds)).tocsr()
        if self.point_stencil is not None:
            A = (A + planes_to_csr(self.point_stencil)).tocsr()
        return A

    def tocsc(self):
        return self.tocsr().tocsc()

    def toarray(self):
        return self.tocsr().toarray()

    def dot(self, x):
        from .plan import apply_operator
        return apply_operator(self, x)

    # -- for the plan cache -----------------------------------------------------------------------
    def factor_blocks(self):
        """(nterms, xfac or None, yfac) as contiguous [nterms][3][g] arrays for the C-ABI; 3-D: (nterms, zfac, yfac, xfac),
        the factors over z, y and x (the terms' X, Y, Z)."""
        if self.dimension == "3d":
            return (len(self.terms),) + tuple(np.ascontiguousarray(np.stack([t[a] for t in self.terms])) for a in range(3))
        yfac = np.ascontiguousarray(np.stack([y for _, y in self.terms]))
        xfac = None if self.dimension == "1d" else np.ascontiguousarray(np.stack([x for x, _ in self.terms]))
        return len(self.terms), xfac, yfac

    def fingerprint(self):
        if self._fingerprint is None:
            h = hashlib.sha1()
            h.update(("%s:%d:%d" % (self.dimension, self.g, len(self.terms))).encode())
            for t in self.terms:
                for a in t:
                    if a is not None:
                        h.update(a.tobytes())
            if self.point_diagonal is not None:
                h.update(b"point_diagonal")
                h.update(self.point_diagonal.tobytes())
            if self.point_bonds is not None:
                names = (b"point_bonds_east", b"point_bonds_south") if self.dimension == "2d" else (b"point_bonds_x", b"point_bonds_y", b"point_bonds_z")
                for name, b in zip(names, self.point_bonds):
                    h.update(name)
                    h.update(b.tobytes())
            if self.point_stencil is not None:
                h.update(b"point_stencil")
                h.update(self.point_stencil.tobytes())
            self._fingerprint = h.hexdigest()
        return self._fingerprint


def _check_point_stencil(G):
    """ValueError unless the (3, 3, g, g) — 3-D: (3, 3, 3, g, g, g) — stencil is zero towards points outside the grid and
    symmetric as a matrix."""
    g = G.shape[-1]
    d = G.ndim // 2
    for off in np.ndindex(*([3] * d)):
        # per axis the rows whose neighbour at this offset lies inside the grid, and that neighbour
        here = tuple(slice(max(0, 1 - o), g - max(0, o - 1)) for o in off)
        there = tuple(slice(h.start + o - 1, h.stop + o - 1) for h, o in zip(here, off))
        inside = np.zeros((g,) * d, dtype=bool)
        inside[here] = True
        if G[off][~inside].any():
            raise ValueError("point_stencil: a coefficient towards a point outside the grid is not zero (plane %s)" % (list(off),))
        opposite = tuple(2 - o for o in off)
        if not np.array_equal(G[off][here], G[opposite][there]):
            raise ValueError("point_stencil is not symmetric: the coefficient of a neighbour in the row of a point must equal the "
                             "coefficient of the point in the row of that neighbour, G[a, b][i, j] == G[2 - a, 2 - b][i + a - 1, j + b - 1] "
                             "(plane %s)" % (list(off),))


def _bonds_to_sparse(E, S):
    """The symmetric matrix with E[i, j] between (i, j) and (i, j + 1) and S[i, j] between (i, j) and (i + 1, j) (zero diagonal)."""
    g = E.shape[0]
    n = g * g
    e = E.reshape(-1)[:n - 1]                  # (E[:, g-1] = 0: nothing wraps into the next row)
    s = S.reshape(-1)[:n - g]
    return sp.diags([s, e, e, s], [-g, -1, 1, g], shape=(n, n), format="csr")


def _bonds3_to_sparse(Bx, By, Bz):
    """The symmetric matrix with Bx[z, y, x] between (z, y, x) and (z, y, x + 1), By towards (z, y + 1, x) and Bz towards
    (z + 1, y, x) (zero diagonal)."""
    g = Bx.shape[0]
    n = g ** 3
    bx = Bx.reshape(-1)[:n - 1]                # (the outward bonds are zero: nothing wraps into the next row or plane)
    by = By.reshape(-1)[:n - g]
    bz = Bz.reshape(-1)[:n - g * g]
    return sp.diags([bz, by, bx, bx, by, bz], [-g * g, -g, -1, 1, g, g * g], shape=(n, n), format="csr")


def laplacian_operator(n, dimension="1d"):
    """Matrix-free counterpart of MGCMTStencilMaker.laplacian (MGCMTStencilMaker.py:15-25)."""
    n = int(n)
    if dimension == "1d":
        return StructuredOperator("1d", n, [(None, tri_laplacian(n))])
    if dimension == "3d":
        # kronsum(kronsum(L, L), L) = I (x) I (x) L + I (x) L (x) I + L (x) I (x) I
        i, L = tri_identity(n), tri_laplacian(n)
        return StructuredOperator("3d", n, [(i, i.copy(), L), (i.copy(), L.copy(), i.copy()), (L.copy(), i.copy(), i.copy())])
    # kronsum(L, L) = I (x) L + L (x) I   (MGCMTStencilMaker.py:23-24)
    return StructuredOperator("2d", n, [(tri_identity(n), tri_laplacian(n)), (tri_laplacian(n), tri_identity(n))])


def mehrstellen_operator(n):
    """The compact fourth-order ("Mehrstellen") 9-point Laplacian the reference's report proposes as the next fine-grid
    stencil (SURVEY.md par. 8(f)3; not in the reference's code):  1/(6 h^2) [[1, 4, 1], [4, -20, 4], [1, 4, 1]]
    =  I (x) L + L (x) I + (h^2 / 6) L (x) L  with the 1-D operator L of MGCMTStencilMaker.py:17-21 (h = 1/n, as there).
    Three Toeplitz terms: the fused kernels take it as a constant 9-point operator on every level."""
    n = int(n)
    h = 1. / n
    L = tri_laplacian(n)
    return StructuredOperator("2d", n, [(tri_identity(n), L.copy()), (L.copy(), tri_identity(n)), (L * (h ** 2 / 6.0), L.copy())])


def mehrstellen_mass(n):
    """M = I + (h^2 / 12) (I (x) L + L (x) I): the right-hand-side operator that goes with mehrstellen_operator —
    Delta_9 u = M (Delta u) + O(h^4), so  -Delta u = f  becomes  Delta_9 u = -M f, and  -Delta u = lambda u  the
    generalised problem  -Delta_9 u = lambda M u."""
    n = int(n)
    h = 1. / n
    L = tri_laplacian(n) * (h ** 2 / 12.0)
    y = L.copy()
    y[1] += 1.0
    return StructuredOperator("2d", n, [(tri_identity(n), y), (L.copy(), tri_identity(n))])


def identity_operator(n, dimension="1d"):
    """sparse.eye(N) as a structured operator (the mass matrix M of rqmin, RQMin.py:18)."""
    n = int(n)
    if dimension == "1d":
        return StructuredOperator("1d", n, [(None, tri_identity(n))])
    if dimension == "3d":
        return StructuredOperator("3d", n, [(tri_identity(n), tri_identity(n), tri_identity(n))])
    return StructuredOperator("2d", n, [(tri_identity(n), tri_identity(n))])


def potential_well_operator(g, depth, inner, scale=-1.0 / np.pi ** 2, dimension="2d"):
    """H = scale * laplacian(g, "2d") + diag(V) with the square-well potential of PotWellSolver.py:150-153 carried to
    2-D: V = `depth` outside the square [inner[0], inner[1])^2 of grid indices and 0 inside (BASELINE config 5).

    V = depth * (1 - chi (x) chi) is a sum of Kronecker products of diagonal factors, so H has three terms:
    I (x) (scale L + depth I)  +  (scale L) (x) I  -  (depth chi) (x) chi.

    dimension="3d": the cube well (a quantum dot) V = depth * (1 - chi (x) chi (x) chi) on g^3 points, four terms:
    I (x) I (x) (scale L + depth I)  +  I (x) (scale L) (x) I  +  (scale L) (x) I (x) I  -  (depth chi) (x) chi (x) chi.
    """
    g = int(g)
    if dimension == "3d":
        lo, hi = int(inner[0]), int(inner[1])
        chi = np.zeros(g)
        chi[lo:hi] = 1.0
        L = tri_laplacian(g) * float(scale)
        z1 = L.copy()
        z1[1] += float(depth)
        dchi = np.zeros((3, g))
        dchi[1] = chi
        i = tri_identity(g)
        return StructuredOperator("3d", g, [(i, i.copy(), z1), (i.copy(), L.copy(), i.copy()), (L.copy(), i.copy(), i.copy()),
                                            (dchi * (-float(depth)), dchi.copy(), dchi.copy())])
    if dimension != "2d":
        raise ValueError("potential_well_operator: dimension must be '2d' or '3d'")
    lo, hi = int(inner[0]), int(inner[1])
    chi = np.zeros(g)
    chi[lo:hi] = 1.0
    L = tri_laplacian(g) * float(scale)
    y1 = L.copy()
    y1[1] += float(depth)
    dchi = np.zeros((3, g))
    dchi[1] = chi
    return StructuredOperator("2d", g, [(tri_identity(g), y1), (L.copy(), tri_identity(g)), (dchi * (-float(depth)), dchi.copy())])


def potential_operator(g, V, scale=-1.0 / np.pi ** 2, dimension="2d"):
    """H = scale * laplacian(g, "2d") + diag(V) for ANY potential: V is a (g, g) array (or g*g values, row-major), V[i, j]
    the value at grid point i*g + j.  Matrix-free: the scaled Laplacian as two Kronecker terms, V as the operator's
    ``point_diagonal`` — for grids that cannot be assembled.  Nothing of V has to be separable (a circular dot, a double
    well, a rotated oscillator, disorder); a V that IS a(x) + b(y) or one square well runs faster through
    ``potential_well_operator`` / ``recognise``, whose plans take the fused kernels on every level.

    dimension="3d": H = scale * laplacian(g, "3d") + diag(V) on g^3 points, V a (g, g, g) array (or g^3 values), V[z, y, x]
    the value at point z*g^2 + y*g + x: three Kronecker terms plus the point diagonal (a spherical dot, a lens, coupled
    dots, disorder)."""
    g = int(g)
    if dimension == "3d":
        i, L = tri_identity(g), tri_laplacian(g) * float(scale)
        return StructuredOperator("3d", g, [(i, i.copy(), L), (i.copy(), L.copy(), i.copy()), (L.copy(), i.copy(), i.copy())], point_diagonal=V)
    if dimension != "2d":
        raise ValueError("potential_operator: dimension must be '2d' or '3d' (any tridiagonal is a 1-D operator already)")
    L = tri_laplacian(g) * float(scale)
    return StructuredOperator("2d", g, [(tri_identity(g), L), (L.copy(), tri_identity(g))], point_diagonal=V)


def _mean_bond(a, b, mean):
    if mean == "harmonic":
        return 2.0 * a * b / (a + b)
    if mean == "arithmetic":
        return 0.5 * (a + b)
    raise ValueError("variable_mass_operator: mean must be 'harmonic' or 'arithmetic', not %r" % (mean,))


def variable_mass_operator(g, inv_mass, V=None, scale=-1.0 / np.pi ** 2, mean="harmonic", dimension="2d"):
    """H = scale * div(w grad) + diag(V) on the g x g grid of ``laplacian(g, "2d")`` with a position-dependent inverse
    effective mass w = inv_mass (a (g, g) array, positive): the BenDaniel-Duke form of the kinetic term across the
    interfaces of a heterostructure.  Matrix-free.  With t = scale * L[0, 1] the neighbour entry of the uniform operator, the
    entry between neighbours a, b is t * m(w_a, w_b) — m the harmonic mean 2ab/(a+b) (flux-conserving; the default) or the
    arithmetic mean — and the diagonal is -t * (the sum of the point's four bond values) + V; a bond towards a ghost point
    outside the grid takes the point's own w, so w = 1, V = 0 is scale * laplacian(g, "2d") exactly.

    The Kronecker terms carry w_ref * scale * Laplacian with w_ref = median(w); ``point_bonds`` and ``point_diagonal`` carry
    the deviations, so a uniform region stores zeros and level 0 keeps a constant 5-point Kronecker part.  A uniform w
    returns what ``potential_operator`` / ``laplacian_operator`` (scaled) would return: no bonds.

    dimension="3d": the same on the g^3 grid of ``laplacian(g, "3d")`` — inv_mass and V are (g, g, g) arrays (or g^3 values),
    index [z, y, x]; six bonds per point, three Kronecker terms, ``point_bonds`` = (Bx, By, Bz)."""
    g = int(g)
    if dimension == "3d":
        return _variable_mass_operator_3d(g, inv_mass, V, scale, mean)
    if dimension != "2d":
        raise ValueError("variable_mass_operator: dimension must be '2d' or '3d'")
    w = np.ascontiguousarray(inv_mass, dtype=np.float64)
    if w.size != g * g:
        raise ValueError("variable_mass_operator: inv_mass must hold g x g = %d x %d values, not %r" % (g, g, w.shape))
    w = w.reshape(g, g)
    if not (w > 0).all():
        raise ValueError("variable_mass_operator: the inverse mass must be positive everywhere")
    _mean_bond(1.0, 1.0, mean)
    if V is not None:
        V = np.ascontiguousarray(V, dtype=np.float64)
        if V.size != g * g:
            raise ValueError("variable_mass_operator: V must hold g x g = %d x %d values, not %r" % (g, g, V.shape))
        V = V.reshape(g, g)
    w_ref = float(np.median(w))
    L = tri_laplacian(g) * float(scale)
    if (w == w_ref).all():
        Lr = L * w_ref
        if V is None:
            return StructuredOperator("2d", g, [(tri_identity(g), Lr), (Lr.copy(), tri_identity(g))])
        return StructuredOperator("2d", g, [(tri_identity(g), Lr), (Lr.copy(), tri_identity(g))], point_diagonal=V)
    t = float(L[2, 0])
    # bond values (multiples of t) towards east / west / south / north; ghosts take the point's own w
    be, bs = w.copy(), w.copy()
    be[:, :-1] = _mean_bond(w[:, :-1], w[:, 1:], mean)
    bs[:-1, :] = _mean_bond(w[:-1, :], w[1:, :], mean)
    bw, bn = w.copy(), w.copy()
    bw[:, 1:] = be[:, :-1]
    bn[1:, :] = bs[:-1, :]
    E, S = np.zeros((g, g)), np.zeros((g, g))
    E[:, :-1] = t * be[:, :-1] - t * w_ref
    S[:-1, :] = t * bs[:-1, :] - t * w_ref
    Lr = L * w_ref
    D = -t * (be + bw + bs + bn) - 2.0 * float(Lr[1, 0])
    if V is not None:
        D = D + V
    return StructuredOperator("2d", g, [(tri_identity(g), Lr), (Lr.copy(), tri_identity(g))], point_diagonal=D, point_bonds=(E, S))


def _variable_mass_operator_3d(g, inv_mass, V, scale, mean):
    w = np.ascontiguousarray(inv_mass, dtype=np.float64)
    if w.size != g ** 3:
        raise ValueError("variable_mass_operator: inv_mass must hold g^3 = %d^3 values, not %r" % (g, w.shape))
    w = w.reshape(g, g, g)
    if not (w > 0).all():
        raise ValueError("variable_mass_operator: the inverse mass must be positive everywhere")
    _mean_bond(1.0, 1.0, mean)
    if V is not None:
        V = np.ascontiguousarray(V, dtype=np.float64)
        if V.size != g ** 3:
            raise ValueError("variable_mass_operator: V must hold g^3 = %d^3 values, not %r" % (g, V.shape))
        V = V.reshape(g, g, g)
    w_ref = float(np.median(w))
    L = tri_laplacian(g) * float(scale)
    i = tri_identity(g)
    Lr = L * w_ref
    terms = [(i, i.copy(), Lr), (i.copy(), Lr.copy(), i.copy()), (Lr.copy(), i.copy(), i.copy())]
    if (w == w_ref).all():
        return StructuredOperator("3d", g, terms) if V is None else StructuredOperator("3d", g, terms, point_diagonal=V)
    t = float(L[2, 0])
    # bond values (multiples of t) towards x+ / y+ / z+ and x- / y- / z-; ghosts take the point's own w
    bxp, byp, bzp = w.copy(), w.copy(), w.copy()
    bxp[:, :, :-1] = _mean_bond(w[:, :, :-1], w[:, :, 1:], mean)
    byp[:, :-1, :] = _mean_bond(w[:, :-1, :], w[:, 1:, :], mean)
    bzp[:-1, :, :] = _mean_bond(w[:-1, :, :], w[1:, :, :], mean)
    bxm, bym, bzm = w.copy(), w.copy(), w.copy()
    bxm[:, :, 1:] = bxp[:, :, :-1]
    bym[:, 1:, :] = byp[:, :-1, :]
    bzm[1:, :, :] = bzp[:-1, :, :]
    Bx, By, Bz = np.zeros((g, g, g)), np.zeros((g, g, g)), np.zeros((g, g, g))
    Bx[:, :, :-1] = t * bxp[:, :, :-1] - t * w_ref
    By[:, :-1, :] = t * byp[:, :-1, :] - t * w_ref
    Bz[:-1, :, :] = t * bzp[:-1, :, :] - t * w_ref
    D = -t * (bxp + bxm + byp + bym + bzp + bzm) - 3.0 * float(Lr[1, 0])
    if V is not None:
        D = D + V
    return StructuredOperator("3d", g, terms, point_diagonal=D, point_bonds=(Bx, By, Bz))


def tensor_mass_operator(g, wxx, wyy, wxy, V=None, scale=-1.0 / np.pi ** 2, mean="harmonic", *, wzz=None, wxz=None, wyz=None, dimension="2d"):
    """H = scale * div(W grad) + diag(V) on the g x g grid of ``laplacian(g, "2d")`` with a position-dependent symmetric 2 x 2
    inverse-mass tensor W = [[wxx, wxy], [wxy, wyy]] ((g, g) arrays indexed [i, j]; positive definite everywhere): anisotropic
    valleys rotated against the grid, strain, a principal axis that turns across an interface.  wxx acts along j (the east / west
    bonds), wyy along i (north / south), wxy is the mixed coefficient in index directions (i, j).  Matrix-free.

    With t = scale * L[0, 1] the neighbour entry of the uniform operator: the east entry between (i, j) and (i, j + 1) is
    t * m(wxx[i, j], wxx[i, j + 1]), the south entry between (i, j) and (i + 1, j) is t * m(wyy[i, j], wyy[i + 1, j]) — m the
    harmonic (default) or arithmetic mean —, the diagonal is -t * (the point's four bond values) + V, a bond towards a ghost
    point taking the point's own wxx / wyy, and the corner entry between (i, j) and (i + a, j + b), a, b = -1 or +1, is
    a * b * t * (wxy[i + a, j] + wxy[i, j + b]) / 4: the mixed derivative as the product of two central differences, made
    symmetric.  W = I, V = 0 is scale * laplacian(g, "2d") exactly.

    The Kronecker terms carry median(wxx) and median(wyy) times the scaled 1-D Laplacians; ``point_stencil`` carries the
    deviations, so a uniform region stores zeros and level 0 keeps a constant 5-point Kronecker part.  wxy = 0 everywhere is a
    diagonal tensor: the operator comes back with ``point_bonds`` (and wxx = wyy as well gives exactly
    ``variable_mass_operator``'s).

    dimension="3d": the same on the g^3 grid of ``laplacian(g, "3d")`` with the symmetric 3 x 3 tensor
    W = [[wxx, wxy, wxz], [wxy, wyy, wyz], [wxz, wyz, wzz]] — all six components and V are (g, g, g) arrays (or g^3 values) indexed
    [z, y, x]; wxx acts along x (the fastest index), wyy along y, wzz along z.  The bond between a point and its neighbour along
    axis u is t * m(w_uu(p), w_uu(p + e_u)), the diagonal -t * (the six bond values, a ghost's bond taking the point's own w_uu)
    + V, and for each pair of axes (u, v) of xy, xz, yz and a, b = -1 or +1 the entry between p and p + a e_u + b e_v is
    a * b * t * (w_uv(p + a e_u) + w_uv(p + b e_v)) / 4 — the 2-D formula in every coordinate plane: a 19-point matrix, the eight
    corner planes of ``point_stencil`` are zero.  Three Toeplitz Kronecker terms carry median(wzz), median(wyy), median(wxx) times
    the scaled 1-D Laplacians.  All three mixed components zero returns the ``point_bonds`` operator, wxx = wyy = wzz as well exactly
    ``variable_mass_operator(..., dimension="3d")``'s."""
    g = int(g)
    if dimension == "3d":
        return _tensor_mass_operator_3d(g, wxx, wyy, wzz, wxy, wxz, wyz, V, scale, mean)
    if dimension != "2d":
        raise ValueError("tensor_mass_operator: dimension must be '2d' or '3d'")
    if wzz is not None or wxz is not None or wyz is not None:
        raise ValueError("tensor_mass_operator: wzz, wxz and wyz are components of a 3-D tensor (dimension='3d')")
    arrs = []
    for name, a in (("wxx", wxx), ("wyy", wyy), ("wxy", wxy)):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.size != g * g:
            raise ValueError("tensor_mass_operator: %s must hold g x g = %d x %d values, not %r" % (name, g, g, a.shape))
        arrs.append(a.reshape(g, g))
    wxx, wyy, wxy = arrs
    if not ((wxx > 0).all() and (wyy > 0).all() and (wxx * wyy > wxy * wxy).all()):
        raise ValueError("tensor_mass_operator: the inverse-mass tensor must be positive definite everywhere (wxx, wyy > 0 and wxx wyy > wxy^2)")
    if mean not in ("harmonic", "arithmetic"):
        raise ValueError("tensor_mass_operator: mean must be 'harmonic' or 'arithmetic', not %r" % (mean,))
    if V is not None:
        V = np.ascontiguousarray(V, dtype=np.float64)
        if V.size != g * g:
            raise ValueError("tensor_mass_operator: V must hold g x g = %d x %d values, not %r" % (g, g, V.shape))
        V = V.reshape(g, g)
    if not wxy.any() and np.array_equal(wxx, wyy):
        return variable_mass_operator(g, wxx, V=V, scale=scale, mean=mean)
    L = tri_laplacian(g) * float(scale)
    t = float(L[2, 0])
    rx, ry = float(np.median(wxx)), float(np.median(wyy))
    Lx, Ly = L * rx, L * ry                       # along j (column factor) / along i (row factor)
    # bond values (multiples of t) towards east / west / south / north; ghosts take the point's own value
    be, bs = wxx.copy(), wyy.copy()
    be[:, :-1] = _mean_bond(wxx[:, :-1], wxx[:, 1:], mean)
    bs[:-1, :] = _mean_bond(wyy[:-1, :], wyy[1:, :], mean)
    bw, bn = wxx.copy(), wyy.copy()
    bw[:, 1:] = be[:, :-1]
    bn[1:, :] = bs[:-1, :]
    E, S = np.zeros((g, g)), np.zeros((g, g))
    E[:, :-1] = t * be[:, :-1] - t * rx
    S[:-1, :] = t * bs[:-1, :] - t * ry
    D = -t * (be + bw + bs + bn) - float(Lx[1, 0]) - float(Ly[1, 0])
    if V is not None:
        D = D + V
    terms = [(tri_identity(g), Lx), (Ly, tri_identity(g))]
    if not wxy.any():
        return StructuredOperator("2d", g, terms, point_diagonal=D, point_bonds=(E, S))
    G = np.zeros((3, 3, g, g))
    G[1, 1] = D
    G[1, 2] = E
    G[1, 0][:, 1:] = E[:, :-1]
    G[2, 1] = S
    G[0, 1][1:, :] = S[:-1, :]
    # corners: a * b * t * (wxy[i + a, j] + wxy[i, j + b]) / 4 between (i, j) and (i + a, j + b)
    q = 0.25 * t
    G[2, 2][:-1, :-1] = q * (wxy[1:, :-1] + wxy[:-1, 1:])
    G[0, 0][1:, 1:] = q * (wxy[:-1, 1:] + wxy[1:, :-1])
    G[2, 0][:-1, 1:] = -q * (wxy[1:, 1:] + wxy[:-1, :-1])
    G[0, 2][1:, :-1] = -q * (wxy[:-1, :-1] + wxy[1:, 1:])
    return StructuredOperator("2d", g, terms, point_stencil=G)


def _tensor_mass_operator_3d(g, wxx, wyy, wzz, wxy, wxz, wyz, V, scale, mean):
    arrs = []
    for name, a in (("wxx", wxx), ("wyy", wyy), ("wzz", wzz), ("wxy", wxy), ("wxz", wxz), ("wyz", wyz)):
        if a is None:
            raise ValueError("tensor_mass_operator: a 3-D tensor needs all six components, %s is missing" % name)
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.size != g ** 3:
            raise ValueError("tensor_mass_operator: %s must hold g^3 = %d^3 values, not %r" % (name, g, a.shape))
        arrs.append(a.reshape(g, g, g))
    wxx, wyy, wzz, wxy, wxz, wyz = arrs
    minor2 = wxx * wyy - wxy * wxy
    det = wzz * minor2 - wxz * (wxz * wyy - wxy * wyz) + wyz * (wxz * wxy - wxx * wyz)
    if not ((wxx > 0).all() and (minor2 > 0).all() and (det > 0).all()):
        raise ValueError("tensor_mass_operator: the inverse-mass tensor must be positive definite everywhere (its leading minors "
                         "wxx, wxx wyy - wxy^2 and det W must be positive)")
    if mean not in ("harmonic", "arithmetic"):
        raise ValueError("tensor_mass_operator: mean must be 'harmonic' or 'arithmetic', not %r" % (mean,))
    if V is not None:
        V = np.ascontiguousarray(V, dtype=np.float64)
        if V.size != g ** 3:
            raise ValueError("tensor_mass_operator: V must hold g^3 = %d^3 values, not %r" % (g, V.shape))
        V = V.reshape(g, g, g)
    mixed = wxy.any() or wxz.any() or wyz.any()
    if not mixed and np.array_equal(wxx, wyy) and np.array_equal(wxx, wzz):
        return variable_mass_operator(g, wxx, V=V, scale=scale, mean=mean, dimension="3d")
    L = tri_laplacian(g) * float(scale)
    t = float(L[2, 0])
    rx, ry, rz = float(np.median(wxx)), float(np.median(wyy)), float(np.median(wzz))
    Lx, Ly, Lz = L * rx, L * ry, L * rz
    i = tri_identity(g)
    terms = [(i, i.copy(), Lx), (i.copy(), Ly, i.copy()), (Lz, i.copy(), i.copy())]
    # bond values (multiples of t) towards x+ / y+ / z+ and x- / y- / z-; ghosts take the point's own value
    bxp, byp, bzp = wxx.copy(), wyy.copy(), wzz.copy()
    bxp[:, :, :-1] = _mean_bond(wxx[:, :, :-1], wxx[:, :, 1:], mean)
    byp[:, :-1, :] = _mean_bond(wyy[:, :-1, :], wyy[:, 1:, :], mean)
    bzp[:-1, :, :] = _mean_bond(wzz[:-1, :, :], wzz[1:, :, :], mean)
    bxm, bym, bzm = wxx.copy(), wyy.copy(), wzz.copy()
    bxm[:, :, 1:] = bxp[:, :, :-1]
    bym[:, 1:, :] = byp[:, :-1, :]
    bzm[1:, :, :] = bzp[:-1, :, :]
    Bx, By, Bz = np.zeros((g, g, g)), np.zeros((g, g, g)), np.zeros((g, g, g))
    Bx[:, :, :-1] = t * bxp[:, :, :-1] - t * rx
    By[:, :-1, :] = t * byp[:, :-1, :] - t * ry
    Bz[:-1, :, :] = t * bzp[:-1, :, :] - t * rz
    D = -t * (bxp + bxm + byp + bym + bzp + bzm) - float(Lx[1, 0]) - float(Ly[1, 0]) - float(Lz[1, 0])
    if V is not None:
        D = D + V
    if not mixed:
        return StructuredOperator("3d", g, terms, point_diagonal=D, point_bonds=(Bx, By, Bz))
    G = np.zeros((3, 3, 3, g, g, g))
    G[1, 1, 1] = D
    G[1, 1, 2] = Bx
    G[1, 1, 0][:, :, 1:] = Bx[:, :, :-1]
    G[1, 2, 1] = By
    G[1, 0, 1][:, 1:, :] = By[:, :-1, :]
    G[2, 1, 1] = Bz
    G[0, 1, 1][1:, :, :] = Bz[:-1, :, :]
    # edges: a * b * t * (w_uv(p + a e_u) + w_uv(p + b e_v)) / 4 between p and p + a e_u + b e_v; array axes: 0 = z, 1 = y, 2 = x
    q = 0.25 * t
    here = {1: slice(0, g - 1), -1: slice(1, g)}          # the rows whose neighbour one step along an axis lies inside
    there = {1: slice(1, g), -1: slice(0, g - 1)}         # ... and that neighbour
    for w, au, av in ((wxy, 2, 1), (wxz, 2, 0), (wyz, 1, 0)):
        for a in (-1, 1):
            for b in (-1, 1):
                off, rows, pu, pv = [1, 1, 1], [slice(None)] * 3, [slice(None)] * 3, [slice(None)] * 3
                off[au], off[av] = 1 + a, 1 + b
                rows[au], rows[av] = here[a], here[b]
                pu[au], pu[av] = there[a], here[b]          # p + a e_u
                pv[au], pv[av] = here[a], there[b]          # p + b e_v
                G[tuple(off)][tuple(rows)] = (a * b * q) * (w[tuple(pu)] + w[tuple(pv)])
    return StructuredOperator("3d", g, terms, point_stencil=G)


class UnrecognisedOperator(ValueError):
    pass


_CACHE = {}


def _digest(A):
    """Content digest of a scipy.sparse matrix (O(nnz), the cost of the structural check itself): a matrix mutated in
    place (``A *= c``, ``A.data[:] = ...``, ``setdiag``) keeps its id, shape and nnz but not this."""
    import hashlib
    h = hashlib.blake2b(digest_size=16)
    fmt = getattr(A, "format", None)
    h.update(str(fmt).encode())
    if fmt in ("csr", "csc", "bsr"):
        parts = (A.data, A.indices, A.indptr)
    elif fmt == "coo":
        parts = (A.data, A.row, A.col)
    elif fmt == "dia":
        parts = (A.data, A.offsets)
    else:                                                    # lil / dok / anything else: go through CSR
        B = A.tocsr()
        parts = (B.data, B.indices, B.indptr)
    for a in parts:
        h.update(np.ascontiguousarray(a).view(np.uint8).data)
    return h.digest()


def _cache_key(A):
    return (id(A), A.shape, getattr(A, "nnz", None), _digest(A))


def recognise(A, dimension=None):
    """StructuredOperator for a scipy.sparse matrix of the shapes the reference's callers build (``_recognise_12``: 1-D
    and 2-D) or a 3-D operator  X (x) I (x) I + I (x) Y (x) I + I (x) I (x) Z  with tridiagonal factors
    (``_recognise_3d``).  With ``dimension=None`` 3-D is tried only after the 1-D and 2-D attempts have failed."""
    if dimension == "3d" and not isinstance(A, StructuredOperator):
        return _recognise_3d(A)
    try:
        return _recognise_12(A, dimension)
    except UnrecognisedOperator as e12:
        if dimension is not None or isinstance(A, StructuredOperator):
            raise
        try:
            return _recognise_3d(A)
        except UnrecognisedOperator:
            raise e12


def recognise_potential(A, dimension="2d"):
    """StructuredOperator for a sparse 2-D 5-point matrix whose off-diagonals have the Kronecker form  I (x) Y + X (x) I
    and whose diagonal is ARBITRARY: a scaled Laplacian plus diag(V) for any potential V.  What ``recognise`` maps — a
    diagonal a(i) + b(j) plus at most one outer product, constant 9-point stencils — is returned as ``recognise`` returns
    it; otherwise the off-diagonals and a constant diagonal (the median entry, so that a potential that vanishes on most
    of the grid leaves mostly zeros) become two Kronecker terms and the rest of the diagonal the operator's
    ``point_diagonal``.  Anything that is not such a 5-point matrix raises UnrecognisedOperator.  ``recognise`` itself
    never returns an operator with a point diagonal.

    dimension="3d": the same for a 7-point matrix on a g^3 grid whose six off-diagonal bands have the form
    X (x) I (x) I + I (x) Y (x) I + I (x) I (x) Z (``_recognise_3d``'s checks)."""
    if dimension == "3d":
        return _recognise_potential_3d(A)
    if dimension != "2d":
        raise UnrecognisedOperator("recognise_potential: dimension must be '2d' or '3d'")
    try:
        return recognise(A, "2d")
    except UnrecognisedOperator:
        if isinstance(A, StructuredOperator):
            raise
    if not sp.issparse(A):
        A = sp.csr_matrix(np.asarray(A, dtype=np.float64))
    key = ("potential",) + _cache_key(A)
    hit = _CACHE.get(key)
    if hit is not None and hit[0] is A:
        return hit[1]
    n = A.shape[0]
    g = int(round(math.sqrt(n)))
    if A.shape[0] != A.shape[1] or g * g != n or np.iscomplexobj(A):
        raise UnrecognisedOperator("recognise_potential: a real square matrix on a g x g grid is needed")
    M = sp.csr_matrix(A, dtype=np.float64, copy=True)
    M.eliminate_zeros()
    d0 = M.diagonal(0).reshape(g, g)
    e, w, s, nn = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    e[:-1], w[1:] = M.diagonal(1), M.diagonal(-1)
    if g < n:
        s[:-g], nn[g:] = M.diagonal(g), M.diagonal(-g)
    counted = sum(np.count_nonzero(a) for a in (d0, e, w, s, nn))
    e, w, s, nn = e.reshape(g, g), w.reshape(g, g), s.reshape(g, g), nn.reshape(g, g)
    ok = counted == M.nnz and not e[:, -1].any() and not w[:, 0].any()
    ok = ok and np.array_equal(e, np.broadcast_to(e[0], (g, g))) and np.array_equal(w, np.broadcast_to(w[0], (g, g)))
    ok = ok and np.array_equal(s, np.broadcast_to(s[:, :1], (g, g))) and np.array_equal(nn, np.broadcast_to(nn[:, :1], (g, g)))
    if not ok:
        raise UnrecognisedOperator(
            "2-D operator is not a 5-point matrix  I (x) Y + X (x) I + diag(V): its off-diagonals do not have the Kronecker "
            "form (an arbitrary potential may sit on the diagonal only)")
    base = float(np.median(d0))
    Y, X = np.zeros((3, g)), np.zeros((3, g))
    Y[0], Y[1], Y[2] = w[0], 0.5 * base, e[0]
    X[0], X[1], X[2] = nn[:, 0], base - 0.5 * base, s[:, 0]
    op = StructuredOperator("2d", g, [(tri_identity(g), Y), (X, tri_identity(g))], point_diagonal=d0 - base)
    if len(_CACHE) > 64:
        _CACHE.clear()
    _CACHE[key] = (A, op)
    return op


def recognise_five_point(A):
    """StructuredOperator for ANY symmetric 5-point matrix on a g x g grid (a Hamiltonian with a position-dependent effective
    mass assembled as a sparse matrix).  What ``recognise`` or ``recognise_potential`` accepts is returned as they return
    it; otherwise the median east / south off-diagonal and the median diagonal go into two Toeplitz Kronecker terms — so
    that a uniform region leaves zeros — and the rest into the operator's ``point_bonds`` and ``point_diagonal``.
    Unsymmetric matrices and anything wider than the 5-point stencil raise UnrecognisedOperator."""
    try:
        return recognise_potential(A, "2d")
    except UnrecognisedOperator:
        if isinstance(A, StructuredOperator):
            raise
    if not sp.issparse(A):
        A = sp.csr_matrix(np.asarray(A, dtype=np.float64))
    key = ("five_point",) + _cache_key(A)
    hit = _CACHE.get(key)
    if hit is not None and hit[0] is A:
        return hit[1]
    n = A.shape[0]
    g = int(round(math.sqrt(n)))
    if A.shape[0] != A.shape[1] or g * g != n or g < 2 or np.iscomplexobj(A):
        raise UnrecognisedOperator("recognise_five_point: a real square matrix on a g x g grid is needed")
    M = sp.csr_matrix(A, dtype=np.float64, copy=True)
    M.eliminate_zeros()
    d0 = M.diagonal(0).reshape(g, g)
    e, w, s, nn = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    e[:-1], w[1:] = M.diagonal(1), M.diagonal(-1)
    s[:-g], nn[g:] = M.diagonal(g), M.diagonal(-g)
    counted = sum(np.count_nonzero(a) for a in (d0, e, w, s, nn))
    e, w, s, nn = e.reshape(g, g), w.reshape(g, g), s.reshape(g, g), nn.reshape(g, g)
    if counted != M.nnz or e[:, -1].any() or w[:, 0].any():
        raise UnrecognisedOperator("2-D operator is not a 5-point matrix: it has entries off the stencil (or across the row ends)")
    if not (np.array_equal(e[:, :-1], w[:, 1:]) and np.array_equal(s[:-1, :], nn[1:, :])):
        raise UnrecognisedOperator("2-D 5-point operator is not symmetric: per-point bonds describe symmetric matrices only")
    base = float(np.median(d0))
    ce, cs = float(np.median(e[:, :-1])), float(np.median(s[:-1, :]))
    Y, X = np.zeros((3, g)), np.zeros((3, g))
    Y[0, 1:], Y[1], Y[2, :-1] = ce, 0.5 * base, ce
    X[0, 1:], X[1], X[2, :-1] = cs, base - 0.5 * base, cs
    E, S = np.zeros((g, g)), np.zeros((g, g))
    E[:, :-1] = e[:, :-1] - ce
    S[:-1, :] = s[:-1, :] - cs
    op = StructuredOperator("2d", g, [(tri_identity(g), Y), (X, tri_identity(g))], point_diagonal=d0 - base, point_bonds=(E, S))
    if len(_CACHE) > 64:
        _CACHE.clear()
    _CACHE[key] = (A, op)
    return op


def recognise_nine_point(A):
    """StructuredOperator for ANY real symmetric 9-point matrix on a g x g grid (a Hamiltonian with a position-dependent
    inverse-mass tensor assembled as a sparse matrix).  What ``recognise``, ``recognise_potential`` or ``recognise_five_point``
    accepts is returned as they return it; otherwise the median east / south off-diagonal and the median diagonal go into two
    Toeplitz Kronecker terms, as ``recognise_five_point`` takes them — so that a uniform region leaves zeros — and the rest into
    the operator's ``point_stencil``.  Unsymmetric matrices, entries outside the 3 x 3 neighbourhood and entries across a row end
    raise UnrecognisedOperator."""
    try:
        return recognise_five_point(A)
    except UnrecognisedOperator:
        if isinstance(A, StructuredOperator):
            raise
    if not sp.issparse(A):
        A = sp.csr_matrix(np.asarray(A, dtype=np.float64))
    key = ("nine_point",) + _cache_key(A)
    hit = _CACHE.get(key)
    if hit is not None and hit[0] is A:
        return hit[1]
    n = A.shape[0]
    g = int(round(math.sqrt(n)))
    if A.shape[0] != A.shape[1] or g * g != n or g < 3 or np.iscomplexobj(A):
        raise UnrecognisedOperator("recognise_nine_point: a real square matrix on a g x g grid is needed")
    M = sp.csr_matrix(A, dtype=np.float64, copy=True)
    M.eliminate_zeros()
    G = np.zeros((3, 3, g, g))
    counted = 0
    for a in range(3):
        for b in range(3):
            off = (a - 1) * g + (b - 1)
            band = np.zeros(n)
            d = M.diagonal(off)
            if off >= 0:
                band[:n - off] = d
            else:
                band[-off:] = d
            counted += np.count_nonzero(band)
            G[a, b] = band.reshape(g, g)                  # [i, j] of the row
    if counted != M.nnz:
        raise UnrecognisedOperator("2-D operator is not a 9-point matrix: it has entries outside the 3 x 3 neighbourhood")
    if G[:, 0, :, 0].any() or G[:, 2, :, -1].any():
        raise UnrecognisedOperator("2-D operator is not a 9-point matrix: it has entries across the row ends")
    try:
        _check_point_stencil(G)
    except ValueError:
        raise UnrecognisedOperator("2-D 9-point operator is not symmetric: a per-point stencil describes symmetric matrices only")
    base = float(np.median(G[1, 1]))
    ce, cs = float(np.median(G[1, 2][:, :-1])), float(np.median(G[2, 1][:-1, :]))
    Y, X = np.zeros((3, g)), np.zeros((3, g))
    Y[0, 1:], Y[1], Y[2, :-1] = ce, 0.5 * base, ce
    X[0, 1:], X[1], X[2, :-1] = cs, base - 0.5 * base, cs
    G[1, 1] -= base
    G[1, 2][:, :-1] -= ce
    G[1, 0][:, 1:] -= ce
    G[2, 1][:-1, :] -= cs
    G[0, 1][1:, :] -= cs
    op = StructuredOperator("2d", g, [(tri_identity(g), Y), (X, tri_identity(g))], point_stencil=G)
    if len(_CACHE) > 64:
        _CACHE.clear()
    _CACHE[key] = (A, op)
    return op


def recognise_seven_point(A):
    """StructuredOperator for ANY symmetric 7-point matrix on a g^3 grid (a 3-D Hamiltonian with a position-dependent effective
    mass assembled as a sparse matrix).  What ``recognise(A, "3d")`` or ``recognise_potential(A, "3d")`` accepts is returned
    as they return it; otherwise the median off-diagonal per direction and the median diagonal go into three Toeplitz
    Kronecker terms — so that a uniform region leaves zeros — and the rest into the operator's ``point_bonds`` and
    ``point_diagonal``.  Unsymmetric matrices, entries off the seven bands and entries across row or plane ends raise
    UnrecognisedOperator."""
    try:
        return recognise_potential(A, "3d")
    except UnrecognisedOperator:
        if isinstance(A, StructuredOperator):
            raise
    if not sp.issparse(A):
        A = sp.csr_matrix(np.asarray(A, dtype=np.float64))
    key = ("seven_point",) + _cache_key(A)
    hit = _CACHE.get(key)
    if hit is not None and hit[0] is A:
        return hit[1]
    n = A.shape[0]
    if A.shape[0] != A.shape[1] or np.iscomplexobj(A):
        raise UnrecognisedOperator("recognise_seven_point: a real square matrix on a g^3 grid is needed")
    g = int(round(n ** (1.0 / 3.0)))
    while g ** 3 > n:
        g -= 1
    while (g + 1) ** 3 <= n:
        g += 1
    if g ** 3 != n or g < 2:
        raise UnrecognisedOperator("3-D operator size %d is not a cube number" % n)
    M = sp.csr_matrix(A, dtype=np.float64, copy=True)
    M.eliminate_zeros()

    def band(off):
        out = np.zeros(n)
        d = M.diagonal(off)
        if off >= 0:
            out[:n - off] = d
        else:
            out[-off:] = d
        return out.reshape(g, g, g)                       # [z, y, x] of the row

    d0 = M.diagonal(0).reshape(g, g, g)
    xp, xm, yp, ym, zp, zm = (band(off) for off in (1, -1, g, -g, g * g, -g * g))
    if sum(np.count_nonzero(b) for b in (xp, xm, yp, ym, zp, zm)) + np.count_nonzero(d0) != M.nnz:
        raise UnrecognisedOperator("3-D operator is not a 7-point matrix: it has entries off the stencil")
    if xp[:, :, -1].any() or xm[:, :, 0].any() or yp[:, -1, :].any() or ym[:, 0, :].any():
        raise UnrecognisedOperator("3-D operator is not a 7-point matrix: it has entries across the row or plane ends")
    if not (np.array_equal(xp[:, :, :-1], xm[:, :, 1:]) and np.array_equal(yp[:, :-1, :], ym[:, 1:, :])
            and np.array_equal(zp[:-1, :, :], zm[1:, :, :])):
        raise UnrecognisedOperator("3-D 7-point operator is not symmetric: per-point bonds describe symmetric matrices only")
    base = float(np.median(d0))
    cx, cy, cz = float(np.median(xp[:, :, :-1])), float(np.median(yp[:, :-1, :])), float(np.median(zp[:-1, :, :]))
    Xt, Yt, Zt = _toeplitz_tri(cx, base - 2.0 * (base / 3.0), cx, g), _toeplitz_tri(cy, base / 3.0, cy, g), _toeplitz_tri(cz, base / 3.0, cz, g)
    Bx, By, Bz = np.zeros((g, g, g)), np.zeros((g, g, g)), np.zeros((g, g, g))
    Bx[:, :, :-1] = xp[:, :, :-1] - cx
    By[:, :-1, :] = yp[:, :-1, :] - cy
    Bz[:-1, :, :] = zp[:-1, :, :] - cz
    i = tri_identity(g)
    op = StructuredOperator("3d", g, [(i, i.copy(), Xt), (i.copy(), Yt, i.copy()), (Zt, i.copy(), i.copy())], point_diagonal=d0 - base,
                            point_bonds=(Bx, By, Bz))
    if len(_CACHE) > 64:
        _CACHE.clear()
    _CACHE[key] = (A, op)
    return op


def recognise_27_point(A):
    """StructuredOperator for ANY real symmetric sparse matrix on a g^3 grid whose entries lie within the 3 x 3 x 3 neighbourhood
    (a 3-D Hamiltonian with a position-dependent inverse-mass tensor assembled as a sparse matrix).  What ``recognise(A, "3d")``,
    ``recognise_potential(A, "3d")`` or ``recognise_seven_point`` accepts is returned as they return it; otherwise the median
    off-diagonal per axis direction and the median diagonal go into three Toeplitz Kronecker terms, as ``recognise_seven_point``
    takes them — so that a uniform region leaves zeros — and the rest into the operator's ``point_stencil``.  Unsymmetric
    matrices, entries outside the neighbourhood and entries across row or plane ends raise UnrecognisedOperator."""
    try:
        return recognise_seven_point(A)
    except UnrecognisedOperator:
        if isinstance(A, StructuredOperator):
            raise
    if not sp.issparse(A):
        A = sp.csr_matrix(np.asarray(A, dtype=np.float64))
    key = ("27_point",) + _cache_key(A)
    hit = _CACHE.get(key)
    if hit is not None and hit[0] is A:
        return hit[1]
    n = A.shape[0]
    if A.shape[0] != A.shape[1] or np.iscomplexobj(A):
        raise UnrecognisedOperator("recognise_27_point: a real square matrix on a g^3 grid is needed")
    g = int(round(n ** (1.0 / 3.0)))
    while g ** 3 > n:
        g -= 1
    while (g + 1) ** 3 <= n:
        g += 1
    if g ** 3 != n or g < 3:          # (on 2^3 points the 27 offsets are not distinct matrix diagonals)
        raise UnrecognisedOperator("3-D operator size %d is not a cube number of at least 3^3" % n)
    M = sp.csr_matrix(A, dtype=np.float64, copy=True)
    M.eliminate_zeros()
    G = np.zeros((3, 3, 3, g, g, g))
    counted = 0
    for a, b, c in np.ndindex(3, 3, 3):
        off = (a - 1) * g * g + (b - 1) * g + (c - 1)
        band = np.zeros(n)
        d = M.diagonal(off)
        if off >= 0:
            band[:n - off] = d
        else:
            band[-off:] = d
        counted += np.count_nonzero(band)
        G[a, b, c] = band.reshape(g, g, g)                # [z, y, x] of the row
    if counted != M.nnz:
        raise UnrecognisedOperator("3-D operator is not a 27-point matrix: it has entries outside the 3 x 3 x 3 neighbourhood")
    if G[:, :, 0, :, :, 0].any() or G[:, :, 2, :, :, -1].any() or G[:, 0, :, :, 0, :].any() or G[:, 2, :, :, -1, :].any():
        raise UnrecognisedOperator("3-D operator is not a 27-point matrix: it has entries across the row or plane ends")
    try:
        _check_point_stencil(G)
    except ValueError:
        raise UnrecognisedOperator("3-D 27-point operator is not symmetric: a per-point stencil describes symmetric matrices only")
    base = float(np.median(G[1, 1, 1]))
    cx, cy, cz = float(np.median(G[1, 1, 2][:, :, :-1])), float(np.median(G[1, 2, 1][:, :-1, :])), float(np.median(G[2, 1, 1][:-1, :, :]))
    Xt, Yt, Zt = _toeplitz_tri(cx, base - 2.0 * (base / 3.0), cx, g), _toeplitz_tri(cy, base / 3.0, cy, g), _toeplitz_tri(cz, base / 3.0, cz, g)
    G[1, 1, 1] -= base
    G[1, 1, 2][:, :, :-1] -= cx
    G[1, 1, 0][:, :, 1:] -= cx
    G[1, 2, 1][:, :-1, :] -= cy
    G[1, 0, 1][:, 1:, :] -= cy
    G[2, 1, 1][:-1, :, :] -= cz
    G[0, 1, 1][1:, :, :] -= cz
    i = tri_identity(g)
    op = StructuredOperator("3d", g, [(i, i.copy(), Xt), (i.copy(), Yt, i.copy()), (Zt, i.copy(), i.copy())], point_stencil=G)
    if len(_CACHE) > 64:
        _CACHE.clear()
    _CACHE[key] = (A, op)
    return op


def _recognise_potential_3d(A):
    """recognise_potential on g^3 grids: what ``recognise(A, "3d")`` maps is returned as it returns it; otherwise the six
    bands (``_bands_3d``'s checks) and the median diagonal entry become three Toeplitz-diagonal Kronecker terms and the rest
    of the diagonal the operator's ``point_diagonal``."""
    try:
        return recognise(A, "3d")
    except UnrecognisedOperator:
        if isinstance(A, StructuredOperator):
            raise
    if not sp.issparse(A):
        A = sp.csr_matrix(np.asarray(A, dtype=np.float64))
    key = ("potential3d",) + _cache_key(A)
    hit = _CACHE.get(key)
    if hit is not None and hit[0] is A:
        return hit[1]
    g, M, d0, xs, ys, zs = _bands_3d(A)
    base = float(np.median(d0))
    Zt, Yt, Xt = np.zeros((3, g)), np.zeros((3, g)), np.zeros((3, g))
    Zt[0], Zt[1], Zt[2] = zs[1], base / 3.0, zs[0]
    Yt[0], Yt[1], Yt[2] = ys[1], base / 3.0, ys[0]
    Xt[0], Xt[1], Xt[2] = xs[1], base - 2.0 * (base / 3.0), xs[0]
    i = tri_identity(g)
    op = StructuredOperator("3d", g, [(i, i.copy(), Xt), (i.copy(), Yt, i.copy()), (Zt, i.copy(), i.copy())], point_diagonal=d0 - base)
    if len(_CACHE) > 64:
        _CACHE.clear()
    _CACHE[key] = (A, op)
    return op


def _bands_3d(A):
    """(g, M, d0, xs, ys, zs) of a sparse 7-point matrix on a g^3 grid whose off-diagonal bands along each axis depend on
    that axis' index only: the diagonal as a [z, y, x] array and per axis the (upper, lower) band as a function of the index.
    Anything else raises UnrecognisedOperator."""
    n = A.shape[0]
    if A.shape[0] != A.shape[1]:
        raise UnrecognisedOperator("operator must be square")
    if np.iscomplexobj(A):
        raise UnrecognisedOperator("complex operators are not supported by the HIP path")
    g = int(round(n ** (1.0 / 3.0)))
    while g ** 3 > n:
        g -= 1
    while (g + 1) ** 3 <= n:
        g += 1
    if g ** 3 != n or g < 2:
        raise UnrecognisedOperator("3-D operator size %d is not a cube number" % n)
    M = sp.csr_matrix(A, dtype=np.float64, copy=True)
    M.eliminate_zeros()

    def band(off):
        out = np.zeros(n)
        d = M.diagonal(off)
        if off >= 0:
            out[:n - off] = d
        else:
            out[-off:] = d
        return out.reshape(g, g, g)                       # [z, y, x] of the row

    d0 = M.diagonal(0).reshape(g, g, g)
    bands = {off: band(off) for off in (1, -1, g, -g, g * g, -g * g)}
    if sum(np.count_nonzero(b) for b in bands.values()) + np.count_nonzero(d0) != M.nnz:
        raise UnrecognisedOperator("3-D operator has entries off the 7-point stencil")

    def along(b, axis):
        """the band's values as a function of the index along `axis` alone, or None"""
        line = np.moveaxis(b, axis, -1)[0, 0]
        return line if np.array_equal(b, np.moveaxis(np.broadcast_to(line, (g, g, g)), -1, axis)) else None

    xs = [along(bands[1], 2), along(bands[-1], 2)]
    ys = [along(bands[g], 1), along(bands[-g], 1)]
    zs = [along(bands[g * g], 0), along(bands[-g * g], 0)]
    if any(a is None for a in xs + ys + zs):
        raise UnrecognisedOperator("3-D operator's off-diagonals are not of the form X (x) I (x) I + I (x) Y (x) I + I (x) I (x) Z")
    return g, M, d0, xs, ys, zs


def _recognise_3d(A):
    """X (x) I (x) I + I (x) Y (x) I + I (x) I (x) Z on a g^3 grid (idx = z g^2 + y g + x): scaled and shifted 3-D
    Laplacians and additively separable diagonals.  The off-diagonals along each axis must depend on that axis' index
    only; the diagonal is split into three parts and the result verified by re-assembly."""
    if not sp.issparse(A):
        A = sp.csr_matrix(np.asarray(A, dtype=np.float64))
    tagged = getattr(A, "_mgcmt_structured", None)
    if tagged is not None and tagged[1] == _digest(A) and tagged[0].dimension == "3d":
        return tagged[0]
    key = _cache_key(A)
    hit = _CACHE.get(key)
    if hit is not None and hit[0] is A and hit[1].dimension == "3d":
        return hit[1]
    g, M, d0, xs, ys, zs = _bands_3d(A)
    c = d0[0, 0, 0] / 3.0
    Zt, Yt, Xt = np.zeros((3, g)), np.zeros((3, g)), np.zeros((3, g))
    Zt[0], Zt[1], Zt[2] = zs[1], d0[:, 0, 0] - 2.0 * c, zs[0]
    Yt[0], Yt[1], Yt[2] = ys[1], d0[0, :, 0] - 2.0 * c, ys[0]
    Xt[0], Xt[1], Xt[2] = xs[1], d0[0, 0, :] - 2.0 * c, xs[0]
    i = tri_identity(g)
    op = StructuredOperator("3d", g, [(i, i.copy(), Xt), (i.copy(), Yt, i.copy()), (Zt, i.copy(), i.copy())])
    D = (M - op.tocsr()).tocsr()
    scale = max(np.abs(M.data).max() if M.nnz else 0.0, 1e-300)
    if D.nnz and np.abs(D.data).max() > 16 * np.finfo(float).eps * scale:
        raise UnrecognisedOperator("3-D operator's diagonal is not additively separable a(z) + b(y) + c(x)")
    if len(_CACHE) > 64:
        _CACHE.clear()
    _CACHE[key] = (A, op)
    return op


def _recognise_12(A, dimension=None):
    """StructuredOperator for a scipy.sparse matrix of the shapes the reference's callers build.

    1-D: any tridiagonal matrix.  2-D: a 5-point operator  I (x) Y + X (x) I  whose diagonal is
    d(i,j) = a(i) + b(j) [+ p(i) q(j)] — scaled / shifted Laplacians, separable potentials, and one product
    potential on top (a square well).  Anything else raises UnrecognisedOperator: the HIP path has no general-sparse kernels and there is no CPU
    fallback.
    """
    if isinstance(A, StructuredOperator):
        if dimension is not None and A.dimension != dimension:
            raise UnrecognisedOperator("operator is %s but dimension=%r was requested" % (A.dimension, dimension))
        return A
    if not sp.issparse(A):
        A = sp.csr_matrix(np.asarray(A, dtype=np.float64))
    tagged = getattr(A, "_mgcmt_structured", None)
    if tagged is not None and tagged[1] == _digest(A) and (dimension is None or tagged[0].dimension == dimension):
        return tagged[0]                      # a matrix this package assembled itself (e.g. a Galerkin level handed to a smoother)
    key = _cache_key(A)
    hit = _CACHE.get(key)
    if hit is not None and hit[0] is A and (dimension is None or hit[1].dimension == dimension):
        return hit[1]
    n = A.shape[0]
    if A.shape[0] != A.shape[1]:
        raise UnrecognisedOperator("operator must be square")
    if np.iscomplexobj(A):
        raise UnrecognisedOperator("complex operators are not supported by the HIP path")
    M = sp.csr_matrix(A, dtype=np.float64, copy=True)
    M.eliminate_zeros()
    nnz = M.nnz
    op = None
    if dimension in (None, "1d"):
        d0, dm, dp = M.diagonal(0), M.diagonal(-1), M.diagonal(1)
        if np.count_nonzero(d0) + np.count_nonzero(dm) + np.count_nonzero(dp) == nnz:
            y = np.zeros((3, n))
            y[0, 1:], y[1], y[2, :-1] = dm, d0, dp
            op = StructuredOperator("1d", n, [(None, y)])
    if op is None and dimension in (None, "2d"):
        g = int(round(math.sqrt(n)))
        if g * g != n:
            raise UnrecognisedOperator("2-D operator size %d is not a square number" % n)
        d0 = M.diagonal(0).reshape(g, g)
        e = np.zeros(n)
        e[:-1] = M.diagonal(1)
        w = np.zeros(n)
        w[1:] = M.diagonal(-1)
        s = np.zeros(n)
        s[:-g] = M.diagonal(g)
        nn = np.zeros(n)
        nn[g:] = M.diagonal(-g)
        counted = sum(np.count_nonzero(a) for a in (d0, e, w, s, nn))
        e, w, s, nn = e.reshape(g, g), w.reshape(g, g), s.reshape(g, g), nn.reshape(g, g)
        ok = counted == nnz and not e[:, -1].any() and not w[:, 0].any()
        ok = ok and np.array_equal(e, np.broadcast_to(e[0], (g, g))) and np.array_equal(w, np.broadcast_to(w[0], (g, g)))
        ok = ok and np.array_equal(s, np.broadcast_to(s[:, :1], (g, g))) and np.array_equal(nn, np.broadcast_to(nn[:, :1], (g, g)))
        extra = None
        if ok:
            c = 0.5 * d0[0, 0]
            yd = d0[0, :] - c
            xd = d0[:, 0] - d0[0, 0] + c
            scale = max(np.abs(d0).max(), 1e-300)
            rest = d0 - (xd[:, None] + yd[None, :])          # what an additively separable diagonal leaves over
            if np.abs(rest).max() > 4 * np.finfo(float).eps * scale:
                # a product potential on top, e.g. the square well V0 (1 - chi (x) chi) of PotWellSolver.py:150-153 in
                # 2-D: the remainder must be ONE outer product p (x) q (the kernels take three Kronecker terms)
                i0, j0 = np.unravel_index(np.argmax(np.abs(rest)), rest.shape)
                p_, q_ = rest[:, j0] / rest[i0, j0], rest[i0, :].copy()
                ok = np.abs(np.outer(p_, q_) - rest).max() <= 64 * np.finfo(float).eps * scale
                extra = (p_, q_)
        if not ok:
            op = _constant_nine_point(M, g)
            if op is None:
                raise UnrecognisedOperator(
                    "2-D operator is neither of the form I (x) Y + X (x) I (+ one product potential p (x) q on the diagonal) "
                    "nor a constant 9-point stencil; the HIP path handles scaled/shifted Laplacians with separable or "
                    "square-well potentials and constant compact stencils only")
            if len(_CACHE) > 64:
                _CACHE.clear()
            _CACHE[key] = (A, op)
            return op
        Y = np.zeros((3, g))
        Y[0], Y[1], Y[2] = w[0], yd, e[0]
        X = np.zeros((3, g))
        X[0], X[1], X[2] = nn[:, 0], xd, s[:, 0]
        terms = [(tri_identity(g), Y), (X, tri_identity(g))]
        if extra is not None:
            dp, dq = np.zeros((3, g)), np.zeros((3, g))
            dp[1], dq[1] = extra
            terms.append((dp, dq))
        op = StructuredOperator("2d", g, terms)
    if op is None:
        raise UnrecognisedOperator("operator is not tridiagonal (1-D)")
    if len(_CACHE) > 64:
        _CACHE.clear()
    _CACHE[key] = (A, op)
    return op


def _toeplitz_tri(lo, di, up, g):
    t = np.zeros((3, g))
    t[0, 1:], t[1], t[2, :-1] = lo, di, up
    return t


def _constant_nine_point(M, g):
    """A constant 3 x 3 stencil c on the g x g grid (zero Dirichlet truncation) — e.g. the Mehrstellen Laplacian, shifted
    or scaled — as  sum_a E_a (x) T(c[a, :])  with E_a the unit sub-/main/super-diagonal: exact, no arithmetic on the
    entries (rows 0 and 2 of a stencil that is symmetric top to bottom share one term).  None if M is not of that form."""
    if g < 3:
        return None
    r0 = g + 1
    row = M.getrow(r0)
    c = np.zeros((3, 3))
    for col, val in zip(row.indices, row.data):
        a, b = col // g - 1 + 1, col % g - 1 + 1
        if not (0 <= a <= 2 and 0 <= b <= 2):
            return None
        c[a, b] = val
    if np.array_equal(c[0], c[2]):
        terms = [(_toeplitz_tri(1.0, 0.0, 1.0, g), _toeplitz_tri(*c[0], g)), (tri_identity(g), _toeplitz_tri(*c[1], g))]
    else:
        terms = [(_toeplitz_tri(1.0, 0.0, 0.0, g), _toeplitz_tri(*c[0], g)), (tri_identity(g), _toeplitz_tri(*c[1], g)),
                 (_toeplitz_tri(0.0, 0.0, 1.0, g), _toeplitz_tri(*c[2], g))]
    terms = [(x, y) for x, y in terms if y.any()]
    if not terms:
        return None
    B = sum(sp.kron(tri_to_sparse(x), tri_to_sparse(y), format="csr") for x, y in terms).tocsr()
    D = (M - B).tocsr()
    if D.nnz and np.abs(D.data).max() != 0.0:
        return None
    return StructuredOperator("2d", g, terms)


def planes_to_csr(G):
    """The sparse matrix of a per-point stencil as ``Plan.point_stencil`` returns it below level 0: G[a, b, i, j] (2-D, nine
    planes) or G[a, b, c, z, y, x] (3-D, 27 planes) is the coefficient of the neighbour at offset (a - 1, b - 1[, c - 1]) in
    the row of the point.  Entries towards points outside the grid are dropped (the library stores zeros there)."""
    G = np.asarray(G)
    d = G.ndim // 2
    gl = G.shape[-1]
    idx = np.meshgrid(*([np.arange(gl)] * d), indexing="ij")
    flat = lambda coords: sum(c * gl ** (d - 1 - k) for k, c in enumerate(coords))
    rows, cols, vals = [], [], []
    for off in np.ndindex(*([3] * d)):
        nb = [i + o - 1 for i, o in zip(idx, off)]
        ok = np.logical_and.reduce([(c >= 0) & (c < gl) for c in nb])
        rows.append(flat(idx)[ok])
        cols.append(flat(nb)[ok])
        vals.append(G[off][ok])
    n = gl ** d
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))


def tag_structured(matrix, op):
    """Remember on a scipy matrix assembled from `op` what it was assembled from (with a content digest, so a matrix
    changed afterwards is not mistaken for it): ``recognise`` then maps it back without the structural check, also for
    the 9-point Galerkin operators that check does not cover."""
    matrix._mgcmt_structured = (op, _digest(matrix))
    return matrix
