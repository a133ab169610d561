"""A dense restatement of the Schroedinger-Poisson loop of drivers.schroedinger_poisson, for the tests: scipy.linalg.eigh for the
states, a sparse LU factorisation for the potential, the same definition of a step, of the change d and of the stopping rule —
written from the matrices the operators stand for (``tocsr``), nothing of the device code."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as sla

from multigridcmt_amd.operators import potential_operator, variable_mass_operator

U = 2.0 ** -53


def gamma(m):
    return m * U / (1.0 - m * U)


def restatement(op, poisson_op, k, occupations, coupling, mixing, tol, maxiter=200):
    """(eigenvalues[k], phi, changes): step m solves H[phi_(m-1)] = op + coupling diag(phi_(m-1)) for its k lowest states,
    rho = sum_j f_j psi_j^2 with unit vectors, poisson_op phi_new = rho, d_m = ||phi_new - phi_(m-1)|| / ||phi_new||,
    phi_m = (1 - mixing) phi_(m-1) + mixing phi_new; phi_0 = 0; the loop ends with the step whose d <= tol.  The eigenvalues are
    those of the last step's operator, as the driver returns them."""
    dense = op.shape[0] <= 2048            # (beyond that: shift-and-invert Lanczos to machine precision on the sparse matrix)
    H0 = op.tocsr().toarray() if dense else op.tocsr().tocsc()
    lu = sla.splu(poisson_op.tocsr().tocsc())
    f = np.asarray(occupations, dtype=np.float64)
    n = H0.shape[0]
    phi, changes, vals = np.zeros(n), [], None
    idx = np.arange(n)
    for _ in range(maxiter):
        if dense:
            H = H0.copy()
            H[idx, idx] += coupling * phi
            vals, vecs = scipy.linalg.eigh(H, subset_by_index=[0, k - 1])
        else:
            vals, vecs = sla.eigsh(H0 + sp.diags(coupling * phi).tocsc(), k=k, sigma=0.0, which="LM", tol=0, v0=np.ones(n))
            order = np.argsort(vals)
            vals, vecs = vals[order], vecs[:, order]
        rho = (vecs ** 2) @ f
        new = lu.solve(rho)
        d = float(np.linalg.norm(new - phi) / np.linalg.norm(new))
        changes.append(d)
        phi = (1.0 - mixing) * phi + mixing * new
        if d <= tol:
            break
    return vals, phi, changes


def case_2d(g=32):
    """the dot of the issue: V_ext = 160 ((x - 0.5)^2 + (y - 0.45)^2) on x_i = (i + 1) / (g + 1), eps = 1 on the left half of the
    columns and 3 on the right; (op, poisson_op)"""
    t = (np.arange(g) + 1.0) / (g + 1)
    X, Y = np.meshgrid(t, t, indexing="ij")
    eps = np.ones((g, g))
    eps[:, g // 2:] = 3.0
    return potential_operator(g, 160.0 * ((X - 0.5) ** 2 + (Y - 0.45) ** 2)), variable_mass_operator(g, eps)


def case_3d(g=16):
    """a 3-D dot, slightly off centre so that no level is degenerate by symmetry, in a host with eps = 1 below the middle z-plane
    and 2 above it; (op, poisson_op)"""
    t = (np.arange(g) + 1.0) / (g + 1)
    Z, Y, X = np.meshgrid(t, t, t, indexing="ij")
    eps = np.ones((g, g, g))
    eps[g // 2:] = 2.0
    V = 120.0 * ((X - 0.5) ** 2 + 1.2 * (Y - 0.45) ** 2 + 1.5 * (Z - 0.55) ** 2)
    return potential_operator(g, V, dimension="3d"), variable_mass_operator(g, eps, dimension="3d")
