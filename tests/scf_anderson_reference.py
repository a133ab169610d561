"""A dense restatement of the Schroedinger-Poisson loop with Anderson (type II, Pulay) mixing of the potential, for the tests:
scipy.linalg.eigh for the states, a sparse LU factorisation for the potential, the Anderson update from the Gram matrix of the
residuals by numpy.linalg.lstsq — written from the matrices the operators stand for (``tocsr``), nothing of the device code.

The iteration.  x_i is the input potential of step i (x_1 = 0), g_i the Poisson solution of that step, r_i = g_i - x_i,
d_i = ||r_i|| / ||g_i||.  The history holds the last p = min(depth + 1, steps since the last restart) pairs (x_i, r_i), oldest
first.  With G_ij = <r_i, r_j> (p x p), D the (p - 1) x p forward-difference matrix (row t: -1 at t, +1 at t + 1) and e_last the
last unit vector:
    A = D G D^T,  b = D G e_last;  s = 1 / sqrt(diag A);  gamma = s * lstsq(s A s, s b, rcond = 1e-12);  alpha = e_last - D^T gamma
(sum alpha = 1; the alpha that minimise ||sum alpha_i r_i||), and x_next = sum_i alpha_i (x_i + beta r_i).  With one pair
alpha = [1]: the damped step x + beta r.  If a diagonal entry of A is not positive or the scaled system is not finite, the
history is restarted: only the newest pair stays, alpha = [1], and the step is recorded as a restart.  The loop ends with the
step whose d <= tol, after its mixing, as the plain loop does."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as sla

from scf_reference import case_2d, case_3d, gamma  # noqa: F401  (the cases and gamma_m of the plain restatement)

RCOND = 1e-12


def anderson_coefficients(G):
    """alpha[p] from the p x p Gram matrix of the residuals (oldest first), or None where the history has to be restarted"""
    G = np.asarray(G, dtype=np.float64)
    p = G.shape[0]
    if p == 1:
        return np.ones(1)
    D = np.zeros((p - 1, p))
    D[np.arange(p - 1), np.arange(p - 1)] = -1.0
    D[np.arange(p - 1), np.arange(1, p)] = 1.0
    A, b = D @ G @ D.T, D @ G[:, -1]
    diag = np.diag(A)
    if not np.all(np.isfinite(diag)) or not np.all(diag > 0.0):
        return None
    s = 1.0 / np.sqrt(diag)
    As, bs = A * s[:, None] * s[None, :], b * s
    if not (np.all(np.isfinite(As)) and np.all(np.isfinite(bs))):
        return None
    alpha = -(D.T @ (s * np.linalg.lstsq(As, bs, rcond=RCOND)[0]))
    alpha[-1] += 1.0
    return alpha if np.all(np.isfinite(alpha)) else None


def restatement(op, poisson_op, k, occupations, coupling, beta, depth, tol, maxiter=200):
    """(eigenvalues[k], phi, changes, depths, restarts): the loop of the module docstring with ``depth`` history vectors beyond
    the newest (depth = 0: plain mixing, the loop of scf_reference.restatement); depths is the p of every step, restarts the
    steps (counted from 1) at which the history was reset; phi is the last mixed potential."""
    dense = op.shape[0] <= 2048            # (beyond that: shift-and-invert Lanczos to machine precision on the sparse matrix)
    H0 = op.tocsr().toarray() if dense else op.tocsr().tocsc()
    lu = sla.splu(poisson_op.tocsr().tocsc())
    f = np.asarray(occupations, dtype=np.float64)
    n = H0.shape[0]
    x, vals = np.zeros(n), None
    xs, rs, changes, depths, restarts = [], [], [], [], []
    idx = np.arange(n)
    for step in range(1, maxiter + 1):
        if dense:
            H = H0.copy()
            H[idx, idx] += coupling * x
            vals, vecs = scipy.linalg.eigh(H, subset_by_index=[0, k - 1])
        else:
            vals, vecs = sla.eigsh(H0 + sp.diags(coupling * x).tocsc(), k=k, sigma=0.0, which="LM", tol=0, v0=np.ones(n))
            order = np.argsort(vals)
            vals, vecs = vals[order], vecs[:, order]
        g = lu.solve((vecs ** 2) @ f)
        r = g - x
        d = float(np.linalg.norm(r) / np.linalg.norm(g))
        changes.append(d)
        xs.append(x)
        rs.append(r)
        del xs[:-(depth + 1)], rs[:-(depth + 1)]
        R = np.stack(rs, axis=1)
        alpha = anderson_coefficients(R.T @ R)
        if alpha is None:
            restarts.append(step)
            del xs[:-1], rs[:-1]
            alpha = np.ones(1)
        depths.append(len(xs))
        x = sum(a * (xi + beta * ri) for a, xi, ri in zip(alpha, xs, rs))
        if d <= tol:
            break
    return vals, x, changes, depths, restarts
