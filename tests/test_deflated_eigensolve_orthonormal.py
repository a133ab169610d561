"""drivers.deflated_eigensolve(basis="orthonormal"): the iteration of tests/test_deflated_eigensolve.py with a Rayleigh-Ritz basis
[X, W, P] whose columns are orthonormal by construction (mgcmt_block_project, mgcmt_block_orthonormalize; DESIGN.md par. 4.22).

The five cases, the accuracy checks and the rule for the iteration caps are those of tests/test_deflated_eigensolve.py:
`restated_orthonormal` below is a NumPy restatement of the orthonormal algorithm (docstring of the driver) on the assembled
matrix with the oracle's V-cycle as preconditioner, a case asserts info["iterations"] <= ceil(1.25 count).  The two 32^2 box
cases run it inside the test against the shared cycle matrix; the other three were run once by hand
(`PYTHONPATH=. python tests/test_deflated_eigensolve_orthonormal.py` from the repository's root) and are recorded in
RESTATED_BY_HAND.

On top of that: min(info["gram_min"]) >= 0.99 — a condition, not a measurement: the scaled Gram matrix of an orthonormal basis
is the identity, the failure mode of the scaled basis sits at 1e-12 —, no column dropped in any of the five cases, equal bits
for equal seeds, basis="scaled" equal to a call without the argument bit for bit, ValueError for an unknown basis."""
import math

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

from multigridcmt_amd import drivers
from test_deflated_eigensolve import CASES, NU, RTOL, _box, _box32_cycle_matrix, _reference, check_solution, oracle_cycle

# the restatement's iteration counts of the cases it does not run in the test: run once by hand (module docstring)
RESTATED_BY_HAND = {"anharmonic64_k24": 34, "box16_3d_k20": 33, "step_bonds32_k20": 35}
# ... and for 40 states of the 32^2 box with lowest = 4 (tests/test_deflated_eigensolve_orthonormal_full_size_gpu.py)
RESTATED_BOX32_K40 = 53


def cholesky_qr_step(W, AW, drop_tol):
    """mgcmt_block_orthonormalize in NumPy: (W T, AW T, columns dropped) with T = D R^-1, D G D = R^T R by the unpivoted
    right-looking Cholesky factorisation of the unit-diagonal Gram matrix; a column with G_jj zero or a pivot <= drop_tol
    leaves the factorisation and comes back as zeros"""
    k = W.shape[1]
    G = W.T @ W
    G = 0.5 * (G + G.T)
    alive = np.diag(G) > 0.0
    d = np.where(alive, 1.0 / np.sqrt(np.where(alive, np.diag(G), 1.0)), 0.0)
    S = G * np.outer(d, d)
    S[np.diag_indices(k)] = alive.astype(float)
    for t in range(k):
        if not alive[t]:
            continue
        if not S[t, t] > drop_tol:
            alive[t] = False
            S[t, :] = S[:, t] = 0.0
            continue
        S[t, t:] /= np.sqrt(S[t, t])
        for i in range(t + 1, k):
            S[i, i:] -= S[t, i] * S[t, i:]
    keep = np.flatnonzero(alive)
    T = np.zeros((k, k))
    if len(keep):
        R = np.triu(S[np.ix_(keep, keep)])
        T[np.ix_(keep, keep)] = scipy.linalg.solve_triangular(R, np.eye(len(keep))) * d[keep, None]
    return W @ T, (None if AW is None else AW @ T), k - len(keep)


def restated_orthonormal(A, k, cycle, *, rtol=RTOL, atol=0.0, block=None, maxiter=200, seed=0, drop_tol=drivers.ORTHONORMAL_DROP_TOL,
                         record=None):
    """The algorithm of drivers.deflated_eigensolve(basis="orthonormal") in NumPy on the assembled matrix A; `cycle`: the
    preconditioner on a matrix of columns.  Returns (iterations, eigenvalues in locking order); record (a dict) receives
    gram_min and dropped per iteration."""
    n = A.shape[0]
    kb = min(16, k + 4) if block is None else block
    rng = np.random.RandomState(seed)
    X = np.stack([rng.random_sample(n) for _ in range(kb)], axis=1)
    AX = A @ X
    Q = np.zeros((n, 0))
    vals, gram_min, dropped = [], [], []

    def ritz(S, AS, main=False):
        H, G = S.T @ AS, S.T @ S
        G, H = 0.5 * (G + G.T), 0.5 * (H + H.T)
        keep = np.flatnonzero(np.diag(G) != 0.0)
        H, G = H[np.ix_(keep, keep)], G[np.ix_(keep, keep)]
        d = 1.0 / np.sqrt(np.diag(G))
        if main:
            gram_min.append(np.linalg.eigvalsh(G * np.outer(d, d))[0])
            dropped.append(S.shape[1] - len(keep))
        evals, evecs = scipy.linalg.eigh(H * np.outer(d, d), G * np.outer(d, d), subset_by_index=[0, kb - 1])
        C = np.zeros((S.shape[1], kb))
        C[keep] = evecs * d[:, None]
        return evals, C

    def residuals_and_locks(X, AX, Q, rho):
        locked_any = False
        while True:
            R = AX - X * rho
            ok = np.linalg.norm(R, axis=0) <= np.maximum(atol, rtol * np.abs(rho))
            nlock = min(kb if ok.all() else int(np.argmin(ok)), k - len(vals))
            if nlock == 0:
                return X, AX, Q, rho, R, locked_any
            Q = np.hstack([Q, X[:, :nlock]])
            vals.extend(rho[:nlock])
            locked_any = True
            if len(vals) == k:
                return X, AX, Q, rho, R, True
            fresh = np.stack([rng.random_sample(n) for _ in range(nlock)], axis=1)
            fresh = fresh - Q @ (Q.T @ fresh)
            X[:, :nlock] = fresh - X[:, nlock:] @ (X[:, nlock:].T @ fresh)
            AX[:, :nlock] = A @ X[:, :nlock]
            rho, C = ritz(X, AX)
            X, AX = X @ C, AX @ C

    rho, C = ritz(X, AX)
    X, AX, Q, rho, R, _ = residuals_and_locks(X @ C, AX @ C, Q, rho)
    P = AP = None
    iterations = 0
    while len(vals) < k and iterations < maxiter:
        iterations += 1
        Wd = cycle(R)
        for _ in range(2):
            if Q.shape[1]:
                Wd = Wd - Q @ (Q.T @ Wd)
            Wd = Wd - X @ (X.T @ Wd)
            Wd = cholesky_qr_step(Wd, None, drop_tol)[0]
        AW = A @ Wd
        if P is not None:
            B, AB = np.hstack([X, Wd]), np.hstack([AX, AW])
            for _ in range(2):
                Cp = B.T @ P
                P, AP = P - B @ Cp, AP - AB @ Cp
                P, AP, _ = cholesky_qr_step(P, AP, drop_tol)
        S, AS = (np.hstack([X, Wd, P]), np.hstack([AX, AW, AP])) if P is not None else (np.hstack([X, Wd]), np.hstack([AX, AW]))
        rho, C = ritz(S, AS, main=True)
        P, AP = S[:, kb:] @ C[kb:], AS[:, kb:] @ C[kb:]
        X, AX = X @ C[:kb] + P, AX @ C[:kb] + AP
        X, AX, Q, rho, R, locked_any = residuals_and_locks(X, AX, Q, rho)
        if locked_any:
            P = AP = None
    if record is not None:
        record.update(gram_min=np.array(gram_min), dropped=np.array(dropped))
    return iterations, np.array(vals)


_shared = {}


def restated_count(name):
    """iterations of the restatement for a case: run here for the two 32^2 box cases, recorded for the others"""
    if name in RESTATED_BY_HAND:
        return RESTATED_BY_HAND[name]
    if name not in _shared:
        make, dim, k, lowest, _ = CASES[name]
        B = _box32_cycle_matrix()
        record = {}
        _shared[name] = restated_orthonormal(sp.csr_matrix(make().tocsr()), k, lambda R: B @ R, record=record)[0]
        assert record["gram_min"].min() >= 0.99 and record["dropped"].sum() == 0       # (the restatement meets its own conditions)
    return _shared[name]


@pytest.mark.parametrize("name", list(CASES))
def test_orthonormal_cases(backend, name):
    """the five cases of tests/test_deflated_eigensolve.py with basis="orthonormal": its accuracy checks, the cap from the
    orthonormal restatement, a scaled Gram matrix whose smallest eigenvalue stays >= 0.99 in every main-loop Ritz problem, and
    no dropped column"""
    make, dim, k, lowest, _ = CASES[name]
    op = make()
    info = {}
    vals, vecs = drivers.deflated_eigensolve(op, k, rtol=RTOL, nu=NU, info=info, basis="orthonormal", **({} if lowest is None else {"lowest": lowest}))
    count = restated_count(name)
    print("%s: the orthonormal restatement takes %d iterations; min gram_min %.15f, dropped %d"
          % (name, count, info["gram_min"].min(), info["dropped"].sum()))
    check_solution(op, k, vals, vecs, info, _reference(name, op, k), math.ceil(1.25 * count))
    assert info["gram_min"].shape == (info["iterations"],) and info["dropped"].shape == (info["iterations"],)
    assert info["gram_min"].min() >= 0.99
    assert info["dropped"].sum() == 0


def test_two_orthonormal_runs_with_one_seed_give_equal_bits(backend):
    """8 states of the 16^2 box with a block of 6 (locks, refills and a final block larger than what is left), twice"""
    runs = []
    for _ in range(2):
        info = {}
        vals, vecs = drivers.deflated_eigensolve(_box(16), 8, block=6, lowest=4, seed=5, info=info, basis="orthonormal")
        assert info["status"] == "converged"
        runs.append((vals, vecs, info["locked_at"], info["residuals"], info["gram_min"], info["dropped"]))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert np.abs(runs[0][0] - drivers.exact_box_eigenvalues(16, "2d", 8)).max() <= 1e-8


def test_scaled_is_the_default_bit_for_bit(backend):
    """basis="scaled" returns the bits of a call without the argument, and neither reports gram_min or dropped"""
    runs = []
    for kw in ({}, {"basis": "scaled"}):
        info = {}
        vals, vecs = drivers.deflated_eigensolve(_box(16), 8, block=6, lowest=4, seed=5, info=info, **kw)
        assert "gram_min" not in info and "dropped" not in info
        runs.append((vals, vecs, info["locked_at"], info["residuals"], np.array(info["iterations"])))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_unknown_basis_is_refused():
    for basis in ("orthogonal", None, 1):
        with pytest.raises(ValueError, match="basis"):
            drivers.deflated_eigensolve(_box(16), 4, basis=basis)


if __name__ == "__main__":
    # the by-hand counts: the restatement with the oracle's cycle column by column; "box32_k40" for RESTATED_BOX32_K40
    import sys
    import time
    for name in sys.argv[1:] or list(RESTATED_BY_HAND):
        if name == "box32_k40":
            A, B = sp.csr_matrix(_box(32).tocsr()), _box32_cycle_matrix()
            cyc, k = (lambda R: B @ R), 40
        else:
            make, dim, k, lowest, _ = CASES[name]
            A = sp.csr_matrix(make().tocsr())
            cycle = oracle_cycle(A, dim, NU, 8 if lowest is None else lowest)
            cyc = lambda R: np.stack([cycle(r) for r in R.T], axis=1)
        t = time.time()
        record = {}
        its, vals = restated_orthonormal(A, k, cyc, record=record)
        print("%s: %d iterations (%.0f s), min gram_min %.15f, dropped %d, eigenvalues %s .. %s"
              % (name, its, time.time() - t, record["gram_min"].min(), record["dropped"].sum(), vals[:2], vals[-2:]), flush=True)
