"""Python-3 counterparts of the compute sections of the reference's driver scripts (no plotting).

* ``shift_invert_eigenpairs``  — 1DPotMatrixVcycle.py:42-80 / 2DPotMatrixVcycle.py:54-109: coarse-grid Lanczos
  guesses, interpolation to the fine grid, then ``max_iters`` rounds of  w = vcycle_matrix(0, V, H, shifts=guesses),
  V = normalised columns of w  (shift-and-invert iteration whose linear solves are single V-cycles).
* ``rayleigh_quotient_multigrid`` — RQMin.py:15-50: ``vcycle_rqmg`` sweeps for the lowest pair with Gram-Schmidt
  deflation.

Every V-cycle, interpolation, Gram-Schmidt and operator application runs on the GPU through MGCMTSolver /
MGCMTProcessor; the coarse-grid ``eigsh`` stays on the host as in the reference (16 .. 256 unknowns).
"""
import math

import numpy as np
import scipy.linalg
import scipy.sparse as sparse
import scipy.sparse.linalg as sparsela

from .processor import MGCMTProcessor
from .solver import MGCMTSolver
from .stencil_maker import MGCMTStencilMaker


def exact_box_eigenvalues(gridsize, dimension, count):
    """Eigenvalues of -laplacian(gridsize)/pi^2 (the discrete operator, not the continuum n^2): in 1-D
    (4 g^2/pi^2) sin^2(k pi / (2 (g+1))), k = 1..g; in 2-D all pairwise sums, in 3-D all triple sums, sorted."""
    k = np.arange(1, gridsize + 1)
    one_d = (4.0 * gridsize ** 2 / np.pi ** 2) * np.sin(k * np.pi / (2.0 * (gridsize + 1))) ** 2
    if dimension == "1d":
        return one_d[:count]
    m = min(gridsize, count + 2)
    if dimension == "3d":
        return np.sort(np.add.outer(np.add.outer(one_d[:m], one_d[:m]), one_d[:m]).ravel())[:count]
    return np.sort(np.add.outer(one_d[:m], one_d[:m]).ravel())[:count]


def shift_invert_eigenpairs(dimension="1d", gridsize=2 ** 7, bad_gridsize=2 ** 4, num_eigenvalues=10, max_iters=10,
                            lowest_level=None, tolerance=1e-4, guesses=None, smoother=None, verbose=False):
    """Returns dict(eigenvalues, eigenvectors, guess_eigenvalues, history) for H = -laplacian/pi^2 on a box.

    Defaults are 1DPotMatrixVcycle.py's (128 points, guesses from 16, ten pairs, ten iterations, coarsest V-cycle
    level 16); 2DPotMatrixVcycle.py uses gridsize 64, bad_gridsize 16, max_iters 5, lowest_level 8,
    tolerance = machine epsilon.  ``guesses`` = (values, vectors) skips the Lanczos step (ARPACK's start vector is
    random, so fixtures store its output).
    """
    stencil_maker, solver = MGCMTStencilMaker(), MGCMTSolver()
    if lowest_level is None:
        lowest_level = 2 ** 4 if dimension == "1d" else 2 ** 3
    hamiltonian = (-1 / np.pi ** 2) * stencil_maker.laplacian(gridsize, dimension=dimension)
    n = hamiltonian.shape[0]
    if guesses is None:
        bad_hamiltonian = (-1. / np.pi ** 2) * stencil_maker.laplacian(bad_gridsize, dimension=dimension)
        bad_eigenvalues, bad_eigenvectors = sparsela.eigsh(bad_hamiltonian, k=num_eigenvalues, which="SM", tol=tolerance)
    else:
        bad_eigenvalues, bad_eigenvectors = guesses
    bad_eigenvectors = np.array(bad_eigenvectors)
    vectors = np.zeros((n, num_eigenvalues))
    for j in range(num_eigenvalues):
        vectors[:, j] = solver.interpolate(bad_eigenvectors[:, j], stencil_maker, gridsize, dimension=dimension)
        vectors[:, j] /= np.linalg.norm(vectors[:, j])
    history = np.zeros((max_iters + 1, num_eigenvalues))
    history[0] = [np.dot(vectors[:, j], hamiltonian.dot(vectors[:, j])) for j in range(num_eigenvalues)]
    w0 = np.zeros((n, num_eigenvalues))
    for it in range(1, max_iters + 1):
        w = solver.vcycle_matrix(w0, vectors, hamiltonian, stencil_maker, shifts=bad_eigenvalues, smoother=smoother,
                                 lowest_level=lowest_level, dimension=dimension)
        for j in range(num_eigenvalues):
            vectors[:, j] = w[:, j] / np.linalg.norm(w[:, j])
            history[it, j] = np.dot(vectors[:, j], hamiltonian.dot(vectors[:, j]))
        if verbose:
            print(it, history[it])
    return {"eigenvalues": history[-1].copy(), "eigenvectors": vectors, "guess_eigenvalues": np.array(bad_eigenvalues),
            "history": history}


def nested_iteration_guesses(plan, k, coarse_level, kind, omega, iterations_per_level=1):
    """Eigenpair guesses by nested iteration (full multigrid for the eigenproblem: the reference's report names it as the
    next step — PDF p.17 "FMG", p.51 "Volgende stappen" — its code starts from straight interpolation of coarse Lanczos
    vectors instead, 2DPotMatrixVcycle.py:59-85).  The k lowest eigenpairs of the plan's Galerkin operator on
    ``coarse_level`` are computed densely on the host (a few hundred unknowns, like the reference's coarse ``eigsh``);
    on the way up every level takes the interpolated vectors and improves them by ``iterations_per_level`` rounds of
    the reference's own outer iteration (k-column V-cycle with the coarse eigenvalues as shifts and Gram-Schmidt, then
    normalisation) on THAT level's operator.  Leaves the guesses in slot F of level 0 (normalised) and returns the
    shifts.  Parity: unpinned (no reference counterpart); checked against the straight-interpolation guesses by the
    residuals it produces (tests/test_drivers.py)."""
    from . import _lib
    from .operators import StructuredOperator
    V, F = _lib.SLOT_V, _lib.SLOT_F
    xf = plan.factors(coarse_level, 0) if plan.dim == 2 else None
    yf = plan.factors(coarse_level, 1)
    terms = [((xf[m].copy() if xf is not None else None), yf[m].copy()) for m in range(yf.shape[0])]
    dense = StructuredOperator("2d" if plan.dim == 2 else "1d", plan.g >> coarse_level, terms).tocsr().toarray()
    values, vectors = scipy.linalg.eigh(0.5 * (dense + dense.T))
    shifts = values[:k].copy()
    for j in range(k):
        plan.upload(coarse_level, F, j, np.ascontiguousarray(vectors[:, j]))
    for l in range(coarse_level - 1, -1, -1):
        for j in range(k):
            plan.prolong(l, (F, j), (F, j), accumulate=False)
        plan.normalize(l, F, k)
        if l > 0:
            for _ in range(int(iterations_per_level)):
                plan.set_shifts(shifts)
                plan.vcycle(4, 4, kind, omega=omega, k=k, nu_coarse=4, gram_schmidt=True, level=l, zero_start=True)
                plan.normalize(l, V, k)
                for j in range(k):
                    plan.copy(l, V, j, F, j)
    return shifts


def shift_invert_eigenpairs_resident(dimension="2d", gridsize=2 ** 10, bad_gridsize=2 ** 4, num_eigenvalues=10, max_iters=5,
                                     lowest_level=None, tolerance=1e-4, guesses=None, smoother=None, stats=None,
                                     gram_schmidt="inside", residuals=None, guess_method="interpolate"):
    """The outer loops of 1DPotMatrixVcycle.py:42-80 / 2DPotMatrixVcycle.py:54-109 / 1DPotMGS.py:50-127 with everything
    between the coarse-grid guesses and the final download resident on the GPU: the guesses are interpolated level by
    level inside the plan; every iteration is one k-column V-cycle (one shift per column), a column normalisation, k
    device copies, and ONE batched pass that yields all k Rayleigh quotients and residual norms ||(H - mu_j) v_j||
    (2DPotMatrixVcycle.py:100-105) with a single synchronisation (mgcmt_rayleigh_residual).

    gram_schmidt: where the columns are orthogonalised — the three variants 1DPotMGS.py compares:
      "inside"  at every level on the way up of the cycle (vcycle_matrix, MGCMTSolver.py:434; 1DPotMGS.py:104-124)
      "after"   once per outer iteration, after normalisation and after the Rayleigh quotients are taken (:77-98)
      "none"    never: k independent single-vector cycles (:50-72)
    guess_method: "interpolate" (the reference: coarse eigenvectors interpolated straight to the fine grid) or "fmg"
    (``nested_iteration_guesses``; ``guesses`` is then ignored and bad_gridsize names the coarsest eigen-grid).
    Returns dict(eigenvalues, eigenvectors, guess_eigenvalues, history[, residual_history]); ``residuals`` (a list)
    also receives the residual norms after every iteration; ``stats`` the seconds spent in the iteration loop."""
    import time
    from . import _lib
    from .operators import laplacian_operator
    from .plan import Plan
    if gram_schmidt not in ("inside", "after", "none"):
        raise ValueError("gram_schmidt must be 'inside', 'after' or 'none'")
    stencil_maker, solver = MGCMTStencilMaker(), MGCMTSolver()
    g, k = int(gridsize), int(num_eigenvalues)
    if lowest_level is None:
        lowest_level = 2 ** 4 if dimension == "1d" else 2 ** 3
    lowest_level = min(int(lowest_level), int(bad_gridsize))
    kind, omega = solver._resolve_smoother(smoother)
    if kind is None:
        raise NotImplementedError("the device-resident loop takes MGCMTSolver's own smoothers; use shift_invert_eigenpairs for a callable")
    V, F = _lib.SLOT_V, _lib.SLOT_F
    plan = Plan(laplacian_operator(g, dimension) * (-1 / np.pi ** 2), lowest_level, nvec=k)
    try:
        lb = (g // int(bad_gridsize)).bit_length() - 1          # level of the guess grid
        if guess_method == "fmg":
            bad_eigenvalues = nested_iteration_guesses(plan, k, lb, kind, omega)
        elif guess_method == "interpolate":
            if guesses is None:
                bad_hamiltonian = (-1. / np.pi ** 2) * stencil_maker.laplacian(bad_gridsize, dimension=dimension)
                bad_eigenvalues, bad_eigenvectors = sparsela.eigsh(bad_hamiltonian, k=k, which="SM", tol=tolerance)
            else:
                bad_eigenvalues, bad_eigenvectors = guesses
            bad_eigenvalues, bad_eigenvectors = np.asarray(bad_eigenvalues, dtype=float), np.array(bad_eigenvectors, dtype=float)
            for j in range(k):
                plan.upload(lb, F, j, bad_eigenvectors[:, j])
                for l in range(lb - 1, -1, -1):
                    plan.prolong(l, (F, j), (F, j), accumulate=False)
            plan.normalize(0, F, k)
        else:
            raise ValueError("guess_method must be 'interpolate' or 'fmg'")
        plan.set_shifts(bad_eigenvalues)

        history = np.zeros((max_iters + 1, k))
        residual_history = np.zeros((max_iters + 1, k))
        history[0], residual_history[0] = plan.rayleigh_residual(0, F, k)
        plan.sync()
        start = time.perf_counter()
        for it in range(1, max_iters + 1):
            plan.vcycle(4, 4, kind, omega=omega, k=k, nu_coarse=4, gram_schmidt=(gram_schmidt == "inside"), zero_start=True)
            plan.normalize(0, V, k)
            for j in range(k):
                plan.copy(0, V, j, F, j)
            history[it], residual_history[it] = plan.rayleigh_residual(0, F, k)
            if residuals is not None:
                residuals.append(residual_history[it].copy())
            if gram_schmidt == "after":
                plan.gramschmidt(0, F, k, modified=1)        # processor.gramschmidt(eigenvectors), 1DPotMGS.py:98
        plan.sync()
        if stats is not None:
            stats["loop_seconds"] = time.perf_counter() - start
        vectors = np.stack([plan.download(0, F, j) for j in range(k)], axis=1)
    finally:
        plan.close()
    return {"eigenvalues": history[-1].copy(), "eigenvectors": vectors, "guess_eigenvalues": np.asarray(bad_eigenvalues),
            "history": history, "residual_history": residual_history}


def rayleigh_quotient_multigrid(gridsize=2 ** 6, first_cycles=2, second_cycles=10, seed=0):
    """RQMin.py:15-50 for the two lowest states of -laplacian(gridsize)/pi^2 with M = I: ``first_cycles`` sweeps of
    vcycle_rqmg on a random start, then ``second_cycles`` sweeps on a second random vector with Gram-Schmidt against
    the first after every sweep.  Returns (rho1, rho2, X)."""
    stencil_maker, solver, processor = MGCMTStencilMaker(), MGCMTSolver(), MGCMTProcessor()
    A = (-1 / np.pi ** 2) * stencil_maker.laplacian(gridsize)
    M = sparse.eye(gridsize)
    rng = np.random.RandomState(seed)
    x = rng.random_sample(gridsize)
    rho = 0.0
    for _ in range(first_cycles):
        x, rho = solver.vcycle_rqmg(x, A, M)
    x_matrix = np.zeros((gridsize, 2))
    x_matrix[:, 0] = x
    x_matrix[:, 1] = rng.random_sample(gridsize)
    rho2 = 0.0
    for _ in range(second_cycles):
        x_matrix[:, 1], rho2 = solver.vcycle_rqmg(x_matrix[:, 1], A, M)
        x_matrix = processor.gramschmidt(x_matrix)
    return rho, rho2, x_matrix


def potential_well_eigensolve(gridsize=2 ** 7, depth=50.0, inner=None, cycles=8, method="vcycle", nu=2, lowest=8,
                              smoother="rb", seed=0, history=None, stats=None, dimension="2d"):
    """BASELINE config 5: the ground state of the 2-D square well  H = -laplacian/pi^2 + V  (V = `depth` outside the
    central square, PotWellSolver.py:150-153 carried to 2-D) by Rayleigh-quotient minimisation on the GPU.

    method="rqmg"    ``cycles`` sweeps of MGCMTSolver.vcycle_rqmg (RQMin.py:25-27 with the 2-D transfers).
    method="vcycle"  Rayleigh-quotient minimisation with a V-cycle preconditioner: every iteration applies one V(nu,nu)
                     cycle of H (from a zero start) to the gradient g = 2 (H x - rho x) and minimises the Rayleigh
                     quotient over span{x, w} — the 2x2 problem of rqmin (MGCMTSolver.py:33-50) with the
                     preconditioned gradient as the search direction — by the two passes of the device-resident rqmin
                     (Plan.rq_line_step: the eight inner products with H w formed in registers, the pencil solved on
                     the device, then x + delta w and its gradient in one pass).  Per iteration: one V-cycle from a zero
                     start (a flag: V is neither cleared nor read) and 48 B per point of vector traffic beside it;
                     nothing comes back to the host inside the loop (the Rayleigh quotients are recorded on the
                     device and fetched once).
    dimension="3d" (addition): the cube well (a quantum dot) on g^3 points, potential_well_operator(..., dimension="3d");
    both methods run on a plan that carries M = I explicitly (the Rayleigh-quotient entries of a 3-D plan need one), and
    ``lowest`` is at most 16.
    Returns (rho, x); ``history`` (a list) receives rho after every cycle, ``stats`` (a dict) the seconds spent in
    the iteration loop alone (start vector generation and the host transfers excluded)."""
    from . import _lib
    from .operators import identity_operator, potential_well_operator
    from .plan import get_plan
    g = int(gridsize)
    if inner is None:
        inner = (g // 4, 3 * g // 4)
    if dimension not in ("2d", "3d"):
        raise ValueError("dimension must be '2d' or '3d'")
    three = dimension == "3d"
    op = potential_well_operator(g, depth, inner, dimension=dimension)
    rng = np.random.RandomState(seed)
    x0 = rng.random_sample(g ** 3 if three else g * g)
    if method == "rqmg":
        solver, M = MGCMTSolver(), identity_operator(g, dimension)
        rho = 0.0
        for _ in range(cycles):
            x0, rho = solver.vcycle_rqmg(x0, op, M, nu1=nu, nu2=nu, nmin=lowest)
            if history is not None:
                history.append(rho)
        return rho, x0
    if method != "vcycle":
        raise ValueError("method must be 'rqmg' or 'vcycle'")
    kind, omega = (_lib.GS_MC, 1.0) if smoother == "rb" else (_lib.WJACOBI, 2. / 3.)
    V, F, W = _lib.SLOT_V, _lib.SLOT_F, _lib.SLOT_W
    # the iterate alternates between the two columns of slot W (x + delta w is written beside x); the V-cycle runs on
    # column 0 with shift 0: right-hand side (F, 0) = the gradient, result (V, 0) = the search direction
    X, XALT, PW, G = (W, 1), (W, 0), (V, 0), (F, 0)
    plan = get_plan(op, int(lowest), nvec=2, mass=identity_operator(g, "3d") if three else None)
    plan.set_shifts([0.0, 0.0])
    plan.upload(0, X[0], X[1], x0)
    plan.scale(0, 1.0 / np.sqrt(plan.dot(0, X, X)), X)
    plan.rq_line_step(0, X, None, None, G)                                            # rho and g = 2 (H x - rho x) of the start vector
    import time
    loop_start = time.perf_counter()
    for it in range(cycles):
        if it and it % _lib.RQ_HISTORY == 0 and history is not None:
            history.extend(plan.rq_history(0, _lib.RQ_HISTORY))
        plan.vcycle(nu, nu, kind, omega=omega, nu_coarse=nu, zero_start=True)        # w = B g  (V is not read: a flag)
        plan.rq_line_step(0, X, PW, XALT, G, record=it % _lib.RQ_HISTORY)             # x <- x + delta w, g <- its gradient
        X, XALT = XALT, X
        if it % 64 == 63:
            # the iterate is never normalised inside the step (nothing in the 2x2 problem depends on its length); keep it
            # of order one over long runs: x and its gradient scale together
            scale = 1.0 / np.sqrt(plan.dot(0, X, X))
            plan.scale(0, scale, X)
            plan.scale(0, scale, G)
    SCRATCH = XALT
    if history is not None and cycles > 0:
        history.extend(plan.rq_history(0, (cycles - 1) % _lib.RQ_HISTORY + 1))
    else:
        plan.sync()
    if stats is not None:
        stats["loop_seconds"] = time.perf_counter() - loop_start
    if cycles > 0:
        # what is returned is MEASURED on the returned vector — <x, H x>/<x, x> — not the running value of the 2x2 problems
        # (which the history holds; the two agree to the accuracy fp64 gives this quotient: eps * |H| / rho, 1e-10 at 8192^2)
        plan.apply(0, X, SCRATCH)
        gram = plan.gram(0, [X, SCRATCH])
        rho = float(gram[0, 1] / gram[0, 0])
        plan.scale(0, 1.0 / np.sqrt(gram[0, 0]), X)                                    # returned with unit length
    else:
        plan.apply(0, X, SCRATCH)
        rho = plan.dot(0, X, SCRATCH)
    return rho, plan.download(0, X[0], X[1])


BLOCK_EIGENSOLVE_MAX = 16   # states of block_eigensolve: S = [X, W, P] is then the 48 vectors of mgcmt_block_pencil


def block_eigensolve(op, k=4, cycles=12, nu=2, lowest=8, smoother="rb", seed=0, guesses=None, history=None, residuals=None,
                     use_p=True, stats=None, mass=None):
    """SURVEY par. 8(f)4: the k lowest eigenpairs of a structured 2-D or 3-D operator — of the pencil (A, M) with ``mass`` — by
    BLOCKED Rayleigh-Ritz with a V-cycle preconditioner: the reference's Rayleigh-quotient routines (rqmin's 2 x 2 problem
    over span{x, p} with its generalised form R y = lambda RM y, MGCMTSolver.py:33-50; the dead vcycle_rqmg2, :59-94, which
    carries M alongside A, :78-79) carried to a block of k vectors with LOBPCG-style updates.  Not in the reference: parity
    unpinned; checked against exact eigenvalues and scipy's eigsh.

    Per iteration, all vectors resident in HBM:  R = A X - M X diag(rho);  W = one V(nu, nu) cycle of A per column of R
    from a zero start (k columns batched);  A W, M W;  Rayleigh-Ritz over S = [X, W, P] (P: the previous update directions;
    use_p=False gives blocked preconditioned steepest descent): the 3k x 3k pencil (S^T A S, S^T M S) from one-pass block
    Gram products, its k lowest pairs on the host, then X, P and their images under A and M updated by tall-skinny
    products.  The host sees Gram matrices only.  1 <= k <= 16: up to four states take the 12 x 4 block kernels
    (mgcmt_block_gram / mgcmt_block_combine, several Gram products per pencil); more take the wide ones — the whole pencil of
    S from ONE mgcmt_block_pencil call (matrix cores), the updates through mgcmt_block_combine_wide, the residual norms from
    one call as well.  ``mass``: a StructuredOperator (None: the identity — nothing of
    M is then stored or applied).

    Returns (eigenvalues, eigenvectors[n, k]) with X^T M X = I; ``history`` receives the Ritz values after every iteration,
    ``residuals`` the norms ||A x_j - rho_j M x_j||."""
    from . import _lib
    from ._lib import OP_M
    from .plan import get_plan
    k = int(k)
    if not 1 <= k <= BLOCK_EIGENSOLVE_MAX:
        raise ValueError("block_eigensolve handles 1..%d eigenpairs at a time" % BLOCK_EIGENSOLVE_MAX)
    wide = k > 4
    kind, omega = (_lib.GS_MC, 1.0) if smoother == "rb" else (_lib.WJACOBI, 2. / 3.)
    V, F, W = _lib.SLOT_V, _lib.SLOT_F, _lib.SLOT_W
    gen = mass is not None
    plan = get_plan(op, int(lowest), nvec=(5 if gen else 3) * k, mass=mass)
    plan.set_shifts(np.zeros(min(plan.nvec, _lib.MAX_VEC)))   # (a plan stores up to 5 k vectors; an entry batches at most MAX_VEC columns)
    n = plan.size(0)
    # what must survive a cycle lives in slot W and in the columns of slot F the cycle does not use (a cycle may exchange
    # the storage of slots V and T, and uses T as its scratch)
    X = [(W, j) for j in range(k)]
    AX = [(W, k + j) for j in range(k)]
    P = [(W, 2 * k + j) for j in range(k)]
    R = [(F, j) for j in range(k)]           # the cycle's right-hand side
    AP = [(F, k + j) for j in range(k)]
    AW = [(F, 2 * k + j) for j in range(k)]
    Wd = [(V, j) for j in range(k)]          # the cycle's output
    # images under M (M = I: the vectors themselves)
    MX = [(W, 3 * k + j) for j in range(k)] if gen else X
    MP = [(W, 4 * k + j) for j in range(k)] if gen else P
    MW = [(F, 3 * k + j) for j in range(k)] if gen else Wd
    rng = np.random.RandomState(seed)
    for j in range(k):
        plan.upload(0, W, j, rng.random_sample(n) if guesses is None else np.asarray(guesses)[:, j])

    def ritz(S, AS, MS, take):
        """k lowest Ritz pairs of the pencil (S^T A S, S^T M S): one wide pencil call, or (k <= 4) Gram products of at most
        four columns each"""
        m = len(S)
        if wide:
            H, G = plan.block_pencil(0, S, AS, MS if gen else None)
        else:
            G, H = np.zeros((m, m)), np.zeros((m, m))
            for c in range(0, m, 4):
                G[:, c:c + 4] = plan.block_gram(0, S, MS[c:c + 4])
                H[:, c:c + 4] = plan.block_gram(0, S, AS[c:c + 4])
        G, H = 0.5 * (G + G.T), 0.5 * (H + H.T)
        d = 1.0 / np.sqrt(np.diag(G))                   # (scaling only: the pencil's eigenvectors are rescaled back)
        evals, evecs = scipy.linalg.eigh(H * np.outer(d, d), G * np.outer(d, d), subset_by_index=[0, take - 1])
        return evals, evecs * d[:, None]

    combine = plan.block_combine_wide if wide else plan.block_combine
    import time
    for j in range(k):
        plan.apply(0, X[j], AX[j])
        if gen:
            plan.apply(0, X[j], MX[j], op=OP_M)
    rho, C = ritz(X, AX, MX, k)
    combine(0, X, X, C)
    combine(0, AX, AX, C)
    if gen:
        combine(0, MX, MX, C)
    have_p = False
    loop_start = time.perf_counter()
    for _ in range(int(cycles)):
        for j in range(k):
            plan.lincomb(0, [(1.0, AX[j]), (-float(rho[j]), MX[j])], R[j])
        if residuals is not None:
            residuals.append(np.sqrt(np.diag(plan.block_pencil(0, R, R)[0] if wide else plan.block_gram(0, R, R))))
        plan.vcycle(nu, nu, kind, omega=omega, k=k, nu_coarse=nu, zero_start=True)
        for j in range(k):
            plan.apply(0, Wd[j], AW[j])
            if gen:
                plan.apply(0, Wd[j], MW[j], op=OP_M)
        if have_p:
            S, AS, MS = X + Wd + P, AX + AW + AP, MX + MW + MP
        else:
            S, AS, MS = X + Wd, AX + AW, MX + MW
        try:
            rho, C = ritz(S, AS, MS, k)
        except (scipy.linalg.LinAlgError, ValueError):   # the directions have become dependent: restart without P
            S, AS, MS = X + Wd, AX + AW, MX + MW
            rho, C = ritz(S, AS, MS, k)
        # P' = [W, P] C_wp, X' = X C_x + P'  (and the same for their images under A and M): P is overwritten first, X uses the new P
        combine(0, S[k:], P, C[k:])
        combine(0, AS[k:], AP, C[k:])
        combine(0, X + P, X, np.vstack([C[:k], np.eye(k)]))
        combine(0, AX + AP, AX, np.vstack([C[:k], np.eye(k)]))
        if gen:
            combine(0, MS[k:], MP, C[k:])
            combine(0, MX + MP, MX, np.vstack([C[:k], np.eye(k)]))
        have_p = bool(use_p)
        if history is not None:
            history.append(np.array(rho))
    plan.sync()
    if stats is not None:
        stats["loop_seconds"] = time.perf_counter() - loop_start
    vecs = np.stack([np.asarray(plan.download(0, W, j)) for j in range(k)], axis=1)
    return np.array(rho), vecs


DEFLATED_EIGENSOLVE_MAX = 64   # states of deflated_eigensolve: the vectors Q of mgcmt_block_deflate
BLOCK_PENCIL_MAX = 48          # MGCMT_BLOCK_WIDE_MAX: vectors of one mgcmt_block_pencil
# deflated_eigensolve(basis="orthonormal"): a column of W or P whose pivot in the Cholesky factorisation of the unit-diagonal
# Gram matrix is at most this leaves the basis (mgcmt_block_orthonormalize).  DESIGN.md par. 4.22 derives the value.
ORTHONORMAL_DROP_TOL = 1e-12


def deflated_eigensolve(op, k, *, rtol=1e-8, atol=0.0, block=None, maxiter=200, nu=2, lowest=8, smoother="rb", seed=0,
                        guesses=None, info=None, mass=None, basis="scaled"):
    """The k lowest eigenpairs of a structured 2-D or 3-D operator, 1 <= k <= 64, solved TO A TOLERANCE: block_eigensolve's
    iteration (LOBPCG with a V-cycle preconditioner) with hard locking.  A Ritz pair whose residual meets the tolerance —
    ||A x - rho x|| <= max(atol, rtol |rho|) — is locked: it leaves the active block for a store of its own, a fresh random
    vector takes its place, and every preconditioned residual is projected against all locked vectors (one
    mgcmt_block_deflate call per iteration, after the cycle and before A is applied) ahead of Rayleigh-Ritz.  Only a
    contiguous prefix of converged pairs is locked, lowest first, and never more than are still wanted.

    The active block holds kb = ``block`` vectors (default min(16, k + 4)) from the first iteration to the last, so the last
    wanted states have guard vectors behind them; it always goes through the wide entries (mgcmt_block_pencil,
    mgcmt_block_combine_wide).  On a lock P is dropped for the next iteration, the fresh vectors — drawn in order from
    np.random.RandomState(seed), uploaded, deflated once, A applied — go to the freed places and Rayleigh-Ritz runs over X
    again.  A fresh vector is a host upload of n doubles: a run of k states uploads about k + kb of them.

    Memory: ONE plan with nvec = 3 kb + ceil(k / 2) <= 80 vectors per slot, the active ones where block_eigensolve keeps them
    (X, AX, P in slot W; R, AP, AW in slot F; the cycle's output in V), the locked ones in the columns from 3 kb on of slots
    W and F only (a cycle exchanges the V / T storage of a level: nothing that must survive lives there).  All four slots
    have nvec columns on every level: 4 x nvec x 8 B x n x 4/3 in 2-D (x 8/7 in 3-D) — 80 columns at 2048^2 are 14.3 GB.

    ``mass`` is refused (the projection would need M Q next to Q); ``smoother``: "rb" or "wjacobi".  Returns
    (eigenvalues[k] ascending, eigenvectors[n, k]).  ``info`` (a dict) receives iterations, status ("converged" or
    "maxiter"), locked_at (the iteration at which each state was locked; -1: not locked), residuals (the final norm per
    state) and column_cycles (active columns summed over the iterations).  With status "maxiter" the states that were not
    locked are returned as they stand — as many as the active block holds: min(k, locked + kb) columns in all.

    ``basis``: how the trial basis [X, W, P] of Rayleigh-Ritz is conditioned.  "scaled" (the default): the vectors as they
    come, the pencil scaled to a unit diagonal.  "orthonormal" (DESIGN.md par. 4.22): in every iteration the cycle's output W is
    projected against the locked vectors and against X and made orthonormal by a Cholesky-QR step, twice
    (mgcmt_block_deflate, mgcmt_block_orthonormalize), A is applied, and P and AP are projected against [X, W] and made
    orthonormal together, twice (mgcmt_block_project, mgcmt_block_orthonormalize with companions); X = S C with C^T G C = I
    stays orthonormal, fresh vectors are also deflated against the X that remain.  The Gram matrix of the Ritz problem is then
    the identity to rounding.  A column whose pivot falls to ORTHONORMAL_DROP_TOL or below comes back as zeros and leaves the
    Ritz problem of that iteration.  ``info`` then also receives gram_min (the smallest eigenvalue of the scaled Gram matrix
    of each main-loop Ritz problem) and dropped (columns dropped, per iteration).

    Known limit of basis="scaled" (DESIGN.md par. 4.21): 40 states of the 1024^2 and 2048^2 boxes stall on the MI355X once 28
    are locked — the Gram matrix of the scaled [X, W, P] loses rank to working accuracy (smallest eigenvalue 1e-12 and below),
    the Ritz vectors then carry errors of 1e-4 and no residual reaches 1e-8 |rho| again; status is "maxiter".  24 states
    converge there (34 iterations at 1024^2, 36 at 2048^2), 40 states converge at 64^2 and 64 at 32^2.  With
    basis="orthonormal" the 40 states of the 1024^2 box converge on the MI355X in 65 iterations (lowest = 4, gram_min >=
    1 - 1e-14); 40 states at 2048^2 with lowest = 8 still ended at "maxiter" with it (DESIGN.md par. 4.22: open).
    Check ``info["status"]``."""
    from .plan import get_plan
    k = int(k)
    if not 1 <= k <= DEFLATED_EIGENSOLVE_MAX:
        raise ValueError("deflated_eigensolve handles 1..%d eigenpairs" % DEFLATED_EIGENSOLVE_MAX)
    kb = min(BLOCK_EIGENSOLVE_MAX, k + 4) if block is None else int(block)
    if not 1 <= kb <= BLOCK_EIGENSOLVE_MAX:
        raise ValueError("deflated_eigensolve: an active block of 1..%d vectors" % BLOCK_EIGENSOLVE_MAX)
    if mass is not None:
        raise ValueError("deflated_eigensolve does not take a mass operator (the locked store would have to keep M Q next to Q)")
    if smoother not in ("rb", "wjacobi"):
        raise ValueError("deflated_eigensolve: smoother is 'rb' or 'wjacobi'")
    if basis not in ("scaled", "orthonormal"):
        raise ValueError("deflated_eigensolve: basis is 'scaled' or 'orthonormal'")
    plan = get_plan(op, int(lowest), nvec=3 * kb + (k + 1) // 2)
    n = plan.size(0)
    rng = np.random.RandomState(seed)
    given = 0 if guesses is None else min(kb, np.asarray(guesses).shape[1])

    def place(j, location):
        """the j-th vector the iteration asks for: a column of the guesses for the first of the start block, else the next draw"""
        plan.upload(0, location[0], location[1], np.asarray(guesses)[:, j] if j < given else rng.random_sample(n))

    vals, where = _deflated_eigensolve_on(plan, k, kb, place, rtol=rtol, atol=atol, maxiter=maxiter, nu=nu, smoother=smoother, basis=basis,
                                          info=info)
    vecs = np.stack([np.asarray(plan.download(0, *v)) for v in where], axis=1)
    return vals, vecs


def _deflated_eigensolve_on(plan, k, kb, place, *, rtol, atol, maxiter, nu, smoother, basis, info):
    """The iteration of deflated_eigensolve on a plan it is given (at least 3 kb + ceil(k / 2) vectors per slot; columns beyond
    those are not touched, nor is anything of slots W and F on levels below 0).  Every start vector and every fresh vector
    comes through ``place(j, (slot, vec))``, j counting the requests from 0: the first kb are the start block X, in order,
    the rest the fresh vectors after locks; it leaves the vector at that location of level 0, stream-ordered.  Nothing is
    downloaded: returns (eigenvalues ascending, the (slot, vec) locations of their vectors in that order) — as many as
    deflated_eigensolve returns.  The arguments have been checked."""
    from . import _lib
    orthonormal = basis == "orthonormal"
    kind, omega = (_lib.GS_MC, 1.0) if smoother == "rb" else (_lib.WJACOBI, 2. / 3.)
    V, F, W = _lib.SLOT_V, _lib.SLOT_F, _lib.SLOT_W
    plan.set_shifts(np.zeros(min(plan.nvec, _lib.MAX_VEC)))
    X = [(W, j) for j in range(kb)]
    AX = [(W, kb + j) for j in range(kb)]
    P = [(W, 2 * kb + j) for j in range(kb)]
    R = [(F, j) for j in range(kb)]
    AP = [(F, kb + j) for j in range(kb)]
    AW = [(F, 2 * kb + j) for j in range(kb)]
    Wd = [(V, j) for j in range(kb)]
    Q = [((W, F)[i % 2], 3 * kb + i // 2) for i in range(k)]          # the locked store
    placed = 0
    for j in range(kb):
        place(placed, X[j])
        placed += 1
        plan.apply(0, X[j], AX[j])

    def ritz(S, AS):
        """the kb lowest Ritz pairs over span S, orthogonal to the locked vectors by construction of S"""
        H, G = plan.block_pencil(0, S, AS)
        G, H = 0.5 * (G + G.T), 0.5 * (H + H.T)
        d = 1.0 / np.sqrt(np.diag(G))                   # (scaling only: the pencil's eigenvectors are rescaled back)
        evals, evecs = scipy.linalg.eigh(H * np.outer(d, d), G * np.outer(d, d), subset_by_index=[0, kb - 1])
        return evals, evecs * d[:, None]

    gram_min, dropped = [], []

    def ritz_orthonormal(S, AS):
        """ritz over a basis whose W and P parts mgcmt_block_orthonormalize made: a column it dropped is exact zeros and shows
        as an exact zero on the diagonal of G — it leaves the Ritz problem and gets a zero coefficient row.  Records the
        smallest eigenvalue of the scaled G and the number of dropped columns."""
        H, G = plan.block_pencil(0, S, AS)
        G, H = 0.5 * (G + G.T), 0.5 * (H + H.T)
        keep = np.flatnonzero(np.diag(G) != 0.0)
        H, G = H[np.ix_(keep, keep)], G[np.ix_(keep, keep)]
        d = 1.0 / np.sqrt(np.diag(G))
        Gs = G * np.outer(d, d)
        gram_min.append(float(np.linalg.eigvalsh(Gs)[0]))
        dropped.append(len(S) - len(keep))
        evals, evecs = scipy.linalg.eigh(H * np.outer(d, d), Gs, subset_by_index=[0, kb - 1])
        C = np.zeros((len(S), kb))
        C[keep] = evecs * d[:, None]
        return evals, C

    def ritz_over_x():
        rho, C = ritz(X, AX)
        plan.block_combine_wide(0, X, X, C)
        plan.block_combine_wide(0, AX, AX, C)
        return rho

    vals, norms_locked, locked_at = [], [], []
    iterations = column_cycles = 0

    def residuals_and_locks(rho):
        """R = A X - X diag(rho) and its norms; locks the converged prefix, refills the block and repeats while pairs lock.
        Returns (rho, norms, whether anything was locked)."""
        nonlocal placed
        locked_any = False
        while True:
            for j in range(kb):
                plan.lincomb(0, [(1.0, AX[j]), (-float(rho[j]), X[j])], R[j])
            norms = np.sqrt(np.diag(plan.block_pencil(0, R, R)[0]))
            ok = norms <= np.maximum(atol, rtol * np.abs(rho))
            nlock = min(kb if ok.all() else int(np.argmin(ok)), k - len(vals))
            if nlock == 0:
                return rho, norms, locked_any
            for j in range(nlock):
                plan.copy(0, X[j][0], X[j][1], *Q[len(vals)])
                vals.append(float(rho[j]))
                norms_locked.append(float(norms[j]))
                locked_at.append(iterations)
            locked_any = True
            if len(vals) == k:
                return rho[nlock:], norms[nlock:], True
            for j in range(nlock):
                place(placed, X[j])
                placed += 1
            plan.block_deflate(0, Q[:len(vals)], X[:nlock])
            if orthonormal and nlock < kb:              # ... and against the X that remain (orthonormal, and orthogonal to Q)
                plan.block_deflate(0, X[nlock:], X[:nlock])
            for j in range(nlock):
                plan.apply(0, X[j], AX[j])
            rho = ritz_over_x()

    main_ritz = ritz_orthonormal if orthonormal else ritz
    rho, norms, _ = residuals_and_locks(ritz_over_x())
    have_p = False
    while len(vals) < k and iterations < int(maxiter):
        iterations += 1
        column_cycles += kb
        plan.vcycle(nu, nu, kind, omega=omega, k=kb, nu_coarse=nu, zero_start=True)
        if orthonormal:
            # [X, Wd, P] with orthonormal columns: Wd against Q and X, P against X and Wd, each projection and Cholesky-QR step
            # twice (the second one works on vectors the first left with a condition number near one)
            for _ in range(2):
                if vals:
                    plan.block_deflate(0, Q[:len(vals)], Wd)
                plan.block_deflate(0, X, Wd)
                plan.block_orthonormalize(0, Wd, drop_tol=ORTHONORMAL_DROP_TOL)
            for j in range(kb):                          # (A of a dropped column, exact zeros, is exact zeros)
                plan.apply(0, Wd[j], AW[j])
            for _ in range(2 if have_p else 0):
                plan.block_project(0, X + Wd, P, AX + AW, AP)
                plan.block_orthonormalize(0, P, AP, drop_tol=ORTHONORMAL_DROP_TOL)
        else:
            if vals:
                plan.block_deflate(0, Q[:len(vals)], Wd)
            for j in range(kb):
                plan.apply(0, Wd[j], AW[j])
        S, AS = (X + Wd + P, AX + AW + AP) if have_p else (X + Wd, AX + AW)
        try:
            rho, C = main_ritz(S, AS)
        except (scipy.linalg.LinAlgError, ValueError):   # the directions have become dependent: restart without P
            S, AS = X + Wd, AX + AW
            del gram_min[iterations - 1:], dropped[iterations - 1:]
            rho, C = main_ritz(S, AS)
        # P' = [W, P] C_wp, X' = X C_x + P' (and their images under A), as block_eigensolve
        plan.block_combine_wide(0, S[kb:], P, C[kb:])
        plan.block_combine_wide(0, AS[kb:], AP, C[kb:])
        plan.block_combine_wide(0, X + P, X, np.vstack([C[:kb], np.eye(kb)]))
        plan.block_combine_wide(0, AX + AP, AX, np.vstack([C[:kb], np.eye(kb)]))
        rho, norms, locked_any = residuals_and_locks(rho)
        have_p = not locked_any
    plan.sync()
    nlocked = len(vals)
    rest = min(k - nlocked, kb)                          # (status "maxiter": the lowest active pairs as they stand)
    where = Q[:nlocked] + X[:rest]
    vals = np.array(vals + [float(r) for r in rho[:rest]])
    norms = np.array(norms_locked + [float(r) for r in norms[:rest]])
    locked_at = np.array(locked_at + [-1] * rest, dtype=np.int64)
    order = np.argsort(vals, kind="stable")
    if info is not None:
        info.update(iterations=iterations, status="converged" if nlocked == k else "maxiter", locked_at=locked_at[order],
                    residuals=norms[order], column_cycles=column_cycles)
        if orthonormal:
            info.update(gram_min=np.array(gram_min), dropped=np.array(dropped, dtype=np.int64))
    return vals[order], [where[j] for j in order]


ANDERSON_RCOND = 1e-12


def anderson_coefficients(G):
    """The coefficients alpha (sum alpha = 1) that minimise ||sum_i alpha_i r_i||_2 from the p x p Gram matrix G_ij = <r_i, r_j>
    of the residuals, newest last — Anderson (type II, Pulay) mixing in the difference form: with D the (p - 1) x p
    forward-difference matrix, (D G D^T) gamma = D G e_last, scaled symmetrically to a unit diagonal and solved by
    numpy.linalg.lstsq with rcond = 1e-12; alpha = e_last - D^T gamma.  None where the history has to be restarted: a
    diagonal entry of D G D^T that is not positive, or a scaled system (or a solution) that is not finite.  Host arithmetic
    on at most 81 numbers."""
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
    alpha = -(D.T @ (s * np.linalg.lstsq(As, bs, rcond=ANDERSON_RCOND)[0]))
    alpha[-1] += 1.0
    return alpha if np.all(np.isfinite(alpha)) else None


def schroedinger_poisson(op, poisson_op, k, occupations, *, coupling, mixing=1.0, mixing_history=0, tol=1e-6, maxiter=50, eigen_rtol=1e-9,
                         poisson_rtol=1e-10, warm_start=True, block=None, lowest=8, poisson_lowest=None, smoother="rb", basis="scaled",
                         seed=0, info=None):
    """The self-consistent Schroedinger-Poisson loop on the device: the k lowest states of H[phi] = op + coupling diag(phi),
    their density rho = sum_j f_j psi_j^2, poisson_op phi = rho, and again until phi stands still.

    ``op``: a 2-D or 3-D operator with a per-point part (potential_operator, variable_mass_operator, tensor_mass_operator); its
    diagonal (the centre plane of a stencil) is the external potential.  ``poisson_op``: an operator MGCMTSolver.solve takes, on
    the same grid — e.g. variable_mass_operator(g, eps) for -div(eps grad), or a sparse matrix that solve recognises (it goes
    through the same recognition, with op's dimension).  ``occupations``: k weights f_j, or a callable
    eigenvalues -> k weights (Fermi filling is host arithmetic on k numbers).  Units live in ``coupling`` and ``poisson_op``.

    One step: deflated_eigensolve's iteration to ``eigen_rtol`` on ONE private plan (the same block, locking, ``smoother`` and
    ``basis``); rho in one pass over the states, each weighted f_j / <psi_j, psi_j> (mgcmt_block_density); a device copy to the
    right-hand side of a second private plan (mgcmt_copy_across); conjugate gradients with the V-cycle preconditioner to
    ``poisson_rtol`` there (from a zero start in the first step, from the last solution afterwards);
    d = ||phi_new - phi||_2 / ||phi_new||_2 (phi = 0 before the first step, so the first d is 1); phi <- (1 - mixing) phi +
    mixing phi_new; a device copy back; the new diagonal V_ext + coupling phi and the per-point planes of every coarser level
    (mgcmt_plan_set_point_diagonal).  The loop ends with the step whose d <= tol, or after ``maxiter`` steps.  With
    coupling == 0 the operator does not depend on phi: the states of the first step stand and no later step solves for them again.
    The host sees eigenvalues, residual norms, the Ritz matrices, the status words of the solves and d: no grid vector crosses
    to the host between the upload of V_ext and the downloads at the end (with warm_start=False every step uploads its random
    start vectors, as deflated_eigensolve does).

    ``mixing_history`` = m, 1 <= m <= 8: Anderson (type II, Pulay) mixing of the potential with m history vectors beyond the
    newest (DESIGN.md par. 4.24).  With x_i the input potential of step i, g_i its Poisson solution and r_i = g_i - x_i, the
    last p = min(m + 1, steps since the last restart) pairs (x_i, r_i) stay on the device in a ring of columns of the Poisson
    plan; one pass writes r_i and returns its inner products with the earlier residuals, <r_i, r_i> and <g_i, g_i>
    (mgcmt_mix_residual: d from the same pass), the host finds the alpha of anderson_coefficients from the p x p Gram matrix,
    and one pass writes x_(i+1) = sum alpha_i (x_i + mixing r_i) (mgcmt_mix_combine).  With one pair this is the damped step;
    a Gram matrix that cannot be used restarts the history with the newest pair.  Only scalars reach the host.  m = 0 (the
    default) is the plain damped iteration, launch for launch what it was before the option existed.

    ``warm_start``: the k states of a step are copied to a pool in the plan's own columns and handed to the next step's
    iteration in order — the first kb as its start block, the others as the fresh vectors after locks —, random vectors only
    behind them.

    Memory: the eigen-plan holds 3 kb + ceil(k / 2) columns per slot for the iteration (deflated_eigensolve), ceil(k / 2) more
    in each of slots W and F for the pool and two for V_ext and rho / phi (slot W; a cycle exchanges the storage of V and T) —
    at most MGCMT_MAX_STORE_VEC = 80, so k <= 30 with the default block.  The Poisson plan holds 6, and 2 (m + 1) more for
    the ring of Anderson mixing.

    Returns (eigenvalues[k], eigenvectors[n, k], phi[n]): the states are those of the last step's operator, phi the mixed
    potential after it.  ``info`` (a dict) receives iterations, status ("converged" / "maxiter"), changes (every d),
    eigen_iterations, eigen_status, poisson_iterations and poisson_status per step, density (rho of the last step, n
    numbers), mixing_history, mixing_depths (the p of every step; all 1 with mixing_history = 0) and mixing_restarts (the steps,
    counted from 1, at which the history was reset).  A Poisson solve that does not reach ``poisson_rtol`` within 200 iterations, breaks down or meets an indefinite
    operator raises RuntimeError: the loop does not go on with a potential that is not one.
    Refused with ValueError: what deflated_eigensolve refuses, an ``op`` without a per-point part, operators on different
    grids, occupations that are not k numbers, a mixing outside (0, 1], a mixing_history that is not an integer in 0..8, more
    columns than a plan stores."""
    from . import _lib
    from .operators import StructuredOperator
    from .plan import Plan
    k = int(k)
    if not 1 <= k <= DEFLATED_EIGENSOLVE_MAX:
        raise ValueError("schroedinger_poisson handles 1..%d states" % DEFLATED_EIGENSOLVE_MAX)
    kb = min(BLOCK_EIGENSOLVE_MAX, k + 4) if block is None else int(block)
    if not 1 <= kb <= BLOCK_EIGENSOLVE_MAX:
        raise ValueError("schroedinger_poisson: an active block of 1..%d vectors" % BLOCK_EIGENSOLVE_MAX)
    if smoother not in ("rb", "wjacobi"):
        raise ValueError("schroedinger_poisson: smoother is 'rb' or 'wjacobi'")
    if basis not in ("scaled", "orthonormal"):
        raise ValueError("schroedinger_poisson: basis is 'scaled' or 'orthonormal'")
    part, arrays = op.point_part()
    if part is None or op.dimension not in ("2d", "3d"):
        raise ValueError("schroedinger_poisson: op needs a per-point part (potential_operator, variable_mass_operator, tensor_mass_operator): "
                         "its diagonal is the external potential")
    if not isinstance(poisson_op, StructuredOperator):
        from .solver import _recognise_entry
        poisson_op = _recognise_entry(poisson_op, op.dimension)          # (raises UnrecognisedOperator, a ValueError, as solve does)
    if poisson_op.dimension != op.dimension or poisson_op.g != op.g:
        raise ValueError("schroedinger_poisson: op (%s, g = %d) and poisson_op (%s, g = %d) live on different grids"
                         % (op.dimension, op.g, poisson_op.dimension, poisson_op.g))
    if not 0.0 < float(mixing) <= 1.0:
        raise ValueError("schroedinger_poisson: mixing lies in (0, 1]")
    if isinstance(mixing_history, bool) or not isinstance(mixing_history, (int, np.integer)) or not 0 <= mixing_history <= _lib.MIX_MAX - 1:
        raise ValueError("schroedinger_poisson: mixing_history is an integer in 0..%d" % (_lib.MIX_MAX - 1))
    history = int(mixing_history)
    if not callable(occupations) and np.asarray(occupations, dtype=np.float64).shape != (k,):
        raise ValueError("schroedinger_poisson: occupations are k = %d numbers (or a callable eigenvalues -> k numbers)" % k)
    half = (k + 1) // 2
    nvec = 3 * kb + 2 * half + 2
    if nvec > _lib.MAX_STORE_VEC:
        raise ValueError("schroedinger_poisson: 3 kb + ceil(k / 2) columns for the iteration, ceil(k / 2) for the pool and 2 for V_ext and "
                         "rho / phi are 3 * %d + %d + %d + 2 = %d columns; a plan stores at most %d (k <= 30 with the default block)"
                         % (kb, half, half, nvec, _lib.MAX_STORE_VEC))
    coupling, mixing = float(coupling), float(mixing)
    kind, omega = (_lib.GS_MC, 1.0) if smoother == "rb" else (_lib.WJACOBI, 2. / 3.)
    F, W = _lib.SLOT_F, _lib.SLOT_W
    POOL = [((W, F)[i % 2], 3 * kb + half + i // 2) for i in range(k)]
    VEXT, RHO = (W, nvec - 2), (W, nvec - 1)                     # (RHO holds rho on the way out and phi on the way back)
    PX, PPHI, PDIFF = (W, 0), (W, 4), (W, 5)                      # the Poisson plan: columns 0..3 of W are x, p, q, p2 of the solve
    # Anderson mixing: a ring of history + 1 pairs (x_i, r_i) behind them, step i in place (i - 1) % (history + 1)
    RING_X = [(W, 6 + c) for c in range(history + 1)] if history else []
    RING_R = [(W, 7 + history + c) for c in range(history + 1)] if history else []
    v_ext = arrays[0] if part != "planes" else arrays[0][(1,) * (arrays[0].ndim // 2)]
    rng = np.random.RandomState(seed)
    changes, eig_its, eig_status, poi_its, poi_status = [], [], [], [], []
    depths, restarts, pairs, gram = [], [], [], {}                # (pairs: the ring places in the history, oldest first; gram: <r_a, r_b> by place)
    eplan = pplan = None
    try:
        eplan = Plan(op, int(lowest), nvec=nvec)
        pplan = Plan(poisson_op, int(lowest if poisson_lowest is None else poisson_lowest), nvec=6 + (2 * (history + 1) if history else 0))
        n = eplan.size(0)
        eplan.upload(0, VEXT[0], VEXT[1], v_ext)
        pplan.set_shifts(np.zeros(6))
        pplan.fill(0, PPHI[0], PPHI[1], 0.0)
        if history:
            pplan.fill(0, RING_X[0][0], RING_X[0][1], 0.0)
        pooled = 0

        def place(j, location):
            if warm_start and j < pooled:
                eplan.copy(0, POOL[j][0], POOL[j][1], location[0], location[1])
            else:
                eplan.upload(0, location[0], location[1], rng.random_sample(n))

        vals = where = None
        status = "maxiter"
        for step in range(1, int(maxiter) + 1):
            if where is None or coupling != 0.0:
                einfo = {}
                vals, where = _deflated_eigensolve_on(eplan, k, kb, place, rtol=eigen_rtol, atol=0.0, maxiter=200, nu=2, smoother=smoother,
                                                      basis=basis, info=einfo)
                eig_its.append(int(einfo["iterations"]))
                eig_status.append(einfo["status"])
                if warm_start:
                    pooled = len(where)
                    for j, v in enumerate(where):
                        eplan.copy(0, v[0], v[1], POOL[j][0], POOL[j][1])
            else:
                eig_its.append(0)
                eig_status.append(eig_status[-1])
            f = np.asarray(occupations(vals) if callable(occupations) else occupations, dtype=np.float64).reshape(-1)[:len(where)]
            norm2 = np.concatenate([np.diag(eplan.block_pencil(0, where[i:i + BLOCK_PENCIL_MAX], where[i:i + BLOCK_PENCIL_MAX])[0])
                                    for i in range(0, len(where), BLOCK_PENCIL_MAX)])      # (a pencil takes at most 48 vectors)
            eplan.block_density(0, where, f / norm2, RHO)
            eplan.copy_across(0, RHO, pplan, (F, 0))
            pplan.pcg_begin([0, 1, 2, 3], float(poisson_rtol), zero_start=step == 1, flexible=kind != _lib.WJACOBI)
            queued, state = 0, _lib.PCG_RUNNING
            while state == _lib.PCG_RUNNING and queued < 200:
                pplan.pcg_iterate(4, 2, 2, kind, omega=omega, nu_coarse=4)
                queued += 4
                done, state, indefinite = pplan.pcg_status()[:3]
            poi_its.append(int(done))
            poi_status.append({_lib.PCG_CONVERGED: "converged", _lib.PCG_BREAKDOWN: "breakdown"}.get(int(state), "maxiter"))
            if poi_status[-1] != "converged" or indefinite:
                raise RuntimeError("schroedinger_poisson: the Poisson solve of step %d ended with status %r%s after %d iterations "
                                   "(poisson_op must be positive definite)" % (step, poi_status[-1], ", indefinite" if indefinite else "", done))
            if history:
                # r = g - x into the ring and its row of the Gram matrix in one pass; alpha on the host; the next x in one pass,
                # into the next place of the ring: a free one, or the oldest pair's, which leaves the history with the next step
                here, nxt = (step - 1) % (history + 1), step % (history + 1)
                if here in pairs:
                    pairs.remove(here)                            # (the oldest pair: the last step wrote this step's x over its x)
                sums = pplan.mix_residual(0, PX, RING_X[here], RING_R[here], [RING_R[c] for c in pairs])
                for c, v in zip(pairs, sums):
                    gram[(c, here)] = gram[(here, c)] = float(v)
                gram[(here, here)] = float(sums[-2])
                d = math.sqrt(sums[-2] / sums[-1])
                changes.append(d)
                pairs.append(here)
                alpha = anderson_coefficients([[gram[(a, b)] for b in pairs] for a in pairs])
                if alpha is None:
                    restarts.append(step)
                    del pairs[:-1]
                    alpha = np.ones(1)
                depths.append(len(pairs))
                pplan.mix_combine(0, [RING_X[c] for c in pairs], [RING_R[c] for c in pairs], alpha, mixing, RING_X[nxt])
                PPHI = RING_X[nxt]
            else:
                pplan.lincomb(0, [(1.0, PX), (-1.0, PPHI)], PDIFF)
                d = math.sqrt(pplan.dot(0, PDIFF, PDIFF) / pplan.dot(0, PX, PX))
                changes.append(d)
                depths.append(1)
                pplan.lincomb(0, [(1.0 - mixing, PPHI), (mixing, PX)], PPHI)
            if coupling != 0.0:
                pplan.copy_across(0, PPHI, eplan, RHO)
                eplan.set_point_diagonal([(1.0, VEXT), (coupling, RHO)])
            if d <= tol:
                status = "converged"
                break
        if info is not None:
            info.update(iterations=len(changes), status=status, changes=changes, eigen_iterations=eig_its, eigen_status=eig_status,
                        poisson_iterations=poi_its, poisson_status=poi_status, mixing_history=history, mixing_depths=depths,
                        mixing_restarts=restarts)
            if coupling != 0.0:                                   # (RHO holds phi by now: the density once more)
                eplan.block_density(0, where, f / norm2, RHO)
            info["density"] = np.array(eplan.download(0, *RHO))
        vecs = np.stack([np.asarray(eplan.download(0, *v)) for v in where], axis=1)
        phi = np.array(pplan.download(0, *PPHI))
        return vals, vecs, phi
    finally:
        for p in (eplan, pplan):
            if p is not None:
                p.close()
