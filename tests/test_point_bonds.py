"""Variable effective mass: 2-D operators with per-point bond coefficients (operators.variable_mass_operator /
recognise_five_point, StructuredOperator(point_bonds=...), mgcmt_plan_create_bonds) against the NumPy oracle
(oracle.sparse_ref.RefSolver, which cycles any sparse matrix) and against scipy's own R*A*P, through the HIP library on the
GPU box and through the emulated kernels on CPU (``backend`` fixture).

Level 0 of such a plan runs kernels of its own (DESIGN par. 4.15): from 128 columns on the marching kernels of
csrc/kernels_bonds.hip (by default the red-black stages and residual + restriction, with MGCMT_BONDS_MARCH=1 every pass),
otherwise and with MGCMT_BONDS_MARCH=0 the flat ones of csrc/kernels_pointwise.hip; the variable 9-point levels below it are
those of a plan with a point diagonal."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import rel_err
from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, _lib, drivers, recognise_five_point, variable_mass_operator
from multigridcmt_amd.operators import (StructuredOperator, UnrecognisedOperator, identity_operator, potential_operator, recognise, recognise_potential,
                                        tri_identity, tri_to_sparse)
from multigridcmt_amd.plan import Plan, get_plan
from oracle.sparse_ref import RefSolver, RefStencilMaker
from test_point_potential import galerkin_chain, smooth_v

TOL = 1e-10          # the bar of tests/test_point_potential.py
SCALE = -1 / np.pi ** 2


@pytest.fixture(autouse=True, scope="module")
def _release_host_buffers():
    yield
    import gc
    from multigridcmt_amd import hostmem
    gc.collect()
    hostmem.drain()


def _centres(g):
    x = (np.arange(g) + 0.5) / g - 0.5
    return np.meshgrid(x, x, indexing="ij")


def _disc(g):
    X, Y = _centres(g)
    return (X - 0.05) ** 2 + (Y + 0.1) ** 2 < 0.3 ** 2


def w_step(g):
    """inverse mass 4 inside a disc (a light particle in the dot), 1 outside, with 20 % disorder: a jump across an interface"""
    return np.where(_disc(g), 4.0, 1.0) * (1.0 + 0.2 * np.random.RandomState(2).rand(g, g))


def v_step(g):
    """the band offset that goes with it: 0 inside the disc, 30 outside"""
    return np.where(_disc(g), 0.0, 30.0)


def w_smooth(g):
    X, Y = _centres(g)
    return 1.0 + 3.0 * np.exp(-((X - 0.05) ** 2 + (Y + 0.1) ** 2) / 0.15 ** 2)


def step_operator(g):
    return variable_mass_operator(g, w_step(g), v_step(g))


def flat(a):
    return np.asarray(a).reshape(-1)


def rb(ref):
    return lambda v, f, A, nu=4: ref.gseidel_mc(v, f, A, nu=nu, dimension="2d")


def assemble_level(plan, level):
    """the matrix of `level`: Kronecker factors (mgcmt_plan_get_factors) plus the per-point part (mgcmt_plan_get_point_stencil);
    entries towards points outside the grid must be exact zeros"""
    gl = plan.g >> level
    xf, yf = plan.factors(level, 0), plan.factors(level, 1)
    A = sum(sp.kron(tri_to_sparse(xf[m]), tri_to_sparse(yf[m]), format="csr") for m in range(xf.shape[0])).tocsr()
    G = plan.point_stencil(level)
    if level == 0:
        assert G.shape == (3, gl, gl)
        assert not G[1][:, -1].any() and not G[2][-1, :].any()
        n = gl * gl
        e, s = G[1].reshape(-1)[:n - 1], G[2].reshape(-1)[:n - gl]
        return (A + sp.diags([s, e, G[0].reshape(-1), e, s], [-gl, -1, 0, 1, gl], shape=(n, n))).tocsr()
    assert G.shape == (3, 3, gl, gl)
    idx = np.arange(gl)
    I, J = np.meshgrid(idx, idx, indexing="ij")
    B = sp.csr_matrix((gl * gl, gl * gl))
    for a in range(3):
        for b in range(3):
            ii, jj = I + a - 1, J + b - 1
            ok = (ii >= 0) & (ii < gl) & (jj >= 0) & (jj < gl)
            assert not G[a, b][~ok].any()          # nothing points outside the grid
            B = B + sp.csr_matrix((G[a, b][ok], ((I * gl + J)[ok], (ii * gl + jj)[ok])), shape=(gl * gl, gl * gl))
    return (A + B).tocsr()


# ---- the operator objects -------------------------------------------------------------------------------------------------

def test_variable_mass_operator_is_the_laplacian_for_unit_mass():
    for g in (16, 32, 64):
        L = SCALE * MGCMTStencilMaker().laplacian(g, dimension="2d")
        op = variable_mass_operator(g, np.ones((g, g)))
        assert op.point_bonds is None and op.point_diagonal is None          # what laplacian_operator (scaled) returns
        assert abs(op.tocsr() - L).max() == 0.0
        V = smooth_v(g)
        op = variable_mass_operator(g, np.ones((g, g)), V)
        assert op.point_bonds is None and abs(op.tocsr() - potential_operator(g, V).tocsr()).max() == 0.0
        # one point differs: the bond form, still the Laplacian everywhere else, to rounding
        w = np.ones((g, g))
        w[3, 5] = 2.0
        op = variable_mass_operator(g, w)
        assert op.point_bonds is not None
        D = (op.tocsr() - L).tocsr()
        D.data[np.abs(D.data) < 1e-12 * abs(L).max()] = 0.0
        D.eliminate_zeros()
        assert set(np.unique(D.nonzero()[0]) // g) <= {2, 3, 4}


def test_variable_mass_operator_entries():
    """bond = t * mean(w_a, w_b), diagonal = -t * (the four bonds, a ghost's with the point's own w) + V"""
    g = 16
    w, V = w_step(g), v_step(g)
    t = SCALE * g * g
    for mean, m in (("harmonic", lambda a, b: 2 * a * b / (a + b)), ("arithmetic", lambda a, b: 0.5 * (a + b))):
        A = variable_mass_operator(g, w, V, mean=mean).tocsr()
        assert abs(A - A.T).max() == 0.0
        for i, j in ((0, 0), (3, 4), (g - 1, g - 1), (0, g - 1), (7, 0)):
            r = i * g + j
            nb = [m(w[i, j], w[i + di, j + dj]) if 0 <= i + di < g and 0 <= j + dj < g else w[i, j] for di, dj in ((0, 1), (0, -1), (1, 0), (-1, 0))]
            assert abs(A[r, r] - (-t * sum(nb) + V[i, j])) <= 1e-13 * abs(A[r, r])
            if j + 1 < g:
                assert abs(A[r, r + 1] - t * nb[0]) <= 1e-13 * abs(t * nb[0])
            if i + 1 < g:
                assert abs(A[r, r + g] - t * nb[2]) <= 1e-13 * abs(t * nb[2])
    with pytest.raises(ValueError):
        variable_mass_operator(g, w, mean="geometric")
    with pytest.raises(ValueError):
        variable_mass_operator(g, np.ones(g))
    with pytest.raises(ValueError):
        variable_mass_operator(g, w, np.ones(g))


def test_operator_algebra_carries_the_bonds():
    g = 8
    op = step_operator(g)
    A = op.tocsr()
    E, S = op.point_bonds
    assert E.shape == (g, g) and S.shape == (g, g) and op.point_diagonal.shape == (g, g)
    # tocsr against a matrix assembled entry by entry
    kron = StructuredOperator("2d", g, op.terms).tocsr().tolil()
    for i in range(g):
        for j in range(g):
            r = i * g + j
            kron[r, r] += op.point_diagonal[i, j]
            if j + 1 < g:
                kron[r, r + 1] += E[i, j]
                kron[r + 1, r] += E[i, j]
            if i + 1 < g:
                kron[r, r + g] += S[i, j]
                kron[r + g, r] += S[i, j]
    assert abs(A - kron.tocsr()).max() <= 1e-13 * abs(A).max()
    assert np.allclose(op.diagonal(), A.diagonal(), rtol=1e-14)
    assert abs((op * 2.5).tocsr() - 2.5 * A).max() <= 1e-13 * abs(A).max()
    assert abs((2.5 * op).tocsr() - 2.5 * A).max() <= 1e-13 * abs(A).max()
    assert abs((-op / 4.0).tocsr() + A / 4.0).max() <= 1e-13 * abs(A).max()
    assert abs(op.shifted(0.7).tocsr() - (A - 0.7 * sp.identity(g * g))).max() <= 1e-13 * abs(A).max()
    assert (op * 2.0).point_bonds is not None and op.shifted(0.7).point_bonds is not None
    assert op.fingerprint() == step_operator(g).fingerprint()
    E2 = E.copy()
    E2[2, 3] += 1e-9
    assert op.fingerprint() != StructuredOperator("2d", g, op.terms, point_diagonal=op.point_diagonal, point_bonds=(E2, S)).fingerprint()
    assert op.fingerprint() != StructuredOperator("2d", g, op.terms, point_diagonal=op.point_diagonal).fingerprint()
    # bonds without a diagonal: D = 0
    nod = StructuredOperator("2d", g, op.terms, point_bonds=(E, S))
    assert nod.point_diagonal is not None and not nod.point_diagonal.any()
    assert abs(nod.tocsr() + sp.diags(op.point_diagonal.reshape(-1)) - A).max() <= 1e-13 * abs(A).max()
    # refusals
    bad = E.copy()
    bad[4, g - 1] = 1.0
    with pytest.raises(ValueError):
        StructuredOperator("2d", g, op.terms, point_bonds=(bad, S))
    bad = S.copy()
    bad[g - 1, 2] = 1.0
    with pytest.raises(ValueError):
        StructuredOperator("2d", g, op.terms, point_bonds=(E, bad))
    with pytest.raises(ValueError):
        StructuredOperator("2d", g, op.terms, point_bonds=(E[:, :-1], S))
    with pytest.raises(ValueError):
        StructuredOperator("2d", g, op.terms, point_bonds=(E,))
    with pytest.raises(ValueError):
        StructuredOperator("1d", g, [(None, np.zeros((3, g)))], point_bonds=(E, S))
    i = tri_identity(g)
    with pytest.raises(ValueError):
        StructuredOperator("3d", g, [(i, i, i)], point_bonds=(E, S))


def test_recognise_five_point_round_trip():
    g = 16
    A = step_operator(g).tocsr()
    op = recognise_five_point(A)
    assert op.point_bonds is not None and abs(op.tocsr() - A).max() <= 1e-13 * abs(A).max()
    assert op is recognise_five_point(A)                                   # cached
    for refuses in (recognise, recognise_potential):
        with pytest.raises(UnrecognisedOperator):
            refuses(A, "2d")
    # arithmetic mean, another potential, a scaled matrix
    B = (variable_mass_operator(g, w_smooth(g), smooth_v(g), mean="arithmetic") * 1.7).tocsr()
    assert abs(recognise_five_point(B).tocsr() - B).max() <= 1e-13 * abs(B).max()
    # constant bonds: what recognise_potential / recognise return
    H = (SCALE * MGCMTStencilMaker().laplacian(g, dimension="2d") + sp.diags(smooth_v(g).reshape(-1))).tocsr()
    assert recognise_five_point(H) is recognise_potential(H) and recognise_five_point(H).point_bonds is None
    L = (SCALE * MGCMTStencilMaker().laplacian(g, dimension="2d")).tocsr()
    assert recognise_five_point(L) is recognise(L, "2d")
    # unsymmetric, and wider than 5-point
    U = A.tolil()
    U[5 * g + 3, 5 * g + 4] *= 1.5
    with pytest.raises(UnrecognisedOperator):
        recognise_five_point(U.tocsr())
    with pytest.raises(UnrecognisedOperator):
        recognise_five_point(sp.random(g * g, g * g, density=0.02, random_state=5, format="csr") + sp.identity(g * g))
    W = A.tolil()
    W[5 * g + 3, 6 * g + 4] = W[6 * g + 4, 5 * g + 3] = 0.25          # a corner entry
    with pytest.raises(UnrecognisedOperator):
        recognise_five_point(W.tocsr())


# ---- level matrices -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", [16, 32, 64])
def test_galerkin_hierarchy_and_apply_on_every_level(backend, g):
    """R*A*P of every level — Kronecker factors plus mgcmt_plan_get_point_stencil — against scipy's product of
    MGCMTStencilMaker's own matrices, and mgcmt_apply on every level against that matrix (with and without the shift)."""
    op = step_operator(g)
    plan = Plan(op, 2, nvec=1)
    try:
        chain = galerkin_chain(op.tocsr(), g, 2)
        assert plan.num_levels == len(chain)
        plan.set_shifts([0.7])
        rng = np.random.RandomState(g)
        for level, want in enumerate(chain):
            assert plan.operator_kind(level) == (_lib.OPK_POINT_BONDS if level == 0 else _lib.OPK_NINE_POINT)
            for kind in (_lib.WJACOBI, _lib.GS_MC):
                assert plan.fused_max_sweeps(level, kind) == 0, (level, kind)
            got = assemble_level(plan, level)
            assert abs(got - want).max() <= 1e-13 * abs(want).max(), level
            assert abs(got - got.T).max() <= 1e-13 * abs(want).max()
            x = rng.rand(want.shape[0]) - 0.5
            plan.upload(level, _lib.SLOT_V, 0, x)
            plan.apply(level, (_lib.SLOT_V, 0), (_lib.SLOT_T, 0))
            assert rel_err(plan.download(level, _lib.SLOT_T, 0), want @ x) < 1e-13, level
            plan.apply(level, (_lib.SLOT_V, 0), (_lib.SLOT_T, 0), with_shift=True)
            assert rel_err(plan.download(level, _lib.SLOT_T, 0), want @ x - 0.7 * x) < 1e-13, level
    finally:
        plan.close()
    op = step_operator(16)
    x = np.random.RandomState(2).rand(256)
    assert rel_err(op.dot(x), op.tocsr() @ x) < 1e-13


def test_single_level_plan_solves_directly(backend):
    """lowest = g: level 0 is the coarsest level, its band matrix carries the bonds"""
    import scipy.sparse.linalg as sla
    g = 8
    op = step_operator(g)
    f = np.random.RandomState(3).rand(g * g)
    plan = Plan(op, g, nvec=1)
    try:
        plan.set_shifts([0.7])
        plan.upload(0, _lib.SLOT_F, 0, f)
        plan.coarse_solve(0)
        want = sla.spsolve((op.tocsr() - 0.7 * sp.identity(g * g)).tocsc(), f)
        assert rel_err(plan.download(0, _lib.SLOT_V, 0), want) < 1e-12
    finally:
        plan.close()


# ---- smoothers and cycles against the oracle ------------------------------------------------------------------------------

def test_smoothers_stand_alone(backend):
    g = 32
    op = step_operator(g)
    A = op.tocsr()
    solver, ref = MGCMTSolver(), RefSolver()
    rng = np.random.RandomState(6)
    v0, f = rng.rand(g * g), rng.rand(g * g)
    want = ref.wjacobi(v0.copy(), f.copy(), A, nu=3)
    assert rel_err(flat(solver.wjacobi(v0.copy(), f.copy(), op, nu=3)), flat(want)) < TOL
    assert rel_err(flat(solver.smooth(v0.copy(), f.copy(), A, nu=3, smoother=solver.wjacobi, dimension="2d")), flat(want)) < TOL
    want = ref.gseidel_mc(v0.copy(), f.copy(), A, nu=2, dimension="2d")
    assert rel_err(flat(solver.gseidel_rb(v0.copy(), f.copy(), A, nu=2, dimension="2d")), flat(want)) < TOL
    assert rel_err(flat(solver.gseidel_rb(v0.copy(), f.copy(), op, nu=2)), flat(want)) < TOL
    want = ref.gseidel_mc(v0.copy(), f.copy(), A, nu=2, omega=1.3, dimension="2d")
    assert rel_err(flat(solver.gseidel_rb(v0.copy(), f.copy(), op, nu=2, omega=1.3)), flat(want)) < TOL


@pytest.mark.parametrize("smoother", ["wjacobi", "rb"])
@pytest.mark.parametrize("shift", [0, 1.9])
@pytest.mark.parametrize("lowest", [2, 8])
@pytest.mark.parametrize("g", [16, 32, 64, 128])
def test_vcycle_against_the_oracle(backend, g, lowest, shift, smoother):
    """V(2,2) for (H - shift I) v = f, H = -div(w grad)/pi^2 + V with the step mass and the step potential (w >= 1 keeps
    H > 2, so the shifted operator is definite on every level): from a zero start, called three times (the second call
    captures the cycle's graph, the third replays it), and from a non-zero start; as the matrix-free operator and as the
    sparse matrix (recognise_five_point inside the 2-D entry point).  The oracle's own residual must fall, so that a
    diverging reference cannot hide a broken comparison.  At 128^2 the red-black stages and residual + restriction of level 0
run the marching kernels."""
    op = step_operator(g)
    A = op.tocsr()
    solver, sm, ref, rsm = MGCMTSolver(), MGCMTStencilMaker(), RefSolver(), RefStencilMaker()
    smo, rsmo = (solver.wjacobi, None) if smoother == "wjacobi" else (solver.gseidel_rb, rb(ref))
    n = g * g
    f = np.random.RandomState(g + lowest).rand(n)
    kw = dict(nu1=2, nu2=2, shift=shift, lowest_level=lowest, dimension="2d")
    shifted = A - shift * sp.identity(n)
    v_ref, res = np.zeros(n), [np.linalg.norm(f)]
    for cycle in range(2):
        v_ref = np.asarray(ref.vcycle(v_ref.copy(), f.copy(), A, rsm, smoother=rsmo, **kw)).reshape(-1)
        res.append(np.linalg.norm(f - shifted @ v_ref))
        assert res[-1] < res[-2], res
    first = ref.vcycle(np.zeros(n), f.copy(), A, rsm, smoother=rsmo, **kw)
    for call in range(3):
        got = solver.vcycle(np.zeros(n), f.copy(), op, sm, smoother=smo, **kw)
        assert rel_err(got, first) < TOL, call
    assert rel_err(solver.vcycle(np.zeros(n), f.copy(), A, sm, smoother=smo, **kw), first) < TOL
    got2 = solver.vcycle(np.array(got), f.copy(), op, sm, smoother=smo, **kw)          # non-zero start: the second cycle
    assert rel_err(got2, v_ref) < TOL
    if g >= 128:
        plan = get_plan(op, lowest, nvec=1)
        assert plan.operator_kind(0) == _lib.OPK_POINT_BONDS and plan.operator_kind(1) == _lib.OPK_NINE_POINT
        kind = _lib.WJACOBI if smoother == "wjacobi" else _lib.GS_MC
        assert plan.fused_max_sweeps(0, kind) == 0


@pytest.mark.parametrize("smoother", ["wjacobi", "rb"])
def test_vcycle_matrix_with_column_shifts(backend, smoother):
    g, lowest, k = 32, 4, 3
    op = step_operator(g)
    A = op.tocsr()
    solver, sm, ref, rsm = MGCMTSolver(), MGCMTStencilMaker(), RefSolver(), RefStencilMaker()
    smo, rsmo = (solver.wjacobi, None) if smoother == "wjacobi" else (solver.gseidel_rb, rb(ref))
    rng = np.random.RandomState(9)
    F = rng.rand(g * g, k)
    shifts = np.array([0.0, 0.9, 1.9])
    kw = dict(nu1=2, nu2=2, shifts=shifts, lowest_level=lowest, dimension="2d")
    want = ref.vcycle_matrix(np.zeros((g * g, k)), F.copy(), A, rsm, smoother=rsmo, **kw)
    for start in (op, A):
        got = solver.vcycle_matrix(np.zeros((g * g, k)), F.copy(), start, sm, smoother=smo, **kw)
        assert rel_err(got, want) < TOL
    V0 = rng.rand(g * g, k)
    want = ref.vcycle_matrix(V0.copy(), F.copy(), A, rsm, smoother=rsmo, **kw)
    assert rel_err(solver.vcycle_matrix(V0.copy(), F.copy(), op, sm, smoother=smo, **kw), want) < TOL


def test_gram_schmidt_per_level_and_column_shifts_on_the_marching_level(backend):
    """vcycle_matrix at 128^2 (level 0 marches): three columns with their own shifts, Gram-Schmidt on every level (:434)"""
    g, lowest, k = 128, 8, 3
    op = step_operator(g)
    A = op.tocsr()
    solver, sm, ref, rsm = MGCMTSolver(), MGCMTStencilMaker(), RefSolver(), RefStencilMaker()
    F = np.random.RandomState(19).rand(g * g, k)
    kw = dict(nu1=2, nu2=2, shifts=np.array([0.0, 0.9, 1.9]), lowest_level=lowest, dimension="2d")
    want = ref.vcycle_matrix(np.zeros((g * g, k)), F.copy(), A, rsm, **kw)
    got = solver.vcycle_matrix(np.zeros((g * g, k)), F.copy(), op, sm, **kw)
    assert rel_err(got, want) < TOL


def test_full_multigrid(backend):
    g = 32
    op = step_operator(g)
    A = op.tocsr()
    solver, sm, ref, rsm = MGCMTSolver(), MGCMTStencilMaker(), RefSolver(), RefStencilMaker()
    f = np.random.RandomState(10).rand(g * g)
    for smo, rsmo in ((solver.wjacobi, ref.wjacobi), (solver.gseidel_rb, rb(ref))):
        got = solver.fmg(f.copy(), op, sm, nu1=2, nu2=2, smoother=smo, shift=0.7, lowest_level=4, dimension="2d")
        want = ref.fmg(f, A, rsm, nu1=2, nu2=2, smoother=rsmo, shift=0.7, lowest_level=4, dimension="2d")
        assert rel_err(got, want) < TOL
    got = solver.fmg(f.copy(), A, sm, nu1=2, nu2=2, shift=0.7, lowest_level=4, dimension="2d")          # the sparse-matrix entry
    assert rel_err(got, ref.fmg(f, A, rsm, nu1=2, nu2=2, shift=0.7, lowest_level=4, dimension="2d")) < TOL


def test_foreign_smoother_sees_the_level_matrices(backend):
    """The seam of MGCMTSolver.py:313,326: a callable smoother receives (R A P - shift I) of every level — level 0 with its
    bonds — and the cycle built around it equals the reference's."""
    g, lowest = 32, 4
    op = step_operator(g)
    A = op.tocsr()
    solver, sm, ref, rsm = MGCMTSolver(), MGCMTStencilMaker(), RefSolver(), RefStencilMaker()
    chain = galerkin_chain(A, g, lowest)
    seen = {}

    def damped(v, f, M, nu=4):
        M = sp.csr_matrix(M)
        seen[M.shape[0]] = M
        v, f = np.asarray(v, dtype=float).reshape(-1).copy(), np.asarray(f, dtype=float).reshape(-1)
        for _ in range(nu):
            v = v + 0.6 * (f - M @ v) / M.diagonal()
        return v.reshape(-1, 1)

    f = np.random.RandomState(12).rand(g * g)
    got = solver.vcycle(np.zeros(g * g), f.copy(), op, sm, nu1=2, nu2=2, smoother=damped, shift=0.7, lowest_level=lowest, dimension="2d")
    assert sorted(seen) == [64, 256, 1024]
    for level, want in enumerate(chain[:-1]):
        M = seen[want.shape[0]]
        assert abs(M - (want - 0.7 * sp.identity(want.shape[0]))).max() <= 1e-13 * abs(want).max(), level
    want = ref.vcycle(np.zeros(g * g), f.copy(), A, rsm, nu1=2, nu2=2, smoother=damped, shift=0.7, lowest_level=lowest, dimension="2d")
    assert rel_err(got, want) < TOL


# ---- marching against flat ------------------------------------------------------------------------------------------------

def _bond_plan(op, lowest, march, nvec=1):
    """a fresh plan (not the cache's) created with MGCMT_BONDS_MARCH set: the library reads it at creation"""
    old = os.environ.get("MGCMT_BONDS_MARCH")
    os.environ["MGCMT_BONDS_MARCH"] = "1" if march else "0"
    try:
        return Plan(op, lowest, nvec=nvec)
    finally:
        if old is None:
            del os.environ["MGCMT_BONDS_MARCH"]
        else:
            os.environ["MGCMT_BONDS_MARCH"] = old


def _pieces(op, lowest, march, v0, f, shifts):
    """per piece the vectors it leaves, all columns: a Jacobi sweep, a red-black sweep (also over-relaxed), the residual
    restricted to level 1, the operator applied, and one V(2,2) cycle of either smoother"""
    k = len(shifts)
    p = _bond_plan(op, lowest, march, nvec=k)
    out = {}
    try:
        p.set_shifts(list(shifts))

        def start():
            for q in range(k):
                p.upload(0, _lib.SLOT_V, q, v0[q])
                p.upload(0, _lib.SLOT_F, q, f[q])

        def column(level, slot):
            return np.stack([np.array(p.download(level, slot, q)) for q in range(k)])

        start()
        p.smooth(0, _lib.WJACOBI, 1, 2. / 3., k=k)
        out["jacobi sweep"] = column(0, _lib.SLOT_V)
        start()
        p.smooth(0, _lib.GS_MC, 1, 1.0, k=k)
        out["red-black sweep"] = column(0, _lib.SLOT_V)
        start()
        p.smooth(0, _lib.GS_MC, 2, 1.3, k=k)
        out["two over-relaxed red-black sweeps"] = column(0, _lib.SLOT_V)
        start()
        for q in range(k):
            p.upload(1, _lib.SLOT_V, q, np.ones(p.size(1)))
            p.upload(0, _lib.SLOT_T, q, np.full(p.size(0), 7.0))
        p.residual_restrict(0, k=k)
        out["restricted residual"] = column(1, _lib.SLOT_F)
        assert not column(1, _lib.SLOT_V).any()
        # the one-pass marching form does not store the fine residual (slot T keeps its marker), the flat pair does
        assert np.all(column(0, _lib.SLOT_T) == 7.0) == bool(march)
        start()
        for q in range(k):
            p.apply(0, (_lib.SLOT_V, q), (_lib.SLOT_T, q), with_shift=True)
        out["apply"] = column(0, _lib.SLOT_T)
        for name, kind, omega in (("jacobi cycle", _lib.WJACOBI, 2. / 3.), ("red-black cycle", _lib.GS_MC, 1.0)):
            start()
            p.vcycle(2, 2, kind, omega=omega, k=k, nu_coarse=2)
            out[name] = column(0, _lib.SLOT_V)
            out[name + ": F[1]"] = column(1, _lib.SLOT_F)
    finally:
        p.close()
    return out


@pytest.mark.parametrize("g,k", [(128, 2), (256, 1), (512, 1)])
def test_marching_kernels_give_the_bits_of_the_flat_ones(backend, g, k):
    """MGCMT_BONDS_MARCH = 1 against 0 on the same operator.  128^2: one wave per row; 256^2: two waves per row of the
    residual + restriction pass (the one-lane overlap) and several row chunks; 512^2: the 256-thread blocks.  A Jacobi sweep,
    a red-black sweep and the applied operator are bit-identical.  The marching residual + restriction sums in k_restrict's
    order, so F[1] is bit-identical to the flat residual followed by k_restrict as well — and with every piece bit-identical
    so is a whole V(2,2) cycle; the issue's bar for the cycle (1e-12) is asserted on top."""
    op = step_operator(g)
    rng = np.random.RandomState(g)
    v0, f = rng.rand(k, g * g) - 0.5, rng.rand(k, g * g)
    shifts = (0.7, 1.9)[:k]
    flat_form = _pieces(op, 8, False, v0, f, shifts)
    march = _pieces(op, 8, True, v0, f, shifts)
    assert sorted(flat_form) == sorted(march)
    for name in march:
        assert np.all(np.isfinite(march[name])), name
        if "cycle" in name:
            assert rel_err(march[name], flat_form[name]) < 1e-12, name
        assert np.array_equal(march[name], flat_form[name]), (name, np.abs(march[name] - flat_form[name]).max())
    # and the flat form is right: a sweep against the assembled matrix
    A = (op.tocsr() - shifts[0] * sp.identity(g * g)).tocsr()
    want = v0[0] + (2. / 3.) * (f[0] - A @ v0[0]) / A.diagonal()
    assert rel_err(march["jacobi sweep"][0], want) < 1e-13
    assert rel_err(march["apply"][0], A @ v0[0]) < 1e-13
    R = MGCMTStencilMaker().restriction(g, g // 2, dimension="2d")
    assert rel_err(march["restricted residual"][0], R @ (f[0] - A @ v0[0])) < 1e-13


# ---- a general Kronecker part plus bonds ----------------------------------------------------------------------------------

def _general_plus_bonds(g):
    """a separable potential left in the factors (so the Kronecker part of level 0 is not a constant 5-point operator) plus
    the bonds and the diagonal of the step mass"""
    base = step_operator(g)
    x = (np.arange(g) + 0.5) / g - 0.5
    Y, X = base.terms[0][1].copy(), base.terms[1][0].copy()
    Y[1] += 20.0 * x * x
    X[1] += 35.0 * (x - 0.1) ** 2
    return StructuredOperator("2d", g, [(tri_identity(g), Y), (X, tri_identity(g))], point_diagonal=base.point_diagonal, point_bonds=base.point_bonds)


def test_general_kronecker_part_plus_bonds(backend):
    g, lowest = 32, 4
    op = _general_plus_bonds(g)
    A = op.tocsr()
    plan = Plan(op, lowest, nvec=1)
    try:
        chain = galerkin_chain(A, g, lowest)
        assert plan.operator_kind(0) == _lib.OPK_POINT_BONDS
        rng = np.random.RandomState(g)
        for level, want in enumerate(chain):
            got = assemble_level(plan, level)
            assert abs(got - want).max() <= 1e-13 * abs(want).max(), level
            x = rng.rand(want.shape[0]) - 0.5
            plan.upload(level, _lib.SLOT_V, 0, x)
            plan.apply(level, (_lib.SLOT_V, 0), (_lib.SLOT_T, 0))
            assert rel_err(plan.download(level, _lib.SLOT_T, 0), want @ x) < 1e-13, level
    finally:
        plan.close()
    solver, sm, ref, rsm = MGCMTSolver(), MGCMTStencilMaker(), RefSolver(), RefStencilMaker()
    f = np.random.RandomState(14).rand(g * g)
    kw = dict(nu1=2, nu2=2, shift=0.7, lowest_level=lowest, dimension="2d")
    for smo, rsmo in ((solver.wjacobi, None), (solver.gseidel_rb, rb(ref))):
        want = ref.vcycle(np.zeros(g * g), f.copy(), A, rsm, smoother=rsmo, **kw)
        assert rel_err(solver.vcycle(np.zeros(g * g), f.copy(), op, sm, smoother=smo, **kw), want) < TOL


# ---- refused entries ------------------------------------------------------------------------------------------------------

def test_refused_entries(backend):
    g = 16
    op = step_operator(g)
    plan = Plan(op, 4, nvec=6)
    lib = _lib.lib()
    h = plan._h
    i6 = (ctypes.c_int * 6)(0, 1, 2, 3, 4, 5)
    out = (ctypes.c_double * 8)()
    calls = {
        "gseidel": lambda: lib.mgcmt_smooth(h, 0, _lib.GS_LEX, 1, 1.0, 1, None),
        "sor": lambda: lib.mgcmt_smooth(h, 0, _lib.SOR_LEX, 1, 1.2, 1, None),
        "vcycle lex": lambda: lib.mgcmt_vcycle(h, 0, 2, 2, 2, _lib.GS_LEX, 1.0, 1, 0, None),
        "twogrid": lambda: lib.mgcmt_twogrid(h, 0, 2, 2, _lib.WJACOBI, 2. / 3., 1, None),
        "rqmin": lambda: lib.mgcmt_rqmin(h, 0, _lib.SLOT_V, i6, 2, 0, out, None),
        "vcycle_rqmg": lambda: lib.mgcmt_vcycle_rqmg(h, _lib.SLOT_V, i6, 2, 2, 0, out, None),
        "ritz_pair": lambda: lib.mgcmt_ritz_pair(h, 0, _lib.SLOT_V, 0, _lib.SLOT_V, 1, _lib.SLOT_V, 2, out, None),
        "rayleigh_residual": lambda: lib.mgcmt_rayleigh_residual(h, 0, _lib.SLOT_V, 1, out, out, None),
        "sharded_vcycle": lambda: lib.mgcmt_sharded_vcycle(h, h, 2, 2, 2, _lib.WJACOBI, 2. / 3., 1, 0, None),
    }
    try:
        for name, call in calls.items():
            assert call() == -4, name          # MGCMT_ERR_UNSUPPORTED
        # creation: no mass operator, no strips, 2-D only, zero bonds towards the outside, no null array
        nterms, xfac, yfac = op.factor_blocks()
        desc = _lib.PlanDesc()
        desc.dim, desc.nterms, desc.g, desc.lowest, desc.nvec = 2, nterms, g, 4, 1
        desc.xfac, desc.yfac = _lib.as_dp(xfac), _lib.as_dp(yfac)
        pd, E, S = (np.ascontiguousarray(a) for a in (op.point_diagonal,) + op.point_bonds)
        dp = _lib.as_dp
        hh = ctypes.c_void_p()
        desc.row_begin, desc.row_end, desc.strip_levels = 0, g // 2, 1
        assert lib.mgcmt_plan_create_bonds(ctypes.byref(desc), dp(pd), dp(E), dp(S), ctypes.byref(hh)) == -4
        desc.row_begin, desc.row_end, desc.strip_levels = 0, 0, 0
        desc.m_nterms, desc.m_xfac, desc.m_yfac = nterms, dp(xfac), dp(yfac)
        assert lib.mgcmt_plan_create_bonds(ctypes.byref(desc), dp(pd), dp(E), dp(S), ctypes.byref(hh)) == -4
        desc.m_nterms = 0
        assert lib.mgcmt_plan_create_bonds(ctypes.byref(desc), dp(pd), None, dp(S), ctypes.byref(hh)) == -1
        assert lib.mgcmt_plan_create_bonds(ctypes.byref(desc), None, dp(E), dp(S), ctypes.byref(hh)) == -1
        bad = E.copy()
        bad[3, g - 1] = 1.0
        assert lib.mgcmt_plan_create_bonds(ctypes.byref(desc), dp(pd), dp(bad), dp(S), ctypes.byref(hh)) == -1
        bad = S.copy()
        bad[g - 1, 3] = 1.0
        assert lib.mgcmt_plan_create_bonds(ctypes.byref(desc), dp(pd), dp(E), dp(bad), ctypes.byref(hh)) == -1
        desc.dim = 1
        assert lib.mgcmt_plan_create_bonds(ctypes.byref(desc), dp(pd), dp(E), dp(S), ctypes.byref(hh)) == -1
    finally:
        plan.close()
    solver, sm = MGCMTSolver(), MGCMTStencilMaker()
    v0, f = np.zeros(g * g), np.ones(g * g)
    A = op.tocsr()
    for bad in (solver.gseidel, solver.sor):
        for start in (op, A):
            with pytest.raises(ValueError, match="wjacobi, gseidel_rb"):
                solver.vcycle(v0.copy(), f.copy(), start, sm, smoother=bad, dimension="2d", lowest_level=4)
    with pytest.raises(ValueError, match="wjacobi, gseidel_rb"):
        solver.gseidel(v0.copy(), f.copy(), op)
    with pytest.raises(ValueError, match="wjacobi, gseidel_rb"):
        solver.sor(v0.copy(), f.copy(), op, omega=1.2)
    for start in (op, A):
        with pytest.raises(ValueError):
            solver.twogrid(v0.copy(), f.copy(), start, sm, dimension="2d")
    with pytest.raises(ValueError):
        solver.rqmin(op, np.ones(g * g), M=sp.identity(g * g, format="csr"))
    with pytest.raises(ValueError):
        Plan(op, 4, mass=identity_operator(g, "2d"))
    # a random matrix that is no 5-point operator is still refused by the 2-D entry points, with recognise's error
    bad = sp.random(g * g, g * g, density=0.02, random_state=1, format="csr") + sp.identity(g * g)
    with pytest.raises(UnrecognisedOperator):
        solver.vcycle(v0.copy(), f.copy(), bad, sm, dimension="2d", lowest_level=4)


# ---- the eigensolver ------------------------------------------------------------------------------------------------------

def test_block_eigensolve_dot_with_a_light_mass_against_eigsh(backend):
    """The lowest three states of the dot — inverse mass 4 inside, 1 outside, barrier 30 — at 64^2 against scipy's eigsh on
    the assembled Hamiltonian (the bar of tests/test_drivers.py).  lambda_2, lambda_3 (about 25.38, 25.58) are a
    near-degenerate pair, so both are in the block."""
    import scipy.sparse.linalg as sla
    g, k = 64, 3
    op = step_operator(g)
    with pytest.raises(UnrecognisedOperator):
        recognise_potential(op.tocsr())
    # 16 iterations, as tests/test_point_potential.py: on the emulation 8 leave 7e-6, 12 leave 2e-10, 16 leave 3e-14
    vals, vecs = drivers.block_eigensolve(op, k=k, cycles=16, lowest=8)
    want = np.sort(sla.eigsh(op.tocsr(), k=k, sigma=0.0, which="LM")[0])
    assert np.allclose(vals, want, rtol=0, atol=1e-8), np.abs(vals - want)
    assert np.abs(vecs.T @ vecs - np.eye(k)).max() < 1e-10
