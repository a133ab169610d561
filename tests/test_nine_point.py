"""Tensor effective mass: 2-D operators with a per-point 9-point stencil (operators.tensor_mass_operator /
recognise_nine_point, StructuredOperator(point_stencil=...), mgcmt_plan_create_nine) against the NumPy oracle
(oracle.sparse_ref.RefSolver, which cycles any sparse matrix) and against scipy's own R*A*P, through the HIP library on the
GPU box and through the emulated kernels on CPU (``backend`` fixture).

Level 0 of such a plan is a nine-plane level like the Galerkin levels of every plan with a per-point part (DESIGN par. 4.17):
from 128 columns on the tile kernels of csrc/kernels_nine_tile.hip, otherwise and with MGCMT_NINE_TILE=0 on the flat ones of
csrc/kernels_pointwise.hip; MGCMT_NINE_TILE=2 puts the Galerkin levels of any point plan on the tile kernels too.

The lowest eigenvalues of the test operators lie between 1.80 and 2.11, so the shifts are 0 and 0.7 (1.9, the shift of the
Laplacian tests, lands next to an eigenvalue — 1.92 at 32^2 smooth — where parity at 1e-10 means nothing)."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import rel_err
from multigridcmt_amd import (MGCMTSolver, MGCMTStencilMaker, _lib, drivers, recognise_five_point, recognise_nine_point, tensor_mass_operator,
                              variable_mass_operator)
from multigridcmt_amd.operators import (StructuredOperator, UnrecognisedOperator, identity_operator, planes_to_csr, potential_operator, recognise,
                                        recognise_potential, tri_identity, tri_to_sparse)
from multigridcmt_amd.plan import Plan, get_plan, release_plans
from oracle.sparse_ref import RefSolver, RefStencilMaker
from test_point_potential import galerkin_chain, rough_v, smooth_v

TOL = 1e-10          # the bar of tests/test_point_potential.py
SCALE = -1 / np.pi ** 2
SHIFTS = (0, 0.7)


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


def tensor(g, profile):
    """(wxx, wyy, wxy) of a tensor with principal values l1, 1 whose first axis is rotated by theta.  smooth: a Gaussian bump
    of both; rough: inside a disc theta = 0.6 and l1 = 4 with 20 % disorder, the identity outside (a jump across an interface)."""
    X, Y = _centres(g)
    r2 = (X - 0.05) ** 2 + (Y + 0.1) ** 2
    if profile == "smooth":
        e = np.exp(-r2 / 0.15 ** 2)
        l1, theta = 1.0 + 3.0 * e, 0.6 * e
    else:
        disc = r2 < 0.3 ** 2
        l1 = np.where(disc, 4.0 * (1.0 + 0.2 * np.random.RandomState(2).rand(g, g)), 1.0)
        theta = np.where(disc, 0.6, 0.0)
    c, s = np.cos(theta), np.sin(theta)
    return c * c * l1 + s * s, s * s * l1 + c * c, c * s * (l1 - 1.0)


def tensor_operator(g, profile, V=None, mean="harmonic"):
    return tensor_mass_operator(g, *tensor(g, profile), V=V, mean=mean)


def flat(a):
    return np.asarray(a).reshape(-1)


def rb(ref):
    return lambda v, f, A, nu=4: ref.gseidel_mc(v, f, A, nu=nu, dimension="2d")


def assemble_level(plan, level):
    """the matrix of `level`: Kronecker factors (mgcmt_plan_get_factors) plus the nine planes (mgcmt_plan_get_point_stencil);
    entries towards points outside the grid must be exact zeros"""
    gl = plan.g >> level
    xf, yf = plan.factors(level, 0), plan.factors(level, 1)
    A = sum(sp.kron(tri_to_sparse(xf[m]), tri_to_sparse(yf[m]), format="csr") for m in range(xf.shape[0])).tocsr()
    G = plan.point_stencil(level)
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


def entry_by_entry(g, wxx, wyy, wxy, V, m):
    """the issue's formulas, one entry at a time"""
    t = SCALE * g * g
    A = sp.lil_matrix((g * g, g * g))
    for i in range(g):
        for j in range(g):
            r = i * g + j
            be = m(wxx[i, j], wxx[i, j + 1]) if j + 1 < g else wxx[i, j]
            bw = m(wxx[i, j], wxx[i, j - 1]) if j > 0 else wxx[i, j]
            bs = m(wyy[i, j], wyy[i + 1, j]) if i + 1 < g else wyy[i, j]
            bn = m(wyy[i, j], wyy[i - 1, j]) if i > 0 else wyy[i, j]
            A[r, r] = -t * (be + bw + bs + bn) + (0.0 if V is None else V[i, j])
            if j + 1 < g:
                A[r, r + 1] = t * be
            if j > 0:
                A[r, r - 1] = t * bw
            if i + 1 < g:
                A[r, r + g] = t * bs
            if i > 0:
                A[r, r - g] = t * bn
            for a in (-1, 1):
                for b in (-1, 1):
                    if 0 <= i + a < g and 0 <= j + b < g:
                        A[r, (i + a) * g + j + b] = a * b * t * (wxy[i + a, j] + wxy[i, j + b]) / 4
    return A.tocsr()


# ---- 1. the operator object -----------------------------------------------------------------------------------------------

def test_constructor_and_operator_algebra():
    g = 8
    op = tensor_operator(g, "rough", V=smooth_v(g))
    G = op.point_stencil
    assert G.shape == (3, 3, g, g) and op.point_diagonal is None and op.point_bonds is None
    A = op.tocsr()
    kron = StructuredOperator("2d", g, op.terms).tocsr()
    assert abs(A - (kron + planes_to_csr(G))).max() == 0.0
    assert abs(A - A.T).max() == 0.0
    assert np.allclose(op.diagonal(), A.diagonal(), rtol=1e-14)
    assert abs((op * 2.5).tocsr() - 2.5 * A).max() <= 1e-13 * abs(A).max()
    assert abs((2.5 * op).tocsr() - 2.5 * A).max() <= 1e-13 * abs(A).max()
    assert abs((-op / 4.0).tocsr() + A / 4.0).max() <= 1e-13 * abs(A).max()
    assert abs(op.shifted(0.7).tocsr() - (A - 0.7 * sp.identity(g * g))).max() <= 1e-13 * abs(A).max()
    assert (op * 2.0).point_stencil is not None and op.shifted(0.7).point_stencil is not None
    assert op.fingerprint() == tensor_operator(g, "rough", V=smooth_v(g)).fingerprint()
    G2 = G.copy()
    G2[2, 2][2, 3] += 1e-9
    G2[0, 0][3, 4] += 1e-9          # (kept symmetric)
    assert op.fingerprint() != StructuredOperator("2d", g, op.terms, point_stencil=G2).fingerprint()
    assert op.fingerprint() != StructuredOperator("2d", g, op.terms).fingerprint()
    # a flat list of 9 g^2 numbers is taken as the planes
    assert StructuredOperator("2d", g, op.terms, point_stencil=G.reshape(-1)).fingerprint() == op.fingerprint()
    # refusals: not 2-D, with a diagonal or bonds, towards the outside, unsymmetric, wrong size
    i = tri_identity(g)
    with pytest.raises(ValueError):
        StructuredOperator("3d", g, [(i, i, i)], point_stencil=G)
    with pytest.raises(ValueError):
        StructuredOperator("1d", g, [(None, np.zeros((3, g)))], point_stencil=G)
    with pytest.raises(ValueError):
        StructuredOperator("2d", g, op.terms, point_diagonal=np.zeros((g, g)), point_stencil=G)
    with pytest.raises(ValueError):
        StructuredOperator("2d", g, op.terms, point_bonds=(np.zeros((g, g)), np.zeros((g, g))), point_stencil=G)
    for (a, b, ii, jj) in ((0, 1, 0, 3), (2, 2, g - 1, 2), (1, 2, 4, g - 1), (2, 0, 3, 0)):
        bad = G.copy()
        bad[a, b][ii, jj] = 1.0
        with pytest.raises(ValueError, match="outside"):
            StructuredOperator("2d", g, op.terms, point_stencil=bad)
    bad = G.copy()
    bad[1, 2][3, 3] += 0.5
    with pytest.raises(ValueError, match="symmetric"):
        StructuredOperator("2d", g, op.terms, point_stencil=bad)
    with pytest.raises(ValueError):
        StructuredOperator("2d", g, op.terms, point_stencil=G[:, :, :-1, :])


# ---- 2. tensor_mass_operator ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("profile", ["smooth", "rough"])
@pytest.mark.parametrize("mean,m", [("harmonic", lambda a, b: 2 * a * b / (a + b)), ("arithmetic", lambda a, b: 0.5 * (a + b))])
def test_tensor_mass_operator_entries(profile, mean, m):
    for g in (16, 32):
        wxx, wyy, wxy = tensor(g, profile)
        V = rough_v(g)
        op = tensor_mass_operator(g, wxx, wyy, wxy, V=V, mean=mean)
        assert op.point_stencil is not None
        A = op.tocsr()
        want = entry_by_entry(g, wxx, wyy, wxy, V, m)
        assert abs(A - want).max() <= 1e-13 * abs(want).max()
        assert abs(A - A.T).max() == 0.0
        # the Kronecker terms carry the medians: a constant 5-point part
        t = SCALE * g * g
        assert np.all(op.terms[0][1][2, :-1] == t * np.median(wxx)) and np.all(op.terms[1][0][2, :-1] == t * np.median(wyy))
    H = tensor_mass_operator(16, *tensor(16, profile)).toarray()
    assert np.linalg.eigvalsh(H).min() > 0.0


def test_tensor_mass_operator_special_cases():
    for g in (16, 32):
        one, zero = np.ones((g, g)), np.zeros((g, g))
        L = SCALE * MGCMTStencilMaker().laplacian(g, dimension="2d")
        op = tensor_mass_operator(g, one, one, zero)
        assert op.point_stencil is None and op.point_bonds is None and op.point_diagonal is None
        assert abs(op.tocsr() - L).max() == 0.0
    g = 16
    wxx, wyy, wxy = tensor(g, "rough")
    V = smooth_v(g)
    # a diagonal tensor: bonds, which the bonds plan takes
    op = tensor_mass_operator(g, wxx, wyy, np.zeros((g, g)), V=V)
    assert op.point_stencil is None and op.point_bonds is not None
    m = lambda a, b: 2 * a * b / (a + b)
    want = entry_by_entry(g, wxx, wyy, np.zeros((g, g)), V, m)
    assert abs(op.tocsr() - want).max() <= 1e-13 * abs(want).max()
    # ... and an isotropic one: exactly variable_mass_operator's
    for mean in ("harmonic", "arithmetic"):
        a = tensor_mass_operator(g, wxx, wxx, np.zeros((g, g)), V=V, mean=mean)
        b = variable_mass_operator(g, wxx, V, mean=mean)
        assert a.fingerprint() == b.fingerprint() and abs(a.tocsr() - b.tocsr()).max() == 0.0
    # refusals
    with pytest.raises(ValueError):
        tensor_mass_operator(g, wxx, wyy, wxy, mean="geometric")
    with pytest.raises(ValueError):
        tensor_mass_operator(g, wxx[:-1], wyy, wxy)
    with pytest.raises(ValueError):
        tensor_mass_operator(g, wxx, wyy, wxy[:, :-1])
    with pytest.raises(ValueError):
        tensor_mass_operator(g, wxx, wyy, wxy, V=np.ones(g))
    with pytest.raises(ValueError, match="positive definite"):
        tensor_mass_operator(g, -wxx, wyy, wxy)
    bad = wyy.copy()
    bad[3, 4] = 0.0
    with pytest.raises(ValueError, match="positive definite"):
        tensor_mass_operator(g, wxx, bad, wxy)
    bad = wxy.copy()
    bad[5, 5] = 10.0          # wxx wyy < wxy^2 there
    with pytest.raises(ValueError, match="positive definite"):
        tensor_mass_operator(g, wxx, wyy, bad)


# ---- 3. recognise_nine_point ----------------------------------------------------------------------------------------------

def test_recognise_nine_point_round_trip():
    g = 16
    A = tensor_operator(g, "rough", V=smooth_v(g)).tocsr()
    op = recognise_nine_point(A)
    assert op.point_stencil is not None and abs(op.tocsr() - A).max() <= 1e-13 * abs(A).max()
    assert op is recognise_nine_point(A)                                   # cached
    assert len(op.terms) == 2 and np.ptp(op.terms[0][1][2, :-1]) == 0 and np.ptp(op.terms[1][0][2, :-1]) == 0          # Toeplitz terms from the medians
    for refuses in (recognise, recognise_potential):
        with pytest.raises(UnrecognisedOperator):
            refuses(A, "2d")
    with pytest.raises(UnrecognisedOperator, match="5-point"):
        recognise_five_point(A)
    B = (tensor_operator(g, "smooth", mean="arithmetic") * 1.7).tocsr()
    assert abs(recognise_nine_point(B).tocsr() - B).max() <= 1e-13 * abs(B).max()
    # what the earlier recognisers accept comes back as theirs, the same cached object
    F = variable_mass_operator(g, tensor(g, "rough")[0], smooth_v(g)).tocsr()
    assert recognise_nine_point(F) is recognise_five_point(F) and recognise_nine_point(F).point_stencil is None
    H = (SCALE * MGCMTStencilMaker().laplacian(g, dimension="2d") + sp.diags(smooth_v(g).reshape(-1))).tocsr()
    assert recognise_nine_point(H) is recognise_potential(H)
    L = (SCALE * MGCMTStencilMaker().laplacian(g, dimension="2d")).tocsr()
    assert recognise_nine_point(L) is recognise(L, "2d")
    sop = tensor_operator(g, "smooth")
    assert recognise_nine_point(sop) is sop
    # refusals: unsymmetric, an entry two columns away, a wrap across a row end, something else entirely
    U = A.tolil()
    U[5 * g + 3, 6 * g + 4] *= 1.5
    with pytest.raises(UnrecognisedOperator, match="symmetric"):
        recognise_nine_point(U.tocsr())
    W = A.tolil()
    W[5 * g + 3, 5 * g + 5] = W[5 * g + 5, 5 * g + 3] = 0.25
    with pytest.raises(UnrecognisedOperator):
        recognise_nine_point(W.tocsr())
    W = A.tolil()
    W[5 * g + g - 1, 6 * g] = W[6 * g, 5 * g + g - 1] = 0.25          # (5, g-1) -> (6, 0): offset +1 across the row end
    with pytest.raises(UnrecognisedOperator, match="row end"):
        recognise_nine_point(W.tocsr())
    with pytest.raises(UnrecognisedOperator):
        recognise_nine_point(sp.random(g * g, g * g, density=0.02, random_state=5, format="csr") + sp.identity(g * g))
    with pytest.raises(UnrecognisedOperator):
        recognise_nine_point(sp.identity(g * g + 1, format="csr") * 2.0 + sp.eye(g * g + 1, k=7, format="csr"))


# ---- 4. level matrices ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", [16, 32, 64])
def test_galerkin_hierarchy_and_apply_on_every_level(backend, g):
    """R*A*P of every level — Kronecker factors plus mgcmt_plan_get_point_stencil — against scipy's product of
    MGCMTStencilMaker's own matrices, and mgcmt_apply on every level against that matrix (with and without the shift)."""
    op = tensor_operator(g, "rough", V=smooth_v(g))
    plan = Plan(op, 4, nvec=1)
    try:
        chain = galerkin_chain(op.tocsr(), g, 4)
        assert plan.num_levels == len(chain)
        plan.set_shifts([0.7])
        rng = np.random.RandomState(g)
        for level, want in enumerate(chain):
            assert plan.operator_kind(level) == _lib.OPK_NINE_POINT
            assert not plan.level_tiled(level)
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
        assert np.array_equal(plan.point_stencil(0), op.point_stencil)
    finally:
        plan.close()
    op = tensor_operator(16, "smooth")
    x = np.random.RandomState(2).rand(256)
    assert rel_err(op.dot(x), op.tocsr() @ x) < 1e-13


def test_single_level_plan_solves_directly(backend):
    """lowest = g: level 0 is the coarsest level, its band matrix carries the nine planes; a cycle on it is that solve"""
    import scipy.sparse.linalg as sla
    g = 8
    op = tensor_operator(g, "rough")
    f = np.random.RandomState(3).rand(g * g)
    want = sla.spsolve((op.tocsr() - 0.7 * sp.identity(g * g)).tocsc(), f)
    plan = Plan(op, g, nvec=1)
    try:
        plan.set_shifts([0.7])
        plan.upload(0, _lib.SLOT_F, 0, f)
        plan.coarse_solve(0)
        assert rel_err(plan.download(0, _lib.SLOT_V, 0), want) < 1e-12
    finally:
        plan.close()
    got = MGCMTSolver().vcycle(np.zeros(g * g), f.copy(), op, MGCMTStencilMaker(), shift=0.7, lowest_level=g, dimension="2d")
    assert rel_err(flat(got), want) < 1e-12
    ref = RefSolver().vcycle(np.zeros(g * g), f.copy(), op.tocsr(), RefStencilMaker(), shift=0.7, lowest_level=g, dimension="2d")
    assert rel_err(flat(got), flat(ref)) < TOL


# ---- 5. / 6. / 7. smoothers and cycles against the oracle ---------------------------------------------------------------------

@pytest.mark.parametrize("g", [16, 32])
def test_smoothers_stand_alone(backend, g):
    op = tensor_operator(g, "rough")
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
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("profile", ["smooth", "rough"])
@pytest.mark.parametrize("g", [16, 32, 64, 128])
def test_vcycle_against_the_oracle(backend, g, profile, shift, smoother):
    """V(2,2) for (H - shift I) v = f with lowest_level = 4: from a zero start, called three times (the second call captures the
    cycle's graph, the third replays it), and from a non-zero start; as the matrix-free operator and as the sparse matrix
    (recognise_nine_point inside the 2-D entry point).  The oracle's own residual must fall, so that a diverging reference
    cannot hide a broken comparison.  At 128^2 level 0 runs the tile kernels, at 64^2 the flat ones."""
    op = tensor_operator(g, profile)
    A = op.tocsr()
    solver, sm, ref, rsm = MGCMTSolver(), MGCMTStencilMaker(), RefSolver(), RefStencilMaker()
    smo, rsmo = (solver.wjacobi, None) if smoother == "wjacobi" else (solver.gseidel_rb, rb(ref))
    n = g * g
    f = np.random.RandomState(1).rand(n)
    kw = dict(nu1=2, nu2=2, shift=shift, lowest_level=4, dimension="2d")
    shifted = A - shift * sp.identity(n)
    first = np.asarray(ref.vcycle(np.zeros(n), f.copy(), A, rsm, smoother=rsmo, **kw)).reshape(-1)
    second = np.asarray(ref.vcycle(first.copy(), f.copy(), A, rsm, smoother=rsmo, **kw)).reshape(-1)
    res = [np.linalg.norm(f), np.linalg.norm(f - shifted @ first), np.linalg.norm(f - shifted @ second)]
    assert res[2] < res[1] < res[0], res
    for call in range(3):
        got = solver.vcycle(np.zeros(n), f.copy(), op, sm, smoother=smo, **kw)
        assert rel_err(got, first) < TOL, call
    assert rel_err(solver.vcycle(np.zeros(n), f.copy(), A, sm, smoother=smo, **kw), first) < TOL
    got2 = solver.vcycle(np.array(got), f.copy(), op, sm, smoother=smo, **kw)          # non-zero start: the second cycle
    assert rel_err(got2, second) < TOL
    if g >= 64:
        plan = get_plan(op, 4, nvec=1)
        assert plan.operator_kind(0) == _lib.OPK_NINE_POINT and plan.operator_kind(1) == _lib.OPK_NINE_POINT
        assert plan.level_tiled(0) == (g >= 128) and not plan.level_tiled(1)
        assert plan.fused_max_sweeps(0, _lib.WJACOBI if smoother == "wjacobi" else _lib.GS_MC) == 0


@pytest.mark.parametrize("smoother", ["wjacobi", "rb"])
def test_vcycle_matrix_with_column_shifts(backend, smoother):
    g, lowest, k = 32, 4, 3
    op = tensor_operator(g, "rough")
    A = op.tocsr()
    solver, sm, ref, rsm = MGCMTSolver(), MGCMTStencilMaker(), RefSolver(), RefStencilMaker()
    smo, rsmo = (solver.wjacobi, None) if smoother == "wjacobi" else (solver.gseidel_rb, rb(ref))
    rng = np.random.RandomState(9)
    F = rng.rand(g * g, k)
    shifts = np.array([0.0, 0.35, 0.7])
    kw = dict(nu1=2, nu2=2, shifts=shifts, lowest_level=lowest, dimension="2d")
    want = ref.vcycle_matrix(np.zeros((g * g, k)), F.copy(), A, rsm, smoother=rsmo, **kw)
    for start in (op, A):
        got = solver.vcycle_matrix(np.zeros((g * g, k)), F.copy(), start, sm, smoother=smo, **kw)
        assert rel_err(got, want) < TOL
    V0 = rng.rand(g * g, k)
    want = ref.vcycle_matrix(V0.copy(), F.copy(), A, rsm, smoother=rsmo, **kw)
    assert rel_err(solver.vcycle_matrix(V0.copy(), F.copy(), op, sm, smoother=smo, **kw), want) < TOL


def test_gram_schmidt_per_level_and_column_shifts_on_the_tiled_level(backend):
    """vcycle_matrix at 128^2 (level 0 on the tile kernels): three columns with their own shifts, Gram-Schmidt on every level"""
    g, lowest, k = 128, 8, 3
    op = tensor_operator(g, "smooth")
    A = op.tocsr()
    solver, sm, ref, rsm = MGCMTSolver(), MGCMTStencilMaker(), RefSolver(), RefStencilMaker()
    F = np.random.RandomState(19).rand(g * g, k)
    kw = dict(nu1=2, nu2=2, shifts=np.array([0.0, 0.35, 0.7]), lowest_level=lowest, dimension="2d")
    want = ref.vcycle_matrix(np.zeros((g * g, k)), F.copy(), A, rsm, **kw)
    got = solver.vcycle_matrix(np.zeros((g * g, k)), F.copy(), op, sm, **kw)
    assert rel_err(got, want) < TOL
    assert get_plan(op, lowest, nvec=k).level_tiled(0)


def test_full_multigrid(backend):
    g = 32
    op = tensor_operator(g, "rough")
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
    """The seam of MGCMTSolver.py:313,326: a callable smoother receives (R A P - shift I) of every level — level 0 assembled
    from the factors plus the nine planes — and the cycle built around it equals the reference's."""
    g, lowest = 32, 4
    op = tensor_operator(g, "rough")
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


# ---- 8. tile against flat -------------------------------------------------------------------------------------------------

def _plan_with(op, lowest, tile, nvec=1):
    """a fresh plan (not the cache's) created with MGCMT_NINE_TILE set: the library reads it at creation"""
    old = os.environ.get("MGCMT_NINE_TILE")
    if tile is None:
        os.environ.pop("MGCMT_NINE_TILE", None)
    else:
        os.environ["MGCMT_NINE_TILE"] = str(tile)
    try:
        return Plan(op, lowest, nvec=nvec)
    finally:
        if old is None:
            os.environ.pop("MGCMT_NINE_TILE", None)
        else:
            os.environ["MGCMT_NINE_TILE"] = old


def _pieces(op, lowest, tile, v0, f, shifts, level=0, tiled_levels=()):
    """per piece the vectors it leaves, all columns: Jacobi sweeps (nu = 1, 2, 3), four-colour sweeps (nu = 1, 2, the second
    over-relaxed), the residual restricted to the next level, and one V(2,2) cycle of either smoother"""
    k = len(shifts)
    p = _plan_with(op, lowest, tile, nvec=k)
    out = {}
    try:
        for l in range(p.num_levels):
            assert p.level_tiled(l) == (l in tiled_levels), (l, tile)
        p.set_shifts(list(shifts))

        def start():
            for q in range(k):
                p.upload(level, _lib.SLOT_V, q, v0[q])
                p.upload(level, _lib.SLOT_F, q, f[q])

        def column(lv, slot):
            return np.stack([np.array(p.download(lv, slot, q)) for q in range(k)])

        for nu in (1, 2, 3):
            start()
            p.smooth(level, _lib.WJACOBI, nu, 2. / 3., k=k)
            out["jacobi nu=%d" % nu] = column(level, _lib.SLOT_V)
        for nu, omega in ((1, 1.0), (2, 1.3)):
            start()
            p.smooth(level, _lib.GS_MC, nu, omega, k=k)
            out["four-colour nu=%d" % nu] = column(level, _lib.SLOT_V)
        start()
        for q in range(k):
            p.upload(level + 1, _lib.SLOT_V, q, np.ones(p.size(level + 1)))
        p.residual_restrict(level, k=k)
        out["restricted residual"] = column(level + 1, _lib.SLOT_F)
        assert not column(level + 1, _lib.SLOT_V).any()
        if level == 0:
            for name, kind, omega in (("jacobi cycle", _lib.WJACOBI, 2. / 3.), ("four-colour cycle", _lib.GS_MC, 1.0)):
                for cyc in range(3):          # (eager, captured, replayed)
                    start()
                    p.vcycle(2, 2, kind, omega=omega, k=k, nu_coarse=2)
                    out["%s %d" % (name, cyc)] = column(0, _lib.SLOT_V)
    finally:
        p.close()
    return out


@pytest.mark.parametrize("g,k", [(128, 3), (256, 1)])
def test_tile_kernels_give_the_bits_of_the_flat_ones(backend, g, k):
    """MGCMT_NINE_TILE = 0 against the default on the same operator: several tiles in both directions, grid edges inside a
    window.  Every sweep, the odd Jacobi sweep behind a pair, and residual + restriction (k_restrict's order) are
    bit-identical per call, with per-column shifts; whole cycles agree to 1e-13 (they are bit-identical too)."""
    release_plans()
    op = tensor_operator(g, "rough")
    rng = np.random.RandomState(g)
    v0, f = rng.rand(k, g * g) - 0.5, rng.rand(k, g * g)
    shifts = (0.7, 0.0, 0.35)[:k]
    flat_form = _pieces(op, 8, 0, v0, f, shifts)
    tiles = _pieces(op, 8, None, v0, f, shifts, tiled_levels=(0,))
    assert sorted(flat_form) == sorted(tiles)
    for name in tiles:
        assert np.all(np.isfinite(tiles[name])), name
        if "cycle" in name:
            assert rel_err(tiles[name], flat_form[name]) < 1e-13, name
        else:
            assert np.array_equal(tiles[name], flat_form[name]), (name, np.abs(tiles[name] - flat_form[name]).max())
    for cyc in (1, 2):
        assert np.array_equal(tiles["jacobi cycle %d" % cyc], tiles["jacobi cycle 0"])
        assert np.array_equal(tiles["four-colour cycle %d" % cyc], tiles["four-colour cycle 0"])
    # and the flat form is right: a sweep and the restricted residual against the assembled matrix
    A = (op.tocsr() - shifts[0] * sp.identity(g * g)).tocsr()
    want = v0[0] + (2. / 3.) * (f[0] - A @ v0[0]) / A.diagonal()
    assert rel_err(tiles["jacobi nu=1"][0], want) < 1e-13
    R = MGCMTStencilMaker().restriction(g, g // 2, dimension="2d")
    assert rel_err(tiles["restricted residual"][0], R @ (f[0] - A @ v0[0])) < 1e-13
    release_plans()


def test_tile_kernels_on_the_galerkin_levels_of_a_potential_plan(backend):
    """MGCMT_NINE_TILE=2: level 1 of a potential_operator plan at 256^2 — a 128^2 nine-plane level over a Kronecker part that
    is NOT a constant 5-point operator (the general-terms form) — takes the tile kernels and gives the bits of the default's
    flat kernels pass by pass; the whole cycle equals the default's to 1e-13."""
    release_plans()
    g, k = 256, 2
    op = potential_operator(g, rough_v(g))
    rng = np.random.RandomState(5)
    n1 = (g // 2) ** 2
    v1, f1 = rng.rand(k, n1) - 0.5, rng.rand(k, n1)
    shifts = (0.7, 0.0)
    default = _pieces(op, 8, None, v1, f1, shifts, level=1)
    tiles = _pieces(op, 8, 2, v1, f1, shifts, level=1, tiled_levels=(1,))
    for name in tiles:
        assert np.array_equal(tiles[name], default[name]), (name, np.abs(tiles[name] - default[name]).max())
    v0, f0 = rng.rand(g * g) - 0.5, rng.rand(g * g)
    cyc = {}
    for tile in (None, 2):
        p = _plan_with(op, 8, tile)
        try:
            assert p.level_tiled(1) == (tile == 2) and not p.level_tiled(0)
            p.set_shifts([0.7])
            for kind, omega in ((_lib.WJACOBI, 2. / 3.), (_lib.GS_MC, 1.0)):
                p.upload(0, _lib.SLOT_V, 0, v0)
                p.upload(0, _lib.SLOT_F, 0, f0)
                p.vcycle(2, 2, kind, omega=omega, k=1, nu_coarse=2)
                cyc[tile, kind] = np.array(p.download(0, _lib.SLOT_V, 0))
        finally:
            p.close()
    for kind in (_lib.WJACOBI, _lib.GS_MC):
        assert rel_err(cyc[2, kind], cyc[None, kind]) < 1e-13
    release_plans()


def test_general_kronecker_part_plus_stencil(backend):
    """a separable potential left in the factors: level 0's Kronecker part is not a constant 5-point operator, so the level
    takes the general-terms form — flat at 32^2 against the oracle, tiled at 128^2 against flat"""
    def general(g):
        base = tensor_operator(g, "rough")
        x = (np.arange(g) + 0.5) / g - 0.5
        Y, X = base.terms[0][1].copy(), base.terms[1][0].copy()
        Y[1] += 20.0 * x * x
        X[1] += 35.0 * (x - 0.1) ** 2
        return StructuredOperator("2d", g, [(tri_identity(g), Y), (X, tri_identity(g))], point_stencil=base.point_stencil)

    g = 32
    op = general(g)
    A = op.tocsr()
    solver, sm, ref, rsm = MGCMTSolver(), MGCMTStencilMaker(), RefSolver(), RefStencilMaker()
    f = np.random.RandomState(14).rand(g * g)
    kw = dict(nu1=2, nu2=2, shift=0.7, lowest_level=4, dimension="2d")
    for smo, rsmo in ((solver.wjacobi, None), (solver.gseidel_rb, rb(ref))):
        want = ref.vcycle(np.zeros(g * g), f.copy(), A, rsm, smoother=rsmo, **kw)
        assert rel_err(solver.vcycle(np.zeros(g * g), f.copy(), op, sm, smoother=smo, **kw), want) < TOL
    g = 128
    op = general(g)
    rng = np.random.RandomState(g)
    v0, f = rng.rand(1, g * g) - 0.5, rng.rand(1, g * g)
    flat_form = _pieces(op, 8, 0, v0, f, (0.7,))
    tiles = _pieces(op, 8, 1, v0, f, (0.7,), tiled_levels=(0,))
    for name in tiles:
        if "cycle" not in name:
            assert np.array_equal(tiles[name], flat_form[name]), name
        assert rel_err(tiles[name], flat_form[name]) < 1e-13, name


# ---- 9. the eigensolver ---------------------------------------------------------------------------------------------------

def test_block_eigensolve_rotated_dot_against_eigsh(backend):
    """The lowest three states of the rough profile with a confining parabola at 32^2 against scipy's eigsh on the assembled
    Hamiltonian (the bar of tests/test_drivers.py)."""
    import scipy.sparse.linalg as sla
    g, k = 32, 3
    X, Y = _centres(g)
    op = tensor_operator(g, "rough", V=60.0 * (X * X + Y * Y))
    assert op.point_stencil is not None
    # lambda_3 = 15.09 has lambda_4 = 15.86 right above it, outside the block, so it converges slowly.  On the emulation 8
    # iterations leave 8e-3, 12 leave 2e-5, 16 leave 4e-8, 20 leave 9e-11, 24 leave 1e-12: 24, two steps past the first that passes
    vals, vecs = drivers.block_eigensolve(op, k=k, cycles=24, lowest=4)
    want = np.sort(sla.eigsh(op.tocsr(), k=k, sigma=0.0, which="LM")[0])
    assert np.allclose(vals, want, rtol=0, atol=1e-8), np.abs(vals - want)
    assert np.abs(vecs.T @ vecs - np.eye(k)).max() < 1e-10


# ---- 10. refused entries --------------------------------------------------------------------------------------------------

def test_refused_entries(backend):
    g = 16
    op = tensor_operator(g, "rough")
    plan = Plan(op, 4, nvec=6)
    lib = _lib.lib()
    h = plan._h
    i6 = (ctypes.c_int * 6)(0, 1, 2, 3, 4, 5)
    i2 = [(ctypes.c_int * 2)(_lib.SLOT_V, q) for q in range(4)]
    out = (ctypes.c_double * 8)()
    calls = {          # the entries of tests/test_point_potential.py::test_unsupported_entries_name_the_point_diagonal
        "gseidel": lambda: lib.mgcmt_smooth(h, 0, _lib.GS_LEX, 1, 1.0, 1, None),
        "sor": lambda: lib.mgcmt_smooth(h, 0, _lib.SOR_LEX, 1, 1.2, 1, None),
        "vcycle lex": lambda: lib.mgcmt_vcycle(h, 0, 2, 2, 2, _lib.GS_LEX, 1.0, 1, 0, None),
        "twogrid": lambda: lib.mgcmt_twogrid(h, 0, 2, 2, _lib.WJACOBI, 2. / 3., 1, None),
        "rqmin": lambda: lib.mgcmt_rqmin(h, 0, _lib.SLOT_V, i6, 2, 0, out, None),
        "rq_line_step": lambda: lib.mgcmt_rq_line_step(h, 0, i2[0], i2[1], i2[2], i2[3], None, 0, -1, None),
        "vcycle_rqmg": lambda: lib.mgcmt_vcycle_rqmg(h, _lib.SLOT_V, i6, 2, 2, 0, out, None),
        "ritz_pair": lambda: lib.mgcmt_ritz_pair(h, 0, _lib.SLOT_V, 0, _lib.SLOT_V, 1, _lib.SLOT_V, 2, out, None),
        "rayleigh_residual": lambda: lib.mgcmt_rayleigh_residual(h, 0, _lib.SLOT_V, 1, out, out, None),
        "comm_init": lambda: lib.mgcmt_comm_init(h, 0, 1, ctypes.create_string_buffer(_lib.UNIQUE_ID_BYTES)),
        "comm_init_external": lambda: lib.mgcmt_comm_init_external(
            h, 0, 1, _lib.P2P_FN(lambda *a: 0), _lib.ALLGATHER_FN(lambda *a: 0), _lib.ALLREDUCE_FN(lambda *a: 0), None),
        "sharded_vcycle": lambda: lib.mgcmt_sharded_vcycle(h, h, 2, 2, 2, _lib.WJACOBI, 2. / 3., 1, 0, None),
    }
    try:
        for name, call in calls.items():
            assert call() == -4, name          # MGCMT_ERR_UNSUPPORTED
            assert b"point diagonal" in lib.mgcmt_last_error(), (name, lib.mgcmt_last_error())
        for kind in (_lib.WJACOBI, _lib.GS_MC):
            assert plan.fused_max_sweeps(0, kind) == 0
        assert lib.mgcmt_fused_pass(h, 0, _lib.WJACOBI, 1, 2. / 3., 0, 1, None) == -4
        # creation: no mass operator, no strips, 2-D only, zero towards the outside, symmetric, no null array
        nterms, xfac, yfac = op.factor_blocks()
        desc = _lib.PlanDesc()
        desc.dim, desc.nterms, desc.g, desc.lowest, desc.nvec = 2, nterms, g, 4, 1
        desc.xfac, desc.yfac = _lib.as_dp(xfac), _lib.as_dp(yfac)
        G = np.ascontiguousarray(op.point_stencil)
        dp = _lib.as_dp
        hh = ctypes.c_void_p()
        desc.row_begin, desc.row_end, desc.strip_levels = 0, g // 2, 1
        assert lib.mgcmt_plan_create_nine(ctypes.byref(desc), dp(G), ctypes.byref(hh)) == -4
        desc.row_begin, desc.row_end, desc.strip_levels = 0, 0, 0
        desc.m_nterms, desc.m_xfac, desc.m_yfac = nterms, dp(xfac), dp(yfac)
        assert lib.mgcmt_plan_create_nine(ctypes.byref(desc), dp(G), ctypes.byref(hh)) == -4
        desc.m_nterms = 0
        assert lib.mgcmt_plan_create_nine(ctypes.byref(desc), None, ctypes.byref(hh)) == -1
        assert lib.mgcmt_plan_create_nine(None, dp(G), ctypes.byref(hh)) == -1
        assert lib.mgcmt_plan_create_nine(ctypes.byref(desc), dp(G), None) == -1
        for (a, b, ii, jj) in ((0, 0, 0, 5), (2, 1, g - 1, 3), (1, 2, 3, g - 1), (0, 0, 4, 0)):
            bad = G.copy()
            bad[a, b][ii, jj] = 1.0
            assert lib.mgcmt_plan_create_nine(ctypes.byref(desc), dp(bad), ctypes.byref(hh)) == -1, (a, b)
            assert b"outside" in lib.mgcmt_last_error()
        bad = G.copy()
        bad[2, 0][3, 3] += 0.5
        assert lib.mgcmt_plan_create_nine(ctypes.byref(desc), dp(bad), ctypes.byref(hh)) == -1
        assert b"symmetric" in lib.mgcmt_last_error()
        desc.dim = 1
        assert lib.mgcmt_plan_create_nine(ctypes.byref(desc), dp(G), ctypes.byref(hh)) == -1
        desc.dim = 2
        assert lib.mgcmt_plan_create_nine(ctypes.byref(desc), dp(G), ctypes.byref(hh)) == 0          # and the untouched one is taken
        lib.mgcmt_plan_destroy(hh)
        t = ctypes.c_int(7)
        assert lib.mgcmt_plan_level_tiled(h, 0, ctypes.byref(t)) == 0 and t.value == 0
        assert lib.mgcmt_plan_level_tiled(h, 99, ctypes.byref(t)) == -1
        assert lib.mgcmt_plan_level_tiled(h, 0, None) == -1
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
    with pytest.raises(ValueError, match="point stencil"):
        Plan(op, 4, mass=identity_operator(g, "2d"))
    with pytest.raises(ValueError, match="point stencil"):
        Plan(op, 4, row_begin=0, row_end=g // 2, strip_levels=1)
    # a random matrix that is no 9-point operator is still refused by the 2-D entry points, with recognise's error
    bad = sp.random(g * g, g * g, density=0.02, random_state=1, format="csr") + sp.identity(g * g)
    with pytest.raises(UnrecognisedOperator):
        solver.vcycle(v0.copy(), f.copy(), bad, sm, dimension="2d", lowest_level=4)
