"""Arbitrary potentials V(x, y, z): 3-D operators with a per-point diagonal (operators.potential_operator(..., "3d") /
recognise_potential(A, "3d"), mgcmt_plan_create3d_pot) against the NumPy oracle (Ref3dSolver of tests/test_3d_cycle.py, which
cycles any sparse matrix) and against scipy's own R*A*P, through the HIP library on the GPU box and through the emulated
kernels on CPU (``backend`` fixture).

The fine level of such a plan — constant 7-point Kronecker part plus the diagonal — runs the marching kernels of
csrc/kernels_3d_point.hip from 64^3 on (the flat ones below, or with MGCMT_3D_POINT_MARCH=0), the 27-plane Galerkin levels its
flat kernels (DESIGN par. 4.14)."""
import ctypes
import math

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import rel_err
from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, _lib, drivers
from multigridcmt_amd.operators import (StructuredOperator, UnrecognisedOperator, planes_to_csr, potential_operator, recognise,
                                        recognise_potential, tri_identity, tri_laplacian, tri_to_sparse)
from multigridcmt_amd.plan import Plan, get_plan
from test_3d_cycle import Ref3dSolver, Ref3dStencilMaker, mc_3d

TOL = 1e-10          # the bar of tests/test_3d_cycle.py
SCALE = -1 / np.pi ** 2


@pytest.fixture(autouse=True, scope="module")
def _release_host_buffers():
    yield
    import gc
    from multigridcmt_amd import hostmem
    gc.collect()
    hostmem.drain()


def smooth_v(g):
    """40 (x^2 + x y + y z + z^2) + 10 exp(-12 (x - y)^2) on the cell centres of [-1/2, 1/2]^3, index [z, y, x]: smooth,
    non-negative and not additively separable"""
    t = (np.arange(g) + 0.5) / g - 0.5
    Z, Y, X = np.meshgrid(t, t, t, indexing="ij")
    return 40.0 * (X * X + X * Y + Y * Z + Z * Z) + 10.0 * np.exp(-12.0 * (X - Y) ** 2)


def rough_v(g, seed=1):
    """the same plus disorder: 5 * uniform noise per point"""
    return smooth_v(g) + 5.0 * np.random.RandomState(seed).rand(g, g, g)


def hamiltonian(g, V):
    """(-1/pi^2) laplacian(g, '3d') + diag(V) as a caller would assemble it"""
    return (SCALE * MGCMTStencilMaker().laplacian(g, dimension="3d") + sp.diags(np.asarray(V).reshape(-1))).tocsr()


def flat(a):
    return np.asarray(a).reshape(-1)


def stencil_matrix(G):
    """the sparse matrix of 27 planes G[a, b, c, z, y, x] (operators.planes_to_csr, which the foreign-smoother seam uses too);
    asserts that nothing points outside the grid"""
    gl = G.shape[-1]
    z, y, x = np.meshgrid(np.arange(gl), np.arange(gl), np.arange(gl), indexing="ij")
    for a in range(3):
        for b in range(3):
            for c in range(3):
                zz, yy, xx = z + a - 1, y + b - 1, x + c - 1
                ok = (zz >= 0) & (zz < gl) & (yy >= 0) & (yy < gl) & (xx >= 0) & (xx < gl)
                assert not G[a, b, c][~ok].view(np.uint64).any(), (a, b, c)          # exact zeros (+0.0) towards outside points
    return planes_to_csr(G)


def assemble_level(plan, level):
    """the matrix of `level`: Kronecker factors (mgcmt_plan_get_factors) plus the per-point part (mgcmt_plan_get_point_stencil)"""
    gl = plan.g >> level
    fs = [plan.factors(level, w) for w in range(3)]
    A = sum(sp.kron(tri_to_sparse(fs[0][m]), sp.kron(tri_to_sparse(fs[1][m]), tri_to_sparse(fs[2][m]), format="csr"), format="csr")
            for m in range(fs[0].shape[0])).tocsr()
    G = plan.point_stencil(level)
    if level == 0:
        assert G.shape == (gl, gl, gl)
        return (A + sp.diags(G.reshape(-1))).tocsr()
    assert G.shape == (3, 3, 3, gl, gl, gl)
    return (A + stencil_matrix(G)).tocsr()


def galerkin_chain(A, g, lowest):
    """[A, R A P, R (R A P) P, ...] down to lowest^3 points with MGCMTStencilMaker's own 3-D matrices"""
    sm = MGCMTStencilMaker()
    out = [sp.csr_matrix(A)]
    while g > lowest:
        R = sm.restriction(g, g // 2, dimension="3d")
        P = sm.interpolation(g // 2, g, dimension="3d")
        out.append((R @ out[-1] @ P).tocsr())
        g //= 2
    return out


# ---- host ----------------------------------------------------------------------------------------------------------------

def test_recognise_potential_3d_round_trip():
    g = 8
    for name, V in (("smooth", smooth_v(g)), ("random", np.random.RandomState(3).rand(g, g, g) * 30.0), ("zero", np.zeros((g, g, g)))):
        A = hamiltonian(g, V)
        op = recognise_potential(A, "3d")
        assert op.dimension == "3d" and abs(op.tocsr() - A).max() <= 1e-13 * abs(A).max(), name
        if name == "zero":
            assert op.point_diagonal is None and op is recognise(A, "3d")      # what recognise returns today
        else:
            assert op.point_diagonal is not None and op.point_diagonal.shape == (g, g, g)
            for t in op.terms:          # the median went into the Kronecker part: its factors stay Toeplitz
                for fac in t:
                    assert np.all(fac[1] == fac[1][0])
            with pytest.raises(UnrecognisedOperator):
                recognise(A, "3d")
    # a separable diagonal stays with recognise's Kronecker terms
    a = np.random.RandomState(4).rand(g)
    sep = a[:, None, None] + 2.0 * a[None, :, None] + 0.5 * a[None, None, :]
    A = hamiltonian(g, sep)
    assert recognise_potential(A, "3d").point_diagonal is None and recognise_potential(A, "3d") is recognise(A, "3d")
    # one entry off the seven bands: still refused
    B = sp.lil_matrix(hamiltonian(g, smooth_v(g)))
    B[5, 5 + 2] = 0.25
    with pytest.raises(UnrecognisedOperator):
        recognise_potential(B.tocsr(), "3d")
    # an x-band that depends on y as well: refused
    C = sp.lil_matrix(hamiltonian(g, smooth_v(g)))
    C[g + 1, g + 2] *= 1.5
    with pytest.raises(UnrecognisedOperator):
        recognise_potential(C.tocsr(), "3d")


def test_operator_algebra_carries_the_point_diagonal_3d():
    g = 8
    V = rough_v(g)
    op = potential_operator(g, V, dimension="3d")
    A = hamiltonian(g, V)
    tol = 1e-13 * abs(A).max()
    assert op.point_diagonal.shape == (g, g, g)
    assert abs(op.tocsr() - A).max() <= tol
    assert abs(potential_operator(g, V.reshape(-1), dimension="3d").tocsr() - A).max() <= tol          # g^3 values
    assert np.allclose(op.diagonal(), A.diagonal(), rtol=1e-14)
    assert abs((op * 2.5).tocsr() - 2.5 * A).max() <= tol
    assert abs((2.5 * op).tocsr() - 2.5 * A).max() <= tol
    assert abs((-op / 4.0).tocsr() + A / 4.0).max() <= tol
    assert abs(op.shifted(0.7).tocsr() - (A - 0.7 * sp.identity(g ** 3))).max() <= tol
    assert op.fingerprint() != potential_operator(g, V + 1e-9, dimension="3d").fingerprint()
    assert op.fingerprint() != potential_operator(g, np.zeros((g, g, g)), dimension="3d").fingerprint()
    with pytest.raises(ValueError):
        potential_operator(g, np.zeros((g, g)), dimension="3d")
    with pytest.raises(ValueError):
        StructuredOperator("1d", g, [(None, np.zeros((3, g)))], point_diagonal=np.zeros(g))
    assert potential_operator(g, np.zeros((g, g))).dimension == "2d"          # the default is unchanged


# ---- hierarchy -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g,lowest", [(8, 2), (16, 2), (16, 4)])
def test_galerkin_hierarchy_and_apply_on_every_level_3d(backend, g, lowest):
    """R*A*P of every level — Kronecker factors plus mgcmt_plan_get_point_stencil — against scipy's product of
    MGCMTStencilMaker's own 3-D matrices, and mgcmt_apply on every level against that matrix (with and without the shift)."""
    V = rough_v(g)
    plan = Plan(potential_operator(g, V, dimension="3d"), lowest, nvec=1)
    try:
        chain = galerkin_chain(hamiltonian(g, V), g, lowest)
        assert plan.num_levels == len(chain)
        plan.set_shifts([0.7])
        rng = np.random.RandomState(g)
        for level, want in enumerate(chain):
            assert plan.level_path_3d(level) == ((_lib.PATH3D_SEVEN_POINT if level == 0 else _lib.PATH3D_PLANES), False)
            got = assemble_level(plan, level)
            assert abs(got - want).max() <= 1e-13 * abs(want).max(), level
            x = rng.rand(want.shape[0]) - 0.5
            plan.upload(level, _lib.SLOT_V, 0, x)
            plan.apply(level, (_lib.SLOT_V, 0), (_lib.SLOT_T, 0))
            assert rel_err(plan.download(level, _lib.SLOT_T, 0), want @ x) < 1e-13, level
            plan.apply(level, (_lib.SLOT_V, 0), (_lib.SLOT_T, 0), with_shift=True)
            assert rel_err(plan.download(level, _lib.SLOT_T, 0), want @ x - 0.7 * x) < 1e-13, level
    finally:
        plan.close()
    op = potential_operator(8, rough_v(8), dimension="3d")          # A.dot(x) of the operator object
    x = np.random.RandomState(2).rand(512)
    assert rel_err(op.dot(x), op.tocsr() @ x) < 1e-13


def test_smoothers_stand_alone_3d(backend):
    g = 16
    V = rough_v(g)
    A, op = hamiltonian(g, V), potential_operator(g, V, dimension="3d")
    solver, ref = MGCMTSolver(), Ref3dSolver()
    rng = np.random.RandomState(6)
    v0, f = rng.rand(g ** 3), rng.rand(g ** 3)
    want = ref.wjacobi(v0.copy(), f.copy(), A, nu=3)
    assert rel_err(flat(solver.wjacobi(v0.copy(), f.copy(), op, nu=3)), flat(want)) < TOL
    assert rel_err(flat(solver.smooth(v0.copy(), f.copy(), A, nu=3, smoother=solver.wjacobi, dimension="3d")), flat(want)) < TOL
    want = mc_3d(v0, f, A, nu=2)
    assert rel_err(flat(solver.gseidel_rb(v0.copy(), f.copy(), A, nu=2, dimension="3d")), want) < TOL
    assert rel_err(flat(solver.gseidel_rb(v0.copy(), f.copy(), op, nu=2, dimension="3d")), want) < TOL
    want = mc_3d(v0, f, A, nu=2, omega=1.3)
    assert rel_err(flat(solver.gseidel_rb(v0.copy(), f.copy(), op, nu=2, omega=1.3, dimension="3d")), want) < TOL


# ---- a Kronecker part that is not the constant 7-point operator, plus a point diagonal --------------------------------------

def mixed_operator(g):
    """a separable potential a(z) + b(x) kept in the (then non-Toeplitz) factors and a non-separable remainder as the point
    diagonal: level 0 is "general terms + point diagonal" (kind 4), whose flat kernels must add D to A v as well as to a_ii"""
    t = (np.arange(g) + 0.5) / g - 0.5
    i, L = tri_identity(g), tri_laplacian(g) * SCALE
    Lz, Lx = L.copy(), L.copy()
    Lz[1] += 25.0 * t * t + np.random.RandomState(7).rand(g)
    Lx[1] += 6.0 * np.cos(3.0 * t) + 6.0
    return StructuredOperator("3d", g, [(i, i.copy(), Lx), (i.copy(), L.copy(), i.copy()), (Lz, i.copy(), i.copy())], point_diagonal=rough_v(g))


@pytest.mark.parametrize("g,lowest", [(8, 2), (16, 4)])
def test_general_terms_plus_point_diagonal_3d(backend, g, lowest):
    """every level's matrix and apply, both smoothers stand-alone and a V(2,2) cycle with each, against the assembled matrix"""
    op = mixed_operator(g)
    A = op.tocsr()
    n = g ** 3
    plan = Plan(op, lowest, nvec=1)
    try:
        chain = galerkin_chain(A, g, lowest)
        plan.set_shifts([0.7])
        rng = np.random.RandomState(g)
        for level, want in enumerate(chain):
            assert plan.level_path_3d(level) == ((_lib.PATH3D_GENERAL_POINT if level == 0 else _lib.PATH3D_PLANES), False)
            assert abs(assemble_level(plan, level) - want).max() <= 1e-13 * abs(want).max(), level
            x = rng.rand(want.shape[0]) - 0.5
            plan.upload(level, _lib.SLOT_V, 0, x)
            plan.apply(level, (_lib.SLOT_V, 0), (_lib.SLOT_T, 0))
            assert rel_err(plan.download(level, _lib.SLOT_T, 0), want @ x) < 1e-13, level
            plan.apply(level, (_lib.SLOT_V, 0), (_lib.SLOT_T, 0), with_shift=True)
            assert rel_err(plan.download(level, _lib.SLOT_T, 0), want @ x - 0.7 * x) < 1e-13, level
    finally:
        plan.close()
    solver, ref = MGCMTSolver(), Ref3dSolver()
    rng = np.random.RandomState(6)
    v0, f = rng.rand(n), rng.rand(n)
    assert rel_err(flat(solver.wjacobi(v0.copy(), f.copy(), op, nu=3)), flat(ref.wjacobi(v0.copy(), f.copy(), A, nu=3))) < TOL
    assert rel_err(flat(solver.gseidel_rb(v0.copy(), f.copy(), op, nu=2, dimension="3d")), mc_3d(v0, f, A, nu=2)) < TOL
    for ours, theirs in ((None, None), (solver.gseidel_rb, mc_3d)):
        kw = dict(nu1=2, nu2=2, shift=0.7, lowest_level=lowest, dimension="3d")
        y = ref.vcycle(v0.copy(), f.copy(), A, Ref3dStencilMaker(), smoother=theirs, **kw)
        assert np.linalg.norm(f - (A @ y - 0.7 * y)) < np.linalg.norm(f - (A @ v0 - 0.7 * v0))
        for _ in range(2):
            assert rel_err(solver.vcycle(v0.copy(), f.copy(), op, MGCMTStencilMaker(), smoother=ours, **kw), y) < TOL


# ---- cycles ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("potential", ["smooth", "rough"])
@pytest.mark.parametrize("smoother", ["wjacobi", "gseidel_rb"])
@pytest.mark.parametrize("shift", [0.0, 1.9])
@pytest.mark.parametrize("g,lowest", [(8, 2), (8, 4), (16, 4), (32, 8), (64, 8)])
def test_vcycle_3d_point_vs_oracle(backend, g, lowest, shift, smoother, potential):
    """V(2,2) for (H - shift I) v = f, H = -laplacian/pi^2 + V (H > 2: the shifted operator is definite on every level).
    64^3 is the smallest grid on which the marching kernels run (two z-chunks): asserted through mgcmt_plan3d_level_path."""
    V = smooth_v(g) if potential == "smooth" else rough_v(g)
    A, op = hamiltonian(g, V), potential_operator(g, V, dimension="3d")
    solver, ref = MGCMTSolver(), Ref3dSolver()
    ours, theirs = (None, None) if smoother == "wjacobi" else (solver.gseidel_rb, mc_3d)
    n = g ** 3
    f = np.random.RandomState(g + lowest).rand(n)
    kw = dict(nu1=2, nu2=2, shift=shift, lowest_level=lowest, dimension="3d")
    y = ref.vcycle(np.zeros(n), f.copy(), A, Ref3dStencilMaker(), smoother=theirs, **kw)
    assert np.linalg.norm(f - (A @ y - shift * y)) < np.linalg.norm(f)          # the oracle's own residual falls
    x = solver.vcycle(np.zeros(n), f.copy(), op, MGCMTStencilMaker(), smoother=ours, **kw)
    assert x.shape == (n,)
    assert rel_err(x, y) < TOL
    if g <= 16:          # the assembled matrix through recognise_potential inside the 3-D entry point
        assert rel_err(solver.vcycle(np.zeros(n), f.copy(), A, MGCMTStencilMaker(), smoother=ours, **kw), y) < TOL
    if g == 64:
        plan = get_plan(op, lowest, nvec=1)
        assert plan.level_path_3d(0) == (_lib.PATH3D_SEVEN_POINT, True)
        assert plan.level_path_3d(1) == (_lib.PATH3D_PLANES, False)


@pytest.mark.parametrize("smoother", ["wjacobi", "gseidel_rb"])
def test_vcycle_3d_point_nonzero_start_and_repeat(backend, smoother):
    # a non-zero start vector, and the same call three times (the second captures the cycle's graph, the third replays it)
    g = 16
    V = rough_v(g)
    A, op = hamiltonian(g, V), potential_operator(g, V, dimension="3d")
    rng = np.random.RandomState(2)
    f, v0 = rng.rand(g ** 3), rng.rand(g ** 3)
    solver, ref = MGCMTSolver(), Ref3dSolver()
    ours, theirs = (None, None) if smoother == "wjacobi" else (solver.gseidel_rb, mc_3d)
    kw = dict(nu1=2, nu2=2, shift=0.7, lowest_level=4, dimension="3d")
    y = ref.vcycle(v0.copy(), f.copy(), A, Ref3dStencilMaker(), smoother=theirs, **kw)
    for _ in range(3):
        assert rel_err(solver.vcycle(v0.copy(), f.copy(), op, MGCMTStencilMaker(), smoother=ours, **kw), y) < TOL


@pytest.mark.parametrize("smoother", ["wjacobi", "gseidel_rb"])
def test_vcycle_matrix_3d_point_with_column_shifts(backend, smoother):
    g, k = 16, 3
    V = rough_v(g)
    A, op = hamiltonian(g, V), potential_operator(g, V, dimension="3d")
    n = g ** 3
    F = np.random.RandomState(5).rand(n, k)
    shifts = np.array([0.0, 0.9, 1.9])
    solver, ref = MGCMTSolver(), Ref3dSolver()
    ours, theirs = (None, None) if smoother == "wjacobi" else (solver.gseidel_rb, mc_3d)
    kw = dict(nu1=2, nu2=2, shifts=shifts, lowest_level=4, dimension="3d")
    y = ref.vcycle_matrix(np.zeros((n, k)), F.copy(), A, Ref3dStencilMaker(), smoother=theirs, **kw)
    for start in (op, A):
        x = solver.vcycle_matrix(np.zeros((n, k)), F.copy(), start, MGCMTStencilMaker(), smoother=ours, **kw)
        assert x.shape == (n, k)
        assert rel_err(x, y) < TOL


def test_foreign_smoother_sees_the_level_matrices_3d(backend):
    """A callable smoother receives (R A P - shift I) of every level, the 27-plane levels included."""
    g, lowest = 16, 4
    V = rough_v(g)
    A, op = hamiltonian(g, V), potential_operator(g, V, dimension="3d")
    chain = galerkin_chain(A, g, lowest)
    seen = {}

    def damped(v, f, M, nu=4):
        M = sp.csr_matrix(M)
        seen[M.shape[0]] = M
        v, f = np.asarray(v, dtype=float).reshape(-1).copy(), np.asarray(f, dtype=float).reshape(-1)
        for _ in range(nu):
            v = v + 0.6 * (f - M @ v) / M.diagonal()
        return v.reshape(-1, 1)

    f = np.random.RandomState(12).rand(g ** 3)
    kw = dict(nu1=2, nu2=2, smoother=damped, shift=0.7, lowest_level=lowest, dimension="3d")
    got = MGCMTSolver().vcycle(np.zeros(g ** 3), f.copy(), op, MGCMTStencilMaker(), **kw)
    assert sorted(seen) == [8 ** 3, 16 ** 3]
    for level, want in enumerate(chain[:-1]):
        M = seen[want.shape[0]]
        assert abs(M - (want - 0.7 * sp.identity(want.shape[0]))).max() <= 1e-13 * abs(want).max(), level
    want = Ref3dSolver().vcycle(np.zeros(g ** 3), f.copy(), A, Ref3dStencilMaker(), **kw)
    assert rel_err(got, want) < TOL


# ---- marching against flat ---------------------------------------------------------------------------------------------------

def _forms(monkeypatch, op, lowest, run):
    """run(plan) on a plan created with the marching kernels (the default) and with MGCMT_3D_POINT_MARCH=0"""
    out = []
    for march in (True, False):
        if march:
            monkeypatch.delenv("MGCMT_3D_POINT_MARCH", raising=False)
        else:
            monkeypatch.setenv("MGCMT_3D_POINT_MARCH", "0")
        p = Plan(op, lowest, nvec=2)
        try:
            assert p.level_path_3d(0) == (_lib.PATH3D_SEVEN_POINT, march)
            out.append(run(p))
        finally:
            p.close()
    return out


def test_marching_and_flat_forms_agree_64(backend, monkeypatch):
    """One Jacobi sweep, one red-black sweep and one V(2,2) cycle at 64^3 with MGCMT_3D_POINT_MARCH=0 against the default.
    Both forms compute a point with the same inline functions: the sweeps agree bit for bit; the cycle's restriction sums
    in another order: 1e-13 relative."""
    g = 64
    op = potential_operator(g, rough_v(g), dimension="3d")
    rng = np.random.RandomState(64)
    v0, f = rng.rand(2, g ** 3), rng.rand(2, g ** 3)
    V, F = _lib.SLOT_V, _lib.SLOT_F

    def run(p):
        p.set_shifts([0.0, 1.9])
        res = []
        for kind, omega in ((_lib.WJACOBI, 2. / 3.), (_lib.GS_MC, 1.0), (_lib.GS_MC, 1.3)):
            for q in range(2):
                p.upload(0, V, q, v0[q])
                p.upload(0, F, q, f[q])
            p.smooth(0, kind, 1, omega=omega, k=2)
            res.append(np.stack([np.array(p.download(0, V, q)) for q in range(2)]))
        for kind, omega in ((_lib.WJACOBI, 2. / 3.), (_lib.GS_MC, 1.0)):
            for q in range(2):
                p.upload(0, V, q, v0[q])
                p.upload(0, F, q, f[q])
            p.vcycle(2, 2, kind, omega=omega, k=2, nu_coarse=2)
            res.append(np.stack([np.array(p.download(0, V, q)) for q in range(2)]))
        return res

    march, flat_ = _forms(monkeypatch, op, 8, run)
    for i in range(3):
        assert np.array_equal(march[i], flat_[i]), i
    for i in (3, 4):
        assert rel_err(march[i], flat_[i]) < 1e-13, i


# ---- eigenpairs ------------------------------------------------------------------------------------------------------------

def two_dots(g):
    """two overlapping spherical dots of different depth in a barrier of height 60, index [z, y, x]"""
    t = (np.arange(g) + 0.5) / g
    Z, Y, X = np.meshgrid(t, t, t, indexing="ij")
    V = 60.0 - 60.0 * ((X - 0.38) ** 2 + (Y - 0.42) ** 2 + (Z - 0.45) ** 2 < 0.24 ** 2) \
        - 45.0 * ((X - 0.66) ** 2 + (Y - 0.60) ** 2 + (Z - 0.55) ** 2 < 0.2 ** 2)
    return np.maximum(V, 0.0)


def test_block_eigensolve_two_spherical_dots_against_eigsh(backend):
    import scipy.sparse.linalg as sla
    g, k = 16, 3
    op = potential_operator(g, two_dots(g), dimension="3d")
    with pytest.raises(UnrecognisedOperator):
        recognise(op.tocsr(), "3d")
    vals, vecs = drivers.block_eigensolve(op, k=k, cycles=24, lowest=4)          # (the third state lies close to the second: 16 iterations leave 1.4e-8)
    want = np.sort(sla.eigsh(op.tocsr(), k=k, sigma=0.0, which="LM")[0])
    assert np.allclose(vals, want, rtol=0, atol=1e-8), np.abs(vals - want)
    assert np.abs(vecs.T @ vecs - np.eye(k)).max() < 1e-10


# ---- what stays unsupported ----------------------------------------------------------------------------------------------------

def test_unsupported_entries_on_a_3d_point_plan(backend):
    g = 8
    op = potential_operator(g, rough_v(g), dimension="3d")
    plan = Plan(op, 2, nvec=6)
    L, h = _lib.lib(), plan._h
    U = -4  # MGCMT_ERR_UNSUPPORTED
    vecs = (ctypes.c_int * 6)(0, 1, 2, 3, 4, 5)
    pair = (ctypes.c_int * 2)(0, 0)
    dbl = ctypes.c_double(0.0)
    i = ctypes.c_int(0)
    out = np.zeros(8)
    dp = _lib.as_dp(out)
    calls = {
        "twogrid": lambda: L.mgcmt_twogrid(h, 0, 2, 2, _lib.WJACOBI, ctypes.c_double(1.0), 1, None),
        "rayleigh_residual": lambda: L.mgcmt_rayleigh_residual(h, 0, 0, 1, dp, dp, None),
        "ritz_pair": lambda: L.mgcmt_ritz_pair(h, 0, 0, 0, 1, 0, 2, 0, dp, None),
        "rqmin": lambda: L.mgcmt_rqmin(h, 0, 0, vecs, 2, 0, ctypes.byref(dbl), None),
        "rq_line_step": lambda: L.mgcmt_rq_line_step(h, 0, pair, None, pair, pair, None, 0, -1, None),
        "rq_history": lambda: L.mgcmt_rq_history(h, 0, 1, dp, None),
        "vcycle_rqmg": lambda: L.mgcmt_vcycle_rqmg(h, 0, vecs, 2, 2, 0, ctypes.byref(dbl), None),
        "fused_pass": lambda: L.mgcmt_fused_pass(h, 0, _lib.WJACOBI, 1, ctypes.c_double(1.0), 0, 1, None),
        "fused_max_sweeps": lambda: L.mgcmt_fused_max_sweeps(h, 0, _lib.WJACOBI, ctypes.byref(i)),
        "fused_max_recompute": lambda: L.mgcmt_fused_max_recompute(h, 0, _lib.WJACOBI, 2, ctypes.byref(i)),
        "level_operator_kind": lambda: L.mgcmt_level_operator_kind(h, 0, ctypes.byref(i)),
        "time_smoother": lambda: L.mgcmt_time_smoother(h, 0, _lib.WJACOBI, 1, ctypes.c_double(1.0), 1, ctypes.byref(dbl), None),
        "time_fused_pass": lambda: L.mgcmt_time_fused_pass(h, 0, _lib.WJACOBI, 1, ctypes.c_double(1.0), 0, 1, ctypes.byref(dbl), None),
        "bandwidth_probe": lambda: L.mgcmt_bandwidth_probe(h, 0, 0, 1, 1, ctypes.byref(dbl), None),
        "comm_init_external": lambda: L.mgcmt_comm_init_external(h, 0, 1, _lib.P2P_FN(0), _lib.ALLGATHER_FN(0), _lib.ALLREDUCE_FN(0), None),
        "comm_set_option": lambda: L.mgcmt_comm_set_option(h, 0, 1),
        "halo_exchange": lambda: L.mgcmt_halo_exchange(h, 0, 1, None),
        "allreduce_sum": lambda: L.mgcmt_allreduce_sum(h, dp, 1, None),
        "sharded_vcycle": lambda: L.mgcmt_sharded_vcycle(h, h, 2, 2, 2, _lib.WJACOBI, ctypes.c_double(1.0), 1, 0, None),
        "gather_coarse": lambda: L.mgcmt_gather_coarse(h, 0, 0, h, 0, 1, None),
        "smooth_lex": lambda: L.mgcmt_smooth(h, 0, _lib.GS_LEX, 1, ctypes.c_double(1.0), 1, None),
        "smooth_sor": lambda: L.mgcmt_smooth(h, 0, _lib.SOR_LEX, 1, ctypes.c_double(1.5), 1, None),
        "vcycle_lex": lambda: L.mgcmt_vcycle(h, 0, 2, 2, 2, _lib.GS_LEX, ctypes.c_double(1.0), 1, 0, None),
    }
    try:
        for name, call in calls.items():
            assert call() == U, name
            msg = L.mgcmt_last_error()
            assert b"3-D" in msg or b"point diagonal" in msg, (name, msg)
        unique = ctypes.create_string_buffer(_lib.UNIQUE_ID_BYTES)
        assert L.mgcmt_comm_init(h, 0, 1, unique) == U
        assert L.mgcmt_apply(h, _lib.OP_M, 0, 0, 0, 2, 0, 0, None) != 0          # there is no mass operator
        assert math.isfinite(dbl.value)
        # creation: a NULL diagonal and lowest > 16 fail cleanly
        nterms, zfac, yfac, xfac = op.factor_blocks()
        desc = _lib.Plan3dDesc()
        desc.nterms, desc.nvec, desc.g, desc.lowest = nterms, 1, 32, 8
        desc.zfac, desc.yfac, desc.xfac = _lib.as_dp(zfac), _lib.as_dp(yfac), _lib.as_dp(xfac)
        hh = ctypes.c_void_p()
        assert L.mgcmt_plan_create3d_pot(ctypes.byref(desc), None, ctypes.byref(hh)) == -1 and not hh.value
        desc.lowest = 32
        pd = np.zeros(32 ** 3)
        assert L.mgcmt_plan_create3d_pot(ctypes.byref(desc), _lib.as_dp(pd), ctypes.byref(hh)) == -1 and not hh.value
        assert b"16" in L.mgcmt_last_error()
    finally:
        plan.close()
    from multigridcmt_amd.operators import identity_operator, laplacian_operator
    plain = Plan(laplacian_operator(g, "3d"), 2)          # a 3-D plan without a point part has no point stencil
    try:
        assert L.mgcmt_plan_get_point_stencil(plain._h, 0, dp, 8) == -1
        assert plain.level_path_3d(0) == (_lib.PATH3D_SEVEN, False) and plain.level_path_3d(1) == (_lib.PATH3D_GENERAL, False)
    finally:
        plain.close()
    # Python: the lexicographic smoothers raise, naming what is supported; a mass operator is refused
    solver, sm = MGCMTSolver(), MGCMTStencilMaker()
    v0, f = np.zeros(g ** 3), np.ones(g ** 3)
    A = hamiltonian(g, rough_v(g))
    for bad in (solver.gseidel, solver.sor):
        for start in (op, A):
            with pytest.raises(ValueError, match="wjacobi"):
                solver.vcycle(v0.copy(), f.copy(), start, sm, smoother=bad, dimension="3d", lowest_level=2)
        with pytest.raises(ValueError, match="wjacobi"):
            solver.vcycle_matrix(np.zeros((g ** 3, 2)), np.ones((g ** 3, 2)), op, sm, smoother=bad, dimension="3d", lowest_level=2)
    with pytest.raises(ValueError, match="wjacobi, gseidel_rb"):
        solver.gseidel(v0.copy(), f.copy(), op)
    with pytest.raises(ValueError, match="point diagonal"):
        Plan(op, 2, nvec=10, mass=identity_operator(g, "3d"))
    with pytest.raises(ValueError, match="point diagonal"):
        solver.vcycle_rqmg(np.ones(g ** 3), op, identity_operator(g, "3d"))
