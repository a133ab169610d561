"""Variable effective mass in 3-D: operators with per-point bonds on g^3 grids (StructuredOperator(..., point_bonds=(Bx, By, Bz)),
operators.variable_mass_operator(..., dimension="3d"), recognise_seven_point, mgcmt_plan_create3d_bonds) against the NumPy
oracle (Ref3dSolver of tests/test_3d_cycle.py, which cycles any sparse matrix) and against scipy's own R*A*P, through the HIP
library on the GPU box and through the emulated kernels on CPU (``backend`` fixture).

Level 0 of such a plan keeps four planes D, Bx, By, Bz.  With a constant 7-point Kronecker part it runs the marching kernels
k3pm_*<BONDS = true> of csrc/kernels_3d_point.hip from 64^3 on (that file's flat ones below, or with MGCMT_3D_POINT_MARCH=0);
the levels below are the 27-plane levels of a point-diagonal plan (DESIGN par. 4.16)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import rel_err
from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, _lib, drivers
from multigridcmt_amd.operators import (StructuredOperator, UnrecognisedOperator, identity_operator, recognise, recognise_potential,
                                        recognise_seven_point, tri_identity, tri_to_sparse, variable_mass_operator)
from multigridcmt_amd.plan import Plan, get_plan
from test_3d_cycle import Ref3dSolver, Ref3dStencilMaker, mc_3d
from test_3d_point_potential import galerkin_chain, stencil_matrix

TOL = 1e-10          # the bar of tests/test_3d_cycle.py
SCALE = -1 / np.pi ** 2


@pytest.fixture(autouse=True, scope="module")
def _release_host_buffers():
    yield
    import gc
    from multigridcmt_amd import hostmem
    gc.collect()
    hostmem.drain()


def _rho(g):
    t = (np.arange(g) + 0.5) / g - 0.5
    Z, Y, X = np.meshgrid(t, t, t, indexing="ij")
    return np.sqrt((X - 0.05) ** 2 + ((Y + 0.03) / 0.8) ** 2 + ((Z - 0.02) / 0.6) ** 2)


def smooth_dot(g):
    """(w, V) of an ellipsoidal GaAs dot in AlGaAs with a smeared interface, index [z, y, x]"""
    s = 0.5 * (1.0 + np.tanh((_rho(g) - 0.3) / 0.08))
    return 1.0 - 0.27 * s, 30.0 * s


def sharp_dot(g):
    """the same dot with a sharp interface: w = 1 / 0.73, V = 0 / 30 inside / outside"""
    inside = _rho(g) < 0.3
    return np.where(inside, 1.0, 0.73), np.where(inside, 0.0, 30.0)


def rough(wv, seed=1):
    """seeded noise on w (kept positive) and V"""
    w, V = wv
    rng = np.random.RandomState(seed)
    return w + 0.2 * rng.rand(*w.shape), V + 5.0 * rng.rand(*V.shape)


def profile(name, g):
    return {"smooth": smooth_dot(g), "sharp": sharp_dot(g), "rough": rough(smooth_dot(g)), "rough_sharp": rough(sharp_dot(g), 2)}[name]


def hamiltonian(g, w, V, mean="harmonic", scale=SCALE):
    """scale * div(w grad) + diag(V) entry by entry, as a caller would assemble it: the neighbour entry t * m(w_a, w_b), the
    diagonal minus t times the six bond values (a ghost takes the point's own w) plus V"""
    m = (lambda a, b: 2.0 * a * b / (a + b)) if mean == "harmonic" else (lambda a, b: 0.5 * (a + b))
    t = scale * g * g
    n = g ** 3
    idx = np.arange(n).reshape(g, g, g)
    diag = np.zeros((g, g, g))
    rows, cols, vals = [], [], []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, g - 1), slice(1, g)
        lo, hi = tuple(lo), tuple(hi)
        b = m(w[lo], w[hi])
        rows += [idx[lo].ravel(), idx[hi].ravel()]
        cols += [idx[hi].ravel(), idx[lo].ravel()]
        vals += [(t * b).ravel(), (t * b).ravel()]
        plus, minus = w.copy(), w.copy()
        plus[lo] = b
        minus[hi] = b
        diag -= t * (plus + minus)
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    return (A + sp.diags((diag + V).ravel())).tocsr()


def flat(a):
    return np.asarray(a).reshape(-1)


def bonds_matrix(Bx, By, Bz):
    g = Bx.shape[0]
    n = g ** 3
    bx, by, bz = Bx.ravel()[:n - 1], By.ravel()[:n - g], Bz.ravel()[:n - g * g]
    return sp.diags([bz, by, bx, bx, by, bz], [-g * g, -g, -1, 1, g, g * g], shape=(n, n), format="csr")


def assemble_level(plan, level):
    """the matrix of `level`: Kronecker factors (mgcmt_plan_get_factors) plus the per-point part (mgcmt_plan_get_point_stencil);
    on level 0 the bonds towards outside points must be exact zeros"""
    gl = plan.g >> level
    fs = [plan.factors(level, w) for w in range(3)]
    A = sum(sp.kron(tri_to_sparse(fs[0][m]), sp.kron(tri_to_sparse(fs[1][m]), tri_to_sparse(fs[2][m]), format="csr"), format="csr")
            for m in range(fs[0].shape[0])).tocsr()
    G = plan.point_stencil(level)
    if level == 0:
        assert G.shape == (4, gl, gl, gl)
        for outward in (G[1][:, :, -1], G[2][:, -1, :], G[3][-1, :, :]):
            assert not np.ascontiguousarray(outward).view(np.uint64).any()
        return (A + sp.diags(G[0].reshape(-1)) + bonds_matrix(G[1], G[2], G[3])).tocsr()
    assert G.shape == (3, 3, 3, gl, gl, gl)
    return (A + stencil_matrix(G)).tocsr()


def check_levels(plan, chain, kind0, shift=0.7):
    """every level's assembled matrix against `chain` to 1e-13, and mgcmt_apply on every level with and without the shift"""
    assert plan.num_levels == len(chain)
    plan.set_shifts([shift])
    rng = np.random.RandomState(plan.g)
    for level, want in enumerate(chain):
        assert plan.level_path_3d(level) == ((kind0 if level == 0 else _lib.PATH3D_PLANES), False)
        got = assemble_level(plan, level)
        assert abs(got - want).max() <= 1e-13 * abs(want).max(), level
        x = rng.rand(want.shape[0]) - 0.5
        plan.upload(level, _lib.SLOT_V, 0, x)
        plan.apply(level, (_lib.SLOT_V, 0), (_lib.SLOT_T, 0))
        assert rel_err(plan.download(level, _lib.SLOT_T, 0), want @ x) < 1e-13, level
        plan.apply(level, (_lib.SLOT_V, 0), (_lib.SLOT_T, 0), with_shift=True)
        assert rel_err(plan.download(level, _lib.SLOT_T, 0), want @ x - shift * x) < 1e-13, level


# ---- host ----------------------------------------------------------------------------------------------------------------

def test_constructor_checks_3d():
    g = 4
    i = tri_identity(g)
    z = np.zeros((g, g, g))
    ok = np.ones((g, g, g))
    bx, by, bz = ok.copy(), ok.copy(), ok.copy()
    bx[:, :, -1] = by[:, -1, :] = bz[-1, :, :] = 0.0
    op = StructuredOperator("3d", g, [(i, i, i)], point_bonds=(bx, by, bz))
    assert op.point_diagonal.shape == (g, g, g) and not op.point_diagonal.any()          # bonds without a diagonal: D = 0
    assert [b.shape for b in op.point_bonds] == [(g, g, g)] * 3
    assert StructuredOperator("3d", g, [(i, i, i)], point_bonds=(bx.ravel(), by.ravel(), bz.ravel())).point_bonds[0].shape == (g, g, g)
    for which in range(3):          # one outward bond in each direction
        bad = [bx.copy(), by.copy(), bz.copy()]
        bad[which][(g - 1,) * 3] = 0.5
        with pytest.raises(ValueError, match="outside"):
            StructuredOperator("3d", g, [(i, i, i)], point_bonds=tuple(bad))
    with pytest.raises(ValueError):          # a pair is the 2-D form
        StructuredOperator("3d", g, [(i, i, i)], point_bonds=(np.zeros((g, g)), np.zeros((g, g))))
    with pytest.raises(ValueError):
        StructuredOperator("3d", g, [(i, i, i)], point_bonds=(z, z))
    with pytest.raises(ValueError):          # wrong sizes
        StructuredOperator("3d", g, [(i, i, i)], point_bonds=(z, z, np.zeros((g, g))))
    with pytest.raises(ValueError):
        StructuredOperator("2d", g, [(i, i)], point_bonds=(np.zeros((g, g)),) * 3)
    with pytest.raises(ValueError):
        StructuredOperator("1d", g, [(None, i)], point_bonds=(z, z, z))


def test_operator_algebra_carries_the_bonds_3d():
    g = 8
    w, V = profile("rough", g)
    op = variable_mass_operator(g, w, V, dimension="3d")
    A = hamiltonian(g, w, V)
    tol = 1e-13 * abs(A).max()
    assert op.point_bonds is not None and len(op.point_bonds) == 3 and op.point_diagonal.shape == (g, g, g)
    assert abs(op.tocsr() - A).max() <= tol
    assert np.allclose(op.diagonal(), A.diagonal(), rtol=1e-13)
    assert abs((op * 2.5).tocsr() - 2.5 * A).max() <= tol and (op * 2.5).point_bonds is not None
    assert abs((2.5 * op).tocsr() - 2.5 * A).max() <= tol
    assert abs((-op / 4.0).tocsr() + A / 4.0).max() <= tol
    sh = op.shifted(0.7)
    assert sh.point_bonds is not None
    assert abs(sh.tocsr() - (A - 0.7 * sp.identity(g ** 3))).max() <= tol
    # the fingerprint sees every plane, each under its own name
    bx, by, bz = op.point_bonds
    for which in range(3):
        planes = [bx.copy(), by.copy(), bz.copy()]
        planes[which][0, 0, 0] += 1e-9
        other = StructuredOperator("3d", g, op.terms, point_diagonal=op.point_diagonal, point_bonds=tuple(planes))
        assert other.fingerprint() != op.fingerprint(), which
    swapped = StructuredOperator("3d", g, op.terms, point_diagonal=op.point_diagonal, point_bonds=(bx, np.zeros_like(by), bz))
    assert swapped.fingerprint() != op.fingerprint()
    assert StructuredOperator("3d", g, op.terms, point_diagonal=op.point_diagonal).fingerprint() != op.fingerprint()
    assert StructuredOperator("3d", g, op.terms, point_diagonal=op.point_diagonal, point_bonds=op.point_bonds).fingerprint() == op.fingerprint()


def test_variable_mass_operator_3d():
    g = 8
    lap = MGCMTStencilMaker().laplacian(g, dimension="3d")
    one = variable_mass_operator(g, np.ones((g, g, g)), dimension="3d")
    assert one.point_bonds is None and one.point_diagonal is None
    assert abs(one.tocsr() - SCALE * lap).max() == 0.0          # w = 1, V = 0: scale * laplacian exactly
    assert abs(hamiltonian(g, np.ones((g, g, g)), np.zeros((g, g, g))) - SCALE * lap).max() <= 1e-13 * abs(SCALE * lap).max()
    uni = variable_mass_operator(g, np.full((g, g, g), 0.73), V=smooth_dot(g)[1], scale=-0.5, dimension="3d")
    assert uni.point_bonds is None and uni.point_diagonal is not None          # a uniform w: no bonds
    assert abs(uni.tocsr() - (-0.5 * 0.73 * lap + sp.diags(smooth_dot(g)[1].ravel()))).max() <= 1e-13 * abs(lap).max()
    for mean in ("harmonic", "arithmetic"):
        for name in ("smooth", "sharp", "rough"):
            w, V = profile(name, g)
            op = variable_mass_operator(g, w, V, mean=mean, dimension="3d")
            A = hamiltonian(g, w, V, mean=mean)
            assert abs(op.tocsr() - A).max() <= 1e-13 * abs(A).max(), (mean, name)
            assert abs(A - A.T).max() == 0.0
            for t in op.terms:          # the Kronecker part stays a constant 7-point operator
                for fac in t:
                    assert np.all(fac[1] == fac[1][0])
    w, V = profile("sharp", g)
    assert abs(variable_mass_operator(g, w.ravel(), V.ravel(), dimension="3d").tocsr() - hamiltonian(g, w, V)).max() <= 1e-13 * 64 * 30
    assert abs(variable_mass_operator(g, w, dimension="3d").tocsr() - hamiltonian(g, w, 0 * V)).max() <= 1e-13 * 64 * 30
    bad = w.copy()
    bad[1, 2, 3] = 0.0
    with pytest.raises(ValueError, match="positive"):
        variable_mass_operator(g, bad, dimension="3d")
    with pytest.raises(ValueError):
        variable_mass_operator(g, w[0], dimension="3d")
    with pytest.raises(ValueError):
        variable_mass_operator(g, w, V[0], dimension="3d")
    with pytest.raises(ValueError, match="mean"):
        variable_mass_operator(g, w, mean="geometric", dimension="3d")
    with pytest.raises(ValueError):
        variable_mass_operator(g, w[0], dimension="1d")
    assert variable_mass_operator(g, w[0]).dimension == "2d"          # the default is unchanged


def test_recognise_seven_point_round_trip():
    g = 8
    for name in ("smooth", "sharp", "rough"):
        w, V = profile(name, g)
        A = hamiltonian(g, w, V)
        with pytest.raises(UnrecognisedOperator):
            recognise_potential(A, "3d")
        op = recognise_seven_point(A)
        assert op.dimension == "3d" and op.point_bonds is not None and len(op.point_bonds) == 3
        assert abs(op.tocsr() - A).max() <= 1e-13 * abs(A).max(), name
        for t in op.terms:          # the medians went into the Kronecker part: its factors are Toeplitz
            for fac in t:
                assert np.all(fac[1] == fac[1][0]) and np.all(fac[0][1:] == fac[0][1]) and np.all(fac[2][:-1] == fac[2][0])
        assert recognise_seven_point(A) is op          # cached
    w, V = profile("rough", g)
    A = hamiltonian(g, w, V)
    # what recognise / recognise_potential accept comes back as their own object
    lap = (SCALE * MGCMTStencilMaker().laplacian(g, dimension="3d")).tocsr()
    assert recognise_seven_point(lap) is recognise(lap, "3d")
    P = (lap + sp.diags(V.ravel())).tocsr()
    assert recognise_seven_point(P) is recognise_potential(P, "3d") and recognise_seven_point(P).point_bonds is None
    sop = variable_mass_operator(g, w, V, dimension="3d")
    assert recognise_seven_point(sop) is sop
    # unsymmetric
    B = sp.lil_matrix(A)
    B[5, 6] = B[5, 6] * 1.5
    with pytest.raises(UnrecognisedOperator, match="symmetric"):
        recognise_seven_point(B.tocsr())
    # an entry off the seven bands
    B = sp.lil_matrix(A)
    B[5, 7] = 0.25
    B[7, 5] = 0.25
    with pytest.raises(UnrecognisedOperator):
        recognise_seven_point(B.tocsr())
    # a wrap across a row end (x = g - 1 to x = 0 of the next row) and across a plane end
    B = sp.lil_matrix(A)
    B[g - 1, g] = 0.25
    B[g, g - 1] = 0.25
    with pytest.raises(UnrecognisedOperator, match="ends"):
        recognise_seven_point(B.tocsr())
    B = sp.lil_matrix(A)
    B[g * g - g, g * g] = 0.25
    B[g * g, g * g - g] = 0.25
    with pytest.raises(UnrecognisedOperator, match="ends"):
        recognise_seven_point(B.tocsr())
    with pytest.raises(UnrecognisedOperator):
        recognise_seven_point(sp.identity(10, format="csr") * 2.0 + sp.diags([np.arange(9.0) + 1], [1]))
    # recognise and recognise_potential stay as they are
    with pytest.raises(UnrecognisedOperator):
        recognise(A, "3d")


# ---- hierarchy -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g,lowest,name", [(8, 2, "rough"), (16, 2, "rough_sharp"), (16, 4, "smooth")])
def test_galerkin_hierarchy_and_apply_on_every_level_3d_bonds(backend, g, lowest, name):
    """R*A*P of every level — Kronecker factors plus mgcmt_plan_get_point_stencil — against scipy's product of
    MGCMTStencilMaker's own 3-D matrices, and mgcmt_apply on every level against that matrix (with and without the shift)."""
    w, V = profile(name, g)
    plan = Plan(variable_mass_operator(g, w, V, dimension="3d"), lowest, nvec=1)
    try:
        check_levels(plan, galerkin_chain(hamiltonian(g, w, V), g, lowest), _lib.PATH3D_SEVEN_BONDS)
    finally:
        plan.close()
    w, V = profile("rough", 8)
    op = variable_mass_operator(8, w, V, dimension="3d")          # A.dot(x) of the operator object
    x = np.random.RandomState(2).rand(512)
    assert rel_err(op.dot(x), op.tocsr() @ x) < 1e-13


def test_smoothers_stand_alone_3d_bonds(backend):
    g = 16
    w, V = profile("rough", g)
    A, op = hamiltonian(g, w, V), variable_mass_operator(g, w, V, dimension="3d")
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


# ---- a Kronecker part that is not the constant 7-point operator, plus bonds (kind 6) -----------------------------------------

def mixed_operator(g):
    """a separable potential a(z) + b(x) kept in the (then non-Toeplitz) factors, the bonds and the diagonal of the rough dot
    on top: level 0 is "general terms + point diagonal + bonds", whose flat kernels add the bonds to the six neighbour products"""
    t = (np.arange(g) + 0.5) / g - 0.5
    base = variable_mass_operator(g, *profile("rough", g), dimension="3d")
    terms = [tuple(a.copy() for a in tr) for tr in base.terms]
    terms[2][0][1] += 25.0 * t * t + np.random.RandomState(7).rand(g)          # the z factor of the z term
    terms[0][2][1] += 6.0 * np.cos(3.0 * t) + 6.0                              # the x factor of the x term
    return StructuredOperator("3d", g, terms, point_diagonal=base.point_diagonal, point_bonds=base.point_bonds)


@pytest.mark.parametrize("g,lowest", [(8, 2), (16, 4)])
def test_general_terms_plus_bonds_3d(backend, g, lowest):
    """every level's matrix and apply, both smoothers stand-alone and a V(2,2) cycle with each, against the assembled matrix"""
    op = mixed_operator(g)
    A = op.tocsr()
    n = g ** 3
    plan = Plan(op, lowest, nvec=1)
    try:
        check_levels(plan, galerkin_chain(A, g, lowest), _lib.PATH3D_GENERAL_BONDS)
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

@pytest.mark.parametrize("name", ["smooth", "rough"])
@pytest.mark.parametrize("smoother", ["wjacobi", "gseidel_rb"])
@pytest.mark.parametrize("shift", [0.0, 1.9])
@pytest.mark.parametrize("g,lowest", [(8, 2), (8, 8), (16, 4), (32, 8), (64, 8)])
def test_vcycle_3d_bonds_vs_oracle(backend, g, lowest, shift, smoother, name):
    """V(2,2) for (H - shift I) v = f, H = -div(w grad)/pi^2 + V (H > 2: the shifted operator is definite on every level).
    (8, 8): level 0 is the coarsest level too — the band matrix takes D and the bonds.  64^3 is the smallest grid on which the
    marching kernels run (two z-chunks): asserted through mgcmt_plan3d_level_path."""
    w, V = profile(name, g)
    A, op = hamiltonian(g, w, V), variable_mass_operator(g, w, V, dimension="3d")
    solver, ref = MGCMTSolver(), Ref3dSolver()
    ours, theirs = (None, None) if smoother == "wjacobi" else (solver.gseidel_rb, mc_3d)
    n = g ** 3
    f = np.random.RandomState(g + lowest).rand(n)
    kw = dict(nu1=2, nu2=2, shift=shift, lowest_level=lowest, dimension="3d")
    y = flat(ref.vcycle(np.zeros(n), f.copy(), A, Ref3dStencilMaker(), smoother=theirs, **kw))
    assert np.linalg.norm(f - (A @ y - shift * y)) < np.linalg.norm(f)          # the oracle's own residual falls
    x = solver.vcycle(np.zeros(n), f.copy(), op, MGCMTStencilMaker(), smoother=ours, **kw)
    assert flat(x).shape == (n,)
    assert rel_err(flat(x), y) < TOL
    if g <= 16:          # the assembled matrix through recognise_seven_point inside the 3-D entry point
        assert rel_err(flat(solver.vcycle(np.zeros(n), f.copy(), A, MGCMTStencilMaker(), smoother=ours, **kw)), y) < TOL
    if g == 64:
        plan = get_plan(op, lowest, nvec=1)
        assert plan.level_path_3d(0) == (_lib.PATH3D_SEVEN_BONDS, True)
        assert plan.level_path_3d(1) == (_lib.PATH3D_PLANES, False)


@pytest.mark.parametrize("smoother", ["wjacobi", "gseidel_rb"])
def test_vcycle_3d_bonds_nonzero_start_and_repeat(backend, smoother):
    # a non-zero start vector, and the same call three times (the second captures the cycle's graph, the third replays it)
    g = 16
    w, V = profile("rough_sharp", g)
    A, op = hamiltonian(g, w, V), variable_mass_operator(g, w, V, dimension="3d")
    rng = np.random.RandomState(2)
    f, v0 = rng.rand(g ** 3), rng.rand(g ** 3)
    solver, ref = MGCMTSolver(), Ref3dSolver()
    ours, theirs = (None, None) if smoother == "wjacobi" else (solver.gseidel_rb, mc_3d)
    kw = dict(nu1=2, nu2=2, shift=0.7, lowest_level=4, dimension="3d")
    y = ref.vcycle(v0.copy(), f.copy(), A, Ref3dStencilMaker(), smoother=theirs, **kw)
    for _ in range(3):
        assert rel_err(solver.vcycle(v0.copy(), f.copy(), op, MGCMTStencilMaker(), smoother=ours, **kw), y) < TOL


@pytest.mark.parametrize("smoother", ["wjacobi", "gseidel_rb"])
def test_vcycle_matrix_3d_bonds_with_column_shifts(backend, smoother):
    g, k = 16, 3
    w, V = profile("rough", g)
    A, op = hamiltonian(g, w, V), variable_mass_operator(g, w, V, dimension="3d")
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


def test_foreign_smoother_sees_the_level_matrices_3d_bonds(backend):
    """A callable smoother receives (R A P - shift I) of every level: level 0 with its bonds, the 27-plane levels below."""
    g, lowest = 16, 4
    w, V = profile("rough", g)
    A, op = hamiltonian(g, w, V), variable_mass_operator(g, w, V, dimension="3d")
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
            assert p.level_path_3d(0) == (_lib.PATH3D_SEVEN_BONDS, march)
            out.append(run(p))
        finally:
            p.close()
    return out


def test_marching_and_flat_forms_agree_64_bonds(backend, monkeypatch):
    """One Jacobi sweep, one red-black sweep (omega 1 and 1.3) and one V(2,2) cycle of each smoother at 64^3 — two 32-plane
    chunks, so the carried Bz(z-1) crosses a chunk boundary —, two columns with the shifts [0, 1.9], MGCMT_3D_POINT_MARCH=0
    against the default.  Both forms compute a point with the same inline functions: the sweeps agree bit for bit; the cycle's
    restriction sums in another order: 1e-13 relative."""
    g = 64
    op = variable_mass_operator(g, *profile("rough", g), dimension="3d")
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

def test_block_eigensolve_sharp_ellipsoid_against_eigsh(backend):
    import scipy.sparse.linalg as sla
    g, k = 16, 3
    w, V = profile("sharp", g)
    op = variable_mass_operator(g, w, V, dimension="3d")
    assert op.point_bonds is not None
    vals, vecs = drivers.block_eigensolve(op, k=k, cycles=24, lowest=4)
    want = np.sort(sla.eigsh(hamiltonian(g, w, V), k=k, sigma=0.0, which="LM")[0])
    assert np.allclose(vals, want, rtol=0, atol=1e-8), np.abs(vals - want)
    assert np.abs(vecs.T @ vecs - np.eye(k)).max() < 1e-10


# ---- what stays unsupported ----------------------------------------------------------------------------------------------------

def test_refusals_on_a_3d_bonds_plan(backend):
    g = 8
    w, V = profile("rough", g)
    op = variable_mass_operator(g, w, V, dimension="3d")
    A = hamiltonian(g, w, V)
    L = _lib.lib()
    U = -4  # MGCMT_ERR_UNSUPPORTED
    plan = Plan(op, 2, nvec=6)
    try:
        h = plan._h
        vecs = (ctypes.c_int * 6)(0, 1, 2, 3, 4, 5)
        dbl = ctypes.c_double(0.0)
        for name, call in {
            "smooth_lex": lambda: L.mgcmt_smooth(h, 0, _lib.GS_LEX, 1, ctypes.c_double(1.0), 1, None),
            "vcycle_sor": lambda: L.mgcmt_vcycle(h, 0, 2, 2, 2, _lib.SOR_LEX, ctypes.c_double(1.0), 1, 0, None),
            "twogrid": lambda: L.mgcmt_twogrid(h, 0, 2, 2, _lib.WJACOBI, ctypes.c_double(1.0), 1, None),
            "rqmin": lambda: L.mgcmt_rqmin(h, 0, 0, vecs, 2, 0, ctypes.byref(dbl), None),
            "vcycle_rqmg": lambda: L.mgcmt_vcycle_rqmg(h, 0, vecs, 2, 2, 0, ctypes.byref(dbl), None),
            "fused_pass": lambda: L.mgcmt_fused_pass(h, 0, _lib.WJACOBI, 1, ctypes.c_double(1.0), 0, 1, None),
        }.items():
            assert call() == U, name
            msg = L.mgcmt_last_error()
            assert b"3-D" in msg or b"point diagonal" in msg, (name, msg)
        # creation: null arrays, outward bonds and lowest > 16 fail cleanly
        nterms, zfac, yfac, xfac = op.factor_blocks()
        desc = _lib.Plan3dDesc()
        desc.nterms, desc.nvec, desc.g, desc.lowest = nterms, 1, g, 2
        desc.zfac, desc.yfac, desc.xfac = _lib.as_dp(zfac), _lib.as_dp(yfac), _lib.as_dp(xfac)
        hh = ctypes.c_void_p()
        d = np.ascontiguousarray(op.point_diagonal)
        planes = [np.ascontiguousarray(b) for b in op.point_bonds]
        dp = _lib.as_dp
        assert L.mgcmt_plan_create3d_bonds(ctypes.byref(desc), None, dp(planes[0]), dp(planes[1]), dp(planes[2]), ctypes.byref(hh)) == -1 and not hh.value
        assert L.mgcmt_plan_create3d_bonds(ctypes.byref(desc), dp(d), dp(planes[0]), None, dp(planes[2]), ctypes.byref(hh)) == -1 and not hh.value
        for which, where in enumerate([(3, 4, g - 1), (3, g - 1, 4), (g - 1, 3, 4)]):
            bad = [b.copy() for b in planes]
            bad[which][where] = 0.125
            assert L.mgcmt_plan_create3d_bonds(ctypes.byref(desc), dp(d), dp(bad[0]), dp(bad[1]), dp(bad[2]), ctypes.byref(hh)) == -1 and not hh.value
            assert b"outside" in L.mgcmt_last_error()
        desc.g, desc.lowest = 32, 32
        big = np.zeros(32 ** 3)
        assert L.mgcmt_plan_create3d_bonds(ctypes.byref(desc), dp(big), dp(big), dp(big), dp(big), ctypes.byref(hh)) == -1 and not hh.value
        assert b"16" in L.mgcmt_last_error()
        assert L.mgcmt_abi_version() == 7
    finally:
        plan.close()
    # Python: the lexicographic smoothers raise, naming what is supported; a mass operator and the Rayleigh-quotient entries are refused
    solver, sm = MGCMTSolver(), MGCMTStencilMaker()
    v0, f = np.zeros(g ** 3), np.ones(g ** 3)
    for bad in (solver.gseidel, solver.sor):
        for start in (op, A):
            with pytest.raises(ValueError, match="wjacobi"):
                solver.vcycle(v0.copy(), f.copy(), start, sm, smoother=bad, dimension="3d", lowest_level=2)
    with pytest.raises(ValueError, match="wjacobi, gseidel_rb"):
        solver.gseidel(v0.copy(), f.copy(), op)
    with pytest.raises(ValueError, match="point bonds"):
        Plan(op, 2, nvec=10, mass=identity_operator(g, "3d"))
    with pytest.raises(ValueError, match="point diagonal"):
        solver.vcycle_rqmg(np.ones(g ** 3), op, identity_operator(g, "3d"))
    # an unsymmetric 7-point matrix stays out of scope: the 3-D entry point raises recognise's error
    B = sp.lil_matrix(A)
    B[5, 6] = B[5, 6] * 1.5
    with pytest.raises(UnrecognisedOperator):
        solver.vcycle(v0.copy(), f.copy(), B.tocsr(), sm, dimension="3d", lowest_level=2)
