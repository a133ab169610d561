"""Tensor effective mass in 3-D: operators with a per-point 27-point stencil (StructuredOperator(..., point_stencil=) in 3-D,
operators.tensor_mass_operator(..., dimension="3d"), recognise_27_point, mgcmt_plan_create3d_stencil) against the NumPy oracle
(Ref3dSolver of tests/test_3d_cycle.py, which cycles any sparse matrix) and against scipy's own R*A*P, through the HIP library on
the GPU box and through the emulated kernels on CPU (``backend`` fixture).

Level 0 of such a plan — constant 7-point Kronecker part plus 27 planes, kind 7 — computes a point with
csrc/stencil27_point.h's p27::seven; from 64^3 on its colour stages and its residual + restriction run the kernels of
csrc/kernels_3d_stencil.hip (MGCMT_3D_STENCIL_TILE=0: the flat ones), which give the bits of the flat form: 64^3 holds two
workgroup tiles (16 x 16 coarse columns, 8 coarse planes) along every axis."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import rel_err
from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, _lib, drivers
from multigridcmt_amd.operators import (StructuredOperator, UnrecognisedOperator, identity_operator, potential_operator, recognise,
                                        recognise_27_point, recognise_potential, recognise_seven_point, tensor_mass_operator,
                                        tri_to_sparse, variable_mass_operator)
from multigridcmt_amd.plan import Plan, get_plan
from test_3d_cycle import Ref3dSolver, Ref3dStencilMaker, mc_3d
from test_3d_point_potential import galerkin_chain, stencil_matrix

TOL = 1e-10          # the bar of tests/test_3d_cycle.py
SCALE = -1 / np.pi ** 2
V, F, T = _lib.SLOT_V, _lib.SLOT_F, _lib.SLOT_T


@pytest.fixture(autouse=True, scope="module")
def _release_host_buffers():
    yield
    import gc
    from multigridcmt_amd import hostmem
    gc.collect()
    hostmem.drain()


# ---- profiles ----------------------------------------------------------------------------------------------------------------

def smooth_w(g):
    """(wxx, wyy, wzz, wxy, wxz, wyz, V), index [z, y, x]: an ellipsoidal dot whose inverse-mass ellipsoid (principal values
    1 / 0.35 / 0.6) is rotated by a position-dependent angle about z and about x, blended into 0.73 I outside; V = 30 s"""
    t = (np.arange(g) + 0.5) / g - 0.5
    Z, Y, X = np.meshgrid(t, t, t, indexing="ij")
    s = 0.5 * (1.0 + np.tanh((np.sqrt((X - 0.05) ** 2 + ((Y + 0.03) / 0.8) ** 2 + ((Z - 0.02) / 0.6) ** 2) - 0.3) / 0.08))
    th, ph = 0.6 + 0.8 * Z, 0.4 - 0.5 * X
    c, sn, cp, sq = np.cos(th), np.sin(th), np.cos(ph), np.sin(ph)
    e = [(c, sn, 0.0 * c), (-sn * cp, c * cp, sq), (sn * sq, -c * sq, cp)]          # columns of Rz(th) Rx(ph), components (x, y, z)
    w = []
    for i, j in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)):
        inside = sum(l * ek[i] * ek[j] for l, ek in zip((1.0, 0.35, 0.6), e))
        w.append((1.0 - s) * inside + s * (0.73 if i == j else 0.0))
    return tuple(w) + (30.0 * s,)


def rough_w(g, seed=1):
    """the same with seeded noise on all six components and on V (the noise keeps W diagonally dominant: positive definite)"""
    wxx, wyy, wzz, wxy, wxz, wyz, Vp = smooth_w(g)
    r = np.random.RandomState(seed)
    return (wxx + 0.2 * r.rand(g, g, g), wyy + 0.2 * r.rand(g, g, g), wzz + 0.2 * r.rand(g, g, g), wxy + 0.04 * (r.rand(g, g, g) - 0.5),
            wxz + 0.04 * (r.rand(g, g, g) - 0.5), wyz + 0.04 * (r.rand(g, g, g) - 0.5), Vp + 5.0 * r.rand(g, g, g))


def tensor_op(g, profile="smooth", mean="harmonic"):
    wxx, wyy, wzz, wxy, wxz, wyz, Vp = smooth_w(g) if profile == "smooth" else rough_w(g)
    return tensor_mass_operator(g, wxx, wyy, wxy, V=Vp, mean=mean, wzz=wzz, wxz=wxz, wyz=wyz, dimension="3d")


@functools.lru_cache(maxsize=None)
def problem(g, profile):
    """(operator, its assembled matrix): built once per size and profile, never modified"""
    op = tensor_op(g, profile)
    return op, op.tocsr()


def flat(a):
    return np.asarray(a).reshape(-1)


def assemble_by_entries(g, w, mean, scale=SCALE):
    """the matrix of the issue's formulas, one entry at a time"""
    wxx, wyy, wzz, wxy, wxz, wyz, Vp = w
    t = scale * g * g
    m = (lambda a, b: 2.0 * a * b / (a + b)) if mean == "harmonic" else (lambda a, b: 0.5 * (a + b))
    diag = {2: wxx, 1: wyy, 0: wzz}                      # array axis -> w_uu
    mixed = {(2, 1): wxy, (2, 0): wxz, (1, 0): wyz}
    A = sp.lil_matrix((g ** 3, g ** 3))
    idx = lambda p: (p[0] * g + p[1]) * g + p[2]
    inside = lambda p: all(0 <= c < g for c in p)
    for p in np.ndindex(g, g, g):
        d = Vp[p]
        for ax in range(3):
            for sgn in (-1, 1):
                nb = list(p)
                nb[ax] += sgn
                nb = tuple(nb)
                bond = m(diag[ax][p], diag[ax][nb]) if inside(nb) else diag[ax][p]
                d -= t * bond
                if inside(nb):
                    A[idx(p), idx(nb)] = t * bond
        A[idx(p), idx(p)] = d
        for (au, av), w_uv in mixed.items():
            for a in (-1, 1):
                for b in (-1, 1):
                    pu, pv, nb = list(p), list(p), list(p)
                    pu[au] += a
                    pv[av] += b
                    nb[au] += a
                    nb[av] += b
                    if inside(nb):
                        A[idx(p), idx(tuple(nb))] = a * b * t * (w_uv[tuple(pu)] + w_uv[tuple(pv)]) / 4.0
    return A.tocsr()


# ---- 1. host: the operator object --------------------------------------------------------------------------------------------

def test_point_stencil_constructor_and_algebra_3d():
    g = 6
    op = tensor_op(g, "rough")
    G = op.point_stencil
    assert G.shape == (3, 3, 3, g, g, g) and op.point_diagonal is None and op.point_bonds is None
    A = op.tocsr()
    assert abs(A - A.T).max() == 0.0
    tol = 1e-13 * abs(A).max()
    plain = StructuredOperator("3d", g, op.terms).tocsr()
    assert abs(A - plain - stencil_matrix(G)).max() <= tol
    assert np.allclose(op.diagonal(), A.diagonal(), rtol=1e-14)
    assert abs((op * 2.5).tocsr() - 2.5 * A).max() <= tol and abs((2.5 * op).tocsr() - 2.5 * A).max() <= tol
    assert abs((-op / 4.0).tocsr() + A / 4.0).max() <= tol
    assert abs(op.shifted(0.7).tocsr() - (A - 0.7 * sp.identity(g ** 3))).max() <= tol
    assert op.shifted(0.7).point_stencil is not None and (op * 2.0).point_stencil is not None
    G2 = G.copy()
    G2[0, 1, 0][3, 4, 2] += 1e-9
    G2[2, 1, 2][2, 4, 1] += 1e-9          # (kept symmetric)
    assert op.fingerprint() != StructuredOperator("3d", g, op.terms, point_stencil=G2).fingerprint()
    assert op.fingerprint() != StructuredOperator("3d", g, op.terms).fingerprint()
    assert StructuredOperator("3d", g, op.terms, point_stencil=G.reshape(-1)).fingerprint() == op.fingerprint()          # 27 g^3 numbers flat
    for gg in (4, 8):
        assert tensor_op(gg).point_stencil.shape == (3, 3, 3, gg, gg, gg)
    # refusals: next to a diagonal or bonds, towards the outside, unsymmetric, wrong sizes (a 2-D stencil among them)
    z3 = np.zeros((g, g, g))
    with pytest.raises(ValueError):
        StructuredOperator("3d", g, op.terms, point_diagonal=z3, point_stencil=G)
    with pytest.raises(ValueError):
        StructuredOperator("3d", g, op.terms, point_bonds=(z3, z3, z3), point_stencil=G)
    for (a, b, c, zz, yy, xx) in ((0, 1, 1, 0, 3, 3), (2, 2, 1, g - 1, 2, 2), (1, 2, 2, 4, g - 1, 1), (1, 1, 0, 3, 3, 0), (2, 0, 2, 1, 0, 1), (0, 0, 0, 2, 2, 0)):
        bad = G.copy()
        bad[a, b, c][zz, yy, xx] = 1.0
        with pytest.raises(ValueError, match="outside"):
            StructuredOperator("3d", g, op.terms, point_stencil=bad)
    bad = G.copy()
    bad[1, 2, 0][3, 3, 3] += 0.5
    with pytest.raises(ValueError, match="symmetric"):
        StructuredOperator("3d", g, op.terms, point_stencil=bad)
    with pytest.raises(ValueError):
        StructuredOperator("3d", g, op.terms, point_stencil=G[:, :, :, :-1])
    with pytest.raises(ValueError):
        StructuredOperator("3d", g, op.terms, point_stencil=np.zeros((3, 3, g, g)))
    with pytest.raises(ValueError):
        StructuredOperator("1d", g, [(None, np.zeros((3, g)))], point_stencil=G)


# ---- 2. host: tensor_mass_operator -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", [8, 16])
@pytest.mark.parametrize("profile", ["smooth", "rough"])
@pytest.mark.parametrize("mean", ["harmonic", "arithmetic"])
def test_tensor_mass_3d_entry_by_entry(g, profile, mean):
    w = smooth_w(g) if profile == "smooth" else rough_w(g)
    op = tensor_op(g, profile, mean)
    want = assemble_by_entries(g, w, mean)
    A = op.tocsr()
    assert abs(A - want).max() <= 1e-13 * abs(want).max()
    assert abs(A - A.T).max() == 0.0
    G = op.point_stencil
    for a, b, c in np.ndindex(3, 3, 3):          # a 19-point matrix: the eight corner planes are zero
        if a != 1 and b != 1 and c != 1:
            assert not G[a, b, c].any()
    for t in op.terms:          # level 0 keeps a constant 7-point Kronecker part
        for fac in t:
            assert np.all(fac[1] == fac[1][0]) and np.all(fac[2][:-1] == fac[2][0])
    if g == 8:
        assert np.linalg.eigvalsh(A.toarray())[0] > 0.7          # shifts 0 and 0.7 leave the operator definite


def test_tensor_mass_3d_degenerate_cases():
    g = 8
    one, zero = np.ones((g, g, g)), np.zeros((g, g, g))
    lap = SCALE * MGCMTStencilMaker().laplacian(g, dimension="3d")
    op = tensor_mass_operator(g, one, one, zero, wzz=one, wxz=zero, wyz=zero, dimension="3d")
    assert abs(op.tocsr() - lap).max() == 0.0          # W = I, V = 0: the scaled Laplacian exactly
    wxx, wyy, wzz, wxy, wxz, wyz, Vp = rough_w(g)
    # zero mixed parts: bonds
    op = tensor_mass_operator(g, wxx, wyy, zero, V=Vp, wzz=wzz, wxz=zero, wyz=zero, dimension="3d")
    assert op.point_stencil is None and op.point_bonds is not None
    assert abs(op.tocsr() - assemble_by_entries(g, (wxx, wyy, wzz, zero, zero, zero, Vp), "harmonic")).max() <= 1e-13 * abs(op.tocsr()).max()
    # equal diagonals as well: variable_mass_operator's operator, exactly
    for mean in ("harmonic", "arithmetic"):
        op = tensor_mass_operator(g, wxx, wxx, zero, V=Vp, mean=mean, wzz=wxx, wxz=zero, wyz=zero, dimension="3d")
        assert op.fingerprint() == variable_mass_operator(g, wxx, V=Vp, mean=mean, dimension="3d").fingerprint()
    # flat input (g^3 values) is taken as [z, y, x]
    a = tensor_mass_operator(g, flat(wxx), flat(wyy), flat(wxy), V=flat(Vp), wzz=flat(wzz), wxz=flat(wxz), wyz=flat(wyz), dimension="3d")
    assert a.fingerprint() == tensor_op(g, "rough").fingerprint()


def test_tensor_mass_3d_value_errors():
    g = 4
    wxx, wyy, wzz, wxy, wxz, wyz, Vp = rough_w(g)
    kw = dict(wzz=wzz, wxz=wxz, wyz=wyz, dimension="3d")
    for missing in ("wzz", "wxz", "wyz"):
        with pytest.raises(ValueError, match=missing):
            tensor_mass_operator(g, wxx, wyy, wxy, **{k: (None if k == missing else v) for k, v in kw.items()})
    with pytest.raises(ValueError):
        tensor_mass_operator(g, wxx[:, :, :-1], wyy, wxy, **kw)
    with pytest.raises(ValueError):
        tensor_mass_operator(g, wxx, wyy, wxy, wzz=wzz[0], wxz=wxz, wyz=wyz, dimension="3d")
    with pytest.raises(ValueError):
        tensor_mass_operator(g, wxx, wyy, wxy, V=Vp[0], **kw)
    with pytest.raises(ValueError, match="mean"):
        tensor_mass_operator(g, wxx, wyy, wxy, mean="geometric", **kw)
    with pytest.raises(ValueError, match="dimension"):
        tensor_mass_operator(g, wxx, wyy, wxy, wzz=wzz, wxz=wxz, wyz=wyz, dimension="4d")
    # not positive definite: a negative diagonal, a large xy part, and a large yz part that only the determinant sees
    with pytest.raises(ValueError, match="positive definite"):
        tensor_mass_operator(g, wxx, wyy, wxy, wzz=-wzz, wxz=wxz, wyz=wyz, dimension="3d")
    with pytest.raises(ValueError, match="positive definite"):
        tensor_mass_operator(g, wxx, wyy, 2.0 * np.ones((g, g, g)), **kw)
    with pytest.raises(ValueError, match="positive definite"):
        tensor_mass_operator(g, wxx, wyy, wxy, wzz=wzz, wxz=wxz, wyz=2.0 * np.ones((g, g, g)), dimension="3d")
    # the 2-D call: the three new components belong to 3-D; and it is what it was (fingerprint recorded before this change)
    t = (np.arange(8) + 0.5) / 8 - 0.5
    Y, X = np.meshgrid(t, t, indexing="ij")
    with pytest.raises(ValueError):
        tensor_mass_operator(8, 1.0 + 0.5 * X * X, 0.75 + 0.25 * Y * Y, 0.25 * X * Y, wzz=np.ones((8, 8)))
    op2 = tensor_mass_operator(8, 1.0 + 0.5 * X * X + 0.125 * Y, 0.75 + 0.25 * Y * Y, 0.25 * X * Y + 0.125 * X, V=5.0 * (X * X + Y * Y))
    assert op2.dimension == "2d" and op2.fingerprint() == "9ba4146d97143b397b85927b4d8f2fdd9020268d"


# ---- 3. host: recognise_27_point ---------------------------------------------------------------------------------------------

def test_recognise_27_point_round_trips():
    g = 8
    op, A = problem(g, "rough")
    r = recognise_27_point(A)
    assert r.dimension == "3d" and r.point_stencil is not None and r.point_stencil.shape == (3, 3, 3, g, g, g)
    assert abs(r.tocsr() - A).max() <= 1e-13 * abs(A).max()
    for t in r.terms:          # the medians went into Toeplitz terms
        for fac in t:
            assert np.all(fac[1] == fac[1][0])
    assert recognise_27_point(A) is r and recognise_27_point(op) is op
    for refuse in (recognise_seven_point, lambda M: recognise_potential(M, "3d"), lambda M: recognise(M, "3d")):
        with pytest.raises(UnrecognisedOperator):
            refuse(A)
    # a full 27-point matrix (a Galerkin level) round trips too
    R, P = MGCMTStencilMaker().restriction(g, g // 2, dimension="3d"), MGCMTStencilMaker().interpolation(g // 2, g, dimension="3d")
    C = (R @ A @ P).tocsr()
    C = (0.5 * (C + C.T)).tocsr()
    rc = recognise_27_point(C)
    assert rc.g == g // 2 and abs(rc.tocsr() - C).max() <= 1e-13 * abs(C).max()
    # what the earlier recognisers accept comes back as theirs
    lap = (SCALE * MGCMTStencilMaker().laplacian(g, dimension="3d")).tocsr()
    assert recognise_27_point(lap) is recognise(lap, "3d")
    pot = (lap + sp.diags(np.random.RandomState(3).rand(g ** 3))).tocsr()
    assert recognise_27_point(pot) is recognise_potential(pot, "3d")
    bonds = variable_mass_operator(g, rough_w(g)[0], dimension="3d").tocsr()
    assert recognise_27_point(bonds) is recognise_seven_point(bonds) and recognise_27_point(bonds).point_bonds is not None
    # refusals: unsymmetric, an entry two columns away, a wrap across a row end
    B = sp.lil_matrix(A)
    B[g * g + g + 1, g * g + 2 * g + 2] += 0.25
    with pytest.raises(UnrecognisedOperator, match="symmetric"):
        recognise_27_point(B.tocsr())
    B = sp.lil_matrix(A)
    B[5, 7] = B[7, 5] = 0.25
    with pytest.raises(UnrecognisedOperator, match="neighbourhood"):
        recognise_27_point(B.tocsr())
    B = sp.lil_matrix(A)
    B[g - 1, g] = B[g, g - 1] = 0.25          # (0, 0, g - 1) and (0, 1, 0): neighbours in the matrix, not on the grid
    with pytest.raises(UnrecognisedOperator, match="ends"):
        recognise_27_point(B.tocsr())
    with pytest.raises(UnrecognisedOperator):
        recognise_27_point(sp.identity(100, format="csr"))


# ---- 4. levels ---------------------------------------------------------------------------------------------------------------

def assemble_level(plan, level):
    """the matrix of `level`: Kronecker factors (mgcmt_plan_get_factors) plus the 27 planes (mgcmt_plan_get_point_stencil), which
    must be exact zeros towards outside points on every level, level 0 included"""
    gl = plan.g >> level
    fs = [plan.factors(level, w) for w in range(3)]
    A = sum(sp.kron(tri_to_sparse(fs[0][m]), sp.kron(tri_to_sparse(fs[1][m]), tri_to_sparse(fs[2][m]), format="csr"), format="csr")
            for m in range(fs[0].shape[0])).tocsr()
    G = plan.point_stencil(level)
    assert G.shape == (3, 3, 3, gl, gl, gl)
    return (A + stencil_matrix(G)).tocsr()


@pytest.mark.parametrize("g,lowest", [(8, 2), (16, 4)])
def test_galerkin_hierarchy_and_apply_on_every_level(backend, g, lowest):
    op, A = problem(g, "rough")
    plan = Plan(op, lowest, nvec=1)
    try:
        chain = galerkin_chain(A, g, lowest)
        assert plan.num_levels == len(chain)
        plan.set_shifts([0.7])
        rng = np.random.RandomState(g)
        for level, want in enumerate(chain):
            assert plan.level_path_3d(level) == ((_lib.PATH3D_SEVEN_PLANES if level == 0 else _lib.PATH3D_PLANES), False)
            got = assemble_level(plan, level)
            assert abs(got - want).max() <= 1e-13 * abs(want).max(), level
            M = MGCMTSolver()._level_matrix(plan, level, 0.7)          # what a foreign smoother sees
            assert abs(M - (want - 0.7 * sp.identity(want.shape[0]))).max() <= 1e-13 * abs(want).max(), level
            x = rng.rand(want.shape[0]) - 0.5
            plan.upload(level, V, 0, x)
            plan.apply(level, (V, 0), (T, 0))
            assert rel_err(plan.download(level, T, 0), want @ x) < 1e-13, level
            plan.apply(level, (V, 0), (T, 0), with_shift=True)
            assert rel_err(plan.download(level, T, 0), want @ x - 0.7 * x) < 1e-13, level
        assert np.array_equal(plan.point_stencil(0), op.point_stencil)
    finally:
        plan.close()
    x = np.random.RandomState(2).rand(g ** 3)
    assert rel_err(op.dot(x), A @ x) < 1e-13          # A.dot(x) of the operator object


# ---- 5. smoothers and cycles against the oracle ------------------------------------------------------------------------------

def test_smoothers_stand_alone(backend):
    g = 16
    op, A = problem(g, "rough")
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


@functools.lru_cache(maxsize=None)
def oracle_cycle(g, lowest, shift, smoother, profile):
    """(f, the oracle's V(2,2) from a zero start): one run per case, shared by the backends"""
    _, A = problem(g, profile)
    n = g ** 3
    f = np.random.RandomState(g + lowest).rand(n)
    y = Ref3dSolver().vcycle(np.zeros(n), f.copy(), A, Ref3dStencilMaker(), nu1=2, nu2=2, smoother=None if smoother == "wjacobi" else mc_3d,
                             shift=shift, lowest_level=lowest, dimension="3d")
    assert np.linalg.norm(f - (A @ flat(y) - shift * flat(y))) < np.linalg.norm(f)          # the oracle's own residual falls
    return f, y


@pytest.mark.parametrize("profile", ["smooth", "rough"])
@pytest.mark.parametrize("smoother", ["wjacobi", "gseidel_rb"])
@pytest.mark.parametrize("shift", [0.0, 0.7])
@pytest.mark.parametrize("g,lowest", [(8, 2), (8, 8), (16, 4), (32, 8), (64, 8)])
def test_vcycle_vs_oracle(backend, g, lowest, shift, smoother, profile):
    """V(2,2) for (H - shift I) v = f.  64^3 is the smallest grid on which the kernels of kernels_3d_stencil.hip run: asserted
    through mgcmt_plan3d_level_path."""
    op, A = problem(g, profile)
    f, y = oracle_cycle(g, lowest, shift, smoother, profile)
    solver = MGCMTSolver()
    n = g ** 3
    kw = dict(nu1=2, nu2=2, shift=shift, lowest_level=lowest, dimension="3d", smoother=None if smoother == "wjacobi" else solver.gseidel_rb)
    x = solver.vcycle(np.zeros(n), f.copy(), op, MGCMTStencilMaker(), **kw)
    assert x.shape == ((n, 1) if lowest == g else (n,))
    assert rel_err(flat(x), flat(y)) < TOL
    if g <= 16:          # the assembled matrix through recognise_27_point inside the 3-D entry point
        assert rel_err(flat(solver.vcycle(np.zeros(n), f.copy(), A, MGCMTStencilMaker(), **kw)), flat(y)) < TOL
    plan = get_plan(op, lowest, nvec=1)
    assert plan.level_path_3d(0) == (_lib.PATH3D_SEVEN_PLANES, g == 64)
    if g > lowest:
        assert plan.level_path_3d(1) == (_lib.PATH3D_PLANES, False)


@pytest.mark.parametrize("smoother", ["wjacobi", "gseidel_rb"])
def test_vcycle_nonzero_start_and_repeat(backend, smoother):
    # a non-zero start vector, and the same call three times (the second captures the cycle's graph, the third replays it)
    g = 16
    op, A = problem(g, "rough")
    rng = np.random.RandomState(2)
    f, v0 = rng.rand(g ** 3), rng.rand(g ** 3)
    solver, ref = MGCMTSolver(), Ref3dSolver()
    ours, theirs = (None, None) if smoother == "wjacobi" else (solver.gseidel_rb, mc_3d)
    kw = dict(nu1=2, nu2=2, shift=0.7, lowest_level=4, dimension="3d")
    y = ref.vcycle(v0.copy(), f.copy(), A, Ref3dStencilMaker(), smoother=theirs, **kw)
    for _ in range(3):
        assert rel_err(solver.vcycle(v0.copy(), f.copy(), op, MGCMTStencilMaker(), smoother=ours, **kw), y) < TOL


@pytest.mark.parametrize("smoother", ["wjacobi", "gseidel_rb"])
def test_vcycle_matrix_with_column_shifts(backend, smoother):
    g, k = 16, 3
    op, A = problem(g, "rough")
    n = g ** 3
    Fm = np.random.RandomState(5).rand(n, k)
    shifts = np.array([0.0, 0.35, 0.7])
    solver, ref = MGCMTSolver(), Ref3dSolver()
    ours, theirs = (None, None) if smoother == "wjacobi" else (solver.gseidel_rb, mc_3d)
    kw = dict(nu1=2, nu2=2, shifts=shifts, lowest_level=4, dimension="3d")
    y = ref.vcycle_matrix(np.zeros((n, k)), Fm.copy(), A, Ref3dStencilMaker(), smoother=theirs, **kw)
    for start in (op, A):
        x = solver.vcycle_matrix(np.zeros((n, k)), Fm.copy(), start, MGCMTStencilMaker(), smoother=ours, **kw)
        assert x.shape == (n, k)
        assert rel_err(x, y) < TOL


def test_foreign_smoother_sees_the_level_matrices(backend):
    """A callable smoother receives (R A P - shift I) of every level, level 0 with its 27 planes included."""
    g, lowest = 16, 4
    op, A = problem(g, "rough")
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


def mixed_operator(g):
    """a separable potential kept in the (then non-Toeplitz) factors plus the rough profile's stencil: level 0 is "general terms
    + 27 planes" (kind 3), the flat kernels through p27::general"""
    base = tensor_op(g, "rough")
    t = (np.arange(g) + 0.5) / g - 0.5
    terms = [tuple(a.copy() for a in term) for term in base.terms]
    terms[0][2][1] += 6.0 * np.cos(3.0 * t) + 6.0          # along x
    terms[2][0][1] += 25.0 * t * t + np.random.RandomState(7).rand(g)          # along z
    return StructuredOperator("3d", g, terms, point_stencil=base.point_stencil)


@pytest.mark.parametrize("g,lowest", [(8, 2), (16, 4)])
def test_general_terms_plus_point_stencil(backend, g, lowest):
    op = mixed_operator(g)
    A = op.tocsr()
    n = g ** 3
    plan = Plan(op, lowest, nvec=1)
    try:
        chain = galerkin_chain(A, g, lowest)
        plan.set_shifts([0.7])
        rng = np.random.RandomState(g)
        for level, want in enumerate(chain):
            assert plan.level_path_3d(level) == (_lib.PATH3D_PLANES, False)
            assert abs(assemble_level(plan, level) - want).max() <= 1e-13 * abs(want).max(), level
            x = rng.rand(want.shape[0]) - 0.5
            plan.upload(level, V, 0, x)
            plan.apply(level, (V, 0), (T, 0), with_shift=True)
            assert rel_err(plan.download(level, T, 0), want @ x - 0.7 * x) < 1e-13, level
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
        for _ in range(2):
            assert rel_err(solver.vcycle(v0.copy(), f.copy(), op, MGCMTStencilMaker(), smoother=ours, **kw), y) < TOL


# ---- 6. the kernels of kernels_3d_stencil.hip against the flat ones, bit for bit ------------------------------------------------

def run_forms(monkeypatch, make_plan, level, modes, cycle_level=None):
    """{mode: results} of the passes of `level` on plans created with MGCMT_3D_STENCIL_TILE = mode: the colour sweep with nu = 1
    and 2, residual + restriction (F and V of the level below), the same for three columns with their own shifts, a V(2,2) cycle
    with each smoother from `cycle_level`"""
    out = {}
    for mode, tiled in modes:
        if mode is None:
            monkeypatch.delenv("MGCMT_3D_STENCIL_TILE", raising=False)
        else:
            monkeypatch.setenv("MGCMT_3D_STENCIL_TILE", mode)
        p = make_plan()
        try:
            assert p.level_path_3d(level)[1] == tiled, mode
            n = p.size(level)
            rng = np.random.RandomState(64)
            v0, f = rng.rand(3, n), rng.rand(3, n)

            def load(k):
                for q in range(k):
                    p.upload(level, V, q, v0[q])
                    p.upload(level, F, q, f[q])

            def get(l, slot, k):
                return np.stack([np.array(p.download(l, slot, q)) for q in range(k)])

            res = {}
            for k, shifts in ((1, [0.0]), (3, [0.0, 0.35, 0.7])):
                p.set_shifts(shifts)
                for nu, omega in ((1, 1.0), (2, 1.0), (1, 1.3)) if k == 1 else ((2, 1.0),):
                    load(k)
                    p.smooth(level, _lib.GS_MC, nu, omega=omega, k=k)
                    res["colour", k, nu, omega] = get(level, V, k)
                load(k)
                p.residual_restrict(level, k=k)
                res["restrict_F", k] = get(level + 1, F, k)
                res["restrict_V", k] = get(level + 1, V, k)
                assert not res["restrict_V", k].any()
            if cycle_level is not None:
                p.set_shifts([0.0, 0.7])
                for kind, omega in ((_lib.WJACOBI, 2. / 3.), (_lib.GS_MC, 1.0)):
                    nc = p.size(cycle_level)
                    for q in range(2):
                        p.upload(cycle_level, V, q, v0[q][:nc])
                        p.upload(cycle_level, F, q, f[q][:nc])
                    p.vcycle(2, 2, kind, omega=omega, k=2, nu_coarse=2, level=cycle_level)
                    res["cycle", kind] = get(cycle_level, V, 2)
            out[mode] = res
        finally:
            p.close()
    return out


def assert_same_bits(a, b, cycle_tol=None):
    assert a.keys() == b.keys()
    for key in a:
        if key[0] == "cycle" and cycle_tol is not None:
            assert rel_err(a[key], b[key]) < cycle_tol, key
        else:
            assert np.array_equal(a[key], b[key]), key
            assert np.all(np.isfinite(a[key])), key


def test_new_kernels_give_the_flat_kernels_bits_64(backend, monkeypatch):
    """level 0 of a 64^3 tensor plan (two tiles along every axis): every pass and a whole cycle bit for bit; the default is "1" """
    op, _ = problem(64, "rough")
    r = run_forms(monkeypatch, lambda: Plan(op, 8, nvec=3), 0, ((None, True), ("0", False), ("2", True)), cycle_level=0)
    assert_same_bits(r[None], r["0"])
    assert_same_bits(r["2"], r["0"])


@pytest.mark.gpu
def test_new_kernels_give_the_flat_kernels_bits_128_gpu(hip_only, monkeypatch):
    """the same at 128^3 (four tiles along x and y, eight chunks), on the device only"""
    op = tensor_op(128, "rough")
    r = run_forms(monkeypatch, lambda: Plan(op, 8, nvec=3), 0, ((None, True), ("0", False)), cycle_level=0)
    assert_same_bits(r[None], r["0"])


def test_galerkin_level_on_the_new_kernels_64(backend, monkeypatch):
    """MGCMT_3D_STENCIL_TILE=2 on level 1 (64^3, general Kronecker terms plus 27 planes) of a 128^3 point-diagonal plan: per pass bit
    for bit and per cycle (from level 1 down) to 1e-13; without the variable the level stays flat"""
    g = 128
    op = potential_operator(g, smooth_w(g)[6] + 5.0 * np.random.RandomState(1).rand(g, g, g), dimension="3d")
    r = run_forms(monkeypatch, lambda: Plan(op, 8, nvec=3), 1, ((None, False), ("2", True)), cycle_level=1)
    assert_same_bits(r["2"], r[None], cycle_tol=1e-13)


# ---- 7. equal-size reduction -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_reductions(g, smoother):
    _, A = problem(g, "smooth")
    n = g ** 3
    f = np.random.RandomState(1).rand(n)
    v = np.zeros(n)
    norms = [np.linalg.norm(f)]
    for _ in range(5):
        v = flat(Ref3dSolver().vcycle(v, f.copy(), A, Ref3dStencilMaker(), nu1=2, nu2=2, smoother=None if smoother == "wjacobi" else mc_3d,
                                      lowest_level=4, dimension="3d"))
        norms.append(np.linalg.norm(f - A @ v))
    return f, np.array(norms[1:]) / np.array(norms[:-1])


@pytest.mark.parametrize("smoother", ["wjacobi", "gseidel_rb"])
def test_reduction_factors_equal_the_oracles_at_the_same_size_64(backend, smoother):
    """five V(2,2) cycles from zero at 64^3, smooth profile, lowest_level = 4: the residual falls in every cycle and the library's
    per-cycle reduction factors are the oracle's at the same size to 1e-6"""
    g = 64
    op, A = problem(g, "smooth")
    f, want = oracle_reductions(g, smoother)
    solver = MGCMTSolver()
    v = np.zeros(g ** 3)
    norms = [np.linalg.norm(f)]
    for _ in range(5):
        v = flat(solver.vcycle(v, f.copy(), op, MGCMTStencilMaker(), nu1=2, nu2=2, smoother=None if smoother == "wjacobi" else solver.gseidel_rb,
                               lowest_level=4, dimension="3d"))
        norms.append(np.linalg.norm(f - A @ v))
    got = np.array(norms[1:]) / np.array(norms[:-1])
    print("reduction factors", smoother, got, want)
    assert np.all(want < 1.0) and np.all(got < 1.0)
    assert np.abs(got - want).max() < 1e-6


# ---- 8. eigenpairs -----------------------------------------------------------------------------------------------------------

def test_block_eigensolve_against_eigsh(backend):
    import scipy.sparse.linalg as sla
    g, k = 16, 3
    wxx, wyy, wzz, wxy, wxz, wyz, Vp = rough_w(g)
    t = (np.arange(g) + 0.5) / g - 0.5
    Z, Y, X = np.meshgrid(t, t, t, indexing="ij")
    Vp = Vp + 60.0 * (X * X + 1.3 * Y * Y + 1.7 * Z * Z)          # a confining parabola
    op = tensor_mass_operator(g, wxx, wyy, wxy, V=Vp, wzz=wzz, wxz=wxz, wyz=wyz, dimension="3d")
    assert op.point_stencil is not None
    vals, vecs = drivers.block_eigensolve(op, k=k, cycles=24, lowest=4)
    want = np.sort(sla.eigsh(op.tocsr(), k=k, sigma=0.0, which="LM")[0])
    assert np.allclose(vals, want, rtol=0, atol=1e-8), np.abs(vals - want)
    assert np.abs(vecs.T @ vecs - np.eye(k)).max() < 1e-10


# ---- 9. what stays unsupported -----------------------------------------------------------------------------------------------

def test_refusals_on_a_3d_stencil_plan(backend):
    g = 8
    op, A = problem(g, "rough")
    plan = Plan(op, 2, nvec=6)
    L, h = _lib.lib(), plan._h
    U = -4  # MGCMT_ERR_UNSUPPORTED
    vecs = (ctypes.c_int * 6)(0, 1, 2, 3, 4, 5)
    pair = (ctypes.c_int * 2)(0, 0)
    dbl = ctypes.c_double(0.0)
    out = np.zeros(8)
    dp = _lib.as_dp(out)
    calls = {
        "twogrid": lambda: L.mgcmt_twogrid(h, 0, 2, 2, _lib.WJACOBI, ctypes.c_double(1.0), 1, None),
        "rayleigh_residual": lambda: L.mgcmt_rayleigh_residual(h, 0, 0, 1, dp, dp, None),
        "rqmin": lambda: L.mgcmt_rqmin(h, 0, 0, vecs, 2, 0, ctypes.byref(dbl), None),
        "rq_line_step": lambda: L.mgcmt_rq_line_step(h, 0, pair, None, pair, pair, None, 0, -1, None),
        "vcycle_rqmg": lambda: L.mgcmt_vcycle_rqmg(h, 0, vecs, 2, 2, 0, ctypes.byref(dbl), None),
        "smooth_lex": lambda: L.mgcmt_smooth(h, 0, _lib.GS_LEX, 1, ctypes.c_double(1.0), 1, None),
        "smooth_sor": lambda: L.mgcmt_smooth(h, 0, _lib.SOR_LEX, 1, ctypes.c_double(1.5), 1, None),
        "vcycle_lex": lambda: L.mgcmt_vcycle(h, 0, 2, 2, 2, _lib.GS_LEX, ctypes.c_double(1.0), 1, 0, None),
    }
    try:
        for name, call in calls.items():
            assert call() == U, name
            msg = L.mgcmt_last_error()
            assert b"3-D" in msg or b"point diagonal" in msg, (name, msg)
        assert L.mgcmt_apply(h, _lib.OP_M, 0, 0, 0, 2, 0, 0, None) != 0          # there is no mass operator
        # creation: a NULL stencil, lowest > 16, a coefficient towards the outside, an unsymmetric stencil
        nterms, zfac, yfac, xfac = op.factor_blocks()
        desc = _lib.Plan3dDesc()
        desc.nterms, desc.nvec, desc.g, desc.lowest = nterms, 1, g, 2
        desc.zfac, desc.yfac, desc.xfac = _lib.as_dp(zfac), _lib.as_dp(yfac), _lib.as_dp(xfac)
        hh = ctypes.c_void_p()
        G = np.ascontiguousarray(op.point_stencil)
        assert L.mgcmt_plan_create3d_stencil(ctypes.byref(desc), None, ctypes.byref(hh)) == -1 and not hh.value
        for (a, b, c, zz, yy, xx) in ((0, 1, 1, 0, 3, 3), (1, 2, 1, 3, g - 1, 3), (1, 1, 0, 3, 3, 0), (2, 2, 2, 1, 1, g - 1)):
            bad = G.copy()
            bad[a, b, c][zz, yy, xx] = 1.0
            assert L.mgcmt_plan_create3d_stencil(ctypes.byref(desc), _lib.as_dp(bad), ctypes.byref(hh)) == -1 and not hh.value
            assert b"outside" in L.mgcmt_last_error()
        bad = G.copy()
        bad[1, 2, 0][3, 3, 3] += 0.5
        assert L.mgcmt_plan_create3d_stencil(ctypes.byref(desc), _lib.as_dp(bad), ctypes.byref(hh)) == -1 and not hh.value
        assert b"symmetric" in L.mgcmt_last_error()
        desc.g, desc.lowest = 32, 32
        big = np.zeros(27 * 32 ** 3)
        z32 = np.zeros((nterms, 3, 32))
        desc.zfac, desc.yfac, desc.xfac = _lib.as_dp(z32), _lib.as_dp(z32), _lib.as_dp(z32)
        assert L.mgcmt_plan_create3d_stencil(ctypes.byref(desc), _lib.as_dp(big), ctypes.byref(hh)) == -1 and not hh.value
        assert b"16" in L.mgcmt_last_error()
    finally:
        plan.close()
    # Python: the lexicographic smoothers raise, naming what is supported; a mass operator, sharding and the Rayleigh-quotient
    # routines are refused
    solver, sm = MGCMTSolver(), MGCMTStencilMaker()
    v0, f = np.zeros(g ** 3), np.ones(g ** 3)
    for bad in (solver.gseidel, solver.sor):
        for start in (op, A):
            with pytest.raises(ValueError, match="wjacobi"):
                solver.vcycle(v0.copy(), f.copy(), start, sm, smoother=bad, dimension="3d", lowest_level=2)
        with pytest.raises(ValueError, match="wjacobi"):
            solver.vcycle_matrix(np.zeros((g ** 3, 2)), np.ones((g ** 3, 2)), op, sm, smoother=bad, dimension="3d", lowest_level=2)
    with pytest.raises(ValueError, match="wjacobi, gseidel_rb"):
        solver.gseidel(v0.copy(), f.copy(), op)
    with pytest.raises(ValueError, match="point stencil"):
        Plan(op, 2, nvec=10, mass=identity_operator(g, "3d"))
    with pytest.raises(ValueError, match="point stencil"):
        Plan(op, 2, row_begin=0, row_end=4)
    with pytest.raises(ValueError):
        solver.vcycle_rqmg(np.ones(g ** 3), op, identity_operator(g, "3d"))
    # an unsymmetric 27-point matrix keeps raising recognise's error at the 3-D entry point
    B = sp.lil_matrix(A)
    B[g * g + g + 1, g * g + 2 * g + 2] += 0.25
    with pytest.raises(UnrecognisedOperator):
        solver.vcycle(v0.copy(), f.copy(), B.tocsr(), sm, dimension="3d", lowest_level=2)
