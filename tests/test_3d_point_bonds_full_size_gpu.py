"""GPU-only checks of the 3-D plans with per-point bonds (mgcmt_plan_create3d_bonds) at sizes where the marching kernels of
csrc/kernels_3d_point.hip (k3pm_*<BONDS = true>) run on several x-tiles and z-chunks.  128^3 (two x-tiles, so Bx(x-1) crosses a tile edge; four
chunks): constant bonds handed over explicitly against the Kronecker plan of the correspondingly scaled Laplacian, zero bonds
plus a rough diagonal against the point-diagonal plan, and the marching kernels against the flat ones.  256^3: the convergence
on the smooth dot against the NumPy oracle's on the same profile at 32^3."""
import numpy as np
import pytest

from conftest import rel_err
from multigridcmt_amd import _lib
from multigridcmt_amd.operators import StructuredOperator, laplacian_operator, potential_operator, variable_mass_operator
from multigridcmt_amd.plan import Plan
from test_3d_cycle import Ref3dSolver, Ref3dStencilMaker

pytestmark = pytest.mark.gpu
SCALE = -1 / np.pi ** 2
SMOOTHERS = [(_lib.WJACOBI, 2. / 3.), (_lib.GS_MC, 1.0)]
V, F, W = _lib.SLOT_V, _lib.SLOT_F, _lib.SLOT_W
BONDS_PATHS = [(_lib.PATH3D_SEVEN_BONDS, True), (_lib.PATH3D_PLANES, False)]


@pytest.fixture(autouse=True, scope="module")
def _release_host_buffers():
    yield
    import gc
    from multigridcmt_amd import hostmem
    gc.collect()
    hostmem.drain()


def _two_cycles(op, f, kind, omega, lowest=8):
    """the iterates after one and two V(2,2) cycles from a zero start, and (kind, marching) of levels 0 and 1"""
    p = Plan(op, lowest, nvec=1)
    try:
        p.set_shifts([0.0])
        p.upload(0, F, 0, f)
        p.vcycle(2, 2, kind, omega=omega, nu_coarse=2, zero_start=True)
        one = np.array(p.download(0, V, 0))
        p.vcycle(2, 2, kind, omega=omega, nu_coarse=2)
        return one, np.array(p.download(0, V, 0)), [p.level_path_3d(l) for l in range(2)]
    finally:
        p.close()


def _outward_zero(g, value):
    bx, by, bz = (np.full((g, g, g), value) for _ in range(3))
    bx[:, :, -1] = 0.0
    by[:, -1, :] = 0.0
    bz[-1, :, :] = 0.0
    return bx, by, bz


@pytest.mark.parametrize("kind,omega", SMOOTHERS)
def test_constant_bonds_equal_scaled_laplacian_128(hip_only, kind, omega):
    """1.5 (scale L) as a Kronecker plan against (scale L) plus the constant bonds 0.5 t and the constant diagonal -3 t that
    make up the rest (t the neighbour entry of scale L; 0.5 t and 3 t are exact, so both plans hold the same matrix)"""
    g = 128
    f = np.random.RandomState(21).rand(g ** 3)
    base = laplacian_operator(g, "3d") * SCALE
    want1, want2, paths = _two_cycles(base * 1.5, f, kind, omega)
    assert paths[0] == (_lib.PATH3D_SEVEN, True)
    t = SCALE * g * g
    op = StructuredOperator("3d", g, base.terms, point_diagonal=np.full((g, g, g), -3.0 * t), point_bonds=_outward_zero(g, 0.5 * t))
    got1, got2, paths = _two_cycles(op, f, kind, omega)
    assert paths == BONDS_PATHS
    assert rel_err(got1, want1) < 1e-10 and rel_err(got2, want2) < 1e-10


def _dot(g, sparse=True):
    """(w, V) of the smooth dot: rho the ellipsoidal radius, s = (1 + tanh((rho - 0.3) / 0.08)) / 2, w = 1 - 0.27 s, V = 30 s"""
    t = (np.arange(g) + 0.5) / g - 0.5
    Z, Y, X = np.meshgrid(t, t, t, indexing="ij", sparse=sparse)
    rho = np.sqrt((X - 0.05) ** 2 + ((Y + 0.03) / 0.8) ** 2 + ((Z - 0.02) / 0.6) ** 2)
    s = 0.5 * (1.0 + np.tanh((rho - 0.3) / 0.08))
    return 1.0 - 0.27 * s, 30.0 * s


@pytest.mark.parametrize("kind,omega", SMOOTHERS)
def test_zero_bonds_equal_point_diagonal_plan_128(hip_only, kind, omega):
    g = 128
    D = _dot(g)[1] + 5.0 * np.random.RandomState(1).rand(g, g, g)
    f = np.random.RandomState(22).rand(g ** 3)
    want1, want2, paths = _two_cycles(potential_operator(g, D, dimension="3d"), f, kind, omega)
    assert paths == [(_lib.PATH3D_SEVEN_POINT, True), (_lib.PATH3D_PLANES, False)]
    base = laplacian_operator(g, "3d") * SCALE
    got1, got2, paths = _two_cycles(StructuredOperator("3d", g, base.terms, point_diagonal=D, point_bonds=_outward_zero(g, 0.0)), f, kind, omega)
    assert paths == BONDS_PATHS
    assert rel_err(got1, want1) < 1e-10 and rel_err(got2, want2) < 1e-10


def test_marching_and_flat_forms_agree_128_bonds(hip_only, monkeypatch):
    """MGCMT_3D_POINT_MARCH=0 against the default: one Jacobi sweep and one red-black sweep (omega 1 and 1.3) bit for bit (both
    forms compute a point with the same inline functions), a V(2,2) cycle of each smoother to 1e-13 (the restriction sums in
    another order); two columns with the shifts [0, 1.9]"""
    g = 128
    w, v = _dot(g)
    rng = np.random.RandomState(1)
    op = variable_mass_operator(g, w + 0.2 * rng.rand(g, g, g), v + 5.0 * rng.rand(g, g, g), dimension="3d")
    rng = np.random.RandomState(128)
    v0, f = rng.rand(2, g ** 3), rng.rand(2, g ** 3)
    res = {}
    for march in (True, False):
        if march:
            monkeypatch.delenv("MGCMT_3D_POINT_MARCH", raising=False)
        else:
            monkeypatch.setenv("MGCMT_3D_POINT_MARCH", "0")
        p = Plan(op, 8, nvec=2)
        try:
            assert p.level_path_3d(0) == (_lib.PATH3D_SEVEN_BONDS, march)
            p.set_shifts([0.0, 1.9])
            out = []
            for what, kind, omega in (("sweep", _lib.WJACOBI, 2. / 3.), ("sweep", _lib.GS_MC, 1.0), ("sweep", _lib.GS_MC, 1.3),
                                      ("cycle", _lib.WJACOBI, 2. / 3.), ("cycle", _lib.GS_MC, 1.0)):
                for q in range(2):
                    p.upload(0, V, q, v0[q])
                    p.upload(0, F, q, f[q])
                if what == "sweep":
                    p.smooth(0, kind, 1, omega=omega, k=2)
                else:
                    p.vcycle(2, 2, kind, omega=omega, k=2, nu_coarse=2)
                out.append(np.stack([np.array(p.download(0, V, q)) for q in range(2)]))
            res[march] = out
        finally:
            p.close()
    for i in (0, 1, 2):
        assert np.array_equal(res[True][i], res[False][i]), i
    for i in (3, 4):
        assert rel_err(res[True][i], res[False][i]) < 1e-13, i


def _sine(g):
    x_ = (np.arange(g) + 1.0) / (g + 1)
    s = np.sin(np.pi * x_) * (1 + 0.5 * x_)
    return (s[:, None, None] * s[None, :, None] * s[None, None, :]).reshape(-1)


def test_vcycle_256_h_independent_reduction_bonds(hip_only):
    """Five V(2,2) Jacobi cycles (nu_coarse = 4) from zero on f = H u at 256^3, H the smooth dot: every factor is below 1 and
    the geometric-mean residual reduction is no worse than 1.1 x the NumPy oracle's for the same profile at 32^3 (the one-sided
    bound of DESIGN par. 4.12).  Both lists are printed."""
    g = 256
    w, v = _dot(g, sparse=False)
    p = Plan(variable_mass_operator(g, w, v, dimension="3d"), 8, nvec=1)
    del w, v
    try:
        assert [p.level_path_3d(l) for l in range(2)] == BONDS_PATHS
        p.set_shifts([0.0])
        p.upload(0, V, 0, _sine(g))
        p.apply(0, (V, 0), (F, 0))                                     # f = H u
        res = [np.sqrt(p.dot(0, (F, 0), (F, 0)))]
        for cycle in range(5):
            p.vcycle(2, 2, _lib.WJACOBI, omega=2. / 3., nu_coarse=4, zero_start=cycle == 0)
            p.apply(0, (V, 0), (W, 0))
            p.axpy(0, -1.0, (F, 0), (W, 0))
            res.append(np.sqrt(p.dot(0, (W, 0), (W, 0))))
    finally:
        p.close()
    ours = np.array(res[1:]) / np.array(res[:-1])
    gs = 32
    A = variable_mass_operator(gs, *_dot(gs, sparse=False), dimension="3d").tocsr()
    f = A @ _sine(gs)
    u, rres = np.zeros(gs ** 3), [np.linalg.norm(f)]
    for _ in range(5):
        u = np.asarray(Ref3dSolver().vcycle(u.copy(), f.copy(), A, Ref3dStencilMaker(), nu1=2, nu2=2, lowest_level=8, dimension="3d")).reshape(-1)
        rres.append(np.linalg.norm(f - A @ u))
    ref = np.array(rres[1:]) / np.array(rres[:-1])
    print("residual reduction per cycle  256^3: %s  oracle 32^3: %s" % (np.round(ours, 4).tolist(), np.round(ref, 4).tolist()))
    assert np.all(ours < 1.0)
    a, b = np.exp(np.log(ours).mean()), np.exp(np.log(ref).mean())
    assert a <= 1.1 * b, (ours, ref)
