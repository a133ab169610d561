"""Rayleigh-quotient eigensolvers on 3-D grids (rqmin, vcycle_rqmg, vcycle_rqmg2, the cube-well driver, block_eigensolve)
against a 3-D restatement of the NumPy oracle, through the HIP library on the GPU box and the emulated kernels on CPU
(``backend`` fixture)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as sla

from conftest import rel_err
from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, _lib, drivers
from multigridcmt_amd.operators import StructuredOperator, identity_operator, laplacian_operator, potential_well_operator
from multigridcmt_amd.plan import Plan, get_plan
from oracle.sparse_ref import RefSolver
from test_3d_cycle import Ref3dStencilMaker

RHO_TOL, X_TOL = 1e-10, 1e-8        # tests/test_fuzz.py's tolerances with the exact pencil


@pytest.fixture(autouse=True, scope="module")
def _release_host_buffers():
    yield
    import gc
    from multigridcmt_amd import hostmem
    gc.collect()
    hostmem.drain()


class Ref3dRQSolver(RefSolver):
    """vcycle_rqmg / vcycle_rqmg2 (MGCMTSolver.py:59-122) with the 3-D transfers: n = cube root of the length, restriction
    (1/8) P^T, the Galerkin pair (R A P, R M P) per level.  rqmin is the oracle's own (dimension-free)."""
    exact_pencil = True

    def __init__(self):
        super().__init__()
        self.sm3 = Ref3dStencilMaker()

    def vcycle_rqmg(self, x, A, M, nu1=4, nu2=4, nmin=2, dimension="3d"):
        k = np.array(x, dtype=float).reshape(-1)
        n = int(round(len(k) ** (1.0 / 3.0)))
        k, rho = self.rqmin(A, k, M, nu=nu1)
        if n > nmin:
            P = self.sm3.interpolation(n // 2, n)
            R = self.sm3.restriction(n, n // 2)
            c, rho = self.vcycle_rqmg(R @ k, R @ A @ P, R @ M @ P, nu1=nu1, nu2=nu2, nmin=nmin)
            k = k + P @ c
            k, rho = self.rqmin(A, k, M, nu=nu2)
        return k, rho

    def vcycle_rqmg2(self, x_matrix, A, M, nu1=4, nu2=4, nmin=2, level=0):
        k = np.array(x_matrix, dtype=float)
        n3, nv = k.shape
        n = int(round(n3 ** (1.0 / 3.0)))
        for i in range(nv):
            k[:, i], _ = self.rqmin(A, k[:, i], M, nu=nu1)
        if level == 0:
            for _ in range(4):
                k = self.processor.gramschmidt(k)
        if n > nmin:
            P = self.sm3.interpolation(n // 2, n)
            R = self.sm3.restriction(n, n // 2)
            c = self.vcycle_rqmg2(R @ k, R @ A @ P, R @ M @ P, nu1=nu1, nu2=nu2, nmin=nmin, level=level + 1)
            for i in range(nv):
                k[:, i] = k[:, i] + P @ c[:, i]
                k[:, i], _ = self.rqmin(A, k[:, i], M, nu=nu2)
        return k


def kron_operator(g, seed=0):
    """a scaled 3-D Laplacian plus a separable diagonal a(z) + b(y) + c(x), built from krons"""
    L = (-1 / np.pi ** 2) * MGCMTStencilMaker().laplacian(g, dimension="1d")
    rng = np.random.RandomState(seed)
    I = sp.identity(g, format="csr")
    a, b, c = (sp.diags(rng.rand(g) * 5.0) for _ in range(3))
    return (sp.kron(L + a, sp.kron(I, I)) + sp.kron(I, sp.kron(L + b, I)) + sp.kron(I, sp.kron(I, L + c))).tocsr()


def tri_mass(g):
    """M = (tridiag(1, 4, 1) / 6)^(x)3 as a structured operator (one Kronecker term, 27 points)"""
    m = np.zeros((3, g))
    m[0, 1:], m[1], m[2, :-1] = 1 / 6, 4 / 6, 1 / 6
    return StructuredOperator("3d", g, [(m, m.copy(), m.copy())])


def masses(g, which):
    """(what the solver is given, the matrix the oracle multiplies by)"""
    if which == "I":
        return sp.identity(g ** 3, format="csr"), sp.identity(g ** 3, format="csr")
    M = tri_mass(g)
    return M, M.tocsr()


@pytest.mark.parametrize("g", [8, 16, 32])
@pytest.mark.parametrize("mass", ["I", "tri"])
def test_rqmin_3d_vs_oracle(backend, g, mass):
    A = kron_operator(g, seed=g)
    Ms, Mr = masses(g, mass)
    x0 = np.random.RandomState(1).rand(g ** 3)
    x, rho = MGCMTSolver().rqmin(A, x0.copy(), Ms, nu=5)
    xr, rr = Ref3dRQSolver().rqmin(A, x0.copy(), Mr, nu=5)
    assert x.shape == (g ** 3,)
    assert abs(rho - rr) < RHO_TOL * abs(rr)
    assert rel_err(x, xr) < X_TOL


@pytest.mark.parametrize("g,nmin", [(8, 2), (8, 4), (16, 2), (16, 4), (16, 8), (32, 4), (32, 8)])
@pytest.mark.parametrize("mass", ["I", "tri"])
def test_vcycle_rqmg_3d_vs_oracle(backend, g, nmin, mass):
    A = (-1 / np.pi ** 2) * MGCMTStencilMaker().laplacian(g, dimension="3d") if mass == "I" else kron_operator(g, seed=3)
    Ms, Mr = masses(g, mass)
    x0 = np.random.RandomState(2).rand(g ** 3)
    solver, ref = MGCMTSolver(), Ref3dRQSolver()
    x, rho = solver.vcycle_rqmg(x0.copy(), A, Ms, nu1=2, nu2=2, nmin=nmin)
    xr, rr = ref.vcycle_rqmg(x0.copy(), A, Mr, nu1=2, nu2=2, nmin=nmin)
    assert abs(rho - rr) < RHO_TOL * abs(rr)
    assert rel_err(x, xr) < X_TOL
    # the second call replays the captured cycle
    x2, rho2 = solver.vcycle_rqmg(x0.copy(), A, Ms, nu1=2, nu2=2, nmin=nmin)
    assert rho2 == rho and np.array_equal(x2, x)


def test_vcycle_rqmg_3d_default_arguments(backend):
    g = 16
    A = (-1 / np.pi ** 2) * MGCMTStencilMaker().laplacian(g, dimension="3d")
    x0 = np.random.RandomState(4).rand(g ** 3)
    x, rho = MGCMTSolver().vcycle_rqmg(x0.copy(), A, sp.eye(g ** 3))
    xr, rr = Ref3dRQSolver().vcycle_rqmg(x0.copy(), A, sp.eye(g ** 3))
    assert abs(rho - rr) < RHO_TOL * abs(rr)
    assert rel_err(x, xr) < X_TOL


def test_vcycle_rqmg2_3d_vs_oracle(backend):
    g = 16
    A = (-1 / np.pi ** 2) * MGCMTStencilMaker().laplacian(g, dimension="3d")
    X0 = np.random.RandomState(5).rand(g ** 3, 2)
    X = MGCMTSolver().vcycle_rqmg2(X0.copy(), A, sp.eye(g ** 3), nu1=2, nu2=2, nmin=4)
    Xr = Ref3dRQSolver().vcycle_rqmg2(X0.copy(), A, sp.eye(g ** 3), nu1=2, nu2=2, nmin=4)
    assert X.shape == (g ** 3, 2)
    assert rel_err(X, Xr) < X_TOL


@pytest.mark.parametrize("switch,g,mass", [("MGCMT_RQ_SMALL", 16, "I"), ("MGCMT_RQ_SMALL", 16, "tri"), ("MGCMT_RQ_MARCH", 64, "I")])
def test_rq3d_forms_agree(backend, monkeypatch, switch, g, mass):
    """The single-workgroup form (levels of at most 16^3) against the passes, and the marching passes of the constant
    7-point level against the flat ones: the same arithmetic per point, other orders of the partial sums, so agreement
    to rounding (amplified by the steps' conditioning)."""
    A = (-1 / np.pi ** 2) * MGCMTStencilMaker().laplacian(g, dimension="3d")
    Ms, _ = masses(g, mass)
    x0 = np.random.RandomState(6).rand(g ** 3)
    out = {}
    for form in ("1", "0"):
        monkeypatch.setenv(switch, form)
        out[form] = MGCMTSolver().rqmin(A, x0.copy(), Ms, nu=5)
    (x1, rho1), (x0_, rho0) = out["1"], out["0"]
    assert abs(rho1 - rho0) < 1e-12 * abs(rho0)
    assert rel_err(x1, x0_) < 1e-10


def test_cube_well_3d_matches_eigsh(backend):
    g, depth = 32, 50.0
    H = potential_well_operator(g, depth, (g // 4, 3 * g // 4), dimension="3d").tocsr()
    lowest = sla.eigsh(H, k=1, which="SA", tol=1e-13)[0][0]
    hist = []
    rho, x = drivers.potential_well_eigensolve(g, depth=depth, cycles=14, method="vcycle", nu=2, lowest=8, dimension="3d", history=hist)
    assert abs(rho - lowest) < 1e-8 * lowest
    assert all(b <= a + 1e-12 for a, b in zip(hist, hist[1:]))          # Rayleigh-Ritz never increases rho
    assert np.linalg.norm(H @ x - rho * x) < 1e-5 * np.linalg.norm(x)
    # the reference's cycle (RQMin.py:25-27 with the 3-D transfers) stagnates: the coarse iterate it adds (:116-118) is the
    # coarse pair's eigenvector, not a correction.  The NumPy restatement stalls the same way; as in 2-D
    # (tests/test_drivers.py), 1e-3 of eigsh
    rho_mg, x_mg = drivers.potential_well_eigensolve(g, depth=depth, cycles=4, method="rqmg", nu=4, lowest=4, dimension="3d")
    assert x_mg.shape == (g ** 3,)
    assert lowest * (1 - 1e-12) <= rho_mg < lowest * (1 + 1e-3)


def test_block_eigensolve_3d_box(backend):
    g = 16
    op = laplacian_operator(g, "3d") * (-1 / np.pi ** 2)
    exact = drivers.exact_box_eigenvalues(g, "3d", 4)
    for mass in (None, identity_operator(g, "3d")):
        vals, vecs = drivers.block_eigensolve(op, k=4, cycles=14, nu=2, lowest=4, mass=mass)
        assert vecs.shape == (g ** 3, 4)
        assert np.allclose(vals, exact, rtol=1e-9, atol=0)


def test_exact_box_eigenvalues_3d():
    g = 8
    dense = (-1 / np.pi ** 2) * MGCMTStencilMaker().laplacian(g, dimension="3d").toarray()
    assert np.allclose(drivers.exact_box_eigenvalues(g, "3d", 10), np.linalg.eigvalsh(dense)[:10], rtol=1e-12, atol=0)
    one = drivers.exact_box_eigenvalues(g, "1d", 8)
    assert np.array_equal(drivers.exact_box_eigenvalues(g, "2d", 5), np.sort(np.add.outer(one[:7], one[:7]).ravel())[:5])


def test_cube_well_operator():
    g = 8
    H = potential_well_operator(g, 30.0, (2, 6), scale=-0.5, dimension="3d")
    chi = np.zeros(g)
    chi[2:6] = 1.0
    V = 30.0 * (1.0 - np.kron(chi, np.kron(chi, chi)))
    want = -0.5 * MGCMTStencilMaker().laplacian(g, dimension="3d") + sp.diags(V)
    assert len(H.terms) == 4
    assert abs(H.tocsr() - want).max() < 1e-12
    assert potential_well_operator(g, 30.0, (2, 6)).shape == (g * g, g * g)          # the 2-D default is unchanged


def test_mass_apply_3d(backend):
    g = 8
    M = tri_mass(g)
    plan = Plan(laplacian_operator(g, "3d"), 2, nvec=2, mass=M)
    x = np.random.RandomState(7).rand(g ** 3)
    plan.upload(0, _lib.SLOT_V, 0, x)
    plan.apply(0, (_lib.SLOT_V, 0), (_lib.SLOT_T, 0), op=_lib.OP_M)
    assert rel_err(plan.download(0, _lib.SLOT_T, 0), M.tocsr() @ x) < 1e-14
    plan.apply(0, (_lib.SLOT_V, 0), (_lib.SLOT_T, 0))
    assert rel_err(plan.download(0, _lib.SLOT_T, 0), laplacian_operator(g, "3d").tocsr() @ x) < 1e-14
    # the coarse levels' M is R M P, per axis
    P, R = Ref3dStencilMaker().interpolation(4, 8), Ref3dStencilMaker().restriction(8, 4)
    xc = x[: 4 ** 3]
    plan.upload(1, _lib.SLOT_V, 0, xc)
    plan.apply(1, (_lib.SLOT_V, 0), (_lib.SLOT_T, 0), op=_lib.OP_M)
    assert rel_err(plan.download(1, _lib.SLOT_T, 0), (R @ M.tocsr() @ P) @ xc) < 1e-14
    plan.close()


def test_mass_errors_3d(backend):
    g = 8
    op = laplacian_operator(g, "3d")
    with pytest.raises(ValueError, match="same"):
        Plan(op, 2, mass=identity_operator(16, "3d"))
    with pytest.raises(ValueError, match="same"):
        Plan(op, 2, mass=identity_operator(g * g * g, "1d"))
    i = np.zeros((3, g))
    i[1] = 0.2
    five = StructuredOperator("3d", g, [(i.copy(), i.copy(), i.copy()) for _ in range(5)])
    with pytest.raises(ValueError, match="terms"):
        Plan(op, 2, mass=five)
    # the C-ABI refuses more than MGCMT_MAX_TERMS mass terms, or none
    nterms, zf, yf, xf = op.factor_blocks()
    desc = _lib.Plan3dDesc()
    desc.nterms, desc.nvec, desc.g, desc.lowest = nterms, 1, g, 2
    desc.zfac, desc.yfac, desc.xfac = _lib.as_dp(zf), _lib.as_dp(yf), _lib.as_dp(xf)
    h = ctypes.c_void_p()
    mz = np.ascontiguousarray(np.stack([i] * 5))
    for bad in (5, 0):
        assert _lib.lib().mgcmt_plan_create3d_mass(ctypes.byref(desc), bad, _lib.as_dp(mz), _lib.as_dp(mz), _lib.as_dp(mz), ctypes.byref(h)) == -1
    with pytest.raises(ValueError, match="nmin"):
        MGCMTSolver().vcycle_rqmg(np.ones(32 ** 3), laplacian_operator(32, "3d"), identity_operator(32, "3d"), nmin=32)
    with pytest.raises(ValueError, match="3-D"):
        MGCMTSolver().twogridrqmin(laplacian_operator(g, "3d"), np.ones(g ** 3), identity_operator(g, "3d"), repaired=True)


def test_rq_entries_need_a_mass_operator_on_3d(backend):
    """A mass-less 3-D plan keeps refusing the Rayleigh-quotient entries (before any argument check); with M = I they run."""
    L = _lib.lib()
    U = -4  # MGCMT_ERR_UNSUPPORTED
    vecs = (ctypes.c_int * 6)(0, 1, 2, 3, 4, 5)
    rho = ctypes.c_double(0.0)
    bare = get_plan(laplacian_operator(8, "3d"), 2, nvec=6)
    assert L.mgcmt_rqmin(bare._h, 0, 0, vecs, 2, 0, ctypes.byref(rho), None) == U
    assert b"3-D" in L.mgcmt_last_error()
    assert L.mgcmt_vcycle_rqmg(bare._h, 0, vecs, 2, 2, 0, ctypes.byref(rho), None) == U
    assert b"3-D" in L.mgcmt_last_error()
    assert L.mgcmt_apply(bare._h, _lib.OP_M, 0, 0, 0, 2, 0, 0, None) != 0
    plan = Plan(laplacian_operator(8, "3d") * (-1 / np.pi ** 2), 2, nvec=6, mass=identity_operator(8, "3d"))
    plan.set_shifts(np.zeros(6))
    plan.upload(0, _lib.SLOT_V, 0, np.random.RandomState(8).rand(512))
    r = plan.vcycle_rqmg(_lib.SLOT_V, list(vecs), 2, 2)
    assert abs(r - drivers.exact_box_eigenvalues(8, "3d", 1)[0]) < 0.05 * r           # one V(2,2) cycle from a random start
    # the line step records into the device-side history, which a mass-carrying 3-D plan serves
    plan.rq_line_step(0, (_lib.SLOT_V, 0), None, None, (_lib.SLOT_F, 0), record=0)
    assert abs(plan.rq_history(0, 1)[0] - r) < 1e-12 * r
    plan.close()
