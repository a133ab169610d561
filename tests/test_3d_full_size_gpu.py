"""3-D path at full size on the MI355X: 128^3 cycles against the oracle, one 512^3 weighted-Jacobi sweep against the
closed form on a sine mode, and the 512^3 cycle's residual reduction against the oracle's at 32^3 (h-independence)."""
import numpy as np
import pytest

from conftest import bind_backend, rel_err
from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker
from multigridcmt_amd.operators import laplacian_operator
from test_3d_cycle import Ref3dSolver, Ref3dStencilMaker, mc_3d

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _release_host_buffers():
    """the GB-sized result arrays of this module go back to the page-locked pool and the pool is emptied afterwards"""
    yield
    import gc
    from multigridcmt_amd import hostmem
    gc.collect()
    hostmem.drain()


@pytest.mark.parametrize("smoother", ["wjacobi", "gseidel_rb"])
def test_vcycle_128_vs_oracle(smoother):
    bind_backend("hip")
    g = 128
    A = (-1 / np.pi ** 2) * MGCMTStencilMaker().laplacian(g, dimension="3d")
    f = np.random.RandomState(0).rand(g ** 3)
    solver = MGCMTSolver()
    ours, theirs = (None, None) if smoother == "wjacobi" else (solver.gseidel_rb, mc_3d)
    x = solver.vcycle(np.zeros(g ** 3), f.copy(), A, MGCMTStencilMaker(), nu1=2, nu2=2, smoother=ours, shift=1.9, lowest_level=8,
                      dimension="3d")
    y = Ref3dSolver().vcycle(np.zeros(g ** 3), f.copy(), A, Ref3dStencilMaker(), nu1=2, nu2=2, smoother=theirs, shift=1.9, lowest_level=8,
                             dimension="3d")
    assert rel_err(x, y) < 1e-10


def _sine(g):
    s = np.sin(np.pi * np.arange(1, g + 1) / (g + 1))
    return s


def test_jacobi_sweep_512_sine_mode():
    bind_backend("hip")
    g = 512
    op = laplacian_operator(g, "3d")
    s = _sine(g)
    u = (s[:, None, None] * s[None, :, None] * s[None, None, :]).reshape(-1)
    omega = 2. / 3.
    x = MGCMTSolver().wjacobi(u.copy(), np.zeros(g ** 3), op, nu=1, omega=omega).reshape(-1)   # (wjacobi reshapes its v0 to (n, 1))
    n2 = float(g) ** 2
    lam = 3.0 * n2 * (2.0 * np.cos(np.pi / (g + 1)) - 2.0)      # eigenvalue of the 7-point operator on this mode
    d = -6.0 * n2
    want = (1.0 - omega * lam / d) * u
    assert rel_err(x, want) < 1e-12


def _reduction_factors(g, cycles, ours):
    x_ = (np.arange(g) + 1.0) / (g + 1)
    s = np.sin(np.pi * x_) * (1 + 0.5 * x_)
    u = (s[:, None, None] * s[None, :, None] * s[None, None, :]).reshape(-1)
    scale = -1 / np.pi ** 2
    if ours:
        A = scale * laplacian_operator(g, "3d")
        f = A.dot(u)
        solver, sm = MGCMTSolver(), MGCMTStencilMaker()
    else:
        A = scale * Ref3dStencilMaker().laplacian(g)
        f = A @ u
        solver, sm = Ref3dSolver(), Ref3dStencilMaker()
    v = np.zeros(g ** 3)
    res = [np.linalg.norm(f)]
    for _ in range(cycles):
        v = np.asarray(solver.vcycle(v, f.copy(), A, sm, nu1=2, nu2=2, lowest_level=8, dimension="3d")).reshape(-1)
        res.append(np.linalg.norm(f - np.asarray(A.dot(v) if ours else A @ v).reshape(-1)))
    return np.array(res[1:]) / np.array(res[:-1])


def test_vcycle_512_h_independent_reduction():
    bind_backend("hip")
    ours = _reduction_factors(512, 5, True)
    ref = _reduction_factors(32, 5, False)
    print("residual reduction per cycle  512^3: %s  oracle 32^3: %s" % (np.round(ours, 4), np.round(ref, 4)))
    assert np.all(ours < 1.0)
    # h-independence: the mean factor over the five cycles (geometric) no worse than 1.1 x the oracle's at 32^3.  Measured on
    # the MI355X: 512^3 [0.180 0.107 0.098 0.104 0.155] (mean 0.125), oracle 32^3 [0.179 0.108 0.111 0.166 0.273] (mean 0.158):
    # the fine grid converges faster on this smooth problem, so a two-sided 10 % band does not hold; the bound is one-sided
    a, b = np.exp(np.log(ours).mean()), np.exp(np.log(ref).mean())
    assert a <= 1.1 * b, (ours, ref)
