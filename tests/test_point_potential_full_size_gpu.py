"""GPU-only checks of the per-point-diagonal plans at full size.  The C oracle has no per-point diagonal, so full size is
checked against paths that are pinned to it already: a constant point diagonal against the Kronecker plan with the constant
folded in, BASELINE config 5's square well handed over as a point diagonal against the Op5V / Op9cv plan, and the
convergence of a non-separable potential at 4096^2 against the NumPy oracle's on the same potential at 128^2."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import rel_err
from multigridcmt_amd import MGCMTStencilMaker, _lib
from multigridcmt_amd.operators import StructuredOperator, laplacian_operator, potential_operator, potential_well_operator
from multigridcmt_amd.plan import Plan
from oracle.sparse_ref import RefSolver, RefStencilMaker

pytestmark = pytest.mark.gpu
SCALE = -1 / np.pi ** 2
SMOOTHERS = [(_lib.WJACOBI, 2. / 3.), (_lib.GS_MC, 1.0)]


def _two_cycles(op, f, kind, omega, lowest=8):
    """the iterates after one and two V(2,2) cycles from a zero start (the second cycle starts from a non-zero iterate)"""
    p = Plan(op, lowest, nvec=1)
    try:
        p.set_shifts([0.0])
        p.upload(0, _lib.SLOT_F, 0, f)
        p.vcycle(2, 2, kind, omega=omega, nu_coarse=2, zero_start=True)
        one = np.array(p.download(0, _lib.SLOT_V, 0))
        p.vcycle(2, 2, kind, omega=omega, nu_coarse=2)
        return one, np.array(p.download(0, _lib.SLOT_V, 0)), [p.operator_kind(l) for l in range(2)]
    finally:
        p.close()


@pytest.mark.parametrize("kind,omega", SMOOTHERS)
def test_constant_point_diagonal_equals_folded_constant_8192(hip_only, kind, omega):
    g, c = 8192, 3.25
    f = np.random.RandomState(21).rand(g * g)
    base = laplacian_operator(g, "2d") * SCALE
    want1, want2, kinds = _two_cycles(base.shifted(-c), f, kind, omega)
    assert kinds[0] == _lib.OPK_FIVE_POINT
    got1, got2, kinds = _two_cycles(StructuredOperator("2d", g, base.terms, point_diagonal=np.full((g, g), c)), f, kind, omega)
    assert kinds == [_lib.OPK_POINT_DIAG, _lib.OPK_NINE_POINT]
    assert rel_err(got1, want1) < 1e-10 and rel_err(got2, want2) < 1e-10


@pytest.mark.parametrize("kind,omega", SMOOTHERS)
def test_square_well_as_point_diagonal_equals_op5v_plan_8192(hip_only, kind, omega):
    """BASELINE config 5's operator: depth (1 - chi (x) chi); the product term handed over as a point diagonal"""
    g, depth = 8192, 50.0
    well = potential_well_operator(g, depth, (g // 4, 3 * g // 4))
    chi = np.zeros(g)
    chi[g // 4:3 * g // 4] = 1.0
    f = np.random.RandomState(22).rand(g * g)
    want1, want2, kinds = _two_cycles(well, f, kind, omega)
    assert kinds == [_lib.OPK_FIVE_DIAG, _lib.OPK_NINE_VAR]
    as_point = StructuredOperator("2d", g, well.terms[:2], point_diagonal=-depth * np.outer(chi, chi))
    got1, got2, kinds = _two_cycles(as_point, f, kind, omega)
    assert kinds == [_lib.OPK_POINT_DIAG, _lib.OPK_NINE_POINT]
    assert rel_err(got1, want1) < 1e-10 and rel_err(got2, want2) < 1e-10


def _potential(g, noise):
    """40 (x^2 + x y + y^2) + 10 exp(-12 (x - y)^2) on the cell centres of [-1/2, 1/2]^2 plus disorder that is constant on
    the cells of a 128 x 128 grid (`noise`), so that every grid size samples the same potential"""
    x = (np.arange(g) + 0.5) / g - 0.5
    X, Y = np.meshgrid(x, x, indexing="ij")
    V = 40.0 * (X * X + X * Y + Y * Y) + 10.0 * np.exp(-12.0 * (X - Y) ** 2)
    return V + np.kron(noise, np.ones((g // 128, g // 128)))


def _sine(g):
    s = np.sin(np.pi * (np.arange(g) + 1.0) / (g + 1.0))
    return np.outer(s, s).reshape(-1)


@pytest.mark.parametrize("kind,omega", SMOOTHERS)
def test_non_separable_potential_4096_convergence(hip_only, kind, omega):
    """Five V(2,2) cycles (V(4,4) below the top level, as the reference's vcycle runs) from zero on f = H u at 4096^2:
    the fused fine-level pass (Op5P) and MGCMT_OPT_FUSED = 0 give the same bits, and the residual reduction of every cycle
    is no worse than 1.1 x what the NumPy oracle gives for the same potential sampled at 128^2 (the rule of DESIGN par.
    4.12, "Checks", applied per cycle).  Both sequences are printed."""
    noise = 5.0 * np.random.RandomState(1).rand(128, 128)
    g = 4096
    op = potential_operator(g, _potential(g, noise))
    V, F, W = (_lib.SLOT_V, 0), (_lib.SLOT_F, 0), (_lib.SLOT_W, 0)
    runs = {}
    for fused in (1, 0):
        p = Plan(op, 8, nvec=1)
        try:
            p.set_option(_lib.OPT_FUSED, fused)
            p.set_shifts([0.0])
            p.upload(0, _lib.SLOT_V, 0, _sine(g))
            p.apply(0, V, F)                                     # f = H u
            res = [np.sqrt(p.dot(0, F, F))]
            for cycle in range(5):
                p.vcycle(2, 2, kind, omega=omega, nu_coarse=4, zero_start=cycle == 0)
                p.apply(0, V, W)
                p.axpy(0, -1.0, F, W)
                res.append(np.sqrt(p.dot(0, W, W)))
            assert p.fused_max_sweeps(0, kind) == (2 if fused else 0)
            runs[fused] = (np.array(p.download(0, _lib.SLOT_V, 0)), np.array(res))
        finally:
            p.close()
    assert np.array_equal(runs[1][0], runs[0][0])
    got = runs[1][1][1:] / runs[1][1][:-1]
    # the oracle at 128^2
    gs = 128
    A = (SCALE * MGCMTStencilMaker().laplacian(gs, dimension="2d") + sp.diags(_potential(gs, noise).reshape(-1))).tocsr()
    ref, rsm = RefSolver(), RefStencilMaker()
    f = A @ _sine(gs)
    smoother = None if kind == _lib.WJACOBI else (lambda v, f, A, nu=4: ref.gseidel_mc(v, f, A, nu=nu, dimension="2d"))
    # (the reference does not forward nu1 / nu2 below the top level, MGCMTSolver.py:320: V(4,4) there — nu_coarse=4 above)
    v, rres = np.zeros(gs * gs), [np.linalg.norm(f)]
    for _ in range(5):
        v = np.asarray(ref.vcycle(v.copy(), f.copy(), A, rsm, nu1=2, nu2=2, smoother=smoother, lowest_level=8, dimension="2d")).reshape(-1)
        rres.append(np.linalg.norm(f - A @ v))
    want = np.array(rres[1:]) / np.array(rres[:-1])
    print("residual reduction per cycle, 4096^2 %s: %s; oracle at 128^2: %s" % ("wjacobi" if kind == _lib.WJACOBI else "red-black",
                                                                                 np.round(got, 4).tolist(), np.round(want, 4).tolist()))
    assert np.all(np.diff(rres) < 0)
    assert np.all(got <= 1.1 * want), (got, want)          # every cycle's factor
