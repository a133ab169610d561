"""GPU-only checks of the plans with per-point bonds at 2048^2, where level 0 runs the marching kernels with 256-thread blocks
and 64 row chunks.  The C oracle has no per-point part, so full size is checked against paths that are pinned to it already:
constant bonds against the Kronecker plan of the correspondingly scaled Laplacian, the marching kernels against the flat
ones, and the convergence for a smooth inverse mass against the NumPy oracle's on the same functions sampled at 128^2."""
import os

import numpy as np
import pytest

from conftest import rel_err
from multigridcmt_amd import _lib, variable_mass_operator
from multigridcmt_amd.operators import StructuredOperator, laplacian_operator
from multigridcmt_amd.plan import Plan
from oracle.sparse_ref import RefSolver, RefStencilMaker
from test_point_bonds import step_operator, w_smooth
from test_point_potential import smooth_v

pytestmark = pytest.mark.gpu
SCALE = -1 / np.pi ** 2
SMOOTHERS = [(_lib.WJACOBI, 2. / 3.), (_lib.GS_MC, 1.0)]
G = 2048


def _plan(op, march=True, lowest=8):
    old = os.environ.get("MGCMT_BONDS_MARCH")
    os.environ["MGCMT_BONDS_MARCH"] = "1" if march else "0"      # read by the library when the plan is created
    try:
        return Plan(op, lowest, nvec=1)
    finally:
        if old is None:
            del os.environ["MGCMT_BONDS_MARCH"]
        else:
            os.environ["MGCMT_BONDS_MARCH"] = old


def _two_cycles(p, f, kind, omega):
    p.set_shifts([0.0])
    p.upload(0, _lib.SLOT_F, 0, f)
    p.vcycle(2, 2, kind, omega=omega, nu_coarse=2, zero_start=True)
    one = np.array(p.download(0, _lib.SLOT_V, 0))
    p.vcycle(2, 2, kind, omega=omega, nu_coarse=2)
    return one, np.array(p.download(0, _lib.SLOT_V, 0))


def _constant_bond_pair(g, frac=0.5):
    """(the bond operator, the Kronecker operator) of the Laplacian scaled by (cw + delta) / cw, delta = frac * cw: constant
    E = S = delta (zero on the last column / row) and the matching constant D = -4 delta — the diagonal counts the bonds
    towards the ghost points too, as variable_mass_operator's rule says"""
    base = laplacian_operator(g, "2d") * SCALE
    cw = SCALE * g * g
    delta = frac * cw
    E, S = np.full((g, g), delta), np.full((g, g), delta)
    E[:, -1] = 0.0
    S[-1, :] = 0.0
    bond = StructuredOperator("2d", g, base.terms, point_diagonal=np.full((g, g), -4.0 * delta), point_bonds=(E, S))
    return bond, base * ((cw + delta) / cw)


@pytest.mark.parametrize("kind,omega", SMOOTHERS)
def test_constant_bonds_equal_the_scaled_laplacian_2048(hip_only, kind, omega):
    small_bond, small_kron = _constant_bond_pair(64)
    A, B = small_bond.tocsr(), small_kron.tocsr()
    assert abs(A - B).max() <= 1e-13 * abs(B).max()          # the same matrix, ghost bonds included
    bond, kron = _constant_bond_pair(G)
    f = np.random.RandomState(21).rand(G * G)
    p = Plan(kron, 8, nvec=1)
    try:
        assert p.operator_kind(0) == _lib.OPK_FIVE_POINT
        want1, want2 = _two_cycles(p, f, kind, omega)
    finally:
        p.close()
    p = _plan(bond)
    try:
        assert [p.operator_kind(l) for l in range(2)] == [_lib.OPK_POINT_BONDS, _lib.OPK_NINE_POINT]
        got1, got2 = _two_cycles(p, f, kind, omega)
    finally:
        p.close()
    assert rel_err(got1, want1) < 1e-10 and rel_err(got2, want2) < 1e-10


@pytest.mark.parametrize("kind,omega", SMOOTHERS)
def test_marching_kernels_against_the_flat_ones_2048(hip_only, kind, omega):
    """a sweep is bit-identical; the marching residual + restriction keeps k_restrict's order, so F[1] is bit-identical too;
    a V(2,2) cycle agrees to 1e-12"""
    op = step_operator(G)
    rng = np.random.RandomState(22)
    v0, f = rng.rand(G * G) - 0.5, rng.rand(G * G)
    out = {}
    for march in (False, True):
        p = _plan(op, march)
        try:
            p.set_shifts([0.7])
            p.upload(0, _lib.SLOT_V, 0, v0)
            p.upload(0, _lib.SLOT_F, 0, f)
            p.smooth(0, kind, 1, omega)
            sweep = np.array(p.download(0, _lib.SLOT_V, 0))
            p.residual_restrict(0)
            coarse = np.array(p.download(1, _lib.SLOT_F, 0))
            p.upload(0, _lib.SLOT_V, 0, v0)
            p.vcycle(2, 2, kind, omega=omega, nu_coarse=2)
            out[march] = (sweep, coarse, np.array(p.download(0, _lib.SLOT_V, 0)))
        finally:
            p.close()
    assert np.all(np.isfinite(out[True][2]))
    assert np.array_equal(out[True][0], out[False][0])
    assert np.array_equal(out[True][1], out[False][1])
    assert rel_err(out[True][2], out[False][2]) < 1e-12


@pytest.mark.parametrize("kind,omega", SMOOTHERS)
def test_smooth_mass_2048_convergence(hip_only, kind, omega):
    """Five V(2,2) cycles (V(4,4) below the top level, as the reference's vcycle runs) from zero on f = A u, u =
    RandomState(7).rand, for w_smooth / smooth_v: the geometric mean of the residual reduction is no worse than 1.1 x what
    the NumPy oracle gives for the same functions sampled at 128^2 (the margin of DESIGN par. 4.12 - 4.14; the oracle's mean
    does not depend on the size: 0.114 / 0.113 / 0.113 for Jacobi and 0.0099 / 0.0100 / 0.0099 for red-black at 128^2 /
    256^2 / 512^2).  Both figures are printed."""
    op = variable_mass_operator(G, w_smooth(G), smooth_v(G))
    V, F, W = (_lib.SLOT_V, 0), (_lib.SLOT_F, 0), (_lib.SLOT_W, 0)
    p = _plan(op)
    try:
        p.set_shifts([0.0])
        p.upload(0, _lib.SLOT_V, 0, np.random.RandomState(7).rand(G * G))
        p.apply(0, V, F)                                     # f = A u
        res = [np.sqrt(p.dot(0, F, F))]
        for cycle in range(5):
            p.vcycle(2, 2, kind, omega=omega, nu_coarse=4, zero_start=cycle == 0)
            p.apply(0, V, W)
            p.axpy(0, -1.0, F, W)
            res.append(np.sqrt(p.dot(0, W, W)))
    finally:
        p.close()
    got = (res[-1] / res[0]) ** 0.2
    gs = 128
    A = variable_mass_operator(gs, w_smooth(gs), smooth_v(gs)).tocsr()
    ref, rsm = RefSolver(), RefStencilMaker()
    f = A @ np.random.RandomState(7).rand(gs * gs)
    smoother = None if kind == _lib.WJACOBI else (lambda v, f, A, nu=4: ref.gseidel_mc(v, f, A, nu=nu, dimension="2d"))
    v, rres = np.zeros(gs * gs), [np.linalg.norm(f)]
    for _ in range(5):
        v = np.asarray(ref.vcycle(v.copy(), f.copy(), A, rsm, nu1=2, nu2=2, smoother=smoother, lowest_level=8, dimension="2d")).reshape(-1)
        rres.append(np.linalg.norm(f - A @ v))
    want = (rres[-1] / rres[0]) ** 0.2
    print("mean residual reduction per cycle, %d^2 %s: %.4f; oracle at 128^2: %.4f" % (G, "wjacobi" if kind == _lib.WJACOBI else "red-black", got, want))
    assert np.all(np.diff(rres) < 0) and np.all(np.diff(res) < 0)
    assert got <= 1.1 * want, (got, want)
