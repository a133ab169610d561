"""GPU-only checks of the 3-D plans with a per-point 27-point stencil (mgcmt_plan_create3d_stencil) at 128^3, where the kernels of
csrc/kernels_3d_stencil.hip run on four tiles along x and y and eight chunks of coarse planes: a diagonal tensor handed over as 27
planes against the plan with bonds, constant planes on top of the Kronecker Laplacian against the plan with the constant folded
into the Kronecker factors, and the new kernels against the flat ones cycle by cycle."""
import numpy as np
import pytest

from conftest import rel_err
from multigridcmt_amd import _lib
from multigridcmt_amd.operators import StructuredOperator, laplacian_operator, tensor_mass_operator
from multigridcmt_amd.plan import Plan
from test_3d_tensor_mass import smooth_w, tensor_op

pytestmark = pytest.mark.gpu
SCALE = -1 / np.pi ** 2
SMOOTHERS = [(_lib.WJACOBI, 2. / 3.), (_lib.GS_MC, 1.0)]
V, F = _lib.SLOT_V, _lib.SLOT_F
STENCIL_PATHS = [(_lib.PATH3D_SEVEN_PLANES, True), (_lib.PATH3D_PLANES, False)]


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


def _planes_of_bonds(D, Bx, By, Bz):
    """the 27 planes that hold a diagonal and bonds"""
    g = D.shape[0]
    G = np.zeros((3, 3, 3, g, g, g))
    G[1, 1, 1] = D
    G[1, 1, 2] = Bx
    G[1, 1, 0][:, :, 1:] = Bx[:, :, :-1]
    G[1, 2, 1] = By
    G[1, 0, 1][:, 1:, :] = By[:, :-1, :]
    G[2, 1, 1] = Bz
    G[0, 1, 1][1:, :, :] = Bz[:-1, :, :]
    return G


@pytest.mark.parametrize("kind,omega", SMOOTHERS)
def test_diagonal_tensor_as_stencil_equals_bonds_plan_128(hip_only, kind, omega):
    g = 128
    wxx, wyy, wzz, _, _, _, Vp = smooth_w(g)
    zero = np.zeros((g, g, g))
    bonds = tensor_mass_operator(g, wxx, wyy, zero, V=Vp, wzz=wzz, wxz=zero, wyz=zero, dimension="3d")
    assert bonds.point_bonds is not None and bonds.point_stencil is None
    f = np.random.RandomState(21).rand(g ** 3)
    want1, want2, paths = _two_cycles(bonds, f, kind, omega)
    assert paths[0] == (_lib.PATH3D_SEVEN_BONDS, True)
    op = StructuredOperator("3d", g, bonds.terms, point_stencil=_planes_of_bonds(bonds.point_diagonal, *bonds.point_bonds))
    got1, got2, paths = _two_cycles(op, f, kind, omega)
    assert paths == STENCIL_PATHS
    assert rel_err(got1, want1) < 1e-10 and rel_err(got2, want2) < 1e-10


@pytest.mark.parametrize("kind,omega", SMOOTHERS)
def test_constant_stencil_equals_scaled_laplacian_128(hip_only, kind, omega):
    """1.5 (scale L) as a Kronecker plan against (scale L) plus constant planes: 0.5 t on the six axis neighbours and -3 t on the
    centre (t the neighbour entry of scale L; 0.5 t and 3 t are exact, so both plans hold the same matrix)"""
    g = 128
    f = np.random.RandomState(22).rand(g ** 3)
    base = laplacian_operator(g, "3d") * SCALE
    want1, want2, paths = _two_cycles(base * 1.5, f, kind, omega)
    assert paths[0] == (_lib.PATH3D_SEVEN, True)
    t = SCALE * g * g
    b = [np.full((g, g, g), 0.5 * t) for _ in range(3)]
    b[0][:, :, -1] = 0.0
    b[1][:, -1, :] = 0.0
    b[2][-1, :, :] = 0.0
    op = StructuredOperator("3d", g, base.terms, point_stencil=_planes_of_bonds(np.full((g, g, g), -3.0 * t), *b))
    got1, got2, paths = _two_cycles(op, f, kind, omega)
    assert paths == STENCIL_PATHS
    assert rel_err(got1, want1) < 1e-10 and rel_err(got2, want2) < 1e-10


@pytest.mark.parametrize("kind,omega", SMOOTHERS)
def test_new_kernels_against_flat_per_cycle_128(hip_only, monkeypatch, kind, omega):
    """two V(2,2) cycles with MGCMT_3D_STENCIL_TILE=0 against the default: the same bits after each"""
    g = 128
    op = tensor_op(g, "rough")
    f = np.random.RandomState(23).rand(g ** 3)
    monkeypatch.setenv("MGCMT_3D_STENCIL_TILE", "0")
    flat1, flat2, paths = _two_cycles(op, f, kind, omega)
    assert paths == [(_lib.PATH3D_SEVEN_PLANES, False), (_lib.PATH3D_PLANES, False)]
    monkeypatch.delenv("MGCMT_3D_STENCIL_TILE")
    new1, new2, paths = _two_cycles(op, f, kind, omega)
    assert paths == STENCIL_PATHS
    assert np.all(np.isfinite(new2)) and np.array_equal(new1, flat1) and np.array_equal(new2, flat2)
