"""3-D path, host side: the stencil maker's 3-D matrices, the matrix-free operator, recognition of 3-D operators, and a
3-D plan's Galerkin factors against R A P assembled by scipy (through the emulation build of the kernel sources)."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import bind_backend, load_golden, rel_err
from multigridcmt_amd import MGCMTStencilMaker, _lib
from multigridcmt_amd.operators import StructuredOperator, UnrecognisedOperator, laplacian_operator, recognise
from multigridcmt_amd.plan import Plan


def _kron3(a, b, c):
    return np.kron(a, np.kron(b, c))


def test_laplacian_3d_is_kronsum_of_golden_1d():
    L = load_golden("operators")["L1d_8"]
    I = np.eye(8)
    want = _kron3(I, I, L) + _kron3(I, L, I) + _kron3(L, I, I)
    got = MGCMTStencilMaker().laplacian(8, dimension="3d").toarray()
    assert got.shape == (512, 512)
    assert np.array_equal(got, want)


def test_interpolation_and_restriction_3d_are_krons_of_golden_1d():
    gold = load_golden("operators")
    sm = MGCMTStencilMaker()
    P1, R1 = gold["P_8_16"], gold["R_16_8"]
    P = sm.interpolation(8, 16, dimension="3d").toarray()
    R = sm.restriction(16, 8, dimension="3d").toarray()
    assert np.array_equal(P, _kron3(P1, P1, P1))
    assert np.array_equal(R, _kron3(R1, R1, R1))          # one-level jump: (1/8) P^T = R1 (x) R1 (x) R1
    assert np.array_equal(R, 0.125 * P.T)
    # multi-level jump: the fixed 1/8 of the 2-D formula's fixed 1/4 (not raised to the level difference)
    P4 = gold["P_4_16"]
    assert np.array_equal(sm.restriction(16, 4, dimension="3d").toarray(), 0.125 * _kron3(P4, P4, P4).T)


def test_matrix_free_laplacian_3d():
    sm = MGCMTStencilMaker()
    op = sm.laplacian(8, dimension="3d", matrix_free=True)
    assert isinstance(op, StructuredOperator) and op.dimension == "3d" and op.shape == (512, 512)
    A = sm.laplacian(8, dimension="3d")
    assert abs(op.tocsr() - A).max() == 0.0
    assert np.array_equal(op.diagonal(), A.diagonal())
    B = (-2.5 * op).shifted(1.25)
    assert abs(B.tocsr() - (-2.5 * A - 1.25 * sp.eye(512))).max() < 1e-9


@pytest.mark.parametrize("scale,shift", [(1.0, 0.0), (-1 / np.pi ** 2, 0.0), (-1 / np.pi ** 2, 1.9), (3.0, -7.5)])
def test_recognise_scaled_shifted_3d(scale, shift):
    A = (scale * MGCMTStencilMaker().laplacian(16, dimension="3d") - shift * sp.eye(16 ** 3)).tocsr()
    for dim in ("3d", None):
        op = recognise(A, dim)
        assert op.dimension == "3d" and op.g == 16
        assert abs(op.tocsr() - A).max() <= 1e-12 * abs(A).max()


def test_recognise_separable_diagonal_3d():
    g = 8
    L = MGCMTStencilMaker().laplacian(g, dimension="3d")
    rng = np.random.RandomState(3)
    a, b, c = rng.rand(g), rng.rand(g), rng.rand(g)
    d = (a[:, None, None] + b[None, :, None] + c[None, None, :]).reshape(-1)
    A = (L + sp.diags(d)).tocsr()
    op = recognise(A, "3d")
    assert abs(op.tocsr() - A).max() <= 1e-12 * abs(A).max()


def test_recognise_rejects_non_separable_3d():
    g = 8
    L = MGCMTStencilMaker().laplacian(g, dimension="3d")
    d = np.random.RandomState(4).rand(g ** 3)          # a diagonal that is not a(z) + b(y) + c(x)
    with pytest.raises(UnrecognisedOperator):
        recognise((L + sp.diags(d)).tocsr(), "3d")
    M = L.tolil()
    M[5, 6] = 3.0                                     # one x-coupling that differs from the rest of its diagonal
    with pytest.raises(UnrecognisedOperator):
        recognise(M.tocsr(), "3d")


def test_recognise_2d_unchanged_for_square_cube_sizes():
    # 4096 = 64^2 = 16^3: a 2-D operator stays 2-D when no dimension is named
    A = MGCMTStencilMaker().laplacian(64, dimension="2d")
    assert recognise(A).dimension == "2d"


@pytest.mark.parametrize("g", [16, 32])
def test_plan_galerkin_factors_3d(g):
    bind_backend("emu")
    sm = MGCMTStencilMaker()
    A = (-1 / np.pi ** 2) * sm.laplacian(g, dimension="3d")
    op = recognise(A, "3d")
    plan = Plan(op, 4, nvec=1)
    try:
        assert plan.num_levels == int(np.log2(g // 4)) + 1
        Al = sp.csr_matrix(A)
        for level in range(1, plan.num_levels):
            n = g >> level
            R = sm.restriction(2 * n, n, dimension="3d")
            P = sm.interpolation(n, 2 * n, dimension="3d")
            Al = (R @ Al @ P).tocsr()
            fs = [plan.factors(level, w) for w in range(3)]
            assert all(f.shape == (3, 3, n) for f in fs)
            got = StructuredOperator("3d", n, [tuple(f[m] for f in fs) for m in range(3)]).tocsr()
            assert abs(got - Al).max() <= 1e-12 * abs(Al).max()
            assert plan.level_shape(level) == (n, n * n, 0)
    finally:
        plan.close()


def test_plan_create3d_rejects_large_lowest_level():
    bind_backend("emu")
    with pytest.raises(ValueError):
        Plan(laplacian_operator(32, "3d"), 32)
    assert _lib.ABI_VERSION == 7
