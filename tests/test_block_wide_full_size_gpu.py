"""The wide block operations at 2048^2 with 48 vectors on the MI355X, against the existing 12 x 4 block kernels.

Four vectors are uploaded; the other 92 (44 of S, 48 of AS) are built on the device with apply and lincomb.  Both forms sum
the same products in different orders, so each is within gamma_n |s_i|^T |as_j| of the exact sum and the two within twice
that (gamma_48 |IN| |C| for the combine).  The absolute-value products are formed on the host from one download."""
import numpy as np
import pytest

from multigridcmt_amd import _lib
from multigridcmt_amd.operators import laplacian_operator
from multigridcmt_amd.plan import Plan

pytestmark = pytest.mark.gpu

V, F, W = _lib.SLOT_V, _lib.SLOT_F, _lib.SLOT_W
G, M = 2048, 48
U = 2.0 ** -53


def gamma(n):
    return n * U / (1.0 - n * U)


@pytest.fixture(scope="module")
def state():
    from conftest import bind_backend
    bind_backend("hip")
    op = laplacian_operator(G, "2d") * (-1 / np.pi ** 2)
    p = Plan(op, 8, nvec=M)
    n = p.size(0)
    rng = np.random.RandomState(4)
    S, AS = [(W, j) for j in range(M)], [(V, j) for j in range(M)]
    for j in range(4):
        p.upload(0, W, j, rng.standard_normal(n))
    scale = 1.0 / (8.0 * G * G / np.pi ** 2)                       # (|A| is about 8 g^2 / pi^2: the vectors stay of order one)
    for j in range(M):
        if j >= 4:
            # s_j = A s_(j-4) / |A| + 0.5 s_(j-3) - 0.25 s_(j-1): AS of column j - 4 exists by now
            p.lincomb(0, [(scale, AS[j - 4]), (0.5, S[j - 3]), (-0.25, S[j - 1])], S[j])
        p.apply(0, S[j], AS[j])
    hs = np.stack([np.array(p.download(0, *v)) for v in S], axis=1)
    has = np.stack([np.array(p.download(0, *v)) for v in AS], axis=1)
    yield p, S, AS, hs, has
    p.close()


def _tiled(p, S, B):
    out = np.zeros((M, M))
    for r in range(0, M, 12):
        for c in range(0, M, 4):
            out[r:r + 12, c:c + 4] = p.block_gram(0, S[r:r + 12], B[c:c + 4])
    return out


def test_pencil_equals_the_tiled_block_gram(state):
    p, S, AS, hs, has = state
    n = p.size(0)
    H, Gm = p.block_pencil(0, S, AS)
    H2, Gm2 = p.block_pencil(0, S, AS)
    assert np.array_equal(H, H2) and np.array_equal(Gm, Gm2)
    Ht, Gt = _tiled(p, S, AS), _tiled(p, S, S)
    bound_h = 2.0 * gamma(n) * (np.abs(hs).T @ np.abs(has))
    bound_g = 2.0 * gamma(n) * (np.abs(hs).T @ np.abs(hs))
    print("pencil: max |wide - tiled| / bound  H %.3g  G %.3g" % ((np.abs(H - Ht) / bound_h).max(), (np.abs(Gm - Gt) / bound_g).max()))
    assert np.all(np.isfinite(H)) and np.all(np.isfinite(Gm))
    assert np.all(np.abs(H - Ht) <= bound_h) and np.all(np.abs(Gm - Gt) <= bound_g)
    # with a third list (MS := AS: nothing in the kernel knows an operator) G is the full square S^T AS
    H3, G3 = p.block_pencil(0, S, AS, AS)
    assert np.array_equal(H3, H) and np.array_equal(G3, H)


def test_combine_equals_the_sliced_block_combine(state):
    p, S, AS, hs, has = state
    rng = np.random.RandomState(9)
    C = rng.standard_normal((M, 16))
    wide, ref, tmp = [(F, j) for j in range(16)], [(F, 16 + j) for j in range(16)], [(F, 32 + j) for j in range(4)]
    p.block_combine_wide(0, S, wide, C)
    for c in range(0, 16, 4):
        p.block_combine(0, S[:12], ref[c:c + 4], C[:12, c:c + 4])
        for r in range(12, M, 12):
            p.block_combine(0, S[r:r + 12], tmp, C[r:r + 12, c:c + 4])
            for j in range(4):
                p.axpy(0, 1.0, tmp[j], ref[c + j])
    bound = 2.0 * gamma(M) * (np.abs(hs) @ np.abs(C))
    worst = 0.0
    for j in range(16):
        a, b = np.array(p.download(0, *wide[j])), np.array(p.download(0, *ref[j]))
        assert np.all(np.isfinite(a))
        worst = max(worst, float((np.abs(a - b) / bound[:, j]).max()))
        assert np.all(np.abs(a - b) <= bound[:, j])
    print("combine: max |wide - sliced| / bound %.3g" % worst)
    for j in (0, 17, 47):                                           # the inputs are left bit for bit
        assert np.array_equal(np.array(p.download(0, *S[j])), hs[:, j])
