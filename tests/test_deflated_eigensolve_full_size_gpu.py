"""mgcmt_block_deflate and drivers.deflated_eigensolve at sizes only the GPU runs: the kernel on a 2048^2 level (2^22 points: 512
blocks of pass 1 with 128 trips each, 4096 blocks of pass 2 with two trips) against float64 NumPy with the bounds of
tests/test_block_deflate.py — gamma_n at n = 2^22 is still 4.7e-10 relative to |Q|^T |W| —, and 24 states of the 1024^2 box
against the exact eigenvalues within the iteration cap of the 32^2 box: multigrid counts are mesh-independent."""
import math

import numpy as np
import pytest

from multigridcmt_amd import _lib, drivers
from multigridcmt_amd.operators import laplacian_operator
from multigridcmt_amd.plan import Plan

F, W = _lib.SLOT_F, _lib.SLOT_W
U = 2.0 ** -53

# iterations of the NumPy restatement of tests/test_deflated_eigensolve.py (`restated` with the matrix of the oracle's cycle,
# lowest = 4) on the 32^2 box for the 24 states asked for here, run once by hand: restated(A, 24, lambda R: B @ R) with
# B = _box32_cycle_matrix().  (The same call with 20 states gives the 26 of that file's box32_k20 case.)
RESTATED_BOX32_K24 = 29


def gamma(n):
    return n * U / (1.0 - n * U)


@pytest.mark.gpu
def test_deflate_2048_squared(hip_only):
    """nq = 64, k = 16 on 2^22 points, vectors spread over slots W and F: coefficients within gamma_n |Q_i|^T |W_j| of NumPy's
    product, the new W within gamma_65 (|W| + |Q| |C|) of W - Q C with the device's own C at every point, Q unchanged, a second
    call on the same inputs bit-identical"""
    rng = np.random.RandomState(31)
    nq, k = 64, 16
    Qv = [((W if t % 2 == 0 else F), t // 2) for t in range(nq)]
    Wv = [((W if t % 2 == 0 else F), 32 + t // 2) for t in range(k)]
    p = Plan(laplacian_operator(2048, "2d") * (-1 / np.pi ** 2), 8, nvec=40)
    try:
        n = p.size(0)
        assert n == 1 << 22
        hq, hw = rng.standard_normal((n, nq)), rng.standard_normal((n, k))
        for v, x in zip(Qv + Wv, np.hstack([hq, hw]).T):
            p.upload(0, v[0], v[1], x)
        C = p.block_deflate(0, Qv, Wv, want_coeffs=True)
        got = np.stack([np.array(p.download(0, *v)) for v in Wv], axis=1)
        err, bound = np.abs(C - hq.T @ hw), gamma(n) * (np.abs(hq).T @ np.abs(hw))
        print("coefficients: max err/bound %.4f" % (err / bound).max())
        assert np.all(err <= bound)
        err, bound = np.abs(got - (hw - hq @ C)), gamma(nq + 1) * (np.abs(hw) + np.abs(hq) @ np.abs(C))
        print("update: max err/bound %.4f" % (err / bound).max())
        assert np.all(err <= bound)
        for t in (0, 31, 63):
            assert np.array_equal(np.array(p.download(0, *Qv[t])), hq[:, t])
        for v, x in zip(Wv, hw.T):
            p.upload(0, v[0], v[1], x)
        C2 = p.block_deflate(0, Qv, Wv, want_coeffs=True)
        assert np.array_equal(C, C2)
        for j in (0, 15):
            assert np.array_equal(np.array(p.download(0, *Wv[j])), got[:, j])
    finally:
        p.close()


@pytest.mark.gpu
def test_deflated_eigensolve_1024_squared(hip_only):
    """24 states of the 1024^2 box, lowest = 4: converged, within 1e-8 of drivers.exact_box_eigenvalues, ascending, and in at
    most ceil(1.25 x 29) = 37 iterations — the cap the 32^2 box gets for the same 24 states: the restatement's count there
    plus a quarter.  Measured on the MI355X: 34 iterations (the 20 states of the 32^2 box take 26 there, the restatement 26
    for 20 states and 29 for 24)."""
    from multigridcmt_amd import plan
    g, k = 1024, 24
    op = laplacian_operator(g, "2d") * (-1 / np.pi ** 2)
    info = {}
    try:
        vals, vecs = drivers.deflated_eigensolve(op, k, lowest=4, info=info)
    finally:
        plan.release_plans()
    want = drivers.exact_box_eigenvalues(g, "2d", k)
    print("iterations %d, eigenvalue error %.2e, locked at %s" % (info["iterations"], np.abs(vals - want).max(), info["locked_at"]))
    assert info["status"] == "converged"
    assert np.all(np.diff(vals) >= 0) and np.abs(vals - want).max() <= 1e-8
    assert np.abs(vecs.T @ vecs - np.eye(k)).max() <= 1e-10
    assert info["iterations"] <= math.ceil(1.25 * RESTATED_BOX32_K24)
