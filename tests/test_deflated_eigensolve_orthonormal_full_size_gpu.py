"""drivers.deflated_eigensolve(basis="orthonormal"), mgcmt_block_project and mgcmt_block_orthonormalize at sizes only the GPU
runs: 40 states of the 1024^2 box — the case the scaled basis stalls on once 28 states are locked (DESIGN.md par. 4.21) —
and the two entries on a 2048^2 level (2^22 points: 512 blocks of the Gram and cross kernels with 128 trips each, 4096 blocks
of the products with two trips) against float64 NumPy with the bounds of tests/test_block_project.py and
tests/test_block_orthonormalize.py."""
import math

import numpy as np
import pytest

from multigridcmt_amd import _lib, drivers
from multigridcmt_amd.operators import laplacian_operator
from multigridcmt_amd.plan import Plan
from test_block_orthonormalize import graded, t_from_gram
from test_deflated_eigensolve_orthonormal import RESTATED_BOX32_K40

F, W = _lib.SLOT_F, _lib.SLOT_W
U = 2.0 ** -53


def gamma(n):
    return n * U / (1.0 - n * U)


@pytest.mark.gpu
def test_orthonormal_40_states_1024_squared(hip_only):
    """40 states of the 1024^2 box, lowest = 4, basis="orthonormal": converged, ascending, within 1e-8 of
    drivers.exact_box_eigenvalues, vectors orthonormal to 1e-10, the smallest eigenvalue of the scaled Gram matrix >= 0.99 in
    every main-loop Ritz problem, and at most ceil(1.25 x 53) = 67 iterations — the cap the 32^2 box gets for the same 40
    states from the orthonormal restatement (tests/test_deflated_eigensolve_orthonormal.py, RESTATED_BOX32_K40, run by hand
    with the matrix of the oracle's cycle): multigrid counts are mesh-independent.  Measured on the MI355X: 65 iterations."""
    from multigridcmt_amd import plan
    g, k = 1024, 40
    op = laplacian_operator(g, "2d") * (-1 / np.pi ** 2)
    info = {}
    try:
        vals, vecs = drivers.deflated_eigensolve(op, k, lowest=4, info=info, basis="orthonormal")
    finally:
        plan.release_plans()
    want = drivers.exact_box_eigenvalues(g, "2d", k)
    print("status %s, iterations %d, eigenvalue error %.2e, min gram_min %.15f, dropped %d, locked at %s"
          % (info["status"], info["iterations"], np.abs(vals - want[:len(vals)]).max(), info["gram_min"].min(), info["dropped"].sum(), info["locked_at"]))
    assert info["status"] == "converged"
    assert np.all(np.diff(vals) >= 0) and np.abs(vals - want).max() <= 1e-8
    assert np.abs(vecs.T @ vecs - np.eye(k)).max() <= 1e-10
    assert info["gram_min"].min() >= 0.99
    assert info["iterations"] <= math.ceil(1.25 * RESTATED_BOX32_K40)


def _accurate_gram(w):
    """w^T w, the float64 Gram matrices of 4096-point chunks accumulated in np.longdouble"""
    G = np.zeros((w.shape[1], w.shape[1]), dtype=np.longdouble)
    for i in range(0, w.shape[0], 4096):
        G += w[i:i + 4096].T @ w[i:i + 4096]
    return G


@pytest.mark.gpu
def test_project_and_orthonormalize_2048_squared(hip_only):
    """nb = 32, k = 16 with companions on 2^22 points.  The projection: coefficients within gamma_n |B_i|^T |W_j| of NumPy's
    product, the new W and AW within gamma_33 (|W| + |B| |C|) and gamma_33 (|AW| + |AB| |C|) of W - B C and AW - AB C with the
    device's own C, B unchanged.  The orthonormalisation, on 16 vectors of condition number 1e3: T upper triangular with a
    positive diagonal, W T and AW T within gamma_17 |W| |T| with the device's own T, and after a second step max |W^T W - I|
    within 4 x the value of two steps of the restatement with an accurately summed Gram matrix; a repeat bit-identical."""
    rng = np.random.RandomState(53)
    nb, k = 32, 16
    Bv, ABv = [(W, t) for t in range(nb)], [(F, t) for t in range(nb)]
    Wv, AWv = [(W, 32 + t) for t in range(k)], [(F, 32 + t) for t in range(k)]
    p = Plan(laplacian_operator(2048, "2d") * (-1 / np.pi ** 2), 8, nvec=48)

    def upload(vs, h):
        for v, x in zip(vs, h.T):
            p.upload(0, v[0], v[1], x)

    def download(vs):
        return np.stack([np.array(p.download(0, *v)) for v in vs], axis=1)
    try:
        n = p.size(0)
        assert n == 1 << 22
        hb, hab = rng.standard_normal((n, nb)), rng.standard_normal((n, nb))
        hw, haw = rng.standard_normal((n, k)), rng.standard_normal((n, k))
        for vs, h in ((Bv, hb), (ABv, hab), (Wv, hw), (AWv, haw)):
            upload(vs, h)
        C = p.block_project(0, Bv, Wv, ABv, AWv, want_coeffs=True)
        got, gota = download(Wv), download(AWv)
        err, bound = np.abs(C - hb.T @ hw), gamma(n) * (np.abs(hb).T @ np.abs(hw))
        print("coefficients: max err/bound %.4f" % (err / bound).max())
        assert np.all(err <= bound)
        for name, out, inp, basis in (("W", got, hw, hb), ("AW", gota, haw, hab)):
            err, bound = np.abs(out - (inp - basis @ C)), gamma(nb + 1) * (np.abs(inp) + np.abs(basis) @ np.abs(C))
            print("%s: max err/bound %.4f" % (name, (err / bound).max()))
            assert np.all(err <= bound)
        for t in (0, 15, 31):
            assert np.array_equal(np.array(p.download(0, *Bv[t])), hb[:, t]) and np.array_equal(np.array(p.download(0, *ABv[t])), hab[:, t])
        del hb, hab, got, gota

        hw = graded(rng, n, k, 1e3)
        upload(Wv, hw)
        upload(AWv, haw)
        tol = drivers.ORTHONORMAL_DROP_TOL
        Tm, mask = p.block_orthonormalize(0, Wv, AWv, drop_tol=tol, want_t=True, want_dropped=True)
        got, gota = download(Wv), download(AWv)
        assert mask == 0 and np.all(np.isfinite(Tm)) and np.all(np.tril(Tm, -1) == 0.0) and np.all(np.diag(Tm) > 0.0)
        for name, out, inp in (("W T", got, hw), ("AW T", gota, haw)):
            err, bound = np.abs(out - inp @ Tm), gamma(k + 1) * (np.abs(inp) @ np.abs(Tm))
            print("%s: max err/bound %.4f" % (name, (err / bound).max()))
            assert np.all(err <= bound)
        upload(Wv, hw)
        upload(AWv, haw)
        assert p.block_orthonormalize(0, Wv, AWv, drop_tol=tol) is None
        assert np.array_equal(download(Wv[:2]), got[:, :2]) and np.array_equal(download(AWv[14:]), gota[:, 14:])
        assert p.block_orthonormalize(0, Wv, AWv, drop_tol=tol, want_dropped=True) == 0
        w2 = download(Wv)
        e_dev = float(np.abs(_accurate_gram(w2) - np.eye(k)).max())
        ref = hw
        for _ in range(2):                               # (the restatement's T for an accurately summed Gram matrix)
            ref = ref @ _restated_t(ref, tol)
        e_ref = float(np.abs(_accurate_gram(ref) - np.eye(k)).max())
        print("two steps: max |W^T W - I| device %.3e, restatement %.3e" % (e_dev, e_ref))
        assert e_dev <= 4 * e_ref
    finally:
        p.close()


def _restated_t(w, tol):
    """T of the float64 restatement (tests/test_block_orthonormalize.py) for the Gram matrix _accurate_gram(w), rounded once"""
    Tm, mask, _ = t_from_gram(_accurate_gram(w).astype(np.float64), tol)
    assert mask == 0
    return Tm
