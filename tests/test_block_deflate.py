"""mgcmt_block_deflate (csrc/kernels_blockwide.hip: k_block_cross on the matrix cores, k_block_deflate) against NumPy:
W_j <- W_j - sum_i <Q_i, W_j> Q_i for up to 64 vectors Q and up to 16 vectors W.

Tolerances, derived as in tests/test_block_wide.py (u = 2^-53, gamma_m = m u / (1 - m u)).  A coefficient is a sum of n
products: against the np.longdouble product it may differ by gamma_n (|Q_i|^T |W_j|), whatever the summation order.  A new W_j
is W_j minus nq products, accumulated one after the other with fused multiply-adds: against W - Q C evaluated in np.longdouble
from the float64 coefficients C THE DEVICE RETURNED it may differ by gamma_(nq+1) (|W_j| + |Q| |C_j|) at every point.  (The
reference of the update is evaluated in extended precision so that the bound holds for the device alone; float64 NumPy
would spend up to the same amount again.)  Nothing wider is used."""
import ctypes

import numpy as np
import pytest

from multigridcmt_amd import _lib
from multigridcmt_amd.operators import laplacian_operator, potential_operator
from multigridcmt_amd.plan import Plan

V, F, T, W = _lib.SLOT_V, _lib.SLOT_F, _lib.SLOT_T, _lib.SLOT_W
U = 2.0 ** -53


def gamma(n):
    return n * U / (1.0 - n * U)


def _box2d(g):
    return laplacian_operator(g, "2d") * (-1 / np.pi ** 2)


def _pot2d(g):
    t = (np.arange(g) + 0.5) / g
    X, Y = np.meshgrid(t, t, indexing="ij")
    return potential_operator(g, 30.0 * ((X - 0.4) ** 2 + (Y - 0.6) ** 2) + np.random.RandomState(5).rand(g, g))


# (operator, lowest, level), the level shapes of tests/test_block_wide.py::PLANS: 2-D levels of 1024, 64, 16 and 4 points — above,
# at and below one block step of 64 points —, a 3-D level of 512, a 2-D plan with a point diagonal
PLANS = {
    "2d_n1024": (lambda: _box2d(32), 2, 0),
    "2d_n64": (lambda: _box2d(32), 2, 2),
    "2d_n16": (lambda: _box2d(32), 2, 3),
    "2d_n4": (lambda: _box2d(32), 2, 4),
    "3d_n512": (lambda: laplacian_operator(8, "3d") * (-1 / np.pi ** 2), 2, 0),
    "2d_point_n1024": (lambda: _pot2d(32), 2, 0),
}
NVEC = 80
NQ = (1, 15, 16, 17, 33, 64)       # below, at and above each tile boundary of k_block_cross<TQ>
KW = (1, 5, 16)


def _spread(m, first=0):
    """m vectors spread over slots W and F: the even ones in W, the odd ones in F"""
    return [((W if t % 2 == 0 else F), first + t // 2) for t in range(m)]


Q_ALL, W_ALL = _spread(64), _spread(16, first=40)       # Q: columns 0..31 of W and F; W: columns 40..47


def _fill_nan(p, level, vectors):
    nan = np.full(p.size(level), np.nan)
    for v in vectors:
        p.upload(level, v[0], v[1], nan)


def _upload(p, level, vectors, host):
    for v, x in zip(vectors, host.T):
        p.upload(level, v[0], v[1], x)


def _download(p, level, vectors):
    return np.stack([np.array(p.download(level, *v)) for v in vectors], axis=1)


def _check_case(p, level, Qv, Wv, hq, hw, what, repeat=True):
    """one call on uploaded Q and W, checked as the module docstring says, and (repeat) twice more for equal bits"""
    n, nq, k = hq.shape[0], len(Qv), len(Wv)
    _upload(p, level, Qv, hq)
    _upload(p, level, Wv, hw)
    C = p.block_deflate(level, Qv, Wv, want_coeffs=True)
    got = _download(p, level, Wv)
    assert C.shape == (nq, k) and np.all(np.isfinite(C)) and np.all(np.isfinite(got)), what
    ql, wl = hq.astype(np.longdouble), hw.astype(np.longdouble)
    err = np.abs(C.astype(np.longdouble) - ql.T @ wl)
    bound = gamma(n) * (np.abs(hq).T @ np.abs(hw))
    print("%s n=%d coefficients: max err/bound %.3f" % (what, n, float((err / bound).max())))
    assert np.all(err <= bound), (what, float((err / bound).max()))
    err = np.abs(got.astype(np.longdouble) - (wl - ql @ C.astype(np.longdouble)))
    bound = gamma(nq + 1) * (np.abs(hw) + np.abs(hq) @ np.abs(C))
    print("%s n=%d update: max err/bound %.3f" % (what, n, float((err / bound).max())))
    assert np.all(err <= bound), (what, float((err / bound).max()))
    assert np.array_equal(_download(p, level, Qv), hq), what + ": Q changed"
    if not repeat:
        return
    # equal inputs, equal bits — with and without the coefficients coming back
    _upload(p, level, Wv, hw)
    C2 = p.block_deflate(level, Qv, Wv, want_coeffs=True)
    assert np.array_equal(C, C2) and np.array_equal(_download(p, level, Wv), got), what + ": not reproducible"
    _upload(p, level, Wv, hw)
    assert p.block_deflate(level, Qv, Wv) is None
    assert np.array_equal(_download(p, level, Wv), got), what + ": differs without coeffs_out"


@pytest.mark.parametrize("name", list(PLANS))
def test_deflate_against_longdouble(backend, name):
    """nq = 1, 15, 16, 17, 33, 64 crossed with k = 1, 5, 16, the vectors spread over slots W and F.  Before every case every
    vector of slots V, F and W that the case does not name is NaN (a padding lane that read a neighbour, a tile that read
    vector nq, a column j >= k that was loaded or stored shows): coefficients within gamma_n |Q_i|^T |W_j| of the longdouble
    product, the new W within gamma_(nq+1) (|W| + |Q| |C|) of W - Q C, Q bitwise unchanged, a repeated call bit-identical, and
    every vector the call did not name still NaN."""
    rng = np.random.RandomState(13)
    make, lowest, level = PLANS[name]
    p = None
    try:
        p = Plan(make(), lowest, nvec=NVEC)
        n = p.size(level)
        everything = [(s, q) for s in (V, F, W) for q in range(NVEC)]
        _fill_nan(p, level, everything)
        for nq in NQ:
            for k in KW:
                Qv, Wv = Q_ALL[:nq], W_ALL[:k]
                _fill_nan(p, level, Q_ALL + W_ALL)
                _check_case(p, level, Qv, Wv, rng.standard_normal((n, nq)), rng.standard_normal((n, k)), "%s nq=%d k=%d" % (name, nq, k))
                for v in Q_ALL[nq:nq + 2] + W_ALL[k:]:
                    assert np.all(np.isnan(np.array(p.download(level, *v)))), (name, nq, k, v)
        named = set(Q_ALL[:NQ[-1]] + W_ALL[:KW[-1]])
        for v in everything:
            if v not in named:
                assert np.all(np.isnan(np.array(p.download(level, *v)))), (name, v)
    finally:
        if p is not None:
            p.close()


# a block of k_block_cross takes a second trip only from n > 512 * 64 points: 256^2 gives every block exactly two trips (the
# prefetch's first and last), a 1-D level of 2^17 points four (first, middle and last)
TRIPS = {
    "2d_n65536_two_trips": (lambda: _box2d(256), 8),
    "1d_n131072_four_trips": (lambda: laplacian_operator(2 ** 17, "1d") * (-1 / np.pi ** 2), 8),
}


@pytest.mark.parametrize("name", list(TRIPS))
def test_deflate_trip_loop(backend, name):
    """nq = 17 (two tiles, the second nearly empty), k = 5 on levels where a block of pass 1 takes two and four trips; the
    same bounds, one call each (the emulation takes seconds per call at these sizes)"""
    rng = np.random.RandomState(17)
    make, lowest = TRIPS[name]
    p = None
    try:
        p = Plan(make(), lowest, nvec=12)
        n = p.size(0)
        assert (n + 63) // 64 == {"2d_n65536_two_trips": 2, "1d_n131072_four_trips": 4}[name] * 512
        Qv, Wv = _spread(17), _spread(5, first=9)
        _fill_nan(p, 0, [(s, q) for s in (F, W) for q in range(12)])
        _check_case(p, 0, Qv, Wv, rng.standard_normal((n, 17)), rng.standard_normal((n, 5)), name, repeat=False)
        for v in ((F, 8), (F, 11)):                     # (the columns of F next to the last Q and the last W)
            assert v not in Qv + Wv and np.all(np.isnan(np.array(p.download(0, *v))))
    finally:
        if p is not None:
            p.close()


ORTHO_CONSTANT = 3.6e-5


def test_deflated_block_is_orthogonal_to_q(backend):
    """Q with orthonormal columns (np.linalg.qr of a random 1024 x 64 matrix), 16 random W: after the call
    max |Q^T W'| <= ORTHO_CONSTANT gamma_n nq max ||W_j||.  The constant comes from the np.longdouble evaluation of
    W - Q (Q^T W) on the same inputs, which is not zero because the float64 Q is orthonormal to rounding only: its
    max |Q^T W'| is 8.87e-6 of gamma_n nq max ||W_j|| (2.16e-15 absolute); four times that, rounded up, is 3.6e-5
    (the test recomputes the reference's value and asserts that the constant is at least four times it)."""
    rng = np.random.RandomState(23)
    p = None
    try:
        p = Plan(_box2d(32), 2, nvec=NVEC)
        n, nq, k = p.size(0), 64, 16
        hq = np.linalg.qr(rng.standard_normal((n, nq)))[0]
        hw = rng.standard_normal((n, k))
        unit = gamma(n) * nq * np.linalg.norm(hw, axis=0).max()
        ql, wl = hq.astype(np.longdouble), hw.astype(np.longdouble)
        ref = float(np.abs(ql.T @ (wl - ql @ (ql.T @ wl))).max())
        print("longdouble reference: max |Q^T W'| = %.3e = %.3e of gamma_n nq max ||W_j||" % (ref, ref / unit))
        assert 4 * ref / unit <= ORTHO_CONSTANT
        Qv, Wv = Q_ALL[:nq], W_ALL[:k]
        _upload(p, 0, Qv, hq)
        _upload(p, 0, Wv, hw)
        p.block_deflate(0, Qv, Wv)
        got = float(np.abs(ql.T @ _download(p, 0, Wv).astype(np.longdouble)).max())
        print("device: max |Q^T W'| = %.3e = %.3e of gamma_n nq max ||W_j||" % (got, got / unit))
        assert got <= ORTHO_CONSTANT * unit
    finally:
        if p is not None:
            p.close()


def test_deflate_refusals(backend):
    """MGCMT_ERR_INVALID, each with its message: null lists, nq and k out of range, a W named twice, a W that is also a Q,
    vectors the plan does not hold; the export is there"""
    assert "mgcmt_block_deflate" in _lib.EXPORTED_SYMBOLS
    p = None
    try:
        p = Plan(_box2d(16), 4, nvec=NVEC)
        L = _lib.lib()
        assert hasattr(L, "mgcmt_block_deflate")
        one = (ctypes.c_int * 1)(W)
        for args in ((None, one, 1, one, one), (one, None, 1, one, one), (one, one, 1, None, one), (one, one, 1, one, None)):
            assert L.mgcmt_block_deflate(p._h, 0, 1, args[0], args[1], args[2], args[3], args[4], None, None) == -1
            assert b"block_deflate: non-null vector lists" in L.mgcmt_last_error()

        def refused(q, w, message):
            with pytest.raises(_lib.MgcmtError) as e:
                p.block_deflate(0, q, w)
            assert "mgcmt error -1:" in str(e.value) and message in str(e.value), str(e.value)       # MGCMT_ERR_INVALID
        Q65 = [(W, t) for t in range(65)]
        refused(Q65, [(F, 0)], "1..64 vectors Q, 1..16 vectors W")
        refused([], [(F, 0)], "1..64 vectors Q, 1..16 vectors W")
        refused(Q65[:3], [(F, j) for j in range(17)], "1..64 vectors Q, 1..16 vectors W")
        refused(Q65[:3], [], "1..64 vectors Q, 1..16 vectors W")
        refused(Q65[:3], [(F, 0), (F, 1), (F, 0)], "a vector W named twice")
        refused(Q65[:3], [(F, 0), (W, 2)], "a vector W that is also a Q")
        with pytest.raises(_lib.MgcmtError) as e:
            p.block_deflate(0, [(W, 80)], [(F, 0)])                 # vectors the plan does not hold
        assert "mgcmt error -1:" in str(e.value)
        with pytest.raises(_lib.MgcmtError) as e:
            p.block_deflate(0, [(W, 0)], [(F, -1)])
        assert "mgcmt error -1:" in str(e.value)
        with pytest.raises(_lib.MgcmtError) as e:
            p.block_deflate(p.num_levels, [(W, 0)], [(F, 0)])       # a level the plan does not have
        assert "mgcmt error -1:" in str(e.value)
        p.block_deflate(0, Q65[:64], [(F, j) for j in range(16)])   # the limits themselves run
    finally:
        if p is not None:
            p.close()
