"""mgcmt_block_project (csrc/kernels_blockwide.hip: k_block_cross on the matrix cores, k_block_deflate once per pair) against
NumPy: W_j <- W_j - sum_i <B_i, W_j> B_i and AW_j <- AW_j - sum_i <B_i, W_j> AB_i for up to 64 vectors B and up to 16 vectors W.

Tolerances: those of tests/test_block_deflate.py (u = 2^-53, gamma_m = m u / (1 - m u)).  A coefficient may differ from the
np.longdouble product by gamma_n (|B_i|^T |W_j|); a new W_j from W - B C, evaluated in np.longdouble from the float64
coefficients C THE DEVICE RETURNED, by gamma_(nb+1) (|W_j| + |B| |C_j|) at every point; a new AW_j from AW - AB C by the same
bound built from AB and AW.  Nothing wider is used."""
import ctypes

import numpy as np
import pytest

from multigridcmt_amd import _lib
from multigridcmt_amd.plan import Plan
from test_block_deflate import PLANS, TRIPS, _box2d, _download, _fill_nan, _upload, gamma

V, F, T, W = _lib.SLOT_V, _lib.SLOT_F, _lib.SLOT_T, _lib.SLOT_W
NVEC = 80
NB = (1, 16, 17, 32)
KW = (1, 5, 16)
# B: columns 0..31 of W, AB: columns 0..31 of F, W: columns 40..55 of W, AW: columns 40..55 of F
B_ALL, AB_ALL = [(W, t) for t in range(32)], [(F, t) for t in range(32)]
W_ALL, AW_ALL = [(W, 40 + t) for t in range(16)], [(F, 40 + t) for t in range(16)]


def _check_case(p, level, Bv, ABv, Wv, AWv, hb, hab, hw, haw, what, repeat=True):
    """one call on uploaded vectors (ABv = AWv = None: without companions), checked as the module docstring says, and (repeat)
    twice more for equal bits"""
    n, nb, k = hb.shape[0], len(Bv), len(Wv)
    comp = ABv is not None

    def load():
        _upload(p, level, Wv, hw)
        if comp:
            _upload(p, level, AWv, haw)
    _upload(p, level, Bv, hb)
    if comp:
        _upload(p, level, ABv, hab)
    load()
    C = p.block_project(level, Bv, Wv, ABv, AWv, want_coeffs=True)
    got = _download(p, level, Wv)
    assert C.shape == (nb, k) and np.all(np.isfinite(C)) and np.all(np.isfinite(got)), what
    bl, wl, Cl = hb.astype(np.longdouble), hw.astype(np.longdouble), C.astype(np.longdouble)
    err = np.abs(Cl - bl.T @ wl)
    bound = gamma(n) * (np.abs(hb).T @ np.abs(hw))
    print("%s n=%d coefficients: max err/bound %.3f" % (what, n, float((err / bound).max())))
    assert np.all(err <= bound), (what, float((err / bound).max()))
    err = np.abs(got.astype(np.longdouble) - (wl - bl @ Cl))
    bound = gamma(nb + 1) * (np.abs(hw) + np.abs(hb) @ np.abs(C))
    print("%s n=%d W: max err/bound %.3f" % (what, n, float((err / bound).max())))
    assert np.all(err <= bound), (what, float((err / bound).max()))
    assert np.array_equal(_download(p, level, Bv), hb), what + ": B changed"
    gota = None
    if comp:
        gota = _download(p, level, AWv)
        assert np.all(np.isfinite(gota)), what
        err = np.abs(gota.astype(np.longdouble) - (haw.astype(np.longdouble) - hab.astype(np.longdouble) @ Cl))
        bound = gamma(nb + 1) * (np.abs(haw) + np.abs(hab) @ np.abs(C))
        print("%s n=%d AW: max err/bound %.3f" % (what, n, float((err / bound).max())))
        assert np.all(err <= bound), (what, float((err / bound).max()))
        assert np.array_equal(_download(p, level, ABv), hab), what + ": AB changed"
    if not repeat:
        return
    load()
    C2 = p.block_project(level, Bv, Wv, ABv, AWv, want_coeffs=True)
    assert np.array_equal(C, C2) and np.array_equal(_download(p, level, Wv), got), what + ": not reproducible"
    assert not comp or np.array_equal(_download(p, level, AWv), gota), what + ": AW not reproducible"
    load()
    assert p.block_project(level, Bv, Wv, ABv, AWv) is None
    assert np.array_equal(_download(p, level, Wv), got), what + ": differs without coeffs_out"
    assert not comp or np.array_equal(_download(p, level, AWv), gota), what + ": AW differs without coeffs_out"


@pytest.mark.parametrize("name", list(PLANS))
def test_project_against_longdouble(backend, name):
    """nb = 1, 16, 17, 32 crossed with k = 1, 5, 16, with companions and without, on the levels of tests/test_block_deflate.py
    (1024, 64, 16 and 4 points, a 3-D level, a plan with a point diagonal).  Before every case every vector of slots V, F and W
    that the case does not name is NaN: the bounds of the module docstring, B and AB bitwise unchanged, repeated calls
    bit-identical, every vector the call did not name still NaN (without companions: the AB and AW columns too)."""
    rng = np.random.RandomState(29)
    make, lowest, level = PLANS[name]
    p = None
    try:
        p = Plan(make(), lowest, nvec=NVEC)
        n = p.size(level)
        everything = [(s, q) for s in (V, F, W) for q in range(NVEC)]
        _fill_nan(p, level, everything)
        for nb in NB:
            for k in KW:
                for comp in (True, False):
                    Bv, Wv = B_ALL[:nb], W_ALL[:k]
                    ABv, AWv = (AB_ALL[:nb], AW_ALL[:k]) if comp else (None, None)
                    _fill_nan(p, level, B_ALL + AB_ALL + W_ALL + AW_ALL)
                    _check_case(p, level, Bv, ABv, Wv, AWv, rng.standard_normal((n, nb)), rng.standard_normal((n, nb)),
                                rng.standard_normal((n, k)), rng.standard_normal((n, k)), "%s nb=%d k=%d companions=%d" % (name, nb, k, comp))
                    untouched = B_ALL[nb:] + W_ALL[k:] + (AB_ALL[nb:] + AW_ALL[k:] if comp else AB_ALL + AW_ALL)
                    for v in untouched:
                        assert np.all(np.isnan(np.array(p.download(level, *v)))), (name, nb, k, comp, v)
        named = set(B_ALL + AB_ALL + W_ALL + AW_ALL)
        for v in everything:
            if v not in named:
                assert np.all(np.isnan(np.array(p.download(level, *v)))), (name, v)
    finally:
        if p is not None:
            p.close()


@pytest.mark.parametrize("name", list(TRIPS))
def test_project_trip_loop(backend, name):
    """nb = 17 (two tiles, the second nearly empty), k = 5 with companions on levels where a block of pass 1 takes two and four
    trips (256^2, 2^17 points); the same bounds, one call each"""
    rng = np.random.RandomState(31)
    make, lowest = TRIPS[name]
    p = None
    try:
        p = Plan(make(), lowest, nvec=24)
        n = p.size(0)
        assert (n + 63) // 64 == {"2d_n65536_two_trips": 2, "1d_n131072_four_trips": 4}[name] * 512
        Bv, ABv = [(W, t) for t in range(17)], [(F, t) for t in range(17)]
        Wv, AWv = [(W, 18 + t) for t in range(5)], [(F, 18 + t) for t in range(5)]
        _fill_nan(p, 0, [(s, q) for s in (F, W) for q in range(24)])
        _check_case(p, 0, Bv, ABv, Wv, AWv, rng.standard_normal((n, 17)), rng.standard_normal((n, 17)), rng.standard_normal((n, 5)),
                    rng.standard_normal((n, 5)), name, repeat=False)
        for v in ((F, 17), (W, 17), (F, 23), (W, 23)):   # (the columns next to the last B, AB, W and AW)
            assert np.all(np.isnan(np.array(p.download(0, *v))))
    finally:
        if p is not None:
            p.close()


def test_projection_carries_the_operator(backend):
    """B orthonormal, AB = A B and AW = A W on entry (the 32^2 box's operator applied in NumPy): on return AW is A W within
    the two update bounds and the float64 five-point products of the test itself — |AW' - A W'| <= gamma_(nb+1) (|AW| + |AB| |C|)
    + |A| gamma_(nb+1) (|W| + |B| |C|) + gamma_5 |A| (|W'| + |W| + |B| |C|)"""
    rng = np.random.RandomState(37)
    op = _box2d(32)
    A = op.tocsr()
    p = None
    try:
        p = Plan(op, 2, nvec=NVEC)
        n, nb, k = p.size(0), 32, 16
        hb = np.linalg.qr(rng.standard_normal((n, nb)))[0]
        hw = rng.standard_normal((n, k))
        hab, haw = A @ hb, A @ hw
        Bv, ABv, Wv, AWv = B_ALL[:nb], AB_ALL[:nb], W_ALL[:k], AW_ALL[:k]
        for vs, h in ((Bv, hb), (ABv, hab), (Wv, hw), (AWv, haw)):
            _upload(p, 0, vs, h)
        C = p.block_project(0, Bv, Wv, ABv, AWv, want_coeffs=True)
        got, gota = _download(p, 0, Wv), _download(p, 0, AWv)
        absA = abs(A)
        bound = gamma(nb + 1) * (np.abs(haw) + np.abs(hab) @ np.abs(C)) + absA @ (gamma(nb + 1) * (np.abs(hw) + np.abs(hb) @ np.abs(C))) \
            + gamma(5) * (absA @ np.abs(got)) + gamma(5) * (absA @ np.abs(hw) + (absA @ np.abs(hb)) @ np.abs(C))
        err = np.abs(gota - A @ got)
        print("AW' against A W': max err/bound %.3f" % float((err / bound).max()))
        assert np.all(err <= bound)
    finally:
        if p is not None:
            p.close()


def test_project_refusals(backend):
    """MGCMT_ERR_INVALID, each with its message: null lists, nb and k out of range, companions given in part, a W named twice, a
    W that is a B or an AB, an AW named twice, an AW that is a B, an AB or a W, vectors the plan does not hold; the export is
    there and the limits themselves run"""
    assert "mgcmt_block_project" in _lib.EXPORTED_SYMBOLS
    p = None
    try:
        p = Plan(_box2d(16), 4, nvec=NVEC)
        L = _lib.lib()
        assert hasattr(L, "mgcmt_block_project")
        one, two = (ctypes.c_int * 1)(W), (ctypes.c_int * 1)(F)
        for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
            assert L.mgcmt_block_project(p._h, 0, 1, args[0], args[1], None, None, 1, args[2], args[3], None, None, None, None) == -1
            assert b"block_project: non-null vector lists" in L.mgcmt_last_error()
        zero, five = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(5)
        full = [two, zero, two, five]                     # AB = (F, 0), AW = (F, 5) for B = (W, 0), W = (W, 5)
        for missing in range(4):
            part = [None if t == missing else full[t] for t in range(4)]
            assert L.mgcmt_block_project(p._h, 0, 1, one, zero, part[0], part[1], 1, one, five, part[2], part[3], None, None) == -1
            assert b"all four or not at all" in L.mgcmt_last_error()

        def refused(b, w, ab, aw, message):
            with pytest.raises(_lib.MgcmtError) as e:
                p.block_project(0, b, w, ab, aw)
            assert "mgcmt error -1:" in str(e.value) and message in str(e.value), str(e.value)       # MGCMT_ERR_INVALID
        B65 = [(W, t) for t in range(65)]
        AB3 = [(F, t) for t in range(3)]
        refused(B65, [(F, 70)], None, None, "1..64 vectors B, 1..16 vectors W")
        refused([], [(F, 70)], None, None, "1..64 vectors B, 1..16 vectors W")
        refused(B65[:3], [(F, 40 + j) for j in range(17)], None, None, "1..64 vectors B, 1..16 vectors W")
        refused(B65[:3], [], None, None, "1..64 vectors B, 1..16 vectors W")
        refused(B65[:3], [(F, 70), (F, 71), (F, 70)], None, None, "a vector W named twice")
        refused(B65[:3], [(F, 70), (W, 2)], None, None, "a vector W that is also a B or an AB")
        refused(B65[:3], [(W, 70), (F, 1)], AB3, [(F, 70), (F, 71)], "a vector W that is also a B or an AB")
        refused(B65[:3], [(W, 70), (W, 71)], AB3, [(F, 70), (F, 70)], "a vector AW named twice")
        refused(B65[:3], [(W, 70), (W, 71)], AB3, [(F, 70), (W, 1)], "a vector AW that is also a B, an AB or a W")
        refused(B65[:3], [(W, 70), (W, 71)], AB3, [(F, 70), (F, 2)], "a vector AW that is also a B, an AB or a W")
        refused(B65[:3], [(W, 70), (W, 71)], AB3, [(W, 71), (F, 70)], "a vector AW that is also a B, an AB or a W")
        with pytest.raises(ValueError):
            p.block_project(0, B65[:3], [(W, 70)], AB3, None)
        with pytest.raises(_lib.MgcmtError) as e:
            p.block_project(0, [(W, 80)], [(F, 0)])                 # vectors the plan does not hold
        assert "mgcmt error -1:" in str(e.value)
        with pytest.raises(_lib.MgcmtError) as e:
            p.block_project(0, [(W, 0)], [(W, 1)], [(F, 0)], [(F, -1)])
        assert "mgcmt error -1:" in str(e.value)
        with pytest.raises(_lib.MgcmtError) as e:
            p.block_project(p.num_levels, [(W, 0)], [(F, 0)])       # a level the plan does not have
        assert "mgcmt error -1:" in str(e.value)
        # the limits themselves run: 64 vectors B (columns 0..31 of W and F), 16 vectors W with companions
        B64 = [((W, F)[t % 2], t // 2) for t in range(64)]
        AB64 = [((W, F)[t % 2], 32 + t // 2) for t in range(64)]
        p.block_project(0, B64, [(V, j) for j in range(16)], AB64, [(V, 16 + j) for j in range(16)])
    finally:
        if p is not None:
            p.close()
