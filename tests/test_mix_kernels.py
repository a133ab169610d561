"""mgcmt_mix_residual and mgcmt_mix_combine (csrc/kernels_mix.hip: k_mix_residual, k_mix_final, k_mix_combine) against np.longdouble:
the two per-point operations of Anderson mixing (DESIGN.md par. 4.24).

Tolerances, with u = 2^-53 and gamma_m = m u / (1 - m u) as in tests/test_block_deflate.py.

mix_residual.  r = out - in is one rounded subtraction per point: it must carry the bits of the float64 difference.  The inner
products are sums over the r the kernel wrote.  The n / 2 double2 elements are dealt to S = min(2048, ceil(n / 512)) slices;
the longest path from a term to a result takes: the thread's own chain, two fused multiply-adds per element it owns
(2 ceil(n / 2 / (256 S)) roundings, the products being fused), the 6 steps of the 64-lane shuffle tree and the 4 wave sums of
the slice; then in the one-workgroup second pass ceil(S / 256) additions per thread, the tree (6) and the wave sums (4) — the
count tests/test_vector_algebra.py makes for reduce_blocks, with this kernel's geometry.  Every result must lie within
D u sum |terms| of the np.longdouble sum, D that chain length.

mix_combine.  The arithmetic of a point is acc = 0; for i ascending: acc = fma(alpha_i, fma(beta, r_i, x_i), acc): term i carries
one rounding of the inner fma and takes part in at most p roundings of the accumulation, so the result differs from the exact
value by at most gamma_(p+1) sum |alpha_i| (|x_i| + |beta r_i|); the bound asserted is gamma_(2p+1) of that sum.  With p = 1 and
alpha = [1] the result is fma(beta, r, x) + 0, which is the value lincomb([(1, x), (beta, r)]) = fma(beta, r, 1 * x) gives; the
bits are equal except where that value is -0 (the added +0 turns it into +0), which needs x = -0 and beta r = -0 and does not
occur in the data here."""
import ctypes

import numpy as np
import pytest

from multigridcmt_amd import _lib
from multigridcmt_amd.plan import Plan
from test_block_deflate import F, TRIPS, U, V, W, _box2d, _download, _fill_nan, _upload, gamma
from test_block_density import PLANS

NVEC = 24
PAIRS = (1, 2, 5, 9)
XS = [(W, 2 * t) for t in range(9)]                  # the x of the pairs, oldest first: even columns of W
RS = [(F, 2 * t + 1) for t in range(9)]              # the residuals: odd columns of F
OUT, IN, DST = (V, 3), (W, 19), (F, 20)
MIX_THREADS, MIX_MAX_SLICES = 256, 2048              # kMixThreads, kMixMaxSlices


def mix_slices(n):
    return max(1, min(MIX_MAX_SLICES, -(-(n // 2) // MIX_THREADS)))


def chain_length(n):
    """the roundings on the longest path from a term to a result of mgcmt_mix_residual (module docstring)"""
    s = mix_slices(n)
    return 2 * -(-(n // 2) // (s * MIX_THREADS)) + 6 + 4 + -(-s // MIX_THREADS) + 6 + 4


assert chain_length(1024) == 2 + 10 + 1 + 10 and chain_length(2048 * 2048) == 8 + 10 + 8 + 10


def _values(rng, n, m):
    """mixed signs, magnitudes from 1e-3 to 1e3 per column and per point, exact zeros among them"""
    x = rng.standard_normal((n, m)) * 10.0 ** rng.randint(-3, 4, size=m) * 10.0 ** rng.randint(-1, 2, size=(n, m))
    x[rng.random_sample((n, m)) < 0.1] = 0.0
    return x


def _check_residual(p, level, out, inp, r, prev, ho, hi, hp, what):
    """one call on uploaded vectors, checked as the module docstring says; returns (r, sums)"""
    n, nprev = ho.shape[0], len(prev)
    _upload(p, level, [out, inp] + prev, np.column_stack([ho, hi, hp]))
    sums = p.mix_residual(level, out, inp, r, prev)
    got = np.array(p.download(level, *r))
    assert np.array_equal(got, ho - hi), what + ": r is not the float64 difference"
    rl, D = got.astype(np.longdouble), chain_length(n)
    others = [hp[:, j] for j in range(nprev)] + [got, None]
    worst = 0.0
    for j, y in enumerate(others):
        a, b = (ho, ho) if y is None else (got, y)
        exact = (a.astype(np.longdouble) * b.astype(np.longdouble)).sum()
        mag = float(np.abs(a.astype(np.longdouble) * b.astype(np.longdouble)).sum())
        err = abs(float(np.longdouble(sums[j]) - exact))
        assert err <= D * U * mag, (what, j, err / (U * mag), D)
        worst = max(worst, err / (D * U * mag) if mag else 0.0)
    print("MIXACC %s residual n=%d nprev=%d: worst err / bound %.3f (D = %d)" % (what, n, nprev, worst, D))
    assert rl.shape == (n,) and sums.shape == (nprev + 2,)
    assert np.array_equal(_download(p, level, [out, inp] + prev), np.column_stack([ho, hi, hp])), what + ": an input changed"
    return got, sums


def _check_combine(p, level, xs, rs, alpha, beta, dst, hx, hr, what):
    """one call on uploaded vectors, checked as the module docstring says; returns the result"""
    np_ = len(xs)
    _upload(p, level, xs + rs, np.column_stack([hx, hr]))
    p.mix_combine(level, xs, rs, alpha, beta, dst)
    got = np.array(p.download(level, *dst))
    al, bl = np.asarray(alpha).astype(np.longdouble), np.longdouble(beta)
    ref = (hx.astype(np.longdouble) + bl * hr.astype(np.longdouble)) @ al
    scale = (np.abs(hx) + np.abs(beta * hr)) @ np.abs(np.asarray(alpha))
    assert np.all(np.isfinite(got)), what
    err, bound = np.abs(got.astype(np.longdouble) - ref), gamma(2 * np_ + 1) * scale
    worst = float((err[scale > 0] / bound[scale > 0]).max()) if (scale > 0).any() else 0.0
    print("MIXACC %s combine n=%d p=%d: worst err / bound %.3f" % (what, hx.shape[0], np_, worst))
    assert np.all(err <= bound), (what, worst)
    if dst not in xs:
        assert np.array_equal(_download(p, level, xs + rs), np.column_stack([hx, hr])), what + ": an input changed"
    return got


@pytest.mark.parametrize("name", list(PLANS))
def test_residual_against_longdouble(backend, name):
    """nprev = 0, 1, 4, 8 (p = 1, 2, 5, 9 pairs).  Before every case every vector of V, F and W the case does not name is NaN (an
    earlier residual j >= nprev that was read, a store beside r shows): r bit-equal to out - in, every inner product within the
    chain bound, the inputs unchanged, two more calls bit-identical, every vector the calls did not name still NaN."""
    rng = np.random.RandomState(41)
    make, lowest, level = PLANS[name]
    p = None
    try:
        p = Plan(make(), lowest, nvec=NVEC)
        n = p.size(level)
        everything = [(s, q) for s in (V, F, W) for q in range(NVEC)]
        _fill_nan(p, level, everything)
        for pairs in PAIRS:
            prev = RS[:pairs - 1]
            _fill_nan(p, level, RS + [OUT, IN, DST])
            ho, hi, hp = _values(rng, n, 1)[:, 0], _values(rng, n, 1)[:, 0], _values(rng, n, pairs - 1)
            got, sums = _check_residual(p, level, OUT, IN, DST, prev, ho, hi, hp, name)
            for _ in range(2):
                p.fill(level, DST[0], DST[1], np.nan)
                again = p.mix_residual(level, OUT, IN, DST, prev)
                assert np.array_equal(again, sums) and np.array_equal(np.array(p.download(level, *DST)), got), (name, pairs, "not reproducible")
            for v in RS[pairs - 1:pairs + 1] + [(F, 19), (F, 21), (W, 20)]:
                assert np.all(np.isnan(np.array(p.download(level, *v)))), (name, pairs, v)
        named = set(RS + [OUT, IN, DST])
        for v in everything:
            if v not in named:
                assert np.all(np.isnan(np.array(p.download(level, *v)))), (name, v)
    finally:
        if p is not None:
            p.close()


@pytest.mark.parametrize("name", list(PLANS))
def test_combine_against_longdouble(backend, name):
    """p = 1, 2, 5, 9 pairs, alpha of mixed sign summing to one, beta = 0.3.  Every vector the case does not name is NaN before
    and after; every point within gamma_(2p+1) sum |alpha_i| (|x_i| + |beta r_i|) of the longdouble value; the inputs unchanged;
    two more calls bit-identical; the same bits with the destination in the column of the oldest x; p = 1 with alpha = [1]
    bit-equal to lincomb([(1, x), (beta, r)])."""
    rng = np.random.RandomState(43)
    make, lowest, level = PLANS[name]
    p = None
    try:
        p = Plan(make(), lowest, nvec=NVEC)
        n = p.size(level)
        everything = [(s, q) for s in (V, F, W) for q in range(NVEC)]
        _fill_nan(p, level, everything)
        for pairs in PAIRS:
            xs, rs = XS[:pairs], RS[:pairs]
            _fill_nan(p, level, XS + RS + [DST])
            hx, hr = _values(rng, n, pairs), _values(rng, n, pairs)
            alpha = rng.standard_normal(pairs) * 3.0
            alpha[-1] += 1.0 - alpha.sum()
            if pairs == 1:
                alpha = np.ones(1)
            got = _check_combine(p, level, xs, rs, alpha, 0.3, DST, hx, hr, name)
            for _ in range(2):
                p.fill(level, DST[0], DST[1], np.nan)
                p.mix_combine(level, xs, rs, alpha, 0.3, DST)
                assert np.array_equal(np.array(p.download(level, *DST)), got), (name, pairs, "not reproducible")
            for v in XS[pairs:pairs + 1] + RS[pairs:pairs + 1] + [(F, 19), (F, 21), (W, 20)]:
                assert np.all(np.isnan(np.array(p.download(level, *v)))), (name, pairs, v)
            if pairs == 1:
                p.lincomb(level, [(1.0, xs[0]), (0.3, rs[0])], DST)
                assert np.array_equal(np.array(p.download(level, *DST)), got), name + ": p = 1 is not the damped step of lincomb"
            p.mix_combine(level, xs, rs, alpha, 0.3, xs[0])                      # the oldest x's column as the destination
            assert np.array_equal(np.array(p.download(level, *xs[0])), got), (name, pairs, "in place")
            assert np.array_equal(_download(p, level, xs[1:] + rs), np.column_stack([hx[:, 1:], hr])), (name, pairs, "in place: an input changed")
        named = set(XS + RS + [DST])
        for v in everything:
            if v not in named:
                assert np.all(np.isnan(np.array(p.download(level, *v)))), (name, v)
    finally:
        if p is not None:
            p.close()


# A thread owns two points.  The residual pass deals 256^2 points to 128 slices and 2^17 points to 256, one workgroup per slice by
# default; the combine pass launches one workgroup per 512 points.  MGCMT_MIX_BLOCKS (read when a plan is created) limits both
# grids: with 64 workgroups each takes two slices / two trips at 256^2 points and four at 2^17.
TRIP_BLOCKS = 64


@pytest.mark.parametrize("name", list(TRIPS))
def test_trip_loops_and_grid_independence(backend, name, monkeypatch):
    """five pairs on the levels of tests/test_block_deflate.py::TRIPS with the grid limited to 64 workgroups (two and four trips
    per workgroup): the same bounds; and the same bits — r, every inner product, the combination — from a plan with the default
    grid (one trip), a different nvec and other columns: the results depend neither on the grid nor on where the vectors lie."""
    rng = np.random.RandomState(47)
    make, lowest = TRIPS[name]
    p = q = None
    try:
        monkeypatch.setenv("MGCMT_MIX_BLOCKS", str(TRIP_BLOCKS))
        p = Plan(make(), lowest, nvec=NVEC)
        monkeypatch.delenv("MGCMT_MIX_BLOCKS")
        n = p.size(0)
        trips = {"2d_n65536_two_trips": 2, "1d_n131072_four_trips": 4}[name]
        assert n // (2 * MIX_THREADS * TRIP_BLOCKS) == trips and mix_slices(n) == trips * TRIP_BLOCKS
        _fill_nan(p, 0, [(s, c) for s in (F, W) for c in range(NVEC)])
        ho, hi, hp = _values(rng, n, 1)[:, 0], _values(rng, n, 1)[:, 0], _values(rng, n, 4)
        r, sums = _check_residual(p, 0, OUT, IN, DST, RS[:4], ho, hi, hp, name)
        hx, hr = _values(rng, n, 5), _values(rng, n, 5)
        alpha = np.array([0.7, -1.3, 2.1, -0.9, 0.4])
        got = _check_combine(p, 0, XS[:5], RS[:5], alpha, 0.5, DST, hx, hr, name)
        for v in ((F, 19), (F, 21), (W, 20), (W, 10), (F, 11)):
            assert np.all(np.isnan(np.array(p.download(0, *v)))), v
        q = Plan(make(), lowest, nvec=13)
        prev2 = [(V, 12 - t) for t in range(4)]
        r2, sums2 = _check_residual(q, 0, (F, 0), (F, 12), (W, 1), prev2, ho, hi, hp, name + " default grid")
        assert np.array_equal(r2, r) and np.array_equal(sums2, sums), name + ": the residual pass depends on the grid or on the placement"
        xs2, rs2 = [(V, 12 - t) for t in range(5)], [(F, t) for t in range(5)]
        got2 = _check_combine(q, 0, xs2, rs2, alpha, 0.5, (W, 12), hx, hr, name + " default grid")
        assert np.array_equal(got2, got), name + ": the combine pass depends on the grid or on the placement"
    finally:
        for plan in (p, q):
            if plan is not None:
                plan.close()


def test_refusals(backend):
    """MGCMT_ERR_INVALID, each with its message: null lists, counts out of range, vectors outside the plan, an alpha or beta that is
    not finite, a destination that is also an input (other than the oldest x of mix_combine); the exports are there.  (An odd
    number of points or a vector that is not 16-byte aligned cannot be reached through a plan: every level holds a power of two
    of at least two points and every level vector is 32-byte aligned; the launchers test the bits all the same, as those of the
    wide entries do.)"""
    assert "mgcmt_mix_residual" in _lib.EXPORTED_SYMBOLS and "mgcmt_mix_combine" in _lib.EXPORTED_SYMBOLS and _lib.MIX_MAX == 9
    p = None
    try:
        p = Plan(_box2d(16), 4, nvec=NVEC)
        L = _lib.lib()
        one, wt, res = (ctypes.c_int * 1)(W), (ctypes.c_double * 1)(1.0), (ctypes.c_double * 3)()
        for args in ((None, one, res), (one, None, res), (one, one, None)):
            assert L.mgcmt_mix_residual(p._h, 0, V, 0, V, 1, V, 2, 1, args[0], args[1], args[2], None) == -1
            assert b"mix_residual: non-null vector lists and output" in L.mgcmt_last_error()
        assert L.mgcmt_mix_residual(p._h, 0, V, 0, V, 1, V, 2, 0, None, None, res, None) == 0       # (no earlier residuals: no lists)
        for args in ((None, one, one, one, wt), (one, None, one, one, wt), (one, one, None, one, wt), (one, one, one, None, wt), (one, one, one, one, None)):
            assert L.mgcmt_mix_combine(p._h, 0, 1, args[0], args[1], args[2], args[3], args[4], 1.0, F, 0, None) == -1
            assert b"mix_combine: non-null vector lists and coefficients" in L.mgcmt_last_error()

        def refused(message, call, *args):
            with pytest.raises(_lib.MgcmtError) as e:
                call(*args)
            assert "mgcmt error -1:" in str(e.value) and message in str(e.value), str(e.value)       # MGCMT_ERR_INVALID
        R9 = [(W, t) for t in range(9)]
        refused("0..8 earlier residuals", p.mix_residual, 0, OUT, IN, DST, R9)
        refused("vector index out of range", p.mix_residual, 0, (V, NVEC), IN, DST, [])
        refused("vector index out of range", p.mix_residual, 0, OUT, (W, -1), DST, [])
        refused("vector index out of range", p.mix_residual, 0, OUT, IN, DST, [(W, NVEC)])
        refused("slot out of range", p.mix_residual, 0, OUT, IN, (4, 0), [])
        refused("level out of range", p.mix_residual, p.num_levels, OUT, IN, DST, [])
        for r in (OUT, IN, (W, 1)):
            refused("the destination r is also a vector that is read", p.mix_residual, 0, OUT, IN, r, R9[:3])
        p.fill(0, OUT[0], OUT[1], 1.0)
        p.fill(0, IN[0], IN[1], 0.25)
        for v in R9[:8]:
            p.fill(0, v[0], v[1], 2.0)
        sums = p.mix_residual(0, OUT, IN, DST, R9[:8])                                  # the limit itself runs
        assert np.array_equal(sums, [1.5 * 256] * 8 + [0.5625 * 256, 256.0])
        X10, R10 = [(F, t) for t in range(10)], [(W, t) for t in range(10)]
        refused("1..9 pairs", p.mix_combine, 0, X10, R10, np.ones(10), 1.0, DST)
        refused("1..9 pairs", p.mix_combine, 0, [], [], [], 1.0, DST)
        refused("vector index out of range", p.mix_combine, 0, [(F, NVEC)], R10[:1], [1.0], 1.0, DST)
        refused("vector index out of range", p.mix_combine, 0, X10[:1], [(W, -1)], [1.0], 1.0, DST)
        refused("vector index out of range", p.mix_combine, 0, X10[:1], R10[:1], [1.0], 1.0, (F, NVEC))
        refused("slot out of range", p.mix_combine, 0, X10[:1], R10[:1], [1.0], 1.0, (4, 0))
        refused("level out of range", p.mix_combine, p.num_levels, X10[:1], R10[:1], [1.0], 1.0, DST)
        for bad in (np.nan, np.inf, -np.inf):
            refused("a coefficient that is not finite", p.mix_combine, 0, X10[:3], R10[:3], [1.0, bad, 2.0], 1.0, DST)
            refused("a coefficient that is not finite", p.mix_combine, 0, X10[:3], R10[:3], [1.0, 1.0, 2.0], bad, DST)
        for dst in (X10[1], X10[2], R10[0], R10[2]):
            refused("the destination is also an input other than the oldest x", p.mix_combine, 0, X10[:3], R10[:3], np.ones(3), 1.0, dst)
        with pytest.raises(ValueError):
            p.mix_combine(0, X10[:3], R10[:2], np.ones(3), 1.0, DST)
        with pytest.raises(ValueError):
            p.mix_combine(0, X10[:3], R10[:3], np.ones(2), 1.0, DST)
        for v in X10[:9] + R10[:9]:
            p.fill(0, v[0], v[1], 1.0)
        p.mix_combine(0, X10[:9], R10[:9], np.full(9, 0.5), 1.0, X10[0])                # the limit itself runs, into the oldest x
        assert np.all(np.array(p.download(0, *X10[0])) == 9.0)
    finally:
        if p is not None:
            p.close()
