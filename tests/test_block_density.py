"""mgcmt_block_density (csrc/kernels_blockwide.hip: k_block_density) against np.longdouble: dst(r) = sum_t w_t x_t(r)^2 for up to
64 vectors.

Tolerance, with u = 2^-53 and gamma_m = m u / (1 - m u) as in tests/test_block_deflate.py.  The kernel's arithmetic at a point
is acc = 0; for t ascending: acc = fma(w_t * x_t, x_t, acc).  Term t carries one rounding in the product w_t x_t and takes part
in at most nq roundings of the accumulation, so the result differs from the exact sum by at most gamma_(nq+1) sum_t |w_t| x_t^2,
and the np.longdouble evaluation of that sum is itself exact to far below u: every point must lie within
gamma_(nq+2) sum_t |w_t| x_t^2 of it.  Nothing wider is used."""
import ctypes

import numpy as np
import pytest

from multigridcmt_amd import _lib
from multigridcmt_amd.operators import laplacian_operator
from multigridcmt_amd.plan import Plan
from test_block_deflate import F, PLANS, TRIPS, V, W, _box2d, _download, _fill_nan, _spread, _upload, gamma

PLANS = dict(PLANS)
del PLANS["3d_n512"]
PLANS["3d_n4096"] = (lambda: laplacian_operator(16, "3d") * (-1 / np.pi ** 2), 4, 0)        # a 16^3 level
NVEC = 80
NQ = (1, 5, 16, 17, 33, 64)        # one vector; the unrolled-by-four loop with a remainder of 1, of 0 after 4 and after 16 rounds; the limit
X_ALL = _spread(64)                # columns 0..31 of W and F
DST = (W, 40)


def _weights(rng, nq):
    """mixed signs and magnitudes from 1e-3 to 1e3, exact zeros among them (none for a single vector)"""
    w = rng.standard_normal(nq) * 10.0 ** rng.randint(-3, 4, size=nq)
    w[2::5] = 0.0
    return w


def _reference(hx, w):
    xl = hx.astype(np.longdouble)
    return (xl * xl) @ w.astype(np.longdouble), (hx * hx) @ np.abs(w)


def _check(p, level, xs, dst, hx, w, what):
    """one call on uploaded vectors, checked as the module docstring says; returns the result"""
    nq = len(xs)
    _upload(p, level, xs, hx)
    p.block_density(level, xs, w, dst)
    got = np.array(p.download(level, *dst))
    ref, scale = _reference(hx, w)
    assert np.all(np.isfinite(got)), what
    err, bound = np.abs(got.astype(np.longdouble) - ref), gamma(nq + 2) * scale
    worst = float((err[scale > 0] / bound[scale > 0]).max()) if (scale > 0).any() else 0.0
    print("%s n=%d nq=%d: max err/bound %.3f" % (what, hx.shape[0], nq, worst))
    assert np.all(err <= bound), (what, worst)
    assert np.array_equal(_download(p, level, xs), hx), what + ": an input changed"
    return got


@pytest.mark.parametrize("name", list(PLANS))
def test_density_against_longdouble(backend, name):
    """nq = 1, 5, 16, 17, 33, 64 with the vectors spread over slots W and F.  Before every case every vector of V, F and W the
    case does not name is NaN (a vector t >= nq that was read, a store beside dst shows): every point within
    gamma_(nq+2) sum |w_t| x_t^2 of the longdouble sum, the inputs bitwise unchanged, two more calls bit-identical, every
    vector the calls did not name still NaN."""
    rng = np.random.RandomState(29)
    make, lowest, level = PLANS[name]
    p = None
    try:
        p = Plan(make(), lowest, nvec=NVEC)
        n = p.size(level)
        everything = [(s, q) for s in (V, F, W) for q in range(NVEC)]
        _fill_nan(p, level, everything)
        for nq in NQ:
            xs = X_ALL[:nq]
            _fill_nan(p, level, X_ALL + [DST])
            hx, w = rng.standard_normal((n, nq)), _weights(rng, nq)
            got = _check(p, level, xs, DST, hx, w, name)
            for _ in range(2):
                p.fill(level, DST[0], DST[1], np.nan)
                p.block_density(level, xs, w, DST)
                assert np.array_equal(np.array(p.download(level, *DST)), got), (name, nq, "not reproducible")
            for v in X_ALL[nq:nq + 2] + [(W, 39), (W, 41), (F, 40)]:
                assert np.all(np.isnan(np.array(p.download(level, *v)))), (name, nq, v)
        named = set(X_ALL + [DST])
        for v in everything:
            if v not in named:
                assert np.all(np.isnan(np.array(p.download(level, *v)))), (name, v)
    finally:
        if p is not None:
            p.close()


# A thread owns two points and a launch has at most 4096 workgroups of 256 threads, so a workgroup takes a second trip through
# its grid-stride loop only beyond 2^21 points.  MGCMT_DENSITY_BLOCKS (read when a plan is created) lowers that limit: with 64
# workgroups a trip covers 2^15 points — 256^2 points are exactly two trips for every workgroup, 2^17 points four.
TRIP_BLOCKS = 64


@pytest.mark.parametrize("name", list(TRIPS))
def test_density_trip_loop_and_grid_independence(backend, name, monkeypatch):
    """nq = 17 on the levels of tests/test_block_deflate.py::TRIPS with the grid limited to 64 workgroups (two and four trips per
    workgroup): the same bound; and the same bits from a plan with the default grid (one trip), a different nvec and other
    columns — the result depends neither on the grid nor on where the vectors lie."""
    rng = np.random.RandomState(31)
    make, lowest = TRIPS[name]
    p = q = None
    try:
        monkeypatch.setenv("MGCMT_DENSITY_BLOCKS", str(TRIP_BLOCKS))
        p = Plan(make(), lowest, nvec=12)
        monkeypatch.delenv("MGCMT_DENSITY_BLOCKS")
        n = p.size(0)
        assert n // (2 * 256 * TRIP_BLOCKS) == {"2d_n65536_two_trips": 2, "1d_n131072_four_trips": 4}[name] and n % (2 * 256 * TRIP_BLOCKS) == 0
        xs, dst = _spread(17), (W, 10)
        _fill_nan(p, 0, [(s, c) for s in (F, W) for c in range(12)])
        hx, w = rng.standard_normal((n, 17)), _weights(rng, 17)
        got = _check(p, 0, xs, dst, hx, w, name)
        for v in ((F, 8), (W, 9), (W, 11), (F, 10)):
            assert v not in xs and np.all(np.isnan(np.array(p.download(0, *v)))), v
        q = Plan(make(), lowest, nvec=19)
        xs2, dst2 = [(F, 18 - t) for t in range(17)], (F, 0)
        _upload(q, 0, xs2, hx)
        q.block_density(0, xs2, w, dst2)
        assert np.array_equal(np.array(q.download(0, *dst2)), got), name + ": depends on the grid or on the placement"
    finally:
        for plan in (p, q):
            if plan is not None:
                plan.close()


def test_density_does_not_depend_on_placement(backend):
    """the same vectors in other slots and columns of a plan with another nvec (another stride between the vectors): equal bits"""
    rng = np.random.RandomState(37)
    p = q = None
    try:
        p, q = Plan(_box2d(32), 2, nvec=NVEC), Plan(_box2d(32), 2, nvec=37)
        n = p.size(0)
        hx, w = rng.standard_normal((n, 33)), _weights(rng, 33)
        got = _check(p, 0, X_ALL[:33], DST, hx, w, "nvec=80")
        xs = [(V, 36 - t) for t in range(33)]
        got2 = _check(q, 0, xs, (F, 5), hx, w, "nvec=37")
        assert np.array_equal(got, got2)
    finally:
        for plan in (p, q):
            if plan is not None:
                plan.close()


def test_density_refusals(backend):
    """MGCMT_ERR_INVALID, each with its message: null lists, nq out of range, a vector outside the plan, dst one of the inputs, a
    weight that is not finite; the export is there.  (The rule of the wide entries — an odd number of points or a vector that is
    not 16-byte aligned — cannot be reached through a plan: every level holds a power of two of at least two points and every
    level vector is 32-byte aligned; the launcher tests the bits all the same, as those of the other wide entries do.)"""
    assert "mgcmt_block_density" in _lib.EXPORTED_SYMBOLS
    p = None
    try:
        p = Plan(_box2d(16), 4, nvec=NVEC)
        L = _lib.lib()
        one, wt = (ctypes.c_int * 1)(W), (ctypes.c_double * 1)(1.0)
        for args in ((None, one, wt), (one, None, wt), (one, one, None)):
            assert L.mgcmt_block_density(p._h, 0, 1, args[0], args[1], args[2], F, 0, None) == -1
            assert b"block_density: non-null vector lists and weights" in L.mgcmt_last_error()

        def refused(plan, level, xs, w, dst, message):
            with pytest.raises(_lib.MgcmtError) as e:
                plan.block_density(level, xs, w, dst)
            assert "mgcmt error -1:" in str(e.value) and message in str(e.value), str(e.value)       # MGCMT_ERR_INVALID
        X65 = [(W, t) for t in range(65)]
        refused(p, 0, X65, np.ones(65), (F, 0), "1..64 vectors X")
        refused(p, 0, [], [], (F, 0), "1..64 vectors X")
        refused(p, 0, [(W, 80)], [1.0], (F, 0), "vector index out of range")
        refused(p, 0, [(W, 0)], [1.0], (F, -1), "vector index out of range")
        refused(p, 0, [(W, 0)], [1.0], (4, 0), "slot out of range")
        refused(p, p.num_levels, [(W, 0)], [1.0], (F, 0), "level out of range")
        refused(p, 0, X65[:3], np.ones(3), (W, 1), "the destination is also an X")
        for bad in (np.nan, np.inf, -np.inf):
            refused(p, 0, X65[:3], [1.0, bad, 2.0], (F, 0), "a weight that is not finite")
        with pytest.raises(ValueError):
            p.block_density(0, X65[:3], [1.0], (F, 0))
        p.block_density(0, X65[:64], np.ones(64), (F, 0))                       # the limit itself runs
        p.fill(0, W, 0, 0.0)
        p.block_density(0, X65[:1], [1.79e308], (F, 0))                         # every finite weight is taken, up to the largest double
        assert np.all(np.array(p.download(0, F, 0)) == 0.0)
    finally:
        if p is not None:
            p.close()
