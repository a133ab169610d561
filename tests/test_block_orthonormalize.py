"""mgcmt_block_orthonormalize (csrc/kernels_blockwide.hip: k_block_gram16 on the matrix cores, k_orth_factor, k_block_transform):
one Cholesky-QR step W <- W T, AW <- AW T on up to 16 vectors, against a np.longdouble restatement of the same step — the
Gram matrix symmetrised and scaled to a unit diagonal, the unpivoted right-looking Cholesky factorisation with the drop rule,
T = D R^-1.

Inputs: W = U diag(1, ..., 1/kappa) V^T with random orthonormal U (n x k) and V (k x k), the singular values graded
geometrically, kappa = 1, 1e3, 1e6 (a level with fewer points than vectors takes min(n, k) vectors); AW = A W with the level's
operator, applied in NumPy.

Bounds (u = 2^-53, gamma_m = m u / (1 - m u)).
* The product.  An output is a product followed by at most k - 1 fused multiply-adds: against W_in T evaluated in np.longdouble
  from the float64 T THE DEVICE RETURNED it may differ by gamma_(k+1) (|W_in| |T|) at every point; AW likewise.
* T.  The restatement is run twice on the same float64 input, in np.longdouble and in float64; e_oracle is the distance
  between the two, max |T_ld - T_64| over max |T_ld|: what the conditioning of the step (cond(W)^2) makes of one unit roundoff
  per operation.  The device's T is within max(4 e_oracle, 8 eps) of T_ld in the same measure (the rule of DESIGN.md par. 4.7).
  The float64 run restates the kernels' step operation by operation, the order of the Gram sum included (the fixed
  point -> (block, wave, lane, trip) map of k_block_gram16).  That order is the float64 run's one degree of freedom, and with
  cond(W)^2 in front it matters: on these inputs BLAS, 64-point chunks and the point-by-point order give T errors up to ten
  times apart, all of them float64 runs of the same step — four times ONE of them is no bar for another.  What the bar then
  catches is a step that is not this step: a missing symmetrisation or scaling, another pivot order, a wrong triangle.
* Two steps.  max |W^T W - I| after two device steps (evaluated in np.longdouble) is within 4 x the value that two steps of the
  LONGDOUBLE-ACCUMULATED restatement reach on the same input: the float64 restatement whose one long sum — the Gram matrix,
  n products per entry — is accumulated in np.longdouble and rounded once (restated_step, accumulated=True); the
  factorisation, T and the products W T are float64 operations, as on the device.  (A restatement that also keeps T and the
  products in np.longdouble is no yardstick for a float64 kernel: with k = 1 its second step leaves | ||w||^2 - 1 | at
  u / sqrt(n), 4e-18 at 1024 points, from the independent roundings of the n entries, where any float64 T = 1 / ||w|| carries a
  relative error of up to u into every entry alike, 2 u into the norm.)  No floor is added.  AW_out against A W_out: the companions took the transformations of W, so
  AW_out - A W_out = (AW_in - A W_in) T1 T2 up to the product bounds; asserted as |AW_out - A W_out| <= 4 x the same quantity
  of the restatement + the float64 product A W_out of the test itself, gamma_(nnz+1) |A| |W_out|.
No family member may lose a column: DROP_TOL = drivers.ORTHONORMAL_DROP_TOL, the largest power of ten for which that holds
with the two-step bound met (DESIGN.md par. 4.22 has the pivots)."""
import ctypes

import numpy as np
import pytest

from multigridcmt_amd import _lib, drivers
from multigridcmt_amd.plan import Plan
from test_block_deflate import PLANS, TRIPS, _box2d, _download, _fill_nan, _upload, gamma

V, F, T, W = _lib.SLOT_V, _lib.SLOT_F, _lib.SLOT_T, _lib.SLOT_W
NVEC = 40
KW = (1, 5, 16)
KAPPAS = (1.0, 1e3, 1e6)
DROP_TOL = drivers.ORTHONORMAL_DROP_TOL
EPS = 2.0 ** -52
W_ALL, AW_ALL = [(W, 3 + t) for t in range(16)], [(F, 5 + t) for t in range(16)]


def _factor(S, alive, drop_tol):
    """the unpivoted right-looking Cholesky factorisation with the drop rule, in place in S's own arithmetic; the pivots taken"""
    k = S.shape[0]
    pivots = []
    for t in range(k):
        if not alive[t]:
            continue
        if not S[t, t] > drop_tol:
            alive[t] = False
            S[t, :] = S[:, t] = 0
            continue
        pivots.append(float(S[t, t]))
        S[t, t:] = S[t, t:] / np.sqrt(S[t, t])
        for i in range(t + 1, k):
            S[i, i:] = S[i, i:] - S[t, i] * S[t, i:]
    return pivots


def _invert(S, alive):
    """R^-1 over the columns that stayed, by back substitution in S's own arithmetic"""
    k = S.shape[0]
    C = np.zeros((k, k), dtype=S.dtype)
    for j in range(k):
        if not alive[j]:
            continue
        C[j, j] = 1 / S[j, j]
        for i in range(j - 1, -1, -1):
            if alive[i]:
                acc = S.dtype.type(0)
                for t in range(i + 1, j + 1):            # (the kernel's order: one product after the other)
                    acc = acc + S[i, t] * C[t, j]
                C[i, j] = -acc / S[i, i]
    return C


def _gram_in_kernel_order(Wm):
    """W^T W in float64 with the kernel's fixed point -> (block, wave, lane, trip) map: step s of 64 points belongs to block
    s mod nb (nb = min(steps, 512)); in a step wave w holds points 16 w .. 16 w + 15 and adds them to its tile in the order
    q = 0..3, lane group 0..3 (point 16 w + 4 group + q) with fused multiply-adds (here: the product and the sum in
    np.longdouble, rounded once); waves are summed 0..3, blocks 0..nb-1."""
    n, k = Wm.shape
    steps = (n + 63) // 64
    nb = max(1, min(steps, 512))
    Wl = Wm.astype(np.longdouble)
    order = [16 * w + 4 * g + q for w in range(4) for q in range(4) for g in range(4)]
    acc = np.zeros((nb, 4, k, k))                         # (all blocks at once: they do not meet before the last sum)
    for trip in range((steps + nb - 1) // nb):
        for t, o in enumerate(order):
            p = 64 * (np.arange(nb) + nb * trip) + o
            b = np.flatnonzero(p < n)
            x = Wl[p[b]]
            acc[b, t // 16] = (x[:, :, None] * x[:, None, :] + acc[b, t // 16]).astype(np.float64)
    total = np.zeros((k, k))
    for b in range(nb):
        total = total + (((acc[b, 0] + acc[b, 1]) + acc[b, 2]) + acc[b, 3])
    return total


def restated_step(Wm, AWm, drop_tol, dtype, accumulated=False):
    """The step on float64 input, every operation in `dtype` arithmetic (np.float64 or np.longdouble): (W T, AW T, T, mask,
    smallest pivot).  The Gram matrix of the float64 run is summed in the kernel's order or, accumulated=True, is the
    np.longdouble sum rounded once."""
    Wd = Wm.astype(dtype)
    if dtype is np.float64 and accumulated:
        G = (Wm.astype(np.longdouble).T @ Wm.astype(np.longdouble)).astype(np.float64)
    elif dtype is np.float64:
        G = _gram_in_kernel_order(Wm)
    else:
        G = Wd.T @ Wd
    Tm, mask, piv = t_from_gram(G, drop_tol)
    return Wd @ Tm, (None if AWm is None else AWm.astype(dtype) @ Tm), Tm, mask, piv


def t_from_gram(G, drop_tol):
    """(T, mask, smallest pivot) of the step for the Gram matrix G, in G's own arithmetic"""
    dtype = G.dtype.type
    k = G.shape[0]
    G = (G + G.T) / dtype(2)
    g = np.diag(G).astype(np.float64)
    alive = (g > 0.0) & np.isfinite(g)
    d = np.zeros(k, dtype=dtype)
    d[alive] = dtype(1) / np.sqrt(np.diag(G)[alive])
    S = (G * d[:, None]) * d[None, :]
    S[np.diag_indices(k)] = alive.astype(dtype)
    pivots = _factor(S, alive, drop_tol)
    Tm = d[:, None] * _invert(S, alive)
    mask = sum(1 << j for j in range(k) if not alive[j])
    return Tm, mask, (min(pivots) if pivots else None)


def graded(rng, n, k, kappa):
    """U diag(1 .. 1/kappa) V^T: k columns of condition number kappa"""
    U = np.linalg.qr(rng.standard_normal((n, k)))[0]
    Vt = np.linalg.qr(rng.standard_normal((k, k)))[0].T
    s = np.logspace(0.0, -np.log10(kappa), k) if k > 1 else np.ones(1)
    return (U * s) @ Vt


def _level_matrix(p, level):
    """the level's operator as NumPy sees it: column j is the device's A e_j (exact in float64 for the stencils used here up
    to the rounding of each entry — the reference only needs SOME fixed linear map that the companions can be checked against,
    and the checks below account for its float64 products)"""
    n = p.size(level)
    A = np.zeros((n, n))
    for j in range(n):
        e = np.zeros(n)
        e[j] = 1.0
        p.upload(level, V, 0, e)
        p.apply(level, (V, 0), (V, 1))
        A[:, j] = np.array(p.download(level, V, 1))
    return A


def _run_step(p, level, Wv, AWv, hw, haw, want=True):
    _upload(p, level, Wv, hw)
    if AWv is not None:
        _upload(p, level, AWv, haw)
    out = p.block_orthonormalize(level, Wv, AWv, drop_tol=DROP_TOL, want_t=want, want_dropped=want)
    return out, _download(p, level, Wv), (None if AWv is None else _download(p, level, AWv))


def _check_one_step(p, level, Wv, AWv, hw, haw, what):
    """one step: T upper triangular with a positive diagonal and near the longdouble restatement's, the products within their
    bounds, repeats bit-identical with and without outputs.  Returns (W_out, AW_out, T)."""
    k = len(Wv)
    (Tm, mask), got, gota = _run_step(p, level, Wv, AWv, hw, haw)
    assert mask == 0, (what, mask)
    assert Tm.shape == (k, k) and np.all(np.isfinite(Tm)) and np.all(np.tril(Tm, -1) == 0.0) and np.all(np.diag(Tm) > 0.0), what
    _, _, T_ld, mask_ld, piv = restated_step(hw, haw, DROP_TOL, np.longdouble)
    _, _, T_64, _, _ = restated_step(hw, haw, DROP_TOL, np.float64)
    assert mask_ld == 0
    scale = float(np.abs(T_ld).max())
    e_oracle = float(np.abs(T_ld - T_64.astype(np.longdouble)).max()) / scale
    e_device = float(np.abs(T_ld - Tm.astype(np.longdouble)).max()) / scale
    print("%s: smallest pivot %.3e, T error %.3e (restatement in float64: %.3e)" % (what, piv, e_device, e_oracle))
    assert e_device <= max(4 * e_oracle, 8 * EPS), (what, e_device, e_oracle)
    Tl = Tm.astype(np.longdouble)
    for name, out, inp in (("W", got, hw), ("AW", gota, haw)):
        if out is None:
            continue
        err = np.abs(out.astype(np.longdouble) - inp.astype(np.longdouble) @ Tl)
        bound = gamma(k + 1) * (np.abs(inp) @ np.abs(Tm))
        ok = err <= bound
        print("%s %s: max err/bound %.3f" % (what, name, float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0))
        assert np.all(ok), (what, name)
    (T2, mask2), got2, gota2 = _run_step(p, level, Wv, AWv, hw, haw)
    assert mask2 == 0 and np.array_equal(Tm, T2) and np.array_equal(got, got2), what + ": not reproducible"
    assert gota is None or np.array_equal(gota, gota2), what + ": AW not reproducible"
    none, got3, gota3 = _run_step(p, level, Wv, AWv, hw, haw, want=False)
    assert none is None and np.array_equal(got, got3) and (gota is None or np.array_equal(gota, gota3)), what + ": differs without outputs"
    return got, gota, Tm


def _restated_two_steps(hw, haw):
    """two steps of the longdouble-accumulated restatement (restated_step, accumulated=True)"""
    w, aw = hw, haw
    for _ in range(2):
        wl, awl, _, mask, _ = restated_step(w, aw, DROP_TOL, np.float64, accumulated=True)
        assert mask == 0
        w, aw = wl.astype(np.float64), (None if awl is None else awl.astype(np.float64))
    return w, aw


def _orth_error(w):
    wl = w.astype(np.longdouble)
    return float(np.abs(wl.T @ wl - np.eye(w.shape[1])).max())


@pytest.mark.parametrize("name", list(PLANS))
def test_orthonormalize_against_longdouble(backend, name):
    """k = 1, 5, 16 crossed with kappa = 1, 1e3, 1e6 on the levels of tests/test_block_deflate.py, with companions AW = A W
    (and, for k = 5, without): the checks of one step, then a second step: max |W^T W - I| within 4 x the restatement's, AW_out
    against A W_out.  Before every case every vector of slots V, F and W that the case does not name is NaN, and still is
    afterwards."""
    rng = np.random.RandomState(41)
    make, lowest, level = PLANS[name]
    p = None
    try:
        p = Plan(make(), lowest, nvec=NVEC)
        n = p.size(level)
        A = _level_matrix(p, level)
        absA, nnz = np.abs(A), int((A != 0).sum(axis=1).max())
        everything = [(s, q) for s in (V, F, W) for q in range(NVEC)]
        _fill_nan(p, level, everything)
        for k in KW:
            kk = min(k, n)
            for kappa in KAPPAS:
                for comp in ((True, False) if k == 5 else (True,)):
                    what = "%s k=%d kappa=%g companions=%d" % (name, kk, kappa, comp)
                    Wv, AWv = W_ALL[:kk], (AW_ALL[:kk] if comp else None)
                    _fill_nan(p, level, W_ALL + AW_ALL)
                    hw = graded(rng, n, kk, kappa)
                    haw = A @ hw if comp else None
                    w1, aw1, _ = _check_one_step(p, level, Wv, AWv, hw, haw, what)
                    # the second step, on what the first left in place
                    out = p.block_orthonormalize(level, Wv, AWv, drop_tol=DROP_TOL, want_dropped=True)
                    assert out == 0, what
                    w2 = _download(p, level, Wv)
                    ref_w, ref_aw = _restated_two_steps(hw, haw)
                    e_dev, e_ref = _orth_error(w2), _orth_error(ref_w)
                    print("%s two steps: max |W^T W - I| device %.3e, restatement %.3e" % (what, e_dev, e_ref))
                    assert e_dev <= 4 * e_ref, (what, e_dev, e_ref)
                    if comp:
                        aw2 = _download(p, level, AWv)
                        a_dev = np.abs(aw2 - A @ w2)
                        a_ref = np.abs(ref_aw - A @ ref_w)
                        slack = gamma(nnz + 1) * (absA @ (np.abs(w2) + np.abs(ref_w)))
                        print("%s two steps: max |AW - A W| device %.3e, restatement %.3e" % (what, a_dev.max(), a_ref.max()))
                        assert a_dev.max() <= 4 * a_ref.max() + slack.max(), (what, a_dev.max(), a_ref.max())
                    for v in W_ALL[kk:] + (AW_ALL[kk:] if comp else AW_ALL):
                        assert np.all(np.isnan(np.array(p.download(level, *v)))), (what, v)
        named = set(W_ALL + AW_ALL)
        for v in everything:
            if v not in named:
                assert np.all(np.isnan(np.array(p.download(level, *v)))), (name, v)
    finally:
        if p is not None:
            p.close()


def test_rank_deficient_columns_are_dropped(backend):
    """8 vectors on 1024 points, kappa = 10 otherwise: column 2 zero; column 5 equal to column 1; column 6 = column 3 + delta r
    with r a unit vector orthogonal to all others and delta = 1e-8, so that its pivot is delta^2 / (1 + delta^2) = 1e-16 < DROP_TOL
    by construction.  Exactly those come back as exact zeros in W and AW, the mask names them, T has zero rows and columns
    there, and after a second step the others are orthonormal within 4 x the restatement's value."""
    rng = np.random.RandomState(43)
    op = _box2d(32)
    A = op.tocsr()
    p = None
    try:
        p = Plan(op, 2, nvec=NVEC)
        n, k = p.size(0), 8
        Qr = np.linalg.qr(rng.standard_normal((n, k + 1)))[0]
        hw = graded(rng, k, k, 10.0)
        hw = Qr[:, :k] @ hw
        hw[:, 2] = 0.0
        hw[:, 5] = hw[:, 1]
        hw[:, 6] = hw[:, 3] / np.linalg.norm(hw[:, 3]) + 1e-8 * Qr[:, k]
        haw = A @ hw
        gone, stay = [2, 5, 6], [0, 1, 3, 4, 7]
        assert DROP_TOL > 1e-15
        Wv, AWv = W_ALL[:k], AW_ALL[:k]
        _fill_nan(p, 0, [(s, q) for s in (V, F, W) for q in range(NVEC)])
        (Tm, mask), got, gota = _run_step(p, 0, Wv, AWv, hw, haw)
        _, _, T_ld, mask_ld, _ = restated_step(hw, haw, DROP_TOL, np.longdouble)
        assert mask == mask_ld == sum(1 << j for j in gone), (mask, mask_ld)
        for j in gone:
            assert np.all(got[:, j] == 0.0) and np.all(gota[:, j] == 0.0) and np.all(Tm[j] == 0.0) and np.all(Tm[:, j] == 0.0), j
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(gota)) and np.all(np.diag(Tm)[stay] > 0.0)
        err = np.abs(got.astype(np.longdouble) - hw.astype(np.longdouble) @ Tm.astype(np.longdouble))
        assert np.all(err <= gamma(k + 1) * (np.abs(hw) @ np.abs(Tm)))
        mask2 = p.block_orthonormalize(0, Wv, AWv, drop_tol=DROP_TOL, want_dropped=True)
        assert mask2 == mask
        w2, aw2 = _download(p, 0, Wv), _download(p, 0, AWv)
        for j in gone:
            assert np.all(w2[:, j] == 0.0) and np.all(aw2[:, j] == 0.0), j
        ref = hw
        for _ in range(2):
            ref = restated_step(ref, None, DROP_TOL, np.float64, accumulated=True)[0]
        e_dev, e_ref = _orth_error(w2[:, stay]), _orth_error(ref[:, stay])
        print("rank-deficient, two steps: max |W^T W - I| device %.3e, restatement %.3e" % (e_dev, e_ref))
        assert e_dev <= 4 * e_ref
        # a column that is not finite is dropped too, and nothing of it reaches the others
        hw[0, 4] = np.inf
        (Tm, mask), got, gota = _run_step(p, 0, Wv, AWv, hw, haw)
        assert mask == sum(1 << j for j in gone + [4]) and np.all(got[:, 4] == 0.0) and np.all(np.isfinite(got)) and np.all(np.isfinite(gota))
        for v in W_ALL[k:] + AW_ALL[k:]:
            assert np.all(np.isnan(np.array(p.download(0, *v)))), v
    finally:
        if p is not None:
            p.close()


@pytest.mark.parametrize("name", list(TRIPS))
def test_orthonormalize_trip_loop(backend, name):
    """k = 5, kappa = 1e3 with companions on levels where a block of the Gram kernel takes two and four trips (256^2, 2^17
    points): the checks of one step (the companion is a second random block: the product bound does not need an operator)"""
    rng = np.random.RandomState(47)
    make, lowest = TRIPS[name]
    p = None
    try:
        p = Plan(make(), lowest, nvec=12)
        n = p.size(0)
        assert (n + 63) // 64 == {"2d_n65536_two_trips": 2, "1d_n131072_four_trips": 4}[name] * 512
        Wv, AWv = [(W, 1 + t) for t in range(5)], [(F, 2 + t) for t in range(5)]
        _fill_nan(p, 0, [(s, q) for s in (F, W) for q in range(12)])
        _check_one_step(p, 0, Wv, AWv, graded(rng, n, 5, 1e3), rng.standard_normal((n, 5)), name)
        for v in ((W, 0), (W, 6), (F, 1), (F, 7)):
            assert np.all(np.isnan(np.array(p.download(0, *v))))
    finally:
        if p is not None:
            p.close()


def test_orthonormalize_refusals(backend):
    """MGCMT_ERR_INVALID, each with its message: null lists, k out of range, one companion list without the other, a W or an AW
    named twice, an AW that is a W, drop_tol outside (0, 1), vectors the plan does not hold; the export is there and the limit
    itself runs"""
    assert "mgcmt_block_orthonormalize" in _lib.EXPORTED_SYMBOLS
    p = None
    try:
        p = Plan(_box2d(16), 4, nvec=NVEC)
        L = _lib.lib()
        assert hasattr(L, "mgcmt_block_orthonormalize")
        one, zero = (ctypes.c_int * 1)(W), (ctypes.c_int * 1)(0)
        tol = ctypes.c_double(1e-13)
        for args in ((None, zero), (one, None)):
            assert L.mgcmt_block_orthonormalize(p._h, 0, 1, args[0], args[1], None, None, tol, None, None, None) == -1
            assert b"block_orthonormalize: non-null vector lists" in L.mgcmt_last_error()
        for args in ((one, None), (None, zero)):
            assert L.mgcmt_block_orthonormalize(p._h, 0, 1, one, zero, args[0], args[1], tol, None, None, None) == -1
            assert b"both or not at all" in L.mgcmt_last_error()

        def refused(w, aw, message, drop_tol=1e-13):
            with pytest.raises(_lib.MgcmtError) as e:
                p.block_orthonormalize(0, w, aw, drop_tol=drop_tol)
            assert "mgcmt error -1:" in str(e.value) and message in str(e.value), str(e.value)       # MGCMT_ERR_INVALID
        refused([], None, "1..16 vectors W")
        refused([(W, j) for j in range(17)], None, "1..16 vectors W")
        refused([(W, 0), (W, 1), (W, 0)], None, "a vector W named twice")
        refused([(W, 0), (W, 1)], [(F, 0), (F, 0)], "a vector AW named twice")
        refused([(W, 0), (W, 1)], [(F, 0), (W, 0)], "a vector AW that is also a W")
        for bad in (0.0, 1.0, -1e-13, 2.0, float("nan"), float("inf")):
            refused([(W, 0)], None, "drop_tol lies in (0, 1)", drop_tol=bad)
        with pytest.raises(ValueError):
            p.block_orthonormalize(0, [(W, 0), (W, 1)], [(F, 0)])
        with pytest.raises(_lib.MgcmtError) as e:
            p.block_orthonormalize(0, [(W, NVEC)], None)            # vectors the plan does not hold
        assert "mgcmt error -1:" in str(e.value)
        with pytest.raises(_lib.MgcmtError) as e:
            p.block_orthonormalize(0, [(W, 0)], [(F, -1)])
        assert "mgcmt error -1:" in str(e.value)
        with pytest.raises(_lib.MgcmtError) as e:
            p.block_orthonormalize(p.num_levels, [(W, 0)], None)    # a level the plan does not have
        assert "mgcmt error -1:" in str(e.value)
        rng = np.random.RandomState(3)
        Wv, AWv = [(W, j) for j in range(16)], [(F, j) for j in range(16)]
        _upload(p, 0, Wv, rng.standard_normal((p.size(0), 16)))
        _upload(p, 0, AWv, rng.standard_normal((p.size(0), 16)))
        assert p.block_orthonormalize(0, Wv, AWv, drop_tol=1e-13, want_dropped=True) == 0      # the limit itself runs
    finally:
        if p is not None:
            p.close()
