"""The wide block operations (csrc/kernels_blockwide.hip: mgcmt_block_pencil on the matrix cores, mgcmt_block_combine_wide)
against NumPy, and drivers.block_eigensolve with more than four states.

Tolerances.  A pencil entry is a sum of n products: against the np.longdouble reference it may differ by
gamma_n (|s_i|^T |as_j|), gamma_n = n u / (1 - n u), u = 2^-53 — the bound of any summation order, fused or not.  A combine
entry is a sum of nin products: gamma_nin (|IN| |C|).  Nothing wider is used."""
import numpy as np
import pytest

from multigridcmt_amd import _lib, drivers
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


# (name, operator, lowest, level): 2-D levels of 1024, 64, 16 and 4 points — above, at and below one block step of 64 points
# (a wave's four K groups take 16 of them) —, a 3-D level of 512, a 2-D plan with a point diagonal
PLANS = {
    "2d_n1024": (lambda: _box2d(32), 2, 0),
    "2d_n64": (lambda: _box2d(32), 2, 2),
    "2d_n16": (lambda: _box2d(32), 2, 3),
    "2d_n4": (lambda: _box2d(32), 2, 4),
    "3d_n512": (lambda: laplacian_operator(8, "3d") * (-1 / np.pi ** 2), 2, 0),
    "2d_point_n1024": (lambda: _pot2d(32), 2, 0),
}
NVEC = 48


def _plan(name):
    make, lowest, level = PLANS[name]
    return Plan(make(), lowest, nvec=NVEC), level


def _poison(p, level, rng, named):
    """NaN in every vector of slots V, F, W on the level, then random numbers in the `named` ones; returns their host copies"""
    n = p.size(level)
    nan = np.full(n, np.nan)
    for slot in (V, F, W):
        for q in range(NVEC):
            p.upload(level, slot, q, nan)
    host = {}
    for v in sorted(named):
        host[v] = rng.standard_normal(n)
        p.upload(level, v[0], v[1], host[v])
    return host


def _spread(m, slot_a, slot_b, first=0):
    """m vectors spread over two slots: the even ones in slot_a, the odd ones in slot_b"""
    return [((slot_a if t % 2 == 0 else slot_b), first + t // 2) for t in range(m)]


@pytest.mark.parametrize("name", list(PLANS))
@pytest.mark.parametrize("with_ms", [False, True])
def test_pencil_against_longdouble(backend, name, with_ms):
    """H = S^T AS and G = S^T MS (S^T S without MS) for m = 1, 5, 16, 17, 39, 48 independent random vectors spread over two
    slots.  Before every call EVERY vector of the three slots that the call does not name is NaN (so a padding lane that read
    a neighbour, or a tile that read vector m, shows): finite, within gamma_n |s_i|^T |as_j| of the longdouble sums,
    bit-identical when the call is repeated, and G exactly symmetric without MS."""
    rng = np.random.RandomState(3)
    # S: W and V alternating, columns 0..23; AS: F columns 0..47; MS: V and W alternating, columns 24..47
    S_all, AS_all, MS_all = _spread(48, W, V), [(F, t) for t in range(48)], _spread(48, V, W, first=24)
    p = None
    try:
        p, level = _plan(name)
        n = p.size(level)
        for m in (1, 5, 16, 17, 39, 48):
            S, AS, MS = S_all[:m], AS_all[:m], MS_all[:m] if with_ms else None
            host = _poison(p, level, rng, set(S + AS + (MS or [])))
            H, G = p.block_pencil(level, S, AS, MS)
            H2, G2 = p.block_pencil(level, S, AS, MS)
            assert H.shape == G.shape == (m, m)
            assert np.all(np.isfinite(H)) and np.all(np.isfinite(G))
            assert np.array_equal(H, H2) and np.array_equal(G, G2)
            if not with_ms:
                assert np.array_equal(G, G.T)
            s = np.stack([host[v] for v in S], axis=1).astype(np.longdouble)
            a = np.stack([host[v] for v in AS], axis=1).astype(np.longdouble)
            b = np.stack([host[v] for v in MS], axis=1).astype(np.longdouble) if with_ms else s
            for got, rhs in ((H, a), (G, b)):
                err = np.abs(got.astype(np.longdouble) - s.T @ rhs)
                bound = gamma(n) * (np.abs(s).T @ np.abs(rhs))
                print("%s m=%d n=%d max err/bound %.3f" % (name, m, n, float((err / bound).max())))
                assert np.all(err <= bound), (name, m, float((err / bound).max()))
    finally:
        if p is not None:
            p.close()


COMBINE_SHAPES = [(1, 1), (13, 5), (32, 16), (48, 16)]


@pytest.mark.parametrize("name", ["2d_n1024", "2d_n64", "2d_n4", "3d_n512", "2d_point_n1024"])
def test_combine_wide_against_numpy(backend, name):
    """OUT = IN C for (nin, nout) = (1, 1), (13, 5), (32, 16), (48, 16), inputs spread over two slots, outputs in a third:
    within gamma_nin |IN| |C| per entry; inputs unchanged; unnamed vectors (NaN) neither read nor written."""
    rng = np.random.RandomState(11)
    IN_all, OUT_all = _spread(48, W, V), [(F, 20 + j) for j in range(16)]
    p = None
    try:
        p, level = _plan(name)
        host = _poison(p, level, rng, set(IN_all))
        n = p.size(level)
        for nin, nout in COMBINE_SHAPES:
            ins, outs = IN_all[:nin], OUT_all[:nout]
            C = rng.standard_normal((nin, nout))
            p.block_combine_wide(level, ins, outs, C)
            X = np.stack([host[v] for v in ins], axis=1)
            want = X.astype(np.longdouble) @ C.astype(np.longdouble)
            bound = gamma(nin) * (np.abs(X) @ np.abs(C))
            got = np.stack([np.array(p.download(level, *v)) for v in outs], axis=1)
            assert np.all(np.isfinite(got))
            err = np.abs(got.astype(np.longdouble) - want)
            assert np.all(err <= bound), (name, nin, nout, float((err / np.maximum(bound, 1e-300)).max()))
            for v in ins:
                assert np.array_equal(np.array(p.download(level, *v)), host[v])
        # the outputs beyond the sixteenth column written and everything unnamed are still NaN
        for v in [(F, 0), (F, 19), (F, 36), (W, 30), (V, 47)]:
            assert np.all(np.isnan(np.array(p.download(level, *v))))
    finally:
        if p is not None:
            p.close()


@pytest.mark.parametrize("g,k", [(32, 16), (32, 7), (2, 3)])
def test_combine_wide_outputs_aliasing_inputs(backend, g, k):
    """[X | P] -> X with C = [C_x; I], and X -> X C, as the eigen-solver issues them: an output may be one of the inputs.
    g = 2: four points per vector."""
    rng = np.random.RandomState(g + k)
    p = None
    try:
        p = Plan(_box2d(max(g, 4)), 2, nvec=NVEC)
        level = p.num_levels - 1 if g == 2 else 0
        n = p.size(level)
        X, P = [(W, j) for j in range(k)], [(W, 2 * k + j) for j in range(k)]
        hx, hp = rng.standard_normal((n, k)), rng.standard_normal((n, k))
        for j in range(k):
            p.upload(level, *X[j], hx[:, j])
            p.upload(level, *P[j], hp[:, j])
        Cx = rng.standard_normal((k, k))
        C = np.vstack([Cx, np.eye(k)])
        p.block_combine_wide(level, X + P, X, C)
        IN = np.hstack([hx, hp])
        got = np.stack([np.array(p.download(level, *v)) for v in X], axis=1)
        err = np.abs(got.astype(np.longdouble) - IN.astype(np.longdouble) @ C.astype(np.longdouble))
        assert np.all(err <= gamma(2 * k) * (np.abs(IN) @ np.abs(C)))
        for j in range(k):
            assert np.array_equal(np.array(p.download(level, *P[j])), hp[:, j])
        p.block_combine_wide(level, X, X, Cx)
        got2 = np.stack([np.array(p.download(level, *v)) for v in X], axis=1)
        err = np.abs(got2.astype(np.longdouble) - got.astype(np.longdouble) @ Cx.astype(np.longdouble))
        assert np.all(err <= gamma(k) * (np.abs(got) @ np.abs(Cx)))
    finally:
        if p is not None:
            p.close()


def test_wide_entries_on_1d_levels(backend):
    """every level of a 1-D plan, 64 points down to 2 (fewer than one lane's run of four).  An odd number of points per
    vector cannot be formed through the library: every level has a power of two of them, and vectors start on 16-byte
    boundaries at least (the one-point-per-thread forms of the kernels are a guard for layouts the plan does not produce today)."""
    rng = np.random.RandomState(2)
    p = None
    try:
        p = Plan(laplacian_operator(64, "1d"), 2, nvec=NVEC)
        for level in range(p.num_levels):
            n = p.size(level)
            nin, nout = 13, 5
            ins, outs = [(W, t) for t in range(nin)], [(F, 3 + j) for j in range(nout)]
            X = rng.standard_normal((n, nin))
            for t in range(nin):
                p.upload(level, *ins[t], X[:, t])
            C = rng.standard_normal((nin, nout))
            p.block_combine_wide(level, ins, outs, C)
            got = np.stack([np.array(p.download(level, *v)) for v in outs], axis=1)
            err = np.abs(got.astype(np.longdouble) - X.astype(np.longdouble) @ C.astype(np.longdouble))
            assert np.all(err <= gamma(nin) * (np.abs(X) @ np.abs(C)))
            H, G = p.block_pencil(level, ins, ins[::-1])
            ref = X.astype(np.longdouble).T @ X[:, ::-1].astype(np.longdouble)
            assert np.all(np.abs(H.astype(np.longdouble) - ref) <= gamma(n) * (np.abs(X).T @ np.abs(X[:, ::-1])))
    finally:
        if p is not None:
            p.close()


def test_refusals(backend):
    """MGCMT_ERR_INVALID for 49 vectors, 17 outputs, an output named twice, nvec = 81, and — on a plan that stores 48 — a cycle,
    a shift set, a Gram-Schmidt, a sharded cycle / gather / halo exchange of 33 columns and an apply with the shift of column
    32 (refused, not overrun: the shifts and the reduction results hold 32)"""
    p = None
    try:
        p = Plan(_box2d(16), 4, nvec=NVEC)
        S49 = [(W, t) for t in range(48)] + [(V, 0)]
        with pytest.raises(_lib.MgcmtError) as e:
            p.block_pencil(0, S49, S49)
        assert "mgcmt error -1:" in str(e.value)          # MGCMT_ERR_INVALID
        with pytest.raises(_lib.MgcmtError) as e:
            p.block_combine_wide(0, S49, [(F, 0)], np.zeros((49, 1)))
        assert "mgcmt error -1:" in str(e.value)          # MGCMT_ERR_INVALID
        with pytest.raises(_lib.MgcmtError) as e:
            p.block_combine_wide(0, S49[:3], [(F, j) for j in range(17)], np.zeros((3, 17)))
        assert "mgcmt error -1:" in str(e.value)          # MGCMT_ERR_INVALID
        with pytest.raises(_lib.MgcmtError) as e:
            p.block_combine_wide(0, S49[:3], [(F, 0), (F, 1), (F, 0)], np.zeros((3, 3)))
        assert "mgcmt error -1:" in str(e.value)          # MGCMT_ERR_INVALID
        with pytest.raises(_lib.MgcmtError) as e:
            p.block_pencil(0, [(W, 48)], [(W, 0)])          # a vector the plan does not hold
        assert "mgcmt error -1:" in str(e.value)          # MGCMT_ERR_INVALID
        with pytest.raises(_lib.MgcmtError) as e:
            p.vcycle(1, 1, _lib.GS_MC, k=33, nu_coarse=1)
        assert "mgcmt error -1:" in str(e.value)          # MGCMT_ERR_INVALID
        with pytest.raises(_lib.MgcmtError) as e:
            p.set_shifts(np.zeros(33))
        assert "mgcmt error -1:" in str(e.value)          # MGCMT_ERR_INVALID
        with pytest.raises(_lib.MgcmtError) as e:
            p.gramschmidt(0, W, 33)
        assert "mgcmt error -1:" in str(e.value)          # MGCMT_ERR_INVALID
        # the shift of a column: the plan holds 32 of them, an apply with a shift of column 32.. would read past them
        with pytest.raises(_lib.MgcmtError) as e:
            p.apply(0, (W, 32), (F, 0), with_shift=True)
        assert "mgcmt error -1:" in str(e.value)
        p.apply(0, (W, 32), (F, 0))                         # without a shift every stored column applies
        p.apply(0, (W, 31), (F, 0), with_shift=True)
        # the sharded entries refuse more than 32 columns before anything else (no communicator is needed to see it)
        c = Plan(_box2d(16), 4, nvec=NVEC)
        try:
            L = _lib.lib()
            for call in (lambda: L.mgcmt_sharded_vcycle(p._h, c._h, 1, 1, 1, _lib.WJACOBI, 2. / 3., 33, 0, None),
                         lambda: L.mgcmt_gather_coarse(p._h, 0, V, c._h, V, 33, None),
                         lambda: L.mgcmt_halo_exchange(p._h, 0, (1 << V) | (33 << 16), None)):
                assert call() == -1 and b"at most 32 columns" in L.mgcmt_last_error()
        finally:
            c.close()
        p.set_shifts(np.zeros(32))
        p.vcycle(1, 1, _lib.GS_MC, k=32, nu_coarse=1)       # 32 columns still run on it
    finally:
        if p is not None:
            p.close()
    with pytest.raises(_lib.MgcmtError) as e:
        Plan(_box2d(16), 4, nvec=81)
    assert "mgcmt error -1:" in str(e.value)          # MGCMT_ERR_INVALID
    Plan(_box2d(16), 4, nvec=80).close()


# ---- the solver ----------------------------------------------------------------------------------------------------------

def _anharmonic(g):
    t = (np.arange(g) + 0.5) / g
    X, Y = np.meshgrid(t, t, indexing="ij")
    return potential_operator(g, 40.0 * ((X - 0.47) ** 2 + 1.7 * (Y - 0.55) ** 2) + 3.0 * np.sin(7 * X) * np.cos(5 * Y) + 3.0)


def _check_solution(op, vals, vecs, want, res, k, mass=None):
    print("eigenvalue errors", np.abs(vals - want).max(), "orthonormality",
          np.abs(vecs.T @ ((mass @ vecs) if mass is not None else vecs) - np.eye(k)).max(), "residual drop", res[-1].max() / res[0].max())
    assert np.allclose(vals, want, rtol=0, atol=1e-8), np.abs(vals - want)
    assert np.abs(vecs.T @ vecs - np.eye(k)).max() < 1e-10
    assert res[-1].max() < res[0].max() * 1e-3


@pytest.mark.parametrize("k", [13, 16])
def test_block_eigensolve_box_wide(backend, k):
    """-laplacian/pi^2 on 64^2, lowest = 4, 20 iterations: k = 13 (the block ends below the gap 19.34 -> 24.17) and k = 16 (the
    16th level degenerate with the 17th) within 1e-8 of the exact discrete eigenvalues, orthonormal to 1e-10, residuals down
    by 1e3."""
    op = _box2d(64)
    res = []
    vals, vecs = drivers.block_eigensolve(op, k=k, cycles=20, lowest=4, residuals=res)
    _check_solution(op, vals, vecs, drivers.exact_box_eigenvalues(64, "2d", k), res, k)


def test_block_eigensolve_anharmonic_wide(backend):
    """an arbitrary potential (the Rayleigh-quotient routines refuse it; this driver is its only eigensolver): 13 states of
    V = 40 ((x - 0.47)^2 + 1.7 (y - 0.55)^2) + 3 sin 7x cos 5y + 3 at 64^2, lowest = 8, 20 iterations, against eigsh(sigma=0)"""
    import scipy.sparse.linalg as sla
    k = 13
    op = _anharmonic(64)
    res = []
    vals, vecs = drivers.block_eigensolve(op, k=k, cycles=20, lowest=8, residuals=res)
    want = np.sort(sla.eigsh(op.tocsr(), k=k, sigma=0.0, which="LM")[0])
    _check_solution(op, vals, vecs, want, res, k)


def test_block_eigensolve_mass_wide(backend):
    """the Mehrstellen pencil of tests/test_drivers.py::test_block_eigensolve_with_a_mass_operator at k = 6: eigsh to 1e-9,
    vectors M-orthonormal"""
    import scipy.sparse.linalg as sla
    from multigridcmt_amd.operators import mehrstellen_mass, mehrstellen_operator
    g, k = 64, 6
    A, M = mehrstellen_operator(g) * (-1 / np.pi ** 2), mehrstellen_mass(g)
    res = []
    vals, vecs = drivers.block_eigensolve(A, k=k, cycles=12, lowest=8, mass=M, residuals=res)
    As, Ms = A.tocsr(), M.tocsr()
    want = np.sort(sla.eigsh(As, k=k, M=Ms, sigma=0.0, which="LM")[0])
    print("eigenvalue errors", np.abs(vals - want).max())
    assert np.allclose(vals, want, rtol=1e-9, atol=1e-9), np.abs(vals - want)
    assert np.abs(vecs.T @ (Ms @ vecs) - np.eye(k)).max() < 1e-9
    assert res[-1].max() < res[0].max() * 1e-3


BOX3D_CYCLES = 16   # the eigenvalue error of the 11th state on the emulation: 1.7e-6 after 12 iterations, 1.4e-9 after 16


def test_block_eigensolve_box_3d_wide(backend):
    """the 16^3 box, k = 11 (levels 3, 6 x3, 9 x3, 11 x3, 12 | 14), lowest = 4: within 1e-8 of drivers.exact_box_eigenvalues after
    16 iterations — the smallest multiple of four that reaches the bar on the emulation (1.7e-6 after 12, 1.4e-9 after 16)."""
    g, k = 16, 11
    op = laplacian_operator(g, "3d") * (-1 / np.pi ** 2)
    res = []
    vals, vecs = drivers.block_eigensolve(op, k=k, cycles=BOX3D_CYCLES, lowest=4, residuals=res)
    assert BOX3D_CYCLES <= 32
    _check_solution(op, vals, vecs, drivers.exact_box_eigenvalues(g, "3d", k), res, k)


def test_block_eigensolve_limit():
    with pytest.raises(ValueError, match="16"):
        drivers.block_eigensolve(_box2d(16), k=17)


def test_block_eigensolve_k4_is_bit_identical_to_the_parent(backend):
    """k = 4 on the 64^2 box with a fixed seed: values and vectors bit-identical to what the commit before the wide kernels
    gave on the same backend (tests/golden/block_eigensolve_k4_box64.npz, generated once from that build: `emu_*` through the
    emulation, `hip_*` on the MI355X)"""
    from conftest import load_golden
    gold = load_golden("block_eigensolve_k4_box64")
    vals, vecs = drivers.block_eigensolve(_box2d(64), k=4, cycles=6, lowest=4, seed=7)
    assert np.array_equal(vals, gold[backend + "_vals"])
    assert np.array_equal(vecs, gold[backend + "_vecs"])
