"""Arbitrary potentials V(x, y): 2-D operators with a per-point diagonal (operators.potential_operator /
recognise_potential, mgcmt_plan_create_pot) against the NumPy oracle (oracle.sparse_ref.RefSolver, which cycles any
sparse matrix) and against scipy's own R*A*P, through the HIP library on the GPU box and through the emulated kernels on
CPU (``backend`` fixture).

The fine level of such a plan runs the fused row-streaming pass (policy Op5P, csrc/fused_kernel.h), the variable 9-point
levels below it the one-launch-per-operation kernels of csrc/kernels_pointwise.hip (DESIGN par. 4.13)."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import rel_err
from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, _lib, drivers
from multigridcmt_amd.operators import (StructuredOperator, UnrecognisedOperator, potential_operator, recognise, recognise_potential,
                                        tri_to_sparse)
from multigridcmt_amd.plan import Plan, get_plan
from oracle.sparse_ref import RefSolver, RefStencilMaker

TOL = 1e-10          # the bar of tests/test_3d_cycle.py
SCALE = -1 / np.pi ** 2


@pytest.fixture(autouse=True, scope="module")
def _release_host_buffers():
    yield
    import gc
    from multigridcmt_amd import hostmem
    gc.collect()
    hostmem.drain()


def smooth_v(g):
    """40 (x^2 + x y + y^2) + 10 exp(-12 (x - y)^2) on the cell centres of [-1/2, 1/2]^2: smooth, non-negative, and not
    a(x) + b(y) plus ONE product (x y alone would be one: recognise takes that) — the ridge along x = y has full rank"""
    x = (np.arange(g) + 0.5) / g - 0.5
    X, Y = np.meshgrid(x, x, indexing="ij")
    return 40.0 * (X * X + X * Y + Y * Y) + 10.0 * np.exp(-12.0 * (X - Y) ** 2)


def rough_v(g, seed=1):
    """the same plus disorder: 5 * uniform noise per point"""
    return smooth_v(g) + 5.0 * np.random.RandomState(seed).rand(g, g)


def hamiltonian(g, V):
    """(-1/pi^2) laplacian(g, '2d') + diag(V) as the reference's callers would assemble it"""
    return (SCALE * MGCMTStencilMaker().laplacian(g, dimension="2d") + sp.diags(np.asarray(V).reshape(-1))).tocsr()


def flat(a):
    return np.asarray(a).reshape(-1)


def rb(ref):
    return lambda v, f, A, nu=4: ref.gseidel_mc(v, f, A, nu=nu, dimension="2d")


def assemble_level(plan, level):
    """the matrix of `level`: Kronecker factors (mgcmt_plan_get_factors) plus the per-point part (mgcmt_plan_get_point_stencil)"""
    gl = plan.g >> level
    xf, yf = plan.factors(level, 0), plan.factors(level, 1)
    A = sum(sp.kron(tri_to_sparse(xf[m]), tri_to_sparse(yf[m]), format="csr") for m in range(xf.shape[0])).tocsr()
    G = plan.point_stencil(level)
    if level == 0:
        assert G.shape == (gl, gl)
        return (A + sp.diags(G.reshape(-1))).tocsr()
    assert G.shape == (3, 3, gl, gl)
    B = sp.lil_matrix((gl * gl, gl * gl))
    for a in range(3):
        for b in range(3):
            for i in range(gl):
                for j in range(gl):
                    ii, jj = i + a - 1, j + b - 1
                    if 0 <= ii < gl and 0 <= jj < gl:
                        B[i * gl + j, ii * gl + jj] = G[a, b, i, j]
                    else:
                        assert G[a, b, i, j] == 0.0          # nothing points outside the grid
    return (A + B.tocsr()).tocsr()


def galerkin_chain(A, g, lowest):
    """[A, R A P, R (R A P) P, ...] down to lowest^2 points with MGCMTStencilMaker's own matrices (MGCMTSolver.py:318)"""
    sm = MGCMTStencilMaker()
    out = [sp.csr_matrix(A)]
    while g > lowest:
        R = sm.restriction(g, g // 2, dimension="2d")
        P = sm.interpolation(g // 2, g, dimension="2d")
        out.append((R @ out[-1] @ P).tocsr())
        g //= 2
    return out


def test_recognise_potential_round_trip():
    """recognise_potential maps a 5-point matrix with ANY diagonal; recognise keeps refusing what it refused."""
    g = 16
    for name, V in (("smooth", smooth_v(g)), ("random", np.random.RandomState(3).rand(g, g) * 30.0), ("zero", np.zeros((g, g)))):
        A = hamiltonian(g, V)
        op = recognise_potential(A)
        assert abs(op.tocsr() - A).max() <= 1e-13 * abs(A).max(), name
        if name == "zero":
            assert op.point_diagonal is None and op is recognise(A, "2d")      # what recognise returns today
        else:
            assert op.point_diagonal is not None and op.point_diagonal.shape == (g, g)
            with pytest.raises(UnrecognisedOperator):
                recognise(A, "2d")
            with pytest.raises(UnrecognisedOperator):
                recognise(A)
    # a separable potential and one square well stay with recognise's Kronecker terms
    a = np.random.RandomState(4).rand(g)
    assert recognise_potential(hamiltonian(g, a[:, None] + 2.0 * a[None, :])).point_diagonal is None
    # not a 5-point matrix: still refused
    with pytest.raises(UnrecognisedOperator):
        recognise_potential(sp.random(g * g, g * g, density=0.02, random_state=5, format="csr") + sp.identity(g * g))


def test_operator_algebra_carries_the_point_diagonal():
    g = 8
    V = rough_v(g)
    op = potential_operator(g, V)
    A = hamiltonian(g, V)
    assert abs(op.tocsr() - A).max() <= 1e-13 * abs(A).max()
    assert np.allclose(op.diagonal(), A.diagonal(), rtol=1e-14)
    assert abs((op * 2.5).tocsr() - 2.5 * A).max() <= 1e-13 * abs(A).max()
    assert abs((-op / 4.0).tocsr() + A / 4.0).max() <= 1e-13 * abs(A).max()
    assert abs(op.shifted(0.7).tocsr() - (A - 0.7 * sp.identity(g * g))).max() <= 1e-13 * abs(A).max()
    assert op.fingerprint() != potential_operator(g, V + 1e-9).fingerprint()
    assert op.fingerprint() != potential_operator(g, np.zeros((g, g))).fingerprint()
    with pytest.raises(ValueError):
        StructuredOperator("1d", g, [(None, np.zeros((3, g)))], point_diagonal=np.zeros(g))
    with pytest.raises(ValueError):
        potential_operator(g, np.zeros(g))


@pytest.mark.parametrize("g", [16, 32, 64])
def test_galerkin_hierarchy_and_apply_on_every_level(backend, g):
    """R*A*P of every level — Kronecker factors plus mgcmt_plan_get_point_stencil — against scipy's product of
    MGCMTStencilMaker's own matrices, and mgcmt_apply on every level against that matrix (with and without the shift)."""
    V = rough_v(g)
    plan = Plan(potential_operator(g, V), 2, nvec=1)
    try:
        chain = galerkin_chain(hamiltonian(g, V), g, 2)
        assert plan.num_levels == len(chain)
        plan.set_shifts([0.7])
        rng = np.random.RandomState(g)
        for level, want in enumerate(chain):
            assert plan.operator_kind(level) == (_lib.OPK_POINT_DIAG if level == 0 else _lib.OPK_NINE_POINT)
            # the fine level on the fused pass (levels of at least 4 x 16 points), the variable 9-point levels per launch
            for kind in (_lib.WJACOBI, _lib.GS_MC):
                assert plan.fused_max_sweeps(level, kind) == (2 if level == 0 else 0), (level, kind)
            got = assemble_level(plan, level)
            assert abs(got - want).max() <= 1e-13 * abs(want).max(), level
            if level:
                assert abs(got - got.T).max() <= 1e-13 * abs(want).max()          # R = P^T / 4: the levels stay symmetric
            x = rng.rand(want.shape[0]) - 0.5
            plan.upload(level, _lib.SLOT_V, 0, x)
            plan.apply(level, (_lib.SLOT_V, 0), (_lib.SLOT_T, 0))
            assert rel_err(plan.download(level, _lib.SLOT_T, 0), want @ x) < 1e-13, level
            plan.apply(level, (_lib.SLOT_V, 0), (_lib.SLOT_T, 0), with_shift=True)
            assert rel_err(plan.download(level, _lib.SLOT_T, 0), want @ x - 0.7 * x) < 1e-13, level
    finally:
        plan.close()
    # A.dot(x) of the operator object
    op = potential_operator(16, rough_v(16))
    x = np.random.RandomState(2).rand(256)
    assert rel_err(op.dot(x), op.tocsr() @ x) < 1e-13


def test_smoothers_stand_alone(backend):
    g = 32
    V = rough_v(g)
    A, op = hamiltonian(g, V), potential_operator(g, V)
    solver, ref = MGCMTSolver(), RefSolver()
    rng = np.random.RandomState(6)
    v0, f = rng.rand(g * g), rng.rand(g * g)
    want = ref.wjacobi(v0.copy(), f.copy(), A, nu=3)
    assert rel_err(flat(solver.wjacobi(v0.copy(), f.copy(), op, nu=3)), flat(want)) < TOL
    assert rel_err(flat(solver.smooth(v0.copy(), f.copy(), A, nu=3, smoother=solver.wjacobi, dimension="2d")), flat(want)) < TOL
    want = ref.gseidel_mc(v0.copy(), f.copy(), A, nu=2, dimension="2d")
    assert rel_err(flat(solver.gseidel_rb(v0.copy(), f.copy(), A, nu=2, dimension="2d")), flat(want)) < TOL
    assert rel_err(flat(solver.gseidel_rb(v0.copy(), f.copy(), op, nu=2)), flat(want)) < TOL
    want = ref.gseidel_mc(v0.copy(), f.copy(), A, nu=2, omega=1.3, dimension="2d")
    assert rel_err(flat(solver.gseidel_rb(v0.copy(), f.copy(), op, nu=2, omega=1.3)), flat(want)) < TOL


@pytest.mark.parametrize("smoother", ["wjacobi", "rb"])
@pytest.mark.parametrize("shift", [0, 1.9])
@pytest.mark.parametrize("lowest", [2, 4, 8])
@pytest.mark.parametrize("g", [16, 32, 64, 128])
def test_vcycle_against_the_oracle(backend, g, lowest, shift, smoother):
    """V(2,2) for (H - shift I) v = f, H = -laplacian/pi^2 + V with the smooth non-separable potential plus disorder
    (H > 2, so the shifted operator is definite on every level): from a zero start, called twice (the second call replays
    the captured graph), and from a non-zero start; as the matrix-free operator and as the sparse matrix
    (recognise_potential inside the 2-D entry point).  The oracle's own residual must fall, so that a diverging reference
    cannot hide a broken comparison."""
    V = rough_v(g)
    A, op = hamiltonian(g, V), potential_operator(g, V)
    solver, sm, ref, rsm = MGCMTSolver(), MGCMTStencilMaker(), RefSolver(), RefStencilMaker()
    smo, rsmo = (solver.wjacobi, None) if smoother == "wjacobi" else (solver.gseidel_rb, rb(ref))
    n = g * g
    f = np.random.RandomState(g + lowest).rand(n)
    kw = dict(nu1=2, nu2=2, shift=shift, lowest_level=lowest, dimension="2d")
    shifted = A - shift * sp.identity(n)
    v_ref, res = np.zeros(n), [np.linalg.norm(f)]
    for cycle in range(2):
        v_ref = np.asarray(ref.vcycle(v_ref.copy(), f.copy(), A, rsm, smoother=rsmo, **kw)).reshape(-1)
        res.append(np.linalg.norm(f - shifted @ v_ref))
        assert res[-1] < res[-2], res
    first = ref.vcycle(np.zeros(n), f.copy(), A, rsm, smoother=rsmo, **kw)
    for call in range(3):          # the second call captures the cycle's graph, the third replays it
        got = solver.vcycle(np.zeros(n), f.copy(), op, sm, smoother=smo, **kw)
        assert rel_err(got, first) < TOL, call
    assert rel_err(solver.vcycle(np.zeros(n), f.copy(), A, sm, smoother=smo, **kw), first) < TOL
    got2 = solver.vcycle(np.array(got), f.copy(), op, sm, smoother=smo, **kw)          # non-zero start: the second cycle
    assert rel_err(got2, v_ref) < TOL
    if g >= 128:          # the fused fine pass ran: the level is Op5P's and the fused kernels cover it
        plan = get_plan(op, lowest, nvec=1)
        assert plan.operator_kind(0) == _lib.OPK_POINT_DIAG and plan.operator_kind(1) == _lib.OPK_NINE_POINT
        kind = _lib.WJACOBI if smoother == "wjacobi" else _lib.GS_MC
        assert plan.fused_max_sweeps(0, kind) >= 1 and plan.fused_max_sweeps(1, kind) == 0


@pytest.mark.parametrize("smoother", ["wjacobi", "rb"])
def test_vcycle_matrix_with_column_shifts(backend, smoother):
    g, lowest, k = 32, 4, 3
    V = rough_v(g)
    A, op = hamiltonian(g, V), potential_operator(g, V)
    solver, sm, ref, rsm = MGCMTSolver(), MGCMTStencilMaker(), RefSolver(), RefStencilMaker()
    smo, rsmo = (solver.wjacobi, None) if smoother == "wjacobi" else (solver.gseidel_rb, rb(ref))
    rng = np.random.RandomState(9)
    F = rng.rand(g * g, k)
    shifts = np.array([0.0, 0.9, 1.9])
    kw = dict(nu1=2, nu2=2, shifts=shifts, lowest_level=lowest, dimension="2d")
    want = ref.vcycle_matrix(np.zeros((g * g, k)), F.copy(), A, rsm, smoother=rsmo, **kw)
    for start in (op, A):
        got = solver.vcycle_matrix(np.zeros((g * g, k)), F.copy(), start, sm, smoother=smo, **kw)
        assert rel_err(got, want) < TOL
    V0 = rng.rand(g * g, k)
    want = ref.vcycle_matrix(V0.copy(), F.copy(), A, rsm, smoother=rsmo, **kw)
    assert rel_err(solver.vcycle_matrix(V0.copy(), F.copy(), op, sm, smoother=smo, **kw), want) < TOL


def test_full_multigrid(backend):
    """fmg against the oracle's FMG on the assembled matrix, and against its own composition on two levels: the restricted
    right-hand side solved on the coarse level, interpolated (MGCMTSolver.interpolate), then one vcycle from that start."""
    import scipy.sparse.linalg as sla
    g = 32
    V = rough_v(g)
    A, op = hamiltonian(g, V), potential_operator(g, V)
    solver, sm, ref, rsm = MGCMTSolver(), MGCMTStencilMaker(), RefSolver(), RefStencilMaker()
    f = np.random.RandomState(10).rand(g * g)
    for smo, rsmo in ((solver.wjacobi, ref.wjacobi), (solver.gseidel_rb, rb(ref))):
        got = solver.fmg(f.copy(), op, sm, nu1=2, nu2=2, smoother=smo, shift=0.7, lowest_level=4, dimension="2d")
        want = ref.fmg(f, A, rsm, nu1=2, nu2=2, smoother=rsmo, shift=0.7, lowest_level=4, dimension="2d")
        assert rel_err(got, want) < TOL
    R, P = sm.restriction(g, g // 2, dimension="2d"), sm.interpolation(g // 2, g, dimension="2d")
    coarse = sla.spsolve(((R @ A @ P) - 0.7 * sp.identity(g * g // 4)).tocsc(), R @ f)
    start = solver.interpolate(coarse, sm, g, dimension="2d")
    want = solver.vcycle(start, f.copy(), op, sm, nu1=2, nu2=2, shift=0.7, lowest_level=g // 2, dimension="2d")
    got = solver.fmg(f.copy(), op, sm, nu1=2, nu2=2, shift=0.7, lowest_level=g // 2, dimension="2d")
    assert rel_err(got, want) < TOL


def _cycles(op, f, v0, kind, omega, fused, recompute, lowest, nus, k=1, shifts=(0.0,), rows=0):
    """iterates after one and two cycles, and the restricted residual the first left on level 1"""
    p = Plan(op, lowest, nvec=k)
    try:
        p.set_option(_lib.OPT_FUSED, fused)
        p.set_option(_lib.OPT_RECOMPUTE, recompute)      # 2: no-store down passes and recomputing up passes on every fused level
        p.set_option(_lib.OPT_FUSED_ROWS, rows)
        p.set_shifts(list(shifts))
        out = []
        for q in range(k):
            p.upload(0, _lib.SLOT_F, q, f[q])
            if v0 is not None:
                p.upload(0, _lib.SLOT_V, q, v0[q])
        for cycle in range(2):
            p.vcycle(nus[0], nus[1], kind, omega=omega, k=k, nu_coarse=nus[2], zero_start=(v0 is None and cycle == 0))
            out.append(np.stack([np.array(p.download(0, _lib.SLOT_V, q)) for q in range(k)]))
            if cycle == 0:
                out.append(np.stack([np.array(p.download(1, _lib.SLOT_F, q)) for q in range(k)]))
        return out
    finally:
        p.close()


@pytest.mark.parametrize("kind,omega", [(_lib.WJACOBI, 2. / 3.), (_lib.GS_MC, 1.0)])
def test_fused_fine_pass_gives_the_bits_of_the_unfused_kernels(backend, kind, omega):
    """MGCMT_OPT_FUSED = 0 against the fused fine-level pass (Op5P) on the same operator: bit-identical iterates and
    restricted residuals — plain, prolong, restrict and zero-in modes, and with MGCMT_OPT_RECOMPUTE = 2 the no-store down
    pass and the recomputing up pass; one and several columns with their own shifts, zero and non-zero start, odd chunk
    lengths, sweep counts that need more than one pass per leg."""
    one, three = (1, (0.7,)), (3, (0.0, 0.9, 1.9))
    every = ((2, 2, 2), (1, 1, 1), (3, 3, 2), (2, 1, 4))
    for g, lowest, columns, sweeps in ((32, 4, (one, three), every), (64, 8, (three,), every[::2]), (128, 8, (one,), every[:1])):
        op = potential_operator(g, rough_v(g))
        rng = np.random.RandomState(g)
        for k, shifts in columns:
            f = rng.rand(k, g * g)
            for v0 in (None, rng.rand(k, g * g)):
                for nus in sweeps:
                    want = _cycles(op, f, v0, kind, omega, 0, 0, lowest, nus, k, shifts)
                    for recompute, rows in ((0, 0), (1, 0), (2, 0), (2, 6)):
                        got = _cycles(op, f, v0, kind, omega, 1, recompute, lowest, nus, k, shifts, rows)
                        for a, b in zip(got, want):
                            assert np.array_equal(a, b), (g, k, v0 is None, nus, recompute, rows)


def test_foreign_smoother_sees_the_level_matrices(backend):
    """The seam of MGCMTSolver.py:313,326: a callable smoother receives (R A P - shift I) of every level — the variable
    9-point levels included — and the cycle built around it equals the reference's."""
    g, lowest = 32, 4
    V = rough_v(g)
    A, op = hamiltonian(g, V), potential_operator(g, V)
    solver, sm, ref, rsm = MGCMTSolver(), MGCMTStencilMaker(), RefSolver(), RefStencilMaker()
    chain = galerkin_chain(A, g, lowest)
    seen = {}

    def damped(v, f, M, nu=4):
        M = sp.csr_matrix(M)
        seen[M.shape[0]] = M
        v, f = np.asarray(v, dtype=float).reshape(-1).copy(), np.asarray(f, dtype=float).reshape(-1)
        for _ in range(nu):
            v = v + 0.6 * (f - M @ v) / M.diagonal()
        return v.reshape(-1, 1)

    f = np.random.RandomState(12).rand(g * g)
    got = solver.vcycle(np.zeros(g * g), f.copy(), op, sm, nu1=2, nu2=2, smoother=damped, shift=0.7, lowest_level=lowest, dimension="2d")
    assert sorted(seen) == [64, 256, 1024]          # 8^2, 16^2, 32^2: every level above the coarsest
    for level, want in enumerate(chain[:-1]):
        M = seen[want.shape[0]]
        assert abs(M - (want - 0.7 * sp.identity(want.shape[0]))).max() <= 1e-13 * abs(want).max(), level
    want = ref.vcycle(np.zeros(g * g), f.copy(), A, rsm, nu1=2, nu2=2, smoother=damped, shift=0.7, lowest_level=lowest, dimension="2d")
    assert rel_err(got, want) < TOL


def test_unsupported_entries_name_the_point_diagonal(backend):
    g = 16
    op = potential_operator(g, rough_v(g))
    plan = Plan(op, 4, nvec=6)
    lib = _lib.lib()
    h = plan._h
    i6 = (ctypes.c_int * 6)(0, 1, 2, 3, 4, 5)
    i2 = [(ctypes.c_int * 2)(_lib.SLOT_V, q) for q in range(4)]
    out = (ctypes.c_double * 8)()
    calls = {
        "gseidel": lambda: lib.mgcmt_smooth(h, 0, _lib.GS_LEX, 1, 1.0, 1, None),
        "sor": lambda: lib.mgcmt_smooth(h, 0, _lib.SOR_LEX, 1, 1.2, 1, None),
        "vcycle lex": lambda: lib.mgcmt_vcycle(h, 0, 2, 2, 2, _lib.GS_LEX, 1.0, 1, 0, None),
        "twogrid": lambda: lib.mgcmt_twogrid(h, 0, 2, 2, _lib.WJACOBI, 2. / 3., 1, None),
        "rqmin": lambda: lib.mgcmt_rqmin(h, 0, _lib.SLOT_V, i6, 2, 0, out, None),
        "rq_line_step": lambda: lib.mgcmt_rq_line_step(h, 0, i2[0], i2[1], i2[2], i2[3], None, 0, -1, None),
        "vcycle_rqmg": lambda: lib.mgcmt_vcycle_rqmg(h, _lib.SLOT_V, i6, 2, 2, 0, out, None),
        "ritz_pair": lambda: lib.mgcmt_ritz_pair(h, 0, _lib.SLOT_V, 0, _lib.SLOT_V, 1, _lib.SLOT_V, 2, out, None),
        "rayleigh_residual": lambda: lib.mgcmt_rayleigh_residual(h, 0, _lib.SLOT_V, 1, out, out, None),
        "comm_init": lambda: lib.mgcmt_comm_init(h, 0, 1, ctypes.create_string_buffer(_lib.UNIQUE_ID_BYTES)),
        "comm_init_external": lambda: lib.mgcmt_comm_init_external(
            h, 0, 1, _lib.P2P_FN(lambda *a: 0), _lib.ALLGATHER_FN(lambda *a: 0), _lib.ALLREDUCE_FN(lambda *a: 0), None),
        "sharded_vcycle": lambda: lib.mgcmt_sharded_vcycle(h, h, 2, 2, 2, _lib.WJACOBI, 2. / 3., 1, 0, None),
    }
    try:
        for name, call in calls.items():
            assert call() == -4, name          # MGCMT_ERR_UNSUPPORTED
            assert b"point diagonal" in lib.mgcmt_last_error(), (name, lib.mgcmt_last_error())
        # creation: no mass operator, no strips, 2-D only
        nterms, xfac, yfac = op.factor_blocks()
        desc = _lib.PlanDesc()
        desc.dim, desc.nterms, desc.g, desc.lowest, desc.nvec = 2, nterms, g, 4, 1
        desc.xfac, desc.yfac = _lib.as_dp(xfac), _lib.as_dp(yfac)
        pd = np.ascontiguousarray(op.point_diagonal)
        hh = ctypes.c_void_p()
        desc.row_begin, desc.row_end, desc.strip_levels = 0, g // 2, 1
        assert lib.mgcmt_plan_create_pot(ctypes.byref(desc), _lib.as_dp(pd), ctypes.byref(hh)) == -4
        assert b"point diagonal" in lib.mgcmt_last_error()
        desc.row_begin, desc.row_end, desc.strip_levels = 0, 0, 0
        desc.m_nterms, desc.m_xfac, desc.m_yfac = nterms, _lib.as_dp(xfac), _lib.as_dp(yfac)
        assert lib.mgcmt_plan_create_pot(ctypes.byref(desc), _lib.as_dp(pd), ctypes.byref(hh)) == -4
        assert b"point diagonal" in lib.mgcmt_last_error()
        desc.m_nterms = 0
        assert lib.mgcmt_plan_create_pot(ctypes.byref(desc), None, ctypes.byref(hh)) == -1
    finally:
        plan.close()
    from multigridcmt_amd.operators import laplacian_operator
    plain = Plan(laplacian_operator(g, "2d"), 4)          # a plan without a point diagonal has no point stencil
    try:
        assert lib.mgcmt_plan_get_point_stencil(plain._h, 0, out, 8) == -1
    finally:
        plain.close()
    # Python: the lexicographic smoothers raise, naming what is supported, everywhere an operator arrives
    solver, sm = MGCMTSolver(), MGCMTStencilMaker()
    v0, f = np.zeros(g * g), np.ones(g * g)
    A = hamiltonian(g, rough_v(g))
    for bad in (solver.gseidel, solver.sor, functools.partial(solver.sor, omega=1.2)):
        for start in (op, A):
            with pytest.raises(ValueError, match="wjacobi, gseidel_rb"):
                solver.vcycle(v0.copy(), f.copy(), start, sm, smoother=bad, dimension="2d", lowest_level=4)
        with pytest.raises(ValueError, match="wjacobi, gseidel_rb"):
            solver.vcycle_matrix(np.zeros((g * g, 2)), np.ones((g * g, 2)), op, sm, smoother=bad, dimension="2d", lowest_level=4)
        with pytest.raises(ValueError, match="wjacobi, gseidel_rb"):
            solver.fmg(f.copy(), op, sm, smoother=bad, dimension="2d", lowest_level=4)
    with pytest.raises(ValueError, match="wjacobi, gseidel_rb"):
        solver.gseidel(v0.copy(), f.copy(), op)
    with pytest.raises(ValueError, match="wjacobi, gseidel_rb"):
        solver.sor(v0.copy(), f.copy(), op, omega=1.2)
    with pytest.raises(ValueError, match="point diagonal"):
        solver.twogrid(v0.copy(), f.copy(), op, sm, dimension="2d")
    with pytest.raises(ValueError, match="point diagonal"):
        solver.twogrid(v0.copy(), f.copy(), A, sm, dimension="2d")
    with pytest.raises(ValueError, match="point diagonal"):
        solver.rqmin(op, np.ones(g * g), M=sp.identity(g * g, format="csr"))
    # a random matrix that is no 5-point operator is still refused by the 2-D entry points
    bad = sp.random(g * g, g * g, density=0.02, random_state=1, format="csr") + sp.identity(g * g)
    with pytest.raises(UnrecognisedOperator):
        solver.vcycle(v0.copy(), f.copy(), bad, sm, dimension="2d", lowest_level=4)


def test_block_eigensolve_non_separable_well_against_eigsh(backend):
    """The lowest four states of a non-separable well — two overlapping circular dots of different depth — at 64^2,
    against scipy's eigsh on the assembled Hamiltonian (the bar of tests/test_drivers.py)."""
    import scipy.sparse.linalg as sla
    g, k = 64, 4
    x = (np.arange(g) + 0.5) / g
    X, Y = np.meshgrid(x, x, indexing="ij")
    V = 60.0 - 60.0 * ((X - 0.36) ** 2 + (Y - 0.42) ** 2 < 0.2 ** 2) - 45.0 * ((X - 0.68) ** 2 + (Y - 0.60) ** 2 < 0.16 ** 2)
    V = np.maximum(V, 0.0)
    op = potential_operator(g, V)
    with pytest.raises(UnrecognisedOperator):
        recognise(op.tocsr(), "2d")
    vals, vecs = drivers.block_eigensolve(op, k=k, cycles=16, lowest=8)
    want = np.sort(sla.eigsh(op.tocsr(), k=k, sigma=0.0, which="LM")[0])
    assert np.allclose(vals, want, rtol=0, atol=1e-8), np.abs(vals - want)
    assert np.abs(vecs.T @ vecs - np.eye(k)).max() < 1e-10
