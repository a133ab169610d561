"""3-D V-cycle against the NumPy oracle (oracle.sparse_ref.RefSolver on kron-built 3-D matrices), through the HIP
library on the GPU box and through the emulated kernels on CPU (``backend`` fixture)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import rel_err
from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, _lib
from multigridcmt_amd.operators import laplacian_operator, recognise
from multigridcmt_amd.plan import get_plan
from oracle.sparse_ref import RefSolver, RefStencilMaker

TOL = 1e-10


@pytest.fixture(autouse=True, scope="module")
def _release_host_buffers():
    """result arrays of this module go back to the page-locked pool and the pool is emptied afterwards"""
    yield
    import gc
    from multigridcmt_amd import hostmem
    gc.collect()
    hostmem.drain()


class Ref3dStencilMaker:
    """3-D transfers as krons of the oracle's 1-D matrices (restriction: (1/8) P^T, the 2-D formula's fixed factor)."""

    def __init__(self):
        self.one = RefStencilMaker()

    def laplacian(self, n, dimension="3d"):
        L = self.one.laplacian(n, dimension="1d")
        return sp.kronsum(sp.kronsum(L, L), L).tocsr()

    def interpolation(self, old, new, dimension="3d"):
        s = self.one.interpolation(old, new, dimension="1d")
        return sp.kron(s, sp.kron(s, s), format="csc")

    def restriction(self, old, new, dimension="3d"):
        return (0.125 * self.interpolation(new, old).T).tocsr()


class Ref3dSolver(RefSolver):
    def _grid(self, n, dimension):
        if dimension == "3d":
            g = int(round(n ** (1.0 / 3.0)))
            return g if g ** 3 == n else n ** (1.0 / 3.0)
        return super()._grid(n, dimension)


def colour_classes_3d(n):
    """(z%2, y%2, x%2) in the order (0,0,1), (0,1,0), (1,0,0), (1,1,1), (0,0,0), (0,1,1), (1,0,1), (1,1,0)."""
    g = int(round(n ** (1.0 / 3.0)))
    idx = np.arange(n)
    z, y, x = idx // (g * g), (idx // g) % g, idx % g
    order = ((0, 0, 1), (0, 1, 0), (1, 0, 0), (1, 1, 1), (0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0))
    return [idx[(z % 2 == a) & (y % 2 == b) & (x % 2 == c)] for a, b, c in order]


def mc_3d(v0, f, A, nu=4, omega=1.0):
    """the oracle's multicolour Gauss-Seidel (RefSolver.gseidel_mc) with the 3-D colour classes"""
    v = np.asarray(v0, dtype=float).reshape(-1).copy()
    f = np.asarray(f, dtype=float).reshape(-1)
    A = sp.csr_matrix(A)
    d = A.diagonal()
    for _ in range(nu):
        for c in colour_classes_3d(len(v)):
            r = f[c] - A[c, :] @ v
            v[c] = v[c] + omega * r / d[c]
    return v


def _problem(g, seed=0):
    A = (-1 / np.pi ** 2) * MGCMTStencilMaker().laplacian(g, dimension="3d")
    f = np.random.RandomState(seed).rand(g ** 3)
    return A, f


CASES = [(8, 2), (8, 4), (16, 4), (16, 8), (32, 8), (64, 8)]   # 64^3: the marching kernels of the 7-point fine level


@pytest.mark.parametrize("g,lowest", CASES)
@pytest.mark.parametrize("shift", [0.0, 1.9])
@pytest.mark.parametrize("smoother", ["wjacobi", "gseidel_rb"])
def test_vcycle_3d_vs_oracle(backend, g, lowest, shift, smoother):
    A, f = _problem(g)
    solver, ref = MGCMTSolver(), Ref3dSolver()
    n = g ** 3
    if smoother == "wjacobi":
        ours, theirs = None, None
    else:
        ours, theirs = solver.gseidel_rb, mc_3d
    x = solver.vcycle(np.zeros(n), f.copy(), A, MGCMTStencilMaker(), nu1=2, nu2=2, smoother=ours, shift=shift, lowest_level=lowest,
                      dimension="3d")
    y = ref.vcycle(np.zeros(n), f.copy(), A, Ref3dStencilMaker(), nu1=2, nu2=2, smoother=theirs, shift=shift, lowest_level=lowest,
                   dimension="3d")
    assert x.shape == (n,)
    assert rel_err(x, y) < TOL


def test_vcycle_3d_nonzero_start_and_repeat(backend):
    # a non-zero start vector, and the same call twice (the second replays the captured cycle)
    g = 16
    A, f = _problem(g, seed=1)
    v0 = np.random.RandomState(2).rand(g ** 3)
    solver, ref = MGCMTSolver(), Ref3dSolver()
    y = ref.vcycle(v0.copy(), f.copy(), A, Ref3dStencilMaker(), nu1=2, nu2=2, shift=0.7, lowest_level=4, dimension="3d")
    for _ in range(2):
        x = solver.vcycle(v0.copy(), f.copy(), A, MGCMTStencilMaker(), nu1=2, nu2=2, shift=0.7, lowest_level=4, dimension="3d")
        assert rel_err(x, y) < TOL


def test_vcycle_3d_on_lowest_level_returns_column(backend):
    A, f = _problem(4)
    x = MGCMTSolver().vcycle(np.zeros(64), f.copy(), A, MGCMTStencilMaker(), shift=0.3, lowest_level=4, dimension="3d")
    y = np.linalg.solve(A.toarray() - 0.3 * np.eye(64), f)
    assert x.shape == (64, 1)
    assert rel_err(x.reshape(-1), y) < TOL


def test_vcycle_matrix_3d(backend):
    g, k = 16, 3
    A, _ = _problem(g)
    n = g ** 3
    F = np.random.RandomState(5).rand(n, k)
    shifts = np.array([0.0, 1.1, 2.3])
    x = MGCMTSolver().vcycle_matrix(np.zeros((n, k)), F.copy(), A, MGCMTStencilMaker(), nu1=2, nu2=2, shifts=shifts, lowest_level=4,
                                    dimension="3d")
    y = Ref3dSolver().vcycle_matrix(np.zeros((n, k)), F.copy(), A, Ref3dStencilMaker(), nu1=2, nu2=2, shifts=shifts, lowest_level=4,
                                    dimension="3d")
    assert x.shape == (n, k)
    assert rel_err(x, y) < TOL


def test_foreign_smoother_3d(backend):
    g = 8
    A, f = _problem(g, seed=7)
    calls = []

    def smoother(v0, f, A, nu=4):
        calls.append(A.shape[0])
        return RefSolver().wjacobi(v0, f, A, nu=nu, omega=0.6)

    x = MGCMTSolver().vcycle(np.zeros(g ** 3), f.copy(), A, MGCMTStencilMaker(), nu1=2, nu2=2, smoother=smoother, shift=0.4, lowest_level=2,
                             dimension="3d")
    y = Ref3dSolver().vcycle(np.zeros(g ** 3), f.copy(), A, Ref3dStencilMaker(), nu1=2, nu2=2, smoother=functools.partial(RefSolver().wjacobi, omega=0.6),
                             shift=0.4, lowest_level=2, dimension="3d")
    assert {512, 64} <= set(calls)
    assert rel_err(x, y) < TOL


def test_smoothers_3d(backend):
    g = 16
    A, f = _problem(g, seed=8)
    v0 = np.random.RandomState(9).rand(g ** 3)
    solver = MGCMTSolver()
    x = solver.wjacobi(v0.copy(), f.copy(), A, nu=3)
    y = RefSolver().wjacobi(v0, f, A, nu=3)
    assert rel_err(x.reshape(-1), y) < TOL
    x = solver.gseidel_rb(v0.copy(), f.copy(), A, nu=2, dimension="3d")
    assert rel_err(x.reshape(-1), mc_3d(v0, f, A, nu=2)) < TOL


def test_apply_3d_32(backend):
    g = 32
    op = (-1 / np.pi ** 2) * laplacian_operator(g, "3d")
    x = np.random.RandomState(11).rand(g ** 3)
    A = (-1 / np.pi ** 2) * MGCMTStencilMaker().laplacian(g, dimension="3d")
    assert rel_err(op.dot(x), A @ x) < 1e-13
    # a Galerkin level (27-point, the general three-term path) against its assembled matrix
    plan = get_plan(recognise(A, "3d"), 4, nvec=1)
    mat = MGCMTSolver()._level_matrix(plan, 1, 0.0)
    xc = x[: 16 ** 3]
    plan.upload(1, _lib.SLOT_V, 0, xc)
    plan.apply(1, (_lib.SLOT_V, 0), (_lib.SLOT_T, 0))
    assert rel_err(plan.download(1, _lib.SLOT_T, 0), mat @ xc) < 1e-13


def test_lexicographic_smoother_raises_3d(backend):
    A, f = _problem(8)
    solver = MGCMTSolver()
    for sm in (solver.gseidel, solver.sor):
        with pytest.raises(ValueError, match="wjacobi"):
            solver.vcycle(np.zeros(512), f.copy(), A, MGCMTStencilMaker(), smoother=sm, lowest_level=2, dimension="3d")
    with pytest.raises(ValueError, match="gseidel_rb"):
        solver.smooth(np.zeros(512), f.copy(), A, smoother=solver.gseidel, dimension="3d")


def test_non_cube_length_returns_none(backend, capsys):
    A, f = _problem(8)
    assert MGCMTSolver().vcycle(np.zeros(500), np.ones(500), A, MGCMTStencilMaker(), dimension="3d") is None
    assert MGCMTSolver().vcycle(np.zeros(27), np.ones(27), A, MGCMTStencilMaker(), dimension="3d") is None   # 3^3
    assert "power of 2" in capsys.readouterr().out


def test_lowest_level_32_raises(backend):
    A, f = _problem(32)
    with pytest.raises(ValueError):
        MGCMTSolver().vcycle(np.zeros(32 ** 3), f, A, MGCMTStencilMaker(), lowest_level=32, dimension="3d")


def test_out_of_scope_entries_unsupported_on_3d_plan(backend):
    plan = get_plan(laplacian_operator(8, "3d"), 2, nvec=2)
    h, L = plan._h, _lib.lib()
    U = -4  # MGCMT_ERR_UNSUPPORTED
    vecs = (ctypes.c_int * 6)(0, 1, 0, 1, 0, 1)
    pair = (ctypes.c_int * 2)(0, 0)
    dbl = ctypes.c_double(0.0)
    i = ctypes.c_int(0)
    out = np.zeros(8)
    dp = _lib.as_dp(out)
    calls = {
        "twogrid": lambda: L.mgcmt_twogrid(h, 0, 2, 2, _lib.WJACOBI, ctypes.c_double(1.0), 1, None),
        "rayleigh_residual": lambda: L.mgcmt_rayleigh_residual(h, 0, 0, 1, dp, dp, None),
        "ritz_pair": lambda: L.mgcmt_ritz_pair(h, 0, 0, 0, 1, 0, 2, 0, dp, None),
        "rqmin": lambda: L.mgcmt_rqmin(h, 0, 0, vecs, 2, 0, ctypes.byref(dbl), None),
        "rq_line_step": lambda: L.mgcmt_rq_line_step(h, 0, pair, None, pair, pair, None, 0, -1, None),
        "rq_history": lambda: L.mgcmt_rq_history(h, 0, 1, dp, None),
        "vcycle_rqmg": lambda: L.mgcmt_vcycle_rqmg(h, 0, vecs, 2, 2, 0, ctypes.byref(dbl), None),
        "fused_pass": lambda: L.mgcmt_fused_pass(h, 0, _lib.WJACOBI, 1, ctypes.c_double(1.0), 0, 1, None),
        "fused_max_sweeps": lambda: L.mgcmt_fused_max_sweeps(h, 0, _lib.WJACOBI, ctypes.byref(i)),
        "fused_max_recompute": lambda: L.mgcmt_fused_max_recompute(h, 0, _lib.WJACOBI, 2, ctypes.byref(i)),
        "level_operator_kind": lambda: L.mgcmt_level_operator_kind(h, 0, ctypes.byref(i)),
        "time_smoother": lambda: L.mgcmt_time_smoother(h, 0, _lib.WJACOBI, 1, ctypes.c_double(1.0), 1, ctypes.byref(dbl), None),
        "time_fused_pass": lambda: L.mgcmt_time_fused_pass(h, 0, _lib.WJACOBI, 1, ctypes.c_double(1.0), 0, 1, ctypes.byref(dbl), None),
        "bandwidth_probe": lambda: L.mgcmt_bandwidth_probe(h, 0, 0, 1, 1, ctypes.byref(dbl), None),
        "comm_init_external": lambda: L.mgcmt_comm_init_external(h, 0, 1, _lib.P2P_FN(0), _lib.ALLGATHER_FN(0), _lib.ALLREDUCE_FN(0), None),
        "comm_set_option": lambda: L.mgcmt_comm_set_option(h, 0, 1),
        "halo_exchange": lambda: L.mgcmt_halo_exchange(h, 0, 1, None),
        "allreduce_sum": lambda: L.mgcmt_allreduce_sum(h, dp, 1, None),
        "sharded_vcycle": lambda: L.mgcmt_sharded_vcycle(h, h, 2, 2, 2, _lib.WJACOBI, ctypes.c_double(1.0), 1, 0, None),
        "gather_coarse": lambda: L.mgcmt_gather_coarse(h, 0, 0, h, 0, 1, None),
        "smooth_lex": lambda: L.mgcmt_smooth(h, 0, _lib.GS_LEX, 1, ctypes.c_double(1.0), 1, None),
        "smooth_sor": lambda: L.mgcmt_smooth(h, 0, _lib.SOR_LEX, 1, ctypes.c_double(1.5), 1, None),
        "vcycle_lex": lambda: L.mgcmt_vcycle(h, 0, 2, 2, 2, _lib.GS_LEX, ctypes.c_double(1.0), 1, 0, None),
    }
    for name, call in calls.items():
        assert call() == U, name
        assert b"3-D" in L.mgcmt_last_error(), name
    unique = ctypes.create_string_buffer(_lib.UNIQUE_ID_BYTES)
    assert L.mgcmt_comm_init(h, 0, 1, unique) == U
    # a 3-D plan has no mass operator and no 2-D answer on its storage: the apply of M is refused too
    assert L.mgcmt_apply(h, _lib.OP_M, 0, 0, 0, 2, 0, 0, None) != 0
    assert math.isfinite(dbl.value)
