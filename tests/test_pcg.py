"""MGCMTSolver.solve — conjugate gradients preconditioned by one V-cycle per iteration, resident on the device
(mgcmt_pcg_begin / mgcmt_pcg_iterate / mgcmt_pcg_status) — against a NumPy restatement of the same iteration whose
preconditioner is the oracle's cycle (oracle.sparse_ref.RefSolver.vcycle), through the HIP library on the GPU box and through
the emulated kernels on the CPU (``backend`` fixture).

Set-up of every case: f = RandomState(1).rand(n), a zero start, V(2,2) on the fine level with the oracle's V(4,4) below,
lowest_level = 4, rtol = 1e-10.  The lowest eigenvalue of (-1/pi^2) laplacian(32, "2d") is 1.879: shifts 1.9 and 3.0 make the
system indefinite, where the plain cycle stalls or crawls and conjugate gradients still converge.

Bounds.  First iterate: 1e-9 relative — the project's single-cycle parity of 1e-10 times the three places a cycle's error
enters x_1 = alpha z (z itself, rho = <z, r> and <p, q> with p = z), with a margin of 3.  Iteration counts: within one of the
reference's (a residual that lands on the tolerance may fall either side of it).  History: the recorded ||r_k|| is the
recurrence's, SciPy's ||f - (A - mu I) x_k|| the true one; they agree to 1e-10 ||f|| over the first five iterations.

The reference iteration counts of the four 2-D rows (wjacobi / red-black; standard beta, and red-black with the flexible beta)
are pinned below as the feature was specified with them; the reference of this file must reproduce them."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import rel_err
from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, _lib, potential_operator, potential_well_operator, variable_mass_operator
from multigridcmt_amd._lib import MgcmtError
from multigridcmt_amd.operators import UnrecognisedOperator, laplacian_operator
from multigridcmt_amd.plan import Plan
from oracle.sparse_ref import RefSolver, RefStencilMaker
from test_3d_cycle import Ref3dSolver, Ref3dStencilMaker, mc_3d
from test_nine_point import tensor_operator

RTOL = 1e-10
SCALE = -1 / np.pi ** 2


@pytest.fixture(autouse=True, scope="module")
def _release_host_buffers():
    """result arrays of this module go back to the page-locked pool and the pool is emptied afterwards"""
    yield
    import gc
    from multigridcmt_amd import hostmem
    gc.collect()
    hostmem.drain()


def disc_mass(g, contrast=1000.0, dimension="2d"):
    """inverse mass `contrast` inside the disc (ball) of radius g / 4 about the grid's centre, 1 outside"""
    x = np.arange(g) + 0.5 - g / 2
    grids = np.meshgrid(*([x] * (2 if dimension == "2d" else 3)), indexing="ij")
    return np.where(sum(c * c for c in grids) < (g / 4) ** 2, contrast, 1.0)


# name -> (dimension, grid, lowest_level, shift, operator)
PROBLEMS = {
    "lap1d": ("1d", 64, 4, 0.0, lambda: laplacian_operator(64, "1d") * SCALE),
    "lap2d_s0": ("2d", 32, 4, 0.0, lambda: laplacian_operator(32, "2d") * SCALE),
    "lap2d_s1.9": ("2d", 32, 4, 1.9, lambda: laplacian_operator(32, "2d") * SCALE),
    "lap2d_s3.0": ("2d", 32, 4, 3.0, lambda: laplacian_operator(32, "2d") * SCALE),
    "vmass2d": ("2d", 32, 4, 0.0, lambda: variable_mass_operator(32, disc_mass(32))),
    "tensor2d": ("2d", 32, 4, 0.0, lambda: tensor_operator(32, "rough")),
    "lap3d": ("3d", 16, 4, 0.0, lambda: laplacian_operator(16, "3d") * SCALE),
    "pot3d": ("3d", 16, 4, 0.0, lambda: potential_operator(16, 5.0 * np.random.RandomState(17).rand(16, 16, 16), dimension="3d")),
}
SMOOTHERS = ["wjacobi", "rb"]
# the specification's table: reference iterations to 1e-10, (wjacobi, red-black) with the standard beta, red-black with the flexible one
PINNED = {"lap2d_s0": ((8, 5), 5), "lap2d_s1.9": ((11, 12), 10), "lap2d_s3.0": ((11, 18), 12), "vmass2d": ((14, 11), 11)}


@functools.lru_cache(maxsize=None)
def problem(name):
    dim, g, lowest, shift, make = PROBLEMS[name]
    op = make()
    A = op.tocsr()
    n = A.shape[0]
    f = np.random.RandomState(1).rand(n)
    shifted = (A - shift * sp.identity(n)).tocsr()
    return dim, g, lowest, shift, op, A, shifted, f


def ref_cycle(name, smoother):
    """r -> one oracle V(2,2) cycle of r from a zero start: the preconditioner"""
    dim, g, lowest, shift, op, A, shifted, f = problem(name)
    n = A.shape[0]
    if dim == "3d":
        ref, rsm = Ref3dSolver(), Ref3dStencilMaker()
        smo = None if smoother == "wjacobi" else mc_3d
    else:
        ref, rsm = RefSolver(), RefStencilMaker()
        smo = None if smoother == "wjacobi" else (lambda v, f, A, nu=4: ref.gseidel_mc(v, f, A, nu=nu, dimension=dim))

    def cycle(r, v0=None):
        v = ref.vcycle(np.zeros(n) if v0 is None else v0.copy(), r.copy(), A, rsm, nu1=2, nu2=2, smoother=smo, shift=shift, lowest_level=lowest,
                       dimension=dim)
        return np.asarray(v, dtype=float).reshape(-1)
    return cycle


def ref_pcg(shifted, f, cycle, rtol, maxiter, flexible, x0=None):
    """the iteration of mgcmt_pcg_iterate in NumPy: (x, [||r_k||], [x_k], indefinite)"""
    x = np.zeros(len(f)) if x0 is None else np.array(x0, dtype=float)
    r = f - shifted @ x
    fnorm = np.linalg.norm(f)
    hist, xs, indefinite = [], [], False
    p = q = None
    alpha = rho_old = 0.0
    for it in range(maxiter):
        z = cycle(r)
        rho = z @ r
        if it == 0:
            p = z.copy()
        else:
            beta = -alpha * (z @ q) / rho_old if flexible else rho / rho_old
            p = z + beta * p
        q = shifted @ p
        pq = p @ q
        indefinite = indefinite or rho < 0 or pq < 0
        alpha = rho / pq
        x = x + alpha * p
        r = r - alpha * q
        rho_old = rho
        hist.append(np.linalg.norm(r))
        xs.append(x.copy())
        if hist[-1] <= rtol * fnorm:
            break
    return x, hist, xs, indefinite


def default_flexible(smoother):
    return smoother != "wjacobi"


@functools.lru_cache(maxsize=None)
def reference(name, smoother, flexible=None):
    """computed once per (problem, smoother, beta form) and shared by the tests; never modified"""
    dim, g, lowest, shift, op, A, shifted, f = problem(name)
    flexible = default_flexible(smoother) if flexible is None else flexible
    return ref_pcg(shifted, f, ref_cycle(name, smoother), RTOL, 60, flexible)


def run(name, smoother, **kw):
    dim, g, lowest, shift, op, A, shifted, f = problem(name)
    solver = MGCMTSolver()
    info = {}
    args = dict(nu1=2, nu2=2, smoother=solver.wjacobi if smoother == "wjacobi" else solver.gseidel_rb, shift=shift, lowest_level=lowest,
                dimension=dim, rtol=RTOL, info=info)
    args.update(kw)
    x = solver.solve(f.copy(), op, MGCMTStencilMaker(), **args)
    return np.array(x), info


CASES = [(n, s) for n in PROBLEMS for s in SMOOTHERS]


@pytest.mark.parametrize("name,smoother", CASES)
def test_first_iterate_against_the_reference(backend, name, smoother):
    x1, info = run(name, smoother, maxiter=1)
    ref_x1 = reference(name, smoother)[2][0]
    err = rel_err(x1, ref_x1)
    print("first iterate %s/%s: rel err %.3e" % (name, smoother, err))
    assert x1.shape == ref_x1.shape and info["iterations"] == 1
    assert err < 1e-9


@pytest.mark.parametrize("name,smoother", CASES)
def test_iteration_counts_and_true_residual(backend, name, smoother):
    """iterations to 1e-10 within one of the reference's, the recomputed residual within twice the tolerance and, on the rows
    of the table, strictly fewer iterations than the plain cycles the same tolerance takes"""
    dim, g, lowest, shift, op, A, shifted, f = problem(name)
    _, hist, _, _ = reference(name, smoother)
    x, info = run(name, smoother, maxiter=60)
    print("%s/%s: iterations %d (reference %d), true residual %.3e" % (name, smoother, info["iterations"], len(hist), info["true_residual"]))
    assert info["status"] == "converged"
    assert abs(info["iterations"] - len(hist)) <= 1
    assert info["true_residual"] <= 2 * RTOL
    assert np.linalg.norm(f - shifted @ x) <= 2 * RTOL * np.linalg.norm(f)
    assert len(info["residuals"]) == info["iterations"] and info["residuals"][-1] <= RTOL
    if name not in PINNED:      # (the rows of the table; the 1-D red-black cycle, for one, is cyclic reduction: exact after one cycle)
        return
    # as many plain cycles as the solve took iterations have not reached the tolerance: the plain cycle needs strictly more
    solver, sm = MGCMTSolver(), MGCMTStencilMaker()
    smo = solver.wjacobi if smoother == "wjacobi" else solver.gseidel_rb
    v = np.zeros(len(f))
    for _ in range(info["iterations"]):
        v = np.array(solver.vcycle(v, f.copy(), op, sm, nu1=2, nu2=2, smoother=smo, shift=shift, lowest_level=lowest, dimension=dim)).reshape(-1)
    plain = np.linalg.norm(f - shifted @ v) / np.linalg.norm(f)
    print("    %d plain cycles: residual %.3e" % (info["iterations"], plain))
    assert not plain <= RTOL


@pytest.mark.parametrize("name", sorted(PINNED))
def test_reference_counts_are_the_pinned_ones(name):
    """the NumPy reference of this file gives the counts the feature was specified with, and fewer than the plain cycle"""
    (wj, rb), rb_flex = PINNED[name]
    assert len(reference(name, "wjacobi", False)[1]) == wj
    assert len(reference(name, "rb", False)[1]) == rb
    assert len(reference(name, "rb", True)[1]) == rb_flex
    assert len(reference(name, "wjacobi", True)[1]) == wj           # a symmetric preconditioner: the two forms agree
    dim, g, lowest, shift, op, A, shifted, f = problem(name)
    for smoother, count in (("wjacobi", wj), ("rb", rb_flex)):
        cycle, v = ref_cycle(name, smoother), np.zeros(len(f))
        for _ in range(count):
            v = cycle(f, v)
        assert np.linalg.norm(f - shifted @ v) > RTOL * np.linalg.norm(f)


@pytest.mark.parametrize("name,smoother", [("lap2d_s0", "rb"), ("lap2d_s1.9", "rb"), ("lap2d_s3.0", "rb"), ("vmass2d", "rb")])
def test_standard_beta_with_the_red_black_cycle(backend, name, smoother):
    """flexible=False on the preconditioner that is not symmetric: the counts of the reference's standard form"""
    _, hist, _, _ = reference(name, smoother, False)
    _, info = run(name, smoother, maxiter=60, flexible=False)
    assert info["status"] == "converged" and abs(info["iterations"] - len(hist)) <= 1


@pytest.mark.parametrize("name,smoother", [("lap1d", "wjacobi"), ("lap2d_s1.9", "wjacobi"), ("lap2d_s1.9", "rb"), ("vmass2d", "rb"), ("tensor2d", "wjacobi"),
                                           ("pot3d", "rb")])
def test_history_is_the_true_residual(backend, name, smoother):
    dim, g, lowest, shift, op, A, shifted, f = problem(name)
    fnorm = np.linalg.norm(f)
    for k in range(1, 6):
        xk, info = run(name, smoother, maxiter=k)
        assert info["iterations"] == k and info["status"] == "maxiter" and len(info["residuals"]) == k
        true = np.linalg.norm(f - shifted @ xk)
        diff = abs(info["residuals"][-1] * fnorm - true)
        print("%s/%s k=%d: recorded %.6e true %.6e" % (name, smoother, k, info["residuals"][-1] * fnorm, true))
        assert diff <= 1e-10 * fnorm
        assert abs(info["true_residual"] * fnorm - true) <= 1e-12 * fnorm


@pytest.mark.parametrize("name,smoother", [("lap2d_s1.9", "wjacobi"), ("vmass2d", "rb"), ("lap3d", "rb"), ("lap1d", "wjacobi")])
def test_queued_iterations_behind_convergence_change_nothing(backend, name, smoother):
    """check_every = 1 stops at the converged iteration; check_every = 8 has up to seven more queued behind it: the same bits"""
    a, ia = run(name, smoother, maxiter=64, check_every=1)
    b, ib = run(name, smoother, maxiter=64, check_every=8)
    assert ia["status"] == ib["status"] == "converged"
    assert ia["iterations"] == ib["iterations"] and ia["iterations"] % 8 != 0
    assert np.array_equal(a, b)
    assert np.array_equal(ia["residuals"], ib["residuals"])


@pytest.mark.parametrize("name,smoother", [("lap2d_s3.0", "rb"), ("tensor2d", "wjacobi"), ("pot3d", "wjacobi")])
def test_two_runs_are_bit_identical(backend, name, smoother):
    a, ia = run(name, smoother, maxiter=60)
    b, ib = run(name, smoother, maxiter=60)
    assert np.array_equal(a, b) and np.array_equal(ia["residuals"], ib["residuals"]) and ia["iterations"] == ib["iterations"]


@pytest.mark.parametrize("smoother", SMOOTHERS)
def test_indefinite_bit(backend, smoother):
    assert run("lap2d_s1.9", smoother, maxiter=60)[1]["indefinite"] is True
    assert reference("lap2d_s1.9", smoother)[3]
    assert run("lap2d_s0", smoother, maxiter=60)[1]["indefinite"] is False
    assert not reference("lap2d_s0", smoother)[3]


@pytest.mark.parametrize("name,smoother", [("lap2d_s1.9", "wjacobi"), ("vmass2d", "rb"), ("lap3d", "wjacobi")])
def test_start_vector(backend, name, smoother):
    dim, g, lowest, shift, op, A, shifted, f = problem(name)
    v0 = np.random.RandomState(5).rand(len(f))
    x, info = run(name, smoother, maxiter=60, v0=v0)
    x_zero, info_zero = run(name, smoother, maxiter=60)
    assert info["status"] == "converged" and info["true_residual"] <= 2 * RTOL and info_zero["true_residual"] <= 2 * RTOL
    # the first iterate from v0 is the reference's (the residual f - (A - mu I) v0 is formed on the device)
    x1, _ = run(name, smoother, maxiter=1, v0=v0)
    ref_x1 = ref_pcg(shifted, f, ref_cycle(name, smoother), RTOL, 1, default_flexible(smoother), x0=v0)[2][0]
    assert rel_err(x1, ref_x1) < 1e-9
    # a start vector that solves the system: converged before the first iteration
    x_again, info_again = run(name, smoother, maxiter=60, v0=x, rtol=1e-9)
    assert info_again["iterations"] == 0 and info_again["status"] == "converged" and np.array_equal(x_again, x)


def test_zero_right_hand_side_and_maxiter_zero(backend):
    dim, g, lowest, shift, op, A, shifted, f = problem("lap2d_s0")
    solver = MGCMTSolver()
    info = {}
    x = solver.solve(np.zeros(len(f)), op, MGCMTStencilMaker(), lowest_level=4, dimension="2d", info=info)
    assert not np.any(x) and info["iterations"] == 0 and info["status"] == "converged"
    x = solver.solve(f.copy(), op, MGCMTStencilMaker(), lowest_level=4, dimension="2d", maxiter=0, info=info)
    assert not np.any(x) and info["iterations"] == 0 and info["status"] == "maxiter" and info["true_residual"] == 1.0


def test_sparse_matrix_entry_and_root_module(backend):
    """the scipy.sparse matrix goes through the recognition path of vcycle; the root module re-exports the class"""
    import MGCMTSolver as root
    dim, g, lowest, shift, op, A, shifted, f = problem("vmass2d")
    a = np.array(root.MGCMTSolver().solve(f.copy(), A, MGCMTStencilMaker(), lowest_level=4, dimension="2d", rtol=RTOL))
    b, _ = run("vmass2d", "wjacobi")
    assert np.array_equal(a, b)


def _plan_with_f(nvec):
    p = Plan(laplacian_operator(32, "2d") * SCALE, 4, nvec=nvec)
    p.set_shifts([0.0])
    p.upload(0, _lib.SLOT_F, 0, np.random.RandomState(1).rand(32 * 32))
    return p


def test_refusals(backend):
    lib = _lib.lib()
    p = _plan_with_f(3)
    with pytest.raises(MgcmtError, match="mgcmt error -1"):
        p.pcg_begin([0, 1, 2, 3], 1e-8, zero_start=True)
    with pytest.raises(MgcmtError, match="mgcmt error -1"):
        p.pcg_iterate(1, 2, 2, _lib.WJACOBI)
    p.close()
    p = _plan_with_f(4)
    for vecs in ([0, 1, 2, 2], [0, 0, 1, 2], [3, 1, 2, 3], [0, 1, 2, 4], [0, 1, 2, -1]):
        with pytest.raises(MgcmtError, match="mgcmt error -1"):
            p.pcg_begin(vecs, 1e-8, zero_start=True)
    with pytest.raises(MgcmtError, match="mgcmt error -1"):          # no begin yet
        p.pcg_iterate(1, 2, 2, _lib.WJACOBI)
    with pytest.raises(MgcmtError, match="mgcmt error -1"):
        p.pcg_status()
    with pytest.raises(MgcmtError, match="mgcmt error -1"):          # an unknown flag
        _lib.check(lib.mgcmt_pcg_begin(p._h, (_lib.c_int * 4)(0, 1, 2, 3), 1e-8, 4, None))
    with pytest.raises(MgcmtError, match="mgcmt error -1"):
        p.pcg_begin([0, 1, 2, 3], -1.0, zero_start=True)
    p.pcg_begin([0, 1, 2, 3], 1e-8, zero_start=True)
    with pytest.raises(MgcmtError, match="mgcmt error -1"):
        p.pcg_iterate(-1, 2, 2, _lib.WJACOBI)
    p.pcg_iterate(2, 2, 2, _lib.WJACOBI, omega=2 / 3)
    assert p.pcg_status()[0] == 2
    p.close()
    # a lexicographic smoother on a plan with a per-point part: the cycle's refusal, through the library and through the class
    p = Plan(variable_mass_operator(32, disc_mass(32)), 4, nvec=4)
    p.set_shifts([0.0])
    p.upload(0, _lib.SLOT_F, 0, np.ones(32 * 32))
    p.pcg_begin([0, 1, 2, 3], 1e-8, zero_start=True)
    with pytest.raises(MgcmtError, match="mgcmt error -4"):
        p.pcg_iterate(1, 2, 2, _lib.GS_LEX)
    p.close()
    solver, sm = MGCMTSolver(), MGCMTStencilMaker()
    dim, g, lowest, shift, op, A, shifted, f = problem("vmass2d")
    with pytest.raises(ValueError, match="lexicographic"):
        solver.solve(f.copy(), op, sm, smoother=solver.gseidel, lowest_level=4, dimension="2d")
    with pytest.raises(ValueError, match="lexicographic"):
        solver.solve(np.ones(16 ** 3), laplacian_operator(16, "3d"), sm, smoother=solver.sor, lowest_level=4, dimension="3d")
    with pytest.raises(NotImplementedError):
        solver.solve(f.copy(), op, sm, smoother=lambda v, f, A, nu=4: v, lowest_level=4, dimension="2d")
    # a 1-D operator that only the general sparse path handles
    n = 64
    general = sp.random(n, n, density=0.2, random_state=3, format="csr") + 10 * sp.identity(n)
    with pytest.raises(UnrecognisedOperator):
        solver.solve(np.ones(n), general, sm, lowest_level=4)
    with pytest.raises(ValueError):
        solver.solve(f.copy(), op, sm, lowest_level=4, dimension="2d", check_every=0)
    with pytest.raises(ValueError):
        solver.solve(f.copy(), op, sm, lowest_level=4, dimension="2d", maxiter=_lib.RQ_HISTORY + 1)


def test_lexicographic_smoother_on_a_kronecker_plan(backend):
    """where the plan's cycle accepts a lexicographic smoother the solve runs with it (the flexible beta: Gauss-Seidel in index
    order is not symmetric)"""
    dim, g, lowest, shift, op, A, shifted, f = problem("lap2d_s0")
    solver = MGCMTSolver()
    info = {}
    x = solver.solve(f.copy(), op, MGCMTStencilMaker(), smoother=solver.gseidel, lowest_level=4, dimension="2d", rtol=RTOL, info=info)
    assert info["status"] == "converged" and info["true_residual"] <= 2 * RTOL
    assert np.linalg.norm(f - shifted @ np.array(x)) <= 2 * RTOL * np.linalg.norm(f)


# ---- the marching direction pass (MGCMT_OPT_PCG_MARCH): direction, application and <p, q> in one launch ---------------------------
# 32^2 is one row chunk, 64^2 two and 128^2 four (chunks of 32 rows whose overlap rows are recomputed); a thread owns two columns,
# so 32^2 and 64^2 leave lanes of the one wave idle and 128^2 fills it; the well adds the product potential's factors.

MARCH_OPS = {"lap": lambda g: laplacian_operator(g, "2d") * SCALE, "well": lambda g: potential_well_operator(g, 20.0, (g // 4, 3 * g // 4))}
X, P, Q, P2 = 0, 1, 2, 3


def _march_plan(opname, g, shift, march):
    p = Plan(MARCH_OPS[opname](g), 4, nvec=4)
    p.set_option(_lib.OPT_PCG_MARCH, march)
    p.set_shifts([shift])
    p.upload(0, _lib.SLOT_F, 0, np.random.RandomState(1).rand(g * g))
    p.pcg_begin([X, P, Q, P2], 0.0, zero_start=True, flexible=False)
    return p


def _w(p, col):
    return np.array(p.download(0, _lib.SLOT_W, col))


def check_marching_against_generic(g, opname, shift, steps=(1, 2, 3)):
    """Iteration k as the generic passes and as the march, from the same state (k - 1 generic iterations, which are
    bit-reproducible): the new direction and (A - mu I) p carry the same bits — the expressions are the generic passes' term by
    term —, alpha agrees to 1e-12 (the partial sums of <p, q> are added in another order); then five marched iterations against
    five generic ones: x to 1e-10."""
    wj = dict(kind=_lib.WJACOBI, omega=2.0 / 3.0)
    for k in steps:
        a, b = _march_plan(opname, g, shift, 0), _march_plan(opname, g, shift, 0)
        a.pcg_iterate(k - 1, 2, 2, **wj)
        b.pcg_iterate(k - 1, 2, 2, **wj)
        x_before = _w(a, X)
        assert np.array_equal(x_before, _w(b, X))
        b.set_option(_lib.OPT_PCG_MARCH, 1)
        a.pcg_iterate(1, 2, 2, **wj)
        b.pcg_iterate(1, 2, 2, **wj)
        pa, pb = _w(a, P), _w(b, P2)                      # the march writes the new direction to the spare vector
        assert np.any(pa) and np.array_equal(pa, pb), k
        assert np.array_equal(_w(a, Q), _w(b, Q)), k
        alpha_a = (_w(a, X) - x_before) @ pa / (pa @ pa)
        alpha_b = (_w(b, X) - x_before) @ pb / (pb @ pb)
        print("g=%d %s shift=%g k=%d: alpha %.17g / %.17g" % (g, opname, shift, k, alpha_a, alpha_b))
        assert abs(alpha_a - alpha_b) <= 1e-12 * abs(alpha_a)
        assert a.pcg_status()[0] == b.pcg_status()[0] == k
        a.close()
        b.close()
    a, b = _march_plan(opname, g, shift, 0), _march_plan(opname, g, shift, 1)
    a.pcg_iterate(5, 2, 2, **wj)
    b.pcg_iterate(5, 2, 2, **wj)
    ha, hb = a.pcg_status(history=5)[4], b.pcg_status(history=5)[4]
    assert rel_err(_w(b, X), _w(a, X)) < 1e-10
    assert np.allclose(ha, hb, rtol=1e-8, atol=0)
    assert rel_err(_w(b, P2), _w(a, P)) < 1e-8            # an odd number of iterations: the direction is in p2
    a.close()
    b.close()


@pytest.mark.parametrize("shift", [0.0, 1.9])
@pytest.mark.parametrize("opname", sorted(MARCH_OPS))
@pytest.mark.parametrize("g", [32, 64, 128])
def test_marching_direction_pass(backend, g, opname, shift):
    check_marching_against_generic(g, opname, shift)


def test_marching_switch_through_the_environment(backend, monkeypatch):
    """MGCMT_PCG_MARCH selects the pass where the plan's option was not set; a level the march does not cover (a per-point
    operator, a 3-D grid) takes the generic passes whatever the switch says"""
    outs = {}
    for march in ("0", "1"):
        monkeypatch.setenv("MGCMT_PCG_MARCH", march)
        from multigridcmt_amd import plan
        plan.release_plans()
        outs[march] = [run(name, "wjacobi", maxiter=60) for name in ("lap2d_s1.9", "vmass2d", "lap3d")]
    monkeypatch.delenv("MGCMT_PCG_MARCH")
    for (xa, ia), (xb, ib), covered in zip(outs["0"], outs["1"], (True, False, False)):
        assert ia["iterations"] == ib["iterations"] and ib["status"] == "converged" and ib["true_residual"] <= 2 * RTOL
        if covered:
            assert rel_err(xb, xa) < 1e-9            # (the other order of the partial sums may show in the last bits)
        else:
            assert np.array_equal(xa, xb)
