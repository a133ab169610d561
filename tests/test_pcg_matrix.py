"""MGCMTSolver.solve_matrix — k systems (A - mu_c I) x_c = f_c in one device-resident conjugate-gradient solve
(mgcmt_pcg_begin_k / mgcmt_pcg_iterate_k / mgcmt_pcg_status_k) — through the HIP library on the GPU box and through the emulated
kernels on the CPU (``backend`` fixture).  The problems, the NumPy iteration and its oracle cycle are tests/test_pcg.py's.

The main assertion is equality of bits: per column the kernels run the workgroups of the single solve in the single solve's
order, and a k-column cycle without Gram-Schmidt gives each column the bits of its own k = 1 cycle, so column c of a batched
solve is ``solve`` run alone on (f_c, mu_c) — iterate, recorded residuals and iteration count.  The red-black rows (flexible
beta) converge after 5 / 10 / 12 iterations at the shifts 0 / 1.9 / 3.0: three columns that freeze at three different iterations.

Bounds that are not equalities are test_pcg.py's: 1e-9 on the first iterate against the oracle-preconditioned reference, 1e-10
on x after five marched iterations against five generic ones."""
import ctypes

import numpy as np
import pytest

from conftest import rel_err
from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, _lib
from multigridcmt_amd._lib import MgcmtError
from multigridcmt_amd.operators import laplacian_operator
from multigridcmt_amd.plan import Plan
from test_pcg import MARCH_OPS, PINNED, PROBLEMS, RTOL, SCALE, problem, ref_pcg, reference  # noqa: F401 (ref_pcg: behind reference)

# the 1-D Laplacian of test_pcg.py at a second shift: a row of its table, so that its helpers serve it unchanged
PROBLEMS.setdefault("lap1d_s0.5", PROBLEMS["lap1d"][:3] + (0.5,) + PROBLEMS["lap1d"][4:])

SHIFTS = (0.0, 1.9, 3.0)
NAMES = ("lap2d_s0", "lap2d_s1.9", "lap2d_s3.0")


@pytest.fixture(autouse=True, scope="module")
def _release_host_buffers():
    yield
    import gc
    from multigridcmt_amd import hostmem
    gc.collect()
    hostmem.drain()


def _smoother(solver, name):
    return solver.wjacobi if name == "wjacobi" else solver.gseidel_rb


def run_matrix(op, F, shifts, smoother, dimension="2d", lowest=4, **kw):
    solver = MGCMTSolver()
    info = {}
    args = dict(nu1=2, nu2=2, smoother=_smoother(solver, smoother), shifts=shifts, lowest_level=lowest, dimension=dimension, rtol=RTOL, info=info)
    args.update(kw)
    x = solver.solve_matrix(np.array(F), op, MGCMTStencilMaker(), **args)
    return np.array(x), info


def run_alone(op, f, shift, smoother, dimension="2d", lowest=4, **kw):
    solver = MGCMTSolver()
    info = {}
    args = dict(nu1=2, nu2=2, smoother=_smoother(solver, smoother), shift=shift, lowest_level=lowest, dimension=dimension, rtol=RTOL, info=info)
    args.update(kw)
    x = solver.solve(np.array(f), op, MGCMTStencilMaker(), **args)
    return np.array(x), info


def assert_columns_are_the_single_solves(op, F, shifts, smoother, X, info, **kw):
    for c, shift in enumerate(shifts):
        v0 = kw.get("v0_matrix")
        extra = {} if v0 is None else {"v0": v0[:, c]}
        xc, ic = run_alone(op, F[:, c], shift, smoother, **{k: v for k, v in kw.items() if k != "v0_matrix"}, **extra)
        print("column %d (shift %g, %s): %d iterations, alone %d; max |dx| %.3e" % (c, shift, smoother, info["iterations"][c], ic["iterations"],
                                                                                   np.max(np.abs(X[:, c] - xc))))
        assert info["iterations"][c] == ic["iterations"] and info["status"][c] == ic["status"] and info["indefinite"][c] == ic["indefinite"]
        assert np.array_equal(X[:, c], xc), c
        assert np.array_equal(info["residuals"][c], ic["residuals"]), c
        assert info["true_residual"][c] <= 2 * kw.get("rtol", RTOL)


# ---- 1. a column against solve ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("smoother", ["wjacobi", "rb"])
@pytest.mark.parametrize("rhs", ["same", "different"])
def test_column_is_the_single_solve(backend, smoother, rhs):
    """wjacobi: the standard beta; red-black: the flexible one.  Counts: those of solve, which test_pcg.py holds within one of the
    pinned 8 / 11 / 11 and 5 / 10 / 12"""
    dim, g, lowest, _, op, A, _, f = problem("lap2d_s0")
    n = len(f)
    F = np.repeat(f[:, None], 3, axis=1) if rhs == "same" else np.random.RandomState(1).rand(n, 3)
    X, info = run_matrix(op, F, SHIFTS, smoother, maxiter=60)
    assert X.shape == (n, 3) and info["status"] == ["converged"] * 3
    assert_columns_are_the_single_solves(op, F, SHIFTS, smoother, X, info, maxiter=60)
    if rhs == "same":
        pinned = [PINNED[name][0][0] if smoother == "wjacobi" else PINNED[name][1] for name in NAMES]
        assert all(abs(a - b) <= 1 for a, b in zip(info["iterations"], pinned)), (info["iterations"], pinned)
        if smoother == "rb":
            assert len(set(info["iterations"])) == 3          # three columns that freeze at three different iterations


# ---- 2. the first iterate against the oracle-preconditioned reference --------------------------------------------------------

@pytest.mark.parametrize("names,smoother", [(("lap1d", "lap1d_s0.5"), "wjacobi"), (("vmass2d", "vmass2d"), "wjacobi"), (("vmass2d", "vmass2d"), "rb"),
                                            (("pot3d", "pot3d"), "wjacobi"), (("pot3d", "pot3d"), "rb")])
def test_first_iterate_against_the_reference(backend, names, smoother):
    dim, g, lowest, _, op, A, _, f = problem(names[0])
    shifts = [problem(name)[3] for name in names]
    X, info = run_matrix(op, np.repeat(f[:, None], len(names), axis=1), shifts, smoother, dimension=dim, lowest=lowest, maxiter=1)
    assert info["iterations"] == [1] * len(names)
    for c, name in enumerate(names):
        ref_x1 = reference(name, smoother)[2][0]
        err = rel_err(X[:, c], ref_x1)
        print("first iterate %s/%s column %d: rel err %.3e" % (name, smoother, c, err))
        assert err < 1e-9


# ---- 3. freezing -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("smoother", ["wjacobi", "rb"])
def test_check_every_and_a_zero_column(backend, smoother):
    """the iterations queued behind a column's convergence change nothing in it; a column with f = 0 stops in the begin"""
    dim, g, lowest, _, op, A, _, f = problem("lap2d_s0")
    F = np.stack([f, np.zeros(len(f)), f, f], axis=1)
    shifts = (0.0, 1.9, 1.9, 3.0)
    a, ia = run_matrix(op, F, shifts, smoother, maxiter=64, check_every=1)
    b, ib = run_matrix(op, F, shifts, smoother, maxiter=64, check_every=8)
    assert np.array_equal(a, b) and ia["iterations"] == ib["iterations"] and ia["status"] == ib["status"] == ["converged"] * 4
    for ra, rb in zip(ia["residuals"], ib["residuals"]):
        assert np.array_equal(ra, rb)
    assert ia["iterations"][1] == 0 and not np.any(a[:, 1]) and len(ia["residuals"][1]) == 0
    assert max(ia["iterations"]) % 8 != 0                    # (iterations were queued behind the last convergence)
    for c in (0, 2, 3):
        xc, ic = run_alone(op, f, shifts[c], smoother, maxiter=64)
        assert np.array_equal(a[:, c], xc) and ia["iterations"][c] == ic["iterations"]


def _plan_k(op, n, k, shifts, F, nvec=None, march=None):
    p = Plan(op, 4, nvec=4 * k if nvec is None else nvec)
    if march is not None:
        p.set_option(_lib.OPT_PCG_MARCH, march)
    p.set_shifts(shifts)
    for c in range(k):
        p.upload(0, _lib.SLOT_F, c, F[:, c])
    return p


def _w(p, col):
    return np.array(p.download(0, _lib.SLOT_W, col))


def test_iterations_queued_after_convergence_change_nothing(backend):
    dim, g, lowest, _, op, A, _, f = problem("lap2d_s0")
    k, n = 3, len(f)
    p = _plan_k(op, n, k, SHIFTS, np.random.RandomState(1).rand(n, k))
    p.pcg_begin_k(k, [0, k, 2 * k, 3 * k], RTOL, zero_start=True, flexible=True)
    p.pcg_iterate_k(20, 2, 2, _lib.GS_MC)
    running, done, status, indefinite, fnorm, hist = p.pcg_status_k(history=24)
    assert running == 0 and list(status) == [_lib.PCG_CONVERGED] * k and 0 < max(done) < 20
    x = [_w(p, c) for c in range(k)]
    p.pcg_iterate_k(5, 2, 2, _lib.GS_MC)
    running2, done2, status2, _, fnorm2, hist2 = p.pcg_status_k(history=24)
    assert running2 == 0 and np.array_equal(done, done2) and np.array_equal(status, status2)
    assert np.array_equal(hist, hist2) and np.array_equal(fnorm, fnorm2)
    for c in range(k):
        assert np.array_equal(x[c], _w(p, c))
        assert not np.any(hist[c, done[c]:])
    p.close()


def test_running_counts_the_columns_without_a_stop_word(backend):
    """the aggregate word, one status per iteration: it falls by one as each of three columns with different counts converges"""
    dim, g, lowest, _, op, A, _, f = problem("lap2d_s0")
    k, n = 3, len(f)
    p = _plan_k(op, n, k, SHIFTS, np.repeat(f[:, None], k, axis=1))
    p.pcg_begin_k(k, [0, k, 2 * k, 3 * k], RTOL, zero_start=True, flexible=True)
    assert p.pcg_status_k()[0] == k
    seen = []
    for _ in range(14):
        p.pcg_iterate_k(1, 2, 2, _lib.GS_MC)
        running, done, status = p.pcg_status_k()[:3]
        assert running == int(np.sum(status == _lib.PCG_RUNNING))
        seen.append(running)
    assert seen[0] == 3 and seen[-1] == 0 and sorted(set(seen)) == [0, 1, 2, 3]
    p.close()


# ---- 4. the marching direction pass against the generic passes ---------------------------------------------------------------

def check_marching_against_generic_k(g, opname, k=3, shifts=SHIFTS):
    """Iteration 1 from the same state: the new direction (the march writes it to the spare range) and (A - mu I) p carry the same
    bits per column; five iterations: x to 1e-10 (the partial sums of <p, q> are added in another order).  k columns with their
    own shifts in one launch."""
    n = g * g
    op = MARCH_OPS[opname](g)
    F = np.random.RandomState(1).rand(n, k)
    wj = dict(kind=_lib.WJACOBI, omega=2.0 / 3.0)
    X, P, Q, P2 = 0, k, 2 * k, 3 * k
    plans = []
    for march in (0, 1):
        p = _plan_k(op, n, k, shifts, F, march=march)
        p.pcg_begin_k(k, [X, P, Q, P2], 0.0, zero_start=True, flexible=False)
        p.pcg_iterate_k(1, 2, 2, **wj)
        plans.append(p)
    a, b = plans
    for c in range(k):
        pa, pb = _w(a, P + c), _w(b, P2 + c)
        assert np.any(pa) and np.array_equal(pa, pb), c
        assert np.array_equal(_w(a, Q + c), _w(b, Q + c)), c
    a.pcg_iterate_k(4, 2, 2, **wj)
    b.pcg_iterate_k(4, 2, 2, **wj)
    assert list(a.pcg_status_k()[1]) == list(b.pcg_status_k()[1]) == [5] * k
    for c in range(k):
        err = rel_err(_w(b, X + c), _w(a, X + c))
        print("%s %d^2 column %d: x after five iterations, march against generic: %.3e" % (opname, g, c, err))
        assert err < 1e-10
    a.close()
    b.close()


@pytest.mark.parametrize("opname", sorted(MARCH_OPS))
def test_marching_against_generic(backend, opname):
    """64^2: two row chunks"""
    check_marching_against_generic_k(64, opname)


# ---- 5. start vectors --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("smoother", ["wjacobi", "rb"])
def test_start_vectors(backend, smoother):
    dim, g, lowest, _, op, A, _, f = problem("lap2d_s0")
    n = len(f)
    F = np.random.RandomState(1).rand(n, 3)
    V0 = np.random.RandomState(5).rand(n, 3)
    X, info = run_matrix(op, F, SHIFTS, smoother, maxiter=60, v0_matrix=V0)
    assert info["status"] == ["converged"] * 3
    assert_columns_are_the_single_solves(op, F, SHIFTS, smoother, X, info, maxiter=60, v0_matrix=V0)


# ---- 6. limits and refusals --------------------------------------------------------------------------------------------------

def test_sixteen_equal_columns(backend):
    dim, g, lowest, _, op, A, _, f = problem("lap2d_s1.9")
    X, info = run_matrix(op, np.repeat(f[:, None], 16, axis=1), [1.9] * 16, "wjacobi", maxiter=60)
    assert X.shape == (len(f), 16) and info["status"] == ["converged"] * 16 and len(set(info["iterations"])) == 1
    for c in range(1, 16):
        assert np.array_equal(X[:, c], X[:, 0]) and np.array_equal(info["residuals"][c], info["residuals"][0])
    x0, i0 = run_alone(op, f, 1.9, "wjacobi", maxiter=60)
    assert np.array_equal(X[:, 0], x0) and info["iterations"][0] == i0["iterations"]


def test_refusals(backend):
    dim, g, lowest, _, op, A, _, f = problem("lap2d_s0")
    n = len(f)
    solver, sm = MGCMTSolver(), MGCMTStencilMaker()
    with pytest.raises(ValueError, match="columns"):
        solver.solve_matrix(np.ones((n, 17)), op, sm, lowest_level=4, dimension="2d")
    with pytest.raises(ValueError, match="shifts"):
        solver.solve_matrix(np.ones((n, 3)), op, sm, shifts=[0.0, 1.0], lowest_level=4, dimension="2d")
    with pytest.raises(NotImplementedError):
        solver.solve_matrix(np.ones((n, 2)), op, sm, smoother=lambda v, f, A, nu=4: v, lowest_level=4, dimension="2d")
    with pytest.raises(ValueError, match="lexicographic"):
        solver.solve_matrix(np.ones((16 ** 3, 2)), laplacian_operator(16, "3d"), sm, smoother=solver.sor, lowest_level=4, dimension="3d")
    with pytest.raises(ValueError, match="lexicographic"):
        solver.solve_matrix(np.ones((n, 2)), problem("vmass2d")[4], sm, smoother=solver.gseidel, lowest_level=4, dimension="2d")
    with pytest.raises(ValueError):
        solver.solve_matrix(np.ones((n, 2)), op, sm, lowest_level=4, dimension="2d", check_every=0)
    k = 3
    F = np.random.RandomState(1).rand(n, k)
    p = _plan_k(op, n, k, SHIFTS, F, nvec=4 * k)
    for call in (lambda: p.pcg_iterate_k(1, 2, 2, _lib.WJACOBI), lambda: p.pcg_status_k()):           # no batched begin yet
        with pytest.raises(MgcmtError, match="mgcmt error -1"):
            call()
    for vecs in ([0, 3, 6, 8], [0, 2, 6, 9], [0, 0, 3, 6], [0, 3, 6, 10], [-1, 3, 6, 9]):              # overlapping / out of range
        with pytest.raises(MgcmtError, match="mgcmt error -1"):
            p.pcg_begin_k(k, vecs, 1e-8, zero_start=True)
    for bad_k in (0, 17):
        with pytest.raises(MgcmtError, match="mgcmt error -1"):
            p.pcg_begin_k(bad_k, [0, 3, 6, 9], 1e-8, zero_start=True)
    with pytest.raises(MgcmtError, match="mgcmt error -1"):                                             # nvec = 12 < 4 * 4
        p.pcg_begin_k(4, [0, 4, 8, 12], 1e-8, zero_start=True)
    with pytest.raises(MgcmtError, match="mgcmt error -1"):                                             # an unknown flag
        _lib.check(_lib.lib().mgcmt_pcg_begin_k(p._h, k, (ctypes.c_int * 4)(0, 3, 6, 9), 1e-8, 4, None))
    # a begin of one kind ends the other kind's solve
    p.pcg_begin_k(k, [0, 3, 6, 9], 1e-8, zero_start=True)
    p.pcg_iterate_k(1, 2, 2, _lib.WJACOBI, omega=2 / 3)
    for call in (lambda: p.pcg_iterate(1, 2, 2, _lib.WJACOBI), lambda: p.pcg_status()):
        with pytest.raises(MgcmtError, match="mgcmt error -1"):
            call()
    p.upload(0, _lib.SLOT_F, 0, F[:, 0])
    p.pcg_begin([0, 1, 2, 3], 1e-8, zero_start=True)
    p.pcg_iterate(1, 2, 2, _lib.WJACOBI, omega=2 / 3)
    assert p.pcg_status()[0] == 1
    for call in (lambda: p.pcg_iterate_k(1, 2, 2, _lib.WJACOBI), lambda: p.pcg_status_k()):
        with pytest.raises(MgcmtError, match="mgcmt error -1"):
            call()
    p.close()


# ---- 6a. one block, one driver: a solve of one kind on the block a solve of the other kind left -------------------------------

@pytest.mark.parametrize("opname,g,shifts,march", [("lap", 32, (1.9, 0.0, 3.0), 0), ("well", 64, (0.0, 1.9, 3.0), 1)])
def test_single_and_batched_solves_share_one_block(backend, opname, g, shifts, march):
    """The single solve is the batched one with k = 1 on the plan's one block.  A single solve on a block that holds three columns,
    after a batched solve has used it, on four distinct unsorted columns of W: the bits of the same solve on a fresh plan, whose
    block holds one column.  Then the reverse: a batched solve after that single one, against the same batched solve on a fresh
    plan.  64^2 with the marching pass: two row chunks, and the p / p2 roles exchange on the one shared vector list."""
    n, k = g * g, 3
    op = MARCH_OPS[opname](g)
    F = np.random.RandomState(1).rand(n, k)
    wj = dict(kind=_lib.WJACOBI, omega=2.0 / 3.0)

    def single(p, vecs):
        p.pcg_begin(vecs, RTOL, zero_start=True, flexible=False)
        p.pcg_iterate(3, 2, 2, **wj)
        p.pcg_iterate(20, 2, 2, **wj)                       # converges on the way: the rest returns early
        return p.pcg_status(history=32), _w(p, vecs[0])

    def batched(p):
        for c in range(k):
            p.upload(0, _lib.SLOT_F, c, F[:, c])
        p.pcg_begin_k(k, [0, 3, 6, 9], RTOL, zero_start=True, flexible=False)
        p.pcg_iterate_k(40, 2, 2, **wj)
        return p.pcg_status_k(history=48), [_w(p, c) for c in range(k)]

    a = _plan_k(op, n, 1, shifts, F, nvec=12, march=march)
    (it_a, st_a, ind_a, fnorm_a, hist_a), x_a = single(a, [0, 1, 2, 3])
    assert st_a == _lib.PCG_CONVERGED and 3 < it_a < 23 and np.any(x_a)

    b = _plan_k(op, n, k, shifts, F, nvec=12, march=march)
    b.pcg_begin_k(k, [0, 3, 6, 9], RTOL, zero_start=True, flexible=False)
    b.pcg_iterate_k(2, 2, 2, **wj)
    b.upload(0, _lib.SLOT_F, 0, F[:, 0])
    (it_b, st_b, ind_b, fnorm_b, hist_b), x_b = single(b, [5, 1, 7, 2])
    print("%s %d^2: single solve, fresh plan %d iterations, after a batched solve %d; max |dx| %.3e" % (opname, g, it_a, it_b, np.max(np.abs(x_a - x_b))))
    assert (it_b, st_b, ind_b) == (it_a, st_a, ind_a) and fnorm_b == fnorm_a
    assert np.array_equal(hist_b, hist_a) and np.array_equal(x_b, x_a)
    for call in (lambda: b.pcg_iterate_k(1, 2, 2, **wj), lambda: b.pcg_status_k()):
        with pytest.raises(MgcmtError, match="mgcmt error -1"):
            call()

    (run_b, done_b, status_b, _, fnorm_kb, hist_kb), xs_b = batched(b)
    c = _plan_k(op, n, k, shifts, F, nvec=12, march=march)
    (run_c, done_c, status_c, _, fnorm_kc, hist_kc), xs_c = batched(c)
    print("%s %d^2: batched solve, fresh plan %s iterations, after a single solve %s" % (opname, g, done_c.tolist(), done_b.tolist()))
    assert run_c == 0 and list(status_c) == [_lib.PCG_CONVERGED] * k
    assert run_b == run_c and np.array_equal(done_b, done_c) and np.array_equal(status_b, status_c) and np.array_equal(fnorm_kb, fnorm_kc)
    assert np.array_equal(hist_kb, hist_kc)
    for col in range(k):
        assert np.array_equal(xs_b[col], xs_c[col]), col
    for p in (a, b, c):
        p.close()


# ---- 7. bit-reproducibility ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,smoother", [("lap2d_s0", "rb"), ("pot3d", "wjacobi")])
def test_two_runs_are_bit_identical(backend, name, smoother):
    dim, g, lowest, _, op, A, _, f = problem(name)
    shifts = SHIFTS if dim == "2d" else (0.0, 2.5, 0.0)
    F = np.random.RandomState(1).rand(len(f), 3)
    a, ia = run_matrix(op, F, shifts, smoother, dimension=dim, lowest=lowest, maxiter=60)
    b, ib = run_matrix(op, F, shifts, smoother, dimension=dim, lowest=lowest, maxiter=60)
    assert np.array_equal(a, b) and ia["iterations"] == ib["iterations"] and ia["status"] == ib["status"]
    for ra, rb in zip(ia["residuals"], ib["residuals"]):
        assert np.array_equal(ra, rb)


# ---- 8. the ABI -----------------------------------------------------------------------------------------------------------------

def test_exports_and_signatures(backend):
    lib = _lib.lib()
    c_int, c_void_p, c_double, ip, dp = ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    expected = {"mgcmt_pcg_begin_k": [c_void_p, c_int, ip, c_double, c_int, c_void_p],
                "mgcmt_pcg_iterate_k": [c_void_p, c_int, c_int, c_int, c_int, c_int, c_double, c_void_p],
                "mgcmt_pcg_status_k": [c_void_p, ip, ip, ip, dp, dp, c_int, c_void_p]}
    for name, args in expected.items():
        assert name in _lib.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is c_int and list(fn.argtypes) == args, name
    assert lib.mgcmt_abi_version() == _lib.ABI_VERSION == 7
    import MGCMTSolver as root
    assert root.MGCMTSolver is MGCMTSolver and hasattr(root.MGCMTSolver, "solve_matrix")
