"""Memory contract of the batched conjugate-gradient entries (csrc/pcg_host.hip, csrc/kernels_pcg.hip: mgcmt_pcg_begin_k,
mgcmt_pcg_iterate_k, mgcmt_pcg_status_k) under the emulated runtime's guard mode: the checks and the case machinery of
tests/test_memory_contract.py, as tests/test_memory_contract_pcg.py uses them, with k = 3 columns at 32^2 (the generic passes),
64^2 (the marching direction pass, two row chunks) and 16^3.

What the entries may write (include/mgcmt_hip.h): the ranges x, p, q of slot W — k consecutive columns each — the begin was
given, the spare range p2 only with the marching pass, F[0] columns 0 .. k - 1 (the residuals replace the right-hand sides) and
what a k-column mgcmt_vcycle writes.  The plans store 4 k + 1 vectors: column 4 k of W lies outside the four ranges, and the
columns k .. of F and V outside the solve; all keep their markers.  Column 1 has f = 0, so its stop word is set in the begin:
its x, p and r must stay what the begin left while the other columns iterate (its z and q are scratch of the cycle and of the
operator application, which know nothing of stop words; the marching pass writes neither).  Once every column has stopped a
further mgcmt_pcg_iterate_k writes the cycle's vectors and, without the marching pass, the q range, and nothing else.

The state words, the histories and the partial sums of the k columns are one block of the plan's own that is not cleared at
allocation: under the guard its payload starts as NaN, so a scalar kernel that read another column's partial sums, or sums no
pass wrote, or a status that returned a word no begin set, would show."""
import numpy as np
import pytest

import test_memory_contract as mc
from multigridcmt_amd import _lib
from test_memory_contract import MC, WJ, F, V, W, Case, Guard

K = 3
X, P, Q, P2 = 0, K, 2 * K, 3 * K          # first columns of the four ranges; column 4 K is outside all of them
NVEC = 4 * K + 1
ZERO_COLUMN = 1


@pytest.fixture
def guard():
    """the guard mode lives in the emulated runtime (host memory): these tests bind the emulation build themselves"""
    from conftest import bind_backend
    from multigridcmt_amd import general, plan
    bind_backend("emu")
    plan.release_plans()
    general.release_plans()
    g = Guard()
    g.enable(False)
    g.take()
    yield g
    g.enable(False)
    g.take()


def _range(first, skip=()):
    return {(0, W, first + c) for c in range(K) if c not in skip}


def _rhs(skip=()):
    return {(0, F, c) for c in range(K) if c not in skip}


def _cycle(p):
    return {(l, s, c) for l in range(p.num_levels) for s in ((V, mc.T) if l == 0 else (V, F, mc.T)) for c in range(K)}


def begin_k(rtol, zero_start, flexible):
    written = (_range(X) if zero_start else _range(Q)) | _rhs()
    return mc.Step("pcg_begin_k(zero=%d,flex=%d)" % (zero_start, flexible),
                   lambda p: p.pcg_begin_k(K, [X, P, Q, P2], rtol, zero_start=zero_start, flexible=flexible), lambda p: set(written))


def iterate_k(n, kind, omega, march, frozen=()):
    """frozen: the columns whose stop word is set before the call — their x, p (p2) and r are not in the set"""
    def writes(p):
        spare = _range(P2, frozen) if march else set()
        # (the generic passes apply the operator to all k columns of p; the marching pass returns for a frozen column)
        q = _range(Q, frozen) if march else _range(Q)
        return _cycle(p) | _range(X, frozen) | _range(P, frozen) | spare | q | _rhs(frozen)
    return mc.Step("pcg_iterate_k(%d,kind=%d,frozen=%s)" % (n, kind, list(frozen)),
                   lambda p: p.pcg_iterate_k(n, 2, 2, kind, omega=omega, nu_coarse=2), writes)


def status_k(history, all_stopped=None):
    def run(p):
        running, done, status, indefinite, fnorm, hist = p.pcg_status_k(history=history)
        if all_stopped is not None:
            assert (running == 0) == all_stopped and done[ZERO_COLUMN] == 0 and status[ZERO_COLUMN] == _lib.PCG_CONVERGED
        return np.concatenate([[running], done, status, indefinite, fnorm, hist.ravel()])
    return mc.Step("pcg_status_k", run, lambda p: set())


def _steps(kind, omega, march=False):
    everything = tuple(range(K))
    new_rhs = [mc.Step("copy F%d -> F%d" % (K + c, c), (lambda c: lambda p: p.copy(0, F, K + c, F, c))(c), (lambda c: lambda p: {(0, F, c)})(c))
               for c in range(K)]
    return [mc.Step("zero F%d" % ZERO_COLUMN, lambda p: p.zero(0, F, ZERO_COLUMN), lambda p: {(0, F, ZERO_COLUMN)}),
            begin_k(1e-9, True, kind != WJ), iterate_k(3, kind, omega, march, frozen=(ZERO_COLUMN,)), status_k(8, all_stopped=False),
            iterate_k(30, kind, omega, march, frozen=(ZERO_COLUMN,)), status_k(40, all_stopped=True),   # converges on the way: the rest returns early
            iterate_k(2, kind, omega, march, frozen=everything), status_k(40, all_stopped=True)] + new_rhs + \
           [begin_k(1e-6, False, True), iterate_k(4, MC, 1.0, march), status_k(8)]                    # from the x the first solve left


def _downloads(march):
    return [(0, W, first + c) for first in ((X, P, Q, P2) if march else (X, P, Q)) for c in range(K)] + [(0, F, c) for c in range(K)]


CASES = [
    Case("pcgk_2d_wj", mc._lap2d, 32, 4, NVEC, K, _steps(WJ, 2.0 / 3.0), _downloads(False), shifts=[1.9, 0.7, 0.0], options={_lib.OPT_PCG_MARCH: 0}),
    Case("pcgk_2d_march", mc._well, 64, 4, NVEC, K, _steps(WJ, 2.0 / 3.0, True), _downloads(True), shifts=[1.9, 0.7, 0.0],
         options={_lib.OPT_PCG_MARCH: 1}),
    Case("pcgk_3d_mc", mc._lap3d, 16, 4, NVEC, K, _steps(MC, 1.0), _downloads(False), shifts=[0.0, 0.4, 2.5]),
]
CASE_IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_guarded_run_is_clean_and_bit_identical_pcg_matrix(guard, case):
    """no red zone touched, no copy out of range, finite results equal to the unguarded run's bit for bit"""
    mc.test_guarded_run_is_clean_and_bit_identical(guard, case)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_halo_and_padding_stay_zero_pcg_matrix(guard, case):
    """halo rows and column padding stay exact zeros; every vector an entry does not name as an output is untouched: the
    columns outside the solve, the W column outside the four ranges, and a frozen column's x, p and r"""
    mc.test_halo_and_padding_stay_zero(guard, case)


def test_guarded_solve_matrix(guard):
    """MGCMTSolver.solve_matrix at 32^2 (shifts 0 / 1.9 / 3.0) and 16^3, guard off and on: no violation, nothing left behind,
    the same bits"""
    from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, plan
    runs = []
    for on in (False, True):
        guard.enable(on)
        solver, sm, outs = MGCMTSolver(), MGCMTStencilMaker(), []
        for op, shifts, dim, smoother in ((mc._lap2d(32), (0.0, 1.9, 3.0), "2d", solver.wjacobi), (mc._lap3d(16), (0.0, 2.5), "3d", solver.gseidel_rb)):
            info = {}
            fm = np.random.RandomState(1).rand(op.shape[0], len(shifts))
            x = solver.solve_matrix(fm, op, sm, smoother=smoother, shifts=shifts, lowest_level=4, dimension=dim, rtol=1e-10, check_every=8, info=info)
            assert guard.take() == []
            assert info["status"] == ["converged"] * len(shifts) and max(info["true_residual"]) <= 2e-10
            outs += [np.array(x), np.concatenate(info["residuals"]), np.array(info["iterations"] + info["true_residual"])]
        plan.release_plans()
        assert guard.take() == [] and guard.live() == 0
        runs.append(outs)
    for x in runs[1]:
        assert np.all(np.isfinite(x))
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)


def test_state_block_grows_with_the_column_count(guard):
    """a begin with more columns than the block holds replaces the block: guarded, nothing left behind"""
    guard.enable(True)
    from multigridcmt_amd.plan import Plan
    p = Plan(mc._lap2d(32), 4, nvec=16)
    try:
        p.set_shifts([0.0, 1.9, 3.0, 0.5])
        for k in (2, 4, 3):
            for c in range(k):
                p.upload(0, F, c, np.random.RandomState(c).rand(32 * 32))
            p.pcg_begin_k(k, [0, 4, 8, 12], 1e-9, zero_start=True)
            p.pcg_iterate_k(16, 2, 2, WJ, omega=2.0 / 3.0)
            running, done, status = p.pcg_status_k(history=16)[:3]
            assert running == 0 and len(done) == k and list(status) == [_lib.PCG_CONVERGED] * k
            assert guard.take() == []
    finally:
        p.close()
    assert guard.take() == [] and guard.live() == 0
