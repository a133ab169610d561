"""Memory contract of the preconditioned conjugate-gradient entries (csrc/pcg_host.hip, csrc/kernels_pcg.hip: mgcmt_pcg_begin,
mgcmt_pcg_iterate, mgcmt_pcg_status) under the emulated runtime's guard mode: the checks and the case machinery of
tests/test_memory_contract.py at 32^2 and 16^3.

What the entries may write (include/mgcmt_hip.h): the columns x, p, q of slot W the begin was given, F[0] column 0 (the residual
replaces the right-hand side) and what mgcmt_vcycle writes; the spare column p2 — which only the marching direction pass
writes (MGCMT_OPT_PCG_MARCH: on in the case at 64^2, two row chunks whose overlap rows reach into the halo, off in the one at
32^2; the per-point and 3-D levels are not covered by it) — and every other column keep their markers.  The state words, the
history and the partial sums are one block of the plan's own that is not cleared at allocation: under the guard its payload
starts as NaN, so a scalar kernel that read a partial sum no pass wrote, or a status that returned a word no begin set, would
show.  The sequences queue more iterations than the solve needs, so the kernels' early return behind the stop
word runs guarded too, and start once from a vector in x (the begin's operator application into q)."""
import numpy as np
import pytest

import test_memory_contract as mc
from multigridcmt_amd import _lib
from test_memory_contract import MC, WJ, F, V, W, Case, Guard

VECS = (0, 1, 2, 3)


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


def pcg_begin(rtol, zero_start, flexible):
    written = {(0, W, VECS[0]), (0, F, 0)} if zero_start else {(0, W, VECS[2]), (0, F, 0)}
    return mc.Step("pcg_begin(zero=%d,flex=%d)" % (zero_start, flexible),
                   lambda p: p.pcg_begin(VECS, rtol, zero_start=zero_start, flexible=flexible), lambda p: set(written))


def pcg_iterate(n, kind, omega, march=False):
    def writes(p):
        cycle = {(l, s, 0) for l in range(p.num_levels) for s in ((V, mc.T) if l == 0 else (V, F, mc.T))}
        spare = {(0, W, VECS[3])} if march else set()       # the marching direction pass alternates between p and p2
        return cycle | spare | {(0, W, VECS[0]), (0, W, VECS[1]), (0, W, VECS[2]), (0, F, 0)}
    return mc.Step("pcg_iterate(%d,kind=%d)" % (n, kind), lambda p: p.pcg_iterate(n, 2, 2, kind, omega=omega, nu_coarse=2), writes)


def pcg_status(history):
    def run(p):
        it, st, indefinite, fnorm, hist = p.pcg_status(history=history)
        return np.concatenate([[it, st, indefinite, fnorm], hist])
    return mc.Step("pcg_status", run, lambda p: set())


def _steps(first_kind, first_omega, march=False):
    return [pcg_begin(1e-9, True, first_kind != WJ), pcg_iterate(3, first_kind, first_omega, march), pcg_status(8),
            pcg_iterate(30, first_kind, first_omega, march), pcg_status(40),              # converges on the way: the rest returns early
            mc.Step("copy F1 -> F0", lambda p: p.copy(0, F, 1, F, 0), lambda p: {(0, F, 0)}),      # a new right-hand side
            pcg_begin(1e-6, False, True), pcg_iterate(4, MC, 1.0, march), pcg_status(8)]  # from the x the first solve left


K = 2
CASES = [
    Case("pcg_2d_wj", mc._lap2d, 32, 4, 6, K, _steps(WJ, 2.0 / 3.0), [(0, W, q) for q in VECS[:3]] + [(0, F, 0)], shifts=[1.9, 0.0],
         options={_lib.OPT_PCG_MARCH: 0}),
    Case("pcg_2d_march", mc._well, 64, 4, 6, K, _steps(WJ, 2.0 / 3.0, True), [(0, W, q) for q in VECS] + [(0, F, 0)], shifts=[1.9, 0.0],
         options={_lib.OPT_PCG_MARCH: 1}),
    Case("pcg_2d_point", mc._point, 32, 4, 6, K, _steps(MC, 1.0), [(0, W, q) for q in VECS[:3]] + [(0, F, 0)], shifts=[0.0, 0.0]),
    Case("pcg_3d_mc", mc._lap3d, 16, 4, 6, K, _steps(MC, 1.0), [(0, W, q) for q in VECS[:3]] + [(0, F, 0)], shifts=[0.0, 0.0]),
]
CASE_IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_guarded_run_is_clean_and_bit_identical_pcg(guard, case):
    """no red zone touched, no copy out of range, finite results equal to the unguarded run's bit for bit"""
    mc.test_guarded_run_is_clean_and_bit_identical(guard, case)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_halo_and_padding_stay_zero_pcg(guard, case):
    """halo rows and column padding stay exact zeros; every vector an entry does not name as an output is untouched"""
    mc.test_halo_and_padding_stay_zero(guard, case)


def test_guarded_solve(guard):
    """MGCMTSolver.solve at 32^2 (shift 1.9) and 16^3, guard off and on: no violation, nothing left behind, the same bits"""
    from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, plan
    runs = []
    for on in (False, True):
        guard.enable(on)
        solver, sm, outs = MGCMTSolver(), MGCMTStencilMaker(), []
        for op, shift, dim, smoother in ((mc._lap2d(32), 1.9, "2d", solver.wjacobi), (mc._lap3d(16), 0.0, "3d", solver.gseidel_rb)):
            info = {}
            f = np.random.RandomState(1).rand(op.shape[0])
            x = solver.solve(f, op, sm, smoother=smoother, shift=shift, lowest_level=4, dimension=dim, rtol=1e-10, check_every=8, info=info)
            assert guard.take() == []
            assert info["status"] == "converged" and info["true_residual"] <= 2e-10
            outs += [np.array(x), np.array(info["residuals"]), np.array([info["iterations"], info["true_residual"]])]
        plan.release_plans()
        assert guard.take() == [] and guard.live() == 0
        runs.append(outs)
    for x in runs[1]:
        assert np.all(np.isfinite(x))
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
