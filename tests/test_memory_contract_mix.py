"""Memory contract of the entries behind Anderson mixing in drivers.schroedinger_poisson — mgcmt_mix_residual and mgcmt_mix_combine
(csrc/kernels_mix.hip: k_mix_residual, k_mix_final, k_mix_combine) — under the emulated runtime's guard mode: the checks and the
case machinery of tests/test_memory_contract.py, as tests/test_memory_contract_scf.py uses them, on a 32^2 and a 16^3 plan.

A residual with the full eight earlier residuals into a column between two others, with none, and on level 1; a combination of
nine pairs into a fresh column, of one pair, and of three pairs into the column of its own oldest x (the one input the entry
lets the destination be).  The inner products the residual returns take part in the bit-for-bit comparison with the unguarded
run.  Then one guarded run of the driver with mixing_history = 3."""
import numpy as np
import pytest

import test_memory_contract as mc
from multigridcmt_amd.operators import potential_operator
from test_memory_contract import F, V, Case, Guard


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


def _point3d(g):
    return potential_operator(g, 5.0 * np.random.RandomState(19).rand(g, g, g), dimension="3d")


def mix_residual(l, out, inp, r, prev):
    return mc.Step("mix_residual(l=%d,nprev=%d)" % (l, len(prev)), lambda p: p.mix_residual(l, out, inp, r, prev), lambda p: {(l,) + tuple(r)})


def mix_combine(l, xs, rs, dst):
    alpha = np.cos(np.arange(len(xs)) + 1.0)
    return mc.Step("mix_combine(l=%d,p=%d)" % (l, len(xs)), lambda p: p.mix_combine(l, xs, rs, alpha, 0.5, dst), lambda p: {(l,) + tuple(dst)})


K = 20                                                   # columns of V and F the case machinery fills on the start levels
_PREV = [(F, q) for q in range(8)]
_XS, _RS = [(V, q) for q in range(9)], [(F, q) for q in range(9)]
_STEPS = [mix_residual(0, (V, 10), (V, 11), (F, 15), _PREV), mix_residual(0, (V, 12), (F, 15), (F, 16), []),
          mix_residual(1, (V, 10), (V, 11), (F, 15), _PREV[:3]), mix_combine(0, _XS, _RS, (F, 17)), mix_combine(0, _XS[:1], _RS[:1], (V, 19)),
          mix_combine(1, _XS[:3], _RS[:3], _XS[0]), mix_combine(0, [(V, 13), (V, 14), (V, 15)], [(F, 15), (F, 16), (F, 17)], (V, 13))]
_DOWNLOADS = [(0, F, 15), (0, F, 16), (1, F, 15), (0, F, 17), (0, V, 19), (1, V, 0), (0, V, 13)]

CASES = [Case("mix_2d", mc._point, 32, 4, 48, K, _STEPS, _DOWNLOADS, init_levels=(0, 1)),
         Case("mix_3d", _point3d, 16, 4, 48, K, _STEPS, _DOWNLOADS, init_levels=(0, 1))]
CASE_IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_guarded_run_is_clean_and_bit_identical_mix(guard, case):
    """no red zone touched, no copy out of range, finite results equal to the unguarded run's bit for bit"""
    mc.test_guarded_run_is_clean_and_bit_identical(guard, case)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_halo_and_padding_stay_zero_mix(guard, case):
    """halo rows / planes and column padding stay exact zeros; every vector other than the one an entry names as its
    destination is bitwise unchanged"""
    mc.test_halo_and_padding_stay_zero(guard, case)


def test_guarded_schroedinger_poisson_with_mixing_history(guard):
    """drivers.schroedinger_poisson with mixing_history = 3 and the guard on — the dot of tests/test_schroedinger_poisson.py, six
    steps, so that the ring of four pairs is full and the steps from the fourth on write over the oldest x —: no violation, nothing left
    behind, finite results"""
    from multigridcmt_amd import drivers, plan
    from scf_reference import case_2d
    op, poisson_op = case_2d()
    guard.enable(True)
    info = {}
    vals, vecs, phi = drivers.schroedinger_poisson(op, poisson_op, 6, [2, 2, 2, 0, 0, 0], coupling=4000.0, mixing=0.5, mixing_history=3, lowest=4,
                                                   maxiter=6, info=info)
    assert guard.take() == []
    plan.release_plans()
    assert guard.take() == [] and guard.live() == 0
    assert info["iterations"] == 6 and info["status"] == "maxiter" and info["mixing_depths"] == [1, 2, 3, 4, 4, 4]
    assert all(np.all(np.isfinite(x)) for x in (vals, vecs, phi, info["density"], np.array(info["changes"])))
