"""Memory contract of the 3-D kernels of a plan with per-point bonds (the k3pm_*<BONDS = true> marching kernels and the kPointBonds
branches of csrc/kernels_3d_point.hip) under the emulated runtime's guard mode: the checks and the case machinery of
tests/test_memory_contract.py, on plans of mgcmt_plan_create3d_bonds.

16^3: the flat kernels of the fine level (constant 7-point + D + bonds) and of the 27-plane levels, entry by entry.  64^3: the
marching kernels of the fine level (two z-chunks, one x-tile).  8^3 with lowest = 8: the band matrix takes D and the bonds.
Plan creation (the four planes' upload, k3p_coarsen's four-plane source), both smoothers, residual + restriction, prolongation + correction, the coarse solve's band assembly, a V(2,2) cycle
and its repeats run with red zones round every device block and NaN payloads; halo planes and column padding stay exact
zeros, columns q >= k keep their markers, and a cycle repeated on the same plan reproduces its first result bit for bit."""
import numpy as np
import pytest

import test_memory_contract as mc
from multigridcmt_amd import _lib
from multigridcmt_amd.operators import variable_mass_operator
from test_memory_contract import MC, WJ, F, T, V, Case, Guard


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


def _bonds3d(g):
    """a smeared ellipsoidal dot with seeded noise on the inverse mass and the potential"""
    t = (np.arange(g) + 0.5) / g - 0.5
    Z, Y, X = np.meshgrid(t, t, t, indexing="ij")
    s = 0.5 * (1.0 + np.tanh((np.sqrt((X - 0.05) ** 2 + ((Y + 0.03) / 0.8) ** 2 + ((Z - 0.02) / 0.6) ** 2) - 0.3) / 0.08))
    rng = np.random.RandomState(17)
    return variable_mass_operator(g, 1.0 - 0.27 * s + 0.2 * rng.rand(g, g, g), 30.0 * s + 5.0 * rng.rand(g, g, g), dimension="3d")


CASES = [
    # flat kernels: the fine level and the 27-plane levels entry by entry, then whole cycles (Gram-Schmidt, zero start)
    Case("bonds3d_16_pieces", _bonds3d, 16, 4, 3, 2,
         [mc.smooth(0, WJ, 2, 2. / 3., 2), mc.smooth(0, MC, 1, 1.0, 2), mc.apply(0, (V, 0), (T, 1), with_shift=True), mc.apply(1, (V, 1), (T, 0)),
          mc.smooth(1, WJ, 2, 2. / 3., 2), mc.smooth(1, MC, 1, 1.2, 2), mc.residual_restrict(0, 2), mc.residual_restrict(1, 2), mc.coarse_solve(2),
          mc.prolong_correct(1, 2), mc.prolong_correct(0, 2), mc.vcycle(2, 2, WJ, 2. / 3., 2, nuc=2), mc.vcycle(2, 2, WJ, 2. / 3., 2, nuc=2),
          mc.vcycle(1, 1, MC, 1.0, 2, nuc=1, gs=True, zero_start=True)],
         mc._vk(2) + mc._vk(2, 1, (F,)) + [(0, T, 1), (1, T, 0)], init_levels=(0, 1)),
    # marching kernels of the fine level: two z-chunks
    Case("bonds3d_64_marching", _bonds3d, 64, 8, 2, 1,
         [mc.smooth(0, WJ, 1, 2. / 3., 1), mc.smooth(0, MC, 1, 1.0, 1), mc.residual_restrict(0, 1), mc.prolong_correct(0, 1),
          mc.vcycle(2, 2, WJ, 2. / 3., 1, nuc=2), mc.vcycle(2, 2, WJ, 2. / 3., 1, nuc=2), mc.vcycle(2, 2, MC, 1.0, 1, nuc=2)],
         mc._vk(1) + mc._vk(1, 1, (F,))),
    # level 0 is the coarsest level too: k3p_band_add's bonds
    Case("bonds3d_8_band", _bonds3d, 8, 8, 2, 2, [mc.coarse_solve(2), mc.vcycle(2, 2, WJ, 2. / 3., 2, nuc=2)], mc._vk(2)),
]
CASE_IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_guarded_run_is_clean_and_bit_identical_3d_point_bonds(guard, case):
    """no red zone touched, no copy out of range, finite results equal to the unguarded run's bit for bit"""
    mc.test_guarded_run_is_clean_and_bit_identical(guard, case)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_halo_and_padding_stay_zero_3d_point_bonds(guard, case):
    """halo planes and column padding stay exact zeros, columns q >= k and every vector an entry does not name are untouched"""
    if case.g == 64:
        p = case.plan()
        try:
            assert p.level_path_3d(0) == (_lib.PATH3D_SEVEN_BONDS, True) and p.level_path_3d(1) == (_lib.PATH3D_PLANES, False)
        finally:
            p.close()
    mc.test_halo_and_padding_stay_zero(guard, case)


@pytest.mark.parametrize("g,lowest", [(16, 4), (64, 8)])
@pytest.mark.parametrize("kind,omega", [(WJ, 2. / 3.), (MC, 1.0)])
def test_repeated_cycle_reproduces_the_first_3d_point_bonds(guard, g, lowest, kind, omega):
    """the same V(2,2) cycle three times on one plan (eager, captured, replayed) from the same start: bit-identical results"""
    guard.enable(True)
    from multigridcmt_amd.plan import Plan
    p = None
    try:
        p = Plan(_bonds3d(g), lowest, nvec=2)
        p.set_shifts([0.4, 0.0])
        rng = np.random.RandomState(g)
        v0, f = rng.rand(g ** 3), rng.rand(g ** 3)
        outs = []
        for _ in range(3):
            p.upload(0, V, 0, v0)
            p.upload(0, F, 0, f)
            p.vcycle(2, 2, kind, omega=omega, k=1, nu_coarse=2)
            outs.append(np.array(p.download(0, V, 0)))
            assert guard.take() == []
        assert np.all(np.isfinite(outs[0]))
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    finally:
        if p is not None:
            p.close()
    assert guard.take() == [] and guard.live() == 0
