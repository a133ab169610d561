"""Memory contract of the kernels of a plan with a per-point 9-point stencil (mgcmt_plan_create_nine: the nine-plane branch of
csrc/kernels_pointwise.hip on level 0, and the tile kernels of csrc/kernels_nine_tile.hip) under the emulated runtime's
guard mode: the checks and the case machinery of tests/test_memory_contract.py.

16^2: the flat kernels, entry by entry, then whole cycles.  128^2: the tile kernels of level 0 — eight tiles of 32 x 64, every
window reaching over a grid edge; a Jacobi pair, the odd sweep, a four-colour sweep, residual + restriction in one pass.
8^2 with lowest = 8: a single level, whose band matrix carries the nine planes.  Plan creation (the upload of the planes,
k_pw_coarsen from them), both smoothers, the applied operator, residual + restriction, prolongation + correction, the coarse
solve's band assembly, V(2,2) cycles and their repeats run with red zones round every device block and NaN payloads; halo rows
and column padding stay exact zeros, columns q >= k keep their markers, and a cycle repeated on the same plan reproduces its
first result bit for bit."""
import numpy as np
import pytest

import test_memory_contract as mc
from multigridcmt_amd import _lib
from multigridcmt_amd.operators import tensor_mass_operator
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


def _tensor(g):
    t = (np.arange(g) + 0.5) / g - 0.5
    X, Y = np.meshgrid(t, t, indexing="ij")
    inside = (X - 0.05) ** 2 + (Y + 0.1) ** 2 < 0.3 ** 2
    l1 = np.where(inside, 4.0 * (1.0 + 0.2 * np.random.RandomState(17).rand(g, g)), 1.0)
    theta = np.where(inside, 0.6, 0.0)
    c, s = np.cos(theta), np.sin(theta)
    return tensor_mass_operator(g, c * c * l1 + s * s, s * s * l1 + c * c, c * s * (l1 - 1.0), V=np.where(inside, 0.0, 30.0))


CASES = [
    # flat kernels: level 0 and the Galerkin levels entry by entry, then whole cycles (Gram-Schmidt, zero start)
    Case("nine_16_pieces", _tensor, 16, 4, 3, 2,
         [mc.smooth(0, WJ, 3, 2. / 3., 2), mc.smooth(0, MC, 1, 1.0, 2), mc.apply(0, (V, 0), (T, 1), with_shift=True), mc.apply(1, (V, 1), (T, 0)),
          mc.smooth(1, WJ, 2, 2. / 3., 2), mc.smooth(1, MC, 1, 1.2, 2), mc.residual_restrict(0, 2), mc.residual_restrict(1, 2),
          mc.coarse_solve(2), mc.prolong_correct(1, 2), mc.prolong_correct(0, 2),
          mc.vcycle(2, 2, WJ, 2. / 3., 2, nuc=2), mc.vcycle(2, 2, WJ, 2. / 3., 2, nuc=2), mc.vcycle(1, 1, MC, 1.0, 2, nuc=1, gs=True, zero_start=True)],
         mc._vk(2) + mc._vk(2, 1, (F,)) + [(0, T, 1), (1, T, 0)], init_levels=(0, 1)),
    # tile kernels of level 0: 4 x 2 tiles, every one at a grid edge
    Case("nine_128_tiles", _tensor, 128, 8, 3, 2,
         [mc.smooth(0, WJ, 1, 2. / 3., 2), mc.smooth(0, WJ, 3, 2. / 3., 2), mc.smooth(0, MC, 1, 1.0, 2), mc.smooth(0, MC, 2, 1.2, 2),
          mc.apply(0, (V, 0), (T, 1), with_shift=True), mc.residual_restrict(0, 2), mc.prolong_correct(0, 2),
          mc.vcycle(2, 2, WJ, 2. / 3., 2, nuc=2), mc.vcycle(2, 2, WJ, 2. / 3., 2, nuc=2), mc.vcycle(2, 2, MC, 1.0, 2, nuc=2),
          mc.vcycle(1, 1, MC, 1.2, 2, nuc=1, gs=True, zero_start=True), mc.vcycle(3, 3, WJ, 2. / 3., 1, nuc=2)],
         mc._vk(2) + mc._vk(2, 1, (F,)) + [(0, T, 1)]),
    # a single level: the coarse solve on level 0, alone and as the whole cycle
    Case("nine_8_single_level", _tensor, 8, 8, 2, 1,
         [mc.apply(0, (V, 0), (T, 1), with_shift=True), mc.smooth(0, WJ, 2, 2. / 3., 1), mc.smooth(0, MC, 1, 1.0, 1), mc.coarse_solve(1),
          mc.vcycle(2, 2, WJ, 2. / 3., 1, nuc=2), mc.vcycle(2, 2, MC, 1.0, 1, nuc=2)],
         mc._vk(1) + [(0, T, 1)]),
]
CASE_IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_guarded_run_is_clean_and_bit_identical_nine_point(guard, case):
    """no red zone touched, no copy out of range, finite results equal to the unguarded run's bit for bit"""
    mc.test_guarded_run_is_clean_and_bit_identical(guard, case)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_halo_and_padding_stay_zero_nine_point(guard, case):
    """halo rows and column padding stay exact zeros, columns q >= k and every vector an entry does not name are untouched"""
    p = case.plan()
    try:
        assert p.operator_kind(0) == _lib.OPK_NINE_POINT
        assert p.point_stencil(0).shape == (3, 3, case.g, case.g)
        assert p.level_tiled(0) == (case.g >= 128)
    finally:
        p.close()
    mc.test_halo_and_padding_stay_zero(guard, case)


@pytest.mark.parametrize("g,lowest", [(16, 4), (128, 8), (8, 8)])
@pytest.mark.parametrize("kind,omega", [(WJ, 2. / 3.), (MC, 1.0)])
def test_repeated_cycle_reproduces_the_first_nine_point(guard, g, lowest, kind, omega):
    """the same V(2,2) cycle three times on one plan (eager, captured, replayed) from the same start: bit-identical results"""
    guard.enable(True)
    from multigridcmt_amd.plan import Plan
    p = None
    try:
        p = Plan(_tensor(g), lowest, nvec=2)
        p.set_shifts([0.4, 0.0])
        rng = np.random.RandomState(g)
        v0, f = rng.rand(g * g), rng.rand(g * g)
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
