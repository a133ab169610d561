"""Memory contract of the 3-D kernels on a plan with a per-point 27-point stencil (mgcmt_plan_create3d_stencil:
csrc/kernels_3d_point.hip through stencil27_point.h, csrc/kernels_3d_stencil.hip) under the emulated runtime's guard mode: the
checks and the case machinery of tests/test_memory_contract.py.

16^3: the flat kernels of level 0 (constant 7-point + 27 planes) and of the 27-plane levels below, entry by entry.  64^3: the
colour stages launched on their own points and the LDS residual + restriction of level 0 (two tiles along every axis, four
chunks of coarse planes).  8^3 with lowest = 8: level 0 is the coarsest level too (its planes go into the band matrix).  Plan
creation (the stencil's upload, k3p_coarsen from 27 planes), both smoothers, residual + restriction, prolongation + correction,
the coarse solve, V(2,2) cycles and their repeats run with red zones round every device block and NaN payloads; halo planes and
column padding stay exact zeros, columns q >= k keep their markers, and a cycle repeated on the same plan reproduces its first
result bit for bit."""
import numpy as np
import pytest

import test_memory_contract as mc
from multigridcmt_amd import _lib
from test_3d_tensor_mass import tensor_op
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


def _tensor3d(g):
    return tensor_op(g, "rough")


CASES = [
    # flat kernels: level 0 and the 27-plane levels entry by entry, then whole cycles (Gram-Schmidt, zero start)
    Case("tensor3d_16_pieces", _tensor3d, 16, 4, 3, 2,
         [mc.smooth(0, WJ, 2, 2. / 3., 2), mc.smooth(0, MC, 1, 1.0, 2), mc.apply(0, (V, 0), (T, 1), with_shift=True), mc.apply(1, (V, 1), (T, 0)),
          mc.smooth(1, WJ, 2, 2. / 3., 2), mc.smooth(1, MC, 1, 1.2, 2), mc.residual_restrict(0, 2), mc.residual_restrict(1, 2), mc.coarse_solve(2),
          mc.prolong_correct(1, 2), mc.prolong_correct(0, 2), mc.vcycle(2, 2, WJ, 2. / 3., 2, nuc=2), mc.vcycle(2, 2, WJ, 2. / 3., 2, nuc=2),
          mc.vcycle(1, 1, MC, 1.0, 2, nuc=1, gs=True, zero_start=True)],
         mc._vk(2) + mc._vk(2, 1, (F,)) + [(0, T, 1), (1, T, 0)], init_levels=(0, 1)),
    # the kernels of kernels_3d_stencil.hip on level 0
    Case("tensor3d_64_new_kernels", _tensor3d, 64, 8, 2, 1,
         [mc.smooth(0, WJ, 1, 2. / 3., 1), mc.smooth(0, MC, 1, 1.0, 1), mc.residual_restrict(0, 1), mc.prolong_correct(0, 1),
          mc.vcycle(2, 2, WJ, 2. / 3., 1, nuc=2), mc.vcycle(2, 2, MC, 1.0, 1, nuc=2), mc.vcycle(2, 2, MC, 1.0, 1, nuc=2)],
         mc._vk(1) + mc._vk(1, 1, (F,))),
    # one level: the 27 planes in the coarsest level's band matrix
    Case("tensor3d_8_single_level", _tensor3d, 8, 8, 3, 2,
         [mc.smooth(0, WJ, 2, 2. / 3., 2), mc.smooth(0, MC, 1, 1.0, 2), mc.apply(0, (V, 0), (T, 1)), mc.coarse_solve(2),
          mc.vcycle(2, 2, WJ, 2. / 3., 2, nuc=2), mc.vcycle(2, 2, MC, 1.0, 2, nuc=2)],
         mc._vk(2) + [(0, T, 1)]),
]
CASE_IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_guarded_run_is_clean_and_bit_identical_3d_stencil(guard, case):
    """no red zone touched, no copy out of range, finite results equal to the unguarded run's bit for bit"""
    mc.test_guarded_run_is_clean_and_bit_identical(guard, case)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_halo_and_padding_stay_zero_3d_stencil(guard, case):
    """halo planes and column padding stay exact zeros, columns q >= k and every vector an entry does not name are untouched"""
    p = case.plan()
    try:
        assert p.level_path_3d(0) == (_lib.PATH3D_SEVEN_PLANES, case.g == 64)
        if p.num_levels > 1:
            assert p.level_path_3d(1) == (_lib.PATH3D_PLANES, False)
    finally:
        p.close()
    mc.test_halo_and_padding_stay_zero(guard, case)


@pytest.mark.parametrize("g,lowest", [(16, 4), (64, 8), (8, 8)])
@pytest.mark.parametrize("kind,omega", [(WJ, 2. / 3.), (MC, 1.0)])
def test_repeated_cycle_reproduces_the_first_3d_stencil(guard, g, lowest, kind, omega):
    """plan creation under the guard, then the same V(2,2) cycle three times on one plan (eager, captured, replayed) from the same
    start: bit-identical results"""
    guard.enable(True)
    from multigridcmt_amd.plan import Plan
    p = None
    try:
        p = Plan(_tensor3d(g), lowest, nvec=2)
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
