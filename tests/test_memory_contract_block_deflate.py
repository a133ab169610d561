"""Memory contract of mgcmt_block_deflate (csrc/kernels_blockwide.hip: k_block_cross, k_block_deflate) under the emulated
runtime's guard mode: the checks and the case machinery of tests/test_memory_contract.py, as
tests/test_memory_contract_block_wide.py uses them, on a 32^2 and a 16^3 plan with nq = 33 (three tiles, the third with one
vector) and k = 5.

The per-workgroup partial tiles and the summed tiles (the coefficients pass 2 reads) are blocks of the plan's own, allocated on
first use: red zones round them, and their NaN payloads show a tile read before it was written, a partial sum beyond the
launch's blocks, a coefficient row beyond nq.  Then drivers.deflated_eigensolve with 20 states at 32^2 with the guard on:
clean and finite."""
import numpy as np
import pytest

import test_memory_contract as mc
from test_memory_contract import MC, F, V, W, Case, Guard


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


def block_deflate(l, q, w, want_coeffs):
    return mc.Step("block_deflate(l=%d,nq=%d,k=%d,coeffs=%d)" % (l, len(q), len(w), want_coeffs),
                   lambda p: p.block_deflate(l, q, w, want_coeffs=want_coeffs), lambda p: {(l,) + tuple(v) for v in w})


K = 20                                                   # columns of V and F the case machinery fills on the start levels
_Q33 = [(V, q) for q in range(20)] + [(F, q) for q in range(13)]
_W5 = [(F, 13 + j) for j in range(5)]

CASES = [
    # 32^2 (16 block steps: more blocks than one) and its 16^2 level; with the coefficients coming back and without; after a
    # cycle has exchanged the V / T storage
    Case("deflate_2d", mc._lap2d, 32, 4, 48, K,
         [block_deflate(0, _Q33, _W5, True), block_deflate(1, _Q33, _W5, False), mc.vcycle(1, 1, MC, 1.0, 4, nuc=1),
          block_deflate(0, _Q33, _W5, False), block_deflate(0, _Q33[:1], _W5[:1], True)],
         [(0,) + v for v in _W5] + [(1,) + v for v in _W5] + mc._vk(4), init_levels=(0, 1)),
    # a 3-D plan: 16^3 = 4096 points
    Case("deflate_3d", mc._lap3d, 16, 4, 48, K, [block_deflate(0, _Q33, _W5, True), block_deflate(0, _Q33, _W5, False)], [(0,) + v for v in _W5]),
]
CASE_IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_guarded_run_is_clean_and_bit_identical_block_deflate(guard, case):
    """no red zone touched, no copy out of range, finite results equal to the unguarded run's bit for bit"""
    mc.test_guarded_run_is_clean_and_bit_identical(guard, case)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_halo_and_padding_stay_zero_block_deflate(guard, case):
    """halo rows / planes and column padding stay exact zeros; every vector other than the k named W is bitwise unchanged"""
    mc.test_halo_and_padding_stay_zero(guard, case)


def test_guarded_deflated_eigensolve(guard):
    """drivers.deflated_eigensolve with 20 states at 32^2 (locks, refills, deflations against 1 to 19 vectors) with the guard
    on: no violation, nothing left behind, finite results"""
    from multigridcmt_amd import drivers, plan
    from multigridcmt_amd.operators import laplacian_operator
    op = laplacian_operator(32, "2d") * (-1 / np.pi ** 2)
    guard.enable(True)
    info = {}
    vals, vecs = drivers.deflated_eigensolve(op, 20, lowest=4, info=info)
    assert guard.take() == []
    plan.release_plans()
    assert guard.take() == [] and guard.live() == 0
    assert info["status"] == "converged"
    assert np.all(np.isfinite(vals)) and np.all(np.isfinite(vecs)) and np.all(np.isfinite(info["residuals"]))
