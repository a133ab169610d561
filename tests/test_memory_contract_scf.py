"""Memory contract of the entries behind drivers.schroedinger_poisson — mgcmt_block_density (csrc/kernels_blockwide.hip:
k_block_density), mgcmt_plan_set_point_diagonal (csrc/hierarchy.hip) and mgcmt_copy_across (csrc/plan.hip) — under the emulated
runtime's guard mode: the checks and the case machinery of tests/test_memory_contract.py, as
tests/test_memory_contract_block_deflate.py uses them, on a 32^2 and a 16^3 plan with a point diagonal.

A density of 33 vectors (eight rounds of the unrolled loop and one more) into a column between two others; a new diagonal from
two vectors — the planes of every level are blocks of the plan's own with red zones round them, and the cycle and the coarse
solve that follow read them —; copies inside the plan.  Then a copy between two plans with the guard on, and one guarded run of
the driver: no violation, nothing left behind, finite results."""
import numpy as np
import pytest

import test_memory_contract as mc
from multigridcmt_amd.operators import potential_operator
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


def _point3d(g):
    return potential_operator(g, 5.0 * np.random.RandomState(19).rand(g, g, g), dimension="3d")


def block_density(l, xs, dst):
    w = np.cos(np.arange(len(xs)) + 1.0)
    return mc.Step("block_density(l=%d,nq=%d)" % (l, len(xs)), lambda p: p.block_density(l, xs, w, dst), lambda p: {(l,) + tuple(dst)})


def set_point_diagonal(terms):
    return mc.Step("set_point_diagonal(%d)" % len(terms), lambda p: p.set_point_diagonal(terms), lambda p: set())


def copy_across(l, src, dst):
    return mc.Step("copy_across(l=%d)" % l, lambda p: p.copy_across(l, src, p, dst), lambda p: {(l,) + tuple(dst)})


K = 20                                                   # columns of V and F the case machinery fills on the start levels
_X33 = [(V, q) for q in range(20)] + [(F, q) for q in range(13)]
_DST = (F, 15)
_STEPS = [block_density(0, _X33, _DST), block_density(1, _X33[:5], _DST), set_point_diagonal([(1.0, (F, 14)), (0.25, _DST)]),
          mc.vcycle(1, 1, MC, 1.0, 4, nuc=1), block_density(0, _X33[:1], (F, 16)), copy_across(0, (F, 16), (F, 17)),
          set_point_diagonal([(1.0, (F, 14))]), mc.coarse_solve(4), copy_across(1, _DST, (V, 19))]
_DOWNLOADS = [(0,) + _DST, (1,) + _DST, (0, F, 16), (0, F, 17), (1, V, 19)] + mc._vk(4)

CASES = [Case("scf_2d", mc._point, 32, 4, 48, K, _STEPS, _DOWNLOADS, init_levels=(0, 1)),
         Case("scf_3d", _point3d, 16, 4, 48, K, _STEPS, _DOWNLOADS, init_levels=(0, 1))]
CASE_IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_guarded_run_is_clean_and_bit_identical_scf(guard, case):
    """no red zone touched, no copy out of range, finite results equal to the unguarded run's bit for bit"""
    mc.test_guarded_run_is_clean_and_bit_identical(guard, case)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_halo_and_padding_stay_zero_scf(guard, case):
    """halo rows / planes and column padding stay exact zeros; every vector other than the one an entry names as its
    destination is bitwise unchanged (mgcmt_plan_set_point_diagonal writes no vector at all)"""
    mc.test_halo_and_padding_stay_zero(guard, case)


@pytest.mark.parametrize("make,g", [(mc._point, 32), (_point3d, 16)], ids=["2d", "3d"])
def test_guarded_copy_between_two_plans(guard, make, g):
    """two plans of different nvec, every block of both guarded: copies there and back on levels 0 and 1 — the last column of
    one into the first of the other — are clean and exact"""
    from multigridcmt_amd.plan import Plan
    guard.enable(True)
    a, b = Plan(make(g), 4, nvec=7), Plan(make(g), 8, nvec=2)
    try:
        for level in (0, 1):
            x = np.random.RandomState(level).rand(a.size(level))
            a.upload(level, W, 6, x)
            a.copy_across(level, (W, 6), b, (V, 0))
            b.copy_across(level, (V, 0), a, (F, 0))
            b.copy_across(level, (V, 0), b, (W, 1))
            assert guard.take() == []
            assert all(np.array_equal(np.array(p.download(level, *v)), x) for p, v in ((b, (V, 0)), (a, (F, 0)), (b, (W, 1))))
    finally:
        a.close()
        b.close()
    assert guard.take() == [] and guard.live() == 0


def test_guarded_schroedinger_poisson(guard):
    """drivers.schroedinger_poisson with the guard on — the dot of tests/test_schroedinger_poisson.py, three steps: warm starts
    from the pool, the density, both copies, the new diagonal and the solves that read it —: no violation, nothing left
    behind, finite results"""
    from multigridcmt_amd import drivers, plan
    from scf_reference import case_2d
    op, poisson_op = case_2d()
    guard.enable(True)
    info = {}
    vals, vecs, phi = drivers.schroedinger_poisson(op, poisson_op, 6, [2, 2, 2, 0, 0, 0], coupling=800.0, lowest=4, maxiter=3, info=info)
    assert guard.take() == []
    plan.release_plans()
    assert guard.take() == [] and guard.live() == 0
    assert info["iterations"] == 3 and info["status"] == "maxiter" and info["eigen_status"] == ["converged"] * 3
    assert all(np.all(np.isfinite(x)) for x in (vals, vecs, phi, info["density"], np.array(info["changes"])))
