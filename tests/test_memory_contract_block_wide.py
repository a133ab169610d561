"""Memory contract of the wide block entries (csrc/kernels_blockwide.hip: mgcmt_block_pencil, mgcmt_block_combine_wide) under
the emulated runtime's guard mode: the checks and the case machinery of tests/test_memory_contract.py on plans that store 48
vectors per slot.

The pencil's per-workgroup partial tiles, its summed tiles and the combine's coefficient / pointer table are blocks of the
plan's own, allocated on first use: red zones round them and NaN payloads show a tile read before it was written, a partial
sum beyond the launch's blocks, a table entry that was not staged.  Then a 13-state block_eigensolve at 32^2 (48-vector slots,
pencils of 26 and 39 vectors, every combine aliasing) with the guard on: clean, finite, bit-identical to the unguarded run."""
import numpy as np
import pytest

import test_memory_contract as mc
from multigridcmt_amd import _lib
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


def block_pencil(l, s, a_s, m_s=None):
    return mc.Step("block_pencil(l=%d,m=%d%s)" % (l, len(s), ",ms" if m_s else ""), lambda p: p.block_pencil(l, s, a_s, m_s), lambda p: set())


def block_combine_wide(l, inputs, outputs, coeffs):
    return mc.Step("block_combine_wide(l=%d,%d->%d)" % (l, len(inputs), len(outputs)), lambda p: p.block_combine_wide(l, inputs, outputs, coeffs),
                   lambda p: {(l,) + tuple(v) for v in outputs})


K = 20                                                   # columns of V and F the case machinery fills on the start levels
_S39 = [(V, q) for q in range(20)] + [(F, q) for q in range(19)]
_AS39 = [(F, q) for q in range(20)] + [(V, q) for q in range(19)]
_C = np.random.RandomState(3).standard_normal((48, 16))
_OUT = [(W, 30 + j) for j in range(16)]

CASES = [
    # 32^2 (16 block steps: more blocks than one) and its 16^2 level; 1, 2 and 3 tiles per side, with and without a third list
    Case("wide_2d", mc._lap2d, 32, 4, 48, K,
         [block_pencil(0, _S39, _AS39), block_pencil(0, _S39[:17], _AS39[:17], _S39[20:37]), block_pencil(1, _S39[:5], _AS39[:5]),
          block_pencil(0, _S39, _AS39, _AS39[::-1]),
          block_combine_wide(0, _S39, _OUT, _C[:39]), block_combine_wide(1, _S39[:13], _OUT[:5], _C[:13, :5]),
          block_combine_wide(0, _S39[:5] + _AS39[:5], _S39[:5], np.vstack([_C[:5, :5], np.eye(5)])),       # [X | P] -> X
          block_pencil(0, _OUT, _S39[:16]), mc.vcycle(1, 1, MC, 1.0, 4, nuc=1), block_pencil(0, _S39[:16], _AS39[:16])],
         [(0, W, 30 + j) for j in range(16)] + [(1, W, 30 + j) for j in range(5)] + mc._vk(5), init_levels=(0, 1)),
    # a 3-D plan: 16^3 = 4096 points
    Case("wide_3d", mc._lap3d, 16, 4, 48, K,
         [block_pencil(0, _S39, _AS39), block_combine_wide(0, _S39[:33], _OUT, _C[:33]), block_pencil(0, _OUT[:7], _OUT[:7], _S39[:7])],
         [(0, W, 30 + j) for j in range(16)]),
]
CASE_IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_guarded_run_is_clean_and_bit_identical_block_wide(guard, case):
    """no red zone touched, no copy out of range, finite results equal to the unguarded run's bit for bit"""
    mc.test_guarded_run_is_clean_and_bit_identical(guard, case)


@pytest.mark.parametrize("case", CASES[:1], ids=CASE_IDS[:1])
def test_halo_and_padding_stay_zero_block_wide(guard, case):
    """halo rows and column padding stay exact zeros; every vector an entry does not name as an output is untouched"""
    mc.test_halo_and_padding_stay_zero(guard, case)


def test_guarded_wide_eigensolve(guard):
    """drivers.block_eigensolve with 13 states at 32^2, guard off and on: no violation, nothing left behind, finite and
    bit-identical results"""
    from multigridcmt_amd import drivers, plan
    from multigridcmt_amd.operators import laplacian_operator
    op = laplacian_operator(32, "2d") * (-1 / np.pi ** 2)
    runs = []
    for on in (False, True):
        guard.enable(on)
        res = []
        vals, vecs = drivers.block_eigensolve(op, k=13, cycles=4, lowest=4, residuals=res)
        assert guard.take() == []
        plan.release_plans()
        assert guard.take() == [] and guard.live() == 0
        runs.append((vals, vecs, np.array(res)))
    for x in runs[1]:
        assert np.all(np.isfinite(x))
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
