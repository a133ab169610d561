"""Memory contract of the carrying two-level up pass (csrc/fused2_kernel.h: CARRY, MGCMT_OPT_CARRY) under the emulated
runtime's guard mode: the checks and the case machinery of tests/test_memory_contract.py.

Four V(2,2) and four V(1,2) weighted-Jacobi cycles in a row at 128^2 (two windows) and 256^2 (three), three columns of
four, short chunks: the first cycle ends in the carrying pass, the others start from what it left in T[1] and end in it
again.  Red zones round every device block, NaN payloads: the pass's clamped loads and its predicated stores of the carried
rows stay inside their blocks, every result is finite and equal to the unguarded run's bit for bit.  (The halo-row case of
test_memory_contract.py takes raw addresses with mgcmt_vec_ptr, which turns carrying off: it has no place here.)"""
import numpy as np
import pytest

import test_memory_contract as mc
from multigridcmt_amd import _lib
from test_memory_contract import WJ, F, V, Case, Guard


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


OPTIONS = {_lib.OPT_TWO_LEVEL: 2, _lib.OPT_CARRY: 2, _lib.OPT_FUSED_ROWS: 22}


def _case(g, nu1):
    steps = [mc.vcycle(nu1, 2, WJ, 2. / 3., 3, nuc=2) for _ in range(4)]
    return Case("carry_%d_nu%d" % (g, nu1), mc._lap2d, g, 8, 4, 3, steps, mc._vk(3) + mc._vk(3, 1, (F,)), options=OPTIONS)


CASES = [_case(128, 2), _case(256, 2), _case(128, 1), _case(256, 1)]
CASE_IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_guarded_run_is_clean_and_bit_identical_carry(guard, case):
    """no red zone touched, no copy out of range, finite results equal to the unguarded run's bit for bit"""
    mc.test_guarded_run_is_clean_and_bit_identical(guard, case)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_guarded_cycles_do_carry(guard, case):
    """the cases run what they are there for: a carry is pending after every cycle, the unused column keeps its marker,
    and the guarded results are those of MGCMT_OPT_CARRY = 0"""
    guard.enable(True)
    outs = []
    for carry in (2, 0):
        p = case.plan()
        try:
            case.start(p, "emu")
            p.set_option(_lib.OPT_CARRY, carry)
            marker = np.random.RandomState(9).rand(p.size(0)) + 1.0
            p.upload(0, V, case.k, marker)
            for st in case.steps:
                st.run(p)
                assert p.carry_pending() == (carry == 2)
                assert guard.take() == [], st.label
            assert np.array_equal(p.download(0, V, case.k), marker)
            outs.append([np.array(p.download(l, s, q)) for l, s, q in case.downloads])
        finally:
            p.close()
        assert guard.take() == [] and guard.live() == 0
    for a, b in zip(*outs):
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)
