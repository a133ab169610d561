"""Memory contract of mgcmt_block_project and mgcmt_block_orthonormalize (csrc/kernels_blockwide.hip: k_block_cross,
k_block_deflate, k_block_gram16, k_orth_factor, k_block_transform) under the emulated runtime's guard mode: the checks and the
case machinery of tests/test_memory_contract.py, as tests/test_memory_contract_block_deflate.py uses them, on a 32^2 and a 16^3
plan with nb = 17 (two tiles, the second with one vector) and k = 5, with companions and without, and one rank-deficient block
(a column copied over its neighbour: the second of the two is dropped and comes back as zeros).

The per-workgroup partial tiles, the summed tiles (the coefficients of the projection, the T of the orthonormalisation) and
the word with the dropped columns are blocks of the plan's own, allocated on first use: red zones round them, and their NaN
payloads show a tile read before it was written, a partial sum beyond the launch's blocks, a coefficient row beyond nb or k.
Then drivers.deflated_eigensolve(basis="orthonormal") with 20 states at 32^2 with the guard on: clean and finite."""
import numpy as np
import pytest

import test_memory_contract as mc
from test_memory_contract import MC, F, V, W, Case, Guard

DROP_TOL = 1e-13


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


def _named(l, *lists):
    return lambda p: {(l,) + tuple(v) for vs in lists if vs is not None for v in vs}


def block_project(l, b, w, ab, aw, want_coeffs):
    return mc.Step("block_project(l=%d,nb=%d,k=%d,companions=%d,coeffs=%d)" % (l, len(b), len(w), ab is not None, want_coeffs),
                   lambda p: p.block_project(l, b, w, ab, aw, want_coeffs=want_coeffs), _named(l, w, aw))


def block_orthonormalize(l, w, aw, want):
    def run(p):
        out = p.block_orthonormalize(l, w, aw, drop_tol=DROP_TOL, want_t=want, want_dropped=want)
        return None if out is None else np.append(out[0].ravel(), float(out[1]))       # (T and the mask as one result)
    return mc.Step("block_orthonormalize(l=%d,k=%d,companions=%d,outputs=%d)" % (l, len(w), aw is not None, want), run, _named(l, w, aw))


def copy(l, src, dst):
    return mc.Step("copy(l=%d)" % l, lambda p: p.copy(l, src[0], src[1], dst[0], dst[1]), _named(l, [dst]))


K = 28                                                   # columns of V and F the case machinery fills on the start levels
# B in V (read before the cycle only: a cycle exchanges the V / T storage), AB, W and AW in F
_B17, _AB17 = [(V, q) for q in range(17)], [(F, q) for q in range(17)]
_W5, _AW5 = [(F, 17 + j) for j in range(5)], [(F, 22 + j) for j in range(5)]
_OUT = [(0,) + v for v in _W5 + _AW5]

CASES = [
    # 32^2 (16 block steps: more blocks than one) and its 16^2 level; with companions and without, with the outputs coming back
    # and without; after a cycle has exchanged the V / T storage; a rank-deficient block last
    Case("orth_2d", mc._lap2d, 32, 4, 48, K,
         [block_project(0, _B17, _W5, _AB17, _AW5, True), block_project(1, _B17, _W5, None, None, False),
          block_orthonormalize(0, _W5, _AW5, True), block_orthonormalize(1, _W5, None, False),
          block_project(0, _B17[:1], _W5[:1], _AB17[:1], _AW5[:1], False), block_orthonormalize(0, _W5[:1], _AW5[:1], False),
          mc.vcycle(1, 1, MC, 1.0, 4, nuc=1),
          block_project(0, _AB17, _AW5, None, None, True), block_orthonormalize(0, _AW5, None, True),
          copy(0, _AB17[2], _AB17[3]), copy(0, _AB17[7], _AB17[8]), block_orthonormalize(0, _AB17[:5], _AB17[5:10], True)],
         _OUT + [(1,) + v for v in _W5] + [(0,) + v for v in _AB17[:10]] + mc._vk(4), init_levels=(0, 1)),
    # a 3-D plan: 16^3 = 4096 points
    Case("orth_3d", mc._lap3d, 16, 4, 48, K,
         [block_project(0, _B17, _W5, _AB17, _AW5, True), block_orthonormalize(0, _W5, _AW5, True),
          block_project(0, _B17, _W5, None, None, False), block_orthonormalize(0, _W5, None, False)], _OUT),
]
CASE_IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_guarded_run_is_clean_and_bit_identical_block_orth(guard, case):
    """no red zone touched, no copy out of range, finite results equal to the unguarded run's bit for bit"""
    mc.test_guarded_run_is_clean_and_bit_identical(guard, case)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_halo_and_padding_stay_zero_block_orth(guard, case):
    """halo rows / planes and column padding stay exact zeros; every vector other than the named W and AW is bitwise unchanged"""
    mc.test_halo_and_padding_stay_zero(guard, case)


def test_the_rank_deficient_step_drops_its_column(guard):
    """the last step of orth_2d: column 3 of the block is a copy of column 2 and comes back as exact zeros with its companion,
    the mask says 8"""
    case = CASES[0]
    guard.enable(True)
    p = case.plan()
    try:
        case.start(p, "emu")
        outs = dict(case.run(p))
        assert guard.take() == []
        last = outs["block_orthonormalize(l=0,k=5,companions=1,outputs=1)"]
        assert last[-1] == 8.0 and np.all(last[:-1].reshape(5, 5)[3] == 0.0) and np.all(last[:-1].reshape(5, 5)[:, 3] == 0.0)
        assert np.all(outs["download(0,%d,3)" % F] == 0.0) and np.all(outs["download(0,%d,8)" % F] == 0.0)
        assert np.any(outs["download(0,%d,2)" % F] != 0.0)
    finally:
        p.close()
    assert guard.take() == [] and guard.live() == 0


def test_guarded_orthonormal_deflated_eigensolve(guard):
    """drivers.deflated_eigensolve(basis="orthonormal") with 20 states at 32^2 (locks, refills, projections against 1 to 32
    vectors, two Cholesky-QR steps per block and iteration) with the guard on: no violation, nothing left behind, finite"""
    from multigridcmt_amd import drivers, plan
    from multigridcmt_amd.operators import laplacian_operator
    op = laplacian_operator(32, "2d") * (-1 / np.pi ** 2)
    guard.enable(True)
    info = {}
    vals, vecs = drivers.deflated_eigensolve(op, 20, lowest=4, info=info, basis="orthonormal")
    assert guard.take() == []
    plan.release_plans()
    assert guard.take() == [] and guard.live() == 0
    assert info["status"] == "converged"
    assert np.all(np.isfinite(vals)) and np.all(np.isfinite(vecs)) and np.all(np.isfinite(info["residuals"]))
    assert np.all(np.isfinite(info["gram_min"])) and info["dropped"].sum() == 0
