"""GPU-only checks of MGCMTSolver.solve_matrix (the batched conjugate-gradient solve, mgcmt_pcg_*_k) at sizes where every pass
runs many workgroups per column, the marching direction pass several column groups and row chunks per column, and the k-column
cycle its fused paths and the dense tail.

2048^2 Laplacian, k = 4, shifts (0, 1.9, 3.0, 1.9), rtol = 1e-8: each column converges within the count of the NumPy reference
at 32^2 for its shift plus MARGIN = 4 (the rule of tests/test_pcg_full_size_gpu.py), and is, bit for bit, ``solve`` run alone on
that column.  128^3 variable-mass ball, k = 2: the same equality."""
import numpy as np
import pytest
import scipy.sparse as sp

from multigridcmt_amd import laplacian_operator, variable_mass_operator
from oracle.sparse_ref import RefSolver, RefStencilMaker
from test_pcg import SCALE, disc_mass, ref_pcg
from test_pcg_full_size_gpu import MARGIN, RTOL
from test_pcg_matrix import assert_columns_are_the_single_solves, check_marching_against_generic_k, run_matrix

pytestmark = pytest.mark.gpu
SHIFTS = (0.0, 1.9, 3.0, 1.9)


@pytest.fixture(autouse=True, scope="module")
def _release_host_buffers():
    yield
    import gc
    from multigridcmt_amd import hostmem, plan
    plan.release_plans()
    gc.collect()
    hostmem.drain()


def _reference_count(shift, smoother, g=32):
    """iterations of the NumPy reference (the oracle's cycle as the preconditioner) to RTOL on the small grid"""
    A = (laplacian_operator(g, "2d") * SCALE).tocsr()
    n = A.shape[0]
    f = np.random.RandomState(1).rand(n)
    ref, rsm = RefSolver(), RefStencilMaker()
    smo = None if smoother == "wjacobi" else (lambda v, f, A, nu=4: ref.gseidel_mc(v, f, A, nu=nu, dimension="2d"))

    def cycle(r):
        return np.asarray(ref.vcycle(np.zeros(n), r.copy(), A, rsm, nu1=2, nu2=2, smoother=smo, shift=shift, lowest_level=4, dimension="2d"),
                          dtype=float).reshape(-1)
    return len(ref_pcg((A - shift * sp.identity(n)).tocsr(), f, cycle, RTOL, 60, smoother != "wjacobi")[1])


@pytest.mark.parametrize("smoother", ["wjacobi", "rb"])
def test_four_shifts_at_2048(hip_only, smoother):
    g = 2048
    op = laplacian_operator(g, "2d") * SCALE
    F = np.random.RandomState(1).rand(g * g, len(SHIFTS))
    X, info = run_matrix(op, F, SHIFTS, smoother, rtol=RTOL, maxiter=60)
    counts = [_reference_count(shift, smoother) for shift in SHIFTS]
    print("%s: iterations %s at 2048^2, reference %s at 32^2, true residuals %s" % (smoother, info["iterations"], counts,
                                                                                  ["%.2e" % t for t in info["true_residual"]]))
    assert X.shape == F.shape and np.all(np.isfinite(X))
    assert info["status"] == ["converged"] * len(SHIFTS) and max(info["true_residual"]) <= 2e-8
    for done, count in zip(info["iterations"], counts):
        assert done <= count + MARGIN
    assert_columns_are_the_single_solves(op, F, SHIFTS, smoother, X, info, rtol=RTOL, maxiter=60)


@pytest.mark.parametrize("opname", ["lap", "well"])
def test_marching_and_generic_paths_agree_2048(hip_only, opname):
    """2048^2: four column groups of 256 threads and 64 row chunks per column, three columns with three shifts"""
    check_marching_against_generic_k(2048, opname)


@pytest.mark.parametrize("smoother", ["wjacobi", "rb"])
def test_variable_mass_ball_at_128(hip_only, smoother):
    """two right-hand sides, the second with a shift of its own (negative: the system stays definite)"""
    g, shifts = 128, (0.0, -0.5)
    op = variable_mass_operator(g, disc_mass(g, dimension="3d"), dimension="3d")
    F = np.random.RandomState(1).rand(g ** 3, 2)
    X, info = run_matrix(op, F, shifts, smoother, dimension="3d", rtol=RTOL, maxiter=60)
    print("%s: iterations %s at 128^3, true residuals %s" % (smoother, info["iterations"], ["%.2e" % t for t in info["true_residual"]]))
    assert info["status"] == ["converged"] * 2 and max(info["true_residual"]) <= 2e-8
    assert_columns_are_the_single_solves(op, F, shifts, smoother, X, info, dimension="3d", rtol=RTOL, maxiter=60)
