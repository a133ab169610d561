"""Two-level fused passes (csrc/fused2_kernel.h, MGCMT_OPT_TWO_LEVEL): a constant 5-point level and its Galerkin level
below in one down-leg and one up-leg launch must give the bits of the four single-level passes they replace.  Both
backends."""
import numpy as np
import pytest

from multigridcmt_amd import _lib
from multigridcmt_amd.operators import laplacian_operator, potential_well_operator
from multigridcmt_amd.plan import Plan

SCALE = -1 / np.pi ** 2


def _cycles(op, g, two_level, nus, k=1, rows=0, zero_start=False, kind=_lib.WJACOBI, omega=2. / 3., gs=False, seed=3):
    """V[0] and F[1] after two cycles, and whether V[1] (filled with a marker first) was left untouched"""
    nu1, nu2, nuc = nus
    rng = np.random.RandomState(seed)
    p = Plan(op, 8, nvec=k)
    p.set_option(_lib.OPT_TWO_LEVEL, two_level)
    p.set_option(_lib.OPT_FUSED_ROWS, rows)
    p.set_shifts(0.4 + 0.15 * np.arange(k))
    n1 = (g // 2) ** 2
    marker = rng.rand(n1) + 7.0
    for q in range(k):
        p.upload(0, _lib.SLOT_V, q, rng.rand(g * g))
        p.upload(0, _lib.SLOT_F, q, rng.rand(g * g))
        p.upload(1, _lib.SLOT_V, q, marker)
    for it in range(2):
        if zero_start and it == 0:
            for q in range(k):
                p.upload(0, _lib.SLOT_V, q, rng.rand(g * g) * 1e3)    # garbage the flagged cycle must not read
        p.vcycle(nu1, nu2, kind, omega=omega, k=k, nu_coarse=nuc, gram_schmidt=gs, zero_start=zero_start and it == 0)
    v = np.stack([p.download(0, _lib.SLOT_V, q) for q in range(k)])
    f1 = np.stack([p.download(1, _lib.SLOT_F, q) for q in range(k)])
    untouched = all(np.array_equal(p.download(1, _lib.SLOT_V, q), marker) for q in range(k))
    p.close()
    return v, f1, untouched


def _check(op, g, nus, paired, **kw):
    a_v, a_f, a_untouched = _cycles(op, g, 2, nus, **kw)
    b_v, b_f, _ = _cycles(op, g, 0, nus, **kw)
    assert np.array_equal(a_v, b_v), (g, nus, kw)
    assert np.array_equal(a_f, b_f), (g, nus, kw)
    assert a_untouched == paired, (g, nus, kw)   # the paired up pass never writes V[1]; the fallback does


@pytest.mark.parametrize("g", [128, 256, 512])
def test_two_level_bit_identical(backend, g):
    op = laplacian_operator(g, "2d") * SCALE
    for nus in ((2, 2, 2), (1, 2, 2), (3, 2, 2), (4, 4, 2)):
        _check(op, g, nus, True)
    _check(op, g, (2, 2, 4), False)          # level 1 needs two passes per leg: today's passes


@pytest.mark.parametrize("rows", [6, 22, 0])
def test_two_level_columns_and_chunks(backend, rows):
    g = 256
    op = laplacian_operator(g, "2d") * SCALE
    for k, zero_start in ((3, False), (1, True), (3, True)):
        _check(op, g, (2, 2, 2), True, k=k, rows=rows, zero_start=zero_start)


def test_two_level_fallbacks(backend):
    g = 128
    op = laplacian_operator(g, "2d") * SCALE
    _check(op, g, (2, 2, 2), False, gs=True, k=2)                           # Gram-Schmidt between the up passes
    _check(op, g, (2, 2, 2), False, kind=_lib.GS_MC, omega=1.0)             # red-black
    well = potential_well_operator(g, 50.0, (g // 4, 3 * g // 4))
    _check(well, g, (2, 2, 2), False)                                       # variable coefficients
