"""mgcmt_copy_across (csrc/plan.hip): one level vector's interior from a plan to another plan of the same dimension and level
shape — bit-equal, between plans of different nvec and operator kind, in 2-D and 3-D, on levels 0 and 1; the neighbours of the
destination, NaN before the call, stay NaN; plans whose level differs in shape or whose dimension differs are refused."""
import numpy as np
import pytest

from multigridcmt_amd import _lib
from multigridcmt_amd.operators import laplacian_operator, potential_operator, variable_mass_operator
from multigridcmt_amd.plan import Plan

V, F, T, W = _lib.SLOT_V, _lib.SLOT_F, _lib.SLOT_T, _lib.SLOT_W
SCALE = -1 / np.pi ** 2


def _pair(dim):
    """a plan with a per-point diagonal and 5 vectors, a plan with bonds (2-D) / without a per-point part (3-D) and 3 vectors"""
    rng = np.random.RandomState(41)
    if dim == 2:
        g = 32
        return Plan(potential_operator(g, rng.rand(g, g)), 4, nvec=5), Plan(variable_mass_operator(g, 1.0 + rng.rand(g, g)), 8, nvec=3)
    g = 16
    return Plan(potential_operator(g, rng.rand(g, g, g), dimension="3d"), 4, nvec=5), Plan(laplacian_operator(g, "3d") * SCALE, 8, nvec=3)


@pytest.mark.parametrize("dim", (2, 3))
def test_copy_across_is_bit_equal_and_touches_nothing_else(backend, dim):
    rng = np.random.RandomState(43)
    a = b = None
    try:
        a, b = _pair(dim)
        for level in (0, 1):
            n = a.size(level)
            assert b.size(level) == n
            nan = np.full(n, np.nan)
            for p in (a, b):
                for s in (V, F, T, W):
                    for q in range(p.nvec):
                        p.upload(level, s, q, nan)
            x, y = rng.standard_normal(n), rng.standard_normal(n)
            a.upload(level, W, 3, x)
            a.copy_across(level, (W, 3), b, (F, 1))                 # there ...
            assert np.array_equal(np.array(b.download(level, F, 1)), x)
            b.upload(level, V, 2, y)
            b.copy_across(level, (V, 2), a, (F, 0))                 # ... and back, first column of a slot
            assert np.array_equal(np.array(a.download(level, F, 0)), y)
            a.copy_across(level, (F, 0), a, (T, 4))                 # within one plan, last column
            assert np.array_equal(np.array(a.download(level, T, 4)), y)
            assert np.array_equal(np.array(a.download(level, W, 3)), x) and np.array_equal(np.array(b.download(level, V, 2)), y)
            named = {(id(a), W, 3), (id(a), F, 0), (id(a), T, 4), (id(b), F, 1), (id(b), V, 2)}
            for p in (a, b):
                for s in (V, F, T, W):
                    for q in range(p.nvec):
                        if (id(p), s, q) not in named:
                            assert np.all(np.isnan(np.array(p.download(level, s, q)))), (level, s, q)
    finally:
        for p in (a, b):
            if p is not None:
                p.close()


def test_copy_across_refusals(backend):
    """MGCMT_ERR_INVALID: another grid size, another dimension (with the same number of points on the level), a level one of the
    plans does not have, vectors outside either plan, the same vector as source and destination, a null plan"""
    assert "mgcmt_copy_across" in _lib.EXPORTED_SYMBOLS
    plans = []
    try:
        a = Plan(laplacian_operator(64, "2d") * SCALE, 8, nvec=2)
        b = Plan(laplacian_operator(32, "2d") * SCALE, 8, nvec=2)
        c = Plan(laplacian_operator(16, "3d") * SCALE, 8, nvec=2)          # 16^3 = 64^2 points
        d = Plan(laplacian_operator(4096, "1d") * SCALE, 8, nvec=2)        # 4096 = 64^2 points
        e = Plan(laplacian_operator(64, "2d") * SCALE, 32, nvec=2)         # the same grid, two levels
        plans = [a, b, c, d, e]
        assert a.size(0) == c.size(0) == d.size(0)

        def refused(src, level, s, dst, t, message):
            with pytest.raises(_lib.MgcmtError) as err:
                src.copy_across(level, s, dst, t)
            assert "mgcmt error -1:" in str(err.value) and message in str(err.value), str(err.value)
        refused(a, 0, (V, 0), b, (V, 0), "the level's shape differs")
        refused(a, 1, (V, 0), b, (V, 0), "the level's shape differs")
        refused(a, 0, (V, 0), c, (V, 0), "differ in dimension")
        refused(d, 0, (V, 0), a, (V, 0), "differ in dimension")
        refused(a, 2, (V, 0), e, (V, 0), "level out of range")
        refused(e, 2, (V, 0), a, (V, 0), "level out of range")
        refused(a, 0, (V, 2), e, (V, 0), "vector index out of range")
        refused(a, 0, (V, 0), e, (V, 2), "vector index out of range")
        refused(a, 0, (4, 0), e, (V, 0), "slot out of range")
        refused(a, 0, (F, 1), a, (F, 1), "the same vector")
        L = _lib.lib()
        assert L.mgcmt_copy_across(None, 0, V, 0, a._h, V, 0, None) == -1 and L.mgcmt_copy_across(a._h, 0, V, 0, None, V, 0, None) == -1
        a.copy_across(1, (V, 0), e, (F, 1))                                # the same shape, plans of different depth: runs
    finally:
        for p in plans:
            p.close()
