"""mgcmt_plan_set_point_diagonal (csrc/hierarchy.hip): a plan whose per-point diagonal is replaced on the device must hold the bits
of a plan created from that diagonal — on every level, and in everything derived from the planes (the coarse solve's
factorisation and explicit inverse, also in front of a replayed cycle graph).

For each kind of per-point part (a diagonal, bonds, a stencil; 2-D and 3-D): plan A is created with a potential V1, runs four
V(2,2) cycles with equal parameters (the first runs eagerly, the second is captured, the others replay the graph on the HIP
backend; on the emulation, where capture is a stub, the same sequence runs eagerly) and one coarse solve with a non-zero
shift, so that a factorisation is cached.  Then its diagonal becomes V_ext + c phi from two of its vectors; plan B is created from
the operator with that diagonal read back from A.  Everything below is compared bit for bit.

Shapes: 32^2 and 16^3 with lowest = 4 (flat kernels, three levels, the band and the explicit-inverse coarse solves); 128^2 for
the 2-D kinds (the fused pass of a point diagonal, the bonds' march, the nine-point tiles start at 128 columns); 64^3 for the 3-D
kinds (their marching and tile kernels need a multiple of 64) — that one on the GPU only: a 64^3 case takes minutes on the
emulation."""
import ctypes

import numpy as np
import pytest

from multigridcmt_amd import _lib
from multigridcmt_amd import plan as plan_module
from multigridcmt_amd.operators import (StructuredOperator, laplacian_operator, potential_operator, tensor_mass_operator,
                                        variable_mass_operator)
from multigridcmt_amd.plan import Plan, get_plan
from test_block_deflate import gamma

V, F, T, W = _lib.SLOT_V, _lib.SLOT_F, _lib.SLOT_T, _lib.SLOT_W
NVEC = 4
SHIFTS = [0.3, 0.1, 0.2]
COUPLING = 0.37


def _fields(g, dim, seed):
    """a smooth potential with disorder on top, and positive coefficient fields, on g^dim points"""
    rng = np.random.RandomState(seed)
    t = (np.arange(g) + 0.5) / g
    grids = np.meshgrid(*([t] * dim), indexing="ij")
    pot = 25.0 * sum((x - 0.4 - 0.1 * a) ** 2 for a, x in enumerate(grids)) + rng.rand(*([g] * dim))
    w = [1.0 + 0.4 * np.sin(2 * np.pi * grids[a]) * np.cos(2 * np.pi * grids[(a + 1) % dim]) for a in range(dim)]
    return pot, w, 0.15 * np.cos(2 * np.pi * grids[0]) * np.sin(2 * np.pi * grids[-1])


def _operator(kind, dim, g):
    pot, w, cross = _fields(g, dim, 3)
    dimension = "%dd" % dim
    if kind == "diag":
        return potential_operator(g, pot, dimension=dimension)
    if kind == "bonds":
        return variable_mass_operator(g, w[0], V=pot, dimension=dimension)
    if dim == 2:
        return tensor_mass_operator(g, w[0], w[1], cross, V=pot)
    return tensor_mass_operator(g, w[0], w[1], cross, V=pot, wzz=w[2], wxz=0.5 * cross, wyz=-0.5 * cross, dimension="3d")


def _centre(kind, dim, planes):
    """the diagonal among the planes of level 0 as Plan.point_stencil(0) returns them"""
    return planes if kind == "diag" else planes[0] if kind == "bonds" else planes[(1,) * dim]


def _with_diagonal(op, kind, dim, planes, D):
    """the operator `op` with the diagonal of its per-point part replaced by D"""
    planes = np.array(planes)
    if kind == "diag":
        planes = D
    elif kind == "bonds":
        planes[0] = D
    else:
        planes[(1,) * dim] = D
    return StructuredOperator(op.dimension, op.g, op.terms, **StructuredOperator.point_keywords(kind, planes))


def _same_planes(a, b, what):
    for l in range(a.num_levels):
        assert np.array_equal(a.point_stencil(l), b.point_stencil(l)), (what, "planes of level %d" % l)


def _same_results(a, b, what):
    """from equal start vectors and right-hand sides: vcycle (both smoothers, shifts, k = 1 and 3), apply, the coarse solve and six
    iterations of conjugate gradients, bit-equal on the two plans"""
    rng = np.random.RandomState(11)
    n, last = a.size(0), a.num_levels - 1
    f, v0 = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    fc = rng.standard_normal((a.size(last), 3))
    out = []
    for p in (a, b):
        res = []
        p.set_shifts(SHIFTS)
        for kind, omega in ((_lib.GS_MC, 1.0), (_lib.WJACOBI, 2. / 3.)):
            for k in (1, 3):
                for c in range(k):
                    p.upload(0, F, c, f[:, c])
                    p.upload(0, V, c, v0[:, c])
                p.vcycle(2, 2, kind, omega=omega, k=k)
                res += [np.array(p.download(0, V, c)) for c in range(k)]
        p.upload(0, V, 0, v0[:, 0])
        p.apply(0, (V, 0), (T, 0), with_shift=True)
        res.append(np.array(p.download(0, T, 0)))
        for c in range(3):
            p.upload(last, F, c, fc[:, c])
        p.coarse_solve(last, k=3)
        res += [np.array(p.download(last, V, c)) for c in range(3)]
        p.upload(0, F, 0, f[:, 0])
        p.pcg_begin([0, 1, 2, 3], 0.0, zero_start=True, flexible=True)
        p.pcg_iterate(6, 2, 2, _lib.GS_MC)
        assert p.pcg_status()[0] == 6
        res.append(np.array(p.download(0, W, 0)))
        out.append(res)
    assert len(out[0]) == len(out[1])
    for i, (x, y) in enumerate(zip(*out)):
        assert np.all(np.isfinite(x)) and np.array_equal(x, y), (what, "result %d" % i)


def _run_case(kind, dim, g, lowest):
    what = "%s %dd g=%d" % (kind, dim, g)
    rng = np.random.RandomState(7)
    op1 = _operator(kind, dim, g)
    part, arrays = op1.point_part()
    assert part == kind
    d1 = np.array(_centre(kind, dim, arrays[0] if kind == "planes" else arrays if kind == "bonds" else arrays[0]))
    a = b = c = None
    try:
        a = Plan(op1, lowest, nvec=NVEC)
        n, last = a.size(0), a.num_levels - 1
        a.set_shifts(SHIFTS)
        a.upload(0, F, 0, rng.standard_normal(n))
        a.fill(0, V, 0, 0.0)
        for _ in range(4):
            a.vcycle(2, 2, _lib.GS_MC, omega=1.0, k=1)
        a.coarse_solve(last, k=1)
        assert np.all(np.isfinite(np.array(a.download(0, V, 0))))
        # the new diagonal from two vectors of the plan
        v_ext, phi = d1 + 3.0 * rng.rand(*d1.shape), rng.standard_normal(d1.shape)
        a.upload(0, W, 0, v_ext)
        a.upload(0, W, 1, phi)
        assert not a.op_stale
        a.set_point_diagonal([(1.0, (W, 0)), (COUPLING, (W, 1))])
        assert a.op_stale
        planes = a.point_stencil(0)
        D = np.array(_centre(kind, dim, planes))
        exact = v_ext.astype(np.longdouble) + np.longdouble(COUPLING) * phi.astype(np.longdouble)
        bound = gamma(3) * (np.abs(v_ext) + np.abs(COUPLING * phi))
        assert np.all(np.abs(D.astype(np.longdouble) - exact) <= bound), what
        if kind != "diag":                               # bonds / the off-centre planes are the operator's still
            mask = np.ones(planes.shape[:-dim], dtype=bool)
            mask[(0,) if kind == "bonds" else (1,) * dim] = False
            assert np.array_equal(planes[mask], np.array(arrays[0] if kind == "planes" else arrays)[mask]), what
        b = Plan(_with_diagonal(op1, kind, dim, planes, D), lowest, nvec=NVEC)
        _same_planes(a, b, what)
        # A replays the graph captured before the update: the cycle it ran four times, first
        f0 = rng.standard_normal(n)
        got = []
        for p in (a, b):
            p.set_shifts(SHIFTS)
            p.upload(0, F, 0, f0)
            p.fill(0, V, 0, 0.0)
            p.vcycle(2, 2, _lib.GS_MC, omega=1.0, k=1)
            p.vcycle(2, 2, _lib.GS_MC, omega=1.0, k=1)
            got.append(np.array(p.download(0, V, 0)))
        assert np.array_equal(got[0], got[1]), (what, "the cycle of the cached graph")
        _same_results(a, b, what)
        # back to V1: the bits of the plan as it was created
        a.upload(0, W, 0, d1)
        a.set_point_diagonal([(1.0, (W, 0))])
        c = Plan(op1, lowest, nvec=NVEC)
        _same_planes(a, c, what + " restored")
        _same_results(a, c, what + " restored")
    finally:
        for p in (a, b, c):
            if p is not None:
                p.close()


KINDS = ("diag", "bonds", "planes")
SMALL = [(kind, 2, 32, 4) for kind in KINDS] + [(kind, 3, 16, 4) for kind in KINDS] + [(kind, 2, 128, 4) for kind in KINDS]


@pytest.mark.parametrize("kind,dim,g,lowest", SMALL, ids=["%s_%dd_%d" % c[:3] for c in SMALL])
def test_updated_plan_equals_fresh_plan(backend, kind, dim, g, lowest):
    _run_case(kind, dim, g, lowest)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_updated_plan_equals_fresh_plan_64_cubed(hip_only, kind):
    """the marching and tile kernels of the 3-D kinds (a multiple of 64 points per axis); GPU only, see the module docstring"""
    _run_case(kind, 3, 64, 4)


def test_set_point_diagonal_refusals(backend):
    """MGCMT_ERR_INVALID: a plan without a per-point part (the message of mgcmt_plan_get_point_stencil), null lists, nterms out of
    range, vectors outside the plan; only level-0 vectors can be named at all (the entry takes no level)"""
    assert "mgcmt_plan_set_point_diagonal" in _lib.EXPORTED_SYMBOLS
    plain = p = None
    try:
        plain = Plan(laplacian_operator(16, "2d") * (-1 / np.pi ** 2), 4, nvec=2)
        with pytest.raises(_lib.MgcmtError) as e:
            plain.set_point_diagonal([(1.0, (W, 0))])
        assert "mgcmt error -1: plan has no point diagonal" in str(e.value)
        assert not plain.op_stale
        p = Plan(_operator("diag", 2, 16), 4, nvec=2)
        L = _lib.lib()
        one, co = (ctypes.c_int * 1)(W), (ctypes.c_double * 1)(1.0)
        for args in ((None, one, one), (co, None, one), (co, one, None)):
            assert L.mgcmt_plan_set_point_diagonal(p._h, 1, args[0], args[1], args[2], None) == -1
            assert b"set_point_diagonal: 1..4 terms, non-null arguments" in L.mgcmt_last_error()
        assert L.mgcmt_plan_set_point_diagonal(None, 1, co, one, one, None) == -1

        def refused(terms, message):
            with pytest.raises(_lib.MgcmtError) as e:
                p.set_point_diagonal(terms)
            assert "mgcmt error -1:" in str(e.value) and message in str(e.value), str(e.value)
        refused([], "1..4 terms")
        refused([(1.0, (W, 0))] * 5, "1..4 terms")
        refused([(1.0, (W, 2))], "vector index out of range")
        refused([(1.0, (W, -1))], "vector index out of range")
        refused([(1.0, (4, 0))], "slot out of range")
        before = p.point_stencil(0)
        assert not p.op_stale and np.array_equal(before, _operator("diag", 2, 16).point_diagonal)      # a refused call changes nothing
        p.upload(0, W, 0, before)
        p.set_point_diagonal([(1.0, (W, 0)), (1.0, (W, 0)), (-1.0, (W, 0)), (0.0, (W, 0))])           # the limit itself runs: x, 2 x, x, x
        assert np.array_equal(p.point_stencil(0), before)
    finally:
        for q in (plain, p):
            if q is not None:
                q.close()


def test_get_plan_forgets_a_plan_whose_diagonal_was_set(backend):
    """a cached plan leaves get_plan's cache when its diagonal is set: the next caller with that operator gets a plan that
    holds the operator's own diagonal"""
    plan_module.release_plans()
    op = _operator("diag", 2, 16)
    try:
        p = get_plan(op, 4, nvec=2)
        assert get_plan(op, 4, nvec=2) is p
        p.upload(0, W, 0, np.full(p.size(0), 5.0))
        p.set_point_diagonal([(1.0, (W, 0))])
        assert p.op_stale and p not in plan_module._PLANS.values()
        q = get_plan(op, 4, nvec=2)
        assert q is not p and not q.op_stale
        assert np.array_equal(q.point_stencil(0), op.point_diagonal) and np.all(p.point_stencil(0) == 5.0)
        p.close()
    finally:
        plan_module.release_plans()
