"""The entries of the Schroedinger-Poisson loop and the loop itself at sizes a user runs (GPU only; a few seconds each):
mgcmt_block_density at 2048^2 with 64 vectors (two trips of every workgroup through its grid-stride loop),
mgcmt_plan_set_point_diagonal at 2048^2 and 128^3, drivers.schroedinger_poisson at 256^2."""
import numpy as np
import pytest

import scf_reference as ref
from multigridcmt_amd import _lib, drivers
from multigridcmt_amd.operators import potential_operator
from multigridcmt_amd.plan import Plan
from scf_reference import gamma

pytestmark = pytest.mark.gpu
F, W = _lib.SLOT_F, _lib.SLOT_W


def test_block_density_2048_squared(hip_only):
    """nq = 64 at 2048^2: within gamma_(nq+2) sum |w_t| x_t^2 (tests/test_block_density.py) of the np.longdouble sum on a seeded
    sample of 2^16 points and on the first and the last 1024.  The 64 vectors are combinations of two uploaded ones, formed on
    the device and downloaded at the sampled points' expense only: what the reference squares is what the kernel read."""
    g, nq = 2048, 64
    p = Plan(potential_operator(g, np.zeros((g, g))), 64, nvec=33)
    try:
        n = p.size(0)
        rng = np.random.RandomState(3)
        xs = [((W, F)[t % 2], t // 2) for t in range(nq)]
        dst = (W, 32)
        p.upload(0, *xs[0], rng.standard_normal(n))
        p.upload(0, *xs[1], rng.standard_normal(n))
        for t, v in enumerate(xs[2:], start=2):
            p.lincomb(0, [(np.cos(t), xs[0]), (np.sin(3 * t), xs[1])], v)
        w = rng.standard_normal(nq) * 10.0 ** rng.randint(-3, 4, size=nq)
        w[2::5] = 0.0
        p.block_density(0, xs, w, dst)
        got = np.array(p.download(0, *dst))
        sample = np.unique(np.concatenate([np.arange(1024), np.arange(n - 1024, n), rng.randint(0, n, size=2 ** 16)]))
        hx = np.stack([np.array(p.download(0, *v))[sample] for v in xs], axis=1)
        xl = hx.astype(np.longdouble)
        exact, scale = (xl * xl) @ w.astype(np.longdouble), (hx * hx) @ np.abs(w)
        err = np.abs(got[sample].astype(np.longdouble) - exact)
        print("2048^2 nq=64: max err/bound %.3f on %d points" % (float((err / (gamma(nq + 2) * scale)).max()), sample.size))
        assert np.all(np.isfinite(got)) and np.all(err <= gamma(nq + 2) * scale)
        p.fill(0, dst[0], dst[1], np.nan)
        p.block_density(0, xs, w, dst)
        assert np.array_equal(np.array(p.download(0, *dst)), got)
    finally:
        p.close()


@pytest.mark.parametrize("dim,g,lowest", [(2, 2048, 64), (3, 128, 8)], ids=["2048_squared", "128_cubed"])
def test_set_point_diagonal_full_size(hip_only, dim, g, lowest):
    """a point-diagonal plan (nvec = 2, so that two plans fit) whose diagonal becomes V_ext + c phi: the planes of every level
    are bit-equal to those of a plan created from that diagonal"""
    rng = np.random.RandomState(5)
    shape = (g,) * dim
    t = (np.arange(g) + 0.5) / g
    v1 = 30.0 * np.add.outer(t, t) if dim == 2 else 30.0 * np.add.outer(np.add.outer(t, t), t)
    a = b = None
    try:
        a = Plan(potential_operator(g, v1, dimension="%dd" % dim), lowest, nvec=2)
        a.upload(0, W, 0, v1 + rng.rand(*shape))
        a.upload(0, W, 1, rng.standard_normal(shape))
        a.set_point_diagonal([(1.0, (W, 0)), (0.37, (W, 1))])
        D = a.point_stencil(0)
        b = Plan(potential_operator(g, D, dimension="%dd" % dim), lowest, nvec=2)
        for l in range(a.num_levels):
            assert np.array_equal(a.point_stencil(l), b.point_stencil(l)), l
    finally:
        for p in (a, b):
            if p is not None:
                p.close()


def test_driver_256_squared(hip_only):
    """The dot of tests/test_schroedinger_poisson.py on 256^2 points with 8 states (occupations [2, 2, 2, 0, ...]) and the same
    coupling strength — the states have unit 2-norm, so the density per grid point falls as h^2 = (g + 1)^-2 and the same
    physical coupling is 800 (257 / 33)^2 (the restatement at 64^2 with 800 (65 / 33)^2 takes the 8 steps of the 32^2 one, with
    changes within 20 % of it step by step) —: it converges at tol = 1e-6, and — a MESH-INDEPENDENCE EXPECTATION: the fixed-point map phi -> phi_new is a
    property of the continuous problem, which the 32^2 and the 256^2 grid both resolve, so its contraction and with it the
    number of steps should not depend on the mesh — its number of steps is within one of the 32^2 restatement's count for the
    same coupling (8; DESIGN.md par. 4.23 records the count measured here)."""
    op32, pop32 = ref.case_2d(32)
    count = len(ref.restatement(op32, pop32, 6, [2, 2, 2, 0, 0, 0], 800.0, 1.0, 1e-6)[2])
    op, pop = ref.case_2d(256)
    info = {}
    vals, vecs, phi = drivers.schroedinger_poisson(op, pop, 8, [2, 2, 2, 0, 0, 0, 0, 0], coupling=800.0 * (257.0 / 33.0) ** 2, tol=1e-6, lowest=8,
                                                   info=info)
    print("256^2: iterations %d (32^2 restatement: %d), changes %s, eigen_iterations %s, poisson_iterations %s, eigenvalues %s"
          % (info["iterations"], count, ["%.3e" % d for d in info["changes"]], info["eigen_iterations"], info["poisson_iterations"], vals))
    assert info["status"] == "converged" and info["eigen_status"] == ["converged"] * info["iterations"]
    assert abs(info["iterations"] - count) <= 1
    assert np.all(np.isfinite(vals)) and np.all(np.isfinite(vecs)) and np.all(np.isfinite(phi))
