"""Anderson mixing at sizes a user runs (GPU only; a few seconds each): drivers.schroedinger_poisson with mixing_history = 5 at
256^2 next to the plain loop of tests/test_schroedinger_poisson_full_size_gpu.py, and mgcmt_mix_residual / mgcmt_mix_combine at
2048^2 with nine pairs — 2^21 double2 elements: four trips of every thread of the residual pass through its slice (2048 slices),
four trips of every workgroup of the combine pass through its grid-stride loop."""
import numpy as np
import pytest

import scf_reference as ref
from multigridcmt_amd import _lib, drivers
from multigridcmt_amd.operators import potential_operator
from multigridcmt_amd.plan import Plan
from scf_reference import gamma
from test_mix_kernels import U, chain_length

pytestmark = pytest.mark.gpu
F, W = _lib.SLOT_F, _lib.SLOT_W


def test_driver_256_squared_with_mixing_history(hip_only):
    """The 256^2 run of tests/test_schroedinger_poisson_full_size_gpu.py (8 states, coupling 800 (257 / 33)^2, mixing = 1) with
    mixing_history = 5: it converges, in no more steps than the plain run of the same configuration, to the same potential
    (2 tol: both stopped with d <= tol at a contraction of about 0.15).  DESIGN.md par. 4.24 records both counts."""
    op, pop = ref.case_2d(256)
    kw = dict(coupling=800.0 * (257.0 / 33.0) ** 2, tol=1e-6, lowest=8)
    plain, mixed = {}, {}
    _, _, phi0 = drivers.schroedinger_poisson(op, pop, 8, [2, 2, 2, 0, 0, 0, 0, 0], info=plain, **kw)
    vals, vecs, phi = drivers.schroedinger_poisson(op, pop, 8, [2, 2, 2, 0, 0, 0, 0, 0], mixing_history=5, info=mixed, **kw)
    print("256^2: plain %d steps, mixing_history=5 %d steps; changes %s; depths %s; restarts %s"
          % (plain["iterations"], mixed["iterations"], ["%.3e" % d for d in mixed["changes"]], mixed["mixing_depths"], mixed["mixing_restarts"]))
    assert plain["status"] == "converged" and mixed["status"] == "converged"
    assert mixed["iterations"] <= plain["iterations"]
    assert mixed["eigen_status"] == ["converged"] * mixed["iterations"] and mixed["poisson_status"] == ["converged"] * mixed["iterations"]
    assert np.all(np.isfinite(vals)) and np.all(np.isfinite(vecs)) and np.all(np.isfinite(phi))
    assert np.linalg.norm(phi - phi0) <= 2e-6 * np.linalg.norm(phi0)


def test_mix_kernels_2048_squared(hip_only):
    """p = 9 at 2048^2.  The vectors are combinations of two uploaded ones, formed on the device and downloaded: what the
    reference uses is what the kernels read.  r bit-equal to out - in on every point; the ten inner products within the chain
    bound of tests/test_mix_kernels.py (D = 36) of the np.longdouble sums over all points; the combination within
    gamma_19 sum |alpha_i| (|x_i| + |beta r_i|) on a seeded sample of 2^16 points and on the first and the last 1024; a second
    call of each bit-identical."""
    g, pairs = 2048, 9
    p = Plan(potential_operator(g, np.zeros((g, g))), 64, nvec=11)
    try:
        n = p.size(0)
        rng = np.random.RandomState(7)
        xs, rs = [(W, t) for t in range(pairs)], [(F, t) for t in range(pairs)]
        out, inp, dst = (W, 9), (W, 10), (F, 9)
        p.upload(0, *xs[0], rng.standard_normal(n))
        p.upload(0, *xs[1], rng.standard_normal(n) * 10.0 ** rng.randint(-2, 3, size=n))
        for t, v in enumerate(xs[2:] + rs[:8] + [out, inp], start=2):
            p.lincomb(0, [(np.cos(t), xs[0]), (np.sin(3 * t), xs[1])], v)
        prev = rs[:8]
        sums = p.mix_residual(0, out, inp, rs[8], prev)
        r = np.array(p.download(0, *rs[8]))
        ho = np.array(p.download(0, *out))
        assert np.array_equal(r, ho - np.array(p.download(0, *inp)))
        D, rl, worst = chain_length(n), r.astype(np.longdouble), 0.0
        assert D == 36
        for j, y in enumerate([np.array(p.download(0, *v)) for v in prev] + [r, None]):
            a, b = (ho.astype(np.longdouble),) * 2 if y is None else (rl, y.astype(np.longdouble))
            exact, mag = (a * b).sum(), float(np.abs(a * b).sum())
            err = abs(float(np.longdouble(sums[j]) - exact))
            assert err <= D * U * mag, (j, err / (U * mag), D)
            worst = max(worst, err / (D * U * mag))
        print("2048^2 residual nprev=8: worst err / bound %.3f (D = %d)" % (worst, D))
        p.fill(0, rs[8][0], rs[8][1], np.nan)
        assert np.array_equal(p.mix_residual(0, out, inp, rs[8], prev), sums) and np.array_equal(np.array(p.download(0, *rs[8])), r)
        alpha, beta = rng.standard_normal(pairs) * 2.0, 0.5
        alpha[-1] += 1.0 - alpha.sum()
        p.mix_combine(0, xs, rs, alpha, beta, dst)
        got = np.array(p.download(0, *dst))
        sample = np.unique(np.concatenate([np.arange(1024), np.arange(n - 1024, n), rng.randint(0, n, size=2 ** 16)]))
        hx = np.stack([np.array(p.download(0, *v))[sample] for v in xs], axis=1)
        hr = np.stack([np.array(p.download(0, *v))[sample] for v in rs], axis=1)
        exact = (hx.astype(np.longdouble) + np.longdouble(beta) * hr.astype(np.longdouble)) @ alpha.astype(np.longdouble)
        scale = (np.abs(hx) + np.abs(beta * hr)) @ np.abs(alpha)
        err = np.abs(got[sample].astype(np.longdouble) - exact)
        print("2048^2 combine p=9: max err/bound %.3f on %d points" % (float((err / (gamma(2 * pairs + 1) * scale)).max()), sample.size))
        assert np.all(np.isfinite(got)) and np.all(err <= gamma(2 * pairs + 1) * scale)
        p.mix_combine(0, xs, rs, alpha, beta, xs[0])                               # into the oldest x's column: the same bits
        assert np.array_equal(np.array(p.download(0, *xs[0])), got)
    finally:
        p.close()
