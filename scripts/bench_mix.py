"""Anderson mixing in the Schroedinger-Poisson loop at size (DESIGN.md par. 4.24; results: profiles/r21_anderson_mixing.md).

1. mgcmt_mix_residual (k_mix_residual + k_mix_final; the call ends in a copy of p + 1 numbers to the host and a synchronisation,
   which the time includes) and mgcmt_mix_combine (k_mix_combine) between two HIP events on the null stream at 4096^2 and 256^3
   for p = 2, 6, 9 pairs against their bytes — 8 (p + 2) n and 8 (2 p + 1) n — and against the triad probe
   (mgcmt_bandwidth_probe kind 1, 24 B per point) of the same run (a 3-D plan has no probe: the rate of the 2-D plan before it,
   of as many points at the default sizes), as scripts/bench_scf.py does for mgcmt_block_density.
2. drivers.schroedinger_poisson, steps and seconds per step (host clock around the whole call, which ends in downloads) for the
   dot of the tests at 256^2 and 1024^2 with 8 states, at the coupling of scripts/bench_scf.py and at 25 times it: plain mixing
   with beta = 1, 0.5, 0.3, 0.2, 0.1 next to mixing_history = 5 with beta = 1 and 0.5.

usage: bench_mix.py [--reps 10] [--skip-kernel] [--skip-loop] [--skip-plain] [--grids 2d:4096,3d:256] [--loop-grids 256,1024]
                    [--factors 1,25] [--maxiter 150]
one JSON line per measurement"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.linalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_deflate import Events, emit                                                      # noqa: E402
from bench_scf import case                                                                  # noqa: E402
from multigridcmt_amd import _lib, drivers                                                  # noqa: E402
from multigridcmt_amd.operators import potential_operator                                   # noqa: E402
from multigridcmt_amd.plan import Plan                                                      # noqa: E402

F, W = _lib.SLOT_F, _lib.SLOT_W


def kernel(dim, g, reps, triad=None):
    """returns the triad rate (TB/s) it compared with: the probe of this plan, or — a 3-D plan has no probe — the one passed in"""
    p = Plan(potential_operator(g, np.zeros((g,) * (3 if dim == "3d" else 2)), dimension=dim), 8, nvec=11)
    n = p.size(0)
    xs, rs = [(W, t) for t in range(9)], [(F, t) for t in range(9)]
    out, inp, dst = (W, 9), (W, 10), (F, 9)
    rng = np.random.RandomState(1)
    p.upload(0, *xs[0], rng.standard_normal(n))
    p.upload(0, *xs[1], rng.standard_normal(n))
    for t, v in enumerate(xs[2:] + rs + [out, inp], start=2):
        p.lincomb(0, [(np.cos(t), xs[0]), (np.sin(t), xs[1])], v)
    p.sync()
    ev = Events()
    if dim != "3d":
        triad_ms = min(p.bandwidth_probe(0, 1, 1024, 5) for _ in range(3))
        triad = 24 * n / (triad_ms * 1e-3) / 1e12
    for pairs in (2, 6, 9):
        alpha = np.cos(np.arange(pairs))
        for what, fn, moved in (("mix_residual", lambda: p.mix_residual(0, out, inp, rs[pairs - 1], rs[:pairs - 1]), 8 * (pairs + 2) * n),
                                ("mix_combine", lambda: p.mix_combine(0, xs[:pairs], rs[:pairs], alpha, 0.5, dst), 8 * (2 * pairs + 1) * n)):
            ms = min(ev.time_ms(fn, reps) for _ in range(3))
            emit(what=what, dim=dim, grid=g, p=pairs, ms=round(ms, 4), GB=round(moved / 1e9, 2), TBps=round(moved / (ms * 1e-3) / 1e12, 3),
                 triad_TBps=round(triad, 3) if triad else None, fraction_of_triad=round(moved / (ms * 1e-3) / 1e12 / triad, 3) if triad else None)
    p.close()
    return triad


def loop(g, maxiter, factors, plain, k=8, lowest=8, tol=1e-6):
    _, op, pop, coupling = case(g)
    f = np.array([2.0, 2.0, 2.0] + [0.0] * (k - 3))
    drivers.schroedinger_poisson(op, pop, k, f, coupling=coupling, tol=tol, lowest=lowest, maxiter=2, mixing_history=1)   # kernels, occupancy queries
    for factor in factors:
        for history, betas in ((0, (1.0, 0.5, 0.3, 0.2, 0.1) if plain else ()), (5, (1.0, 0.5))):
            for beta in betas:
                info = {}
                t = time.perf_counter()
                try:
                    drivers.schroedinger_poisson(op, pop, k, f, coupling=factor * coupling, mixing=beta, mixing_history=history, tol=tol, lowest=lowest,
                                                 maxiter=maxiter, info=info)
                except (RuntimeError, scipy.linalg.LinAlgError) as e:     # (a Poisson solve that did not converge; a Rayleigh-Ritz
                    # step of the eigen-solver whose Gram matrix was not positive definite: the loop gave up)
                    emit(what="schroedinger_poisson", grid=g, k=k, coupling_factor=factor, mixing=beta, mixing_history=history, status="error: %s" % str(e)[:120])
                    continue
                t = time.perf_counter() - t
                emit(what="schroedinger_poisson", grid=g, k=k, coupling_factor=factor, mixing=beta, mixing_history=history, status=info["status"],
                     steps=info["iterations"], seconds=round(t, 3), seconds_per_step=round(t / info["iterations"], 4), last_change="%.2e" % info["changes"][-1],
                     eigen_iterations=sum(info["eigen_iterations"]), poisson_iterations=sum(info["poisson_iterations"]), restarts=info["mixing_restarts"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--grids", default="2d:4096,3d:256")
    ap.add_argument("--loop-grids", default="256,1024")
    ap.add_argument("--maxiter", type=int, default=150)
    ap.add_argument("--factors", default="1,25")
    ap.add_argument("--skip-plain", action="store_true")
    args = ap.parse_args()
    emit(what="device", name=_lib.device_name(0))
    if not args.skip_kernel:
        triad = None
        for item in [x for x in args.grids.split(",") if x]:
            dim, g = item.split(":")
            triad = kernel(dim, int(g), args.reps, triad)
    if not args.skip_loop:
        for g in [int(x) for x in args.loop_grids.split(",") if x]:
            loop(g, args.maxiter, [float(x) for x in args.factors.split(",") if x], not args.skip_plain)
