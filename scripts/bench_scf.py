"""The Schroedinger-Poisson loop on the device at size (DESIGN.md par. 4.23; results: profiles/r19_schroedinger_poisson.md).

1. mgcmt_block_density (k_block_density) between two HIP events on the null stream at 4096^2 and 256^3 for nq = 16, 32, 64 against
   its bytes — 8 (nq + 1) n — and against the triad probe (mgcmt_bandwidth_probe kind 1, 24 B per point) of the same run (a 3-D
   plan has no probe: the rate of the 2-D plan before it, of as many points at the default sizes), as scripts/bench_deflate.py.
2. mgcmt_plan_set_point_diagonal at 2048^2 and 128^3 (HIP events) next to what a user does today for a new potential: creating
   a plan with the same nvec from the host arrays (host clock, the creation synchronises), in the same session.
3. drivers.schroedinger_poisson per step (host clock around the whole call, which ends in downloads) for the dot of the tests at
   256^2 and at 1024^2 with 8 states, next to the same loop written with the public interface as it was before these entries:
   a new operator and plan in every step (plan.get_plan through drivers.deflated_eigensolve, the previous states as guesses), the
   states through the host, the density in NumPy, MGCMTSolver.solve for the potential.

usage: bench_scf.py [--reps 10] [--skip-kernel] [--skip-update] [--skip-loop] [--loop-grids 256,1024]    one JSON line per measurement"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_deflate import Events, emit                                                      # noqa: E402
from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, _lib, drivers                  # noqa: E402
from multigridcmt_amd.operators import potential_operator, variable_mass_operator           # noqa: E402
from multigridcmt_amd.plan import Plan, release_plans                                       # noqa: E402

F, W = _lib.SLOT_F, _lib.SLOT_W


def kernel(dim, g, reps, triad=None):
    """returns the triad rate (TB/s) it compared with: the probe of this plan, or — a 3-D plan has no probe — the one passed in"""
    p = Plan(potential_operator(g, np.zeros((g,) * (3 if dim == "3d" else 2)), dimension=dim), 8, nvec=33)
    n = p.size(0)
    xs = [((W, F)[t % 2], t // 2) for t in range(64)]
    rng = np.random.RandomState(1)
    p.upload(0, *xs[0], rng.standard_normal(n))
    p.upload(0, *xs[1], rng.standard_normal(n))
    for t, v in enumerate(xs[2:], start=2):
        p.lincomb(0, [(np.cos(t), xs[0]), (np.sin(t), xs[1])], v)
    p.sync()
    ev = Events()
    if dim != "3d":
        triad_ms = min(p.bandwidth_probe(0, 1, 1024, 5) for _ in range(3))
        triad = 24 * n / (triad_ms * 1e-3) / 1e12
    for nq in (16, 32, 64):
        w = np.cos(np.arange(nq))
        ms = min(ev.time_ms(lambda: p.block_density(0, xs[:nq], w, (W, 32)), reps) for _ in range(3))
        moved = 8 * (nq + 1) * n
        emit(what="block_density", dim=dim, grid=g, nq=nq, ms=round(ms, 3), GB=round(moved / 1e9, 2), TBps=round(moved / (ms * 1e-3) / 1e12, 3),
             triad_TBps=round(triad, 3) if triad else None, fraction_of_triad=round(moved / (ms * 1e-3) / 1e12 / triad, 3) if triad else None)
    p.close()
    return triad


def update(dim, g, lowest, nvec, reps):
    shape = (g,) * (3 if dim == "3d" else 2)
    rng = np.random.RandomState(2)
    v = 30.0 * rng.rand(*shape)
    t = time.perf_counter()
    p = Plan(potential_operator(g, v, dimension=dim), lowest, nvec=nvec)
    p.sync()
    first = time.perf_counter() - t
    p.close()
    creates = []
    for _ in range(3):
        t = time.perf_counter()
        p = Plan(potential_operator(g, v, dimension=dim), lowest, nvec=nvec)
        p.sync()
        creates.append(time.perf_counter() - t)
        if _ < 2:
            p.close()
    p.upload(0, W, 0, v)
    p.upload(0, W, 1, rng.standard_normal(shape))
    ev = Events()
    ms = min(ev.time_ms(lambda: p.set_point_diagonal([(1.0, (W, 0)), (0.5, (W, 1))]), reps) for _ in range(3))
    emit(what="set_point_diagonal", dim=dim, grid=g, nvec=nvec, levels=p.num_levels, ms=round(ms, 3), plan_creation_ms=round(min(creates) * 1e3, 2),
         first_plan_creation_ms=round(first * 1e3, 2), ratio=round(min(creates) * 1e3 / ms, 1))
    p.close()


def case(g):
    """the dot of tests/test_schroedinger_poisson.py on g^2 points, the coupling scaled with the mesh (unit vectors: the density
    per point falls as (g + 1)^-2)"""
    t = (np.arange(g) + 1.0) / (g + 1)
    X, Y = np.meshgrid(t, t, indexing="ij")
    eps = np.ones((g, g))
    eps[:, g // 2:] = 3.0
    v_ext = 160.0 * ((X - 0.5) ** 2 + (Y - 0.45) ** 2)
    return v_ext, potential_operator(g, v_ext), variable_mass_operator(g, eps), 800.0 * ((g + 1) / 33.0) ** 2


def host_loop(g, v_ext, pop, k, f, coupling, tol, lowest, maxiter=50):
    """the loop with the public interface as it was: (steps, eigenvalues, phi)"""
    solver, sm = MGCMTSolver(), MGCMTStencilMaker()
    phi, vecs, vals = np.zeros(g * g), None, None
    for step in range(1, maxiter + 1):
        op = potential_operator(g, v_ext + coupling * phi.reshape(g, g))
        vals, vecs = drivers.deflated_eigensolve(op, k, rtol=1e-9, lowest=lowest, guesses=vecs)
        rho = (vecs ** 2 / (vecs ** 2).sum(axis=0)) @ f
        new = np.asarray(solver.solve(rho, pop, sm, v0=phi if step > 1 else None, nu1=2, nu2=2, smoother=solver.gseidel_rb, lowest_level=lowest,
                                      dimension="2d", rtol=1e-10)).reshape(-1)
        d = np.linalg.norm(new - phi) / np.linalg.norm(new)
        phi = new
        if d <= tol:
            break
    return step, vals, phi


def loop(g, k=8, lowest=8, tol=1e-6):
    v_ext, op, pop, coupling = case(g)
    f = np.array([2.0, 2.0, 2.0] + [0.0] * (k - 3))
    drivers.schroedinger_poisson(op, pop, k, f, coupling=coupling, tol=tol, lowest=lowest, maxiter=2)          # kernels, occupancy queries
    info = {}
    t = time.perf_counter()
    vals, _, phi = drivers.schroedinger_poisson(op, pop, k, f, coupling=coupling, tol=tol, lowest=lowest, info=info)
    t = time.perf_counter() - t
    emit(what="schroedinger_poisson", grid=g, k=k, status=info["status"], steps=info["iterations"], seconds=round(t, 3),
         seconds_per_step=round(t / info["iterations"], 4), eigen_iterations=info["eigen_iterations"], poisson_iterations=info["poisson_iterations"],
         changes=["%.2e" % d for d in info["changes"]])
    host_loop(g, v_ext, pop, k, f, coupling, tol, lowest, maxiter=2)
    release_plans()
    th = time.perf_counter()
    steps, hvals, hphi = host_loop(g, v_ext, pop, k, f, coupling, tol, lowest)
    th = time.perf_counter() - th
    release_plans()
    emit(what="host_loop", grid=g, k=k, steps=steps, seconds=round(th, 3), seconds_per_step=round(th / steps, 4),
         ratio_per_step=round((th / steps) / (t / info["iterations"]), 2), eigenvalue_difference=float(np.abs(hvals - vals).max()),
         phi_difference=float(np.linalg.norm(hphi - phi) / np.linalg.norm(phi)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-update", action="store_true")
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--grids", default="2d:4096,3d:256")
    ap.add_argument("--update-grids", default="2d:2048,3d:128")
    ap.add_argument("--loop-grids", default="256,1024")
    args = ap.parse_args()
    emit(what="device", name=_lib.device_name(0))
    if not args.skip_kernel:
        triad = None
        for item in [x for x in args.grids.split(",") if x]:
            dim, g = item.split(":")
            triad = kernel(dim, int(g), args.reps, triad)
    if not args.skip_update:
        for item in [x for x in args.update_grids.split(",") if x]:
            dim, g = item.split(":")
            update(dim, int(g), 8, 4, args.reps)
    if not args.skip_loop:
        for g in [int(x) for x in args.loop_grids.split(",") if x]:
            loop(g)
