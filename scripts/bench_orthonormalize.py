"""mgcmt_block_project, mgcmt_block_orthonormalize and drivers.deflated_eigensolve(basis="orthonormal") at size (DESIGN.md par.
4.22; results: profiles/r18_orthonormal_basis.md).

1. The two entries between two HIP events on the null stream at 4096^2 and 256^3 with k = 16 (the projection with nb = 16 and
   32, with companions), each against the bytes it has to move and the triad probe of the same run, as bench_deflate.py does.
   Bytes (8 n each): projection pass 1 nb + k, pass 2 (nb + 2 k) per pair; orthonormalisation Gram k, product 2 k per block.
2. One drivers.deflated_eigensolve of --solve-states states at --solve-grid^2 with the chosen basis, per iteration; `--maxiter`
   bounds a run that is only timed (the scaled basis does not converge for 40 states at 1024^2 and 2048^2).
   `--package-root DIR` imports the package from another checkout (the parent commit's, built there) for the same measurement.

usage: bench_orthonormalize.py [--reps 10] [--skip-kernel] [--skip-solve] [--solve-grid 1024] [--solve-states 24]
                               [--basis scaled|orthonormal|default] [--maxiter 200] [--package-root DIR]      one JSON line each"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def emit(**rec):
    print(json.dumps(rec), flush=True)


def kernel(dim, g, reps, triad=None):
    from bench_deflate import Events
    from multigridcmt_amd import _lib, drivers
    from multigridcmt_amd.operators import laplacian_operator
    from multigridcmt_amd.plan import Plan
    F, W = _lib.SLOT_F, _lib.SLOT_W
    p = Plan(laplacian_operator(g, dim) * (-1 / np.pi ** 2), 8, nvec=48)
    n = p.size(0)
    B, AB = [(W, t) for t in range(32)], [(F, t) for t in range(32)]
    Wv, AWv = [(W, 32 + t) for t in range(16)], [(F, 32 + t) for t in range(16)]
    rng = np.random.RandomState(1)
    a, b = B[0], B[1]
    p.upload(0, *a, rng.standard_normal(n) / (8 * np.sqrt(n)))
    p.upload(0, *b, rng.standard_normal(n) / (8 * np.sqrt(n)))
    for q, v in enumerate(B[2:] + AB + AWv, start=2):
        p.lincomb(0, [(np.cos(q), a), (np.sin(q), b)], v)      # (distinct data everywhere, |B B^T| < 1: repeated calls stay finite)
    for j, v in enumerate(Wv):
        p.upload(0, *v, rng.standard_normal(n))                # (independent columns: nothing is dropped)
    p.sync()
    ev = Events()
    if dim != "3d":
        triad_ms = min(p.bandwidth_probe(0, 1, 1024, 5) for _ in range(3))
        triad = 24 * n / (triad_ms * 1e-3) / 1e12

    def report(what, ms, moved, **more):
        rate = moved / (ms * 1e-3) / 1e12
        emit(what=what, dim=dim, grid=g, k=16, ms=round(ms, 3), GB=round(moved / 1e9, 2), TBps=round(rate, 3),
             triad_TBps=round(triad, 3) if triad else None, fraction_of_triad=round(rate / triad, 3) if triad else None, **more)
    for nb in (16, 32):
        ms = min(ev.time_ms(lambda: p.block_deflate(0, B[:nb], Wv), reps) for _ in range(3))       # (the same launches: the run's yardstick)
        report("block_deflate", ms, 8 * n * ((nb + 16) + (nb + 32)), nb=nb)
        for comp in (False, True):
            args = (AB[:nb], AWv) if comp else (None, None)
            ms = min(ev.time_ms(lambda: p.block_project(0, B[:nb], Wv, *args), reps) for _ in range(3))
            report("block_project", ms, 8 * n * ((nb + 16) + (nb + 32) * (2 if comp else 1)), nb=nb, companions=comp)
    for comp in (False, True):
        run = lambda: p.block_orthonormalize(0, Wv, AWv if comp else None, drop_tol=drivers.ORTHONORMAL_DROP_TOL)
        ms = min(ev.time_ms(run, reps) for _ in range(3))
        report("block_orthonormalize", ms, 8 * n * (16 + 32 * (2 if comp else 1)), companions=comp)
    assert p.block_orthonormalize(0, Wv, AWv, drop_tol=drivers.ORTHONORMAL_DROP_TOL, want_dropped=True) == 0
    p.close()
    return triad


def solve(g, k, basis, maxiter):
    from multigridcmt_amd import drivers
    from multigridcmt_amd.operators import laplacian_operator
    from multigridcmt_amd.plan import release_plans
    kw = {} if basis == "default" else {"basis": basis}
    op = laplacian_operator(g, "2d") * (-1 / np.pi ** 2)
    drivers.deflated_eigensolve(op, k, lowest=8, maxiter=2, **kw)                             # plan, kernels, graph capture
    for _ in range(3):
        info = {}
        t = time.perf_counter()
        vals, _ = drivers.deflated_eigensolve(op, k, lowest=8, info=info, maxiter=maxiter, **kw)
        t = time.perf_counter() - t
        err = float(np.abs(vals - drivers.exact_box_eigenvalues(g, "2d", k)[:len(vals)]).max())
        emit(what="deflated_eigensolve", package=os.path.dirname(os.path.abspath(drivers.__file__)), basis=basis, grid=g, k=k,
             status=info["status"], iterations=info["iterations"], seconds=round(t, 3), ms_per_iteration=round(t / info["iterations"] * 1e3, 3),
             eigenvalue_error=err, gram_min=float(np.min(info["gram_min"])) if "gram_min" in info else None,
             dropped=int(np.sum(info["dropped"])) if "dropped" in info else None)
    release_plans()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-solve", action="store_true")
    ap.add_argument("--solve-grid", type=int, default=1024)
    ap.add_argument("--solve-states", type=int, default=24)
    ap.add_argument("--basis", default="orthonormal")
    ap.add_argument("--maxiter", type=int, default=200)
    ap.add_argument("--grids", default="2d:4096,3d:256")
    ap.add_argument("--package-root", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
    from multigridcmt_amd import _lib
    emit(what="device", name=_lib.device_name(0))
    if not args.skip_kernel:
        triad = None
        for item in [x for x in args.grids.split(",") if x]:
            dim, g = item.split(":")
            triad = kernel(dim, int(g), args.reps, triad)
    if not args.skip_solve:
        solve(args.solve_grid, args.solve_states, args.basis, args.maxiter)
