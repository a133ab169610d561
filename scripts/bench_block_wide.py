"""The wide block operations at size (DESIGN.md par. 4.11b; results: profiles/r08_block_wide.md).

1. mgcmt_block_pencil against the same pencil assembled from 12 x 4 tiles of mgcmt_block_gram: m = 12 and 48 at 4096^2 and 8192^2.
2. mgcmt_block_combine_wide (48 -> 16) against mgcmt_block_combine (12 -> 4), in time per byte moved.
3. one drivers.block_eigensolve iteration at 4096^2 for k = 4 (12 x 4 kernels), 8 and 16 (wide kernels), split by entry.

usage: bench_block_wide.py [--grids 4096,8192] [--reps 5] [--skip-iteration]     one JSON line per measurement"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multigridcmt_amd import _lib, drivers                      # noqa: E402
from multigridcmt_amd.operators import laplacian_operator       # noqa: E402
from multigridcmt_amd.plan import Plan                          # noqa: E402

V, F, W = _lib.SLOT_V, _lib.SLOT_F, _lib.SLOT_W


def emit(**rec):
    print(json.dumps(rec), flush=True)


def best(fn, reps):
    """fastest of `reps` timed calls after one untimed (fn ends synchronised)"""
    fn()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t)
    return min(times), sorted(times)[len(times) // 2]


def fill_random(p, vectors):
    """distinct random data in every vector from two uploads: v_q = cos(q) r0 + sin(q) r1 (zero-filled operands flatter a kernel)"""
    n = p.size(0)
    rng = np.random.RandomState(1)
    a, b = vectors[0], vectors[1]
    p.upload(0, *a, rng.standard_normal(n))
    p.upload(0, *b, rng.standard_normal(n))
    for q, v in enumerate(vectors[2:], start=2):
        p.lincomb(0, [(np.cos(q), a), (np.sin(q), b)], v)
    p.sync()


def pencil_and_combine(g, reps):
    op = laplacian_operator(g, "2d") * (-1 / np.pi ** 2)
    p = Plan(op, 8, nvec=48)
    n = p.size(0)
    S, AS, MS = [(W, q) for q in range(48)], [(F, q) for q in range(48)], [(V, q) for q in range(48)]
    fill_random(p, S + AS + MS)
    for m in (12, 48):
        def wide():
            p.block_pencil(0, S[:m], AS[:m])

        def tiled():
            for B in (AS, S):
                for r in range(0, m, 12):
                    for c in range(0, m, 4):
                        p.block_gram(0, S[r:r + 12], B[c:c + 4])
        tw, tw_med = best(wide, reps)
        tt, tt_med = best(tiled, reps)
        emit(what="pencil", grid=g, m=m, wide_ms=round(tw * 1e3, 3), wide_ms_median=round(tw_med * 1e3, 3), tiled_ms=round(tt * 1e3, 3),
             tiled_ms_median=round(tt_med * 1e3, 3), speedup=round(tt / tw, 2), wide_TBps_of_2m_vectors=round(2 * m * n * 8 / tw / 1e12, 3),
             tiled_launches=2 * (m // 12) * (m // 4), tiled_TBps_of_its_reads=round(2 * (m // 12) * (m // 4) * 16 * n * 8 / tt / 1e12, 3))

        def wide_mass():
            p.block_pencil(0, S[:m], AS[:m], MS[:m])
        tm, _ = best(wide_mass, reps)
        emit(what="pencil with a third list", grid=g, m=m, wide_ms=round(tm * 1e3, 3), wide_TBps_of_3m_vectors=round(3 * m * n * 8 / tm / 1e12, 3))
    C = np.random.RandomState(2).standard_normal((48, 16))
    OUT = [(V, q) for q in range(16)]
    inner = 4

    def wide_c():
        for _ in range(inner):
            p.block_combine_wide(0, S, OUT, C)
        p.sync()

    def old_c():
        for _ in range(inner):
            p.block_combine(0, S[:12], OUT[:4], C[:12, :4])
        p.sync()
    tw, _ = best(wide_c, reps)
    to, _ = best(old_c, reps)
    bw, bo = (48 + 16) * n * 8, (12 + 4) * n * 8
    emit(what="combine", grid=g, wide_48_16_ms=round(tw / inner * 1e3, 3), old_12_4_ms=round(to / inner * 1e3, 3),
         wide_TBps=round(bw / (tw / inner) / 1e12, 3), old_TBps=round(bo / (to / inner) / 1e12, 3),
         time_per_byte_ratio_wide_over_old=round((tw / bw) / (to / bo), 3))
    p.close()


def iteration_split(g, k, cycles):
    """one block_eigensolve iteration split by entry: every Plan call of the loop timed with a synchronisation behind it"""
    from multigridcmt_amd import plan as plan_mod
    groups = {"vcycle": "cycles", "apply": "applications", "block_pencil": "pencil", "block_gram": "pencil", "block_combine": "combines",
              "block_combine_wide": "combines", "lincomb": "residual vectors"}
    spent = {}
    originals = {}

    def wrap(name, fn):
        def timed(self, *a, **kw):
            t = time.perf_counter()
            r = fn(self, *a, **kw)
            check_sync(self)
            spent[groups[name]] = spent.get(groups[name], 0.0) + time.perf_counter() - t
            return r
        return timed

    def check_sync(p):
        _lib.check(_lib.lib().mgcmt_sync(None))
    op = laplacian_operator(g, "2d") * (-1 / np.pi ** 2)
    stats = {}
    drivers.block_eigensolve(op, k=k, cycles=2, lowest=8)                                   # plan, kernels, graph capture
    drivers.block_eigensolve(op, k=k, cycles=cycles, lowest=8, stats=stats)
    untimed = stats["loop_seconds"] / cycles
    for name in groups:
        originals[name] = getattr(plan_mod.Plan, name)
        setattr(plan_mod.Plan, name, wrap(name, originals[name]))
    try:
        drivers.block_eigensolve(op, k=k, cycles=cycles, lowest=8)
        whole = dict(spent)
        spent.clear()
        drivers.block_eigensolve(op, k=k, cycles=0, lowest=8)      # the set-up before the loop alone: taken off
        split = {key: (val - spent.get(key, 0.0)) / cycles for key, val in whole.items()}
    finally:
        for name, fn in originals.items():
            setattr(plan_mod.Plan, name, fn)
    emit(what="iteration", grid=g, k=k, kernels="wide" if k > 4 else "12 x 4", ms_per_iteration=round(untimed * 1e3, 3),
         split_ms={key: round(val * 1e3, 3) for key, val in sorted(split.items())})
    plan_mod.release_plans()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="4096,8192")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-iteration", action="store_true")
    ap.add_argument("--iteration-grid", type=int, default=4096)
    args = ap.parse_args()
    emit(what="device", name=_lib.device_name(0))
    for g in [int(x) for x in args.grids.split(",") if x]:
        pencil_and_combine(g, args.reps)
    if not args.skip_iteration:
        for k in (4, 8, 16):
            iteration_split(args.iteration_grid, k, 6)
