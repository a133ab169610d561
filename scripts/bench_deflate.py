"""mgcmt_block_deflate and drivers.deflated_eigensolve at size (DESIGN.md par. 4.21; results: profiles/r17_deflated_eigensolve.md).

1. The entry (pass 1 k_block_cross + k_pencil_final, pass 2 k_block_deflate) between two HIP events on the null stream at 4096^2
   and 256^3 for nq = 16, 32, 64 and k = 16, against its bytes — 8 (nq + k) n read by pass 1, 8 (nq + 2 k) n moved by pass 2 —
   and against the triad probe (mgcmt_bandwidth_probe kind 1, 24 B per point) of the same run (a 3-D plan has no probe: the
   rate of the 2-D plan before it, of as many points at the default sizes).  The split between the two passes
   comes from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python scripts/bench_deflate.py --skip-solve).
2. One drivers.deflated_eigensolve of 40 states at 2048^2 next to drivers.block_eigensolve(k=16) at the same size, per iteration.

usage: bench_deflate.py [--reps 10] [--skip-kernel] [--skip-solve] [--solve-grid 2048]     one JSON line per measurement"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multigridcmt_amd import _lib, drivers                      # noqa: E402
from multigridcmt_amd.operators import laplacian_operator       # noqa: E402
from multigridcmt_amd.plan import Plan, release_plans           # noqa: E402

F, W = _lib.SLOT_F, _lib.SLOT_W


def emit(**rec):
    print(json.dumps(rec), flush=True)


class Events:
    """two HIP events of the runtime the library has loaded"""

    def __init__(self):
        self.hip = None
        for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6", "/opt/rocm/lib/libamdhip64.so"):
            try:
                self.hip = ctypes.CDLL(name)
                break
            except OSError:
                pass
        assert self.hip is not None, "the HIP runtime library was not found"
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(ctypes.byref(e)) == 0

    def time_ms(self, fn, reps):
        """average milliseconds of `reps` calls of fn (stream-ordered on the null stream) after one untimed call"""
        fn()
        assert self.hip.hipEventRecord(self.a, None) == 0
        for _ in range(reps):
            fn()
        assert self.hip.hipEventRecord(self.b, None) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = ctypes.c_float(0.0)
        assert self.hip.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b) == 0
        return ms.value / reps


def kernel(dim, g, reps, triad=None):
    """returns the triad rate (TB/s) it compared with: the probe of this plan, or — a 3-D plan has no probe — the one passed in"""
    op = laplacian_operator(g, dim) * (-1 / np.pi ** 2)
    p = Plan(op, 8, nvec=40)
    n = p.size(0)
    Q = [((W, F)[t % 2], t // 2) for t in range(64)]
    Wv = [((W, F)[t % 2], 32 + t // 2) for t in range(16)]
    rng = np.random.RandomState(1)
    a, b = Q[0], Q[1]
    p.upload(0, *a, rng.standard_normal(n) / (8 * np.sqrt(n)))
    p.upload(0, *b, rng.standard_normal(n) / (8 * np.sqrt(n)))
    for q, v in enumerate(Q[2:] + Wv, start=2):
        p.lincomb(0, [(np.cos(q), a), (np.sin(q), b)], v)      # (distinct data everywhere, |Q Q^T| < 1: repeated calls stay finite)
    p.sync()
    ev = Events()
    if dim != "3d":
        triad_ms = min(p.bandwidth_probe(0, 1, 1024, 5) for _ in range(3))
        triad = 24 * n / (triad_ms * 1e-3) / 1e12
    for nq in (16, 32, 64):
        ms = min(ev.time_ms(lambda: p.block_deflate(0, Q[:nq], Wv), reps) for _ in range(3))
        moved = 8 * (nq + 16) * n + 8 * (nq + 32) * n
        emit(what="block_deflate", dim=dim, grid=g, nq=nq, k=16, ms=round(ms, 3), pass1_GB=round(8 * (nq + 16) * n / 1e9, 2),
             pass2_GB=round(8 * (nq + 32) * n / 1e9, 2), TBps=round(moved / (ms * 1e-3) / 1e12, 3), triad_TBps=round(triad, 3) if triad else None,
             fraction_of_triad=round(moved / (ms * 1e-3) / 1e12 / triad, 3) if triad else None)
    p.close()
    return triad


def solve(g, k, reps_block):
    op = laplacian_operator(g, "2d") * (-1 / np.pi ** 2)
    drivers.deflated_eigensolve(op, k, lowest=8, maxiter=2)                                   # plan, kernels, graph capture
    info = {}
    t = time.perf_counter()
    vals, _ = drivers.deflated_eigensolve(op, k, lowest=8, info=info)
    t = time.perf_counter() - t
    err = float(np.abs(vals - drivers.exact_box_eigenvalues(g, "2d", k)).max())
    emit(what="deflated_eigensolve", grid=g, k=k, status=info["status"], iterations=info["iterations"], seconds=round(t, 3),
         ms_per_iteration=round(t / info["iterations"] * 1e3, 3), column_cycles=info["column_cycles"], eigenvalue_error=err,
         locked_at=[int(x) for x in info["locked_at"]])
    release_plans()
    stats = {}
    drivers.block_eigensolve(op, k=16, cycles=2, lowest=8)
    drivers.block_eigensolve(op, k=16, cycles=reps_block, lowest=8, stats=stats)
    emit(what="block_eigensolve", grid=g, k=16, cycles=reps_block, ms_per_iteration=round(stats["loop_seconds"] / reps_block * 1e3, 3))
    release_plans()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-solve", action="store_true")
    ap.add_argument("--solve-grid", type=int, default=2048)
    ap.add_argument("--grids", default="2d:4096,3d:256")
    args = ap.parse_args()
    emit(what="device", name=_lib.device_name(0))
    if not args.skip_kernel:
        triad = None
        for item in [x for x in args.grids.split(",") if x]:
            dim, g = item.split(":")
            triad = kernel(dim, int(g), args.reps, triad)
    if not args.skip_solve:
        solve(args.solve_grid, 40, 10)
