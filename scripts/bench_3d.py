"""3-D V-cycle at 512^3 (fp64): V(2,2) with weighted Jacobi and with red-black Gauss-Seidel, the fine level's passes one by
one with their compulsory bytes per point and fraction of 8 TB/s, and a 128^3 cycle checked against the oracle.  Prints
one JSON line.

    python scripts/bench_3d.py [--g 512] [--cycles 20] [--reps 20] [--no-check]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multigridcmt_amd import _lib  # noqa: E402
from multigridcmt_amd._lib import GS_MC, SLOT_F, SLOT_T, SLOT_V, WJACOBI  # noqa: E402
from multigridcmt_amd.operators import laplacian_operator  # noqa: E402
from multigridcmt_amd.plan import get_plan  # noqa: E402

PEAK = 8.0e12  # bytes/s, MI355X HBM3E


def timed(plan, fn, reps):
    """average milliseconds of fn() over reps back-to-back launches on the default stream (one synchronisation)"""
    fn()
    plan.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    plan.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g", type=int, default=512)
    ap.add_argument("--lowest", type=int, default=8)
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    g = a.g
    pts = float(g) ** 3
    op = (-1 / np.pi ** 2) * laplacian_operator(g, "3d")
    plan = get_plan(op, a.lowest, nvec=1)
    plan.set_shifts([0.0])
    plan.upload(0, SLOT_F, 0, np.random.RandomState(0).rand(g ** 3))
    plan.upload(0, SLOT_V, 0, np.zeros(g ** 3))
    out = {"bench": "vcycle_3d", "g": g, "lowest_level": a.lowest, "device": _lib.device_name(0), "peak_bytes_per_s": PEAK}
    # whole cycles (HIP-graph replays after the first two calls)
    levels_factor = 8.0 / 7.0  # every coarser level moves 1/8 of the bytes of the one above it
    cycle_bytes = {"wjacobi": 24 + 24 + 18 + 25 + 24, "red_black": 32 + 32 + 18 + 17 + 32 + 32}  # fine-level B/point per V(2,2)
    for name, kind, omega in (("wjacobi", WJACOBI, 2. / 3.), ("red_black", GS_MC, 1.0)):
        ms = timed(plan, lambda: plan.vcycle(2, 2, kind, omega=omega, k=1, nu_coarse=4), a.cycles)
        b = cycle_bytes[name] * pts * levels_factor
        out[name] = {"ms_per_cycle": round(ms, 4), "mlups": round(pts / ms / 1e3, 1), "cycles_per_s": round(1e3 / ms, 2),
                     "compulsory_bytes_per_fine_point": cycle_bytes[name],
                     "cycle_compulsory_fraction": round(b / (ms * 1e-3) / PEAK, 3)}
    # fine-level passes one by one (compulsory bytes per fine point: what must cross HBM at least once)
    passes = {}
    plan.residual_restrict(0)  # (allocates level 1)

    def one(name, fn, bpp):
        ms = timed(plan, fn, a.reps)
        passes[name] = {"ms": round(ms, 4), "bytes_per_point": bpp, "fraction_of_8TBs": round(bpp * pts / (ms * 1e-3) / PEAK, 3)}

    one("wjacobi_sweep", lambda: plan.smooth(0, WJACOBI, 1, omega=2. / 3.), 24)                # read v, f; write v'
    one("red_black_sweep", lambda: plan.smooth(0, GS_MC, 1, omega=1.0), 32)                    # two parity passes: read v, f/2; write v/2
    one("residual_restrict", lambda: plan.residual_restrict(0), 18)                            # read v, f; write F, V of level 1
    one("prolong_correct", lambda: plan.prolong_correct(0), 17)                                # read v, e/8; write v
    one("apply", lambda: plan.apply(0, (SLOT_V, 0), (SLOT_T, 0)), 16)                          # read v; write A v
    out["fine_passes"] = passes
    if not a.no_check:
        from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker
        from test_3d_cycle import Ref3dSolver, Ref3dStencilMaker
        gc = 128
        A = (-1 / np.pi ** 2) * MGCMTStencilMaker().laplacian(gc, dimension="3d")
        f = np.random.RandomState(1).rand(gc ** 3)
        x = MGCMTSolver().vcycle(np.zeros(gc ** 3), f.copy(), A, MGCMTStencilMaker(), nu1=2, nu2=2, shift=0.5, lowest_level=8, dimension="3d")
        y = Ref3dSolver().vcycle(np.zeros(gc ** 3), f.copy(), A, Ref3dStencilMaker(), nu1=2, nu2=2, shift=0.5, lowest_level=8, dimension="3d")
        out["check_128"] = {"checksum": float(np.sum(x)), "oracle_checksum": float(np.sum(y)),
                            "rel_err": float(np.linalg.norm(x - y) / np.linalg.norm(y))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
