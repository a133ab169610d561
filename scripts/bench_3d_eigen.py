"""3-D Rayleigh-quotient eigensolvers (fp64): one vcycle_rqmg cycle of the scaled Laplacian (V(4,4), the reference's default,
and V(2,2); M = I carried explicitly, nmin 2; the iterate resident on the GPU), one rqmin step on the fine level alone (the
two marching passes and their scalar kernels), and one iteration of the cube-well eigensolver
(drivers.potential_well_eigensolve, method "vcycle").  Prints one JSON line.  The per-pass HBM fraction of the marching
passes comes from a separate `rocprofv3 --kernel-trace --stats` run of `--trace` (nothing but the rqmin steps):
32 B per point and pass / kernel time / 8 TB/s.

    python scripts/bench_3d_eigen.py [--g 256] [--cycles 5] [--trace]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multigridcmt_amd import _lib, drivers  # noqa: E402
from multigridcmt_amd.operators import identity_operator, laplacian_operator  # noqa: E402
from multigridcmt_amd.solver import MGCMTSolver  # noqa: E402

PEAK = 8.0e12  # bytes/s, MI355X HBM3E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g", type=int, default=256)
    ap.add_argument("--cycles", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="only rqmin steps on the fine level (for a kernel trace)")
    a = ap.parse_args()
    g, n = a.g, a.cycles
    pts = float(g) ** 3
    S = MGCMTSolver()
    op, M = laplacian_operator(g, "3d") * (-1 / np.pi ** 2), identity_operator(g, "3d")
    plan = S._rq_plan(op, M, 2)
    plan.set_shifts(np.zeros(S._RQ_REGS))
    plan.upload(0, _lib.SLOT_V, S._X, np.random.RandomState(0).random_sample(g ** 3))
    out = {"bench": "eigen_3d", "g": g, "device": _lib.device_name(0), "peak_bytes_per_s": PEAK}

    def timed(fn, reps):
        fn()
        plan.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        plan.sync()
        return (time.perf_counter() - t0) * 1e3 / reps

    # rqmin on the fine level alone: nu steps of two marching passes (32 B per point each) + the initial pair
    nu = 4
    ms = timed(lambda: S._rqmin_device(plan, 0, nu, want_rho=False), n)
    out["rqmin_fine_level"] = {"nu": nu, "ms": round(ms, 4), "ms_per_step": round(ms / (nu + 1), 4),
                               "compulsory_fraction": round(((nu * 64.0 + 24.0) * pts) / (ms * 1e-3) / PEAK, 3)}
    if a.trace:
        print(json.dumps(out))
        return
    for nu1 in (4, 2):
        rhos = []
        ms = timed(lambda: rhos.append(S._rqmg_levels(plan, 0, nu1, nu1)[1]), n)
        out["vcycle_rqmg_V%d%d" % (nu1, nu1)] = {"ms_per_cycle": round(ms, 4), "last_rho": rhos[-1],
                                                "exact_rho": float(drivers.exact_box_eigenvalues(g, "3d", 1)[0])}
    plan.close()
    # one iteration of the cube-well eigensolver (V(2,2) red-black cycle of H from a zero start + one line step)
    stats, hist = {}, []
    iters = 10
    rho, _ = drivers.potential_well_eigensolve(g, depth=50.0, cycles=iters, method="vcycle", nu=2, lowest=8, dimension="3d", stats=stats,
                                               history=hist)
    out["well_iteration"] = {"ms_per_iteration": round(stats["loop_seconds"] * 1e3 / iters, 4), "rho": rho, "iterations": iters}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
