"""3-D cycles with a per-point diagonal (mgcmt_plan_create3d_pot) at 256^3 and 512^3 (fp64): the fine level's marching passes
(constant 7-point + D, "kind 2") one by one next to the same passes of the constant 7-point level, with their compulsory
bytes per point and the acceptance t(point) / t(constant) <= 1.10 x the byte ratio; the flat 27-plane passes of level 1; whole
V(2,2) cycles with both smoothers, with the marching and (MGCMT_3D_POINT_MARCH=0) the flat fine level.  One JSON line per
grid size, appended to --out.

    python scripts/bench_3d_potential.py [--g 256 512] [--cycles 10] [--reps 10] [--out profiles/r07_point_potential_3d.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multigridcmt_amd import _lib  # noqa: E402
from multigridcmt_amd._lib import GS_MC, SLOT_F, SLOT_T, SLOT_V, WJACOBI  # noqa: E402
from multigridcmt_amd.operators import laplacian_operator, potential_operator  # noqa: E402
from multigridcmt_amd.plan import Plan  # noqa: E402

PEAK = 8.0e12  # bytes/s, MI355X HBM3E
# compulsory bytes per fine point, constant 7-point level / the same plus D (8 B wherever a point is updated or its residual formed)
BYTES = {"wjacobi_sweep": (24, 32),          # read v, f (, D); write v'
         "red_black_sweep": (32, 40),        # two parity stages: read v, f/2 (, D/2); write v/2
         "residual_restrict": (18, 26)}      # read v, f (, D); write F and V of level 1 (1/8 each)


def timed(plan, fn, reps):
    fn()
    plan.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    plan.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def smooth_v(g):
    t = (np.arange(g) + 0.5) / g - 0.5
    Z, Y, X = np.meshgrid(t, t, t, indexing="ij", sparse=True)
    return 40.0 * (X * X + X * Y + Y * Z + Z * Z) + 10.0 * np.exp(-12.0 * (X - Y) ** 2) + 0.0 * Z


def passes(plan, level, reps, names):
    fns = {"wjacobi_sweep": lambda: plan.smooth(level, WJACOBI, 1, omega=2. / 3.),
           "red_black_sweep": lambda: plan.smooth(level, GS_MC, 1, omega=1.0),
           "residual_restrict": lambda: plan.residual_restrict(level),
           "apply": lambda: plan.apply(level, (SLOT_V, 0), (SLOT_T, 0))}
    return {n: timed(plan, fns[n], reps) for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--lowest", type=int, default=8)
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_point_potential_3d.jsonl"))
    a = ap.parse_args()
    for g in a.g:
        pts = float(g) ** 3
        f = np.random.RandomState(0).rand(g ** 3)
        out = {"bench": "vcycle_3d_point_potential", "g": g, "lowest_level": a.lowest, "device": _lib.device_name(0)}
        rows = {}
        for which in ("constant", "point", "point_flat"):
            if which == "point_flat":
                os.environ["MGCMT_3D_POINT_MARCH"] = "0"
            else:
                os.environ.pop("MGCMT_3D_POINT_MARCH", None)
            op = (-1 / np.pi ** 2) * laplacian_operator(g, "3d") if which == "constant" else potential_operator(g, smooth_v(g), dimension="3d")
            t0 = time.perf_counter()
            plan = Plan(op, a.lowest, nvec=1)
            plan.sync()
            created = time.perf_counter() - t0
            try:
                plan.set_shifts([0.0])
                plan.upload(0, SLOT_F, 0, f)
                plan.upload(0, SLOT_V, 0, np.zeros(g ** 3))
                r = {"plan_create_s": round(created, 3), "level_paths": [list(plan.level_path_3d(l)) for l in range(2)]}
                for name, kind, omega in (("wjacobi", WJACOBI, 2. / 3.), ("red_black", GS_MC, 1.0)):
                    ms = timed(plan, lambda: plan.vcycle(2, 2, kind, omega=omega, k=1, nu_coarse=4), a.cycles)
                    r["cycle_" + name + "_ms"] = round(ms, 4)
                r["fine"] = {k: round(v, 4) for k, v in passes(plan, 0, a.reps, list(BYTES)).items()}
                if which == "point":
                    r["level1_27_planes"] = {k: round(v, 4) for k, v in passes(plan, 1, a.reps, list(BYTES) + ["apply"]).items()}
                rows[which] = r
            finally:
                plan.close()
        out.update(rows)
        acc = {}
        for name, (b0, b1) in BYTES.items():
            tc, tp = rows["constant"]["fine"][name], rows["point"]["fine"][name]
            ratio, allowed = tp / tc, 1.10 * b1 / b0
            acc[name] = {"bytes_constant": b0, "bytes_point": b1, "t_constant_ms": tc, "t_point_ms": tp, "ratio": round(ratio, 3),
                         "allowed": round(allowed, 3), "verdict": "met" if ratio <= allowed else "missed",
                         "point_fraction_of_8TBs": round(b1 * pts / (tp * 1e-3) / PEAK, 3)}
        out["acceptance"] = acc
        line = json.dumps(out)
        print(line)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
