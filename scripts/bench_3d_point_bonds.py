"""3-D cycles with per-point bonds (mgcmt_plan_create3d_bonds) at 256^3 and 512^3 (fp64): the fine level's passes (constant
7-point + D + bonds, "kind 5") one by one, marching and (MGCMT_3D_POINT_MARCH=0) flat, next to the same passes of a
point-diagonal plan (kind 2, the yardstick), with their compulsory bytes per point and the acceptance
t(bonds) / t(point diagonal) <= 1.10 x the byte ratio; whole V(2,2) cycles with both smoothers.  One JSON line per grid size,
appended to --out.  Times are wall-clock averages of back-to-back launches; the prolongation + correction + Jacobi pass has no
entry of its own and shows in a kernel trace only:

    python scripts/bench_3d_point_bonds.py [--g 256 512] [--cycles 8] [--reps 10] [--out profiles/r09_point_bonds_3d.jsonl]
    rocprofv3 --kernel-trace --stats ... -- python scripts/bench_3d_point_bonds.py --trace bonds --g 256

--trace PLAN (point, bonds or bonds_flat) only runs --cycles V(2,2) cycles of each smoother with HIP graphs off, for a kernel trace.
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
from multigridcmt_amd._lib import GS_MC, SLOT_F, SLOT_V, WJACOBI  # noqa: E402
from multigridcmt_amd.operators import potential_operator, variable_mass_operator  # noqa: E402
from multigridcmt_amd.plan import Plan  # noqa: E402

PEAK = 8.0e12  # bytes/s, MI355X HBM3E
# compulsory bytes per fine point, point-diagonal level / the same plus three bond planes (a parity stage reads all three: each
# bond joins two points of opposite parity)
BYTES = {"wjacobi_sweep": (32, 56),          # read v, f, D (, Bx, By, Bz); write v'
         "red_black_sweep": (40, 88),        # two parity stages: read v, f/2, D/2 (, Bx, By, Bz); write v/2
         "residual_restrict": (26, 50),      # read v, f, D (, Bx, By, Bz); write F and V of level 1 (1/8 each)
         "prolong_jacobi": (33, 57)}         # the same as the Jacobi sweep plus e of level 1 (1/8)
SMOOTHERS = (("wjacobi", WJACOBI, 2. / 3.), ("red_black", GS_MC, 1.0))


def timed(plan, fn, reps):
    fn()
    plan.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    plan.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def smooth_dot(g):
    """(w, V): an ellipsoidal GaAs dot in AlGaAs with a smeared interface, index [z, y, x]"""
    t = (np.arange(g) + 0.5) / g - 0.5
    Z, Y, X = np.meshgrid(t, t, t, indexing="ij", sparse=True)
    s = 0.5 * (1.0 + np.tanh((np.sqrt((X - 0.05) ** 2 + ((Y + 0.03) / 0.8) ** 2 + ((Z - 0.02) / 0.6) ** 2) - 0.3) / 0.08))
    return 1.0 - 0.27 * s, 30.0 * s


def make_plan(which, g, lowest):
    if which == "bonds_flat":
        os.environ["MGCMT_3D_POINT_MARCH"] = "0"
    else:
        os.environ.pop("MGCMT_3D_POINT_MARCH", None)
    w, V = smooth_dot(g)
    op = potential_operator(g, V, dimension="3d") if which == "point" else variable_mass_operator(g, w, V, dimension="3d")
    del w, V
    t0 = time.perf_counter()
    plan = Plan(op, lowest, nvec=1)
    plan.sync()
    return plan, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--lowest", type=int, default=8)
    ap.add_argument("--cycles", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace", choices=["point", "bonds", "bonds_flat"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_point_bonds_3d.jsonl"))
    a = ap.parse_args()
    for g in a.g:
        pts = float(g) ** 3
        f = np.random.RandomState(0).rand(g ** 3)
        if a.trace:
            plan, _ = make_plan(a.trace, g, a.lowest)
            try:
                plan.set_option(_lib.OPT_GRAPH, 0)
                plan.set_shifts([0.0])
                plan.upload(0, SLOT_F, 0, f)
                for _, kind, omega in SMOOTHERS:
                    plan.upload(0, SLOT_V, 0, np.zeros(g ** 3))
                    for _ in range(a.cycles):
                        plan.vcycle(2, 2, kind, omega=omega, k=1, nu_coarse=4)
                plan.sync()
                print(json.dumps({"trace": a.trace, "g": g, "level_paths": [list(plan.level_path_3d(l)) for l in range(2)]}))
            finally:
                plan.close()
            continue
        out = {"bench": "vcycle_3d_point_bonds", "g": g, "lowest_level": a.lowest, "device": _lib.device_name(0)}
        rows = {}
        for which in ("point", "bonds", "bonds_flat"):
            plan, created = make_plan(which, g, a.lowest)
            try:
                plan.set_shifts([0.0])
                plan.upload(0, SLOT_F, 0, f)
                plan.upload(0, SLOT_V, 0, np.zeros(g ** 3))
                r = {"plan_create_s": round(created, 3), "level_paths": [list(plan.level_path_3d(l)) for l in range(2)]}
                for name, kind, omega in SMOOTHERS:
                    ms = timed(plan, lambda: plan.vcycle(2, 2, kind, omega=omega, k=1, nu_coarse=4), a.cycles)
                    r["cycle_" + name + "_ms"] = round(ms, 4)
                fns = {"wjacobi_sweep": lambda: plan.smooth(0, WJACOBI, 1, omega=2. / 3.),
                       "red_black_sweep": lambda: plan.smooth(0, GS_MC, 1, omega=1.0),
                       "residual_restrict": lambda: plan.residual_restrict(0)}
                r["fine"] = {k: round(timed(plan, fn, a.reps), 4) for k, fn in fns.items()}
                rows[which] = r
            finally:
                plan.close()
        out.update(rows)
        acc = {}
        for name in rows["bonds"]["fine"]:
            b0, b1 = BYTES[name]
            tp, tb, tf = (rows[w]["fine"][name] for w in ("point", "bonds", "bonds_flat"))
            ratio, allowed = tb / tp, 1.10 * b1 / b0
            acc[name] = {"bytes_point": b0, "bytes_bonds": b1, "t_point_ms": tp, "t_bonds_ms": tb, "t_bonds_flat_ms": tf, "ratio": round(ratio, 3),
                         "allowed": round(allowed, 3), "verdict": "met" if ratio <= allowed else "missed",
                         "bonds_fraction_of_8TBs": round(b1 * pts / (tb * 1e-3) / PEAK, 3)}
        out["acceptance"] = acc
        line = json.dumps(out)
        print(line)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
