"""2-D cycles with per-point bonds (mgcmt_plan_create_bonds, fp64): the fine level's passes one by one — weighted-Jacobi sweep,
red-black sweep (two parity stages), residual + restriction, the applied operator — in the marching form (csrc/kernels_bonds.hip)
and the flat form (MGCMT_BONDS_MARCH=0), next to the yardstick: the one-launch-per-operation kernels of a plan with a point
diagonal and MGCMT_OPT_FUSED = 0 (k_pw_wjacobi, four k_pw_mc_colour, k_pw_residual + k_restrict + the clearing of V[1]); and
whole V(2,2) cycles with both smoothers.  Compulsory bytes per fine point are kept here, next to the acceptance
t(marching bond pass) / t(yardstick pass) <= 1.10 x the byte ratio.

    python scripts/bench_point_bonds.py passes --which march|flat|yardstick [--g 8192] [--reps 100] [--tree DIR]
    python scripts/bench_point_bonds.py cycles [--g 4096 8192] [--cycles 20]
    python scripts/bench_point_bonds.py ab --parent DIR [--rounds 3] [--g 8192] [--out profiles/r08_point_bonds.jsonl]

`passes --which yardstick` uses nothing newer than the point-diagonal plans, so `--tree DIR` can point it at a checkout of an
earlier commit (built there); `ab` alternates that checkout and this tree, one process per measurement, and prints the medians
with the acceptance.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8.0e12  # bytes/s, MI355X HBM3E
# compulsory bytes per fine point: (yardstick on a point-diagonal level, bond level)
BYTES = {"wjacobi_sweep": (32, 48),          # read v, f, D (, E, S); write v'
         "red_black_sweep": (48, 72),        # yardstick: four colours of 12 (v: own quarter + two colours of neighbours, f, D, v' a quarter each);
                                             # bonds: two parity stages of 36 (v 8, all of E and S 16, f, D, v' half each)
         "residual_restrict": (44, 44)}      # yardstick: residual 32 (v, f, D; r) + restriction 10 (r; F[1]) + clearing V[1] 2;
                                             # bonds: v, f, D, E, S in, F[1] and V[1] out, no residual stored


def timed(plan, fn, reps):
    for _ in range(3):
        fn()
    plan.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    plan.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def fields(g):
    """a dot with a light mass: inverse mass 4 inside a disc, 1 outside, 20 % disorder; barrier 30 outside"""
    x = (np.arange(g) + 0.5) / g - 0.5
    X, Y = np.meshgrid(x, x, indexing="ij", sparse=True)
    inside = (X - 0.05) ** 2 + (Y + 0.1) ** 2 < 0.3 ** 2
    w = np.where(inside, 4.0, 1.0) * (1.0 + 0.2 * np.random.RandomState(2).rand(g, g))
    return w, np.where(inside, 0.0, 30.0)


def make_plan(which, g, lowest, tree):
    sys.path.insert(0, tree)
    from multigridcmt_amd import _lib
    from multigridcmt_amd import operators
    from multigridcmt_amd.plan import Plan
    w, V = fields(g)
    if which == "yardstick":
        plan = Plan(operators.potential_operator(g, V), lowest, nvec=1)
        plan.set_option(_lib.OPT_FUSED, 0)
    else:
        os.environ["MGCMT_BONDS_MARCH"] = "1" if which == "march" else "0"
        plan = Plan(operators.variable_mass_operator(g, w, V), lowest, nvec=1)
    plan.set_shifts([0.0])
    rng = np.random.RandomState(0)
    plan.upload(0, _lib.SLOT_F, 0, rng.rand(g * g))
    plan.upload(0, _lib.SLOT_V, 0, rng.rand(g * g))
    return plan, _lib


def run_passes(a):
    plan, _lib = make_plan(a.which, a.g[0], a.lowest, a.tree)
    try:
        g = a.g[0]
        fns = {"wjacobi_sweep": lambda: plan.smooth(0, _lib.WJACOBI, 1, omega=2. / 3.),
               "red_black_sweep": lambda: plan.smooth(0, _lib.GS_MC, 1, omega=1.0),
               "residual_restrict": lambda: plan.residual_restrict(0),
               "apply": lambda: plan.apply(0, (_lib.SLOT_V, 0), (_lib.SLOT_T, 0))}
        out = {"bench": "point_bonds_passes", "which": a.which, "g": g, "reps": a.reps, "tree": os.path.abspath(a.tree),
               "device": _lib.device_name(0), "operator_kind": plan.operator_kind(0)}
        out["ms"] = {n: round(timed(plan, fn, a.reps), 5) for n, fn in fns.items()}
        col = 0 if a.which == "yardstick" else 1
        out["fraction_of_8TBs"] = {n: round(BYTES[n][col] * float(g) * g / (out["ms"][n] * 1e-3) / PEAK, 3) for n in BYTES}
        print(json.dumps(out), flush=True)
    finally:
        plan.close()


def run_cycles(a):
    for g in a.g:
        for which in ("march", "flat", "yardstick"):
            plan, _lib = make_plan(which, g, a.lowest, a.tree)
            try:
                out = {"bench": "point_bonds_cycles", "which": which, "g": g, "cycles": a.cycles, "device": _lib.device_name(0)}
                for name, kind, omega in (("wjacobi", _lib.WJACOBI, 2. / 3.), ("red_black", _lib.GS_MC, 1.0)):
                    out["cycle_" + name + "_ms"] = round(timed(plan, lambda: plan.vcycle(2, 2, kind, omega=omega, k=1, nu_coarse=2), a.cycles), 4)
                print(json.dumps(out), flush=True)
            finally:
                plan.close()


def run_ab(a):
    """alternate the parent checkout's yardstick and this tree's three forms, one process each, `rounds` times"""
    me = os.path.abspath(__file__)
    runs = [("parent", a.parent, "yardstick"), ("branch", ROOT, "march"), ("branch", ROOT, "flat"), ("branch", ROOT, "yardstick")]
    got = {}
    for r in range(a.rounds):
        for side, tree, which in runs:
            cmd = [sys.executable, me, "passes", "--which", which, "--g", str(a.g[0]), "--reps", str(a.reps), "--lowest", str(a.lowest), "--tree", tree]
            line = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=a.timeout).stdout.decode().strip().splitlines()[-1]
            rec = json.loads(line)
            rec["side"], rec["round"] = side, r
            got.setdefault((side, which), []).append(rec["ms"])
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
    med = {"%s_%s" % k: {n: statistics.median(x[n] for x in v) for n in v[0]} for k, v in got.items()}
    spread = {"%s_%s" % k: {n: round(max(x[n] for x in v) / min(x[n] for x in v), 3) for n in v[0]} for k, v in got.items()}
    acc = {}
    pts = float(a.g[0]) ** 2
    for name, (b0, b1) in BYTES.items():
        tp, tm, tf = med["parent_yardstick"][name], med["branch_march"][name], med["branch_flat"][name]
        ratio, allowed = tm / tp, 1.10 * b1 / b0
        acc[name] = {"bytes_yardstick": b0, "bytes_bonds": b1, "t_parent_yardstick_ms": tp, "t_march_ms": tm, "t_flat_ms": tf,
                     "ratio": round(ratio, 3), "allowed": round(allowed, 3), "verdict": "met" if ratio <= allowed else "missed",
                     "march_fraction_of_8TBs": round(b1 * pts / (tm * 1e-3) / PEAK, 3), "march_faster_than_flat": bool(tm < tf)}
    rec = {"bench": "point_bonds_ab", "g": a.g[0], "rounds": a.rounds, "median_ms": med, "max_over_min": spread, "acceptance": acc}
    print(json.dumps(rec), flush=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["passes", "cycles", "ab"])
    ap.add_argument("--which", default="march", choices=["march", "flat", "yardstick"])
    ap.add_argument("--g", type=int, nargs="+", default=None)
    ap.add_argument("--lowest", type=int, default=8)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=240.0, help="ab: seconds one measurement process may take")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package (and built library) is measured")
    ap.add_argument("--parent", default=None, help="ab: a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_point_bonds.jsonl"))
    a = ap.parse_args()
    if a.g is None:
        a.g = [4096, 8192] if a.mode == "cycles" else [8192]
    if a.mode == "passes":
        run_passes(a)
    elif a.mode == "cycles":
        run_cycles(a)
    else:
        if not a.parent:
            ap.error("ab needs --parent DIR")
        run_ab(a)


if __name__ == "__main__":
    main()
