"""2-D cycles with a per-point 9-point stencil (mgcmt_plan_create_nine, fp64): the passes of a nine-plane level one by one — two
weighted-Jacobi sweeps, two four-colour sweeps (mgcmt_time_smoother, nu = 2) and residual + restriction — in the tile form
(csrc/kernels_nine_tile.hip) and the flat form (csrc/kernels_pointwise.hip), and whole V(2,2) cycles with both smoothers.

    python scripts/bench_nine_point.py passes --which tile|flat [--g 4096] [--reps 50]
    python scripts/bench_nine_point.py passes --which galerkin_tile|galerkin_flat [--g 8192] [--tree DIR]
    python scripts/bench_nine_point.py cycles [--g 4096 8192] [--cycles 20]
    python scripts/bench_nine_point.py ab --parent DIR [--rounds 3] [--out profiles/r10_nine_point.jsonl]

`tile` / `flat`: level 0 of a tensor plan of --g (MGCMT_NINE_TILE unset / 0).  `galerkin_*`: level 1 of a potential_operator
plan of --g, a nine-plane level of (g/2)^2 points over general Kronecker terms — `galerkin_flat` uses nothing newer than the
point-diagonal plans, so `--tree DIR` can point it at a built checkout of an earlier commit (the yardstick); `galerkin_tile`
sets MGCMT_NINE_TILE=2.  `ab` alternates the parent checkout's galerkin_flat with this tree's four forms, one process per
measurement, and prints the medians with the rule "a pass whose tile form is slower than 1.03 x its flat time stays flat".
One JSON line per measurement.  Compulsory bytes per point of the level are kept here."""
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
# compulsory bytes per point of the level and pass (nu = 2): (flat, tile)
BYTES = {"wjacobi_2": (192, 96),             # flat: two sweeps of v, f, nine planes in, v' out; tile: one launch for the pair
         "four_colour_2": (192, 192),        # a sweep reads v, f, the planes and writes v' once in either form (the flat stages at half-line granularity)
         "residual_restrict": (108, 92)}     # flat: residual 96 (v, f, planes; r) + restriction 10 + clearing V[l+1] 2; tile: 88 + F[l+1] and V[l+1]
SLOWER = 1.03                                # the pool's box-to-box spread


def timed(plan, fn, reps):
    for _ in range(3):
        fn()
    plan.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    plan.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def tensor_fields(g):
    """a rotated anisotropic dot: inside a disc the principal values (4 with 20 % disorder, 1) on axes turned by 0.6, W = I outside"""
    x = (np.arange(g) + 0.5) / g - 0.5
    X, Y = np.meshgrid(x, x, indexing="ij", sparse=True)
    inside = (X - 0.05) ** 2 + (Y + 0.1) ** 2 < 0.3 ** 2
    l1 = np.where(inside, 4.0 * (1.0 + 0.2 * np.random.RandomState(2).rand(g, g)), 1.0)
    theta = np.where(inside, 0.6, 0.0)
    c, s = np.cos(theta), np.sin(theta)
    return c * c * l1 + s * s, s * s * l1 + c * c, c * s * (l1 - 1.0)


def make_plan(which, g, lowest, tree):
    sys.path.insert(0, tree)
    from multigridcmt_amd import _lib, operators
    from multigridcmt_amd.plan import Plan
    if which.startswith("galerkin"):
        x = (np.arange(g) + 0.5) / g - 0.5
        X, Y = np.meshgrid(x, x, indexing="ij", sparse=True)
        V = 40.0 * (X * X + X * Y + Y * Y) + 5.0 * np.random.RandomState(1).rand(g, g)
        if which == "galerkin_tile":
            os.environ["MGCMT_NINE_TILE"] = "2"
        else:
            os.environ.pop("MGCMT_NINE_TILE", None)
        plan, level = Plan(operators.potential_operator(g, V), lowest, nvec=1), 1
    else:
        if which == "flat":
            os.environ["MGCMT_NINE_TILE"] = "0"
        else:
            os.environ.pop("MGCMT_NINE_TILE", None)
        plan, level = Plan(operators.tensor_mass_operator(g, *tensor_fields(g)), lowest, nvec=1), 0
    plan.set_shifts([0.0])
    rng = np.random.RandomState(0)
    n = plan.size(level)
    plan.upload(level, _lib.SLOT_F, 0, rng.rand(n))
    plan.upload(level, _lib.SLOT_V, 0, rng.rand(n))
    return plan, level, _lib


def run_passes(a):
    plan, level, _lib = make_plan(a.which, a.g[0], a.lowest, a.tree)
    try:
        gl = a.g[0] >> level
        tiled = bool(plan.level_tiled(level)) if hasattr(plan, "level_tiled") else False
        out = {"bench": "nine_point_passes", "which": a.which, "g": a.g[0], "level": level, "level_g": gl, "reps": a.reps, "tree": os.path.abspath(a.tree),
               "device": _lib.device_name(0), "operator_kind": plan.operator_kind(level), "tiled": tiled}
        for kind, omega in ((_lib.WJACOBI, 2. / 3.), (_lib.GS_MC, 1.0)):
            plan.time_smoother(level, kind, 2, omega, 3)          # warm-up
        # (mgcmt_time_smoother returns the time of all `reps` calls between two HIP events)
        ms = {"wjacobi_2": plan.time_smoother(level, _lib.WJACOBI, 2, 2. / 3., a.reps) / a.reps,
              "four_colour_2": plan.time_smoother(level, _lib.GS_MC, 2, 1.0, a.reps) / a.reps,
              "residual_restrict": timed(plan, lambda: plan.residual_restrict(level), a.reps)}
        out["ms"] = {n: round(v, 5) for n, v in ms.items()}
        col = 1 if tiled else 0
        out["fraction_of_8TBs"] = {n: round(BYTES[n][col] * float(gl) * gl / (out["ms"][n] * 1e-3) / PEAK, 3) for n in BYTES}
        print(json.dumps(out), flush=True)
    finally:
        plan.close()


def run_cycles(a):
    for g in a.g:
        for which in ("tile", "flat"):
            plan, _, _lib = make_plan(which, g, a.lowest, a.tree)
            try:
                out = {"bench": "nine_point_cycles", "which": which, "g": g, "cycles": a.cycles, "device": _lib.device_name(0), "tiled": bool(plan.level_tiled(0))}
                for name, kind, omega in (("wjacobi", _lib.WJACOBI, 2. / 3.), ("four_colour", _lib.GS_MC, 1.0)):
                    out["cycle_" + name + "_ms"] = round(timed(plan, lambda: plan.vcycle(2, 2, kind, omega=omega, k=1, nu_coarse=2), a.cycles), 4)
                print(json.dumps(out), flush=True)
            finally:
                plan.close()


def run_ab(a):
    """alternate the parent checkout's flat Galerkin level and this tree's forms, one process each, `rounds` times"""
    me = os.path.abspath(__file__)
    gg, gt = str(a.g[0]), str(a.g[0] // 2)
    runs = [("parent", a.parent, "galerkin_flat", gg), ("branch", ROOT, "galerkin_tile", gg), ("branch", ROOT, "galerkin_flat", gg),
            ("branch", ROOT, "tile", gt), ("branch", ROOT, "flat", gt)]
    got = {}
    for r in range(a.rounds):
        for side, tree, which, g in runs:
            # (the parent has no bench_nine_point.py: this file runs against its package)
            cmd = [sys.executable, me, "passes", "--which", which, "--g", g, "--reps", str(a.reps), "--lowest", str(a.lowest), "--tree", tree]
            line = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, timeout=a.timeout).stdout.decode().strip().splitlines()[-1]
            rec = json.loads(line)
            rec["side"], rec["round"] = side, r
            got.setdefault((side, which), []).append(rec["ms"])
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
    med = {"%s_%s" % k: {n: statistics.median(x[n] for x in v) for n in v[0]} for k, v in got.items()}
    spread = {"%s_%s" % k: {n: round(max(x[n] for x in v) / min(x[n] for x in v), 3) for n in v[0]} for k, v in got.items()}
    rule = {}
    for name in BYTES:
        tp, gt_, gf = med["parent_galerkin_flat"][name], med["branch_galerkin_tile"][name], med["branch_galerkin_flat"][name]
        t0, f0 = med["branch_tile"][name], med["branch_flat"][name]
        rule[name] = {"t_parent_flat_ms": tp, "t_galerkin_tile_ms": gt_, "t_galerkin_flat_ms": gf, "galerkin_tile_over_parent": round(gt_ / tp, 3),
                      "t_level0_tile_ms": t0, "t_level0_flat_ms": f0, "level0_tile_over_flat": round(t0 / f0, 3),
                      "level0_default": "flat" if t0 > SLOWER * f0 else "tile"}
    rec = {"bench": "nine_point_ab", "g": a.g[0], "rounds": a.rounds, "median_ms": med, "max_over_min": spread, "rule": rule}
    print(json.dumps(rec), flush=True)
    with open(a.out, "a") as fh:
        fh.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["passes", "cycles", "ab"])
    ap.add_argument("--which", default="tile", choices=["tile", "flat", "galerkin_tile", "galerkin_flat"])
    ap.add_argument("--g", type=int, nargs="+", default=None)
    ap.add_argument("--lowest", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=240.0, help="ab: seconds one measurement process may take")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package (and built library) is measured")
    ap.add_argument("--parent", default=None, help="ab: a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_nine_point.jsonl"))
    a = ap.parse_args()
    if a.g is None:
        a.g = [4096, 8192] if a.mode == "cycles" else [8192] if (a.mode == "ab" or a.which.startswith("galerkin")) else [4096]
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
