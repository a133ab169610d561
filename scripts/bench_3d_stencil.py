"""3-D cycles with a per-point 27-point stencil (a tensor effective mass, mgcmt_plan_create3d_stencil; fp64): the passes of a
256^3 27-plane level with nu = 2 — the eight-colour sweep, the weighted-Jacobi sweep, residual + restriction — on the flat
kernels and on those of csrc/kernels_3d_stencil.hip (MGCMT_3D_STENCIL_TILE), with each new pass's compulsory bytes per point
and the rule "slower than 1.03 x flat stays flat"; whole V(2,2) cycles with both smoothers.

    python scripts/bench_3d_stencil.py one --plan tensor --g 256 --tile 1          # one measurement, one JSON line
    python scripts/bench_3d_stencil.py one --plan point --g 512 --level 1 --tile 2
    python scripts/bench_3d_stencil.py ab --parent DIR [--rounds 3] [--out FILE]   # the whole table

`one` measures in this process: level 0 of a tensor plan of g^3 points ("tensor") or level `--level` of a point-diagonal plan
("point": its Galerkin levels are 27-plane levels with general Kronecker terms).  `ab` starts one process per measurement,
a built checkout of the parent commit (--parent: its flat kernels on level 1 of the 512^3 point-diagonal plan) alternating with
this tree, --rounds times, and prints medians with max / min.  Times are device-synchronised wall-clock averages of --reps
back-to-back calls after a warm-up call.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK = 8.0e12  # bytes/s, MI355X HBM3E


def compulsory_bytes(nu):
    """bytes per point of a 27-plane level that each pass has to move, from the shapes: 27 coefficient planes, v and f"""
    planes, dbl = 27, 8
    return {
        # every stage reads the coefficients and f of its own points (1/8 of the level each), reads v and writes its points
        "colour_sweep": nu * (planes * dbl + dbl + 2 * dbl),
        "wjacobi_sweep": nu * (planes * dbl + 3 * dbl),              # coefficients, v, f read, v' written
        "residual_restrict": planes * dbl + 2 * dbl + 2 * dbl / 8,   # coefficients, v, f read; F and V of the level below written
    }


def dot_profile(g):
    """An L-valley-like ellipsoid (principal inverse masses 1 / 0.35 / 0.6) whose axes turn with position, inside an ellipsoidal
    dot with a smeared interface, blended into 0.73 I outside; V = 30 s.  Index [z, y, x]; (wxx, wyy, wzz, wxy, wxz, wyz, V)."""
    t = ((np.arange(g) + 0.5) / g - 0.5)
    Z, Y, X = np.meshgrid(t, t, t, indexing="ij")
    s = 0.5 * (1.0 + np.tanh((np.sqrt((X - 0.05) ** 2 + ((Y + 0.03) / 0.8) ** 2 + ((Z - 0.02) / 0.6) ** 2) - 0.3) / 0.08))
    th, ph = 0.6 + 0.8 * Z, 0.4 - 0.5 * X
    c, sn, cp, sp_ = np.cos(th), np.sin(th), np.cos(ph), np.sin(ph)
    # columns of R = Rz(th) Rx(ph), components (x, y, z)
    e = [(c, sn, 0.0 * c), (-sn * cp, c * cp, sp_), (sn * sp_, -c * sp_, cp)]
    lam = (1.0, 0.35, 0.6)
    w = {}
    for name, (i, j) in (("xx", (0, 0)), ("yy", (1, 1)), ("zz", (2, 2)), ("xy", (0, 1)), ("xz", (0, 2)), ("yz", (1, 2))):
        inside = sum(l * ek[i] * ek[j] for l, ek in zip(lam, e))
        w[name] = (1.0 - s) * inside + s * (0.73 if i == j else 0.0)
    return w["xx"], w["yy"], w["zz"], w["xy"], w["xz"], w["yz"], 30.0 * s


def timed(plan, fn, reps):
    fn()
    plan.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    plan.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def one(a):
    sys.path.insert(0, a.root)
    if a.tile is None:
        os.environ.pop("MGCMT_3D_STENCIL_TILE", None)
    else:
        os.environ["MGCMT_3D_STENCIL_TILE"] = str(a.tile)
    from multigridcmt_amd import _lib
    from multigridcmt_amd._lib import GS_MC, SLOT_F, SLOT_V, WJACOBI
    from multigridcmt_amd.plan import Plan
    g, lv = a.g, a.level
    if a.plan == "tensor":
        from multigridcmt_amd.operators import tensor_mass_operator
        wxx, wyy, wzz, wxy, wxz, wyz, V = dot_profile(g)
        op = tensor_mass_operator(g, wxx, wyy, wxy, V=V, wzz=wzz, wxz=wxz, wyz=wyz, dimension="3d")
        del wxx, wyy, wzz, wxy, wxz, wyz, V
    else:
        from multigridcmt_amd.operators import potential_operator
        op = potential_operator(g, dot_profile(g)[6], dimension="3d")
    t0 = time.perf_counter()
    plan = Plan(op, a.lowest, nvec=1)
    plan.sync()
    out = {"plan": a.plan, "g": g, "level": lv, "tile": a.tile, "root": os.path.basename(os.path.abspath(a.root)), "nu": a.nu,
           "plan_create_s": round(time.perf_counter() - t0, 2), "device": _lib.device_name(0)}
    try:
        if hasattr(plan, "level_path_3d"):
            out["level_path"] = list(plan.level_path_3d(lv))
        n = (g >> lv) ** 3
        rng = np.random.RandomState(0)
        plan.set_shifts([0.0])
        plan.upload(lv, SLOT_F, 0, rng.rand(n))
        plan.upload(lv, SLOT_V, 0, rng.rand(n))
        fns = {"colour_sweep": lambda: plan.smooth(lv, GS_MC, a.nu, omega=1.0),
               "wjacobi_sweep": lambda: plan.smooth(lv, WJACOBI, a.nu, omega=2. / 3.),
               "residual_restrict": lambda: plan.residual_restrict(lv)}
        out["passes_ms"] = {k: round(timed(plan, fn, a.reps), 4) for k, fn in fns.items()}
        by = compulsory_bytes(a.nu)
        out["bytes_per_point"] = by
        out["fraction_of_8TBs"] = {k: round(by[k] * n / (out["passes_ms"][k] * 1e-3) / PEAK, 3) for k in by}
        if a.cycles and lv == 0:
            f = rng.rand(n)
            plan.upload(0, SLOT_F, 0, f)
            for name, kind, omega in (("wjacobi", WJACOBI, 2. / 3.), ("eight_colour", GS_MC, 1.0)):
                plan.upload(0, SLOT_V, 0, np.zeros(n))
                out["cycle_" + name + "_ms"] = round(timed(plan, lambda: plan.vcycle(2, 2, kind, omega=omega, k=1, nu_coarse=4), a.cycles), 4)
    finally:
        plan.close()
    print(json.dumps(out), flush=True)


def ab(a):
    me = os.path.abspath(__file__)
    runs = [("parent_point512_l1_flat", a.parent, ["--plan", "point", "--g", "512", "--level", "1"]),
            ("tree_point512_l1_flat", HERE, ["--plan", "point", "--g", "512", "--level", "1", "--tile", "0"]),
            ("tree_point512_l1_new", HERE, ["--plan", "point", "--g", "512", "--level", "1", "--tile", "2"]),
            ("tree_tensor256_flat", HERE, ["--plan", "tensor", "--g", "256", "--tile", "0", "--cycles", str(a.cycles)]),
            ("tree_tensor256_new", HERE, ["--plan", "tensor", "--g", "256", "--tile", "2", "--cycles", str(a.cycles)]),
            ("tree_tensor128_flat", HERE, ["--plan", "tensor", "--g", "128", "--tile", "0", "--cycles", str(a.cycles)]),
            ("tree_tensor128_new", HERE, ["--plan", "tensor", "--g", "128", "--tile", "2", "--cycles", str(a.cycles)])]
    rows = {name: [] for name, _, _ in runs}
    for rnd in range(a.rounds):
        for name, root, args in runs:
            cmd = [sys.executable, me, "one", "--root", root, "--reps", str(a.reps), "--nu", str(a.nu)] + args
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=a.timeout)
            text = r.stdout.decode()
            if r.returncode:          # nothing more is started on the device after a failure
                sys.stderr.write(text)
                raise SystemExit("measurement %s failed with status %d" % (name, r.returncode))
            rec = json.loads(text.strip().splitlines()[-1])
            rec["name"], rec["round"] = name, rnd
            rows[name].append(rec)
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")
    summary = {}
    for name, recs in rows.items():
        keys = list(recs[0]["passes_ms"]) + [k for k in recs[0] if k.startswith("cycle_")]
        summary[name] = {}
        for k in keys:
            vals = sorted((r["passes_ms"][k] if k in r["passes_ms"] else r[k]) for r in recs)
            summary[name][k] = {"median": vals[len(vals) // 2], "min": vals[0], "max": vals[-1]}
    line = json.dumps({"summary": summary, "rounds": a.rounds, "reps": a.reps, "nu": a.nu})
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    o = sub.add_parser("one")
    o.add_argument("--root", default=HERE)
    o.add_argument("--plan", choices=["tensor", "point"], default="tensor")
    o.add_argument("--g", type=int, default=256)
    o.add_argument("--level", type=int, default=0)
    o.add_argument("--lowest", type=int, default=8)
    o.add_argument("--tile", type=int, default=None)
    o.add_argument("--nu", type=int, default=2)
    o.add_argument("--reps", type=int, default=20)
    o.add_argument("--cycles", type=int, default=0)
    b = sub.add_parser("ab")
    b.add_argument("--parent", required=True)
    b.add_argument("--rounds", type=int, default=3)
    b.add_argument("--reps", type=int, default=20)
    b.add_argument("--nu", type=int, default=2)
    b.add_argument("--cycles", type=int, default=8)
    b.add_argument("--timeout", type=int, default=400)
    b.add_argument("--out", default=None)
    a = ap.parse_args()
    one(a) if a.cmd == "one" else ab(a)


if __name__ == "__main__":
    main()
