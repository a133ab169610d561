"""V-cycle-preconditioned conjugate gradients (MGCMTSolver.solve, mgcmt_pcg_*) at size: 4096^2 and 8192^2 (the Laplacian at
shift 1.9) and 256^3 (variable effective mass, a ball of inverse mass 1000).  Per size, one JSON line with

  * ms per iteration, split into the cycle, the operator application and each new pass (mgcmt_pcg_time_pass: the pass with the
    scalar kernel behind it), and the whole iteration timed as queued (generic passes, and the marching direction pass where
    the level takes it);
  * each new pass's achieved TB/s against its compulsory bytes per point (dots 24, direction 24, curvature 16, update 48;
    the fused direction pass 32) beside the triad figure of mgcmt_bandwidth_probe from the same run (24 B per point; a 3-D
    plan has no probe: the 2-D plan with as many points gives it);
  * time to rtol = 1e-8 by the solve against the same plan's plain cycles (capped at 200), with the counts.

``--ab N`` (default 5): marching against generic at the largest 2-D size, alternating, N runs each, medians of the ms per
iteration.  Everything goes to stdout; ``--out FILE`` appends the JSON lines to a file as well.

    python scripts/bench_pcg.py [--cases 2d:4096,2d:8192,3d:256] [--smoother wjacobi|rb] [--ab 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multigridcmt_amd import _lib, laplacian_operator, variable_mass_operator  # noqa: E402
from multigridcmt_amd.plan import Plan  # noqa: E402

SCALE = -1 / np.pi ** 2
V, F, W = _lib.SLOT_V, _lib.SLOT_F, _lib.SLOT_W
VECS = [0, 1, 2, 3]
FCOPY, RES = 4, 5          # columns of slot W: the right-hand side kept on the device (every timed region copies it from there), a residual
PASSES = [("dots", _lib.PCG_PASS_DOTS, 24), ("direction", _lib.PCG_PASS_DIRECTION, 24), ("curvature", _lib.PCG_PASS_CURVATURE, 16),
          ("update", _lib.PCG_PASS_UPDATE, 48), ("march", _lib.PCG_PASS_MARCH, 32)]


def ball(g):
    x = np.arange(g) + 0.5 - g / 2
    Z, Y, X = np.meshgrid(x, x, x, indexing="ij", sparse=True)
    return np.where(Z * Z + Y * Y + X * X < (g / 4) ** 2, 1000.0, 1.0)


def make_case(dim, g):
    if dim == "2d":
        return laplacian_operator(g, "2d") * SCALE, 1.9, 4
    return variable_mass_operator(g, ball(g), dimension="3d"), 0.0, 8


def timed(plan, fn, reps):
    fn()
    plan.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    plan.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def begin(plan, f, rtol, flexible, march):
    plan.set_option(_lib.OPT_PCG_MARCH, march)
    plan.copy(0, W, FCOPY, F, 0)
    plan.pcg_begin(VECS, rtol, zero_start=True, flexible=flexible)


def iteration_ms(plan, f, kind, omega, flexible, march, reps):
    """ms per queued iteration (rtol = 0: nothing stops), the first two iterations (graph capture) untimed"""
    begin(plan, f, 0.0, flexible, march)
    plan.pcg_iterate(2, 2, 2, kind, omega=omega)
    plan.sync()
    t0 = time.perf_counter()
    plan.pcg_iterate(reps, 2, 2, kind, omega=omega)
    plan.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def solve(plan, f, kind, omega, flexible, march, rtol, maxiter=200, check_every=4):
    plan.sync()
    t0 = time.perf_counter()
    begin(plan, f, rtol, flexible, march)
    queued, status = 0, _lib.PCG_RUNNING
    while status == _lib.PCG_RUNNING and queued < maxiter:
        plan.pcg_iterate(check_every, 2, 2, kind, omega=omega)
        queued += check_every
        status = plan.pcg_status()[1]
    ms = (time.perf_counter() - t0) * 1e3
    its, status, indefinite, fnorm, hist = plan.pcg_status(history=maxiter)
    return {"ms": ms, "iterations": its, "converged": status == _lib.PCG_CONVERGED, "indefinite": indefinite,
            "residual": float(hist[its - 1] / fnorm) if its else None}


def plain_cycles(plan, f, kind, omega, rtol, cap=200, check_every=4):
    """the same plan's plain V(2,2) cycles to the same tolerance: the residual norm is read every `check_every` cycles (one
    application, one axpy, one synchronising dot each), as a caller's loop would"""
    fnorm = float(np.linalg.norm(f))
    plan.sync()
    t0 = time.perf_counter()
    plan.copy(0, W, FCOPY, F, 0)
    cycles, res = 0, 1.0
    while cycles < cap:
        for _ in range(check_every):
            plan.vcycle(2, 2, kind, omega=omega, zero_start=cycles == 0)
            cycles += 1
        plan.apply(0, (V, 0), (W, RES), with_shift=True)
        plan.axpy(0, -1.0, (W, FCOPY), (W, RES))
        res = np.sqrt(plan.dot(0, (W, RES), (W, RES))) / fnorm
        if not res > rtol:
            break
    return {"ms": (time.perf_counter() - t0) * 1e3, "cycles": cycles, "converged": bool(res <= rtol), "residual": float(res)}


def bench_case(dim, g, smoother, reps, rtol):
    op, shift, lowest = make_case(dim, g)
    kind, omega, flexible = (_lib.WJACOBI, 2.0 / 3.0, False) if smoother == "wjacobi" else (_lib.GS_MC, 1.0, True)
    plan = Plan(op, lowest, nvec=6)
    plan.set_shifts([shift])
    n = plan.size(0)
    f = np.random.RandomState(1).rand(n)
    plan.upload(0, W, FCOPY, f)
    rec = {"case": "%s:%d" % (dim, g), "points": n, "smoother": smoother, "shift": shift, "device": _lib.device_name(0)}
    # the triad ceiling of this run
    if dim == "2d":
        triad_ms = plan.bandwidth_probe(0, 1, 1024, 5)
    else:
        side = int(round(n ** 0.5))
        probe = Plan(laplacian_operator(side, "2d") * SCALE, side, nvec=1) if side * side == n else None
        triad_ms = probe.bandwidth_probe(0, 1, 1024, 5) if probe else None
        if probe:
            probe.close()
    rec["triad_TBs"] = n * 24 / (triad_ms * 1e-3) / 1e12 if triad_ms else None
    # the pieces of an iteration
    begin(plan, f, 0.0, flexible, 0)
    plan.pcg_iterate(2, 2, 2, kind, omega=omega)
    pieces = {"cycle": timed(plan, lambda: plan.vcycle(2, 2, kind, omega=omega, zero_start=True), reps),
              "apply": timed(plan, lambda: plan.apply(0, (W, 1), (W, 2), with_shift=False), reps)}
    passes = {}
    for name, which, bpp in PASSES:
        begin(plan, f, 0.0, flexible, 0)
        plan.pcg_iterate(2, 2, 2, kind, omega=omega)
        try:
            ms = plan.pcg_time_pass(which, reps)
        except _lib.MgcmtError:
            continue                                # (the march does not cover this level)
        pieces[name] = ms
        passes[name] = {"ms": ms, "bytes_per_point": bpp, "TBs": n * bpp / (ms * 1e-3) / 1e12,
                        "of_triad": (n * bpp / (ms * 1e-3) / 1e12) / rec["triad_TBs"] if rec["triad_TBs"] else None}
    rec["ms_pieces"], rec["passes"] = pieces, passes
    rec["ms_per_iteration_generic"] = iteration_ms(plan, f, kind, omega, flexible, 0, reps)
    if "march" in passes:
        rec["ms_per_iteration_march"] = iteration_ms(plan, f, kind, omega, flexible, 1, reps)
    # to a tolerance: the solve against plain cycles
    rec["solve"] = solve(plan, f, kind, omega, flexible, -1, rtol)     # (-1: the library's default choice of the direction pass)
    rec["plain"] = plain_cycles(plan, f, kind, omega, rtol)
    return rec, plan, (f, kind, omega, flexible)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2d:4096,2d:8192,3d:256")
    ap.add_argument("--smoother", default="wjacobi", choices=["wjacobi", "rb"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--ab", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    cases = [c.split(":") for c in args.cases.split(",") if c]
    largest_2d = max((int(g) for d, g in cases if d == "2d"), default=None)
    for dim, g in cases:
        rec, plan, (f, kind, omega, flexible) = bench_case(dim, int(g), args.smoother, args.reps, args.rtol)
        emit(rec)
        if dim == "2d" and int(g) == largest_2d and args.ab > 0 and "march" in rec["passes"]:
            runs = {0: [], 1: []}
            for _ in range(args.ab):
                for march in (0, 1):
                    runs[march].append(iteration_ms(plan, f, kind, omega, flexible, march, args.reps))
            emit({"case": rec["case"], "ab": "march against generic, alternating, ms per iteration", "smoother": args.smoother,
                  "generic": runs[0], "march": runs[1], "median_generic": statistics.median(runs[0]), "median_march": statistics.median(runs[1])})
        plan.close()


if __name__ == "__main__":
    main()
