"""k shifted systems at once (MGCMTSolver.solve_matrix, mgcmt_pcg_*_k) against k consecutive MGCMTSolver.solve calls.  Cases:
the Laplacian at 4096^2 with k = 1, 4, 8, 16 shifts spread around 1.9; the same at 256^2 with k = 16 (the launch-bound end);
128^3 variable effective mass (a ball of inverse mass 1000), k = 4.  Per case one JSON line with

  * wall time from upload to download to rtol = 1e-8: one batched solve against k consecutive single solves (medians of
    ``--runs`` alternating runs on warm plans; both include every transfer and status read), with the iteration counts;
  * ms per queued iteration of the batched solve (rtol = 0: no column stops) beside k times the single solve's;
  * per pass (mgcmt_pcg_time_pass: the pass on all k columns with its scalar kernel), the k-column cycle and the k-column
    operator application: ms batched, ms single, and the ratio batched / (k * single);
  * the triad figure of mgcmt_bandwidth_probe from the same run (a 3-D plan has no probe: a 2-D plan of as many points gives it).

    python scripts/bench_pcg_matrix.py [--cases 2d:4096:1,2d:4096:4,2d:4096:8,2d:4096:16,2d:256:16,3d:128:4] [--smoother wjacobi|rb]
                                       [--runs 3] [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, _lib, laplacian_operator, variable_mass_operator  # noqa: E402
from multigridcmt_amd.plan import Plan  # noqa: E402

SCALE = -1 / np.pi ** 2
V, F, W = _lib.SLOT_V, _lib.SLOT_F, _lib.SLOT_W
PASSES = [("dots", _lib.PCG_PASS_DOTS, 24), ("direction", _lib.PCG_PASS_DIRECTION, 24), ("curvature", _lib.PCG_PASS_CURVATURE, 16),
          ("update", _lib.PCG_PASS_UPDATE, 48), ("march", _lib.PCG_PASS_MARCH, 32)]


def ball(g):
    x = np.arange(g) + 0.5 - g / 2
    Z, Y, X = np.meshgrid(x, x, x, indexing="ij", sparse=True)
    return np.where(Z * Z + Y * Y + X * X < (g / 4) ** 2, 1000.0, 1.0)


def make_case(dim, g, k):
    if dim == "2d":
        return laplacian_operator(g, "2d") * SCALE, 1.9 + 0.004 * (np.arange(k) - (k - 1) / 2.0), 4
    return variable_mass_operator(g, ball(g), dimension="3d"), np.zeros(k), 8


def timed(plan, fn, reps):
    fn()
    plan.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    plan.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def pieces(op, lowest, shifts, fm, k, kind, omega, flexible, reps):
    """ms of one queued iteration and of its parts on k columns (k = 1: the single solve's kernels, through the same entries)"""
    plan = Plan(op, lowest, nvec=4 * k)
    plan.set_shifts(shifts[:k])
    vecs = [0, k, 2 * k, 3 * k]

    def begin():
        for c in range(k):
            plan.upload(0, F, c, fm[:, c])
        plan.pcg_begin_k(k, vecs, 0.0, zero_start=True, flexible=flexible)        # rtol = 0: no column stops
        plan.pcg_iterate_k(2, 2, 2, kind, omega=omega)                            # (the second cycle captures the graph)
    begin()
    plan.sync()
    t0 = time.perf_counter()
    plan.pcg_iterate_k(reps, 2, 2, kind, omega=omega)
    plan.sync()
    out = {"iteration": (time.perf_counter() - t0) * 1e3 / reps}
    for name, which, _ in PASSES:
        begin()
        try:
            out[name] = plan.pcg_time_pass(which, reps)
        except _lib.MgcmtError:
            continue                                # (the march does not cover this level)
    begin()
    out["cycle"] = timed(plan, lambda: plan.vcycle(2, 2, kind, omega=omega, k=k, zero_start=True), reps)
    plan.close()
    return out


def bench_case(dim, g, k, smoother, runs, reps, rtol):
    op, shifts, lowest = make_case(dim, g, k)
    solver, sm = MGCMTSolver(), MGCMTStencilMaker()
    smo = solver.wjacobi if smoother == "wjacobi" else solver.gseidel_rb
    kind, omega, flexible = (_lib.WJACOBI, 2.0 / 3.0, False) if smoother == "wjacobi" else (_lib.GS_MC, 1.0, True)
    n = op.shape[0]
    fm = np.random.RandomState(1).rand(n, k)
    rec = {"case": "%s:%d:%d" % (dim, g, k), "points": n, "k": k, "smoother": smoother, "shifts": [float(s) for s in shifts],
           "device": _lib.device_name(0)}
    side = g if dim == "2d" else int(round(n ** 0.5))
    if side * side == n:
        probe = Plan(laplacian_operator(side, "2d") * SCALE, side, nvec=1)
        rec["triad_TBs"] = n * 24 / (probe.bandwidth_probe(0, 1, 1024, 5) * 1e-3) / 1e12
        probe.close()
    kw = dict(nu1=2, nu2=2, smoother=smo, lowest_level=lowest, dimension=dim, rtol=rtol, maxiter=200)

    def batched():
        info = {}
        t0 = time.perf_counter()
        solver.solve_matrix(fm, op, sm, shifts=shifts, info=info, **kw)
        return (time.perf_counter() - t0) * 1e3, info

    def consecutive():
        its = []
        t0 = time.perf_counter()
        for c in range(k):
            info = {}
            solver.solve(fm[:, c], op, sm, shift=float(shifts[c]), info=info, **kw)
            its.append(info["iterations"])
        return (time.perf_counter() - t0) * 1e3, its
    batched()
    consecutive()                                   # warm plans, captured graphs, page-locked buffers
    tb, tc = [], []
    for _ in range(runs):
        ms, info = batched()
        tb.append(ms)
        ms, its = consecutive()
        tc.append(ms)
    rec["solve_ms_batched"], rec["solve_ms_consecutive"] = statistics.median(tb), statistics.median(tc)
    rec["solve_ms_batched_runs"], rec["solve_ms_consecutive_runs"] = tb, tc
    rec["batched_over_consecutive"] = rec["solve_ms_batched"] / rec["solve_ms_consecutive"]
    rec["iterations_batched"], rec["iterations_consecutive"] = info["iterations"], its
    rec["status"], rec["true_residual_max"] = sorted(set(info["status"])), max(info["true_residual"])
    from multigridcmt_amd import plan as plan_module
    plan_module.release_plans()
    pk = pieces(op, lowest, shifts, fm, k, kind, omega, flexible, reps)
    p1 = pk if k == 1 else pieces(op, lowest, shifts, fm, 1, kind, omega, flexible, reps)
    rec["ms_pieces"] = {name: {"batched": pk[name], "single": p1[name], "ratio_to_k_singles": pk[name] / (k * p1[name])} for name in pk if name in p1}
    for name, _, bpp in PASSES:
        if name in pk:
            rec["ms_pieces"][name]["TBs_batched"] = k * n * bpp / (pk[name] * 1e-3) / 1e12
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="2d:4096:1,2d:4096:4,2d:4096:8,2d:4096:16,2d:256:16,3d:128:4")
    ap.add_argument("--smoother", default="wjacobi", choices=["wjacobi", "rb"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for case in [c.split(":") for c in args.cases.split(",") if c]:
        rec = bench_case(case[0], int(case[1]), int(case[2]), args.smoother, args.runs, args.reps, args.rtol)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
