"""Solve (A - shift I) x = f to a tolerance with MGCMTSolver.solve — conjugate gradients preconditioned by one V-cycle per
iteration, resident on the device — next to the plain V-cycle iteration a caller of ``vcycle`` would write, on the two problems
the plain cycle is weakest on:

  * the scaled Laplacian at shift 1.9, next to its lowest eigenvalue (1.879 at 32^2, 2 in the limit): the regime of the
    reference's shift-and-invert drivers.  The system is indefinite or nearly singular; the plain cycle stalls or diverges;
  * a high-contrast variable effective mass (operators.variable_mass_operator): a disc of inverse mass 1000 in a barrier of 1.

For each it prints the number of plain cycles (capped) beside the number of solve iterations, with the residuals reached.
usage: solve_to_tolerance.py [gridsize] [rtol]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, laplacian_operator, variable_mass_operator  # noqa: E402

g = int(sys.argv[1]) if len(sys.argv) > 1 else 2 ** 9
rtol = float(sys.argv[2]) if len(sys.argv) > 2 else 1e-8
CAP = 100
solver, sm = MGCMTSolver(), MGCMTStencilMaker()
x = np.arange(g) + 0.5 - g / 2
X, Y = np.meshgrid(x, x, indexing="ij")
disc = X * X + Y * Y < (g / 4) ** 2
problems = [("Laplacian, shift 1.9", laplacian_operator(g, "2d") * (-1 / np.pi ** 2), 1.9),
            ("variable mass, contrast 1000", variable_mass_operator(g, np.where(disc, 1000.0, 1.0)), 0.0)]
f = np.random.RandomState(1).rand(g * g)
fnorm = np.linalg.norm(f)
for name, op, shift in problems:
    A = op.tocsr() if g <= 1024 else None          # (only to print the plain iteration's residual; the solve never assembles)
    for sname, smoother in (("wjacobi", solver.wjacobi), ("red-black", solver.gseidel_rb)):
        kw = dict(nu1=2, nu2=2, smoother=smoother, shift=shift, lowest_level=4, dimension="2d")
        # the plain iteration: one vcycle call per cycle, the residual on the host
        v, cycles, res = np.zeros(g * g), 0, 1.0
        start = time.perf_counter()
        while A is not None and cycles < CAP and res > rtol and np.isfinite(res):
            v = np.array(solver.vcycle(v, f.copy(), op, sm, **kw)).reshape(-1)
            cycles += 1
            res = np.linalg.norm(f - (A @ v - shift * v)) / fnorm
        plain_s = time.perf_counter() - start
        info = {}
        start = time.perf_counter()
        solver.solve(f, op, sm, rtol=rtol, maxiter=CAP, info=info, **kw)
        solve_s = time.perf_counter() - start
        plain = "not run above 1024^2" if A is None else "%s%d cycles, residual %.1e, %.3f s" % ("" if res <= rtol else "> ", cycles, res, plain_s)
        print("%-30s %-9s grid %d^2  plain: %s   solve: %d iterations (%s%s), residual %.1e, %.3f s"
              % (name, sname, g, plain, info["iterations"], info["status"], ", indefinite" if info["indefinite"] else "", info["true_residual"], solve_s))
