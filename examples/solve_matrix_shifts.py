"""Six shifted systems in one call: MGCMTSolver.solve_matrix on the 2-D box, (A - mu_c I) x_c = f_c with mu_c placed next to
the first six exact eigenvalues of A = -laplacian / pi^2 (drivers.exact_box_eigenvalues) — the systems of a shift-and-invert
step, one per wanted eigenpair.  Each is indefinite (but for the first) and nearly singular.  The batched solve — conjugate
gradients preconditioned by one V-cycle per iteration, all columns in every launch, a column frozen once it has converged —
reaches the tolerance in every column; as many cycles of ``vcycle_matrix`` (the reference's k-column cycle, with its
Gram-Schmidt of the columns) as the slowest column took iterations do not: next to an eigenvalue the plain cycle stalls or
diverges.  Both residuals ||f_c - (A - mu_c I) x_c|| / ||f_c|| are printed per column.
usage: solve_matrix_shifts.py [gridsize] [rtol] [offset]      (mu_c = lambda_c * (1 + offset), default 0.01)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, laplacian_operator  # noqa: E402
from multigridcmt_amd.drivers import exact_box_eigenvalues  # noqa: E402

g = int(sys.argv[1]) if len(sys.argv) > 1 else 2 ** 8
rtol = float(sys.argv[2]) if len(sys.argv) > 2 else 1e-8
offset = float(sys.argv[3]) if len(sys.argv) > 3 else 0.01
K = 6
solver, sm = MGCMTSolver(), MGCMTStencilMaker()
op = laplacian_operator(g, "2d") * (-1 / np.pi ** 2)
A = op.tocsr()                                   # (only to print residuals; the solve never assembles)
eigenvalues = exact_box_eigenvalues(g, "2d", K)
shifts = eigenvalues * (1.0 + offset)
F = np.random.RandomState(1).rand(g * g, K)
fnorm = np.linalg.norm(F, axis=0)


def residuals(Xm):
    return [np.linalg.norm(F[:, c] - (A @ Xm[:, c] - shifts[c] * Xm[:, c])) / fnorm[c] for c in range(K)]


kw = dict(nu1=2, nu2=2, smoother=solver.wjacobi, shifts=shifts, lowest_level=4, dimension="2d")
info = {}
start = time.perf_counter()
X = solver.solve_matrix(F, op, sm, rtol=rtol, maxiter=200, info=info, **kw)
solve_s = time.perf_counter() - start
cycles = max(info["iterations"])
V = np.zeros((g * g, K))
start = time.perf_counter()
for _ in range(cycles):
    V = np.array(solver.vcycle_matrix(V, F.copy(), op, sm, **kw))
plain_s = time.perf_counter() - start
res_solve, res_plain = residuals(np.array(X)), residuals(V)
print("grid %d^2, rtol %.0e, %d columns, shifts = eigenvalues * %g" % (g, rtol, K, 1.0 + offset))
for c in range(K):
    print("  column %d  eigenvalue %.6f  shift %.6f   solve_matrix: %3d iterations (%s%s), residual %.1e   %d vcycle_matrix cycles: residual %.1e"
          % (c, eigenvalues[c], shifts[c], info["iterations"][c], info["status"][c], ", indefinite" if info["indefinite"][c] else "",
             res_solve[c], cycles, res_plain[c]))
print("solve_matrix %.3f s; %d vcycle_matrix cycles %.3f s" % (solve_s, cycles, plain_s))
reached = all(r <= 2 * rtol for r in res_solve)
print("solve_matrix reached %.0e in every column: %s; vcycle_matrix in %d of %d" % (rtol, reached, sum(r <= 2 * rtol for r in res_plain), K))
sys.exit(0 if reached else 1)
