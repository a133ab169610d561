"""The lowest states of an ellipsoidal GaAs quantum dot in an AlGaAs barrier with a position-dependent effective mass:
H = -div(w grad) / pi^2 + V on g^3 points, w = 1 and V = 0 inside the dot, w = 0.73 and V = 30 in the barrier (BenDaniel-Duke:
the harmonic mean of w across the interface).  The operator is matrix-free (operators.variable_mass_operator(...,
dimension="3d"): a reference mass times the scaled Laplacian as three Kronecker terms, the deviations as per-point bonds and
a per-point diagonal).  First a few V-cycles on H u = f, then the eigenpairs from the blocked Rayleigh-Ritz solver with a
V-cycle preconditioner (drivers.block_eigensolve).
usage: effective_mass_3d.py [gridsize] [cycles]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, drivers, variable_mass_operator  # noqa: E402

g = int(sys.argv[1]) if len(sys.argv) > 1 else 64
cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 30
t = (np.arange(g) + 0.5) / g - 0.5
Z, Y, X = np.meshgrid(t, t, t, indexing="ij")
inside = np.sqrt((X - 0.05) ** 2 + ((Y + 0.03) / 0.8) ** 2 + ((Z - 0.02) / 0.6) ** 2) < 0.3
op = variable_mass_operator(g, np.where(inside, 1.0, 0.73), np.where(inside, 0.0, 30.0), dimension="3d")

solver, sm = MGCMTSolver(), MGCMTStencilMaker()
lowest = 8 if g >= 16 else 4
f = np.random.RandomState(0).rand(g ** 3)
v = np.zeros(g ** 3)
for cycle in range(4):
    v = np.asarray(solver.vcycle(v, f.copy(), op, sm, nu1=2, nu2=2, smoother=solver.gseidel_rb, lowest_level=lowest, dimension="3d")).reshape(-1)
    print("V-cycle %d  |f - H v| / |f| = %.3e" % (cycle + 1, np.linalg.norm(f - op.dot(v)) / np.linalg.norm(f)))

res = []
start = time.perf_counter()
vals, vecs = drivers.block_eigensolve(op, k=3, cycles=cycles, lowest=lowest, residuals=res)
elapsed = time.perf_counter() - start
print("grid %d^3  %d iterations  %.3f s" % (g, cycles, elapsed))
for j, (lam, r) in enumerate(zip(vals, res[-1])):
    print("state %d  E = %.10f  residual %.2e  weight inside the dot %.3f" % (j, lam, r, float(np.sum(vecs[:, j].reshape(g, g, g) ** 2 * inside))))
