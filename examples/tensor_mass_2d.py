"""The lowest states of a rotated anisotropic quantum dot: H = -div(W grad) / pi^2 + V(x, y) with a position-dependent
symmetric 2 x 2 inverse-mass tensor W — inside the dot the principal values 4 and 1 on axes turned by 0.6 rad against the grid
(an anisotropic valley), the identity in the barrier — and a band offset of 30 outside.  The mixed derivative puts entries on
the four corner neighbours: a symmetric 9-point operator with per-point coefficients.  The operator is matrix-free
(operators.tensor_mass_operator: the uniform part as Kronecker terms, the deviations as a per-point 9-point stencil) and the
eigenpairs come from the blocked Rayleigh-Ritz solver with a V-cycle preconditioner (drivers.block_eigensolve).  For comparison
the same dot with its axes along the grid (a diagonal tensor: operators.tensor_mass_operator returns per-point bonds).
usage: tensor_mass_2d.py [gridsize] [cycles] [states]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigridcmt_amd import drivers, tensor_mass_operator  # noqa: E402

g = int(sys.argv[1]) if len(sys.argv) > 1 else 2 ** 9
cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 24
states = int(sys.argv[3]) if len(sys.argv) > 3 else 3
x = (np.arange(g) + 0.5) / g - 0.5
X, Y = np.meshgrid(x, x, indexing="ij")
inside = (X - 0.05) ** 2 + (Y + 0.1) ** 2 < 0.3 ** 2
V = np.where(inside, 0.0, 30.0)
l1 = np.where(inside, 4.0, 1.0)
for name, theta in (("axes turned by 0.6", 0.6), ("axes along the grid", 0.0)):
    c, s = np.cos(np.where(inside, theta, 0.0)), np.sin(np.where(inside, theta, 0.0))
    op = tensor_mass_operator(g, c * c * l1 + s * s, s * s * l1 + c * c, c * s * (l1 - 1.0), V)
    kind = "point stencil" if op.point_stencil is not None else "point bonds"
    res = []
    start = time.perf_counter()
    vals, vecs = drivers.block_eigensolve(op, k=states, cycles=cycles, lowest=8, residuals=res)
    elapsed = time.perf_counter() - start
    print("%s (%s): grid %d^2  %d iterations  %.3f s" % (name, kind, g, cycles, elapsed))
    for j, (lam, r) in enumerate(zip(vals, res[-1])):
        weight = float(np.sum(vecs[:, j].reshape(g, g) ** 2 * inside))
        print("  state %d  E = %.10f  residual %.2e  weight inside the dot %.3f" % (j, lam, r, weight))
