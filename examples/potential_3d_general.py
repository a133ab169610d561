"""The lowest states of a 3-D potential that is not separable: two overlapping spherical quantum dots of different depth in
a box, H = -laplacian / pi^2 + V(x, y, z).  The operator is matrix-free (operators.potential_operator(..., dimension="3d"):
the scaled Laplacian as three Kronecker terms, V as a per-point diagonal) and the eigenpairs come from the blocked
Rayleigh-Ritz solver with a V-cycle preconditioner (drivers.block_eigensolve).
usage: potential_3d_general.py [gridsize] [cycles]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigridcmt_amd import drivers, potential_operator  # noqa: E402

g = int(sys.argv[1]) if len(sys.argv) > 1 else 64
cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 40
t = (np.arange(g) + 0.5) / g
Z, Y, X = np.meshgrid(t, t, t, indexing="ij")
V = 60.0 - 60.0 * ((X - 0.38) ** 2 + (Y - 0.42) ** 2 + (Z - 0.45) ** 2 < 0.24 ** 2) \
    - 45.0 * ((X - 0.66) ** 2 + (Y - 0.60) ** 2 + (Z - 0.55) ** 2 < 0.2 ** 2)
V = np.maximum(V, 0.0)
op = potential_operator(g, V, dimension="3d")
res = []
start = time.perf_counter()
vals, vecs = drivers.block_eigensolve(op, k=3, cycles=cycles, lowest=8 if g >= 16 else 4, residuals=res)
elapsed = time.perf_counter() - start
print("grid %d^3  %d iterations  %.3f s" % (g, cycles, elapsed))
for j, (lam, r) in enumerate(zip(vals, res[-1])):
    inside = float(np.sum(vecs[:, j].reshape(g, g, g) ** 2 * (V <= 15.0)))
    print("state %d  E = %.10f  residual %.2e  weight inside the dots %.3f" % (j, lam, r, inside))
