"""The lowest states (four, or as many as asked for, up to 16) of a potential that is not separable: two overlapping circular quantum dots of different depth in
a 2-D box, H = -laplacian / pi^2 + V(x, y).  The operator is matrix-free (operators.potential_operator: the scaled
Laplacian as Kronecker terms, V as a per-point diagonal) and the eigenpairs come from the blocked Rayleigh-Ritz solver with
a V-cycle preconditioner (drivers.block_eigensolve).  usage: potential_2d_general.py [gridsize] [cycles] [states]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigridcmt_amd import drivers, potential_operator  # noqa: E402

g = int(sys.argv[1]) if len(sys.argv) > 1 else 2 ** 9
cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 16
states = int(sys.argv[3]) if len(sys.argv) > 3 else 4
x = (np.arange(g) + 0.5) / g
X, Y = np.meshgrid(x, x, indexing="ij")
V = 60.0 - 60.0 * ((X - 0.36) ** 2 + (Y - 0.42) ** 2 < 0.2 ** 2) - 45.0 * ((X - 0.68) ** 2 + (Y - 0.60) ** 2 < 0.16 ** 2)
op = potential_operator(g, np.maximum(V, 0.0))
res = []
start = time.perf_counter()
vals, vecs = drivers.block_eigensolve(op, k=states, cycles=cycles, lowest=8, residuals=res)
elapsed = time.perf_counter() - start
print("grid %d^2  %d iterations  %.3f s" % (g, cycles, elapsed))
for j, (lam, r) in enumerate(zip(vals, res[-1])):
    inside = float(np.sum(vecs[:, j].reshape(g, g) ** 2 * (V <= 15.0)))
    print("state %d  E = %.10f  residual %.2e  weight inside the dots %.3f" % (j, lam, r, inside))
