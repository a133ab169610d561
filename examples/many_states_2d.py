"""Forty states (or as many as asked for, up to 64) of the non-separable dot of examples/potential_2d_general.py — two
overlapping circular quantum dots of different depth in a 2-D box, H = -laplacian / pi^2 + V(x, y) — solved to a tolerance by
drivers.deflated_eigensolve: the blocked Rayleigh-Ritz iteration of drivers.block_eigensolve with hard locking, an active block
of 16 vectors and one deflation pass per iteration (mgcmt_block_deflate).  A fourth argument chooses the Rayleigh-Ritz basis:
"scaled" (the default) or "orthonormal" — W and P projected against X and made orthonormal on the device in every iteration
(mgcmt_block_project, mgcmt_block_orthonormalize), the choice for many states on fine grids; info then also holds the smallest
eigenvalue of the Gram matrix per iteration.  usage: many_states_2d.py [gridsize] [states] [rtol] [basis]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigridcmt_amd import drivers, potential_operator  # noqa: E402

g = int(sys.argv[1]) if len(sys.argv) > 1 else 2 ** 9
states = int(sys.argv[2]) if len(sys.argv) > 2 else 40
rtol = float(sys.argv[3]) if len(sys.argv) > 3 else 1e-8
basis = sys.argv[4] if len(sys.argv) > 4 else "scaled"
x = (np.arange(g) + 0.5) / g
X, Y = np.meshgrid(x, x, indexing="ij")
V = 60.0 - 60.0 * ((X - 0.36) ** 2 + (Y - 0.42) ** 2 < 0.2 ** 2) - 45.0 * ((X - 0.68) ** 2 + (Y - 0.60) ** 2 < 0.16 ** 2)
op = potential_operator(g, np.maximum(V, 0.0))
info = {}
start = time.perf_counter()
vals, vecs = drivers.deflated_eigensolve(op, states, rtol=rtol, lowest=8, info=info, basis=basis)
elapsed = time.perf_counter() - start
print("grid %d^2  %s after %d iterations (%d column cycles)  %.3f s" % (g, info["status"], info["iterations"], info["column_cycles"], elapsed))
if "gram_min" in info:
    print("smallest eigenvalue of the scaled Gram matrix over the run %.12f, columns dropped %d" % (info["gram_min"].min(), info["dropped"].sum()))
for j, (lam, r, at) in enumerate(zip(vals, info["residuals"], info["locked_at"])):
    inside = float(np.sum(vecs[:, j].reshape(g, g) ** 2 * (V <= 15.0)))
    print("state %2d  E = %.10f  residual %.2e  locked at iteration %3d  weight inside the dots %.3f" % (j, lam, r, at, inside))
