"""The lowest states of a circular quantum dot with a light effective mass inside: H = -div(w grad) / pi^2 + V(x, y) with
the inverse mass w = 4 inside the dot and 1 in the barrier (the BenDaniel-Duke form of the kinetic term, harmonic mean
across the interface) and a band offset of 30 outside — a GaAs dot in an AlGaAs barrier in the units of this package.  The
operator is matrix-free (operators.variable_mass_operator: the uniform part as Kronecker terms, the deviations as per-point
bonds and a per-point diagonal) and the eigenpairs come from the blocked Rayleigh-Ritz solver with a V-cycle preconditioner
(drivers.block_eigensolve).  For comparison the same dot with the barrier's mass everywhere (operators.potential_operator).
usage: effective_mass_2d.py [gridsize] [cycles] [states]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigridcmt_amd import drivers, potential_operator, variable_mass_operator  # noqa: E402

g = int(sys.argv[1]) if len(sys.argv) > 1 else 2 ** 9
cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 16
states = int(sys.argv[3]) if len(sys.argv) > 3 else 3
x = (np.arange(g) + 0.5) / g - 0.5
X, Y = np.meshgrid(x, x, indexing="ij")
inside = (X - 0.05) ** 2 + (Y + 0.1) ** 2 < 0.3 ** 2
V = np.where(inside, 0.0, 30.0)
for name, op in (("light mass inside (w = 4)", variable_mass_operator(g, np.where(inside, 4.0, 1.0), V)),
                 ("uniform mass (w = 1)", potential_operator(g, V))):
    res = []
    start = time.perf_counter()
    vals, vecs = drivers.block_eigensolve(op, k=states, cycles=cycles, lowest=8, residuals=res)
    elapsed = time.perf_counter() - start
    print("%s: grid %d^2  %d iterations  %.3f s" % (name, g, cycles, elapsed))
    for j, (lam, r) in enumerate(zip(vals, res[-1])):
        weight = float(np.sum(vecs[:, j].reshape(g, g) ** 2 * inside))
        print("  state %d  E = %.10f  residual %.2e  weight inside the dot %.3f" % (j, lam, r, weight))
