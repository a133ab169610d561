"""A quantum dot in a host of two dielectrics, solved self-consistently by drivers.schroedinger_poisson: the lowest states of
H[phi] = -laplacian / pi^2 + V_ext(x, y) + coupling phi, their charge density rho = sum_j f_j psi_j^2, the potential of that
charge from -div(eps grad phi) / pi^2 = rho with eps = 1 on the left half and 3 on the right, and again until phi stands still.
Between the upload of V_ext and the downloads at the end every step stays on the device: the density in one pass over the
states (mgcmt_block_density), the new potential written into the plan's own hierarchy (mgcmt_plan_set_point_diagonal), the next
eigensolve started from the previous states.  The coupling is given for the 32^2 grid of the tests and scaled with the mesh (the
states have unit 2-norm, so the density per grid point falls as h^2).  A fifth argument turns on Anderson mixing with that many
history vectors (mgcmt_mix_residual, mgcmt_mix_combine): try "256 8 20000 0.5 5" next to "256 8 20000 0.2".
usage: schroedinger_poisson_2d.py [gridsize] [states] [coupling at 32^2] [mixing] [mixing_history]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigridcmt_amd import drivers, potential_operator, variable_mass_operator  # noqa: E402

g = int(sys.argv[1]) if len(sys.argv) > 1 else 2 ** 8
states = int(sys.argv[2]) if len(sys.argv) > 2 else 8
coupling = (float(sys.argv[3]) if len(sys.argv) > 3 else 800.0) * ((g + 1) / 33.0) ** 2
mixing = float(sys.argv[4]) if len(sys.argv) > 4 else 1.0
mixing_history = int(sys.argv[5]) if len(sys.argv) > 5 else 0
x = (np.arange(g) + 1.0) / (g + 1)
X, Y = np.meshgrid(x, x, indexing="ij")
eps = np.where(Y < 0.5, 1.0, 3.0)
op = potential_operator(g, 160.0 * ((X - 0.5) ** 2 + (Y - 0.45) ** 2))
poisson_op = variable_mass_operator(g, eps)
occupations = [2.0] * min(3, states) + [0.0] * max(0, states - 3)          # three doubly occupied levels, the rest are guards
info = {}
start = time.perf_counter()
vals, vecs, phi = drivers.schroedinger_poisson(op, poisson_op, states, occupations, coupling=coupling, mixing=mixing, mixing_history=mixing_history,
                                               tol=1e-6, lowest=8, info=info)
elapsed = time.perf_counter() - start
print("grid %d^2  %s after %d steps  %.3f s" % (g, info["status"], info["iterations"], elapsed))
for step, (d, ei, pi) in enumerate(zip(info["changes"], info["eigen_iterations"], info["poisson_iterations"]), start=1):
    print("step %2d  change of phi %.3e  eigen-solver iterations %3d  conjugate-gradient iterations %2d" % (step, d, ei, pi))
print("max coupling * phi = %.6f" % (coupling * np.abs(phi).max()))
for j, (lam, f) in enumerate(zip(vals, occupations)):
    right = float(np.sum(vecs[:, j].reshape(g, g) ** 2 * (Y >= 0.5)))
    print("state %2d  E = %.10f  occupation %.1f  weight in the eps = 3 half %.3f" % (j, lam, f, right))
