"""The lowest states of a rotated-valley ellipsoidal quantum dot: H = -div(W grad) / pi^2 + V(x, y, z) with a position-dependent
symmetric 3 x 3 inverse-mass tensor W — inside the dot an L-valley-like ellipsoid with the principal values 1, 0.35 and 0.6 on axes
turned against the grid (by 0.6 rad about z, then 0.4 rad about x), 0.73 times the identity in the barrier, blended across a
smeared interface — and a band offset of 30 outside.  The mixed derivatives put entries on the twelve edge neighbours: a symmetric
19-point operator with per-point coefficients.  The operator is matrix-free (operators.tensor_mass_operator(..., dimension="3d"):
the uniform part as Kronecker terms, the deviations as a per-point 27-point stencil) and the eigenpairs come from the blocked
Rayleigh-Ritz solver with a V-cycle preconditioner (drivers.block_eigensolve).  For comparison the same dot with its axes along
the grid (a diagonal tensor: operators.tensor_mass_operator returns per-point bonds).
usage: tensor_mass_3d.py [gridsize] [cycles] [states]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multigridcmt_amd import drivers, tensor_mass_operator  # noqa: E402

g = int(sys.argv[1]) if len(sys.argv) > 1 else 2 ** 7
cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 24
states = int(sys.argv[3]) if len(sys.argv) > 3 else 3
t = (np.arange(g) + 0.5) / g - 0.5
Z, Y, X = np.meshgrid(t, t, t, indexing="ij")
s = 0.5 * (1.0 + np.tanh((np.sqrt((X - 0.05) ** 2 + ((Y + 0.03) / 0.8) ** 2 + ((Z - 0.02) / 0.6) ** 2) - 0.3) / 0.08))          # 0 inside, 1 outside
V = 30.0 * s
lam = (1.0, 0.35, 0.6)
for name, theta, phi in (("axes turned by 0.6 about z, 0.4 about x", 0.6, 0.4), ("axes along the grid", 0.0, 0.0)):
    c, sn, cp, sp = np.cos(theta), np.sin(theta), np.cos(phi), np.sin(phi)
    axes = [(c, sn, 0.0), (-sn * cp, c * cp, sp), (sn * sp, -c * sp, cp)]          # columns of Rz(theta) Rx(phi), components (x, y, z)
    w = {}
    for key, (i, j) in (("xx", (0, 0)), ("yy", (1, 1)), ("zz", (2, 2)), ("xy", (0, 1)), ("xz", (0, 2)), ("yz", (1, 2))):
        inside = sum(l * e[i] * e[j] for l, e in zip(lam, axes))
        w[key] = (1.0 - s) * inside + s * (0.73 if i == j else 0.0)
    op = tensor_mass_operator(g, w["xx"], w["yy"], w["xy"], V, wzz=w["zz"], wxz=w["xz"], wyz=w["yz"], dimension="3d")
    kind = "point stencil" if op.point_stencil is not None else "point bonds"
    res = []
    start = time.perf_counter()
    vals, vecs = drivers.block_eigensolve(op, k=states, cycles=cycles, lowest=8, residuals=res)
    elapsed = time.perf_counter() - start
    print("%s (%s): grid %d^3  %d iterations  %.3f s" % (name, kind, g, cycles, elapsed))
    for j, (e, r) in enumerate(zip(vals, res[-1])):
        weight = float(np.sum(vecs[:, j].reshape(g, g, g) ** 2 * (1.0 - s)))
        print("  state %d  E = %.10f  residual %.2e  weight inside the dot %.3f" % (j, e, r, weight))
