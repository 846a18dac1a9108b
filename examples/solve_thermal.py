"""A slender bar under a temperature gradient through its thickness (solver.NewtonPMG(thermal=), thermal.py).

A bar of length L along x and thickness W, clamped at x = 0 (side set 6), is heated by theta = g y: warmer on top.  A temperature field
that is linear in space is stress-free: the bar bends into the curvature alpha g without stress, and its tip moves by -alpha g L^2 / 2
in y (to first order in alpha g L).  The script prints the tip deflection beside that closed form and the largest nodal von Mises
stress over the half of the bar away from the clamp -- near zero -- beside the stress the clamp's restraint leaves at x = 0, and the
largest axial stress there beside what postprocess.Stress reports WITHOUT the thermal term, where the free expansion shows as stress
(an isotropic one, which the von Mises stress does not see).
With --problem hyperFS the thermal term follows the body (added in every residual, its tangent in the outer Jacobian); alpha is the
linearised coefficient there, so the figures agree with the closed form to first order in alpha theta only.

    python examples/solve_thermal.py                          # on the device
    python examples/solve_thermal.py --oracle                 # on the CPU oracle (portable NumPy form)
    python examples/solve_thermal.py --oracle --problem hyperFS
"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.postprocess import Stress
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG

ap = argparse.ArgumentParser()
ap.add_argument("--oracle", action="store_true"); ap.add_argument("--problem", default="linElas", choices=["linElas", "hyperSS", "hyperFS"])
ap.add_argument("--elements", type=int, default=8); ap.add_argument("--degree", type=int, default=2)
ap.add_argument("--alpha", type=float, default=1e-4); ap.add_argument("--gradient", type=float, default=20.0, metavar="g")
ap.add_argument("--E", type=float, default=50.0); ap.add_argument("--nu", type=float, default=0.3)
a = ap.parse_args()
c = cd.Ceed(cd.CeedLib(os.path.join(ROOT, "oracle", "liboracle_ceed.so")), "/cpu/self/oracle") if a.oracle else cd.Ceed(cd.CeedLib(cd.PRODUCT_LIB), "/gpu/hip/mi355x")
L, Wd = 2.0, 0.1
prob = SolidProblem(c, box_mesh(a.elements, 1, 1, lo=(0.0, -Wd / 2, -Wd / 2), hi=(L, Wd / 2, Wd / 2)), a.degree, a.problem, nu=a.nu, E=a.E, bc_sides=[6])
thermal = dict(alpha=a.alpha, theta=lambda X: a.gradient * X[:, 1])
sol = NewtonPMG(prob, thermal=thermal, ksp_rtol=1e-12, snes_rtol=1e-10)
st = sol.solve(num_increments=1)
X = prob.levels[prob.fine].dofmap.node_coords
u = sol.U.to_numpy()[:3 * len(X)].reshape(-1, 3)
print(f"resource {c.resource}; {a.problem}, {prob.lsize()} dofs, {sol.nlev} levels; {st.newton_its} Newton / {st.ksp_its} Krylov iterations, "
      f"converged {st.converged}; follower {sol.has_followers()}; kernels {sol.thermal.kernel_name}")
tip = u[np.abs(X[:, 0] - L) < 1e-9, 1].mean()                                   # (the y^2 - z^2 part of u_y has zero mean over the square section)
print(f"tip deflection {tip:.6e} (closed form -alpha g L^2 / 2 = {-a.alpha * a.gradient * L * L / 2:.6e})")
with_t, without = Stress(prob, a.problem, thermal=sol.thermal), Stress(prob, a.problem)
far = X[:, 0] > L / 2
sg, sg0 = with_t.nodal(sol.Xloc), without.nodal(sol.Xloc)
vm = Stress.von_mises(sg)
scale = a.E * a.alpha * a.gradient * Wd / 2
print(f"for x > L / 2: largest von Mises stress {vm[far].max():.3e}, largest |sigma_xx| {np.abs(sg[far, 0]).max():.3e} with the thermal term and "
      f"{np.abs(sg0[far, 0]).max():.3e} without it (E alpha theta at the surface = {scale:.3e}); von Mises at the clamp {vm[~far].max():.3e}")
with_t.destroy(); without.destroy(); sol.destroy(); prob.destroy()
