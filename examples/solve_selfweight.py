"""A clamped column of two materials under its own weight, and a spinning bar (solver.NewtonPMG(density=, gravity=, spin=)).

A column of 1 x 1 x nz elements and height H, linElas with nu = 0, stands clamped on its base (side set 1); its lower half has the density
rho1, its upper half rho2 (mass.DensityField.per_element), and gravity pulls along -z.  The solution is uniaxial: the script prints the
base reaction E A u_z'(0) beside the total weight, and the settlement of the top beside g (rho1 h^2 + rho2 (H^2 - h^2)) / (2 E), h = H / 2.
With --spin OMEGA a bar of length L along x, clamped at x = 0, spins about the y axis instead, and the script prints its tip
displacement beside sin(kL) / (k cos kL) - L, k = OMEGA sqrt(rho / E): the centrifugal load follows the material points.

    python examples/solve_selfweight.py                     # on the device
    python examples/solve_selfweight.py --oracle            # on the CPU oracle (portable mass operator)
    python examples/solve_selfweight.py --oracle --spin 1.2
"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mass import DensityField
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG

ap = argparse.ArgumentParser()
ap.add_argument("--oracle", action="store_true"); ap.add_argument("--layers", type=int, default=4); ap.add_argument("--degree", type=int, default=2)
ap.add_argument("--rho", type=float, nargs=2, default=(1.0, 3.0)); ap.add_argument("--g", type=float, default=0.5); ap.add_argument("--E", type=float, default=50.0)
ap.add_argument("--spin", type=float, default=None, metavar="OMEGA")
a = ap.parse_args()
c = cd.Ceed(cd.CeedLib(os.path.join(ROOT, "oracle", "liboracle_ceed.so")), "/cpu/self/oracle") if a.oracle else cd.Ceed(cd.CeedLib(cd.PRODUCT_LIB), "/gpu/hip/mi355x")
E, H, Wd = a.E, 2.0, 0.1
if a.layers % 2:
    ap.error("--layers must be even: the two materials meet on an element boundary")
if a.spin is None:
    mesh = box_mesh(1, 1, a.layers, lo=(-Wd / 2, -Wd / 2, 0.0), hi=(Wd / 2, Wd / 2, H))
    prob = SolidProblem(c, mesh, a.degree, "linElas", nu=0.0, E=E, bc_sides=[1])
    rho = np.where(np.arange(mesh.nelem) < a.layers // 2, a.rho[0], a.rho[1])       # elements are ordered along z
    sol = NewtonPMG(prob, density=DensityField.per_element(rho), gravity=(0.0, 0.0, -a.g), ksp_rtol=1e-12, snes_rtol=1e-10)
else:
    prob = SolidProblem(c, box_mesh(max(a.layers, 2), 1, 1, lo=(0.0, -Wd / 2, -Wd / 2), hi=(H, Wd / 2, Wd / 2)), max(a.degree, 4), "linElas", nu=0.0, E=E, bc_sides=[6])
    sol = NewtonPMG(prob, density=a.rho[0], spin=dict(omega=a.spin, axis=(0, 1, 0)), ksp_rtol=1e-12, snes_rtol=1e-10)
st = sol.solve(num_increments=1)
X = prob.levels[prob.fine].dofmap.node_coords
u = sol.U.to_numpy()[:3 * len(X)].reshape(-1, 3)
print(f"resource {c.resource}; {prob.lsize()} dofs, {sol.nlev} levels; {st.newton_its} Newton / {st.ksp_its} Krylov iterations, converged {st.converged}; "
      f"mass operator {sol.body_mass.kernel_name}")
if a.spin is None:
    h = H / 2
    weight = a.g * Wd * Wd * h * (a.rho[0] + a.rho[1])
    zs = np.unique(np.round(X[:, 2], 12))[:a.degree + 1]                         # the node layers of the bottom element
    uz = np.array([u[np.abs(X[:, 2] - z) < 1e-9, 2].mean() for z in zs])
    slope = np.polyval(np.polyder(np.polyfit(zs, uz, a.degree)), 0.0)                          # u_z'(0) of the element's own polynomial
    print(f"base reaction E A u_z'(0) = {-E * Wd * Wd * slope:.6e} (total weight {weight:.6e})")
    print(f"settlement of the top {u[np.abs(X[:, 2] - H) < 1e-9, 2].mean():.6e} "
          f"(closed form {-a.g * (a.rho[0] * h * h + a.rho[1] * (H * H - h * h)) / (2 * E):.6e})")
else:
    k = a.spin * np.sqrt(a.rho[0] / E)
    print(f"k L = {k * H:.4f}; tip displacement {u[np.abs(X[:, 0] - H) < 1e-9, 0].mean():.6e} "
          f"(closed form sin(kL) / (k cos kL) - L = {np.sin(k * H) / (k * np.cos(k * H)) - H:.6e}; "
          f"the dead load alone would give {a.rho[0] * a.spin ** 2 * H ** 3 / (3 * E):.6e})")
sol.destroy(); prob.destroy()
