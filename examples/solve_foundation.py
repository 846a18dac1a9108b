"""A block on an elastic (Winkler) foundation, held by nothing else (solver.NewtonPMG(support=)).

A block of nx x ny x nz elements, linElas, rests with its bottom (side set 1) on a bed of springs kn (normal) and kt (tangential) per unit
area and carries a uniform pressure sigma on its top (side set 2).  There is no Dirichlet set: the springs alone hold the rigid-body
modes.  With nu = 0 the exact solution is uniaxial, u_z = -sigma / kn - sigma z / E, and the script prints the settlement of the bottom and
of the top beside it; with nu > 0 the block also spreads against the tangential springs and the closed form is only the average.

    python examples/solve_foundation.py            # on the device
    python examples/solve_foundation.py --oracle   # on the CPU oracle (portable support term)
"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG

ap = argparse.ArgumentParser()
ap.add_argument("--oracle", action="store_true"); ap.add_argument("--elements", type=int, nargs=3, default=(4, 4, 4)); ap.add_argument("--degree", type=int, default=2)
ap.add_argument("--nu", type=float, default=0.0); ap.add_argument("--kn", type=float, default=2.0); ap.add_argument("--kt", type=float, default=1.0)
ap.add_argument("--pressure", type=float, default=0.01)
a = ap.parse_args()
c = cd.Ceed(cd.CeedLib(os.path.join(ROOT, "oracle", "liboracle_ceed.so")), "/cpu/self/oracle") if a.oracle else cd.Ceed(cd.CeedLib(cd.PRODUCT_LIB), "/gpu/hip/mi355x")
E = 1.0
prob = SolidProblem(c, box_mesh(*a.elements), a.degree, "linElas", nu=a.nu, E=E, bc_sides=[])
sol = NewtonPMG(prob, support={1: dict(kn=a.kn, kt=a.kt)}, traction={2: (0.0, 0.0, -a.pressure)}, coarse="cg", snes_rtol=1e-10)
st = sol.solve(num_increments=1)
u = sol.U.to_numpy().reshape(-1, 3)
z = prob.levels[prob.fine].dofmap.node_coords[:, 2]
sup = sol.supports[0]
print(f"resource {c.resource}; {prob.lsize()} dofs, {sol.nlev} levels; {st.newton_its} Newton / {st.ksp_its} Krylov iterations, converged {st.converged}")
print(f"supported area {sup['levels'][sol.nlev - 1].area(sup['spring']):.6f}; kernel {sup['levels'][sol.nlev - 1].kernel_name}")
print(f"settlement of the bottom {u[z == 0.0, 2].mean():.6e} (closed form -sigma / kn = {-a.pressure / a.kn:.6e})")
print(f"settlement of the top    {u[z == 1.0, 2].mean():.6e} (closed form -sigma / kn - sigma H / E = {-a.pressure / a.kn - a.pressure / E:.6e})")
print(f"largest lateral displacement {np.abs(u[:, :2]).max():.3e}")
