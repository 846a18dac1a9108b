#!/usr/bin/env python3
"""A wall with water on one face: hyperFS, a slab clamped at its base, the hydrostatic pressure gamma <level - z> on its face x+
evaluated at the CURRENT position of every point (NewtonPMG(hydrostatic={5: dict(gamma=, level=)}); surface.py,
csrc/kernels_surface.hip).

Prints the deflection of the crest beside the cantilever value w0 L^4 / (30 EI) of a triangular load (w0 = gamma L b at the base,
I = b t^3 / 12; with the level at the crest, L the height) and the base reaction in x beside gamma (level - z0)^2 b / 2 -- both for
orientation: the beam value knows no shear, no Poisson effect and no follower effect -- and the Newton counts with the hydrostatic
tangent in the outer Jacobian and without it.
    python examples/solve_dam.py [--nx 2 --ny 2 --nz 12] [--degree 2] [--thickness 0.2 --width 0.4 --height 1.0] [--level 1.0] [--gamma 0.002] [--increments 2] [--oracle]
"""
import argparse, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
import numpy as np
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mesh import box_mesh, side_set_nodes
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG

ap = argparse.ArgumentParser()
ap.add_argument("--nx", type=int, default=2); ap.add_argument("--ny", type=int, default=2); ap.add_argument("--nz", type=int, default=12)
ap.add_argument("--degree", type=int, default=2)
ap.add_argument("--thickness", type=float, default=0.2); ap.add_argument("--width", type=float, default=0.4); ap.add_argument("--height", type=float, default=1.0)
ap.add_argument("--E", type=float, default=1.0); ap.add_argument("--nu", type=float, default=0.3)
ap.add_argument("--gamma", type=float, default=0.002, help="weight of the fluid per unit volume, in units of E per unit length")
ap.add_argument("--level", type=float, default=None, help="default: the crest")
ap.add_argument("--increments", type=int, default=2)
ap.add_argument("--oracle", action="store_true", help="TESTS ONLY: the same solve on the CPU oracle (portable surface load)")
args = ap.parse_args()
if args.oracle:
    lib = cd.CeedLib(os.path.join(ROOT, "oracle", "liboracle_ceed.so")); c = cd.Ceed(lib, "/cpu/self/oracle")
else:
    lib = cd.CeedLib(cd.PRODUCT_LIB); c = cd.Ceed(lib, "/gpu/hip/mi355x")
t, b, L = args.thickness, args.width, args.height
level = L if args.level is None else args.level
gamma = args.gamma * args.E
mesh = box_mesh(args.nx, args.ny, args.nz, hi=(t, b, L))
out = {}
for tangent in ("full", "none"):
    p = SolidProblem(c, mesh, args.degree, "hyperFS", nu=args.nu, E=args.E, bc_sides=[1])
    s = NewtonPMG(p, hydrostatic={5: dict(gamma=gamma, level=level, up=(0.0, 0.0, 1.0))}, pressure_tangent=tangent)
    st = s.solve(args.increments)
    dm = p.levels[p.fine].dofmap
    u = s.U.to_numpy() + s.bcv.to_numpy()
    if tangent == "full":
        # the base reaction: the sum of F_int over the clamped nodes, from a problem without Dirichlet sets
        q = SolidProblem(c, mesh, args.degree, "hyperFS", nu=args.nu, E=args.E, multigrid="none")
        Xv, Yv = c.vector(u.size).set_array(u), c.vector(u.size)
        q.form_residual(Xv, Yv)
        f = Yv.to_numpy().reshape(-1, 3)
        base = side_set_nodes(mesh, dm, [1])
        crest = side_set_nodes(mesh, dm, [2])
        h = min(level, L)
        out.update({"resource": c.resource, "elements": mesh.nelem, "degree": args.degree, "dofs": p.lsize(),
                    "surface_kernel": s.field_loads[0][1].kernel_name, "gamma_over_E": args.gamma, "level": level,
                    "crest_deflection": float(-u.reshape(-1, 3)[crest, 0].mean()),
                    "cantilever_w0_L4_over_30_EI": gamma * L * b * L ** 4 / (30.0 * args.E * b * t ** 3 / 12.0) if level == L else None,
                    "base_reaction_x": float(math.fsum(f[base, 0])), "gamma_h2_b_over_2": gamma * h * h * b / 2.0})
        q.destroy()
    out[f"converged_{tangent}"] = st.converged
    out[f"snes_its_{tangent}"], out[f"ksp_its_{tangent}"] = st.newton_its, st.ksp_its
    s.destroy(); p.destroy()
print(json.dumps(out))
sys.exit(0 if out["converged_full"] and out["converged_none"] else 1)
