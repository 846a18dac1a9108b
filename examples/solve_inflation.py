#!/usr/bin/env python3
"""Inflation of a thick-walled tube: hyperFS, a hollow cylinder with both ends clamped, a pressure on the inner wall that follows the
deforming surface (NewtonPMG(pressure={996: p}); surface.py, csrc/kernels_surface.hip).

Prints the Newton and Krylov iteration counts and the inner radius at mid-height.  ``--tangent none`` leaves the pressure's tangent out
of the outer Jacobian (modified Newton): the same solution in more Newton steps.  ``--stress`` adds a second line: the largest nodal
von Mises stress with its node's coordinates, and the hoop stress at the inner and the outer wall at mid-height (postprocess.Stress)
beside Lame's values for the applied pressure -- for orientation only: the ends are clamped and the model is finite-strain.
    python examples/solve_inflation.py [--nr 2 --nth 16 --nz 8] [--degree 2] [--pressure 0.02] [--increments 5] [--tangent full|none] [--stress] [--oracle]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
import numpy as np
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mesh import hollow_cylinder_mesh, side_set_nodes
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG

ap = argparse.ArgumentParser()
ap.add_argument("--nr", type=int, default=2)
ap.add_argument("--nth", type=int, default=16)
ap.add_argument("--nz", type=int, default=8, help="even: a node layer lies at mid-height")
ap.add_argument("--degree", type=int, default=2)
ap.add_argument("--E", type=float, default=1.0)
ap.add_argument("--nu", type=float, default=0.3)
ap.add_argument("--pressure", type=float, default=0.02, help="in units of E")
ap.add_argument("--increments", type=int, default=5)
ap.add_argument("--tangent", choices=("full", "none"), default="full")
ap.add_argument("--stress", action="store_true", help="report the von Mises and hoop stresses of the solution")
ap.add_argument("--oracle", action="store_true", help="TESTS ONLY: the same solve on the CPU oracle (portable surface load)")
args = ap.parse_args()
if args.oracle:
    lib = cd.CeedLib(os.path.join(ROOT, "oracle", "liboracle_ceed.so")); c = cd.Ceed(lib, "/cpu/self/oracle")
else:
    lib = cd.CeedLib(cd.PRODUCT_LIB); c = cd.Ceed(lib, "/gpu/hip/mi355x")
r_in = 0.5
mesh = hollow_cylinder_mesh(args.nr, args.nth, args.nz, r_in=r_in, r_out=1.0, z0=-1.0, z1=1.0)
p = SolidProblem(c, mesh, args.degree, "hyperFS", nu=args.nu, E=args.E, bc_sides=[998, 999])
s = NewtonPMG(p, pressure={996: args.pressure * args.E}, pressure_tangent=args.tangent)
st = s.solve(args.increments)
dm = p.levels[p.fine].dofmap
wall = side_set_nodes(mesh, dm, [996])
mid = wall[np.abs(dm.node_coords[wall, 2]) < 1e-12]
x = (dm.node_coords + (s.U.to_numpy() + s.bcv.to_numpy()).reshape(-1, 3))[mid]
radius = np.linalg.norm(x[:, :2], axis=1)
print(json.dumps({"resource": c.resource, "elements": mesh.nelem, "degree": args.degree, "dofs": p.lsize(), "pressure_over_E": args.pressure,
                  "pressure_tangent": args.tangent, "surface_kernel": s.pressure_loads[0][0].kernel_name, "converged": st.converged,
                  "increments": st.increments, "snes_its": st.newton_its, "ksp_its": st.ksp_its, "snes_solve_s": st.seconds,
                  "inner_radius_reference": float(np.linalg.norm(dm.node_coords[mid, :2], axis=1).mean()),
                  "inner_radius_mid_height": float(radius.mean()), "inner_radius_spread": float(radius.max() - radius.min())}))
if args.stress:
    from ceedpetscsolid_amd.postprocess import Stress
    xloc = c.vector(p.lsize()).set_array(s.U.to_numpy() + s.bcv.to_numpy())      # the displacement with the boundary values inserted
    sr = Stress(p, "hyperFS")
    vm, node = sr.max_von_mises(xloc)
    sig = sr.nodal(xloc)
    pos = dm.node_coords + xloc.to_numpy().reshape(-1, 3)

    def hoop(side):
        nodes = side_set_nodes(mesh, dm, [side])
        nodes = nodes[np.abs(dm.node_coords[nodes, 2]) < 1e-12]
        t = np.stack([-pos[nodes, 1], pos[nodes, 0]], axis=1) / np.linalg.norm(pos[nodes, :2], axis=1)[:, None]     # e_theta at the deformed position
        xx, yy, xy = sig[nodes, 0], sig[nodes, 1], sig[nodes, 5]
        return float((t[:, 0] ** 2 * xx + t[:, 1] ** 2 * yy + 2 * t[:, 0] * t[:, 1] * xy).mean())

    pr, a2, b2 = args.pressure * args.E, r_in ** 2, 1.0
    lame = lambda r2: pr * a2 / (b2 - a2) * (1 + b2 / r2)
    print(json.dumps({"stress_kernels": sr.kernel_names, "max_von_mises": vm, "max_von_mises_node": node,
                      "max_von_mises_at": [float(v) for v in dm.node_coords[node]],
                      "hoop_inner_wall_mid_height": hoop(996), "hoop_inner_lame": lame(a2),
                      "hoop_outer_wall_mid_height": hoop(997), "hoop_outer_lame": lame(b2)}))
    sr.destroy()
sys.exit(0 if st.converged else 1)
