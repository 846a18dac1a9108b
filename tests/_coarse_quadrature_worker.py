"""Worker of the two-rank gloo solve with coarse_quadrature="own" (test_coarse_quadrature.py): operators are per rank and the
stored state is element-local, so the option needs nothing from the halo exchange."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MESH = (1, 6, 4)          # hollow cylinder, z in [-1, 1]
DEGREE, PROBLEM = 3, "hyperSS"      # levels p = 1, 2, 3: p = 1 is assembled (coarse="amg"), p = 2 a MATRIX-FREE own-quadrature level (Q_c = 3 under P_f = 4)
CLAMP_998 = (0.0, -0.05, 0.1)


def run(rank, world, initfile, outdir, coarse):
    from ceedpetscsolid_amd import ceed as cd
    from ceedpetscsolid_amd.halo import HaloExchange
    from ceedpetscsolid_amd.mesh import hollow_cylinder_mesh, partition_slabs, submesh
    from ceedpetscsolid_amd.solid import SolidProblem
    from ceedpetscsolid_amd.solver import NewtonPMG
    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world)
    lib = cd.CeedLib(os.path.join(ROOT, "oracle", "liboracle_ceed.so"))   # tests only: the oracle as local operator
    ceed = cd.Ceed(lib, "/cpu/self/oracle")
    full = hollow_cylinder_mesh(*MESH, z0=-1.0, z1=1.0)
    mesh = submesh(full, partition_slabs(full, world)[rank])
    bc = [s for s in (998, 999) if s in mesh.side_sets and len(mesh.side_sets[s])]
    p = SolidProblem(ceed, mesh, DEGREE, PROBLEM, nu=0.3, E=10.0, bc_sides=bc, coarse_quadrature="own")
    halos = [HaloExchange(mesh, lv.dofmap, device="cpu") for lv in p.levels]
    clamp = {s: ({"translate": CLAMP_998} if s == 998 else {}) for s in bc}
    s = NewtonPMG(p, clamp=clamp, halo=halos, coarse=coarse)
    st = s.solve(1)
    lvf = p.levels[p.fine]
    np.savez(os.path.join(outdir, f"own_{rank}.npz"), coords=lvf.dofmap.node_coords, U=s.U.to_numpy(),
             converged=st.converged, newton=st.newton_its, ksp=st.ksp_its, points=np.array([lv.Q for lv in p.levels]))
    dist.barrier()
    dist.destroy_process_group()
