"""One support state formation, force add, tangent add and diagonal add on the inner wall of a hollow cylinder beside the fine Jacobian
apply of the same problem.  Host clock around `reps` calls that end in a synchronise, after a warm-up of every shape; three repeats
each, alternating.  One JSON line; profiles/support.txt keeps what it printed."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mesh import hollow_cylinder_mesh
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.support import SupportSurface

ap = argparse.ArgumentParser()
ap.add_argument("--nr", type=int, default=10); ap.add_argument("--nth", type=int, default=110); ap.add_argument("--nz", type=int, default=90)
ap.add_argument("--degree", type=int, default=4); ap.add_argument("--reps", type=int, default=200); ap.add_argument("--oracle", action="store_true")
a = ap.parse_args()
c = cd.Ceed(cd.CeedLib(os.path.join(ROOT, "oracle", "liboracle_ceed.so")), "/cpu/self/oracle") if a.oracle else cd.Ceed(cd.CeedLib(cd.PRODUCT_LIB), "/gpu/hip/mi355x")
mesh = hollow_cylinder_mesh(a.nr, a.nth, a.nz)
p = SolidProblem(c, mesh, a.degree, "hyperFS", nu=0.3, E=1.0, bc_sides=[998, 999], multigrid="none")
lv = p.levels[p.fine]
n = p.lsize()
sp = SupportSurface(c, mesh, lv.dofmap, [996], p.Q, mask=lv.mask)
U, R, DU, Y = c.vector(n).set_array(p.smooth_state(0.05)), c.vector(n), c.vector(n).set_array(np.random.default_rng(0).uniform(-1, 1, n)), c.vector(n).set_value(0.0)
S = sp.new_state()
p.form_residual(U, R)
work = {"jacobian_apply": lambda: p.apply_jacobian(p.fine, DU, Y), "form_state": lambda: sp.form_state(3.0, 1.0, S),
        "force_add": lambda: sp.force_add(1.0, S, U, R), "tangent_add": lambda: sp.tangent_add(1.0, S, DU, Y), "diagonal_add": lambda: sp.diagonal_add(1.0, S, Y)}
names = {}
for k, f in work.items():
    for _ in range(5):
        f()
    names[k] = lv.opJacob.kernel_name if k == "jacobian_apply" else sp.kernel_name
c.synchronize()
times = {k: [] for k in work}
for rep in range(3):
    for k, f in work.items():
        reps = a.reps if k != "jacobian_apply" else max(a.reps // 4, 1)
        c.synchronize(); t0 = time.perf_counter()
        for _ in range(reps):
            f()
        c.synchronize()
        times[k].append(1e6 * (time.perf_counter() - t0) / reps)
area = sp.area(S)
print(json.dumps({"resource": c.resource, "elements": mesh.nelem, "degree": a.degree, "dofs": n, "faces": sp.nface, "kernels": names,
                  "area": area, "area_of_the_prism": 2 * a.nth * 0.5 * np.sin(np.pi / a.nth) * 10.0, "reps": a.reps,
                  "us_per_call": {k: [round(t, 2) for t in v] for k, v in times.items()}}))
