"""The set-up and post-processing operators on a hollow cylinder: MMS forcing, MMS true solution, strain energy and the eight diagnostics
(hyperFS), the transpose of an offsets restriction and its multiplicity.  Host clock around one call that ends in a synchronise: the
FIRST call of each (it builds whatever the call builds lazily -- for the energy, the diagnostics and the restriction, which own their
output restriction, the transpose map), the second, and the mean of `reps` more.  CEEDPETSCSOLID_MI355X_LIB selects the build, so that
two builds can be run one after the other on the same box."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mesh import hollow_cylinder_mesh
from ceedpetscsolid_amd.postprocess import Diagnostics, StrainEnergy
from ceedpetscsolid_amd.solid import SolidProblem

ap = argparse.ArgumentParser()
ap.add_argument("--nr", type=int, default=10); ap.add_argument("--nth", type=int, default=110); ap.add_argument("--nz", type=int, default=90)
ap.add_argument("--degree", type=int, default=4); ap.add_argument("--reps", type=int, default=5); ap.add_argument("--label", default=""); ap.add_argument("--oracle", action="store_true")
a = ap.parse_args()
c = cd.Ceed(cd.CeedLib(os.path.join(ROOT, "oracle", "liboracle_ceed.so")), "/cpu/self/oracle") if a.oracle else cd.Ceed(cd.CeedLib(cd.PRODUCT_LIB), "/gpu/hip/mi355x")
mesh = hollow_cylinder_mesh(a.nr, a.nth, a.nz)
p = SolidProblem(c, mesh, a.degree, "hyperFS", nu=0.3, E=1.0, bc_sides=[998, 999], multigrid="none")
lv = p.levels[p.fine]
n, P = p.lsize(), lv.degree + 1


def coord_operator(kind):
    """opSetupForce / opTrue as the reference wires them (setuplibceed.c:555-583, 608-636)"""
    if kind == "true":
        qf = c.qfunction("MMSTrueSoln", source="qfunctions/manufacturedTrue.h:MMSTrueSoln")
        qf.add_input("x", 3, cd.EVAL_INTERP).add_output("true_soln", 3, cd.EVAL_NONE)
        op = c.operator(qf)
        op.set_field("x", p.Erestrictx, c.basis_lagrange(3, 3, 2, P, cd.GAUSS_LOBATTO), "active")
        op.set_field("true_soln", lv.Erestrictu, None, "active")
    else:
        qf = c.qfunction("SetupMMSForce", source="qfunctions/manufacturedForce.h:SetupMMSForce")
        qf.add_input("x", 3, cd.EVAL_INTERP).add_input("qdata", 10, cd.EVAL_NONE).add_output("force", 3, cd.EVAL_INTERP)
        qf.set_context(p.phys)
        op = c.operator(qf)
        op.set_field("x", p.Erestrictx, p.basisx, "active")
        op.set_field("qdata", p.Erestrictqdi, None, p.qdata)
        op.set_field("force", lv.Erestrictu, lv.basisu, "active")
    return op


U = c.vector(n).set_array(p.smooth_state(0.05))
se, dg = StrainEnergy(p, "hyperFS"), Diagnostics(p, "hyperFS")
force, true = coord_operator("mms"), coord_operator("true")
rstr = c.elem_restriction(mesh.nelem, P ** 3, 3, 1, n, lv.dofmap.offsets())        # a restriction of its own: no map yet
E, L, M, F = rstr.create_evector().set_value(1.0), c.vector(n).set_value(0.0), c.vector(n), c.vector(n)
work = {"forcing_mms": lambda: force.apply(p.xcoord, F), "true_solution": lambda: true.apply(p.xcoord, F),
        "energy": lambda: se.op.apply(U, se.eloc), "diagnostics": lambda: dg.op.apply(U, dg.dloc),
        "restriction_transpose": lambda: rstr.apply(cd.TRANSPOSE, E, L), "multiplicity": lambda: rstr.multiplicity(M)}


def timed(f, reps=1):
    c.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        f()
    c.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


ms = {k: {"first": round(timed(f), 3), "second": round(timed(f), 3), "mean_of_more": round(timed(f, a.reps), 3)} for k, f in work.items()}
sums = {"true_solution": float(np.abs(F.to_numpy()).sum()), "energy": float(se.eloc.to_numpy().sum()), "diagnostics": float(np.abs(dg.dloc.to_numpy()).sum()),
        "multiplicity": float(M.to_numpy().sum())}
print(json.dumps({"label": a.label, "library": cd.PRODUCT_LIB, "resource": c.resource, "elements": mesh.nelem, "degree": a.degree, "dofs": n,
                  "reps": a.reps, "ms_per_call": ms, "checksums": sums}))
