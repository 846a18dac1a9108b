"""The thermal load kernels (thermal.ThermalLoad, postprocess.Stress(thermal=); csrc/kernels_stress.hip: k_stress's modes with a temperature
field) beside the stress and mass kernels of the same problem: the figures of profiles/thermal.txt.

hyperFS at --degree (default 4) on config 3's 5 580-element cylinder and on the 99 000-element one (--meshes).  Device-event times
(CeedXOperatorSetTiming: everything an apply queues -- the kernel and the ordered node sum), the MEDIAN of five repeats of `--reps`
applies after a warm-up, the operators taken in turn within every repeat (interleaved), so a drift of the clock falls on all of them.
One JSON line per mesh."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mass import MassOperator
from ceedpetscsolid_amd.mesh import hollow_cylinder_mesh, load_mesh_npz
from ceedpetscsolid_amd.postprocess import Stress
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.thermal import ThermalLoad

ap = argparse.ArgumentParser()
ap.add_argument("--meshes", default="config3,cylinder99000")
ap.add_argument("--degree", type=int, default=4); ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()
c = cd.Ceed(cd.CeedLib(cd.PRODUCT_LIB), "/gpu/hip/mi355x")
c.set_stream(torch.cuda.current_stream().cuda_stream)

for which in a.meshes.split(","):
    mesh = load_mesh_npz(os.path.join(ROOT, "tests", "golden", "mesh_cylinder8_5580e_4ss_us.npz")) if which == "config3" else hollow_cylinder_mesh(10, 110, 90)
    p = SolidProblem(c, mesh, a.degree, "hyperFS", nu=0.3, E=1.0, bc_sides=[998, 999], multigrid="none")
    n, ne = p.lsize(), mesh.nelem
    tl = ThermalLoad(p, 0, 1e-3, lambda X: 20.0 * (1.0 + 0.5 * np.sin(X[:, 2])), "hyperFS")
    st, st0, m = Stress(p, "hyperFS", thermal=tl), Stress(p, "hyperFS"), MassOperator(p, 0, 2.0)
    U, D, Y = c.vector(n).set_array(p.smooth_state(0.05)), c.vector(n).set_array(np.random.default_rng(0).uniform(-1, 1, n)), c.vector(n)
    tl.force(U, Y)                                       # the state is loaded once; the timed applies go to the operators themselves
    runs = {"thermal force": (tl.op_force, lambda: tl.op_force.apply(tl.theta_vec, Y)),
            "thermal tangent": (tl.op_tangent, lambda: tl.op_tangent.apply(D, Y)),
            "stress points + thermal": (st.op_pts, lambda: st.op_pts.apply(U, st.spts)),
            "stress points": (st0.op_pts, lambda: st0.op_pts.apply(U, st0.spts)),
            "stress nodal + thermal": (st.op_nod, lambda: st.op_nod.apply(U, st.snod)),
            "stress nodal": (st0.op_nod, lambda: st0.op_nod.apply(U, st0.snod)),
            "mass apply": (m.op, lambda: m.apply(D, Y))}
    for _ in range(3):                                   # warm-up
        for op, f in runs.values():
            f()
    c.synchronize()
    us = {k: [] for k in runs}
    for _ in range(5):
        for k, (op, f) in runs.items():                  # interleaved: every operator once per repeat
            op.set_timing(True)
            for _ in range(a.reps):
                f()
            ms, launches = op.get_timing()
            op.set_timing(False)
            us[k].append(1e3 * ms / max(launches, 1))
    print(json.dumps(dict(resource=c.resource, mesh=which, elements=ne, degree=a.degree, P=a.degree + 1, Q=p.Q, dofs=n, reps=a.reps,
                          kernels={k: op.kernel_name for k, (op, f) in runs.items()},
                          us_median_of_5={k: round(statistics.median(v), 2) for k, v in us.items()})), flush=True)
    for o in (st, st0, m, tl):
        o.destroy()
    p.destroy()
