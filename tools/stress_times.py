"""Stress recovery (postprocess.Stress, csrc/kernels_stress.hip) beside the diagnostic operator and one residual apply of the same problem:
the figures of profiles/stress.txt.

hyperFS at --degree (default 4) on config 3's 5 580-element cylinder and on the 99 000-element one (--meshes).  Device-event times
(CeedXOperatorSetTiming: everything an apply queues -- the stress kernel alone for the points, the kernel and the ordered node sum for
the nodal form; the fused residual kernel and its sum), the MEDIAN of five repeats of `--reps` applies after a warm-up.  Between two
events of torch's on the Ceed's stream, the same way: the diagnostic operator's apply (its family records no device events), and the node
sum alone -- the transpose of the 7-component output restriction on an E-vector of the same size.  The byte floor of the stress kernel
is COUNTED from shapes, not measured by counters: per element 28 P^3 gathered with offsets, 80 Q^3 of qdata, and 48 Q^3 (points) or
56 P^3 (nodal) stored.  One JSON line per mesh."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mesh import hollow_cylinder_mesh, load_mesh_npz
from ceedpetscsolid_amd.postprocess import Diagnostics, Stress
from ceedpetscsolid_amd.solid import SolidProblem

ap = argparse.ArgumentParser()
ap.add_argument("--meshes", default="config3,cylinder99000")
ap.add_argument("--degree", type=int, default=4); ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--hbm-tbs", type=float, default=8.0, help="the HBM rate the byte floor is held against, TB/s")
a = ap.parse_args()
c = cd.Ceed(cd.CeedLib(cd.PRODUCT_LIB), "/gpu/hip/mi355x")
c.set_stream(torch.cuda.current_stream().cuda_stream)


def timed(op, f):
    """median over five repeats of the device time of one apply, microseconds"""
    us = []
    for _ in range(5):
        op.set_timing(True)
        for _ in range(a.reps):
            f()
        ms, launches = op.get_timing()
        op.set_timing(False)
        us.append(1e3 * ms / max(launches, 1))
    return round(statistics.median(us), 2)


def timed_events(f):
    """the same between two events on the stream"""
    us = []
    for _ in range(5):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.reps):
            f()
        t1.record(); t1.synchronize()
        us.append(1e3 * t0.elapsed_time(t1) / a.reps)
    return round(statistics.median(us), 2)


for which in a.meshes.split(","):
    mesh = load_mesh_npz(os.path.join(ROOT, "tests", "golden", "mesh_cylinder8_5580e_4ss_us.npz")) if which == "config3" else hollow_cylinder_mesh(10, 110, 90)
    p = SolidProblem(c, mesh, a.degree, "hyperFS", nu=0.3, E=1.0, bc_sides=[998, 999], multigrid="none")
    n, P, Q, ne = p.lsize(), a.degree + 1, p.Q, mesh.nelem
    st, dg = Stress(p, "hyperFS"), Diagnostics(p, "hyperFS")
    U, R = c.vector(n).set_array(p.smooth_state(0.05)), c.vector(n)
    ops = {"stress_points": (st.op_pts, lambda: st.op_pts.apply(U, st.spts)), "stress_nodal": (st.op_nod, lambda: st.op_nod.apply(U, st.snod)),
           "diagnostic": (dg.op, lambda: dg.op.apply(U, dg.dloc)), "residual": (p.opApply, lambda: p.opApply.apply(U, R))}
    for _, f in ops.values():
        for _ in range(3):
            f()
    c.synchronize()
    us = {k: timed(op, f) for k, (op, f) in ops.items() if k != "diagnostic"}
    ev, lv = st.rstr_nod.create_evector().set_value(1.0), c.vector(7 * st.nnodes)
    ev.device_pointer(); lv.device_pointer()
    us["diagnostic"] = timed_events(ops["diagnostic"][1])
    us["node_sum_alone"] = timed_events(lambda: st.rstr_nod.apply(cd.TRANSPOSE, ev, lv))
    floor = {"points": ne * (28 * P ** 3 + 80 * Q ** 3 + 48 * Q ** 3), "nodal": ne * (28 * P ** 3 + 80 * Q ** 3 + 56 * P ** 3)}
    print(json.dumps(dict(resource=c.resource, mesh=which, elements=ne, degree=a.degree, P=P, Q=Q, dofs=n, reps=a.reps,
                          kernels=dict(st.kernel_names, diagnostic=dg.op.kernel_name, residual=p.opApply.kernel_name),
                          us_per_apply_median_of_5=us,
                          kernel_byte_floor_MB_counted={k: round(v / 1e6, 2) for k, v in floor.items()},
                          floor_us_at_hbm_rate={k: round(v / (a.hbm_tbs * 1e6), 2) for k, v in floor.items()},
                          points_fraction_of_floor=round(floor["points"] / (a.hbm_tbs * 1e6) / us["stress_points"], 3),
                          nodal_kernel_fraction_of_floor=round(floor["nodal"] / (a.hbm_tbs * 1e6) / max(us["stress_nodal"] - us["node_sum_alone"], 1e-9), 3))), flush=True)
    st.destroy(); p.destroy()
