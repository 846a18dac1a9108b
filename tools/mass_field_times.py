"""The mass operator with a density field (mass.MassOperator(..., density=), csrc/kernels_mass.hip: k_mass's modes with a field) beside
the constant-coefficient one of the same problem: the figures of profiles/mass_field.txt.

linElas at --degree (default 4) on config 3's 5 580-element cylinder and on the 99 000-element one (--meshes).  Device-event times
(CeedXOperatorSetTiming: everything an apply queues -- the mass kernel and the ordered node sum), the MEDIAN of five repeats of `--reps`
applies after a warm-up; the diagonal between two events of torch's on the Ceed's stream (the diagonal records no device events).
The bytes are COUNTED from shapes, not measured by counters: per element 4 P^3 of offsets, 24 P^3 gathered, 8 Q^3 of qdata and
24 P^3 stored; the field adds 4 P^3 of its offsets and 8 P^3 gathered.  One JSON line per mesh."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mass import DensityField, MassOperator
from ceedpetscsolid_amd.mesh import hollow_cylinder_mesh, load_mesh_npz
from ceedpetscsolid_amd.solid import SolidProblem

ap = argparse.ArgumentParser()
ap.add_argument("--meshes", default="config3,cylinder99000")
ap.add_argument("--degree", type=int, default=4); ap.add_argument("--reps", type=int, default=20)
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
    p = SolidProblem(c, mesh, a.degree, "linElas", nu=0.3, E=1.0, bc_sides=[998, 999], multigrid="none")
    n, P, Q, ne = p.lsize(), a.degree + 1, p.Q, mesh.nelem
    ops = {"mass": MassOperator(p, 0, 2.0),
           "mass_field_nodal": MassOperator(p, 0, 2.0, density=DensityField.nodal(lambda X: 1.0 + 0.5 * np.sin(X[:, 2]) ** 2)),
           "mass_field_per_element": MassOperator(p, 0, 2.0, density=DensityField.per_element(1.0 + np.arange(ne) % 2))}
    X, Y, D = c.vector(n).set_array(np.random.default_rng(0).uniform(-1, 1, n)), c.vector(n), c.vector(n)
    us, names = {}, {}
    for k, m in ops.items():
        for _ in range(3):
            m.apply(X, Y); m.diagonal(D)
        c.synchronize()
        us[k + " apply"] = timed(m.op, lambda m=m: m.apply(X, Y))
        names[k + " apply"] = m.kernel_name
        us[k + " diagonal"] = timed_events(lambda m=m: m.diagonal(D))
        names[k + " diagonal"] = m.kernel_name
    base, extra = ne * (4 * P ** 3 + 48 * P ** 3 + 8 * Q ** 3), ne * (4 * P ** 3 + 8 * P ** 3)
    print(json.dumps(dict(resource=c.resource, mesh=which, elements=ne, degree=a.degree, P=P, Q=Q, dofs=n, reps=a.reps, kernels=names,
                          us_median_of_5=us, kernel_MB_counted=dict(mass=round(base / 1e6, 2), mass_field=round((base + extra) / 1e6, 2)),
                          counted_bytes_ratio=round((base + extra) / base, 3),
                          apply_time_ratio_nodal=round(us["mass_field_nodal apply"] / us["mass apply"], 3))), flush=True)
    for m in ops.values():
        m.destroy()
    p.destroy()
