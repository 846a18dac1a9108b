"""One explicit time step (dynamics.ExplicitDynamics) beside the residual apply of the same problem, and the fused step kernel
(CeedXVectorLeapfrogStep) beside the SAME update composed from the existing vector calls.

Device-event times (events on the stream the Ceed queues on) over `--reps` calls after a warm-up, three repeats each, the variants
alternating; the step kernel's byte floor is 8 B x (x, vh read and written, r, m read: 6 streams; with a load vector f: 7) per dof,
held against `--hbm-tbs` (the copy rate DESIGN 4 records).  The composed update is  q = r .* (-1/m);  vo = vh;  vh = c1 vh + c2 q;
vo = (vo + vh) / 2;  tally = sum m vo vo;  x += dt vh  (pointwise_mult, a copy, three axpby, a weighted dot: 17 streams), and with a load
vector  g = load f - r  first (waxpby: 20 streams).  Steps per second by the host clock around a synchronise, eager and replayed
(`run(graph=True)`), no sampling.  One JSON line per mesh."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.dynamics import ExplicitDynamics
from ceedpetscsolid_amd.mesh import hollow_cylinder_mesh, load_mesh_npz
from ceedpetscsolid_amd.solid import SolidProblem

ap = argparse.ArgumentParser()
ap.add_argument("--mesh", default="config3", help="'cylinder' (nr x nth x nz hexes) or 'config3' (tests/golden/mesh_cylinder8_5580e_4ss_us.npz)")
ap.add_argument("--nr", type=int, default=10); ap.add_argument("--nth", type=int, default=110); ap.add_argument("--nz", type=int, default=90)
ap.add_argument("--degree", type=int, default=4); ap.add_argument("--reps", type=int, default=100); ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--hbm-tbs", type=float, default=6.29, help="the HBM rate the byte floor is held against, TB/s")
ap.add_argument("--gravity", type=float, default=1e-3); ap.add_argument("--density", type=float, default=1.0)
a = ap.parse_args()
c = cd.Ceed(cd.CeedLib(cd.PRODUCT_LIB), "/gpu/hip/mi355x")
mesh = hollow_cylinder_mesh(a.nr, a.nth, a.nz) if a.mesh == "cylinder" else load_mesh_npz(os.path.join(ROOT, "tests", "golden", "mesh_cylinder8_5580e_4ss_us.npz"))
p = SolidProblem(c, mesh, a.degree, "hyperFS", nu=0.3, E=1.0, bc_sides=[998, 999], multigrid="none")
n = p.lsize()
probe = ExplicitDynamics(p, a.density)
m_host = probe.m.to_numpy()
probe.destroy()
sol = ExplicitDynamics(p, a.density, forcing=m_host * np.tile([0.0, 0.0, -a.gravity], n // 3))
sol.set_initial()
out = {"resource": c.resource, "mesh": a.mesh, "elements": mesh.nelem, "degree": a.degree, "dofs": n, "dt": sol.dt, "emax": sol.emax_K,
       "min_free_mass": float(m_host[sol.free].min()), "reps": a.reps}
print(json.dumps(out), file=sys.stderr, flush=True)


def timed(fn):
    """ms per call: events around `reps` calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / a.reps


# work vectors of the composed update, and copies of the state the kernels may overwrite freely (dt = 0: x and vh stay bounded)
x, vh, vo, q, g = (c.vector(n).set_value(0.0) for _ in range(5))
nminv = c.vector(n).set_array(np.where(m_host > 0.0, -1.0 / np.where(m_host > 0.0, m_host, 1.0), 0.0))
sc = c.vector(4).set_value(0.0)
R, f, m = sol.R, sol.fv, sol.m
c1, c2, dt, load = 1.0, 0.0, 0.0, 1.0


def composed(with_f):
    if with_f:
        g.waxpby(load, f, -1.0, R)
        q.pointwise_mult(g, nminv)          # (the sign of q differs between the two forms: the traffic is what is timed)
    else:
        q.pointwise_mult(R, nminv)
    vo.axpby(1.0, vh, 0.0)
    vh.axpby(c2, q, c1)
    vo.axpby(0.5, vh, 0.5)
    vo.dot_to(vo, sc, 0, m)
    x.axpby(dt, vh, 1.0)


variants = {
    "residual_apply": lambda: p.form_residual(sol.x, sol.R),
    "step_f_tally": lambda: x.leapfrog_step(vh, R, f, m, load, c1, c2, dt, n, sc, 1),
    "step_f": lambda: x.leapfrog_step(vh, R, f, m, load, c1, c2, dt, n),
    "step_tally": lambda: x.leapfrog_step(vh, R, None, m, load, c1, c2, dt, n, sc, 1),
    "step": lambda: x.leapfrog_step(vh, R, None, m, load, c1, c2, dt, n),
    "composed_f_tally": lambda: composed(True),
    "composed_tally": lambda: composed(False),
}
for fn in variants.values():
    for _ in range(3):
        fn()
c.synchronize()
ms = {k: [] for k in variants}
for rep in range(3):
    for k, fn in variants.items():
        ms[k].append(round(timed(fn), 5))
best = {k: min(v) for k, v in ms.items()}
p.form_residual(sol.x, sol.R)              # (R is the state's again)
floor = {k: 8 * (7 if "_f" in k else 6) * n for k in variants if k.startswith("step")}
out.update(ms_per_call=ms,
           step_TBs_on_floor={k: round(floor[k] / best[k] / 1e9, 3) for k in floor},
           step_fraction_of_copy_rate={k: round(floor[k] / best[k] / 1e9 / a.hbm_tbs, 3) for k in floor},
           composed_over_fused={"with_f": round(best["composed_f_tally"] / best["step_f_tally"], 2), "without_f": round(best["composed_tally"] / best["step_tally"], 2)},
           step_over_residual_apply=round((best["step_f"] + best["residual_apply"]) / best["residual_apply"], 3))
rates = {}
for graph in (False, True):
    sol.run(3, graph=graph)                # warm-up of the form
    h = sol.run(a.steps, graph=graph)
    rates["replayed" if graph else "eager"] = round(h["steps"] / h["seconds"], 1)
out.update(steps_per_second=rates, max_disp=float(np.abs(sol.x.to_numpy() - sol._x_start).max()))
print(json.dumps(out))
