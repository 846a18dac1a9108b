"""The mass operator beside the Jacobian apply of the same problem, and one Newmark step beside one static load increment.

Device-event times (CeedXOperatorSetTiming: the mass kernel with its k_assemble, the fused kernel with its k_assemble) over `reps` applies
after a warm-up, three repeats each, alternating; the mass apply's byte floor counted from shapes,
nelem (4 P^3 + 48 P^3 + 8 Q^3) + 16 lsize (offsets, gather and E-vector store, w det J; the sum's read of y and store), as a fraction
of `--hbm-tbs`; the diagonal by the host clock around a synchronise.  `--solve`: one Newmark step (dynamics.NewmarkPMG) and the first
of `--increments` static load increments (solver.NewtonPMG) on the same mesh, clamps and body force (rho M g).  One JSON line."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mass import MassOperator
from ceedpetscsolid_amd.mesh import hollow_cylinder_mesh, load_mesh_npz
from ceedpetscsolid_amd.solid import SolidProblem

ap = argparse.ArgumentParser()
ap.add_argument("--mesh", default="cylinder", help="'cylinder' (nr x nth x nz hexes) or 'config3' (tests/golden/mesh_cylinder8_5580e_4ss_us.npz)")
ap.add_argument("--nr", type=int, default=10); ap.add_argument("--nth", type=int, default=110); ap.add_argument("--nz", type=int, default=90)
ap.add_argument("--degree", type=int, default=4); ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--hbm-tbs", type=float, default=8.0, help="the HBM rate the byte floor is held against, TB/s")
ap.add_argument("--solve", action="store_true"); ap.add_argument("--increments", type=int, default=10)
ap.add_argument("--coarse", default="assembled", choices=["chebyshev", "assembled", "amg"])
ap.add_argument("--gravity", type=float, default=1e-2); ap.add_argument("--dt", type=float, default=0.5); ap.add_argument("--density", type=float, default=1.0)
a = ap.parse_args()
c = cd.Ceed(cd.CeedLib(cd.PRODUCT_LIB), "/gpu/hip/mi355x")
mesh = hollow_cylinder_mesh(a.nr, a.nth, a.nz) if a.mesh == "cylinder" else load_mesh_npz(os.path.join(ROOT, "tests", "golden", "mesh_cylinder8_5580e_4ss_us.npz"))
bc = [998, 999]                                           # both ends clamped (config 3's Dirichlet sets)
out = {"resource": c.resource, "mesh": a.mesh, "elements": mesh.nelem, "degree": a.degree}

p = SolidProblem(c, mesh, a.degree, "hyperFS", nu=0.3, E=1.0, bc_sides=bc, multigrid="none")
lv = p.levels[p.fine]
n, P, Q = p.lsize(), a.degree + 1, p.Q
m = MassOperator(p, p.fine, a.density)
U, R, X, Y, D = c.vector(n).set_array(p.smooth_state(0.05)), c.vector(n), c.vector(n).set_array(np.random.default_rng(0).uniform(-1, 1, n)), c.vector(n), c.vector(n)
p.form_residual(U, R)
ops = {"jacobian_apply": (lv.opJacob, lambda: p.apply_jacobian(p.fine, X, Y)), "mass_apply": (m.op, lambda: m.apply(X, Y)),
       "mass_apply_add": (m.op, lambda: m.apply_add(X, Y))}
for _, f in ops.values():
    for _ in range(5):
        f()
c.synchronize()
us = {k: [] for k in ops}
for rep in range(3):
    for k, (op, f) in ops.items():
        op.set_timing(True)
        for _ in range(a.reps):
            f()
        ms, launches = op.get_timing()
        op.set_timing(False)
        us[k].append(round(1e3 * ms / max(launches, 1), 2))
names = {"jacobian_apply": lv.opJacob.kernel_name, "mass_apply": m.kernel_name}
m.diagonal(D); c.synchronize()
t0 = time.perf_counter()
for _ in range(a.reps):
    m.diagonal(D)
c.synchronize()
us["mass_diagonal_host_clock"] = [round(1e6 * (time.perf_counter() - t0) / a.reps, 2)]
names["mass_diagonal"] = m.kernel_name
floor = mesh.nelem * (4 * P ** 3 + 48 * P ** 3 + 8 * Q ** 3) + 16 * n
best = min(us["mass_apply"])
out.update(dofs=n, P=P, Q=Q, kernels=names, reps=a.reps, us_per_apply=us, mass_byte_floor_MB=round(floor / 1e6, 2),
           mass_floor_us_at_hbm_rate=round(floor / (a.hbm_tbs * 1e6), 2), mass_fraction_of_floor=round(floor / (a.hbm_tbs * 1e6) / best, 3),
           mass_GBs_on_floor=round(floor / best / 1e3, 1))
m.destroy(); p.destroy()

if a.solve:
    print(json.dumps(out), file=sys.stderr, flush=True)      # (the operator figures, should the solves below be cut short)
    from ceedpetscsolid_amd.dynamics import NewmarkPMG
    from ceedpetscsolid_amd.solver import NewtonPMG
    p = SolidProblem(c, mesh, a.degree, "hyperFS", nu=0.3, E=1.0, bc_sides=bc)
    n = p.lsize()
    # a consistent body force rho M g, g = --gravity along -z (nodal values would grow with the number of nodes)
    mg = MassOperator(p, p.fine, a.density, mask_mode=2)
    G, F = c.vector(n).set_array(np.tile([0.0, 0.0, -a.gravity], n // 3)), c.vector(n)
    mg.apply(G, F)
    force = F.to_numpy().copy()
    mg.destroy()
    kw = dict(forcing=force, coarse=a.coarse, graph="auto", fuse_epilogue="auto")
    s = NewtonPMG(p, **kw)
    s.solve(num_increments=a.increments, stop_after=1)    # the first solve also pays the one-time set-up (maps, the forms' timing)
    s.stats = type(s.stats)()
    print("static increment warmed", file=sys.stderr, flush=True)
    st = s.solve(num_increments=a.increments, stop_after=1)
    out["static_increment"] = dict(newton=st.newton_its, krylov=st.ksp_its, seconds=round(st.seconds, 3), converged=st.converged, tuning=s.tuning)
    d = NewmarkPMG(p, a.density, a.dt, **dict(kw, fuse_epilogue=False))
    d.set_initial(load=1.0 / a.increments)
    d.step()                                              # (as above)
    st = d.step()
    out["newmark_step"] = dict(newton=st.newton_its, krylov=st.ksp_its, seconds=round(st.seconds, 3), converged=st.converged, tuning=d.tuning,
                               dt=a.dt, a0_density=d.a0 * a.density)
print(json.dumps(out))
