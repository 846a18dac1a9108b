"""The effective tangent K + a0 rho M of dynamics.NewmarkPMG as two passes (the Jacobian apply, then the mass operator in add mode) beside
ONE apply of the Jacobian operator with the mass term (CeedXOperatorSetMassTerm, k_fused_pencil_mass), hyperFS at `--degree`.

Per level of the ladder, device-event times (events on the stream the Ceed queues on) over `--reps` calls after a warm-up, three repeats
each, the variants alternating: the Jacobian apply alone, K then M, the fused apply; and the same three for the smoother's Chebyshev
step (CeedXOperatorApplyChebyshev where the operator carries its consumer; the apply, M, then the vector step where it cannot).  Then
the V-cycle of solver.NewtonPMG (static) and of NewmarkPMG with fused_mass False / True, each as the best of its eager form and its
replayed recording, with the consumers in the epilogue wherever the operator allows (fuse_epilogue=True: the two-pass dynamic solve
cannot); and one Newmark step each way by the host clock around a synchronise.  The baseline of every fused figure is the two-pass
figure of the SAME call.  One JSON line per mesh."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.dynamics import NewmarkPMG
from ceedpetscsolid_amd.mass import MassOperator
from ceedpetscsolid_amd.mesh import hollow_cylinder_mesh, load_mesh_npz
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG

ap = argparse.ArgumentParser()
ap.add_argument("--mesh", default="config3", help="'cylinder' (nr x nth x nz hexes) or 'config3' (tests/golden/mesh_cylinder8_5580e_4ss_us.npz)")
ap.add_argument("--nr", type=int, default=10); ap.add_argument("--nth", type=int, default=110); ap.add_argument("--nz", type=int, default=90)
ap.add_argument("--degree", type=int, default=4); ap.add_argument("--reps", type=int, default=50); ap.add_argument("--vcycle-reps", type=int, default=10)
ap.add_argument("--density", type=float, default=1.0); ap.add_argument("--dt", type=float, default=0.05)
ap.add_argument("--coarse", default="amg"); ap.add_argument("--steps", type=int, default=2); ap.add_argument("--gravity", type=float, default=1e-3)
a = ap.parse_args()
c = cd.Ceed(cd.CeedLib(cd.PRODUCT_LIB), "/gpu/hip/mi355x")
mesh = hollow_cylinder_mesh(a.nr, a.nth, a.nz) if a.mesh == "cylinder" else load_mesh_npz(os.path.join(ROOT, "tests", "golden", "mesh_cylinder8_5580e_4ss_us.npz"))
p = SolidProblem(c, mesh, a.degree, "hyperFS", nu=0.3, E=1.0, bc_sides=[998, 999])
n = p.lsize()
coef = a.density / (0.25 * a.dt * a.dt)          # a0 rho
X, Y = c.vector(n).set_array(p.smooth_state(0.05)), c.vector(n)
p.form_residual(X, Y)                            # the stored state of the tangents
out = {"resource": c.resource, "mesh": a.mesh, "elements": mesh.nelem, "degree": a.degree, "dofs": n, "a0_rho": coef, "reps": a.reps,
       "levels": [(lv.degree + 1, lv.Q) for lv in p.levels]}
print(json.dumps(out), file=sys.stderr, flush=True)


def timed(fn, reps):
    """ms per call: events around `reps` calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def best_of(variants, reps):
    for fn in variants.values():
        for _ in range(3):
            fn()
    c.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(3):
        for k, fn in variants.items():
            ms[k].append(round(timed(fn, reps), 5))
    return ms


# ---- per level: the apply and the smoother step, three ways ---------------------------------------------------------------------------
levels = {}
for lv, level in enumerate(p.levels):
    nl = p.lsize(lv)
    op = level.opJacob
    if not op.mass_term_available():
        levels[lv] = {"P": level.degree + 1, "Q": level.Q, "fused": None}
        continue
    M = MassOperator(p, lv, coef)
    x, y, t, d, b, dinv = (c.vector(nl).set_array(np.random.default_rng(3 + k).uniform(-1, 1, nl) * (level.mask == 0)) for k in range(6))
    dinv.set_value(0.0)                          # the step's traffic with d = 0: x stays what it is over the repetitions

    def with_term(on, fn):
        op.set_mass_term(coef if on else 0.0)
        fn()

    def two_pass_apply():
        op.apply(x, y); M.apply_add(x, y)

    def two_pass_step():
        op.apply(x, t); M.apply_add(x, t)
        x.chebyshev_step(d, None, b, t, dinv, 0.37, 0.21, False)

    variants = {
        "jacobian": lambda: with_term(False, lambda: op.apply(x, y)),
        "two_pass": lambda: with_term(False, two_pass_apply),
        "fused": lambda: with_term(True, lambda: op.apply(x, y)),
        "jacobian_step": lambda: with_term(False, lambda: op.apply_chebyshev(x, t, x, d, None, b, dinv, 0.37, 0.21)),
        "two_pass_step": lambda: with_term(False, two_pass_step),
        "fused_step": lambda: with_term(True, lambda: op.apply_chebyshev(x, t, x, d, None, b, dinv, 0.37, 0.21)),
    }
    ms = best_of(variants, a.reps)
    with_term(True, lambda: op.apply(x, y))
    name = op.kernel_name
    op.set_mass_term(0.0)
    bst = {k: min(v) for k, v in ms.items()}
    levels[lv] = {"P": level.degree + 1, "Q": level.Q, "dofs": nl, "kernel": name, "ms": ms,
                  "fused_over_two_pass": round(bst["fused"] / bst["two_pass"], 3), "fused_over_jacobian": round(bst["fused"] / bst["jacobian"], 3),
                  "fused_step_over_two_pass_step": round(bst["fused_step"] / bst["two_pass_step"], 3),
                  "fused_step_over_jacobian_step": round(bst["fused_step"] / bst["jacobian_step"], 3)}
    M.destroy()
    for v in (x, y, t, d, b, dinv):
        v.destroy()
out["per_level"] = levels
print(json.dumps({"per_level": levels}), file=sys.stderr, flush=True)


# ---- the V-cycle: static, two-pass dynamic, fused dynamic; the best of eager and replayed ------------------------------------------------
def vcycle_ms(sol):
    sol.U.set_value(0.0)                         # the tangent of the undeformed state: positive definite on every mesh
    sol.residual(sol.U, sol.R)
    sol.setup_preconditioner()
    top = sol.nlev - 1
    r, z = sol._vec(n, top), sol._vec(n, top)
    sol._set(r, np.random.default_rng(9).uniform(-1, 1, n) * sol.free)
    run = lambda: sol.vcycle(top, r, z)
    run(); c.synchronize()
    g = c.capture(run)
    ms = best_of({"eager": run, "replayed": g.launch}, a.vcycle_reps)
    g.destroy()
    return ms


solvers = {"static": lambda: NewtonPMG(p, coarse=a.coarse, fuse_epilogue=True),
           "two_pass": lambda: NewmarkPMG(p, a.density, a.dt, coarse=a.coarse, fuse_epilogue=True, fused_mass=False),
           "fused": lambda: NewmarkPMG(p, a.density, a.dt, coarse=a.coarse, fuse_epilogue=True, fused_mass="auto")}
vc = {}
for k, make in solvers.items():
    sol = make()
    vc[k] = vcycle_ms(sol)
    if k == "fused":
        out["fused_levels"] = list(sol._mass_in_op)
    sol.destroy()
vbest = {k: min(min(v) for v in ms.values()) for k, ms in vc.items()}
out.update(vcycle_ms=vc, vcycle_best_ms={k: round(v, 4) for k, v in vbest.items()},
           vcycle_fused_over_two_pass=round(vbest["fused"] / vbest["two_pass"], 3), vcycle_fused_over_static=round(vbest["fused"] / vbest["static"], 3),
           vcycle_two_pass_over_static=round(vbest["two_pass"] / vbest["static"], 3))
print(json.dumps({"vcycle_best_ms": out["vcycle_best_ms"]}), file=sys.stderr, flush=True)

# ---- one Newmark step each way (host clock around a synchronise; graph="auto" picks the V-cycle's form by timing it) ----------------------
steps = {}
lump, mv = MassOperator(p, p.fine, a.density, mask_mode=2), c.vector(n)
lump.lumped(mv)
force = mv.to_numpy() * np.tile([0.0, 0.0, -a.gravity], n // 3)          # the body force rho M g
lump.destroy(); mv.destroy()
for k, fused in (("two_pass", False), ("fused", "auto")):
    sol = NewmarkPMG(p, a.density, a.dt, coarse=a.coarse, forcing=force, fuse_epilogue="auto", graph="auto", fused_mass=fused)
    sol.set_initial()
    sol.step()                                   # warm-up: first-use set-up and the timing of the V-cycle's forms
    ts, its = [], []
    for _ in range(a.steps):
        c.synchronize(); t0 = time.perf_counter()
        st = sol.step()
        c.synchronize(); ts.append(round(1e3 * (time.perf_counter() - t0), 3))
        its.append((st.newton_its, st.ksp_its))
    steps[k] = {"ms": ts, "newton_ksp": its, "tuning": sol.tuning}
    sol.destroy()
out["newmark_step"] = steps
out["newmark_step_fused_over_two_pass"] = round(min(steps["fused"]["ms"]) / min(steps["two_pass"]["ms"]), 3)
print(json.dumps(out))
