"""Free vibration of a clamped bar released from a bent state (dynamics.NewmarkPMG).

A bar of 4 x 1 x 1 elements, 4 long, 1 wide and 0.5 thick (linElas, p = 2; the thin direction makes the lowest bending mode a single one), the end x = 0 clamped, is bent by a static transverse body force (solver.NewtonPMG), then released:
the force is switched off and the bar is stepped with the average-acceleration rule (beta = 1/4, gamma = 1/2).  The scheme is linear
here, so every mode of K phi = omega^2 rho M phi evolves on its own: the component q_n = phi_1 . M u_n / phi_1 . M phi_1 of the lowest
mode is exactly q_0 cos(n theta), theta = 2 atan(omega_1 dt / 2).  The script forms K and M densely from unit-vector applies (243 dofs),
prints that exact theta beside the one measured from q_1 / q_0, the period 2 pi dt / theta of the discrete motion beside the one read off
the zero crossings of q_n and the continuous 2 pi / omega_1, and the total energy 1/2 v . M v + 1/2 u . K u at the start and the end.

    python examples/solve_vibration.py            # on the device
    python examples/solve_vibration.py --oracle   # on the CPU oracle (portable mass operator)
    python examples/solve_vibration.py --fused-mass auto   # K + a0 rho M in ONE fused apply per level where the library has the kernel
"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.dynamics import NewmarkPMG
from ceedpetscsolid_amd.mass import MassOperator
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG

ap = argparse.ArgumentParser()
ap.add_argument("--oracle", action="store_true"); ap.add_argument("--steps-per-period", type=int, default=40)
ap.add_argument("--periods", type=float, default=2.0); ap.add_argument("--density", type=float, default=1.0)
ap.add_argument("--fused-mass", choices=["off", "on", "auto"], default="off", help="NewmarkPMG(fused_mass=False / True / 'auto')")
a = ap.parse_args()
c = cd.Ceed(cd.CeedLib(os.path.join(ROOT, "oracle", "liboracle_ceed.so")), "/cpu/self/oracle") if a.oracle else cd.Ceed(cd.CeedLib(cd.PRODUCT_LIB), "/gpu/hip/mi355x")
prob = SolidProblem(c, box_mesh(4, 1, 1, hi=(4.0, 1.0, 0.5)), 2, "linElas", nu=0.3, E=1.0, bc_sides=[6])
n = prob.lsize()
free = np.nonzero(prob.levels[prob.fine].mask == 0)[0]


def dense(apply):
    X, Y, A = c.vector(n), c.vector(n), np.zeros((free.size, free.size))
    for k, j in enumerate(free):
        e = np.zeros(n); e[j] = 1.0
        X.set_array(e); apply(X, Y)
        A[:, k] = Y.to_numpy()[free]
    return 0.5 * (A + A.T)


mop = MassOperator(prob, prob.fine, a.density)
K, M = dense(lambda x, y: prob.apply_jacobian(prob.fine, x, y)), dense(mop.apply)
L = np.linalg.cholesky(M)
w2, Yv = np.linalg.eigh(np.linalg.solve(L, np.linalg.solve(L, K).T).T)
omega, phi = float(np.sqrt(w2[0])), np.linalg.solve(L.T, Yv[:, 0])

# the bent state: static equilibrium under a transverse body force
bend = NewtonPMG(prob, forcing=np.tile([0.0, 0.0, -2e-6], n // 3), ksp_rtol=1e-10, snes_rtol=1e-10)
bend.solve(num_increments=1)
u0 = bend.U.to_numpy().copy()
bend.destroy()                                  # (the static solver's vectors go before the time stepper makes its own)
dt = 2.0 * np.pi / omega / a.steps_per_period
theta = 2.0 * np.arctan(0.5 * omega * dt)
sol = NewmarkPMG(prob, a.density, dt, ksp_rtol=1e-10, snes_rtol=1e-10, fused_mass={"off": False, "on": True, "auto": "auto"}[a.fused_mass])
sol.set_initial(u0=u0)
q = lambda u: float(phi @ M @ u[free]) / float(phi @ M @ phi)
energy = lambda: 0.5 * sol.vn.to_numpy()[free] @ M @ sol.vn.to_numpy()[free] + 0.5 * sol.xn.to_numpy()[free] @ K @ sol.xn.to_numpy()[free]
e0, qs = energy(), [q(u0)]
nsteps = int(round(a.periods * a.steps_per_period))
kin, its = [], []
for _ in range(nsteps):
    st = sol.step()
    qs.append(q(sol.U.to_numpy())); kin.append(sol.kinetic_energy()); its.append((st.newton_its, st.ksp_its))
qs = np.array(qs)
theta_meas = float(np.arccos(np.clip(qs[1] / qs[0], -1.0, 1.0)))
down = [k + qs[k] / (qs[k] - qs[k + 1]) for k in range(nsteps) if qs[k] > 0.0 >= qs[k + 1]]         # downward zero crossings, in steps
period_meas = (down[1] - down[0]) * dt if len(down) > 1 else float("nan")
print(f"resource {c.resource}; mass operator: {mop.kernel_name}; {free.size} free dofs, omega_1 = {omega:.8f}, dt = {dt:.6f}")
print(f"tip deflection of the bent state {np.abs(u0).max():.4e}; lowest mode carries {abs(qs[0]) * np.sqrt(phi @ M @ phi) / np.sqrt(u0[free] @ M @ u0[free]):.4f} of |u0|_M")
print(f"theta  exact 2 atan(omega dt / 2) = {theta:.12f}   measured acos(q_1 / q_0) = {theta_meas:.12f}")
print(f"period continuous 2 pi / omega = {2 * np.pi / omega:.6f}   discrete 2 pi dt / theta = {2 * np.pi * dt / theta:.6f}   from zero crossings = {period_meas:.6f}")
print(f"worst |q_n - q_0 cos(n theta)| / |q_0| over {nsteps} steps = {np.abs(qs - qs[0] * np.cos(theta * np.arange(nsteps + 1))).max() / abs(qs[0]):.3e}")
print(f"energy at the start {e0:.12e}   at the end {energy():.12e}   kinetic energy peak {max(kin):.6e}")
print(f"Newton / Krylov iterations per step: {its[-1][0]} / {its[-1][1]}")
print(f"tangent of the fine level: {prob.levels[prob.fine].opJacob.kernel_name}" + ("" if sol._mass_in_op else " + the mass operator (two passes)"))
