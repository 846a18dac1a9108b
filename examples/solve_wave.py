"""A longitudinal wave in a clamped bar under a step load (dynamics.ExplicitDynamics).

A bar of n x 1 x 1 elements, L long, the end x = 0 clamped, linElas with nu = 0 (no lateral contraction: a one-dimensional wave,
speed c = sqrt(E / rho)), at rest until a traction along the bar is switched on at the free end at t = 0.  The front reaches the
mid-section at L / (2 c).  The script steps with the central-difference rule at the solver's stable step, samples the axial displacement
of the mid-section, and prints the time at which it first exceeds a small fraction of the static end deflection beside L / (2 sqrt(E / rho)),
and the steps per second.  (The discrete front is smeared over a few elements, so the printed time depends a little on the threshold;
it approaches the exact one as the mesh is refined.)

    python examples/solve_wave.py            # on the device
    python examples/solve_wave.py --oracle   # on the CPU oracle (portable step and mass operator)
    python examples/solve_wave.py --absorbing   # the far end lets the wave leave

``--absorbing``: the bar is not clamped; the traction acts at x = 0 and the end x = L carries the dashpots of a Lysmer-Kuhlemeyer
boundary (dynamics.absorbing_support).  The step travels down the bar and leaves: behind the front the whole bar moves at sigma / (rho c),
which the script prints beside the mean axial velocity after 1.2 transits (a free end would double it, a clamped end stop it).
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.dynamics import ExplicitDynamics, absorbing_support
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem

ap = argparse.ArgumentParser()
ap.add_argument("--oracle", action="store_true"); ap.add_argument("--elements", type=int, default=40); ap.add_argument("--degree", type=int, default=2)
ap.add_argument("--length", type=float, default=10.0); ap.add_argument("--density", type=float, default=1.0); ap.add_argument("--traction", type=float, default=1e-3)
ap.add_argument("--threshold", type=float, default=0.01, help="the mid-section 'moves' at this fraction of the static end deflection t L / E")
ap.add_argument("--graph", action="store_true", help="replay a recorded step (device only)")
ap.add_argument("--absorbing", action="store_true", help="no clamp: load at x = 0, an absorbing boundary at x = L")
a = ap.parse_args()
c = cd.Ceed(cd.CeedLib(os.path.join(ROOT, "oracle", "liboracle_ceed.so")), "/cpu/self/oracle") if a.oracle else cd.Ceed(cd.CeedLib(cd.PRODUCT_LIB), "/gpu/hip/mi355x")
E, L = 1.0, a.length
prob = SolidProblem(c, box_mesh(a.elements, 1, 1, hi=(L, 1.0, 1.0)), a.degree, "linElas", nu=0.0, E=E, bc_sides=[] if a.absorbing else [6], multigrid="none")
if a.absorbing:
    sol = ExplicitDynamics(prob, a.density, traction={6: (a.traction, 0.0, 0.0)}, support={5: absorbing_support(prob, a.density)})
else:
    sol = ExplicitDynamics(prob, a.density, traction={5: (a.traction, 0.0, 0.0)})
sol.set_initial()
X = prob.levels[prob.fine].dofmap.node_coords
mid = np.flatnonzero(np.abs(X[:, 0] - 0.5 * L) < 1e-9 * L)
assert mid.size, "no node row at the mid-section: take an even number of elements"
speed = np.sqrt(E / a.density)
nsteps = int(np.ceil(1.2 * L / speed / sol.dt))            # until the front has run the bar's length and a little more
arrival, every = None, 1
t0 = time.perf_counter()
if a.graph:
    sol.run(nsteps, graph=True)
else:
    for k in range(nsteps):
        sol.step()
        if arrival is None and k % every == 0:
            u = sol.x.to_numpy().reshape(-1, 3)[mid, 0]
            if np.abs(u).mean() > a.threshold * a.traction * L / E:
                arrival = sol.t
sol.ceed.synchronize()
sec = time.perf_counter() - t0
u_end = sol.x.to_numpy().reshape(-1, 3)[np.flatnonzero(np.abs(X[:, 0] - L) < 1e-9 * L), 0].mean()
print(f"resource {c.resource}; {prob.lsize()} dofs, dt = {sol.dt:.5f} (estimate of lambda_max {sol.emax_K:.4f}), {nsteps} steps")
if arrival is not None:
    print(f"the mid-section starts to move at t = {arrival:.4f}; L / (2 sqrt(E / rho)) = {0.5 * L / speed:.4f}")
if a.absorbing:
    print(f"mean axial velocity at t = {sol.t:.3f}: {sol.velocity().reshape(-1, 3)[:, 0].mean():.4e}; sigma / (rho c) = {a.traction / (a.density * speed):.4e}")
else:
    print(f"end deflection at t = {sol.t:.3f}: {u_end:.4e} (static t L / E = {a.traction * L / E:.4e}; the undamped response swings to twice that)")
print(f"{nsteps / sec:.1f} steps per second" + (" (replayed)" if a.graph else " (eager, the mid-section read on the host every step until it moves)"))
