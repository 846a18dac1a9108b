"""Natural frequencies and mode shapes of a bar (modal.Eigenmodes): LOBPCG with the p-multigrid V-cycle as preconditioner.

A bar of 8 x 1 x 1 elements, 8 long, 1 wide and 0.6 thick (p = 2, E = 1, nu = 0.3, density 1.5), the end x = 0 clamped.  The first modes
are printed beside the Euler-Bernoulli bending frequencies of a cantilever, omega_k = (beta_k L)^2 sqrt(E I / (rho A L^4)), about both
axes of the cross-section (beta_k L = 1.8751, 4.6941, 7.8548); the beam formula leaves shear and rotary inertia out, so the solid's
frequencies lie a few per cent below it, more so for the higher modes and the thicker direction.  Torsional and axial modes have no
bending partner and are printed with a dash.  Nothing is asserted.

    python examples/solve_modes.py                # the clamped bar, on the device
    python examples/solve_modes.py --prestress    # hyperFS: the modes after a static solve under a transverse load, beside the unloaded ones
    python examples/solve_modes.py --free         # no clamped side: six rigid-body modes at zero through the shift of a Newmark solver
    python examples/solve_modes.py --oracle       # any of them on the CPU oracle (portable block operations)
    python examples/solve_modes.py --cylinder 10,110,90 --degree 4 --problem hyperFS --nmodes 6 --coarse amg --profile
                                                  # a hollow cylinder clamped at both ends, with the time split of an iteration
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.dynamics import NewmarkPMG
from ceedpetscsolid_amd.mesh import box_mesh, hollow_cylinder_mesh, load_mesh_npz
from ceedpetscsolid_amd.modal import Eigenmodes
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG

ap = argparse.ArgumentParser()
ap.add_argument("--oracle", action="store_true"); ap.add_argument("--prestress", action="store_true"); ap.add_argument("--free", action="store_true")
ap.add_argument("--nmodes", type=int, default=6); ap.add_argument("--guard", type=int, default=2); ap.add_argument("--tol", type=float, default=1e-8)
ap.add_argument("--degree", type=int, default=2); ap.add_argument("--problem", default=None); ap.add_argument("--density", type=float, default=1.5)
ap.add_argument("--shift", type=float, default=0.1, help="--free: a0 of the Newmark solver, the spectral shift")
ap.add_argument("--load", type=float, default=-1e-6, help="--prestress: transverse nodal force")
ap.add_argument("--cylinder", default=None, metavar="NR,NTH,NZ", help="a hollow cylinder clamped at both ends instead of the bar")
ap.add_argument("--mesh", default=None, help="a mesh file (tests/golden/mesh_*.npz), clamped on its side sets 998 and 999, instead of the bar")
ap.add_argument("--coarse", default="cg", choices=["cg", "chebyshev", "assembled", "amg"]); ap.add_argument("--graph", action="store_true")
ap.add_argument("--profile", action="store_true", help="synchronise behind every part of an iteration and print the time split")
ap.add_argument("--maxit", type=int, default=200)
a = ap.parse_args()
c = cd.Ceed(cd.CeedLib(os.path.join(ROOT, "oracle", "liboracle_ceed.so")), "/cpu/self/oracle") if a.oracle else cd.Ceed(cd.CeedLib(cd.PRODUCT_LIB), "/gpu/hip/mi355x")
E, NU, L, B, H = 1.0, 0.3, 8.0, 1.0, 0.6
problem = a.problem or ("hyperFS" if a.prestress else "linElas")
if a.cylinder or a.mesh:
    mesh = hollow_cylinder_mesh(*[int(v) for v in a.cylinder.split(",")]) if a.cylinder else load_mesh_npz(a.mesh)
    sides = [] if a.free else [s for s in (998, 999) if s in mesh.side_sets and len(mesh.side_sets[s])]
else:
    mesh, sides = box_mesh(8, 1, 1, hi=(L, B, H)), ([] if a.free else [6])
t0 = time.perf_counter()
prob = SolidProblem(c, mesh, a.degree, problem, nu=NU, E=E, bc_sides=sides)
n = prob.lsize()
kw = dict(coarse=a.coarse, graph=a.graph)
if a.free:
    sol = NewmarkPMG(prob, a.density, float(np.sqrt(4.0 / a.shift)), **kw)
else:
    sol = NewtonPMG(prob, forcing=np.tile([0.0, 0.0, a.load], n // 3) if a.prestress else None, **kw)
t_setup = time.perf_counter() - t0


def modes(label):
    em = Eigenmodes(sol, a.density, a.nmodes, guard=a.guard, tol=a.tol, maxit=a.maxit, profile=a.profile)
    res = em.solve()
    print(f"{label}: {res.iterations} iterations, {res.seconds:.3f} s, converged {res.converged}, block calls {em.block_calls}, "
          f"worst residual {res.residuals.max():.2e}")
    if a.profile:
        per = {k: v / max(res.iterations, 1) for k, v in res.timings.items()}
        print("   seconds per iteration (each part behind a synchronisation; set-up and the first Rayleigh-Ritz included in the totals): "
              + json.dumps({k: round(v, 6) for k, v in per.items()}) + f"   block share {100 * (per.get('gram', 0) + per.get('combine', 0)) / sum(per.values()):.1f} %")
    em.destroy()
    return res


print(f"resource {c.resource}; {mesh.nelem} elements, p = {a.degree}, {problem}, {prob.n_free()} free dofs, levels {prob.degrees}; set-up {t_setup:.2f} s")
if a.prestress:
    r0 = modes("unloaded")
    st = sol.solve(num_increments=4)
    print(f"static solve: converged {st.converged}, tip deflection {np.abs(sol.U.to_numpy()).max():.4f}")
    r1 = modes("prestressed")
    for i in range(a.nmodes):
        print(f"  mode {i + 1}: omega unloaded {r0.frequencies[i]:.10f}   prestressed {r1.frequencies[i]:.10f}   ratio {r1.frequencies[i] / r0.frequencies[i]:.6f}")
else:
    res = modes("free-free (shift %g)" % a.shift if a.free else "clamped")
    beam = []
    if not a.cylinder and not a.mesh and not a.free:
        for I, axis in ((B * H ** 3 / 12.0, "z"), (H * B ** 3 / 12.0, "y")):
            beam += [(bl ** 2 * np.sqrt(E * I / (a.density * B * H * L ** 4)), f"bending in {axis}, beta L = {bl}") for bl in (1.8751, 4.6941, 7.8548)]
    beam.sort()
    for i in range(a.nmodes):
        near = min(beam, key=lambda b: abs(b[0] - res.frequencies[i])) if beam else None
        tag = f"   Euler-Bernoulli {near[0]:.6f} ({near[1]}), ratio {res.frequencies[i] / near[0]:.4f}" if near and abs(near[0] / res.frequencies[i] - 1.0) < 0.15 else "   -"
        print(f"  mode {i + 1}: lambda {res.eigenvalues[i]: .12e}   omega {res.frequencies[i]:.10f}   rn {res.residuals[i]:.1e}{tag}")
