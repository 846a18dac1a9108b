"""Whole solves with spring and dashpot supports on the device: the cases of test_support.py (``_support_cases``) with the library's
kernels in the residual, in every level's operator and in every level's diagonal, under the same bounds as on the CPU -- the Winkler
bed against its closed form (100 x the Newton tolerance), the absorbing end under both time steppers (the CPU test's mesh and tol),
the explicit run replayed from a recording against the eager run bit for bit, and one Newmark step with the mass term fused into the
Jacobian apply against the two-pass step (test_fused_mass_solver_gpu.py's bound)."""
import numpy as np
import pytest

import _support_cases as sc
from ceedpetscsolid_amd.dynamics import NewmarkPMG
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem

pytestmark = pytest.mark.gpu

STEP_TOL = 1e-9              # x, v, a after a step: the bound of tests/test_fused_mass_solver_gpu.py


@pytest.mark.parametrize("degree", [2, 3])
def test_winkler_bed_closed_form(gpu, degree):
    prob = sc.winkler_problem(gpu, degree)
    s = sc.winkler_solver(prob)
    st = s.solve(num_increments=1)
    sc.check_winkler(prob, s, st, f"Winkler bed on the device, degree {degree}")
    sup = s.supports[0]
    assert sorted(sup["levels"]) == list(range(s.nlev)) and not any(sf.portable for sf in sup["levels"].values())
    assert sup["levels"][s.nlev - 1].kernel_name.startswith(f"contact<P={degree + 1},Q={degree + 1},")
    assert abs(sup["levels"][s.nlev - 1].area(sup["spring"]) - 1.0) <= 1e-13
    s.destroy(); prob.destroy()


def test_absorbing_end_under_both_steppers(gpu):
    prob = sc.absorbing_problem(gpu)
    runs = {}
    for graph in (False, True):
        ex, nsteps = sc.absorbing_explicit_recordable(prob, graph)
        assert ex.nsteps_done == nsteps and ex.t > sc.LENGTH / sc.SPEED + sc.T_RAMP
        assert not ex.supports[0]["levels"][ex.nlev - 1].portable
        runs[graph] = (ex.x.to_numpy().copy(), ex.vh.to_numpy().copy(), ex.R.to_numpy().copy(), ex.velocity().reshape(-1, 3), ex.dt)
        ex.destroy()
    for a, b in zip(runs[True][:3], runs[False][:3]):
        assert np.array_equal(a, b) and np.abs(a).max() > 0                   # the replayed steps give the eager bits
    sc.check_absorbed(runs[False][3], f"explicit on the device, {nsteps} steps of {runs[False][4]:.4f}")
    sc.check_absorbed(sc.absorbing_newmark(prob, runs[False][4], nsteps), "Newmark on the device at the same dt")
    prob.destroy()


def test_one_newmark_step_with_the_fused_mass_term(gpu):
    prob = SolidProblem(gpu, box_mesh(2, 2, 2), 2, "hyperFS", nu=0.3, E=1.0, bc_sides=[1])
    X = prob.levels[prob.fine].dofmap.node_coords
    v0 = 0.05 * np.sin(X @ np.array([[1.0, 2.0, 0.5], [0.3, 1.1, 2.0], [2.2, 0.4, 1.0]])).reshape(-1)
    out = {}
    for fused in (False, "auto"):
        nm = NewmarkPMG(prob, 1.2, 0.1, support={2: dict(kn=2.0, kt=1.0), 3: dict(cn=0.5, ct=0.3)}, coarse="cg", ksp_rtol=1e-10, snes_rtol=1e-10,
                        fused_mass=fused)
        assert nm._mass_in_op == (list(range(nm.nlev)) if fused else []) and all(nm._fused_op(lv) is None for lv in range(nm.nlev))
        nm.set_initial(v0=v0)
        assert nm.step().converged
        out[fused] = [v.to_numpy().copy() for v in (nm.xn, nm.vn, nm.an)]
        nm.destroy()
    for name, a, b in zip("xva", out["auto"], out[False]):
        err = np.abs(a - b).max() / np.abs(b).max()
        print(f"support + fused mass, one step: {name} fused vs two passes {err:.2e}")
        assert err <= STEP_TOL, (name, err)
    prob.destroy()
