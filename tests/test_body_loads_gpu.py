"""Body loads and a density field in the solvers on the device, against the closed forms and against the same runs on the CPU oracle:
the hanging bar and the follower spin of tests/test_body_loads.py (gravity=, spin=, the point-block multiply followed by the mass apply
with a field or a float in mask mode 2, the spin term of A_outer), and one Newmark step and 20 explicit steps with a per-element density.
The closed-form bounds are those of the oracle tests: 10 x the error measured there (profiles/mass_field.txt)."""
import numpy as np
import pytest

import test_body_loads as bl
from ceedpetscsolid_amd.dynamics import ExplicitDynamics, NewmarkPMG
from ceedpetscsolid_amd.mass import DensityField
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem

pytestmark = pytest.mark.gpu

RHO_E = np.array([1.0, 3.0, 2.0])
G = (0.3, 0.0, -1.0)
SPIN = dict(omega=0.8, axis=(0, 1, 0), origin=(0.1, 0.0, 0.0))


def test_hanging_bar_on_the_device(gpu, oracle):
    exact = bl.RHO * bl.G * bl.L * bl.L / (2 * bl.E)
    tips = {}
    for name, c in (("oracle", oracle), ("device", gpu)):
        prob = bl.bar(c, 2, 2)
        sol = bl.solve(prob, density=bl.RHO, gravity=(bl.G, 0.0, 0.0))
        tips[name] = bl.tip(prob, sol)
        if name == "device":
            assert sol.body_mass.kernel_name == "mass<3,3>"
        sol.destroy(); prob.destroy()
    err, diff = abs(tips["device"] - exact) / exact, abs(tips["device"] - tips["oracle"]) / exact
    print(f"hanging bar: device {tips['device']:.15e}  oracle {tips['oracle']:.15e}  closed form {exact:.15e}  error {err:.2e}  device - oracle {diff:.2e}")
    assert err <= 10 * bl.MEASURED["hanging"] and diff <= 10 * bl.MEASURED["hanging"]


def test_follower_spin_on_the_device(gpu, oracle):
    omega, exact = bl.follower_case()
    tips = {}
    for name, c in (("oracle", oracle), ("device", gpu)):
        prob = bl.bar(c, 4, 2)
        sol = bl.solve(prob, density=DensityField.per_element([bl.RHO, bl.RHO]), spin=dict(omega=omega, axis=(0, 1, 0)))
        assert sol.has_followers()
        tips[name] = bl.tip(prob, sol)
        if name == "device":
            assert sol.body_mass.kernel_name == "mass_field<5,5>"
        sol.destroy(); prob.destroy()
    err, diff = abs(tips["device"] - exact) / exact, abs(tips["device"] - tips["oracle"]) / exact
    print(f"follower spin: device {tips['device']:.15e}  oracle {tips['oracle']:.15e}  closed form {exact:.15e}  error {err:.2e}  device - oracle {diff:.2e}")
    assert err <= 10 * bl.MEASURED["follower_spin"] and diff <= 10 * bl.MEASURED["follower_spin"]


def dyn_bar(c):
    return SolidProblem(c, box_mesh(3, 1, 1, lo=(0.0, -0.2, -0.2), hi=(2.0, 0.2, 0.2)), 2, "linElas", nu=0.3, E=50.0, bc_sides=[6])


def test_one_newmark_step_with_a_per_element_density(gpu, oracle):
    out = {}
    for name, c in (("oracle", oracle), ("device", gpu)):
        prob = dyn_bar(c)
        v0 = 1e-2 * np.random.default_rng(1).uniform(-1, 1, prob.lsize())
        s = NewmarkPMG(prob, DensityField.per_element(RHO_E), 0.05, ksp_rtol=1e-14, snes_rtol=1e-13, gravity=G, spin=SPIN)
        s.set_initial(v0=v0)
        assert s.step().converged
        out[name] = (s.U.to_numpy(), s.vn.to_numpy(), s.an.to_numpy())
        if name == "device":
            assert s.mass_res.kernel_name == "mass_field<3,3>" and s.body_mass.kernel_name == "mass_field<3,3>"
        s.destroy(); prob.destroy()
    for what, d, o in zip("uva", out["device"], out["oracle"]):
        e = np.abs(d - o).max() / np.abs(o).max()
        print(f"Newmark step, {what}: device against oracle {e:.2e}")
        assert e <= 1e-10


def test_twenty_explicit_steps_with_a_per_element_density(gpu, oracle):
    out = {}
    for name, c in (("oracle", oracle), ("device", gpu)):
        prob = dyn_bar(c)
        v0 = 1e-2 * np.random.default_rng(3).uniform(-1, 1, prob.lsize())
        e = ExplicitDynamics(prob, DensityField.per_element(RHO_E), dt=2e-3, gravity=G, spin=SPIN)
        e.set_initial(v0=v0)
        e.run(20)
        out[name] = (e.x.to_numpy(), e.vh.to_numpy(), e.m.to_numpy())
        if name == "device":
            assert e.mass_lumped.kernel_name == "mass_field<3,3>"
        e.destroy(); prob.destroy()
    for what, d, o in zip(("x", "vh", "m"), out["device"], out["oracle"]):
        err = np.abs(d - o).max() / np.abs(o).max()
        print(f"20 explicit steps, {what}: device against oracle {err:.2e}")
        assert err <= 1e-10
