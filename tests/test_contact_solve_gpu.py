"""Whole solves with contact (NewtonPMG(contact=, contact_tangent=)) on the device: the cases of test_contact_solve.py with the
library's kernels (csrc/kernels_contact.hip) in the residual, in every level's operator and in every level's diagonal.

The closed-form case, its exact solution and the bound 1e-7 delta at snes_rtol = 1e-10: ``_contact_solve``; the condition number of
K + C that the margin rests on is printed (and held below 1e3) by the CPU test.  The V-cycle runs in its four forms -- consumers fused
behind the apply or in two passes, eager or as a replayed graph (which needs the reduction-free Chebyshev coarse solve) -- and with the
default CG coarse solve; on the levels that carry the contact term the consumers are never fused, whatever the switch says."""
import numpy as np
import pytest

import _contact_solve as cs
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG

pytestmark = pytest.mark.gpu

FORMS = {"cg": dict(), "fused+eager": dict(coarse="chebyshev", fuse_epilogue=True, graph=False),
         "two_pass+eager": dict(coarse="chebyshev", fuse_epilogue=False, graph=False),
         "fused+graph": dict(coarse="chebyshev", fuse_epilogue=True, graph=True),
         "two_pass+graph": dict(coarse="chebyshev", fuse_epilogue=False, graph=True)}


@pytest.fixture(scope="module")
def prob(gpu):
    p = cs.closed_form_problem(gpu)
    yield p
    p.destroy()


@pytest.mark.parametrize("tangent", ["levels", "outer"])
@pytest.mark.parametrize("form", list(FORMS))
def test_closed_form(prob, form, tangent):
    s = cs.closed_form_solver(prob, contact_tangent=tangent, **FORMS[form])
    st = s.solve(num_increments=1)
    cs.check_closed_form(prob, s, st, f"closed form, {form}, contact_tangent={tangent}")
    fine = s.contacts[0]["levels"][s.nlev - 1]
    assert not fine.portable and fine.kernel_name.startswith("contact<P=3,Q=3,")
    assert sorted(s.contacts[0]["levels"]) == (list(range(s.nlev)) if tangent == "levels" else [s.nlev - 1])
    s.destroy()


@pytest.mark.parametrize("tangent", ["levels", "outer"])
def test_separated_is_the_rigid_translation_and_adds_exactly_zero(prob, tangent):
    s = cs.closed_form_solver(prob, delta=0.01, contact_tangent=tangent, fuse_epilogue=False)
    st = s.solve(num_increments=1)
    cs.check_separated(prob, s, st, f"separated, contact_tangent={tangent}")
    plain = cs.closed_form_solver(prob, delta=0.01, contact=False, fuse_epilogue=False)
    plain.solve(num_increments=1)
    assert np.array_equal(s.U.to_numpy(), plain.U.to_numpy()) and np.array_equal(s.R.to_numpy(), plain.R.to_numpy())
    s.destroy(); plain.destroy()


@pytest.mark.parametrize("tangent", ["levels", "outer"])
def test_sphere_indents_a_clamped_block(gpu, tangent):
    prob, s, st, f = cs.indentation(gpu, contact_tangent=tangent)
    assert st.converged and st.increments == 3                      # Newton converged in every increment
    for inc in (1, 2, 3):
        rn0 = st.initial_residuals[inc - 1]
        last = [h for h in st.history if h[0] == inc][-1]
        print(f"increment {inc}: |R|_0 = {rn0:.3e}, |R| = {last[4]:.3e} after {last[1]} Newton steps")
        assert last[4] <= s.snes_rtol * rn0                          # |R| is at tolerance
    mean = f["force"] / (f["eps"] * f["area"])
    print(f"indentation, contact_tangent={tangent}: {st.newton_its} Newton / {st.ksp_its} Krylov its; force along z {f['force_z']:.4e}, "
          f"active area {f['area']:.4e} ({f['active']:.2f} of the points), mean penetration F / (eps A_active) = {mean:.4e}, "
          f"largest -min_gap = {-f['min_gap']:.4e}")
    assert abs(f["min_gap"] - f["portable_min_gap"]) <= 1e-12        # the device's state against the portable form at the same u
    assert 0 < mean <= -f["min_gap"] * (1 + 1e-12) and -f["min_gap"] < f["depth"]
    s.destroy(); prob.destroy()


def test_no_contact_given_takes_no_new_path(gpu):
    prob = SolidProblem(gpu, box_mesh(2, 2, 2), 2, "hyperFS", nu=0.3, E=1.0, bc_sides=[1])
    force = 0.01 * np.random.default_rng(2).uniform(-1, 1, prob.lsize())
    a = NewtonPMG(prob, forcing=force)
    a.solve(num_increments=1)
    b = NewtonPMG(prob, forcing=force, contact=None, contact_tangent="outer")
    b.solve(num_increments=1)
    assert b.contacts == [] and b._contact_levels == set()
    assert b._fused_op(b.nlev - 1) is a._fused_op(a.nlev - 1) is not None
    assert np.array_equal(a.U.to_numpy(), b.U.to_numpy()) and np.abs(a.U.to_numpy()).max() > 0
    assert a.stats.history == b.stats.history
    a.destroy(); b.destroy(); prob.destroy()
