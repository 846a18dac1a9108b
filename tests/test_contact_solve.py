"""Whole solves with contact (NewtonPMG(contact=, contact_tangent=)) on the CPU oracle, where contact.py takes its portable form.

The closed-form case and its exact solution: ``_contact_solve``.  It must agree to 1e-7 delta with snes_rtol = 1e-10: Newton stops at
|R| <= 1e-10 |R|_0, and the error of the solution is at most cond(K + C) times that relative to the solution's size, so the margin over
the Newton tolerance is the condition number of K + C on this mesh.  The test prints it from the dense matrix and holds it below 1e3;
were it larger, snes_rtol would have to be tightened, not the bound.

The penetration check of the indentation: F = int eps <-g> dA0 over the A_active of the active points gives the MEAN penetration
F / (eps A_active), which the largest penetration -min_gap() cannot fall below; both are printed.  (The same figures appear in
profiles/contact.txt.)"""
import numpy as np
import pytest

import _contact_solve as cs
from ceedpetscsolid_amd.dynamics import ExplicitDynamics, NewmarkPMG
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG


@pytest.fixture(scope="module")
def prob(oracle):
    p = cs.closed_form_problem(oracle)
    yield p
    p.destroy()


def test_condition_number_of_the_closed_form_tangent(prob):
    s = cs.closed_form_solver(prob)
    st = s.solve(num_increments=1)
    cs.check_closed_form(prob, s, st, "closed form, levels")
    n, top = prob.lsize(), s.nlev - 1
    free = np.flatnonzero(prob.levels[prob.fine].mask == 0)
    X, Y = prob.ceed.vector(n), prob.ceed.vector(n)
    A = np.zeros((free.size, free.size))
    for k, i in enumerate(free):
        e = np.zeros(n); e[i] = 1.0
        X.set_array(e)
        s.A(top, X, Y)
        A[:, k] = Y.to_numpy()[free]
    assert np.abs(A - A.T).max() <= 1e-12 * np.abs(A).max()
    ev = np.linalg.eigvalsh(0.5 * (A + A.T))
    cond = ev[-1] / ev[0]
    print(f"K + C on the free dofs ({free.size}): eigenvalues {ev[0]:.3e} .. {ev[-1]:.3e}, condition number {cond:.1f}; "
          f"cond x snes_rtol = {cond * cs.SNES_RTOL:.1e} against the bound 1e-7")
    assert ev[0] > 0 and cond <= 1e3
    s.destroy()


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("tangent", ["levels", "outer"])
def test_closed_form(prob, tangent, fuse):
    s = cs.closed_form_solver(prob, contact_tangent=tangent, fuse_epilogue=fuse)
    st = s.solve(num_increments=1)
    cs.check_closed_form(prob, s, st, f"closed form, contact_tangent={tangent}, fuse_epilogue={fuse}")
    assert (s._fused_op(s.nlev - 1) is None) == (tangent == "levels" or not fuse)
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


def test_sphere_indents_a_clamped_block(oracle):
    prob, s, st, f = cs.indentation(oracle)
    assert st.converged and st.increments == 3                      # Newton converged in every increment
    for inc in (1, 2, 3):
        rn0 = st.initial_residuals[inc - 1]
        last = [h for h in st.history if h[0] == inc][-1]
        print(f"increment {inc}: |R|_0 = {rn0:.3e}, |R| = {last[4]:.3e} after {last[1]} Newton steps")
        assert last[4] <= s.snes_rtol * rn0                          # |R| is at tolerance
    mean = f["force"] / (f["eps"] * f["area"])
    print(f"indentation: {st.newton_its} Newton / {st.ksp_its} Krylov its; force along z {f['force_z']:.4e}, active area {f['area']:.4e} "
          f"({f['active']:.2f} of the points), mean penetration F / (eps A_active) = {mean:.4e}, largest -min_gap = {-f['min_gap']:.4e}")
    assert abs(f["min_gap"] - f["portable_min_gap"]) <= 1e-12
    assert 0 < mean <= -f["min_gap"] * (1 + 1e-12) and -f["min_gap"] < f["depth"]
    s.destroy(); prob.destroy()


def test_no_contact_given_takes_no_new_path(oracle):
    prob = SolidProblem(oracle, box_mesh(2, 2, 2), 2, "hyperFS", nu=0.3, E=1.0, bc_sides=[1])
    force = 0.01 * np.random.default_rng(2).uniform(-1, 1, prob.lsize())
    a = NewtonPMG(prob, forcing=force)
    a.solve(num_increments=1)
    b = NewtonPMG(prob, forcing=force, contact=None, contact_tangent="outer")
    b.solve(num_increments=1)
    assert b.contacts == [] and b._contact_levels == set() and b.min_gap() == float("inf") and b.active_fraction() == 0.0
    assert b._fused_op(b.nlev - 1) is a._fused_op(a.nlev - 1) is not None
    assert np.array_equal(a.U.to_numpy(), b.U.to_numpy()) and np.abs(a.U.to_numpy()).max() > 0
    assert a.stats.history == b.stats.history
    a.destroy(); b.destroy(); prob.destroy()


def test_solver_argument_checks(oracle):
    mesh = box_mesh(2, 2, 1)
    prob = SolidProblem(oracle, mesh, 2, "hyperFS", nu=0.3, E=1.0, bc_sides=[1], multigrid="none")
    plane = dict(plane=((0, 0, 1.1), (0, 0, -1.0)), penalty=5.0)
    with pytest.raises(ValueError, match="Dirichlet side set"):
        NewtonPMG(prob, contact={1: plane})
    with pytest.raises(ValueError, match="no such side set"):
        NewtonPMG(prob, contact={77: plane})
    with pytest.raises(ValueError, match="contact_tangent"):
        NewtonPMG(prob, contact={2: plane}, contact_tangent="inner")
    with pytest.raises(ValueError, match="pbjacobi"):
        NewtonPMG(prob, contact={2: plane}, smoother="pbjacobi")
    with pytest.raises(ValueError, match="penalty"):
        NewtonPMG(prob, contact={2: dict(plane=plane["plane"])})
    with pytest.raises(ValueError, match="penalty 0 is not positive"):
        NewtonPMG(prob, contact={2: dict(plane=plane["plane"], penalty=0.0)})
    with pytest.raises(ValueError, match="length 2, not 1"):
        NewtonPMG(prob, contact={2: dict(plane=((0, 0, 1.1), (0, 0, -2.0)), penalty=1.0)})
    with pytest.raises(ValueError, match="exactly one"):
        NewtonPMG(prob, contact={2: dict(penalty=1.0)})

    class TwoRanks:
        world = 2
    with pytest.raises(ValueError, match="several ranks"):
        NewtonPMG(prob, halo=TwoRanks(), contact={2: plane})
    for make in (lambda: NewmarkPMG(prob, 1.0, 0.1, contact={2: plane}), lambda: ExplicitDynamics(prob, 1.0, 0.1, contact={2: plane})):
        with pytest.raises(ValueError, match="static solves only"):
            make()
    s = NewtonPMG(prob, contact={2: plane})
    assert len(s.contacts) == 1 and s._contact_levels == {0} and s._fused_op(0) is None
    s.destroy()
    assert s.contacts == []
    prob.destroy()
