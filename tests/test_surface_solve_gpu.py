"""Whole solves under surface loads (NewtonPMG(traction=, pressure=, pressure_tangent=)) on the device, small.

The equilibrium checks are measured against the solver's own convergence: ten times the last Newton residual norm of SolveStats
(the l2 norm over the free dofs bounds the sum of one component over N <= 100 free nodes by sqrt(N) <= 10 times itself)."""
import math

import numpy as np
import pytest

from ceedpetscsolid_amd.mesh import box_mesh, hollow_cylinder_mesh, side_set_nodes
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG
from ceedpetscsolid_amd.surface import SurfaceLoad

pytestmark = pytest.mark.gpu

E, NU = 1.0, 0.3


def problem(gpu, mesh, bc):
    return SolidProblem(gpu, mesh, 2, "hyperFS", nu=NU, E=E, bc_sides=bc)


def total_displacement(s):
    """Free part of the solution plus the boundary values of the last increment."""
    return s.U.to_numpy() + s.bcv.to_numpy()


def internal_force(gpu, mesh, u):
    """F_int(u) on every node, from a second problem without Dirichlet sets."""
    q = SolidProblem(gpu, mesh, 2, "hyperFS", nu=NU, E=E, multigrid="none")
    X, Y = gpu.vector(u.size).set_array(u), gpu.vector(u.size)
    q.form_residual(X, Y)
    f = Y.to_numpy().copy()
    q.destroy()
    return f.reshape(-1, 3)


@pytest.fixture(scope="module")
def traction_solve(gpu):
    mesh = box_mesh(2, 2, 2)
    prob = problem(gpu, mesh, [1])
    s = NewtonPMG(prob, traction={2: (0.0, 0.01 * E, 0.02 * E)})
    st = s.solve(num_increments=1)
    return mesh, prob, s, st


def test_dead_traction_and_global_equilibrium(gpu, traction_solve):
    mesh, prob, s, st = traction_solve
    assert st.converged and st.newton_its >= 1
    rnorm = st.history[-1][4]
    t, A = np.array([0.0, 0.01 * E, 0.02 * E]), 1.0
    u = total_displacement(s)
    assert np.abs(u).max() > 1e-3                                        # the body did deform
    f = internal_force(gpu, mesh, u)
    clamped = np.zeros(f.shape[0], dtype=bool)
    clamped[side_set_nodes(mesh, prob.levels[prob.fine].dofmap, [1])] = True
    exact_sum = lambda a: np.array([math.fsum(a[:, c]) for c in range(3)])     # (no rounding of the check's own beside the solver's)
    carried, reaction = exact_sum(f[~clamped]), exact_sum(f[clamped])
    print(f"traction solve: {st.newton_its} Newton / {st.ksp_its} Krylov its, |R| = {rnorm:.3e}, "
          f"sum F_int off the clamp - t A = {carried - t * A}, reactions + t A = {reaction + t * A}")
    assert np.abs(carried - t * A).max() <= 10 * rnorm                   # the free nodes carry the whole load ...
    assert np.abs(reaction + t * A).max() <= 10 * rnorm                  # ... and the clamp's reactions balance it


def test_no_load_given_takes_no_new_path(gpu, traction_solve):
    mesh, prob, _, _ = traction_solve
    force = 0.01 * np.random.default_rng(2).uniform(-1, 1, prob.lsize())
    a = NewtonPMG(prob, forcing=force)
    a.solve(num_increments=1)
    b = NewtonPMG(prob, forcing=force, pressure=None, traction=None)
    b.solve(num_increments=1)
    assert b.pressure_loads == [] and b.surface_loads == []
    assert np.array_equal(a.U.to_numpy(), b.U.to_numpy()) and np.abs(a.U.to_numpy()).max() > 0


def test_clamped_plate_under_follower_pressure(gpu):
    mesh = box_mesh(2, 2, 2)
    prob = problem(gpu, mesh, [3, 4, 5, 6])                              # the rim of side 2 is clamped: the tangent is symmetric
    p = 0.02 * E
    full = NewtonPMG(prob, pressure={2: p}, pressure_tangent="full", snes_rtol=1e-10)
    st = full.solve(num_increments=1)
    assert st.converged
    rnorm = st.history[-1][4]
    lv = prob.levels[prob.fine]
    n = prob.lsize()
    u = total_displacement(full)
    X, Y = gpu.vector(n).set_array(u), gpu.vector(n)
    prob.form_residual(X, Y)                                             # constrained rows dropped
    ref = SurfaceLoad(gpu, mesh, lv.dofmap, [2], Q=prob.Q, mask=lv.mask, portable=True)
    r = Y.to_numpy() + 1.0 * p * ref.pressure_host(u)
    free = lv.mask == 0
    assert np.all(r[~free] == 0.0)
    print(f"pressure plate, full tangent: {st.newton_its} Newton / {st.ksp_its} Krylov its, |R| = {rnorm:.3e}, recomputed |R| = {np.linalg.norm(r[free]):.3e}")
    assert np.linalg.norm(r[free]) <= 10 * rnorm
    assert u.reshape(-1, 3)[side_set_nodes(mesh, lv.dofmap, [2]), 2].min() < -1e-4       # p > 0 pushes on the body: the top goes down
    none = NewtonPMG(prob, pressure={2: p}, pressure_tangent="none", snes_rtol=1e-10)
    st0 = none.solve(num_increments=1)
    assert st0.converged
    u0 = total_displacement(none)
    print(f"pressure plate, no tangent: {st0.newton_its} Newton / {st0.ksp_its} Krylov its, |U - U_full| / |U_full| = {np.linalg.norm(u0 - u) / np.linalg.norm(u):.2e}")
    assert np.linalg.norm(u0 - u) <= 1e-6 * np.linalg.norm(u)
    full.destroy(); none.destroy()
    prob.destroy()


def test_inflation_of_a_clamped_tube(gpu):
    mesh = hollow_cylinder_mesh(1, 8, 2, z0=-1, z1=1)
    prob = problem(gpu, mesh, [998, 999])
    s = NewtonPMG(prob, pressure={996: 0.02 * E})
    st = s.solve(num_increments=5)
    assert st.converged and st.increments == 5
    dm = prob.levels[prob.fine].dofmap
    wall = side_set_nodes(mesh, dm, [996])
    X = dm.node_coords[wall]
    mid = wall[np.abs(X[:, 2]) < 1e-12]
    assert mid.size == 16                                                # 8 vertices and 8 edge nodes at mid-height
    Xm = dm.node_coords[mid]
    rhat = Xm[:, :2] / np.linalg.norm(Xm[:, :2], axis=1)[:, None]
    ur = np.einsum("nc,nc->n", total_displacement(s).reshape(-1, 3)[mid, :2], rhat)
    print(f"inflation: {st.newton_its} Newton / {st.ksp_its} Krylov its, radial displacement at mid-height {ur.min():.4e} .. {ur.max():.4e}")
    assert np.all(ur > 0)
    s.destroy()
    prob.destroy()
