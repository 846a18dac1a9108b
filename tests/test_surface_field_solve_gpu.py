"""Whole solves under surface loads that vary over a side set (NewtonPMG(pressure_field=, hydrostatic=)) on the device, small: the two
solves of tests/test_surface_field.py, against their results on the CPU oracle.

The solutions of the two backends are compared to 1e-6 of the solution's norm, the tolerance tests/test_surface_solve_gpu.py puts on
two solves of one problem that both converged to snes_rtol = 1e-10; the equilibrium check is measured against the solver's own
convergence, ten times the last Newton residual norm, as there."""
import numpy as np
import pytest

from ceedpetscsolid_amd.mesh import box_mesh, side_set_nodes
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG
from test_surface_field import E, NU, hydrostatic_block, reaction_balance, total_displacement

pytestmark = pytest.mark.gpu


def test_constant_pressure_field_solve_against_the_oracle(gpu, oracle):
    mesh = box_mesh(2, 2, 2)
    out = {}
    for name, ceed in (("oracle", oracle), ("gpu", gpu)):
        prob = SolidProblem(ceed, mesh, 2, "hyperFS", nu=NU, E=E, bc_sides=[3, 4, 5, 6])
        nn = prob.levels[prob.fine].dofmap.nnodes
        a = NewtonPMG(prob, pressure={2: 0.02 * E}, snes_rtol=1e-10)
        sa = a.solve(num_increments=1)
        b = NewtonPMG(prob, pressure_field={2: np.full(nn, 0.02 * E)}, snes_rtol=1e-10)
        sb = b.solve(num_increments=1)
        assert sa.converged and sb.converged
        ua, ub = total_displacement(a), total_displacement(b)
        assert (sb.newton_its, sb.ksp_its) == (sa.newton_its, sa.ksp_its), name
        assert np.linalg.norm(ub - ua) <= 1e-10 * np.linalg.norm(ua), name
        if name == "gpu":
            assert b.field_loads[0][1].kernel_name == "surface_field<P=3,Q=3>" and a.pressure_loads[0][0].kernel_name == "surface<P=3,Q=3>"
        out[name] = (ub, sb)
        a.destroy(); b.destroy(); prob.destroy()
    (uo, so), (ug, sg) = out["oracle"], out["gpu"]
    print(f"constant pressure field: oracle {so.newton_its} / {so.ksp_its}, device {sg.newton_its} / {sg.ksp_its}, "
          f"|U_gpu - U_oracle| / |U_oracle| = {np.linalg.norm(ug - uo) / np.linalg.norm(uo):.2e}")
    assert np.linalg.norm(ug - uo) <= 1e-6 * np.linalg.norm(uo)


def test_hydrostatic_block_against_the_oracle(gpu, oracle):
    mesh, prob_o, s_o, st_o = hydrostatic_block(oracle, "full")
    u_o = total_displacement(s_o)
    s_o.destroy(); prob_o.destroy()
    mesh, prob, full, st = hydrostatic_block(gpu, "full")
    assert st.converged and st_o.converged
    assert full.field_loads[0][1].kernel_name == "surface_field<P=3,Q=3>"
    carried, reaction, rnorm, G, u = reaction_balance(gpu, mesh, prob, full, st)
    print(f"hydrostatic block on the device: {st.newton_its} Newton / {st.ksp_its} Krylov (oracle {st_o.newton_its} / {st_o.ksp_its}), "
          f"|R| = {rnorm:.3e}, carried + G = {carried}, reactions - G = {reaction}, "
          f"|U_gpu - U_oracle| / |U_oracle| = {np.linalg.norm(u - u_o) / np.linalg.norm(u_o):.2e}")
    assert np.abs(carried).max() <= 10 * rnorm and np.abs(reaction).max() <= 10 * rnorm
    assert np.linalg.norm(u - u_o) <= 1e-6 * np.linalg.norm(u_o)
    assert u.reshape(-1, 3)[side_set_nodes(mesh, prob.levels[prob.fine].dofmap, [2]), 0].max() < 0
    _, prob0, none, st0 = hydrostatic_block(gpu, "none")
    assert st0.converged and st.newton_its <= st0.newton_its
    assert np.linalg.norm(total_displacement(none) - u) <= 1e-6 * np.linalg.norm(u)
    full.destroy(); none.destroy(); prob.destroy(); prob0.destroy()
