"""Modal analysis (modal.Eigenmodes) on the CPU oracle against the dense generalised eigenproblem of _modal_common.py: a clamped bar
(p = 2, linElas), a clamped bar through three multigrid levels with the aggregation coarse solve (p = 3, hyperFS), and a free bar
through the spectral shift of a Newmark solver; the prestressed modes after a static solve; a second seed; the refusals; and no new
path in an existing solve.  The oracle exports no block entry points, so the block operations here are the portable forms."""
import numpy as np
import pytest

import _modal_common as mc
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.dynamics import NewmarkPMG
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.modal import Eigenmodes
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG


@pytest.mark.parametrize("name", mc.CASES)
def test_modes_match_the_dense_pencil(oracle, name):
    prob, sol, nmodes, guard, nrigid = mc.make_case(oracle, name)
    res, calls = mc.run(sol, nmodes, guard)
    assert calls["gram"] > 0 and calls["combine"] > 0
    K, M, free, lam, Phi = mc.dense_reference(oracle, prob)
    mc.check_result(res, K, M, free, lam, Phi, nmodes, nrigid, name)
    assert np.allclose(res.frequencies, np.sqrt(np.maximum(res.eigenvalues, 0.0)))
    res2, _ = mc.run(sol, nmodes, guard, seed=7)          # a second seed: the same eigenvalues within the same bounds
    mc.check_result(res2, K, M, free, lam, Phi, nmodes, nrigid, name + " seed 7")
    mc.teardown(prob, sol)


def test_prestressed_modes(oracle):
    name = "clamped_p3_hyperfs_amg"
    prob, sol, nmodes, guard, _ = mc.make_case(oracle, name)
    lam0 = mc.run(sol, nmodes, guard)[0].eigenvalues
    mc.teardown(prob, sol)
    prob, sol, nmodes, guard, _ = mc.make_case(oracle, name, tip_fz=mc.TIP_FZ)
    st = sol.solve(num_increments=2)
    assert st.converged
    tip = np.abs(sol.U.to_numpy()).max()
    print(f"tip deflection {tip:.4f} of a bar 3 long")
    assert 0.01 * 3.0 <= tip <= 0.1 * 3.0                 # a few per cent of the length
    res, _ = mc.run(sol, nmodes, guard)
    K, M, free, lam, Phi = mc.dense_reference(oracle, prob)          # the dense pencil at THAT state
    mc.check_result(res, K, M, free, lam, Phi, nmodes, 0, name + " prestressed")
    print(f"lambda_1 unstressed {lam0[0]:.12e}, prestressed {res.eigenvalues[0]:.12e}")
    assert abs(res.eigenvalues[0] - lam0[0]) > 1e-6 * lam0[0]        # the control: the solver linearises about the current state
    mc.teardown(prob, sol)


def test_refusals(oracle):
    clamped = SolidProblem(oracle, box_mesh(2, 1, 1), 2, "linElas", nu=mc.NU, E=mc.E, bc_sides=[6])
    free = SolidProblem(oracle, box_mesh(2, 1, 1), 2, "linElas", nu=mc.NU, E=mc.E, bc_sides=[])
    sol = NewtonPMG(clamped)
    with pytest.raises(ValueError, match="no constrained dof and no shift"):
        Eigenmodes(NewtonPMG(free), mc.RHO, 4)
    with pytest.raises(ValueError, match="pressure loads"):
        Eigenmodes(NewtonPMG(clamped, pressure={5: 0.01}), mc.RHO, 4)
    with pytest.raises(ValueError, match=r"nmodes \+ guard = 17 > 16"):
        Eigenmodes(sol, mc.RHO, 15, guard=2)
    with pytest.raises(ValueError, match="differs from the Newmark solver's"):
        Eigenmodes(NewmarkPMG(free, mc.RHO, 1.0), 2.0 * mc.RHO, 4)
    with pytest.raises(ValueError, match="smoother='pbjacobi' is not provided"):
        Eigenmodes(NewmarkPMG(free, mc.RHO, 1.0, smoother="pbjacobi"), mc.RHO, 4)
    with pytest.raises(ValueError, match="density must be positive"):
        Eigenmodes(sol, 0.0, 4)

    class SeveralRanks:                                   # what a solver built with a halo over several ranks shows
        halos, pressure_loads = [object()], []
    with pytest.raises(ValueError, match="not provided with a halo"):
        Eigenmodes(SeveralRanks(), mc.RHO, 4)


def test_an_existing_solve_takes_no_new_path(oracle, monkeypatch):
    import ceedpetscsolid_amd.dynamics as dynamics
    import ceedpetscsolid_amd.solver as solver
    for mod in (solver, dynamics):
        src = open(mod.__file__).read()
        assert "modal" not in src and "Eigenmodes" not in src and "BlockVector" not in src

    def refuse(*a, **k):
        raise AssertionError("an existing solve built a BlockVector")
    monkeypatch.setattr(cd.BlockVector, "__init__", refuse)
    prob = SolidProblem(oracle, box_mesh(2, 1, 1), 2, "linElas", nu=mc.NU, E=mc.E, bc_sides=[6])
    sol = NewtonPMG(prob, forcing=np.tile([0.0, 0.0, -1e-4], prob.lsize() // 3))
    assert sol.solve(num_increments=1).converged
    dyn = NewmarkPMG(prob, mc.RHO, 0.5, forcing=np.tile([0.0, 0.0, -1e-4], prob.lsize() // 3))
    dyn.set_initial()
    assert dyn.step().converged
