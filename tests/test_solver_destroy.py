"""Who owns the solver layer's memory: ``destroy()`` of body.LoadedBody and its subclasses (solver.NewtonPMG, dynamics.NewmarkPMG,
dynamics.ExplicitDynamics) releases every vector the object made, its surface loads, its recorded V-cycle, its assembled level and
its aggregation hierarchy, and nothing it was handed; and ExplicitDynamics, a LoadedBody, makes no vector of a preconditioner.

The problem is the jittered 2 x 2 x 2 two-level hyperFS one of tests/test_object_lifetime_gpu.py, on a Ceed of the test's own, whose
destruction is the last step of each case.  ``ceed.vector`` is wrapped between the solver's construction and its ``destroy()``: every
vector made in between -- by the solver, its assembled level, its hierarchy, its mass operators, its surface loads -- is collected."""
import numpy as np
import pytest

from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.dynamics import ExplicitDynamics, NewmarkPMG
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG

RHO = 1.5


def own_ceed(request, backend):
    """a Ceed of the test's own on either backend"""
    if backend == "gpu":
        return cd.Ceed(request.getfixturevalue("product_lib"), "/gpu/hip/mi355x")
    return cd.Ceed(request.getfixturevalue("oracle_lib"), "/cpu/self/oracle")


def problem(ceed, multigrid="uniform"):
    mesh = box_mesh(2, 2, 2)
    mesh.coords[:] += np.random.default_rng(5).uniform(-0.04, 0.04, mesh.coords.shape)
    p = SolidProblem(ceed, mesh, 2, "hyperFS", nu=0.3, E=1.0, bc_sides=[1], multigrid=multigrid)
    assert ceed.scalars.h          # (the Ceed's register file of scalars, made at first use, is the Ceed's: it exists before the solver)
    assert [lv.degree for lv in p.levels] == ([1, 2] if multigrid == "uniform" else [2])
    return p


class Collected:
    """``with Collected(ceed) as made``: the Vectors that ceed.vector returned inside the block (tensor vectors come through it too)"""

    def __init__(self, ceed):
        self.ceed, self.made = ceed, []

    def __enter__(self):
        inner = self.ceed.vector

        def vector(n):
            v = inner(n)
            self.made.append(v)
            return v
        self.ceed.vector = vector
        return self.made

    def __exit__(self, *exc):
        del self.ceed.vector


def force(prob):
    return np.tile([0.002, 0.0, 0.001], prob.lsize() // 3)


def newton_amg_with_surface_loads(prob):
    return NewtonPMG(prob, coarse="amg", traction={2: (0.0, 0.01, 0.0)}, pressure={3: 0.01})


def newton_after_a_recorded_solve(prob):
    sol = NewtonPMG(prob, coarse="chebyshev", graph=True, forcing=force(prob))
    recorded = []
    capture = sol.ceed.capture
    sol.ceed.capture = lambda fn: recorded.append(capture(fn)) or recorded[-1]
    try:
        assert sol.solve(1).converged
    finally:
        del sol.ceed.capture
    assert recorded and all(not g.h for g in recorded)          # a recording has existed, and solve() dropped it
    sol.setup_preconditioner()
    sol.record_preconditioner(sol.w[sol.nlev - 1]["b"], sol.kz)
    assert sol._pc_graph is not None                            # one that is alive when destroy() comes
    return sol


def newmark_after_two_steps(prob):
    sol = NewmarkPMG(prob, RHO, 0.4, forcing=force(prob), coarse="amg", pressure={3: 0.01})
    sol.set_initial()
    for _ in range(2):
        assert sol.step().converged
    return sol


def explicit_after_three_steps(prob):
    sol = ExplicitDynamics(prob, RHO, forcing=force(prob), traction={2: (0.0, 0.01, 0.0)})
    sol.set_initial()
    for _ in range(3):
        sol.step()
    return sol


CASES = {"newton-amg-surface-loads": newton_amg_with_surface_loads, "newton-recorded-vcycle": newton_after_a_recorded_solve,
         "newmark-two-steps": newmark_after_two_steps, "explicit-three-steps": explicit_after_three_steps}
# (the oracle records nothing: the recorded V-cycle exists on the device alone)
RUNS = [pytest.param(case, be, marks=[pytest.mark.gpu] if be == "gpu" else [], id=f"{case}-{be}")
        for case in CASES for be in ("oracle", "gpu") if not (case == "newton-recorded-vcycle" and be == "oracle")]


@pytest.mark.parametrize("case,backend", RUNS)
def test_destroy_releases_what_the_solver_made(request, case, backend):
    ceed, make = own_ceed(request, backend), CASES[case]
    prob = problem(ceed)
    with Collected(ceed) as made:
        sol = make(prob)
        asm, amg, loads = getattr(sol, "asm", None), getattr(sol, "amg", None), list(sol.surface_loads)
        masses = list(getattr(sol, "mass", [])) + [m for m in (getattr(sol, "mass_res", None), getattr(sol, "mass_lumped", None)) if m]
        assert (amg is not None) == (case in ("newton-amg-surface-loads", "newmark-two-steps"))
        assert bool(loads) == (case != "newton-recorded-vcycle")
        sol.destroy()
    print(f"{case}: {len(made)} vectors made, {len(sol._vectors)} still listed")
    assert len(made) > 5 and all(not v.h for v in made)
    assert getattr(sol, "_pc_graph", None) is None
    assert sol.surface_loads == [] and all(sl.handle is None and sl.X is None for sl in loads)
    if asm is not None:
        assert not asm.csr.h and not asm.op.h and not asm.coo.h
    if amg is not None:
        assert amg.levels == [] and amg.rc is None
    assert all(m.op is None for m in masses)
    with Collected(ceed) as again:
        sol.destroy()                                            # a second call does nothing
    assert again == []
    prob.destroy()                                               # what the solver was handed is still the caller's to destroy
    ceed.destroy()


# ---- the split: a LoadedBody holds no vector of a preconditioner (oracle only) --------------------------------------------------------
def explicit_vectors(oracle_lib, multigrid):
    c = cd.Ceed(oracle_lib, "/cpu/self/oracle")
    prob = problem(c, multigrid)
    sizes = [prob.lsize(lv) for lv in range(len(prob.levels))]
    with Collected(c) as made:
        sol = explicit_after_three_steps(prob)
        attrs = set(vars(sol))
        sol.destroy()
    prob.destroy(); c.destroy()
    return [v.n for v in made], sizes, attrs


def test_explicit_dynamics_makes_no_vector_of_a_preconditioner(oracle_lib):
    two, sizes2, attrs = explicit_vectors(oracle_lib, "uniform")
    one, sizes1, _ = explicit_vectors(oracle_lib, "none")
    assert len(sizes2) == 2 and sizes2[1] == sizes1[0] and sizes2[0] < sizes2[1]
    print(f"ExplicitDynamics made {len(two)} vectors on two levels, {len(one)} on one; sizes {sorted(set(two))}")
    assert len(two) == len(one) and sorted(two) == sorted(one)
    assert sizes2[0] not in two
    assert not attrs & {"w", "kz", "dU"}


def test_explicit_dynamics_refuses_a_preconditioner_keyword(oracle):
    prob = problem(oracle)
    with pytest.raises(TypeError, match="coarse"):
        ExplicitDynamics(prob, RHO, coarse="amg")
    prob.destroy()
