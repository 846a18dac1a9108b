"""dynamics.NewmarkPMG(fused_mass=True) on the device: the effective tangent K + a0 rho M as ONE apply of the level's Jacobian operator
(CeedXOperatorSetMassTerm), beside the two-pass form, against the dense references of tests/_newmark_dense.py, in the four V-cycle
forms, and what it leaves behind."""
import numpy as np
import pytest

import _newmark_dense as nd
from _mass_common import E, NU, RHO, dense_from_applies, dense_K_M, hyperfs_run, lowest_mode
from ceedpetscsolid_amd.dynamics import NewmarkPMG
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem

pytestmark = pytest.mark.gpu

STEP_TOL = 1e-9              # x, v, a after a step: the bound of tests/test_dynamics_dense_gpu.py


def jacobian_names(prob):
    return [lv.opJacob.kernel_name for lv in prob.levels]


def test_fused_steps_equal_two_pass_steps(gpu):
    """Three steps of _mass_common.hyperfs_run's case at p = 2: the same Newton and Krylov counts, x, v, a within 1e-9."""
    runs = {}
    for fused in (False, True):
        sol, prob, out, stats = hyperfs_run(gpu, box_mesh(2, 2, 2), 3, coarse="amg", fused_mass=fused)
        assert sol._mass_in_op == ([1] if fused else [])          # level 0 is assembled: its matrix holds the term
        names = jacobian_names(prob)
        assert ("+mass" in names[1]) == fused and "+mass" not in names[0], names
        runs[fused] = ([(st.newton_its, st.ksp_its) for st in stats], [v.to_numpy() for v in (sol.xn, sol.vn, sol.an)], out)
        sol.destroy(); prob.destroy()
    assert runs[True][0] == runs[False][0], (runs[True][0], runs[False][0])
    for name, a, b in zip("xva", runs[True][1], runs[False][1]):
        err = nd.relmax(a, b)
        print(f"FUSED MASS hyperFS p = 2, three steps: {name} fused vs two passes {err:.2e}")
        assert err <= STEP_TOL, (name, err)


def eigenvector_steps(ceed, nsteps, fused_mass):
    """_mass_common.eigenvector_run's case stepped here, so that every step's counts and the state reach the caller: a 2 x 1 x 1 box,
    p = 2, linElas, the end x = 0 clamped, released from 0.01 x its lowest mode, 20 steps per period.  Returns ([(newton_its, ksp_its)],
    [(x, v, a) per step], worst |u_n - phi cos(n theta)| / |phi|, the run's bound 10 nsteps cond(K + a0 M) 1e-10)."""
    prob = SolidProblem(ceed, box_mesh(2, 1, 1), 2, "linElas", nu=NU, E=E, bc_sides=[6])
    K, M, free = dense_K_M(ceed, prob, RHO)
    w, phi = lowest_mode(K, M)
    phi *= 0.01 / np.abs(phi).max()
    dt = 2.0 * np.pi / w / 20
    theta = 2.0 * np.arctan(0.5 * w * dt)
    sol = NewmarkPMG(prob, RHO, dt, ksp_rtol=1e-10, snes_rtol=1e-10, fused_mass=fused_mass)
    assert sol._mass_in_op == (list(range(sol.nlev)) if fused_mass else [])
    bound = 10.0 * nsteps * np.linalg.cond(K + sol.a0 * M) * 1e-10
    u0 = np.zeros(prob.lsize())
    u0[free] = phi
    sol.set_initial(u0=u0)
    counts, states, worst = [], [], 0.0
    for n in range(1, nsteps + 1):
        st = sol.step()
        assert st.converged, (n, st.history)
        counts.append((st.newton_its, st.ksp_its))
        states.append(tuple(v.to_numpy() for v in (sol.xn, sol.vn, sol.an)))
        worst = max(worst, np.linalg.norm(sol.U.to_numpy()[free] - phi * np.cos(n * theta)) / np.linalg.norm(phi))
    names = jacobian_names(prob)
    sol.destroy(); prob.destroy()
    return counts, states, worst, bound, names


def test_eigenvector_run_with_the_fused_tangent(gpu):
    """The eigenvector run, fused beside two passes: the same Newton and Krylov counts in every step, x, v, a of every step within 1e-9;
    and the fused run against the exact discrete solution of the average-acceleration rule inside the run's own bound."""
    nsteps = 40
    two = eigenvector_steps(gpu, nsteps, False)
    one = eigenvector_steps(gpu, nsteps, True)
    assert all("+mass" in nm for nm in one[4]) and not any("+mass" in nm for nm in two[4]), (one[4], two[4])
    assert one[0] == two[0], (one[0], two[0])
    worst = {"x": 0.0, "v": 0.0, "a": 0.0}
    for sa, sb in zip(one[1], two[1]):
        for name, a, b in zip("xva", sa, sb):
            worst[name] = max(worst[name], nd.relmax(a, b))
    print(f"FUSED MASS eigenvector run, {nsteps} steps: Newton / Krylov counts {sorted(set(one[0]))} both ways; worst over the steps, fused vs two "
          f"passes: x {worst['x']:.2e} v {worst['v']:.2e} a {worst['a']:.2e}; |u - exact| / |phi| fused {one[2]:.2e} two passes {two[2]:.2e} bound {one[3]:.2e}")
    for name, err in worst.items():
        assert err <= STEP_TOL, (name, err)
    assert one[2] <= one[3]


VARIANTS = {       # name -> (SolidProblem keywords, solver keywords, (P, Q) per level, levels whose operator carries the term)
    "fine-amg": (dict(coarse_quadrature="fine"), dict(coarse="amg"), [(2, 4), (3, 4), (4, 4)], [1, 2]),
    "fine-assembled": (dict(coarse_quadrature="fine"), dict(coarse="assembled"), [(2, 4), (3, 4), (4, 4)], [1, 2]),
    "own-cg": (dict(coarse_quadrature="own"), dict(coarse="cg"), [(2, 2), (3, 3), (4, 4)], [0, 1, 2]),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_level_against_the_dense_effective_operator(gpu, oracle, variant):
    """NewmarkPMG(fused_mass=True).A(lv) column by column against K_lv + a0 rho M_lv of the oracle's problem linearised at the same
    deformed state (hyperFS, p = 3), within 1e-10; on an assembled level the matrix carries M exactly once."""
    prob_kw, sol_kw, pq, fused_levels = VARIANTS[variant]
    prob, sol = nd.hyperfs_solver(gpu, 3, 2, prob_kw, fused_mass=True, **sol_kw)
    assert [(lv.degree + 1, lv.Q) for lv in prob.levels] == pq and sol._mass_in_op == fused_levels
    sol.residual(sol.U, sol.R)
    sol.setup_preconditioner()
    U = sol.U.to_numpy()
    assert np.abs(U).max() > 0.1
    rprob, rsol = nd.hyperfs_solver(oracle, 3, 2, prob_kw, **sol_kw)
    rsol._set(rsol.U, U)
    rsol.residual(rsol.U, rsol.R)
    coef = 1.0 / (0.25 * nd.DT_FS * nd.DT_FS) * RHO
    assert sol.a0 * sol.density == coef
    for lv in range(sol.nlev):
        n = prob.lsize(lv)
        mask = prob.levels[lv].mask != 0
        assembled = lv == 0 and sol.asm is not None
        ref, Mterm = nd.level_reference(rprob, lv, coef, assembled)
        A = dense_from_applies(gpu, n, lambda x, y: sol.A(lv, x, y), range(n))
        name = prob.levels[lv].opJacob.kernel_name
        assert ("+mass" in name) == (lv in fused_levels), (lv, name)
        err = nd.relmax(A, ref)
        share = float(np.abs(Mterm).max() / np.abs(ref).max())
        print(f"FUSED MASS dense {variant} level {lv} (P, Q) = {pq[lv]}: |A - ref| / max|ref| = {err:.2e}, max|a0 rho M| / max|ref| = {share:.2f}; {name}")
        assert err <= nd.TOL and share >= 0.1, (lv, err, share)
        if not assembled:
            assert not A[mask].any() and not A[:, mask].any()
        # the smoother's diagonal keeps its form: diag K + a0 rho diag M
        D = gpu.vector(n).set_value(3.0)
        sol._get_diag(lv, D)
        assert nd.relmax(D.to_numpy(), np.where(mask, 0.0, np.diag(ref))) <= nd.TOL
        D.destroy()
    nd.teardown(rsol, rprob)
    nd.teardown(sol, prob)


def test_the_four_vcycle_forms_give_the_same_bits(gpu):
    """fuse_epilogue x graph with the fused tangent: the smoother step and the residual in the apply's epilogue (K + a0 rho M there too)
    and the replayed recording give the bits of apply-then-step, eager."""
    out = {}
    for fuse in (False, True):
        for graph in (False, True):
            prob, sol = nd.hyperfs_solver(gpu, 3, 1, None, coarse="amg", fused_mass=True, fuse_epilogue=fuse, graph=graph)
            assert (sol._fused_op(2) is not None) == fuse and sol._fused_op(0) is None
            sol.residual(sol.U, sol.R)
            sol.setup_preconditioner()
            top = sol.nlev - 1
            n = prob.lsize()
            r = np.random.default_rng(9).uniform(-1, 1, n) * (prob.levels[top].mask == 0)
            Rv, Zv = gpu.vector(n).set_array(r), gpu.vector(n)
            sol.vcycle(top, Rv, Zv)                            # eager once (first-use set-up), then the form under test
            if graph:
                g = gpu.capture(lambda: sol.vcycle(top, Rv, Zv))
                Zv.set_value(-5.0); Zv.device_pointer()
                g.launch()
                z = Zv.to_numpy()
                g.destroy()
            else:
                sol.vcycle(top, Rv, Zv)
                z = Zv.to_numpy()
            assert all("+mass" in nm for nm in jacobian_names(prob)[1:])
            out[(fuse, graph)] = z
            nd.teardown(sol, prob)
    base = out[(False, False)]
    assert np.abs(base).max() > 0
    for key, z in out.items():
        assert np.array_equal(z, base), (key, np.abs(z - base).max())


def test_destroy_leaves_the_operators_as_found_and_the_default_never_fuses(gpu):
    prob, sol = nd.hyperfs_solver(gpu, 2, 1, None, coarse="cg")                     # the default: fused_mass=False
    assert sol.fused_mass is False and sol._mass_in_op == [] and all(sol._fused_op(lv) is None for lv in range(sol.nlev))
    assert not any("+mass" in nm for nm in jacobian_names(prob))
    sol.destroy()
    n = prob.lsize()
    X, Y = gpu.vector(n).set_array(np.random.default_rng(2).uniform(-1, 1, n)), gpu.vector(n)
    prob.apply_jacobian(prob.fine, X, Y)
    before = Y.to_numpy()
    sol = NewmarkPMG(prob, RHO, nd.DT_FS, coarse="cg", fused_mass=True)
    assert sol._mass_in_op == list(range(sol.nlev))
    for lv in range(sol.nlev):
        x = gpu.vector(prob.lsize(lv)).set_value(1.0)
        y = gpu.vector(prob.lsize(lv))
        sol.A(lv, x, y)
    assert all("+mass" in nm for nm in jacobian_names(prob))
    sol.destroy()
    prob.apply_jacobian(prob.fine, X, Y)
    assert np.array_equal(Y.to_numpy(), before)
    for lv in range(len(prob.levels) - 1):
        x = gpu.vector(prob.lsize(lv)).set_value(1.0)
        prob.apply_jacobian(lv, x, gpu.vector(prob.lsize(lv)))
    assert not any("+mass" in nm for nm in jacobian_names(prob)), jacobian_names(prob)
    # "auto" sets what True sets here; a refusal of True leaves nothing set (the library has every kernel of this ladder, so the
    # refusal itself is the CPU oracle's test)
    sol = NewmarkPMG(prob, RHO, nd.DT_FS, coarse="assembled", fused_mass="auto")
    assert sol._mass_in_op == list(range(1, sol.nlev))
    sol.destroy()
    with pytest.raises(ValueError, match="fused_mass must be"):
        NewmarkPMG(prob, RHO, nd.DT_FS, fused_mass="yes")
    prob.destroy()
