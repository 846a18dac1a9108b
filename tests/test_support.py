"""Spring and dashpot supports (support.py, body.LoadedBody(support=), the solvers), the portable NumPy form on the CPU oracle against
facts: the state on a planar and on a curved side set, the operator's symmetry, semi-definiteness and diagonal, the coarse p-level's
tangent as the Galerkin product of the fine one, what the force and the tangent read on a rim shared with a clamped set, a Winkler bed
against its closed form, Newmark's energy identity, an absorbing end under both time steppers, the explicit stepper's stable step against
the spectral radius of the dense one-step matrix, and the refusals.  The shared solves: ``_support_cases``.

The symmetric, diagonal, Galerkin and mask identities hold to rounding of sums of a few hundred O(1) terms: 1e-12 relative (contact's
bound, the same sums).  The planar state is a product of three numbers per entry: 1e-14 relative."""
import numpy as np
import pytest

import _support_cases as sc
from ceedpetscsolid_amd.dynamics import ExplicitDynamics, NewmarkPMG, absorbing_support
from ceedpetscsolid_amd.body import LoadedBody
from ceedpetscsolid_amd.mesh import box_mesh, build_dofmap, dirichlet_mask, gll_nodes, hollow_cylinder_mesh, side_set_nodes
from ceedpetscsolid_amd.portable import lagrange_tables
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG
from ceedpetscsolid_amd.support import NSTATE, SupportSurface

KN, KT = 3.0, 0.75
SIX = [1, 2, 3, 4, 5, 6]


def full(state):
    """K_q as [face][point][3][3] from a state [face][7][Q^2]."""
    K = np.empty(state.shape[:1] + state.shape[2:] + (3, 3))
    for k, (i, j) in enumerate(((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))):
        K[..., i, j] = K[..., j, i] = state[:, k]
    return K


def test_state_on_a_planar_face(oracle):
    mesh = box_mesh(2, 3, 1, hi=(1.5, 2.0, 1.0))
    for P, Q in ((2, 2), (3, 4), (5, 6)):
        dm = build_dofmap(mesh, P - 1)
        sp = SupportSurface(oracle, mesh, dm, [1], Q, portable=True)
        state = sp.state_host(KN, KT)
        assert state.shape == (6, NSTATE, Q * Q)
        w = lagrange_tables(P, Q)[2]
        wJ = np.broadcast_to((np.outer(w, w) * 0.75 * (2.0 / 3) / 4).reshape(-1), (6, Q * Q))     # J = (hx / 2) (hy / 2) on [-1, 1]^2
        assert np.abs(state[:, 6] - wJ).max() <= 1e-14 * wJ.max()
        want = wJ[..., None, None] * np.diag([KT, KT, KN])
        err = np.abs(full(state) - want).max() / np.abs(want).max()
        print(f"P={P} Q={Q}: planar K_q against wJ diag(kt, kt, kn): {err:.2e}; area {sp.area(state)!r}")
        assert err <= 1e-14
        assert abs(sp.area(state) - 3.0) <= 1e-13 * 3.0
        S = sp.new_state()
        sp.form_state(KN, KT, S)
        assert np.array_equal(S.to_numpy()[:state.size], state.reshape(-1)) and sp.area(S) == sp.area(state)
        S.destroy()


def test_state_on_a_curved_wall(oracle):
    mesh = hollow_cylinder_mesh(1, 6, 2)
    P, Q = 4, 5
    dm = build_dofmap(mesh, P - 1)
    sp = SupportSurface(oracle, mesh, dm, [996], Q, portable=True)
    state = sp.state_host(KN, KT)
    K = full(state)
    assert np.array_equal(K, np.swapaxes(K, -1, -2))
    # the geometry at the points, formed here from the tables alone
    B, D, w = lagrange_tables(P, Q)
    Xf = sp.Xh.reshape(-1, 3)[sp.faces].reshape(sp.nface, P, P, 3)
    Xa, Xb, Xq = (np.einsum("bj,ai,fjic->fbac", L, R, Xf).reshape(sp.nface, Q * Q, 3) for L, R in ((B, D), (D, B), (B, B)))
    m = np.cross(Xa, Xb)
    J = np.linalg.norm(m, axis=-1)
    n, wJ = m / J[..., None], J * np.outer(w, w).reshape(-1)
    assert np.abs(state[:, 6] - wJ).max() <= 1e-13 * wJ.max()
    ev = np.linalg.eigvalsh(K)
    want = wJ[..., None] * np.sort([KT, KT, KN])
    assert np.abs(ev - want).max() <= 1e-12 * want.max()
    assert np.abs(np.einsum("fqcd,fqd->fqc", K, n) - (wJ * KN)[..., None] * n).max() <= 1e-12 * want.max()     # n is the eigenvector of kn
    # the interpolated wall is a prism of six planar facets (trilinear elements): a facet's normal is the radial direction of its centre
    radial = Xq.mean(axis=1, keepdims=True) * [1.0, 1.0, 0.0]
    radial /= np.linalg.norm(radial, axis=-1)[..., None]
    cosine = np.abs(np.einsum("fqc,fqc->fq", n, np.broadcast_to(radial, n.shape)))
    print(f"curved wall: |n . e_r(facet centre)| >= {cosine.min()!r}")
    assert cosine.min() >= 1.0 - 1e-12


def test_degenerate_point_gets_no_normal(oracle):
    mesh = box_mesh(1, 1, 1)
    mesh.coords[mesh.coords[:, 2] == 0.0, :2] = 0.5                        # side 1 collapsed to a point: J = 0 everywhere on it
    dm = build_dofmap(mesh, 1)
    sp = SupportSurface(oracle, mesh, dm, [1], 2, portable=True)
    assert np.all(sp.state_host(KN, KT) == 0.0)


def surfaces(oracle, P, Q, mask=None, shape="six sides"):
    mesh, sides = (box_mesh(2, 2, 1), SIX) if shape == "six sides" else (hollow_cylinder_mesh(1, 5, 2), [996])
    dm = build_dofmap(mesh, P - 1)
    return SupportSurface(oracle, mesh, dm, sides, Q, mask=mask, portable=True), mesh, dm


@pytest.mark.parametrize("shape,P,Q", [("six sides", 3, 4), ("curved wall", 3, 3)])
def test_operator_is_symmetric_positive_semidefinite_with_its_diagonal(oracle, shape, P, Q):
    sp, _, dm = surfaces(oracle, P, Q, shape=shape)
    state = sp.state_host(KN, KT)
    rng = np.random.default_rng(5)
    for _ in range(3):
        v, w = rng.uniform(-1, 1, dm.lsize), rng.uniform(-1, 1, dm.lsize)
        kv, kw = sp.tangent_host(state, v), sp.tangent_host(state, w)
        d, bound = abs(w @ kv - v @ kw), np.linalg.norm(w) * np.linalg.norm(kv) + np.linalg.norm(v) * np.linalg.norm(kw)
        assert bound > 0 and d <= 1e-12 * bound
        assert v @ kv > 0 and abs(sp.energy_host(state, v) - 0.5 * v @ kv) <= 1e-12 * (v @ kv)
        assert np.array_equal(kv, sp.force_host(state, v))                  # no mask: the force is the tangent
    dense = np.stack([sp.tangent_host(state, e) for e in np.eye(dm.lsize)], axis=1)
    assert np.abs(dense - dense.T).max() <= 1e-12 * np.abs(dense).max()
    assert np.linalg.eigvalsh(0.5 * (dense + dense.T)).min() >= -1e-12 * np.abs(dense).max()
    diag = sp.diagonal_host(state)
    err = np.abs(diag - np.diag(dense)).max() / np.abs(diag).max()
    print(f"{shape} P={P} Q={Q}: diagonal against the dense matrix's: {err:.2e}")
    assert err <= 1e-12
    on = np.zeros(dm.nnodes, dtype=bool); on[np.unique(sp.faces)] = True
    assert np.all(diag.reshape(-1, 3)[~on] == 0.0) and np.all(diag.reshape(-1, 3)[on] > 0.0)


def interpolation(Pc, Pf):
    """I [Pf][Pc]: the Pc Lagrange functions on the Gauss-Lobatto points at the Pf Gauss-Lobatto points."""
    xc, xf = gll_nodes(Pc), gll_nodes(Pf)
    I = np.ones((Pf, Pc))
    for i in range(Pc):
        for k in range(Pc):
            if k != i:
                I[:, i] *= (xf - xc[k]) / (xc[i] - xc[k])
    return I


@pytest.mark.parametrize("Pc,Pf,Q", [(2, 3, 3), (2, 5, 6), (3, 5, 5)])
def test_coarse_tangent_is_the_galerkin_product(oracle, Pc, Pf, Q):
    fine, mesh, dmf = surfaces(oracle, Pf, Q)
    state = fine.state_host(KN, KT)
    dmc = build_dofmap(mesh, Pc - 1)
    coarse = SupportSurface(oracle, mesh, dmc, SIX, Q, portable=True)
    assert coarse.nface == fine.nface
    I2 = np.kron(interpolation(Pc, Pf), interpolation(Pc, Pf))
    Pmat = np.zeros((dmf.nnodes, dmc.nnodes))
    for ff, fc in zip(fine.faces, coarse.faces):
        Pmat[ff] = 0.0
        Pmat[ff[:, None], fc[None, :]] = I2
    v = np.random.default_rng(Pc + Pf).uniform(-1, 1, dmc.lsize)
    vf = (Pmat @ v.reshape(-1, 3)).reshape(-1)
    want = (Pmat.T @ fine.tangent_host(state, vf).reshape(-1, 3)).reshape(-1)
    got = coarse.tangent_host(state, v)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"Pc={Pc} Pf={Pf} Q={Q}: coarse tangent against I^T K I, relative max-norm error {err:.2e}")
    assert err <= 1e-12
    dc = coarse.diagonal_host(state)
    i = 3 * int(coarse.faces[0, 0]) + 2
    e = np.zeros(dmc.lsize); e[i] = 1.0
    assert abs(coarse.tangent_host(state, e)[i] - dc[i]) <= 1e-12 * np.abs(dc).max()


def test_force_reads_the_rim_and_the_tangent_does_not(oracle):
    mesh = box_mesh(2, 2, 1)
    dm = build_dofmap(mesh, 2)
    mask = dirichlet_mask(dm, side_set_nodes(mesh, dm, [6])).copy()           # clamp x-: its edge with side 1 is the rim
    m = mask != 0
    sp = SupportSurface(oracle, mesh, dm, [1], 4, mask=mask, portable=True)
    free = SupportSurface(oracle, mesh, dm, [1], 4, portable=True)
    state = sp.state_host(KN, KT)
    assert np.array_equal(state, free.state_host(KN, KT))                      # the state knows no mask
    x = np.random.default_rng(3).uniform(-1, 1, dm.lsize)
    x0 = np.where(m, 0.0, x)
    f, t = sp.force_host(state, x), sp.tangent_host(state, x)
    assert np.all(f[m] == 0.0) and np.all(t[m] == 0.0)                         # neither writes a masked row
    assert np.array_equal(f[~m], free.force_host(state, x)[~m])                # the force reads the rim's values ...
    assert np.array_equal(t[~m], free.force_host(state, x0)[~m])               # ... the tangent reads them as zero
    assert np.abs(f - t).max() > 1e-3 * np.abs(f).max()
    junk = x.copy(); junk[m] = 1e30
    assert np.array_equal(sp.tangent_host(state, junk), t)
    # on vectors of the Ceed: y += scale ..., rows off the surface and masked rows keep their bits
    n = dm.lsize
    y0 = np.random.default_rng(4).uniform(-1, 1, n)
    X, S = oracle.vector(n).set_array(x), sp.new_state()
    sp.form_state(KN, KT, S)
    on = np.zeros(dm.nnodes, dtype=bool); on[side_set_nodes(mesh, dm, [1])] = True
    for call, want in ((lambda y: sp.force_add(0.5, S, X, y), 0.5 * f), (lambda y: sp.tangent_add(0.5, S, X, y), 0.5 * t),
                       (lambda y: sp.diagonal_add(0.5, S, y), 0.5 * sp.diagonal_host(state))):
        Y = oracle.vector(n).set_array(y0)
        call(Y)
        y = Y.to_numpy()
        touched = y != y0
        assert touched.any() and not touched[m].any() and not touched[~np.repeat(on, 3)].any()
        assert np.allclose(y, y0 + want, rtol=0, atol=1e-15)
        Y.destroy()


@pytest.mark.parametrize("degree", [2, 3])
def test_winkler_bed_closed_form(oracle, degree):
    """Measured on the oracle: 1.0e-13 (degree 2) and 2.3e-17 (degree 3) beside the bound 1.5e-10."""
    prob = sc.winkler_problem(oracle, degree)
    s = sc.winkler_solver(prob)
    assert s._fused_op(s.nlev - 1) is None and len(s.supports) == 1 and set(s.supports[0]["levels"]) == {s.nlev - 1}
    st = s.solve(num_increments=1)
    sc.check_winkler(prob, s, st, f"Winkler bed, degree {degree}")
    assert set(s.supports[0]["levels"]) == set(range(s.nlev))                  # every level's operator carried the term
    s.destroy()
    assert s.supports == []
    for coarse in ("amg", "assembled"):
        with pytest.raises(ValueError, match="no Dirichlet dof"):
            sc.winkler_solver(prob, coarse=coarse)
    prob.destroy()


def test_newmark_energy_identity(oracle):
    """E_{n+1} - E_n = -dt vbar . C_d vbar with the average-acceleration rule on a linear body.  Measured: the largest defect over 10
    steps is 2e-13 of E_0 (bound 100 x snes_rtol = 1e-8)."""
    rtol = 1e-10
    prob = SolidProblem(oracle, box_mesh(2, 2, 2), 2, "linElas", nu=0.3, E=1.0, bc_sides=[])
    n, dt = prob.lsize(), 0.1
    X = prob.levels[prob.fine].dofmap.node_coords
    rng = np.random.default_rng(11)
    v0 = (np.sin(X @ rng.uniform(1, 3, (3, 3))) * rng.uniform(-1, 1, 3)).reshape(-1)
    nm = NewmarkPMG(prob, 1.3, dt, support={1: dict(kn=2.0, kt=1.0), 2: dict(cn=0.5, ct=0.3)}, coarse="cg", snes_rtol=rtol, ksp_rtol=1e-12)
    nm.set_initial(v0=v0, load=0.0)
    top = nm.nlev - 1
    tmp, vbar = oracle.vector(n).set_value(0.0), oracle.vector(n).set_value(0.0)

    def energy():
        nm.p.apply_jacobian(top, nm.xn, tmp)                                   # linElas: K u
        return nm.kinetic_energy() + 0.5 * nm.dot(nm.xn, tmp, True) + nm.support_energy()
    E = [energy()]
    assert E[0] > 0 and nm.support_energy() == 0.0
    worst = 0.0
    for _ in range(10):
        vbar.axpby(0.5, nm.vn, 0.0)
        assert nm.step().converged
        vbar.axpby(0.5, nm.vn, 1.0)
        tmp.set_value(0.0)
        nm.support_force_add("dashpot", vbar, tmp)
        loss = dt * nm.dot(vbar, tmp, True)
        E.append(energy())
        assert loss > 0 and E[-1] < E[-2]
        worst = max(worst, abs(E[-1] - E[-2] + loss) / E[0])
    print(f"Newmark energy identity: E_0 = {E[0]:.6e}, E_10 = {E[-1]:.6e}, worst defect {worst:.2e} of E_0, spring energy {nm.support_energy():.3e}")
    assert worst <= 100 * rtol and nm.support_energy() > 0
    tmp.destroy(); vbar.destroy(); nm.destroy(); prob.destroy()


def test_absorbing_end_under_both_steppers(oracle):
    """tol = 3 x the explicit portable run's error, 2.22e-2 sigma0 / (rho c) (Newmark at the same dt: 7.2e-3): 6.7 % of the exact
    velocity, where a free end gives about twice and a clamped end about none of it."""
    prob = sc.absorbing_problem(oracle)
    ab = absorbing_support(prob, sc.RHO)
    assert ab == dict(cn=1.0, ct=float(np.sqrt(0.5)))                          # rho c_p, rho c_s at nu = 0, E = rho = 1
    ex, nsteps = sc.absorbing_explicit(prob)
    for _ in range(nsteps):
        ex.step()
    assert ex.t > sc.LENGTH / sc.SPEED + sc.T_RAMP
    sc.check_absorbed(ex.velocity().reshape(-1, 3), f"explicit, {nsteps} steps of {ex.dt:.4f}")
    dt = ex.dt
    ex.destroy()
    sc.check_absorbed(sc.absorbing_newmark(prob, dt, nsteps), "Newmark at the same dt")
    prob.destroy()


def test_stable_dt_against_the_dense_one_step_matrix(oracle):
    prob = SolidProblem(oracle, box_mesh(1, 1, 2), 2, "linElas", nu=0.3, E=1.0, bc_sides=[], multigrid="none")
    n = prob.lsize()
    sup = {1: dict(kn=4.0, kt=2.0), 2: dict(cn=3.0, ct=1.0)}
    ex = ExplicitDynamics(prob, 1.0, support=sup, safety=0.9)
    ex.set_initial()
    top = ex.nlev - 1
    x, y = oracle.vector(n), oracle.vector(n)

    def dense(apply):
        cols = []
        for e in np.eye(n):
            x.set_array(e); y.set_value(0.0)
            apply(x, y)
            cols.append(y.to_numpy().copy())
        return np.stack(cols, axis=1)
    K = dense(lambda a, b: ex.A(top, a, b))                                    # K + K_s
    Cd = dense(lambda a, b: ex.supports[1]["levels"][top].tangent_add(1.0, ex.supports[1]["dashpot"], a, b))
    assert np.abs(K - K.T).max() <= 1e-12 * np.abs(K).max() and np.abs(Cd - Cd.T).max() <= 1e-12 * np.abs(Cd).max() and np.abs(Cd).max() > 0
    minv = 1.0 / ex.m.to_numpy()
    limit = ex.stable_dt() / ex.safety
    assert ex.emax_C is not None and ex.dt == ex.safety * limit
    w2, c = np.linalg.eigvals(minv[:, None] * K).real.max(), np.linalg.eigvals(minv[:, None] * Cd).real.max()
    assert 0.9 * w2 <= ex.emax_K <= w2 * (1 + 1e-12) and 0.9 * c <= ex.emax_C <= c * (1 + 1e-12)     # Lanczos: from below

    def radius(dt):
        I = np.eye(n)
        V = I - dt * minv[:, None] * Cd                                        # vh+ = V vh - dt m^-1 K x;  x+ = x + dt vh+
        G = np.block([[I - dt * dt * minv[:, None] * K, dt * V], [-dt * minv[:, None] * K, V]])
        return np.abs(np.linalg.eigvals(G)).max()
    rho, beyond = radius(0.999 * limit), radius(1.25 * (-c + np.sqrt(c * c + 4 * w2)) / w2)
    print(f"stable_dt: limit {limit:.5f}; emax {ex.emax_K:.4f} of {w2:.4f}, {ex.emax_C:.4f} of {c:.4f}; spectral radius {rho:.12f}, at 1.25 x the exact bound {beyond:.4f}")
    assert rho <= 1 + 1e-10 and beyond > 1 + 1e-3
    ex.destroy()
    ex = ExplicitDynamics(prob, 1.0, dt=1.01 * limit, support=sup, safety=0.9)
    with pytest.raises(ValueError, match="above the stable step .* lambda_max\\(m\\^-1 C_d\\)"):
        ex.set_initial()
    ex.destroy()
    # no dashpot: the expression of old, bit for bit
    ex = ExplicitDynamics(prob, 1.0, support={1: sup[1]}, safety=0.9)
    ex.set_initial()
    assert ex.stable_dt() == ex.safety * 2.0 / np.sqrt(1.1 * ex.emax_K) and ex.emax_C is None
    ex.destroy(); prob.destroy()


def test_refusals(oracle):
    mesh = box_mesh(2, 2, 1)
    prob = SolidProblem(oracle, mesh, 2, "linElas", nu=0.3, E=1.0, bc_sides=[1], multigrid="none")
    ok = dict(kn=1.0, kt=0.5)
    for make in (lambda **kw: NewtonPMG(prob, **kw), lambda **kw: LoadedBody(prob, **kw), lambda **kw: NewmarkPMG(prob, 1.0, 0.1, **kw),
                 lambda **kw: ExplicitDynamics(prob, 1.0, 0.1, **kw)):
        for sup, msg in (({77: ok}, "no such side set"), ({1: ok}, "Dirichlet side set"), ({2: dict(kn=1.0, k=2.0)}, "dict\\(kn=0., kt=0., cn=0., ct=0.\\) expected"),
                         ({2: dict(kn=-1.0)}, "not finite and non-negative"), ({2: dict(kn=float("inf"))}, "not finite and non-negative"),
                         ({2: dict(kn=0.0, kt=0.0, cn=0.0, ct=0.0)}, "all four coefficients are zero"), ({2: dict()}, "all four coefficients are zero")):
            with pytest.raises(ValueError, match=msg):
                make(support=sup)

        class TwoRanks:
            world = 2
        with pytest.raises(ValueError, match="several ranks"):
            make(support={2: ok}, halo=TwoRanks())
    with pytest.raises(ValueError, match="pbjacobi"):
        NewtonPMG(prob, support={2: ok}, smoother="pbjacobi")
    for sup in ({2: dict(kn=1.0, cn=0.1)}, {2: dict(ct=0.1)}):
        with pytest.raises(ValueError, match="dashpot coefficient"):
            NewtonPMG(prob, support=sup)
    plane = dict(plane=((0, 0, 1.1), (0, 0, -1.0)), penalty=5.0)
    for make in (lambda: NewmarkPMG(prob, 1.0, 0.1, contact={2: plane}, support={3: ok}), lambda: ExplicitDynamics(prob, 1.0, 0.1, contact={2: plane}, support={3: ok})):
        with pytest.raises(ValueError, match="static solves only"):            # the refusal of contact in dynamics stays
            make()
    sp = SupportSurface(oracle, mesh, prob.levels[0].dofmap, [2], prob.Q, portable=True)
    for kn, kt in ((-1.0, 1.0), (1.0, float("nan")), (float("inf"), 0.0)):
        with pytest.raises(ValueError, match="not finite and non-negative"):
            sp.state_host(kn, kt)
    # with a clamp, an assembled coarse level is accepted (its matrix lacks the term: documented)
    prob2 = SolidProblem(oracle, mesh, 2, "linElas", nu=0.3, E=1.0, bc_sides=[1])
    s = NewtonPMG(prob2, support={2: ok}, coarse="assembled")
    assert len(s.supports) == 1 and s.supports[0]["dashpot"] is None and s._fused_op(s.nlev - 1) is None
    s.destroy(); prob2.destroy(); prob.destroy()


def test_no_support_given_takes_no_new_path(oracle):
    prob = SolidProblem(oracle, box_mesh(2, 2, 2), 2, "hyperFS", nu=0.3, E=1.0, bc_sides=[1])
    force = 0.01 * np.random.default_rng(2).uniform(-1, 1, prob.lsize())
    a = NewtonPMG(prob, forcing=force)
    a.solve(num_increments=1)
    b = NewtonPMG(prob, forcing=force, support=None)
    b.solve(num_increments=1)
    c = NewtonPMG(prob, forcing=force, support={})
    assert b.supports == [] == c.supports and not b.has_dashpots()
    assert b._fused_op(b.nlev - 1) is a._fused_op(a.nlev - 1) is not None
    assert np.array_equal(a.U.to_numpy(), b.U.to_numpy()) and np.abs(a.U.to_numpy()).max() > 0
    assert a.stats.history == b.stats.history
    a.destroy(); b.destroy(); c.destroy()
    ex = ExplicitDynamics(prob, 1.0)
    ex.set_initial()
    assert ex.supports == [] and ex.emax_C is None and ex.dt == ex.safety * 2.0 / np.sqrt(1.1 * ex.emax_K)
    nm = NewmarkPMG(prob, 1.0, 0.1)
    assert nm.supports == [] and nm._vnew is None and nm.support_energy() == 0.0
    ex.destroy(); nm.destroy(); prob.destroy()
