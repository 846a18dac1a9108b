"""Surface loads that vary over a side set (surface.py, "Fields"), the portable NumPy form against facts: constant fields give the
constant kinds, Archimedes' principle on a submerged box, the triangular load on a wall, the tangents as exact derivatives, the
hydrostatic tangent's symmetry on a closed surface, the Dirichlet mask, whole solves on the CPU oracle and the solver's refusals.

The bounds are stated per test; where a closed form is used it is exact for the quadrature, and the argument stands with the test."""
import math

import numpy as np
import pytest

from ceedpetscsolid_amd.dynamics import ExplicitDynamics, NewmarkPMG
from ceedpetscsolid_amd.mesh import box_mesh, build_dofmap, dirichlet_mask, side_set_nodes
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG
from ceedpetscsolid_amd.surface import SurfaceLoad

ALL_SIDES = [1, 2, 3, 4, 5, 6]            # box_mesh: z-, z+, y-, y+, x+, x-
E, NU = 1.0, 0.3
F_AFFINE = np.array([[1.10, 0.20, -0.05], [0.03, 0.90, 0.15], [-0.12, 0.07, 1.25]])
C_AFFINE = np.array([0.4, -0.2, 0.1])


def load(oracle, mesh, p, sides, **kw):
    dm = build_dofmap(mesh, p)
    return SurfaceLoad(oracle, mesh, dm, sides, portable=True, **kw), dm


def smooth(X, k):
    """A smooth, non-polynomial 3-vector field of the coordinates, entries in [-1, 1]."""
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    return np.stack([np.sin(1.3 * x + 0.7 * y + k) * np.cos(0.9 * z), np.cos(1.1 * y - 0.4 * z + k) * np.sin(0.8 * x + 0.3),
                     np.sin(0.6 * x - 1.2 * y + 0.5 * z + 2 * k)], axis=1)


# ---- constant fields -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3])
def test_constant_fields_give_the_constant_kinds(oracle, p):
    """Bound 1e-13 of the max norm: sum_b N_b = 1 to a few roundings, everything else is the same sum."""
    sl, dm = load(oracle, box_mesh(2, 3, 1, hi=(1.0, 2.0, 3.0)), p, [2, 5])
    rng = np.random.default_rng(p)
    u, du = 0.1 * rng.uniform(-1, 1, dm.lsize), rng.uniform(-1, 1, dm.lsize)
    t, pv = np.array([0.3, -1.1, 0.7]), 0.37
    pairs = {"traction": (sl.traction_field_host(np.tile(t, dm.nnodes)), sl.traction_host(t)),
             "pressure": (sl.pressure_field_host(np.full(dm.nnodes, pv), u), pv * sl.pressure_host(u)),
             "pressure(u=0)": (sl.pressure_field_host(np.full(dm.nnodes, pv)), pv * sl.pressure_host()),
             "tangent": (sl.pressure_field_tangent_host(np.full(dm.nnodes, pv), u, du), pv * sl.tangent_host(u, du))}
    for kind, (got, want) in pairs.items():
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"p={p} {kind}: {err:.2e}")
        assert err <= 1e-13, (kind, err)


# ---- Archimedes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3])
def test_archimedes(oracle, p):
    """The closed surface of a box under x = F X + c, fully submerged: the nodal vectors sum to -gamma det(F) V0 e and have no moment
    about the centroid of buoyancy.  Exact for the quadrature: x is affine in (xi, eta) on every face, so the summed integrands have
    degree 1 (force) and 2 (moment) per direction.  Bound 1e-12 relative to gamma det(F) V0 (times the unit length for the moment)."""
    mesh = box_mesh(2, 2, 2)
    sl, dm = load(oracle, mesh, p, ALL_SIDES)
    gamma, up, level = 1.7, np.array([0.2, -0.3, 1.0]), 4.0
    e = up / np.linalg.norm(up)
    X = dm.node_coords
    V0 = float(np.prod(X.max(axis=0) - X.min(axis=0)))
    x = X @ F_AFFINE.T + C_AFFINE
    u = (x - X).reshape(-1)
    assert sl.depth_host(level, up, u).min() > 0.5                        # fully submerged
    g = sl.hydrostatic_host(gamma, level, up, u).reshape(-1, 3)
    want = -gamma * np.linalg.det(F_AFFINE) * V0 * e
    xc = F_AFFINE @ (0.5 * (X.max(axis=0) + X.min(axis=0))) + C_AFFINE    # the centroid of the deformed box
    force = np.array([math.fsum(g[:, c]) for c in range(3)])
    mom = np.cross(x - xc, g)
    moment = np.array([math.fsum(mom[:, c]) for c in range(3)])
    scale = gamma * np.linalg.det(F_AFFINE) * V0
    print(f"p={p}: buoyancy error {np.abs(force - want).max() / scale:.2e}, moment {np.abs(moment).max() / scale:.2e}")
    assert np.abs(force - want).max() <= 1e-12 * scale
    assert np.abs(moment).max() <= 1e-12 * scale


# ---- the ramp --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3])
def test_ramp_on_a_wall(oracle, p):
    """Side x+ of a column of four elements with the level ON an element boundary: the resultant is gamma h^2 b / 2 along the outward
    normal (the pressure is linear on the wet faces: exact), and the dry faces contribute exact zeros (d < 0 at their points)."""
    b, H = 1.5, 2.0
    mesh = box_mesh(1, 1, 4, hi=(1.0, b, H))
    sl, dm = load(oracle, mesh, p, [5])
    gamma, level = 2.5, 1.0
    g = sl.hydrostatic_host(gamma, level, (0.0, 0.0, 1.0)).reshape(-1, 3)
    want = gamma * level ** 2 * b / 2
    total = np.array([math.fsum(g[:, c]) for c in range(3)])
    print(f"p={p}: resultant {total}, gamma h^2 b / 2 = {want}")
    assert np.abs(total - np.array([want, 0.0, 0.0])).max() <= 1e-12 * want
    dry = dm.node_coords[:, 2] > level + 1e-12
    assert dry.any() and np.all(g[dry] == 0.0)
    assert np.abs(g[~dry]).max() > 0


# ---- tangents as derivatives -----------------------------------------------------------------------------------------------------
STEP = 1e-2


def tangent_case(oracle, p):
    mesh = box_mesh(2, 2, 2)
    sl, dm = load(oracle, mesh, p, [5, 2])
    X = dm.node_coords
    return sl, dm, (0.02 * smooth(X, 0.3)).reshape(-1), smooth(X, 1.1).reshape(-1), np.cos(X @ np.array([0.7, -0.5, 1.2]))


@pytest.mark.parametrize("p", [1, 2, 3])
def test_pressure_field_tangent_is_the_derivative(oracle, p):
    """g is quadratic in u: the central difference is exact up to rounding.  Step 1e-2, bound 1e-10 relative."""
    sl, dm, u, du, pf = tangent_case(oracle, p)
    T = sl.pressure_field_tangent_host(pf, u, du)
    fd = (sl.pressure_field_host(pf, u + STEP * du) - sl.pressure_field_host(pf, u - STEP * du)) / (2 * STEP)
    err = np.abs(T - fd).max() / np.abs(T).max()
    print(f"p={p}: pressure-field tangent against the central difference {err:.2e}")
    assert err <= 1e-10


@pytest.mark.parametrize("p", [1, 2, 3])
def test_hydrostatic_tangent_is_the_derivative(oracle, p):
    """g is cubic in u away from the kink: the 5-point stencil is exact up to rounding.  Step 1e-2, bound 1e-10 relative.  The
    level passes through the body; no point's depth lies within 2 step max|du| of zero, so no point changes sides in the stencil."""
    sl, dm, u, du, _ = tangent_case(oracle, p)
    gamma, level, up = 1.3, 0.61, (0.1, 0.0, 1.0)
    d = sl.depth_host(level, up, u)
    assert (d > 0).any() and (d < 0).any()
    assert np.abs(d).min() >= 2 * STEP * np.abs(du).max(), np.abs(d).min()
    g = lambda s: sl.hydrostatic_host(gamma, level, up, u + s * STEP * du)
    T = sl.hydrostatic_tangent_host(gamma, level, up, u, du)
    fd = (-g(2) + 8 * g(1) - 8 * g(-1) + g(-2)) / (12 * STEP)
    err = np.abs(T - fd).max() / np.abs(T).max()
    print(f"p={p}: hydrostatic tangent against the 5-point stencil {err:.2e}, min |d| = {np.abs(d).min():.3f}")
    assert err <= 1e-10


# ---- symmetry --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,Q,cells", [(1, 2, (2, 2, 2)), (2, 4, (2, 2, 2)), (3, 6, (2, 1, 1))])
def test_hydrostatic_tangent_is_symmetric_on_a_closed_submerged_surface(oracle, p, Q, cells):
    """The fluid's potential gamma int_v d dv depends on the closed surface alone; where the sums g_a are exact integrals g is its
    gradient and T its Hessian.  With N_a inside, the integrand N_a d (x_xi x x_eta) has degree p + p + (2p - 1) = 4p - 1 per direction,
    so Q = 2p Gauss points are exact (at Q = P the discrete form is defined by the quadrature and is symmetric only to the quadrature
    error: measured 6e-7 at p = 2, Q = 3 on this surface).  T is formed densely (375 columns at most);
    |v . T w - w . T v| <= 1e-12 |v| |w| |T|."""
    mesh = box_mesh(*cells)
    dm = build_dofmap(mesh, p)
    sl = SurfaceLoad(oracle, mesh, dm, ALL_SIDES, Q=Q, portable=True)
    n = dm.lsize
    u = (0.05 * smooth(dm.node_coords, 0.7)).reshape(-1)
    gamma, level, up = 0.9, 3.0, (0.3, 0.2, 1.0)
    assert sl.depth_host(level, up, u).min() > 0.5
    T = np.stack([sl.hydrostatic_tangent_host(gamma, level, up, u, col) for col in np.eye(n)], axis=1)
    norm = np.linalg.norm(T, 2)
    rng = np.random.default_rng(p)
    v, w = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    skew = abs(v @ (T @ w) - w @ (T @ v))
    print(f"p={p} Q={Q}: |v.Tw - w.Tv| / (|v||w||T|) = {skew / (np.linalg.norm(v) * np.linalg.norm(w) * norm):.2e}, "
          f"max|T - T^T| / |T| = {np.abs(T - T.T).max() / norm:.2e}")
    assert skew <= 1e-12 * np.linalg.norm(v) * np.linalg.norm(w) * norm
    assert np.abs(T - T.T).max() <= 1e-12 * norm


# ---- masks -----------------------------------------------------------------------------------------------------------------------
def test_masked_rows_are_never_written(oracle):
    mesh = box_mesh(2, 3, 1, hi=(1.0, 2.0, 3.0))
    dm = build_dofmap(mesh, 2)
    mask = dirichlet_mask(dm, side_set_nodes(mesh, dm, [6])).copy()     # clamp x-: its edge with side 2 is masked
    mask[3 * side_set_nodes(mesh, dm, [2])[4] + 1] = 1                   # and one component of one more node
    m = mask != 0
    sl = SurfaceLoad(oracle, mesh, dm, [2], mask=mask, portable=True)
    free = SurfaceLoad(oracle, mesh, dm, [2], portable=True)
    X = dm.node_coords
    u, du = (0.1 * smooth(X, 0.2)).reshape(-1), smooth(X, 0.9).reshape(-1)
    tf, pf = smooth(X, 1.7).reshape(-1), 1.0 + 0.5 * np.sin(X[:, 0] + 2 * X[:, 1])
    hyd = (1.1, 3.4, (0.0, 0.2, 1.0))
    junk = du.copy(); junk[m] = 1e30
    zeroed = np.where(m, 0.0, du)
    for name, f, tangent in (("traction field", lambda s, d: s.traction_field_host(tf), False),
                             ("pressure field", lambda s, d: s.pressure_field_host(pf, u), False),
                             ("hydrostatic", lambda s, d: s.hydrostatic_host(*hyd, u), False),
                             ("pressure-field tangent", lambda s, d: s.pressure_field_tangent_host(pf, u, d), True),
                             ("hydrostatic tangent", lambda s, d: s.hydrostatic_tangent_host(*hyd, u, d), True)):
        g, g0 = f(sl, du), f(free, zeroed if tangent else du)
        assert np.all(g[m] == 0.0) and np.array_equal(g[~m], g0[~m]) and np.abs(g0[m]).max() > 0, name
        if tangent:
            assert np.array_equal(g, f(sl, junk)), name                  # masked du is never read as it is
    # y += on vectors: rows off the surface and masked rows keep their bits
    y0 = np.random.default_rng(3).uniform(-1, 1, dm.lsize)
    Y, U = oracle.vector(dm.lsize).set_array(y0), oracle.vector(dm.lsize).set_array(u)
    PF = oracle.vector(dm.nnodes).set_array(pf)
    sl.pressure_field_add(PF, 0.5, U, Y)
    sl.hydrostatic_add(*hyd, 0.25, U, Y)
    y = Y.to_numpy()
    touched = y != y0
    on = np.zeros(dm.nnodes, dtype=bool); on[side_set_nodes(mesh, dm, [2])] = True
    assert touched.any() and not touched[m].any() and not touched[~np.repeat(on, 3)].any()
    assert np.allclose(y, y0 + 0.5 * sl.pressure_field_host(pf, u) + 0.25 * sl.hydrostatic_host(*hyd, u), rtol=0, atol=1e-15)


# ---- solves on the oracle --------------------------------------------------------------------------------------------------------
def total_displacement(s):
    return s.U.to_numpy() + s.bcv.to_numpy()


def test_a_constant_pressure_field_solves_like_the_constant_pressure(oracle):
    mesh = box_mesh(2, 2, 2)
    prob = SolidProblem(oracle, mesh, 2, "hyperFS", nu=NU, E=E, bc_sides=[3, 4, 5, 6])
    nn = prob.levels[prob.fine].dofmap.nnodes
    a = NewtonPMG(prob, pressure={2: 0.02 * E}, snes_rtol=1e-10)
    sa = a.solve(num_increments=1)
    b = NewtonPMG(prob, pressure_field={2: np.full(nn, 0.02 * E)}, snes_rtol=1e-10)
    sb = b.solve(num_increments=1)
    c = NewtonPMG(prob, pressure_field={2: lambda X: np.full(X.shape[0], 0.02 * E)}, snes_rtol=1e-10)
    sc = c.solve(num_increments=1)
    ua, ub = total_displacement(a), total_displacement(b)
    print(f"constant pressure {sa.newton_its} / {sa.ksp_its}, constant field {sb.newton_its} / {sb.ksp_its}, "
          f"|U_field - U| / |U| = {np.linalg.norm(ub - ua) / np.linalg.norm(ua):.2e}")
    assert sa.converged and sb.converged and sc.converged and np.abs(ua).max() > 1e-4
    assert (sb.newton_its, sb.ksp_its) == (sa.newton_its, sa.ksp_its)
    assert np.linalg.norm(ub - ua) <= 1e-10 * np.linalg.norm(ua)
    assert np.array_equal(total_displacement(c), ub)                     # the callable is the array
    assert len(b.field_loads) == 1 and b.pressure_loads == [] and b.has_followers()
    for s in (a, b, c):
        s.destroy()
    assert b.field_loads == [] and b.surface_loads == []
    prob.destroy()


HYDRO_BLOCK = dict(gamma=0.08 * E, level=0.8, up=(0.0, 0.0, 1.0))


def hydrostatic_block(ceed, tangent):
    """A block clamped at its base (z-) with water against side x+ up to 0.8 of its height: (mesh, prob, solver, stats)."""
    mesh = box_mesh(2, 2, 2)
    prob = SolidProblem(ceed, mesh, 2, "hyperFS", nu=NU, E=E, bc_sides=[1])
    s = NewtonPMG(prob, hydrostatic={5: HYDRO_BLOCK}, pressure_tangent=tangent)
    return mesh, prob, s, s.solve(num_increments=1)


def reaction_balance(ceed, mesh, prob, s, st):
    """(sum of F_int over the free nodes + the load they carry, the clamp's reactions - that load, the last residual norm): the load
    is the portable resultant at the converged state on the rows the solver writes."""
    lv = prob.levels[prob.fine]
    u = total_displacement(s)
    q = SolidProblem(ceed, mesh, 2, "hyperFS", nu=NU, E=E, multigrid="none")
    Xv, Yv = ceed.vector(u.size).set_array(u), ceed.vector(u.size)
    q.form_residual(Xv, Yv)
    f = Yv.to_numpy().copy().reshape(-1, 3)
    q.destroy()
    ref = SurfaceLoad(ceed, mesh, lv.dofmap, [5], Q=prob.Q, mask=lv.mask, portable=True)
    g = ref.hydrostatic_host(HYDRO_BLOCK["gamma"], HYDRO_BLOCK["level"], HYDRO_BLOCK["up"], u).reshape(-1, 3)
    clamped = np.zeros(f.shape[0], dtype=bool)
    clamped[side_set_nodes(mesh, lv.dofmap, [1])] = True
    exact_sum = lambda a: np.array([math.fsum(a[:, c]) for c in range(3)])
    G = exact_sum(g)
    return exact_sum(f[~clamped]) + G, exact_sum(f[clamped]) - G, st.history[-1][4], G, u


def test_hydrostatic_block_reactions_and_tangent(oracle):
    mesh, prob, full, st = hydrostatic_block(oracle, "full")
    assert st.converged
    carried, reaction, rnorm, G, u = reaction_balance(oracle, mesh, prob, full, st)
    print(f"hydrostatic block, full tangent: {st.newton_its} Newton / {st.ksp_its} Krylov, |R| = {rnorm:.3e}, resultant {G}, "
          f"carried + G = {carried}, reactions - G = {reaction}")
    assert G[0] > 1e-3 and np.abs(u).max() > 1e-3                        # the water pushes the wall towards -x: R gains +G
    assert u.reshape(-1, 3)[side_set_nodes(mesh, prob.levels[prob.fine].dofmap, [2]), 0].max() < 0
    assert np.abs(carried).max() <= 10 * rnorm
    assert np.abs(reaction).max() <= 10 * rnorm
    _, prob0, none, st0 = hydrostatic_block(oracle, "none")
    assert st0.converged
    print(f"hydrostatic block, no tangent: {st0.newton_its} Newton / {st0.ksp_its} Krylov")
    assert st.newton_its <= st0.newton_its
    assert np.linalg.norm(total_displacement(none) - u) <= 1e-6 * np.linalg.norm(u)
    full.destroy(); none.destroy(); prob.destroy(); prob0.destroy()


def follower_host(s, x):
    """load sum_s g_s(x) of the solver's pressure fields and hydrostatic loads, by the portable forms, on the rows it writes."""
    lv = s.p.levels[s.p.fine]
    out = np.zeros(s.p.lsize())
    for kind, sl, par in s.field_loads:
        ref = SurfaceLoad(s.ceed, s.p.mesh, lv.dofmap, sl.side_ids, Q=s.p.Q, mask=lv.mask, portable=True)
        out += ref.pressure_field_host(par.to_numpy(), x) if kind == "pressure_field" else ref.hydrostatic_host(par[0], par[1], par[2], x)
    return s.load * out


FIELDS = dict(pressure_field={2: lambda X: 0.01 * E * (1.0 + X[:, 0])}, hydrostatic={5: HYDRO_BLOCK})


def test_a_newmark_step_matches_a_hand_formed_residual(oracle):
    mesh = box_mesh(2, 2, 1)
    prob = SolidProblem(oracle, mesh, 2, "hyperFS", nu=NU, E=E, bc_sides=[1])
    s = NewmarkPMG(prob, density=1.0, dt=0.05, **FIELDS)
    plain = NewmarkPMG(prob, density=1.0, dt=0.05)
    s.set_initial(); plain.set_initial()
    st = s.step()
    assert st.converged and np.abs(s.U.to_numpy()).max() > 1e-6
    plain.step()
    for name in ("U", "bcv", "xn", "vn", "an", "_pred"):                 # the loaded solver's state into the plain one
        plain._set(getattr(plain, name), getattr(s, name).to_numpy())
    n = prob.lsize()
    R1, R2 = oracle.vector(n).set_value(0.0), oracle.vector(n).set_value(0.0)
    s.residual(s.U, R1); plain.residual(plain.U, R2)
    hand = R2.to_numpy() + follower_host(s, s.Xloc.to_numpy())
    scale = np.abs(hand).max() + np.abs(follower_host(s, s.Xloc.to_numpy())).max()
    print(f"Newmark: |R - hand| / scale = {np.abs(R1.to_numpy() - hand).max() / scale:.2e}")
    assert np.abs(R1.to_numpy() - hand).max() <= 1e-13 * scale
    s.destroy(); plain.destroy(); prob.destroy()


def test_explicit_steps_match_a_hand_formed_residual(oracle):
    mesh = box_mesh(2, 2, 1)
    prob = SolidProblem(oracle, mesh, 2, "hyperFS", nu=NU, E=E, bc_sides=[1])
    s = ExplicitDynamics(prob, density=1.0, **FIELDS)
    s.set_initial()
    for _ in range(3):
        s.step()
    x = s.x.to_numpy()
    assert np.all(np.isfinite(x)) and np.abs(x).max() > 0
    n = prob.lsize()
    X, R = oracle.vector(n).set_array(x), oracle.vector(n).set_value(0.0)
    prob.form_residual(X, R)
    g = follower_host(s, x)
    hand = R.to_numpy() + g
    scale = np.abs(hand).max() + np.abs(g).max()
    print(f"explicit: |R - hand| / scale = {np.abs(s.R.to_numpy() - hand).max() / scale:.2e}")
    assert np.abs(g).max() > 0 and np.abs(s.R.to_numpy() - hand).max() <= 1e-13 * scale
    s.destroy(); prob.destroy()


def test_no_new_keyword_takes_no_new_path(oracle):
    mesh = box_mesh(2, 2, 1)
    prob = SolidProblem(oracle, mesh, 2, "hyperFS", nu=NU, E=E, bc_sides=[1])
    force = 0.01 * np.random.default_rng(2).uniform(-1, 1, prob.lsize())
    kw = dict(forcing=force, traction={2: (0.0, 0.0, 0.005)}, pressure={5: 0.01})
    a = NewtonPMG(prob, **kw)
    a.solve(num_increments=1)
    b = NewtonPMG(prob, traction_field=None, pressure_field={}, hydrostatic=None, **kw)
    b.solve(num_increments=1)
    assert b.field_loads == [] and len(b.surface_loads) == 2 and len(b.pressure_loads) == 1
    assert np.array_equal(a.U.to_numpy(), b.U.to_numpy()) and np.abs(a.U.to_numpy()).max() > 0
    # the parent form of the residual: F_int - load f + load p g^pressure, by the calls the parent made
    n = prob.lsize()
    R, Rp = oracle.vector(n).set_value(0.0), oracle.vector(n).set_value(0.0)
    b.residual(b.U, R)
    prob.form_residual(b.Xloc, Rp)
    Rp.axpby(-b.load, b.fv, 1.0)
    for sl, pval in b.pressure_loads:
        sl.pressure_add(pval, b.load, b.Xloc, Rp)
    assert np.array_equal(R.to_numpy(), Rp.to_numpy())
    a.destroy(); b.destroy(); prob.destroy()


def test_traction_field_is_folded_into_the_load_vector(oracle):
    mesh = box_mesh(2, 2, 1)
    prob = SolidProblem(oracle, mesh, 2, "hyperFS", nu=NU, E=E, bc_sides=[1])
    lv = prob.levels[prob.fine]
    t = (0.0, 0.01, -0.02)
    a = NewtonPMG(prob, traction={2: t})
    b = NewtonPMG(prob, traction_field={2: np.tile(t, (lv.dofmap.nnodes, 1))})
    fa, fb = a.fv.to_numpy(), b.fv.to_numpy()
    assert np.abs(fa - fb).max() <= 1e-13 * np.abs(fa).max() and np.all(fb[lv.mask != 0] == 0.0)
    c = NewtonPMG(prob, traction_field={2: lambda X: X * 0.01})
    ref = SurfaceLoad(oracle, mesh, lv.dofmap, [2], Q=prob.Q, mask=lv.mask, portable=True)
    assert np.array_equal(c.fv.to_numpy(), ref.traction_field_host(0.01 * lv.dofmap.node_coords))
    for s in (a, b, c):
        s.destroy()
    prob.destroy()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(oracle):
    mesh = box_mesh(2, 2, 1)
    prob = SolidProblem(oracle, mesh, 2, "hyperFS", nu=NU, E=E, bc_sides=[1], multigrid="none")
    nn = prob.levels[prob.fine].dofmap.nnodes
    tf, pf, hy = np.zeros((nn, 3)), np.zeros(nn), dict(gamma=1.0, level=0.5)

    class TwoRanks:
        world = 2
    for kw in (dict(traction_field={2: tf}), dict(pressure_field={2: pf}), dict(hydrostatic={2: hy})):
        with pytest.raises(ValueError, match="several ranks"):
            NewtonPMG(prob, halo=TwoRanks(), **kw)
        (key, val), = kw.items()
        with pytest.raises(ValueError, match="no such side set"):
            NewtonPMG(prob, **{key: {77: val[2]}})
        with pytest.raises(ValueError, match="Dirichlet side set"):
            NewtonPMG(prob, **{key: {1: val[2]}})
    for bad in (np.zeros((nn, 2)), np.zeros(3 * nn), np.zeros((nn + 1, 3)), lambda X: X[:, 0]):
        with pytest.raises(ValueError, match="traction_field on side set 2: an array of shape"):
            NewtonPMG(prob, traction_field={2: bad})
    for bad in (np.zeros((nn, 3)), np.zeros(nn - 1), 0.5, lambda X: X):
        with pytest.raises(ValueError, match="pressure_field on side set 2: an array of shape"):
            NewtonPMG(prob, pressure_field={2: bad})
    with pytest.raises(ValueError, match="not finite"):
        NewtonPMG(prob, pressure_field={2: np.full(nn, np.nan)})
    for bad in (dict(gamma=1.0, level=0.5, depth=1.0), dict(gamma=1.0), dict(level=1.0), 3.0, (1.0, 0.5)):
        with pytest.raises(ValueError, match=r"hydrostatic on side set 2: dict\(gamma=, level=, up="):
            NewtonPMG(prob, hydrostatic={2: bad})
    for bad in (dict(gamma=np.inf, level=0.5), dict(gamma=1.0, level=np.nan)):
        with pytest.raises(ValueError, match="must be finite"):
            NewtonPMG(prob, hydrostatic={2: bad})
    for up in ((0.0, 0.0, 0.0), (0.0, np.inf, 1.0), (1.0, 0.0)):
        with pytest.raises(ValueError, match="finite, non-zero 3-vector"):
            NewtonPMG(prob, hydrostatic={2: dict(gamma=1.0, level=0.5, up=up)})
    # the portable methods refuse the same shapes
    sl, dm = load(oracle, mesh, 2, [2])
    with pytest.raises(ValueError, match="traction field"):
        sl.traction_field_host(np.zeros(dm.lsize - 3))
    with pytest.raises(ValueError, match="pressure field"):
        sl.pressure_field_host(np.zeros(dm.lsize))
    with pytest.raises(ValueError, match="finite, non-zero"):
        sl.hydrostatic_host(1.0, 0.5, (0, 0, 0))
    with pytest.raises(ValueError, match="pressure_tangent"):
        NewtonPMG(prob, hydrostatic={2: hy}, pressure_tangent="symmetrised")
    assert NewtonPMG(prob).field_loads == []
    prob.destroy()
