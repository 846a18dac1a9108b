"""Penalty contact (contact.py), the portable NumPy form against facts: the residual as the derivative of the potential and the tangent
as the derivative of the residual, the tangent's symmetry, the diagonal, the coarse p-level's tangent as the Galerkin product of the fine
one, exact zeros where nothing touches, and the Dirichlet mask.

Inputs and their input condition (min |g| >= 1e-6, 10 % .. 90 % of the points active): ``_contact_inputs``; every test that uses them
asserts the condition first.

The central differences take h = 1e-7 along a direction |du| <= 1.
  * Plane: r is piecewise linear in u and the potential piecewise quadratic, so the central difference of r is EXACT up to rounding as
    long as no point changes side along the step; a point moves by at most h |du| Lambda^2 ~ 1e-7 x (the Lebesgue constant, < 3 for
    P <= 8, squared) < 1e-6, the margin of the input condition.
  * Sphere: the truncation error is h^2 / 6 times a third derivative of O(eps / R^2): 1e-14 relative, far below the rounding.
  * Rounding: a nodal value of r is a sum of n_terms ~ 4 Q^2 (a corner of four faces) products of O(1) table entries, each carrying a
    few eps of relative error, so |fd - C du| <~ n_terms eps max|r| / h = 256 x 1.1e-16 x max|r| / 1e-7 ~ 3e-7 max|r| at Q = 8, and
    max|r| ~ eps_pen w J <-g> <~ 0.1 max|C du| (penetrations here are below 0.1 of a length, |du| ~ 1).  Bound: 1e-6 max|C du|.
  * The same count for the potential: |fd - du . r| <~ n_points eps Pi / h with Pi ~ 0.1 |du . r|: the bound 1e-6 |du| |r| (norms) is
    loose by orders.
The symmetric, diagonal, Galerkin and mask identities hold to rounding of sums of a few hundred O(1) terms: 1e-12 relative."""
import numpy as np
import pytest

import _contact_inputs as ci
from ceedpetscsolid_amd.contact import ContactSurface, obstacle_parameters
from ceedpetscsolid_amd.mesh import box_mesh, build_dofmap, dirichlet_mask, gll_nodes, hollow_cylinder_mesh, side_set_nodes

SHAPES = {"six sides": (lambda: box_mesh(2, 2, 1), [1, 2, 3, 4, 5, 6]), "curved wall": (lambda: hollow_cylinder_mesh(1, 5, 2), [996]),
          "side 1": (lambda: box_mesh(2, 2, 1), [1])}
H = 1e-7


def surface(oracle, shape, P, Q, which, mask=None):
    make, sides = SHAPES[shape]
    mesh = make()
    dm = build_dofmap(mesh, P - 1)
    cs = ContactSurface(oracle, mesh, dm, sides, Q, mask=mask, portable=True)
    u, du = ci.displacement(dm, P, Q)
    ci.set_obstacle(cs, which, u)
    return cs, mesh, dm, u, du


CASES = [("six sides", 3, 4), ("curved wall", 3, 3), ("side 1", 5, 6)]


@pytest.mark.parametrize("which", ci.OBSTACLES)
@pytest.mark.parametrize("shape,P,Q", CASES)
def test_residual_is_the_derivative_of_the_potential(oracle, shape, P, Q, which):
    cs, _, _, u, du = surface(oracle, shape, P, Q, which)
    gmin, share = ci.input_condition(cs, u)
    r, _ = cs.residual_host(u)
    fd = (cs.energy_host(u + H * du) - cs.energy_host(u - H * du)) / (2 * H)
    err, scale = abs(fd - du @ r), np.linalg.norm(du) * np.linalg.norm(r)
    print(f"{shape} P={P} Q={Q} {which}: min|g| {gmin:.2e}, active {share:.2f}, |fd - du.r| = {err:.2e} of |du||r| = {scale:.2e}")
    assert scale > 0 and err <= 1e-6 * scale


@pytest.mark.parametrize("which", ci.OBSTACLES)
@pytest.mark.parametrize("shape,P,Q", CASES)
def test_tangent_is_the_derivative_of_the_residual(oracle, shape, P, Q, which):
    cs, _, _, u, du = surface(oracle, shape, P, Q, which)
    ci.input_condition(cs, u)
    _, state = cs.residual_host(u)
    fd = (cs.residual_host(u + H * du)[0] - cs.residual_host(u - H * du)[0]) / (2 * H)
    cv = cs.tangent_host(state, du)
    err, scale = np.abs(fd - cv).max(), np.abs(cv).max()
    print(f"{shape} P={P} Q={Q} {which}: max|fd - C du| = {err:.2e} of max|C du| = {scale:.2e}")
    assert scale > 0 and err <= 1e-6 * scale


@pytest.mark.parametrize("which", ci.OBSTACLES)
@pytest.mark.parametrize("shape,P,Q", CASES)
def test_tangent_is_symmetric(oracle, shape, P, Q, which):
    cs, _, dm, u, v = surface(oracle, shape, P, Q, which)
    ci.input_condition(cs, u)
    _, state = cs.residual_host(u)
    w = np.random.default_rng(5).uniform(-1, 1, dm.lsize)
    cv, cw = cs.tangent_host(state, v), cs.tangent_host(state, w)
    d, bound = abs(w @ cv - v @ cw), np.linalg.norm(w) * np.linalg.norm(cv) + np.linalg.norm(v) * np.linalg.norm(cw)
    print(f"{shape} P={P} Q={Q} {which}: |w.Cv - v.Cw| = {d:.2e} of {bound:.2e}")
    assert bound > 0 and d <= 1e-12 * bound


@pytest.mark.parametrize("which", ci.OBSTACLES)
def test_diagonal_is_the_tangent_on_unit_vectors(oracle, which):
    cs, _, dm, u, _ = surface(oracle, "side 1", 3, 4, which)
    ci.input_condition(cs, u)
    _, state = cs.residual_host(u)
    d = cs.diagonal_host(state)
    on = np.unique(cs.faces)
    assert np.all(np.delete(d.reshape(-1, 3), on, axis=0) == 0.0) and np.abs(d).max() > 0
    worst = 0.0
    for i in (3 * on[:, None] + np.arange(3)).reshape(-1):
        e = np.zeros(dm.lsize); e[i] = 1.0
        worst = max(worst, abs(cs.tangent_host(state, e)[i] - d[i]))
    print(f"{which}: max |e_i.C e_i - d_i| = {worst:.2e} of {np.abs(d).max():.2e}")
    assert worst <= 1e-12 * np.abs(d).max()


def interpolation(Pc, Pf):
    """I [Pf][Pc]: the Pc Lagrange functions on the Gauss-Lobatto points (the nodes of ``lagrange_tables``) at the Pf Gauss-Lobatto points."""
    xc, xf = gll_nodes(Pc), gll_nodes(Pf)
    I = np.ones((Pf, Pc))
    for i in range(Pc):
        for k in range(Pc):
            if k != i:
                I[:, i] *= (xf - xc[k]) / (xc[i] - xc[k])
    return I


@pytest.mark.parametrize("which", ci.OBSTACLES)
@pytest.mark.parametrize("Pc,Pf,Q", [(2, 3, 3), (2, 5, 6), (3, 5, 5)])
def test_coarse_tangent_is_the_galerkin_product(oracle, Pc, Pf, Q, which):
    fine, mesh, dmf, u, _ = surface(oracle, "six sides", Pf, Q, which)
    ci.input_condition(fine, u)
    _, state = fine.residual_host(u)
    dmc = build_dofmap(mesh, Pc - 1)
    coarse = ContactSurface(oracle, mesh, dmc, SHAPES["six sides"][1], Q, portable=True)       # no obstacle, no geometry use: the state alone
    assert coarse.nface == fine.nface
    # the nodal prolongation on the surface, row by row from the faces (a shared edge gets the same row from either face)
    I2 = np.kron(interpolation(Pc, Pf), interpolation(Pc, Pf))                                 # [j i of the fine face][j i of the coarse face]
    Pmat = np.zeros((dmf.nnodes, dmc.nnodes))
    for ff, fc in zip(fine.faces, coarse.faces):
        Pmat[ff] = 0.0
        Pmat[ff[:, None], fc[None, :]] = I2
    v = np.random.default_rng(Pc + Pf).uniform(-1, 1, dmc.lsize)
    vf = (Pmat @ v.reshape(-1, 3)).reshape(-1)
    want = (Pmat.T @ fine.tangent_host(state, vf).reshape(-1, 3)).reshape(-1)
    got = coarse.tangent_host(state, v)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"Pc={Pc} Pf={Pf} Q={Q} {which}: coarse tangent against I^T C I, relative max-norm error {err:.2e}")
    assert err <= 1e-12
    dc = coarse.diagonal_host(state)                                                           # and the coarse diagonal is this operator's
    i = 3 * int(coarse.faces[0, 0]) + 2
    e = np.zeros(dmc.lsize); e[i] = 1.0
    assert abs(coarse.tangent_host(state, e)[i] - dc[i]) <= 1e-12 * np.abs(dc).max()


@pytest.mark.parametrize("kind", ["plane", "ball", "cavity"])
def test_separated_everywhere_is_exactly_zero(oracle, kind):
    mesh = box_mesh(2, 2, 1)
    dm = build_dofmap(mesh, 2)
    cs = ContactSurface(oracle, mesh, dm, [1, 5], 4, portable=True)
    u = 0.1 * np.random.default_rng(2).uniform(-1, 1, dm.lsize)
    far = {"plane": dict(plane=((0, 0, -5.0), (0, 0, 1.0))), "ball": dict(sphere=((0.5, 0.5, -5.0), 1.0, 1)),
           "cavity": dict(sphere=((0.5, 0.5, 0.5), 50.0, -1))}[kind]
    cs.set_obstacle(penalty=3.0, **far)
    r, state = cs.residual_host(u)
    assert np.all(r == 0.0) and np.all(state[:, :6] == 0.0) and np.all(state[:, 6] > 0.0) and cs.energy_host(u) == 0.0
    y0 = np.random.default_rng(3).uniform(-1, 1, dm.lsize)
    Y, U, S = oracle.vector(dm.lsize).set_array(y0), oracle.vector(dm.lsize).set_array(u), cs.new_state()
    cs.residual_add(1.0, U, Y, S)
    cs.tangent_add(1.0, S, U, Y)
    cs.diagonal_add(1.0, S, Y)
    assert np.array_equal(Y.to_numpy(), y0)                                   # no row is touched: the same bits
    assert cs.active_fraction(S) == 0.0 and cs.min_gap(S) == state[:, 6].min() > 0


def test_mask_rows_unchanged_and_masked_variation_ignored(oracle):
    mesh = box_mesh(2, 2, 1)
    dm = build_dofmap(mesh, 2)
    mask = dirichlet_mask(dm, side_set_nodes(mesh, dm, [6])).copy()           # clamp x-: its edge with side 1 is masked
    mask[3 * side_set_nodes(mesh, dm, [1])[4] + 1] = 1                         # and one component of one more node
    m = mask != 0
    cs = ContactSurface(oracle, mesh, dm, [1], 4, mask=mask, portable=True)
    free = ContactSurface(oracle, mesh, dm, [1], 4, portable=True)
    u, du = ci.displacement(dm, 3, 4)
    kw = ci.set_obstacle(cs, "ball", u)
    free.set_obstacle(**kw)
    ci.input_condition(cs, u)
    (r, state), (r0, state0) = cs.residual_host(u), free.residual_host(u)
    assert np.array_equal(state, state0)                                       # the state knows no mask
    assert np.all(r[m] == 0.0) and np.array_equal(r[~m], r0[~m]) and np.abs(r0[m]).max() > 0
    t = cs.tangent_host(state, du)
    junk = du.copy(); junk[m] = 1e30
    assert np.array_equal(t, cs.tangent_host(state, junk)) and np.all(t[m] == 0.0)
    assert np.array_equal(t[~m], free.tangent_host(state, np.where(m, 0.0, du))[~m])
    d = cs.diagonal_host(state)
    assert np.all(d[m] == 0.0) and np.array_equal(d[~m], free.diagonal_host(state)[~m])
    y0 = np.random.default_rng(4).uniform(-1, 1, dm.lsize)
    Y, U, S = oracle.vector(dm.lsize).set_array(y0), oracle.vector(dm.lsize).set_array(u), cs.new_state()
    cs.residual_add(0.5, U, Y, S)
    y = Y.to_numpy()
    touched = y != y0
    on = np.zeros(dm.nnodes, dtype=bool); on[side_set_nodes(mesh, dm, [1])] = True
    assert touched.any() and not touched[m].any() and not touched[~np.repeat(on, 3)].any()
    assert np.allclose(y, y0 + 0.5 * r, rtol=0, atol=1e-15)
    assert np.array_equal(S.to_numpy()[:state.size], state.reshape(-1))       # never scaled
    assert cs.min_gap(S) == state[:, 6].min() < 0 and 0.1 <= cs.active_fraction(S) <= 0.9


def test_obstacle_refusals():
    for kw, msg in ((dict(plane=((0, 0, 0), (0, 0, 2.0))), "length 2, not 1"), (dict(plane=((0, 0, 0), (0, 0, 0))), "length 0, not 1"),
                    (dict(sphere=((0, 0, 0), 0.0, 1)), "radius 0 is not positive"), (dict(sphere=((0, 0, 0), 1.0, 2)), "neither \\+1"),
                    (dict(), "exactly one"), (dict(plane=((0, 0, 0), (0, 0, 1)), sphere=((0, 0, 0), 1.0, 1)), "exactly one")):
        with pytest.raises(ValueError, match=msg):
            obstacle_parameters(**kw)
