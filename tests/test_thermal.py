"""Thermal loads (thermal.py, body.LoadedBody(thermal=), postprocess.Stress(thermal=)) on the CPU oracle, where the portable NumPy form runs:
free expansions that are force-free on every row, the force as the derivative of the coupling energy and the tangent as the force's
(central differences with a bound derived from the step), the default path bit for bit, the load fraction, a bar's axial strain and the
refusals.  The closed-form bound is 10 x the error measured on the oracle (profiles/thermal.txt)."""
import numpy as np
import pytest

from _numbering import distorted_box
from ceedpetscsolid_amd import postprocess, thermal
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.postprocess import Stress
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG
from ceedpetscsolid_amd.thermal import ThermalLoad

NU, E, ALPHA, THETA = 0.3, 2.0, 1.5e-3, 40.0
FREE_TOL = 1e-12
# Measured on the oracle (profiles/thermal.txt, "closed form"): relative error of the bar's axial strain over its outer half.  The full
# clamp also holds the lateral expansion at x = 0; four p = 2 elements along the bar do not resolve how that dies out, and what is left
# of it at mid-length is this discretisation error.
KSP_RTOL = 1e-13
MEASURED_AXIAL = 1.38e-3


def problem(ceed, mesh, p, name, nu=NU, bc=()):
    return SolidProblem(ceed, mesh, p, name, nu=nu, E=E, multigrid="none", bc_sides=list(bc))


def internal_force(ceed, prob, u):
    n = prob.lsize()
    X, Y = ceed.vector(n).set_array(u), ceed.vector(n)
    prob.form_residual(X, Y)
    return X, Y.to_numpy()


def free_expansion_case(ceed, p):
    """linElas, uniform theta, u* = alpha theta X on a distorted 2 x 2 x 2 box: (problem, u*, theta)."""
    prob = problem(ceed, distorted_box(2, 2, 2), p, "linElas")
    X = prob.levels[prob.fine].dofmap.node_coords
    return prob, (ALPHA * THETA * X).reshape(-1), THETA


def linear_field_case(ceed, p):
    """theta = g y, u* = alpha g (x y, (y^2 - x^2 - z^2) / 2, y z) on the affine 2 x 2 x 2 box: strain alpha theta I at every point."""
    g = 25.0
    prob = problem(ceed, box_mesh(2, 2, 2), p, "linElas")
    x, y, z = prob.levels[prob.fine].dofmap.node_coords.T
    return prob, (ALPHA * g * np.stack([x * y, (y * y - x * x - z * z) / 2, y * z], axis=1)).reshape(-1), (lambda X: g * X[:, 1])


def hyperfs_case(ceed, p=2, s=0.05):
    """hyperFS, u = s X: theta* = [mu ((1 + s)^2 - 1) + lambda l] / beta makes P = 0, l the model's own series logarithm of J."""
    prob = problem(ceed, distorted_box(2, 2, 2), p, "hyperFS")
    two_mu = E / (1 + NU)
    lam = (3 * (E / (3 * (1 - 2 * NU))) - two_mu) / 3
    ell = float(postprocess._series4_shifted(np.array((1 + s) ** 6 - 1.0))) / 2          # the series of ln(J^2) = ln det C, halved
    beta = thermal.thermal_beta(NU, E, ALPHA)
    theta = (two_mu / 2 * ((1 + s) ** 2 - 1) + lam * ell) / beta
    return prob, (s * prob.levels[prob.fine].dofmap.node_coords).reshape(-1), theta, beta


def residual_error(ceed, prob, u, theta, name):
    """max |F_int(u) + R_theta(u)| / max |F_int(u)| over ALL rows: no Dirichlet set."""
    assert not np.any(prob.levels[prob.fine].mask)
    tl = ThermalLoad(prob, prob.fine, ALPHA, theta, name)
    X, fint = internal_force(ceed, prob, u)
    R = ceed.vector(prob.lsize()).set_array(fint)
    tl.force(X, R, add=True)
    err = np.abs(R.to_numpy()).max() / np.abs(fint).max()
    assert np.abs(fint).max() > 1e-3 * thermal.thermal_beta(NU, E, ALPHA) * 1.0
    tl.destroy()
    return err


@pytest.mark.parametrize("p", [1, 2, 3])
def test_free_expansion_is_force_free(oracle, p):
    prob, u, theta = free_expansion_case(oracle, p)
    err = residual_error(oracle, prob, u, theta, "linElas")
    print(f"free expansion, p = {p}: residual / F_int {err:.2e} (bound {FREE_TOL:.0e})")
    assert err <= FREE_TOL
    prob.destroy()


@pytest.mark.parametrize("p", [2, 3])
def test_linear_field_is_force_free(oracle, p):
    prob, u, theta = linear_field_case(oracle, p)
    err = residual_error(oracle, prob, u, theta, "linElas")
    print(f"linear field, p = {p}: residual / F_int {err:.2e} (bound {FREE_TOL:.0e})")
    assert err <= FREE_TOL
    prob.destroy()


def test_hyperfs_free_expansion(oracle):
    prob, u, theta, beta = hyperfs_case(oracle)
    err = residual_error(oracle, prob, u, theta, "hyperFS")
    st = Stress(prob, "hyperFS", thermal=dict(alpha=ALPHA, theta=theta))
    X = oracle.vector(prob.lsize()).set_array(u)
    serr = np.abs(st.points(X)).max() / (beta * theta)
    plain = Stress(prob, "hyperFS")
    assert np.abs(plain.points(X)).max() > 0.5 * beta * theta / 1.05 ** 3          # without the field the free expansion shows as stress
    print(f"hyperFS free expansion: residual / F_int {err:.2e}, stress / (beta theta) {serr:.2e} (bounds {FREE_TOL:.0e})")
    assert err <= FREE_TOL and serr <= FREE_TOL
    st.destroy(); plain.destroy(); prob.destroy()


# ---- the force is the energy's derivative, the tangent the force's ---------------------------------------------------------------------
FD_STEP = 1e-4


def fd_case(ceed):
    prob = problem(ceed, distorted_box(2, 2, 1), 2, "hyperFS")
    X = prob.levels[prob.fine].dofmap.node_coords
    rng = np.random.default_rng(4)
    theta = 30.0 * (1 + 0.5 * np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.3 * X[:, 2])
    tl = ThermalLoad(prob, prob.fine, ALPHA, theta, "hyperFS", portable=True)
    n = prob.lsize()
    return prob, tl, 1e-2 * rng.uniform(-1, 1, n), rng


def test_force_is_the_energy_derivative_and_tangent_the_force_derivative(oracle):
    """Central differences with the step h = FD_STEP along a direction d (nodal values in [-1, 1]), B = F^-1 grad d at the points.
    Energy: d^3/dh^3 ln det(F + h grad d) = 2 tr B^3, so |FD - f . d| <= h^2 / 3 sum_q w |beta theta| |B|^3.  Force, contracted with a
    second direction v: d^3/dh^3 F^-T = -6 (F^-T grad d^T)^3 F^-T, so |FD - v . T d| <= h^2 sum_q w |beta theta| |B|^3 |F^-1| |grad v|
    (Frobenius norms).  Both bounds are doubled for the next term of the series (h |B| < 1e-2) and carry the rounding of the difference
    quotient, 2^-52 / h times the sum of the magnitudes of the summed terms."""
    prob, tl, u, rng = fd_case(oracle)
    h, eps = FD_STEP, 2.0 ** -52
    W = tl._tables()[2]
    wbt = W * np.abs(tl.beta * tl.theta_points())
    Finv = np.linalg.inv(tl.grad_host(u) + np.eye(3))
    fro = lambda M: np.sqrt((M * M).sum(axis=(-1, -2)))
    worst_e = worst_t = 0.0
    for _ in range(4):
        d, v = rng.uniform(-1, 1, u.size), rng.uniform(-1, 1, u.size)
        B = Finv @ tl.grad_host(d)
        assert h * fro(B).max() < 1e-2
        fd = (tl.energy_host(u + h * d) - tl.energy_host(u - h * d)) / (2 * h)
        got = tl.force_host(u) @ d
        lnJ = np.abs(np.log(np.linalg.det(tl.grad_host(u) + np.eye(3))))
        bound = 2 * h * h / 3 * np.sum(wbt * fro(B) ** 3) + 8 * eps / h * np.sum(wbt * (lnJ + h * fro(B)))
        print(f"energy -> force: |FD - f.d| {abs(fd - got):.2e}, bound {bound:.2e}, f.d {got:.3e}")
        assert abs(fd - got) <= bound
        worst_e = max(worst_e, abs(fd - got) / bound)
        fd = v @ (tl.force_host(u + h * d) - tl.force_host(u - h * d)) / (2 * h)
        got = v @ tl.tangent_host(u, d)
        gv = fro(tl.grad_host(v))
        bound = 2 * h * h * np.sum(wbt * fro(B) ** 3 * fro(Finv) * gv) + 8 * eps / h * np.sum(wbt * fro(Finv) * gv)
        print(f"force -> tangent: |FD - v.Td| {abs(fd - got):.2e}, bound {bound:.2e}, v.Td {got:.3e}")
        assert abs(fd - got) <= bound
        worst_t = max(worst_t, abs(fd - got) / bound)
    print(f"largest error / bound: energy {worst_e:.2e}, tangent {worst_t:.2e}")
    tl.destroy(); prob.destroy()


def test_tangent_is_symmetric_on_a_dense_column_sweep(oracle):
    prob, tl, u, _ = fd_case(oracle)
    n = u.size
    T = np.stack([tl.tangent_host(u, np.eye(n)[j]) for j in range(n)], axis=1)
    asym = np.abs(T - T.T).max()
    print(f"|T - T^T| {asym:.2e} with |T| {np.abs(T).max():.2e} on {n} columns")
    assert np.abs(T).max() > 1e-3 and asym <= 1e-12
    tl.destroy(); prob.destroy()


# ---- the solvers ------------------------------------------------------------------------------------------------------------------------
L_BAR, W_BAR = 2.0, 0.2


def bar(ceed, name, nu=0.0, p=2, nx=4):
    return SolidProblem(ceed, box_mesh(nx, 1, 1, lo=(0.0, -W_BAR / 2, -W_BAR / 2), hi=(L_BAR, W_BAR / 2, W_BAR / 2)), p, name, nu=nu, E=E,
                        bc_sides=[6])


def axial_strain(prob, sol):
    """(u_x(L) - u_x(L / 2)) / (L / 2), means over the two cross-sections: the clamp's lateral restraint has died out there."""
    X = prob.levels[prob.fine].dofmap.node_coords
    u = sol.U.to_numpy()[:3 * len(X)].reshape(-1, 3)
    at = lambda x: u[np.abs(X[:, 0] - x) < 1e-12, 0].mean()
    return (at(L_BAR) - at(L_BAR / 2)) / (L_BAR / 2)


def evaluate(sol, u, dx):
    """(R(u), A_outer dx) of a solver at its current load."""
    n = sol.p.lsize()
    U, R, D, Y = (sol.ceed.vector(n) for _ in range(4))
    U.set_array(u * sol.free); D.set_array(dx * sol.free)
    sol._set(sol.bcv, sol.bc_values(sol.load))
    sol.residual(U, R)
    sol.A_outer(sol.nlev - 1, D, Y)
    return R.to_numpy(), Y.to_numpy()


@pytest.mark.parametrize("name", ["linElas", "hyperFS"])
def test_default_keeps_its_bits_and_makes_no_thermal_operator(oracle, monkeypatch, name):
    prob = bar(oracle, name, nu=NU)
    rng = np.random.default_rng(8)
    u, dx = 1e-2 * rng.uniform(-1, 1, prob.lsize()), rng.uniform(-1, 1, prob.lsize())
    a = NewtonPMG(prob)
    ra, ya = evaluate(a, u, dx)

    def refuse(*args, **kw):
        raise AssertionError("a thermal operator was made without thermal=")
    monkeypatch.setattr(ThermalLoad, "__init__", refuse)
    b = NewtonPMG(prob, thermal=None)
    rb, yb = evaluate(b, u, dx)
    assert b.thermal is None and not b.thermal_follows and not b.has_followers()
    assert np.array_equal(ra, rb) and np.array_equal(ya, yb)
    X = oracle.vector(prob.lsize()).set_array(u)
    s0, s1 = Stress(prob, name), Stress(prob, name, thermal=None)
    assert s1.thermal is None
    assert np.array_equal(s0.points(X), s1.points(X)) and np.array_equal(s0.nodal(X), s1.nodal(X))
    for o in (a, b, s0, s1):
        o.destroy()
    prob.destroy()


@pytest.mark.parametrize("name", ["linElas", "hyperSS", "hyperFS"])
def test_half_the_load_is_half_the_temperature(oracle, name):
    prob = bar(oracle, name, nu=NU)
    rng = np.random.default_rng(9)
    u, dx = 1e-2 * rng.uniform(-1, 1, prob.lsize()), rng.uniform(-1, 1, prob.lsize())
    theta = lambda X: THETA * (1 + X[:, 1] / W_BAR)
    a = NewtonPMG(prob, thermal=dict(alpha=ALPHA, theta=theta))
    b = NewtonPMG(prob, thermal=dict(alpha=ALPHA, theta=lambda X: theta(X) / 2))
    plain = NewtonPMG(prob)
    a.load = 0.5
    (ra, ya), (rb, yb), (r0, y0) = evaluate(a, u, dx), evaluate(b, u, dx), evaluate(plain, u, dx)
    assert a.has_followers() == (name == "hyperFS") == b.has_followers()
    scale = np.abs(rb - r0).max()
    assert scale > 1e-4 and np.abs(ra - rb).max() <= 1e-13 * max(scale, np.abs(rb).max())
    assert np.abs(ya - yb).max() <= 1e-13 * np.abs(yb).max()
    if name == "hyperFS":                                                      # the tangent is in A_outer, and "none" leaves it out
        assert np.abs(yb - y0).max() > 1e-6 * np.abs(y0).max()
        c = NewtonPMG(prob, thermal=dict(alpha=ALPHA, theta=theta, tangent="none"))
        rc, yc = evaluate(c, u, dx)
        assert np.array_equal(yc, y0) and np.abs(rc - r0).max() > 1e-4
        c.destroy()
    else:
        assert np.array_equal(yb, y0)
    for o in (a, b, plain):
        o.destroy()
    assert a.thermal is None
    prob.destroy()


def solve_bar(ceed, **kw):
    prob = bar(ceed, "linElas")
    sol = NewtonPMG(prob, ksp_rtol=KSP_RTOL, snes_rtol=1e-12, thermal=dict(alpha=ALPHA, theta=THETA), **kw)
    sol.solve(num_increments=1)
    return prob, sol


def test_axial_strain_of_a_heated_bar(oracle):
    """linElas, nu = 0, uniform theta, clamped at x = 0: away from the clamp the bar grows by alpha theta per unit length."""
    prob, sol = solve_bar(oracle)
    err = abs(axial_strain(prob, sol) - ALPHA * THETA) / (ALPHA * THETA)
    print(f"heated bar: axial strain {axial_strain(prob, sol):.15e}  closed form {ALPHA * THETA:.15e}  relative error {err:.2e}")
    assert err <= 10 * MEASURED_AXIAL
    sol.destroy(); prob.destroy()


def test_refusals(oracle):
    prob = bar(oracle, "linElas")
    nn = prob.levels[prob.fine].dofmap.nnodes

    class TwoRanks:
        world = 2
    with pytest.raises(ValueError, match="several ranks"):
        NewtonPMG(prob, halo=TwoRanks(), thermal=dict(alpha=ALPHA, theta=THETA))
    with pytest.raises(ValueError, match="alpha must be finite"):
        NewtonPMG(prob, thermal=dict(alpha=np.nan, theta=THETA))
    with pytest.raises(ValueError, match="alpha must be finite"):
        ThermalLoad(prob, prob.fine, np.inf, THETA, "linElas")
    with pytest.raises(ValueError, match="theta has shape"):
        NewtonPMG(prob, thermal=dict(alpha=ALPHA, theta=np.ones(nn - 1)))
    with pytest.raises(ValueError, match="theta is not finite"):
        NewtonPMG(prob, thermal=dict(alpha=ALPHA, theta=np.full(nn, np.nan)))
    with pytest.raises(ValueError, match="tangent must be 'full' or 'none'"):
        NewtonPMG(prob, thermal=dict(alpha=ALPHA, theta=THETA, tangent="levels"))
    with pytest.raises(ValueError, match="dict\\(alpha=, theta=, tangent='full'\\) expected"):
        NewtonPMG(prob, thermal=dict(alpha=ALPHA))
    with pytest.raises(ValueError, match="thermal is a thermal.ThermalLoad or dict"):
        Stress(prob, "linElas", thermal=dict(alpha=ALPHA))
    tl = ThermalLoad(prob, prob.fine, ALPHA, THETA, "linElas")
    n = prob.lsize()
    with pytest.raises(ValueError, match="ThermalTangent: the thermal load of linElas is dead and has no tangent"):
        tl.tangent(oracle.vector(n).set_value(0.0), oracle.vector(n).set_value(0.0), oracle.vector(n))
    tl.destroy(); prob.destroy()
