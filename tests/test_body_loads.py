"""Body loads of body.LoadedBody through solver.NewtonPMG on the CPU oracle: gravity, a nodal acceleration field and the centrifugal
load of a spinning body, dead and following, against the hand-made load vector, closed forms of a bar (linElas, nu = 0, axial load)
and a central difference of the follower.

The bounds of the closed-form solves are 10 x the error measured on the oracle (profiles/mass_field.txt, "closed forms"): one decade
for the Krylov stopping point varying between backends."""
import numpy as np
import pytest

from ceedpetscsolid_amd import mass as mass_module
from ceedpetscsolid_amd.mass import DensityField, MassOperator
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG

E, RHO, G, L = 50.0, 2.0, 3.0, 2.0
W = 0.05                                                                # the bar's width: thin, so that a lateral load hardly bends it
KSP_RTOL = 1e-13
# Measured on the oracle (profiles/mass_field.txt): relative error of the tip displacement against the closed form.  The two solves
# that are exact in the space came out at 1.2e-16 and 6.9e-16, below the relative residual the Krylov iteration stops at; what a
# backend may differ by is that stopping point, so their figure is floored at it.
MEASURED = {"hanging": max(1.2e-16, KSP_RTOL), "graded": max(6.9e-16, KSP_RTOL), "dead_spin": 9.1e-9, "follower_spin": 6.9e-9}


def bar(ceed, p, nx):
    """A bar 0 <= x <= L of width W centred on the x axis, clamped at x = 0 (side set 6)."""
    return SolidProblem(ceed, box_mesh(nx, 1, 1, lo=(0.0, -W / 2, -W / 2), hi=(L, W / 2, W / 2)), p, "linElas", nu=0.0, E=E, bc_sides=[6])


def tip(prob, sol):
    X = prob.levels[prob.fine].dofmap.node_coords
    u = sol.U.to_numpy()[:3 * len(X)].reshape(-1, 3)
    return u[np.abs(X[:, 0] - L) < 1e-12, 0].mean()


def solve(prob, **kw):
    sol = NewtonPMG(prob, ksp_rtol=KSP_RTOL, snes_rtol=1e-12, **kw)
    sol.solve(num_increments=1)
    return sol


def test_gravity_is_the_hand_made_load_bitwise_and_sums_to_the_weight(oracle):
    prob = bar(oracle, 2, 3)
    n = prob.lsize()
    g = np.array([0.3, -0.2, -G])
    sol = NewtonPMG(prob, density=RHO, gravity=g)
    m = MassOperator(prob, prob.fine, RHO, mask_mode=2)
    Xv, Y = oracle.vector(n).set_array(np.tile(g, n // 3)), oracle.vector(n)
    m.apply(Xv, Y)
    assert np.array_equal(sol.fv.to_numpy(), Y.to_numpy())
    # the whole weight: the rows the clamp drops included (apply_host drops none)
    w = m.apply_host(np.tile(g, n // 3)).reshape(-1, 3).sum(axis=0)
    assert np.abs(w - RHO * L * W * W * g).max() <= 1e-13 * RHO * L * W * W * G
    # a field that is constant gives the same load to rounding, and forcing= is added to, not replaced
    f0 = np.random.default_rng(0).uniform(-1, 1, n)
    sol2 = NewtonPMG(prob, density=DensityField.per_element(np.full(3, RHO)), gravity=g, forcing=f0)
    want = f0 * sol.free + Y.to_numpy()
    assert np.abs(sol2.fv.to_numpy() - want).max() <= 1e-13 * np.abs(want).max()
    # an acceleration field that is constant is gravity
    sol3 = NewtonPMG(prob, density=RHO, acceleration_field=lambda X: np.tile(g, (len(X), 1)))
    assert np.array_equal(sol3.fv.to_numpy(), Y.to_numpy())
    for s in (sol, sol2, sol3):
        s.destroy()
    prob.destroy()


def test_hanging_bar(oracle):
    """u(L) = rho g L^2 / (2 E): quadratic, in the space at p = 2."""
    prob = bar(oracle, 2, 2)
    sol = solve(prob, density=RHO, gravity=(G, 0.0, 0.0))
    exact = RHO * G * L * L / (2 * E)
    err = abs(tip(prob, sol) - exact) / exact
    print(f"hanging bar: tip {tip(prob, sol):.15e}  closed form {exact:.15e}  relative error {err:.2e}")
    assert err <= 10 * MEASURED["hanging"]
    sol.destroy(); prob.destroy()


def test_graded_bar(oracle):
    """rho = rho0 (1 + x / L): u(L) = 5 rho0 g L^2 / (6 E), cubic, in the space at p = 3."""
    prob = bar(oracle, 3, 2)
    sol = solve(prob, density=DensityField.nodal(lambda X: RHO * (1 + X[:, 0] / L)), gravity=(G, 0.0, 0.0))
    exact = 5 * RHO * G * L * L / (6 * E)
    err = abs(tip(prob, sol) - exact) / exact
    print(f"graded bar: tip {tip(prob, sol):.15e}  closed form {exact:.15e}  relative error {err:.2e}")
    assert err <= 10 * MEASURED["graded"]
    sol.destroy(); prob.destroy()


OMEGA_DEAD = 1.5


def test_dead_spin(oracle):
    """Spin about the y axis through the origin, follow=False: the axial load rho Omega^2 x gives u(L) = rho Omega^2 L^3 / (3 E) at
    p = 3; the lateral part rho Omega^2 z acts on a thin bar (width W) and the clamp, which holds the lateral displacement too, couples
    it to the axial one only near x = 0: the measured error carries that."""
    prob = bar(oracle, 3, 2)
    sol = solve(prob, density=RHO, spin=dict(omega=OMEGA_DEAD, axis=(0, 1, 0), follow=False))
    assert not sol.has_followers() and sol.spin is None
    exact = RHO * OMEGA_DEAD ** 2 * L ** 3 / (3 * E)
    err = abs(tip(prob, sol) - exact) / exact
    print(f"dead spin: tip {tip(prob, sol):.15e}  closed form {exact:.15e}  relative error {err:.2e}")
    assert err <= 10 * MEASURED["dead_spin"]
    sol.destroy(); prob.destroy()


def follower_case():
    k = 0.5 / L                                                         # k L = 0.5
    return k * np.sqrt(E / RHO), np.sin(k * L) / (k * np.cos(k * L)) - L


def test_follower_spin(oracle):
    """E u'' + rho Omega^2 (x + u) = 0, u(0) = 0, u'(L) = 0: u(L) = sin(kL) / (k cos kL) - L, k = Omega sqrt(rho / E); p = 4 on 2
    elements at k L = 0.5."""
    prob = bar(oracle, 4, 2)
    omega, exact = follower_case()
    sol = solve(prob, density=RHO, spin=dict(omega=omega, axis=(0, 1, 0)))
    assert sol.has_followers()
    err = abs(tip(prob, sol) - exact) / exact
    dead = RHO * omega ** 2 * L ** 3 / (3 * E)
    print(f"follower spin: tip {tip(prob, sol):.15e}  closed form {exact:.15e}  relative error {err:.2e}  (dead load alone {dead:.6e})")
    assert err <= 10 * MEASURED["follower_spin"]
    assert abs(dead - exact) / exact > 0.05                                # the follower part is what is tested
    sol.destroy(); prob.destroy()


def test_spin_tangent_is_the_central_difference_of_the_follower_and_symmetric(oracle):
    prob = bar(oracle, 2, 2)
    n = prob.lsize()
    sol = NewtonPMG(prob, density=DensityField.per_element([1.0, 3.0]), spin=dict(omega=0.7, axis=(1, 2, 3), origin=(0.1, 0.0, 0.2)))
    sol.load = 0.75
    free = sol.free
    rng = np.random.default_rng(4)
    x, dx, dy = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n) * free, rng.uniform(-1, 1, n) * free
    vec = lambda a: oracle.vector(n).set_array(a)

    def follower(xx):
        R = oracle.vector(n).set_value(0.0)
        sol.follower_add(vec(xx), R)
        return R.to_numpy()
    h = 0.5
    fd = (follower(x + h * dx) - follower(x - h * dx)) / (2 * h)
    T = {}
    for name, d in (("dx", dx), ("dy", dy)):
        Y = oracle.vector(n).set_value(0.0)
        sol.spin_tangent_add(vec(d), Y)
        T[name] = Y.to_numpy()
    assert np.abs(T["dx"]).max() > 0 and np.all(T["dx"][~free] == 0.0)
    assert np.abs(fd - T["dx"]).max() <= 1e-13 * np.abs(T["dx"]).max()
    a, b = dy @ T["dx"], dx @ T["dy"]
    assert abs(a - b) <= 1e-13 * max(abs(a), abs(b))
    assert dx @ T["dx"] < 0.0                                               # negative semi-definite: the spin softening
    # A_outer carries it, A does not
    YA, YO = oracle.vector(n), oracle.vector(n)
    sol.residual(sol.U, sol.R)
    sol.A(sol.nlev - 1, vec(dx), YA); sol.A_outer(sol.nlev - 1, vec(dx), YO)
    assert np.abs((YO.to_numpy() - YA.to_numpy()) - T["dx"]).max() <= 1e-12 * np.abs(YA.to_numpy()).max()
    sol.destroy()
    none = NewtonPMG(prob, density=1.0, spin=dict(omega=0.7, tangent="none"))
    Y = oracle.vector(n).set_value(0.0)
    none.spin_tangent_add(vec(dx), Y)
    assert np.all(Y.to_numpy() == 0.0) and none.has_followers()
    none.destroy(); prob.destroy()


def test_load_increments_scale_the_body_loads(oracle):
    prob = bar(oracle, 2, 2)
    omega, _ = follower_case()
    kw = dict(density=RHO, gravity=(G, 0.0, 0.0), spin=dict(omega=omega, axis=(0, 1, 0)), ksp_rtol=1e-13, snes_rtol=1e-12)
    one, two, half = NewtonPMG(prob, **kw), NewtonPMG(prob, **kw), NewtonPMG(prob, **kw)
    one.solve(num_increments=1); two.solve(num_increments=2); half.solve(num_increments=2, stop_after=1)
    u1, u2, uh = one.U.to_numpy(), two.U.to_numpy(), half.U.to_numpy()
    assert np.abs(u2 - u1).max() <= 1e-9 * np.abs(u1).max()
    # at half the load both the dead and the follower part are halved: (K - l S) u = l f is not linear in l, so u(1/2) != u(1) / 2
    assert 1e-4 < np.abs(2 * uh - u1).max() / np.abs(u1).max() < 0.2
    for s in (one, two, half):
        s.destroy()
    prob.destroy()


def test_no_mass_operator_without_a_keyword(oracle, monkeypatch):
    made = []
    init = MassOperator.__init__
    monkeypatch.setattr(mass_module.MassOperator, "__init__", lambda self, *a, **k: (made.append(1), init(self, *a, **k))[1])
    prob = bar(oracle, 2, 2)
    sol = NewtonPMG(prob, forcing=np.ones(prob.lsize()))
    assert not made and sol.body_mass is None and sol.spin is None and not sol.has_followers()
    sol.destroy()
    sol = NewtonPMG(prob, density=RHO)                                      # a density alone asks for no load
    assert not made and sol.body_mass is None and sol.fv is None
    sol.destroy()
    sol = NewtonPMG(prob, density=RHO, gravity=(0, 0, -1))
    assert len(made) == 1
    sol.destroy(); prob.destroy()


def test_refusals(oracle):
    prob = bar(oracle, 2, 2)
    nn = prob.levels[prob.fine].dofmap.nnodes
    for kw in (dict(gravity=(0, 0, -1)), dict(acceleration_field=np.zeros((nn, 3))), dict(spin=dict(omega=1.0))):
        with pytest.raises(ValueError, match="need density="):
            NewtonPMG(prob, **kw)
    for bad in (0.0, -1.0, float("nan"), "steel"):
        with pytest.raises(ValueError, match="density must be a positive float or a mass.DensityField"):
            NewtonPMG(prob, density=bad, gravity=(0, 0, -1))
    for g in ((0, 0), (0, 0, float("inf"))):
        with pytest.raises(ValueError, match="gravity: three finite components"):
            NewtonPMG(prob, density=1.0, gravity=g)
    with pytest.raises(ValueError, match="acceleration_field: a finite array of shape"):
        NewtonPMG(prob, density=1.0, acceleration_field=np.zeros((nn, 2)))
    for spin in (dict(axis=(0, 0, 1)), dict(omega=1.0, speed=2), dict(omega=1.0, axis=(0, 0, 0)), dict(omega=float("nan")), 3.0):
        with pytest.raises(ValueError, match="spin: "):
            NewtonPMG(prob, density=1.0, spin=spin)
    with pytest.raises(ValueError, match="tangent must be 'full' or 'none'"):
        NewtonPMG(prob, density=1.0, spin=dict(omega=1.0, tangent="levels"))
    prob.destroy()
