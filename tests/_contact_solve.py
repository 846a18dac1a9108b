"""The solves the contact solve tests share (CPU oracle with the portable form, device with the library's kernels).

Closed form: box_mesh(2, 2, 1) (height H = 1), linElas, nu = 0, E = 1, degree 2.  The top (side 2) is clamped and translated by
(0, 0, -delta); the bottom (side 1) meets the rigid plane z = -g0, n = (0, 0, 1), penalty eps.  The exact solution is uniaxial and linear
in z, so it lies in the FE space: with k = E / H the bottom penetrates by pen = k (delta - g0) / (eps + k),
u_z(z) = -(g0 + pen) + (z / H) (g0 + pen - delta), u_x = u_y = 0, and the smallest gap is -pen.  With delta < g0 nothing touches and the
body translates rigidly."""
import numpy as np

from ceedpetscsolid_amd.contact import ContactSurface
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG

DELTA, G0, EPS, E, HEIGHT = 0.05, 0.02, 10.0, 1.0, 1.0
PEN = (E / HEIGHT) * (DELTA - G0) / (EPS + E / HEIGHT)
SNES_RTOL = 1e-10
TOL = 1e-7 * DELTA


def total_displacement(s):
    """Free part of the solution plus the boundary values of the last increment."""
    return s.U.to_numpy() + s.bcv.to_numpy()


def closed_form_problem(ceed):
    return SolidProblem(ceed, box_mesh(2, 2, 1), 2, "linElas", nu=0.0, E=E, bc_sides=[2])


def closed_form_solver(prob, delta=DELTA, contact=True, **kw):
    kw.setdefault("snes_rtol", SNES_RTOL)
    con = {1: dict(plane=((0.0, 0.0, -G0), (0.0, 0.0, 1.0)), penalty=EPS)} if contact else None
    return NewtonPMG(prob, clamp={2: dict(translate=(0.0, 0.0, -delta))}, contact=con, **kw)


def check_closed_form(prob, s, st, label):
    """The pressed case against its exact solution, to 1e-7 delta."""
    assert st.converged
    u = total_displacement(s).reshape(-1, 3)
    z = prob.levels[prob.fine].dofmap.node_coords[:, 2]
    want = -(G0 + PEN) + (z / HEIGHT) * (G0 + PEN - DELTA)
    ez, exy, eg = np.abs(u[:, 2] - want).max(), np.abs(u[:, :2]).max(), abs(s.min_gap() + PEN)
    print(f"{label}: {st.newton_its} Newton / {st.ksp_its} Krylov its; errors u_z {ez:.2e}, u_xy {exy:.2e}, min gap {eg:.2e} "
          f"(bound {TOL:.1e}); pen = {PEN:.6e}, active {s.active_fraction():.2f}")
    assert ez <= TOL and exy <= TOL and eg <= TOL
    assert s.active_fraction() == 1.0
    return st.ksp_its


def check_separated(prob, s, st, label):
    """delta = 0.01 < g0: the rigid translation, nothing active, and the same bits as the solve without contact."""
    delta = 0.01
    assert st.converged
    u = total_displacement(s).reshape(-1, 3)
    ez, exy = np.abs(u[:, 2] + delta).max(), np.abs(u[:, :2]).max()
    print(f"{label}: {st.newton_its} Newton / {st.ksp_its} Krylov its; errors u_z {ez:.2e}, u_xy {exy:.2e}; min gap {s.min_gap():.6e}")
    assert ez <= 1e-7 * delta and exy <= 1e-7 * delta
    assert s.active_fraction() == 0.0 and abs(s.min_gap() - (G0 - delta)) <= 1e-7 * delta
    for c in s.contacts:
        assert np.all(c["state"].to_numpy().reshape(-1, 7, prob.Q ** 2)[:, :6] == 0.0)      # K = 0: the tangent and the diagonal add zeros


def indentation(ceed, contact_tangent="levels", increments=3, **kw):
    """hyperFS: a rigid ball of radius 1, its axis a little off the centre, pressed 0.08 into the top of the clamped unit cube (2 x 2 x 2 elements, degree 2) over the
    load increments.  Returns (prob, solver, stats, figures of the final state)."""
    prob = SolidProblem(ceed, box_mesh(2, 2, 2), 2, "hyperFS", nu=0.3, E=E, bc_sides=[1])
    eps, R, depth = 20.0, 1.0, 0.08
    s = NewtonPMG(prob, contact={2: dict(sphere=((0.45, 0.55, 1.0 + R), R, 1), penalty=eps, travel=(0.0, 0.0, -depth))},
                  contact_tangent=contact_tangent, snes_rtol=1e-8, **kw)
    st = s.solve(num_increments=increments)
    lv = prob.levels[prob.fine]
    ref = ContactSurface(ceed, prob.mesh, lv.dofmap, [2], prob.Q, mask=lv.mask, portable=True)
    ref.set_obstacle(sphere=((0.45, 0.55, 1.0 + R - depth), R, 1), penalty=eps)
    wJ, g, n, _ = ref._points(total_displacement(s))
    pen = np.maximum(-g, 0.0)
    fig = dict(eps=eps, depth=depth, R=R, min_gap=s.min_gap(), active=s.active_fraction(), area=float(wJ[g < 0].sum()),
               force=eps * float((wJ * pen).sum()),                         # int eps <-g> dA0: the sum of the point forces' magnitudes
               force_z=eps * float((wJ * pen * n[..., 2]).sum()),           # the resultant the ball exerts along -z
               portable_min_gap=float(g.min()))
    return prob, s, st, fig
