"""Frictionless penalty contact of side sets with a rigid analytic obstacle: a plane or a sphere.

The contact surface Gamma is a union of element faces named by side-set ids; the faces, their node order and their Gauss points are those
of ``surface.py`` (``mesh.side_set_faces``, ``portable.lagrange_tables``).  The obstacle is a signed distance g(x), g > 0 meaning
separated, with n = grad g:

    plane    g = (x - x0) . n          n the unit normal pointing from the obstacle to the body;  grad grad g = 0
    sphere   g = s (|x - c| - R)       s = +1 a body outside a ball, s = -1 a body inside a spherical cavity
             n = s (x - c) / |x - c|   grad grad g = s (I - n (x) n) / |x - c|

The obstacle may translate with the load fraction (``body.LoadedBody``: x0 or c at load l is x0 + l travel).  The penalty eps is per
unit REFERENCE area, so the term has a potential and an exactly symmetric tangent.  With x = X + u, <a> = max(a, 0), H the step function:

    Pi(u)       = int_Gamma0 1/2 eps <-g(x)>^2 dA0
    r_a(u)      = d Pi / d u_a = -int N_a eps <-g> n dA0                       added to R = F_int - ...
    C(u) du |_a = int N_a K_q (sum_b N_b du_b),     K_q = w_q J_q eps [H(-g) n (x) n - <-g> grad grad g]

integrated on the fine level's Q x Q Gauss points, J = |X_xi x X_eta|.  The residual evaluation writes the CONTACT STATE, a vector
[face][7][Q^2]: per point the six entries of K_q in the order (xx, yy, zz, yz, xz, xy) -- w J eps is inside them -- and the gap g.  The
tangent and the diagonal at ANY p-level are B^T K_q B with that level's (P_level, Q_fine) tables on this one state: a coarse level needs
no obstacle, no geometry and no coarse displacement, and because the p-spaces are nested on the same mesh its contact tangent equals the
Galerkin product P^T C_fine P on the free dofs.  The diagonal is d_{a,c} = sum_q B_a(q)^2 K_q[c][c] (squared tables).

On the device these are the library's CeedXContact* entry points (include/ceed_contact.h, csrc/kernels_contact.hip).  Where the library
lacks them (the CPU oracle), or with ``portable=True``, the same sums are formed in NumPy on the tensor layer of ``portable.py``.

Out of scope: friction, deformable-deformable contact, augmented Lagrangian updates, several ranks, dynamics.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import ceed as cd
from . import portable as pt
from .mesh import DofMap, HexMesh
from .surface import FaceTerm

NSTATE = cd.CONTACT_NSTATE
_SYM = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))            # the six stored entries of K: xx, yy, zz, yz, xz, xy


def obstacle_parameters(plane=None, sphere=None):
    """(kind, the eight parameters of CeedXContactSetObstacle) of ``plane=(x0, n)`` or ``sphere=(c, R, s)``; what the library refuses
    is refused here with the same words (ValueError)."""
    if (plane is None) == (sphere is None):
        raise ValueError("contact obstacle: give exactly one of plane=(x0, n) and sphere=(c, R, s)")
    par = np.zeros(8)
    if plane is not None:
        x0, n = (np.asarray(v, dtype=np.float64).reshape(-1) for v in plane)
        if x0.size != 3 or n.size != 3:
            raise ValueError("contact plane: x0 and n have three components")
        if not abs(np.sqrt(np.square(n).sum()) - 1.0) <= 1e-12:
            raise ValueError(f"contact plane: the plane normal has length {np.sqrt(np.square(n).sum()):g}, not 1")
        par[:3], par[3:6] = x0, n
        return cd.CONTACT_PLANE, par
    c, R, s = sphere
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    if c.size != 3:
        raise ValueError("contact sphere: c has three components")
    if not float(R) > 0.0:
        raise ValueError(f"contact sphere: the sphere radius {float(R):g} is not positive")
    if float(s) not in (1.0, -1.0):
        raise ValueError(f"contact sphere: the sphere side s = {float(s):g} is neither +1 (ball) nor -1 (cavity)")
    par[:3], par[3], par[4] = c, float(R), float(s)
    return cd.CONTACT_SPHERE, par


class ContactSurface(FaceTerm):
    """The contact term of the faces of ``side_ids`` (surface.FaceTerm).  ``Q``: Gauss points per direction, the FINE level's on every
    level.  The state is a vector of the Ceed with ``state_size`` entries (``new_state``); a coarse level's surface takes the one its
    fine level's residual wrote."""
    HANDLE = cd.ContactHandle

    def __init__(self, ceed: cd.Ceed, mesh: HexMesh, dm: DofMap, side_ids, Q: int, mask=None, portable: bool = False):
        super().__init__(ceed, mesh, dm, side_ids, Q, mask, portable)
        self.state_size = self.nface * NSTATE * self.Q ** 2
        self.kind = self.par = self.penalty = None

    def set_obstacle(self, plane=None, sphere=None, penalty: float = 1.0):
        """The obstacle and the penalty eps > 0 of the residual evaluations that follow."""
        kind, par = obstacle_parameters(plane, sphere)
        if not (float(penalty) > 0.0 and np.isfinite(penalty)):
            raise ValueError(f"contact: the penalty {float(penalty):g} is not positive")
        self.kind, self.par, self.penalty = kind, par, float(penalty)
        if self.handle is not None:
            self.handle.set_obstacle(kind, par, self.penalty)

    def new_state(self) -> cd.Vector:
        """A zeroed state vector (no point active, every gap 0); the caller destroys it."""
        return self.ceed.vector(max(self.state_size, 1)).set_value(0.0)

    # ---- the portable form: NumPy on host arrays ---------------------------------------------------------------------------
    def _points(self, u):
        """(w J, g, n, h) at the points [face][b][a]: the weighted reference area element, the gap, n = grad g and the factor of
        grad grad g = h (I - n (x) n)."""
        if self.kind is None:
            raise ValueError("contact: no obstacle set (set_obstacle)")
        Xa, Xb = self._derivs(self.Xh)
        x = pt.to_points(self._gather(self.Xh) + self._gather(u), self.B, self.B)
        wJ = np.linalg.norm(np.cross(Xa, Xb), axis=-1) * (self.w[:, None] * self.w[None, :])[None]
        if self.kind == cd.CONTACT_PLANE:
            n = np.broadcast_to(self.par[3:6], x.shape)
            g = np.einsum("fbac,c->fba", x - self.par[:3], self.par[3:6])
            h = np.zeros_like(g)
        else:
            d, R, s = x - self.par[:3], self.par[3], self.par[4]
            r = np.sqrt(np.square(d).sum(axis=-1))
            with np.errstate(divide="ignore"):
                rinv = np.where(r > 0.0, 1.0 / r, 0.0)
            n, g, h = s * d * rinv[..., None], s * (r - R), s * rinv
        return wJ, g, n, h

    def gap_host(self, u) -> np.ndarray:
        """g at the points, [face][Q^2] (xi fastest)."""
        return self._points(u)[1].reshape(self.nface, -1)

    def energy_host(self, u) -> float:
        """Pi(u)."""
        wJ, g, _, _ = self._points(u)
        return float(0.5 * self.penalty * (wJ * np.square(np.maximum(-g, 0.0))).sum())

    def residual_host(self, u):
        """(r(u) as an L-vector, the state [face][7][Q^2])."""
        wJ, g, n, h = self._points(u)
        pen, act = np.maximum(-g, 0.0), (g < 0.0).astype(np.float64)
        wje = wJ * self.penalty
        k0 = wje * pen * h
        k1 = act * wje + k0                                                # K = k1 n (x) n - k0 I
        state = np.empty((self.nface, NSTATE, self.Q * self.Q))
        for k, (i, j) in enumerate(_SYM):
            state[:, k] = (k1 * n[..., i] * n[..., j] - (k0 if i == j else 0.0)).reshape(self.nface, -1)
        state[:, 6] = g.reshape(self.nface, -1)
        return self._to_nodes(-(wje * pen)[..., None] * n, self.B), state

    def _K(self, state) -> np.ndarray:
        """K_q as full matrices [face][b][a][3][3] from a state."""
        s = np.asarray(state, dtype=np.float64).reshape(-1)[:self.state_size].reshape(self.nface, NSTATE, self.Q, self.Q)
        K = np.empty((self.nface, self.Q, self.Q, 3, 3))
        for k, (i, j) in enumerate(_SYM):
            K[..., i, j] = K[..., j, i] = s[:, k]
        return K

    def tangent_host(self, state, du) -> np.ndarray:
        """C du as an L-vector from a state (of this or of a finer p-level); masked entries of du read as zero."""
        dq = pt.to_points(self._gather(self._free(du)), self.B, self.B)
        return self._to_nodes(np.einsum("fbacd,fbad->fbac", self._K(state), dq), self.B)

    def diagonal_host(self, state) -> np.ndarray:
        """diag C as an L-vector from a state."""
        K = self._K(state)
        return self._to_nodes(np.stack([K[..., c, c] for c in range(3)], axis=-1), np.square(self.B))

    # ---- y += ..., on vectors of the Ceed ----------------------------------------------------------------------------------------
    def residual_add(self, scale: float, u: cd.Vector, y: cd.Vector, state: cd.Vector):
        """y += scale r(u); state := the contact state at u (never scaled)."""
        if self.handle is not None:
            self.handle.apply_residual_add(scale, self.X, u, y, state)
        else:
            r, st = self.residual_host(u.to_numpy())
            pt.assign(state, st)
            if self.nface:
                pt.add(y, scale * r)

    def tangent_add(self, scale: float, state: cd.Vector, du: cd.Vector, y: cd.Vector):
        """y += scale C du."""
        if self.handle is not None:
            self.handle.apply_tangent_add(scale, state, du, y)
        elif self.nface:
            pt.add(y, scale * self.tangent_host(state.to_numpy(), du.to_numpy()))

    def diagonal_add(self, scale: float, state: cd.Vector, d: cd.Vector):
        """d += scale diag C."""
        if self.handle is not None:
            self.handle.diagonal_add(scale, state, d)
        elif self.nface:
            pt.add(d, scale * self.diagonal_host(state.to_numpy()))

    # ---- read from the state -------------------------------------------------------------------------------------------------------
    def _gaps(self, state) -> np.ndarray:
        s = state.to_numpy() if isinstance(state, cd.Vector) else np.asarray(state)
        return s.reshape(-1)[:self.state_size].reshape(self.nface, NSTATE, self.Q * self.Q)[:, 6]

    def min_gap(self, state) -> float:
        """The smallest gap over the points (negative: the largest penetration); +inf without faces."""
        g = self._gaps(state)
        return float(g.min()) if g.size else float("inf")

    def active_fraction(self, state) -> float:
        """The share of the points in contact (g < 0)."""
        g = self._gaps(state)
        return float((g < 0.0).mean()) if g.size else 0.0
