"""Surface loads on side sets: a dead traction, a pressure that follows the deforming surface, and that pressure's exact tangent.

The loaded surface is a union of element faces named by side-set ids.  On a face the nodes are the element's P^2 face nodes, N_a the
tensor Lagrange functions on the Gauss-Lobatto points, (xi, eta) the two in-face reference directions ordered so that X_xi x X_eta
points out of the body (``mesh.side_set_faces``), x = X + u the current position, and the quadrature Q Gauss points per direction
(exact for everything below: summed over a, the integrands have degree <= 2p - 1 per direction).  Three geometric vectors, with signs
and load factors left to the caller (``solver.NewtonPMG``):

    traction   g_a      = int N_a t |X_xi x X_eta| dxi deta               dead load, per unit reference area; t a constant 3-vector
    pressure   g_a(u)   = int N_a (x_xi x x_eta) dxi deta                 area-weighted current outward normal; quadratic in u
    tangent    T(u) du |_a = int N_a (du_xi x x_eta + x_xi x du_eta)      the exact derivative of g(u)

T(u) is symmetric on the variations that vanish on the rim of the loaded surface -- a closed surface, or a patch whose rim is clamped
(a tube with clamped ends) -- and not otherwise: a follower pressure on a patch with a free rim is not conservative.

Fields.  Five further vectors for loads that vary over the side set, with t_h, p_h, x_h, du_h the nodal values interpolated to the
point (sum_b N_b t_b, ...), e the unit "up" vector, d = level - e . x_h the depth of the CURRENT point, <d> = max(d, 0), H the step:

    traction field        g_a      = sum_q w_q N_a t_h |X_xi x X_eta|                  t_b a nodal 3-vector field; dead, evaluated once
    pressure field        g_a(u)   = sum_q w_q N_a p_h (x_xi x x_eta)                  p_b a nodal scalar field on the material points
    its tangent           T du |_a = sum_q w_q N_a p_h (du_xi x x_eta + x_xi x du_eta)
    hydrostatic           g_a(u)   = sum_q w_q N_a gamma <d> (x_xi x x_eta)
    its tangent           T du |_a = sum_q w_q N_a gamma [<d> (du_xi x x_eta + x_xi x du_eta) - H(d) (e . du_h) (x_xi x x_eta)]

These sums are NOT exact integrals at Q = P once p >= 3 (the integrands reach degree 3p - 1 per direction): the discrete form is DEFINED
by the quadrature, and each tangent is the exact derivative of that discrete form (the hydrostatic one away from d = 0).

On the device these are the library's CeedXSurfaceLoad* entry points (csrc/kernels_surface.hip).  Where the library lacks them (the CPU
oracle), or with ``portable=True``, the same sums are formed in NumPy on the tensor layer and the tables of ``portable.py`` (which form
runs where, and why it is the device tests' yardstick: DESIGN.md 2).
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import ceed as cd
from . import portable as pt
from .mesh import DofMap, HexMesh, side_set_faces
from .portable import lagrange_tables          # (importable from here too, as before)


def check_field(f, n: int, what: str) -> np.ndarray:
    """The nodal field ``f`` as a flat float64 array of exactly ``n`` values."""
    f = np.asarray(f, dtype=np.float64).reshape(-1)
    if f.size != n:
        raise ValueError(f"{what}: {f.size} values where {n} are expected")
    return f


def unit_vector(up) -> np.ndarray:
    """up / |up|; a vector that is not three finite components, or is zero, is refused."""
    e = np.asarray(up, dtype=np.float64).reshape(-1)
    if e.size != 3 or not np.all(np.isfinite(e)) or not np.any(e != 0.0):
        raise ValueError(f"hydrostatic: up = {up!r} is not a finite, non-zero 3-vector")
    return e / np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])


def check_hydrostatic(gamma, level, up):
    if not (np.isfinite(float(gamma)) and np.isfinite(float(level))):
        raise ValueError(f"hydrostatic: gamma = {gamma!r} and level = {level!r} must be finite")
    unit_vector(up)


class FaceTerm:
    """What a term on the faces of ``side_ids`` of ``mesh`` under the numbering ``dm`` keeps: the face list, the node coordinates (``Xh``
    on the host; ``X``, a device L-vector made when first asked for), the tables of (P nodes, Q Gauss points), the Dirichlet byte mask
    over the L-vector -- masked rows of a result are never written, masked entries of du read as zero, u is read as it is (it carries the
    boundary values) -- and the library's handle (``HANDLE``, a ceed._FaceHandle), or none in the portable NumPy form."""
    HANDLE = None

    def __init__(self, ceed: cd.Ceed, mesh: HexMesh, dm: DofMap, side_ids, Q: int, mask=None, portable: bool = False):
        self.ceed, self.L = ceed, ceed.L
        self.P, self.lsize, self.Q = dm.P, dm.lsize, int(Q)
        self.side_ids = list(side_ids)
        self.faces = side_set_faces(mesh, dm, self.side_ids)
        self.nface = self.faces.shape[0]
        self.Xh = np.ascontiguousarray(dm.node_coords, dtype=np.float64).reshape(-1)
        self.portable = bool(portable) or not self.L.has(self.HANDLE.PREFIX + "Create")
        self.B, self.D, self.w = lagrange_tables(self.P, self.Q)
        self.mask = self._X = None
        self.handle = None if self.portable else self.HANDLE(ceed, self.P, self.Q, 3 * self.faces, self.lsize)
        if mask is not None:
            self.set_mask(mask)

    def set_mask(self, mask):
        self.mask = None if mask is None else (np.asarray(mask).reshape(-1)[:self.lsize] != 0)
        if self.handle is not None:
            self.handle.set_dirichlet_mask(None if mask is None else self.mask.astype(np.uint8))

    @property
    def kernel_name(self) -> str:
        return "portable" if self.handle is None else self.handle.kernel_name

    @property
    def X(self) -> Optional[cd.Vector]:
        if self._X is None and self.handle is not None:
            self._X = self.ceed.vector(self.lsize).set_array(self.Xh)
        return self._X

    @X.setter
    def X(self, v: Optional[cd.Vector]):
        self._X = v

    def destroy(self):
        if self.handle is not None:
            self.handle.destroy()
            self.handle = None
        if self._X is not None:
            self._X.destroy()
            self._X = None

    # ---- the portable form: NumPy on host arrays ---------------------------------------------------------------------------
    def _gather(self, field: np.ndarray) -> np.ndarray:
        """The face nodes' values [face][j (eta)][i (xi)][c] of a nodal field (L-vector)."""
        return pt.gather(field, self.faces.reshape(self.nface, self.P, self.P), self.lsize)

    def _derivs(self, field: np.ndarray):
        """d / d xi and d / d eta at the points, [face][b][a][c], of a nodal field (L-vector)."""
        f = self._gather(field)
        return pt.to_points(f, self.D, self.B), pt.to_points(f, self.B, self.D)

    def _free(self, du) -> np.ndarray:
        """du with its masked entries as zeros."""
        du = np.asarray(du, dtype=np.float64).reshape(-1)[:self.lsize]
        return du if self.mask is None else np.where(self.mask, 0.0, du)

    def _to_nodes(self, val: np.ndarray, B: np.ndarray) -> np.ndarray:
        """The L-vector of sum_q B_a(q) val(q), val [face][b][a][c] with the weights inside: face results added in face order; masked
        rows are zero."""
        out = pt.node_sum(self.faces, pt.to_nodes(val, B, B), self.lsize // 3).reshape(-1)
        if self.mask is not None:
            out[self.mask] = 0.0
        return out


class SurfaceLoad(FaceTerm):
    """The surface loads of the faces of ``side_ids`` (FaceTerm).  ``Q``: Gauss points per direction (default P: the fine level's
    Q = P + qextra is the caller's to pass)."""
    HANDLE = cd.SurfaceLoadHandle

    def __init__(self, ceed: cd.Ceed, mesh: HexMesh, dm: DofMap, side_ids, Q: Optional[int] = None, mask=None, portable: bool = False):
        super().__init__(ceed, mesh, dm, side_ids, dm.P if Q is None else Q, mask, portable)

    def _weighted(self, val: np.ndarray) -> np.ndarray:
        """The L-vector of sum_q w_q N_a(q) val(q)."""
        return self._to_nodes(val * (self.w[:, None] * self.w[None, :])[None, :, :, None], self.B)

    def _position(self, u) -> np.ndarray:
        return self.Xh if u is None else self.Xh + np.asarray(u, dtype=np.float64).reshape(-1)[:self.lsize]

    def traction_host(self, t) -> np.ndarray:
        """g of a traction t as an L-vector (NumPy)."""
        Xa, Xb = self._derivs(self.Xh)
        J = np.linalg.norm(np.cross(Xa, Xb), axis=-1)
        return self._weighted(J[..., None] * np.asarray(t, dtype=np.float64))

    def pressure_host(self, u=None) -> np.ndarray:
        """g(u) of a unit pressure as an L-vector (NumPy); ``u`` None: the reference configuration."""
        xa, xb = self._derivs(self._position(u))
        return self._weighted(np.cross(xa, xb))

    def tangent_host(self, u, du) -> np.ndarray:
        """T(u) du of a unit pressure as an L-vector (NumPy); masked entries of du read as zero."""
        xa, xb = self._derivs(self._position(u))
        da, db = self._derivs(self._free(du))
        return self._weighted(np.cross(da, xb) + np.cross(xa, db))

    # ---- loads that vary over the side set (the module's docstring, "Fields"): NumPy ----------------------------------------------
    def _values(self, field: np.ndarray) -> np.ndarray:
        """The values at the points, [face][b][a][c], of a nodal field (L-vector)."""
        return pt.to_points(self._gather(field), self.B, self.B)

    def _scalar_values(self, p) -> np.ndarray:
        """The values at the points, [face][b][a], of a nodal scalar field (one value per node)."""
        p = check_field(p, self.lsize // 3, "pressure field")
        return pt.to_points(p[self.faces.reshape(self.nface, self.P, self.P)], self.B, self.B)

    def depth_host(self, level: float, up=(0.0, 0.0, 1.0), u=None) -> np.ndarray:
        """d = level - e . x_h at the points, [face][b][a]: positive under the surface of the fluid."""
        return float(level) - self._values(self._position(u)) @ unit_vector(up)

    def traction_field_host(self, t) -> np.ndarray:
        """g of the nodal traction field t (L-vector, or [node][3]) as an L-vector (NumPy)."""
        Xa, Xb = self._derivs(self.Xh)
        J = np.linalg.norm(np.cross(Xa, Xb), axis=-1)
        return self._weighted(J[..., None] * self._values(check_field(t, self.lsize, "traction field")))

    def pressure_field_host(self, p, u=None) -> np.ndarray:
        """g(u) of the nodal pressure field p (one value per node) as an L-vector (NumPy)."""
        xa, xb = self._derivs(self._position(u))
        return self._weighted(self._scalar_values(p)[..., None] * np.cross(xa, xb))

    def pressure_field_tangent_host(self, p, u, du) -> np.ndarray:
        """The derivative of ``pressure_field_host`` in the direction du (NumPy); masked entries of du read as zero."""
        xa, xb = self._derivs(self._position(u))
        da, db = self._derivs(self._free(du))
        return self._weighted(self._scalar_values(p)[..., None] * (np.cross(da, xb) + np.cross(xa, db)))

    def hydrostatic_host(self, gamma: float, level: float, up=(0.0, 0.0, 1.0), u=None) -> np.ndarray:
        """g(u) of the pressure gamma <level - e . x> of a fluid at rest as an L-vector (NumPy)."""
        check_hydrostatic(gamma, level, up)
        xa, xb = self._derivs(self._position(u))
        d = self.depth_host(level, up, u)
        return self._weighted((float(gamma) * np.maximum(d, 0.0))[..., None] * np.cross(xa, xb))

    def hydrostatic_tangent_host(self, gamma: float, level: float, up, u, du) -> np.ndarray:
        """The derivative of ``hydrostatic_host`` in the direction du away from d = 0 (NumPy); masked entries of du read as zero."""
        check_hydrostatic(gamma, level, up)
        xa, xb = self._derivs(self._position(u))
        free = self._free(du)
        da, db = self._derivs(free)
        d = self.depth_host(level, up, u)
        rise = self._values(free) @ unit_vector(up)
        val = np.maximum(d, 0.0)[..., None] * (np.cross(da, xb) + np.cross(xa, db)) - ((d > 0.0) * rise)[..., None] * np.cross(xa, xb)
        return self._weighted(float(gamma) * val)

    # ---- y += ..., on vectors of the Ceed ----------------------------------------------------------------------------------------
    def traction_field_add(self, t: cd.Vector, scale: float, y: cd.Vector):
        """y += scale g^traction(t), t a nodal traction field (an L-vector)."""
        if self.handle is not None:
            self.handle.apply_field_add(cd.SURFACE_TRACTION, t, scale, self.X, None, y)
        else:
            pt.add(y, scale * self.traction_field_host(t.to_numpy()))

    def pressure_field_add(self, p: cd.Vector, scale: float, u: Optional[cd.Vector], y: cd.Vector):
        """y += scale g^pressure(p; u), p a nodal pressure field (a vector of lsize / 3 values)."""
        if self.handle is not None:
            self.handle.apply_field_add(cd.SURFACE_PRESSURE, p, scale, self.X, u, y)
        else:
            pt.add(y, scale * self.pressure_field_host(p.to_numpy(), None if u is None else u.to_numpy()))

    def pressure_field_tangent_add(self, p: cd.Vector, scale: float, u: Optional[cd.Vector], du: cd.Vector, y: cd.Vector):
        """y += scale T^pressure(p; u) du."""
        if self.handle is not None:
            self.handle.apply_field_tangent_add(p, scale, self.X, u, du, y)
        else:
            pt.add(y, scale * self.pressure_field_tangent_host(p.to_numpy(), None if u is None else u.to_numpy(), du.to_numpy()))

    def hydrostatic_add(self, gamma: float, level: float, up, scale: float, u: Optional[cd.Vector], y: cd.Vector):
        """y += scale g^hydrostatic(u): the fluid of weight gamma per unit volume standing up to ``level`` along ``up``."""
        if self.handle is not None:
            check_hydrostatic(gamma, level, up)
            self.handle.apply_hydrostatic_add(gamma, level, up, scale, self.X, u, y)
        else:
            pt.add(y, scale * self.hydrostatic_host(gamma, level, up, None if u is None else u.to_numpy()))

    def hydrostatic_tangent_add(self, gamma: float, level: float, up, scale: float, u: Optional[cd.Vector], du: cd.Vector, y: cd.Vector):
        """y += scale T^hydrostatic(u) du."""
        if self.handle is not None:
            check_hydrostatic(gamma, level, up)
            self.handle.apply_hydrostatic_tangent_add(gamma, level, up, scale, self.X, u, du, y)
        else:
            pt.add(y, scale * self.hydrostatic_tangent_host(gamma, level, up, None if u is None else u.to_numpy(), du.to_numpy()))

    def traction_add(self, t, scale: float, y: cd.Vector):
        """y += scale g^traction(t)."""
        if self.handle is not None:
            self.handle.apply_add(cd.SURFACE_TRACTION, t, scale, self.X, None, y)
        else:
            pt.add(y, scale * self.traction_host(t))

    def pressure_add(self, p: float, scale: float, u: Optional[cd.Vector], y: cd.Vector):
        """y += scale p g^pressure(u)."""
        if self.handle is not None:
            self.handle.apply_add(cd.SURFACE_PRESSURE, (p, 0.0, 0.0), scale, self.X, u, y)
        else:
            pt.add(y, scale * p * self.pressure_host(None if u is None else u.to_numpy()))

    def tangent_add(self, p: float, scale: float, u: Optional[cd.Vector], du: cd.Vector, y: cd.Vector):
        """y += scale p T(u) du."""
        if self.handle is not None:
            self.handle.apply_tangent_add(p, scale, self.X, u, du, y)
        else:
            pt.add(y, scale * p * self.tangent_host(None if u is None else u.to_numpy(), du.to_numpy()))
