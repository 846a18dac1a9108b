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

On the device these are the library's CeedXSurfaceLoad* entry points (csrc/kernels_surface.hip).  Where the library lacks them (the CPU
oracle), or with ``portable=True``, the same sums are formed in NumPy: plain ``einsum`` in float64 with tables built from
``mesh.gll_nodes`` and ``numpy.polynomial.legendre.leggauss``, face contributions added in face order.  The portable form is the
tests' yardstick for the device, as the point-block diagonal's portable form is.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import ceed as cd
from .mesh import DofMap, HexMesh, gll_nodes, side_set_faces


def lagrange_tables(P: int, Q: int):
    """(B, D, w): values and derivatives (Q x P) of the P Lagrange functions on the Gauss-Lobatto points at the Q Gauss points, and the
    Gauss weights."""
    nodes = gll_nodes(P)
    pts, w = np.polynomial.legendre.leggauss(Q)
    B, D = np.zeros((Q, P)), np.zeros((Q, P))
    for i in range(P):
        others = [k for k in range(P) if k != i]
        den = np.prod([nodes[i] - nodes[k] for k in others])
        B[:, i] = np.prod([pts - nodes[k] for k in others], axis=0) / den
        for m in others:
            D[:, i] += np.prod([pts - nodes[k] for k in others if k != m] + [np.ones(Q)], axis=0) / den
    return B, D, w


class SurfaceLoad:
    """The faces of ``side_ids`` of ``mesh`` under the numbering ``dm``, the node coordinates X (a device L-vector with the library's
    form) and the library's handle.  ``Q``: Gauss points per direction (default P: the fine level's Q = P + qextra is the caller's to
    pass).  ``mask``: the Dirichlet byte mask over the L-vector -- masked rows of y are never written, masked entries of du read as
    zero, u is read as it is (it carries the boundary values)."""

    def __init__(self, ceed: cd.Ceed, mesh: HexMesh, dm: DofMap, side_ids, Q: Optional[int] = None, mask=None, portable: bool = False):
        self.ceed, self.L = ceed, ceed.L
        self.P, self.lsize = dm.P, dm.lsize
        self.Q = self.P if Q is None else int(Q)
        self.side_ids = list(side_ids)
        self.faces = side_set_faces(mesh, dm, self.side_ids)
        self.nface = self.faces.shape[0]
        self.Xh = np.ascontiguousarray(dm.node_coords, dtype=np.float64).reshape(-1)
        self.portable = bool(portable) or not self.L.has("CeedXSurfaceLoadCreate")
        self.B, self.D, self.w = lagrange_tables(self.P, self.Q)
        self.mask = None
        self.handle = self.X = None
        if not self.portable:
            self.X = ceed.vector(self.lsize).set_array(self.Xh)
            self.handle = cd.SurfaceLoadHandle(ceed, self.P, self.Q, 3 * self.faces, self.lsize)
        if mask is not None:
            self.set_mask(mask)

    def set_mask(self, mask):
        self.mask = None if mask is None else (np.asarray(mask).reshape(-1)[:self.lsize] != 0)
        if self.handle is not None:
            self.handle.set_dirichlet_mask(None if mask is None else self.mask.astype(np.uint8))

    @property
    def kernel_name(self) -> str:
        return "portable" if self.handle is None else self.handle.kernel_name

    # ---- the portable form: NumPy on host arrays ---------------------------------------------------------------------------
    def _derivs(self, field: np.ndarray):
        """d / d xi and d / d eta at the points, [face][b][a][c], of a nodal field (L-vector)."""
        P = self.P
        f = field.reshape(-1, 3)[self.faces].reshape(self.nface, P, P, 3)          # [face][j (eta)][i (xi)][c]
        return np.einsum("ai,bj,fjic->fbac", self.D, self.B, f), np.einsum("ai,bj,fjic->fbac", self.B, self.D, f)

    def _to_nodes(self, val: np.ndarray) -> np.ndarray:
        """The L-vector of sum_q w_q N_a(q) val(q): the face results added in face order; masked rows are zero."""
        W = self.w[:, None] * self.w[None, :]
        ge = np.einsum("ai,bj,fbac->fjic", self.B, self.B, val * W[None, :, :, None])
        out = np.zeros((self.lsize // 3, 3))
        np.add.at(out, self.faces.reshape(-1), ge.reshape(-1, 3))
        out = out.reshape(-1)
        if self.mask is not None:
            out[self.mask] = 0.0
        return out

    def _position(self, u) -> np.ndarray:
        return self.Xh if u is None else self.Xh + np.asarray(u, dtype=np.float64).reshape(-1)[:self.lsize]

    def traction_host(self, t) -> np.ndarray:
        """g of a traction t as an L-vector (NumPy)."""
        Xa, Xb = self._derivs(self.Xh)
        J = np.linalg.norm(np.cross(Xa, Xb), axis=-1)
        return self._to_nodes(J[..., None] * np.asarray(t, dtype=np.float64))

    def pressure_host(self, u=None) -> np.ndarray:
        """g(u) of a unit pressure as an L-vector (NumPy); ``u`` None: the reference configuration."""
        xa, xb = self._derivs(self._position(u))
        return self._to_nodes(np.cross(xa, xb))

    def tangent_host(self, u, du) -> np.ndarray:
        """T(u) du of a unit pressure as an L-vector (NumPy); masked entries of du read as zero."""
        du = np.asarray(du, dtype=np.float64).reshape(-1)[:self.lsize]
        if self.mask is not None:
            du = np.where(self.mask, 0.0, du)
        xa, xb = self._derivs(self._position(u))
        da, db = self._derivs(du)
        return self._to_nodes(np.cross(da, xb) + np.cross(xa, db))

    @staticmethod
    def _add_host(y: cd.Vector, add: np.ndarray):
        v = y.to_numpy().copy()
        v[:add.size] += add
        y.set_array(v)

    # ---- y += ..., on vectors of the Ceed ----------------------------------------------------------------------------------------
    def traction_add(self, t, scale: float, y: cd.Vector):
        """y += scale g^traction(t)."""
        if self.handle is not None:
            self.handle.apply_add(cd.SURFACE_TRACTION, t, scale, self.X, None, y)
        else:
            self._add_host(y, scale * self.traction_host(t))

    def pressure_add(self, p: float, scale: float, u: Optional[cd.Vector], y: cd.Vector):
        """y += scale p g^pressure(u)."""
        if self.handle is not None:
            self.handle.apply_add(cd.SURFACE_PRESSURE, (p, 0.0, 0.0), scale, self.X, u, y)
        else:
            self._add_host(y, scale * p * self.pressure_host(None if u is None else u.to_numpy()))

    def tangent_add(self, p: float, scale: float, u: Optional[cd.Vector], du: cd.Vector, y: cd.Vector):
        """y += scale p T(u) du."""
        if self.handle is not None:
            self.handle.apply_tangent_add(p, scale, self.X, u, du, y)
        else:
            self._add_host(y, scale * p * self.tangent_host(None if u is None else u.to_numpy(), du.to_numpy()))

    def destroy(self):
        if self.handle is not None:
            self.handle.destroy()
            self.handle = None
        if self.X is not None:
            self.X.destroy()
            self.X = None
