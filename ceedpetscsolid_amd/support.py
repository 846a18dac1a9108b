"""Linear spring and dashpot supports on side sets: an elastic (Winkler) foundation, a dashpot layer, an absorbing boundary.

The supported surface Gamma is a union of element faces named by side-set ids; the faces, their node order and their Gauss points are
those of ``surface.py``.  A layer has a normal and a tangential coefficient per unit REFERENCE area -- (kn, kt) for springs, (cn, ct) for
dashpots -- and is fixed in the reference configuration, with J = |X_xi x X_eta| and n = X_xi x X_eta / J (its sign is immaterial):

    K_q      = w_q J_q [kt I + (kn - kt) n (x) n]                 symmetric, positive semi-definite
    f_a      = int N_a K (sum_b N_b x_b) dA0                      the force of a field x READ AS IT IS (boundary values included)
    K dx |_a = int N_a K (sum_b N_b dx_b) dA0                     the tangent: masked entries of dx read as zero
    d_{a,c}  = sum_q N_a(q)^2 K_q[c][c]

The spring force is K_s u, the dashpot force C_d v; u and v carry the prescribed motion of a rim shared with a clamped set, which is
why the force does not read flagged entries as zero while the tangent (a variation vanishes there) does.  ``form_state`` writes the
SUPPORT STATE, a vector [face][7][Q^2] laid out as the contact state (contact.py): the six entries of K_q in the order (xx, yy, zz,
yz, xz, xy), then w_q J_q, whose sum is the area of Gamma.  Force, tangent and diagonal at ANY p-level are B^T K_q B with that level's
(P_level, Q_fine) tables on this one state, so a coarse level's term is the Galerkin product of the fine one, and a linear combination
of states (K_s + a1 C_d) is the state of the combined layer -- except its entry 6, which then means nothing.

On the device these are the library's CeedXSupport* entry points (include/ceed_support.h; the support modes of k_contact and its
tangent and diagonal modes, csrc/kernels_contact.hip).  Where the library lacks them (the CPU oracle), or with ``portable=True``, the
same sums are formed in NumPy on the tensor layer of ``portable.py``.

Out of scope: supports in an assembled matrix, several ranks, unilateral or non-linear springs, spatially varying coefficients.
"""
from __future__ import annotations

import numpy as np

from . import ceed as cd
from . import portable as pt
from .contact import _SYM
from .mesh import DofMap, HexMesh
from .surface import FaceTerm

NSTATE = cd.CONTACT_NSTATE


def check_coefficients(who: str, kn: float, kt: float):
    """What CeedXSupportFormState refuses, refused with the same words (ValueError)."""
    kn, kt = float(kn), float(kt)
    if not (kn >= 0.0 and kt >= 0.0 and np.isfinite(kn) and np.isfinite(kt)):
        raise ValueError(f"{who}: the coefficients kn = {kn:g}, kt = {kt:g} are not finite and non-negative")
    return kn, kt


class SupportSurface(FaceTerm):
    """The support term of the faces of ``side_ids`` (surface.FaceTerm).  ``Q``: Gauss points per direction, the FINE level's on every
    level.  A state is a vector of the Ceed with ``state_size`` entries (``new_state``); a coarse level's surface takes the one its fine
    level formed."""
    HANDLE = cd.SupportHandle
    PREFIX = "CeedXSupport"

    def __init__(self, ceed: cd.Ceed, mesh: HexMesh, dm: DofMap, side_ids, Q: int, mask=None, portable: bool = False):
        super().__init__(ceed, mesh, dm, side_ids, Q, mask, portable)
        self.state_size = self.nface * NSTATE * self.Q ** 2

    def new_state(self) -> cd.Vector:
        """A zeroed state vector (no layer); the caller destroys it."""
        return self.ceed.vector(max(self.state_size, 1)).set_value(0.0)

    # ---- the portable form: NumPy on host arrays ---------------------------------------------------------------------------
    def state_host(self, kn: float, kt: float) -> np.ndarray:
        """The state [face][7][Q^2] of the layer (kn, kt)."""
        kn, kt = check_coefficients("support", kn, kt)
        Xa, Xb = self._derivs(self.Xh)
        m = np.cross(Xa, Xb)
        J = np.sqrt(np.square(m).sum(axis=-1))
        with np.errstate(divide="ignore"):
            jinv = np.where(J > 0.0, 1.0 / J, 0.0)
        n = m * jinv[..., None]
        wJ = (self.w[:, None] * self.w[None, :])[None] * J
        k0, k1 = wJ * kt, wJ * (kn - kt)                                   # K = k0 I + k1 n (x) n
        state = np.empty((self.nface, NSTATE, self.Q * self.Q))
        for k, (i, j) in enumerate(_SYM):
            state[:, k] = ((k0 if i == j else 0.0) + k1 * n[..., i] * n[..., j]).reshape(self.nface, -1)
        state[:, 6] = wJ.reshape(self.nface, -1)
        return state

    def _K(self, state) -> np.ndarray:
        """K_q as full matrices [face][b][a][3][3] from a state."""
        s = np.asarray(state, dtype=np.float64).reshape(-1)[:self.state_size].reshape(self.nface, NSTATE, self.Q, self.Q)
        K = np.empty((self.nface, self.Q, self.Q, 3, 3))
        for k, (i, j) in enumerate(_SYM):
            K[..., i, j] = K[..., j, i] = s[:, k]
        return K

    def _apply(self, state, field: np.ndarray) -> np.ndarray:
        xq = pt.to_points(self._gather(field), self.B, self.B)
        return self._to_nodes(np.einsum("fbacd,fbad->fbac", self._K(state), xq), self.B)

    def force_host(self, state, x) -> np.ndarray:
        """K x as an L-vector from a state; x is read as it is, masked rows of the result are zero."""
        return self._apply(state, np.asarray(x, dtype=np.float64).reshape(-1)[:self.lsize])

    def tangent_host(self, state, dx) -> np.ndarray:
        """K dx as an L-vector from a state (of this or of a finer p-level); masked entries of dx read as zero."""
        return self._apply(state, self._free(dx))

    def diagonal_host(self, state) -> np.ndarray:
        """diag K as an L-vector from a state."""
        K = self._K(state)
        return self._to_nodes(np.stack([K[..., c, c] for c in range(3)], axis=-1), np.square(self.B))

    def energy_host(self, state, u) -> float:
        """1/2 u . K u, u read as it is (every row counts, masked ones too)."""
        uq = pt.to_points(self._gather(np.asarray(u, dtype=np.float64).reshape(-1)[:self.lsize]), self.B, self.B)
        return float(0.5 * np.einsum("fbac,fbacd,fbad->", uq, self._K(state), uq))

    # ---- on vectors of the Ceed --------------------------------------------------------------------------------------------
    def form_state(self, kn: float, kt: float, state: cd.Vector):
        """state := the state of the layer (kn, kt)."""
        kn, kt = check_coefficients("support", kn, kt)
        if self.handle is not None:
            self.handle.form_state(kn, kt, self.X, state)
        elif self.nface:
            pt.assign(state, self.state_host(kn, kt))

    def force_add(self, scale: float, state: cd.Vector, x: cd.Vector, y: cd.Vector):
        """y += scale K x, x read as it is."""
        if self.handle is not None:
            self.handle.apply_force_add(scale, state, x, y)
        elif self.nface:
            pt.add(y, scale * self.force_host(state.to_numpy(), x.to_numpy()))

    def tangent_add(self, scale: float, state: cd.Vector, dx: cd.Vector, y: cd.Vector):
        """y += scale K dx."""
        if self.handle is not None:
            self.handle.apply_tangent_add(scale, state, dx, y)
        elif self.nface:
            pt.add(y, scale * self.tangent_host(state.to_numpy(), dx.to_numpy()))

    def diagonal_add(self, scale: float, state: cd.Vector, d: cd.Vector):
        """d += scale diag K."""
        if self.handle is not None:
            self.handle.diagonal_add(scale, state, d)
        elif self.nface:
            pt.add(d, scale * self.diagonal_host(state.to_numpy()))

    def area(self, state) -> float:
        """The reference area of the faces: the sum of entry 6 of a state that ``form_state`` wrote."""
        s = state.to_numpy() if isinstance(state, cd.Vector) else np.asarray(state)
        return float(s.reshape(-1)[:self.state_size].reshape(self.nface, NSTATE, self.Q * self.Q)[:, 6].sum())
