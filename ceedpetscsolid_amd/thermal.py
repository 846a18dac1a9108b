"""Thermal loads: a nodal temperature change theta from the stress-free state, in the residual, the tangent and the reported stress.

    beta = E alpha / (1 - 2 nu) (= 3 K alpha),      theta_h(q) = sum_m N_m(q) theta(m)

theta is interpolated with the displacement's basis through a scalar restriction of its own on the level's nodes, as the density of
``mass.MassOperator(density=)`` is.  The thermal term is the derivative of a coupling energy added to the model's strain energy:

    linElas, hyperSS   Phi = -int beta theta_h tr eps dV     R(v) = -int beta theta_h div v dV       a dead load: no tangent
    hyperFS            Phi = -int beta theta_h ln J dV       R(v) = -int beta theta_h F^-T : grad_X v dV   (first Piola -beta theta_h F^-T)
                       T(u)[du](v) = +int beta theta_h (F^-T (grad_X du)^T F^-T) : grad_X v dV       symmetric: it derives from Phi

(the reference's shear quirk of linElas touches off-diagonal entries only, so it does not enter).  The Cauchy stress the residual then
integrates is sigma - beta theta_h I (linElas, hyperSS) or sigma - (beta theta_h / det F) I (hyperFS): ``postprocess.Stress(thermal=)``.

alpha is the LINEARISED coefficient of expansion.  In linElas the free expansion of a uniform theta is the strain alpha theta exactly.
hyperSS (lambda log1p(tr eps)) and hyperFS (lambda ln J) are logarithmic in the volume change, so there the stress-free stretch is
alpha theta to first order in alpha theta only.

On the device these are the operator graphs of the QFunctions ``ThermalForce`` and ``ThermalTangent`` (include/ceed.h;
csrc/kernels_stress.hip, k_stress's modes with a field).  Where the library has no functor of that name (the CPU oracle), or with
``portable=True``, the same sums are formed in NumPy on the tensor layer of ``portable.py`` with the tables of ``lv.basisu`` and the
quadrature data read back once (which form runs where, and why it is the device tests' yardstick: DESIGN.md 2).

Dirichlet mask (the level's): ``force`` reads the displacement as it is, boundary values included, and ``tangent`` reads masked entries
of dx as zero; masked rows of y are stored as zeros (``add=False``) or left alone (``add=True``).
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import ceed as cd
from . import portable as pt
from .solid import SolidProblem

MODEL = {"linElas": 0, "hyperSS": 1, "hyperFS": 2}


def thermal_beta(nu: float, E: float, alpha: float) -> float:
    return E * alpha / (1 - 2 * nu)


class ThermalLoad:
    def __init__(self, prob: SolidProblem, level: int, alpha: float, theta, problem: str, portable: Optional[bool] = None):
        """``theta``: a float (uniform), an array ``(nnodes,)`` of the level's nodes, or a callable ``f(X) -> (n,)`` on ``node_coords``."""
        if problem not in MODEL:
            raise ValueError(f"unknown problem {problem!r}")
        alpha = float(alpha)
        if not np.isfinite(alpha):
            raise ValueError(f"thermal: alpha must be finite, not {alpha!r}")
        c = self.ceed = prob.ceed
        self.p, self.problem, self.model, self.alpha = prob, problem, MODEL[problem], alpha
        lv = self.lv = prob.levels[level]
        dm = lv.dofmap
        self.P, self.Q, self.ne = lv.degree + 1, lv.Q, prob.mesh.nelem
        self.nnodes, self.lsize = dm.nnodes, dm.lsize
        self.nu, self.E = float(prob.phys[0]), float(prob.phys[1])
        self.beta = thermal_beta(self.nu, self.E, alpha)
        P3 = self.P ** 3
        self.offsets = (np.asarray(dm.offsets(), dtype=np.int64) & 0x1FFFFFFF).reshape(self.ne, P3)
        self.nodes = (self.offsets // 3).reshape((self.ne,) + 3 * (self.P,))                      # [e][k][j][i], of the displacement
        self.theta_nodes = np.asarray(dm.elem_nodes, dtype=np.int64).reshape(self.ne, P3)         # [e][P^3] plain indices into theta
        self.theta = self._theta_values(theta)
        self.mask = (np.asarray(lv.mask).reshape(-1)[:self.lsize] != 0) if prob.fused_bc else None
        self.portable = (not c.has_qfunction("ThermalForce")) if portable is None else bool(portable)
        self._tab = None
        self.scale = 1.0
        self.theta_vec = self.theta_rstr = self.theta_basis = self.state = None
        self.qf_force = self.op_force = self.qf_tangent = self.op_tangent = None
        if not self.portable:
            self.theta_vec = c.vector(self.nnodes).set_array(self.theta)
            self.theta_rstr = c.elem_restriction(self.ne, P3, 1, 1, self.nnodes, self.theta_nodes.astype(np.int32).reshape(-1))
            self.theta_basis = c.basis_lagrange(3, 1, self.P, self.Q, cd.GAUSS)
            fs = self.model == 2
            if fs:
                self.state = c.vector(self.lsize).set_value(0.0)           # the displacement the two operators read: force() / tangent() copy into it
            m8 = self.mask.astype(np.uint8) if self.mask is not None else None
            qf = self.qf_force = c.qfunction("ThermalForce", source="qfunctions/thermal.h:ThermalForce")
            qf.add_input("theta", 1, cd.EVAL_INTERP).add_input("qdata", 10, cd.EVAL_NONE)
            if fs:
                qf.add_input("du", 9, cd.EVAL_GRAD)
            qf.add_output("dv", 9, cd.EVAL_GRAD)
            qf.set_context([self.nu, self.E, alpha, float(self.model)])
            op = self.op_force = c.operator(qf)
            op.set_field("theta", self.theta_rstr, self.theta_basis, "active")
            op.set_field("qdata", lv.Erestrictqdi, None, lv.qdata)
            if fs:
                op.set_field("du", lv.Erestrictu, lv.basisu, self.state)
            op.set_field("dv", lv.Erestrictu, lv.basisu, "active")
            if m8 is not None:
                op.set_dirichlet_mask_mode(m8, None, 2)
            if fs:
                qf = self.qf_tangent = c.qfunction("ThermalTangent", source="qfunctions/thermal.h:ThermalTangent")
                qf.add_input("ddu", 9, cd.EVAL_GRAD).add_input("du", 9, cd.EVAL_GRAD).add_input("theta", 1, cd.EVAL_INTERP)
                qf.add_input("qdata", 10, cd.EVAL_NONE).add_output("dv", 9, cd.EVAL_GRAD)
                qf.set_context([self.nu, self.E, alpha, float(self.model)])
                op = self.op_tangent = c.operator(qf)
                op.set_field("ddu", lv.Erestrictu, lv.basisu, "active")
                op.set_field("du", lv.Erestrictu, lv.basisu, self.state)
                op.set_field("theta", self.theta_rstr, self.theta_basis, self.theta_vec)
                op.set_field("qdata", lv.Erestrictqdi, None, lv.qdata)
                op.set_field("dv", lv.Erestrictu, lv.basisu, "active")
                if m8 is not None:
                    op.set_dirichlet_mask_mode(m8, None, 3)

    def _theta_values(self, theta) -> np.ndarray:
        if callable(theta):
            t = np.asarray(theta(np.asarray(self.lv.dofmap.node_coords)), dtype=np.float64)
        elif np.ndim(theta) == 0:
            t = np.full(self.nnodes, float(theta))
        else:
            t = np.asarray(theta, dtype=np.float64)
        if t.shape != (self.nnodes,):
            raise ValueError(f"thermal: theta has shape {t.shape} for the {self.nnodes} nodes of the level (a float, an array (nnodes,) "
                             "or a callable of the node coordinates expected)")
        if not np.all(np.isfinite(t)):
            raise ValueError("thermal: theta is not finite")
        return t.copy()

    @property
    def kernel_name(self) -> dict:
        """The kernels of the last ``force`` and ``tangent`` (``"portable"`` for the NumPy form, ``""`` before the first apply)."""
        if self.portable:
            return {"force": "portable", "tangent": "portable"}
        return {"force": self.op_force.kernel_name, "tangent": self.op_tangent.kernel_name if self.op_tangent is not None else ""}

    def set_scale(self, scale: float):
        """theta is multiplied by ``scale`` (the load fraction) in the next applies: it rides in the context's alpha, which is re-read at
        every apply (a recorded apply keeps the value it was made with)."""
        self.scale = float(scale)
        for qf in (self.qf_force, self.qf_tangent):
            if qf is not None:
                qf._ctx[2] = self.alpha * self.scale

    def set_theta_values(self, theta):
        """New values of the temperature field, written behind the same address: a recorded apply sees them."""
        self.theta = self._theta_values(theta)
        if self.theta_vec is not None:
            self.theta_vec.fill(self.theta)
            if self.ceed.preferred_memtype == cd.MEM_DEVICE:
                self.theta_vec.device_pointer()             # on the device now: a replay reads the address, it runs no host code

    # ---- the portable form: NumPy on host arrays ---------------------------------------------------------------------------
    def _tables(self):
        if self._tab is None:
            Q = self.Q
            qd = self.lv.qdata.to_numpy().reshape(self.ne, 10, Q, Q, Q)
            self._tab = (self.lv.basisu.interp1d, self.lv.basisu.grad1d, qd[:, 0].copy(),
                         qd[:, 1:].reshape(self.ne, 3, 3, Q, Q, Q).copy())                 # B, G [q][p]; w det J [e][k][j][i]; dXdx [e][r][s][k][j][i]
        return self._tab

    def theta_points(self) -> np.ndarray:
        """theta_h at the points, [nelem][Q][Q][Q] (unscaled)."""
        B = self._tables()[0]
        return pt.to_points(self.theta[self.theta_nodes].reshape((self.ne,) + 3 * (self.P,)), B, B, B)

    def grad_host(self, x) -> np.ndarray:
        """The physical gradient at the points of an L-vector, [nelem][Q][Q][Q][c][n] = d x_c / d X_n."""
        B, G, _, dX = self._tables()
        ue = pt.gather(x, self.nodes, self.lsize)                                          # [e][k][j][i][c]
        du = np.stack([pt.to_points(ue, *t) for t in ((G, B, B), (B, G, B), (B, B, G))], axis=-1)          # [e][k][j][i][c][m]
        return np.einsum("ekjicm,emnkji->ekjicn", du, dX)

    def _from_flux(self, T: np.ndarray) -> np.ndarray:
        """int T : grad_X v for every nodal v as an L-vector: T[e][k][j][i][c][n] a first Piola stress at the points."""
        B, G, W, dX = self._tables()
        dv = np.einsum("ekjicn,emnkji->ekjicm", T, dX) * W[..., None, None]               # dv[c][m] = w det J sum_n dXdx[m][n] T[c][n]
        ve = sum(pt.to_nodes(dv[..., m], *t) for m, t in enumerate(((G, B, B), (B, G, B), (B, B, G))))
        return pt.node_sum(self.nodes, ve, self.lsize // 3 + 1).reshape(-1)[:self.lsize]

    def _finv_t(self, x):
        """(F^-T, det F) at the points; the identity and one for the small-strain models."""
        if self.model != 2:
            return np.broadcast_to(np.eye(3), (self.ne,) + 3 * (self.Q,) + (3, 3)), 1.0
        F = self.grad_host(x) + np.eye(3)
        return np.swapaxes(np.linalg.inv(F), -1, -2), np.linalg.det(F)

    def energy_host(self, x) -> float:
        """Phi(x) = -sum_q w det J beta theta_h {tr eps | ln det F}; the exact logarithm, whose derivative ``force_host`` is."""
        W = self._tables()[2]
        g = self.grad_host(x)
        s = np.log(np.linalg.det(g + np.eye(3))) if self.model == 2 else g[..., 0, 0] + g[..., 1, 1] + g[..., 2, 2]
        return -float(np.sum(W * self.beta * self.scale * self.theta_points() * s))

    def force_host(self, x=None) -> np.ndarray:
        """R_theta as an L-vector, ALL rows (masked rows are NOT dropped here: ``force`` does).  ``x``: the displacement with its boundary
        values; the small-strain models do not read it."""
        FiT, _ = self._finv_t(x)
        return self._from_flux((-self.beta * self.scale * self.theta_points())[..., None, None] * FiT)

    def tangent_host(self, x, dx, mask_in: bool = True) -> np.ndarray:
        """T_theta(x) dx as an L-vector, all rows; masked entries of dx read as zero unless ``mask_in`` is False."""
        if self.model != 2:
            raise ValueError(f"ThermalTangent: the thermal load of {self.problem} is dead and has no tangent (hyperFS alone has one)")
        dx = np.asarray(dx, dtype=np.float64).reshape(-1)[:self.lsize]
        if mask_in and self.mask is not None:
            dx = np.where(self.mask, 0.0, dx)
        FiT, _ = self._finv_t(x)
        A = self.grad_host(dx)
        return self._from_flux((self.beta * self.scale * self.theta_points())[..., None, None] * (FiT @ np.swapaxes(A, -1, -2) @ FiT))

    def _free_rows(self, r: np.ndarray) -> np.ndarray:
        return r if self.mask is None else np.where(self.mask, 0.0, r)

    # ---- on vectors of the Ceed ----------------------------------------------------------------------------------------------
    def _load_state(self, xloc):
        if self.state is not None and xloc is not self.state:
            self.state.axpby(1.0, xloc, 0.0)

    def force(self, xloc: Optional[cd.Vector], y: cd.Vector, add: bool = False):
        """y (+)= R_theta(xloc); masked rows zero (``add``: left alone).  ``xloc`` may be None for the small-strain models."""
        if self.op_force is not None:
            if self.model == 2:
                self._load_state(xloc)
            (self.op_force.apply_add if add else self.op_force.apply)(self.theta_vec, y)
        else:
            r = self._free_rows(self.force_host(xloc.to_numpy() if self.model == 2 else None))
            pt.add(y, r) if add else pt.assign(y, r, y.n)

    def tangent(self, xloc: cd.Vector, dx: cd.Vector, y: cd.Vector, add: bool = False):
        """y (+)= T_theta(xloc) dx (hyperFS only)."""
        if self.model != 2:
            raise ValueError(f"ThermalTangent: the thermal load of {self.problem} is dead and has no tangent (hyperFS alone has one)")
        if self.op_tangent is not None:
            self._load_state(xloc)
            (self.op_tangent.apply_add if add else self.op_tangent.apply)(dx, y)
        else:
            r = self._free_rows(self.tangent_host(xloc.to_numpy(), dx.to_numpy()))
            pt.add(y, r) if add else pt.assign(y, r, y.n)

    def destroy(self):
        for o in (self.op_force, self.op_tangent, self.qf_force, self.qf_tangent, self.theta_rstr, self.theta_basis, self.theta_vec, self.state):
            if o is not None:
                o.destroy()
        self.op_force = self.op_tangent = self.qf_force = self.qf_tangent = None
        self.theta_rstr = self.theta_basis = self.theta_vec = self.state = None
