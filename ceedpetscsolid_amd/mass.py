"""The mass operator of the elastodynamic solve: y = c B^T (w det J) B x on the three displacement components of a multigrid level.

    (M x)_a,c = c sum_e sum_q N_a(q) w_q det J_e(q) sum_b N_b(q) x_b,c

N the tensor Lagrange functions of the level's basis (P nodes per direction on the Gauss-Lobatto points), the quadrature the level's own
(``lv.basisu``: Q Gauss points per direction, Q >= P, exact for the products N_a N_b on affine elements), w det J component 0 of the
level's quadrature data, c a coefficient (the density, or a0 x density in the effective tangent K + a0 M of ``dynamics.NewmarkPMG``).

On the device this is the library's operator graph of the QFunction ``Mass`` (include/ceed.h; csrc/kernels_mass.hip): u INTERP active,
qdata NONE passive, v INTERP active, the coefficient in the context.  Where the library has no functor of that name (the CPU oracle), or
with ``portable=True``, the same sums are formed in NumPy on the tensor layer of ``portable.py`` with the 1-D table of ``lv.basisu`` and
component 0 of the quadrature data read back once (which form runs where, and why it is the device tests' yardstick: DESIGN.md 2).

Dirichlet mask (the level's, unless a restriction of the caller's is given): masked entries of x read as zero (``mask_mode`` 3, the
tangent's form) or as they are (``mask_mode`` 2, the residual's form: x carries the boundary values); masked rows of y are stored as
zeros by ``apply`` and left alone by ``apply_add``; the diagonal is zero there.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import ceed as cd
from . import portable as pt
from .solid import SolidProblem


class MassOperator:
    def __init__(self, prob: SolidProblem, level: int, coef: float, portable: Optional[bool] = None,
                 rstr: Optional[cd.ElemRestriction] = None, offsets=None, mask_mode: int = 3):
        """``rstr`` / ``offsets``: a restriction of the caller's on the level's elements and nodes-per-element (and its component-0
        offsets, [nelem][P^3], for the portable form) in place of the level's own -- the element-discontinuous one of
        ``assembly.AssembledLevel``; no mask is applied then."""
        c = self.ceed = prob.ceed
        self.L = c.L
        lv = self.lv = prob.levels[level]
        self.P, self.Q, self.ne = lv.degree + 1, lv.Q, prob.mesh.nelem
        self.coef = float(coef)
        if mask_mode not in (2, 3):
            raise ValueError(f"mask_mode must be 2 (rows dropped) or 3 (rows dropped, input read as zero), not {mask_mode!r}")
        self.mask_mode = mask_mode
        own = rstr is None
        self.rstr = lv.Erestrictu if own else rstr
        self.lsize = lv.dofmap.lsize if own else int(rstr.lsize)
        off = lv.dofmap.offsets() if own else offsets
        if off is None:
            raise ValueError("a restriction of the caller's needs its offsets too")
        self.offsets = np.asarray(off, dtype=np.int64).reshape(self.ne, self.P ** 3)
        self.nodes = (self.offsets // 3).reshape((self.ne,) + 3 * (self.P,))                      # [e][k][j][i]
        self.mask = (np.asarray(lv.mask).reshape(-1)[:self.lsize] != 0) if own and prob.fused_bc else None
        self.portable = (not c.has_qfunction("Mass")) if portable is None else bool(portable)
        self._B = self._W = None
        self.qf = self.op = None
        if not self.portable:
            self.qf = c.qfunction("Mass", source="qfunctions/mass.h:Mass")
            self.qf.add_input("u", 3, cd.EVAL_INTERP).add_input("qdata", 10, cd.EVAL_NONE).add_output("v", 3, cd.EVAL_INTERP)
            self.qf.set_context([self.coef])
            self.op = c.operator(self.qf)
            self.op.set_field("u", self.rstr, lv.basisu, "active")
            self.op.set_field("qdata", lv.Erestrictqdi, None, lv.qdata)
            self.op.set_field("v", self.rstr, lv.basisu, "active")
            if self.mask is not None:
                self.op.set_dirichlet_mask_mode(self.mask.astype(np.uint8), None, mask_mode)

    @property
    def kernel_name(self) -> str:
        return "portable" if self.op is None else self.op.kernel_name

    def set_coef(self, coef: float):
        """The coefficient of the next applies (the context is borrowed and re-read; a recorded apply keeps the value it was made with)."""
        self.coef = float(coef)
        if self.qf is not None:
            self.qf._ctx[0] = self.coef

    # ---- the portable form: NumPy on host arrays ---------------------------------------------------------------------------
    def _tables(self):
        if self._B is None:
            Q = self.Q
            self._B = self.lv.basisu.interp1d                                                   # [q][p]
            self._W = self.lv.qdata.to_numpy().reshape(self.ne, 10, Q, Q, Q)[:, 0].copy()       # w det J, [e][kk][b][a]
        return self._B, self._W

    def _sum(self, ve: np.ndarray) -> np.ndarray:
        """Element results [e][k][j][i][3] added into an L-vector in element order."""
        return pt.node_sum(self.nodes, ve, self.lsize // 3 + 1).reshape(-1)[:self.lsize]

    def apply_host(self, x, mask_mode: Optional[int] = None) -> np.ndarray:
        """M x as an L-vector (NumPy), in the operator's mask mode unless one is given; masked rows are NOT dropped here (``apply`` /
        ``apply_add`` do)."""
        B, W = self._tables()
        x = np.asarray(x, dtype=np.float64).reshape(-1)[:self.lsize]
        if self.mask is not None and (self.mask_mode if mask_mode is None else mask_mode) & 1:
            x = np.where(self.mask, 0.0, x)
        uq = pt.to_points(pt.gather(x, self.nodes, self.lsize), B, B, B)
        return self._sum(pt.to_nodes(uq * (self.coef * W)[..., None], B, B, B))

    def diagonal_host(self) -> np.ndarray:
        B, W = self._tables()
        B2 = B * B
        d = self._sum(np.repeat(pt.to_nodes(self.coef * W, B2, B2, B2)[..., None], 3, axis=-1))
        if self.mask is not None:
            d[self.mask] = 0.0
        return d

    def _free_rows(self, r: np.ndarray) -> np.ndarray:
        return r if self.mask is None else np.where(self.mask, 0.0, r)

    # ---- on vectors of the Ceed ----------------------------------------------------------------------------------------------
    def apply(self, x: cd.Vector, y: cd.Vector):
        """y = M x (masked rows zero)."""
        if self.op is not None:
            self.op.apply(x, y)
        else:
            pt.assign(y, self._free_rows(self.apply_host(x.to_numpy())), y.n)

    def apply_add(self, x: cd.Vector, y: cd.Vector):
        """y += M x (masked rows and everything beyond the L-size left alone)."""
        if self.op is not None:
            self.op.apply_add(x, y)
        else:
            pt.add(y, self._free_rows(self.apply_host(x.to_numpy())))

    def diagonal(self, d: cd.Vector):
        """d = diag M: c sum_q N_a(q)^2 w det J(q), the same for the three components; zero on masked rows."""
        if self.op is not None:
            self.op.assemble_diagonal(d)
        else:
            pt.assign(d, self.diagonal_host(), d.n)

    # ---- the lumped mass: row sums ---------------------------------------------------------------------------------------------
    def lumped_host(self) -> np.ndarray:
        """m_i = c sum_e sum_q N_i(q) w det J(q), the row sums of the consistent mass matrix (M 1 with the ones read unmasked, whatever
        the mask mode); zero on masked rows.  Positive on Gauss-Lobatto nodes for the meshes of this project."""
        d = self.apply_host(np.ones(self.lsize), mask_mode=2)
        if self.mask is not None:
            d[self.mask] = 0.0
        return d

    def lumped(self, d: cd.Vector):
        """d = the lumped mass (``lumped_host``) on a vector of the Ceed: the mass apply on a vector of ones; entries of d beyond the
        L-size are zero."""
        if self.op is None:
            return pt.assign(d, self.lumped_host(), d.n)
        ones = self.ceed.vector(self.lsize).set_value(1.0)
        swap = self.mask is not None and self.mask_mode != 2
        m8 = self.mask.astype(np.uint8) if swap else None
        if swap:                          # the ones are read on the masked entries too: the residual's mask form for this one apply
            self.op.set_dirichlet_mask_mode(m8, None, 2)
        try:
            self.op.apply(ones, d)
        finally:
            if swap:
                self.op.set_dirichlet_mask_mode(m8, None, self.mask_mode)
            ones.destroy()

    def destroy(self):
        for o in (self.op, self.qf):
            if o is not None:
                o.destroy()
        self.op = self.qf = None
