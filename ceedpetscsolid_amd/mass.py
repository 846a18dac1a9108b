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

A density FIELD (``DensityField``, ``MassOperator(..., density=field)``) makes the operator c M_rho,

    (M_rho x)_a,c = sum_e sum_q N_a(q) rho_h(e, q) w_q det J_e(q) sum_b N_b(q) x_b,c,     rho_h(e, q) = sum_m N_m(q) rho(e, m),

the density interpolated with the basis of x from a scalar vector through a restriction of its own on the level's nodes: a continuous
one for a nodal field, an element-discontinuous one (offsets e P^3 + n) for per-element values.  On the device that is the QFunction
``MassField`` (include/ceed.h; k_mass's modes with a field); the portable form multiplies w det J by ``to_points(gather(rho))`` once.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import ceed as cd
from . import portable as pt
from .solid import SolidProblem


def _positive(values, what: str) -> np.ndarray:
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    if v.size == 0 or not np.all(np.isfinite(v)) or not np.all(v > 0.0):
        raise ValueError(f"{what}: every density must be finite and positive (high-order interpolation of a non-positive nodal field "
                         "can give a negative density at a point)")
    return v


class DensityField:
    """A density that varies over the body: ``nodal`` (continuous, one value per node of a level) or ``per_element`` (one value per
    element, the same on every p-multigrid level, which keeps the elements)."""

    def __init__(self, kind: str, values=None, fn=None):
        self.kind, self.values, self.fn = kind, values, fn

    @classmethod
    def nodal(cls, f) -> "DensityField":
        """``f``: a callable ``f(X) -> (n,)`` on node coordinates ``X`` (n, 3), evaluated on each level's nodes, or an array
        ``(nnodes,)`` that holds on the fine level only."""
        if callable(f):
            return cls("nodal", fn=f)
        a = np.asarray(f, dtype=np.float64)
        if a.ndim != 1:
            raise ValueError(f"DensityField.nodal: an array of nodal values has shape (nnodes,), not {a.shape}")
        return cls("nodal", values=_positive(a, "DensityField.nodal"))

    @classmethod
    def per_element(cls, values) -> "DensityField":
        a = np.asarray(values, dtype=np.float64)
        if a.ndim != 1:
            raise ValueError(f"DensityField.per_element: the values have shape (nelem,), not {a.shape}")
        return cls("per_element", values=_positive(a, "DensityField.per_element"))

    def on_level(self, prob: SolidProblem, level: int):
        """(rho, offsets): the scalar vector of the level and the plain indices [nelem][P^3] of every element's nodes into it."""
        lv, ne = prob.levels[level], prob.mesh.nelem
        dm = lv.dofmap
        P3 = (lv.degree + 1) ** 3
        if self.kind == "per_element":
            if self.values.size != ne:
                raise ValueError(f"DensityField.per_element: {self.values.size} values for {ne} elements")
            return np.repeat(self.values, P3), np.arange(ne * P3, dtype=np.int64).reshape(ne, P3)
        if self.fn is not None:
            rho = np.asarray(self.fn(np.asarray(dm.node_coords)), dtype=np.float64)
            if rho.shape != (dm.nnodes,):
                raise ValueError(f"DensityField.nodal: the callable returned shape {rho.shape} for {dm.nnodes} nodes")
            rho = _positive(rho, "DensityField.nodal")
        else:
            if level != prob.fine:
                raise ValueError(f"DensityField.nodal: an array of nodal values holds on the fine level only, not on level {level}: "
                                 "give a callable or per-element values")
            if self.values.size != dm.nnodes:
                raise ValueError(f"DensityField.nodal: {self.values.size} values for the {dm.nnodes} nodes of the fine level")
            rho = self.values
        return rho.copy(), np.asarray(dm.elem_nodes, dtype=np.int64).reshape(ne, P3)


def split_density(density, message: str):
    """(rho, field) of a solver's ``density``: a positive float is (rho, None); a ``DensityField`` is (1.0, field), so that every
    coefficient the solver forms with rho (a0 rho, ...) multiplies M_rho as it multiplied M.  Anything else is a ValueError with the caller's ``message``."""
    if isinstance(density, DensityField):
        return 1.0, density
    if not (isinstance(density, (int, float, np.integer, np.floating)) and density > 0.0):
        raise ValueError(message)
    return float(density), None


class MassOperator:
    def __init__(self, prob: SolidProblem, level: int, coef: float, portable: Optional[bool] = None,
                 rstr: Optional[cd.ElemRestriction] = None, offsets=None, mask_mode: int = 3, density: Optional[DensityField] = None):
        """``rstr`` / ``offsets``: a restriction of the caller's on the level's elements and nodes-per-element (and its component-0
        offsets, [nelem][P^3], for the portable form) in place of the level's own -- the element-discontinuous one of
        ``assembly.AssembledLevel``; no mask is applied then.  ``density``: a ``DensityField`` -- the operator is then ``coef`` M_rho;
        rho always goes through a restriction of its own on the level's nodes, whatever the restriction of x."""
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
        if density is not None and not isinstance(density, DensityField):
            raise ValueError(f"density must be a DensityField (a constant density is the coefficient), not {type(density).__name__}")
        self.density = density
        self.rho = self.rho_nodes = self.rho_vec = self.rho_rstr = self.rho_basis = None
        if density is not None:
            self.rho, self.rho_nodes = density.on_level(prob, level)                              # [n], [e][P^3]
        name = "Mass" if density is None else "MassField"
        self.portable = (not c.has_qfunction(name)) if portable is None else bool(portable)
        self._B = self._W = None
        self.qf = self.op = None
        if not self.portable and density is not None:
            P3 = self.P ** 3
            self.rho_vec = c.vector(self.rho.size).set_array(self.rho)
            self.rho_rstr = c.elem_restriction(self.ne, P3, 1, 1, self.rho.size, self.rho_nodes.astype(np.int32).reshape(-1))
            self.rho_basis = c.basis_lagrange(3, 1, self.P, self.Q, cd.GAUSS)
            self.qf = c.qfunction("MassField", source="qfunctions/mass.h:MassField")
            self.qf.add_input("u", 3, cd.EVAL_INTERP).add_input("rho", 1, cd.EVAL_INTERP).add_input("qdata", 10, cd.EVAL_NONE)
            self.qf.add_output("v", 3, cd.EVAL_INTERP)
            self.qf.set_context([self.coef])
            self.op = c.operator(self.qf)
            self.op.set_field("u", self.rstr, lv.basisu, "active")
            self.op.set_field("rho", self.rho_rstr, self.rho_basis, self.rho_vec)
            self.op.set_field("qdata", lv.Erestrictqdi, None, lv.qdata)
            self.op.set_field("v", self.rstr, lv.basisu, "active")
            if self.mask is not None:
                self.op.set_dirichlet_mask_mode(self.mask.astype(np.uint8), None, mask_mode)
        elif not self.portable:
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
            if self.rho is not None:                                                            # rho_h w det J at the points
                B = self._B
                self._W *= pt.to_points(self.rho[self.rho_nodes].reshape((self.ne,) + 3 * (self.P,)), B, B, B)
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

    def set_density_values(self, rho):
        """New values of the scalar density vector (``self.rho``'s layout), written behind the same address: a recorded apply sees them."""
        rho = _positive(rho, "set_density_values")
        if self.rho is None or rho.size != self.rho.size:
            raise ValueError("set_density_values: the operator has no density field of that size")
        self.rho, self._B, self._W = rho.copy(), None, None
        if self.rho_vec is not None:
            self.rho_vec.fill(self.rho)
            if self.ceed.preferred_memtype == cd.MEM_DEVICE:
                self.rho_vec.device_pointer()               # on the device now: a replay reads the address, it runs no host code

    def destroy(self):
        for o in (self.op, self.qf, self.rho_rstr, self.rho_basis, self.rho_vec):
            if o is not None:
                o.destroy()
        self.op = self.qf = self.rho_rstr = self.rho_basis = self.rho_vec = None
