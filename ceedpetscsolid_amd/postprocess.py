"""Post-processing operators on top of the path.

`StrainEnergy` mirrors `ComputeStrainEnergy` (matops.c:247-296) with the operator graph of
setuplibceed.c:651-670: du --GRAD(basisu)--> {LinElas,HyperSS,HyperFS}Energy with qdata
--INTERP^T(basisEnergy, 1 component)--> energy L-vector, whose sum is the strain energy.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import ceed as cd
from . import portable as pt
from .solid import SolidProblem

ENERGY_QF = {"linElas": ("linElas.h", "LinElasEnergy"), "hyperSS": ("hyperSS.h", "HyperSSEnergy"),
             "hyperFS": ("hyperFS.h", "HyperFSEnergy")}


class StrainEnergy:
    def __init__(self, prob: SolidProblem, problem: str):
        self.p = prob
        c = prob.ceed
        lv = prob.levels[prob.fine]
        P, Q = lv.degree + 1, prob.Q
        ne = prob.mesh.nelem
        src, name = ENERGY_QF[problem]
        self.nnodes = lv.dofmap.nnodes
        off_e = (np.asarray(lv.dofmap.offsets(), dtype=np.int64) // 3).astype(np.int32)       # one dof per node
        self.rstr = c.elem_restriction(ne, P ** 3, 1, 1, self.nnodes, off_e)                   # ErestrictEnergy
        self.basis = c.basis_lagrange(3, 1, P, Q, cd.GAUSS)                                   # basisEnergy, :343-345
        self.qf = c.qfunction(name, source=f"qfunctions/{src}:{name}")
        self.qf.add_input("du", 9, cd.EVAL_GRAD).add_input("qdata", 10, cd.EVAL_NONE).add_output("energy", 1, cd.EVAL_INTERP)
        self.qf.set_context(prob.phys)
        self.op = c.operator(self.qf)
        self.op.set_field("du", lv.Erestrictu, lv.basisu, "active")
        self.op.set_field("qdata", prob.Erestrictqdi, None, prob.qdata)
        self.op.set_field("energy", self.rstr, self.basis, "active")
        self.eloc = c.vector(self.nnodes)

    def compute(self, xloc: cd.Vector) -> float:
        """xloc: the local displacement vector with the boundary values inserted (matops.c:256-261)."""
        self.op.apply(xloc, self.eloc)
        return float(self.eloc.to_numpy().sum())

    def destroy(self):
        for o in (self.op, self.qf, self.basis, self.rstr, self.eloc):
            o.destroy()


STRESS_QF = {"linElas": ("linElas.h", "LinElasStress"), "hyperSS": ("hyperSS.h", "HyperSSStress"),
             "hyperFS": ("hyperFS.h", "HyperFSStress")}
VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))          # xx, yy, zz, yz, xz, xy: the packing of hyperFS.h:91


def _series4(x):
    """2 atanh(x / (2 + x)) to four terms: the reference's log1p (hyperSS.h:43-55), not libm's -- they differ by up to 3e-8"""
    y = x / (2.0 + x)
    y2 = y * y
    s = y.copy()
    y = y * y2; s += y * (1.0 / 3)
    y = y * y2; s += y * (1.0 / 5)
    y = y * y2; s += y * (1.0 / 7)
    return 2 * s


def _series4_shifted(x):
    """the same with the range shifts of hyperFS.h:45-67"""
    sqrt2, ln2h = 1.4142135623730951, 0.6931471805599453 / 2
    lo, hi = x < sqrt2 / 2 - 1, x > sqrt2 - 1
    return 2 * np.where(lo, -ln2h, np.where(hi, ln2h, 0.0)) + _series4(np.where(lo, 1 + 2 * x, np.where(hi, (x - 1) / 2, x)))


def stress_law(problem: str, nu: float, E: float, g: np.ndarray, iso=None) -> np.ndarray:
    """The Cauchy stress THE RESIDUAL INTEGRATES at physical gradients g[..., c, k] = d u_c / d x_k, as [..., 6] in the order xx, yy, zz,
    yz, xz, xy (float64 NumPy; the portable form of ``Stress`` and the device kernel's yardstick).

    linElas: sigma as linElas.h:133-139 WRITES it -- the shear entries are ss (1 - 2 nu) e_ij / 2 = mu e_ij with the TENSOR strain e_ij,
    HALF of Hooke's 2 mu e_ij.  That quirk of the reference makes the model anisotropic; the stress reported is the one the residual
    integrates and is NOT corrected here.  hyperSS: lambda log1p(tr e) I + 2 mu e.  hyperFS: F S F^T / det F, S = lambda ln J C^-1 +
    mu C^-1 (C - I) (= mu I + (lambda ln J - mu) C^-1, in the residual's cancellation-free form).  Both logarithms are the reference's
    four-term series.

    ``iso`` (optional, broadcast over the points): beta theta_h of a thermal field (thermal.py); the stress is then sigma - iso I
    (linElas, hyperSS) or sigma - (iso / det F) I (hyperFS), the stress the residual with the thermal term integrates."""
    g = np.asarray(g, dtype=np.float64)
    two_mu = E / (1 + nu)
    lam = (3 * (E / (3 * (1 - 2 * nu))) - two_mu) / 3
    gt = np.swapaxes(g, -1, -2)
    eye = np.eye(3)
    if problem == "linElas":
        e = (g + gt) / 2
        ss = E / ((1 + nu) * (1 - 2 * nu))
        sig = ss * (1 - 2 * nu) * e * 0.5
        tr = e[..., 0, 0] + e[..., 1, 1] + e[..., 2, 2]
        for a in range(3):
            sig[..., a, a] = ss * ((1 - 2 * nu) * e[..., a, a] + nu * tr)
    elif problem == "hyperSS":
        e = (g + gt) / 2
        sig = two_mu * e + (lam * _series4(e[..., 0, 0] + e[..., 1, 1] + e[..., 2, 2]))[..., None, None] * eye
    elif problem == "hyperFS":
        mu = two_mu / 2
        E2 = g + gt + gt @ g
        a, b, c, d, e_, f = E2[..., 0, 0], E2[..., 1, 1], E2[..., 2, 2], E2[..., 1, 2], E2[..., 0, 2], E2[..., 0, 1]
        det_c_m1 = (a * (b * c - d * d) + f * (e_ * d - f * c) + e_ * (f * d - e_ * b) + a + b + c + a * b + a * c + b * c
                    - f * f - e_ * e_ - d * d)                                                   # hyperFS.h:72-80
        C = E2 + eye
        adj = np.empty_like(C)
        for r in range(3):
            for s in range(3):
                r1, r2, s1, s2 = (r + 1) % 3, (r + 2) % 3, (s + 1) % 3, (s + 2) % 3
                adj[..., r, s] = C[..., s1, r1] * C[..., s2, r2] - C[..., s1, r2] * C[..., s2, r1]
        Cinv = adj / (det_c_m1 + 1)[..., None, None]
        S = (lam * _series4_shifted(det_c_m1) / 2)[..., None, None] * Cinv + mu * (Cinv @ E2)
        F = g + eye
        sig = F @ S @ np.swapaxes(F, -1, -2) / np.linalg.det(F)[..., None, None]
    else:
        raise ValueError(f"unknown problem {problem!r}")
    if iso is not None:
        iso = np.asarray(iso, dtype=np.float64)
        if problem == "hyperFS":
            iso = iso / np.linalg.det(g + eye)
        sig = sig - iso[..., None, None] * eye
    return np.stack([sig[..., i, j] for i, j in VOIGT], axis=-1)


class Stress:
    """Stress recovery on the fine level: the Cauchy stress THE RESIDUAL INTEGRATES (``stress_law``), six components in the
    order xx, yy, zz, yz, xz, xy, at the quadrature points and, by the lumped L2 projection

        sigma_a = sum_e sum_q N_a(q) w det J sigma(q) / sum_e sum_q N_a(q) w det J,

    at the nodes.  NOTE for ``linElas``: the reference's shear entries are mu e_ij, half of Hooke's law (linElas.h:137-139); the
    stress reported keeps that, so the virtual work of it IS the residual and reactions computed from it agree with the solver.

    ``xloc`` is the local displacement vector WITH the boundary values inserted, as ``StrainEnergy`` and ``Diagnostics`` take it.  On the
    device these are two operator graphs of the QFunctions ``{LinElas,HyperSS,HyperFS}Stress`` (csrc/kernels_stress.hip): (du GRAD
    active, qdata NONE) -> stress NONE(6) on a strided restriction, or -> stress INTERP(7) -- w det J {sigma, 1} summed per node in
    element order -- on a 7-component restriction.  Where the library has no functor of that name (the CPU oracle), or with
    ``portable=True``, the same sums are formed in NumPy on the tensor layer of ``portable.py`` with the tables of ``lv.basisu`` and the
    quadrature data read back once (which form runs where, and why it is the device tests' yardstick: DESIGN.md 2).  Several ranks
    are refused: the interface nodes of an element partition would need both sums exchanged."""

    def __init__(self, prob: SolidProblem, problem: str, portable: Optional[bool] = None, halo=None, thermal=None):
        """``thermal``: a ``thermal.ThermalLoad`` of the fine level, or dict(alpha=, theta=) from which one is made (and owned): the stress
        reported is then the one the residual with the thermal term integrates, sigma - beta theta_h I (hyperFS: / det F), with the
        load's current ``scale`` on theta.  With ``thermal=None`` this is the object it was."""
        if problem not in STRESS_QF:
            raise ValueError(f"unknown problem {problem!r}")
        hl = halo if halo is None or isinstance(halo, (list, tuple)) else [halo]
        if prob._shared_multiplicity is not None or (hl and hl[-1].world > 1):
            raise ValueError("Stress is not provided with a halo (several ranks): the interface nodes of an element partition need the "
                             "weighted stress sums and the nodal volumes exchanged before the division")
        import torch
        self._torch = torch
        self.p, self.problem = prob, problem
        c = self.ceed = prob.ceed
        lv = self.lv = prob.levels[prob.fine]
        self.P, self.Q, self.ne = lv.degree + 1, prob.Q, prob.mesh.nelem
        self.nnodes = lv.dofmap.nnodes
        self.nu, self.E = float(prob.phys[0]), float(prob.phys[1])
        self.offsets = (np.asarray(lv.dofmap.offsets(), dtype=np.int64) & 0x1FFFFFFF).reshape(self.ne, self.P ** 3)
        self.nodes = (self.offsets // 3).reshape((self.ne,) + 3 * (self.P,))                      # [e][k][j][i]
        src, name = STRESS_QF[problem]
        self.thermal, self._own_thermal = None, False
        if thermal is not None:
            from .thermal import ThermalLoad
            name += "Thermal"
            self._own_thermal = not isinstance(thermal, ThermalLoad)
            if self._own_thermal and (not isinstance(thermal, dict) or set(thermal) != {"alpha", "theta"}):
                raise ValueError("Stress: thermal is a thermal.ThermalLoad or dict(alpha=, theta=)")
        self.portable = (not c.has_qfunction(name)) if portable is None else bool(portable)
        if thermal is not None:
            self.thermal = ThermalLoad(prob, prob.fine, thermal["alpha"], thermal["theta"], problem, portable=self.portable) if self._own_thermal else thermal
            if self.thermal.problem != problem or self.thermal.lv is not lv or (not self.portable and self.thermal.portable):
                raise ValueError("Stress: the thermal load must be one of the fine level, of the same problem and, for the device form, on the device")
        self._tab = None
        self._have_volume = False
        self.qf_pts = self.qf_nod = self.op_pts = self.op_nod = self.rstr_pts = self.rstr_nod = self.basis_nod = None
        npts = self.ne * self.Q ** 3
        device = "cpu" if self.portable else "cuda"
        self.spts = c.tensor_vector(6 * npts, device)            # [elem][6][Q^3]
        self.snod = c.tensor_vector(7 * self.nnodes, device)     # [node][7]: w det J {sigma, 1} summed, then sigma in place
        if not self.portable:
            P3, Q3 = self.P ** 3, self.Q ** 3
            self.rstr_pts = c.strided_restriction(self.ne, Q3, 6, 6 * npts)
            self.rstr_nod = c.elem_restriction(self.ne, P3, 7, 1, 7 * self.nnodes, (self.offsets // 3 * 7).astype(np.int32))
            self.basis_nod = c.basis_lagrange(3, 7, self.P, self.Q, cd.GAUSS)
            self.qf_pts, self.op_pts = self._graph(src, name, 6, cd.EVAL_NONE, self.rstr_pts, None)
            self.qf_nod, self.op_nod = self._graph(src, name, 7, cd.EVAL_INTERP, self.rstr_nod, self.basis_nod)

    def _graph(self, src, name, size, emode, rstr, basis):
        c, lv, tl = self.ceed, self.lv, self.thermal
        qf = c.qfunction(name, source=f"qfunctions/{src}:{name}")
        qf.add_input("du", 9, cd.EVAL_GRAD)
        if tl is not None:
            qf.add_input("theta", 1, cd.EVAL_INTERP)
        qf.add_input("qdata", 10, cd.EVAL_NONE).add_output("stress", size, emode)
        qf.set_context(self.p.phys if tl is None else [self.nu, self.E, tl.alpha * tl.scale])
        op = c.operator(qf)
        op.set_field("du", lv.Erestrictu, lv.basisu, "active")
        if tl is not None:
            op.set_field("theta", tl.theta_rstr, tl.theta_basis, tl.theta_vec)
        op.set_field("qdata", self.p.Erestrictqdi, None, self.p.qdata)
        op.set_field("stress", rstr, basis, "active")
        return qf, op

    @property
    def kernel_names(self) -> dict:
        """The kernels of the last ``points`` and ``nodal`` (``"portable"`` for the NumPy form, ``""`` before the first apply)."""
        if self.portable:
            return {"points": "portable", "nodal": "portable"}
        return {"points": self.op_pts.kernel_name, "nodal": self.op_nod.kernel_name}

    # ---- the portable form: NumPy on host arrays ---------------------------------------------------------------------------
    def _tables(self):
        if self._tab is None:
            Q = self.Q
            qd = self.lv.qdata.to_numpy().reshape(self.ne, 10, Q, Q, Q)
            self._tab = (self.lv.basisu.interp1d, self.lv.basisu.grad1d, qd[:, 0].copy(),
                         qd[:, 1:].reshape(self.ne, 3, 3, Q, Q, Q).copy())                 # B, G [q][p]; w det J [e][k][j][i]; dXdx [e][r][s][k][j][i]
        return self._tab

    def grad_host(self, x) -> np.ndarray:
        """The physical displacement gradient at the points, [nelem][Q][Q][Q][c][n] = d u_c / d x_n, from a host array."""
        B, G, _, dX = self._tables()
        ue = pt.gather(x, self.nodes, 3 * self.nnodes)                                     # [e][k][j][i][c]
        du = np.stack([pt.to_points(ue, *t) for t in ((G, B, B), (B, G, B), (B, B, G))], axis=-1)          # [e][k][j][i][c][m]
        return np.einsum("ekjicm,emnkji->ekjicn", du, dX)                                  # g[c][n] = sum_m du[c][m] dXdx[m][n]

    def points_host(self, x) -> np.ndarray:
        """[nelem][6][Q^3] from a host array."""
        tl = self.thermal
        iso = None if tl is None else tl.beta * tl.scale * tl.theta_points()
        sig = stress_law(self.problem, self.nu, self.E, self.grad_host(x), iso)            # [e][k][j][i][6]
        return np.ascontiguousarray(np.moveaxis(sig, -1, 1)).reshape(self.ne, 6, self.Q ** 3)

    def nodal_sums_host(self, x) -> np.ndarray:
        """[nnodes][7]: w det J {sigma, 1} through B^T, element contributions added in element order."""
        B, _, W, _ = self._tables()
        Q = self.Q
        v = np.concatenate([self.points_host(x).reshape(self.ne, 6, Q, Q, Q), np.ones((self.ne, 1, Q, Q, Q))], axis=1) * W[:, None]
        return pt.node_sum(self.nodes, pt.to_nodes(np.moveaxis(v, 1, -1), B, B, B), self.nnodes)      # (a view: v stays [e][m][d][b][a])

    # ---- on vectors of the Ceed ----------------------------------------------------------------------------------------------
    def _sync(self):
        """The Ceed's stream and torch's are ordered by the host: post-processing, never inside a recording."""
        if not self.portable and self.thermal is not None:       # the load's current scale on theta rides in the context's alpha
            self.qf_pts._ctx[2] = self.qf_nod._ctx[2] = self.thermal.alpha * self.thermal.scale
        if not self.portable:
            self.ceed.synchronize()
            self._torch.cuda.current_stream().synchronize()

    def points(self, xloc: cd.Vector, numpy: bool = True):
        """The stress at the quadrature points, [nelem][6][Q^3] (point i + Q (j + Q k)): a host copy, or with ``numpy=False`` the
        tensor behind the output vector (valid until the next call)."""
        if self.portable:
            pt.assign(self.spts, self.points_host(xloc.to_numpy()))
        else:
            self._sync()
            self.op_pts.apply(xloc, self.spts)
            self._sync()
        t = self.spts.t.view(self.ne, 6, self.Q ** 3)
        return t.cpu().numpy().copy() if numpy else t

    def _nodal(self, xloc: Optional[cd.Vector]):
        torch = self._torch
        if self.portable:
            x = np.zeros(self.lv.dofmap.lsize) if xloc is None else xloc.to_numpy()
            pt.assign(self.snod, self.nodal_sums_host(x))
        else:
            x = xloc if xloc is not None else self.ceed.vector(self.lv.dofmap.lsize).set_value(0.0)
            self._sync()
            self.op_nod.apply(x, self.snod)
            self._sync()
            if xloc is None:
                x.destroy()
        t = self.snod.t.view(self.nnodes, 7)
        s, w = t[:, :6], t[:, 6:7]
        s.copy_(torch.where(w > 0, s / w, torch.zeros((), dtype=t.dtype, device=t.device)))      # a node no element holds: volume 0, stress 0
        self.snod.touched()
        self._sync()
        self._have_volume = True
        return t

    def nodal(self, xloc: cd.Vector, numpy: bool = True):
        """The stress at the nodes, [nnodes][6]; zero at a node no element holds."""
        t = self._nodal(xloc)[:, :6]
        return t.cpu().numpy().copy() if numpy else t

    def nodal_volume(self, numpy: bool = True):
        """The denominator of the projection, [nnodes]: sum_e sum_q N_a(q) w det J (it sums to the volume of the mesh)."""
        if not self._have_volume:
            self._nodal(None)
        t = self.snod.t.view(self.nnodes, 7)[:, 6]
        return t.cpu().numpy().copy() if numpy else t

    @staticmethod
    def von_mises(sigma):
        """sqrt(3/2 s:s), s = sigma - tr sigma / 3 I, of any [..., 6] array or tensor in the order xx, yy, zz, yz, xz, xy."""
        xx, yy, zz, yz, xz, xy = (sigma[..., i] for i in range(6))
        j = 0.5 * ((xx - yy) ** 2 + (yy - zz) ** 2 + (zz - xx) ** 2) + 3.0 * (yz ** 2 + xz ** 2 + xy ** 2)
        return np.sqrt(j) if isinstance(j, (np.ndarray, np.generic, float)) else j.sqrt()

    def max_von_mises(self, xloc: cd.Vector):
        """(the largest nodal von Mises stress, its node), reduced with torch on the memory the nodal stress lives in."""
        vm = self.von_mises(self.nodal(xloc, numpy=False))
        node = self._torch.argmax(vm)
        return float(vm[node]), int(node)

    def destroy(self):
        if self._own_thermal and self.thermal is not None:
            self.thermal.destroy()
        self.thermal = None
        for o in (self.op_pts, self.op_nod, self.qf_pts, self.qf_nod, self.basis_nod, self.rstr_pts, self.rstr_nod, self.spts, self.snod):
            if o is not None:
                o.destroy()
        self.op_pts = self.op_nod = self.qf_pts = self.qf_nod = self.basis_nod = self.rstr_pts = self.rstr_nod = self.spts = self.snod = None


DIAG_QF = {"linElas": ("linElas.h", "LinElasDiagnostic"), "hyperSS": ("hyperSS.h", "HyperSSDiagnostic"),
           "hyperFS": ("hyperFS.h", "HyperFSDiagnostic")}
DIAG_FIELDS = ("displacement_x", "displacement_y", "displacement_z", "pressure", "trace_E", "trace_E2", "det_J",
               "strain_energy_density")          # elasticity.c:181-188


class Diagnostics:
    """opDiagnostic (setuplibceed.c:679-737) + the multiplicity division of ViewDiagnosticQuantities
    (misc.c:217-311): the 8 nodal diagnostic fields of the fine level, evaluated on the GLL points
    (= the nodes) with a second SetupGeo on those points."""

    def __init__(self, prob: SolidProblem, problem: str):
        self.p = prob
        c = prob.ceed
        lv = prob.levels[prob.fine]
        P = lv.degree + 1
        ne, P3 = prob.mesh.nelem, P ** 3
        self.nnodes = lv.dofmap.nnodes
        # geometry on the GLL points (:679-708)
        self.basisx = c.basis_lagrange(3, 3, 2, P, cd.GAUSS_LOBATTO)
        self.rstr_qd = c.strided_restriction(ne, P3, 10, 10 * ne * P3)
        self.qdata = c.vector(10 * ne * P3)
        qfg = c.qfunction("SetupGeo", source="qfunctions/common.h:SetupGeo")
        qfg.add_input("dx", 9, cd.EVAL_GRAD).add_input("weight", 1, cd.EVAL_WEIGHT).add_output("qdata", 10, cd.EVAL_NONE)
        opg = c.operator(qfg)
        opg.set_field("dx", prob.Erestrictx, self.basisx, "active")
        opg.set_field("weight", None, self.basisx, None)
        opg.set_field("qdata", self.rstr_qd, None, "active")
        opg.apply(prob.xcoord, self.qdata)
        opg.destroy(); qfg.destroy()
        # the diagnostic operator (:712-737)
        self.basis = c.basis_lagrange(3, 3, P, P, cd.GAUSS_LOBATTO)                           # basisDiagnostic, :347-348
        off_d = (np.asarray(lv.dofmap.offsets(), dtype=np.int64) // 3 * 8).astype(np.int32)
        self.rstr = c.elem_restriction(ne, P3, 8, 1, 8 * self.nnodes, off_d)                  # ErestrictDiagnostic
        src, name = DIAG_QF[problem]
        self.qf = c.qfunction(name, source=f"qfunctions/{src}:{name}")
        self.qf.add_input("u", 3, cd.EVAL_INTERP).add_input("du", 9, cd.EVAL_GRAD).add_input("qdata", 10, cd.EVAL_NONE)
        self.qf.add_output("diagnostic", 8, cd.EVAL_NONE)
        self.qf.set_context(prob.phys)
        self.op = c.operator(self.qf)
        self.op.set_field("u", lv.Erestrictu, self.basis, "active")
        self.op.set_field("du", lv.Erestrictu, self.basis, "active")
        self.op.set_field("qdata", self.rstr_qd, None, self.qdata)
        self.op.set_field("diagnostic", self.rstr, None, "active")
        self.dloc = c.vector(8 * self.nnodes)
        m = c.vector(prob.lsize())
        lv.Erestrictu.multiplicity(m)
        self.mult = m.to_numpy().reshape(-1, 3)[:, 0].copy()

    def compute(self, xloc: cd.Vector) -> np.ndarray:
        """[nnodes][8] nodal fields (DIAG_FIELDS), averaged over the elements sharing each node."""
        self.op.apply(xloc, self.dloc)
        return self.dloc.to_numpy().reshape(self.nnodes, 8) / self.mult[:, None]
