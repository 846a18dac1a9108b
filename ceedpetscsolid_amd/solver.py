"""Newton - CG - p-multigrid solve on top of the operator path (BASELINE config 3).

The reference wires this out of PETSc objects (elasticity.c:386-673): SNES Newton with the
critical-point line search (:596-601) over load increments (:637-673); KSPCG in the natural norm,
rtol 1e-10 (:504-507); PCMG multiplicative V-cycle with 3 Chebyshev(+Jacobi) smoothing steps per
level, eigenvalue bounds (0, 0.1, 0, 1.1) x the estimate (:539-552, :588-590); prolongation /
restriction MatShells (Prolong_Ceed / Restrict_Ceed); a coarse solve by GAMG on the FD-coloured
p=1 matrix (:457-483,:568-585).  PETSc is absent here, so this is this build's own control flow with
the same structure; every vector and operator operation runs on the device through the C ABI
(CeedOperatorApply, CeedOperatorLinearAssembleDiagonal, CeedX vector helpers), through the methods of ceed.py; the eigenvalue
estimate and the Chebyshev coefficients of the smoother are those of krylov.py.  The coarse level is solved, by choice
(``coarse``): by Jacobi-preconditioned CG on the p=1 operator itself ("cg", the default), by a fixed Chebyshev polynomial on that
operator ("chebyshev") or on the assembled p=1 matrix ("assembled", assembly.py), or by one cycle of a smoothed-aggregation
hierarchy on the assembled matrix ("amg", amg.py: what the reference asks of PCGAMG).  Because the CG coarse solve makes the
preconditioner mildly non-linear the outer Krylov method is the flexible (Polak-Ribiere) CG, which coincides with CG for a
fixed preconditioner.

Iteration counts are therefore this build's own, not PETSc's; the throughput figure reported is the
reference's "DoFs/Sec in SNES" = 1e-6 * Ugsz * (total KSP iterations) / (solve time)
(elasticity.c:755-764).
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np

from . import ceed as cd
from .krylov import chebyshev_coefficients, lanczos_device, lanczos_emax
from .solid import SolidProblem


# ---- boundary functions (src/boundary.c) -------------------------------------------------------
def bc_mms(X: np.ndarray, load: float) -> np.ndarray:
    """BCMMS, boundary.c:31-50."""
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    return np.stack([np.exp(2 * x) * np.sin(3 * y) * np.cos(4 * z), np.exp(3 * y) * np.sin(4 * z) * np.cos(2 * x),
                     np.exp(4 * z) * np.sin(2 * x) * np.cos(3 * y)], axis=1) / 1e8 * load


def bc_clamp(X: np.ndarray, load: float, translate=(0., 0., 0.), axis=(0., 0., 1.), angle_over_pi: float = 0.0) -> np.ndarray:
    """BCClamp, boundary.c:53-74: translation + rotation about `axis` by angle_over_pi*pi, scaled by the load
    fraction.  The x-component's (1-c) term is reproduced AS WRITTEN at boundary.c:69
    (`-ky*ky + kz*kz*x + ...`)."""
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    lx, ly, lz = (t * load for t in translate)
    kx, ky, kz = axis
    th = angle_over_pi * np.pi * load
    c, s = np.cos(th), np.sin(th)
    u0 = lx + s * (-kz * y + ky * z) + (1 - c) * (-ky * ky + kz * kz * x + kx * ky * y + kx * kz * z)
    u1 = ly + s * (kz * x + -kx * z) + (1 - c) * (kx * ky * x - (kx * kx + kz * kz) * y + ky * kz * z)
    u2 = lz + s * (-ky * x + kx * y) + (1 - c) * (kx * kz * x + ky * kz * y - (kx * kx + ky * ky) * z)
    return np.stack([u0, u1, u2], axis=1)


@dataclass
class SolveStats:
    newton_its: int = 0
    ksp_its: int = 0
    coarse_its: int = 0
    jacobian_applies: int = 0
    coarse_spmv: int = 0
    residual_evals: int = 0
    seconds: float = 0.0
    increments: int = 0
    converged: bool = True
    history: list = field(default_factory=list)
    initial_residuals: list = field(default_factory=list)   # |R| at the start of every load increment (what snes_rtol is relative to)


class NewtonPMG:
    _asm_kwargs: dict = {}          # keywords of the assembled coarse level (dynamics.NewmarkPMG: its mass term); none here

    def __init__(self, prob: SolidProblem, clamp: Optional[Dict[int, dict]] = None, mms: bool = False, forcing=None,
                 halo=None, rccl="auto", lead_elements: int = 0, smooth_its: int = 3, coarse_rtol: float = 1e-3, coarse_maxit: int = 200,
                 coarse: str = "cg", coarse_cheb_its: int = 40, coarse_cheb_ratio: float = 100.0, graph: bool = False,
                 amg_smooth_its: int = 3, amg_smooth_ratio: float = 10.0, amg_max_coarse_dofs: int = 1500, amg_coarse_cycles: int = 1,
                 ksp_rtol: float = 1e-10, snes_rtol: float = 1e-8, snes_maxit: int = 50, verbose: bool = False,
                 line_search: str = "cp", fuse_epilogue: bool = True, smoother: str = "jacobi",
                 traction: Optional[Dict[int, tuple]] = None, pressure: Optional[Dict[int, float]] = None, pressure_tangent: str = "full"):
        """``clamp``: {side_set_id: dict(translate=(..), axis=(..), angle_over_pi=..)} as
        -bc_clamp_<id>_translate / _rotate (cloptions.c:86-131); ids present in the problem's Dirichlet
        set but absent here are held at zero.
        Surface loads (surface.py; one rank, and never on a clamped side set):
        ``traction``: {side_set_id: (tx, ty, tz)} -- a dead load per unit REFERENCE area acting on the body in the direction t, scaled by
        the load fraction like the body force; evaluated once and folded into the load vector.
        ``pressure``: {side_set_id: p} -- a pressure on the CURRENT surface, p > 0 pushing on the body, scaled by the load fraction;
        evaluated in every residual, R = F_int(u) - load (f + sum_s g_s^traction) + load sum_s p_s g_s^pressure(u).
        ``pressure_tangent``: "full" adds load sum_s p_s T_s(u) to the Jacobian of the OUTER Krylov iteration (the V-cycle, its
        smoothers, diagonals and eigenvalue estimates do not see it: the preconditioner is the volume operator's); "none" omits it
        (modified Newton).  T(u) is symmetric only on the variations that vanish on the rim of the loaded surface: a closed surface, or
        a patch whose rim is clamped (a tube with clamped ends).  The outer CG assumes a symmetric operator; a follower pressure on a
        patch with a free rim is the caller's responsibility, as with any non-conservative load."""
        self.p, self.ceed, self.L = prob, prob.ceed, prob.ceed.L
        # smoother: what the Chebyshev iteration of every p-multigrid level, its eigenvalue estimate and the Jacobi-preconditioned
        # coarse CG are preconditioned with -- "jacobi" (default, the reference: PCJACOBI on GetDiag_Ceed) or "pbjacobi": the inverted
        # 3 x 3 nodal blocks (PCPBJACOBI on CeedOperatorLinearAssemblePointBlockDiagonal), which keep the coupling between the
        # displacement components of a node that the scalar diagonal drops.  One rank only: the blocks of the interface nodes of
        # an element partition would have to be summed over the ranks before they are inverted, and no exchange here carries nine
        # values per node.
        if smoother not in ("jacobi", "pbjacobi"):
            raise ValueError(f"smoother must be 'jacobi' or 'pbjacobi', not {smoother!r}")
        # Several ranks (one element partition per rank, halo.py): `halo` is one HaloExchange per multigrid level (a single one stands
        # for a one-level list).  Every vector then aliases a torch tensor (host memory for the CPU oracle, device memory otherwise;
        # the Ceed's stream must be torch's current stream, as in bench.py), so the interface sums of halo.add() act on the operators'
        # outputs in place: the L -> G sum of matops.c:57 after each Jacobian / residual / transfer / diagonal.  Dots are owner-weighted.
        single = halo is not None and not isinstance(halo, (list, tuple))
        halo = [halo] if single else halo
        many = halo is not None and halo[-1].world > 1
        if smoother == "pbjacobi" and many:
            raise ValueError("smoother='pbjacobi' is not provided with a halo (several ranks): the nodal blocks of the interface nodes "
                             "are not summed over the ranks")
        if many and (traction or pressure):
            # partial face sums at the interface nodes would need the exchange between the add and its consumer
            raise ValueError("surface loads (traction=, pressure=) are not provided with a halo (several ranks): the face sums of the "
                             "interface nodes are not summed over the ranks")
        if many and single and len(prob.levels) > 1:
            raise ValueError("a multi-rank multigrid solve needs one HaloExchange per level")
        if many and len(halo) != len(prob.levels):
            raise ValueError("one HaloExchange per multigrid level expected")
        self.halos = list(halo) if many else None
        self.halo = self.halos[-1] if self.halos else None
        self.smoother, self._pb = smoother, smoother == "pbjacobi"
        self.clamp, self.mms = clamp or {}, mms
        # "cp": critical-point secant search, up to three secant steps, a step outside (0, 10] ends the search (this build's default);
        # "cp-petsc": SNESLINESEARCHCP with PETSc's defaults (elasticity.c:596-601 sets the type and nothing else) as recalled from its
        # source, which is NOT in this image (unverified): ONE secant step from (0, 1), downhill slope enforced, direction switched below
        # steptol, lambda kept above maxstep, never a rejection; "full": lambda = 1 (SNESLINESEARCHBASIC)
        if line_search not in ("cp", "cp-petsc", "full"):
            raise ValueError(f"line_search {line_search!r}")
        self.line_search = line_search
        # fuse_epilogue: the smoother's Chebyshev step and the V-cycle's residual formed in the epilogue of the Jacobian apply
        # (CeedXOperatorApplyChebyshev / ApplyResidual: same bits as apply + update); one rank only (no interface sum in between)
        # "auto" (either switch): the forms give the same bits, so the first call of record_preconditioner TIMES the V-cycle in each
        # combination on the problem at hand and keeps the fastest (measured, 99 000 hexes at p = 4: eager + fused 6.1 ms, graph +
        # two passes 6.4-6.6, graph + fused 6.8-7.0, eager + two passes 6.5-6.7; 5 580 hexes: the replayed graph wins by 2x)
        self._auto_fuse = fuse_epilogue == "auto"
        self.fuse_epilogue = True if self._auto_fuse else bool(fuse_epilogue)
        self.tuning = None
        self.smooth_its, self.coarse_rtol, self.coarse_maxit = smooth_its, coarse_rtol, coarse_maxit
        # coarse solver: "cg" (Jacobi-PCG to coarse_rtol: accurate, but two host-synchronised dots per
        # iteration) or "chebyshev" (fixed polynomial over [emax/ratio, 1.1 emax]: no reductions, no host
        # sync, a fixed linear operator; the few lowest modes are left to the outer Krylov method)
        self.coarse, self.coarse_cheb_its, self.coarse_cheb_ratio = coarse, coarse_cheb_its, coarse_cheb_ratio
        # graph=True: record the V-cycle (a fixed sequence of ~150 small launches once the eigenvalue
        # estimates are known) into a hipGraph per Newton step and replay it per Krylov iteration;
        # needs the reduction-free Chebyshev coarse solver
        self._auto_graph = graph == "auto"
        self.graph = False if self._auto_graph else bool(graph)
        if self._auto_graph and coarse not in ("chebyshev", "assembled", "amg"):
            self._auto_graph = False               # (the CG coarse solve cannot be recorded: eager)
        if self.graph and coarse not in ("chebyshev", "assembled", "amg"):
            raise ValueError("graph=True needs coarse='chebyshev', 'assembled' or 'amg' (the CG coarse solve reads dot products on the host)")
        # coarse="assembled": the same Chebyshev polynomial, but on the ASSEMBLED p=1 matrix (assembly.py): a
        # coarse iteration is one SpMV on 81 entries per row instead of a matrix-free apply on the fine quadrature
        # coarse="amg": ONE cycle of a two-level smoothed-aggregation hierarchy on the assembled matrix (amg.py) -- what
        # the reference asks of PCGAMG under KSPPREONLY (elasticity.c:568-585): Chebyshev(amg_smooth_its) on
        # [emax / amg_smooth_ratio, 1.1 emax], the rigid-body-mode coarse correction with an exactly inverted
        # Galerkin matrix, Chebyshev again.  8 matrix products per cycle instead of 40, and 2.3x fewer outer iterations.
        self.asm = self.amg = None
        self.amg_smooth_its, self.amg_smooth_ratio = amg_smooth_its, amg_smooth_ratio
        if coarse in ("assembled", "amg") and len(prob.levels) > 1:
            from .assembly import AssembledLevel
            # several ranks: every rank assembles ITS OWN p = 1 matrix (its elements' sum; the operator is A = sum_r R_r^T A_r R_r, applied as
            # "local product, then the interface sum" like the matrix-free levels); with "amg" the first transfer of the aggregation
            # hierarchy is distributed over the ranks and everything under it is small and replicated (amg.py, round 5; rounds 3-4
            # all-gathered all element matrices and replicated the whole level)
            self.asm = AssembledLevel(prob, 0, **self._asm_kwargs)
            if coarse == "amg":
                from .amg import AggregationAMG
                self.amg = AggregationAMG(self.asm, verbose=verbose, max_coarse_dofs=amg_max_coarse_dofs,
                                          smooth_its=amg_smooth_its, smooth_ratio=amg_smooth_ratio, coarse_cycles=amg_coarse_cycles,
                                          dist_halo=self.halos[0] if self.halos else None)
        self._pc_graph, self._pc_graph_io, self._pc_graph_counts, self._pc_warm = None, None, (0, 0), False
        self.ksp_rtol, self.snes_rtol, self.snes_maxit, self.verbose = ksp_rtol, snes_rtol, snes_maxit, verbose
        self.nlev = len(prob.levels)
        # the library's exchange per level (halo.RcclHalo), or None: torch.distributed point-to-point + index ops
        self.rhalos = None
        if self.halos:
            if isinstance(rccl, (list, tuple)):
                self.rhalos = list(rccl)
            elif rccl == "auto":
                import torch.distributed as dist
                if dist.is_initialized() and dist.get_backend(self.halos[-1].group) == "nccl" and self.halos[-1].device.type == "cuda":
                    from .halo import RcclHalo
                    self.rhalos = [RcclHalo(self.ceed, h) for h in self.halos]
            if self.rhalos is not None and len(self.rhalos) != len(prob.levels):
                raise ValueError("one RcclHalo per multigrid level expected")
            if self.graph and self.rhalos is None:
                raise ValueError("graph=True on several ranks needs the library's exchange (torch.distributed calls cannot be recorded)")
            if self.rhalos is None:
                self._auto_graph = False
            if self.rhalos is not None and lead_elements > 0:      # split-phase Jacobians: exchange under the interior elements
                for lv, level in enumerate(prob.levels):
                    level.opJacob.set_overlap_split(int(lead_elements), self.halos[lv].interface_dof_mask())
        self._split = bool(self.rhalos) and lead_elements > 0
        self.w = [{k: self._vec(prob.lsize(lv), lv) for k in ("x", "b", "r", "d", "t", "dinv", "z")} for lv in range(self.nlev)]
        if self._pb:
            for lv in range(self.nlev):
                self.w[lv]["pb"] = self._vec(3 * prob.lsize(lv), lv)      # the inverted 3 x 3 blocks, [node][c out][c in]
        self.emax = [1.0] * self.nlev
        self._x0 = {}
        n = prob.lsize()
        top = self.nlev - 1
        self.U, self.R, self.dU, self.Xloc, self.bcv, self.Rtry, self.Utry = (self._vec(n, top) for _ in range(7))
        self.kp, self.kz, self.kAp = (self._vec(n, top) for _ in range(3))
        self.free = prob.levels[prob.fine].mask == 0
        self.weights = [None] * self.nlev
        if self.halos:
            for lv in range(self.nlev):
                wv = self._vec(prob.lsize(lv), lv)
                self._set(wv, self.halos[lv].owner_weight * (prob.levels[lv].mask == 0))
                self.weights[lv] = wv
                self._refresh_multiplicity(lv)
        # body force vector (opSetupForce output, setuplibceed.c:555-583): SNESSolve(snes, F, U) solves
        # residual(U) = load * F on the unconstrained dofs (elasticity.c:645-654)
        self.fv = None
        if forcing is not None:
            self.fv = self._vec(n, top)
            self._set(self.fv, np.asarray(forcing, dtype=np.float64) * self.free)
            self._halo_sum(top, self.fv)
        self.load = 1.0
        self.stats = SolveStats()
        self._bc_nodes = self._collect_bc_nodes()
        self._setup_surface_loads(traction, pressure, pressure_tangent)
        if self.amg is not None:
            # setup, not solve: aggregates, prolongation and the product patterns from the Jacobian of the undeformed state
            self.U.set_value(0.0)
            self.p.form_residual(self.U, self.R)
            self.asm.assemble()
            self.amg.build()

    # ---- surface loads (surface.py) -----------------------------------------------------------
    def _setup_surface_loads(self, traction, pressure, pressure_tangent):
        """With no surface load given nothing here runs beyond the argument checks, and no solve takes a new path."""
        if pressure_tangent not in ("full", "none"):
            raise ValueError(f"pressure_tangent must be 'full' or 'none', not {pressure_tangent!r}")
        self.pressure_tangent = pressure_tangent
        self.pressure_loads = []                     # (SurfaceLoad, p) per loaded side set
        self.surface_loads = []                      # every SurfaceLoad made here (destroy_surface_loads)
        if not traction and not pressure:
            return
        from .mesh import side_set_nodes
        from .surface import SurfaceLoad
        prob, lv = self.p, self.p.levels[self.p.fine]
        for sid in list(traction or {}) + list(pressure or {}):
            if sid not in prob.mesh.side_sets:
                raise ValueError(f"surface load on side set {sid}: the mesh has no such side set")
            nodes = side_set_nodes(prob.mesh, lv.dofmap, [sid])
            if sid in prob.bc_sides or (nodes.size and lv.mask.reshape(-1, 3)[nodes].all()):
                raise ValueError(f"surface load on side set {sid}, which is one of the problem's Dirichlet side sets")
        n, top = prob.lsize(), self.nlev - 1
        make = lambda sid: SurfaceLoad(self.ceed, prob.mesh, lv.dofmap, [sid], Q=prob.Q, mask=lv.mask)
        for sid, t in (traction or {}).items():
            t = np.asarray(t, dtype=np.float64).reshape(-1)
            if t.size != 3:
                raise ValueError(f"traction on side set {sid}: three components expected")
            if self.fv is None:
                self.fv = self._vec(n, top)
            sl = make(sid)
            sl.traction_add(t, 1.0, self.fv)         # masked rows are never written: fv stays zero on the constrained dofs
            self.surface_loads.append(sl)
        for sid, pval in (pressure or {}).items():
            sl = make(sid)
            self.pressure_loads.append((sl, float(pval)))
            self.surface_loads.append(sl)

    def destroy_surface_loads(self):
        for sl in self.surface_loads:
            sl.destroy()
        self.surface_loads, self.pressure_loads = [], []

    def A_outer(self, lv, x, y):
        """The Jacobian of the outer Krylov iteration: the level's operator plus load sum_s p_s T_s(u) x, u the state of the last
        residual evaluation (Xloc: free part + boundary values).  Masked entries of x read as zero and masked rows are not written,
        as in the volume operator."""
        self.A(lv, x, y)
        if self.pressure_tangent == "full":
            for sl, pval in self.pressure_loads:
                sl.tangent_add(pval, self.load, self.Xloc, x, y)

    # ---- vector helpers ---------------------------------------------------------------------
    def axpby(self, y, a, x, b):
        y.axpby(a, x, b)

    def copy(self, dst, src):
        dst.axpby(1.0, src, 0.0)

    def minv(self, lv, z, r):
        """z = M^-1 r with the smoother's preconditioner of level lv: the inverted diagonal, or the inverted nodal blocks."""
        if self._pb:
            cd.pointblock_mult(z, self.w[lv]["pb"], r)
        else:
            z.pointwise_mult(r, self.w[lv]["dinv"])

    def dot(self, x, y, fine_weight=False, lv=None) -> float:
        """x . y; on several ranks each dof counts once (owner weights of level `lv`, default the fine level)."""
        lv = self.nlev - 1 if lv is None else lv
        if self.rhalos:      # the sum over the ranks on the device (ncclAllReduce on the Ceed's stream), ONE read at the end
            sc = self.ceed.scalars
            x.dot_to(y, sc, 7, self.weights[lv])
            self.ceed.all_reduce(sc, 7, 1)
            return float(sc.to_numpy()[7])
        v = x.dot(y, self.weights[lv])
        if self.halos:
            import torch, torch.distributed as dist
            t = torch.tensor([v], dtype=torch.float64, device="cpu" if self.halos[lv].device.type == "cpu" or self.halos[lv].stage_host else self.halos[lv].device)
            dist.all_reduce(t, group=self.halos[lv].group)
            v = float(t.item())
        return v

    # ---- vectors that alias torch tensors (several ranks only) ----------------------------------------
    def _vec(self, n, lv):
        return self.ceed.tensor_vector(n, self.halos[lv].device) if self.halos else self.ceed.vector(n).set_value(0.0)

    def _set(self, vec, arr):
        """vec := arr (host array), keeping the torch alias intact."""
        vec.fill(arr)

    def _halo_sum(self, lv, vec):
        """Interface sum of an operator output at level lv (the DMLocalToGlobal(ADD_VALUES) of matops.c:57)."""
        if self.rhalos:               # the library's exchange, on the Ceed's stream: nothing to synchronise, nothing to re-wrap
            self.rhalos[lv].add(vec)
        elif self.halos:
            if vec.t.device.type == "cuda":
                self.ceed.synchronize()
            self.halos[lv].add(vec.t)
            vec.touched()

    def _refresh_multiplicity(self, lv):
        """multVec of misc.c:115-143 counted over ALL ranks: 1 / (halo-summed element multiplicity)."""
        level = self.p.levels[lv]
        m = self._vec(self.p.lsize(lv), lv)
        level.Erestrictu.multiplicity(m)
        self._halo_sum(lv, m)
        self._set(level.multinv, 1.0 / m.to_numpy())

    # ---- operators ---------------------------------------------------------------------------
    def A(self, lv, x, y):
        if lv == 0 and self.asm is not None:
            self.asm.apply(x, y)
            self.stats.coarse_spmv += 1
        elif self._split:             # ApplyLocalCeedOp + DMLocalToGlobal(ADD_VALUES) in one library call, exchange overlapped
            self.p.levels[lv].opJacob.apply_with_halo(x, y, self.rhalos[lv])
            self.stats.jacobian_applies += 1
            return
        else:
            self.p.apply_jacobian(lv, x, y)
            self.stats.jacobian_applies += 1
        self._halo_sum(lv, y)

    def _fused_op(self, lv):
        """The level's Jacobian operator if its consumers may be fused behind it: matrix-free level, no interface sum."""
        if not self.fuse_epilogue or self.halos or self.rhalos or (lv == 0 and self.asm is not None):
            return None
        return self.p.levels[lv].opJacob

    def level_residual(self, lv, b, x, z):
        """z = b - A x on level lv (t: the level's scratch)."""
        w, op = self.w[lv], self._fused_op(lv)
        if op is not None:
            op.apply_residual(x, w["t"], b, z)
            self.stats.jacobian_applies += 1
        else:
            self.A(lv, x, w["t"])
            z.waxpby(1.0, b, -1.0, w["t"])

    def _collect_bc_nodes(self):
        from .mesh import side_set_nodes
        lv = self.p.levels[self.p.fine]
        return {sid: side_set_nodes(self.p.mesh, lv.dofmap, [sid]) for sid in self.clamp}

    def bc_values(self, load: float) -> np.ndarray:
        """DMPlexInsertBoundaryValues at `time = loadIncrement` (matops.c:70-72)."""
        lv = self.p.levels[self.p.fine]
        v = np.zeros((lv.dofmap.nnodes, 3))
        if self.mms:
            nodes = np.nonzero(lv.mask.reshape(-1, 3)[:, 0])[0]
            v[nodes] = bc_mms(lv.dofmap.node_coords[nodes], load)
        for sid, par in self.clamp.items():
            nodes = self._bc_nodes[sid]
            v[nodes] = bc_clamp(lv.dofmap.node_coords[nodes], load, **par)
        return (v.reshape(-1) * (lv.mask != 0))

    def residual(self, U, R):
        """FormResidual_Ceed: Xloc = free part of U + boundary values; R = F(Xloc), constrained rows dropped."""
        self.copy(self.Xloc, U)
        self.axpby(self.Xloc, 1.0, self.bcv, 1.0)
        self.p.form_residual(self.Xloc, R)
        self._halo_sum(self.nlev - 1, R)
        if self.fv is not None:
            self.axpby(R, -self.load, self.fv, 1.0)
        for sl, pval in self.pressure_loads:           # follower pressure on the current surface (constrained rows are not written)
            sl.pressure_add(pval, self.load, self.Xloc, R)
        self.stats.residual_evals += 1

    # ---- multigrid preconditioner ---------------------------------------------------------------
    def setup_preconditioner(self):
        """Per Newton step: diagonals (GetDiag_Ceed), Chebyshev eigenvalue estimates."""
        if self.asm is not None:
            self.asm.assemble()
            self.stats.jacobian_applies += self.asm.nd
            if self.amg is not None:
                self.amg.setup()                # Galerkin matrix of THIS Jacobian and its inverse
        for lv in range(self.nlev):
            w = self.w[lv]
            if self._pb:
                # the 3 x 3 nodal blocks and their inverses; constrained components come out of the masked operator as zero rows and
                # columns and are dropped by the inversion, as the reciprocal leaves the zeros of the scalar diagonal alone
                self.p.get_pointblock_diag(lv, w["pb"])
                n_bad = cd.pointblock_invert(w["pb"])
                if n_bad:
                    raise RuntimeError(f"smoother='pbjacobi': {n_bad} nodal blocks of level {lv} have a non-positive or non-finite pivot")
            else:
                self._get_diag(lv, w["dinv"])
                self._halo_sum(lv, w["dinv"])
                # 1 / diagonal; constrained rows come out of the masked operator as zeros and stay zero (CeedVectorReciprocal
                # leaves zeros alone): residuals and corrections are zero there anyway.  No trip through the host.
                w["dinv"].reciprocal()
                w["dinv"].touched()
            mask = self.p.levels[lv].mask != 0
            # The start vector of the eigenvalue estimate is drawn once per level; no BLAS on the host (a threaded BLAS
            # call leaves its worker pool spinning, which starves a CPU-quota'd process for ~0.1 s a call).
            if lv not in self._x0:
                if self.halos:   # shared nodes must get the same value on every rank: a hash of the coordinates
                    X = self.p.levels[lv].dofmap.node_coords
                    k = np.array([[12.9898, 78.233, 37.719], [93.989, 67.345, 24.113], [45.164, 11.135, 83.951]])
                    v = np.sin(X @ k.T) * 437.5453
                    x = (2.0 * (v - np.floor(v)) - 1.0).reshape(-1) * (~mask)
                else:
                    x = np.random.default_rng(1234 + lv).uniform(-1, 1, mask.size) * (~mask)
                x0 = self._vec(mask.size, lv)
                self._set(x0, x / np.sqrt(np.square(x).sum()))     # (any positive scale: the iteration renormalises)
                self._x0[lv] = x0
            # largest eigenvalue of D^-1 A: 10 steps of Jacobi-preconditioned CG on the noisy right-hand side and
            # the largest eigenvalue of its Lanczos tridiagonal -- what KSPChebyshevEstEig does (elasticity.c:546-549).
            # (A plain power iteration from the same vector was 2x low after 12 steps on the config-3 mesh.)
            self.emax[lv] = lanczos_emax(*(self._lanczos_host(lv, 10) if (self.halos and not self.rhalos) else self._lanczos_device(lv, 10)))

    def _get_diag(self, lv, d):
        """The diagonal of level lv's operator (a subclass with more terms in its operator adds theirs)."""
        self.p.get_diag(lv, d)

    def _lanczos_host(self, lv, steps):
        """CG coefficients with every dot product read on the host (several ranks: the dots are all-reduced)."""
        w = self.w[lv]
        r, z, pv, Ap = w["r"], w["z"], w["d"], w["t"]
        self.copy(r, self._x0[lv])
        self.minv(lv, z, r); self.copy(pv, z)
        rz = self.dot(r, z, lv=lv)
        alphas, betas = [], []
        for _ in range(steps):
            self.A(lv, pv, Ap)
            pAp = self.dot(pv, Ap, lv=lv)
            if not (pAp > 0.0 and rz > 0.0):
                break
            alpha = rz / pAp
            self.axpby(r, -alpha, Ap, 1.0)
            self.minv(lv, z, r)
            rz_new = self.dot(r, z, lv=lv)
            alphas.append(alpha); betas.append(rz_new / rz)
            self.axpby(pv, 1.0, z, rz_new / rz)
            rz = rz_new
        return alphas, betas

    def _lanczos_device(self, lv, steps):
        """The same recurrence, scalars kept on the device; several ranks: every dof counts once, the library sums the dots."""
        w = self.w[lv]
        return lanczos_device(self.ceed, lambda x, y: self.A(lv, x, y), lambda z, r: self.minv(lv, z, r), self._x0[lv],
                              w["r"], w["z"], w["d"], w["t"], steps, weight=self.weights[lv], all_reduce=bool(self.rhalos))

    def chebyshev(self, lv, b, x, its, zero_guess, lmin_frac=0.1):
        """Chebyshev iteration on D^-1 A with bounds [0.1, 1.1] x emax (KSPChebyshevEstEigSet(0,0.1,0,1.1)).  As KSPCHEBYSHEV does, the
        residual is RECOMPUTED from the iterate in every step (r_k = b - A x_k), not carried by a recurrence (r -= A d): the operator is
        applied to x, and the step reads b, dinv, d, x and writes d, x -- no residual vector is read or written (round 5: 48 instead of
        56 B per dof in the step; the two are equal in exact arithmetic)."""
        w = self.w[lv]
        d, t = w["d"], w["t"]
        op = self._fused_op(lv)

        def one(c1, c2, have_x):
            """d = c1 dinv (b - A x) + c2 d;  x (+)= d   (have_x False: x = 0, no apply)"""
            if self._pb:              # the inverted nodal blocks for dinv: the apply, then the block step (the fused epilogue is a
                if have_x:            # lane-per-dof kernel and has no block form)
                    self.A(lv, x, t)
                cd.chebyshev_step_pointblock(x, d, None, b, t if have_x else None, w["pb"], c1, c2, not have_x)
            elif not have_x:
                x.chebyshev_step(d, None, b, None, w["dinv"], c1, c2, True)
            elif op is not None:      # the apply and the step in one: A x is consumed where it is formed
                op.apply_chebyshev(x, t, x, d, None, b, w["dinv"], c1, c2)
                self.stats.jacobian_applies += 1
            else:
                self.A(lv, x, t)
                x.chebyshev_step(d, None, b, t, w["dinv"], c1, c2, False)
        for k, (c1, c2) in enumerate(chebyshev_coefficients(self.emax[lv], lmin_frac, its)):
            one(c1, c2, k > 0 or not zero_guess)

    def coarse_solve(self, b, x):
        """Jacobi-preconditioned CG on the coarsest operator (stands in for GAMG on the FD-coloured matrix)."""
        w = self.w[0]
        r, d, t, z = w["r"], w["d"], w["t"], w["z"]
        x.set_value(0.0)
        self.copy(r, b)
        self.minv(0, z, r); self.copy(d, z)
        rz = self.dot(r, z, lv=0)
        rz0 = rz
        if rz0 <= 0.0:
            return
        for it in range(self.coarse_maxit):
            self.A(0, d, t)
            alpha = rz / self.dot(d, t, lv=0)
            self.axpby(x, alpha, d, 1.0); self.axpby(r, -alpha, t, 1.0)
            self.minv(0, z, r)
            rz_new = self.dot(r, z, lv=0)
            self.stats.coarse_its += 1
            if rz_new <= self.coarse_rtol ** 2 * rz0:
                break
            self.axpby(d, 1.0, z, rz_new / rz)
            rz = rz_new

    def amg_cycle(self, b, x):
        """One V-cycle of the aggregation hierarchy under the assembled level (amg.py): the coarse solve."""
        w, amg = self.w[0], self.amg
        lf = 1.0 / self.amg_smooth_ratio
        self.chebyshev(0, b, x, self.amg_smooth_its, True, lf)
        self.A(0, x, w["t"])
        w["z"].waxpby(1.0, b, -1.0, w["t"])                                # residual
        amg.restrict(w["z"])
        amg.solve_coarsest()
        amg.prolong(w["z"])
        self.axpby(x, 1.0, w["z"], 1.0)
        self.chebyshev(0, b, x, self.amg_smooth_its, False, lf)
        self.stats.coarse_its += 2 * self.amg_smooth_its

    def vcycle(self, lv, b, x):
        """PC_MG_MULTIPLICATIVE V-cycle, 3 smoothing steps down and up (elasticity.c:588-590)."""
        if lv == 0:
            if self.nlev == 1:
                self.chebyshev(0, b, x, self.smooth_its, True)
            elif self.amg is not None:
                self.amg_cycle(b, x)
            elif self.coarse in ("chebyshev", "assembled"):
                self.chebyshev(0, b, x, self.coarse_cheb_its, True, 1.0 / self.coarse_cheb_ratio)
                self.stats.coarse_its += self.coarse_cheb_its
            else:
                self.coarse_solve(b, x)
            return
        w, wc = self.w[lv], self.w[lv - 1]
        self.chebyshev(lv, b, x, self.smooth_its, True)
        self.level_residual(lv, b, x, w["z"])
        self.p.restrict(lv, w["z"], wc["b"])                                # Restrict_Ceed
        self._halo_sum(lv - 1, wc["b"])
        self.vcycle(lv - 1, wc["b"], wc["x"])
        if not self.halos and self.fuse_epilogue:   # one rank: the correction added in place by the prolongation's owners (same bits)
            self.p.prolong_add(lv, wc["x"], x)
        else:
            self.p.prolong(lv, wc["x"], w["z"])                             # Prolong_Ceed
            self._halo_sum(lv, w["z"])
            self.axpby(x, 1.0, w["z"], 1.0)
        self.chebyshev(lv, b, x, self.smooth_its, False)

    def _autotune_vcycle(self, r, z, reps=2):
        """Pick (fused consumers?, replayed graph?) by timing the V-cycle in every combination left open ("auto")."""
        top = self.nlev - 1
        keep = (self.stats.jacobian_applies, self.stats.coarse_its, self.stats.coarse_spmv)
        fuses = (True, False) if (self._auto_fuse and self._fused_op(top) is not None) else (self.fuse_epilogue,)
        graphs = (True, False) if self._auto_graph else (self.graph,)
        times = {}
        for f in fuses:
            self.fuse_epilogue = f
            self.vcycle(top, r, z)                 # first-use set-up of this form is neither recorded nor timed
            for g in graphs:
                run, gr = (lambda: self.vcycle(top, r, z)), None
                if g:
                    try:
                        gr = self.ceed.capture(run)
                    except cd.CeedError:           # a backend that cannot record (the CPU oracle): eager only
                        continue
                    run = gr.launch
                run(); self.ceed.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    run()
                self.ceed.synchronize()
                times[(f, g)] = (time.perf_counter() - t0) / reps
                if gr is not None:
                    gr.destroy()
        (self.fuse_epilogue, self.graph), _ = min(times.items(), key=lambda kv: kv[1])
        self._auto_fuse = self._auto_graph = False
        self._pc_warm = True
        self.stats.jacobian_applies, self.stats.coarse_its, self.stats.coarse_spmv = keep
        self.tuning = {"fused_epilogue": self.fuse_epilogue, "vcycle_graph": self.graph,
                       "vcycle_ms": {f"{'fused' if f else 'two_pass'}+{'graph' if g else 'eager'}": 1e3 * t for (f, g), t in times.items()}}
        if self.verbose:
            print("V-cycle forms (ms):", self.tuning["vcycle_ms"], "->", "fused" if self.fuse_epilogue else "two passes", "+", "graph" if self.graph else "eager")

    def record_preconditioner(self, r, z):
        """Capture vcycle(r -> z) for the current diagonals / eigenvalue bounds (call after setup_preconditioner)."""
        if self._pc_graph is not None:
            self._pc_graph.destroy()
            self._pc_graph = None
        if (self._auto_fuse or self._auto_graph) and self.nlev > 1:
            self._autotune_vcycle(r, z)
        if not self.graph or self.nlev == 1:
            return
        top = self.nlev - 1
        if not self._pc_warm:                      # first-use setup (CSR maps, scratch) must not be recorded
            self.vcycle(top, r, z)
            self._pc_warm = True
        j0, c0 = self.stats.jacobian_applies, self.stats.coarse_its
        self._pc_graph = self.ceed.capture(lambda: self.vcycle(top, r, z))
        self._pc_graph_counts = (self.stats.jacobian_applies - j0, self.stats.coarse_its - c0)
        self.stats.jacobian_applies, self.stats.coarse_its = j0, c0
        self._pc_graph_io = (r, z)

    def precondition(self, r, z):
        if self._pc_graph is not None and self._pc_graph_io[0] is r and self._pc_graph_io[1] is z and self._pc_graph.stale():
            # a vector the recording depends on was overwritten behind it (CeedXGraphIsStale; the check is LOCAL to this rank): the
            # recording is dropped and this rank runs the V-cycle eagerly -- the same launches and, on several ranks, the same RCCL
            # exchanges in the same order as its peers' replays, so nobody waits for a message that never comes
            self._pc_graph.destroy()
            self._pc_graph = None
        if self._pc_graph is not None and self._pc_graph_io[0] is r and self._pc_graph_io[1] is z:
            self._pc_graph.launch()
            self.stats.jacobian_applies += self._pc_graph_counts[0]
            self.stats.coarse_its += self._pc_graph_counts[1]
            return
        if self.nlev == 1:          # -multigrid none: Jacobi (elasticity.c:516-519)
            self.minv(0, z, r)
        else:
            self.vcycle(self.nlev - 1, r, z)

    # ---- Krylov ---------------------------------------------------------------------------------
    def fcg(self, b, x, rtol):
        """Flexible preconditioned CG, natural-norm convergence test (KSP_NORM_NATURAL: sqrt(r'z))."""
        fine = self.nlev - 1
        r, z, p, Ap = self.w[fine]["b"], self.kz, self.kp, self.kAp
        x.set_value(0.0)
        self.copy(r, b)
        self.precondition(r, z)
        self.copy(p, z)
        rz = self.dot(r, z, True)
        rz0 = rz
        its = 0
        if rz0 <= 0.0:
            return 0
        apply_A = self.A_outer if self.pressure_loads else self.A
        for its in range(1, 500):
            apply_A(fine, p, Ap)
            alpha = rz / self.dot(p, Ap, True)
            self.axpby(x, alpha, p, 1.0); self.axpby(r, -alpha, Ap, 1.0)
            r_zold = self.dot(r, z, True)                    # r_new . z_old, taken BEFORE the preconditioner overwrites z (no copy of z)
            self.precondition(r, z)
            rz_new = self.dot(r, z, True)
            if self.verbose:
                print(f"      ksp {its:3d}  natural norm {np.sqrt(abs(rz_new)):.3e}")
            if rz_new <= rtol ** 2 * rz0:
                break
            beta = (rz_new - r_zold) / rz                    # Polak-Ribiere: flexible
            self.axpby(p, 1.0, z, beta)
            rz = rz_new
        return its

    # ---- Newton with load increments ---------------------------------------------------------------
    def solve(self, num_increments: int = 10, stop_after: Optional[int] = None) -> SolveStats:
        """``stop_after``: run only the first so many of the ``num_increments`` load increments (load studies)."""
        st = self.stats
        t0 = time.perf_counter()
        self.U.set_value(0.0)
        for inc in range(1, (stop_after or num_increments) + 1):
            load = inc / num_increments
            self.load = load
            self._set(self.bcv, self.bc_values(load))
            self.residual(self.U, self.R)
            rnorm0 = np.sqrt(self.dot(self.R, self.R, True))
            rnorm = rnorm0
            st.initial_residuals.append(rnorm0)
            if self.verbose:
                print(f"increment {inc}/{num_increments}: |R| = {rnorm0:.6e}")
            for it in range(self.snes_maxit):
                if rnorm <= self.snes_rtol * rnorm0 or rnorm < 1e-50:
                    break
                self.setup_preconditioner()
                self.record_preconditioner(self.w[self.nlev - 1]["b"], self.kz)
                self.axpby(self.Rtry, -1.0, self.R, 0.0)                 # rhs = -R
                k = self.fcg(self.Rtry, self.dU, self.ksp_rtol)
                st.ksp_its += k
                # critical-point line search (SNESLINESEARCHCP): secant on phi(l) = dU . R(U + l dU)
                lam, lam_old = 1.0, 0.0
                phi_old = self.dot(self.dU, self.R, True)
                for _ in range(0 if self.line_search == "full" else (1 if self.line_search == "cp-petsc" else 3)):
                    self.copy(self.Utry, self.U); self.axpby(self.Utry, lam, self.dU, 1.0)
                    self.residual(self.Utry, self.Rtry)
                    phi = self.dot(self.dU, self.Rtry, True)
                    if abs(phi) <= 1e-8 * abs(phi_old) or abs(phi - phi_old) < 1e-300:
                        break
                    if self.line_search == "cp-petsc":
                        # ONE secant step in the form of PETSc's SNESLineSearchApply_CP (max_its 1, linear order) AS RECALLED -- PETSc's
                        # source is not in this image, so this is unverified against it: with fty = Y . F(X - lambda Y)
                        # (Y = -dU, so fty = -phi) the slope s = d fty / d lambda is made negative ("always go downhill"), the update is
                        # lambda - fty / s, a result below steptol (1e-12) switches direction (lambda + fty / s), one above maxstep (1e8)
                        # or a NaN leaves lambda as it was; the step is never rejected.  (Round 4 clamped the plain secant result to
                        # [1e-12, 1e8] instead: a negative secant step then took lambda = 1e-12, i.e. no step.)
                        fty, fty_old = -phi, -phi_old
                        sl = (fty - fty_old) / (lam - lam_old)
                        if sl > 0.0:
                            sl = -sl
                        if sl != 0.0:
                            lam_up = lam - fty / sl
                            if lam_up < 1e-12:
                                lam_up = lam + fty / sl
                            if np.isfinite(lam_up) and lam_up <= 1e8:
                                lam = lam_up
                        break
                    lam_new = lam - phi * (lam - lam_old) / (phi - phi_old)
                    if not np.isfinite(lam_new) or abs(lam_new - lam) < 1e-8 or lam_new <= 0.0 or lam_new > 10.0:
                        break
                    lam_old, phi_old, lam = lam, phi, lam_new
                self.axpby(self.U, lam, self.dU, 1.0)
                self.residual(self.U, self.R)                              # also refreshes the stored state
                rnorm = np.sqrt(self.dot(self.R, self.R, True))
                st.newton_its += 1
                st.history.append((inc, it + 1, k, lam, rnorm))
                if self.verbose:
                    print(f"   newton {it + 1:2d}: ksp its {k:3d}  lambda {lam:.4f}  |R| = {rnorm:.6e}")
            # decided on the residual itself: a step that meets the tolerance in the LAST allowed iteration has converged
            if not (rnorm <= self.snes_rtol * rnorm0 or rnorm < 1e-50):
                st.converged = False
            st.increments = inc
            if not np.isfinite(rnorm) or not st.converged:
                st.converged = False
                break
        self.ceed.synchronize()
        st.seconds = time.perf_counter() - t0
        if self._pc_graph is not None:
            self._pc_graph.destroy()
            self._pc_graph = None
        return st
