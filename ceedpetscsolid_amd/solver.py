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

The body, its loads and the ownership of every vector are body.LoadedBody's; the class here adds the preconditioner, the Krylov method
and ONE Newton iteration (``_newton``, ``_line_search``: dynamics.NewmarkPMG runs it too); the coarse level's CG is krylov.pcg.

Iteration counts are therefore this build's own, not PETSc's; the throughput figure reported is the
reference's "DoFs/Sec in SNES" = 1e-6 * Ugsz * (total KSP iterations) / (solve time)
(elasticity.c:755-764).
"""
from __future__ import annotations

import time
from typing import Dict, Optional

import numpy as np

from . import ceed as cd
from .body import LoadedBody, SolveStats, bc_clamp, bc_mms  # noqa: F401 -- (the boundary functions stay importable from here)
from .krylov import chebyshev_coefficients, lanczos_device, lanczos_emax, pcg
from .solid import SolidProblem


class NewtonPMG(LoadedBody):
    _asm_kwargs: dict = {}          # keywords of the assembled coarse level (dynamics.NewmarkPMG: its mass term); none here
    _DASHPOTS = False               # whether support= may carry dashpots (dynamics.NewmarkPMG: yes; a static solve would ignore them)

    def __init__(self, prob: SolidProblem, clamp: Optional[Dict[int, dict]] = None, mms: bool = False, forcing=None,
                 halo=None, rccl="auto", lead_elements: int = 0, smooth_its: int = 3, coarse_rtol: float = 1e-3, coarse_maxit: int = 200,
                 coarse: str = "cg", coarse_cheb_its: int = 40, coarse_cheb_ratio: float = 100.0, graph: bool = False,
                 amg_smooth_its: int = 3, amg_smooth_ratio: float = 10.0, amg_max_coarse_dofs: int = 1500, amg_coarse_cycles: int = 1,
                 ksp_rtol: float = 1e-10, snes_rtol: float = 1e-8, snes_maxit: int = 50, verbose: bool = False,
                 line_search: str = "cp", fuse_epilogue: bool = True, smoother: str = "jacobi",
                 traction: Optional[Dict[int, tuple]] = None, pressure: Optional[Dict[int, float]] = None, pressure_tangent: str = "full",
                 contact: Optional[Dict[int, dict]] = None, contact_tangent: str = "levels", support: Optional[Dict[int, dict]] = None,
                 traction_field: Optional[Dict[int, object]] = None, pressure_field: Optional[Dict[int, object]] = None,
                 hydrostatic: Optional[Dict[int, dict]] = None, density=None, gravity=None, acceleration_field=None,
                 spin: Optional[dict] = None, thermal: Optional[dict] = None):
        """The body and its loads (``clamp, mms, forcing, halo, rccl, traction, pressure, pressure_tangent, contact, traction_field,
        pressure_field, hydrostatic, density, gravity, acceleration_field, spin, thermal``): body.LoadedBody.  Of a spin's softening
        tangent and of the finite-strain thermal tangent, as of a follower pressure's, the V-cycle sees nothing.
        Of a follower pressure's tangent the V-cycle, its smoothers, diagonals and eigenvalue estimates see nothing: the preconditioner
        is the volume operator's.
        ``contact_tangent``: "levels" (default) adds the contact tangent C to the operator ``A`` and to the diagonal of EVERY
        matrix-free level -- one contact.ContactSurface per level with that level's dofmap and mask and the fine Q, all reading the
        state the fine residual stored, so a coarse level's term is the Galerkin product of the fine one -- and switches the fused
        consumers off on those levels (the term is added between the apply and its consumer).  "outer" adds it in ``A_outer`` only,
        the follower pressure's form: the preconditioner then knows nothing of the contact.  With coarse="assembled" or "amg" the
        assembled level-0 matrix does NOT carry the contact term (the matrix-free levels above it do).  smoother="pbjacobi" with
        contact is refused: the nodal blocks would lack the term.
        ``support`` (body.LoadedBody, support.py): the spring tangent K_s is in ``A`` and in the diagonal of every matrix-free level
        (one support.SupportSurface per level on the one state, so a coarse level's term is the Galerkin product) and the fused
        consumers are off on those levels, as for contact.  With coarse="assembled" or "amg" the assembled level-0 matrix does NOT
        carry the term (the matrix-free levels above it do), so a problem with NO Dirichlet dof, whose assembled matrix would be
        singular, is refused with those two.  Refused too: smoother="pbjacobi" with support= (the nodal blocks would lack the term) and
        a dashpot coefficient (cn, ct) in a static solve, which would be ignored."""
        # smoother: what the Chebyshev iteration of every p-multigrid level, its eigenvalue estimate and the Jacobi-preconditioned
        # coarse CG are preconditioned with -- "jacobi" (default, the reference: PCJACOBI on GetDiag_Ceed) or "pbjacobi": the inverted
        # 3 x 3 nodal blocks (PCPBJACOBI on CeedOperatorLinearAssemblePointBlockDiagonal), which keep the coupling between the
        # displacement components of a node that the scalar diagonal drops.  One rank only: the blocks of the interface nodes of
        # an element partition would have to be summed over the ranks before they are inverted, and no exchange here carries nine
        # values per node.
        if smoother not in ("jacobi", "pbjacobi"):
            raise ValueError(f"smoother must be 'jacobi' or 'pbjacobi', not {smoother!r}")
        if smoother == "pbjacobi":
            self._refuse_several_ranks(halo, "smoother='pbjacobi' is", "the nodal blocks of the interface nodes are not summed over the ranks")
        if smoother == "pbjacobi" and contact:
            raise ValueError("smoother='pbjacobi' with contact= is not provided: the nodal blocks would lack the contact term")
        if smoother == "pbjacobi" and support:
            raise ValueError("smoother='pbjacobi' with support= is not provided: the nodal blocks would lack the support term")
        if support and not self._DASHPOTS and any(isinstance(sp, dict) and (sp.get("cn") or sp.get("ct")) for sp in support.values()):
            raise ValueError("support=: a dashpot coefficient (cn, ct) in a static solve would be ignored; dashpots are the time steppers' (dynamics.py)")
        if support and coarse in ("assembled", "amg") and not np.any(prob.levels[prob.fine].mask):
            raise ValueError(f"support= with coarse={coarse!r} on a problem with no Dirichlet dof: the assembled level-0 matrix does not carry "
                             "the support term and would be singular; use coarse='cg' or 'chebyshev'")
        if line_search not in ("cp", "cp-petsc", "full"):           # (_line_search)
            raise ValueError(f"line_search {line_search!r}")
        recordable = coarse in ("chebyshev", "assembled", "amg")
        if graph != "auto" and graph and not recordable:
            raise ValueError("graph=True needs coarse='chebyshev', 'assembled' or 'amg' (the CG coarse solve reads dot products on the host)")
        super().__init__(prob, clamp=clamp, mms=mms, forcing=forcing, halo=halo, rccl=rccl, traction=traction, pressure=pressure,
                         pressure_tangent=pressure_tangent, verbose=verbose, contact=contact, contact_tangent=contact_tangent,
                         support=support, traction_field=traction_field, pressure_field=pressure_field, hydrostatic=hydrostatic,
                         density=density, gravity=gravity, acceleration_field=acceleration_field, spin=spin, thermal=thermal)
        self.smoother, self._pb, self.line_search = smoother, smoother == "pbjacobi", line_search
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
        # needs the reduction-free Chebyshev coarse solver (the CG coarse solve cannot be recorded: eager)
        self._auto_graph = graph == "auto" and recordable
        self.graph = graph != "auto" and bool(graph)
        if self.halos and self.rhalos is None:
            if self.graph:
                raise ValueError("graph=True on several ranks needs the library's exchange (torch.distributed calls cannot be recorded)")
            self._auto_graph = False
        if self.rhalos is not None and lead_elements > 0:      # split-phase Jacobians: exchange under the interior elements
            for lv, level in enumerate(prob.levels):
                level.opJacob.set_overlap_split(int(lead_elements), self.halos[lv].interface_dof_mask())
        self._split = bool(self.rhalos) and lead_elements > 0
        # coarse="assembled": the same Chebyshev polynomial, but on the ASSEMBLED p=1 matrix (assembly.py): a
        # coarse iteration is one SpMV on 81 entries per row instead of a matrix-free apply on the fine quadrature
        # coarse="amg": ONE cycle of a two-level smoothed-aggregation hierarchy on the assembled matrix (amg.py) -- what
        # the reference asks of PCGAMG under KSPPREONLY (elasticity.c:568-585): Chebyshev(amg_smooth_its) on
        # [emax / amg_smooth_ratio, 1.1 emax], the rigid-body-mode coarse correction with an exactly inverted
        # Galerkin matrix, Chebyshev again.  8 matrix products per cycle instead of 40, and 2.3x fewer outer iterations.
        self.asm = self.amg = None
        self.amg_smooth_its, self.amg_smooth_ratio = amg_smooth_its, amg_smooth_ratio
        if coarse in ("assembled", "amg") and self.nlev > 1:
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
        # contact_tangent="levels": the levels whose operator carries the contact tangent, and their surfaces (body.destroy_contacts
        # releases them with the fine one)
        self._contact_levels = set()
        if self.contacts and contact_tangent == "levels":
            from .contact import ContactSurface
            self._contact_levels = {lv for lv in range(self.nlev) if not (lv == 0 and self.asm is not None)}
            for c in self.contacts:
                for lv in self._contact_levels - set(c["levels"]):
                    level = prob.levels[lv]
                    c["levels"][lv] = ContactSurface(self.ceed, prob.mesh, level.dofmap, [c["sid"]], prob.Q, mask=level.mask)
        self.ksp_rtol, self.snes_rtol, self.snes_maxit = ksp_rtol, snes_rtol, snes_maxit
        self.w = [{k: self._vec(prob.lsize(lv), lv) for k in ("x", "b", "r", "d", "t", "dinv", "z")} for lv in range(self.nlev)]
        if self._pb:
            for lv in range(self.nlev):
                self.w[lv]["pb"] = self._vec(3 * prob.lsize(lv), lv)      # the inverted 3 x 3 blocks, [node][c out][c in]
        self.emax = [1.0] * self.nlev
        n, top = prob.lsize(), self.nlev - 1
        self.U, self.dU, self.Rtry, self.Utry, self.kp, self.kz, self.kAp = (self._vec(n, top) for _ in range(7))
        if self.amg is not None:
            # setup, not solve: aggregates, prolongation and the product patterns from the Jacobian of the undeformed state
            self.U.set_value(0.0)
            self.p.form_residual(self.U, self.R)
            self.asm.assemble()
            self.amg.build()

    def destroy(self):
        """The recorded V-cycle, the aggregation hierarchy and the assembled level, then what the body made (idempotent)."""
        self._drop_pc_graph()
        for o in (self.amg, self.asm):
            if o is not None:
                o.destroy()
        super().destroy()

    # ---- vector helpers ---------------------------------------------------------------------
    def minv(self, lv, z, r):
        """z = M^-1 r with the smoother's preconditioner of level lv: the inverted diagonal, or the inverted nodal blocks."""
        if self._pb:
            cd.pointblock_mult(z, self.w[lv]["pb"], r)
        else:
            z.pointwise_mult(r, self.w[lv]["dinv"])

    # ---- operators ---------------------------------------------------------------------------
    def A(self, lv, x, y):
        if lv == 0 and self.asm is not None:
            self.asm.apply(x, y)
            self.stats.coarse_spmv += 1
            self._halo_sum(lv, y)
        elif self._split:             # ApplyLocalCeedOp + DMLocalToGlobal(ADD_VALUES) in one library call, exchange overlapped
            self.p.levels[lv].opJacob.apply_with_halo(x, y, self.rhalos[lv])
            self.stats.jacobian_applies += 1
        else:
            super().A(lv, x, y)
        if lv in self._contact_levels:
            self.contact_tangent_add(lv, x, y)

    def _fused_op(self, lv):
        """The level's Jacobian operator if its consumers may be fused behind it: matrix-free level, no interface sum, no contact term
        (which is added between the apply and its consumer)."""
        if not self.fuse_epilogue or self.halos or self.rhalos or (lv == 0 and self.asm is not None) or lv in self._contact_levels:
            return None
        if self.supports:            # (the support term is added between the apply and its consumer too)
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
            self._start_vector(lv)
            # largest eigenvalue of D^-1 A: 10 steps of Jacobi-preconditioned CG on the noisy right-hand side and
            # the largest eigenvalue of its Lanczos tridiagonal -- what KSPChebyshevEstEig does (elasticity.c:546-549).
            # (A plain power iteration from the same vector was 2x low after 12 steps on the config-3 mesh.)
            self.emax[lv] = lanczos_emax(*(self._lanczos_host(lv, 10) if (self.halos and not self.rhalos) else self._lanczos_device(lv, 10)))

    def _get_diag(self, lv, d):
        """The diagonal of level lv's operator (a subclass with more terms in its operator adds theirs)."""
        self.p.get_diag(lv, d)
        if lv in self._contact_levels:
            for c in self.contacts:
                c["levels"][lv].diagonal_add(1.0, c["state"], d)
        if self.supports and not (lv == 0 and self.asm is not None):
            self.support_diagonal_add(lv, d)

    def _lanczos_host(self, lv, steps):
        """CG coefficients with every dot product read on the host (several ranks: the dots are all-reduced)."""
        w = self.w[lv]
        return pcg(lambda x, y: self.A(lv, x, y), lambda z, r: self.minv(lv, z, r), lambda x, y: self.dot(x, y, lv=lv), self._x0[lv],
                   None, w["r"], w["z"], w["d"], w["t"], 0.0, steps)[1:]

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
        its, _, _ = pcg(lambda x, y: self.A(0, x, y), lambda z, r: self.minv(0, z, r), lambda x, y: self.dot(x, y, lv=0), b, x,
                        w["r"], w["z"], w["d"], w["t"], self.coarse_rtol, self.coarse_maxit)
        self.stats.coarse_its += its

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

    def _drop_pc_graph(self):
        """Destroy and forget the recorded V-cycle, if there is one."""
        if self._pc_graph is not None:
            self._pc_graph.destroy()
            self._pc_graph = None

    def record_preconditioner(self, r, z):
        """Capture vcycle(r -> z) for the current diagonals / eigenvalue bounds (call after setup_preconditioner)."""
        self._drop_pc_graph()
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
            self._drop_pc_graph()
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
        """Flexible preconditioned CG, natural-norm convergence test (KSP_NORM_NATURAL: sqrt(r'z)).  Not krylov.pcg: the Polak-Ribiere
        beta takes a third dot per step (r_new . z_old), and r, z are the fixed pair a recorded V-cycle reads and writes."""
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
        apply_A = self.A_outer if (self.has_followers() or (self.contacts and self.contact_tangent == "outer")) else self.A
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
    def _line_search(self) -> float:
        """The step length along dU from U.  "cp": the critical-point search (SNESLINESEARCHCP), a secant iteration on
        phi(l) = dU . R(U + l dU): up to three secant steps, a step outside (0, 10] ends the search (this build's default);
        "cp-petsc": SNESLINESEARCHCP with PETSc's defaults (elasticity.c:596-601 sets the type and nothing else), see below;
        "full": l = 1 (SNESLINESEARCHBASIC)."""
        lam, lam_old = 1.0, 0.0
        if self.line_search == "full":
            return lam
        phi_old = self.dot(self.dU, self.R, True)
        for _ in range(1 if self.line_search == "cp-petsc" else 3):
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
        return lam

    def _newton(self, label, head: str):
        """Newton's iteration on U from the residual already in R, until |R| <= snes_rtol |R|_0 or snes_maxit steps; ``label``: the
        first entry of this call's history tuples (label, iteration, Krylov iterations, step length, |R|); ``head``: what the verbose
        line of |R|_0 begins with.  Returns (|R|_0, |R|); the caller decides what they mean."""
        st = self.stats
        rnorm0 = rnorm = np.sqrt(self.dot(self.R, self.R, True))
        st.initial_residuals.append(rnorm0)
        if self.verbose:
            print(f"{head}: |R| = {rnorm0:.6e}")
        for it in range(self.snes_maxit):
            if rnorm <= self.snes_rtol * rnorm0 or rnorm < 1e-50:
                break
            self.setup_preconditioner()
            self.record_preconditioner(self.w[self.nlev - 1]["b"], self.kz)
            self.axpby(self.Rtry, -1.0, self.R, 0.0)                 # rhs = -R
            k = self.fcg(self.Rtry, self.dU, self.ksp_rtol)
            st.ksp_its += k
            lam = self._line_search()
            self.axpby(self.U, lam, self.dU, 1.0)
            self.residual(self.U, self.R)                              # also refreshes the stored state and Xloc
            rnorm = np.sqrt(self.dot(self.R, self.R, True))
            st.newton_its += 1
            st.history.append((label, it + 1, k, lam, rnorm))
            if self.verbose:
                print(f"   newton {it + 1:2d}: ksp its {k:3d}  lambda {lam:.4f}  |R| = {rnorm:.6e}")
        return rnorm0, rnorm

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
            rnorm0, rnorm = self._newton(inc, f"increment {inc}/{num_increments}")
            # decided on the residual itself: a step that meets the tolerance in the LAST allowed iteration has converged
            if not (rnorm <= self.snes_rtol * rnorm0 or rnorm < 1e-50):
                st.converged = False
            st.increments = inc
            if not np.isfinite(rnorm) or not st.converged:
                st.converged = False
                break
        self.ceed.synchronize()
        st.seconds = time.perf_counter() - t0
        self._drop_pc_graph()
        return st
