"""Elastodynamics: implicit Newmark time stepping (``NewmarkPMG``: the Newton iteration of its parent solver.NewtonPMG on a residual with
the inertia term), and explicit central-difference stepping with a lumped mass (``ExplicitDynamics``, a body.LoadedBody, at the end).

The semi-discrete equations, with the sign and load conventions of ``solver.NewtonPMG`` (R = F_int - load (f + tractions) + load
sum_s p_s g_s^pressure, a pressure p > 0 pushing on the body),

    rho M a_{n+1} + F_int(u_{n+1}) = load(t_{n+1}) (f + tractions) - load(t_{n+1}) sum_s p_s g_s^pressure(u_{n+1})

are closed by Newmark's update (beta = 1/4, gamma = 1/2: the average-acceleration rule, unconditionally stable and energy-conserving
for a linear material):

    a_{n+1} = a0 (u_{n+1} - u_n) - a2 v_n - a3 a_n,     a0 = 1 / (beta dt^2),  a2 = 1 / (beta dt),  a3 = 1 / (2 beta) - 1
    v_{n+1} = v_n + dt ((1 - gamma) a_n + gamma a_{n+1})

u, v, a are L-vectors WITH the boundary values (clamp values follow load(t) as they follow the load fraction of a quasi-static solve;
the formulas above then give the clamped nodes the velocity and acceleration of that motion).  Every step is a Newton solve for
u_{n+1} with the residual above and the effective tangent K + a0 rho M on every multigrid level: ``A`` is the parent's apply followed by
the level's mass operator (mass.py) in add mode; the smoother's diagonal is diag K + a0 rho diag M; an assembled coarse level
(``coarse="assembled"`` / ``"amg"``) carries a0 rho M in its element matrices, so the p = 1 matrix and the aggregation hierarchy under
it are those of the effective operator.  By default (``fused_mass=False``) the consumers fused into the Jacobian apply's epilogue
are not used (they have no mass term: ``_fused_op`` is None) and every form is two passes.  dt is fixed per solver object: a recorded
V-cycle keeps the coefficient a0 rho it was recorded with.

``fused_mass=True`` / ``"auto"``: the level's Jacobian operator carries the term itself (``ceed.Operator.set_mass_term(a0 rho)``,
CeedXOperatorSetMassTerm: K + a0 rho M in the launches of K), ``A`` is ONE apply of it on every matrix-free level, and ``_fused_op``
hands it to the smoother step and the V-cycle's residual again, so ``fuse_epilogue=`` and ``graph=`` act as in the parent.  ``True``
raises a ValueError where the library or a level has no such kernel; ``"auto"`` keeps two passes on that level.  The term is never
set on a level whose matrix is assembled (its matrix already holds a0 rho M); the diagonal, the residual's inertia term, the start-up
mass solve and the kinetic energy keep the mass operator of mass.py; ``destroy()`` clears every term it set.
The term is state of the PROBLEM's operator (``prob.levels[lv].opJacob``), not of this object: while a solver with fused_mass lives,
``prob.apply_jacobian(lv)`` -- and any other user of that operator, a second solver on the same problem among them -- gets
K + a0 rho M on the levels of ``_mass_in_op``; a second NewmarkPMG with fused_mass on the same problem overwrites the coefficient
(another dt), and destroying either clears the term under the other.  One solver with fused_mass per problem at a time.

Supports (``support=``, body.LoadedBody, support.py): springs K_s and dashpots C_d on side sets.  With Newmark's velocity
v_{n+1} = v_n + dt (1 - gamma) a_n + gamma dt (a0 x_{n+1} + pred) the residual adds K_s x_{n+1} + C_d v_{n+1} and the tangent and the
diagonal of every matrix-free level K_s + a1 C_d, a1 = gamma / (beta dt): ONE combined state per support (a linear combination of the
two states, formed once: dt is fixed), so one launch per level.  ``set_initial`` puts -K_s u_0 - C_d v_0 into a_0.  The explicit stepper
adds K_s x_n + C_d vh_{n-1/2} to its force -- the half-step velocity lagged, the standard central-difference form -- and its
``stable_dt`` knows both terms.  ``absorbing_support`` gives the dashpots of a Lysmer-Kuhlemeyer boundary.

Refused: ``smoother="pbjacobi"`` (the nodal blocks of M are not built) and a halo with several ranks (the mass operator's interface sums
were never run there).
"""
from __future__ import annotations

import time
from typing import Callable, Optional, Union

import numpy as np

from .body import LoadedBody
from .krylov import lanczos_device, lanczos_emax, pcg
from .mass import MassOperator, split_density
from .solid import SolidProblem
from .solver import NewtonPMG, SolveStats


def _refuse_contact(kw):
    """Contact (body.LoadedBody, contact=) covers static solves only: the mass term of the coarse levels and stable_dt know nothing of
    the penalty."""
    if kw.get("contact"):
        raise ValueError("contact= is not provided for dynamics (static solves only: stable_dt knows nothing of the penalty)")


def absorbing_support(prob: SolidProblem, density: float) -> dict:
    """The dashpots of a Lysmer-Kuhlemeyer absorbing boundary for ``support=``: dict(cn=rho c_p, ct=rho c_s) with
    c_p = sqrt((lambda + 2 mu) / rho) and c_s = sqrt(mu / rho) from the problem's (E, nu).  Exact for plane waves at normal incidence."""
    if not density > 0.0:
        raise ValueError("density must be positive")
    nu, E = (float(v) for v in prob.phys[:2])
    mu, lam = E / (2.0 * (1.0 + nu)), E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
    return dict(cn=float(np.sqrt((lam + 2.0 * mu) * density)), ct=float(np.sqrt(mu * density)))


class NewmarkPMG(NewtonPMG):
    _DASHPOTS = True

    def __init__(self, prob: SolidProblem, density, dt: float, beta: float = 0.25, gamma: float = 0.5, fused_mass=False, **kw):
        """``density``: a positive float, or a mass.DensityField: every mass operator here is then M_rho of that field (each level's own,
        the assembled level's too) and ``self.density`` is the factor 1 in front of it.  The fused mass term holds one scalar, so
        ``fused_mass=True`` with a field is refused and "auto" keeps the two-pass form."""
        rho, field = split_density(density, "density, dt and beta must be positive")
        self.density_field = field
        if not (dt > 0.0 and beta > 0.0):
            raise ValueError("density, dt and beta must be positive")
        if field is not None and fused_mass is True:
            raise ValueError("NewmarkPMG(fused_mass=True) with a DensityField is not provided: the fused mass term K + c M holds one scalar; "
                             "fused_mass='auto' or False takes the two-pass form")
        _refuse_contact(kw)
        if not (fused_mass is True or fused_mass is False or fused_mass == "auto"):
            raise ValueError(f"fused_mass must be False, True or 'auto', not {fused_mass!r}")
        if kw.get("smoother", "jacobi") == "pbjacobi":
            raise ValueError("NewmarkPMG: smoother='pbjacobi' is not provided: the 3 x 3 nodal blocks of the mass operator are not built")
        self._refuse_several_ranks(kw.get("halo"), "NewmarkPMG is", "the mass operator's sums at the interface nodes have not been run "
                                   "over several ranks")
        if kw.get("line_search", "cp") == "cp-petsc":
            raise ValueError("NewmarkPMG: line_search must be 'cp' or 'full'")
        self.density, self.dt, self.beta, self.gamma = rho, float(dt), float(beta), float(gamma)
        self.a0, self.a2, self.a3 = 1.0 / (beta * dt * dt), 1.0 / (beta * dt), 1.0 / (2.0 * beta) - 1.0
        self.a1 = gamma / (beta * dt)    # d v_{n+1} / d x_{n+1}: the factor of the dashpots in the tangent
        self._asm_kwargs = {"mass_coef": self.a0 * self.density}
        if field is not None:
            self._asm_kwargs["mass_density"] = field
        # the tangent's mass term per level (read by A and _get_diag, which the parent's constructor may already call)
        self.mass = [MassOperator(prob, lv, self.a0 * self.density, density=field) for lv in range(len(prob.levels))]
        self._mdiag = {}
        self.fused_mass = fused_mass = False if field is not None else fused_mass     # (a field: "auto" is the two-pass form)
        self._mass_in_op = []            # the levels whose Jacobian operator carries a0 rho M (fused_mass): cleared by destroy()
        if any(kw.get(k) is not None for k in ("gravity", "acceleration_field", "spin")):
            kw.setdefault("density", density)            # the body loads (body.LoadedBody) weigh the body with the stepper's density
        super().__init__(prob, **kw)
        if fused_mass is not False:
            try:
                self._set_mass_terms()
            except Exception:            # (fused_mass=True without the kernel): nothing of this object is left behind, no term stays set
                self._clear_mass_terms()
                for m in self.mass:
                    m.destroy()
                NewtonPMG.destroy(self)
                raise
        n, top = prob.lsize(), self.nlev - 1
        self.mass_res = MassOperator(prob, prob.fine, self.density, mask_mode=2, density=field)      # the residual's: reads the boundary values
        self.xn, self.vn, self.an, self._pred, self._acc, self._mt = (self._vec(n, top) for _ in range(6))
        self._vnew = self._vec(n, top) if self.supports else None      # v_{n+1} of the dashpot force; 1/2 u . K_s u's product
        self.t = 0.0
        self.last_rnorm = 0.0
        self._load_fn: Callable[[float], float] = lambda t: 1.0
        self._started = False

    # ---- the effective operator K + a0 rho M --------------------------------------------------------------------------------
    def _set_mass_terms(self):
        """fused_mass: a0 rho M into the Jacobian operator of every matrix-free level that has the kernel.  Never on a level whose matrix
        is assembled: AssembledLevel(mass_coef=) already adds M there, and its probes apply this operator."""
        for lv, level in enumerate(self.p.levels):
            if lv == 0 and self.asm is not None:
                continue
            op = level.opJacob
            if not (op.L.has("CeedXOperatorSetMassTerm") and op.mass_term_available()):
                if self.fused_mass is True:
                    raise ValueError(f"NewmarkPMG(fused_mass=True): no fused Jacobian kernel with the mass term for level {lv} "
                                     f"(P={level.degree + 1}, Q={level.Q}) in this library; fused_mass='auto' keeps two passes there")
                continue
            op.set_mass_term(self.a0 * self.density)
            self._mass_in_op.append(lv)

    def _clear_mass_terms(self):
        for lv in self._mass_in_op:
            self.p.levels[lv].opJacob.set_mass_term(0.0)
        self._mass_in_op = []

    def A(self, lv, x, y):
        super().A(lv, x, y)           # (a level in _mass_in_op: K + a0 rho M in this one apply)
        if lv not in self._mass_in_op and not (lv == 0 and self.asm is not None):     # (the assembled level holds its mass term in the matrix)
            self.mass[lv].apply_add(x, y)

    def _fused_op(self, lv):
        """The level's Jacobian operator where it carries the mass term itself (the parent's conditions besides); None: two passes."""
        return super()._fused_op(lv) if lv in self._mass_in_op else None

    def _support_tangent_state(self, s):
        """K_s + a1 C_d as ONE state, formed at the first call (dt is fixed per solver); its entry 6 means nothing and is never read."""
        if s["dashpot"] is None:
            return s["spring"]
        if s.get("combined") is None:
            c = s["combined"] = s["levels"][self.nlev - 1].new_state()
            if s["spring"] is not None:
                c.waxpby(1.0, s["spring"], self.a1, s["dashpot"])
            else:
                c.axpby(self.a1, s["dashpot"], 0.0)
        return s["combined"]

    def _get_diag(self, lv, d):
        super()._get_diag(lv, d)
        if lv not in self._mdiag:                # M does not change: its diagonal is formed once per level
            m = self._vec(self.p.lsize(lv), lv)
            self.mass[lv].diagonal(m)
            self._mdiag[lv] = m
        d.axpby(1.0, self._mdiag[lv], 1.0)

    # ---- residual with the inertia term ----------------------------------------------------------------------------------------
    def residual(self, U, R):
        """R = F_int(x) - load f (+ pressure) + rho M (a0 x + pred), x = U + boundary values, pred = -(a0 x_n + a2 v_n + a3 a_n)."""
        super().residual(U, R)
        self._acc.waxpby(self.a0, self.Xloc, 1.0, self._pred)
        self.mass_res.apply_add(self._acc, R)
        if self.supports and self.has_dashpots():        # C_d v_{n+1}, v_{n+1} = v_n + dt ((1 - gamma) a_n + gamma a_{n+1})
            self._vnew.waxpby(1.0, self.vn, self.dt * (1.0 - self.gamma), self.an)
            self.axpby(self._vnew, self.dt * self.gamma, self._acc, 1.0)
            self.support_force_add("dashpot", self._vnew, R)

    def support_energy(self) -> float:
        """1/2 u . K_s u of the springs at the current displacement, over the free rows (the rows the force writes)."""
        if not self.supports:
            return 0.0
        self._vnew.set_value(0.0)
        self.support_force_add("spring", self.xn, self._vnew)
        return 0.5 * self.dot(self.xn, self._vnew, True)

    def kinetic_energy(self) -> float:
        """1/2 v . rho M v over the free rows."""
        self.mass_res.apply(self.vn, self._mt)
        return 0.5 * self.dot(self.vn, self._mt, True)

    # ---- start ---------------------------------------------------------------------------------------------------------------
    def set_initial(self, u0=None, v0=None, load: Union[float, Callable[[float], float]] = 1.0):
        """State at t = 0: displacement u0 and velocity v0 (host L-vectors; None: zero) on the free dofs, the boundary values of
        load(0) on the others, and a_0 = (rho M)^-1 (load f - F_int(u_0) - pressure terms) on the free dofs by Jacobi-preconditioned CG
        on the mass operator (its condition number is O(1))."""
        self._load_fn = self._load_function(load)
        n = self.p.lsize()
        free = self.free
        self.t = 0.0
        self.load = float(self._load_fn(0.0))
        self._set(self.bcv, self.bc_values(self.load))
        self._set(self.U, (np.zeros(n) if u0 is None else np.asarray(u0, dtype=np.float64).reshape(-1)[:n]) * free)
        self._set(self.vn, (np.zeros(n) if v0 is None else np.asarray(v0, dtype=np.float64).reshape(-1)[:n]) * free)
        NewtonPMG.residual(self, self.U, self.R)         # the static residual (no inertia); also Xloc = U + boundary values
        self.copy(self.xn, self.Xloc)
        if self.supports and self.has_dashpots():        # a_0 takes -C_d v_0 beside the -K_s u_0 of the static residual
            self.support_force_add("dashpot", self.vn, self.R)
        self.axpby(self.Rtry, -1.0, self.R, 0.0)
        self._mass_solve(self.Rtry, self.an)             # a_0 = -(rho M)^-1 R_static
        self._started = True

    def _mass_solve(self, b, x, rtol: float = 1e-13, maxit: int = 200):
        """x = (rho M)^-1 b on the free dofs: Jacobi-preconditioned CG with the fine level's tangent mass operator at coefficient rho."""
        M, w = self.mass[self.nlev - 1], self.w[self.nlev - 1]
        M.set_coef(self.density)
        dinv = w["x"]
        M.diagonal(dinv)
        dinv.reciprocal()
        pcg(M.apply, lambda z, r: z.pointwise_mult(r, dinv), lambda u, v: self.dot(u, v, True), b, x, w["r"], w["z"], w["d"], w["t"], rtol, maxit)
        M.set_coef(self.a0 * self.density)

    # ---- one step ------------------------------------------------------------------------------------------------------------
    def step(self) -> SolveStats:
        """Advance (u, v, a) from t to t + dt; returns this step's SolveStats (``history``: (step count, Newton iteration, Krylov
        iterations, line-search step, |R|) per Newton iteration)."""
        if not self._started:
            self.set_initial()
        st = self.stats = SolveStats()
        t0 = time.perf_counter()
        self.t += self.dt
        self.load = float(self._load_fn(self.t))
        self._set(self.bcv, self.bc_values(self.load))
        # pred = -(a0 x_n + a2 v_n + a3 a_n)
        self._pred.waxpby(-self.a0, self.xn, -self.a2, self.vn)
        self.axpby(self._pred, -self.a3, self.an, 1.0)
        self.residual(self.U, self.R)                    # the start of the iteration: u_n on the free dofs
        rnorm0, rnorm = self._newton(1, f"t = {self.t:.6g}")
        st.converged = bool(np.isfinite(rnorm) and (rnorm <= self.snes_rtol * rnorm0 or rnorm < 1e-50))
        st.increments = 1
        self.last_rnorm = float(rnorm)
        # a_{n+1} = a0 x_{n+1} + pred;  v_{n+1} = v_n + dt ((1 - gamma) a_n + gamma a_{n+1});  Xloc is x_{n+1} (the last residual's)
        self._acc.waxpby(self.a0, self.Xloc, 1.0, self._pred)
        self.axpby(self.vn, self.dt * (1.0 - self.gamma), self.an, 1.0)
        self.axpby(self.vn, self.dt * self.gamma, self._acc, 1.0)
        self.copy(self.an, self._acc)
        self.copy(self.xn, self.Xloc)
        self.ceed.synchronize()
        st.seconds = time.perf_counter() - t0
        self._drop_pc_graph()
        return st

    def run(self, nsteps: int, load: Union[float, Callable[[float], float], None] = None) -> dict:
        """``nsteps`` steps from the current state (``set_initial`` first; ``load`` given here replaces its load function).  Returns the
        history: per step t, |u| and max |u| over the free dofs, the kinetic energy 1/2 v . rho M v, Newton and Krylov counts, the last
        Newton residual norm and whether the step converged."""
        if load is not None:
            self._load_fn = self._load_function(load)
        if not self._started:
            self.set_initial(load=self._load_fn)
        h = {k: [] for k in ("t", "norm_u", "max_u", "kinetic", "newton_its", "ksp_its", "rnorm", "converged")}
        for _ in range(nsteps):
            st = self.step()
            u = self.U.to_numpy()
            h["t"].append(self.t); h["norm_u"].append(float(np.sqrt(np.square(u).sum()))); h["max_u"].append(float(np.abs(u).max()))
            h["kinetic"].append(self.kinetic_energy())
            h["newton_its"].append(st.newton_its); h["ksp_its"].append(st.ksp_its)
            h["rnorm"].append(self.last_rnorm); h["converged"].append(st.converged)
            if not st.converged:
                break
        return h

    def destroy_mass(self):
        for m in self.mass + [self.mass_res]:
            m.destroy()

    def destroy(self):
        self._drop_pc_graph()            # (a recording holds the coefficient: gone before the term is)
        self._clear_mass_terms()         # the problem's operators are left as they were found
        self.destroy_mass()
        super().destroy()


class ExplicitDynamics(LoadedBody):
    """Explicit elastodynamics: the central-difference ("leapfrog") rule with a lumped mass m (mass.MassOperator.lumped: the row sums of
    rho M) and a mass-proportional damping alpha,

        m a_n + alpha m v_n + R(x_n, t_n) = 0,      R = F_int(x) - load(t) (f + tractions) + load(t) sum_s p_s g_s^pressure(x)
        a_n = (vh_{n+1/2} - vh_{n-1/2}) / dt,       v_n = (vh_{n+1/2} + vh_{n-1/2}) / 2
        vh_{n+1/2} = c1 vh_{n-1/2} + c2 (-R_n / m), c1 = (1 - alpha dt/2) / (1 + alpha dt/2),  c2 = dt / (1 + alpha dt/2)
        x_{n+1} = x_n + dt vh_{n+1/2}

    on the free rows; the constrained rows of x carry the boundary values of load(t) (``bc_values``), m is zero there and the step
    leaves them alone.  A step is ONE vector kernel (CeedXVectorLeapfrogStep, csrc/kernels_explicit.hip; its NumPy form on the CPU
    oracle) and one evaluation of the residual: no preconditioner, no Krylov loop, no coarse level -- the class is a body.LoadedBody
    (the boundary values, the load vector, the surface loads and ``A``, the tangent of the stable-step estimate) and takes its
    keywords only; a preconditioner keyword is a TypeError.  With a constant load nothing between two steps touches the host.

    State: ``x`` (the L-vector WITH the boundary values: what the residual reads; it is the parent's ``Xloc``), ``vh`` (the half-step
    velocity), ``R`` (the residual at x), ``m``.  After ``step()``: x = x_{n+1}, vh = vh_{n+1/2}, R = R(x_{n+1}), t = t_{n+1}.

    The step is conditionally stable: dt < 2 / sqrt(lambda_max(m^-1 K_T)).  ``stable_dt`` estimates the bound with the Lanczos
    recurrence of krylov.py and the margin 1.1 the Chebyshev smoothers put on the same estimate; ``dt=None`` takes it at
    ``set_initial``, a given dt beyond it is refused there.  dt is fixed per object.  Supports (``support=``): the force adds
    K_s x_n + C_d vh_{n-1/2} and ``stable_dt`` becomes safety (-c + sqrt(c^2 + 4 w^2)) / w^2 with w^2 = 1.1 emax(m^-1 (K_T + K_s)) and
    c = 1.1 emax(m^-1 C_d); without a dashpot the old expression is evaluated.

    Refused: a halo with several ranks (the mass operator's interface sums were never run there), density <= 0, dt <= 0, damping < 0,
    and at ``set_initial`` a lumped mass with a non-positive free row."""

    def __init__(self, prob: SolidProblem, density, dt: Optional[float] = None, damping: float = 0.0, safety: float = 0.9, **kw):
        """``density``: a positive float or a mass.DensityField; the lumped mass is formed from it, and ``stable_dt`` follows."""
        rho, field = split_density(density, "density and dt must be positive")
        self.density_field = field
        if not (dt is None or dt > 0.0):
            raise ValueError("density and dt must be positive")
        _refuse_contact(kw)
        if not damping >= 0.0:
            raise ValueError("damping (the mass-proportional coefficient alpha) must not be negative")
        if not 0.0 < safety <= 1.0:
            raise ValueError("safety must lie in (0, 1]")
        self._refuse_several_ranks(kw.get("halo"), "ExplicitDynamics is", "the mass operator's sums at the interface nodes have not been "
                                   "run over several ranks")
        if any(kw.get(k) is not None for k in ("gravity", "acceleration_field", "spin")):
            kw.setdefault("density", density)            # the body loads (body.LoadedBody) weigh the body with the stepper's density
        super().__init__(prob, **kw)
        self.density, self.damping, self.safety = rho, float(damping), float(safety)
        self.dt = None if dt is None else float(dt)
        self.c1 = self.c2 = None
        n, top = prob.lsize(), self.nlev - 1
        self.x = self.Xloc                      # (the body's name for "free part + boundary values": A_outer reads it)
        self.vh, self.m, self.minv_m, self._freev = (self._vec(n, top) for _ in range(4))
        self._tally = self._vec(2, top)         # slot 0: the kinetic energy of a sampled step
        self._lanczos_work = None               # the four work vectors of stable_dt, made at its first call
        self.mass_lumped = MassOperator(prob, prob.fine, self.density, mask_mode=2, density=field)
        self.mass_lumped.lumped(self.m)         # formed once per solver object
        self._set(self._freev, self.free.astype(np.float64))
        self.t, self.nsteps_done = 0.0, 0
        self._load_fn: Callable[[float], float] = lambda t: 1.0
        self._load_const = True
        self._started = self._have_R = False
        self._x_start = None
        self.emax_K = self.emax_C = None

    # ---- pieces ---------------------------------------------------------------------------------------------------------------
    def _force(self):
        """R = F_int(x) + load sum_s p_s g_s^pressure(x) (every follower load: body.follower_add), constrained rows dropped (the load vector
        enters in the step itself)."""
        self.p.form_residual(self.x, self.R)
        self.follower_add(self.x, self.R)
        if self.supports:                        # K_s x_n + C_d vh_{n-1/2}: the half-step velocity lagged
            self.support_force_add("spring", self.x, self.R)
            self.support_force_add("dashpot", self.vh, self.R)
        self.stats.residual_evals += 1
        self._have_R = True

    def _set_boundary(self, load: float):
        """The constrained rows of x := the boundary values at ``load`` (one upload; the free rows keep their bits: x * 1 + 0)."""
        self._set(self.bcv, self.bc_values(load))
        self.x.pointwise_mult(self.x, self._freev)
        self.axpby(self.x, 1.0, self.bcv, 1.0)

    def _check_mass(self) -> np.ndarray:
        m = self.m.to_numpy()
        bad = self.free & ~(m > 0.0)
        if bad.any():
            rows = np.flatnonzero(bad)
            worst = int(rows[np.argmin(np.where(np.isnan(m[rows]), -np.inf, m[rows]))])
            raise ValueError(f"ExplicitDynamics: the lumped mass is not positive on {rows.size} free rows; the worst is row {worst} "
                             f"(m = {m[worst]!r})")
        return m

    def _q_host(self, m: np.ndarray) -> np.ndarray:
        """(load f - R) / m on the free rows (host), zero elsewhere: the undamped acceleration at the state of the last residual."""
        g = -self.R.to_numpy()
        if self.fv is not None:
            g = self.load * self.fv.to_numpy() + g
        q = np.zeros_like(g)
        q[self.free] = g[self.free] / m[self.free]
        return q

    # ---- the stable step ------------------------------------------------------------------------------------------------------------
    def stable_dt(self, steps: int = 20) -> float:
        """safety * 2 / sqrt(1.1 emax), emax the Lanczos estimate (``steps`` steps; an estimate from below, hence the margin 1.1 of
        ``krylov.chebyshev_coefficients``) of lambda_max(m^-1 K_T), K_T the tangent at the state of the last residual evaluation."""
        if not self._have_R:
            self._force()
        self._set(self.minv_m, np.where(self.free, 1.0 / np.where(self.free, self._check_mass(), 1.0), 0.0))
        top = self.nlev - 1
        if self._lanczos_work is None:
            self._lanczos_work = [self._vec(self.free.size, top) for _ in range(4)]
        al, be = lanczos_device(self.ceed, lambda x, y: self.A(top, x, y), lambda z, r: z.pointwise_mult(r, self.minv_m),
                                self._start_vector(top), *self._lanczos_work, steps)
        self.emax_K = lanczos_emax(al, be)
        if not (self.supports and self.has_dashpots()):
            return self.safety * 2.0 / np.sqrt(1.1 * self.emax_K)
        # dashpots, lagged: the scalar Jury condition 4 - dt^2 w^2 - 2 c dt > 0 with w^2 = 1.1 emax(m^-1 (K_T + K_s)) (``A`` carries
        # the springs) and c = 1.1 emax(m^-1 C_d) from a second recurrence

        def C(x, y):
            y.set_value(0.0)
            for s in self.supports:
                if s["dashpot"] is not None:
                    s["levels"][top].tangent_add(1.0, s["dashpot"], x, y)
        al, be = lanczos_device(self.ceed, C, lambda z, r: z.pointwise_mult(r, self.minv_m), self._start_vector(top), *self._lanczos_work, steps)
        self.emax_C = lanczos_emax(al, be)
        w2, c = 1.1 * self.emax_K, 1.1 * self.emax_C
        return self.safety * (-c + np.sqrt(c * c + 4.0 * w2)) / w2

    # ---- start ---------------------------------------------------------------------------------------------------------------------
    def set_initial(self, u0=None, v0=None, load: Union[float, Callable[[float], float]] = 1.0):
        """State at t = 0: u0, v0 (host L-vectors; None: zero) on the free rows, the boundary values of load(0) on the others;
        a_0 = (load f - R(x_0)) / m - alpha v_0 (the damping term in the form the step takes it) and vh_{-1/2} = v_0 - dt/2 a_0, so
        that (vh_{-1/2} + vh_{1/2}) / 2 = v_0.  dt is settled here: ``stable_dt()`` if none was given; a given one above
        stable_dt() / safety is refused."""
        self._load_const = not callable(load)
        self._load_fn = self._load_function(load)
        n, free = self.p.lsize(), self.free
        m = self._check_mass()
        self.t, self.nsteps_done = 0.0, 0
        self.load = float(self._load_fn(0.0))
        as_l = lambda a: np.zeros(n) if a is None else np.asarray(a, dtype=np.float64).reshape(-1)[:n]
        x0 = as_l(u0) * free + self.bc_values(self.load)
        self._set(self.x, x0)
        self._x_start = x0
        if self.supports and self.has_dashpots():          # the dashpot force of a_0 is C_d v_0
            self._set(self.vh, as_l(v0) * free)
        self._force()
        limit = self.stable_dt()
        if self.dt is None:
            self.dt = float(limit)
        elif self.dt > limit / self.safety:
            how = (f"2 / sqrt(1.1 x the estimate {self.emax_K:.6g} of lambda_max(m^-1 K_T))" if self.emax_C is None else
                   f"(-c + sqrt(c^2 + 4 w^2)) / w^2 with w^2, c = 1.1 x the estimates {self.emax_K:.6g}, {self.emax_C:.6g} of "
                   "lambda_max(m^-1 (K_T + K_s)), lambda_max(m^-1 C_d)")
            raise ValueError(f"ExplicitDynamics: dt = {self.dt:.6g} is above the stable step {limit / self.safety:.6g} ({how})")
        h = 0.5 * self.damping * self.dt
        self.c1, self.c2 = (1.0 - h) / (1.0 + h), self.dt / (1.0 + h)
        v = as_l(v0) * free
        self._set(self.vh, (v - 0.5 * self.dt * (self._q_host(m) - self.damping * v)) * free)
        self._started = True

    # ---- one step --------------------------------------------------------------------------------------------------------------------
    def _kernel(self, tally: bool):
        self.x.leapfrog_step(self.vh, self.R, self.fv, self.m, self.load, self.c1, self.c2, self.dt, self.p.lsize(),
                             self._tally if tally else None, 0)

    def _device_step(self, tally: bool):
        """The kernel and the residual of one step at a load that does not change: everything here is queued, nothing read."""
        self._kernel(tally)
        self._force()

    def step(self, tally: bool = False):
        """(x_n, vh_{n-1/2}, R_n) -> (x_{n+1}, vh_{n+1/2}, R_{n+1}); ``tally``: the kinetic energy 1/2 sum m v_n^2 goes to the device
        slot that ``run`` samples."""
        if not self._started:
            self.set_initial()
        self._kernel(tally)
        self.nsteps_done += 1
        self.t = self.nsteps_done * self.dt
        load = float(self._load_fn(self.t))
        if load != self.load:                    # (a constant load: no upload, no host read between two steps)
            self._set_boundary(load)
            self.load = load
        self._force()

    def set_load(self, load: Union[float, Callable[[float], float]]):
        """Replace the load (a constant, or a function of time) from the current time on.  A constant makes ``run(graph=True)`` possible
        again after a load function has run its course, e.g. once a ramp has reached its plateau."""
        self._load_const = not callable(load)
        self._load_fn = self._load_function(load)
        value = float(self._load_fn(self.t))
        if self._started and value != self.load:
            self._set_boundary(value)
            self.load = value
            self._force()

    def run(self, nsteps: int, sample_every: int = 0, graph: bool = False) -> dict:
        """``nsteps`` steps from the current state.  Every ``sample_every`` steps (0: never; the kernel then sums nothing) the history
        takes t (the time of x), the kinetic energy and its time t - dt (the step the tally belongs to) and max |x - x_0|; the run ends
        with ``diverged`` at the first sample that is not finite.  ``graph``: after one eager step, one step (kernel + residual) is
        recorded and replayed; load, c1, c2, dt are frozen in the recording, so a load FUNCTION is refused, and the tally is recorded
        in or out according to sample_every > 0."""
        if graph and not self._load_const:
            raise ValueError("ExplicitDynamics.run: graph=True needs a constant load (the load is a launch argument frozen in the recording)")
        if sample_every < 0:
            raise ValueError("sample_every must not be negative")
        if not self._started:
            self.set_initial(load=self._load_fn if not self._load_const else self.load)
        h = {"t": [], "t_kinetic": [], "kinetic": [], "max_disp": [], "steps": 0, "diverged": False, "seconds": 0.0}
        rec = None
        t0 = time.perf_counter()
        try:
            for k in range(nsteps):
                sample = sample_every > 0 and (k + 1) % sample_every == 0
                if graph and k == 1:
                    rec = self.ceed.capture(lambda: self._device_step(sample_every > 0))
                    self.stats.residual_evals -= 1
                if rec is not None:
                    rec.launch()
                    self.nsteps_done += 1
                    self.t = self.nsteps_done * self.dt
                    self.stats.residual_evals += 1
                else:
                    self.step(sample or (graph and sample_every > 0))
                h["steps"] += 1
                if sample:
                    ke = float(self._tally.to_numpy()[0])
                    d = float(np.abs(self.x.to_numpy() - self._x_start).max())
                    h["t"].append(self.t); h["t_kinetic"].append(self.t - self.dt); h["kinetic"].append(ke); h["max_disp"].append(d)
                    if graph:                    # a replay writes the arrays behind the vectors: the host mirrors just made are dropped
                        self._drop_host_mirrors()
                    if not (np.isfinite(ke) and np.isfinite(d)):
                        h["diverged"] = True
                        break
            self.ceed.synchronize()
        finally:
            if rec is not None:
                rec.destroy()
                self._drop_host_mirrors()
        h["seconds"] = time.perf_counter() - t0
        return h

    def _drop_host_mirrors(self):
        """A replayed recording writes x, vh, R and the tally by device address, which their validity flags do not see: asking for the
        device array with write access (no copy, no synchronisation: the device side is the valid one) drops a host mirror."""
        for v in (self.x, self.vh, self.R, self._tally):
            v.device_pointer()

    # ---- off the hot path ------------------------------------------------------------------------------------------------------------
    def velocity(self) -> np.ndarray:
        """The full-step velocity at the time of x (host): (vh_{n-1/2} + vh_{n+1/2}) / 2 with the half step ahead formed from the
        current R as the kernel will form it; zero on the constrained rows."""
        vh = self.vh.to_numpy()
        vn = self.c1 * vh + self.c2 * self._q_host(self.m.to_numpy())
        return 0.5 * (vh + vn) * self.free

    def kinetic_energy(self) -> float:
        """1/2 sum m v^2 over the free rows, v = ``velocity()``."""
        v = self.velocity()
        return 0.5 * float(np.sum(self.m.to_numpy() * (v * v)))

    def destroy_mass(self):
        self.mass_lumped.destroy()
        for v in (self.vh, self.m, self.minv_m, self._freev, self._tally):
            v.destroy()

    def destroy(self):
        self.destroy_mass()
        super().destroy()
