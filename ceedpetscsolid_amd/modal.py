"""Modal analysis: the lowest natural frequencies and mode shapes of the body a solver object describes, by LOBPCG (locally optimal
block preconditioned conjugate gradients, Knyazev 2001) with the solver's own p-multigrid V-cycle as preconditioner.

    A x = mu B x,      B = rho M (mass.MassOperator on the fine level),      A = the solver's fine-level operator ``sol.A(top, ., .)``:

- ``solver.NewtonPMG``: A = K, the tangent stiffness at the state of the solver's last residual evaluation (U = 0 if none was made; after
  ``sol.solve()`` the modes of the PRESTRESSED body), lambda = mu;
- ``dynamics.NewmarkPMG``: A = K + a0 rho M with the same density -- the same eigenvectors, lambda = mu - a0.  This is the spectral shift
  that makes a body with no clamped side tractable: its six rigid-body modes sit at lambda ~ 0 and A stays positive definite for the
  V-cycle.

omega_i = sqrt(lambda_i).  The preconditioner is ``sol.precondition`` after ``sol.setup_preconditioner()`` (symmetric positive definite:
tests/test_vcycle_dense*.py), replayed from its recorded graph where the solver was built with ``graph=``.

With m = nmodes + guard columns, every block lives in the Ceed's memory (``ceed.BlockVector``): S = [W | X | P] and its images A S, B S
are blocks of 3 m columns, so the Rayleigh-Ritz step of an iteration is two Gram matrices of 3 m x 3 m (``BlockVector.gram``) and three
combinations with a 3 m x 2 m matrix that give [X | P] of the next iteration (``BlockVector.combine``, into a second set of blocks
that is then swapped in).  Only those small matrices cross to the host, where the dense algebra is ``numpy.linalg``.  The operators, the
mass apply and the V-cycle take the columns one at a time.

    X = random (seeded), masked to the free dofs;  Rayleigh-Ritz on X
    repeat:  R = A X - B X diag(mu);  rn_i = |R_i| / (|A X_i| + |mu_i| |B X_i|);  stop when rn_i < tol for all i < nmodes
             W = T R;  W -= X (B X)^T W;  A W, B W
             G_B = S^T B S, G_A = S^T A S;  scaled by diag(G_B)^-1/2, Cholesky of G_B, eigh of the reduced G_A
                 (no P in the first iteration; a failed Cholesky: the same without P for this iteration)
             C = the first m Ritz vectors, C_P = C with its X rows zeroed;  [X | P] <- S [C | C_P], and the same for A S and B S

Refused (ValueError): no constrained dof and no shift (K is singular and so is the V-cycle's operator); pressure loads on the solver
(their tangent is not symmetric in general); a halo with several ranks (the mass operator and the block reductions were never run
there); nmodes + guard > 16 (3 m columns must fit the 48 of a block operation).  Soft locking of converged columns and a recorded graph of
the whole iteration are not provided.
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import ceed as cd
from .mass import MassOperator, split_density

MAX_COLUMNS = 16


@dataclass
class ModalResult:
    frequencies: np.ndarray            # omega_i = sqrt(max(lambda_i, 0)), ascending
    eigenvalues: np.ndarray            # lambda_i (the shift taken off)
    modes: "cd.BlockVector"            # nmodes columns, (rho M)-orthonormal, zero on the constrained dofs
    iterations: int
    residuals: np.ndarray              # rn_i of the returned modes
    converged: bool
    history: list = field(default_factory=list)    # max rn_i over the wanted modes, per iteration
    seconds: float = 0.0
    timings: dict = field(default_factory=dict)    # profile=True: seconds per part, each behind a synchronisation


def _ritz(GA: np.ndarray, GB: np.ndarray, m: int):
    """The m lowest Ritz pairs of the pencil (GA, GB): GB scaled to a unit diagonal, its Cholesky factor, eigh of the reduced GA.
    Raises numpy.linalg.LinAlgError where GB is not positive definite to rounding."""
    GA, GB = 0.5 * (GA + GA.T), 0.5 * (GB + GB.T)
    d = np.diag(GB)
    if not (np.all(np.isfinite(d)) and np.all(d > 0.0)):
        raise np.linalg.LinAlgError("non-positive diagonal of S^T B S")
    d = 1.0 / np.sqrt(d)
    L = np.linalg.cholesky(GB * d[:, None] * d[None, :])
    Li = np.linalg.inv(L)
    H = Li @ (GA * d[:, None] * d[None, :]) @ Li.T
    th, Z = np.linalg.eigh(0.5 * (H + H.T))
    return th[:m], d[:, None] * (Li.T @ Z[:, :m])


class Eigenmodes:
    def __init__(self, sol, density: float, nmodes: int, guard: int = 2, tol: float = 1e-8, maxit: int = 200, seed: int = 0,
                 profile: bool = False):
        from .dynamics import NewmarkPMG
        if nmodes < 1 or guard < 0:
            raise ValueError("nmodes must be at least 1 and guard must not be negative")
        if nmodes + guard > MAX_COLUMNS:
            raise ValueError(f"nmodes + guard = {nmodes + guard} > {MAX_COLUMNS}: the 3 (nmodes + guard) columns of [W | X | P] must fit the "
                             f"{cd.BLOCK_MAX_COLS} columns of a block operation")
        rho, field = split_density(density, "density must be positive")     # a mass.DensityField: B = M_rho
        if sol.halos:
            raise ValueError("Eigenmodes is not provided with a halo (several ranks): the mass operator's interface sums and the block "
                             "reductions have not been run over several ranks")
        if sol.pressure_loads or getattr(sol, "field_loads", None):
            raise ValueError("Eigenmodes is not provided with pressure loads on the solver: the tangent T(u) of a follower pressure is not "
                             "symmetric in general")
        self.shift = 0.0
        if isinstance(sol, NewmarkPMG):
            if sol.smoother == "pbjacobi":
                raise ValueError("Eigenmodes: smoother='pbjacobi' is not provided with a Newmark solver")
            if field is not sol.density_field or abs(sol.density - rho) > 1e-14 * abs(rho):
                raise ValueError(f"Eigenmodes: density {density!r} differs from the Newmark solver's {sol.density!r}: its operator "
                                 "K + a0 rho M shifts the spectrum by a0 only with the same rho")
            self.shift = sol.a0
        elif bool(np.all(sol.free)):
            raise ValueError("Eigenmodes: no constrained dof and no shift: K is singular (six rigid-body modes); build the solver as a "
                             "dynamics.NewmarkPMG, whose operator K + a0 rho M is positive definite")
        self.sol, self.prob, self.ceed = sol, sol.p, sol.ceed
        self.density, self.density_field, self.nmodes, self.guard, self.m = rho, field, int(nmodes), int(guard), int(nmodes + guard)
        self.tol, self.maxit, self.seed, self.profile = float(tol), int(maxit), int(seed), bool(profile)
        self.n, self.top = self.prob.lsize(), sol.nlev - 1
        if self.m > int(np.count_nonzero(sol.free)):
            raise ValueError("nmodes + guard exceeds the number of free dofs")
        self.mass = MassOperator(self.prob, self.prob.fine, self.density, density=field)
        self.blocks = None
        self.block_calls = {"gram": 0, "combine": 0}

    # ---- pieces -------------------------------------------------------------------------------------------------------------------
    def _tick(self, key, t0):
        if self.profile:
            self.ceed.synchronize()
            self.timings[key] = self.timings.get(key, 0.0) + time.perf_counter() - t0
            return time.perf_counter()
        return t0

    def _gram(self, Ab, Bb, a0, ka, b0, kb) -> np.ndarray:
        t0 = time.perf_counter()
        Ab.gram(Bb, self._G, a0=a0, ka=ka, b0=b0, kb=kb)
        self.block_calls["gram"] += 1
        t0 = self._tick("gram", t0)
        g = self._G.to_numpy()[:ka * kb].reshape(ka, kb)
        self._tick("host", t0)
        return g

    def _combine(self, Yb, Ab, Cm, y0, ky, a0, ka, beta=0.0):
        t0 = time.perf_counter()
        Yb.combine(Ab, Cm, y0=y0, ky=ky, a0=a0, ka=ka, beta=beta)
        self.block_calls["combine"] += 1
        self._tick("combine", t0)

    def _apply_AB(self, S, AS, BS, first, count):
        t0 = time.perf_counter()
        for j in range(first, first + count):
            self.sol.A(self.top, S[j], AS[j])
        t0 = self._tick("A", t0)
        for j in range(first, first + count):
            self.mass.apply(S[j], BS[j])
        self._tick("B", t0)

    def _precondition(self, r, z):
        sol = self.sol
        if sol._pc_graph is not None:           # the recording reads and writes the solver's own pair of vectors
            gr, gz = sol._pc_graph_io
            sol.copy(gr, r)
            sol.precondition(gr, gz)
            sol.copy(z, gz)
        else:
            sol.precondition(r, z)

    # ---- the iteration ------------------------------------------------------------------------------------------------------------
    def solve(self) -> ModalResult:
        from .solver import NewtonPMG
        sol, c, n, m = self.sol, self.ceed, self.n, self.m
        self.timings = {}
        t_start = time.perf_counter()
        if sol.stats.residual_evals == 0:          # the state the operator is linearised about: the undeformed body
            sol.U.set_value(0.0)
            NewtonPMG.residual(sol, sol.U, sol.R)
        sol.setup_preconditioner()
        if sol.graph or sol._auto_graph or sol._auto_fuse:
            sol.record_preconditioner(sol.w[self.top]["b"], sol.kz)
        # two sets of [W | X | P] with their images: the combinations are not in place
        cur = [c.block(n, 3 * m) for _ in range(3)]
        nxt = [c.block(n, 3 * m) for _ in range(3)]
        R = c.block(n, m)
        self._G = c.vector(9 * m * m)
        self.blocks = cur + nxt + [R]
        free = np.asarray(sol.free, dtype=np.float64)
        X0 = np.random.default_rng(self.seed).uniform(-1.0, 1.0, (m, n)) * free[None, :]
        S, AS, BS = cur
        S.fill(X0, first=m)
        self._apply_AB(S, AS, BS, m, m)
        t0 = time.perf_counter()
        mu, Cm = _ritz(self._gram(S, AS, m, m, m, m), self._gram(S, BS, m, m, m, m), m)
        self._tick("host", t0)
        for dst, src in zip(nxt, cur):
            self._combine(dst, src, Cm, m, m, m, m)
        cur, nxt = nxt, cur
        have_P, its, history, rn = False, 0, [], np.full(m, np.inf)
        converged = False
        while True:
            S, AS, BS = cur
            for i in range(m):
                R[i].waxpby(1.0, AS[m + i], -float(mu[i]), BS[m + i])
            nr = np.sqrt(np.abs(np.diag(self._gram(R, R, 0, m, 0, m))))
            na = np.sqrt(np.abs(np.diag(self._gram(AS, AS, m, m, m, m))))
            nb = np.sqrt(np.abs(np.diag(self._gram(BS, BS, m, m, m, m))))
            rn = nr / (na + np.abs(mu) * nb)
            history.append(float(rn[:self.nmodes].max()))
            if np.all(rn[:self.nmodes] < self.tol):
                converged = True
                break
            if its >= self.maxit or not np.all(np.isfinite(rn)):
                break
            its += 1
            t0 = time.perf_counter()
            for i in range(m):
                self._precondition(R[i], S[i])
            self._tick("vcycle", t0)
            self._combine(S, S, -self._gram(BS, S, m, m, 0, m), 0, m, m, m, beta=1.0)        # W -= X (B X)^T W
            self._apply_AB(S, AS, BS, 0, m)
            k = 3 * m if have_P else 2 * m
            while True:
                GA, GB = self._gram(S, AS, 0, k, 0, k), self._gram(S, BS, 0, k, 0, k)
                t0 = time.perf_counter()
                try:
                    mu, Cm = _ritz(GA, GB, m)
                    self._tick("host", t0)
                    break
                except np.linalg.LinAlgError:
                    if k == 2 * m:
                        raise RuntimeError(f"Eigenmodes: S^T B S of [W | X] is not positive definite in iteration {its}")
                    k = 2 * m
            CP = Cm.copy()
            CP[m:2 * m] = 0.0
            C2 = np.concatenate([Cm, CP], axis=1)                                             # [X | P] of the next iteration
            for dst, src in zip(nxt, cur):
                self._combine(dst, src, C2, m, 2 * m, 0, k)
            cur, nxt = nxt, cur
            have_P = True
        modes = c.block(n, self.nmodes)
        modes.combine(cur[0], np.eye(m)[:, :self.nmodes], a0=m, ka=m)
        self.block_calls["combine"] += 1
        lam = mu[:self.nmodes] - self.shift
        c.synchronize()
        res = ModalResult(frequencies=np.sqrt(np.maximum(lam, 0.0)), eigenvalues=lam, modes=modes, iterations=its,
                          residuals=rn[:self.nmodes].copy(), converged=converged, history=history,
                          seconds=time.perf_counter() - t_start, timings=dict(self.timings))
        self._release()
        return res

    def _release(self):
        for b in self.blocks or []:
            b.destroy()
        self.blocks = None
        if getattr(self, "_G", None) is not None:
            self._G.destroy()
            self._G = None

    def destroy(self):
        self._release()
        if self.mass is not None:
            self.mass.destroy()
            self.mass = None
