"""What the p-multigrid levels (solver.py) and the aggregation levels under them (amg.py) share: the eigenvalue estimate of the
Chebyshev smoother -- KSPChebyshevEstEig's preconditioned CG and its Lanczos tridiagonal (elasticity.c:546-549) --, the
coefficients of the Chebyshev iteration itself, and the one CG whose scalars are read on the host (``pcg``: the coarse solve, the mass
solve of dynamics.py, the eigenvalue estimate over torch.distributed).  Only `ceed.py` methods are called: no mesh, no operator, any
backend of the ABI."""
from __future__ import annotations

import numpy as np


def lanczos_device(ceed, apply_A, apply_Minv, x0, r, z, p, Ap, steps, weight=None, all_reduce=False):
    """(alphas, betas) of `steps` steps of preconditioned CG from the right-hand side x0, its scalars kept on the device
    (CeedXVectorDotTo / CeedXScalarDivide / CeedXVectorAXPBYScalars): one read of the 2 * steps coefficients at the end instead of
    2 * steps + 1 host round trips.  ``apply_A(p, Ap)``, ``apply_Minv(z, r)``: operator and preconditioner; r, z, p, Ap: work vectors;
    ``weight``: every dof counts once in the dots (several ranks); ``all_reduce``: each dot is summed over the ranks where it lies.
    Slots: 0 / 3 rz of the even / odd steps, 1 pAp, 8 + 2 j alpha_j, 9 + 2 j beta_j.  The lists end before the first step that broke down."""
    sc = ceed.scalars
    sc.set_value(0.0)
    r.axpby(1.0, x0, 0.0)
    apply_Minv(z, r)
    p.axpby(1.0, z, 0.0)

    def dot_to(a, b, slot):
        a.dot_to(b, sc, slot, weight)
        if all_reduce:               # summed over the ranks where it lies: the scalar never leaves the device
            ceed.all_reduce(sc, slot, 1)
    dot_to(r, z, 0)
    for j in range(steps):
        (rz, rz_new), ja, jb = ((0, 3) if j % 2 == 0 else (3, 0)), 8 + 2 * j, 9 + 2 * j
        apply_A(p, Ap)
        dot_to(p, Ap, 1)
        ceed.scalar_divide(sc, ja, rz, 1)                    # alpha_j = rz / pAp (0 on breakdown)
        r.axpby_scalars(sc, ja, -1.0, Ap, -1, 1.0)           # r -= alpha Ap
        apply_Minv(z, r)
        dot_to(r, z, rz_new)
        ceed.scalar_divide(sc, jb, rz_new, rz)               # beta_j = rz_new / rz
        p.axpby_scalars(sc, -1, 1.0, z, jb, 1.0)             # p = z + beta p
    v = sc.to_numpy()
    alphas, betas = v[8:8 + 2 * steps:2], v[9:9 + 2 * steps:2]
    good = (alphas > 0.0) & np.isfinite(betas)
    k = steps if good.all() else int(np.argmin(good))
    return alphas[:k].tolist(), betas[:k].tolist()


def pcg(apply_A, apply_Minv, dot, b, x, r, z, d, t, rtol, maxit):
    """Preconditioned CG with its scalars on the host: x = A^-1 b from x = 0 until r . z <= rtol^2 (r . z)_0 or ``maxit`` steps.
    ``apply_A(d, t)``, ``apply_Minv(z, r)``, ``dot(u, v) -> float``; r, z, d, t: work vectors.  Returns (steps made, alphas, betas).
    ``x=None``: no iterate is formed -- with rtol = 0 the coefficients of ``maxit`` steps from the right-hand side b, which
    ``lanczos_emax`` takes (``lanczos_device`` is the same recurrence with the scalars left on the device).  A step whose r . z or
    d . A d is not positive (breakdown, an indefinite operator, a NaN) ends the iteration before anything is divided by it."""
    if x is not None:
        x.set_value(0.0)
    r.axpby(1.0, b, 0.0)
    apply_Minv(z, r)
    d.axpby(1.0, z, 0.0)
    rz = rz0 = dot(r, z)
    alphas, betas = [], []
    for _ in range(maxit):
        if not rz > 0.0:
            break
        apply_A(d, t)
        pAp = dot(d, t)
        if not pAp > 0.0:
            break
        alpha = rz / pAp
        if x is not None:
            x.axpby(alpha, d, 1.0)
        r.axpby(-alpha, t, 1.0)
        apply_Minv(z, r)
        rz_new = dot(r, z)
        alphas.append(alpha); betas.append(rz_new / rz)
        if rz_new <= rtol ** 2 * rz0:
            break
        d.axpby(1.0, z, rz_new / rz)
        rz = rz_new
    return len(alphas), alphas, betas


def lanczos_emax(alphas, betas) -> float:
    """Largest eigenvalue of the Lanczos tridiagonal of the CG coefficients: the estimate of lambda_max(M^-1 A).  1.0 without any."""
    k = len(alphas)
    if not k:
        return 1.0
    T = np.zeros((k, k))
    for j in range(k):
        T[j, j] = 1.0 / alphas[j] + (betas[j - 1] / alphas[j - 1] if j else 0.0)
        if j + 1 < k:
            T[j, j + 1] = T[j + 1, j] = np.sqrt(max(betas[j], 0.0)) / alphas[j]
    return float(np.linalg.eigvalsh(T).max())


def chebyshev_coefficients_on(lmin, lmax, its):
    """(c1, c2) of every step of a Chebyshev iteration on [lmin, lmax]: d = c1 M^-1 r + c2 d; x += d (the first: c2 = 0).
    The coefficients are shared, the steps that take them are two and stay two: the solver's levels recompute the residual from
    the iterate in every step (ChebyshevStep, fused behind the apply or in two passes, or the block step), the aggregation levels
    carry it by recurrence (ChebyshevStart / ChebyshevUpdate).  They differ in bits and in bytes moved."""
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma = theta / delta
    rho = 1.0 / sigma
    yield 1.0 / theta, 0.0
    for _ in range(1, its):
        rho_new = 1.0 / (2.0 * sigma - rho)
        yield 2.0 * rho_new / delta, rho_new * rho
        rho = rho_new


def chebyshev_coefficients(emax, lmin_frac, its):
    """The same on [lmin_frac, 1.1] x emax (KSPChebyshevEstEigSet(0, lmin_frac, 0, 1.1))."""
    return chebyshev_coefficients_on(lmin_frac * emax, 1.1 * emax, its)
