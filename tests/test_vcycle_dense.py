"""The p-multigrid V-cycle of solver.NewtonPMG and the flexible PCG around it against dense references on the CPU oracle
(tests/_vcycle_dense.py; the same checks run on the device in tests/test_vcycle_dense_gpu.py): the V-cycle as ONE matrix against its
closed form, its symmetry and definiteness, the eigenvalue estimates of the smoothers, fcg against a dense PCG -- and the controls:
three seeded faults that leave the iteration counts (almost) alone and that the comparison must miss by orders of magnitude."""
import numpy as np
import pytest
import scipy.linalg

import _vcycle_dense as vd


def test_the_helpers_on_known_systems():
    """The closed forms themselves.  The Chebyshev polynomial against its three-term recurrence on both sides of |t| = 1; the
    smoother's factors against the Chebyshev ITERATION written out in NumPy (coefficients derived here from the recurrence of
    T_k, not taken from the project); the two-sided form against a V-cycle run step by step; the dense PCG against a solve."""
    rng = np.random.default_rng(5)
    n, k = 12, 3
    G = rng.uniform(-1, 1, (n, n))
    A = G @ G.T + 0.5 * np.eye(n)
    M = np.diag(np.diag(A))
    top = float(scipy.linalg.eigh(A, M, eigvals_only=True).max())
    lmin, lmax = 0.15 * top, 0.8 * top                               # the top of the spectrum of M^-1 A lies OUTSIDE the interval
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    lam = np.linspace(0.01 * top, 1.2 * top, 41)

    def T(t, k):
        a, b = np.ones_like(t), t
        for _ in range(k - 1):
            a, b = b, 2.0 * t * b - a
        return b if k else a
    for kk in (1, 2, 3, 4, 7):
        want = T((theta - lam) / delta, kk) / T(np.array(theta / delta), kk)
        assert np.abs(vd.chebyshev_polynomial(lam, lmin, lmax, kk) - want).max() <= 1e-12 * np.abs(want).max()
    E, S1, S2, _ = vd.smoother_factors(A, M, lmin, lmax, k)

    def sweep(b, x):
        """k steps of the textbook Chebyshev iteration for M^-1 A on [lmin, lmax] from x."""
        sigma = theta / delta
        rho = 1.0 / sigma
        d = np.linalg.solve(M, b - A @ x) / theta
        x = x + d
        for _ in range(k - 1):
            rho_new = 1.0 / (2.0 * sigma - rho)
            d = rho_new * rho * d + 2.0 * rho_new / delta * np.linalg.solve(M, b - A @ x)
            x = x + d
            rho = rho_new
        return x
    b, x0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    xs = np.linalg.solve(A, b)
    assert np.abs(sweep(b, np.zeros(n)) - S1 @ b).max() <= 1e-13
    assert np.abs((sweep(b, x0) - xs) - E @ (x0 - xs)).max() <= 1e-13
    P = rng.uniform(-1, 1, (n, 4))
    Bc = vd.spd_inverse(P.T @ A @ P)
    x = sweep(b, np.zeros(n))
    x = x + P @ (Bc @ (P.T @ (b - A @ x)))
    x = sweep(b, x)
    assert np.abs(x - vd.two_sided(E, S2, P, Bc) @ b).max() <= 1e-13
    assert np.linalg.eigvalsh(S2).min() < 0.0                        # |p_k| > 1 at the modes left out: such a V-cycle is indefinite
    E, _, S2, _ = vd.smoother_factors(A, M, 0.1 * top, 1.1 * top, k)  # an interval that covers the top: a definite preconditioner
    xp, its = vd.dense_pcg(A, vd.two_sided(E, S2, P, Bc), b, 1e-12)
    assert np.abs(xp - xs).max() <= 1e-11 and 1 < its < n


@pytest.mark.parametrize("degree,multigrid", [(3, "uniform"), (4, "logarithmic")])
def test_prolongation_reproduces_affine_fields(oracle, degree, multigrid):
    vd.affine_prolongation_check(oracle, degree, multigrid, "oracle")


@pytest.mark.parametrize("name", list(vd.CASES))
def test_vcycle_and_pcg_against_the_dense_references(oracle, name):
    vd.vcycle_check(oracle, oracle, name, "oracle")


@pytest.mark.parametrize("smoother", ["jacobi", "pbjacobi"])
def test_one_level_preconditioner_is_the_inverted_smoother_matrix(oracle, smoother):
    vd.one_level_check(oracle, oracle, smoother, "oracle")


def test_factors_of_the_recursion_one_by_one(oracle):
    out = vd.factors_check(oracle, oracle, "a", "oracle")
    assert len(out) == 8


def test_controls_seeded_faults_are_missed_by_the_check(oracle):
    """emax[1] x 1.05, the restricted residual x 0.98, a post-smoother one step short: each moves B by more than 1e-4 (2.5e-3, 9.2e-3
    and 5.9e-2 were measured) where the clean solver is within 1e-12, and the last one breaks the symmetry of B; the fcg counts
    printed beside them (16 -> 16, 16, 20) are what the iteration bands of the other tests would have seen."""
    out = vd.controls_check(oracle)
    assert len(out) == 3
