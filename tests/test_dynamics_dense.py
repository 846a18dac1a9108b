"""The Newmark solve and its tangent K + a0 rho M against dense references on the CPU oracle (tests/_newmark_dense.py; the same checks
run on the device in tests/test_dynamics_dense_gpu.py): the effective operator and the smoother's diagonal level by level, the tangent
as the derivative of the residual, eight steps against the dense recursion, and a restart on the same solver object."""
import numpy as np
import pytest

import _newmark_dense as nd


def test_solve_refined_and_recursion_on_a_known_system():
    """The helper itself: one dof, K = k, M = m, no load, released from x0 at rest -- the average-acceleration rule's exact discrete
    solution is x_n = x0 cos(n theta), theta = 2 atan(omega dt / 2)."""
    k, m, rho, dt, x0 = 3.0, 2.0, 1.5, 0.1, 0.7
    K, M = np.array([[k, 0.0], [0.0, 0.0]]), np.array([[m, 0.0], [0.0, 1.0]])
    free = np.array([True, False])
    ref = nd.newmark_reference(K, M, free, np.zeros(2), lambda l: np.zeros(2), lambda t: 1.0, np.array([x0, 9.0]), np.zeros(2), rho, dt,
                               0.25, 0.5, 25)
    theta = 2.0 * np.arctan(0.5 * np.sqrt(k / (rho * m)) * dt)
    assert max(abs(ref[n][0][0] - x0 * np.cos(n * theta)) for n in range(26)) <= 1e-13
    assert all(ref[n][0][1] == 0.0 for n in range(26))
    A = np.array([[4.0, 1.0], [1.0, 3.0]])
    assert np.abs(A @ nd.solve_refined(A, np.array([1.0, 2.0])) - [1.0, 2.0]).max() <= 1e-15


@pytest.mark.parametrize("variant", list(nd.LEVEL_VARIANTS))
def test_effective_operator_level_by_level(oracle, variant):
    figures = nd.effective_operator_check(oracle, oracle, variant, "oracle")
    assert len(figures) == 3


def test_tangent_is_the_derivative_of_the_residual(oracle):
    nd.tangent_fd_check(oracle, "oracle")


@pytest.mark.parametrize("variant", list(nd.NEWMARK_VARIANTS))
def test_newmark_against_the_dense_recursion(oracle, variant):
    nd.newmark_dense_check(oracle, oracle, variant, "oracle")


def test_restart_on_the_same_solver_gives_the_same_bits(oracle):
    nd.restart_check(oracle, "oracle")
