"""Whole Newmark solves (dynamics.NewmarkPMG) on the device, small: the exact discrete solution on an eigenvector, the dynamic residual
identity of a finite-strain run eager and with the recorded V-cycle, and the device against the CPU oracle."""
import numpy as np
import pytest

from _mass_common import eigenvector_run, hyperfs_run
from ceedpetscsolid_amd.mesh import box_mesh

pytestmark = pytest.mark.gpu

STEPS = 5


def test_newmark_reproduces_the_exact_discrete_solution(gpu):
    worst_u, worst_e, bound, theta, theta_meas = eigenvector_run(gpu)
    print(f"eigenvector run (device): worst |u_n - phi cos(n theta)| / |phi| = {worst_u:.3e}, worst energy drift {worst_e:.3e}, "
          f"bound {bound:.3e}; theta exact {theta:.12f}, measured {theta_meas:.12f}")
    assert worst_u <= bound
    assert worst_e <= bound


@pytest.fixture(scope="module")
def eager(gpu):
    sol, prob, out, stats = hyperfs_run(gpu, box_mesh(2, 2, 2), STEPS, coarse="amg")
    return sol.U.to_numpy().copy(), out, stats, sol.mass[prob.fine].kernel_name


def test_hyperfs_dynamic_residual_identity(eager):
    U, out, stats, kname = eager
    assert kname == "mass<3,3>"
    for k, (rec, last) in enumerate(out):
        print(f"step {k + 1}: recomputed |F_int + rho M a - load f| = {rec:.3e}, last Newton |R| = {last:.3e}, "
              f"{stats[k].newton_its} Newton / {stats[k].ksp_its} Krylov its")
        assert rec <= 10 * last
    assert np.abs(U).max() > 1e-3


def test_recorded_vcycle_gives_the_eager_bits(gpu, eager):
    U, out, stats, _ = eager
    sol, prob, out_g, stats_g = hyperfs_run(gpu, box_mesh(2, 2, 2), STEPS, coarse="amg", graph=True)
    for (rec, last) in out_g:
        assert rec <= 10 * last
    assert [(s.newton_its, s.ksp_its) for s in stats_g] == [(s.newton_its, s.ksp_its) for s in stats]
    assert np.array_equal(sol.U.to_numpy(), U)


def test_device_against_oracle(oracle, eager):
    U, _, stats, _ = eager
    sol, prob, out, stats_c = hyperfs_run(oracle, box_mesh(2, 2, 2), STEPS, coarse="amg")
    Uc = sol.U.to_numpy()
    err = np.linalg.norm(U - Uc) / np.linalg.norm(Uc)
    print(f"device against oracle after {STEPS} steps: |U_dev - U_cpu| / |U_cpu| = {err:.3e}; Newton its device "
          f"{[s.newton_its for s in stats]} oracle {[s.newton_its for s in stats_c]}")
    assert err <= 1e-6
