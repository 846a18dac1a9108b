"""Modal analysis (modal.Eigenmodes) on the device: the three problems of _modal_common.py against the dense pencil formed on the
device, within the bounds stated there; the device eigenvalues against the CPU oracle's within the sum of both bounds; the prestressed
modes; the V-cycle replayed from its recorded graph; and the block operations really are the library's."""
import numpy as np
import pytest

import _modal_common as mc
from ceedpetscsolid_amd import ceed as cd

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", mc.CASES)
def test_modes_match_the_dense_pencil_and_the_oracle(gpu, oracle, name, monkeypatch):
    assert gpu.L.has("CeedXVectorBlockGram") and gpu.L.has("CeedXVectorBlockCombine")
    # the portable forms are never taken on the device
    monkeypatch.setattr(cd, "block_gram_host", lambda *a, **k: pytest.fail("portable Gram matrix on the device"))
    monkeypatch.setattr(cd, "block_combine_host", lambda *a, **k: pytest.fail("portable combination on the device"))
    prob, sol, nmodes, guard, nrigid = mc.make_case(gpu, name)
    res, calls = mc.run(sol, nmodes, guard)
    assert res.modes.on_device
    assert calls["gram"] >= 2 * res.iterations and calls["combine"] >= 3 * res.iterations
    K, M, free, lam, Phi = mc.dense_reference(gpu, prob)
    bounds, _ = mc.check_result(res, K, M, free, lam, Phi, nmodes, nrigid, name + " (device)")
    res2, _ = mc.run(sol, nmodes, guard, seed=7)
    mc.check_result(res2, K, M, free, lam, Phi, nmodes, nrigid, name + " (device, seed 7)")
    monkeypatch.undo()
    prob_o, sol_o, _, _, _ = mc.make_case(oracle, name)
    res_o, _ = mc.run(sol_o, nmodes, guard)
    Ko, Mo, free_o, lam_o, Phi_o = mc.dense_reference(oracle, prob_o)
    bounds_o, _ = mc.check_result(res_o, Ko, Mo, free_o, lam_o, Phi_o, nmodes, nrigid, name + " (oracle)")
    diff = np.abs(res.eigenvalues - res_o.eigenvalues)
    print(f"{name}: |lambda device - lambda oracle| = {diff}, bounds {bounds + bounds_o}")
    assert np.all(diff <= bounds + bounds_o)
    mc.teardown(prob, sol); mc.teardown(prob_o, sol_o)


def test_prestressed_modes_with_the_recorded_vcycle(gpu):
    name = "clamped_p3_hyperfs_amg"
    prob, sol, nmodes, guard, _ = mc.make_case(gpu, name)
    lam0 = mc.run(sol, nmodes, guard)[0].eigenvalues
    mc.teardown(prob, sol)
    prob, sol, nmodes, guard, _ = mc.make_case(gpu, name, tip_fz=mc.TIP_FZ, graph=True)
    assert sol.solve(num_increments=2).converged
    tip = np.abs(sol.U.to_numpy()).max()
    assert 0.01 * 3.0 <= tip <= 0.1 * 3.0
    res, _ = mc.run(sol, nmodes, guard)
    assert sol._pc_graph is not None                      # the V-cycle was replayed from its recording
    K, M, free, lam, Phi = mc.dense_reference(gpu, prob)
    mc.check_result(res, K, M, free, lam, Phi, nmodes, 0, name + " prestressed (device, recorded V-cycle)")
    print(f"lambda_1 unstressed {lam0[0]:.12e}, prestressed {res.eigenvalues[0]:.12e}")
    assert abs(res.eigenvalues[0] - lam0[0]) > 1e-6 * lam0[0]
    mc.teardown(prob, sol)                                # (the recording still alive goes with the solver)
