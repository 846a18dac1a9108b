"""The Newmark solve and its tangent K + a0 rho M on the device against dense references formed on the CPU oracle
(tests/_newmark_dense.py; the same checks run on the oracle alone in tests/test_dynamics_dense.py): the effective operator of every
multigrid level (k_mass<P,Q> at P < Q on the coarse levels, the device-assembled p = 1 matrix with its mass columns, the smoother's
diagonal and its cache), the tangent as the derivative of the residual, eight steps against the dense recursion, a restart with the
recorded V-cycle, and the mass operator under caller-chosen node numberings."""
import numpy as np
import pytest

import _newmark_dense as nd
import _numbering as nb
from ceedpetscsolid_amd.mass import MassOperator

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", list(nd.LEVEL_VARIANTS))
def test_effective_operator_level_by_level(gpu, oracle, variant):
    figures = nd.effective_operator_check(gpu, oracle, variant, "device")
    assert len(figures) == 3


def test_tangent_is_the_derivative_of_the_residual(gpu):
    nd.tangent_fd_check(gpu, "device")


@pytest.mark.parametrize("variant", list(nd.NEWMARK_VARIANTS))
def test_newmark_against_the_dense_recursion(gpu, oracle, variant):
    nd.newmark_dense_check(gpu, oracle, variant, "device")


def test_restart_with_the_recorded_vcycle_gives_the_same_bits(gpu):
    nd.restart_check(gpu, "device", graph=True)


# ---- the mass operator under caller-chosen numberings ----------------------------------------------------------------------------------
COEF = 1.75
SENTINEL = -3.25
_default = {}


def _default_portable(monkeypatch, oracle, x_def):
    """The default numbering's portable results (apply on x_def, diagonal), once."""
    if not _default:
        p = nb.problem_under(monkeypatch, nb.default, oracle, nb.distorted_box(2, 2, 1), 2, "linElas", [1], qextra=1)
        ref = MassOperator(p, p.fine, COEF, portable=True)
        mask = p.levels[p.fine].mask != 0
        _default["apply"] = np.where(mask, 0.0, ref.apply_host(x_def))
        _default["diagonal"] = ref.diagonal_host()
        p.destroy()
    return _default


@pytest.mark.parametrize("numbering", ["permuted", "gaps"])
def test_mass_operator_under_the_numbering(monkeypatch, gpu, oracle, numbering):
    """mass<3,4> and mass_diag<3,4> on distorted_box(2, 2, 1), p = 2, qextra = 1, side 1 clamped, under a numbering: against the
    portable form of the oracle's problem under the SAME numbering, and, carried to the default numbering, against the default
    numbering's portable form, both within 1e-10 of max |want|.  Entries of nodes no element holds: untouched by apply_add, zero after
    the overwriting apply and in the diagonal (as the portable form and the Jacobian operators leave them)."""
    mesh = nb.distorted_box(2, 2, 1)
    p = nb.problem_under(monkeypatch, nb.NUMBERINGS[numbering], gpu, mesh, 2, "linElas", [1], qextra=1)
    po = nb.problem_under(monkeypatch, nb.NUMBERINGS[numbering], oracle, mesh, 2, "linElas", [1], qextra=1)
    dm = p.levels[p.fine].dofmap
    n = p.lsize()
    mask = p.levels[p.fine].mask != 0
    held = nb.referenced(dm)
    assert held.all() == (numbering != "gaps") and mask.any() and (p.levels[p.fine].degree + 1, p.levels[p.fine].Q) == (3, 4)
    rng = np.random.default_rng(77)
    x_def, y_def = rng.uniform(-1, 1, 3 * dm.new.size), rng.uniform(-1, 1, 3 * dm.new.size)
    x, y0 = nb.from_default(x_def, dm, nb.UNREAD), nb.from_default(y_def, dm, SENTINEL)
    dev, ref = MassOperator(p, p.fine, COEF), MassOperator(po, po.fine, COEF, portable=True)
    assert not dev.portable and ref.portable
    want = np.where(mask | ~held, 0.0, ref.apply_host(np.where(held, x, 0.0)))
    want_d = ref.diagonal_host()
    X, Y = gpu.vector(n).set_array(x), gpu.vector(n).set_value(SENTINEL)
    dev.apply(X, Y)
    assert dev.kernel_name == "mass<3,4>"
    y = Y.to_numpy()
    Y.set_array(y0)
    dev.apply_add(X, Y)
    ya = Y.to_numpy()
    D = gpu.vector(n).set_value(SENTINEL)
    dev.diagonal(D)
    assert dev.kernel_name == "mass_diag<3,4>"
    d = D.to_numpy()
    e = dict(apply=nd.relmax(y, want), apply_add=float(np.abs(ya - (y0 + want)).max() / np.abs(want).max()), diagonal=nd.relmax(d, want_d))
    base = _default_portable(monkeypatch, oracle, x_def)
    e["apply, default"] = nd.relmax(nb.to_default(y, dm), base["apply"])
    e["apply_add, default"] = float(np.abs(nb.to_default(ya, dm) - (y_def + base["apply"])).max() / np.abs(base["apply"]).max())
    e["diagonal, default"] = nd.relmax(nb.to_default(d, dm), base["diagonal"])
    print(f"DENSE item 6 device {numbering}: " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert all(v <= nd.TOL for v in e.values()), e
    assert np.array_equal(ya[~held], y0[~held]) and np.all(ya[~held] == SENTINEL)          # the sentinel's bits
    assert np.array_equal(ya[mask], y0[mask])                                             # masked rows are left alone by the add
    assert not y[~held].any() and not y[mask].any() and not d[~held].any() and not d[mask].any()
    assert np.all(d[held & ~mask] > 0.0) and np.abs(want).max() > 0
    for v in (X, Y, D):
        v.destroy()
    dev.destroy(); p.destroy(); po.destroy()
