"""Component-wise Dirichlet masks on the CPU: the masks themselves, and the reference tests/test_component_masks_gpu.py
leans on.

The masks: `_component_masks.component_mask` gives every class of nodes -- (number of elements holding the node, element-interior or
not) -- all eight patterns of masked components on every level of every case; the coverage is asserted here for every ladder the two
files use.

The reference: the CPU oracle under these masks against a dense form that contains NO mask code.  The matrices of the oracle's UNMASKED
operators (all-zero masks) are taken column by column from unit vectors, multiplied by the 0/1 diagonals in NumPy, and held against
the oracle's masked operators on random vectors: the Jacobian in modes 1, 2 and 3, the diagonal, the point-block diagonal (portable
form), prolong and restrict with independent masks on their two sides, the mode-2 residual, and MassOperator in mask_mode 2 and 3.
Degrees 1 and 2 of the 3 x 3 x 3 distorted box, hyperFS and linElas.

Bound: 1e-13 relative (the project's bound between two forms of one operator): the oracle sums element by element, NumPy's A @ x sums
at most 1029 products of a row in another order; nothing else differs.  Masked rows are exactly zero.  (The host index builders under
the same patterns: tests/test_index_maps.py.)"""
import numpy as np
import pytest

import _component_masks as cm
from ceedpetscsolid_amd.mass import MassOperator
from ceedpetscsolid_amd.mesh import build_dofmap, hollow_cylinder_mesh
from ceedpetscsolid_amd.solid import level_degrees
from conftest import rel_err

TOL = 1e-13
CASES = [(phys, deg) for phys in ("hyperFS", "linElas") for deg in (1, 2)]
GPU_LADDERS = sorted({d for deg in (1, 2, 3, 4, 6) for d in level_degrees(deg)})     # every degree a level of either file has


@pytest.mark.parametrize("degree", GPU_LADDERS)
def test_every_class_of_the_box_holds_all_eight_patterns(degree):
    dm = build_dofmap(cm.MESH(), degree)
    classes = cm.node_classes(dm)
    assert (8, False) in classes and classes[(8, False)].size == 8            # the interior vertices: exactly eight
    assert ((1, True) in classes) == (degree >= 2)
    assert all(nodes.size >= 8 for nodes in classes.values()), {k: v.size for k, v in classes.items()}
    for shift in (0, 1, 4, 7):
        cov = cm.coverage(dm, cm.component_mask(dm, shift))
        assert set(cov) == set(classes) and all(got == list(range(8)) for got in cov.values()), (degree, shift, cov)
    a, b = cm.component_mask(dm, 1), cm.component_mask(dm, 4)
    assert np.all((a.reshape(-1, 3) != b.reshape(-1, 3)).any(axis=1))          # another shift: another pattern on EVERY node


def test_a_mesh_that_cannot_hold_the_patterns_is_refused():
    from ceedpetscsolid_amd.mesh import box_mesh
    with pytest.raises(AssertionError, match="not to be used"):
        cm.component_mask(build_dofmap(box_mesh(2, 2, 2), 2), 0)                # one interior vertex


def test_classes_of_the_cylinder_of_the_geometry_case():
    """hollow_cylinder_mesh(2, 8, 3), the mesh of the GPU file's geometry-form-3 case: 16 nodes held by eight elements (the wall's mid
    surface, away from the two ends), no class below eight nodes on either level of degree 2 -- the condition holds there unshortened."""
    for degree, want in ((1, {(2, False): 32, (4, False): 48, (8, False): 16}),
                         (2, {(1, False): 112, (1, True): 48, (2, False): 264, (4, False): 120, (8, False): 16})):
        dm = build_dofmap(hollow_cylinder_mesh(2, 8, 3), degree)
        assert {k: v.size for k, v in cm.node_classes(dm).items()} == want
        assert all(got == list(range(8)) for got in cm.coverage(dm, cm.component_mask(dm, 2 + degree)).values())


# ------------------------------------------------------------------------------------------------------------------------------
# the oracle under component masks against dense forms of its unmasked operators
# ------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, oracle, physics, degree):
        self.c = oracle
        mesh = cm.MESH()
        self.pu, self.pm = cm.unmasked(oracle, mesh, degree, physics), cm.unmasked(oracle, mesh, degree, physics)
        self.masks = cm.install(self.pm)
        n = self.pu.lsize()
        self.u = self.pu.smooth_state(0.1)
        self.res = []
        for p in (self.pu, self.pm):                                             # stores the state the Jacobians read
            X, Y = oracle.vector(n).set_array(self.u), oracle.vector(n).set_value(-3.0)
            p.form_residual(X, Y)
            self.res.append(Y.to_numpy())
            X.destroy(); Y.destroy()
        self.A = [cm.dense(oracle, lambda x, y, k=k: self.pu.apply_jacobian(k, x, y), self.pu.lsize(k), self.pu.lsize(k)) for k in range(len(self.pu.levels))]
        self.rng = np.random.default_rng(5)

    def run(self, apply, x, n_out, preset=-3.0):
        X, Y = self.c.vector(x.size).set_array(x), self.c.vector(n_out).set_value(preset)
        apply(X, Y)
        y = Y.to_numpy()
        X.destroy(); Y.destroy()
        return y

    def destroy(self):
        self.pu.destroy(); self.pm.destroy()


@pytest.fixture(scope="module", params=CASES, ids=[f"{p}-p{d}" for p, d in CASES])
def case(request, oracle):
    k = Case(oracle, *request.param)
    yield k
    k.destroy()


def held(what, got, want, mask_out=None):
    err = rel_err(got, want)
    print(f"  {what}: {err:.2e}")
    assert np.linalg.norm(want) > 0 and err <= TOL, (what, err)
    if mask_out is not None:
        assert np.all(got[mask_out != 0] == 0.0), what


def test_oracle_jacobian_in_modes_1_2_3(case):
    for k, lv in enumerate(case.pm.levels):
        m, x = case.masks[k], case.rng.uniform(-1, 1, case.pm.lsize(k))
        for mode in (1, 2, 3):
            lv.opJacob.set_dirichlet_mask_mode(m, None, mode)
            y = case.run(lambda X, Y: case.pm.apply_jacobian(k, X, Y), x, x.size)
            held(f"level {k} mode {mode}", y, cm.masked_matrix(case.A[k], m, m, mode) @ x, m if mode & 2 else None)
            if not mode & 2:
                assert np.all(y[m != 0] != 0.0)
        lv.opJacob.set_dirichlet_mask_mode(m, None, 3)                           # back to the mode `install` set


def test_oracle_residual_in_mode_2(case):
    m = case.masks[-1]
    assert np.all(case.res[0] != 0.0)
    assert np.array_equal(case.res[1], cm.keep(m, case.res[0]))                  # rows dropped, the input read as it is: a select of the same numbers


def test_oracle_diagonal_and_point_blocks(case):
    for k in range(len(case.pm.levels)):
        m, n = case.masks[k], case.pm.lsize(k)
        D = case.c.vector(n).set_value(-3.0)
        case.pm.get_diag(k, D)
        held(f"diagonal level {k}", D.to_numpy(), cm.keep(m, np.diag(case.A[k])), m)
        B = case.c.vector(3 * n).set_value(-3.0)
        case.pm.get_pointblock_diag(k, B)
        got, want = B.to_numpy(), cm.blocks_of(case.A[k], m)
        held(f"point blocks level {k}", got, want)
        assert np.all(got[want == 0.0] == 0.0)                                   # dropped rows and columns: exactly zero
        D.destroy(); B.destroy()


def test_oracle_transfers_with_independent_masks(case):
    p = case.pm
    assert len(p.levels) == len(level_degrees(p.levels[-1].degree))             # degree 1 is a single level: nothing below
    for k in range(1, len(p.levels)):
        nf, nc, mf, mc = p.lsize(k), p.lsize(k - 1), case.masks[k], case.masks[k - 1]
        Pm = cm.dense(case.c, lambda x, y: case.pu.prolong(k, x, y), nc, nf)
        Rm = cm.dense(case.c, lambda x, y: case.pu.restrict(k, x, y), nf, nc)
        xc, xf = case.rng.uniform(-1, 1, nc), case.rng.uniform(-1, 1, nf)
        held(f"prolong to level {k}", case.run(lambda X, Y: p.prolong(k, X, Y), xc, nf), cm.masked_matrix(Pm, mc, mf) @ xc, mf)
        held(f"restrict from level {k}", case.run(lambda X, Y: p.restrict(k, X, Y), xf, nc), cm.masked_matrix(Rm, mf, mc) @ xf, mc)
        y0 = case.rng.uniform(-1, 1, nf)
        X, Y = case.c.vector(nc).set_array(xc), case.c.vector(nf).set_array(y0)
        p.prolong_add(k, X, Y)
        ya = Y.to_numpy()
        held(f"prolong_add to level {k}", ya, y0 + cm.masked_matrix(Pm, mc, mf) @ xc)
        assert np.array_equal(ya[mf != 0], y0[mf != 0])
        X.destroy(); Y.destroy()


@pytest.mark.parametrize("mask_mode", [2, 3])
def test_oracle_mass_operator(case, mask_mode):
    for k in range(len(case.pm.levels)):
        m, n = case.masks[k], case.pm.lsize(k)
        mu, mm = MassOperator(case.pu, k, 1.5), MassOperator(case.pm, k, 1.5, mask_mode=mask_mode)
        assert mu.mask is None or not mu.mask.any()
        M = cm.dense(case.c, mu.apply, n, n)
        x, y0 = case.rng.uniform(-1, 1, n), case.rng.uniform(-1, 1, n)
        Mm = cm.masked_matrix(M, m, m, mask_mode)
        held(f"mass level {k}", case.run(mm.apply, x, n), Mm @ x, m)
        X, Y = case.c.vector(n).set_array(x), case.c.vector(n).set_array(y0)
        mm.apply_add(X, Y)
        ya = Y.to_numpy()
        held(f"mass apply_add level {k}", ya, y0 + Mm @ x)
        assert np.array_equal(ya[m != 0], y0[m != 0])
        D = case.c.vector(n).set_value(-3.0)
        mm.diagonal(D)
        held(f"mass diagonal level {k}", D.to_numpy(), cm.keep(m, np.diag(M)), m)
        mm.lumped(D)
        held(f"lumped mass level {k}", D.to_numpy(), cm.keep(m, M @ np.ones(n)), m)
        X.destroy(); Y.destroy(); D.destroy()
        mu.destroy(); mm.destroy()
