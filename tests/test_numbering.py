"""The yardstick of tests/test_numbering_gpu.py and its helper, on the CPU: the oracle's operators do not depend on how the caller
numbers the nodes.  Under every numbering of tests/_numbering.py the residual, the Jacobian action (overwriting and ApplyAdd), the
diagonal, prolong and restrict of every level map back to the default numbering's results BITWISE -- the oracle sums a node's
contributors in element order whatever the node is called -- and entries no element holds read 0 after an overwriting apply and are
untouched by an adding one.  A wrong ``new`` in the helper, or keys / coordinates / elements transformed apart, shows here.
The periodically wrapped numbering has no default twin: its tangent is symmetric and restrict is the transpose of prolong, at the
bounds tests/test_gpu_parity.py::_tangent_properties and ::test_full_size_transfers_and_fused_step_config4 use (1e-11, 1e-12; they
are rounding bounds of a dot product of O(1) entries, not equalities, because v'(Jw) and w'(Jv) add in different orders)."""
import numpy as np
import pytest

import _numbering as nb
from _pointblock_common import dense_jacobian
from ceedpetscsolid_amd.mesh import box_mesh, hollow_cylinder_mesh

CASES = {
    "cyl p3 fs": (lambda: hollow_cylinder_mesh(2, 6, 2), 3, "hyperFS", [998]),
    "box p2 le": (lambda: box_mesh(3, 2, 2), 2, "linElas", [1]),
}
_default = {}


def default_results(monkeypatch, oracle, case):
    """The default numbering's results, computed once per case and shared (read-only) by its numberings."""
    if case not in _default:
        mk, degree, model, bc = CASES[case]
        p = nb.problem_under(monkeypatch, nb.default, oracle, mk(), degree, model, bc)
        _default[case] = (p.smooth_state(0.1), nb.run_operators(p, p.smooth_state(0.1), pointblock=False)[0])
        p.destroy()
    return _default[case]


def test_helper_numberings_are_what_they_say():
    mesh = hollow_cylinder_mesh(2, 6, 2)
    d = nb.default(mesh, 3)
    for name, f in nb.NUMBERINGS.items():
        dm = f(mesh, 3)
        assert dm.p == 3 and dm.elem_nodes.dtype == np.int32 and dm.new.shape == (d.nnodes,)
        assert np.array_equal(dm.elem_nodes, dm.new[d.elem_nodes]), name
        assert np.array_equal(dm.node_coords[dm.new], d.node_coords) and np.array_equal(dm.node_keys[dm.new], d.node_keys), name
        assert (dm.nnodes == d.nnodes) == (name != "gaps") and np.unique(dm.new).size == d.nnodes
        v = np.random.default_rng(1).uniform(-1, 1, 3 * d.nnodes)
        assert np.array_equal(nb.to_default(nb.from_default(v, dm, 9.0), dm), v)
        assert not np.array_equal(dm.new, d.new), name                       # none of them is the default in disguise
    m = 2                                                                     # interior nodes per edge at p = 3
    cf, en = nb.cells_first(mesh, 3), nb.entity(mesh, 3)
    assert np.all(cf.node_keys[:mesh.nelem * m ** 3, 0] == 3) and np.all(cf.node_keys[-mesh.nvert:, 0] == 0)
    assert np.all(en.node_keys[:mesh.nvert, 0] == 0) and np.all(en.node_keys[-mesh.nelem * m ** 3:, 0] == 3)
    assert cf.elem_nodes[0].min() == 0 and cf.elem_nodes[0].max() >= cf.nnodes - mesh.nvert      # interiors in front, vertices behind
    g = nb.gaps(mesh, 3)
    hit = nb.referenced(g).reshape(-1, 3)[:, 0]
    assert g.nnodes == d.nnodes + (d.nnodes - 1) // 2 + 3 and not hit[0] and not hit[::3].any() and not hit[-2:].any() and hit.sum() == d.nnodes
    assert np.all(g.node_keys[~hit, 0] == -1) and not g.node_coords[~hit].any()
    r = nb.reversed_(mesh, 3)
    assert np.array_equal(r.new, d.nnodes - 1 - np.arange(d.nnodes))
    a, b = nb.permuted(7)(mesh, 3), nb.permuted(7)(mesh, 2)
    assert not np.array_equal(a.new[:b.new.size], b.new)                      # another permutation on another level


@pytest.mark.parametrize("numbering", list(nb.NUMBERINGS))
@pytest.mark.parametrize("case", list(CASES))
def test_oracle_is_invariant_under_the_numbering(monkeypatch, oracle, case, numbering):
    u_def, want = default_results(monkeypatch, oracle, case)
    mk, degree, model, bc = CASES[case]
    p = nb.problem_under(monkeypatch, nb.NUMBERINGS[numbering], oracle, mk(), degree, model, bc)
    fine = p.levels[p.fine].dofmap
    u = nb.from_default(u_def, fine, nb.UNREAD)
    assert np.array_equal(u[nb.referenced(fine)], p.smooth_state(0.1)[nb.referenced(fine)])     # coordinates moved with the nodes
    got, _ = nb.run_operators(p, u, pointblock=False)
    assert set(got) == set(want)
    for name, g in got.items():
        k, ncomp = nb.level_of(name)
        if k is None:
            assert np.array_equal(g, want[name]), name                        # q-point data: element order, not node order
            continue
        dm = p.levels[k].dofmap
        assert np.array_equal(nb.to_default(g, dm), want[name]), (name, np.abs(nb.to_default(g, dm) - want[name]).max())
        stray = g[~nb.referenced(dm, ncomp)]
        assert np.all(stray == (nb.KEPT if "_add" in name else 0.0)), name   # overwritten with 0 / left alone by ApplyAdd
    assert np.abs(got["residual"]).max() > 0
    p.destroy()


@pytest.mark.parametrize("nx,ny,nz", [(1, 2, 2), (2, 2, 2)])
def test_oracle_on_a_periodically_wrapped_numbering(monkeypatch, oracle, nx, ny, nz):
    p = nb.problem_under(monkeypatch, nb.wrapped, oracle, box_mesh(nx, ny, nz), 3, "hyperFS", [1])
    for lv in p.levels:
        en, P = lv.dofmap.elem_nodes, lv.degree + 1
        if nx == 1:
            assert np.array_equal(en[:, 0::P], en[:, P - 1::P])              # the x = 0 and x = 1 node of every line of an element: one node
            assert en[0, 0] == en[0, lv.degree]
        else:
            assert np.array_equal(en[0::2, 0::P], en[1::2, P - 1::P]) and not np.array_equal(en[:, 0::P], en[:, P - 1::P])
    nb.check_wrapped(p)
    # get_diag is libCEED's: the diagonals of the ELEMENT matrices summed over the element entries of a node.  That is the diagonal of
    # the assembled operator unless one element holds a node twice: the coupling between the two entries is then left out (measured
    # here: 42 % of the largest entry at p = 1, 6 % at p = 3).  The first bound is rounding, two sums of at most a few hundred terms
    # in different orders (measured 3e-15); the second only says that the nx = 1 case still is that situation.
    for k in range(len(p.levels)):
        A = dense_jacobian(p, k)
        D = oracle.vector(p.lsize(k)).set_value(nb.PRESET)
        p.get_diag(k, D)
        gap = np.abs(np.diag(A) - D.to_numpy()).max() / np.abs(D.to_numpy()).max()
        assert np.abs(A - A.T).max() <= 1e-13 * np.abs(A).max()
        assert gap > 1e-2 if nx == 1 else gap < 1e-13, (k, gap)
    p.destroy()
