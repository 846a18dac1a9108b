"""The lifetime rule of DESIGN.md 3 on the device: every device array a library object owns is a DevArray (csrc/dev_array.hpp), so an
object destroyed -- or its derived state set again -- while a recorded hipGraph is alive leaves the arrays the graph's kernel nodes point
at in place until the last graph goes.  Each case records launches, replays, destroys or re-sets what the launches read, and replays
again: the same bits, which are the eager result's.

Between the destruction and the second replay, vectors of zeros are created and written: memory the allocator had got back would be handed
out again and overwritten with offsets and row pointers that are all zero (in bounds, and plainly wrong), so a freed array shows as a failed
comparison.

The mask set again under a live graph is asserted by test_operator_plan_gpu.py::test_a_recorded_apply_replays_after_its_mask_was_set_again;
the overlap split set again is the third case here.

Shapes: a jittered 2 x 2 x 2 box (general hexes: the geometry-provenance arrays exist), hyperFS at degree 2 (P = Q = 3: one element-interior
node, so the shell map and the interior list exist) under degree 1, one clamped side (flagged offsets and row flags exist)."""
import numpy as np
import pytest

from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem
from test_amg import random_pieces

pytestmark = pytest.mark.gpu


@pytest.fixture
def ceed(product_lib):
    """a Ceed of the test's own: the last step of each case is its destruction"""
    c = cd.Ceed(product_lib, "/gpu/hip/mi355x")
    yield c
    c.destroy()


def two_level_problem(ceed):
    mesh = box_mesh(2, 2, 2)
    mesh.coords[:] += np.random.default_rng(5).uniform(-0.04, 0.04, mesh.coords.shape)
    p = SolidProblem(ceed, mesh, 2, "hyperFS", nu=0.3, E=1.0, bc_sides=[1], multigrid="uniform")
    assert [lv.degree for lv in p.levels] == [1, 2] and any(lv.mask.any() for lv in p.levels)
    n = p.lsize()
    X, R = ceed.vector(n).set_array(p.smooth_state(0.1)), ceed.vector(n)
    p.form_residual(X, R)                       # stores grad u (and the tangent's derived state beside it)
    X.destroy(); R.destroy()
    return p


def overwrite_what_was_freed(ceed, sizes):
    """vectors of zeros, of the sizes the retired arrays had and a few more: whatever the allocator got back is handed out and zeroed"""
    vs = [ceed.vector(n) for n in sizes for _ in range(3)]
    for v in vs:
        v.set_value(0.0)                         # (allocated and zeroed on the device)
    ceed.synchronize()
    return vs


def replay(graph, outs):
    for v in outs:
        v.set_value(-7.0)
    graph.launch()
    return [v.to_numpy() for v in outs]


def test_operators_and_restrictions_destroyed_under_a_live_graph(ceed):
    p = two_level_problem(ceed)
    co, fi = p.levels[0], p.levels[1]
    nc, nf = p.lsize(0), p.lsize(1)
    rng = np.random.default_rng(11)
    Xf, Xc = ceed.vector(nf).set_array(rng.uniform(-1, 1, nf)), ceed.vector(nc).set_array(rng.uniform(-1, 1, nc))
    Yj, Yr, Yp, D = ceed.vector(nf), ceed.vector(nc), ceed.vector(nf), ceed.vector(nf)
    outs = [Yj, Yr, Yp, D]

    def work():
        p.apply_jacobian(p.fine, Xf, Yj)
        p.restrict(p.fine, Xf, Yr)
        p.prolong(p.fine, Xc, Yp)
        p.get_diag(p.fine, D)

    work()
    assert "dXdx recomputed per point" in fi.opJacob.kernel_name      # general hexes: the launch read the provenance arrays
    eager = [v.to_numpy() for v in outs]
    assert all(np.any(e != 0.0) for e in eager)
    graph = ceed.capture(work)
    try:
        first = replay(graph, outs)
        for a, e in zip(first, eager):
            assert np.array_equal(a, e)
        # everything the recorded launches read beside the vectors goes: operators, QFunctions, restrictions of both levels (the residual
        # operator too, the last holder of the fine restriction) -- not the vectors, not qdata, not gradu
        for lv in (fi, co):
            for op in (lv.opJacob, lv.opProlong, lv.opRestrict):
                if op is not None:
                    op.destroy(); op.qf.destroy()
            lv.Erestrictu.destroy()
        p.opApply.destroy(); p.qfApply.destroy()
        scratch = overwrite_what_was_freed(ceed, [8 * 27, 8 * 8, 8 * 19, nf // 3 + 1, nf, 64])
        again = replay(graph, outs)
        for a, b, e in zip(again, first, eager):
            assert np.array_equal(a, b) and np.array_equal(a, e)
    finally:
        graph.destroy()
    for v in scratch + outs + [Xf, Xc]:
        v.destroy()
    p.destroy()                                  # (what is left of it: the wrappers of the destroyed objects hold null handles)


def test_a_matrix_destroyed_under_a_live_graph(ceed):
    rng, A, P, Pt, a = random_pieces(ceed)
    n = A.shape[0]
    assert n == 57
    a.assemble(ceed.vector(A.nnz).set_array(A.data))
    x = rng.standard_normal(n)
    X, Y = ceed.vector(n).set_array(x), ceed.vector(n)
    a.apply(X, Y)
    eager = Y.to_numpy()
    assert np.abs(eager - A @ x).max() < 1e-13 * np.abs(A @ x).max()
    graph = ceed.capture(lambda: a.apply(X, Y))
    try:
        first, = replay(graph, [Y])
        assert np.array_equal(first, eager)
        a.destroy()
        scratch = overwrite_what_was_freed(ceed, [n + 1, A.nnz, A.nnz // 2 + 1, 8])
        again, = replay(graph, [Y])
        assert np.array_equal(again, eager)
    finally:
        graph.destroy()
    for v in scratch + [X, Y]:
        v.destroy()


def test_a_recorded_split_phase_apply_replays_after_the_split_was_set_again(ceed):
    p = two_level_problem(ceed)
    lv = p.levels[p.fine]
    n = p.lsize()
    nlead = 4
    touched_by_rest = np.zeros(lv.dofmap.nnodes, dtype=bool)
    touched_by_rest[lv.dofmap.elem_nodes[nlead:].ravel()] = True
    prio = np.repeat((~touched_by_rest).astype(np.uint8), 3)
    assert prio.any() and not prio.all()
    X, Y, W = ceed.vector(n).set_array(np.random.default_rng(12).uniform(-1, 1, n)), ceed.vector(n), ceed.vector(n)
    op = lv.opJacob
    op.apply(X, W)
    whole = W.to_numpy()

    def work():
        op.apply_phase(X, Y, 0)
        op.apply_phase(X, Y, 1)

    op.set_overlap_split(nlead, prio)
    work()
    assert np.array_equal(Y.to_numpy(), whole)
    graph = ceed.capture(work)
    try:
        first, = replay(graph, [Y])
        assert np.array_equal(first, whole)
        op.set_overlap_split(nlead, prio)       # a new split map; its row flags follow at the next eager apply
        scratch = overwrite_what_was_freed(ceed, [8 * 19, lv.dofmap.nnodes + 1, lv.dofmap.nnodes, 64])
        again, = replay(graph, [Y])
        assert np.array_equal(again, whole)
        work()                                  # the new flags come into being
        assert np.array_equal(Y.to_numpy(), whole)
        again, = replay(graph, [Y])
        assert np.array_equal(again, whole)
    finally:
        graph.destroy()
    for v in scratch + [X, Y, W]:
        v.destroy()
    p.destroy()
