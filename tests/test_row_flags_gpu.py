"""The Dirichlet row flags of the fused apply: ONE cache per operator, keyed by the row map the apply sums -- the
restriction's shell map, its whole map, a pipelined re-ordering, the operator's own split map.  In every form the flags follow the mask
when it is set again, no form makes them while a graph is recorded, and a (P, Q, QFunction) without a kernel is refused by the dispatch
with the message written for it, whatever the form.

Shape: the jittered 2 x 2 x 2 box of test_object_lifetime_gpu.py, hyperFS at degree 2 -- P = Q = 3 gives one element-interior node per
element (the shell map exists), eight elements at four per group are two groups (two pipeline segments exist).  Mask A clamps the side
z-, mask B the side z+: each constrains nodes the other leaves free, so flags left over from the other mask show on both sides."""
import numpy as np
import pytest

from _ceed_env import ceed_with_env
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mesh import box_mesh, dirichlet_mask, side_set_nodes
from ceedpetscsolid_amd.solid import SolidProblem
from conftest import rel_err
from test_object_lifetime_gpu import two_level_problem

pytestmark = pytest.mark.gpu

NLEAD = 4
# form -> (environment of its Ceed, segments launch_info must report or None)
FORMS = {
    "shell map": ({}, 1),
    "whole restriction map": ({"CEED_MI355X_DIRECT": "0"}, None),
    "pipelined": ({"CEED_MI355X_PIPE_MIN_ROUNDS": "0", "CEED_MI355X_PIPE_SEGMENTS": "2"}, 2),
    "split map": ({}, None),
}


class Form:
    """opJacob of the fine level on a Ceed of the form's own, applied the form's way: X -> Y"""

    def __init__(self, product_lib, form):
        env, self.segments = FORMS[form]
        self.ceed = ceed_with_env(product_lib, env)
        self.p = two_level_problem(self.ceed)
        lv = self.p.levels[self.p.fine]
        self.op, n = lv.opJacob, self.p.lsize()
        self.X, self.Y = self.ceed.vector(n).set_array(np.random.default_rng(21).uniform(-1, 1, n)), self.ceed.vector(n)
        self.split = form == "split map"
        if self.split:                                   # as the lifetime test: the nodes only the leading elements touch come first
            touched_by_rest = np.zeros(lv.dofmap.nnodes, dtype=bool)
            touched_by_rest[lv.dofmap.elem_nodes[NLEAD:].ravel()] = True
            prio = np.repeat((~touched_by_rest).astype(np.uint8), 3)
            assert prio.any() and not prio.all()
            self.op.set_overlap_split(NLEAD, prio)

    def apply(self):
        if self.split:
            self.op.apply_phase(self.X, self.Y, 0)
            self.op.apply_phase(self.X, self.Y, 1)
        else:
            self.op.apply(self.X, self.Y)

    def applied(self, mask):
        self.op.set_dirichlet_mask(mask)
        self.Y.set_value(-7.0)
        self.apply()
        if self.segments is not None:
            assert self.op.launch_info()["segments"] == self.segments, self.op.launch_info()
        return self.Y.to_numpy()

    def destroy(self):
        self.X.destroy(); self.Y.destroy()
        self.p.destroy(); self.ceed.destroy()


@pytest.fixture(scope="module")
def reference(product_lib, oracle):
    """masks A and B, and under A, B and no mask the oracle's result and the default form's bits: computed once, never changed"""
    f = Form(product_lib, "shell map")
    lv = f.p.levels[f.p.fine]
    A = lv.mask.copy()
    B = dirichlet_mask(lv.dofmap, side_set_nodes(f.p.mesh, lv.dofmap, [2]))
    assert (A & ~B).any() and (B & ~A).any()
    po = two_level_problem(oracle)
    n = po.lsize()
    Xo, Yo = oracle.vector(n).set_array(f.X.to_numpy()), oracle.vector(n)
    ref = {"A": A, "B": B, "oracle": [], "default": []}
    for m in (A, B, None):
        po.levels[po.fine].opJacob.set_dirichlet_mask(m)
        po.apply_jacobian(po.fine, Xo, Yo)
        ref["oracle"].append(Yo.to_numpy())
        ref["default"].append(f.applied(m))
    for v in ref["oracle"] + ref["default"]:
        v.setflags(write=False)
    Xo.destroy(); Yo.destroy(); po.destroy(); f.destroy()
    return ref


@pytest.mark.parametrize("form", list(FORMS))
def test_row_flags_follow_the_mask_in_every_form(product_lib, reference, form):
    A, B = reference["A"] != 0, reference["B"] != 0
    f = Form(product_lib, form)
    ys = [f.applied(m) for m in (reference["A"], reference["B"], None)]      # one operator: mask A, then B, then none
    for k, y in enumerate(ys):
        err = rel_err(y, reference["oracle"][k])
        print(f"{form}, mask {'AB-'[k]}: {err:.2e} against the oracle")
        assert err < 1e-10, (form, k, err)
        assert np.array_equal(y, reference["default"][k]), (form, k)
    yA, yB, y0 = ys
    assert np.all(yA[A] == 0.0) and np.all(yB[B] == 0.0)
    assert np.all(yA[B & ~A] != 0.0)             # rows only B constrains: exactly zero after the mask was set again, not before
    assert np.all(yB[A & ~B] != 0.0)             # rows only A constrained: free again (flags left from A would zero them)
    assert np.all(y0[A | B] != 0.0)
    f.destroy()


@pytest.mark.parametrize("form", list(FORMS))
def test_no_form_makes_row_flags_while_a_graph_is_recorded(product_lib, reference, form):
    f = Form(product_lib, form)
    f.applied(reference["A"])                    # warm: maps, scratch, the flags of mask A
    f.op.set_dirichlet_mask(reference["B"])      # flags gone; the next EAGER apply makes them
    f.Y.set_value(-7.0)
    with pytest.raises(cd.CeedError, match="once before recording"):
        f.ceed.capture(f.apply)
    assert np.all(f.Y.to_numpy() == -7.0)        # refused on the host before any launch
    f.apply()                                    # the Ceed stays usable; the flags come into being
    eager = f.Y.to_numpy()
    assert np.array_equal(eager, reference["default"][1])
    g = f.ceed.capture(f.apply)
    try:
        for _ in range(2):
            f.Y.set_value(-7.0)
            g.launch()
            assert np.array_equal(f.Y.to_numpy(), eager)
    finally:
        g.destroy()
    f.destroy()


@pytest.mark.parametrize("env", [{}, {"CEED_MI355X_ASSEMBLE": "serial"}], ids=["default", "serial"])
def test_a_missing_instantiation_is_named_by_the_dispatch(product_lib, env):
    """Residual kernels exist for Q - P <= 2 only: degree 1 with qextra = 3 (P = 2, Q = 5) has none, and says so in every form."""
    ceed = ceed_with_env(product_lib, env)
    p = SolidProblem(ceed, box_mesh(2, 2, 2), 1, "hyperFS", nu=0.3, E=1.0, bc_sides=[1], multigrid="none", qextra=3)
    n = p.lsize()
    X, Y = ceed.vector(n).set_array(p.smooth_state(0.1)), ceed.vector(n)
    Y.set_value(-7.0)
    with pytest.raises(cd.CeedError, match="no fused kernel instantiated for P=2 Q=5"):
        p.form_residual(X, Y)
    assert np.all(Y.to_numpy() == -7.0)          # refused by the dispatch: nothing was launched
    X.destroy(); Y.destroy()
    p.destroy(); ceed.destroy()
