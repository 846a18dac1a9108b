"""The shared-node sum from the stencil code of its rows (row_code.hpp, kernel_node_sum.hpp: node_sum3_coded) against the
plain form, rowptr / cols for every row.  Both forms add every row's contributors in contributor order, one lane per row, so every result
must be the SAME BITS (np.array_equal, no tolerance) between a Ceed created under CEED_MI355X_ROWMAP=plain and a default one in the same
process: the Jacobian apply in overwrite and add mode with the Dirichlet flags on and off, the fused Chebyshev step and residual (also
against their two-pass forms), the split-phase pair under a priority mask, and the pipelined form forced to two segments.
(The XCD-local order of the row blocks was built and measured with the code and left the sources again: profiles/assemble_row_code.txt.)

Shapes: boxes 2 x 2 x 2, 3 x 3 x 3, 4 x 4 x 3 at degrees 1, 2, 4 (at degree 4: 3, 6 and 10 workgroups of 256 rows, the last one ragged); a
2 x 6 x 2 hollow cylinder (the contributors across the theta wrap lie far apart); a 3 x 3 x 3 box with elements in random order and
orientation (many stencils), also under a table limit of 4 stencils (escape rows beside coded ones in one wave)."""
import numpy as np
import pytest

from _ceed_env import ceed_with_env
from ceedpetscsolid_amd.mesh import box_mesh, hollow_cylinder_mesh, scramble_mesh
from ceedpetscsolid_amd.solid import SolidProblem

pytestmark = pytest.mark.gpu

PLAIN = {"CEED_MI355X_ROWMAP": "plain"}


def _distorted(mesh, seed=5):
    mesh.coords[:] += np.random.default_rng(seed).uniform(-0.03, 0.03, mesh.coords.shape)     # no affine / swept shortcut, no symmetric sums
    return mesh


def _problem(ceed, mesh, degree):
    p = SolidProblem(ceed, mesh, degree, "hyperFS", nu=0.3, E=1.0, bc_sides=sorted(mesh.side_sets)[:1], multigrid="none")
    n = p.lsize()
    X, R = ceed.vector(n).set_array(p.smooth_state(0.08)), ceed.vector(n)
    p.form_residual(X, R)                       # the stored state of the tangent
    X.destroy(); R.destroy()
    return p


def _results(p, seed=11, split=None):
    """name -> array of every form of the Jacobian apply that sums shared nodes, all from the same host arrays"""
    c, lv = p.ceed, p.levels[p.fine]
    op, n = lv.opJacob, p.lsize()
    rng = np.random.default_rng(seed)
    free = (lv.mask == 0).astype(np.float64)
    x, y0, b, d, r = (rng.uniform(-1, 1, n) for _ in range(5))
    dinv = rng.uniform(0.5, 2.0, n) * free
    vec = lambda a: c.vector(n).set_array(a)
    out = {}
    X = vec(x)
    for flags in ("flags", "no flags"):
        op.set_dirichlet_mask(lv.mask if flags == "flags" else None)
        Y = c.vector(n).set_value(-7.0)
        op.apply(X, Y)
        out[f"apply, {flags}"] = Y.to_numpy()
        Y = vec(y0)
        op.apply_add(X, Y)
        out[f"apply add, {flags}"] = Y.to_numpy()
        # the fused consumers and their two-pass forms: a first Chebyshev step (r = b - A x), a recurrence step (r -= A d), the residual
        for first in (True, False):
            for fused in (True, False):
                v = {k: vec(a * free) for k, a in (("x", x), ("d", d), ("r", r), ("b", b))}
                D, T = vec(dinv), c.vector(n).set_value(-3.0)
                src = v["x"] if first else v["d"]
                if fused:
                    op.apply_chebyshev(src, T, v["x"], v["d"], v["r"], v["b"] if first else None, D, 0.37, 0.0 if first else 0.21)
                else:
                    op.apply(src, T)
                    if first:
                        v["x"].chebyshev_start(v["d"], v["r"], v["b"], T, D, 0.37, False)
                    else:
                        v["x"].chebyshev_update(v["d"], v["r"], T, D, 0.37, 0.21, False)
                for k in ("x", "d", "r"):
                    out[f"chebyshev {'first' if first else 'next'} {k}, {'fused' if fused else 'two passes'}, {flags}"] = v[k].to_numpy()
        B, T, W = vec(b), c.vector(n).set_value(9.0), c.vector(n)
        op.apply_residual(X, T, B, W)
        out[f"residual, fused, {flags}"] = W.to_numpy()
        op.apply(X, T)
        W.waxpby(1.0, B, -1.0, T)
        out[f"residual, two passes, {flags}"] = W.to_numpy()
    op.set_dirichlet_mask(lv.mask)
    if split is not None:
        nlead, prio = split
        op.set_overlap_split(nlead, prio)
        Y = c.vector(n).set_value(-7.0)
        op.apply_phase(X, Y, 0)
        out["split phase 0"] = Y.to_numpy()
        op.apply_phase(X, Y, 1)
        out["split phases 0 + 1"] = Y.to_numpy()
        op.set_overlap_split(0, None)
    return out


def _priority(p, nlead):
    """the nodes only the leading elements touch, as a priority mask per L-vector entry"""
    dm = p.levels[p.fine].dofmap
    rest = np.zeros(dm.nnodes, dtype=bool)
    rest[dm.elem_nodes[nlead:].ravel()] = True
    prio = np.repeat((~rest).astype(np.uint8), 3)
    assert prio.any() and not prio.all()
    return prio


def _compare(product_lib, mk, degree, env_new=None, env_ref=PLAIN, split=True):
    ref_ceed, new_ceed = ceed_with_env(product_lib, env_ref), ceed_with_env(product_lib, env_new or {})
    outs = []
    for c in (ref_ceed, new_ceed):
        p = _problem(c, mk(), degree)
        nlead = max(1, p.mesh.nelem // 3)
        outs.append(_results(p, split=(nlead, _priority(p, nlead)) if split else None))
        p.destroy()
    ref, new = outs
    assert ref.keys() == new.keys()
    for k in ref:
        assert np.all(np.isfinite(ref[k])) and np.abs(ref[k]).max() > 0, k
        assert np.array_equal(ref[k], new[k]), (k, np.abs(ref[k] - new[k]).max(), int((ref[k] != new[k]).sum()))
    for o in outs:                                   # each build's fused consumers against its own two passes, its split pair against its whole apply
        for k in o:
            if ", fused" in k:
                assert np.array_equal(o[k], o[k.replace(", fused", ", two passes")]), k
        if split:
            assert np.array_equal(o["split phases 0 + 1"], o["apply, flags"])
    ref_ceed.destroy(); new_ceed.destroy()


BOXES = {"2x2x2": (2, 2, 2), "3x3x3": (3, 3, 3), "4x4x3": (4, 4, 3)}


@pytest.mark.parametrize("degree", [1, 2, 4])
@pytest.mark.parametrize("box", list(BOXES))
def test_coded_sum_equals_the_plain_one_on_boxes(product_lib, box, degree):
    _compare(product_lib, lambda: _distorted(box_mesh(*BOXES[box])), degree)


def test_coded_sum_across_the_theta_wrap_of_a_cylinder(product_lib):
    _compare(product_lib, lambda: hollow_cylinder_mesh(2, 6, 2), 4)


@pytest.mark.parametrize("limit", [None, 4], ids=["whole table", "table of 4: escape rows"])
def test_coded_sum_on_a_scrambled_rotated_box(product_lib, limit):
    env = {} if limit is None else {"CEED_MI355X_ROWCODE_MAX": str(limit)}
    _compare(product_lib, lambda: scramble_mesh(_distorted(box_mesh(3, 3, 3)), seed=3, order=True, orient=True), 4, env_new=env)
    _compare(product_lib, lambda: scramble_mesh(_distorted(box_mesh(3, 3, 3)), seed=3, order=True, orient=True), 2, env_new=env, split=False)


@pytest.mark.parametrize("degree", [2, 4])
def test_pipelined_form_in_two_segments_sums_coded_rows_of_each_segment(product_lib, degree):
    """2 x 2 x 2 elements: two groups of four at degree 2, four groups of two at degree 4 -- the smallest meshes with two segments; the
    rows of a segment start at a row offset inside the re-ordered map."""
    pipe = {"CEED_MI355X_PIPE_MIN_ROUNDS": "0", "CEED_MI355X_PIPE_SEGMENTS": "2"}
    ys = []
    for env in (PLAIN, dict(PLAIN, **pipe), pipe):
        c = ceed_with_env(product_lib, env)
        p = _problem(c, _distorted(box_mesh(2, 2, 2)), degree)
        op, n = p.levels[p.fine].opJacob, p.lsize()
        X, Y = c.vector(n).set_array(np.random.default_rng(21).uniform(-1, 1, n)), c.vector(n).set_value(-7.0)
        op.apply(X, Y)
        assert op.launch_info()["segments"] == (2 if "CEED_MI355X_PIPE_SEGMENTS" in env else 1), (env, op.launch_info())
        ys.append(Y.to_numpy())
        p.destroy(); c.destroy()
    assert np.abs(ys[0]).max() > 0
    assert np.array_equal(ys[0], ys[1]) and np.array_equal(ys[0], ys[2])
