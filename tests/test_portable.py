"""portable.py on the CPU oracle: the tensor layer (gather, to_points, to_nodes, node_sum) against plain Python loops, and the write-back
(assign, add) on plain, tensor-backed and longer vectors, directly and through every public entry that writes a portable result.

Bound of the tensor checks: a sum of n products formed in two orders differs by at most 2 (n + 3) u S, u = 2^-53, S the sum of the
absolute products (each of the three multiplications and each addition rounds once); n = P^d."""
import itertools

import numpy as np
import pytest

import _contact_inputs as ci
from _pointblock_common import jittered_box, problem_with_state, spd_blocks
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd import portable as pt
from ceedpetscsolid_amd.contact import ContactSurface
from ceedpetscsolid_amd.mesh import box_mesh, build_dofmap
from ceedpetscsolid_amd.surface import SurfaceLoad

U = 2.0 ** -53


def items(dim, P):
    """Node lists [2][P]..[P] of two items that share a side (a face of two hexes, an edge of two faces) on a line of 2 P - 1 nodes in
    the fastest direction; in 2-D the second face is degenerate: its last node is its first once more."""
    nx = 2 * P - 1
    idx = np.indices((P,) * dim)[::-1]                                   # idx[0]: the fastest direction
    flat = sum(idx[m] * (nx * P ** (m - 1) if m else 1) for m in range(dim))
    nodes = np.stack([flat, flat + P - 1])
    if dim == 2:
        nodes[1, -1, -1] = nodes[1, 0, 0]
    return nodes, nx * P ** (dim - 1)


def loops(u, tables, transpose):
    """to_points (or its transpose) of one component-free operand by loops; returns (result, sum of the absolute products)."""
    dim = len(tables)
    Q, P = tables[0].shape
    dst = (P,) * dim if transpose else (Q,) * dim
    out, S = np.zeros((u.shape[0],) + dst), np.zeros((u.shape[0],) + dst)
    for e in range(u.shape[0]):
        for q in itertools.product(range(Q), repeat=dim):                # q = (.., b, a): slowest direction first, as the arrays are
            for n in itertools.product(range(P), repeat=dim):
                w = 1.0
                for m in range(dim):                                     # tables[m] acts on direction m, the m-th FROM THE END of the index
                    w = w * tables[m][q[dim - 1 - m], n[dim - 1 - m]]
                s, d = (q, n) if transpose else (n, q)
                out[(e,) + d] += w * u[(e,) + s]
                S[(e,) + d] += abs(w * u[(e,) + s])
    return out, S


@pytest.mark.parametrize("dim,P,Q", [(3, 2, 3), (3, 3, 3), (2, 2, 2), (2, 3, 5)])
def test_the_tensor_layer_against_loops(dim, P, Q):
    rng = np.random.default_rng(10 * P + Q + dim)
    nodes, nnodes = items(dim, P)
    lsize = 3 * nnodes
    field = rng.uniform(-1, 1, lsize + 2)                                # two entries past the L-size: never read
    tables = [rng.uniform(-1, 1, (Q, P)) for _ in range(dim)]            # a different table per direction: a swapped direction shows
    # gather: exact
    ue = pt.gather(field, nodes, lsize)
    assert ue.shape == nodes.shape + (3,) and ue.flags.c_contiguous
    for ix in np.ndindex(nodes.shape):
        assert np.array_equal(ue[ix], field[3 * nodes[ix]:3 * nodes[ix] + 3])
    pad = pt.gather(field, np.array([[nnodes, 0]]), lsize)               # the node past the end reads as zero
    assert np.array_equal(pad[0, 0], np.zeros(3)) and np.array_equal(pad[0, 1], field[:3])
    # to_points, with and without the component axis
    uq = pt.to_points(ue, *tables)
    assert uq.shape == (2,) + (Q,) * dim + (3,)
    worst = 0.0
    for c in range(3):
        want, S = loops(ue[..., c], tables, False)
        worst = max(worst, (np.abs(uq[..., c] - want) / S).max())
        assert np.all(np.abs(pt.to_points(np.ascontiguousarray(ue[..., c]), *tables) - want) <= 2 * (P ** dim + 3) * U * S)
    # to_nodes
    vq = rng.uniform(-1, 1, uq.shape)
    vn = pt.to_nodes(vq, *tables)
    assert vn.shape == ue.shape
    for c in range(3):
        want, S = loops(vq[..., c], tables, True)
        worst = max(worst, (np.abs(vn[..., c] - want) / S).max())
        assert np.all(np.abs(pt.to_nodes(np.ascontiguousarray(vq[..., c]), *tables) - want) <= 2 * (Q ** dim + 3) * U * S)
    print(f"dim {dim} P {P} Q {Q}: worst |einsum - loops| / sum |products| = {worst:.2e}")
    assert worst <= 2 * (max(P, Q) ** dim + 3) * U
    # the transpose: <to_points u, v> = <u, to_nodes v>
    lhs, rhs = float((uq * vq).sum()), float((ue * vn).sum())
    assert abs(lhs - rhs) <= 1e-14 * np.linalg.norm(uq) * np.linalg.norm(vq)
    # node_sum: item order, exact against the loop; a node twice in an item (2-D) and in two items (the shared side)
    assert np.unique(nodes).size < nodes.size
    got = pt.node_sum(nodes, vn, nnodes)
    want = np.zeros((nnodes, 3))
    for ix in np.ndindex(nodes.shape):
        want[nodes[ix]] += vn[ix]
    assert got.shape == want.shape and np.array_equal(got, want)


def test_node_sum_adds_in_item_order():
    """(1e16 + 1) - 1e16 = 0 in the order of the items; any other order of the three gives 1."""
    nodes = np.array([[2, 0], [2, 1], [2, 0]])
    contrib = np.array([[[1e16], [3.0]], [[1.0], [4.0]], [[-1e16], [5.0]]])
    out = pt.node_sum(nodes, contrib, 4)
    assert np.array_equal(out, [[8.0], [4.0], [0.0], [0.0]])
    assert np.array_equal(pt.node_sum(nodes[[0, 2, 1]], contrib[[0, 2, 1]], 4), [[8.0], [4.0], [1.0], [0.0]])
    assert pt.node_sum(np.zeros((0, 4), dtype=np.int64), np.zeros((0, 4, 3)), 5).shape == (5, 3)          # no item at all


def test_the_einsum_subscripts_and_operand_order_are_the_recorded_ones(monkeypatch):
    """The bits of every portable form follow from these strings and from the tables coming first, in the order given."""
    seen = []
    real = np.einsum
    monkeypatch.setattr(pt.np, "einsum", lambda spec, *ops: seen.append((spec, ops)) or real(spec, *ops))
    B, G, D = np.ones((3, 2)), 2 * np.ones((3, 2)), 3 * np.ones((3, 2))
    u3, u2 = np.ones((1, 2, 2, 2, 3)), np.ones((1, 2, 2, 3))
    pt.to_points(u3, G, B, D); pt.to_nodes(np.ones((1, 3, 3, 3, 3)), G, B, D); pt.to_nodes(np.ones((1, 3, 3, 3)), G, B, D)
    pt.to_points(u2, D, B); pt.to_nodes(np.ones((1, 3, 3, 3)), B, D); pt.to_points(np.ones((1, 2, 2)), B, B)
    assert [s for s, _ in seen] == ["ai,bj,dk,ekjic->edbac", "ai,bj,dk,edbac->ekjic", "ai,bj,dk,edba->ekji", "ai,bj,fjic->fbac",
                                    "ai,bj,fbac->fjic", "ai,bj,fji->fba"]
    assert [o is t for o, t in zip(seen[0][1], (G, B, D, u3))] == [True] * 4
    assert [o is t for o, t in zip(seen[3][1], (D, B, u2))] == [True] * 3


# ---------------------------------------------------------------- the write-back
def vectors(oracle, n):
    """(kind, vector of n entries prefilled with 100, 101, ...): a plain one and one over a CPU tensor."""
    plain, tens = oracle.vector(n).set_array(100.0 + np.arange(n)), oracle.tensor_vector(n, "cpu")
    tens.fill(100.0 + np.arange(n))
    assert tens.t is not None and np.array_equal(tens.t.numpy(), plain.to_numpy())
    return [("plain", plain), ("tensor", tens)]


def coherent(v, want):
    """The vector reads as ``want``, and so does the tensor behind it if it has one."""
    assert np.array_equal(v.to_numpy(), want), (v.to_numpy(), want)
    if v.t is not None:
        assert np.array_equal(v.t.numpy(), want), (v.t.numpy(), want)


@pytest.mark.parametrize("extra", [0, 4])
def test_assign_and_add_on_plain_tensor_backed_and_longer_vectors(oracle, extra):
    vals = np.array([1.5, -2.0, 0.25, 8.0, -0.5, 3.0])
    n = vals.size + extra
    tail = 100.0 + np.arange(n)[vals.size:]
    for kind, v in vectors(oracle, n):
        pt.assign(v, vals)
        coherent(v, np.concatenate([vals, tail]))                        # the values land, the tail is untouched
        pt.add(v, 2.0 * vals.reshape(2, 3))                              # (any shape: the values are taken flat)
        coherent(v, np.concatenate([3.0 * vals, tail]))
        pt.assign(v, vals[:2], n=vals.size)                              # zeros up to n, the rest left alone
        coherent(v, np.concatenate([vals[:2], np.zeros(vals.size - 2), tail]))
        pt.assign(v, vals[:3], n=n)
        coherent(v, np.concatenate([vals[:3], np.zeros(n - 3)]))
        with pytest.raises(ValueError):
            pt.assign(v, np.zeros(n + 1))
        v.destroy()


def test_the_three_recorded_cases_keep_the_tensor_and_the_vector_equal(oracle):
    """What went apart before the write-back was one function: a copy into a tensor-backed vector, a face term's addition, the
    point-block product."""
    v = oracle.tensor_vector(6, "cpu")
    v.fill(np.arange(6.0))
    pt.assign(v, np.arange(6.0) + 10)
    coherent(v, np.arange(6.0) + 10)
    y = oracle.tensor_vector(7, "cpu")
    y.fill(np.ones(7))
    pt.add(y, 2.0 * np.ones(6))
    coherent(y, np.array([3.0] * 6 + [1.0]))
    w, x, blocks = oracle.tensor_vector(3, "cpu"), oracle.vector(3).set_value(1.0), oracle.vector(9).set_array(2.0 * np.eye(3).reshape(-1))
    cd.pointblock_mult(w, blocks, x)
    coherent(w, np.full(3, 2.0))
    for o in (v, y, w, x, blocks):
        o.destroy()


def test_the_point_block_entries_write_through_a_tensor_backed_vector(oracle, oracle_lib):
    assert not oracle_lib.has("CeedXVectorPointBlockMult")               # the portable forms run here
    nn = 5
    rng = np.random.default_rng(2)
    blocks = spd_blocks(nn, rng)
    a = {k: rng.uniform(-1, 1, 3 * nn) for k in "xdbt"}
    res = {}
    for kind in ("plain", "tensor"):
        new = (lambda n: oracle.tensor_vector(n, "cpu")) if kind == "tensor" else oracle.vector
        V = new(9 * nn)
        V.fill(blocks.reshape(-1))
        assert cd.pointblock_invert(V) == 0
        v = {k: new(3 * nn) for k in a}
        for k in a:
            v[k].fill(a[k])
        W, R = new(3 * nn), new(3 * nn)
        cd.pointblock_mult(W, V, v["x"])
        cd.chebyshev_step_pointblock(v["x"], v["d"], R, v["b"], v["t"], V, 0.4, 0.3, False)
        res[kind] = [o.to_numpy() for o in (V, W, R, v["x"], v["d"])]
        for o, want in zip((V, W, R, v["x"], v["d"]), res[kind]):
            coherent(o, want)
        for o in [V, W, R] + list(v.values()):
            o.destroy()
    inv, _ = pt.pointblock_invert_host(blocks)
    assert np.array_equal(res["plain"][0], inv.reshape(-1)) and np.array_equal(res["plain"][1], pt.pointblock_mult_host(inv, a["x"]))
    for p, t in zip(res["plain"], res["tensor"]):
        assert np.array_equal(p, t)


def test_the_face_terms_write_through_a_tensor_backed_vector(oracle):
    mesh = box_mesh(2, 2, 1)
    dm = build_dofmap(mesh, 1)
    n = dm.lsize
    u, du = ci.displacement(dm, 2, 2)
    sl = SurfaceLoad(oracle, mesh, dm, [1, 5], 2, portable=True)
    cs = ContactSurface(oracle, mesh, dm, [1, 5], 2, portable=True)
    ci.set_obstacle(cs, "plane", u)
    r, st = cs.residual_host(u)
    U_, DU = oracle.vector(n).set_array(u), oracle.vector(n).set_array(du)
    for (kind, y), (_, state) in zip(vectors(oracle, n + 2), vectors(oracle, cs.state_size + 3)):
        want = 100.0 + np.arange(n + 2)
        sl.traction_add([0.3, -0.2, 1.1], 1.5, y)
        want[:n] += 1.5 * sl.traction_host([0.3, -0.2, 1.1])
        coherent(y, want)
        cs.residual_add(2.0, U_, y, state)
        want[:n] += 2.0 * r
        coherent(y, want)
        coherent(state, np.concatenate([st.reshape(-1), 100.0 + np.arange(cs.state_size, cs.state_size + 3)]))
        cs.tangent_add(0.5, state, DU, y)
        want[:n] += 0.5 * cs.tangent_host(st, du)
        coherent(y, want)
        cs.diagonal_add(-0.25, state, y)
        want[:n] += -0.25 * cs.diagonal_host(st)
        coherent(y, want)
        assert np.abs(r).max() > 0 and np.abs(cs.diagonal_host(st)).max() > 0
        y.destroy(); state.destroy()


def test_the_point_block_diagonal_writes_through_a_tensor_backed_vector(oracle):
    p = problem_with_state(oracle, jittered_box(), 1, "linElas")
    n = 3 * p.lsize()
    B, T = oracle.vector(n).set_value(3.0), oracle.tensor_vector(n, "cpu")
    p.get_pointblock_diag(p.fine, B)
    p.get_pointblock_diag(p.fine, T)
    assert np.abs(B.to_numpy()).max() > 0 and not np.any(B.to_numpy() == 3.0)
    coherent(T, B.to_numpy())
    p.destroy()
