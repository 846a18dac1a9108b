"""Shared by test_pointblock.py (CPU oracle) and test_pointblock_gpu.py (device): the tiny meshes, the dense Jacobian of a level from
unit-vector applies, and the check of the block algebra -- CeedXVectorPointBlockInvert / Mult / ChebyshevStepPointBlock or their portable
forms -- against NumPy."""
import numpy as np
import pytest

from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem


def jittered_box(nx=2, seed=3):
    """Two hexes that share a face (one with nx=1), every vertex moved: the smallest general geometry with a shared-node sum."""
    mesh = box_mesh(nx, 1, 1, hi=(float(nx), 1.0, 1.0))
    mesh.coords[:] += np.random.default_rng(seed).uniform(-0.08, 0.08, mesh.coords.shape)
    return mesh


def problem_with_state(ceed, mesh, degree, model, qextra=0, nu=0.3, bc_sides=(6,)):
    p = SolidProblem(ceed, mesh, degree, model, nu=nu, E=1.0, bc_sides=list(bc_sides), qextra=qextra, multigrid="none")
    n = p.lsize()
    X, R = ceed.vector(n).set_array(p.smooth_state(0.1)), ceed.vector(n)
    p.form_residual(X, R)              # stores grad u for the hyperelastic tangents
    return p


def level_problem(ceed, mesh, P, Q, model, nu=0.3, bc_sides=(6,)):
    """(problem, level) whose Jacobian has P nodes and Q points per direction, grad u of the smooth state stored.  Q - P <= 2 is a fine
    level with qextra = Q - P; a larger gap exists only as a coarse level under a fine one with Q points (the residual operator, which
    stores the state, runs on the fine level alone): the uniform ladder of degree Q - 1, whose level of degree P - 1 is taken."""
    if Q - P <= 2:
        p = problem_with_state(ceed, mesh, P - 1, model, qextra=Q - P, nu=nu, bc_sides=bc_sides)
        return p, p.fine
    p = SolidProblem(ceed, mesh, Q - 1, model, nu=nu, E=1.0, bc_sides=list(bc_sides), multigrid="uniform")
    n = p.lsize()
    X, R = ceed.vector(n).set_array(p.smooth_state(0.1)), ceed.vector(n)
    p.form_residual(X, R)
    assert p.levels[P - 2].degree == P - 1 and p.levels[P - 2].basisu.Q == Q
    return p, P - 2


def dense_jacobian(p, level):
    c, n = p.ceed, p.lsize(level)
    A = np.zeros((n, n))
    X, Y = c.vector(n), c.vector(n)
    e = np.zeros(n)
    for j in range(n):
        e[j] = 1.0
        X.set_array(e)
        p.apply_jacobian(level, X, Y)
        A[:, j] = Y.to_numpy()
        e[j] = 0.0
    return A


def blocks_of_dense(A):
    nn = A.shape[0] // 3
    i = np.arange(nn)
    return A.reshape(nn, 3, nn, 3)[i, :, i, :]          # [node][c out][c in]


def spd_blocks(n, rng, cond=100.0):
    """n random symmetric positive definite 3 x 3 blocks with condition number <= cond."""
    Qm = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    ev = np.exp(rng.uniform(0.0, np.log(cond), (n, 3))) * rng.uniform(0.5, 2.0, (n, 1))
    return np.einsum("nij,nj,nkj->nik", Qm, ev, Qm)


def drop_patterns(blocks, rng):
    """All eight keep / drop patterns in turn: a dropped component has a zero DIAGONAL entry; its other entries stay (they must be
    ignored)."""
    pat = np.arange(len(blocks)) % 8
    for c in range(3):
        blocks[(pat >> c) & 1 == 1, c, c] = 0.0
    return pat


def embedded_inverse(blocks):
    out = np.zeros_like(blocks)
    for n, B in enumerate(blocks):
        k = np.nonzero(np.diag(B) != 0.0)[0]
        if k.size:
            out[n][np.ix_(k, k)] = np.linalg.inv(B[np.ix_(k, k)])
    return out


def embedded_inverse_stacked(blocks):
    """embedded_inverse without the loop over the nodes, for block counts the loop takes minutes over: a dropped component becomes a
    unit row and column (an inverse of its own, untouched by the others: products with 1 and 0 are exact), one stacked inverse, the
    dropped rows and columns zeroed.  Within 3e-16 of the loop's entries on 4 000 blocks of every pattern."""
    keep = np.einsum("nii->ni", blocks) != 0.0
    kk = keep[:, :, None] & keep[:, None, :]
    return np.where(kk, np.linalg.inv(np.where(kk, blocks, np.eye(3))), 0.0)


STACKED_FROM = 4096      # block counts from which check_block_algebra forms its references stacked


def check_block_algebra(ceed, nnodes, tol, seed=0, bad_sets=None):
    """CeedXVectorPointBlockInvert / Mult / ChebyshevStepPointBlock (or their portable forms) against NumPy.  ``bad_sets``: lists of
    nodes, each planted in turn with blocks that are not positive definite -- the count must be the list's length (default: the first
    and the last node)."""
    rng = np.random.default_rng(seed + nnodes)
    blocks = spd_blocks(nnodes, rng)
    drop_patterns(blocks, rng)
    stacked = nnodes >= STACKED_FROM
    want_inv = embedded_inverse_stacked(blocks) if stacked else embedded_inverse(blocks)
    V = ceed.vector(9 * nnodes).set_array(blocks.reshape(-1))
    assert cd.pointblock_invert(V) == 0
    got = V.to_numpy().reshape(-1, 3, 3)
    scale = np.abs(want_inv).max(axis=(1, 2), keepdims=True)
    scale = scale + (scale == 0.0)                                   # (a block dropped whole: absolute)
    err = (np.abs(got - want_inv) / scale).max()
    zero = np.einsum("nii->ni", blocks) == 0.0
    dropped = zero[:, :, None] | zero[:, None, :]
    assert np.all(got[dropped] == 0.0)
    # for a block whose dropped rows and columns are zero the result is the pseudo-inverse
    clean = np.where(dropped, 0.0, blocks)
    if stacked:
        perr = (np.abs(np.linalg.pinv(clean, rcond=1e-12) - got) / scale).max()
    else:
        perr = max((np.abs(np.linalg.pinv(c, rcond=1e-12) - g).max() / s.max() for c, g, s in zip(clean, got, scale)), default=0.0)
    n = 3 * nnodes
    a = {k: rng.uniform(-1, 1, n) for k in ("x", "d", "b", "t")}
    v = {k: ceed.vector(n).set_array(a[k]) for k in a}
    W, R = ceed.vector(n), ceed.vector(n)
    cd.pointblock_mult(W, V, v["x"])
    want_w = np.einsum("nij,nj->ni", want_inv, a["x"].reshape(-1, 3)).reshape(-1)
    merr = np.abs(W.to_numpy() - want_w).max() / max(np.abs(want_w).max(), 1e-300)
    serr = 0.0
    x, d = a["x"].copy(), a["d"].copy()
    for (c1, c2, assign, use_t, use_r) in [(0.7, 0.0, True, False, False), (0.4, 0.3, False, True, True), (0.9, -0.2, False, True, False)]:
        cd.chebyshev_step_pointblock(v["x"], v["d"], R if use_r else None, v["b"], v["t"] if use_t else None, V, c1, c2, assign)
        ri = a["b"] - a["t"] if use_t else a["b"]
        d = c1 * np.einsum("nij,nj->ni", want_inv, ri.reshape(-1, 3)).reshape(-1) + c2 * d
        x = d.copy() if assign else x + d
        den = max(np.abs(x).max(), 1e-300)
        serr = max(serr, np.abs(v["x"].to_numpy() - x).max() / den, np.abs(v["d"].to_numpy() - d).max() / den)
        if use_r:
            assert np.array_equal(R.to_numpy(), ri)
        assert np.array_equal(v["b"].to_numpy(), a["b"]) and np.array_equal(v["t"].to_numpy(), a["t"])
    print(f"{nnodes} nodes: inverse {err:.2e} (vs pinv {perr:.2e}), multiply {merr:.2e}, step {serr:.2e}")
    assert err <= tol and perr <= tol and merr <= tol and serr <= tol
    # an indefinite block (positive diagonal) and a negative one, planted: counted, nothing else is
    good = spd_blocks(nnodes, rng)
    for nodes in ([sorted({0, nnodes - 1})] if bad_sets is None else bad_sets):
        bad = good.copy()
        for k, node in enumerate(nodes):              # in turn: indefinite with a positive diagonal, negative definite
            bad[node] = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) if k % 2 == 0 else -bad[node]
        V.set_array(bad.reshape(-1))
        assert cd.pointblock_invert(V) == len(nodes), nodes
    # a zero vector stays zero
    V.set_value(0.0)
    assert cd.pointblock_invert(V) == 0 and not V.to_numpy().any()
    V.set_array(blocks.reshape(-1))
    assert cd.pointblock_invert(V, want_n_bad=False) is None
    assert np.array_equal(V.to_numpy().reshape(-1, 3, 3), got)
    # lengths
    short, odd = ceed.vector(9 * nnodes - 9 if nnodes > 1 else 3), ceed.vector(n + 1)
    with pytest.raises(cd.CeedError, match="shorter"):
        cd.pointblock_mult(W, short, v["x"])
    with pytest.raises(cd.CeedError, match="shorter"):
        cd.chebyshev_step_pointblock(v["x"], v["d"], None, v["b"], None, short, 1.0, 0.0, True)
    with pytest.raises(cd.CeedError, match="multiple of 3"):
        cd.pointblock_mult(odd, ceed.vector(3 * (n + 1)), odd)
    for o in list(v.values()) + [V, W, R, short, odd]:
        o.destroy()
