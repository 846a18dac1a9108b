"""The portable NumPy forms: what the optional entry points of include/ceed.h compute, restated in float64 NumPy on host arrays.  They run
where the library lacks an entry point (the CPU oracle) and are the yardstick of the device parity tests ("Portable forms").
NumPy only; vectors are taken by duck typing (``n``, ``to_numpy()``, ``fill()``); ``ceed.py`` imports from here, never the reverse.

WHICH FORM RUNS is decided per object at construction for operators and face terms (``Ceed.has_qfunction(name)``, ``L.has(PREFIX +
"Create")``: ``MassOperator``, ``Stress``, ``FaceTerm``), per call for the vector operations (``L.has(symbol)``: point-block, leapfrog,
block Gram / combine, the point-block diagonal); ``portable=True`` forces the NumPy form.  The device library exports every entry point
(``build()`` checks), so on the device a NumPy form never stands in for a kernel.

Sections: (a) array forms on host arrays, no Ceed objects; (b) the tensor layer of the element (3-D) and face (2-D) terms: gather through
the offsets, the 1-D tables along each direction, the sum into an L-vector in item order; (c) the write-back into a vector of the Ceed.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .mesh import gll_nodes


def _np_f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


# ---- (a) array forms: point-block Jacobi (CeedXVectorPointBlock*, CeedXVectorChebyshevStepPointBlock) ------------------------------
def pointblock_invert_host(blocks: np.ndarray):
    """(inverses, n_bad) of 3 x 3 blocks [n][c out][c in], as CeedXVectorPointBlockInvert defines them: a component whose diagonal
    entry is exactly zero is dropped, the inverse of the remaining principal sub-block is embedded in zeros; n_bad counts the blocks
    with a non-finite or non-positive pivot of the elimination without interchanges."""
    B = _np_f64(blocks).reshape(-1, 3, 3)
    keep = B[:, [0, 1, 2], [0, 1, 2]] != 0.0
    kk = keep[:, :, None] & keep[:, None, :]
    M = np.where(kk, B, np.eye(3)[None])
    with np.errstate(all="ignore"):
        p0 = M[:, 0, 0]
        l1, l2 = M[:, 1, 0] / p0, M[:, 2, 0] / p0
        b11, b12 = M[:, 1, 1] - l1 * M[:, 0, 1], M[:, 1, 2] - l1 * M[:, 0, 2]
        b21, b22 = M[:, 2, 1] - l2 * M[:, 0, 1], M[:, 2, 2] - l2 * M[:, 0, 2]
        p1 = b11
        p2 = b22 - (b21 / p1) * b12
        ok = np.ones(len(M), dtype=bool)
        for p in (p0, p1, p2):
            ok &= (p > 0.0) & np.isfinite(p)
        c00 = M[:, 1, 1] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 1]
        c01 = M[:, 1, 2] * M[:, 2, 0] - M[:, 1, 0] * M[:, 2, 2]
        c02 = M[:, 1, 0] * M[:, 2, 1] - M[:, 1, 1] * M[:, 2, 0]
        det = (M[:, 0, 0] * c00 + M[:, 0, 1] * c01) + M[:, 0, 2] * c02
        inv = np.empty_like(M)
        inv[:, 0, 0], inv[:, 1, 0], inv[:, 2, 0] = c00 / det, c01 / det, c02 / det
        inv[:, 0, 1] = (M[:, 0, 2] * M[:, 2, 1] - M[:, 0, 1] * M[:, 2, 2]) / det
        inv[:, 1, 1] = (M[:, 0, 0] * M[:, 2, 2] - M[:, 0, 2] * M[:, 2, 0]) / det
        inv[:, 2, 1] = (M[:, 0, 1] * M[:, 2, 0] - M[:, 0, 0] * M[:, 2, 1]) / det
        inv[:, 0, 2] = (M[:, 0, 1] * M[:, 1, 2] - M[:, 0, 2] * M[:, 1, 1]) / det
        inv[:, 1, 2] = (M[:, 0, 2] * M[:, 1, 0] - M[:, 0, 0] * M[:, 1, 2]) / det
        inv[:, 2, 2] = (M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 1, 0]) / det
    return np.where(kk, inv, 0.0), int((~ok).sum())


def pointblock_mult_host(blocks: np.ndarray, x: np.ndarray) -> np.ndarray:
    """w_n = B_n x_n on host arrays (x of 3 n entries, blocks of at least 9 n)."""
    xv = _np_f64(x).reshape(-1, 3)
    B = _np_f64(blocks)[:9 * len(xv)].reshape(-1, 3, 3)
    return ((B[:, :, 0] * xv[:, None, 0] + B[:, :, 1] * xv[:, None, 1]) + B[:, :, 2] * xv[:, None, 2]).reshape(-1)


def chebyshev_step_pointblock_host(x, d, b, t, blocks, c1, c2, assign_x):
    """(x, d, ri) after one step of CeedXVectorChebyshevStepPointBlock on host arrays: ri = b - t (t may be None),
    d = c1 B ri + c2 d, x = d or x + d."""
    ri = _np_f64(b) - _np_f64(t) if t is not None else _np_f64(b).copy()
    dn = c1 * pointblock_mult_host(blocks, ri)
    if c2 != 0.0:
        dn = c2 * _np_f64(d) + dn
    return (dn.copy() if assign_x else _np_f64(x) + dn), dn, ri


# ---- (a) explicit dynamics: CeedXVectorLeapfrogStep -------------------------------------------------------------------------------
def leapfrog_step_host(x: np.ndarray, vh: np.ndarray, r: np.ndarray, f: Optional[np.ndarray], m: np.ndarray, load: float, c1: float,
                       c2: float, dt: float, tally: bool = True) -> Optional[float]:
    """One leapfrog step IN PLACE on the float64 host arrays x and vh (all arrays of one length), as CeedXVectorLeapfrogStep defines it
    (include/ceed.h): the same operations in the same order, each rounded on its own, so x and vh carry the bits of the device kernel.
    Rows with m <= 0 are neither read into a result nor written.  Returns 0.5 sum m vm^2 (``tally``), else None."""
    act = m > 0.0
    mi, ri, vo = m[act], r[act], vh[act]
    g = load * f[act] - ri if f is not None else -ri
    q = g / mi
    vn = c1 * vo + c2 * q
    ke = None
    if tally:
        vm = 0.5 * (vo + vn)
        ke = 0.5 * float(np.sum(mi * (vm * vm)))
    vh[act] = vn
    x[act] = x[act] + dt * vn
    return ke


# ---- (a) block vectors: CeedXVectorBlockGram / CeedXVectorBlockCombine ------------------------------------------------------------
BLOCK_HOST_CHUNK = 1024          # rows per np.add.reduce of the portable Gram matrix: a fixed chunking, so it is deterministic too


def block_gram_host(A: np.ndarray, B: np.ndarray, w: Optional[np.ndarray] = None) -> np.ndarray:
    """G[i][j] = sum_r w[r] (A[i][r] B[j][r]) of host arrays [ka][n], [kb][n]: the products of BLOCK_HOST_CHUNK rows summed by
    np.add.reduce, the chunks added in row order."""
    ka, n = A.shape
    G = np.zeros((ka, B.shape[0]))
    for c in range(0, n, BLOCK_HOST_CHUNK):
        T = A[:, None, c:c + BLOCK_HOST_CHUNK] * B[None, :, c:c + BLOCK_HOST_CHUNK]
        if w is not None:
            T = w[c:c + BLOCK_HOST_CHUNK] * T
        G += np.add.reduce(T, axis=2)
    return G


def block_combine_host(Y: np.ndarray, A: np.ndarray, Cm: np.ndarray, beta: float):
    """Y[j] = sum_i A[i] Cm[i][j] + beta Y[j] in place on host arrays [ky][n], [ka][n]; i in order; beta == 0 does not read Y."""
    acc = np.zeros(Y.shape)
    for i in range(A.shape[0]):
        acc += Cm[i][:, None] * A[i][None, :]
    Y[...] = acc if beta == 0.0 else acc + beta * Y


# ---- (a) tables, and the point-block diagonal from element matrices ---------------------------------------------------------------
def lagrange_tables(P: int, Q: int):
    """(B, D, w): values and derivatives (Q x P) of the P Lagrange functions on the Gauss-Lobatto points at the Q Gauss points, and the
    Gauss weights."""
    nodes = gll_nodes(P)
    pts, w = np.polynomial.legendre.leggauss(Q)
    B, D = np.zeros((Q, P)), np.zeros((Q, P))
    for i in range(P):
        others = [k for k in range(P) if k != i]
        den = np.prod([nodes[i] - nodes[k] for k in others])
        B[:, i] = np.prod([pts - nodes[k] for k in others], axis=0) / den
        for m in others:
            D[:, i] += np.prod([pts - nodes[k] for k in others if k != m] + [np.ones(Q)], axis=0) / den
    return B, D, w


def pointblock_diag_host(columns: np.ndarray, nodes: np.ndarray, nblocks: int, mask=None) -> np.ndarray:
    """The 3 x 3 nodal blocks [nblocks][c out][c in] of element matrices given by columns, [n' c_in][e][n c_out] (AssembledLevel.coo):
    their diagonal blocks summed over the elements of a node (``nodes`` [e][n]) in element order; the rows and columns of the masked
    entries (``mask``: an L-vector of flags) are zero."""
    ne, P3 = nodes.shape
    K = _np_f64(columns).reshape(P3, 3, ne, P3, 3)
    n = np.arange(P3)
    eb = K[n, :, :, n, :].transpose(2, 0, 3, 1)                   # [e][n][c_out][c_in]
    out = node_sum(nodes, eb.reshape(ne, P3, 9), nblocks).reshape(-1, 3, 3)
    if mask is not None:
        m = np.asarray(mask).reshape(-1, 3) != 0
        out[:m.shape[0]][m[:, :, None] | m[:, None, :]] = 0.0
    return out


# ---- (b) the tensor layer: items are elements (three tables, [e][k][j][i]) or faces (two tables, [f][j][i]) ------------------------
def _tensor(x: np.ndarray, tables, transpose: bool) -> np.ndarray:
    """The einsum of ``len(tables)`` directions between the nodal and the point operand: "ai,bj,dk", "ekjic", "edbac" (elements), "ai,bj",
    "fjic", "fbac" (faces); the trailing component axis is there if ``x`` has one."""
    d = len(tables)
    item, c = "ef"[3 - d], "c" * (x.ndim - d - 1)
    nod, pts = item + "ijk"[d - 1::-1] + c, item + "abd"[d - 1::-1] + c
    return np.einsum(",".join(p + i for p, i in zip("abd", "ijk"[:d])) + (f",{pts}->{nod}" if transpose else f",{nod}->{pts}"), *tables, x)


def gather(field, nodes: np.ndarray, lsize: int) -> np.ndarray:
    """The nodal values [nodes.shape][c] of the L-vector ``field`` (its first ``lsize`` entries; node ``lsize // 3`` reads as zero)."""
    f = np.concatenate([np.asarray(field, dtype=np.float64).reshape(-1)[:lsize], np.zeros(3)])
    return f.reshape(-1, 3)[nodes]


def to_points(u: np.ndarray, *tables) -> np.ndarray:
    """Nodal values [item][..][j][i]([c]) to the points [item][..][b][a]([c]); ``tables[0]`` ([a][i]) acts on the fastest direction."""
    return _tensor(u, tables, False)


def to_nodes(v: np.ndarray, *tables) -> np.ndarray:
    """The transpose of ``to_points``: point values [item][..][b][a]([c]) to nodal sums [item][..][j][i]([c])."""
    return _tensor(v, tables, True)


def node_sum(nodes: np.ndarray, contrib: np.ndarray, nnodes: int) -> np.ndarray:
    """[nnodes][m]: the rows of ``contrib`` ([nodes.shape][m], items in order) added by ``np.add.at``, in that order."""
    out = np.zeros((nnodes, contrib.shape[-1]))
    np.add.at(out, nodes.reshape(-1), contrib.reshape(-1, contrib.shape[-1]))
    return out


# ---- (c) the write-back -------------------------------------------------------------------------------------------------------------
# ``assign`` and ``add`` hand the whole changed array to ``Vector.fill``: a plain vector takes it with ``set_array``, a tensor-backed one
# (``Ceed.tensor_vector``) copies it into its tensor and keeps its alias -- ``set_array`` would give it private storage the tensor never
# sees.  The third legitimate form is in place: ``Vector.leapfrog_step`` through ``host_view``, the block operations on the block's tensor.
def assign(y, values, n: Optional[int] = None):
    """y[:len(values)] = values; entries up to ``n`` (default: none) are zeroed, the rest of a longer vector is left alone."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    full = np.zeros(y.n) if y.n in (n, v.size) else y.to_numpy()          # nothing of y survives: it is not read
    full[:v.size], full[v.size:max(n or 0, v.size)] = v, 0.0
    y.fill(full)


def add(y, values):
    """y[:len(values)] += values."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    assign(y, y.to_numpy()[:v.size] + v)
