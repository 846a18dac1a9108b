"""Component-wise Dirichlet masks as data (three flag bits a node, one per component), for tests/test_component_masks.py
and tests/test_component_masks_gpu.py.  No tests here.

``component_mask(dofmap, shift)``: the nodes are classified by (number of elements holding the node, element-interior or not); inside
a class the k-th node (in node order) gets the pattern (k + shift) % 8, bit c = component c masked.  The coverage condition -- each of
the eight patterns in every class -- is asserted: a mesh with a class of fewer than eight nodes is refused.  Different shifts on the
levels of a ladder give coincident coarse and fine nodes different patterns.

The rest is what both files share: the masks laid onto every operator of a SolidProblem (``install``), matrices from unit-vector
applies, and 0/1 diagonals applied as a select."""
import numpy as np

from ceedpetscsolid_amd.solid import SolidProblem
from _numbering import distorted_box

MESH = lambda: distorted_box(3, 3, 3)       # eight interior vertices: the only box with all eight patterns on the 8-contributor nodes
PHYS = dict(nu=0.3, E=2.0)


def node_classes(dm):
    """(contributors, element-interior) -> ascending node ids.  A node is element-interior when its local index in the element that
    holds it has no coordinate on the element's surface."""
    P = dm.P
    count = np.bincount(dm.elem_nodes.ravel(), minlength=dm.nnodes)
    a = np.arange(P)
    inner1 = (a > 0) & (a < P - 1)
    inner = (inner1[:, None, None] & inner1[None, :, None] & inner1[None, None, :]).ravel()      # local node a + P b + P^2 c
    interior = np.zeros(dm.nnodes, dtype=bool)
    interior[dm.elem_nodes[:, inner].ravel()] = True
    assert np.all(count[interior] == 1)
    out = {}
    for n in range(dm.nnodes):
        if count[n]:
            out.setdefault((int(count[n]), bool(interior[n])), []).append(n)
    return {k: np.array(v) for k, v in sorted(out.items())}


def node_patterns(dm, shift):
    """int per node: its pattern 0..7 (nodes no element holds: 0)."""
    pat = np.zeros(dm.nnodes, dtype=np.int64)
    for nodes in node_classes(dm).values():
        pat[nodes] = (np.arange(nodes.size) + shift) % 8
    return pat


def coverage(dm, mask):
    """class -> sorted patterns that occur in it under ``mask``"""
    m = np.asarray(mask).reshape(dm.nnodes, 3) != 0
    pat = m[:, 0] * 1 + m[:, 1] * 2 + m[:, 2] * 4
    return {k: sorted(set(pat[nodes].tolist())) for k, nodes in node_classes(dm).items()}


def component_mask(dm, shift):
    pat = node_patterns(dm, shift)
    mask = ((pat[:, None] >> np.arange(3)[None, :]) & 1).astype(np.uint8).ravel()
    for k, got in coverage(dm, mask).items():
        assert got == list(range(8)), f"class {k} of degree {dm.p} holds the patterns {got} only: this mesh is not to be used"
    return mask


def install(p: SolidProblem, shifts=None):
    """Component masks on every level of ``p`` (level k: shift ``shifts[k]``, default 1 + 3 k) and on every operator that reads one,
    in the modes SolidProblem itself sets.  Returns the masks."""
    shifts = [1 + 3 * k for k in range(len(p.levels))] if shifts is None else shifts
    for lv, s in zip(p.levels, shifts):
        lv.mask = component_mask(lv.dofmap, s)
    fine = p.levels[p.fine]
    p.opApply.set_dirichlet_mask_mode(fine.mask, None, 2)
    for k, lv in enumerate(p.levels):
        lv.opJacob.set_dirichlet_mask_mode(lv.mask, None, 3)
        if lv.opState is not None:
            lv.opState.set_dirichlet_mask_mode(fine.mask, None, 2)
        if k > 0:
            co = p.levels[k - 1]
            lv.opProlong.set_dirichlet_mask_mode(co.mask, lv.mask, 3)
            lv.opRestrict.set_dirichlet_mask_mode(lv.mask, co.mask, 3)
    p._pb_asm = {}
    return [lv.mask for lv in p.levels]


def unmasked(ceed, mesh, degree, physics, **kw):
    """A SolidProblem whose operators carry no constraint at all (the all-zero mask of ``bc_sides=None``)."""
    p = SolidProblem(ceed, mesh, degree, physics, bc_sides=None, **PHYS, **kw)
    assert all(not lv.mask.any() for lv in p.levels)
    return p


def keep(mask, v):
    """K v, K the 0/1 diagonal of ``mask`` -- as a select: no product, so neither NaN nor the sign of zero is at issue."""
    return np.where(np.asarray(mask) != 0, 0.0, v)


def dense(ceed, apply, n_in, n_out):
    """The n_out x n_in matrix of ``apply(X, Y)``, column by column from unit vectors."""
    X, Y = ceed.vector(n_in), ceed.vector(n_out)
    A = np.zeros((n_out, n_in))
    e = np.zeros(n_in)
    for j in range(n_in):
        e[j] = 1.0
        X.set_array(e)
        Y.set_value(-3.0)
        apply(X, Y)
        A[:, j] = Y.to_numpy()
        e[j] = 0.0
    X.destroy(); Y.destroy()
    return A


def masked_matrix(A, mask_in, mask_out, mode=3):
    """K_out A K_in of the mask mode: 1 = input only, 2 = rows only, 3 = both."""
    A = A.copy()
    if mode & 1:
        A[:, np.asarray(mask_in) != 0] = 0.0
    if mode & 2:
        A[np.asarray(mask_out) != 0, :] = 0.0
    return A


def blocks_of(A, mask):
    """The 3 x 3 nodal blocks [node][out][in] of K A K as one vector."""
    n = A.shape[0] // 3
    Am = masked_matrix(A, mask, mask)
    return np.stack([Am[3 * k:3 * k + 3, 3 * k:3 * k + 3] for k in range(n)]).reshape(-1)
