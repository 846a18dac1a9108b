"""Node numberings a caller may hand to the restriction boundary ("the boundary takes ANY offsets"), as replacements
for ``ceedpetscsolid_amd.solid.build_dofmap``:

    monkeypatch.setattr(solid, "build_dofmap", NUMBERINGS["permuted"])

Each replacement calls the real ``build_dofmap`` (the default, locality-ordered numbering: shell nodes in first-touch order, then one
contiguous run of interior nodes per element, no unused entry) and returns a ``NumberedDofMap``: ``elem_nodes``, ``node_keys``,
``node_coords`` and ``nnodes`` transformed TOGETHER -- side_set_nodes, dirichlet_mask, smooth_state, AssembledLevel and the AMG's
rigid-body modes all read the DofMap -- plus ``new``, the node of this numbering that holds default node n.  ``to_default`` /
``from_default`` carry 3-component L-vectors between the two.  No tests here; tests/test_numbering.py guards this file on the CPU.

Offsets whose component 0 is not a multiple of 3 are out of reach: ``DofMap.offsets()`` is 3 x the node."""
from dataclasses import dataclass

import numpy as np

from ceedpetscsolid_amd import solid
from ceedpetscsolid_amd.mesh import DofMap, box_mesh
from ceedpetscsolid_amd.solid import SolidProblem, smooth_displacement
from ceedpetscsolid_amd.mesh import build_dofmap as default_dofmap      # bound here: the tests replace solid.build_dofmap, not this


def distorted_box(nx, ny, nz, seed=0, amp=0.04):
    m = box_mesh(nx, ny, nz)
    rng = np.random.default_rng(seed)
    m.coords += amp / max(nx, ny, nz) * rng.uniform(-1, 1, m.coords.shape)
    return m


@dataclass
class NumberedDofMap(DofMap):
    new: np.ndarray = None        # (default nnodes,) int64: default node -> node of this numbering (not injective under `wrapped`)


def renumbered(dm: DofMap, new: np.ndarray, nnodes: int) -> NumberedDofMap:
    """``dm`` under default node n -> new[n], ``nnodes`` nodes in all.  Nodes no default node maps to are phantoms: key type -1, zero
    coordinates, held by no element.  Where two default nodes share a new node (`wrapped`) the FIRST in default order gives key and
    coordinates."""
    new = np.asarray(new, dtype=np.int64)
    assert new.shape == (dm.nnodes,) and new.min() >= 0 and new.max() < nnodes
    keys = np.zeros((nnodes, dm.node_keys.shape[1]), dtype=np.int64)
    keys[:, 0] = -1
    coords = np.zeros((nnodes, 3))
    keys[new[::-1]] = dm.node_keys[::-1]           # last write wins: the lowest default node
    coords[new[::-1]] = dm.node_coords[::-1]
    return NumberedDofMap(dm.p, int(nnodes), new[dm.elem_nodes].astype(np.int32), keys, coords, dm.ncomp, new)


def default(mesh, p, ncomp=3, locality_order=True):
    dm = default_dofmap(mesh, p, ncomp)
    return renumbered(dm, np.arange(dm.nnodes), dm.nnodes)


def _entity_pair(mesh, p, ncomp):
    """(default DofMap, the generator's entity-ordered DofMap, default node -> entity node from matching the two elem_nodes arrays)."""
    dm, de = default_dofmap(mesh, p, ncomp), default_dofmap(mesh, p, ncomp, locality_order=False)
    assert de.nnodes == dm.nnodes
    new = np.full(dm.nnodes, -1, dtype=np.int64)
    new[dm.elem_nodes.ravel()] = de.elem_nodes.ravel()
    assert np.array_equal(new[dm.elem_nodes], de.elem_nodes) and np.array_equal(np.sort(new), np.arange(dm.nnodes))
    return dm, de, new


def entity(mesh, p, ncomp=3, locality_order=True):
    """The generator's own second mode: vertices, edges, faces, interiors.  The DofMap is the generator's, not a transform of the
    default one; that the two describe the same nodes is asserted."""
    dm, de, new = _entity_pair(mesh, p, ncomp)
    chk = renumbered(dm, new, dm.nnodes)
    assert np.array_equal(chk.node_keys, de.node_keys) and np.array_equal(chk.node_coords, de.node_coords)
    return NumberedDofMap(de.p, de.nnodes, de.elem_nodes, de.node_keys, de.node_coords, de.ncomp, new)


def cells_first(mesh, p, ncomp=3, locality_order=True):
    """The four entity blocks in reverse order -- all interiors, faces, edges, vertices -- as a DMPlex section numbers them
    (cells first, vertices last); the order inside a block is the generator's."""
    dm, de, new = _entity_pair(mesh, p, ncomp)
    kind = de.node_keys[:, 0]
    assert np.all(np.diff(kind) >= 0)                                   # entity order: the key types ascend
    order = np.argsort(-kind, kind="stable")
    e2c = np.empty(de.nnodes, dtype=np.int64)
    e2c[order] = np.arange(de.nnodes)
    return renumbered(dm, e2c[new], dm.nnodes)


def permuted(seed=0):
    def numbering(mesh, p, ncomp=3, locality_order=True):
        dm = default_dofmap(mesh, p, ncomp)
        return renumbered(dm, np.random.default_rng([seed, p]).permutation(dm.nnodes), dm.nnodes)     # another permutation per level
    return numbering


def reversed_(mesh, p, ncomp=3, locality_order=True):
    dm = default_dofmap(mesh, p, ncomp)
    return renumbered(dm, dm.nnodes - 1 - np.arange(dm.nnodes), dm.nnodes)


def gaps(mesh, p, ncomp=3, locality_order=True):
    """new[n] = n + n // 2 + 1 and two more nodes behind the last: node 0, every third node and the last two are held by no element."""
    dm = default_dofmap(mesh, p, ncomp)
    n = np.arange(dm.nnodes)
    new = n + n // 2 + 1
    return renumbered(dm, new, int(new[-1]) + 3)


def wrapped(mesh, p, ncomp=3, locality_order=True):
    """Periodic in x: on an undistorted box_mesh over [0,1]^3 every node with x = 1 is its partner at x = 0 (same y and z, exactly),
    the numbers compacted.  mesh.cells (the coordinate restriction) stays unwrapped, so the geometry is the box's.  With one element
    in x a node occurs twice inside an element; with two the partners are no neighbours in element order."""
    dm = default_dofmap(mesh, p, ncomp)
    X = dm.node_coords
    assert X[:, 0].min() == 0.0 and X[:, 0].max() == 1.0, "wrapped: a box_mesh over [0,1] in x"
    at0, at1 = np.flatnonzero(X[:, 0] == 0.0), np.flatnonzero(X[:, 0] == 1.0)
    partner = {(y, z): n for n, (y, z) in zip(at0, X[at0, 1:].tolist())}
    keep = np.ones(dm.nnodes, dtype=bool)
    keep[at1] = False
    new = np.full(dm.nnodes, -1, dtype=np.int64)
    new[keep] = np.arange(int(keep.sum()))
    new[at1] = [new[partner[(y, z)]] for y, z in X[at1, 1:].tolist()]    # KeyError: no partner with exactly these (y, z)
    assert at0.size == at1.size and new.min() >= 0
    return renumbered(dm, new, int(keep.sum()))


NUMBERINGS = {"entity": entity, "cells_first": cells_first, "permuted": permuted(7), "reversed": reversed_, "gaps": gaps}
ALL_NUMBERINGS = dict(NUMBERINGS, default=default, wrapped=wrapped)


def referenced(dm: DofMap, per_node=None) -> np.ndarray:
    """bool per L-vector entry (or per entry of a vector with ``per_node`` values a node): some element holds its node."""
    hit = np.zeros(dm.nnodes, dtype=bool)
    hit[dm.elem_nodes.ravel()] = True
    return np.repeat(hit, per_node or dm.ncomp)


def to_default(vec, dm: NumberedDofMap) -> np.ndarray:
    """The 3-component L-vector ``vec`` of numbering ``dm`` in the default numbering."""
    return np.asarray(vec).reshape(dm.nnodes, -1)[dm.new].reshape(-1)


def from_default(vec, dm: NumberedDofMap, fill=0.0) -> np.ndarray:
    """The default-numbered 3-component L-vector ``vec`` in numbering ``dm``; entries of nodes no element holds get ``fill``."""
    v = np.asarray(vec).reshape(dm.new.size, -1)
    out = np.full((dm.nnodes, v.shape[1]), fill, dtype=v.dtype)
    out[dm.new] = v
    return out.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------
# every operator of a SolidProblem on inputs that are the same field whatever the numbering
# ---------------------------------------------------------------------------------------------------------------------------
PRESET, KEPT, UNREAD = 3.0, 7.0, 5.0     # outputs before an overwriting apply; phantom entries of an ApplyAdd output; of every input


def run_operators(p, u, seed=42, pointblock=True, transfers=True, own_numbering=False):
    """Residual (+ stored state of every level that carries one), and on every level the Jacobian action, CeedOperatorApplyAdd of it,
    the diagonal, the point-block diagonal, and prolong / restrict on every level pair, of SolidProblem ``p`` built under a
    NumberedDofMap numbering.  ``u``: the displacement in p's numbering.  The other inputs are drawn in the DEFAULT numbering from
    ``seed`` and carried over with from_default, so every numbering of one mesh sees the same fields; input entries no element holds
    are UNREAD (nothing may read them), outputs are preset to PRESET before an overwriting call.  ``own_numbering``: draw the inputs
    in p's numbering itself instead (`wrapped`, where two default nodes are one node and there is no default twin to compare with).
    Returns (vectors, names): name -> numpy array in p's numbering (q-point data as stored); name -> kernel_name / launch_info."""
    import ctypes as C
    c, L = p.ceed, p.ceed.L
    rng = np.random.default_rng(seed)
    out, names = {}, {}
    dms = [lv.dofmap for lv in p.levels]
    vec = lambda arr: c.vector(arr.size).set_array(arr)
    draw = lambda dm: rng.uniform(-1, 1, 3 * (dm.nnodes if own_numbering else dm.new.size))
    carry = lambda v, dm, fill: v if own_numbering else from_default(v, dm, fill)
    fresh = lambda n: c.vector(n).set_value(PRESET)
    n = p.lsize()
    Y = fresh(n)
    p.form_residual(vec(u), Y)
    out["residual"], names["residual"] = Y.to_numpy(), p.opApply.kernel_name
    for k, lv in enumerate(p.levels):
        if lv.gradu is not None and (k == p.fine or lv.own_quadrature):
            out[f"gradu{k}"] = lv.gradu.to_numpy()
    for k, lv in enumerate(p.levels):
        dm, nl = dms[k], p.lsize(k)
        xd, y0d = draw(dm), draw(dm)
        X = vec(carry(xd, dm, UNREAD))
        Y = fresh(nl)
        p.apply_jacobian(k, X, Y)
        out[f"jacobian{k}"], names[f"jacobian{k}"] = Y.to_numpy(), lv.opJacob.kernel_name
        names[f"launch{k}"] = lv.opJacob.launch_info() if L.has("CeedXOperatorGetLaunchInfo") else None
        Y = vec(carry(y0d, dm, KEPT))
        L.chk(L.lib.CeedOperatorApplyAdd(lv.opJacob.h, X.h, Y.h, C.c_void_p(L.REQUEST_IMMEDIATE)))
        out[f"jacobian_add{k}"] = Y.to_numpy()
        D = fresh(nl)
        p.get_diag(k, D)
        out[f"diag{k}"], names[f"diag{k}"] = D.to_numpy(), lv.opJacob.kernel_name
        if pointblock:
            B = fresh(3 * nl)
            p.get_pointblock_diag(k, B)
            out[f"pointblock{k}"], names[f"pointblock{k}"] = B.to_numpy(), lv.opJacob.kernel_name
        if k > 0 and transfers:
            dc, nc = dms[k - 1], p.lsize(k - 1)
            Xc, Yf = vec(carry(draw(dc), dc, UNREAD)), fresh(nl)
            p.prolong(k, Xc, Yf)
            out[f"prolong{k}"], names[f"prolong{k}"] = Yf.to_numpy(), lv.opProlong.kernel_name
            Yf = vec(carry(y0d, dm, KEPT))
            p.prolong_add(k, Xc, Yf)
            out[f"prolong_add{k}"] = Yf.to_numpy()
            Yc = fresh(nc)
            p.restrict(k, X, Yc)
            out[f"restrict{k}"], names[f"restrict{k}"] = Yc.to_numpy(), lv.opRestrict.kernel_name
    return out, names


def level_of(name: str):
    """(level whose numbering the vector `name` of run_operators is in, components per node) -- None for q-point data."""
    name = name.split(" ")[-1]                        # a caller's prefix ("own residual")
    if name.startswith("gradu"):
        return None, 0
    if name == "residual":
        return -1, 3
    k = int(name[-1])
    return (k - 1 if name.startswith("restrict") else k), (9 if name.startswith("pointblock") else 3)


def problem_under(monkeypatch, numbering, ceed, mesh, degree, model, bc, **kw):
    monkeypatch.setattr(solid, "build_dofmap", numbering)
    return SolidProblem(ceed, mesh, degree, model, nu=0.3, E=2.0, bc_sides=bc, **kw)


def wrapped_state(p):
    """A smooth displacement of a problem under `wrapped`: 1-periodic in x, so it is smooth across the identified faces too."""
    return smooth_displacement(p.levels[p.fine].dofmap.node_coords, 0.1, origin=(0., 0., 0.), span=(1., 1., 1.))


def check_wrapped(p, seed=3):
    """Symmetry of the tangent on every level and <yf, P xc> = <R yf, xc> on every level pair of a problem under `wrapped`; returns the
    outputs so that a second backend can be compared on the same inputs."""
    c, rng, outs = p.ceed, np.random.default_rng(seed), {}
    n = p.lsize()
    u = wrapped_state(p)
    Y = c.vector(n)
    p.form_residual(c.vector(n).set_array(u), Y)
    outs["residual"] = Y.to_numpy()
    for k, lv in enumerate(p.levels):
        nl = p.lsize(k)
        free = lv.mask == 0
        v, w = rng.uniform(-1, 1, nl), rng.uniform(-1, 1, nl)
        J = {}
        for name, z in (("v", v), ("w", w)):
            Y = c.vector(nl).set_value(PRESET)
            p.apply_jacobian(k, c.vector(nl).set_array(z), Y)
            J[name] = outs[f"jacobian{k}{name}"] = Y.to_numpy()
        assert np.all(J["v"][~free] == 0.0) and np.abs(J["v"]).max() > 0
        lhs, rhs = (v * free) @ J["w"], (w * free) @ J["v"]
        assert abs(lhs - rhs) < 1e-11 * abs(lhs), (k, lhs, rhs)
        D = c.vector(nl).set_value(PRESET)
        p.get_diag(k, D)
        outs[f"diag{k}"] = D.to_numpy()
        if k > 0:
            nc = p.lsize(k - 1)
            xc = rng.uniform(-1, 1, nc)
            Yf, Yc = c.vector(nl).set_value(PRESET), c.vector(nc).set_value(PRESET)
            p.prolong(k, c.vector(nc).set_array(xc), Yf); p.restrict(k, c.vector(nl).set_array(v), Yc)
            outs[f"prolong{k}"], outs[f"restrict{k}"] = Yf.to_numpy(), Yc.to_numpy()
            lhs, rhs = float(outs[f"prolong{k}"] @ v), float(xc @ outs[f"restrict{k}"])
            assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (k, lhs, rhs)
    return outs
