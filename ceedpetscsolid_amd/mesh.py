"""Hex meshes -> element restrictions: the step in front of the operator path.

Replaces what the reference gets from PETSc DMPlex (src/setupdm.c:40-201,
src/setuplibceed.c:194-240 ``CreateRestrictionPlex``): HEX8 topology from a
structured generator or an Exodus file, high-order Gauss-Lobatto node numbering
with interlaced ``[node][comp]`` L-vectors, tensor (x-fastest) element closure
order (setupdm.c:194), Dirichlet node sets from side sets, and an element
partition with interface lists for the multi-GPU halo sum.

DMPlex's own local numbering cannot be reproduced without PETSc;
the numbering here is deterministic and chosen for gather locality: nodes are
numbered in order of first touch while sweeping elements, so an element's new
nodes are contiguous in the L-vector.

Pure numpy, host side, set-up time only.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

# tensor-order corner c = i + 2 j + 4 k  (i,j,k in {0,1}; x fastest)
# local faces: 0:x- 1:x+ 2:y- 3:y+ 4:z- 5:z+
_EXO_TO_TENSOR = np.array([0, 1, 3, 2, 4, 5, 7, 6])
# Exodus HEX8 side (1-based) -> tensor local face
_EXO_SIDE_TO_FACE = {1: 2, 2: 1, 3: 3, 4: 0, 5: 4, 6: 5}


@dataclass
class HexMesh:
    coords: np.ndarray            # (nv, 3) vertex coordinates
    cells: np.ndarray             # (ne, 8) vertex ids, tensor order
    side_sets: Dict[int, np.ndarray] = field(default_factory=dict)  # id -> (nf, 2) [elem, local face]
    vertex_gid: Optional[np.ndarray] = None  # (nv,) global vertex ids (sub-meshes)
    name: str = "mesh"

    @property
    def nelem(self) -> int:
        return self.cells.shape[0]

    @property
    def nvert(self) -> int:
        return self.coords.shape[0]

    def gid(self) -> np.ndarray:
        return np.arange(self.nvert, dtype=np.int64) if self.vertex_gid is None else self.vertex_gid


# --------------------------------------------------------------------------
# generators
# --------------------------------------------------------------------------
def box_mesh(nx: int, ny: int, nz: int, lo=(0., 0., 0.), hi=(1., 1., 1.)) -> HexMesh:
    """Structured box, as ``-dm_plex_box_faces nx,ny,nz`` (setupdm.c:49-52).  Face sets
    follow PETSc's box labels: 1 z-, 2 z+, 3 y-, 4 y+, 5 x+, 6 x-."""
    xs = [np.linspace(lo[d], hi[d], n + 1) for d, n in enumerate((nx, ny, nz))]
    Z, Y, X = np.meshgrid(xs[2], xs[1], xs[0], indexing="ij")
    coords = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    vid = lambda i, j, k: (k * (ny + 1) + j) * (nx + 1) + i
    K, J, I = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    I, J, K = I.ravel(), J.ravel(), K.ravel()
    cells = np.stack([vid(I + (c & 1), J + ((c >> 1) & 1), K + ((c >> 2) & 1)) for c in range(8)], axis=1)
    e = np.arange(cells.shape[0])
    ss = {}
    for sid, (mask, face) in {6: (I == 0, 0), 5: (I == nx - 1, 1), 3: (J == 0, 2), 4: (J == ny - 1, 3),
                              1: (K == 0, 4), 2: (K == nz - 1, 5)}.items():
        ss[sid] = np.stack([e[mask], np.full(mask.sum(), face)], axis=1)
    return HexMesh(coords, cells.astype(np.int64), ss, name=f"box{nx}x{ny}x{nz}")


def hollow_cylinder_mesh(nr: int, nth: int, nz: int, r_in=0.5, r_out=1.0, z0=-5.0, z1=5.0) -> HexMesh:
    """Structured hollow cylinder with the geometry and side-set ids of the reference's
    ``cylinder8_*_4ss_us.exo`` family (meshes/cylinder8.jou):
    996 inner, 997 outer, 998 z=z0, 999 z=z1.  Stand-in for the absent
    ``cylinder8_99Ke_4ss_us.exo`` (.MISSING_LARGE_BLOBS:6).  Elements are ordered
    r fastest, then theta, then z."""
    r = np.linspace(r_in, r_out, nr + 1)
    th = 2 * np.pi * np.arange(nth) / nth
    z = np.linspace(z0, z1, nz + 1)
    Zg, Tg, Rg = np.meshgrid(z, th, r, indexing="ij")
    coords = np.stack([(Rg * np.cos(Tg)).ravel(), (Rg * np.sin(Tg)).ravel(), Zg.ravel()], axis=1)
    vid = lambda i, j, k: (k * nth + (j % nth)) * (nr + 1) + i
    K, J, I = np.meshgrid(np.arange(nz), np.arange(nth), np.arange(nr), indexing="ij")
    I, J, K = I.ravel(), J.ravel(), K.ravel()
    # local x = r, y = theta, z = z is right-handed (r, theta, z)
    cells = np.stack([vid(I + (c & 1), J + ((c >> 1) & 1), K + ((c >> 2) & 1)) for c in range(8)], axis=1)
    e = np.arange(cells.shape[0])
    ss = {}
    for sid, (mask, face) in {996: (I == 0, 0), 997: (I == nr - 1, 1), 998: (K == 0, 4), 999: (K == nz - 1, 5)}.items():
        ss[sid] = np.stack([e[mask], np.full(mask.sum(), face)], axis=1)
    return HexMesh(coords, cells.astype(np.int64), ss, name=f"cyl{nr}x{nth}x{nz}")


def read_exodus(path: str) -> HexMesh:
    """Exodus II (NetCDF classic CDF-2) reader for the reference's ``meshes/*.exo``: HEX8 blocks, and HEX27 blocks through
    their eight corner nodes (the first eight of an Exodus HEX27; the mid-edge / mid-face / centre nodes carry no
    information for an isoparametric trilinear geometry and are dropped).  Boundaries: side sets (``*_ss_*``), or -- the
    ``*_ns_*`` files, SURVEY App. D -- node sets, turned into side sets: a BOUNDARY face (one owned by exactly one element)
    belongs to set ``id`` when all four of its corner nodes do (interior faces never: a mesh one element thick between two
    surfaces of a set would otherwise turn them into boundary faces -- ADVICE r2)."""
    from scipy.io import netcdf_file
    f = netcdf_file(path, "r", mmap=False)
    v = f.variables
    if "coordx" in v:
        coords = np.stack([np.array(v[k][:], dtype=np.float64) for k in ("coordx", "coordy", "coordz")], axis=1)
    else:
        coords = np.array(v["coord"][:], dtype=np.float64).T.copy()
    conn = []
    b = 1
    while f"connect{b}" in v:
        c = np.array(v[f"connect{b}"][:], dtype=np.int64) - 1
        if c.shape[1] not in (8, 27):
            raise ValueError(f"{path}: block {b} is neither HEX8 nor HEX27")
        conn.append(c[:, :8])
        b += 1
    cells = np.concatenate(conn, axis=0)[:, _EXO_TO_TENSOR]
    ss: Dict[int, np.ndarray] = {}
    if "ss_prop1" in v:
        ids = np.array(v["ss_prop1"][:], dtype=np.int64)
        for k, sid in enumerate(ids, start=1):
            el = np.array(v[f"elem_ss{k}"][:], dtype=np.int64) - 1
            sd = np.array(v[f"side_ss{k}"][:], dtype=np.int64)
            ss[int(sid)] = np.stack([el, np.array([_EXO_SIDE_TO_FACE[int(s)] for s in sd])], axis=1)
    node_sets = {}
    if "ns_prop1" in v:
        for k, sid in enumerate(np.array(v["ns_prop1"][:], dtype=np.int64), start=1):
            node_sets[int(sid)] = np.array(v[f"node_ns{k}"][:], dtype=np.int64) - 1
    f.close()
    used = np.unique(cells)                       # HEX27: keep the corner vertices only
    if used.size != coords.shape[0]:
        renum = np.full(coords.shape[0], -1, dtype=np.int64)
        renum[used] = np.arange(used.size)
        cells, coords = renum[cells], coords[used]
        node_sets = {sid: renum[ns][renum[ns] >= 0] for sid, ns in node_sets.items()}
    boundary = None
    if node_sets:                                   # faces owned by exactly one element, per local face
        allf = np.concatenate([np.sort(cells[:, [c for c in range(8) if ((c >> (f // 2)) & 1) == f % 2]], axis=1) for f in range(6)], axis=0)
        _, inv, cnt = np.unique(allf, axis=0, return_inverse=True, return_counts=True)
        boundary = (cnt[inv] == 1).reshape(6, cells.shape[0])
    for sid, ns in node_sets.items():
        inset = np.zeros(coords.shape[0], dtype=bool)
        inset[ns] = True
        faces = []
        for face in range(6):                       # local faces as in box_mesh: 0 x-, 1 x+, 2 y-, 3 y+, 4 z-, 5 z+
            axis, side = face // 2, face % 2
            corners = [c for c in range(8) if ((c >> axis) & 1) == side]
            el = np.nonzero(inset[cells[:, corners]].all(axis=1) & boundary[face])[0]
            faces.append(np.stack([el, np.full(el.size, face)], axis=1))
        ss.setdefault(sid, np.concatenate(faces, axis=0))
    mesh = HexMesh(coords, cells, ss, name=path.split("/")[-1])
    _fix_orientation(mesh)
    return mesh


def _fix_orientation(mesh: HexMesh):
    """Make every element right-handed (detJ > 0 at the centre) by mirroring in local z."""
    X = mesh.coords[mesh.cells]  # (ne, 8, 3)
    dx = (X[:, 1::2] - X[:, 0::2]).mean(axis=1)
    dy = (X[:, [2, 3, 6, 7]] - X[:, [0, 1, 4, 5]]).mean(axis=1)
    dz = (X[:, 4:] - X[:, :4]).mean(axis=1)
    det = np.einsum("ij,ij->i", np.cross(dx, dy), dz)
    bad = det < 0
    if bad.any():
        mesh.cells[bad] = mesh.cells[bad][:, [4, 5, 6, 7, 0, 1, 2, 3]]
        for sid, fs in mesh.side_sets.items():
            flip = bad[fs[:, 0]] & (fs[:, 1] >= 4)
            fs[flip, 1] = 9 - fs[flip, 1]


def save_mesh_npz(mesh: HexMesh, path: str):
    d = {"coords": mesh.coords, "cells": mesh.cells.astype(np.int32)}
    for sid, fs in mesh.side_sets.items():
        d[f"ss_{sid}"] = fs.astype(np.int32)
    np.savez_compressed(path, **d)


def load_mesh_npz(path: str) -> HexMesh:
    z = np.load(path)
    ss = {int(k[3:]): z[k].astype(np.int64) for k in z.files if k.startswith("ss_")}
    return HexMesh(z["coords"].astype(np.float64), z["cells"].astype(np.int64), ss, name=path.split("/")[-1])


# --------------------------------------------------------------------------
# Gauss-Lobatto nodes (reference coordinates of the solution nodes)
# --------------------------------------------------------------------------
def gll_nodes(P: int) -> np.ndarray:
    if P == 2:
        return np.array([-1.0, 1.0])
    inner = np.polynomial.legendre.Legendre.basis(P - 1).deriv().roots()
    x = np.concatenate([[-1.0], np.sort(inner.real), [1.0]])
    return 0.5 * (x - x[::-1])  # enforce symmetry


# --------------------------------------------------------------------------
# high-order numbering
# --------------------------------------------------------------------------
@dataclass
class DofMap:
    """Degree-p nodes of a mesh.  ``elem_nodes[e, n]`` is the node id of local tensor
    node n = a + P b + P^2 c (x fastest) -- the closure order of setupdm.c:194."""
    p: int
    nnodes: int
    elem_nodes: np.ndarray        # (ne, P^3) int32
    node_keys: np.ndarray         # (nnodes, 7) int64 partition-independent topological keys
    node_coords: np.ndarray       # (nnodes, 3)
    ncomp: int = 3

    @property
    def P(self) -> int:
        return self.p + 1

    @property
    def lsize(self) -> int:
        return self.nnodes * self.ncomp

    def offsets(self) -> np.ndarray:
        """Per-node offset of component 0 in the interlaced L-vector (compstride 1),
        as CreateRestrictionPlex hands them to CeedElemRestrictionCreate (:235)."""
        return (self.elem_nodes.astype(np.int64) * self.ncomp).astype(np.int32)


def _local_face_nodes(P: int, face: int) -> np.ndarray:
    a = np.arange(P)
    A, B = np.meshgrid(a, a, indexing="ij")
    fixed = 0 if face % 2 == 0 else P - 1
    if face < 2:
        i, j, k = np.full_like(A, fixed), A, B
    elif face < 4:
        i, j, k = A, np.full_like(A, fixed), B
    else:
        i, j, k = A, B, np.full_like(A, fixed)
    return (i + P * j + P * P * k).ravel()


def build_dofmap(mesh: HexMesh, p: int, ncomp: int = 3, locality_order: bool = True) -> DofMap:
    P = p + 1
    ne = mesh.nelem
    cells = mesh.cells
    gcells = mesh.gid()[cells]       # global vertex ids: canonical orientations agree across ranks
    V = mesh.nvert
    m = p - 1                        # interior nodes per edge
    ids = np.empty((ne, P, P, P), dtype=np.int64)     # [e, c(z), b(y), a(x)]
    keys = np.zeros((ne, P, P, P, 7), dtype=np.int64)
    corner = lambda i, j, k: i + 2 * j + 4 * k

    # vertices
    for k in (0, 1):
        for j in (0, 1):
            for i in (0, 1):
                c = corner(i, j, k)
                ids[:, k * p, j * p, i * p] = cells[:, c]
                keys[:, k * p, j * p, i * p, 0] = 0
                keys[:, k * p, j * p, i * p, 1] = gcells[:, c]
    nE = nF = 0
    if m > 0:
        t = np.arange(1, p)
        # ---- edges: 12 per element --------------------------------------
        edge_list = []  # (axis, fixed (u,v) bits)
        for axis in range(3):
            for u in (0, 1):
                for v in (0, 1):
                    edge_list.append((axis, u, v))
        ev0 = np.empty((ne, 12), dtype=np.int64)
        ev1 = np.empty((ne, 12), dtype=np.int64)
        for n, (axis, u, v) in enumerate(edge_list):
            bits0 = [0, 0, 0]
            others = [d for d in range(3) if d != axis]
            bits0[others[0]], bits0[others[1]] = u, v
            bits1 = list(bits0)
            bits1[axis] = 1
            ev0[:, n] = corner(*bits0)
            ev1[:, n] = corner(*bits1)
        g0 = np.take_along_axis(gcells, ev0, axis=1)
        g1 = np.take_along_axis(gcells, ev1, axis=1)
        lo, hi = np.minimum(g0, g1), np.maximum(g0, g1)
        pair = np.stack([lo.ravel(), hi.ravel()], axis=1)
        uniq_e, eid = np.unique(pair, axis=0, return_inverse=True)
        eid = eid.reshape(ne, 12)
        nE = uniq_e.shape[0]
        for n, (axis, u, v) in enumerate(edge_list):
            fwd = (g0[:, n] < g1[:, n])[:, None]
            pos = np.where(fwd, t[None, :], p - t[None, :])            # (ne, m) position from the min vertex
            nid = V + eid[:, n][:, None] * m + (pos - 1)
            others = [d for d in range(3) if d != axis]
            idx = [None, None, None]
            idx[axis] = t
            idx[others[0]] = u * p
            idx[others[1]] = v * p
            sl = (slice(None), idx[2], idx[1], idx[0])
            ids[sl] = nid
            keys[sl + (0,)] = 1
            keys[sl + (1,)] = lo[:, n][:, None]
            keys[sl + (2,)] = hi[:, n][:, None]
            keys[sl + (5,)] = pos
        # ---- faces: 6 per element ---------------------------------------
        fc = np.empty((ne, 6, 4), dtype=np.int64)  # corners in local (s,t) order: 00,10,01,11
        for f in range(6):
            axis, side = f // 2, f % 2
            others = [d for d in range(3) if d != axis]
            for q, (s_, t_) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
                bits = [0, 0, 0]
                bits[axis] = side
                bits[others[0]], bits[others[1]] = s_, t_
                fc[:, f, q] = gcells[:, corner(*bits)]
        srt = np.sort(fc, axis=2).reshape(ne * 6, 4)
        uniq_f, fid = np.unique(srt, axis=0, return_inverse=True)
        fid = fid.reshape(ne, 6)
        nF = uniq_f.shape[0]
        S, T = np.meshgrid(t, t, indexing="ij")      # local (s,t) interior positions
        S, T = S.ravel(), T.ravel()
        for f in range(6):
            axis, side = f // 2, f % 2
            others = [d for d in range(3) if d != axis]
            c4 = fc[:, f, :]
            o = np.argmin(c4, axis=1)                                        # origin corner
            ns = np.take_along_axis(c4, (o ^ 1)[:, None], axis=1)[:, 0]      # neighbour along s
            nt = np.take_along_axis(c4, (o ^ 2)[:, None], axis=1)[:, 0]      # neighbour along t
            swap = (nt < ns)[:, None]
            srel = np.where(((o & 1) == 0)[:, None], S[None, :], p - S[None, :])
            trel = np.where(((o & 2) == 0)[:, None], T[None, :], p - T[None, :])
            s2 = np.where(swap, trel, srel)
            t2 = np.where(swap, srel, trel)
            nid = V + nE * m + fid[:, f][:, None] * m * m + (s2 - 1) * m + (t2 - 1)
            idx = [None, None, None]
            idx[axis] = np.full(S.shape, side * p)
            idx[others[0]] = S
            idx[others[1]] = T
            sl = (slice(None), idx[2], idx[1], idx[0])
            ids[sl] = nid
            keys[sl + (0,)] = 2
            sq = np.sort(c4, axis=1)
            for q in range(4):
                keys[sl + (1 + q,)] = sq[:, q][:, None]
            keys[sl + (5,)] = s2
            keys[sl + (6,)] = t2
        # ---- interiors ---------------------------------------------------
        C_, B_, A_ = np.meshgrid(t, t, t, indexing="ij")
        loc = ((C_ - 1) * m + (B_ - 1)) * m + (A_ - 1)
        base = V + nE * m + nF * m * m
        sl = (slice(None), C_.ravel(), B_.ravel(), A_.ravel())
        ids[sl] = base + np.arange(ne)[:, None] * m ** 3 + loc.ravel()[None, :]
        keys[sl + (0,)] = 3
        # element identity must be global for keys: use the element's min global vertex + its sorted corners hash
        keys[sl + (1,)] = np.sort(gcells, axis=1)[:, 0][:, None]
        keys[sl + (2,)] = np.sort(gcells, axis=1)[:, 7][:, None]
        keys[sl + (3,)] = np.sort(gcells, axis=1)[:, 3][:, None]
        keys[sl + (5,)] = loc.ravel()[None, :]
    nn = V + nE * m + nF * m * m + ne * m ** 3
    flat = ids.reshape(ne, P ** 3)
    kflat = keys.reshape(ne * P ** 3, 7)
    if locality_order:
        # shell nodes (vertices, edges, faces: shared between elements) in first-touch order of the element sweep, so an
        # element's new nodes are contiguous; then the element-INTERIOR nodes, [element][k][j][i]: one contiguous run per
        # element, which the fused kernel reads and writes as whole lines (FusedGradArgs::direct)
        uniq, first = np.unique(flat.ravel(), return_index=True)
        assert uniq.size == nn, (uniq.size, nn)
        n_int = ne * max(m, 0) ** 3
        shell = uniq < nn - n_int                     # raw ids: interiors are the last ne * m^3
        order = np.concatenate([np.flatnonzero(shell)[np.argsort(first[shell], kind="stable")], np.flatnonzero(~shell)])
        new = np.empty(nn, dtype=np.int64)
        new[uniq[order]] = np.arange(nn)
        flat = new[flat]
        first_sorted = first[order]
    else:
        _, first = np.unique(flat.ravel(), return_index=True)
        first_sorted = first
    node_keys = kflat[first_sorted]
    # node coordinates by the trilinear map of the GLL reference positions
    xi = 0.5 * (gll_nodes(P) + 1.0)
    N1 = np.stack([1 - xi, xi], axis=0)              # (2, P)
    X = mesh.coords[cells]                            # (ne, 8, 3)
    w = np.einsum("kc,jb,ia->kjicba", N1, N1, N1).reshape(8, P ** 3)  # corner c=i+2j+4k; node a+P b+P^2 c
    # reorder: w[corner, node]; corner index = i + 2j + 4k -> axes (k,j,i)
    xn = np.einsum("cn,ecd->end", w, X)
    node_coords = np.empty((nn, 3))
    node_coords[flat.ravel()] = xn.reshape(-1, 3)
    return DofMap(p, nn, flat.astype(np.int32), node_keys, node_coords, ncomp)


def side_set_nodes(mesh: HexMesh, dm: DofMap, side_ids) -> np.ndarray:
    """Sorted unique node ids lying on the given side sets."""
    out = []
    for sid in side_ids:
        fs = mesh.side_sets[sid]
        for f in range(6):
            el = fs[fs[:, 1] == f, 0]
            if el.size:
                out.append(dm.elem_nodes[el][:, _local_face_nodes(dm.P, f)].ravel())
    return np.unique(np.concatenate(out)) if out else np.zeros(0, dtype=np.int64)


# _local_face_nodes lists a face's nodes with its SECOND in-face direction fastest: (y, z) on the x-faces, (x, z) on the y-faces, (x, y) on
# the z-faces.  With xi the fastest and eta the other direction, X_xi x X_eta of a right-handed element is then z x y = -x, z x x = +y and
# y x x = -z: outward on the local faces 0 (x-), 3 (y+), 4 (z-), inward on 1, 2, 5, whose lists are transposed.
_FACE_FLIP = (False, True, True, False, False, True)


def side_set_faces(mesh: HexMesh, dm: DofMap, side_ids) -> np.ndarray:
    """(nface, P^2) node ids of the faces of the given side sets, xi fastest, (xi, eta) ordered so that X_xi x X_eta points out of the
    body (elements are right-handed, ``_fix_orientation``: the order depends on the local face alone).  Faces come in side-set
    order, then element order."""
    P = dm.P
    loc = []
    for f in range(6):
        n = _local_face_nodes(P, f).reshape(P, P)
        loc.append((n.T if _FACE_FLIP[f] else n).ravel())
    loc = np.stack(loc)                                               # (6, P^2) local nodes of every local face
    out = []
    for sid in side_ids:
        fs = np.asarray(mesh.side_sets[sid], dtype=np.int64).reshape(-1, 2)
        fs = fs[np.argsort(fs[:, 0], kind="stable")]
        out.append(dm.elem_nodes[fs[:, 0][:, None], loc[fs[:, 1]]].astype(np.int64))
    return np.concatenate(out, axis=0) if out else np.zeros((0, P * P), dtype=np.int64)


def boundary_nodes(mesh: HexMesh, dm: DofMap) -> np.ndarray:
    """Nodes on faces that belong to exactly one element of this (sub-)mesh: the whole
    boundary -- the "marker" label of -test mode (setupdm.c:160-170) -- and, on a
    partition, also the interface candidates."""
    g = mesh.gid()[mesh.cells]
    faces = []
    for f in range(6):
        axis, side = f // 2, f % 2
        cs = [c for c in range(8) if ((c >> axis) & 1) == side]
        faces.append(np.sort(g[:, cs], axis=1))
    allf = np.concatenate(faces, axis=0)
    _, inv, cnt = np.unique(allf, axis=0, return_inverse=True, return_counts=True)
    single = (cnt[inv] == 1).reshape(6, mesh.nelem)
    out = []
    for f in range(6):
        el = np.nonzero(single[f])[0]
        if el.size:
            out.append(dm.elem_nodes[el][:, _local_face_nodes(dm.P, f)].ravel())
    return np.unique(np.concatenate(out))


def dirichlet_mask(dm: DofMap, nodes: np.ndarray) -> np.ndarray:
    """uint8 mask over the L-vector: 1 on constrained dofs (all components of ``nodes``)."""
    m = np.zeros((dm.nnodes, dm.ncomp), dtype=np.uint8)
    m[nodes] = 1
    return m.ravel()


# --------------------------------------------------------------------------
# partitioning (element-wise, overlap 0: setupdm.c:57-64)
# --------------------------------------------------------------------------
def partition_slabs(mesh: HexMesh, nparts: int, axis: int = 2) -> List[np.ndarray]:
    """Contiguous equal-count chunks of elements sorted by centroid along ``axis``."""
    cen = mesh.coords[mesh.cells].mean(axis=1)[:, axis]
    order = np.argsort(cen, kind="stable")
    return [np.sort(ch) for ch in np.array_split(order, nparts)]


def submesh(mesh: HexMesh, elems: np.ndarray) -> HexMesh:
    cells = mesh.cells[elems]
    used, inv = np.unique(cells.ravel(), return_inverse=True)
    emap = -np.ones(mesh.nelem, dtype=np.int64)
    emap[elems] = np.arange(elems.size)
    ss = {}
    for sid, fs in mesh.side_sets.items():
        keep = emap[fs[:, 0]] >= 0
        ss[sid] = np.stack([emap[fs[keep, 0]], fs[keep, 1]], axis=1)
    return HexMesh(mesh.coords[used], inv.reshape(cells.shape).astype(np.int64), ss,
                   vertex_gid=mesh.gid()[used], name=mesh.name + f"[{elems.size}e]")


def reorder_elements_first(mesh: HexMesh, first: np.ndarray) -> HexMesh:
    """Same mesh with the elements flagged in ``first`` (bool per element) moved to the front, order
    otherwise preserved (split-phase apply: interface-touching elements lead)."""
    first = np.asarray(first, dtype=bool)
    perm = np.concatenate([np.nonzero(first)[0], np.nonzero(~first)[0]])
    inv = np.empty_like(perm); inv[perm] = np.arange(perm.size)
    ss = {sid: np.stack([inv[fs[:, 0]], fs[:, 1]], axis=1) if len(fs) else fs for sid, fs in mesh.side_sets.items()}
    return HexMesh(mesh.coords, mesh.cells[perm], ss, vertex_gid=mesh.vertex_gid, name=mesh.name + "[reordered]")


def hex_rotations():
    """The 24 orientation-preserving relabellings of a hexahedron's local axes: (perm, sign) with new axis d = sign[d] x old axis
    perm[d] and det = +1; for each the old tensor-order vertex index of every new one and the old local face of every new one."""
    import itertools
    out = []
    for perm in itertools.permutations(range(3)):
        par = 1 if perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1)) else -1
        for sg in itertools.product((1, -1), repeat=3):
            if par * sg[0] * sg[1] * sg[2] != 1:
                continue
            vmap = np.zeros(8, dtype=np.int64)
            for c in range(8):
                old = 0
                for d in range(3):
                    b = (c >> d) & 1
                    old |= (b if sg[d] > 0 else 1 - b) << perm[d]
                vmap[c] = old
            fmap = np.array([2 * perm[f // 2] + ((f % 2) if sg[f // 2] > 0 else 1 - (f % 2)) for f in range(6)], dtype=np.int64)
            out.append((vmap, fmap))
    return out


def scramble_mesh(mesh: HexMesh, seed: int = 0, order: bool = True, orient: bool = False) -> HexMesh:
    """The same mesh as an unstructured generator might hand it over: ``order`` -- elements and vertices in random order (no
    locality left in either numbering); ``orient`` -- every element's local axes relabelled by a random one of the 24 rotations
    (neighbours no longer agree on which local direction is which: no common sweep direction, no aligned faces).  Geometry, side
    sets and the discrete problem are unchanged."""
    rng = np.random.default_rng(seed)
    cells, coords, gid = mesh.cells.copy(), mesh.coords, mesh.gid()
    ss = {sid: np.array(fs, dtype=np.int64).reshape(-1, 2).copy() for sid, fs in mesh.side_sets.items()}
    if orient:
        rots = hex_rotations()
        which = rng.integers(0, len(rots), mesh.nelem)
        vm = np.stack([r[0] for r in rots])[which]                  # (ne, 8): old vertex slot of every new slot
        cells = np.take_along_axis(cells, vm, axis=1)
        inv_f = np.stack([np.argsort(r[1]) for r in rots])          # old face -> new face
        for sid, fs in ss.items():
            if len(fs):
                fs[:, 1] = inv_f[which[fs[:, 0]], fs[:, 1]]
    if order:
        vperm = rng.permutation(mesh.nvert)                          # new vertex v is old vertex vperm[v]
        vinv = np.empty_like(vperm); vinv[vperm] = np.arange(vperm.size)
        coords, gid, cells = coords[vperm], gid[vperm], vinv[cells]
        eperm = rng.permutation(mesh.nelem)
        einv = np.empty_like(eperm); einv[eperm] = np.arange(eperm.size)
        cells = cells[eperm]
        for sid, fs in ss.items():
            if len(fs):
                fs[:, 0] = einv[fs[:, 0]]
    return HexMesh(coords, cells.astype(np.int64), ss, vertex_gid=gid if (order or mesh.vertex_gid is not None) else None,
                   name=mesh.name + "[scrambled" + (" order" if order else "") + (" orientation" if orient else "") + "]")


def reorder_elements_locality(mesh: HexMesh, bits: int = 10) -> HexMesh:
    """Elements sorted along a Morton (Z-order) curve through their centroids: what the step before the path can do for a mesh whose
    generator numbered its elements without locality ("enables cache-friendly element / dof ordering").  The
    high-order nodes are numbered in first-touch order over the element sweep (build_dofmap), so consecutive elements then share
    their nodes through one L2 and their E-vector blocks sit next to each other.  Geometry, side sets and the problem are unchanged."""
    cen = mesh.coords[mesh.cells].mean(axis=1)
    lo, hi = cen.min(axis=0), cen.max(axis=0)
    q = np.minimum(((cen - lo) / np.maximum(hi - lo, 1e-300) * (1 << bits)).astype(np.uint64), (1 << bits) - 1)
    code = np.zeros(mesh.nelem, dtype=np.uint64)
    for b in range(bits):
        for d in range(3):
            code |= ((q[:, d] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + d)
    perm = np.argsort(code, kind="stable")
    inv = np.empty_like(perm); inv[perm] = np.arange(perm.size)
    ss = {sid: (np.stack([inv[np.asarray(fs)[:, 0]], np.asarray(fs)[:, 1]], axis=1) if len(fs) else np.asarray(fs)) for sid, fs in mesh.side_sets.items()}
    return HexMesh(mesh.coords, mesh.cells[perm], ss, vertex_gid=mesh.vertex_gid, name=mesh.name + "[morton]")


def refine_swept_mesh(mesh: HexMesh, nz: int, tol: float = 1e-6) -> HexMesh:
    """A swept (extruded along z) HEX8 mesh re-made with its CROSS-SECTION refined 2 x 2 and ``nz`` uniform layers: the unstructured
    cross-section an external generator paved (e.g. the 468 CUBIT quads of the reference's cylinder8_44928e_2ss_us.exo) at another size --
    a stand-in for the absent cylinder8_99Ke_4ss_us.exo that keeps a REAL unstructured topology (468 x 4 quads x 53 layers = 99 216 hexes).
    New vertices on edges whose two ends lie on one circle about the z axis are put on that circle (the annulus keeps its shape).  Elements
    are numbered layer by layer, within a layer in the generator's order (the four children of a quad together); side sets: the original
    ids of the two end caps (a set ALL of whose face vertices lie at z0 / z1), local faces k- / k+; lateral side sets are dropped with a warning."""
    z = mesh.coords[:, 2]
    z0, z1 = z.min(), z.max()
    bottom = np.abs(z - z0) < tol * max(1.0, z1 - z0)
    quads = []                                            # cross-section quads, tensor order [v00, v10, v01, v11], from the elements on the bottom cap
    for cell in mesh.cells:
        onb = bottom[cell]
        if onb.sum() != 4:
            continue
        for d in range(3):                                # the local direction of the sweep: the bottom vertices are one side of it
            side0 = [c for c in range(8) if not (c >> d) & 1]
            side1 = [c for c in range(8) if (c >> d) & 1]
            for side in (side0, side1):
                if onb[side].all():
                    quads.append(cell[side])
    quads = np.array(quads, dtype=np.int64)
    assert len(quads) > 0 and mesh.nelem % len(quads) == 0, "not a swept mesh with a flat bottom cap"
    used, inv = np.unique(quads.ravel(), return_inverse=True)
    q = inv.reshape(-1, 4)
    xy = mesh.coords[used, :2]
    # orientation: counter-clockwise in (x, y) so that (i, j, z) is right-handed
    a, b = xy[q[:, 1]] - xy[q[:, 0]], xy[q[:, 2]] - xy[q[:, 0]]
    flip = (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]) < 0
    q[flip] = q[flip][:, [1, 0, 3, 2]]
    nv = len(xy)
    edges = {}
    pts = [xy]
    def mid(u, v):
        key = (min(u, v), max(u, v))
        if key not in edges:
            m = 0.5 * (xy[u] + xy[v])
            ru, rv = np.hypot(*xy[u]), np.hypot(*xy[v])
            if abs(ru - rv) < 1e-9 * max(ru, 1.0) and np.hypot(*m) > 0:       # both ends on one circle: stay on it
                m = m * (ru / np.hypot(*m))
            edges[key] = nv + len(edges)
            pts.append(m[None, :])
        return edges[key]
    child = []
    centres = []
    for v00, v10, v01, v11 in q:
        e0, e1, e2, e3 = mid(v00, v10), mid(v01, v11), mid(v00, v01), mid(v10, v11)   # bottom, top, left, right
        centres.append((v00, v10, v01, v11, e0, e1, e2, e3))
    nmid = len(edges)
    mids = np.concatenate(pts[1:], axis=0) if nmid else np.zeros((0, 2))
    cpts = []
    for n, (v00, v10, v01, v11, e0, e1, e2, e3) in enumerate(centres):
        cc = nv + nmid + n
        cpts.append(0.25 * (mids[e0 - nv] + mids[e1 - nv] + mids[e2 - nv] + mids[e3 - nv]))
        child += [[v00, e0, e2, cc], [e0, v10, cc, e3], [e2, cc, v01, e1], [cc, e3, e1, v11]]
    xy2 = np.concatenate([xy, mids, np.array(cpts)], axis=0)
    q2 = np.array(child, dtype=np.int64)
    n2, nq = len(xy2), len(q2)
    zs = np.linspace(z0, z1, nz + 1)
    coords = np.concatenate([np.column_stack([xy2, np.full(n2, zz)]) for zz in zs], axis=0)
    cells = np.concatenate([np.concatenate([q2 + k * n2, q2 + (k + 1) * n2], axis=1) for k in range(nz)], axis=0)
    ss = {}
    caps, dropped = {}, []
    ztol = tol * max(1.0, z1 - z0)
    for sid, fs in mesh.side_sets.items():                 # which original id is which end cap: EVERY vertex of EVERY face of the set at z0 (z1)
        fs = np.asarray(fs)
        if not len(fs):
            continue
        zf = np.concatenate([z[mesh.cells[fs[fs[:, 1] == f, 0]][:, [c for c in range(8) if ((c >> (f // 2)) & 1) == f % 2]]].ravel()
                             for f in range(6) if (fs[:, 1] == f).any()])
        if np.all(np.abs(zf - z0) < ztol) and "lo" not in caps:
            caps["lo"] = sid
        elif np.all(np.abs(zf - z1) < ztol) and "hi" not in caps:
            caps["hi"] = sid
        else:
            dropped.append(sid)                           # a lateral surface (or a second set on a cap): not carried over
    if dropped:
        import warnings
        warnings.warn(f"refine_swept_mesh: side sets {sorted(dropped)} are not end caps of the sweep and are not carried over to the refined mesh")
    e = np.arange(nq)
    if "lo" in caps:
        ss[caps["lo"]] = np.stack([e, np.full(nq, 4)], axis=1)
    if "hi" in caps:
        ss[caps["hi"]] = np.stack([e + (nz - 1) * nq, np.full(nq, 5)], axis=1)
    out = HexMesh(coords, cells, ss, name=mesh.name + f"[cross-section 2x2, {nz} layers]")
    _fix_orientation(out)
    return out


def key_bytes(keys: np.ndarray) -> np.ndarray:
    """Topological keys as fixed-size byte strings (hashable / sortable across ranks)."""
    k = np.ascontiguousarray(keys, dtype=np.int64)
    return k.view(np.dtype((np.void, k.shape[1] * 8))).ravel()
