"""The launch arithmetic of the fused kernel restated as data, and the meshes on which its persistent group loop runs several rounds
(tests/test_fused_rounds.py holds the arithmetic on the CPU, tests/test_fused_rounds_gpu.py runs the meshes; no tests in here).

The product: csrc/kernels.hpp (pencil_group_elems, pencil_lds_bytes, pencil_waves_per_cu), the grid of launch_fused_pencil_t
(kernel_fused_pencil.hpp) and the work list at the top of kernel_fused_pencil_body.hpp (nxcd, wrank, wper, gend, grp += wper).  A
one-wave workgroup walks a strided list of element groups; a ROUND is one iteration of that walk.  The sweep of
tests/test_kernel_matrix_gpu.py launches at most as many groups as the grid holds workgroups (the launcher caps the grid at the group
count), so every workgroup there runs one round; the meshes below, under CEED_MI355X_PENCIL_WAVES=1 on a 256-CU device, give the low
wave ranks of every XCD chunk three rounds -- a first, a middle and a last iteration -- and the other ranks two."""
import functools

import numpy as np

GEO_NCOEF = 21                       # kernels.hpp: doubles per element of the trilinear map's coefficients
PENCIL_MINW = 2                      # kernels.hpp: waves per SIMD the register allocation is held to
LDS_PER_CU = 160 * 1024


def pencil_group_elems(Q):
    return 8 if Q <= 2 else (4 if Q <= 4 else (2 if Q == 5 else 1))


def pencil_lds_bytes(Q):
    return (pencil_group_elems(Q) * (9 * Q ** 3 + (5 if Q == 5 else 1) + GEO_NCOEF) + 2 * Q) * 8


def pencil_waves_per_cu(Q):
    by_lds = LDS_PER_CU // pencil_lds_bytes(Q)
    return 1 if by_lds < 1 else min(by_lds, 4 * PENCIL_MINW)


def ngroups_of(nelem, Q):
    E = pencil_group_elems(Q)
    return (nelem + E - 1) // E


def grid_of(ngroups, Q, ncu, waves_per_cu=0):
    """Workgroups of the persistent launch (FusedLaunch::wave_groups == 0): CUs x waves per CU, at most one per group."""
    return min(ncu * (waves_per_cu if waves_per_cu > 0 else pencil_waves_per_cu(Q)), ngroups)


def walk(ngroups, grid):
    """Per workgroup b = 0 .. grid - 1 the groups it visits, in order (a range): the work list of the kernel body."""
    grp, gend, wper = walk_bounds(ngroups, grid)
    return [range(a, b, wper) for a, b in zip(grp.tolist(), gend.tolist())]


def walk_bounds(ngroups, grid):
    """(grp, gend, wper) of every workgroup, as arrays over blockIdx.x: block b serves chunk b % nxcd with wave rank b / nxcd; it starts at
    grp = chunk begin + wrank and goes on by grp += wper while grp < gend (grp >= gend at the start: `if (grp >= gend) return`)."""
    b = np.arange(grid, dtype=np.int64)
    nxcd = 8 if grid % 8 == 0 else 1
    wrank, wper, chunk = b // nxcd, grid // nxcd, (ngroups + nxcd - 1) // nxcd
    return (b % nxcd) * chunk + wrank, np.minimum(ngroups, (b % nxcd + 1) * chunk), wper


def rounds(nelem, Q, ncu, waves_per_cu=0):
    """Per workgroup the list of groups it visits in a whole launch of `nelem` elements at Q points per direction on `ncu` CUs;
    waves_per_cu > 0: CEED_MI355X_PENCIL_WAVES."""
    ng = ngroups_of(nelem, Q)
    return [list(r) for r in walk(ng, grid_of(ng, Q, ncu, waves_per_cu))]


def chunk_sizes(ngroups, grid):
    """Groups of each XCD chunk (one chunk where the grid is no multiple of 8)."""
    nxcd = 8 if grid % 8 == 0 else 1
    chunk = (ngroups + nxcd - 1) // nxcd
    return [max(0, min(ngroups, (c + 1) * chunk) - c * chunk) for c in range(nxcd)]


def round_of_group(lists, ngroups):
    """group -> the round (position in its workgroup's list) it is reached in; -1 for a group no workgroup visits."""
    r = np.full(ngroups, -1, dtype=np.int64)
    for gl in lists:
        for k, g in enumerate(gl):
            r[g] = k
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# the meshes: the smallest sizes that give three rounds on 256 CUs with one wave per CU (not the workload's size)
# ---------------------------------------------------------------------------------------------------------------------------------
# (The Q = 2 cylinder: 17 x 17 elements per z layer, as the box.  A cylinder of 5 x 51 x 17, the same 4335 elements, has end layers of 255
# elements = groups 0 .. 31 and 510 .. 541: exactly the first round of chunk 0 and nothing of the first round of the last chunk, so side
# 998 would own no element of a round >= 1 and side 999 none of round 0 -- the last condition of describe() below.)
SIZES = {2: ((17, 17, 15), (17, 17, 15)), 3: ((13, 13, 13), (13, 13, 13)), 4: ((13, 13, 13), (13, 13, 13)), 5: ((9, 11, 11), (3, 33, 11)),
         6: ((7, 9, 9), (3, 21, 9)), 7: ((7, 9, 9), (3, 21, 9)), 8: ((7, 9, 9), (3, 21, 9))}      # Q -> box (nx, ny, nz), cylinder (nr, nth, nz)
SIZE_CLASSES = {"Q2": 2, "Q3-4": 3, "Q5": 5, "Q6-8": 6}          # size class -> one Q of it
MESHES = ("general", "affine", "swept0", "swept1", "swept2")
SWEPT_PERM = {"swept0": [1, 2, 0], "swept1": [2, 0, 1], "swept2": [0, 1, 2]}     # the sweep (z) along reference direction 0, 1, 2


def nelem_of(Q):
    box, cyl = SIZES[Q]
    assert int(np.prod(box)) == cyl[0] * cyl[1] * cyl[2]
    return int(np.prod(box))


def clamped_sides(meshname):
    """The two opposite sides the sweep clamps: the first and the last elements in element order."""
    return [1, 2] if meshname in ("general", "affine") else [998, 999]


@functools.lru_cache(maxsize=8)
def rounds_mesh(meshname, Q):
    """(mesh, clamped side sets) of the sweep: `general` every vertex moved, `affine` a sheared box, `swept*` a hollow cylinder with the
    sweep along each reference direction."""
    from ceedpetscsolid_amd.mesh import box_mesh, hollow_cylinder_mesh
    from test_gpu_parity import _relabel_axes, distorted_box
    from test_kernel_matrix_gpu import SHEAR
    box, cyl = SIZES[Q]
    if meshname == "general":
        m = distorted_box(*box, seed=2, amp=0.2)
    elif meshname == "affine":
        m = box_mesh(*box)
        m.coords = m.coords @ SHEAR.T + np.array([0.3, -0.1, 0.2])
    else:
        base = hollow_cylinder_mesh(*cyl)
        m = base if meshname == "swept2" else _relabel_axes(base, SWEPT_PERM[meshname])
    assert m.nelem == nelem_of(Q)
    return m, clamped_sides(meshname)


def side_elements(meshname, Q):
    """side set -> its elements, from the sizes alone (box_mesh and hollow_cylinder_mesh number the elements x / r fastest, z slowest;
    sides 1, 998 are the first z layer, 2, 999 the last)."""
    box, cyl = SIZES[Q]
    n = box if meshname in ("general", "affine") else cyl
    layer, ne = n[0] * n[1], n[0] * n[1] * n[2]
    lo, hi = clamped_sides(meshname)
    return {lo: np.arange(layer), hi: np.arange(ne - layer, ne)}


# ---------------------------------------------------------------------------------------------------------------------------------
# what a launch of one of these meshes must look like for the loop-carried path to run
# ---------------------------------------------------------------------------------------------------------------------------------
def describe(Q, ncu, waves_per_cu, meshname="general"):
    """The figures of a whole launch of the Q mesh: groups, grid, chunks, the histogram of rounds per workgroup, and the conditions of
    the sweep one by one (`conditions`: name -> bool)."""
    nelem, E = nelem_of(Q), pencil_group_elems(Q)
    ng = ngroups_of(nelem, Q)
    grid = grid_of(ng, Q, ncu, waves_per_cu)
    lists = walk(ng, grid)
    n_rounds = [len(gl) for gl in lists]
    hist = {k: n_rounds.count(k) for k in sorted(set(n_rounds))}
    chunks = chunk_sizes(ng, grid)
    rg = round_of_group(lists, ng)
    cond = {
        "a workgroup runs three rounds": max(n_rounds) >= 3,
        "a workgroup runs exactly two rounds": 2 in hist,
        "the last chunk is shorter than the others": len(chunks) > 1 and all(chunks[-1] < c for c in chunks[:-1]),
    }
    if E > 1:
        assert nelem % E != 0
        cond["the partial group is reached in a round >= 1"] = bool(rg[ng - 1] >= 1)
    for side, elems in side_elements(meshname, Q).items():
        r = rg[elems // E]
        cond[f"side {side} owns elements of a round >= 1"] = bool((r >= 1).any())
        cond[f"side {side} owns elements of round 0"] = bool((r == 0).any())
    return {"Q": Q, "nelem": nelem, "E": E, "ngroups": ng, "grid": grid, "nxcd": len(chunks), "chunks": chunks, "hist": hist, "conditions": cond}


def loop_runs(ncu, Q, meshname="general"):
    """(ok, message): with one persistent wave per CU the launch of the Q mesh on `ncu` CUs meets every condition of the sweep."""
    d = describe(Q, ncu, 1, meshname)
    missed = [k for k, v in d["conditions"].items() if not v]
    return not missed, f"Q={Q} {meshname} on {ncu} CUs: {d['ngroups']} groups, grid {d['grid']}, chunks {d['chunks']}, rounds {d['hist']}: not met: {missed}"
