#!/usr/bin/env python3
"""CPU model of what k_assemble reads (profiles/assemble_row_code.txt): for a mesh and a degree, from the repository's own
dof map and shell ranks, rows in ascending node order as build_csr makes them --

  rows      shell rows of the transpose map, contributors, bytes of the plain map (rowptr 4 + node_off 4 + flags 1 + cols 4 per
            contributor) and of the coded one (pos0 4 + sid 2 + node_off 4 + flags 1) per row;
  lines     distinct 128-byte lines of the E-vector ([element][shell rank][3] doubles) that a block of consecutive rows touches,
            over the useful bytes, per block size (256 rows = one workgroup of k_assemble);
  runs      mean length of the runs of consecutive rows whose contributors all advance by one record (what a run descriptor could code);
  stencils  distinct (contributor count, distances from the first contributor) patterns -- the table of csrc/row_code.hpp.

    python tools/assemble_line_model.py --nr 10 --nth 110 --nz 8 --degree 4        (the figures of the records)
    python tools/assemble_line_model.py --workload box --nr 3 --nth 3 --nz 3 --degree 2

NumPy only; no GPU, no library build."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceedpetscsolid_amd.mesh import box_mesh, build_dofmap, hollow_cylinder_mesh  # noqa: E402

LINE = 128      # bytes of a cache line
RECORD = 24     # bytes of one contributor: three doubles


def shell_rank_table(P):
    """element-local node -> rank among the shell nodes (kernels.hpp: node_shell_rank, face-major), -1 for element-interior nodes"""
    m = P - 2
    rank = np.full(P * P * P, -1, dtype=np.int64)
    for n in range(P * P * P):
        i, j, k = n % P, (n // P) % P, n // (P * P)
        if 0 < i < P - 1 and 0 < j < P - 1 and 0 < k < P - 1:
            continue
        if k == 0:
            r = j * P + i
        elif k == P - 1:
            r = P * P + j * P + i
        elif j == 0:
            r = 2 * P * P + (k - 1) * P + i
        elif j == P - 1:
            r = 2 * P * P + P * m + (k - 1) * P + i
        elif i == 0:
            r = 2 * P * P + 2 * P * m + (k - 1) * m + (j - 1)
        else:
            r = 2 * P * P + 2 * P * m + m * m + (k - 1) * m + (j - 1)
        rank[n] = r
    return rank


def transpose_map(elem_nodes, P):
    """(rowptr, cols) of the shell map: rows in ascending node order, a row's contributors in element order"""
    ne, P3 = elem_nodes.shape
    rank = shell_rank_table(P)
    shell = np.flatnonzero(rank >= 0) if P > 2 else np.arange(P3)
    nshell = shell.size
    node = elem_nodes[:, shell].ravel()
    pos = (np.arange(ne)[:, None] * nshell + (rank[shell] if P > 2 else shell)[None, :]).ravel()
    order = np.lexsort((pos, node))                      # by node, then by position: element order within a node
    node, pos = node[order], pos[order]
    starts = np.flatnonzero(np.r_[True, node[1:] != node[:-1]])
    rowptr = np.r_[starts, node.size].astype(np.int64)
    return rowptr, pos          # (position order IS element order: a conforming mesh holds a node once per element)


def lines_per_useful(rowptr, cols, block):
    nrows = rowptr.size - 1
    lines = 0
    for r0 in range(0, nrows, block):
        c = cols[rowptr[r0]:rowptr[min(r0 + block, nrows)]]
        first, last = c * RECORD // LINE, (c * RECORD + RECORD - 1) // LINE
        lines += np.unique(np.r_[first, last]).size
    return lines * LINE / (cols.size * RECORD)


def run_lengths(rowptr, cols):
    """mean length of maximal runs of consecutive rows with equal counts whose contributors each advance by one record"""
    nrows = rowptr.size - 1
    cnt = np.diff(rowptr)
    runs, r = 0, 0
    while r < nrows:
        q = r + 1
        while q < nrows and cnt[q] == cnt[r] and np.array_equal(cols[rowptr[q]:rowptr[q + 1]], cols[rowptr[q - 1]:rowptr[q]] + 1):
            q += 1
        runs += 1
        r = q
    return nrows / max(runs, 1)


def stencils(rowptr, cols):
    seen = {}
    for r in range(rowptr.size - 1):
        c = cols[rowptr[r]:rowptr[r + 1]]
        key = (c.size,) + tuple((c[1:] - c[0]).tolist())
        seen[key] = seen.get(key, 0) + 1
    return seen


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="cylinder", choices=["cylinder", "box"])
    ap.add_argument("--nr", type=int, default=10)
    ap.add_argument("--nth", type=int, default=110)
    ap.add_argument("--nz", type=int, default=8)
    ap.add_argument("--degree", type=int, default=4)
    ap.add_argument("--blocks", type=int, nargs="*", default=[64, 256, 1024, 4096, 16384])
    args = ap.parse_args()
    mesh = hollow_cylinder_mesh(args.nr, args.nth, args.nz) if args.workload == "cylinder" else box_mesh(args.nr, args.nth, args.nz)
    P = args.degree + 1
    dm = build_dofmap(mesh, args.degree)
    rowptr, cols = transpose_map(np.asarray(dm.elem_nodes, dtype=np.int64), P)
    nrows, nnz = rowptr.size - 1, cols.size
    print(f"{args.workload} {args.nr}x{args.nth}x{args.nz}, degree {args.degree}: {mesh.nelem} elements, {nrows} shell rows, "
          f"{nnz} contributors ({nnz / nrows:.2f} per row), E-vector {nnz * RECORD / 1e6:.1f} MB")
    plain, coded = 4 + 4 + 1 + 4 * nnz / nrows, 4 + 2 + 4 + 1
    print(f"map bytes per row: plain {plain:.1f}, coded {coded:.1f}  ({(plain - coded) * nrows / 1e6:.2f} MB less for this mesh)")
    print("E-vector lines touched / useful bytes, per block of consecutive rows:")
    for b in args.blocks:
        print(f"  {b:6d} rows: {lines_per_useful(rowptr, cols, b):.2f}")
    print(f"runs of rows whose contributors advance by one record: {run_lengths(rowptr, cols):.2f} rows on average")
    st = stencils(rowptr, cols)
    big = sum(n for k, n in st.items() if k[0] > 8)
    print(f"stencils (count, distances from the first contributor): {len(st)} distinct over {nrows} rows; rows of more than 8 contributors: {big}")


if __name__ == "__main__":
    main()
