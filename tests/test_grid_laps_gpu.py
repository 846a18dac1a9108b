"""The plain device kernels past one grid (tests/_plain_kernels.py: the table of their launch forms and caps).  Most of them are
launched on a capped grid and reach everything beyond it with a stride loop; the tests of their own files stay far below the caps, so a
wrong stride, an accumulator that survives into the second lap or a counter dropped between laps would pass there.  Here every such
kernel runs at G - 1, G, G + 1 and 2 G + 3 items (G: what one grid covers) or on the one mesh that crosses several caps at once,
box_mesh(12, 12, 12) at degree 7: 614 125 nodes, 1 119 744 dofs of element-interior nodes, an E-vector of 2 654 208 entries.

References are NumPy / SciPy in float64 and never call the library, except where the reference IS another route through it (the fused
epilogue against its two passes, the folded halo against apply-then-exchange, the row form of a product against the plain form): those
are bit for bit.  Every bound is the bound of the kernel's own small test; none is new.  Inputs are random, so that the second lap's
data differ from the first.  Measured figures: profiles/grid_laps.txt."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from _ceed_env import ceed_with_env
from _plain_kernels import CAPS, GRID_FOR_ITEMS, STREAM_ITEMS, lap_sizes
from _vector_model import same_bits
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd import portable as pt
from ceedpetscsolid_amd.mesh import box_mesh, build_dofmap, gll_nodes, side_set_nodes
from ceedpetscsolid_amd.solid import SolidProblem

pytestmark = pytest.mark.gpu

u = 2.0 ** -53
PRESET = -7.0
STREAM_SIZES = lap_sizes(STREAM_ITEMS)
GRID_FOR_SIZES = lap_sizes(GRID_FOR_ITEMS)
# the degree-7 box
BOX7, BOX7_DEGREE = (12, 12, 12), 7
BOX7_NODES = (7 * 12 + 1) ** 3
BOX7_LSIZE = 3 * BOX7_NODES
BOX7_INTERIOR_DOFS = 3 * 6 ** 3 * 12 ** 3
UNPACK_ITEMS = CAPS["assemble unpack"].items
FOLDED_HALO_SIZES = [UNPACK_ITEMS - 1, UNPACK_ITEMS, UNPACK_ITEMS + 1, BOX7_LSIZE // 3]
# the sheet whose bottom holds more face-node rows than one grid of k_surface_sum
SHEET, SHEET_DEGREE = (362, 362, 1), 2
SHEET_ROWS = (2 * 362 + 1) ** 2
# rows of C of the sparse products: the row form's grid covers 32 768 rows, the plain form's 65 536; the plain form runs the operands
# of the row form plus ONE row whose product row is longer than 4 096 entries
ROW_ITEMS, PLAIN_ITEMS = CAPS["spgemm row"].items, CAPS["spgemm plain"].items
ROW_PRODUCT_ROWS = [ROW_ITEMS + 5, 2 * ROW_ITEMS + 3, PLAIN_ITEMS + 4]
PLAIN_PRODUCT_ROWS = [n + 1 for n in ROW_PRODUCT_ROWS]

assert BOX7_NODES > STREAM_ITEMS and BOX7_INTERIOR_DOFS > CAPS["assemble_epi interior"].items and SHEET_ROWS > STREAM_ITEMS


def ordered_sums(group, values, ngroups):
    """[ngroups]: per group the values added one after the other from 0.0, in the order they stand in -- what a lane that walks its
    row does -- without a Python loop over the entries: the k-th member of every group is added in the k-th pass."""
    group = np.asarray(group, dtype=np.int64)
    order = np.argsort(group, kind="stable")
    g, v = group[order], np.asarray(values, dtype=np.float64)[order]
    first = np.r_[True, g[1:] != g[:-1]] if g.size else np.zeros(0, dtype=bool)
    rank = np.arange(g.size) - np.flatnonzero(first)[np.cumsum(first) - 1] if g.size else np.zeros(0, dtype=np.int64)
    acc = np.zeros(ngroups)
    for k in range(int(rank.max()) + 1 if g.size else 0):
        sel = rank == k
        acc[g[sel]] = acc[g[sel]] + v[sel]                 # (a group holds one k-th member: no index twice)
    return acc


def ordered_transpose(lay, E, y0):
    """test_restriction_transpose_gpu.expected_transpose -- rows by ascending offset, a row's contributors in E-vector order into an
    accumulator from 0.0, one add onto y0 -- in the vectorised form of ordered_sums."""
    nelem, elemsize, ncomp, compstride, lsize, offsets = lay
    offsets = np.asarray(offsets, dtype=np.int64).ravel()
    rows, row_of = np.unique(offsets, return_inverse=True)
    Ev, y = E.reshape(nelem, ncomp, elemsize), y0.copy()
    e, n = np.divmod(np.arange(offsets.size), elemsize)
    for c in range(ncomp):
        y[rows + c * compstride] = y0[rows + c * compstride] + ordered_sums(row_of, Ev[e, c, n], rows.size)
    return y


@pytest.fixture(scope="module")
def box7():
    mesh = box_mesh(*BOX7)
    dm = build_dofmap(mesh, BOX7_DEGREE)
    assert (dm.nnodes, dm.lsize) == (BOX7_NODES, BOX7_LSIZE)
    return mesh, dm


# ---------------------------------------------------------------------------------------------------------------------------------
# k_rstr, k_rstr_transpose, k_multiplicity
# ---------------------------------------------------------------------------------------------------------------------------------
def check_restriction(gpu, lay, rng):
    """Gather, transpose-add (twice: the same bits) and multiplicity of the layout, each bit for bit."""
    nelem, elemsize, ncomp, compstride, lsize, offsets = lay
    offsets = np.asarray(offsets, dtype=np.int64).ravel()
    r = gpu.elem_restriction(nelem, elemsize, ncomp, compstride, lsize, offsets)
    idx = (offsets.reshape(nelem, 1, elemsize) + compstride * np.arange(ncomp).reshape(1, ncomp, 1)).ravel()     # [elem][comp][node]
    l, E, y0 = rng.uniform(-1, 1, lsize), rng.uniform(-1, 1, idx.size), rng.uniform(-1, 1, lsize)
    Lv, Ev = gpu.vector(lsize).set_array(l), gpu.vector(idx.size).set_value(PRESET)
    r.apply(cd.NOTRANSPOSE, Lv, Ev)
    assert np.array_equal(Ev.to_numpy(), l[idx])
    want = ordered_transpose(lay, E, y0)
    Ev.set_array(E)
    for _ in range(2):
        Lv.set_array(y0)
        r.apply(cd.TRANSPOSE, Ev, Lv)
        got = Lv.to_numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (bad.size, bad[:5], got[bad[:5]], want[bad[:5]])
    M = gpu.vector(lsize + 2).set_value(PRESET)
    r.multiplicity(M)
    m = M.to_numpy()
    assert np.array_equal(m[:lsize], np.bincount(idx, minlength=lsize).astype(np.float64)) and not m[lsize:].any()
    for o in (Lv, Ev, M, r):
        o.destroy()


@pytest.mark.parametrize("n", STREAM_SIZES)
def test_restriction_around_one_grid(gpu, n):
    """One node per element and one component, so that the item counts are exact: (a) n E-vector entries over an L-vector half as long
    (k_rstr at n items; every row of the transpose map has contributors from both laps of the E-vector); (b) n rows, half of them with
    further contributors (k_rstr_transpose and k_multiplicity at n items)."""
    rng = np.random.default_rng(n)
    lsize = n // 2 + 1
    check_restriction(gpu, (n, 1, 1, 1, lsize, rng.integers(0, lsize, n)), rng)
    offsets = rng.permutation(np.r_[np.arange(n), rng.integers(0, n, n // 2)])
    assert np.unique(offsets).size == n
    check_restriction(gpu, (offsets.size, 1, 1, 1, n, offsets), rng)


def test_restriction_on_the_degree7_box(gpu, box7):
    """Three interlaced components on the mesh: 2 654 208 E-vector entries (five laps and a part), 1 842 375 rows x components (three
    and a part), rows of 1, 2, 4 and 8 contributors."""
    mesh, dm = box7
    lay = (mesh.nelem, dm.P ** 3, 3, 1, dm.lsize, dm.offsets())
    assert lay[0] * lay[1] * 3 > 5 * STREAM_ITEMS and dm.lsize > 3 * STREAM_ITEMS
    check_restriction(gpu, lay, np.random.default_rng(7))


# ---------------------------------------------------------------------------------------------------------------------------------
# k_pb_assemble
# ---------------------------------------------------------------------------------------------------------------------------------
def test_pointblock_diagonal_on_the_degree7_box(oracle, gpu, box7):
    """The assembled blocks of linear elasticity against the sum of portable.pointblock_diag_host.  Its input, the element matrices of
    all 1 728 elements, would be 32 GB at P = 8; every element of the uniform box has the same matrix, so the element blocks are those of
    ONE element of that size from the oracle (pointblock_diag_host on its 1 536 columns), repeated, and summed over a node's elements in
    element order by the same portable.node_sum, the rows and columns of the clamped side zeroed as pointblock_diag_host zeroes them.
    Bound: 1e-10 of the largest entry, as test_pointblock_gpu.device_blocks_match."""
    from _pointblock_common import level_problem, problem_with_state
    mesh, dm = box7
    one = box_mesh(1, 1, 1, hi=(1.0 / BOX7[0], 1.0 / BOX7[1], 1.0 / BOX7[2]))
    po, lv = level_problem(oracle, one, dm.P, dm.P, "linElas", bc_sides=())
    B1 = oracle.vector(3 * po.lsize(lv))
    po.get_pointblock_diag(lv, B1)
    eb = B1.to_numpy().reshape(-1, 9)[po.levels[lv].dofmap.elem_nodes[0]]                  # [local node][c out, c in]
    B1.destroy(); po.destroy()
    assert np.abs(eb).min(axis=1).max() > 0
    p = problem_with_state(gpu, mesh, BOX7_DEGREE, "linElas", bc_sides=(1,))
    level = p.levels[p.fine]
    assert np.array_equal(level.dofmap.elem_nodes, dm.elem_nodes)
    want = pt.node_sum(dm.elem_nodes, np.broadcast_to(eb, (mesh.nelem,) + eb.shape), dm.nnodes).reshape(-1, 3, 3)
    m = level.mask.reshape(-1, 3) != 0
    want[m[:, :, None] | m[:, None, :]] = 0.0
    B = gpu.vector(3 * dm.lsize).set_value(3.0)
    p.get_pointblock_diag(p.fine, B)
    got = B.to_numpy().reshape(-1, 3, 3)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"point-block diagonal, {dm.nnodes} nodes: device vs the summed oracle element blocks {err:.2e}")
    assert err <= 1e-10
    assert m.any() and np.all(got[m[:, :, None] | m[:, None, :]] == 0.0)
    B.destroy(); p.destroy()


# ---------------------------------------------------------------------------------------------------------------------------------
# k_xfer_weights
# ---------------------------------------------------------------------------------------------------------------------------------
def lagrange_interpolation(Pc, Pf):
    """[Pf][Pc]: the Pc Lagrange functions on the Gauss-Lobatto points of the coarse element at those of the fine one."""
    xc, xf = gll_nodes(Pc), gll_nodes(Pf)
    out = np.ones((Pf, Pc))
    for i in range(Pc):
        for k in range(Pc):
            if k != i:
                out[:, i] *= (xf - xc[k]) / (xc[i] - xc[k])
    return out


def test_transfer_weights_see_an_entry_beyond_one_grid(gpu, box7):
    """The weights of the owner-form transfers, w = fine-side scale x local multiplicity over the 1 842 375 fine dofs.  With scale =
    1 / multiplicity the kernel counts no weight other than 1 and the transfers run without weights.  Then ONE entry of the scale,
    beyond one grid and in a lane that goes on to two further laps of unit weights, is halved: the count the lane carries must reach
    the atomic, or the transfers go on without weights.  Prolongation and restriction (5 -> 8 nodes per direction) against NumPy's
    tensor interpolation at the parity bound of test_transfer_gpu, and the halved entry against the plain run as
    test_kernel_matrix_gpu holds the weighted path."""
    mesh, dmf = box7
    dmc = build_dofmap(mesh, 4)
    ne, nf, nc = mesh.nelem, dmf.lsize, dmc.lsize
    rc = gpu.elem_restriction(ne, 125, 3, 1, nc, dmc.offsets())
    rf = gpu.elem_restriction(ne, 512, 3, 1, nf, dmf.offsets())
    basis = gpu.basis_lagrange(3, 3, 5, 8, cd.GAUSS_LOBATTO)
    opP, opR = gpu.operator(gpu.qfunction_identity(3, cd.EVAL_INTERP, cd.EVAL_NONE)), gpu.operator(gpu.qfunction_identity(3, cd.EVAL_NONE, cd.EVAL_INTERP))
    opP.set_field("input", rc, basis, "active"); opP.set_field("output", rf, None, "active")
    opR.set_field("input", rf, None, "active"); opR.set_field("output", rc, basis, "active")
    mult = np.repeat(np.bincount(dmf.elem_nodes.ravel(), minlength=dmf.nnodes), 3).astype(np.float64)
    scale = 1.0 / mult
    star = STREAM_ITEMS + 3 * 1000 + 1                                           # second lap of its lane, which has two more to go
    assert star + 2 * STREAM_ITEMS < nf
    S = gpu.vector(nf).set_array(scale)
    for op in (opP, opR):
        op.set_fine_scale(S)
    rng = np.random.default_rng(5)
    xc, xf = rng.uniform(-1, 1, nc), rng.uniform(-1, 1, nf)
    Xc, Xf, Yf, Yc = gpu.vector(nc).set_array(xc), gpu.vector(nf).set_array(xf), gpu.vector(nf), gpu.vector(nc)
    I = lagrange_interpolation(5, 8)
    node, at = np.unique(dmf.elem_nodes.ravel(), return_index=True)              # the fine nodes, each in ONE of its elements
    results = []
    for trial in range(2):
        if trial == 1:
            scale[star] *= 0.5
            S.set_array(scale)                                                   # rewritten in place: the next apply recomputes the weights
        w = mult * scale
        Yf.set_value(5.0); Yc.set_value(5.0)
        opP.apply(Xc, Yf); opR.apply(Xf, Yc)
        yf, yc = Yf.to_numpy(), Yc.to_numpy()
        fe = np.einsum("ai,bj,dk,ekjic->edbac", I, I, I, xc.reshape(-1, 3)[dmc.elem_nodes].reshape(ne, 5, 5, 5, 3), optimize=True).reshape(ne * 512, 3)
        ref_f = np.zeros((dmf.nnodes, 3))
        ref_f[node] = fe[at]
        ref_f = ref_f.reshape(-1) * w
        owned = np.zeros((ne * 512, 3))
        owned[at] = (w * xf).reshape(-1, 3)[node]
        ce = np.einsum("ai,bj,dk,edbac->ekjic", I, I, I, owned.reshape(ne, 8, 8, 8, 3), optimize=True).reshape(ne, 125, 3)
        ref_c = pt.node_sum(dmc.elem_nodes, ce, dmc.nnodes).reshape(-1)
        ef, ec = np.abs(yf - ref_f).max() / np.abs(ref_f).max(), np.abs(yc - ref_c).max() / np.abs(ref_c).max()
        print(f"transfer 5 -> 8 on {ne} elements, trial {trial}: prolong {ef:.2e}, restrict {ec:.2e} against NumPy")
        assert ef < 1e-10 and ec < 1e-10, (trial, ef, ec)
        results.append((yf, yc))
    (pf, pc), (wf, wc) = results
    rest = np.arange(nf) != star
    assert pf[star] != 0.0 and np.isclose(wf[star], 0.5 * pf[star], rtol=1e-12, atol=0)
    assert np.allclose(wf[rest], pf[rest], rtol=1e-12, atol=1e-15)
    assert not np.array_equal(wc, pc)
    for o in (opP, opR, rc, rf, basis, S, Xc, Xf, Yf, Yc):
        o.destroy()


# ---------------------------------------------------------------------------------------------------------------------------------
# k_assemble_epi: the workgroups of the element-interior dofs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["serial", "default"])
def test_fused_epilogue_on_the_degree7_box(product_lib, box7, form):
    """The fused Chebyshev step and the fused residual against their two passes, bit for bit (test_fused_epilogue_gpu), where the
    1 119 744 dofs of element-interior nodes exceed the 4 096 x 256 the interior workgroups cover.  The fused forms sum the rows in one
    segment whatever the form of the plain apply: one launch holds every interior dof under both."""
    from test_fused_epilogue_gpu import _arrays, _cheb_pair
    mesh, dm = box7
    gpu = ceed_with_env(product_lib, {"CEED_MI355X_ASSEMBLE": "serial"} if form == "serial" else {})
    p = SolidProblem(gpu, mesh, BOX7_DEGREE, "linElas", nu=0.3, E=1.0, bc_sides=[1], multigrid="none")
    lv, n = p.fine, p.lsize()
    op, L = p.levels[lv].opJacob, gpu.L
    arrs = _arrays(p, lv, 107)
    for first in (False, True, "recomputed"):
        for in_place in (True, False):
            a, b = _cheb_pair(p, lv, arrs, first, in_place)
            for k in ("x", "d", "r"):
                assert np.array_equal(a[k], b[k]), (first, in_place, k, np.abs(a[k] - b[k]).max())
            assert np.abs(b["d"]).max() > 0
        assert op.launch_info()["segments"] == 1, op.launch_info()
    X, B, T, W1, W2 = (gpu.vector(n).set_array(arrs["x"]), gpu.vector(n).set_array(arrs["b"]), gpu.vector(n), gpu.vector(n), gpu.vector(n))
    op.apply(X, T)
    L.chk(L.lib.CeedXVectorWAXPBY(W1.h, C.c_double(1.0), B.h, C.c_double(-1.0), T.h))
    T.set_value(9.0)
    L.chk(L.lib.CeedXOperatorApplyResidual(op.h, X.h, T.h, B.h, W2.h))
    assert op.launch_info()["segments"] == 1
    assert np.array_equal(W1.to_numpy(), W2.to_numpy())
    p.destroy()


# ---------------------------------------------------------------------------------------------------------------------------------
# k_halo_pack, k_halo_unpack_add; k_assemble's unpack workgroups
# ---------------------------------------------------------------------------------------------------------------------------------
def self_communicator(ceed):
    """A one-rank RCCL communicator whose only neighbour is the rank itself (test_gpu_parity.test_halo_exchange_through_rccl_on_one_gpu)."""
    ident = C.create_string_buffer(128)
    ceed.L.chk(ceed.L.lib.CeedXCommGetUniqueId(ceed.h, ident))
    ceed.L.chk(ceed.L.lib.CeedXCommInit(ceed.h, 1, 0, ident))


def self_halo(ceed, lists):
    h = C.c_void_p()
    lists = [np.ascontiguousarray(a, dtype=np.int32) for a in lists]
    k = len(lists)
    ceed.L.chk(ceed.L.lib.CeedXHaloCreate(ceed.h, k, (C.c_int * k)(*([0] * k)), (C.c_int * k)(*[a.size for a in lists]),
                                          (C.POINTER(C.c_int) * k)(*[a.ctypes.data_as(C.POINTER(C.c_int)) for a in lists]), C.byref(h)))
    return h


def test_halo_exchange_around_one_grid(product_lib):
    """y[idx] += y[idx] through the library's pack kernel, RCCL to the rank itself and the unpack-add kernel, bit for bit against "pack
    everything, then add".  For every size s: s entries over s - 777 distinct destinations (the pack at s items), and s + 777 entries
    over s destinations (the unpack at s items); three lists, the second in scrambled order with destinations of the first, the
    third empty."""
    ceed = cd.Ceed(product_lib, "/gpu/hip/mi355x")
    L = ceed.L
    self_communicator(ceed)
    n = 1_300_003
    rng = np.random.default_rng(8)
    for s in STREAM_SIZES:
        for total, distinct in ((s, s - 777), (s + 777, s)):
            dst = rng.choice(n, distinct, replace=False)
            lists = [np.sort(dst), rng.permutation(dst)[:total - distinct], np.zeros(0, dtype=np.int64)]
            h = self_halo(ceed, lists)
            y0 = rng.uniform(-1, 1, n)
            Y = ceed.vector(n).set_array(y0)
            want = y0.copy()
            for rep in range(2):
                L.chk(L.lib.CeedXHaloStart(h, Y.h))
                L.chk(L.lib.CeedXHaloFinish(h, Y.h))
                packed = [want[a].copy() for a in lists]              # all lists are packed BEFORE any is added
                for a, p in zip(lists, packed):
                    want[a] += p
                got = Y.to_numpy()
                assert np.array_equal(got, want), (total, distinct, rep, int((got != want).sum()))
            L.chk(L.lib.CeedXHaloDestroy(C.byref(h)))
            Y.destroy()
    L.chk(L.lib.CeedXCommDestroy(ceed.h))


@pytest.mark.parametrize("mode,fold", [(m, f) for m in (0, 1, 2) for f in (0, 1)])
def test_folded_halo_on_the_degree7_box(product_lib, box7, mode, fold):
    """The one-call apply with its exchange (CeedXOperatorApplyWithHalo) against the apply followed by the exchange, bit for bit, with
    halos of more destinations than the 1 024 x 256 the unpack workgroups of k_assemble cover -- under every form of the call: whole
    apply then exchange (0), split-phase on one stream (1) and on two (2), the pack folded into the rows' launch (1) or a launch of its
    own (0).  The leading elements are the lower eleven of the twelve element layers; the halo's entries lie on their priority rows: the
    nodes no other element holds, without the element-interior nodes, which the fused kernel stores itself and which are no rows of the
    sum (a real interface lies on element faces)."""
    mesh, dm = box7
    ceed = ceed_with_env(product_lib, {"CEED_MI355X_OVL_MODE": str(mode), "CEED_MI355X_FOLD_PACK": str(fold)})
    self_communicator(ceed)
    p = SolidProblem(ceed, mesh, BOX7_DEGREE, "linElas", nu=0.3, E=1.0, bc_sides=[1], multigrid="none")
    level = p.levels[p.fine]
    n, nlead = p.lsize(), BOX7[0] * BOX7[1] * 11
    rest = np.zeros(dm.nnodes, dtype=bool)
    rest[level.dofmap.elem_nodes[nlead:].ravel()] = True
    prio = np.repeat((~rest).astype(np.uint8), 3)
    a = np.arange(dm.P)
    inner = ((a > 0) & (a < dm.P - 1))
    inner = (inner[:, None, None] & inner[None, :, None] & inner[None, None, :]).ravel()      # local nodes a + P b + P^2 c off every face
    shell = np.ones(dm.nnodes, dtype=bool)
    shell[level.dofmap.elem_nodes[:, inner].ravel()] = False
    rows = np.flatnonzero(prio & np.repeat(shell, 3))
    assert rows.size >= max(FOLDED_HALO_SIZES)
    op = level.opJacob
    op.set_overlap_split(nlead, prio)
    rng = np.random.default_rng(100 * mode + fold)
    X, Y1, Y2 = ceed.vector(n).set_array(rng.uniform(-1, 1, n) * (level.mask == 0)), ceed.vector(n), ceed.vector(n)
    p.apply_jacobian(p.fine, X, Y1)
    y1 = Y1.to_numpy()
    assert np.isfinite(y1).all() and np.abs(y1).max() > 0
    for size in FOLDED_HALO_SIZES:
        sub = np.sort(rng.choice(rows, size, replace=False))
        h = self_halo(ceed, [sub])
        Y2.set_value(7.0)
        op.apply_with_halo(X, Y2, h)
        expect = y1.copy()
        expect[sub] += y1[sub]
        got = Y2.to_numpy()
        assert np.array_equal(got, expect), (size, int((got != expect).sum()))
        ceed.L.chk(ceed.L.lib.CeedXHaloDestroy(C.byref(h)))
    p.destroy()
    ceed.L.chk(ceed.L.lib.CeedXCommDestroy(ceed.h))


# ---------------------------------------------------------------------------------------------------------------------------------
# k_csr_sum, k_csr_unit_diag, k_csr_diag
# ---------------------------------------------------------------------------------------------------------------------------------
def banded_pattern(nd, extras, nempty, rng):
    """(rowptr, cols, diag_slot): nd rows with a diagonal entry, the first `extras` of them with a neighbouring column too (columns
    ascending), and nempty rows without entries at random places; diag_slot[r] = -1 for those."""
    N = nd + nempty
    holds = np.ones(N, dtype=bool)
    holds[rng.choice(N, nempty, replace=False)] = False
    rows = np.flatnonzero(holds)
    lens = np.zeros(N, dtype=np.int64)
    lens[rows] = 1
    lens[rows[:extras]] = 2
    rowptr = np.r_[0, np.cumsum(lens)]
    cols = np.zeros(rowptr[-1], dtype=np.int64)
    diag_slot = np.full(N, -1, dtype=np.int64)
    two, one = rows[:extras], rows[extras:]
    nb = np.where(two + 1 < N, two + 1, two - 1)
    cols[rowptr[two]], cols[rowptr[two] + 1] = np.minimum(two, nb), np.maximum(two, nb)
    cols[rowptr[one]] = one
    diag_slot[two], diag_slot[one] = rowptr[two] + (nb < two), rowptr[one]
    return rowptr, cols, diag_slot


def csr_case_shape(kind, s):
    """(rows with a diagonal, of them with a neighbour, empty rows, unit rows) such that the item count of ONE of the three kernels is
    exactly s: the entries of the pattern (k_csr_sum), the unit rows (k_csr_unit_diag), the rows (k_csr_diag)."""
    if kind == "entries":
        return s - 1000, 1000, 50, (s - 1000) // 2
    if kind == "unit rows":
        return s + 50, (s + 50) // 3, 50, s
    return s - 100, (s - 100) // 3, 100, (s - 100) // 2


@pytest.mark.parametrize("s", GRID_FOR_SIZES)
@pytest.mark.parametrize("kind", ["entries", "unit rows", "rows"])
def test_csr_assembly_around_one_grid(gpu, kind, s):
    """CeedXCsrAssemble / GetDiagonal / Apply on a banded pattern with a long constrained tail, against the arithmetic of
    test_linalg_kernels.coo_expected (a slot's entries added from 0.0 in ascending COO order, then the unit diagonals), bit for bit as
    coo_case: duplicates in scrambled order over twelve decades, dropped entries, slots no entry maps to."""
    from test_linalg_kernels import check_spmv_values, coo_values
    rng = np.random.default_rng(s + len(kind))
    nd, extras, nempty, nunit = csr_case_shape(kind, s)
    rowptr, cols, diag_slot = banded_pattern(nd, extras, nempty, rng)
    N, nnz = rowptr.size - 1, cols.size
    unit = np.flatnonzero(diag_slot >= 0)[-nunit:]                              # the tail
    assert {"entries": nnz, "unit rows": unit.size, "rows": N}[kind] == s
    unmapped = rng.choice(nnz, nnz // 10, replace=False)
    slot = rng.choice(np.setdiff1d(np.arange(nnz), unmapped), 2 * nnz)
    slot[rng.random(slot.size) < 0.1] = -1
    a = cd.Csr(gpu, rowptr, cols, slot, unit)
    V, D = gpu.vector(slot.size), gpu.vector(N)
    for trial in range(2):
        v = coo_values(rng, slot.size)
        a.assemble(V.set_array(v))
        vals = a.values()
        exp = ordered_sums(slot[slot >= 0], v[slot >= 0], nnz)
        exp[diag_slot[unit]] = 1.0
        bad = np.flatnonzero(exp.view(np.int64) != vals.view(np.int64))
        assert bad.size == 0, (bad.size, bad[:5], vals[bad[:5]], exp[bad[:5]])
        D.set_array(np.full(N, np.nan))
        a.diagonal(D)
        assert same_bits(D.to_numpy(), np.where(diag_slot >= 0, exp[np.maximum(diag_slot, 0)], 0.0))
        A = sp.csr_matrix((exp, cols, rowptr), shape=(N, N))
        x = rng.uniform(-1, 1, N)
        X, Y = gpu.vector(N).set_array(x), gpu.vector(N).set_array(np.full(N, np.nan))
        a.apply(X, Y)
        check_spmv_values(A, x, Y.to_numpy())
        X.destroy(); Y.destroy()
    for o in (a, V, D):
        o.destroy()


# ---------------------------------------------------------------------------------------------------------------------------------
# k_csr_spgemm_row, k_csr_spgemm, k_csr_spgemm_dense
# ---------------------------------------------------------------------------------------------------------------------------------
def check_product_sparse(ceed, L, R):
    """test_linalg_kernels.check_product for a sparse result too large to hold as a dense array: the sorted SciPy pattern, per entry
    |C_ij - ref_ij| <= 2 (len(L_i) + 2) u (|L| |R|)_ij, the same bits from a second update.  Returns the values."""
    from test_linalg_kernels import rect
    l, r = rect(ceed, L), rect(ceed, R)
    Cm = cd.Csr.product(l, r, variable=0)
    Cm.update()
    vals = Cm.values()
    Cm.update()
    assert same_bits(Cm.values(), vals)
    nr, nc, nz, rp, cl = Cm.pattern()
    mag, ref = (abs(L) @ abs(R)).tocsr(), (L @ R).tocsr()
    mag.sort_indices(); ref.sort_indices()
    assert (nr, nc) == (L.shape[0], R.shape[1]) and np.array_equal(rp, mag.indptr) and np.array_equal(cl, mag.indices)
    assert np.array_equal(ref.indptr, mag.indptr) and np.array_equal(ref.indices, mag.indices)
    bound = 2 * (np.repeat(np.diff(L.indptr), np.diff(mag.indptr)) + 2) * u * mag.data
    bad = np.flatnonzero(~(np.abs(vals - ref.data) <= bound))
    assert bad.size == 0, (bad.size, bad[:5], vals[bad[:5]], ref.data[bad[:5]])
    for o in (Cm, l, r):
        o.destroy()
    return vals


def lap_operands(n, rng, G=ROW_ITEMS, m=64, q=5000):
    """L (n x m), R (m x q) for the row form past one grid of G workgroups.  Workgroup b takes the rows b, b + G, b + 2 G: the rows of
    the FIRST lap give long rows of C (two to four of R's rows 1 .. 8, about forty columns each, overlapping), those of the SECOND lap
    short ones (one of R's short rows) where b is even and EMPTY ones where it is odd, those of the third long ones again -- the
    accumulator and the column list a workgroup keeps in LDS shrink, vanish and grow between its laps.  R's row 0 holds 4 200 columns
    and no row of L names it: the row that sends the product to the plain form does (plain_operand)."""
    rrows = [np.sort(rng.choice(q, 4200, replace=False))]
    rrows += [np.sort(rng.choice(400, int(k), replace=False)) for k in rng.integers(30, 50, 8)]
    rrows += [np.sort(rng.choice(q, int(k), replace=False)) for k in rng.integers(1, 4, m - 9)]
    rp = np.r_[0, np.cumsum([c.size for c in rrows])]
    R = sp.csr_matrix((rng.uniform(-1, 1, rp[-1]), np.concatenate(rrows), rp), shape=(m, q))
    i = np.arange(n)
    lap, b = i // G, i % G
    lens = np.where(lap % 2 == 0, rng.integers(2, 5, n), np.where(b % 2 == 0, 1, 0))
    lp = np.r_[0, np.cumsum(lens)]
    row = np.repeat(i, lens)
    pos = np.arange(lp[-1]) - lp[row]
    long_cols = 1 + (rng.integers(0, 8, n)[row] + pos) % 8                       # distinct within a row: consecutive modulo 8
    lcols = np.where(lap[row] % 2 == 0, long_cols, rng.integers(9, m, lp[-1]))
    L = sp.csr_matrix((rng.uniform(-1, 1, lp[-1]), lcols, lp), shape=(n, m))
    L.sort_indices()
    return L, R


def plain_operand(L):
    """L and one more row that names R's long row: the product's longest row exceeds 4 096 entries and the whole product takes the plain form."""
    return sp.vstack([L, sp.csr_matrix(([0.5, -0.25], [0, 3], [0, 2]), shape=(1, L.shape[1]))]).tocsr()


@pytest.mark.parametrize("n", ROW_PRODUCT_ROWS)
def test_products_past_one_grid_of_rows(gpu, n):
    """C = L R with more rows than one grid: the row form (k_csr_spgemm_row, n rows) and the plain form (k_csr_spgemm, n + 1 rows)
    against SciPy at check_product's bound, and the row form against the plain form bit for bit, as product_forms_agree_case."""
    L, R = lap_operands(n, np.random.default_rng(n))
    Lx = plain_operand(L)
    lens = (abs(L) @ abs(R)).getnnz(axis=1)
    assert 64 < lens.max() <= 4096 < (abs(Lx) @ abs(R)).getnnz(axis=1).max()
    second = lens[ROW_ITEMS:2 * ROW_ITEMS]
    assert second[::2].min() >= 1 and second[::2].max() <= 3 and not second[1::2].any() and lens[:ROW_ITEMS].min() > 30
    v_row = check_product_sparse(gpu, L, R)
    v_gen = check_product_sparse(gpu, Lx, R)
    assert same_bits(v_gen[:v_row.size], v_row)


def test_a_dense_product_cannot_outgrow_its_grid(gpu):
    """k_csr_spgemm_dense takes a product only as a dense SQUARE result of at most 4 096 columns, so of at most 4 096 rows: fewer than
    the 8 192 workgroups its launcher allows, and its loop over the rows never takes a second lap (test_linalg_kernels'
    test_dense_product_on_device runs its largest launch).  Pinned here: a dense result of 8 192 + 5 rows and 8 columns is refused, and a
    square one that large is formed by the plain kernel, not this one -- were either to change, tests/_plain_kernels.py is to change."""
    from test_linalg_kernels import csr_rows, rect
    rng = np.random.default_rng(3)
    n = CAPS["spgemm dense"].items + 5
    l, r = rect(gpu, csr_rows(rng.integers(0, 4, n), 16, rng)), rect(gpu, csr_rows([3] * 16, 8, rng))
    with pytest.raises(cd.CeedError, match="a dense result must be square"):
        cd.Csr.product(l, r, variable=0, dense=True)
    l.destroy(); r.destroy()


# ---------------------------------------------------------------------------------------------------------------------------------
# k_surface_sum
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sheet():
    """The bottom (side 1) of a one-element-thick sheet: 725^2 = 525 625 face-node rows at degree 2, and a mask that flags about a tenth
    of the dofs, so rows of both laps."""
    mesh = box_mesh(*SHEET)
    dm = build_dofmap(mesh, SHEET_DEGREE)
    assert side_set_nodes(mesh, dm, [1]).size == SHEET_ROWS
    mask = (np.random.default_rng(1).random(dm.lsize) < 0.1).astype(np.uint8)
    return mesh, dm, mask


def test_surface_loads_on_a_sheet_past_one_grid(gpu, sheet):
    import test_surface_load_gpu as ts
    mesh, dm, mask = sheet
    P, Q = SHEET_DEGREE + 1, SHEET_DEGREE + 1
    dev, ref = ts.both(gpu, mesh, dm, [1], Q, mask=mask)
    rng = np.random.default_rng(100 * P + Q)
    uu, du = 0.1 * rng.uniform(-1, 1, dm.lsize), rng.uniform(-1, 1, dm.lsize)
    got = ts.device_results(gpu, dev, uu, du, dm.lsize)
    want = [ref.traction_host(ts.T), ref.pressure_host(uu), ref.pressure_host(), ref.tangent_host(uu, du)]
    assert dev.kernel_name == f"surface<P={P},Q={Q}>"
    m = mask != 0
    for kind, a, b in zip(("traction", "pressure", "pressure(u=0)", "tangent"), got, want):
        err = np.abs(a - b).max() / np.abs(b).max()
        print(f"{kind} on {dev.nface} faces, {SHEET_ROWS} rows: device vs portable {err:.2e}")
        assert err <= ts.TOL, (kind, err)
        assert not a[m].any() and a[~m].any()                                  # masked rows are never written
    dev.destroy()


CONTACT_AMPLITUDE = 100.0


def test_contact_on_a_sheet_past_one_grid(gpu, sheet):
    """The contact residual, state, tangent and diagonal of the sheet's bottom against the portable form at test_contact_gpu's bound.
    The inputs must meet _contact_inputs' condition -- no Gauss point within 1e-6 of the obstacle -- over 1.2 million points: with
    displacements of 0.1 the gaps spread over ~0.2 and about ten points would lie inside that margin, so the displacement is
    uniform(-100, 100) instead (gaps over ~200: 0.01 points expected inside; the kinematics are sums of products either way).  One
    obstacle, the plane: the row sum under test does not know the obstacle, and the portable form takes seconds per obstacle here."""
    import _contact_inputs as ci
    import test_contact_gpu as tc
    mesh, dm, mask = sheet
    P, Q = SHEET_DEGREE + 1, SHEET_DEGREE + 1
    dev, ref = tc.both(gpu, mesh, dm, [1], Q, mask=mask)
    rng = np.random.default_rng(100 * P + Q)
    uu, du = CONTACT_AMPLITUDE * rng.uniform(-1, 1, dm.lsize), rng.uniform(-1, 1, dm.lsize)
    m = mask != 0
    for which in ("plane",):
        dev.set_obstacle(**ci.set_obstacle(ref, which, uu))
        ci.input_condition(ref, uu)
        got = tc.device_results(gpu, dev, uu, du, dm.lsize, name=f"contact<P={P},Q={Q},{{}}>")
        worst = tc.compare(got, ref, uu, du, which)
        print(f"contact, {which}, {dev.nface} faces, {SHEET_ROWS} rows: worst device-vs-portable error {worst:.2e}")
        for a in (got[0], got[2], got[3]):
            assert not a[m].any() and a[~m].any()
    dev.destroy()
