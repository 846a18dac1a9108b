"""CeedXVectorBlockGram / CeedXVectorBlockCombine on the device (csrc/kernels_block.hip) against extended precision within the derived
bounds of _block_common.py.  Shapes: the rows around a lane pair, a wave, a workgroup and a chunk of either kernel (read from the library:
``ceed.block_limits``), one past a full grid of either kernel so that the grid-stride loops and the final sum wrap; the column counts at
both limits, ragged tiles (3 x 5, 47 x 48) and the solver's (8 x 8, 24 x 24; 24 -> 8, 48 -> 16); every leading dimension with a NaN
padding.  Properties: same bits twice, a bitwise symmetric G(A, A), weight absent = weight of ones, beta = 0 reads no Y, the padding
keeps its bits.  Then every refusal with its message, the mirror rule of ``BlockVector`` in both orders, and a recorded graph."""
import ctypes as C

import numpy as np
import pytest

from _block_common import combine_reference, gram_reference, make_block, padding_bits, worst_ratio
from ceedpetscsolid_amd import ceed as cd

pytestmark = pytest.mark.gpu

ROWS = (1, 2, 63, 64, 65, 255, 256, 257)
GRAM_COLS = ((1, 1), (1, 48), (48, 1), (3, 5), (8, 8), (24, 24), (47, 48), (48, 48))
COMBINE_COLS = ((1, 1), (24, 8), (48, 16), (48, 48), (5, 3))
worst = {"gram": 0.0, "combine": 0.0}


@pytest.fixture(scope="module")
def limits(gpu):
    lim = cd.block_limits(gpu.L)
    assert gpu.L.has("CeedXVectorBlockGram") and gpu.L.has("CeedXVectorBlockCombine")
    assert lim[0] == cd.BLOCK_MAX_COLS == 48 and all(v and v > 0 for v in lim)
    return lim


def check_gram(gpu, n, ka, kb, pads=(0, 1, 7), a0=2, b0=1):
    for pad in pads:
        A, a = make_block(gpu, n, a0 + ka, n + pad, 11)
        B, b = make_block(gpu, n, b0 + kb, n + pad, 12)
        w = np.random.default_rng(13).uniform(0.0, 2.0, n)
        W = gpu.vector(n).set_array(w)
        G = gpu.vector(ka * kb + 2).set_value(-7.0)
        for weight, wh in ((None, None), (W, w)):
            A.gram(B, G, a0=a0, ka=ka, b0=b0, kb=kb, weight=weight)
            g = G.to_numpy()
            assert np.all(g[ka * kb:] == -7.0)
            ref, bound = gram_reference(a[a0:], b[b0:], wh)
            ratio = worst_ratio(g[:ka * kb].reshape(ka, kb), ref, bound)
            worst["gram"] = max(worst["gram"], ratio)
            print(f"gram n={n} ld={n + pad} {ka}x{kb} weight={weight is not None}: worst |G - ref| / bound = {ratio:.3f}")
            assert ratio <= 1.0
            A.gram(B, G, a0=a0, ka=ka, b0=b0, kb=kb, weight=weight)
            assert np.array_equal(G.to_numpy(), g)        # two calls, the same bits
        for o in (A, B, W, G):
            o.destroy()


@pytest.mark.parametrize("ka,kb", GRAM_COLS)
def test_gram_rows_and_columns(gpu, limits, ka, kb):
    R = limits[1]
    for n in sorted(set(ROWS) | {R - 1, R, R + 1}):
        check_gram(gpu, n, ka, kb)


def test_gram_past_a_full_grid_of_partials(gpu, limits):
    _, R, pmax, _, _ = limits
    check_gram(gpu, pmax * R + 1, 8, 8, pads=(1,), a0=1, b0=0)
    check_gram(gpu, 3 * pmax * R - 5, 3, 5, pads=(0,), a0=0, b0=0)


def test_gram_properties(gpu):
    n, k = 1000, 48
    A, a = make_block(gpu, n, k, n + 1, 14)
    G, G1 = gpu.vector(k * k), gpu.vector(k * k)
    ones = gpu.vector(n).set_value(1.0)
    for kk in (48, 24, 7, 1):
        A.gram(A, G, ka=kk, kb=kk)
        g = G.to_numpy()[:kk * kk].reshape(kk, kk)
        assert np.array_equal(g, g.T), kk                 # bit for bit: one order for every entry, and products commute
        A.gram(A, G1, ka=kk, kb=kk, weight=ones)
        assert np.array_equal(G1.to_numpy()[:kk * kk].reshape(kk, kk), g), kk     # weight absent = weight of ones
    A.gram(A, G1, a0=1, ka=24, b0=13, kb=30)              # one block, overlapping ranges
    ref, bound = gram_reference(a[1:25], a[13:43])
    assert worst_ratio(G1.to_numpy()[:720].reshape(24, 30), ref, bound) <= 1.0
    for o in (A, G, G1, ones):
        o.destroy()


def check_combine(gpu, n, ka, ky, pads=(0, 1, 7), a0=1, y0=2):
    for pad in pads:
        A, a = make_block(gpu, n, a0 + ka, n + pad, 15)
        Cm = np.random.default_rng(16).uniform(-1.0, 1.0, (ka, ky))
        for beta in (0.0, 1.0, -0.5):
            Y, y = make_block(gpu, n, y0 + ky, n + pad, 17)
            before = padding_bits(Y)
            if beta == 0.0:
                Y.fill(np.full((ky, n), np.nan), first=y0)    # beta = 0 does not read Y: the NaN does not propagate
            Y.combine(A, Cm, y0=y0, ky=ky, a0=a0, ka=ka, beta=beta)
            out = Y.to_numpy()
            ref, bound = combine_reference(y[y0:], a[a0:], Cm, beta)
            ratio = worst_ratio(out[y0:], ref, bound)
            worst["combine"] = max(worst["combine"], ratio)
            print(f"combine n={n} ld={n + pad} {ka}->{ky} beta={beta}: worst |Y - ref| / bound = {ratio:.3f}")
            assert ratio <= 1.0
            assert np.array_equal(out[:y0], y[:y0])           # the columns outside the range keep their bits
            assert np.array_equal(padding_bits(Y), before)    # and so does the padding
            Y.destroy()
        A.destroy()


@pytest.mark.parametrize("ka,ky", COMBINE_COLS)
def test_combine_rows_and_columns(gpu, limits, ka, ky):
    rows = limits[3]
    for n in sorted(set(ROWS) | {rows - 1, rows, rows + 1}):
        check_combine(gpu, n, ka, ky)


def test_combine_past_a_full_grid(gpu, limits):
    rows, groups = limits[3], limits[4]
    check_combine(gpu, groups * rows + 1, 1, 1, pads=(1,), a0=0, y0=0)
    check_combine(gpu, 3 * rows + 300, 24, 8, pads=(7,))


def test_beta_one_accumulates(gpu):
    n = 300
    A, a = make_block(gpu, n, 2, n, 18)
    Y, y = make_block(gpu, n, 1, n, 19)
    Y.combine(A, np.array([[1.0], [0.0]]), beta=1.0)
    assert np.array_equal(Y.to_numpy()[0], a[0] + y[0])
    A.destroy(); Y.destroy()


# ---- refusals: every message, and nothing launched after one -------------------------------------------------------------------
def _gram(L, A, a0, ka, B, b0, kb, n, ld, w, G):
    L.chk(L.lib.CeedXVectorBlockGram(A.h, C.c_int(a0), C.c_int(ka), B.h, C.c_int(b0), C.c_int(kb), C.c_int(n), C.c_int(ld), cd._h(w), G.h))


def _combine(L, Y, y0, ky, A, a0, ka, Cv, beta, n, ld):
    L.chk(L.lib.CeedXVectorBlockCombine(Y.h, C.c_int(y0), C.c_int(ky), A.h, C.c_int(a0), C.c_int(ka), Cv.h, C.c_double(beta), C.c_int(n), C.c_int(ld)))


def test_refusals(gpu):
    L, n, ld, k = gpu.L, 10, 12, 4
    A, B, Y = (gpu.vector(k * ld).set_value(1.0) for _ in range(3))
    G, Cv, small = gpu.vector(16).set_value(-7.0), gpu.vector(16).set_value(1.0), gpu.vector(3).set_value(1.0)
    Y.set_value(-7.0)
    gram_cases = [
        ((A, 0, 2, B, 0, 2, 0, ld, None, G), "the number of rows n must be at least 1"),
        ((A, 0, 2, B, 0, 2, n, n - 1, None, G), "the leading dimension ld must be at least n"),
        ((A, 0, 0, B, 0, 2, n, ld, None, G), "A: a column count must lie in 1 .. 48"),
        ((A, 0, 2, B, 0, 49, n, ld, None, G), "B: a column count must lie in 1 .. 48"),
        ((A, -1, 2, B, 0, 2, n, ld, None, G), "A: a first column must not be negative"),
        ((A, 3, 2, B, 0, 2, n, ld, None, G), "A: the column range reaches past the end of its vector"),
        ((A, 0, 2, B, 2, 3, n, ld, None, G), "B: the column range reaches past the end of its vector"),
        ((A, 0, 2, B, 0, 2, n, ld, None, small), "G holds 3 entries, 2 x 2 are written"),
        ((A, 0, 2, B, 0, 2, n, ld, small, G), "the weight holds 3 entries, n = 10 are read"),
        ((A, 0, 2, B, 0, 2, n, ld, None, A), "G must not be one of the operands"),
    ]
    for args, msg in gram_cases:
        with pytest.raises(cd.CeedError, match="CeedXVectorBlockGram: .*" + msg.replace("(", r"\(").replace(")", r"\)")):
            _gram(L, *args)
    combine_cases = [
        ((Y, 0, 2, A, 0, 2, Cv, 0.0, 0, ld), "the number of rows n must be at least 1"),
        ((Y, 0, 2, A, 0, 2, Cv, 0.0, n, n - 1), "the leading dimension ld must be at least n"),
        ((Y, 0, 49, A, 0, 2, Cv, 0.0, n, ld), "Y: a column count must lie in 1 .. 48"),
        ((Y, 0, 2, A, 0, 0, Cv, 0.0, n, ld), "A: a column count must lie in 1 .. 48"),
        ((Y, -2, 2, A, 0, 2, Cv, 0.0, n, ld), "Y: a first column must not be negative"),
        ((Y, 2, 3, A, 0, 2, Cv, 0.0, n, ld), "Y: the column range reaches past the end of its vector"),
        ((Y, 0, 2, A, 4, 1, Cv, 0.0, n, ld), "A: the column range reaches past the end of its vector"),
        ((Y, 0, 2, A, 0, 2, small, 0.0, n, ld), "C holds 3 entries, 2 x 2 are read"),
        ((Y, 0, 2, Y, 1, 2, Cv, 0.0, n, ld), "the columns 0 .. 2 of Y overlap the columns 1 .. 3 of A"),
        ((Y, 0, 2, A, 0, 2, Y, 0.0, n, ld), "C must not be the output"),
    ]
    for args, msg in combine_cases:
        with pytest.raises(cd.CeedError, match="CeedXVectorBlockCombine: .*" + msg):
            _combine(L, *args)
    # the last row of a range that ends exactly at the end of its vector is accepted: (x0 + kx) ld - (ld - n) = length
    tight = gpu.vector(k * ld - (ld - n)).set_value(1.0)
    _gram(L, tight, 0, k, tight, 2, 2, n, ld, None, G)
    assert np.array_equal(G.to_numpy()[:8], np.full(8, float(n)))
    G.set_value(-7.0)
    with pytest.raises(cd.CeedError, match="reaches past the end"):
        _gram(L, tight, 1, k, B, 0, 2, n, ld, None, G)
    gpu.synchronize()
    assert np.all(G.to_numpy() == -7.0) and np.all(Y.to_numpy() == -7.0)      # the outputs keep their sentinel
    _combine(L, Y, 0, 2, Y, 2, 2, Cv, 0.0, n, ld)                             # disjoint ranges of one vector are fine


def test_two_vectors_over_one_allocation_are_seen_to_overlap(gpu):
    A, _ = make_block(gpu, 20, 4, 20, 20)
    view = gpu.vector(40).set_device_pointer(A.t.data_ptr() + 8 * 20)         # columns 1 .. 3 of A through another vector
    with pytest.raises(cd.CeedError, match="overlap"):
        _combine(gpu.L, view, 0, 2, A.owner, 2, 2, gpu.vector(4).set_value(1.0), 0.0, 20, 20)
    _combine(gpu.L, view, 0, 1, A.owner, 2, 2, gpu.vector(4).set_value(1.0), 0.0, 20, 20)      # column 1 from columns 2, 3
    A.touched()
    a = A.to_numpy()
    assert np.array_equal(a[1], a[2] + a[3])


def test_portable_form_is_never_taken_on_device_data(gpu, monkeypatch):
    A, _ = make_block(gpu, 16, 2, 16, 21)
    G = gpu.vector(4)
    monkeypatch.setattr(gpu.L, "has", lambda symbol: False)
    with pytest.raises(cd.CeedError, match="the portable form works on host arrays only"):
        A.gram(A, G)
    with pytest.raises(cd.CeedError, match="the portable form works on host arrays only"):
        A.combine(A, np.ones((1, 1)), y0=0, ky=1, a0=1, ka=1)


# ---- mirrors -----------------------------------------------------------------------------------------------------------------------
def test_column_writes_and_block_writes_see_each_other(gpu):
    from ceedpetscsolid_amd.mass import MassOperator
    from ceedpetscsolid_amd.mesh import box_mesh
    from ceedpetscsolid_amd.solid import SolidProblem
    prob = SolidProblem(gpu, box_mesh(2, 1, 1), 2, "linElas", nu=0.3, E=1.0, bc_sides=[6])
    n, k = prob.lsize(), 4
    mop = MassOperator(prob, prob.fine, 1.5)
    assert mop.kernel_name != "portable"
    A, a = make_block(gpu, n, k, n, 22)
    G = gpu.vector(k * k)
    x, y = gpu.vector(n).set_array(a[0]), gpu.vector(n)
    mop.apply(x, y)
    a[1] = y.to_numpy()
    # the owner is read on the host (it now has a host mirror), then a column is written by an operator apply
    assert np.array_equal(A.owner.to_numpy().reshape(k, n)[1], A.to_numpy()[1])
    mop.apply(x, A[1])
    A.gram(A, G)
    ref, bound = gram_reference(a, a)
    assert worst_ratio(G.to_numpy().reshape(k, k), ref, bound) <= 1.0
    assert np.array_equal(A.to_numpy()[1], a[1])
    # a column is read on the host (it now has a host mirror), then the block is written
    assert np.array_equal(A[2].to_numpy(), a[2])
    A.combine(A, np.array([[0.0, 1.0], [1.0, 0.0]]), y0=2, ky=2, a0=0, ka=2)
    assert np.array_equal(A[2].to_numpy(), a[1]) and np.array_equal(A[3].to_numpy(), a[0])
    # and the column read is seen by the next operator apply on it
    mop.apply(A[3], y)
    mop.apply(x, A[0])
    assert np.array_equal(y.to_numpy(), a[1]) and np.array_equal(A.to_numpy()[0], a[1])


# ---- graph ---------------------------------------------------------------------------------------------------------------------------
def test_recorded_gram_and_combine_give_the_eager_bits(gpu):
    n, ld = 3000, 3001
    A, a = make_block(gpu, n, 24, ld, 23)
    Y, _ = make_block(gpu, n, 8, ld, 24)
    G = gpu.vector(24 * 24).set_value(0.0)
    Cv = gpu.vector(24 * 8).set_array(np.random.default_rng(25).uniform(-1.0, 1.0, 24 * 8))
    A.gram(A, G); Y.combine(A, Cv)                        # eager first: the coefficient matrix reaches the device
    g_eager, y_eager = G.to_numpy(), Y.to_numpy()
    G.set_value(0.0); Y.fill(np.zeros((8, n)))
    graph = gpu.capture(lambda: (A.gram(A, G), Y.combine(A, Cv)))
    graph.launch()
    assert np.array_equal(G.to_numpy(), g_eager) and np.array_equal(Y.to_numpy(), y_eager)
    A.fill(2.0 * a)                                       # the replay reads the block as it is now
    graph.launch()
    G.device_pointer()                                    # (a replay writes behind the vector's flags: device access drops G's host mirror)
    assert np.array_equal(G.to_numpy(), 4.0 * g_eager) and np.array_equal(Y.to_numpy(), 2.0 * y_eager)
    graph.destroy()


def test_print_the_worst_ratios():
    """(runs last in the file) the figures profiles/modal.txt records"""
    print(f"worst error / bound over this file's cases: gram {worst['gram']:.3f}, combine {worst['combine']:.3f}")
    assert worst["gram"] <= 1.0 and worst["combine"] <= 1.0
