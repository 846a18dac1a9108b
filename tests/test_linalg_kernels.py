"""The assembled coarse level and the Krylov vector helpers at their edge shapes: CSR-stream SpMV (CeedXCsrApply), the COO sum
(CeedXCsrAssemble / GetDiagonal), the three Galerkin-product kernels (CeedXCsrUpdate: dense, row and generic form), the dot
products, the elementwise helpers, and the rest of kernels_vector.hip -- SetValue, Reciprocal, the Chebyshev entries, ScalarDivide and
AXPBYScalars -- bit for bit on vectors that are windows between sentinels.  Each case is a function of the Ceed; a thin test runs it on the CPU oracle and a thin
`gpu` test on the device.  References are numpy / scipy / math.fsum in f64, and every bound is PER ENTRY, scaled by the absolute
product and the summation depth of the kernel, so that one dropped or doubled term fails it."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp

from _vector_model import PAD, DeviceBuffer, HostBuffer, intact, same_bits   # noqa: F401  (same_bits: -0.0 is not 0.0, a NaN equals itself)
from ceedpetscsolid_amd import ceed as cd

u = 2.0 ** -53
GRID_CAP = 2048 * 256                 # threads of the vector kernels' grid (2048-block cap): beyond it they stride


def csr_rows(lens, ncols, rng):
    """nrows x ncols CSR with rows of the given lengths: distinct sorted columns, values in U(-1, 1)."""
    lens = np.asarray(lens, dtype=np.int64)
    cols = [np.arange(k) if k == ncols else np.sort(rng.choice(ncols, k, replace=False)) for k in lens]
    cols = np.concatenate(cols).astype(np.int64) if len(cols) and lens.sum() else np.zeros(0, np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    return sp.csr_matrix((rng.uniform(-1, 1, cols.size), cols, indptr), shape=(lens.size, ncols))


def rect(ceed, M):
    return cd.Csr.rect(ceed, M.shape[0], M.shape[1], M.indptr, M.indices, M.data)


def short(rng, k):
    return list(rng.integers(5, 31, k))


def band_pair(n, nc, c0, c1, rng):
    """The distributed hierarchy's pair (amg.py, the rank's share): P (n x nc) whose columns are this rank's aggregates, a
    contiguous band [c0, c1), and P^T (nc x n), whose rows outside the band -- the other ranks' aggregates -- are empty."""
    lens = rng.integers(1, 7, n)
    cols = np.concatenate([np.sort(c0 + rng.choice(c1 - c0, k, replace=False)) for k in lens])
    P = sp.csr_matrix((rng.uniform(-1, 1, cols.size), cols, np.concatenate([[0], np.cumsum(lens)])), shape=(n, nc))
    P.sort_indices()
    Pt = P.T.tocsr()
    Pt.sort_indices()
    return P, Pt


def spmv_shapes():
    """name -> scipy CSR, built explicitly around the CSR-stream limits: runs of <= 256 rows and <= 2 048 entries, a longer row alone."""
    rng = np.random.default_rng(17)
    S = {}
    for nr in (1, 256, 257, 700):
        S[f"nnz0_{nr}"] = csr_rows([0] * nr, 40, rng)
    S["nrows0"] = csr_rows([], 40, rng)
    S["300_then_600_empty"] = csr_rows(list(rng.integers(1, 21, 300)) + [0] * 600, 500, rng)
    S["1_then_257_empty"] = csr_rows([7] + [0] * 257, 40, rng)
    S["600_empty_leading"] = csr_rows([0] * 600 + short(rng, 100), 500, rng)
    S["600_empty_band"] = csr_rows(short(rng, 100) + [0] * 600 + short(rng, 100), 500, rng)
    for nr in (256, 257):
        S[f"{nr}x8"] = csr_rows([8] * nr, 600, rng)
        S[f"{nr}x1"] = csr_rows([1] * nr, 600, rng)
    for L in (2048, 2049):
        S[f"row{L}_between_short"] = csr_rows(short(rng, 50) + [L] + short(rng, 50), 3000, rng)
        S[f"row{L}_last"] = csr_rows(short(rng, 50) + [L], 3000, rng)
    S["two_long_rows"] = csr_rows(short(rng, 20) + [3000, 2500] + short(rng, 20), 3500, rng)
    S["long_row_first"] = csr_rows([3000] + short(rng, 50), 3500, rng)
    for name, (c0, c1) in (("leading", (0, 300)), ("middle", (450, 750))):
        P, Pt = band_pair(3000, 1200, c0, c1, rng)
        S[f"P_band_{name}"], S[f"Pt_band_{name}"] = P, Pt
    for n in (1, 1500, 2048, 2049):
        S[f"dense{n}"] = csr_rows([n] * n, n, rng)
    return S


SPMV = spmv_shapes()


def spmv_input(A, seed=5):
    """x in U(-1, 1) with NaN in every entry no row references: a kernel that multiplies a padded entry by zero shows up."""
    x = np.random.default_rng(seed).uniform(-1, 1, A.shape[1])
    used = np.zeros(A.shape[1], dtype=bool)
    used[A.indices] = True
    x[~used] = np.nan
    return x


def check_spmv_values(A, x, y):
    """|y_i - (A x)_i| <= 2 (len_i + 10) u (|A| |x|)_i per row (the kernel's and scipy's summation depth); an empty row is 0.0."""
    lens = np.diff(A.indptr)
    ref, mag = A @ x, abs(A) @ np.abs(x)
    assert y.shape == ref.shape
    bad = ~(np.abs(y - ref) <= 2 * (lens + 10) * u * mag)
    assert not bad.any(), (np.flatnonzero(bad)[:10], y[bad][:5], ref[bad][:5])
    assert np.all(y[lens == 0] == 0.0)


def spmv_case(ceed, name):
    A = SPMV[name]
    nr, nc = A.shape
    x = spmv_input(A)
    a = rect(ceed, A)
    X = ceed.vector(nc).set_array(x)
    out = []
    for _ in range(2):
        Y = ceed.vector(nr).set_array(np.full(nr, np.nan))
        a.apply(X, Y)
        out.append(Y.to_numpy())
        Y.destroy()
    check_spmv_values(A, x, out[0])
    assert same_bits(out[0], out[1])                      # the same bits twice
    a.destroy(); X.destroy()


def recorded_spmv_case(ceed, name):
    """The apply recorded into a graph (the V-cycle replays restrict like this): the replay gives the eager bits."""
    A = SPMV[name]
    nr, nc = A.shape
    x = spmv_input(A)
    a = rect(ceed, A)
    X, Y, Yg = ceed.vector(nc).set_array(x), ceed.vector(nr), ceed.vector(nr).set_array(np.full(nr, np.nan))
    a.apply(X, Y)                                         # the first apply cuts the runs (not recordable)
    Yg.device_pointer()
    g = ceed.capture(lambda: a.apply(X, Yg))
    g.launch()
    ceed.synchronize()
    y, yg = Y.to_numpy(), Yg.to_numpy()
    check_spmv_values(A, x, y)
    assert same_bits(yg, y)
    g.destroy(); a.destroy()


# ---- COO assembly --------------------------------------------------------------------------------------------------------
def coo_pattern(rng, n=300):
    """Square pattern with empty rows, rows with and without a diagonal entry; unit rows among those with one; COO entries:
    duplicates in scrambled order, dropped (-1) entries, and slots that no entry maps to."""
    lens = rng.integers(0, 13, n)
    lens[rng.choice(n, 30, replace=False)] = 0
    rows = []
    for r, k in enumerate(lens):
        c = set(rng.choice(n, k, replace=False).tolist())
        if k and r % 3 == 0:
            c.add(r)
        elif r % 3 == 1:
            c.discard(r)
        rows.append(sorted(c))
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in rows])])
    cols = np.array([c for row in rows for c in row], dtype=np.int64)
    nnz = cols.size
    diag_rows = [r for r in range(n) if r in rows[r]]
    unit = np.array(sorted(rng.choice(diag_rows, 12, replace=False)), dtype=np.int64)
    unmapped = rng.choice(nnz, nnz // 10, replace=False)
    mapped = np.setdiff1d(np.arange(nnz), unmapped)
    slot = rng.choice(mapped, 4 * nnz)
    slot[rng.random(slot.size) < 0.1] = -1
    return rowptr, cols, slot, unit, unmapped


def coo_values(rng, ncoo):
    # magnitudes over twelve decades: the sum of one slot depends on its order
    return rng.uniform(-1, 1, ncoo) * 10.0 ** rng.integers(-6, 7, ncoo)


def coo_expected(nnz, slot, v, rowptr, cols, unit):
    vals = [0.0] * nnz
    for k in range(slot.size):                            # from 0.0, in ascending COO index order
        if slot[k] >= 0:
            vals[slot[k]] += float(v[k])
    vals = np.array(vals)
    for r in unit:
        s = rowptr[r] + np.flatnonzero(cols[rowptr[r]:rowptr[r + 1]] == r)[0]
        vals[s] = 1.0
    return vals


def coo_case(ceed):
    """CeedXCsrAssemble / GetDiagonal / Apply, assembled twice; returns the values of both assemblies."""
    rng = np.random.default_rng(29)
    rowptr, cols, slot, unit, unmapped = coo_pattern(rng)
    n, nnz = rowptr.size - 1, cols.size
    a = cd.Csr(ceed, rowptr, cols, slot, unit)
    out = []
    for trial in range(2):
        v = coo_values(rng, slot.size)
        a.assemble(ceed.vector(slot.size).set_array(v))
        vals = a.values()
        exp = coo_expected(nnz, slot, v, rowptr, cols, unit)
        assert same_bits(vals, exp)
        assert np.all(vals[unmapped] == 0.0)
        diag_slot = {r: rowptr[r] + int(np.flatnonzero(cols[rowptr[r]:rowptr[r + 1]] == r)[0])
                     for r in range(n) if r in cols[rowptr[r]:rowptr[r + 1]]}
        for r in unit:
            assert vals[diag_slot[r]] == 1.0
        D = ceed.vector(n).set_array(np.full(n, np.nan))
        a.diagonal(D)
        d = D.to_numpy()
        assert same_bits(d, [vals[diag_slot[r]] if r in diag_slot else 0.0 for r in range(n)])
        A = sp.csr_matrix((exp, cols, rowptr), shape=(n, n))
        x = rng.uniform(-1, 1, n)
        Y = ceed.vector(n).set_array(np.full(n, np.nan))
        a.apply(ceed.vector(n).set_array(x), Y)
        check_spmv_values(A, x, Y.to_numpy())
        out.append(vals)
    a.destroy()
    return out


# ---- Galerkin products ----------------------------------------------------------------------------------------------------
def check_product(ceed, L, R, dense=False, variable=0):
    """C = L R through CeedXCsrCreateProduct / Update against scipy: |C_ij - ref_ij| <= 2 (len(L_i) + 2) u (|L| |R|)_ij per entry
    (the kernels sum an entry along L's row), entries the product does not reach exactly 0.0, the sorted scipy pattern when not
    dense, and the same bits from a second update.  Returns the values."""
    l, r = rect(ceed, L), rect(ceed, R)
    Cm = cd.Csr.product(l, r, variable=variable, dense=dense)
    Cm.update()
    vals = Cm.values()
    Cm.update()
    assert same_bits(Cm.values(), vals)
    nr, nc, nz, rp, cl = Cm.pattern()
    assert (nr, nc) == (L.shape[0], R.shape[1])
    mag = (abs(L) @ abs(R)).tocsr()
    mag.sort_indices()
    if dense:
        assert nz == nr * nc and np.array_equal(rp, np.arange(nr + 1) * nc) and np.array_equal(cl, np.tile(np.arange(nc), nr))
    else:
        assert np.array_equal(rp, mag.indptr) and np.array_equal(cl, mag.indices)
    Cd = np.zeros((nr, nc))
    Cd[np.repeat(np.arange(nr), np.diff(rp)), cl] = vals
    ref, magd = (L @ R).toarray(), mag.toarray()
    bound = 2 * (np.diff(L.indptr)[:, None] + 2) * u * magd
    bad = ~(np.abs(Cd - ref) <= bound)
    assert not bad.any(), (np.argwhere(bad)[:10], Cd[bad][:5], ref[bad][:5])
    assert np.all(Cd[magd == 0] == 0.0)
    for o in (Cm, l, r):
        o.destroy()
    return vals


def dense_product_case(ceed, n):
    """A dense n x n result: the LDS-row kernel up to 4 096 columns, the generic one beyond.  Empty rows of L, an empty row of R,
    entries the product does not reach."""
    rng = np.random.default_rng(n)
    m = 16
    llens = rng.integers(0, 4, n)
    L = csr_rows(llens, m, rng)
    rlens = rng.integers(n // 3, n // 2, m)
    rlens[5] = 0
    R = csr_rows(rlens, n, rng)
    check_product(ceed, L, R, dense=True)


def row_form_operands(K, rng, nr=300, m=40):
    """L (nr x m), R (m x q) whose product's longest row holds exactly K entries (row 0 of C: R's row 0 and three rows inside
    its columns); every other row of C holds at most 40.  Empty rows in L, R and C."""
    q = K + 500
    top = np.sort(rng.choice(q, K, replace=False))
    rrows = [top] + [np.sort(rng.choice(top, K // 2, replace=False)) for _ in range(3)]
    rrows += [np.sort(rng.choice(q, k, replace=False)) for k in rng.integers(1, 11, m - 4)]
    rrows[6] = np.zeros(0, np.int64)
    rp = np.concatenate([[0], np.cumsum([c.size for c in rrows])])
    R = sp.csr_matrix((rng.uniform(-1, 1, rp[-1]), np.concatenate(rrows), rp), shape=(m, q))
    lrows = [np.array([0, 1, 2, 3])]
    for i in range(1, nr):
        k = 0 if i % 7 == 0 else int(rng.integers(1, 5))
        lrows.append(np.sort(4 + rng.choice(m - 4, k, replace=False)))
    lp = np.concatenate([[0], np.cumsum([c.size for c in lrows])])
    L = sp.csr_matrix((rng.uniform(-1, 1, lp[-1]), np.concatenate(lrows), lp), shape=(nr, m))
    return L, R


def row_form_case(ceed, K):
    L, R = row_form_operands(K, np.random.default_rng(K))
    assert int((abs(L) @ abs(R)).getnnz(axis=1).max()) == K
    check_product(ceed, L, R)


def distributed_product_case(ceed):
    """P^T T of the distributed hierarchy: the left operand's rows outside this rank's band are empty (rows of zeros in the
    dense result, empty rows in the sparse one); the right operand is the variable one, as in amg.py."""
    rng = np.random.default_rng(41)
    n, nc = 2000, 600
    P, Pt = band_pair(n, nc, 200, 380, rng)
    A = csr_rows(rng.integers(3, 12, n), n, rng)
    T = (A @ P).tocsr()
    T.sort_indices()
    for dense in (True, False):
        check_product(ceed, Pt, T, dense=dense, variable=1)


def product_forms_agree_case(ceed):
    """The comment on the kernels: every form sums an entry along L's row, term for term, so they give the same bits.
    (1) a product whose natural pattern is full, formed dense (LDS-row kernel) and not (row kernel);  (2) the row kernel on L
    against the generic one on L plus one row whose product row is longer than 4 096 entries (which sends the whole product
    to the generic kernel)."""
    rng = np.random.default_rng(7)
    n, m = 300, 12
    L = csr_rows(rng.integers(2, 7, n), m, rng)
    R = csr_rows([n] * m, n, rng)                          # every row of R holds every column
    vd = check_product(ceed, L, R, dense=True)
    vr = check_product(ceed, L, R, dense=False)
    assert same_bits(vd, vr)
    q = 5000
    R2 = csr_rows([4200] + list(rng.integers(20, 60, m - 1)), q, rng)
    L2 = csr_rows(list(rng.integers(2, 7, n)), m - 1, rng)
    L2 = sp.csr_matrix((L2.data, L2.indices + 1, L2.indptr), shape=(n, m))     # rows of R2 other than the long one
    Lx = sp.vstack([L2, sp.csr_matrix(([0.5, -0.25], [0, 3], [0, 2]), shape=(1, m))]).tocsr()
    assert (abs(L2) @ abs(R2)).getnnz(axis=1).max() <= 4096 < (abs(Lx) @ abs(R2)).getnnz(axis=1).max()
    v_row = check_product(ceed, L2, R2)
    v_gen = check_product(ceed, Lx, R2)
    assert same_bits(v_gen[:v_row.size], v_row)


# ---- vector helpers --------------------------------------------------------------------------------------------------------
DOT_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, GRID_CAP - 1, GRID_CAP, GRID_CAP + 1, 3 * 2 ** 20 + 7]


def dot_data(n, kind):
    rng = np.random.default_rng(n + 3)
    if kind == "positive":
        return rng.uniform(0, 1, n), rng.uniform(0, 1, n), None
    x, y = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    if kind == "mixed":
        return x, y, None
    w = rng.uniform(0.5, 2.0, n) * (rng.random(n) < 0.7)  # zeros where a Dirichlet mask has them
    if kind == "positive_masked":
        return np.abs(x), np.abs(y), w
    return x, y, w


def dot_depth_device(n):
    """Error depth of k_dot + k_dot_final: ceil(n / 2^19) terms per thread, 6 levels of the wave's butterfly, 3 additions of the
    four waves' sums, up to 8 partials per thread of the final kernel and its 8-level tree, 2 roundings of the product: within 32."""
    return math.ceil(n / GRID_CAP) + 32


def dot_depth_sequential(n):
    return n + 2


def dot_case(ceed, n, kind, depth):
    L = ceed.L
    x, y, w = dot_data(n, kind)
    X, Y = ceed.vector(n).set_array(x), ceed.vector(n).set_array(y)
    W = ceed.vector(n).set_array(w) if w is not None else None
    wh = W.h if W is not None else None
    terms = (w if w is not None else 1.0) * x * y
    ref, mag = math.fsum(terms), math.fsum(np.abs(terms))
    d = []
    for _ in range(2):
        r = C.c_double()
        L.chk(L.lib.CeedXVectorDot(X.h, Y.h, wh, C.byref(r)))
        d.append(r.value)
    assert same_bits(d[0], d[1])
    if n == 0:
        assert same_bits(d[0], 0.0)
    assert abs(d[0] - ref) <= depth(n) * u * mag, (n, kind, d[0], ref, (d[0] - ref) / (u * mag) if mag else None)
    sc = ceed.vector(4).set_array(np.full(4, np.nan))
    L.chk(L.lib.CeedXVectorDotTo(X.h, Y.h, wh, sc.h, 2))
    s = sc.to_numpy()
    assert same_bits(s[2], d[0])
    assert np.all(np.isnan(s[[0, 1, 3]]))


ELEM_SIZES = [1, 257, GRID_CAP + 1, 3 * 2 ** 20 + 7]


def two_prod(a, b):
    """a * b == p + e exactly (Dekker's product by Veltkamp splitting; numpy evaluates every operation on its own)."""
    p = a * b
    def split(v):
        t = 134217729.0 * v
        hi = t - (t - v)
        return hi, v - hi
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def axpby_error(got, a, x, b, y):
    """got - (a x + b y), the latter exact (a double-double): the error of the kernel alone, not of a rounded reference."""
    p1, e1 = two_prod(np.full_like(x, a), x)
    p2, e2 = two_prod(np.full_like(y, b), y)
    s = p1 + p2
    bb = s - p1
    lo = (p1 - (s - bb)) + (p2 - bb) + (e1 + e2)          # s + lo == a x + b y up to u^2 terms
    return (got - s) - lo


def elementwise_case(ceed, n):
    L = ceed.L
    rng = np.random.default_rng(n)
    x, y = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    x[::97] = 0.0                                          # some -0.0 products below
    X, Y = ceed.vector(n).set_array(x), ceed.vector(n).set_array(y)
    W = ceed.vector(n).set_array(np.full(n, np.nan))
    L.chk(L.lib.CeedXVectorPointwiseMult(W.h, X.h, Y.h))
    assert same_bits(W.to_numpy(), x * y)
    # b = 0 is a copy (amg.py, solver.py): a x + 0.0 even over NaN, -0.0 products turned into +0.0
    for a in (1.0, -0.75):
        T = ceed.vector(n).set_array(np.full(n, np.nan))
        L.chk(L.lib.CeedXVectorAXPBY(T.h, C.c_double(a), X.h, C.c_double(0.0)))
        t = T.to_numpy()
        assert same_bits(t, a * x + 0.0)
        T.destroy()
    a, b = 0.7, -1.3
    bound = 2 * u * (np.abs(a * x) + np.abs(b * y))
    T = ceed.vector(n).set_array(y)
    L.chk(L.lib.CeedXVectorAXPBY(T.h, C.c_double(a), X.h, C.c_double(b)))
    assert np.all(np.abs(axpby_error(T.to_numpy(), a, x, b, y)) <= bound)
    L.chk(L.lib.CeedXVectorWAXPBY(W.h, C.c_double(a), X.h, C.c_double(b), Y.h))
    assert np.all(np.abs(axpby_error(W.to_numpy(), a, x, b, y)) <= bound)
    for o in (X, Y, W, T):
        o.destroy()


def refusal_case(ceed):
    """Short operands are refused before any kernel runs (the kernels walk the length of one vector only); longer ones stay
    legal.  The target is left as it was."""
    L = ceed.L
    rng = np.random.default_rng(2)
    n = 300
    vec = lambda k: ceed.vector(k).set_array(rng.uniform(-1, 1, k))
    full, shorter, longer = vec(n), vec(n - 1), vec(n + 5)
    w0 = rng.uniform(-1, 1, n)
    W = ceed.vector(n).set_array(w0)
    for x, y in ((shorter, full), (full, shorter)):
        with pytest.raises(cd.CeedError):
            L.chk(L.lib.CeedXVectorPointwiseMult(W.h, x.h, y.h))
        assert np.array_equal(W.to_numpy(), w0)
    with pytest.raises(cd.CeedError):
        L.chk(L.lib.CeedXVectorAXPBY(W.h, C.c_double(2.0), shorter.h, C.c_double(1.0)))
    with pytest.raises(cd.CeedError):
        L.chk(L.lib.CeedXVectorAXPBY(W.h, C.c_double(2.0), shorter.h, C.c_double(0.0)))
    assert np.array_equal(W.to_numpy(), w0)
    r = C.c_double(12.5)
    for y, wt in ((shorter, None), (full, shorter.h)):
        with pytest.raises(cd.CeedError):
            L.chk(L.lib.CeedXVectorDot(W.h, y.h, wt, C.byref(r)))
        assert r.value == 12.5
    s0 = rng.uniform(-1, 1, 4)
    S = ceed.vector(4).set_array(s0)
    for y, wt in ((shorter, None), (full, shorter.h)):
        with pytest.raises(cd.CeedError):
            L.chk(L.lib.CeedXVectorDotTo(W.h, y.h, wt, S.h, 1))
        assert np.array_equal(S.to_numpy(), s0)
    # longer operands: legal, the first n entries used
    f, g = full.to_numpy(), longer.to_numpy()
    L.chk(L.lib.CeedXVectorPointwiseMult(W.h, longer.h, full.h))
    assert same_bits(W.to_numpy(), g[:n] * f)
    L.chk(L.lib.CeedXVectorAXPBY(W.h, C.c_double(-0.5), longer.h, C.c_double(0.0)))
    assert same_bits(W.to_numpy(), -0.5 * g[:n] + 0.0)
    L.chk(L.lib.CeedXVectorDot(full.h, longer.h, longer.h, C.byref(r)))
    terms = g[:n] * f * g[:n]
    assert abs(r.value - math.fsum(terms)) <= (n + 2) * u * math.fsum(np.abs(terms))
    L.chk(L.lib.CeedXVectorDotTo(full.h, full.h, longer.h, S.h, 1))
    terms = g[:n] * f * f
    assert abs(S.to_numpy()[1] - math.fsum(terms)) <= (n + 2) * u * math.fsum(np.abs(terms))


# ---- the remaining vector kernels: k_set_value, k_reciprocal, k_cheb_update, k_scalar_div, k_axpby_dev ---------------------------
# (k_masked_copy is launched by no entry point of the ABI, so there is nothing to call it through.)
# Sizes: the wave and workgroup edges of a 256-thread block, one grid-stride pass plus one element, two passes plus a tail.
EDGE_SIZES = [1, 63, 64, 65, 257, GRID_CAP + 1, 2 * GRID_CAP + 3]


def on_device(ceed):
    return "mi355x" in ceed.L.path.rsplit("/", 1)[-1]


class Window:
    """A vector of `ceed` that is a window into a longer allocation (a device tensor behind set_device_pointer; on the oracle a host
    array behind set_array(copy=False)), PAD sentinel entries either side.  read() is the window as the BUFFER holds it -- the
    library's results must be there without a further call -- and asserts that the sentinels are intact."""

    def __init__(self, ceed, data):
        data = np.asarray(data, dtype=np.float64)
        self.ceed, self.n, self.dev = ceed, data.size, on_device(ceed)
        self.buf = DeviceBuffer(data, "cuda") if self.dev else HostBuffer(data)
        self.v = ceed.vector(self.n)
        ceed.L.CeedVectorSetArray(self.v.h, cd.MEM_DEVICE if self.dev else cd.MEM_HOST, cd.USE_POINTER, self.buf.pointer())
        self.h = self.v.h

    def read(self):
        if self.dev:
            self.ceed.synchronize()
        full = self.buf.read()
        intact(full, "a window")
        return full[PAD:PAD + self.n].copy()

    def destroy(self):
        self.v.take_array(cd.MEM_DEVICE if self.dev else cd.MEM_HOST)
        self.v.destroy()


def set_value_case(ceed, n):
    """Every entry has the value's bits -- +0.0 (the memset path of the device) and -0.0 are different values."""
    w = Window(ceed, np.full(n, 7.0))
    for val in (0.0, -0.0, 1.5, np.nan, np.inf, 5e-324):
        w.v.set_value(val)
        assert same_bits(w.read(), np.full(n, val)), (n, val, w.read()[:4])
        w.v.set_value(7.0)
        assert same_bits(w.read(), np.full(n, 7.0))
    w.destroy()


PLANTED = [0.0, -0.0, 1e-300, -1e-300, np.nextafter(1e-300, 1.0), 5e-324, -5e-324, np.inf, -np.inf, np.nan, 3.0, 1e308, 1.7e308,
           -np.nextafter(1e-300, 1.0), -1.7e308]


def reciprocal_case(ceed, n):
    """CeedVectorReciprocal: 1 / v where |v| > 1e-300 (the correctly rounded quotient, denormal results included), v left as it is
    elsewhere (zeros of either sign, +-1e-300 itself, denormals, NaN).  Planted at fixed positions, the first and the last entry
    among them; a vector too short for all of them takes them in turns."""
    rng = np.random.default_rng(n)
    rounds = 1 if n >= len(PLANTED) else -(-len(PLANTED) // n)
    for k in range(rounds):
        v = rng.uniform(-4, 4, n)
        if n >= len(PLANTED):
            pos = [(j * (n - 1)) // (len(PLANTED) - 1) for j in range(len(PLANTED))]       # pos[0] = 0, pos[-1] = n - 1
            v[pos] = PLANTED
        else:
            part = PLANTED[k * n:(k + 1) * n]
            v[:len(part)] = part
            v[-1] = PLANTED[(k * n + len(part) - 1) % len(PLANTED)]
        with np.errstate(all="ignore"):
            exp = np.where(np.abs(v) > 1e-300, 1.0 / v, v)
        w = Window(ceed, v)
        w.v.reciprocal()
        got = w.read()
        bad = np.flatnonzero(got.view(np.int64) != exp.view(np.int64))
        assert bad.size == 0, (n, bad[:5], v[bad[:5]], got[bad[:5]], exp[bad[:5]])
        w.destroy()


# -- the Chebyshev entries.  What cheb_dof_regs (kernel_node_sum.hpp) does per entry, one rounding per line:
#      ri = rbase - t          (rbase: b in Start and Step, r in Update; without t, ri = rbase and nothing is rounded)
#      m  = c1 * dinv
#      di = m * ri
#      di = fma(c2, d, di)     (only if c2 != 0: ONE rounding of c2 d + di)
#      x  = di  or  x + di
#    r = ri is stored by Start, by Step if r is given, by Update if t is given.
def fma(a, b, c):
    """The correctly rounded a b + c (CPython rounds int / int correctly, and so Fraction.__float__)."""
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def cheb_data(n):
    """Operands for which the one-ulp bound between the fused and the unfused c2 d + di is a theorem: per entry c2 d and di have
    the same sign (sigma), so nothing cancels.  [With p = fl(c2 d), |p - c2 d| <= ulp(c2 d) / 2 <= ulp(s) / 2 for s = c2 d + di,
    because |c2 d| <= |s|; two reals no further apart than half the spacing of the grid round to the same or to neighbouring
    grid points, also across a power of two.]  x is of either sign."""
    rng = np.random.default_rng(100 + n)
    sigma = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return {"x": rng.uniform(-2, 2, n), "d": sigma * rng.uniform(0.1, 2, n), "r": sigma * rng.uniform(1, 2, n),
            "b": sigma * rng.uniform(1, 2, n), "t": sigma * rng.uniform(0.01, 0.9, n), "dinv": rng.uniform(0.1, 3, n)}


def cheb_subsample(n):
    if n <= 4096:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(300), np.arange(n - 300, n), np.linspace(300, n - 301, 3496).astype(np.int64)]))


def cheb_case(ceed, n, entry):
    """Every combination CeedXVectorChebyshevStart / Update / Step accepts: t given or absent, r given or absent (Step), assign_x 0 or
    1, c2 zero or not.  The vectors the formula must not read hold NaN, the vectors it must not write keep their bits."""
    L = ceed.L
    base, sub, dev = cheb_data(n), cheb_subsample(n), on_device(ceed)
    c1 = 0.7
    for has_t in (True, False):
        for has_r in ((True, False) if entry == "Step" else (True,)):
            for assign_x in (0, 1):
                for c2 in ((0.0,) if entry == "Start" else (0.0, 0.45)):
                    a = {k: v.copy() for k, v in base.items()}
                    if assign_x:
                        a["x"][:] = np.nan
                    if c2 == 0.0:
                        a["d"][:] = np.nan
                    if entry != "Update":
                        a["r"][:] = np.nan
                    w = {k: Window(ceed, v) for k, v in a.items()}
                    th, rh = (w["t"].h if has_t else None), (w["r"].h if has_r else None)
                    if entry == "Start":
                        L.CeedXVectorChebyshevStart(w["x"].h, w["d"].h, rh, w["b"].h, th, w["dinv"].h, c1, assign_x)
                    elif entry == "Step":
                        L.CeedXVectorChebyshevStep(w["x"].h, w["d"].h, rh, w["b"].h, th, w["dinv"].h, c1, c2, assign_x)
                    else:
                        L.CeedXVectorChebyshevUpdate(w["x"].h, w["d"].h, rh, th, w["dinv"].h, c1, c2, assign_x)
                    got = {k: w[k].read() for k in w}
                    what = (entry, n, has_t, has_r, assign_x, c2)
                    rbase = a["r"] if entry == "Update" else a["b"]
                    ri = rbase - a["t"] if has_t else rbase
                    di = (c1 * a["dinv"]) * ri
                    if c2 != 0.0:
                        unfused = c2 * a["d"] + di                         # numpy rounds the product, then the sum
                        exact = np.array([fma(c2, a["d"][i], di[i]) for i in sub])
                        assert np.all(np.abs(got["d"] - unfused) <= np.spacing(np.abs(unfused))), what
                        if dev:                                            # (the oracle's compiler is free to contract: not the yardstick for bits)
                            assert same_bits(got["d"][sub], exact), what
                    elif dev:
                        assert same_bits(got["d"], di), what
                    else:
                        assert np.all(np.abs(got["d"] - di) <= np.spacing(np.abs(di))), what
                    assert same_bits(got["x"], got["d"] if assign_x else a["x"] + got["d"]), what
                    stored = has_r and (entry != "Update" or has_t)
                    assert same_bits(got["r"], ri if stored else a["r"]), what
                    for k in ("b", "t", "dinv"):
                        assert same_bits(got[k], a[k]), (what, k)
                    assert np.all(np.isfinite(got["d"])) and np.all(np.isfinite(got["x"])), what
                    for o in w.values():
                        o.destroy()


def cheb_alias_case(ceed):
    """The rule of include/ceed.h: the outputs x, d, r pairwise distinct and none of them t, dinv or b.  Each alias is refused and
    the vectors are left as they were."""
    L = ceed.L
    n = 300
    base = cheb_data(n)
    w = {k: Window(ceed, v) for k, v in base.items()}
    outs, ins = ("x", "d", "r"), ("t", "dinv", "b")
    pairs = [(p, q) for i, p in enumerate(outs) for q in outs[:i]] + [(i, o) for i in ins for o in outs]
    for entry in ("Start", "Update", "Step"):
        for role, other in pairs:                                         # the vector `other` stands in `role`'s place as well
            if entry == "Update" and role == "b":
                continue
            h = {k: w[k].h for k in w}
            h[role] = w[other].h
            with pytest.raises(cd.CeedError, match="alias|of its own"):
                if entry == "Start":
                    L.CeedXVectorChebyshevStart(h["x"], h["d"], h["r"], h["b"], h["t"], h["dinv"], 0.7, 0)
                elif entry == "Step":
                    L.CeedXVectorChebyshevStep(h["x"], h["d"], h["r"], h["b"], h["t"], h["dinv"], 0.7, 0.45, 0)
                else:
                    L.CeedXVectorChebyshevUpdate(h["x"], h["d"], h["r"], h["t"], h["dinv"], 0.7, 0.45, 0)
            for k in w:
                assert same_bits(w[k].read(), base[k]), (entry, role, other, k)
    # absent vectors alias nothing
    L.CeedXVectorChebyshevStep(w["x"].h, w["d"].h, None, w["b"].h, None, w["dinv"].h, 0.7, 0.45, 0)
    L.CeedXVectorChebyshevUpdate(w["x"].h, w["d"].h, w["r"].h, None, w["dinv"].h, 0.7, 0.45, 0)
    for o in w.values():
        o.destroy()


def scalar_divide_case(ceed):
    """k_scalar_div: s[dst] = (scale * s[num]) / s[den] -- the product rounded, then the quotient rounded; den < 0: scale * s[num],
    one rounding; a denominator that is not > 0 (0.0, negative, NaN) gives +0.0.  dst may be num or den.  No other slot is written."""
    L = ceed.L
    scale, num = -2.3, 0.7310585786300049
    for den, dst in [(None, 5), (3.3, 5), (0.0, 5), (-0.0, 5), (-2.0, 5), (np.nan, 5), (5e-324, 5), (np.inf, 5),
                     (None, 1), (3.3, 1), (3.3, 2), (0.0, 2), (np.nan, 1)]:            # slot 1 holds num, slot 2 den
        s = np.full(8, np.nan)
        s[1] = num
        if den is not None:
            s[2] = den
        w = Window(ceed, s)
        L.CeedXScalarDivide(w.h, dst, 1, 2 if den is not None else -1, scale)
        with np.errstate(all="ignore"):
            exp = np.float64(scale * num) if den is None else (np.float64(scale * num) / np.float64(den) if den > 0.0 else 0.0)
        got = w.read()
        assert same_bits(got[dst], exp), (den, dst, got[dst], exp)
        s[dst] = exp
        assert same_bits(got, s), (den, dst, got)
        w.destroy()
    w = Window(ceed, np.arange(8.0))
    for dst, nm, dn in ((-1, 1, 2), (8, 1, 2), (3, -1, 2), (3, 8, 2), (3, 1, 8)):
        with pytest.raises(cd.CeedError, match="out of range"):
            L.CeedXScalarDivide(w.h, dst, nm, dn, 1.0)
        assert same_bits(w.read(), np.arange(8.0))
    w.destroy()


def fma_everywhere(got, a, x, c):
    """got_i == fma(a, x_i, c_i) bit for bit on EVERY entry.  Vectorised: a x_i = p + e exactly (two_prod), p + c_i = s + t exactly
    (two-sum), and s + fl(t + e) is the fused value unless the two roundings of the tail meet a tie; an entry where it differs from
    `got` is decided by the exact `fma` -- up to 64 of them, more than that is a kernel that does not compute this."""
    p, e = two_prod(np.full_like(x, a), x)
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    differ = np.flatnonzero((s + (t + e)).view(np.int64) != got.view(np.int64))
    return differ.size <= 64 and all(same_bits(got[i], fma(a, x[i], c[i])) for i in differ)


def axpby_scalars_case(ceed, n):
    """k_axpby_dev: a = sa * s[ia] and b = sb * s[ib], each rounded once (a negative index: the factor 1, so a = sa, b = sb), then
    y = a x + b y per entry, compared on EVERY entry, bit for bit.  The compiler may contract that sum; the correct evaluations are
    the unfused fl(fl(a x) + fl(b y)), fma(a, x, fl(b y)) and fma(b, y, fl(a x)).  The device build is pinned to the one it is
    compiled to -- v_mul_f64 of b y, then v_fmac_f64 with a and x in the kernel's loop, and the form the MI355X matched: fma(a, x,
    fl(b y)) -- so that a change of contraction is noticed; the oracle's compiler is free to choose, and one form gives all of its
    entries.  Besides, every entry lies within 2 u (|a x| + |b y|) of the exact a x + b y."""
    L = ceed.L
    rng = np.random.default_rng(n + 11)
    x, y0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    s = np.full(6, np.nan)
    s[1], s[4] = 1.7320508075688772, -0.5772156649015329
    X, S = Window(ceed, x), Window(ceed, s)
    for ia, ib in ((1, 4), (-1, 4), (1, -1), (-1, -3), (4, 4)):
        sa, sb = 0.7, -1.3
        a, b = sa * (1.0 if ia < 0 else s[ia]), sb * (1.0 if ib < 0 else s[ib])
        Y = Window(ceed, y0)
        L.CeedXVectorAXPBYScalars(Y.h, S.h, ia, sa, X.h, ib, sb)
        got = Y.read()
        assert np.all(np.abs(axpby_error(got, a, x, b, y0)) <= 2 * u * (np.abs(a * x) + np.abs(b * y0))), (n, ia, ib)
        if on_device(ceed):
            assert fma_everywhere(got, a, x, b * y0), (n, ia, ib)
        else:
            assert same_bits(got, a * x + b * y0) or fma_everywhere(got, a, x, b * y0) or fma_everywhere(got, b, y0, a * x), (n, ia, ib)
        assert same_bits(X.read(), x) and same_bits(S.read(), s)
        Y.destroy()
    Y = Window(ceed, y0)
    for args in ((Y.h, S.h, 6, 1.0, X.h, 1, 1.0), (Y.h, S.h, 1, 1.0, X.h, 6, 1.0), (Y.h, S.h, 1, 1.0, Y.h, 4, 1.0)):
        with pytest.raises(cd.CeedError):
            L.CeedXVectorAXPBYScalars(*args)
        assert same_bits(Y.read(), y0)
    for o in (X, Y, S):
        o.destroy()


# ---- on the oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_set_value_on_oracle(oracle, n):
    set_value_case(oracle, n)


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_reciprocal_on_oracle(oracle, n):
    reciprocal_case(oracle, n)


@pytest.mark.parametrize("entry", ["Start", "Update", "Step"])
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_chebyshev_entries_on_oracle(oracle, n, entry):
    cheb_case(oracle, n, entry)


def test_chebyshev_aliases_refused_on_oracle(oracle):
    cheb_alias_case(oracle)


def test_scalar_divide_on_oracle(oracle):
    scalar_divide_case(oracle)


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_axpby_scalars_on_oracle(oracle, n):
    axpby_scalars_case(oracle, n)


@pytest.mark.parametrize("name", list(SPMV))
def test_spmv_shapes_on_oracle(oracle, name):
    spmv_case(oracle, name)


def test_coo_assembly_on_oracle(oracle):
    coo_case(oracle)


@pytest.mark.parametrize("n", [4096, 4097])
def test_dense_product_on_oracle(oracle, n):
    dense_product_case(oracle, n)


@pytest.mark.parametrize("K", [64, 65, 4096, 4097])
def test_product_row_lengths_on_oracle(oracle, K):
    row_form_case(oracle, K)


def test_distributed_product_on_oracle(oracle):
    distributed_product_case(oracle)


def test_product_forms_agree_on_oracle(oracle):
    product_forms_agree_case(oracle)


@pytest.mark.parametrize("kind", ["positive", "mixed", "masked", "positive_masked"])
@pytest.mark.parametrize("n", DOT_SIZES)
def test_dot_on_oracle(oracle, n, kind):
    dot_case(oracle, n, kind, dot_depth_sequential)


@pytest.mark.parametrize("n", ELEM_SIZES)
def test_elementwise_helpers_on_oracle(oracle, n):
    elementwise_case(oracle, n)


def test_short_operands_refused_on_oracle(oracle):
    refusal_case(oracle)


# ---- on the device --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SPMV))
def test_spmv_shapes_on_device(gpu, name):
    spmv_case(gpu, name)


@pytest.mark.gpu
def test_recorded_spmv_replays_eager_bits_on_device(gpu):
    recorded_spmv_case(gpu, "Pt_band_middle")


@pytest.mark.gpu
def test_coo_assembly_on_device_matches_oracle(oracle, gpu):
    vo, vg = coo_case(oracle), coo_case(gpu)
    for a, b in zip(vo, vg):
        assert same_bits(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4096, 4097])
def test_dense_product_on_device(gpu, n):
    dense_product_case(gpu, n)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [64, 65, 4096, 4097])
def test_product_row_lengths_on_device(gpu, K):
    row_form_case(gpu, K)


@pytest.mark.gpu
def test_distributed_product_on_device(gpu):
    distributed_product_case(gpu)


@pytest.mark.gpu
def test_product_forms_agree_on_device(gpu):
    product_forms_agree_case(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["positive", "mixed", "masked", "positive_masked"])
@pytest.mark.parametrize("n", DOT_SIZES)
def test_dot_on_device(gpu, n, kind):
    dot_case(gpu, n, kind, dot_depth_device)


@pytest.mark.gpu
@pytest.mark.parametrize("n", ELEM_SIZES)
def test_elementwise_helpers_on_device(gpu, n):
    elementwise_case(gpu, n)


@pytest.mark.gpu
def test_short_operands_refused_on_device(gpu):
    refusal_case(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_set_value_on_device(gpu, n):
    set_value_case(gpu, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_reciprocal_on_device(gpu, n):
    reciprocal_case(gpu, n)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["Start", "Update", "Step"])
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_chebyshev_entries_on_device(gpu, n, entry):
    cheb_case(gpu, n, entry)


@pytest.mark.gpu
def test_chebyshev_aliases_refused_on_device(gpu):
    cheb_alias_case(gpu)


@pytest.mark.gpu
def test_scalar_divide_on_device(gpu):
    scalar_divide_case(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_axpby_scalars_on_device(gpu, n):
    axpby_scalars_case(gpu, n)
