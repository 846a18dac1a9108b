"""krylov.py on both backends through ceed.Csr: no mesh, no operator.  The device-scalar Lanczos recurrence against its restatement
in NumPy float64 (same order of operations, sums taken front to back as the oracle takes them), its breakdown and its empty case,
the weighted dots, and the Chebyshev coefficients against their closed forms."""
import functools

import numpy as np
import pytest

from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.krylov import chebyshev_coefficients, lanczos_device, lanczos_emax
from conftest import rel_err

# host against device coefficients, as tests/test_solver.py::lanczos_paths_agree has them
TOL = {"oracle": 1e-15, "gpu": 1e-12}


@pytest.fixture(params=["oracle", pytest.param("gpu", marks=pytest.mark.gpu)])
def backend(request):
    return request.getfixturevalue(request.param), TOL[request.param]


def laplacian_1d(n):
    """(rowptr, cols, vals) of tridiag(-1, 2, -1)."""
    rows = [[(j, 2.0 if j == i else -1.0) for j in (i - 1, i, i + 1) if 0 <= j < n] for i in range(n)]
    rowptr = np.cumsum([0] + [len(r) for r in rows])
    return rowptr, np.array([j for r in rows for j, _ in r]), np.array([v for r in rows for _, v in r])


def dense(rowptr, cols, vals):
    n = rowptr.size - 1
    A = np.zeros((n, n))
    for i in range(n):
        A[i, cols[rowptr[i]:rowptr[i + 1]]] = vals[rowptr[i]:rowptr[i + 1]]
    return A


def seq_dot(a, b):
    s = 0.0
    for p in a * b:
        s += p
    return float(s)


def lanczos_numpy(csr, dinv, x0, steps):
    """The recurrence of krylov.lanczos_device in NumPy float64, CeedXScalarDivide's rule included (a non-positive denominator
    gives 0), cut like the device lists: before the first non-positive alpha or non-finite beta."""
    rowptr, cols, vals = csr

    def A(x):
        return np.array([seq_dot(vals[rowptr[i]:rowptr[i + 1]], x[cols[rowptr[i]:rowptr[i + 1]]]) for i in range(x.size)])
    div = lambda num, den: num / den if den > 0.0 else 0.0
    r = 1.0 * x0 + 0.0 * np.zeros_like(x0)
    z = r * dinv
    p = z.copy()
    rz = seq_dot(r, z)
    coef = []
    for _ in range(steps):
        Ap = A(p)
        alpha = div(rz, seq_dot(p, Ap))
        r = -alpha * Ap + 1.0 * r
        z = r * dinv
        rz_new = seq_dot(r, z)
        beta = div(rz_new, rz)
        p = 1.0 * z + beta * p
        rz = rz_new
        coef.append((alpha, beta))
    alphas, betas = [], []
    for alpha, beta in coef:
        if not (alpha > 0.0) or not np.isfinite(beta):
            break
        alphas.append(alpha); betas.append(beta)
    return alphas, betas


@functools.lru_cache(maxsize=None)
def reference(n, start, steps=10):
    """(csr, dinv, x0, NumPy coefficients) of the 1-D Laplacian with its Jacobi preconditioner: computed once, shared by the backends."""
    csr = laplacian_1d(n)
    dinv = np.full(n, 0.5)
    if start == "random":
        x0 = np.random.default_rng(50).uniform(-1.0, 1.0, n)
        x0 /= np.sqrt(np.square(x0).sum())
    else:
        x0 = np.full(n, {"ones": 1.0, "zero": 0.0}[start])
    for a in csr + (dinv, x0):
        a.setflags(write=False)
    return csr, dinv, x0, lanczos_numpy(csr, dinv, x0, steps)


def run(ceed, n, start, steps=10, weighted=False):
    (rowptr, cols, vals), dinv, x0, _ = reference(n, start, steps)
    A = cd.Csr.rect(ceed, n, n, rowptr, cols, vals)
    v = {k: ceed.vector(n).set_value(0.0) for k in ("r", "z", "p", "Ap")}
    v["x0"], v["dinv"] = ceed.vector(n).set_array(x0), ceed.vector(n).set_array(dinv)
    if weighted:
        v["w"] = ceed.vector(n).set_value(1.0)
    out = lanczos_device(ceed, A.apply, lambda z, r: z.pointwise_mult(r, v["dinv"]), v["x0"], v["r"], v["z"], v["p"], v["Ap"], steps,
                         weight=v.get("w"))
    for o in list(v.values()) + [A]:
        o.destroy()
    return out


def test_coefficients_against_the_numpy_recurrence(backend):
    ceed, tol = backend
    alphas, betas = run(ceed, 50, "random")
    want_a, want_b = reference(50, "random")[3]
    assert len(want_a) == 10 and len(alphas) == len(betas) == 10
    ea, eb = rel_err(np.array(alphas), np.array(want_a)), rel_err(np.array(betas), np.array(want_b))
    print(f"n = 50, 10 steps: alphas {ea:.2e}, betas {eb:.2e} from the NumPy recurrence (allowed {tol:.0e})")
    assert ea < tol and eb < tol
    A = dense(*reference(50, "random")[0])
    lam = np.linalg.eigvalsh(A / 2.0).max()                     # D^-1/2 A D^-1/2 with D = 2 I
    emax = lanczos_emax(alphas, betas)
    print(f"emax {emax:.6f}, largest eigenvalue {lam:.6f}")
    assert 0.7 * lam < emax <= 1.05 * lam                       # a Ritz value: a lower bound, close (as tests/test_amg.py asserts)


def test_lists_are_cut_where_the_recurrence_breaks_down(backend):
    """n = 4 from the vector of ones: every number of the recurrence is a small dyadic rational, the residual is exactly zero after
    two steps, and the third alpha is 0 / 0 -> 0 by CeedXScalarDivide's rule."""
    ceed, tol = backend
    want_a, want_b = reference(4, "ones")[3]
    assert (want_a, want_b) == ([4.0, 1.0], [1.0, 0.0])        # the restatement itself breaks down within the 10 steps
    alphas, betas = run(ceed, 4, "ones")
    assert len(alphas) == len(betas) == 2
    assert rel_err(np.array(alphas), np.array(want_a)) < tol and rel_err(np.array(betas), np.array(want_b)) < tol
    assert np.isfinite(lanczos_emax(alphas, betas))


def test_zero_start_vector_gives_empty_lists(backend):
    ceed, _ = backend
    alphas, betas = run(ceed, 50, "zero")
    assert alphas == [] and betas == [] and reference(50, "zero")[3] == ([], [])
    assert lanczos_emax(alphas, betas) == 1.0


def test_weight_of_ones_gives_the_bits_of_no_weight(backend):
    ceed, _ = backend
    assert run(ceed, 50, "random", weighted=True) == run(ceed, 50, "random")


def test_chebyshev_coefficients_closed_forms():
    """emax = 2, lmin_frac = 0.1: the interval [0.2, 2.2], theta = 1.2, delta = 1, sigma = 1.2.  With the Chebyshev polynomials
    T_0 .. T_3 (sigma) = 1, 1.2, 1.88, 3.312: c1_0 = 1 / theta, c1_k = 2 T_k / (delta T_k+1), c2_k = T_k-1 / T_k+1.  A dozen
    roundings without cancellation lie between the two forms: 1e-14 relative."""
    got = list(chebyshev_coefficients(2.0, 0.1, 3))
    want = [(5.0 / 6.0, 0.0), (60.0 / 47.0, 25.0 / 47.0), (235.0 / 207.0, 25.0 / 69.0)]
    assert len(got) == 3 and got[0][1] == 0.0
    for (c1, c2), (w1, w2) in zip(got, want):
        assert c1 == pytest.approx(w1, rel=1e-14) and c2 == pytest.approx(w2, rel=1e-14, abs=0.0)
    one = list(chebyshev_coefficients(2.0, 0.1, 1))
    assert len(one) == 1 and one[0][1] == 0.0 and one[0][0] == pytest.approx(5.0 / 6.0, rel=1e-14)
