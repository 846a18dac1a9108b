"""krylov.py on both backends through ceed.Csr: no mesh, no operator.  The device-scalar Lanczos recurrence against its restatement
in NumPy float64 (same order of operations, sums taken front to back as the oracle takes them), its breakdown and its empty case,
the weighted dots, the Chebyshev coefficients against their closed forms, and the host-scalar CG (krylov.pcg) on a dense matrix of
order 9: its solution, its coefficients against lanczos_device's, an indefinite matrix, and the run without an iterate."""
import functools

import numpy as np
import pytest

from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.krylov import chebyshev_coefficients, lanczos_device, lanczos_emax, pcg
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


# ---- krylov.pcg: a dense matrix of order 9 with its Jacobi preconditioner -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense9(kind):
    """(A, b): A = Q diag(lambda) Q^T with a random orthogonal Q; "spd": lambda = 1 .. 10, "indefinite": three of them negative (the
    diagonal, which the preconditioner inverts, stays positive: checked)."""
    rng = np.random.default_rng(9)
    Q, _ = np.linalg.qr(rng.standard_normal((9, 9)))
    lam = np.linspace(1.0, 10.0, 9)
    if kind == "indefinite":
        lam[[1, 4, 7]] *= -0.2
    A = (Q * lam) @ Q.T
    A = 0.5 * (A + A.T)
    assert np.all(np.diag(A) > 0.1)
    b = rng.uniform(-1.0, 1.0, 9)
    A.setflags(write=False); b.setflags(write=False)
    return A, b


def run_pcg(ceed, kind, rtol, maxit, iterate=True):
    """krylov.pcg on Ceed vectors; returns (its, alphas, betas, x or None, b after the call, the four work vectors after the call)"""
    A, b = dense9(kind)
    M = cd.Csr.rect(ceed, 9, 9, np.arange(0, 82, 9), np.tile(np.arange(9), 9), A.reshape(-1))
    v = {k: ceed.vector(9).set_value(0.0) for k in ("x", "r", "z", "d", "t")}
    v["b"], v["dinv"] = ceed.vector(9).set_array(b), ceed.vector(9).set_array(1.0 / np.diag(A))
    its, alphas, betas = pcg(M.apply, lambda z, r: z.pointwise_mult(r, v["dinv"]), lambda p, q: p.dot(q), v["b"],
                             v["x"] if iterate else None, v["r"], v["z"], v["d"], v["t"], rtol, maxit)
    out = (its, alphas, betas, v["x"].to_numpy(), v["b"].to_numpy(), [v[k].to_numpy() for k in ("r", "z", "d", "t")])
    for o in list(v.values()) + [M]:
        o.destroy()
    return out


def test_pcg_solves_to_the_bound_of_its_stop_rule(backend):
    """The stop rule r . D^-1 r <= rtol^2 b . D^-1 b gives |r| <= sqrt(dmax / dmin) rtol |b|, and |x - x*| <= |A^-1| |r|,
    |b| <= |A| |x*|: |x - x*| / |x*| <= cond(A) sqrt(dmax / dmin) rtol.  The recurrence's r drifts from b - A x by rounding, a few
    u |A| |x| per step (Greenbaum); 20 steps' worth at 10 u each is allowed for: + 200 u cond(A)."""
    ceed, _ = backend
    A, b = dense9("spd")
    d = np.diag(A)
    bound = np.linalg.cond(A) * np.sqrt(d.max() / d.min()) * 1e-13 + 200 * 2.0 ** -53 * np.linalg.cond(A)
    assert bound <= 1e-10
    its, alphas, betas, x, _, _ = run_pcg(ceed, "spd", 1e-13, 50)
    want = np.linalg.solve(A, b)
    err = np.linalg.norm(x - want) / np.linalg.norm(want)
    print(f"order 9, cond {np.linalg.cond(A):.1f}: {its} steps, |x - x*| / |x*| = {err:.2e} (bound {bound:.2e})")
    assert its == len(alphas) == len(betas) and 0 < its < 50           # the stop rule ended it, not the step limit
    assert err <= bound


def test_pcg_coefficients_are_those_of_lanczos_device(backend):
    ceed, tol = backend
    A, b = dense9("spd")
    steps = 6
    its, alphas, betas, x, _, _ = run_pcg(ceed, "spd", 0.0, steps, iterate=False)
    assert its == steps
    M = cd.Csr.rect(ceed, 9, 9, np.arange(0, 82, 9), np.tile(np.arange(9), 9), A.reshape(-1))
    v = {k: ceed.vector(9).set_value(0.0) for k in ("r", "z", "p", "Ap")}
    v["b"], v["dinv"] = ceed.vector(9).set_array(b), ceed.vector(9).set_array(1.0 / np.diag(A))
    want_a, want_b = lanczos_device(ceed, M.apply, lambda z, r: z.pointwise_mult(r, v["dinv"]), v["b"], v["r"], v["z"], v["p"], v["Ap"], steps)
    for o in list(v.values()) + [M]:
        o.destroy()
    ea, eb = rel_err(np.array(alphas), np.array(want_a)), rel_err(np.array(betas), np.array(want_b))
    print(f"order 9, {steps} steps: alphas {ea:.2e}, betas {eb:.2e} from lanczos_device (allowed {tol:.0e})")
    assert len(want_a) == steps and ea < tol and eb < tol


def test_pcg_on_an_indefinite_matrix_ends_with_finite_output(backend):
    ceed, _ = backend
    A, _ = dense9("indefinite")
    assert np.linalg.eigvalsh(A).min() < -0.1
    its, alphas, betas, x, _, work = run_pcg(ceed, "indefinite", 1e-13, 50)
    print(f"indefinite, order 9: ended after {its} steps")
    assert its < 50 and all(a > 0.0 for a in alphas)                   # a direction of non-positive curvature ended it
    assert np.all(np.isfinite(alphas)) and np.all(np.isfinite(betas)) and np.all(np.isfinite(x))
    assert all(np.all(np.isfinite(w)) for w in work)


def test_pcg_without_an_iterate_writes_the_work_vectors_only(backend):
    ceed, _ = backend
    _, b = dense9("spd")
    its, alphas, betas, x, b_after, work = run_pcg(ceed, "spd", 0.0, 6, iterate=False)
    with_x = run_pcg(ceed, "spd", 0.0, 6, iterate=True)
    assert np.array_equal(b_after, b) and not x.any()                  # the vector not handed over stayed as it was made
    assert (its, alphas, betas) == with_x[:3] and with_x[3].any()      # the iterate does not enter the coefficients
    assert all(np.array_equal(p, q) for p, q in zip(work, with_x[5]))
