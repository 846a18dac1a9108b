"""Dense references for the p-multigrid V-cycle of solver.NewtonPMG (Chebyshev smoother, transfers, coarse solves, the aggregation
hierarchy under an assembled level) and for the flexible PCG around it, and the checks that use them; shared by
tests/test_vcycle_dense.py (the CPU oracle, with the controls) and tests/test_vcycle_dense_gpu.py (the device).  Every function takes
the Ceed under test and the oracle's Ceed: level matrices and transfers are formed on a problem and solver of the ORACLE linearised at
the same host array U, and reach the comparison as host arrays only.

With a fixed coarse solve the V-cycle is ONE linear operator B on the free dofs, and it has a closed form that runs none of the
project's recurrences (all plain NumPy / SciPy in float64):

  level matrices  A_lv: unit-vector applies of the oracle solver's A(lv, . , .), free-free block
  transfers       P_lv, R_lv: unit-vector applies of the oracle problem's prolong(lv) / restrict(lv), free rows and columns
  smoother        k Chebyshev steps on [lmin, lmax] with preconditioner M have the error propagator E = p_k(M^-1 A),
                  p_k(l) = T_k((theta - l) / delta) / T_k(theta / delta); with A v = l M v, V^T M V = I (scipy.linalg.eigh(A, M)):
                  E = V p_k(L) V^T M,  (I - E) A^-1 = V (1 - p_k(L)) / L V^T,  A E A^-1 = E^T
  V-cycle         B_lv = (I - E (I - P B_{lv-1} P^T A_lv) E) A_lv^-1 = V (1 - p_k(L)^2) / L V^T + E P B_{lv-1} P^T E^T
  coarsest level  (I - p_k(D^-1 A_0)) A_0^-1 ("chebyshev", "assembled"), A_0^-1 ("cg"), or the two-sided form again through the
                  aggregation levels ("amg"): prolongators read back as given, Galerkin matrices P_a^T A P_a formed HERE, the inner
                  cycle's error propagator to the power coarse_cycles, the last level inverted
  PCG             solver.fcg's rule with dense A and B: Polak-Ribiere beta, natural-norm test r . z <= rtol^2 r_0 . z_0

lmin / lmax are lmin_frac emax and 1.1 emax with emax READ from the solver under test: a parameter of the polynomial, checked on its
own against the dense eigenproblem (emax_check)."""
import numpy as np
import scipy.linalg

import _newmark_dense as nd
from _mass_common import dense_from_applies
from _numbering import distorted_box
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG

TOL_ORACLE = 1e-12           # the oracle reproduces the closed form to 7e-15; two and a half orders for another libm / LAPACK
TOL_DEVICE = 1e-10           # the project's device-against-oracle bound (tests/_newmark_dense.py)
TOL_SYM = 1e-12
SENTINEL = 7.25

# name -> problem, distorted_box sizes, degree, level ladder, degrees of the levels, free dofs, solver options.
# The Chebyshev coarse solves (a, b, e) take 100 steps, not the solver's default 40: the coarse polynomial 1 - p_k overshoots 1 by up
# to 1 / T_k(theta / delta) on the coarse modes (1e-3 at k = 40 on [emax / 100, 1.1 emax]), which puts lambda_max(B_ref A) at
# 1 + 1.2e-6 ... 1 + 1.7e-6 with the default (measured; B itself agrees with B_ref to 2e-15 there too) -- over LAMBDA_MAX, a condition on
# the fixtures.  With 100 steps it is 1 + 1e-11; lambda_min, cond(A) and the fcg counts (16, 19, 15) are those of the default.
CHEB = dict(coarse_cheb_its=100)
CASES = {
    "a": dict(problem="hyperFS", box=(2, 1, 1), degree=3, multigrid="uniform", degrees=[1, 2, 3], free=252, opts=dict(coarse="chebyshev", **CHEB)),
    "b": dict(problem="hyperFS", box=(2, 1, 1), degree=4, multigrid="logarithmic", degrees=[1, 2, 4], free=540, opts=dict(coarse="assembled", **CHEB)),
    "c": dict(problem="hyperFS", box=(3, 2, 2), degree=2, multigrid="logarithmic", degrees=[1, 2], free=420, opts=dict(coarse="amg")),
    # level 0 only: sol.vcycle(0, b, x) over the 525 rows of the p = 1 level, aggregation hierarchy 525 -> 72 -> 6
    "d1": dict(problem="hyperFS", box=(6, 4, 4), degree=2, multigrid="logarithmic", degrees=[1, 2], free=420, level0=True, amg_rows=[525, 72, 6],
               opts=dict(coarse="amg", amg_max_coarse_dofs=30, amg_coarse_cycles=1)),
    "d2": dict(problem="hyperFS", box=(6, 4, 4), degree=2, multigrid="logarithmic", degrees=[1, 2], free=420, level0=True, amg_rows=[525, 72, 6],
               opts=dict(coarse="amg", amg_max_coarse_dofs=30, amg_coarse_cycles=2)),
    "e": dict(problem="hyperFS", box=(2, 1, 1), degree=3, multigrid="uniform", degrees=[1, 2, 3], free=252,
              opts=dict(coarse="chebyshev", smoother="pbjacobi", **CHEB)),
    "f": dict(problem="hyperSS", box=(2, 2, 1), degree=3, multigrid="uniform", degrees=[1, 2, 3], free=441, opts=dict(coarse="cg", coarse_rtol=1e-14)),
    # the two-element linElas box: lambda_min(B_ref A) = 0.267 was measured, so it is held to the upper bound only
    "g": dict(problem="linElas", box=(2, 1, 1), degree=2, multigrid="logarithmic", degrees=[1, 2], free=90, quality="upper",
              opts=dict(coarse="cg", coarse_rtol=1e-14)),
    # NewmarkPMG after two steps (its own start): levels from its own A(lv) = K_lv + a0 rho M_lv
    "h": dict(newmark=True, degrees=[1, 2, 3], opts=dict(coarse="amg")),
    # case a with the solver's DEFAULT coarse polynomial (40 steps): everything but the quality of the reference (see above)
    "a40": dict(problem="hyperFS", box=(2, 1, 1), degree=3, multigrid="uniform", degrees=[1, 2, 3], free=252, quality=None,
                opts=dict(coarse="chebyshev")),
}
LAMBDA_MIN = 0.3             # quality of the REFERENCE as a preconditioner: a condition on the fixtures
LAMBDA_MAX = 1.0 + 1e-8


relmax = nd.relmax           # max |got - want| / max |want|


def asymmetry(B):
    return float(np.abs(B - B.T).max() / np.abs(B).max())


# ---- 1. dense references ------------------------------------------------------------------------------------------------------------
def chebyshev_polynomial(lam, lmin, lmax, k):
    """p_k(lam) = T_k((theta - lam) / delta) / T_k(theta / delta): cos form inside [-1, 1], cosh form outside."""
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)

    def T(t):
        t = np.asarray(t, dtype=np.float64)
        a = np.abs(t)
        inside = np.cos(k * np.arccos(np.clip(t, -1.0, 1.0)))
        outside = np.cosh(k * np.arccosh(np.maximum(a, 1.0))) * np.where((t < 0) & (k % 2 == 1), -1.0, 1.0)
        return np.where(a <= 1.0, inside, outside)
    return T((theta - lam) / delta) / T(theta / delta)


def smoother_factors(A, M, lmin, lmax, k):
    """(E, S1, S2, lam) of k Chebyshev steps on [lmin, lmax] preconditioned with M: E = p_k(M^-1 A), S1 = (I - E) A^-1 (the sweep from
    a zero guess), S2 = (I - E E) A^-1 (pre- and post-sweep without a coarse correction), lam the eigenvalues of M^-1 A."""
    lam, V = scipy.linalg.eigh(A, M)
    p = chebyshev_polynomial(lam, lmin, lmax, k)
    E = (V * p) @ V.T @ M
    return E, (V * ((1.0 - p) / lam)) @ V.T, (V * ((1.0 - p * p) / lam)) @ V.T, lam


def two_sided(E, S2, P, Bc):
    """(I - E (I - P Bc P^T A) E) A^-1 = S2 + E P Bc P^T E^T   (A E A^-1 = E^T)."""
    EP = E @ P
    return S2 + EP @ Bc @ EP.T


def spd_inverse(A):
    A = 0.5 * (A + A.T)
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(A), np.eye(A.shape[0]))


def smoother_matrix(sol, A, node_of):
    """M of the level's smoother: diag(A), or the nodal blocks of A on the free components ("pbjacobi")."""
    if sol.smoother == "jacobi":
        return np.diag(np.diag(A))
    return np.where(node_of[:, None] == node_of[None, :], A, 0.0)


def csr_dense(csr, ceed):
    """A library CSR matrix (amg.py's prolongators) read back as given."""
    nr, nc, nz, rp, cl = csr.pattern()
    vals = csr.values(ceed)
    out = np.zeros((nr, nc))
    rows = np.repeat(np.arange(nr), np.diff(rp))
    np.add.at(out, (rows, cl[:nz]), vals[:nz])
    return out


def level_matrices(rsol, top=None):
    """Per level (up to ``top``, default the finest) of the ORACLE solver ``rsol`` in its current linearisation: dict(A, P, R, free,
    node_of); A the free-free block of A(lv, . , .), P / R the free blocks of prolong(lv) / restrict(lv) (level 0 has none)."""
    prob, ceed = rsol.p, rsol.ceed
    out = []
    for lv in range((rsol.nlev - 1 if top is None else top) + 1):
        n = prob.lsize(lv)
        fr = np.flatnonzero(prob.levels[lv].mask == 0)
        A = dense_from_applies(ceed, n, lambda x, y: rsol.A(lv, x, y), fr)
        assert not A[prob.levels[lv].mask != 0].any()                     # free columns reach no constrained row
        m = dict(A=A[fr], free=fr, node_of=fr // 3, n=n, P=None, R=None)
        if lv > 0:
            nc, frc = prob.lsize(lv - 1), out[-1]["free"]
            X, Y = ceed.vector(nc), ceed.vector(n)
            P = np.zeros((n, frc.size))
            for k, j in enumerate(frc):
                e = np.zeros(nc); e[j] = 1.0
                X.set_array(e); prob.prolong(lv, X, Y)
                P[:, k] = Y.to_numpy()
            X.destroy(); Y.destroy()
            X, Y = ceed.vector(n), ceed.vector(nc)
            R = np.zeros((nc, fr.size))
            for k, j in enumerate(fr):
                e = np.zeros(n); e[j] = 1.0
                X.set_array(e); prob.restrict(lv, X, Y)
                R[:, k] = Y.to_numpy()
            X.destroy(); Y.destroy()
            assert not P[prob.levels[lv].mask != 0].any() and not R[prob.levels[lv - 1].mask != 0].any()     # masked rows are dropped
            m["P"], m["R"] = P[fr], R[frc]
        out.append(m)
    return out


def amg_reference(sol, A0, E0, S20, free0, figures):
    """Level 0 under ``coarse="amg"``: the solver's own sweeps (E0, S20) around the correction P_a B_c P_a^T through amg.levels."""
    amg = sol.amg
    Ps = [csr_dense(l.P, sol.ceed) for l in amg.levels]
    assert not np.delete(Ps[0], free0, axis=0).any()                     # constrained rows of the first prolongator are zero

    def below(i, A):
        """What the hierarchy applies for A^-1, A the matrix under transfer i - 1 (amg.levels[i - 1].Anext)."""
        up, lv = amg.levels[i - 1], amg.levels[i]
        E, _, S2, lam = smoother_factors(A, np.diag(np.diag(A)), up.emax / amg.smooth_ratio, 1.1 * up.emax, amg.smooth_its)
        figures["emax"].append((f"aggregation level {i}", up.emax, float(lam.max())))
        P = Ps[i]
        Ac = P.T @ A @ P
        Bc = spd_inverse(Ac) if lv.dense_next else below(i + 1, Ac)
        B1 = two_sided(E, S2, P, Bc)
        Ec, Bk, Ej = np.eye(A.shape[0]) - B1 @ A, B1.copy(), np.eye(A.shape[0])
        for _ in range(1, amg.coarse_cycles):                               # (I - Ec^k) A^-1 = (I + Ec + ... + Ec^(k-1)) B1
            Ej = Ej @ Ec
            Bk = Bk + Ej @ B1
        return Bk
    P = Ps[0][free0]
    Ac = P.T @ A0 @ P
    Bc = spd_inverse(Ac) if amg.levels[0].dense_next else below(1, Ac)
    return two_sided(E0, S20, P, Bc)


def vcycle_reference(sol, mats, top=None):
    """(B_ref of level ``top`` (default: the finest), figures): the recursion of the module docstring with the level matrices
    ``mats`` (level_matrices of the oracle) and emax / the aggregation prolongators of ``sol``, the solver under test."""
    top = sol.nlev - 1 if top is None else top
    figures = dict(emax=[])
    m = mats[0]
    M = smoother_matrix(sol, m["A"], m["node_of"])
    if sol.nlev == 1:
        return spd_inverse(M), figures
    if sol.amg is not None:
        E, _, S2, lam = smoother_factors(m["A"], M, sol.emax[0] / sol.amg_smooth_ratio, 1.1 * sol.emax[0], sol.amg_smooth_its)
        B = amg_reference(sol, m["A"], E, S2, m["free"], figures)
    elif sol.coarse in ("chebyshev", "assembled"):
        _, B, _, lam = smoother_factors(m["A"], M, sol.emax[0] / sol.coarse_cheb_ratio, 1.1 * sol.emax[0], sol.coarse_cheb_its)
    else:
        B, lam = spd_inverse(m["A"]), scipy.linalg.eigh(m["A"], M, eigvals_only=True)
    figures["emax"].append(("level 0", sol.emax[0], float(lam.max())))
    for lv in range(1, top + 1):
        m = mats[lv]
        M = smoother_matrix(sol, m["A"], m["node_of"])
        E, _, S2, lam = smoother_factors(m["A"], M, 0.1 * sol.emax[lv], 1.1 * sol.emax[lv], sol.smooth_its)
        figures["emax"].append((f"level {lv}", sol.emax[lv], float(lam.max())))
        B = two_sided(E, S2, m["P"], B)                                     # (R = P^T exactly: transfers_check)
    return B, figures


def dense_pcg(A, B, b, rtol, maxit=499):
    """solver.fcg's rule with dense A and B; returns (x, iterations)."""
    x = np.zeros_like(b)
    r = b.copy()
    z = B @ r
    p = z.copy()
    rz = rz0 = float(r @ z)
    its = 0
    if rz0 <= 0.0:
        return x, 0
    for its in range(1, maxit + 1):
        Ap = A @ p
        alpha = rz / float(p @ Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        r_zold = float(r @ z)
        z = B @ r
        rz_new = float(r @ z)
        if rz_new <= rtol ** 2 * rz0:
            break
        p = z + ((rz_new - r_zold) / rz) * p
        rz = rz_new
    return x, its


# ---- 2. the operator under test ------------------------------------------------------------------------------------------------------
def build(ceed, name, U=None):
    """(problem, solver) of case ``name`` on ``ceed``, linearised at ``U`` (default: smooth_state(0.1) on the free dofs; case h: its
    own state after two Newmark steps), the preconditioner set up."""
    case = CASES[name]
    if case.get("newmark"):
        prob, sol = nd.hyperfs_solver(ceed, 3, 2, **case["opts"])
        if U is not None:
            sol._set(sol.U, U)
    else:
        prob = SolidProblem(ceed, distorted_box(*case["box"]), case["degree"], case["problem"], nu=0.3, E=1.0, bc_sides=[1],
                            multigrid=case["multigrid"])
        sol = NewtonPMG(prob, **case["opts"])
        sol._set(sol.U, prob.smooth_state(0.1) * sol.free if U is None else U)
        assert int(sol.free.sum()) == case["free"] or case.get("level0")
    assert [lv.degree for lv in prob.levels] == case["degrees"]
    sol.residual(sol.U, sol.R)
    sol.setup_preconditioner()
    return prob, sol


def teardown(prob, sol):
    sol.destroy()
    prob.destroy()


def operator_io(sol, level0):
    """(right-hand side, result, run, mask) of the operator under test: precondition(r, z) on the vectors fcg hands it, or
    vcycle(0, b, x) on level 0's own (case d)."""
    if level0:
        r, z = sol.w[0]["b"], sol.w[0]["x"]
        return r, z, (lambda: sol.vcycle(0, r, z)), sol.p.levels[0].mask != 0
    r, z = sol.w[sol.nlev - 1]["b"], sol.kz
    return r, z, (lambda: sol.precondition(r, z)), ~sol.free


def columns(sol, cols, level0=False, run=None):
    """Columns ``cols`` (indices into the free dofs) of the operator under test on the free dofs; constrained entries of every
    result must be exactly zero."""
    r, z, run0, mask = operator_io(sol, level0)
    run = run or run0
    fr = np.flatnonzero(~mask)
    on_device = sol.ceed.preferred_memtype == cd.MEM_DEVICE
    B = np.zeros((fr.size, len(cols)))
    e = np.zeros(mask.size)
    for k, j in enumerate(cols):
        e[fr[j]] = 1.0
        sol._set(r, e)
        if on_device:
            r.device_pointer()               # on the device before a replayed recording reads it
        z.set_value(3.0)                     # every entry is to be written; and no host copy of an earlier result is left to be read
        e[fr[j]] = 0.0
        run()
        y = z.to_numpy()
        assert not y[mask].any(), f"column {j}: constrained entries of the result are not zero"
        B[:, k] = y[fr]
    return B


# ---- 3. the checks -----------------------------------------------------------------------------------------------------------------
def transfers_check(mats):
    """R_lv == P_lv^T exactly (the oracle measured 0.0)."""
    for lv, m in enumerate(mats):
        if lv:
            assert np.array_equal(m["R"], m["P"].T), (lv, float(np.abs(m["R"] - m["P"].T).max()))
            assert np.abs(m["P"]).max() > 0


def affine_prolongation_check(ceed, degree, multigrid, tag):
    """On an undistorted SHEARED box (affine elements) the prolongation maps the nodal values of u = a + B x on the coarse level to
    those on the fine level at every free node, to 1e-13 -- the one check of P that does not come from the project's transfer code.
    Twice: without a clamped side (any a, B: every node is free), and with side 1 clamped (the plane z = 0, which the shear keeps)
    and a field that vanishes on it (u = c z: the masked coarse entries read as zero ARE its boundary values)."""
    worst = 0.0
    rng = np.random.default_rng(17)
    S = np.array([[1.0, 0.2, 0.3], [0.0, 1.0, 0.1], [0.0, 0.0, 1.0]])
    for bc in ([], [1]):
        mesh = box_mesh(2, 2, 1)
        mesh.coords = mesh.coords @ S.T
        prob = SolidProblem(ceed, mesh, degree, "linElas", nu=0.3, E=1.0, bc_sides=bc, multigrid=multigrid)
        a, Bm = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, (3, 3))
        if bc:
            a, Bm = np.zeros(3), np.outer(rng.uniform(-1, 1, 3), [0.0, 0.0, 1.0])
        field = lambda lv: (a + prob.levels[lv].dofmap.node_coords @ Bm.T).reshape(-1)
        for lv in range(1, len(prob.levels)):
            free = prob.levels[lv].mask == 0
            assert bool(bc) == bool((~free).any())
            X, Y = ceed.vector(prob.lsize(lv - 1)).set_array(field(lv - 1)), ceed.vector(prob.lsize(lv)).set_value(3.0)
            prob.prolong(lv, X, Y)
            got, want = Y.to_numpy(), field(lv)
            assert not got[~free].any() and np.abs(want[free]).max() > 0.1
            err = float(np.abs(got - want)[free].max())
            print(f"VCYCLE {tag} affine field through prolong({lv}) (degrees {prob.levels[lv - 1].degree} -> {prob.levels[lv].degree}, "
                  f"clamped sides {bc}): max |P u_c - u_f| on the free nodes = {err:.2e}")
            worst = max(worst, err)
            X.destroy(); Y.destroy()
        prob.destroy()
    assert worst <= 1e-13, worst
    return worst


def emax_check(figures, tag):
    """1.1 emax >= lambda_max(M^-1 A) (else the Chebyshev interval leaves the top modes out and |p_k| > 1 there) and
    emax <= lambda_max (1 + 1e-10) (Ritz values lie inside the spectrum), on every level that smooths."""
    ratios = []
    for where, emax, lmax in figures["emax"]:
        ratios.append(emax / lmax)
        assert 1.1 * emax >= lmax, (tag, where, emax, lmax)
        assert emax <= lmax * (1.0 + 1e-10), (tag, where, emax, lmax)
    return ratios


def spectrum_of_product(B, A):
    """Eigenvalues of B A, from the similar matrix L^T B L with A = L L^T."""
    L = np.linalg.cholesky(0.5 * (A + A.T))
    return np.linalg.eigvals(L.T @ B @ L)


def reference_for(ceed, oracle, name, sol):
    """The level matrices of the oracle's solver linearised at the state of ``sol`` (of ``sol`` itself on the oracle)."""
    top = 0 if CASES[name].get("level0") else None
    if ceed is oracle:
        return level_matrices(sol, top)
    rprob, rsol = build(oracle, name, U=sol.U.to_numpy())
    mats = level_matrices(rsol, top)
    teardown(rprob, rsol)
    return mats


def measure(sol, A, B_ref, level0):
    """The figures of the matrix under test against B_ref: error, asymmetry, definiteness, the spectrum of B A."""
    B = columns(sol, range(A.shape[0]), level0)
    err, asym = relmax(B, B_ref), asymmetry(B)
    lmin_sym = float(np.linalg.eigvalsh(0.5 * (B + B.T)).min())
    ev = spectrum_of_product(B, A)
    return dict(B=B, error=err, asymmetry=asym, lmin_sym=lmin_sym, ev=ev)


def vcycle_check(ceed, oracle, name, tag, pcg=True):
    """Items 1-3 for one case: B against the closed form, symmetry and definiteness of the matrix under test, the quality of the
    reference, the eigenvalue estimates, and fcg against the dense PCG.  Returns the figures."""
    case = CASES[name]
    level0 = bool(case.get("level0"))
    device = ceed is not oracle
    tol = TOL_DEVICE if device else TOL_ORACLE
    prob, sol = build(ceed, name)
    if name == "h":
        assert np.abs(sol.U.to_numpy()).max() > 1e-3
    if "amg_rows" in case:
        assert sol.amg.info["levels"] == 3 and sol.amg.info["rows"] == case["amg_rows"], sol.amg.info["rows"]
    mats = reference_for(ceed, oracle, name, sol)
    if not device:
        transfers_check(mats)
    top = 0 if level0 else sol.nlev - 1
    A = mats[top]["A"]
    assert level0 or A.shape[0] == int(sol.free.sum())
    assert A.shape[0] == case.get("free", A.shape[0])
    B_ref, figures = vcycle_reference(sol, mats, top)
    got = measure(sol, A, B_ref, level0)
    cond = float(np.linalg.cond(A))
    ev_ref = np.sort(spectrum_of_product(B_ref, A).real)
    ratios = emax_check(figures, tag)
    out = dict(case=name, n=A.shape[0], error=got["error"], asymmetry=got["asymmetry"], cond=cond, emax_ratio=(min(ratios), max(ratios)),
               spectrum=(float(ev_ref[0]), float(ev_ref[-1])))
    print(f"VCYCLE {tag} case {name} ({A.shape[0]} free dofs, {sol.nlev} levels, {sol.coarse}, {sol.smoother}): |B - B_ref| / max|B_ref| = "
          f"{got['error']:.2e}, |B - B^T| / max|B| = {got['asymmetry']:.2e}, |B_ref - B_ref^T| = {asymmetry(B_ref):.1e}, cond(A) = {cond:.2e}, "
          f"spectrum of B_ref A in [{ev_ref[0]:.4f}, {ev_ref[-1]:.10f}], emax / lambda_max in [{min(ratios):.4f}, {max(ratios):.4f}]")
    if name == "h":
        share = min(float(np.abs(nd.level_reference(sol.p, lv, sol.a0 * sol.density, lv == 0)[1]).max() / np.abs(mats[lv]["A"]).max())
                    for lv in range(sol.nlev)) if not device else None
        if share is not None:
            print(f"VCYCLE {tag} case h: smallest max|a0 rho M| / max|A| over the levels = {share:.2f}")
            assert share >= 0.1, share
    # B against the reference
    assert got["error"] <= tol, (name, got["error"])
    # symmetry and definiteness of the matrix under test
    assert got["asymmetry"] <= TOL_SYM, (name, got["asymmetry"])
    assert got["lmin_sym"] > 0.0, (name, got["lmin_sym"])
    ev = got["ev"]
    assert np.abs(ev.imag).max() <= 1e-9 * np.abs(ev).max() and ev.real.min() > 0.0, (name, ev.real.min(), np.abs(ev.imag).max())
    # quality, on the reference alone
    quality = case.get("quality", "both")
    if quality is not None:
        assert ev_ref[-1] <= LAMBDA_MAX, (name, ev_ref[-1])
    if quality == "both":
        assert ev_ref[0] >= LAMBDA_MIN, (name, ev_ref[0])
    # the outer Krylov iteration
    if pcg and not level0:
        out.update(pcg_check(sol, A, B_ref, tag, name))
    teardown(prob, sol)
    return out


def pcg_check(sol, A, B_ref, tag, name, report_only=False):
    """fcg(b, x, 1e-12) with a seeded random b on the free dofs against the dense PCG with B_ref: iteration counts equal within one
    (a tolerance crossing at round-off), x against the refined A^-1 b."""
    n = sol.p.lsize()
    fr = np.flatnonzero(sol.free)
    b = np.random.default_rng(91).uniform(-1, 1, n) * sol.free
    sol._set(sol.Rtry, b)
    its = sol.fcg(sol.Rtry, sol.dU, 1e-12)
    x = sol.dU.to_numpy()
    x_ref, its_ref = dense_pcg(A, B_ref, b[fr], 1e-12)
    want = nd.solve_refined(A, b[fr])
    err = relmax(x[fr], want)
    if report_only:
        return dict(fcg_its=its, dense_its=its_ref, solution=err)
    print(f"VCYCLE {tag} case {name}: fcg {its} iterations, dense PCG with B_ref {its_ref}; |x - A^-1 b| / max|A^-1 b| = {err:.2e} "
          f"(dense PCG: {relmax(x_ref, want):.2e})")
    assert not x[~sol.free].any()
    assert abs(its - its_ref) <= 1, (name, its, its_ref)
    assert err <= 1e-10, (name, err)
    return dict(fcg_its=its, dense_its=its_ref, solution=err)


def one_level_check(ceed, oracle, smoother, tag):
    """multigrid="none": precondition is M^-1, the inverted diagonal or the inverted nodal blocks."""
    device = ceed is not oracle
    mk = lambda c: SolidProblem(c, distorted_box(2, 1, 1), 2, "hyperFS", nu=0.3, E=1.0, bc_sides=[1], multigrid="none")
    prob = mk(ceed)
    sol = NewtonPMG(prob, smoother=smoother)
    U = prob.smooth_state(0.1) * sol.free
    sol._set(sol.U, U)
    sol.residual(sol.U, sol.R)
    sol.setup_preconditioner()
    assert sol.nlev == 1
    if device:
        rprob = mk(oracle)
        rsol = NewtonPMG(rprob, smoother=smoother)
        rsol._set(rsol.U, U)
        rsol.residual(rsol.U, rsol.R)
        mats = level_matrices(rsol)
        teardown(rprob, rsol)
    else:
        mats = level_matrices(sol)
    B_ref, _ = vcycle_reference(sol, mats)
    B = columns(sol, range(B_ref.shape[0]))
    err = relmax(B, B_ref)
    print(f"VCYCLE {tag} one level, {smoother}: |B - M^-1| / max|M^-1| = {err:.2e}")
    assert err <= (TOL_DEVICE if device else TOL_ORACLE), err
    assert smoother == "jacobi" or np.abs(B_ref - np.diag(np.diag(B_ref))).max() > 1e-3 * np.abs(B_ref).max()     # the blocks couple
    teardown(prob, sol)
    return err


# ---- the controls: seeded faults the check must MISS (CPU oracle only: pure Python changes to a solver object) ---------------------
def seed_emax(sol):
    sol.emax[1] *= 1.05


def seed_restriction(sol):
    """The restricted residual scaled by 0.98."""
    inner = sol.p.restrict

    def restrict(lv, xf, yc):
        inner(lv, xf, yc)
        yc.axpby(0.98, yc, 0.0)
    sol.p.restrict = restrict


def seed_short_post_smoother(sol):
    """The post-smoother (the sweep from a given iterate) one step short."""
    inner = sol.chebyshev

    def chebyshev(lv, b, x, its, zero_guess, lmin_frac=0.1):
        inner(lv, b, x, its if zero_guess else its - 1, zero_guess, lmin_frac)
    sol.chebyshev = chebyshev


CONTROLS = {"emax[1] *= 1.05": (seed_emax, False), "restricted residual x 0.98": (seed_restriction, False),
            "post-smoother one step short": (seed_short_post_smoother, True)}


def controls_check(oracle, tag="oracle", name="a"):
    """The same comparison on case a with each seeded fault: the error must exceed 1e-4 (eight orders above the oracle's bound), and the
    short post-smoother must also miss the symmetry bound.  The fcg counts beside the clean one show what iteration counts alone see."""
    prob, sol = build(oracle, name)
    mats = level_matrices(sol)
    B_ref, _ = vcycle_reference(sol, mats)                   # from the CLEAN solver: emax as estimated
    A = mats[-1]["A"]
    clean = relmax(columns(sol, range(A.shape[0])), B_ref)
    its_clean = pcg_check(sol, A, B_ref, tag, name, report_only=True)["fcg_its"]
    teardown(prob, sol)
    assert clean <= TOL_ORACLE
    out = {}
    for what, (seed, breaks_symmetry) in CONTROLS.items():
        prob, sol = build(oracle, name)
        seed(sol)
        B = columns(sol, range(A.shape[0]))
        err, asym = relmax(B, B_ref), asymmetry(B)
        its = pcg_check(sol, A, B_ref, tag, name, report_only=True)["fcg_its"]
        print(f"VCYCLE {tag} control on case {name}, {what}: |B - B_ref| / max|B_ref| = {err:.2e} (clean {clean:.1e}), asymmetry {asym:.2e}; "
              f"fcg iterations {its_clean} -> {its}")
        out[what] = (err, asym, its_clean, its)
        assert err > 1e-4, (what, err)                        # missed by eight orders
        assert (asym > TOL_SYM) == breaks_symmetry, (what, asym)
        teardown(prob, sol)
    return out


# ---- 4. if something fails: the factors of the recursion, one by one ------------------------------------------------------------------
def factors_check(ceed, oracle, name, tag):
    """Every level's sweep from zero, residual, restriction and prolongation of the solver under test as dense matrices against their
    reference factors (S1, -A, P^T, P): names the term of the recursion that disagrees when vcycle_check fails.  Returns
    {(level, factor): error}."""
    device = ceed is not oracle
    tol = TOL_DEVICE if device else TOL_ORACLE
    prob, sol = build(ceed, name)
    mats = reference_for(ceed, oracle, name, sol)
    out = {}
    for lv in range(1, sol.nlev):
        m, mc = mats[lv], mats[lv - 1]
        w, wc = sol.w[lv], sol.w[lv - 1]
        n, fr, frc = m["n"], m["free"], mc["free"]
        M = smoother_matrix(sol, m["A"], m["node_of"])
        _, S1, _, _ = smoother_factors(m["A"], M, 0.1 * sol.emax[lv], 1.1 * sol.emax[lv], sol.smooth_its)
        zero = ceed.vector(n).set_value(0.0)
        ops = {
            "sweep": (lambda x, y: sol.chebyshev(lv, x, y, sol.smooth_its, True), n, n, fr, fr, S1),
            "residual": (lambda x, y: sol.level_residual(lv, zero, x, y), n, n, fr, fr, -m["A"]),
            "restrict": (lambda x, y: sol.p.restrict(lv, x, y), n, mc["n"], fr, frc, m["P"].T),
            "prolong_add": (lambda x, y: (y.set_value(0.0), sol.p.prolong_add(lv, x, y)), mc["n"], n, frc, fr, m["P"]),
        }
        for what, (apply, n_in, n_out, cols, rows, want) in ops.items():
            X, Y = ceed.vector(n_in), ceed.vector(n_out).set_value(0.0)
            got = np.zeros((rows.size, cols.size))
            for k, j in enumerate(cols):
                e = np.zeros(n_in); e[j] = 1.0
                X.set_array(e)
                apply(X, Y)
                got[:, k] = Y.to_numpy()[rows]
            X.destroy(); Y.destroy()
            out[(lv, what)] = relmax(got, want)
        zero.destroy()
    print(f"VCYCLE {tag} case {name}, factors: " + "  ".join(f"level {lv} {what} {e:.1e}" for (lv, what), e in out.items()))
    teardown(prob, sol)
    assert all(e <= tol for e in out.values()), out
    return out


# ---- the device's forms ----------------------------------------------------------------------------------------------------------------
def forms_check(gpu, name, tag="device", ncols=32):
    """The V-cycle of case ``name`` in its forms on the device -- fused consumers or two passes (fuse_epilogue), each eager or
    replayed through record_preconditioner -- BITWISE on the same ``ncols`` columns drawn with a fixed seed from the free dofs.  "cg"
    cannot be recorded: its two eager forms.  Case d (level 0 alone, assembled: nothing to fuse): eager against a recording of
    vcycle(0, b, x) itself, which replays the aggregation levels' own cycle.  That the fused form ran its fused entries is asserted by counting the calls of
    apply_chebyshev / apply_residual on the levels' operators and, with the scalar smoother, by the scratch vector t of every such
    level: the fused entries never write t at the shell nodes, an apply of its own writes all of it."""
    case = CASES[name]
    level0 = bool(case.get("level0"))
    prob, sol = build(gpu, name)
    r, z, run0, mask = operator_io(sol, level0)
    nfree = int((~mask).sum())
    cols = np.sort(np.random.default_rng(2024).choice(nfree, size=ncols, replace=False))
    assert sol.fuse_epilogue and not sol.graph and sol._pc_graph is None            # the default form: fused consumers, eager
    fused_levels = [lv for lv in range(sol.nlev) if sol._fused_op(lv) is not None]
    calls = {}
    for lv in range(sol.nlev):
        op = prob.levels[lv].opJacob
        for entry in ("apply_chebyshev", "apply_residual"):
            def counted(*a, _inner=getattr(op, entry), _key=(lv, entry)):
                calls[_key] = calls.get(_key, 0) + 1
                return _inner(*a)
            setattr(op, entry, counted)
    # levels whose scratch t only the smoother and the residual write: not level 0 under a CG coarse solve (its applies write t)
    watch = [lv for lv in fused_levels if sol.smoother == "jacobi" and (lv > 0 or sol.coarse == "chebyshev") and not level0]
    results, graphs = {}, []
    recordable = sol.coarse in ("chebyshev", "assembled", "amg")
    for fuse in ((True,) if level0 else (True, False)):      # (level 0 of case d is assembled: nothing to fuse, eager and replayed only)
        for graph in ((False, True) if recordable else (False,)):
            sol.fuse_epilogue = fuse
            calls.clear()
            for lv in watch:
                sol.w[lv]["t"].set_value(SENTINEL)
            run = None
            if graph and level0:
                g = gpu.capture(run0)
                graphs.append(g)
                run = g.launch
            elif graph:
                sol.graph = True
                sol.record_preconditioner(r, z)
                assert sol._pc_graph is not None
            B = columns(sol, cols, level0, run)
            if graph and not level0:
                sol._drop_pc_graph()
                sol.graph = False
            form = ("fused" if fuse else "two-pass") + "+" + ("replayed" if graph else "eager")
            results[form] = B
            n_fused = sum(calls.values())
            if level0:
                assert n_fused == 0, (form, calls)
            elif fuse and fused_levels:
                assert all(calls.get((lv, "apply_residual"), 0) > 0 for lv in fused_levels if lv > 0), (form, calls)
                if sol.smoother == "jacobi":
                    assert all(calls.get((lv, "apply_chebyshev"), 0) > 0 for lv in fused_levels if lv > 0 or sol.coarse == "chebyshev"), (form, calls)
            else:
                assert n_fused == 0, (form, calls)
            for lv in watch:
                kept = int((sol.w[lv]["t"].to_numpy() == SENTINEL).sum())
                assert (kept > 0) == fuse, (form, lv, kept)
    names = list(results)
    assert np.abs(results[names[0]]).max() > 0
    same = {f: bool(np.array_equal(results[f], results[names[0]])) for f in names[1:]}
    diff = {f: float(np.abs(results[f] - results[names[0]]).max()) for f in names[1:]}
    print(f"VCYCLE {tag} case {name}: {ncols} columns, forms bitwise equal to {names[0]}: {same} (max abs differences {diff}); "
          f"levels with fused consumers {fused_levels}")
    for g in graphs:
        g.destroy()
    teardown(prob, sol)
    assert all(same.values()), diff
    return same
