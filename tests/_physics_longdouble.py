"""The pointwise physics once more in numpy `longdouble` (64-bit mantissa on x86: eps 1.1e-19), as a yardstick for what double
rounding alone does to a result: the formulas of qfunctions/common.h, linElas.h, hyperSS.h and hyperFS.h as oracle/oracle_qfunctions.c
restates them -- the 4-term series with its range shifts, NOT libm's log1p -- on the same double inputs.  Where the reference's own
double result is d away from this evaluation, no restatement in another operation order can be asked to come closer to the reference
than a small multiple of d.  No tests here; test_physics_edges.py and test_physics_edges_gpu.py use it.

Array conventions are those of the QFunctions: ug[(d*3 + c)][i] = d u_c / d xi_d; qdata[0][i] = w det J, qdata[1 + 3r + s][i] = dXdx[r][s];
stored state[(3c + k)][i] = d u_c / d x_k; output dv[(k*3 + c)][i]."""
import numpy as np

LD = np.longdouble
EXTENDED = np.finfo(LD).eps < 1e-18           # false where longdouble is double: the yardstick is then no finer than what it measures
_I = np.eye(3, dtype=LD)
_LEFT, _RIGHT = np.sqrt(2.0) / 2 - 1, np.sqrt(2.0) - 1          # the branch is chosen as the double code chooses it


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def _mm(a, b):
    return np.einsum("qij,qjk->qik", a, b)


def _t(a):
    return a.transpose(0, 2, 1)


def _tr(a):
    return a[:, 0, 0] + a[:, 1, 1] + a[:, 2, 2]


def _adj(M):
    """adjugate of [q][3][3]: M adj(M) = det(M) I"""
    A = np.empty_like(M)
    for r in range(3):
        for s in range(3):
            r1, r2, s1, s2 = (r + 1) % 3, (r + 2) % 3, (s + 1) % 3, (s + 2) % 3
            A[:, r, s] = M[:, s1, r1] * M[:, s2, r2] - M[:, s1, r2] * M[:, s2, r1]
    return A


def _det(M, A):
    return M[:, 0, 0] * A[:, 0, 0] + M[:, 0, 1] * A[:, 1, 0] + M[:, 0, 2] * A[:, 2, 0]


def _load(ug, qd):
    ug, qd = _ld(ug), _ld(qd)
    Q = ug.shape[1]
    du = ug.T.reshape(Q, 3, 3).transpose(0, 2, 1)              # [q][c][d]
    dX = qd[1:].T.reshape(Q, 3, 3)                             # [q][r][s]
    return du, dX, qd[0], _mm(du, dX)                          # g[c][k] = sum_m du[c][m] dXdx[m][k]


def _pull_back(T, dX, wdetJ):
    dv = np.einsum("qkm,qcm->qkc", dX, T) * wdetJ[:, None, None]
    return dv.reshape(len(wdetJ), 9).T


def _state(g):
    return g.reshape(len(g), 9).T


def lame(nu, E):
    nu, E = LD(nu), LD(E)
    two_mu = E / (1 + nu)
    return (3 * (E / (3 * (1 - 2 * nu))) - two_mu) / 3, two_mu


def series4(x):
    y = x / (2 + x)
    y2 = y * y
    return 2 * (y + y * y2 / 3 + y * y2 * y2 / 5 + y * y2 * y2 * y2 / 7)


def series4_shifted(x):
    lo, hi = x < _LEFT, x > _RIGHT
    ln2h = np.log(LD(2)) / 2
    return np.where(lo, -2 * ln2h, np.where(hi, 2 * ln2h, LD(0))) + series4(np.where(lo, 1 + 2 * x, np.where(hi, (x - 1) / 2, x)))


def setup_geo_ld(Jg, w):
    """common.h:47-101 on longdouble inputs, no rounding to double on the way in.  Jg[(d*3 + c)][i] = d x_c / d xi_d"""
    Q = Jg.shape[1]
    J = Jg.T.reshape(Q, 3, 3).transpose(0, 2, 1)               # J[r][s] = d x_r / d xi_s
    A = _adj(J)
    det = _det(J, A)
    return np.concatenate([(w * det)[None], (A / det[:, None, None]).reshape(Q, 9).T])


def setup_geo(Jg, w):
    """setup_geo_ld of double inputs"""
    return setup_geo_ld(_ld(Jg), _ld(w).reshape(-1))


def _hooke(nu, E, e):
    nu, E = LD(nu), LD(E)
    ss = E / ((1 + nu) * (1 - 2 * nu))
    sig = ss * (1 - 2 * nu) * e / 2
    tr = _tr(e)
    for a in range(3):
        sig[:, a, a] = ss * ((1 - 2 * nu) * e[:, a, a] + nu * tr)
    return sig


def linelas(nu, E, ug, qd):
    du, dX, w, g = _load(ug, qd)
    return _pull_back(_hooke(nu, E, (g + _t(g)) / 2), dX, w)


def hyperss_f(nu, E, ug, qd):
    lam, two_mu = lame(nu, E)
    du, dX, w, g = _load(ug, qd)
    e = (g + _t(g)) / 2
    sig = two_mu * e + (lam * series4(_tr(e)))[:, None, None] * _I
    return _pull_back(sig, dX, w), _state(g)


def hyperss_df(nu, E, dug, qd, state):
    lam, two_mu = lame(nu, E)
    du, dX, w, dg = _load(dug, qd)
    st = _ld(state)
    de = (dg + _t(dg)) / 2
    ltr = lam / (1 + (st[0] + st[4] + st[8])) * _tr(de)
    return _pull_back(two_mu * de + ltr[:, None, None] * _I, dX, w)


def _fs_state(lam, mu, g):
    E2 = g + _t(g) + _mm(_t(g), g)
    a, b, c, d, e, f = E2[:, 0, 0], E2[:, 1, 1], E2[:, 2, 2], E2[:, 1, 2], E2[:, 0, 2], E2[:, 0, 1]
    det_c_m1 = (a * (b * c - d * d) + f * (e * d - f * c) + e * (f * d - e * b) + a + b + c + a * b + a * c + b * c
                - f * f - e * e - d * d)                       # hyperFS.h:72-80
    C = E2 + _I
    Cinv = _adj(C) / (det_c_m1 + 1)[:, None, None]
    llnj = lam * series4_shifted(det_c_m1) / 2
    S = llnj[:, None, None] * Cinv + mu * _mm(Cinv, E2)
    return E2, det_c_m1, Cinv, llnj, S


def hyperfs_f(nu, E, ug, qd):
    lam, two_mu = lame(nu, E)
    du, dX, w, g = _load(ug, qd)
    S = _fs_state(lam, two_mu / 2, g)[4]
    return _pull_back(_mm(g + _I, S), dX, w), _state(g)


def hyperfs_df(nu, E, dug, qd, state):
    lam, two_mu = lame(nu, E)
    mu = two_mu / 2
    du, dX, w, dg = _load(dug, qd)
    g = _ld(state).T.reshape(-1, 3, 3)
    F = g + _I
    _, _, Cinv, llnj, S = _fs_state(lam, mu, g)
    dE = (_mm(_t(dg), F) + _mm(_t(F), dg)) / 2
    cinv_de = np.einsum("qab,qab->q", Cinv, dE)
    dS = (lam * cinv_de)[:, None, None] * Cinv - (2 * (llnj - mu))[:, None, None] * _mm(Cinv, _mm(dE, Cinv))
    return _pull_back(_mm(dg, S) + _mm(F, dS), dX, w)


def energy(model, nu, E, ug, qd):
    """energy density x w det J: linElas.h:285-370, hyperSS.h:326-412, hyperFS.h:469-553, as written"""
    lam, two_mu = lame(nu, E)
    mu = two_mu / 2
    du, dX, w, g = _load(ug, qd)
    if model == "HyperFS":
        E2, det_c_m1 = _fs_state(lam, mu, g)[:2]
        logj = series4_shifted(det_c_m1) / 2
        en = lam * logj * logj / 2 - mu * logj + mu * _tr(E2) / 2
    else:
        e = (g + _t(g)) / 2
        sv = _tr(e)
        shear = (e[:, 0, 1] ** 2 + e[:, 0, 2] ** 2 + e[:, 1, 2] ** 2) * 2 * mu
        en = lam * sv * sv / 2 + sv * mu + shear if model == "LinElas" else lam * (1 + sv) * (series4(sv) - 1) + sv * mu + shear
    return (en * w)[None]


def evaluate(name, nu, E, ins):
    """QFunction `name` on the inputs `ins` (in the QFunction's order) -> list of its outputs, longdouble"""
    if name in ("LinElasF", "LinElasdF"):
        return [linelas(nu, E, *ins)]
    if name.endswith("Energy"):
        return [energy(name[:-6], nu, E, *ins)]
    f = {"HyperSSF": hyperss_f, "HyperSSdF": hyperss_df, "HyperFSF": hyperfs_f, "HyperFSdF": hyperfs_df}[name]
    out = f(nu, E, *ins)
    return list(out) if isinstance(out, tuple) else [out]


def distance(a, want):
    """|a - want| / |want| in the 2-norm, formed in longdouble"""
    a, want = np.asarray(a, dtype=LD), np.asarray(want, dtype=LD)
    return float(np.sqrt(((a - want) ** 2).sum()) / np.sqrt((want ** 2).sum()))


def mesh_qdata(coords, cells, interp1d, grad1d, qweight1d):
    """SetupGeo on a mesh of trilinear hexes, [element][10][Q^3] (point i + Q (j + Q k), vertex a + 2 b + 4 c): the Jacobian of the
    trilinear map from the 1-D tables of the (2, Q) coordinate basis, its adjugate and a division, all in longdouble."""
    B, G, w = _ld(interp1d), _ld(grad1d), _ld(qweight1d)
    Q = B.shape[0]
    X = _ld(coords)[np.asarray(cells)].reshape(-1, 2, 2, 2, 3)                 # [e][c][b][a][component]
    Jg = np.stack([np.einsum("kc,jb,ia,ecbav->ekjiv", *tabs, X) for tabs in ((B, B, G), (B, G, B), (G, B, B))], axis=1)  # [e][d][k][j][i][v]
    ne = X.shape[0]
    Jg = Jg.reshape(ne, 3, Q ** 3, 3).transpose(0, 1, 3, 2).reshape(ne, 9, Q ** 3)                        # [(d*3 + v)][point]
    w3 = np.einsum("k,j,i->kji", w, w, w).reshape(-1)
    return np.stack([setup_geo_ld(Jg[e], w3) for e in range(ne)])

