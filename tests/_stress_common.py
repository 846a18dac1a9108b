"""What the CPU and the device tests of stress recovery (postprocess.Stress) share: the closed forms of the three stress laws in
longdouble from tests/_physics_longdouble.py (the reference's series, never numpy.log), displacement fields, and the virtual work of a
point stress formed in NumPy.  No tests here."""
import numpy as np

import _physics_longdouble as pl
from ceedpetscsolid_amd.postprocess import VOIGT

MODELS = ("linElas", "hyperSS", "hyperFS")
# a fixed full 3 x 3 gradient: entries <= 0.05 for the small-strain models, up to 0.3 with det F > 0 for the finite-strain one
G_SMALL = np.array([[0.031, -0.017, 0.044], [0.05, -0.023, 0.012], [-0.038, 0.027, 0.019]])
G_FINITE = np.array([[0.21, -0.13, 0.3], [0.08, -0.17, 0.11], [-0.25, 0.19, 0.14]])
assert np.abs(G_SMALL).max() <= 0.05 and np.abs(G_FINITE).max() <= 0.3 and np.linalg.det(np.eye(3) + G_FINITE) > 0.5


def gradient_of(problem):
    return G_FINITE if problem == "hyperFS" else G_SMALL


def closed_form(problem, nu, E, G):
    """The six stress components (xx, yy, zz, yz, xz, xy) at the constant gradient G[c][k] = d u_c / d x_k, in longdouble."""
    g = np.asarray(G, dtype=np.float64).astype(pl.LD)[None]
    e = (g + pl._t(g)) / 2
    if problem == "linElas":
        sig = pl._hooke(nu, E, e)
    elif problem == "hyperSS":
        lam, two_mu = pl.lame(nu, E)
        sig = two_mu * e + (lam * pl.series4(pl._tr(e)))[:, None, None] * pl._I
    else:
        lam, two_mu = pl.lame(nu, E)
        S = pl._fs_state(lam, two_mu / 2, g)[4]
        F = g + pl._I
        sig = pl._mm(F, pl._mm(S, pl._t(F))) / pl._det(F, pl._adj(F))[:, None, None]
    return np.array([sig[0, i, j] for i, j in VOIGT], dtype=pl.LD)


def linear_field(X, G):
    """u = G X at the node coordinates X, an L-vector: grad_X u = G exactly, and u lies in every Lagrange space of a trilinear mesh"""
    return (np.asarray(X) @ np.asarray(G).T).reshape(-1)


def smooth_field(X, amp):
    """A smooth non-homogeneous displacement of amplitude `amp` at the node coordinates X, an L-vector."""
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    u = np.stack([np.sin(1.3 * x + 0.7 * y) * np.cos(0.4 * z), np.cos(0.9 * y - 0.5 * z) + 0.3 * x * y, np.sin(0.6 * z + 1.1 * x) - 0.2 * y * y], axis=1)
    return (amp * u).reshape(-1)


def full_tensor(s6):
    """[..., 6] -> [..., 3, 3]"""
    s = np.empty(s6.shape[:-1] + (3, 3))
    for m, (i, j) in enumerate(VOIGT):
        s[..., i, j] = s[..., j, i] = s6[..., m]
    return s


def virtual_work(st, x, points):
    """sum_e sum_q w det J P : grad_X N_a as an L-vector, from the point stress `points` ([nelem][6][Q^3], what Stress.points returned
    for the host array x): P = sigma for the small-strain models, the first Piola-Kirchhoff stress J sigma F^-T for hyperFS.  The
    tables, w det J and dXdx are those of the Stress object's portable form; the sum over the elements is in element order."""
    B, G, W, dX = st._tables()
    ne, P, Q = st.ne, st.P, st.Q
    sig = full_tensor(np.moveaxis(np.asarray(points).reshape(ne, 6, Q, Q, Q), 1, -1))       # [e][k][j][i][3][3]
    if st.problem == "hyperFS":
        F = st.grad_host(x) + np.eye(3)
        sig = np.linalg.det(F)[..., None, None] * (sig @ np.swapaxes(np.linalg.inv(F), -1, -2))
    dv = np.einsum("edba,emndba,edbacn->emdbac", W, dX, sig)                                # w sum_n dXdx[m][n] P[c][n]
    re = sum(np.einsum("ai,bj,dk,edbac->ekjic", *t, dv[:, m]) for m, t in enumerate(((G, B, B), (B, G, B), (B, B, G))))
    out = np.zeros((st.nnodes, 3))
    np.add.at(out, (st.offsets // 3).reshape(-1), re.reshape(-1, 3))
    return out.reshape(-1)
