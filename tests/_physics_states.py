"""States that take the finite-strain log series through all three of its branches, and the smallest meshes that are ragged for the
fused kernels' elements-per-wave packing -- shared by test_coord_energy_gpu.py, test_physics_edges.py (CPU: the preconditions, from the
oracle) and test_physics_edges_gpu.py (the device at those states).  No tests here.

The series of hyperFS.h:45-67 shifts its argument det C - 1 below LEFT = sqrt(2)/2 - 1 and above RIGHT = sqrt(2) - 1.  No amplitude of
smooth_displacement gets there (it nearly preserves volume), so the states here are built on u = s X:
  stretch(s)  u = s X + smooth_state(0.002): det C - 1 = (1 + s)^6 - 1 to rounding of the small part, all points on ONE side, closely
              for s = -0.06 | -0.05 (LEFT between) and 0.059 | 0.06 (RIGHT between);
  ramp        u = (-0.14 + 0.28 t)(X - X_min), t the normalised global z: all three branches inside every element, so the lanes of one
              wave diverge;
  tiny        smooth_state(1e-7): strains at rounding level.
`assert_preconditions` reads from the ORACLE's stored state that a state does what it is for, before anything is compared."""
import numpy as np

from ceedpetscsolid_amd.mesh import box_mesh, hollow_cylinder_mesh
from _numbering import distorted_box

LEFT, RIGHT = np.sqrt(2.0) / 2 - 1, np.sqrt(2.0) - 1      # the range shifts of log1p_series_shifted (hyperFS.h:45-67), in det C - 1
SHEAR = np.array([[1.0, 0.3, -0.2], [0.1, 0.7, 0.25], [-0.15, 0.2, 1.4]])     # of test_affine_elements_take_the_per_element_factors
SHEAR_OFFSET = np.array([0.3, -0.1, 0.2])
STRETCHES = [(-0.25, "left"), (-0.06, "left"), (-0.05, "middle"), (0.059, "middle"), (0.06, "right"), (0.3, "right")]
MIN_SHARE = 0.10          # ramp: at least this part of every element's points in each branch
MIN_J_RAMP = 0.6          # det F under ramp stays above this (0.86^3 = 0.636 at the clamped end)
MIN_J = 0.4               # and under every state above this (0.75^3 = 0.422 under stretch(-0.25))


def errors(got, want):
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    n2, ninf = np.linalg.norm(want), np.abs(want).max()
    assert n2 > 0
    return np.linalg.norm(got - want) / n2, np.abs(got - want).max() / ninf


def det_c_minus_1(p, u):
    """det C - 1 at every quadrature point of problem `p` (the oracle's) under displacement u, in numpy from the oracle's q-data and
    basis tables: grad u = sum_m du/dxi_m dXdx[m][.], C = F^T F."""
    lv = p.levels[-1]
    B, G = lv.basisu.interp1d, lv.basisu.grad1d                       # [Q][P]
    Pn, ne = lv.degree + 1, p.mesh.nelem
    U = u.reshape(-1, 3)[lv.dofmap.elem_nodes].reshape(ne, Pn, Pn, Pn, 3)      # [e][z][y][x][component]
    dU = np.stack([np.einsum("kc,jb,ia,ecbav->ekjiv", *tabs, U) for tabs in ((B, B, G), (B, G, B), (G, B, B))], axis=-1)   # [..][v][m]
    dXdx = p.qdata.to_numpy().reshape(ne, 10, -1)[:, 1:, :].reshape(ne, 3, 3, -1)          # [e][m][k][q]
    g = np.einsum("eqvm,emkq->eqvk", dU.reshape(ne, -1, 3, 3), dXdx)
    return np.linalg.det(np.eye(3) + g) ** 2 - 1


# --------------------------------------------------------------------------------------------------------------------------------
# meshes: 3 (4) elements -- a last wave (Q = 3: 4 elements a wave, Q = 5: 2) that is partly empty
# --------------------------------------------------------------------------------------------------------------------------------
def general_mesh():
    return distorted_box(3, 1, 1, seed=3, amp=0.2)


def swept_mesh():
    return hollow_cylinder_mesh(1, 4, 1)


def affine_mesh():
    m = box_mesh(3, 1, 1)
    m.coords = m.coords @ SHEAR.T + SHEAR_OFFSET
    return m


MESHES = {"general": general_mesh, "swept": swept_mesh, "affine": affine_mesh}
GEOMETRY_PATH = {"general": "recomputed", "swept": "swept elements", "affine": "affine elements"}     # in the device's kernel_name


def clamped_side(mesh):
    return [1] if 1 in mesh.side_sets else [998]


# --------------------------------------------------------------------------------------------------------------------------------
# states, as functions of the problem (its fine-level node coordinates)
# --------------------------------------------------------------------------------------------------------------------------------
def stretch(p, s):
    return s * p.levels[p.fine].dofmap.node_coords.reshape(-1) + p.smooth_state(0.002)


def ramp(p):
    X = p.levels[p.fine].dofmap.node_coords
    lo = X.min(axis=0)
    t = (X[:, 2] - lo[2]) / (X[:, 2].max() - lo[2])
    return ((-0.14 + 0.28 * t)[:, None] * (X - lo)).reshape(-1)


def tiny(p):
    return p.smooth_state(1e-7)


def state(p, kind):
    """kind: "ramp", "tiny" or ("stretch", s)"""
    if kind == "ramp":
        return ramp(p)
    if kind == "tiny":
        return tiny(p)
    assert kind[0] == "stretch"
    return stretch(p, kind[1])


def state_id(kind):
    return kind if isinstance(kind, str) else f"s={kind[1]}"


# --------------------------------------------------------------------------------------------------------------------------------
# what the oracle saw
# --------------------------------------------------------------------------------------------------------------------------------
def stored_det_f(lv, nelem):
    """det F at every point of level `lv`, [element][point], from the state the oracle's residual stored there."""
    g = lv.gradu.to_numpy().reshape(nelem, 3, 3, -1).transpose(0, 3, 1, 2)
    return np.linalg.det(np.eye(3) + g)


def own_levels(p):
    """the levels of `p` that carry a quadrature of their own: the fine one, and under coarse_quadrature="own" every other"""
    return [k for k, lv in enumerate(p.levels) if k == p.fine or lv.own_quadrature]


def branch_shares(x):
    """x: det C - 1, [element][point] -> the part of each element's points in the left, middle and right branch, [element][3]"""
    return np.stack([(x < LEFT).mean(axis=1), ((x >= LEFT) & (x <= RIGHT)).mean(axis=1), (x > RIGHT).mean(axis=1)], axis=1)


def on_its_side(x, branch):
    return np.all(x < LEFT) if branch == "left" else (np.all(x > RIGHT) if branch == "right" else np.all((x >= LEFT) & (x <= RIGHT)))


def assert_preconditions(p, kind):
    """`p`: the ORACLE's hyperFS problem after form_residual at state `kind`.  Asserts, at the points of every level that carries a
    quadrature of its own, what the state is for; returns {level: (Q, min det C - 1, max det C - 1, min share [3], min J)}."""
    assert p.problem == "hyperFS"
    seen = {}
    for k in own_levels(p):
        lv = p.levels[k]
        J = stored_det_f(lv, p.mesh.nelem)
        x = J * J - 1
        shares = branch_shares(x).min(axis=0)
        seen[k] = (lv.Q, x.min(), x.max(), shares, J.min())
        assert J.min() > (MIN_J_RAMP if kind == "ramp" else MIN_J), (kind, k, J.min())
        if kind == "ramp":
            # Q = 2 (an own-quadrature coarse level): two Gauss points along z reach two branches only
            assert (shares >= MIN_SHARE).sum() >= (3 if lv.Q >= 3 else 2), (kind, k, lv.Q, shares)
        elif kind == "tiny":
            assert np.abs(x).max() < 1e-6, (kind, k, np.abs(x).max())
        else:
            branch = dict(STRETCHES)[kind[1]]
            assert on_its_side(x, branch), (kind, k, branch, x.min(), x.max())
    return seen
