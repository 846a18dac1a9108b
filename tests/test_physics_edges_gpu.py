"""The fused kernels' physics away from nu = 0.3, small strain and the unit frame: device against oracle on identical inputs.

qfunctions_device.hpp states the shifted finite-strain series twice (log1p_series4_shifted in fs_state, the HyperFSF residual;
log1p_series4_shifted_fast in the plain tangent qf_hyperfs_df, in fs_derived_state and so behind qf_hyperfs_df_ds), and before this
file no state of the GPU suite left the middle branch on anything but one affine box at Q = 3 with uniform strain.  Here the states of
_physics_states.py -- six stretches closely on both sides of both shifts, a ramp that puts all three branches inside every element,
strains of 1e-7 -- meet the three geometry forms (general, swept, affine: the smallest ragged mesh of each), Q = 3, 5, 6, 8 (4, 2, 1, 1
elements a wave; the plain tangent below Q = 6, the derived-state tangent from there, on coarse levels too), qextra, own-quadrature
coarse levels (k_state_at_points, then the plain tangent at Q = 2, 3), the small-strain model at its largest tr e, Poisson ratios
from -0.3 to 0.4999, E from 1e-3 to 2e11, and meshes in millimetres, in kilometres, 100 extents from the origin and turned.

Every case compares residual, stored state, the Jacobian action and the scalar diagonal on every level and the point-block diagonal on
the fine level, at the project's parity bar: 1e-10 relative to the oracle in the 2-norm AND in the max norm (1e-12 for the stored
state), and asserts from kernel_name which path ran.  What a state is for is asserted from the ORACLE before anything is compared
(_physics_states.assert_preconditions; the same assertions run on the CPU in test_physics_edges.py).  No case is held to more than the
parity bar: the long-double yardstick of test_physics_edges.py shows no residual or tangent of the oracle more than 1e-14 from long
double at any of these materials.  With CPS_PHYSICS_EDGES_REPORT=<file> the worst figures are written there."""
import os
import time

import numpy as np
import pytest

from ceedpetscsolid_amd.solid import SolidProblem
from _ceed_env import ceed_with_env
import _physics_longdouble as pl
import _physics_states as ps
from _physics_states import errors

pytestmark = pytest.mark.gpu

TOL = 1e-10          # device against oracle, 2-norm and max norm
TOL_STATE = 1e-12    # the stored state: one 3 x 3 product per point
TOL_FORMS = 1e-13    # two forms of one device kernel (test_gpu_parity.py: derived / plain, swept / general, affine / general)
TOL_SCALE = 1e-12    # one mesh in two units
TOL_QDATA = 1e-13    # q-data against long double, unless the oracle's own error on that mesh is above a quarter of it
STRETCHES = [("stretch", s) for s, _ in ps.STRETCHES]
DEGREES = (2, 4, 5, 7)          # Q = 3, 5, 6, 8; ladders P = 2, 3 | 2, 3, 5 | 2, 3, 5, 6 | 2, 3, 5, 8
MODEL = {"linElas": "LinElas", "hyperSS": "HyperSSdF", "hyperFS": "HyperFSdF"}


# --------------------------------------------------------------------------------------------------------------------------------
# the record of a run
# --------------------------------------------------------------------------------------------------------------------------------
EDIT_RUNS = "two edits of qfunctions_device.hpp on scratch copies"       # the heading of the hand-entered part of the record


class Record:
    def __init__(self):
        self.worst, self.shares, self.qdata, self.frames, self.t0 = {}, {}, {}, {}, time.time()

    def write(self, path):
        """everything measured in this run; the part of an existing file from EDIT_RUNS on (runs against scratch builds, entered by hand) is kept"""
        kept = ""
        if os.path.exists(path):
            with open(path) as f:
                kept = f.read().partition(EDIT_RUNS)
            kept = kept[1] + kept[2]
        with open(path, "w") as f:
            f.write(f"physics edges (tests/test_physics_edges_gpu.py), {time.time() - self.t0:.1f} s from the first test of the file to the last\n")
            f.write("device against the oracle, worst relative error over meshes, materials and levels: 2-norm | max norm (bar 1e-10; stored state 1e-12)\n")
            for (family, Q, kind), (e2, einf) in sorted(self.worst.items()):
                f.write(f"  {family:24s} Q={Q}  {kind:8s} {e2:.2e} | {einf:.2e}\n")
            f.write("branch shares the oracle showed under ramp, least over the elements: left | middle | right (at least 0.10 each; two at Q = 2)\n")
            for (mesh, Q), s in sorted(self.shares.items()):
                f.write(f"  {mesh:28s} Q={Q}  {s[0]:.3f} | {s[1]:.3f} | {s[2]:.3f}\n")
            f.write("q-data against long double, w det J | dXdx: oracle, device (bar max(1e-13, 4 x the oracle's)); and the geometry path the device chose\n")
            for case, (o, d, path_) in sorted(self.qdata.items()):
                f.write(f"  {case:28s} oracle {o[0]:.2e} | {o[1]:.2e}  device {d[0]:.2e} | {d[1]:.2e}  {path_}\n")
            f.write("one mesh in two units, device: residual / scale^2 | Jacobian action / scale against the unit mesh, worst of 2-norm and max norm (bar 1e-12)\n")
            for case, (r, j) in sorted(self.frames.items()):
                f.write(f"  {case:28s} {r:.2e} | {j:.2e}\n")
            from conftest import GOLDEN
            from test_physics_edges import reference_against_long_double
            f.write("the reference's own results (tests/golden/qfunctions_edges.npz) against long double, worst over the 15 materials (CPU; test_physics_edges.py)\n")
            for (name, key, kind), d in sorted(reference_against_long_double(np.load(os.path.join(GOLDEN, "qfunctions_edges.npz"))).items()):
                f.write(f"  {key:28s} {kind:8s} {d:.2e}\n")
            f.write(kept)


RECORD = Record()


@pytest.fixture(scope="module", autouse=True)
def report():
    RECORD.t0 = time.time()
    yield
    path = os.environ.get("CPS_PHYSICS_EDGES_REPORT")
    if path:
        RECORD.write(path)


def hold(family, Q, kind, what, got, want, tol=TOL):
    e2, einf = errors(got, want)
    key = (family, Q, kind if isinstance(kind, str) else "stretch")
    w = RECORD.worst.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], e2), max(w[1], einf)
    print(f"  {family} Q={Q} {ps.state_id(kind)} {what}: {e2:.2e} | {einf:.2e}")
    assert e2 <= tol and einf <= tol, (family, Q, kind, what, e2, einf)


# --------------------------------------------------------------------------------------------------------------------------------
# one case
# --------------------------------------------------------------------------------------------------------------------------------
def problems(ceeds, mesh, degree, physics, nu=0.3, E=2.5, **kw):
    return [SolidProblem(c, mesh, degree, physics, nu=nu, E=E, bc_sides=ps.clamped_side(mesh), **kw) for c in ceeds]


def vec(c, arr):
    return c.vector(arr.size).set_array(arr)


def kernel_of(op):
    """the kernel the device's last launch of `op` ran; the oracle has none to name"""
    return op.kernel_name if op.L.has("CeedXOperatorGetKernelName") else ""


def evaluate(p, u, seed=7):
    """Everything a case compares, of problem `p` at displacement u: residual, stored state of every level that has one of its own,
    and per level Jacobian action on a drawn vector, kernel that ran it, scalar diagonal; the point-block diagonal of the fine level."""
    c, n = p.ceed, p.lsize()
    X, R = vec(c, u), c.vector(n)
    p.form_residual(X, R)
    out = {"residual": R.to_numpy(), "residual kernel": kernel_of(p.opApply), "state": {}, "jacobian": [], "diag": [], "kernel": []}
    if p.gradu is not None:
        out["state"] = {k: p.levels[k].gradu.to_numpy() for k in ps.own_levels(p)}
    for lv in range(len(p.levels)):
        nl = p.lsize(lv)
        x, y, d = vec(c, np.random.default_rng(seed + lv).uniform(-1, 1, nl)), c.vector(nl), c.vector(nl).set_value(7.0)
        p.apply_jacobian(lv, x, y)
        out["kernel"].append(kernel_of(p.levels[lv].opJacob))
        p.get_diag(lv, d)
        out["jacobian"].append(y.to_numpy())
        out["diag"].append(d.to_numpy())
        for v in (x, y, d):
            v.destroy()
    B = c.vector(3 * n).set_value(3.0)
    p.get_pointblock_diag(p.fine, B)
    out["pbdiag"] = B.to_numpy()
    for v in (X, R, B):
        v.destroy()
    return out


def assert_paths(p, got, geometry):
    """which kernels the device ran: the geometry form (None: not prescribed), and the derived-state tangent exactly at Q >= 6"""
    if geometry is not None:
        assert geometry in got["residual kernel"], got["residual kernel"]
    for lv, name in zip(p.levels, got["kernel"]):
        assert f"Q={lv.Q},{MODEL[p.problem]}" in name and f"<P={lv.degree + 1}," in name, name
        assert ("HyperFSdF+derived" in name) == (p.problem == "hyperFS" and lv.Q >= 6), (name, lv.Q)
        if geometry is not None:
            assert geometry in name, name


def compare(want, got, p, kind):
    """`got` (the device's `evaluate`) against `want` (the oracle's) of problem `p`"""
    Q = p.Q
    hold("residual", Q, kind, "", got["residual"], want["residual"])
    for k in want["state"]:
        hold("stored state", p.levels[k].Q, kind, f"level {k}", got["state"][k], want["state"][k], TOL_STATE)
    for k, lv in enumerate(p.levels):
        derived = "+derived" if "+derived" in got["kernel"][k] else ""
        hold(f"jacobian {MODEL[p.problem]}{derived}", lv.Q, kind, f"level {k} P={lv.degree + 1}", got["jacobian"][k], want["jacobian"][k])
        hold(f"diag {MODEL[p.problem]}", lv.Q, kind, f"level {k} P={lv.degree + 1}", got["diag"][k], want["diag"][k])
    hold(f"pbdiag {MODEL[p.problem]}", Q, kind, f"P={p.levels[p.fine].degree + 1}", got["pbdiag"], want["pbdiag"])


def oracle_side(po, kind, meshname):
    """The oracle's evaluation at state `kind`, with what the state is for asserted from it BEFORE anything is compared."""
    u = ps.state(po, kind)
    want = evaluate(po, u)
    if po.problem == "hyperFS":
        for k, (Q, lo, hi, shares, minJ) in ps.assert_preconditions(po, kind).items():
            print(f"  oracle level {k} Q={Q}: det C - 1 in [{lo:.5f}, {hi:.5f}], least shares {np.round(shares, 3)}, min det F {minJ:.3f}")
            if kind == "ramp":
                old = RECORD.shares.get((meshname, Q), shares)
                RECORD.shares[(meshname, Q)] = np.minimum(old, shares)
    elif po.problem == "hyperSS":
        g = po.gradu.to_numpy().reshape(po.mesh.nelem, 9, -1)
        tr = g[:, 0] + g[:, 4] + g[:, 8]
        print(f"  oracle: 1 + tr e in [{1 + tr.min():.4f}, {1 + tr.max():.4f}]")
        assert 1 + tr.min() > 0.2                                 # the denominator of lambda_bar (hyperSS.h:294-295) stays positive
        if kind == ("stretch", -0.25):
            assert 1 + tr.max() < 0.3
        if kind == ("stretch", 0.3):
            assert 1 + tr.min() > 1.85
    return u, want


def run_case(oracle, gpu, meshname, degree, physics, kind, geometry="default", mesh=None, **kw):
    mesh = ps.MESHES[meshname]() if mesh is None else mesh
    po, pg = problems((oracle, gpu), mesh, degree, physics, **kw)
    u, want = oracle_side(po, kind, meshname)
    got = evaluate(pg, u)
    assert_paths(pg, got, ps.GEOMETRY_PATH[meshname] if geometry == "default" else geometry)
    compare(want, got, pg, kind)
    po.destroy(); pg.destroy()
    return want, got


# --------------------------------------------------------------------------------------------------------------------------------
# the branches of the finite-strain series, in every kernel that states it
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", STRETCHES + ["ramp"], ids=ps.state_id)
@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("meshname", list(ps.MESHES))
def test_finite_strain_branches(oracle, gpu, meshname, degree, kind):
    run_case(oracle, gpu, meshname, degree, "hyperFS", kind)


@pytest.mark.parametrize("meshname", list(ps.MESHES))
def test_finite_strain_branches_with_qextra(oracle, gpu, meshname):
    """P = 5 at Q = 6: the derived state on a fine level with P < Q"""
    run_case(oracle, gpu, meshname, 4, "hyperFS", "ramp", qextra=1)


@pytest.mark.parametrize("meshname", list(ps.MESHES))
def test_finite_strain_branches_on_own_quadrature_levels(oracle, gpu, meshname):
    """k_state_at_points writes the coarse levels' state at Q = 2, 3; the plain tangent reads it"""
    mesh = ps.MESHES[meshname]()
    po, pg = problems((oracle, gpu), mesh, 4, "hyperFS", coarse_quadrature="own")
    u, want = oracle_side(po, "ramp", meshname)
    got = evaluate(pg, u)
    assert [lv.Q for lv in pg.levels] == [2, 3, 5] and sorted(want["state"]) == [0, 1, 2]
    assert [lv.opState.kernel_name for lv in pg.levels[:-1]] == ["state<Pf=5,Qc=2>", "state<Pf=5,Qc=3>"]
    assert_paths(pg, got, ps.GEOMETRY_PATH[meshname])
    compare(want, got, pg, "ramp")
    po.destroy(); pg.destroy()


@pytest.mark.parametrize("kind", [("stretch", -0.25), ("stretch", 0.3), "ramp"], ids=ps.state_id)
@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("meshname", list(ps.MESHES))
def test_small_strain_model_at_its_largest_trace(oracle, gpu, meshname, degree, kind):
    """tr e = 3 s enters the series of the residual and the denominator of lambda_bar in the tangent: 1 + tr e from 0.25 to 1.9"""
    run_case(oracle, gpu, meshname, degree, "hyperSS", kind)


# --------------------------------------------------------------------------------------------------------------------------------
# two forms of one kernel agree where the series shifts
# --------------------------------------------------------------------------------------------------------------------------------
def forms_agree(gpu, other, mesh, degree, physics, kind, tell):
    pa, pb = problems((gpu, other), mesh, degree, physics)
    u = ps.state(pa, kind)
    a, b = evaluate(pa, u), evaluate(pb, u)
    tell(a["kernel"], b["kernel"])
    pairs = [("residual", a["residual"], b["residual"])] + [(f"state {k}", a["state"][k], b["state"][k]) for k in a["state"]]
    pairs += [(f"jacobian {k}", x, y) for k, (x, y) in enumerate(zip(a["jacobian"], b["jacobian"]))]
    pairs += [(f"diag {k}", x, y) for k, (x, y) in enumerate(zip(a["diag"], b["diag"]))] + [("pbdiag", a["pbdiag"], b["pbdiag"])]
    for what, x, y in pairs:
        e2, einf = errors(x, y)
        print(f"  {what}: {e2:.2e} | {einf:.2e}")
        assert e2 <= TOL_FORMS and einf <= TOL_FORMS, (what, e2, einf)
    pa.destroy(); pb.destroy()


def test_derived_and_plain_tangent_agree_across_the_branches(gpu, product_lib):
    def tell(default, plain):
        assert all("+derived" in k for k in default) and not any("derived" in k for k in plain)
    forms_agree(gpu, ceed_with_env(product_lib, {"CEED_MI355X_DERIVED": "0"}), ps.general_mesh(), 5, "hyperFS", "ramp", tell)


@pytest.mark.parametrize("physics", ["linElas", "hyperSS", "hyperFS"])
@pytest.mark.parametrize("degree", [2, 5])
@pytest.mark.parametrize("meshname,switch", [("swept", "CEED_MI355X_SWEPT"), ("affine", "CEED_MI355X_AFFINE")])
def test_special_and_general_geometry_agree_across_the_branches(gpu, product_lib, meshname, switch, degree, physics):
    def tell(default, general):
        assert all(ps.GEOMETRY_PATH[meshname] in k for k in default), default
        assert all("[dXdx recomputed per point]" in k for k in general), general
    forms_agree(gpu, ceed_with_env(product_lib, {switch: "0"}), ps.MESHES[meshname](), degree, physics, "ramp", tell)


# --------------------------------------------------------------------------------------------------------------------------------
# the material
# --------------------------------------------------------------------------------------------------------------------------------
MATERIALS = [(nu, 2.5, kind) for nu in (-0.3, 0.0, 0.49, 0.4999) for kind in ("ramp", "tiny")] + [(0.3, E, "ramp") for E in (1e-3, 2e11)]


@pytest.mark.parametrize("nu,E,kind", MATERIALS, ids=[f"nu={nu}-E={E:g}-{kind}" for nu, E, kind in MATERIALS])
@pytest.mark.parametrize("physics", ["linElas", "hyperSS", "hyperFS"])
@pytest.mark.parametrize("degree", [4, 5])
def test_material_range(oracle, gpu, degree, physics, nu, E, kind):
    """lambda / mu from -0.375 to 5e3, E over 14 decades: the plain tangent (Q = 5) and the derived state (Q = 6, whose tenth entry
    lambda ln J - mu cancels at strains of 1e-7) on the general mesh"""
    run_case(oracle, gpu, "general", degree, physics, kind, nu=nu, E=E)


# --------------------------------------------------------------------------------------------------------------------------------
# the mesh frame: millimetres, kilometres, far from the origin, turned
# --------------------------------------------------------------------------------------------------------------------------------
def rotated_x(coords, degrees=30.0):
    a = np.deg2rad(degrees)
    return coords @ np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]).T


FRAMES = {"x1e-3": lambda X: 1e-3 * X, "x1e3": lambda X: 1e3 * X,
          "moved": lambda X: X + 100 * (X.max(axis=0) - X.min(axis=0)) * np.array([1.0, -1.0, 1.0]), "turned": rotated_x}
FRAME_CASES = [(m, f) for m in ps.MESHES for f in ("x1e-3", "x1e3", "moved")] + [("swept", "turned")]


def qdata_errors(p, ld):
    qd = p.qdata.to_numpy().reshape(p.mesh.nelem, 10, -1)
    return pl.distance(qd[:, 0], ld[:, 0]), pl.distance(qd[:, 1:], ld[:, 1:])


@pytest.mark.parametrize("degree", [2, 5])
@pytest.mark.parametrize("meshname,frame", FRAME_CASES, ids=[f"{m}-{f}" for m, f in FRAME_CASES])
def test_mesh_frame(oracle, gpu, meshname, frame, degree):
    """The relative classification thresholds of k_geo_affine / k_geo_swept and the rcp_nr of det J on coordinates of 1e-3, 1e3 and
    100 +- 1: q-data against SetupGeo in long double (trilinear map, adjugate, one division), the operators against the oracle, and
    the scaled meshes against the unit one -- the residual of the scaled displacement is scale^2 x, the Jacobian action on one vector
    scale x the unit mesh's.  Which geometry form the device chose is recorded, not prescribed: the translated box is affine to
    1e-14 only."""
    mesh = ps.MESHES[meshname]()
    unit_coords = mesh.coords.copy()
    mesh.coords = FRAMES[frame](mesh.coords)
    po, pg = problems((oracle, gpu), mesh, degree, "hyperFS")
    b = po.basisx
    ld = pl.mesh_qdata(mesh.coords, mesh.cells, b.interp1d, b.grad1d, b.qweight1d)
    eo, eg = qdata_errors(po, ld), qdata_errors(pg, ld)
    u, want = oracle_side(po, "ramp", f"{meshname} {frame}")
    got = evaluate(pg, u)
    path = got["kernel"][-1].partition(" ")[2]                     # "[affine elements: ...]", "[dXdx recomputed per point]", ...
    RECORD.qdata[f"{meshname} {frame} Q={pg.Q}"] = (eo, eg, path)
    print(f"  q-data against long double, w det J | dXdx: oracle {eo[0]:.2e} | {eo[1]:.2e}, device {eg[0]:.2e} | {eg[1]:.2e}; device path {path}")
    for o, g in zip(eo, eg):
        assert g <= max(TOL_QDATA, 4 * o), (eo, eg)
    assert_paths(pg, got, None)
    compare(want, got, pg, "ramp")
    po.destroy(); pg.destroy()
    if frame in ("x1e-3", "x1e3"):
        scale = float(frame[1:])
        mesh.coords = unit_coords
        (pu,) = problems((gpu,), mesh, degree, "hyperFS")
        unit = evaluate(pu, ps.state(pu, "ramp"))
        r = max(errors(got["residual"] / scale ** 2, unit["residual"]))
        j = max(max(errors(a / scale, b)) for a, b in zip(got["jacobian"], unit["jacobian"]))
        RECORD.frames[f"{meshname} {frame} Q={pg.Q}"] = (r, j)
        print(f"  against the unit mesh: residual / scale^2 {r:.2e}, Jacobian action / scale {j:.2e}")
        assert r <= TOL_SCALE and j <= TOL_SCALE, (r, j)
        pu.destroy()
