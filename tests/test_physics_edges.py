"""The oracle's restated physics pinned to the REFERENCE away from the one point of tests/golden/qfunctions.npz ({nu, E} = {0.3, 2.5},
strains of 0.02), and the preconditions of test_physics_edges_gpu.py checked where a bad input costs nothing.

tests/golden/qfunctions_edges.npz (oracle/gen_golden.py, the reference's own callbacks): nu in {-0.3, 0, 0.3, 0.49, 0.4999} x E in
{1e-3, 2.5, 2e11} on 15 shared points with full 3 x 3 dXdx, whose physical gradients are s I + 0.01 random for six s that put
det C - 1 closely on both sides of both range shifts of the finite-strain series (tr e = 3 s for the small-strain model), random at
0.3 and random at 1e-7.  The oracle is compared KIND BY KIND of point, not over all 15 at once: in one 2-norm the points at 1e-7
(outputs 1e-7 of the others') would not count.  Bar 1e-13, that of test_oracle_qfunctions.py, everywhere -- no group needed more:
with its pointwise physics built without fused multiply-adds the oracle reproduces the reference bit for bit at every one of these
points (measured 0.0 for all 15 x 9 x 8); with them, lambda = (3 K - 2 mu) / 3 at nu = 0 was the rounding error of 3 K, 1e-17 E,
where the reference has 0, and HyperSSEnergy -- which carries lambda itself as a term -- sat 3.9e-10 from the reference at strains of
1e-7, the reference 5e-17 from long double.

The long-double yardstick (_physics_longdouble.py), worst over the 15 materials, reference = oracle against long double:
  every residual, tangent and stored state, every kind      <= 1.0e-14   (HyperSSF at s = -0.25; all others <= 1.7e-15)
  LinElasEnergy, HyperSSEnergy                              <= 4.1e-15
  HyperFSEnergy at strains of 1e-7                             4.0e-09   (nu = -0.3; 3e-13 at nu = 0.4999)
The last is conditioning, not a defect: lambda ln^2 J / 2 - mu ln J + mu tr E is second order in the strain, its terms first order.
No operator of test_physics_edges_gpu.py reads an energy, and no residual or tangent is more than 1e-11 from long double: none of
its cases is held to more than the parity bar."""
import os
import sys

import numpy as np
import pytest

from ceedpetscsolid_amd.solid import SolidProblem
from conftest import REF_QF_LIB, ROOT, GOLDEN, _ensure_oracle
from test_oracle_qfunctions import call, table
import _physics_longdouble as pl
import _physics_states as ps

sys.path.insert(0, os.path.join(ROOT, "oracle"))
from gen_golden import EDGE_CASES, EDGE_ES, EDGE_NUS, EDGE_STRETCHES, edge_groups  # noqa: E402

TOL = 1e-13                     # test_oracle_qfunctions.py: same arithmetic in another operation order
# what long double may show of the reference's own rounding (module docstring): (bar, QFunction, kind) -- first match
YARDSTICK_BARS = [(1e-8, "HyperFSEnergy", "tiny"), (1e-13, None, None)]
GROUPS = edge_groups()


@pytest.fixture(scope="module")
def edges():
    return np.load(os.path.join(GOLDEN, "qfunctions_edges.npz"))


def kinds_of(g):
    return list(dict.fromkeys(str(k) for k in g["kind"]))


def outputs(get, g, name, nu, E):
    """[(key, what `get`'s QFunction `name` gives)], the stored state under the key "gradu" """
    ins, sizes, keys = EDGE_CASES[name]
    outs = call(get(name), [nu, E], g["w"].shape[1], [g[k] for k in ins], list(sizes))
    return [(key or "gradu", o) for key, o in zip(keys, outs)]


def wanted(g, key, k):
    return g["gradu"] if key == "gradu" else g[key][k]


def test_the_fixture_holds_every_material_and_gradient_kind(edges):
    """no larger than qfunctions.npz; 15 materials; full 3 x 3 dXdx; gradients s I + 0.01 random for the six s, random at 0.3 and at 1e-7"""
    g = edges
    assert os.path.getsize(os.path.join(GOLDEN, "qfunctions_edges.npz")) <= os.path.getsize(os.path.join(GOLDEN, "qfunctions.npz"))
    assert np.array_equal(g["nus"], EDGE_NUS) and np.array_equal(g["Es"], EDGE_ES) and len(GROUPS) == 15
    Q = g["w"].shape[1]
    assert np.all(np.abs(g["SetupGeo.qdata"][1:]) > 1e-4)                  # general geometry: all nine entries of dXdx
    gu = g["gradu"].T.reshape(Q, 3, 3)
    for i, kind in enumerate(g["kind"]):
        kind = str(kind)
        if kind.startswith("s="):
            s = float(kind[2:])
            assert s in EDGE_STRETCHES and np.abs(gu[i] - s * np.eye(3)).max() <= 0.01 + 1e-12 and abs(np.trace(gu[i]) - 3 * s) <= 0.03
            assert np.abs(gu[i] - s * np.eye(3)).min() > 1e-5               # and no multiple of the identity
        else:
            amp = {"large": 0.3, "tiny": 1e-7}[kind]
            assert 0.3 * amp < np.abs(gu[i]).max() <= amp * (1 + 1e-9)
    for key in (k for _, _, ks in EDGE_CASES.values() for k in ks if k):
        assert g[key].shape[0] == 15 and g[key].shape[2] == Q and np.isfinite(g[key]).all()


def test_the_fixture_has_points_on_each_side_of_each_shift(edges):
    """hyperFS.h:45-67: left of sqrt(2)/2 - 1, between, right of sqrt(2) - 1 -- and within 0.03 of either shift on both of its sides"""
    gu = edges["gradu"].T.reshape(-1, 3, 3)
    x = np.linalg.det(np.eye(3) + gu) ** 2 - 1
    print("det C - 1:", np.round(np.sort(x), 4))
    for shift in (ps.LEFT, ps.RIGHT):
        assert ((x < shift) & (x > shift - 0.03)).any() and ((x > shift) & (x < shift + 0.03)).any(), shift
    assert (x < ps.LEFT - 0.3).any() and (x > ps.RIGHT + 1).any() and (np.abs(x) < 1e-6).any()
    tr = gu[:, 0, 0] + gu[:, 1, 1] + gu[:, 2, 2]                             # the small-strain model: 1 + tr e from 0.25 to 1.9
    assert tr.min() < -0.7 and tr.max() > 0.85


def test_setup_geo_at_the_edge_points(edges):
    g = edges
    (qd,) = call(table(_ensure_oracle(), "OracleGetQFunction")("SetupGeo"), [0.0, 0.0], g["w"].shape[1], [g["J"], g["w"]], [10])
    assert pl.distance(qd, g["SetupGeo.qdata"]) < TOL


@pytest.mark.parametrize("name", list(EDGE_CASES))
@pytest.mark.parametrize("k", range(len(GROUPS)), ids=[grp[0] for grp in GROUPS])
def test_oracle_matches_the_reference_at_the_edges(edges, k, name):
    g, (group, nu, E) = edges, GROUPS[k]
    for key, o in outputs(table(_ensure_oracle(), "OracleGetQFunction"), g, name, nu, E):
        want = wanted(g, key, k)
        for kind in kinds_of(g):
            m = g["kind"] == kind
            d = pl.distance(o[:, m], want[:, m])
            print(f"  {group} {key} {kind}: {d:.2e}")
            assert d < TOL, (group, key, kind, d)


@pytest.mark.skipif(not os.path.exists(REF_QF_LIB), reason="oracle/_ref not built (reference tree absent)")
@pytest.mark.parametrize("k", range(len(GROUPS)), ids=[grp[0] for grp in GROUPS])
def test_live_reference_reproduces_the_edge_fixture(edges, k):
    g, (group, nu, E) = edges, GROUPS[k]
    get = table(REF_QF_LIB, "RefGetQFunction")
    (qd,) = call(get("SetupGeo"), [nu, E], g["w"].shape[1], [g["J"], g["w"]], [10])
    assert np.array_equal(qd, g["SetupGeo.qdata"])
    for name in EDGE_CASES:
        for key, o in outputs(get, g, name, nu, E):
            assert np.array_equal(o, wanted(g, key, k)), (group, key)


def reference_against_long_double(g):
    """{(QFunction, output, kind): worst distance over the 15 materials of the fixture's (the reference's) values from long double}"""
    worst = {}
    for k, (group, nu, E) in enumerate(GROUPS):
        for name, (ins, sizes, keys) in EDGE_CASES.items():
            for key, ld in zip(keys, pl.evaluate(name, nu, E, [g[i] for i in ins])):
                want = wanted(g, key or "gradu", k)
                for kind in kinds_of(g):
                    m = g["kind"] == kind
                    at = (name, key or "gradu", "stretch" if kind.startswith("s=") else kind)
                    worst[at] = max(worst.get(at, 0.0), pl.distance(want[:, m], ld[:, m]))
    worst[("SetupGeo", "SetupGeo.qdata", "all")] = pl.distance(g["SetupGeo.qdata"], pl.setup_geo(g["J"], g["w"]))
    return worst


def test_the_reference_against_long_double(edges):
    """The yardstick: how far double rounding alone takes the reference's own result from the same formulas in long double.  Nothing
    but the finite-strain energy at strains of 1e-7 is ill-conditioned enough to show above the bar."""
    if not pl.EXTENDED:
        pytest.skip("numpy longdouble is no wider than double on this platform")
    for (name, key, kind), d in sorted(reference_against_long_double(edges).items()):
        bar = next(b for b, n, kd in YARDSTICK_BARS if n in (None, name) and kd in (None, kind))
        print(f"  {key:24s} {kind:8s} {d:.2e}  (bar {bar:.0e})")
        assert d < bar, (name, key, kind, d)


# --------------------------------------------------------------------------------------------------------------------------------
# the states of test_physics_edges_gpu.py do what they are for: asserted here from the oracle, on the CPU
# --------------------------------------------------------------------------------------------------------------------------------
CONFIGS = [(2, {}), (4, {}), (5, {}), (7, {}), (4, dict(qextra=1)), (4, dict(coarse_quadrature="own"))]
KINDS = [("stretch", s) for s, _ in ps.STRETCHES] + ["ramp", "tiny"]


@pytest.mark.parametrize("degree,kw", CONFIGS, ids=[f"p{d}" + "".join(f"-{k}={v}" for k, v in kw.items()) for d, kw in CONFIGS])
@pytest.mark.parametrize("meshname", list(ps.MESHES))
def test_states_reach_the_branches_they_are_for(oracle, meshname, degree, kw):
    """stretch(s): every point on the intended side of both shifts; ramp: every element holds >= 10 % of its points in each of the
    three branches (two at Q = 2) and det F > 0.6; tiny: |det C - 1| < 1e-6 -- at the points of every level with a quadrature of
    its own, from the state the oracle's residual stored; at the fine level once more from its q-data and basis tables."""
    mesh = ps.MESHES[meshname]()
    p = SolidProblem(oracle, mesh, degree, "hyperFS", nu=0.3, E=2.5, bc_sides=ps.clamped_side(mesh), **kw)
    assert len(ps.own_levels(p)) == (len(p.levels) if kw.get("coarse_quadrature") == "own" else 1)
    n = p.lsize()
    X, Y = oracle.vector(n), oracle.vector(n)
    for kind in KINDS:
        u = ps.state(p, kind)
        X.set_array(u)
        p.form_residual(X, Y)
        seen = ps.assert_preconditions(p, kind)
        for lv, (Q, lo, hi, shares, minJ) in seen.items():
            print(f"  {meshname} p{degree} {ps.state_id(kind)} level {lv} Q={Q}: det C - 1 in [{lo:.5f}, {hi:.5f}], least shares {np.round(shares, 3)}, min det F {minJ:.3f}")
        J = ps.stored_det_f(p.levels[p.fine], mesh.nelem)
        assert np.abs(ps.det_c_minus_1(p, u) - (J * J - 1)).max() < 1e-12
    p.destroy()


def test_the_three_meshes_are_ragged_and_of_the_three_kinds():
    """3 (4) elements: no multiple of the 4 and 2 elements a wave takes at Q = 3 and 5 (one a wave from Q = 6); every vertex of the
    general mesh moved, the affine one a sheared box away from the origin, the swept one a ring of four prisms."""
    assert [ps.MESHES[k]().nelem for k in ("general", "swept", "affine")] == [3, 4, 3]
    X = ps.affine_mesh()
    e = X.coords[X.cells]                                                   # [element][8][3], tensor order
    assert np.abs(e[:, 3] - e[:, 2] - e[:, 1] + e[:, 0]).max() < 1e-14 and np.abs(e[:, 7] - e[:, 6] - e[:, 5] + e[:, 4]).max() < 1e-14
    c = ps.swept_mesh()
    z = c.coords[c.cells][:, :, 2]
    assert np.all(z[:, :4] == z[:, :1]) and np.all(z[:, 4:] == z[:, 4:5]) and np.all(z[:, 4] > z[:, 0])
