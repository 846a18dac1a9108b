"""Every device kernel a default build instantiates, launched against the oracle (the matrix and the plan: tests/_kernel_matrix.py;
tests/test_kernel_inventory.py holds both against the code objects of the build).

The sweep: one test per build of the plan -- Q = 2..8, qextra 0..2, the three physics, multigrid="uniform" (every P <= the fine one is a
level), six geometry cases -- on meshes with more elements than a wave packs, a count that is no multiple of the pack, and neighbours:
qdata, the residual with its stored state, and on every level the Jacobian action, the diagonal into a pre-filled vector, exact zeros
in the constrained rows and both transfers, device against oracle on identical inputs.  After every apply kernel_name must be exactly
the instantiation and the geometry form the plan expects: a mesh that falls back to another form fails.  The device forms are held
against each other where there are two (stored / recomputed, affine / general, swept / general, derived / plain tangent).

Tolerances are the project's own: 1e-10 relative to the oracle (BASELINE.json north_star) in the 2-norm, and the same in the max norm --
one wrong entry of one element moves an entry by order one; 1e-12 for the stored state, 1e-13 for qdata and between two device forms
(test_gpu_parity.py).  With CPS_KERNEL_MATRIX_REPORT=<file> the worst figure per family and Q and the kernels launched are written
there."""
import functools
import os
import time
from collections import OrderedDict

import numpy as np
import pytest

import _kernel_matrix as km
from ceedpetscsolid_amd import solid
from ceedpetscsolid_amd.mesh import box_mesh, dirichlet_mask, hollow_cylinder_mesh, side_set_nodes
from ceedpetscsolid_amd.solid import SolidProblem
from _ceed_env import ceed_with_env
from test_coarse_quadrature_gpu import meshes as state_meshes, state_both
from test_gpu_parity import _relabel_axes, distorted_box

pytestmark = pytest.mark.gpu

TOL = 1e-10          # device against oracle, 2-norm and max norm
TOL_STATE = 1e-12    # stored grad u
TOL_QDATA = 1e-13
TOL_FORMS = 1e-13    # two device forms of the same operator

PLAN = km.plan()
SWITCHED = [("CEED_MI355X_GEO",), ("CEED_MI355X_AFFINE",), ("CEED_MI355X_SWEPT",), ("CEED_MI355X_DERIVED",), ("CEED_MI355X_DERIVED", "CEED_MI355X_GEO")]
SHEAR = np.array([[1.0, 0.3, -0.2], [0.1, 0.7, 0.25], [-0.15, 0.2, 1.4]])      # no axis-aligned box: a diagonal dXdx would hide a wrong off-diagonal index


# --------------------------------------------------------------------------------------------------------------------------------
# the record of a run
# --------------------------------------------------------------------------------------------------------------------------------
class Record:
    def __init__(self):
        self.worst, self.launched, self.ran, self.t0 = {}, set(), set(), time.time()

    def error(self, family, Q, e2, einf):
        w = self.worst.setdefault((family, Q), [0.0, 0.0])
        w[0], w[1] = max(w[0], e2), max(w[1], einf)

    def write(self, path):
        want = km.matrix()
        with open(path, "w") as f:
            f.write(f"kernel matrix sweep: {len(self.ran)} of {len(PLAN)} builds of the plan, {time.time() - self.t0:.1f} s from the first test of the file to the last\n")
            f.write("kernels launched / instantiated per family (fused, setup_geo, transfer and state by the reported kernel_name; diag by the basis of the level; "
                    "weighted transfers by the changed answer):\n")
            for fam in km.FAMILIES:
                f.write(f"  {fam:10s} {len({k for k in self.launched if k[0] == fam}):4d} / {len(want[fam])}\n")
            f.write("worst error against the oracle (device forms against each other: family 'forms'), relative, 2-norm | max norm:\n")
            for (fam, Q), (e2, einf) in sorted(self.worst.items()):
                f.write(f"  {fam:14s} Q={Q}  {e2:.2e} | {einf:.2e}\n")


RECORD = Record()


@pytest.fixture(scope="module", autouse=True)
def report():
    RECORD.t0 = time.time()
    yield
    path = os.environ.get("CPS_KERNEL_MATRIX_REPORT")
    if path:
        RECORD.write(path)


def errors(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    n2, ninf = np.linalg.norm(want), np.abs(want).max()
    assert n2 > 0
    return np.linalg.norm(got - want) / n2, np.abs(got - want).max() / ninf


def hold(family, Q, what, got, want, tol2, tolinf=TOL):
    e2, einf = errors(got, want)
    RECORD.error(family, Q, e2, einf)
    print(f"  {family} Q={Q} {what}: {e2:.2e} | {einf:.2e}")
    assert e2 <= tol2 and einf <= tolinf, (family, Q, what, e2, einf)


# --------------------------------------------------------------------------------------------------------------------------------
# meshes and runs
# --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sweep_mesh(name, Q):
    """(mesh, clamped side set).  Counts: 27 and 21 elements for Q <= 5 (a wave packs 8, 4, 4, 2), 12 and 10 for Q >= 6 (one)."""
    small = Q >= 6
    if name == "general":                                       # every vertex moved: no affine element, no sweep
        return distorted_box(3, 2, 2, seed=2, amp=0.2) if small else distorted_box(3, 3, 3, seed=2, amp=0.2), 1
    if name == "affine":
        m = box_mesh(3, 2, 2) if small else box_mesh(3, 3, 3)
        m.coords = m.coords @ SHEAR.T + np.array([0.3, -0.1, 0.2])
        return m, 1
    base = hollow_cylinder_mesh(1, 5, 2) if small else hollow_cylinder_mesh(1, 7, 3)
    perm = {"swept0": [1, 2, 0], "swept1": [2, 0, 1], "swept2": [0, 1, 2]}[name]    # the sweep (z) along reference direction 0, 1, 2
    return (base if name == "swept2" else _relabel_axes(base, perm)), 998


def run_build(ceed, meshname, Q, qextra, physics, names):
    """Everything the sweep compares, of one SolidProblem on `ceed`; with `names` the kernel_name after every apply as well."""
    mesh, side = sweep_mesh(meshname, Q)
    assert mesh.nelem > km.group_elems(Q) and (km.group_elems(Q) == 1 or mesh.nelem % km.group_elems(Q) != 0)
    p = SolidProblem(ceed, mesh, Q - 1 - qextra, physics, nu=0.3, E=2.0, bc_sides=[side], multigrid="uniform", qextra=qextra)
    out, nm = {"qdata": p.qdata.to_numpy()}, {}
    assert [lv.degree + 1 for lv in p.levels] == list(range(2, Q - qextra + 1)) and p.Q == Q
    n = p.lsize()
    X, Y = ceed.vector(n).set_array(p.smooth_state(0.1)), ceed.vector(n)
    p.form_residual(X, Y)
    out["residual"] = Y.to_numpy()
    if p.gradu is not None:
        out["state"] = p.gradu.to_numpy()
    if names:
        nm["setup_geo"], nm["residual"] = p.setupgeo_kernel, p.opApply.kernel_name
    for lv in range(len(p.levels)):
        nl = p.lsize(lv)
        x = np.random.default_rng(7 + lv).uniform(-1, 1, nl)
        Xl, Yl, D = ceed.vector(nl).set_array(x), ceed.vector(nl), ceed.vector(nl)
        p.apply_jacobian(lv, Xl, Yl)
        if names:
            nm[f"jacobian{lv}"] = p.levels[lv].opJacob.kernel_name
        D.set_value(7.0)                                        # overwrite semantics
        p.get_diag(lv, D)
        out[f"jacobian{lv}"], out[f"diag{lv}"], out[f"mask{lv}"] = Yl.to_numpy(), D.to_numpy(), p.levels[lv].mask.copy()
        if lv > 0:
            nc = p.lsize(lv - 1)
            Xc, Yf, Yc = ceed.vector(nc).set_array(np.random.default_rng(70 + lv).uniform(-1, 1, nc)), ceed.vector(nl), ceed.vector(nc)
            Yf.set_value(5.0); Yc.set_value(5.0)
            p.prolong(lv, Xc, Yf); p.restrict(lv, Xl, Yc)
            out[f"prolong{lv}"], out[f"restrict{lv}"] = Yf.to_numpy(), Yc.to_numpy()
            if names:
                nm[f"prolong{lv}"], nm[f"restrict{lv}"] = p.levels[lv].opProlong.kernel_name, p.levels[lv].opRestrict.kernel_name
            for v in (Xc, Yf, Yc):
                v.destroy()
        for v in (Xl, Yl, D):
            v.destroy()
    X.destroy(); Y.destroy()
    p.destroy()
    return out, nm


_RUNS = OrderedDict()      # the last few runs: the builds of one (Q, qextra, physics) share the oracle's run and the compared device forms


def run_once(key, ceed, names):
    if key not in _RUNS:
        _RUNS[key] = run_build(ceed, *key[1:], names)
        while len(_RUNS) > 12:
            _RUNS.popitem(last=False)
    return _RUNS[key]


@pytest.fixture(scope="module")
def ceeds(gpu, product_lib):
    made = {(): gpu}
    for sw in SWITCHED:
        made[sw] = ceed_with_env(product_lib, {s: "0" for s in sw})
    return made


def expected_names(b, geo, derived):
    """kernel_name after every apply of build `b`, its fused kernels on geometry form `geo`, the tangent with or without the derived state."""
    Pfine = km.build_degree(b) + 1
    jac = km.PHYSICS[b.physics][1]
    if jac == "HyperFSdF" and derived and km.derived_state(b.Q):
        jac += "+derived"
    nm = {"setup_geo": f"setup_geo<Q={b.Q}>", "residual": km.fused_name(Pfine, b.Q, km.PHYSICS[b.physics][0], geo)}
    for lv, P in enumerate(range(2, Pfine + 1)):
        nm[f"jacobian{lv}"] = km.fused_name(P, b.Q, jac, geo)
        if lv > 0:
            nm[f"prolong{lv}"], nm[f"restrict{lv}"] = f"prolong<Pc={P - 1},Pf={P}>", f"restrict<Pc={P - 1},Pf={P}>"
    return nm


def against_oracle(b, got, want):
    Q = b.Q
    hold("setup_geo", Q, "qdata", got["qdata"], want["qdata"], TOL_QDATA)
    hold("fused", Q, "residual", got["residual"], want["residual"], TOL)
    if "state" in want:
        hold("fused state", Q, "stored state", got["state"], want["state"], TOL_STATE)
    for lv in range(km.build_degree(b)):
        mask = want[f"mask{lv}"]
        assert np.array_equal(got[f"mask{lv}"], mask)
        hold("fused", Q, f"jacobian level {lv}", got[f"jacobian{lv}"], want[f"jacobian{lv}"], TOL)
        assert np.all(got[f"jacobian{lv}"][mask != 0] == 0.0), ("constrained rows of the Jacobian", lv)
        hold("diag", Q, f"diagonal level {lv}", got[f"diag{lv}"], want[f"diag{lv}"], TOL)
        if lv > 0:
            hold("transfer", Q, f"prolong to level {lv}", got[f"prolong{lv}"], want[f"prolong{lv}"], TOL)
            hold("transfer", Q, f"restrict from level {lv}", got[f"restrict{lv}"], want[f"restrict{lv}"], TOL)
            assert np.all(got[f"prolong{lv}"][mask != 0] == 0.0) and np.all(got[f"restrict{lv}"][want[f"mask{lv - 1}"] != 0] == 0.0)


def against_form(b, got, other):
    for k in got:
        if k.startswith(("residual", "state", "jacobian")):
            hold("forms", b.Q, k, got[k], other[k], TOL_FORMS)


def launched_by(b, nm, geo):
    """The kernels the reported names stand for (the diagonal entry point reports none: its shape follows from the level's basis)."""
    ks = set()
    for what, name in nm.items():
        if what == "setup_geo":
            ks.add(("setup_geo", int(name[len("setup_geo<Q="):-1])))
        elif what.startswith(("prolong", "restrict")):
            c, f = name[name.index("<") + 1:-1].split(",")
            ks.add(("transfer", int(c[3:]), int(f[3:]), what.startswith("prolong"), False))
        else:
            head = name[len("fused_grad<"):name.index(">/pencil")].split(",")
            ks.add(("fused", int(head[0][2:]), int(head[1][2:]), head[2], geo))
    for P in range(2, km.build_degree(b) + 2):
        ks.add(("diag", P, b.Q, km.PHYSICS[b.physics][1]))
    return ks


@pytest.mark.parametrize("b", PLAN, ids=[km.build_id(b) for b in PLAN])
def test_build_matches_the_oracle_on_the_planned_kernels(oracle, ceeds, b):
    meshname, geo, _ = km.GEOMETRIES[b.geometry]
    key = (meshname, b.Q, b.qextra, b.physics)
    want, _ = run_once(("oracle",) + key, oracle, False)
    got, nm = run_once((km.build_switches(b),) + key, ceeds[km.build_switches(b)], True)
    # the instantiation and the geometry form of every apply: a fallback to another form is a failure, whatever it computes
    assert nm == expected_names(b, geo, b.derived), (nm, expected_names(b, geo, b.derived))
    launched = launched_by(b, nm, geo)
    assert launched == km.build_kernels(b), sorted(map(km.show, launched ^ km.build_kernels(b)))
    against_oracle(b, got, want)
    if not b.derived:                  # the plain tangent against the one that reads the derived state HyperFSF wrote (same geometry form)
        sw = tuple(s for s in km.build_switches(b) if s != "CEED_MI355X_DERIVED")
        other, onm = run_once((sw,) + key, ceeds[sw], True)
        assert onm == expected_names(b, geo, True)
        against_form(b, got, other)
    elif b.geometry in km.COMPARE:     # the other device form of the same geometry
        sw, ogeo = km.COMPARE[b.geometry]
        other, onm = run_once((sw,) + key, ceeds[sw], True)
        assert onm == expected_names(b, ogeo, True), (onm, expected_names(b, ogeo, True))
        against_form(b, got, other)
    RECORD.launched |= launched
    RECORD.ran.add(b)


# --------------------------------------------------------------------------------------------------------------------------------
# the smaller families
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Pf,Qc", km.STATE_PAIRS)
@pytest.mark.parametrize("meshname", ["cylinder", "three elements"])
def test_state_kernel_on_every_instantiated_pair(oracle, gpu, meshname, Pf, Qc):
    mesh, bc = state_meshes(meshname)
    want, got = state_both(oracle, gpu, mesh, bc, "hyperFS", Pf, Qc)        # (asserts the kernel name)
    assert got.size == 9 * mesh.nelem * Qc ** 3 and not np.any(got == -7.0)  # every entry written
    hold("state", Qc, f"{meshname} state<Pf={Pf},Qc={Qc}>", got, want, TOL)
    RECORD.launched.add(("state", Pf, Qc))


@pytest.mark.parametrize("degree,kind", km.TRANSFER_LADDERS, ids=[f"p{d}-{k}" for d, k in km.TRANSFER_LADDERS])
def test_transfers_plain_and_weighted_on_every_pair(oracle, gpu, monkeypatch, degree, kind):
    """Every (Pc, Pf) pair, both directions, with the unit weights of one rank (the plain kernels) and with a fine-side scale that counts
    phantom neighbours on one face (the weighted kernels: test_weighted_owner_form_of_an_element_partition); (2, 4) and (2, 5) are the
    two-level ladders [1, 3] and [1, 4], which no multigrid option produces.  Restrict = Prolong^T on the device in both forms."""
    if kind == "two-level":
        monkeypatch.setattr(solid, "level_degrees", lambda d, mg="logarithmic": [1, d])
    mesh = distorted_box(3, 3, 2, seed=4)                       # 18 elements: a wave packs 4, 4, 2, 1 (xfer_group_elems)
    probs = [SolidProblem(c, mesh, degree, "linElas", nu=0.3, E=1.0, bc_sides=[1], multigrid="uniform" if kind == "uniform" else "logarithmic")
             for c in (oracle, gpu)]
    pairs = km.ladder_pairs(degree, kind)
    assert [(a.degree + 1, b.degree + 1) for a, b in zip(probs[1].levels[:-1], probs[1].levels[1:])] == pairs
    rng, scales = np.random.default_rng(7), []
    for lv, (Pc, Pf) in enumerate(pairs, start=1):
        nf, nc = probs[0].lsize(lv), probs[0].lsize(lv - 1)
        xc, xf = rng.uniform(-1, 1, nc), rng.uniform(-1, 1, nf)
        dm = probs[0].levels[lv].dofmap
        phantom = dirichlet_mask(dm, side_set_nodes(mesh, dm, [2])).astype(np.float64)      # the dofs of the free z+ face
        assert 0 < phantom.sum() < nf
        scale = probs[0].levels[lv].multinv.to_numpy() / (1.0 + phantom)
        plain = None
        for weighted in (False, True):
            res = []
            for p in probs:
                c, L = p.ceed, p.ceed.L
                if weighted:
                    sc = c.vector(nf).set_array(scale)
                    scales.append(sc)                           # alive to the end of the test
                    for op in (p.levels[lv].opProlong, p.levels[lv].opRestrict):
                        L.chk(L.lib.CeedXOperatorSetFineScale(op.h, sc.h))
                Xc, Yf, Xf, Yc = c.vector(nc).set_array(xc), c.vector(nf), c.vector(nf).set_array(xf), c.vector(nc)
                Yf.set_value(5.0); Yc.set_value(5.0)
                p.prolong(lv, Xc, Yf); p.restrict(lv, Xf, Yc)
                res.append((Yf.to_numpy(), Yc.to_numpy()))
            form = "weighted" if weighted else "plain"
            hold("transfer", Pf, f"{form} prolong<Pc={Pc},Pf={Pf}>", res[1][0], res[0][0], TOL)
            hold("transfer", Pf, f"{form} restrict<Pc={Pc},Pf={Pf}>", res[1][1], res[0][1], TOL)
            g = probs[1].levels[lv]
            assert (g.opProlong.kernel_name, g.opRestrict.kernel_name) == (f"prolong<Pc={Pc},Pf={Pf}>", f"restrict<Pc={Pc},Pf={Pf}>")
            assert np.all(res[1][0][g.mask != 0] == 0.0) and np.all(res[1][1][probs[1].levels[lv - 1].mask != 0] == 0.0)
            lhs, rhs = float(res[1][0] @ xf), float(xc @ res[1][1])
            assert abs(lhs - rhs) <= 1e-13 * max(abs(lhs), abs(rhs), 1.0), (form, Pc, Pf, lhs, rhs)
            if weighted:       # the weighted path ran: half the plain value at the phantom face (where it is not constrained), the plain one elsewhere
                face = (phantom != 0) & (g.mask == 0)
                assert np.abs(plain[0][face]).max() > 0 and np.allclose(res[1][0][face], 0.5 * plain[0][face], rtol=1e-12, atol=0)
                assert np.allclose(res[1][0][~face], plain[0][~face], rtol=1e-12, atol=1e-15)
                assert not np.array_equal(res[1][1], plain[1])
            else:
                plain = res[1]
            RECORD.launched |= {("transfer", Pc, Pf, pro, weighted) for pro in (True, False)}
    for p in probs:
        p.destroy()


def test_the_sweep_launched_nothing_outside_the_matrix_and_all_of_it_when_whole():
    """Runs last: what the tests above launched (by the names the library reported) is inside the matrix, and IS the matrix when every
    build of the plan, every state pair and every ladder ran in this session (a selection with -k or -x checks the first half only)."""
    want = set().union(*km.matrix().values())
    assert RECORD.launched <= want, sorted(map(km.show, RECORD.launched - want))
    if RECORD.ran == set(PLAN) and {k for k in RECORD.launched if k[0] in ("state", "transfer")} == km.state_kernels() | km.transfer_kernels():
        assert RECORD.launched == want, sorted(map(km.show, want - RECORD.launched))
