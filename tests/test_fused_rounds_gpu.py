"""The persistent group loop of the fused kernels, walked in every instantiation (k_fused_pencil<P, Q, QF, GEO> and k_fused_pencil_mass;
csrc/kernel_fused_pencil_body.hpp, `for (;;)` ... `if (!more) break`).

The sweep of tests/test_kernel_matrix_gpu.py launches every kernel on meshes of a few groups: the launcher caps the grid at the group
count, so every wave there takes one group, requests no next one (g_nx == grp) and leaves after one iteration.  Here the same builds
(_kernel_matrix.plan()) run on the meshes of tests/_fused_rounds.py with CEED_MI355X_PENCIL_WAVES=1: on a 256-CU device the grid is 256
workgroups in eight XCD chunks, the low wave ranks of a chunk take a first, a middle and a last round, the others two, the last chunk is
shorter, and the partial group (E > 1) is reached in a later round.  What crosses an iteration -- the next group's offsets (off_nx ->
off, with the Dirichlet flags in their top bits), the q-point register sets refilled for `this group or the next`, x of the next group
loaded behind the k-transpose, the bases of state_in / state_out / evec of round two -- is then run in every kernel.

(a) bitwise: an element's arithmetic does not depend on which wave runs it and the node sum is ordered, so the results
under one wave per CU ARE those of the default Ceed, which on these meshes runs one round per wave.  (b) a subset against the oracle,
so that the pair of (a) cannot be wrong together.  (c) a segment of the pipelined form that begins behind element 0 and runs several
rounds.  Tolerances are those of the matrix sweep: 1e-10 in the 2-norm and the max norm, 1e-12 for the stored state.

With CPS_FUSED_ROUNDS_REPORT=<file> the launch figures, the builds run and the worst oracle error per Q are written there."""
import ctypes as C
import os
import time
from collections import OrderedDict

import numpy as np
import pytest
import torch

import _fused_rounds as fr
import _kernel_matrix as km
from _ceed_env import ceed_with_env
from ceedpetscsolid_amd.mass import MassOperator
from ceedpetscsolid_amd.solid import SolidProblem
from test_fused_mass_gpu import mass_name
from test_kernel_matrix_gpu import TOL, TOL_STATE, errors, expected_names

pytestmark = pytest.mark.gpu

PLAN = km.plan()
NU, E_MOD = 0.3, 2.0
MASS_C = 1.75 * E_MOD
WAVES1 = {"CEED_MI355X_PENCIL_WAVES": "1"}
# (c): two segments whatever the size.  pipe_elem_bound (index_maps.hpp) without a minimum of rounds cuts at group ngroups / 2: elements
# 544 of 1089 at Q = 5 (545 in the last segment, 273 groups), 283 of 567 at Q = 7 (284 groups) -- more than the 256 workgroups either way.
PIPED = dict(WAVES1, CEED_MI355X_PIPE_SEGMENTS="2", CEED_MI355X_PIPE_MIN_ROUNDS="0")
PHYSICS = list(km.PHYSICS)


def oracle_subset():
    """(b): per Q and geometry case one physics at qextra 0, rotating so that every physics meets every geometry at some Q, and the
    plain finite-strain tangents from Q = 6."""
    want = {(Q, g): PHYSICS[(iq + ig) % 3] for iq, Q in enumerate(km.QS) for ig, g in enumerate(km.GEOMETRIES)}
    out = [b for b in PLAN if b.qextra == 0 and (not b.derived or want[(b.Q, b.geometry)] == b.physics)]
    assert all({b.physics for b in out if b.geometry == g and b.derived} == set(PHYSICS) for g in km.GEOMETRIES)
    return out


ORACLE_SUBSET = oracle_subset()


class Record:
    def __init__(self):
        self.tried, self.ran, self.names, self.anchored, self.worst, self.t0 = set(), set(), set(), set(), {}, time.time()

    def error(self, Q, e2, einf):
        w = self.worst.setdefault(Q, [0.0, 0.0])
        w[0], w[1] = max(w[0], e2), max(w[1], einf)

    def write(self, path, ncu):
        with open(path, "w") as f:
            f.write(f"fused rounds sweep on {ncu} CUs: {len(self.ran)} of {len(PLAN)} builds of the plan bitwise, {len(self.anchored)} of "
                    f"{len(ORACLE_SUBSET)} against the oracle, {time.time() - self.t0:.1f} s from the first test of the file to the last\n")
            f.write("launch of the whole mesh per size class (groups, grid, XCD chunks, workgroups per number of rounds):\n")
            for cls, Q in fr.SIZE_CLASSES.items():
                for what, w in (("CEED_MI355X_PENCIL_WAVES=1", 1), ("default", 0)):
                    d = fr.describe(Q, ncu, w)
                    f.write(f"  {cls:5s} {d['nelem']:5d} elements  {what:27s} groups {d['ngroups']:4d}  grid {d['grid']:4d}  chunks {d['chunks']}  rounds {d['hist']}\n")
            fused = {k for k in self.names if "+mass" not in k}
            f.write(f"kernel names reported under one wave per CU: {len(fused)} without the mass term, {len(self.names) - len(fused)} with it\n")
            f.write("builds run / builds of the plan (_kernel_matrix.plan(): qextra 0 .. 2 x three physics x six geometry cases, and the plain tangents from Q = 6):\n")
            for Q in km.QS:
                f.write(f"  Q={Q}  {sum(1 for b in self.ran if b.Q == Q):3d} / {sum(1 for b in PLAN if b.Q == Q)}\n")
            if self.ran != set(PLAN):
                f.write("  not run: " + " ".join(km.build_id(b) for b in PLAN if b not in self.ran) + "\n")
            f.write("worst error against the oracle under one wave per CU, relative, 2-norm | max norm:\n")
            for Q, (e2, einf) in sorted(self.worst.items()):
                f.write(f"  Q={Q}  {e2:.2e} | {einf:.2e}\n")


RECORD = Record()


@pytest.fixture(scope="module")
def ncu():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module", autouse=True)
def report(ncu):
    RECORD.t0 = time.time()
    yield
    path = os.environ.get("CPS_FUSED_ROUNDS_REPORT")
    if path:
        RECORD.write(path, ncu)


@pytest.fixture(scope="module")
def ceeds(gpu, product_lib):
    """(switches set to 0, further variables) -> Ceed, made when first asked for; ((), ()) is the default `gpu`."""
    made = {((), ()): gpu}

    def get(switches, extra=()):
        key = (tuple(switches), tuple(sorted(dict(extra).items())))
        if key not in made:
            made[key] = ceed_with_env(product_lib, dict({s: "0" for s in switches}, **dict(extra)))
        return made[key]
    return get


def the_loop_must_run(ncu, Q, meshname):
    ok, msg = fr.loop_runs(ncu, Q, meshname)
    assert ok, "this device does not run the group loop of the fused kernel on the sweep's mesh: " + msg
    d = fr.describe(Q, ncu, 0, meshname)
    assert d["hist"] == {1: d["ngroups"]}, ("the default Ceed is the one-round reference of the sweep", d)


# --------------------------------------------------------------------------------------------------------------------------------
# one run of one problem
# --------------------------------------------------------------------------------------------------------------------------------
def run_build(ceed, meshname, Q, qextra, physics, reference=False):
    """What the sweep compares, of one SolidProblem on `ceed`: (arrays, kernel names, launch infos).  `reference` (the oracle): no names,
    and M x of the fine level from the portable mass operator in place of the fused term."""
    mesh, sides = fr.rounds_mesh(meshname, Q)
    p = SolidProblem(ceed, mesh, Q - 1 - qextra, physics, nu=NU, E=E_MOD, bc_sides=sides, multigrid="uniform", qextra=qextra)
    assert [lv.degree + 1 for lv in p.levels] == list(range(2, Q - qextra + 1)) and p.Q == Q
    out, nm, info = {}, {}, {}
    n = p.lsize()
    X, Y = ceed.vector(n).set_array(p.smooth_state(0.1)), ceed.vector(n)
    Y.set_value(5.0)
    p.form_residual(X, Y)
    out["residual"] = Y.to_numpy()
    if p.gradu is not None:
        out["state"] = p.gradu.to_numpy()
    if not reference:
        nm["residual"], info["residual"] = p.opApply.kernel_name, p.opApply.launch_info()
    for lv, level in enumerate(p.levels):
        nl = p.lsize(lv)
        x = np.random.default_rng(7 + lv).uniform(-1, 1, nl)
        Xl, Yl = ceed.vector(nl).set_array(x), ceed.vector(nl)
        Yl.set_value(5.0)                                       # overwrite semantics
        p.apply_jacobian(lv, Xl, Yl)
        out[f"jacobian{lv}"], out[f"mask{lv}"] = Yl.to_numpy(), level.mask.copy()
        op = level.opJacob
        if reference:
            if lv == p.fine and Q <= 7:
                out["mass_x"] = np.where(level.mask == 0, MassOperator(p, lv, MASS_C, portable=True).apply_host(x), 0.0)
        else:
            nm[f"jacobian{lv}"], info[f"jacobian{lv}"] = op.kernel_name, op.launch_info()
            if op.mass_term_available():
                op.set_mass_term(MASS_C)
                Yl.set_value(-3.0)
                op.apply(Xl, Yl)
                out[f"mass{lv}"], nm[f"mass{lv}"], info[f"mass{lv}"] = Yl.to_numpy(), op.kernel_name, op.launch_info()
                op.set_mass_term(0.0)
        Xl.destroy(); Yl.destroy()
    X.destroy(); Y.destroy()
    p.destroy()
    return out, nm, info


_RUNS = OrderedDict()      # the last few runs: the builds of one (Q, qextra, physics) share the default Ceed's and the oracle's run


def run_once(which, ceed, key, reference=False):
    k = (which,) + key
    if k not in _RUNS:
        _RUNS[k] = run_build(ceed, *key, reference)
        while len(_RUNS) > 8:
            _RUNS.popitem(last=False)
    return _RUNS[k]


def names_of(b, geo, nm):
    """The names build `b` must report on geometry form `geo`: those of the matrix sweep's fused applies, and with the term where there is one."""
    want = {k: v for k, v in expected_names(b, geo, b.derived).items() if k.startswith(("residual", "jacobian"))}
    for lv, P in enumerate(range(2, km.build_degree(b) + 2)):
        if f"mass{lv}" in nm:
            want[f"mass{lv}"] = mass_name(P, b.Q, km.jacobian_qf(b), geo)
    return want


def same_bits(got, ref, what):
    assert sorted(got) == sorted(ref), what
    for k in ref:
        assert got[k].shape == ref[k].shape and np.isfinite(ref[k]).all(), (what, k)
        if not k.startswith("mask"):
            assert np.abs(ref[k]).max() > 0, (what, k)
        assert np.array_equal(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()), float(np.abs(got[k] - ref[k]).max()))


def constrained_rows_are_zero(out, what):
    nlev = sum(1 for k in out if k.startswith("mask"))
    for lv in range(nlev):
        fixed = out[f"mask{lv}"] != 0
        assert fixed.any()
        for k in (f"jacobian{lv}", f"mass{lv}"):
            if k in out:
                assert np.all(out[k][fixed] == 0.0), (what, k)


def build_run(ceeds, b, extra, which):
    """The run of build `b` on the Ceed of its switches and the variables `extra`; names and the serial launch form asserted."""
    meshname, geo, _ = km.GEOMETRIES[b.geometry]
    sw = km.build_switches(b)
    out, nm, info = run_once((which, sw), ceeds(sw, extra), (meshname, b.Q, b.qextra, b.physics))
    # the instantiation and the geometry form of every apply: a fallback to another form is a failure, whatever it computes
    assert nm == names_of(b, geo, nm), (which, nm, names_of(b, geo, nm))
    assert all(i["segments"] == 1 and i["last_segment_elements"] == fr.nelem_of(b.Q) for i in info.values()), (which, info)
    assert ("mass0" in nm) == (b.Q <= 7), "the kernels with the mass term: Q = 2 .. 7"
    return out, nm


# --------------------------------------------------------------------------------------------------------------------------------
# (a) every build of the plan: the bits of one round per wave
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", PLAN, ids=[km.build_id(b) for b in PLAN])
def test_rounds_give_the_bits_of_one_round_per_wave(ceeds, ncu, b):
    the_loop_must_run(ncu, b.Q, km.GEOMETRIES[b.geometry][0])
    RECORD.tried.add(b)
    ref, got = build_run(ceeds, b, (), "default"), build_run(ceeds, b, WAVES1, "waves1")
    assert sorted(ref[1]) == sorted(got[1])
    same_bits(got[0], ref[0], km.build_id(b))
    constrained_rows_are_zero(got[0], km.build_id(b))
    constrained_rows_are_zero(ref[0], km.build_id(b))
    RECORD.names |= set(got[1].values())
    RECORD.ran.add(b)


# --------------------------------------------------------------------------------------------------------------------------------
# (b) the anchor: the results under one wave per CU against the oracle
# --------------------------------------------------------------------------------------------------------------------------------
def hold(Q, what, got, want, tol2, tolinf=TOL):
    e2, einf = errors(got, want)
    RECORD.error(Q, e2, einf)
    print(f"  Q={Q} {what}: {e2:.2e} | {einf:.2e}")
    assert e2 <= tol2 and einf <= tolinf, (Q, what, e2, einf)


@pytest.mark.parametrize("b", ORACLE_SUBSET, ids=[km.build_id(b) for b in ORACLE_SUBSET])
def test_rounds_match_the_oracle(oracle, oracle_lib, ceeds, ncu, b):
    meshname = km.GEOMETRIES[b.geometry][0]
    the_loop_must_run(ncu, b.Q, meshname)
    got, nm = build_run(ceeds, b, WAVES1, "waves1")
    oracle_lib.lib.OracleSetNumThreads(C.c_int(max(1, min(16, len(os.sched_getaffinity(0))))))
    try:
        want, _, _ = run_once(("oracle",), oracle, (meshname, b.Q, b.qextra, b.physics), reference=True)
    finally:
        oracle_lib.lib.OracleSetNumThreads(C.c_int(1))
    hold(b.Q, "residual", got["residual"], want["residual"], TOL)
    if "state" in want:
        hold(b.Q, "stored state", got["state"], want["state"], TOL_STATE)
    fine = km.build_degree(b) - 1
    for lv in range(fine + 1):
        assert np.array_equal(got[f"mask{lv}"], want[f"mask{lv}"])
        hold(b.Q, f"jacobian level {lv}", got[f"jacobian{lv}"], want[f"jacobian{lv}"], TOL)
    if f"mass{fine}" in got:
        assert "+mass" in nm[f"mass{fine}"]
        hold(b.Q, f"jacobian with the mass term, level {fine}", got[f"mass{fine}"], want[f"jacobian{fine}"] + want["mass_x"], TOL)
        # the term is in the sum: on these fine meshes c M x is small beside K x (5e-4 of it at Q = 2), and still 1e5 times the bound above
        assert np.abs(want["mass_x"]).max() > 1e5 * TOL * np.abs(want[f"jacobian{fine}"]).max()
    RECORD.anchored.add(b)


# --------------------------------------------------------------------------------------------------------------------------------
# (c) a segment that begins behind element 0 and runs several rounds
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [km.Build(5, 0, "hyperFS", "general", True), km.Build(7, 0, "hyperFS", "affine", True)], ids=km.build_id)
def test_a_later_segment_of_several_rounds_gives_the_serial_bits(ceeds, ncu, b):
    meshname, geo, _ = km.GEOMETRIES[b.geometry]
    the_loop_must_run(ncu, b.Q, meshname)
    key, E = (meshname, b.Q, b.qextra, b.physics), fr.pencil_group_elems(b.Q)
    ref, rnm, rinfo = run_once(("default", ()), ceeds(()), key)
    got, nm, info = run_once(("piped", ()), ceeds((), PIPED), key)
    assert all(i["segments"] == 1 for i in rinfo.values()), rinfo
    assert nm == names_of(b, geo, nm) == rnm
    for what, i in info.items():
        assert i["segments"] == 2 and i["streams"] == 2, (what, i)
        last = i["last_segment_elements"]
        assert ncu * E < last < fr.nelem_of(b.Q), (what, i)
        # the launch of the last segment alone: more groups than workgroups, so some of them take a second round
        lists = fr.rounds(last, b.Q, ncu, 1)
        assert max(len(gl) for gl in lists) >= 2 and (fr.nelem_of(b.Q) - last) % E == 0, (what, i)
    same_bits(got, ref, km.build_id(b))
    constrained_rows_are_zero(got, km.build_id(b))


def test_every_build_ran_and_every_fused_kernel_looped():
    """Runs last.  In a whole run of the file: every build of the plan went through (a), every build of the subset through (b), and every
    kernel of the matrix's fused family is among the names the Ceed with one wave per CU reported (a selection with -k checks nothing)."""
    whole = len(RECORD.tried) == len(PLAN)
    reported = set()
    for name in RECORD.names:
        if "+mass" in name:
            continue
        head = name[len("fused_grad<"):name.index(">/pencil")].split(",")
        geo = {v: k for k, v in km.GEO_TEXT.items()}[name[name.index("[") + 1:-1]]
        reported.add(("fused", int(head[0][2:]), int(head[1][2:]), head[2], geo))
    want = km.matrix()["fused"]
    assert reported <= want, sorted(map(km.show, reported - want))
    if whole:
        assert RECORD.ran == set(PLAN) and len(RECORD.ran) == len(km.plan())
        assert reported == want, sorted(map(km.show, want - reported))
        assert sum(1 for n in RECORD.names if "+mass" in n) > 0
    if len(RECORD.anchored) == len(ORACLE_SUBSET):
        assert set(RECORD.worst) == set(km.QS)
