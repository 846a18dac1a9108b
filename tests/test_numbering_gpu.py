"""The device operators under caller-chosen node numberings ("the boundary takes ANY offsets").

Every other GPU test numbers its nodes with build_dofmap's locality order -- shell nodes 0 .. nshell-1 in first-touch order, then one
contiguous interior run per element, no unused entry -- under which node_off[r] == 3 r in the serial transpose map, int_off is a
run, the owner of a fine node has the lowest number and every L-vector entry is covered.  Here the numberings of tests/_numbering.py
replace it (tests/test_numbering.py checks on the CPU that the oracle, the yardstick, does not see the difference).

Two comparisons per output.  Against the oracle under the SAME numbering: rel_err < 1e-10, this suite's device-vs-oracle bar.  Against
the device under the DEFAULT numbering, mapped back: np.array_equal, because nothing the device adds depends on what a node is
called: per-element arithmetic never sees the numbering, node_sum3 and the nine-wide sum add a row's contributors in element order,
the owner of a fine node is its first element entry either way."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import _numbering as nb
import test_gpu_parity as parity
from _ceed_env import ceed_with_env
from _newton_tolerance import straddling_snes_rtol
from ceedpetscsolid_amd import solid
from ceedpetscsolid_amd.mesh import box_mesh, hollow_cylinder_mesh, load_mesh_npz
from ceedpetscsolid_amd.solver import NewtonPMG
from conftest import GOLDEN, rel_err
from test_fused_epilogue_gpu import _arrays, _cheb_pair

pytestmark = pytest.mark.gpu
TOL = 1e-10
CYL672 = os.path.join(GOLDEN, "mesh_cylinder8_672e_4ss_us.npz")

MESHES = {   # the smallest problems at which each kernel shape is still exercised
    "cyl p3 fs": (lambda: hollow_cylinder_mesh(2, 6, 2), 3, "hyperFS", [998]),                      # swept; Q = 4, four per group; levels 1, 2, 3
    "box p4 fs": (lambda: nb.distorted_box(3, 2, 3, seed=2, amp=0.2), 4, "hyperFS", [1]),          # general; Q = 5, two per group; 27 interior nodes
    "box p1 le": (lambda: nb.distorted_box(5, 3, 1, seed=5), 1, "linElas", [1]),                   # Q = 2, eight per group, ragged; no interior nodes
    "box p6 fs": (lambda: box_mesh(2, 2, 1), 6, "hyperFS", [1]),                                   # Q = 7, one per group; derived state; 125 interior
    "cyl672 p2 ss": (lambda: load_mesh_npz(CYL672), 2, "hyperSS", [998, 999]),                     # unstructured: rows of 3 and 6 contributors
}
WRAPPED = {
    "wrap 1x3x2 p3 fs": (lambda: box_mesh(1, 3, 2), 3, "hyperFS", [1]),      # a node twice inside an element
    "wrap 2x2x2 p2 ss": (lambda: box_mesh(2, 2, 2), 2, "hyperSS", [1]),      # shared with a non-neighbour in element order
}
_cache = {}


def _own_pass(p):
    return len(p.levels) > 1 and p.info["state"]


def _all_outputs(monkeypatch, numbering, ceed, case, u_def=None):
    """run_operators of the case under the numbering on `ceed`, every level on the fine quadrature; then, where there is a ladder with a
    stored state, once more under coarse_quadrature="own" (residual with refresh_level_state, the levels' states, Jacobian, diagonal).
    Returns (default-numbered smooth state, outputs, names, dofmaps)."""
    mk, degree, model, bc = MESHES[case]
    mesh = mk()
    p = nb.problem_under(monkeypatch, numbering, ceed, mesh, degree, model, bc)
    dms = [lv.dofmap for lv in p.levels]
    if u_def is None:
        u_def = nb.to_default(p.smooth_state(0.1), dms[-1])
    u = nb.from_default(u_def, dms[-1], nb.UNREAD)
    out, names = nb.run_operators(p, u)
    own = _own_pass(p)
    p.destroy()
    if own:
        p = nb.problem_under(monkeypatch, numbering, ceed, mesh, degree, model, bc, coarse_quadrature="own")
        o2, n2 = nb.run_operators(p, u, seed=43, pointblock=False, transfers=False)
        out.update({"own " + k: v for k, v in o2.items()}); names.update({"own " + k: v for k, v in n2.items()})
        p.destroy()
    return u_def, out, names, dms


def _default_device(monkeypatch, gpu, case):
    """The device under the default numbering: once per case, shared read-only by the case's numberings."""
    if case not in _cache:
        _cache[case] = _all_outputs(monkeypatch, nb.default, gpu, case)
    return _cache[case]


@pytest.mark.parametrize("numbering", list(nb.NUMBERINGS))
@pytest.mark.parametrize("case", list(MESHES))
def test_every_operator_under_the_numbering(monkeypatch, oracle, gpu, case, numbering):
    """(a) Residual, stored grad u (q-point data, compared unmapped), Jacobian action into an output preset to 3.0, CeedOperatorApplyAdd,
    get_diag, get_pointblock_diag, prolong / prolong_add / restrict on every level (pair), and the states refresh_level_state writes
    under coarse_quadrature="own".  Device under the numbering vs the oracle under the numbering < 1e-10; vs the device under the default
    numbering mapped back: np.array_equal, no exception; entries no element holds (`gaps`) exactly 0 after an overwriting call and
    exactly untouched after an adding one; the kernels and launch forms of the default numbering on every level."""
    t0 = time.perf_counter()
    u_def, want, want_names, _ = _default_device(monkeypatch, gpu, case)
    t1 = time.perf_counter()
    _, got, names, dms = _all_outputs(monkeypatch, nb.NUMBERINGS[numbering], gpu, case, u_def)
    t2 = time.perf_counter()
    _, orc, _, _ = _all_outputs(monkeypatch, nb.NUMBERINGS[numbering], oracle, case, u_def)
    t3 = time.perf_counter()
    assert set(got) == set(want) == set(orc)
    bad, worst, report = [], 0.0, []
    for name in got:
        g = got[name]
        err = rel_err(g, orc[name])
        worst = max(worst, err)
        if not err < TOL:
            bad.append(f"{name}: device vs oracle {err:.2e}")
        k, ncomp = nb.level_of(name)
        if k is None:
            same = np.array_equal(g, want[name])
        else:
            dm = dms[k]
            same = np.array_equal(nb.to_default(g, dm), want[name])
            stray = g[~nb.referenced(dm, ncomp)]
            keep = nb.KEPT if "_add" in name else 0.0
            if not np.all(stray == keep):
                bad.append(f"{name}: {np.count_nonzero(stray != keep)} of {stray.size} entries no element holds are not {keep}")
        report.append(f"{name}={'yes' if same else 'NO'}")
        if not same:
            d = g - want[name] if k is None else nb.to_default(g, dms[k]) - want[name]
            bad.append(f"{name}: not bitwise the default numbering's (max abs diff {np.abs(d).max():.2e}, {np.count_nonzero(d)} entries)")
    for key, val in names.items():
        if val != want_names[key]:
            bad.append(f"{key}: ran {val}, the default numbering {want_names[key]}")
        if "launch" in key:
            assert val["segments"] == 1 and val["streams"] == 1, (key, val)       # meshes this small take the serial form
    if numbering == "gaps":
        assert not all(nb.referenced(dm).all() for dm in dms)
    print(f"NUMBERING (a) {numbering:12s} {case:13s} worst rel_err vs oracle {worst:.2e}; bitwise vs default: {' '.join(report)}; "
          f"seconds: default device {t1 - t0:.3f} (shared) device {t2 - t1:.3f} oracle {t3 - t2:.3f} test {time.perf_counter() - t0:.3f}")
    assert not bad, "\n".join(bad)
    assert np.abs(got["residual"]).max() > 0 and np.abs(got["jacobian0"]).max() > 0


def _wrapped_outputs(monkeypatch, ceed, case):
    """Under `wrapped` on `ceed`: check_wrapped's outputs (and its symmetry / adjointness assertions), then run_operators with the
    inputs drawn in the wrapped numbering itself, then its coarse_quadrature="own" pass as in _all_outputs."""
    mk, degree, model, bc = WRAPPED[case]
    mesh = mk()
    p = nb.problem_under(monkeypatch, nb.wrapped, ceed, mesh, degree, model, bc)
    if case.startswith("wrap 1x"):
        for lv in p.levels:
            assert lv.dofmap.elem_nodes[0, 0] == lv.dofmap.elem_nodes[0, lv.degree]       # the case still repeats a node in an element
    assert p.levels[p.fine].mask.any() and all(nb.referenced(lv.dofmap).all() for lv in p.levels)
    out = {"properties " + k: v for k, v in nb.check_wrapped(p).items()}
    u = nb.wrapped_state(p)
    o, names = nb.run_operators(p, u, own_numbering=True)
    out.update(o)
    assert _own_pass(p)
    p.destroy()
    p = nb.problem_under(monkeypatch, nb.wrapped, ceed, mesh, degree, model, bc, coarse_quadrature="own")
    o2, n2 = nb.run_operators(p, u, seed=43, pointblock=False, transfers=False, own_numbering=True)
    out.update({"own " + k: v for k, v in o2.items()}); names.update({"own " + k: v for k, v in n2.items()})
    p.destroy()
    return out, names


@pytest.mark.parametrize("case", list(WRAPPED))
def test_every_operator_under_the_wrapped_numbering(monkeypatch, oracle, gpu, case):
    """(a) for `wrapped`: the whole output list of test_every_operator_under_the_numbering -- residual, stored grad u, Jacobian action,
    CeedOperatorApplyAdd, get_diag, get_pointblock_diag, prolong / prolong_add / restrict, and the pass under coarse_quadrature="own"
    with the states refresh_level_state writes -- device against the oracle under the same numbering < 1e-10, inputs drawn in the
    wrapped numbering.  It has no default-numbering twin, so in place of the bitwise comparison: on the device itself the symmetry of
    the tangent (1e-11) and restrict = prolong^T (1e-12), the bounds of _numbering.check_wrapped -- rounding bounds of dot products
    that add in different orders, as in tests/test_gpu_parity.py.  With one element in x a row has two E-vector contributors from ONE
    element, own_f one owner entry among two candidates of one element, and the state refresh gathers one node twice.
    get_diag and get_pointblock_diag are, on both backends, libCEED's: the diagonal (blocks) of each ELEMENT matrix summed over the
    element entries of a node.  For a node held twice by one element that leaves out the coupling between its two entries, which the
    assembled operator's diagonal has; tests/test_numbering.py shows the size of that on the oracle.  Device and oracle agree."""
    t0 = time.perf_counter()
    got, names = _wrapped_outputs(monkeypatch, gpu, case)
    orc, _ = _wrapped_outputs(monkeypatch, oracle, case)
    assert set(got) == set(orc)
    worst, bad = {}, []
    for name in got:
        err = rel_err(got[name], orc[name])
        kind = name.rstrip("0123456789vw")
        worst[kind] = max(worst.get(kind, 0.0), err)
        if not err < TOL:
            bad.append(f"{name}: device vs oracle {err:.2e}")
    for key, val in names.items():
        if "launch" in key:
            assert val["segments"] == 1 and val["streams"] == 1, (key, val)
    print(f"NUMBERING (a) wrapped      {case:17s} worst rel_err vs oracle {max(worst.values()):.2e} over {len(got)} outputs "
          f"({' '.join(f'{k}:{v:.1e}' for k, v in worst.items())}); seconds {time.perf_counter() - t0:.3f}")
    assert not bad, "\n".join(bad)
    assert np.abs(got["pointblock0"]).max() > 0 and np.abs(got["own gradu0"]).max() > 0


FUSED = {"cyl p3 fs": MESHES["cyl p3 fs"], "cyl672 p2 ss": MESHES["cyl672 p2 ss"]}


@pytest.mark.parametrize("numbering", ["permuted", "cells_first", "gaps"])
@pytest.mark.parametrize("case", list(FUSED))
def test_fused_epilogue_under_the_numbering(monkeypatch, product_lib, oracle, case, numbering):
    """(b) CeedXOperatorApplyChebyshev / ApplyResidual (tests/test_fused_epilogue_gpu.py) under a numbering: fused == two steps bitwise,
    and the oracle's restatement < 1e-10.  k_assemble_epi redistributes node_off with a shuffle and its interior workgroups walk
    int_off.  Under `gaps` the library declines to fuse (no full cover) and must return the two-step bits.  dinv, b, x, d and r are zero
    on entries no element holds (a smoother's vectors are) and x, d, r must stay zero there."""
    t0 = time.perf_counter()
    mk, degree, model, bc = FUSED[case]
    mesh = mk()
    gpu = ceed_with_env(product_lib, {"CEED_MI355X_ASSEMBLE": "serial"})
    p = nb.problem_under(monkeypatch, nb.NUMBERINGS[numbering], gpu, mesh, degree, model, bc)
    po = nb.problem_under(monkeypatch, nb.NUMBERINGS[numbering], oracle, mesh, degree, model, bc)
    n = p.lsize()
    u = p.smooth_state(0.08)
    for q in (p, po):
        q.form_residual(q.ceed.vector(n).set_array(u), q.ceed.vector(n))
    worst = 0.0
    for lv in range(len(p.levels)):
        held = nb.referenced(p.levels[lv].dofmap)
        assert held.all() == (numbering != "gaps")
        arrs = {k: v * held for k, v in _arrays(p, lv, 100 + lv).items()}
        for first in (False, True, "recomputed"):
            for in_place in (True, False):
                a, b = _cheb_pair(p, lv, arrs, first, in_place)
                for k in ("x", "d", "r"):
                    assert np.array_equal(a[k], b[k]), (lv, first, in_place, k, np.abs(a[k] - b[k]).max())
                    assert not b[k][~held].any(), (lv, first, in_place, k)
            oa, ob = _cheb_pair(po, lv, arrs, first)
            for k in ("x", "d", "r"):
                worst = max(worst, rel_err(b[k], ob[k]))
                assert np.array_equal(oa[k], ob[k]) and rel_err(b[k], ob[k]) < TOL, (lv, first, k, rel_err(b[k], ob[k]))
        assert p.levels[lv].opJacob.launch_info()["segments"] == 1
        c, L, op = p.ceed, p.ceed.L, p.levels[lv].opJacob
        nl = p.lsize(lv)
        X, B, T, W1, W2 = (c.vector(nl).set_array(arrs["x"]), c.vector(nl).set_array(arrs["b"]), c.vector(nl), c.vector(nl), c.vector(nl))
        op.apply(X, T)
        L.chk(L.lib.CeedXVectorWAXPBY(W1.h, C.c_double(1.0), B.h, C.c_double(-1.0), T.h))
        T.set_value(9.0)
        L.chk(L.lib.CeedXOperatorApplyResidual(op.h, X.h, T.h, B.h, W2.h))
        assert np.array_equal(W1.to_numpy(), W2.to_numpy()), lv
        assert not W2.to_numpy()[~held].any(), lv
    p.destroy(); po.destroy()
    print(f"NUMBERING (b) {numbering:12s} {case:13s} fused == two steps bitwise; worst rel_err vs oracle {worst:.2e}; seconds {time.perf_counter() - t0:.2f}")


@pytest.mark.parametrize("numbering", ["permuted", "reversed"])
@pytest.mark.parametrize("mk,degree,problem", [(lambda: nb.distorted_box(9, 7, 5), 1, "linElas"), (lambda: hollow_cylinder_mesh(4, 24, 16), 4, "hyperFS")],
                         ids=["box p1", "cyl1536 p4"])
def test_pipelined_assembly_equals_serial_under_the_numbering(monkeypatch, product_lib, mk, degree, problem, numbering):
    """(c) tests/test_gpu_parity.py::test_pipelined_assembly_equals_serial_assembly_bitwise, its body and its switches (three segments),
    under a numbering in which the rows of a segment are no contiguous range of offsets: bitwise over 12 alternating applies."""
    t0 = time.perf_counter()
    monkeypatch.setattr(solid, "build_dofmap", nb.NUMBERINGS[numbering])
    mesh = mk()
    parity.pipelined_assembly_equals_serial_assembly(product_lib, mesh, degree, problem)
    print(f"NUMBERING (c) {numbering:12s} {mesh.name} p{degree} {problem}: pipelined == serial bitwise, 3 segments; seconds {time.perf_counter() - t0:.3f}")


def test_split_phase_apply_under_a_permutation(monkeypatch, gpu):
    """(d) tests/test_gpu_parity.py::test_split_phase_apply_equals_full_apply, its body, under `permuted`: the priority rows come first in
    a map whose node offsets are scattered over the vector."""
    monkeypatch.setattr(solid, "build_dofmap", nb.NUMBERINGS["permuted"])
    t0 = time.perf_counter()
    parity.split_phase_equals_full_apply(gpu)
    print(f"NUMBERING (d) permuted     distorted_box(4,4,4) p3 hyperFS: phase 0 + phase 1 == whole apply bitwise; seconds {time.perf_counter() - t0:.3f}")


CLAMP = {998: dict(translate=(0.0, -0.05, 0.1)), 999: dict()}


def _solve(monkeypatch, gpu, numbering, snes_rtol):
    p = nb.problem_under(monkeypatch, numbering, gpu, hollow_cylinder_mesh(2, 8, 3), 2, "hyperSS", [998, 999])
    s = NewtonPMG(p, clamp=CLAMP, coarse="amg", graph=True, snes_rtol=snes_rtol)
    st = s.solve(2)
    u = nb.to_default(s.U.to_numpy(), p.levels[p.fine].dofmap)
    p.destroy()
    return st, u


@pytest.mark.parametrize("numbering", ["permuted", "cells_first"])
def test_one_whole_solve_under_the_numbering(monkeypatch, gpu, numbering):
    """(e) Newton with p-multigrid and the AMG coarse solve, recorded V-cycle, two load increments.  The operators are bitwise the default
    numbering's, but the dot products of the Krylov method add in another order and the AMG aggregates in another order, so the iterates
    differ in rounding: NOT bitwise.  As tests/test_pointblock_gpu.py::test_config3_solve_with_pbjacobi: the same Newton counts, and the
    displacement (mapped back) within 10 x what the Newton tolerance leaves open, which is the distance between two default-numbering
    solves at snes_rtol and snes_rtol / 10 (straddling_snes_rtol puts the pair where they stop at different iterates).  Krylov counts
    are printed, not asserted."""
    t0 = time.perf_counter()
    if "solve" not in _cache:
        rtol = straddling_snes_rtol(_solve(monkeypatch, gpu, nb.default, 1e-8)[0])
        _cache["solve"] = (rtol, _solve(monkeypatch, gpu, nb.default, rtol), _solve(monkeypatch, gpu, nb.default, rtol / 10))
    rtol, (st_d, u_d), (st_t, u_t) = _cache["solve"]
    st_n, u_n = _solve(monkeypatch, gpu, nb.NUMBERINGS[numbering], rtol)
    print(f"NUMBERING (e) {numbering:12s} snes_rtol {rtol:.2e}; Newton default {st_d.newton_its} (tight {st_t.newton_its}) numbered {st_n.newton_its}; "
          f"Krylov default {st_d.ksp_its} numbered {st_n.ksp_its}; |u_numbered - u_default| {np.linalg.norm(u_n - u_d):.3e} allowed "
          f"{10 * np.linalg.norm(u_d - u_t):.3e}; seconds {time.perf_counter() - t0:.2f}")
    assert st_d.converged and st_t.converged and st_n.converged and st_n.increments == 2
    assert st_t.newton_its > st_d.newton_its                       # the tolerance is what ends the solves
    assert st_n.newton_its == st_d.newton_its
    assert np.linalg.norm(u_n - u_d) <= 10.0 * np.linalg.norm(u_d - u_t)
