"""Every volume kernel under component-wise Dirichlet masks (three flag bits a node, one per COMPONENT).  The masks of
tests/_component_masks.py give every class of nodes -- (contributors, element-interior or not) -- all eight patterns on every level, so
every gather, store, row, block and transfer below meets flag values 1..6, not 0 and 7 alone.

Two references for every result:
  (a) the device against itself, NO tolerance: the masked operator gives the bits of the device's own UNMASKED operator (a second
      problem with all-zero masks) applied to np.where(mask_in, 0.0, x) and followed by np.where(mask_out, 0.0, y).  Masking is a
      select at every site, so np.array_equal holds for every family below; none is held at a tolerance instead.
  (b) the CPU oracle under the same masks (pinned to mask-free dense forms by tests/test_component_masks.py), at the bounds of
      test_kernel_matrix_gpu.py: TOL = 1e-10 in the 2-norm and the max norm, 1e-12 for a stored state.
And: masked rows == 0.0 after apply, masked rows keep the BITS of y after apply_add, and where the input is "read as zero" the result
has the same bits with NaN in the masked input entries (a kernel that multiplies by zero instead of selecting fails there).

Site -> test (all on the distorted 3 x 3 x 3 box unless noted; 27 elements: several groups per wave-round and a ragged last group, whose
dead elements take the flags 7u, at every P):
  fused gather (fl & 1u / 2u / 4u), all fused kernels      test_jacobian_in_modes_1_2_3, test_residual_and_stored_state (ladders below)
  k_fused_pencil_mass gather                                test_fused_mass_term
  fused store of element-interior nodes (ka->mask_out)      test_jacobian_in_modes_1_2_3 (class (1, True), levels with P >= 3), apply_add too
  k_assemble (flags[r])                                     test_jacobian_in_modes_1_2_3; test_row_flag_forms_and_epilogues (every map)
  k_assemble_epi                                            test_row_flag_forms_and_epilogues (Chebyshev first / next, residual)
  folded halo pack                                          test_folded_halo_pack_under_a_partial_mask (a rank of a partitioned cylinder)
  kernels_mass.hip (mask_in, mask_out)                      test_mass_operator
  kernels_state.hip (mask_in)                               test_state_kernel_of_own_quadrature_levels
  kernels_transfer.hip (mask_c, mask_f)                     test_transfers_with_independent_masks
  k_diag_sf (fl >> c)                                       test_diagonal
  k_pbdiag_sf (fl_in >> c, fl_out >> co)                    test_point_blocks_their_inverse_and_a_smoother_step
  k_pb_invert on ASSEMBLED blocks                           test_point_blocks_their_inverse_and_a_smoother_step

Ladders: hyperFS degree 4 (P = 2, 3, 5 at Q = 5), linElas degree 3 with qextra = 1 (P = 2, 3, 4 at Q = 5: P < Q), hyperSS degree 6
(P = 2, 3, 5, 7 at Q = 7; 20 577 dofs, the largest), and for the fused kernel's geometry form 3 (ug arrays re-ordered by geo_axis)
hollow_cylinder_mesh(2, 8, 3) with hyperFS at degree 2.  That mesh's classes: degree 1 -- (2, F) 32, (4, F) 48, (8, F) 16 nodes; degree 2
-- (1, F) 112, (1, T) 48, (2, F) 264, (4, F) 120, (8, F) 16: no class below eight nodes, each holds all eight patterns
(test_component_masks.py counts them).  The oracle's point blocks are 3 P^3 applies: compared where P <= 5, (a) holds at every P.

With CPS_COMPONENT_MASKS_REPORT=<file> the worst error per family against the oracle, the families that met (a) and the wall time of
the file are written there (profiles/component_masks.txt)."""
import os
import time

import numpy as np
import pytest

import _component_masks as cm
import _kernel_matrix as km
from _ceed_env import ceed_with_env
from _pointblock_common import embedded_inverse_stacked
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mass import MassOperator
from ceedpetscsolid_amd.mesh import hollow_cylinder_mesh
from test_assemble_coded_gpu import _priority, _results
from test_kernel_matrix_gpu import TOL, TOL_STATE, errors

pytestmark = pytest.mark.gpu

LADDERS = {      # name -> (mesh, degree, physics, keywords, geometry form the fused kernels must report)
    "hyperFS p4": (cm.MESH, 4, "hyperFS", {}, 1),
    "linElas p3 qextra 1": (cm.MESH, 3, "linElas", dict(qextra=1), 1),
    "hyperSS p6": (cm.MESH, 6, "hyperSS", {}, 1),
    "cylinder hyperFS p2": (lambda: hollow_cylinder_mesh(2, 8, 3), 2, "hyperFS", {}, 3),
}
NAN = float("nan")


class Record:
    def __init__(self):
        self.worst, self.bits, self.t0 = {}, {}, time.time()

    def write(self, path):
        with open(path, "w") as f:
            f.write(f"component masks on the device: {time.time() - self.t0:.1f} s from the first test of the file to the last\n")
            f.write("worst error against the oracle under the same masks, relative, 2-norm | max norm:\n")
            for fam, (e2, einf) in sorted(self.worst.items()):
                f.write(f"  {fam:28s} {e2:.2e} | {einf:.2e}\n")
            f.write("bitwise check (a), the masked operator against the device's own unmasked one -- comparisons met / made:\n")
            for fam, (ok, n) in sorted(self.bits.items()):
                f.write(f"  {fam:28s} {ok} / {n}\n")


RECORD = Record()


@pytest.fixture(scope="module", autouse=True)
def report():
    RECORD.t0 = time.time()
    yield
    path = os.environ.get("CPS_COMPONENT_MASKS_REPORT")
    if path:
        RECORD.write(path)


def hold(family, what, got, want, tol2=TOL, tolinf=TOL):
    e2, einf = errors(got, want)
    w = RECORD.worst.setdefault(family, [0.0, 0.0])
    w[0], w[1] = max(w[0], e2), max(w[1], einf)
    print(f"  {family} {what}: {e2:.2e} | {einf:.2e}")
    assert e2 <= tol2 and einf <= tolinf, (family, what, e2, einf)


def same_bits(family, what, got, want):
    ok = np.array_equal(got, want, equal_nan=False)
    b = RECORD.bits.setdefault(family, [0, 0])
    b[0] += int(ok); b[1] += 1
    assert ok, (family, what, int((got != want).sum()), float(np.nanmax(np.abs(got - want))))


def run(c, fn, x, n_out, y0=None):
    """fn(X, Y) on a Ceed's vectors: X = x, Y preset to -7 (or to y0: an adding call)."""
    X = c.vector(x.size).set_array(x)
    Y = c.vector(n_out).set_value(-7.0) if y0 is None else c.vector(n_out).set_array(y0)
    fn(X, Y)
    y = Y.to_numpy()
    X.destroy(); Y.destroy()
    return y


def check_linear(family, what, c, o, masked, unmasked, oracle_op, m_in, m_out, mode, n_in, n_out, rng, add=None):
    """One masked linear operator on the device `c` -- masked(X, Y), add(X, Y) -- against (a) unmasked(X, Y) of the same device between
    two selects and (b) oracle_op(X, Y) on the oracle `o` under the same masks; zero rows, kept rows, NaN in the masked input."""
    x, y0 = rng.uniform(-1, 1, n_in), rng.uniform(-1, 1, n_out)
    got = run(c, masked, x, n_out)
    want = run(c, unmasked, cm.keep(m_in, x) if mode & 1 else x, n_out)
    same_bits(family, what, got, cm.keep(m_out, want) if mode & 2 else want)
    yo = run(o, oracle_op, x, n_out)
    hold(family, what, got, yo)
    if mode & 2:
        assert np.all(got[m_out != 0] == 0.0), (family, what, "masked rows after apply")
    xn = np.where(m_in != 0, NAN, x)
    if mode & 1:
        assert np.isnan(xn).any()
        same_bits(family, what + ", NaN in the masked input", run(c, masked, xn, n_out), got)
    if add is not None:
        ya = run(c, add, x, n_out, y0)
        hold(family, what + " add", ya, y0 + yo)
        if mode & 2:
            assert np.array_equal(ya[m_out != 0], y0[m_out != 0]), (family, what, "masked rows after apply_add")
        if mode & 1:
            same_bits(family, what + " add, NaN in the masked input", run(c, add, xn, n_out, y0), ya)


# --------------------------------------------------------------------------------------------------------------------------------
# the ladders: oracle and device under the same masks, the device once more without any
# --------------------------------------------------------------------------------------------------------------------------------
class Ladder:
    def __init__(self, oracle, gpu, name, **kw):
        mk, degree, physics, more, self.geo = LADDERS[name]
        self.name, self.physics, self.c, self.oc = name, physics, gpu, oracle
        kw = dict(more, **kw)
        self.o, self.u, self.m = (cm.unmasked(c, mk(), degree, physics, **kw) for c in (oracle, gpu, gpu))
        self.masks = cm.install(self.m)
        assert all(np.array_equal(a, b) for a, b in zip(cm.install(self.o), self.masks))
        self.Q, self.nlev = self.m.Q, len(self.m.levels)
        self.rng = np.random.default_rng(17)
        n = self.m.lsize()
        self.disp = self.m.smooth_state(0.1)
        self.residual = {}
        for key, p in (("o", self.o), ("u", self.u), ("m", self.m)):          # stores the state every Jacobian below reads
            self.residual[key] = run(p.ceed, p.form_residual, self.disp, n)

    def destroy(self):
        for p in (self.o, self.u, self.m):
            p.destroy()


@pytest.fixture(scope="module")
def ladders(oracle, gpu):
    """name -> Ladder, each built at its first use, once, and destroyed with the module"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = Ladder(oracle, gpu, name)
        return made[name]
    yield get
    for ld in made.values():
        ld.destroy()


@pytest.fixture
def ladder(ladders, name):
    return ladders(name)


every_ladder = pytest.mark.parametrize("name", list(LADDERS))
mass_ladders = pytest.mark.parametrize("name", ["hyperFS p4", "linElas p3 qextra 1"])      # P = Q and P < Q at Q = 5: the mass kernels read w det J alone


@every_ladder
def test_residual_and_stored_state(ladder):
    """Mode 2: the boundary values are read as they are, the masked rows dropped; the state is the unmasked one's."""
    ld, m = ladder, ladder.masks[-1]
    P = ld.m.levels[-1].degree + 1
    assert ld.m.opApply.kernel_name == km.fused_name(P, ld.Q, km.PHYSICS[ld.physics][0], ld.geo), ld.m.opApply.kernel_name
    same_bits("fused residual", ld.name, ld.residual["m"], cm.keep(m, ld.residual["u"]))
    assert np.all(ld.residual["u"] != 0.0) and np.all(ld.residual["m"][m != 0] == 0.0)
    hold("fused residual", ld.name, ld.residual["m"], ld.residual["o"])
    if ld.m.gradu is not None:
        same_bits("fused state", ld.name, ld.m.gradu.to_numpy(), ld.u.gradu.to_numpy())
        hold("fused state", ld.name, ld.m.gradu.to_numpy(), ld.o.gradu.to_numpy(), TOL_STATE)
    y0 = ld.rng.uniform(-1, 1, m.size)
    ya = run(ld.c, ld.m.opApply.apply_add, ld.disp, m.size, y0)
    assert np.array_equal(ya[m != 0], y0[m != 0])
    hold("fused residual", ld.name + " add", ya, y0 + ld.residual["o"])


@every_ladder
def test_jacobian_in_modes_1_2_3(ladder):
    ld = ladder
    jac = km.PHYSICS[ld.physics][1] + ("+derived" if ld.physics == "hyperFS" and km.derived_state(ld.Q) else "")
    for k in range(ld.nlev):
        m, n = ld.masks[k], ld.m.lsize(k)
        opm, opu, opo = (p.levels[k].opJacob for p in (ld.m, ld.u, ld.o))
        try:
            for mode in (1, 2, 3):
                for op in (opm, opo):
                    op.set_dirichlet_mask_mode(m, None, mode)
                check_linear("fused jacobian", f"{ld.name} level {k} mode {mode}", ld.c, ld.oc, opm.apply, opu.apply, opo.apply,
                             m, m, mode, n, n, ld.rng, add=opm.apply_add)
                assert opm.kernel_name == km.fused_name(ld.m.levels[k].degree + 1, ld.Q, jac, ld.geo), opm.kernel_name
        finally:                                   # the ladder is shared: a failure here leaves the later tests the mode they expect
            for op in (opm, opo):
                op.set_dirichlet_mask_mode(m, None, 3)


@every_ladder
def test_diagonal(ladder):
    ld = ladder
    for k in range(ld.nlev):
        m, n = ld.masks[k], ld.m.lsize(k)
        d = {key: run(p.ceed, lambda X, Y: p.get_diag(k, Y), np.zeros(1), n) for key, p in (("o", ld.o), ("u", ld.u), ("m", ld.m))}
        same_bits("diag", f"{ld.name} level {k}", d["m"], cm.keep(m, d["u"]))
        hold("diag", f"{ld.name} level {k}", d["m"], d["o"])
        assert np.all(d["u"] != 0.0) and np.all(d["m"][m != 0] == 0.0)


@every_ladder
def test_point_blocks_their_inverse_and_a_smoother_step(ladder):
    ld = ladder
    for k in range(ld.nlev):
        m, n = ld.masks[k], ld.m.lsize(k)
        bu, bm = (run(p.ceed, lambda X, Y: p.get_pointblock_diag(k, Y), np.zeros(1), 3 * n).reshape(-1, 3, 3) for p in (ld.u, ld.m))
        mn = m.reshape(-1, 3) != 0
        dropped = mn[:, :, None] | mn[:, None, :]                              # [node][row][column]
        same_bits("point blocks", f"{ld.name} level {k}", bm, np.where(dropped, 0.0, bu))
        assert np.all(bm[dropped] == 0.0) and np.all(np.einsum("nii->ni", bu) > 0.0)
        if ld.m.levels[k].degree + 1 <= 5:
            bo = run(ld.oc, lambda X, Y: ld.o.get_pointblock_diag(k, Y), np.zeros(1), 3 * n).reshape(-1, 3, 3)
            hold("point blocks", f"{ld.name} level {k}", bm.ravel(), bo.ravel())
            assert np.all(bo[dropped] == 0.0)
        # the inverse of the kept principal sub-block of the ASSEMBLED blocks, every pattern: against NumPy's
        s = np.einsum("nii->ni", bm).max(axis=1)
        kept = np.where(dropped, np.eye(3) * (s + (s == 0.0))[:, None, None], bm)      # a dropped component at the block's own scale
        assert np.linalg.cond(kept).max() <= 100.0                             # the conditioning the 1e-13 of test_pointblock_gpu.py is stated for
        want = embedded_inverse_stacked(bm)
        V = ld.c.vector(9 * (n // 3)).set_array(bm.ravel())
        assert cd.pointblock_invert(V) == 0
        got = V.to_numpy().reshape(-1, 3, 3)
        scale = np.abs(want).max(axis=(1, 2), keepdims=True)
        err = (np.abs(got - want) / (scale + (scale == 0.0))).max()
        w = RECORD.worst.setdefault("point-block inverse", [0.0, 0.0])
        w[1] = max(w[1], err)
        print(f"  point-block inverse {ld.name} level {k}: {err:.2e}")
        assert err <= 1e-13 and np.all(got[dropped] == 0.0)
        # one point-block Chebyshev step with them: d = c1 B^-1 (b - t) + c2 d, x += d
        a = {key: ld.rng.uniform(-1, 1, n) for key in ("x", "d", "b", "t")}
        v = {key: ld.c.vector(n).set_array(arr) for key, arr in a.items()}
        cd.chebyshev_step_pointblock(v["x"], v["d"], None, v["b"], v["t"], V, 0.4, 0.3, False)
        dn = 0.4 * np.einsum("nij,nj->ni", want, (a["b"] - a["t"]).reshape(-1, 3)).reshape(-1) + 0.3 * a["d"]
        serr = max(np.abs(v["d"].to_numpy() - dn).max(), np.abs(v["x"].to_numpy() - (a["x"] + dn)).max()) / np.abs(a["x"] + dn).max()
        w = RECORD.worst.setdefault("point-block step", [0.0, 0.0])
        w[1] = max(w[1], serr)
        assert serr <= 1e-13, serr
        assert np.array_equal(v["d"].to_numpy()[m != 0], 0.3 * a["d"][m != 0])    # a dropped component gets nothing from the blocks
        for o in list(v.values()) + [V]:
            o.destroy()


@every_ladder
def test_transfers_with_independent_masks(ladder):
    ld = ladder
    for k in range(1, ld.nlev):
        nf, nc, mf, mc = ld.m.lsize(k), ld.m.lsize(k - 1), ld.masks[k], ld.masks[k - 1]
        assert not np.array_equal(mf.reshape(-1, 3)[:8], mc.reshape(-1, 3)[:8])
        lm, lu, lo = (p.levels[k] for p in (ld.m, ld.u, ld.o))
        check_linear("transfer", f"{ld.name} prolong to level {k}", ld.c, ld.oc, lm.opProlong.apply, lu.opProlong.apply, lo.opProlong.apply,
                     mc, mf, 3, nc, nf, ld.rng, add=lm.opProlong.apply_add)
        check_linear("transfer", f"{ld.name} restrict from level {k}", ld.c, ld.oc, lm.opRestrict.apply, lu.opRestrict.apply, lo.opRestrict.apply,
                     mf, mc, 3, nf, nc, ld.rng)
        x, y = ld.rng.uniform(-1, 1, nf), ld.rng.uniform(-1, 1, nc)            # <R x, y> = <x, P y> with both masks in force
        lhs, rhs = float(run(ld.c, lm.opRestrict.apply, x, nc) @ y), float(x @ run(ld.c, lm.opProlong.apply, y, nf))
        assert abs(lhs - rhs) <= 1e-13 * max(abs(lhs), abs(rhs), 1.0), (k, lhs, rhs)


@mass_ladders
@pytest.mark.parametrize("mask_mode", [2, 3])
def test_mass_operator(ladder, mask_mode):
    ld = ladder
    for k in range(ld.nlev):
        m, n = ld.masks[k], ld.m.lsize(k)
        mm, mu, mo = MassOperator(ld.m, k, 1.5, mask_mode=mask_mode), MassOperator(ld.u, k, 1.5), MassOperator(ld.o, k, 1.5, mask_mode=mask_mode)
        assert not mm.portable and mo.mask is not None and np.array_equal(mo.mask, m != 0)
        check_linear("mass", f"{ld.name} level {k} mask_mode {mask_mode}", ld.c, ld.oc, mm.apply, mu.apply, mo.apply, m, m, mask_mode, n, n, ld.rng,
                     add=mm.apply_add)
        for what, fn in (("diagonal", "diagonal"), ("lumped", "lumped")):
            d = {key: run(op.ceed, lambda X, Y: getattr(op, fn)(Y), np.zeros(1), n) for key, op in (("o", mo), ("u", mu), ("m", mm))}
            same_bits("mass", f"{ld.name} level {k} {what}", d["m"], cm.keep(m, d["u"]))
            hold("mass", f"{ld.name} level {k} {what}", d["m"], d["o"])
            assert np.all(d["m"][m != 0] == 0.0) and np.all(d["u"] > 0.0)
        for op in (mm, mu, mo):
            op.destroy()


@mass_ladders
def test_fused_mass_term(ladder):
    """set_mass_term: (K + c M) x in the launches of K (k_fused_pencil_mass) -- a level with P = Q (hyperFS p4, fine) and levels with
    P < Q.  The oracle's K x plus the portable mass operator on the masked input, masked rows dropped."""
    ld, c = ladder, 1.75
    for k in range(ld.nlev):
        m, n = ld.masks[k], ld.m.lsize(k)
        opm, opu, opo = (p.levels[k].opJacob for p in (ld.m, ld.u, ld.o))
        assert opm.mass_term_available()
        ref = MassOperator(ld.o, k, c, portable=True)
        oracle_op = lambda X, Y: (opo.apply(X, Y), Y.set_array(Y.to_numpy() + cm.keep(m, ref.apply_host(X.to_numpy()))))
        for op in (opm, opu):
            op.set_mass_term(c)
        try:
            check_linear("fused mass term", f"{ld.name} level {k}", ld.c, ld.oc, opm.apply, opu.apply, oracle_op, m, m, 3, n, n, ld.rng, add=opm.apply_add)
            assert "+mass" in opm.kernel_name, opm.kernel_name
        finally:
            for op in (opm, opu):
                op.set_mass_term(0.0)
            ref.destroy()


# --------------------------------------------------------------------------------------------------------------------------------
# the state kernel of own-quadrature levels
# --------------------------------------------------------------------------------------------------------------------------------
def test_state_kernel_of_own_quadrature_levels(oracle, gpu):
    """coarse_quadrature="own", hyperFS degree 4: the coarse levels' stored state from a partially masked fine displacement.  Mode 2 (what
    SolidProblem sets: boundary values are read as they are): the unmasked state's bits.  Mode 3 on the same operator, which reaches the
    kernel's decode of the flags: the bits of the unmasked operator on the selected displacement."""
    ld = Ladder(oracle, gpu, "hyperFS p4", coarse_quadrature="own")
    n, m = ld.m.lsize(), ld.masks[-1]
    X = {key: p.ceed.vector(n).set_array(ld.disp) for key, p in (("o", ld.o), ("u", ld.u), ("m", ld.m))}
    Xsel = ld.c.vector(n).set_array(cm.keep(m, ld.disp))
    Xnan = ld.c.vector(n).set_array(np.where(m != 0, NAN, ld.disp))
    seen = 0
    for k in range(ld.nlev - 1):
        lm, lu, lo = (p.levels[k] for p in (ld.m, ld.u, ld.o))
        assert lm.own_quadrature and lm.opState is not None
        seen += 1
        what = f"level {k} state<Pf=5,Qc={lm.Q}>"
        same_bits("state", what + " mode 2", lm.gradu.to_numpy(), lu.gradu.to_numpy())          # as form_residual left them
        hold("state", what + " mode 2", lm.gradu.to_numpy(), lo.gradu.to_numpy(), TOL_STATE)
        assert lm.opState.kernel_name == f"state<Pf=5,Qc={lm.Q}>", lm.opState.kernel_name
        for op in (lm.opState, lo.opState):
            op.set_dirichlet_mask_mode(m, None, 3)
        lm.opState.apply_state(X["m"])
        got = lm.gradu.to_numpy()
        lu.opState.apply_state(Xsel)
        same_bits("state", what + " mode 3", got, lu.gradu.to_numpy())
        scratch = ld.oc.vector(n)
        lo.opState.apply(X["o"], scratch)
        hold("state", what + " mode 3", got, lo.gradu.to_numpy(), TOL_STATE)
        lm.gradu.set_value(-7.0)
        lm.opState.apply_state(Xnan)
        same_bits("state", what + " mode 3, NaN in the masked input", lm.gradu.to_numpy(), got)
        scratch.destroy()
    assert seen == 2
    for v in list(X.values()) + [Xsel, Xnan]:
        v.destroy()
    ld.destroy()


# --------------------------------------------------------------------------------------------------------------------------------
# the row-flag forms of the shared-node sum and its epilogues
# --------------------------------------------------------------------------------------------------------------------------------
ROW_FORMS = {      # test_row_flags_gpu.FORMS (the split map is a part of every form's results) and the plain row map
    "shell map": {},
    "whole restriction map": {"CEED_MI355X_DIRECT": "0"},
    "pipelined": {"CEED_MI355X_PIPE_MIN_ROUNDS": "0", "CEED_MI355X_PIPE_SEGMENTS": "2"},
    "plain row map": {"CEED_MI355X_ROWMAP": "plain"},
}
NLEAD = 9


def form_results(ceed, masked):
    """Every form of the Jacobian apply that sums shared nodes (test_assemble_coded_gpu._results: apply, apply_add, Chebyshev first /
    next step and residual, fused and as two passes, the split pair; dinv zero on masked dofs), hyperFS degree 2 on the box."""
    p = cm.unmasked(ceed, cm.MESH(), 2, "hyperFS", multigrid="none")
    if masked:
        cm.install(p, shifts=[2])
    run(ceed, p.form_residual, p.smooth_state(0.08), p.lsize())
    out = _results(p, split=(NLEAD, _priority(p, NLEAD)))
    run(ceed, p.levels[p.fine].opJacob.apply, np.ones(p.lsize()), p.lsize())          # launch_info speaks of the last apply: a whole one
    out["segments"] = p.levels[p.fine].opJacob.launch_info()["segments"]
    mask = p.levels[p.fine].mask.copy()
    p.destroy()
    return out, mask


@pytest.fixture(scope="module")
def default_form(oracle, gpu):
    """The default form's results under the component mask; its plain apply held against the unmasked device and the oracle."""
    out, m = form_results(gpu, True)
    n = m.size
    rng = np.random.default_rng(11)
    x, y0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)                        # the first two draws of _results
    po = cm.unmasked(oracle, cm.MESH(), 2, "hyperFS", multigrid="none")
    cm.install(po, shifts=[2])
    run(oracle, po.form_residual, po.smooth_state(0.08), n)
    yo = run(oracle, po.levels[po.fine].opJacob.apply, x, n)
    pu = cm.unmasked(gpu, cm.MESH(), 2, "hyperFS", multigrid="none")
    run(gpu, pu.form_residual, pu.smooth_state(0.08), n)
    want = cm.keep(m, run(gpu, pu.levels[pu.fine].opJacob.apply, cm.keep(m, x), n))
    po.destroy(); pu.destroy()
    same_bits("row-flag forms", "default form against the unmasked device", out["apply, flags"], want)
    hold("row-flag forms", "default form", out["apply, flags"], yo)
    assert np.all(out["apply, flags"][m != 0] == 0.0)
    assert np.array_equal(out["apply add, flags"][m != 0], y0[m != 0])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out, m


@pytest.mark.parametrize("form", list(ROW_FORMS))
def test_row_flag_forms_and_epilogues(product_lib, default_form, form):
    ref, m = default_form
    ceed = ceed_with_env(product_lib, ROW_FORMS[form])
    out, m2 = form_results(ceed, True)
    ceed.destroy()
    assert np.array_equal(m, m2) and out.keys() == ref.keys()
    assert out["segments"] == (2 if form == "pipelined" else 1), out["segments"]
    for k in ref:
        if k == "segments":
            continue
        assert np.isfinite(out[k]).all() and np.abs(out[k]).max() > 0, k
        same_bits("row-flag forms", f"{form}: {k}", out[k], ref[k])
        if ", fused" in k:
            same_bits("epilogues", f"{form}: {k} against two passes", out[k], out[k.replace(", fused", ", two passes")])
    same_bits("row-flag forms", f"{form}: split phases 0 + 1", out["split phases 0 + 1"], out["apply, flags"])
    masked = m != 0
    assert np.all(out["chebyshev first d, fused, flags"][masked] == 0.0)                 # dinv is zero there: d = c1 dinv r
    assert np.all(out["apply, no flags"][masked] != 0.0)                                 # the flags, nothing else, zero the rows above


# --------------------------------------------------------------------------------------------------------------------------------
# the folded halo pack
# --------------------------------------------------------------------------------------------------------------------------------
def test_folded_halo_pack_under_a_partial_mask(product_lib):
    """One emulated rank (RcclHalo(..., emulate_self=True)) of the smallest partition test_gpu_parity.py uses -- rank 1 of 4 of a
    12 x 8 cylinder, hyperFS degree 2 -- with node n of the sub-mesh carrying pattern n % 8 (a partition is no box: the class condition
    is the box's; here every pattern lies on interface rows, asserted).  The one call, phase 0 / start / phase 1 / finish and
    apply-then-exchange give equal bits, and those of NumPy's y[idx] += y[idx] on the masked local result."""
    from ceedpetscsolid_amd.halo import HaloExchange, RcclHalo, interface_elements, part_cylinder, virtual_world
    from ceedpetscsolid_amd.mesh import reorder_elements_first
    ceed = ceed_with_env(product_lib, {})
    part = lambda r: part_cylinder(r, 4, 3, 12, 8)
    mesh = part(1)
    vw = virtual_world(1, 4, mesh, part, 2)
    lead = interface_elements(mesh, virtual=vw)
    mesh = reorder_elements_first(mesh, lead)
    p = cm.unmasked(ceed, mesh, 2, "hyperFS", multigrid="none")
    dm = p.levels[p.fine].dofmap
    halo = HaloExchange(mesh, dm, device="cuda", virtual=vw)
    ch = RcclHalo(ceed, halo, emulate_self=True)
    n = p.lsize()
    pat = np.arange(dm.nnodes) % 8
    m = ((pat[:, None] >> np.arange(3)[None, :]) & 1).astype(np.uint8).ravel()
    lists = [nb.dof_idx.cpu().numpy() for nb in halo.neigh]
    on_interface = np.unique(np.concatenate(lists) // 3)
    assert set(pat[on_interface].tolist()) == set(range(8)) and len(lists) >= 1
    run(ceed, p.form_residual, p.smooth_state(0.05), n)
    op = p.levels[p.fine].opJacob
    op.set_dirichlet_mask_mode(m, None, 3)
    x = np.random.default_rng(5).uniform(-1, 1, n)
    local = run(ceed, op.apply, x, n)
    want = local.copy()
    for idx in lists:
        want[idx] += local[idx]
    op.set_overlap_split(int(lead.sum()), halo.interface_dof_mask())
    ya = run(ceed, lambda X, Y: op.apply_with_halo(X, Y, ch), x, n)
    yb = run(ceed, lambda X, Y: (op.apply_phase(X, Y, 0), ch.start(Y), op.apply_phase(X, Y, 1), ch.finish(Y)), x, n)
    yc = run(ceed, lambda X, Y: (op.apply(X, Y), ch.add(Y)), x, n)
    yn = run(ceed, lambda X, Y: op.apply_with_halo(X, Y, ch), np.where(m != 0, NAN, x), n)
    for what, y in (("one call", ya), ("phases", yb), ("apply, then exchange", yc), ("one call, NaN in the masked input", yn)):
        same_bits("folded halo pack", what, y, want)
    assert np.all(ya[m != 0] == 0.0) and np.abs(ya[np.concatenate(lists)]).max() > 0
    ch.destroy(); p.destroy(); ceed.destroy()
