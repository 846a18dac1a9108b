"""The mass term of the Jacobian operators on the device (CeedXOperatorSetMassTerm: K + c M in the launches of K; k_fused_pencil_mass,
csrc/kernel_fused_pencil.hpp and its body file).

Yardsticks of the apply: the two-pass form on the device (the Jacobian apply, then mass.MassOperator in add mode with mask mode 3) and
the oracle's Jacobian apply plus MassOperator(portable=True).apply_host.  Bound: 1e-10 of max |y|, the project's operator bound.  The
coefficients are 1e-3, 1.75 and 1e6 times E: with the largest the mass term dominates, so a wrong weight or a wrong point index cannot
hide under K x.  Every shipped (P, Q) up to Q = 7 is a level of one of the uniform ladders built here (P = 2 .. Q at the fine
quadrature); every geometry form of the kernel has a mesh (general, affine, swept, and a qdata vector written over: qdata read); one
and two elements are a launch of one partial group up to Q = 5."""
import ctypes as C

import numpy as np
import pytest

import _kernel_matrix as km
import _numbering as nb
from _ceed_env import ceed_with_env
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mass import MassOperator
from ceedpetscsolid_amd.mesh import box_mesh, hollow_cylinder_mesh
from ceedpetscsolid_amd.solid import SolidProblem
from test_fused_epilogue_gpu import _arrays
from test_gpu_parity import distorted_box

pytestmark = pytest.mark.gpu

TOL = 1e-10                      # of max |y|
E_MOD, NU = 2.0, 0.3
COEFS = [1e-3 * E_MOD, 1.75 * E_MOD, 1e6 * E_MOD]
SHEAR = np.array([[1.0, 0.3, -0.2], [0.1, 0.7, 0.25], [-0.15, 0.2, 1.4]])
JACOBIAN = {"linElas": "LinElas", "hyperSS": "HyperSSdF", "hyperFS": "HyperFSdF"}


def mesh_case(name):
    """(mesh, clamped side set, GEO the fused kernels must report)."""
    if name in ("general", "stored"):
        return distorted_box(3, 3, 3, seed=2, amp=0.2), 1, (1 if name == "general" else 0)
    if name == "one":
        return distorted_box(1, 1, 1, seed=3, amp=0.2), 1, 1
    if name == "two":
        return distorted_box(2, 1, 1, seed=4, amp=0.2), 1, 1
    if name == "affine":
        m = box_mesh(3, 2, 2)
        m.coords = m.coords @ SHEAR.T + np.array([0.3, -0.1, 0.2])
        return m, 1, 2
    assert name == "swept"
    return hollow_cylinder_mesh(1, 5, 2), 998, 3


MESH_CASES = ["general", "one", "two", "affine", "swept", "stored"]


def build(ceed, meshname, Q, physics, qextra=0, **kw):
    mesh, side, geo = mesh_case(meshname)
    p = SolidProblem(ceed, mesh, Q - 1 - qextra, physics, nu=NU, E=E_MOD, bc_sides=[side], multigrid="uniform", qextra=qextra, **kw)
    assert p.Q == Q and [lv.degree + 1 for lv in p.levels] == list(range(2, Q - qextra + 1))
    n = p.lsize()
    X, Y = ceed.vector(n).set_array(p.smooth_state(0.1)), ceed.vector(n)
    p.form_residual(X, Y)                       # the stored state of the tangents, at a non-zero displacement
    if meshname == "stored":                    # a qdata vector written from outside: the operators read it (GEO 0)
        p.qdata.set_array(p.qdata.to_numpy().copy())
    X.destroy(); Y.destroy()
    return p, geo


def mass_name(P, Q, qf, geo):
    return f"fused_grad<P={P},Q={Q},{qf}+mass>/pencil [{km.GEO_TEXT[geo]}]"


def close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert np.isfinite(got).all() and got.shape == want.shape
    scale = np.abs(want).max()
    err = np.abs(got - want).max() / scale
    print(f"  {what}: {err:.2e} of max |y| = {scale:.3e}")
    assert scale > 0 and err <= TOL, (what, err)
    return err


def two_pass(p, lv, c, X, Y):
    """Y = K X, then += c M X with the level's mass operator in mask mode 3: the form dynamics.NewmarkPMG takes without the term."""
    op = p.levels[lv].opJacob
    op.set_mass_term(0.0)
    op.apply(X, Y)
    m = MassOperator(p, lv, c, mask_mode=3)
    m.apply_add(X, Y)
    m.destroy()


def parity_of_a_build(gpu, oracle, meshname, Q, physics, derived=True):
    p, geo = build(gpu, meshname, Q, physics)
    po, _ = build(oracle, meshname, Q, physics)
    qf = JACOBIAN[physics] + ("+derived" if physics == "hyperFS" and derived and km.derived_state(Q) else "")
    for lv, level in enumerate(p.levels):
        P, nl = level.degree + 1, p.lsize(lv)
        op = level.opJacob
        assert op.mass_term_available()
        x = np.random.default_rng(11 + lv).uniform(-1, 1, nl)
        X, Y, Xo, Yo = gpu.vector(nl).set_array(x), gpu.vector(nl), oracle.vector(nl).set_array(x), oracle.vector(nl)
        po.apply_jacobian(lv, Xo, Yo)
        ko = Yo.to_numpy()
        free = po.levels[lv].mask == 0
        for c in COEFS:
            ref = MassOperator(po, lv, c, portable=True)
            want_o = ko + np.where(free, ref.apply_host(x), 0.0)
            two_pass(p, lv, c, X, Y)
            want_d = Y.to_numpy()
            assert op.kernel_name == km.fused_name(P, Q, qf, geo), op.kernel_name
            Y.set_value(3.0)
            op.set_mass_term(c)
            op.apply(X, Y)
            got = Y.to_numpy()
            assert op.kernel_name == mass_name(P, Q, qf, geo), op.kernel_name
            close(got, want_d, f"{meshname} Q={Q} P={P} {qf} c={c:g} vs two passes on the device")
            close(got, want_o, f"{meshname} Q={Q} P={P} {qf} c={c:g} vs the oracle")
            assert np.all(got[~free] == 0.0)
            if c == COEFS[-1]:                  # the mass term dominates (at p = 4 on 12 elements M x is ~1e3 K x, more on coarser
                assert np.abs(got - ko).max() > 10.0 * np.abs(ko).max()      # levels): the comparison above is one of M x
            op.set_mass_term(0.0)
        for v in (X, Y, Xo, Yo):
            v.destroy()
    p.destroy(); po.destroy()


@pytest.mark.parametrize("meshname", MESH_CASES)
@pytest.mark.parametrize("physics", list(JACOBIAN))
@pytest.mark.parametrize("Q", range(2, 8))
def test_apply_with_the_term_matches_two_passes_and_the_oracle(gpu, oracle, Q, physics, meshname):
    parity_of_a_build(gpu, oracle, meshname, Q, physics)


@pytest.mark.parametrize("Q", [6, 7])
def test_plain_finite_strain_tangent_from_q6(product_lib, oracle, Q):
    """HyperFSdF without the derived state at Q >= 6 (the one route to it: the derived state switched off)."""
    plain = ceed_with_env(product_lib, {"CEED_MI355X_DERIVED": "0"})
    parity_of_a_build(plain, oracle, "general", Q, "hyperFS", derived=False)


@pytest.mark.parametrize("Q,qextra", [(3, 1), (4, 2), (5, 1), (6, 2), (7, 1), (7, 2)])
def test_levels_under_qextra(gpu, oracle, Q, qextra):
    """P = Q - 1 and P = Q - 2 as the FINE level (its stored state written by the residual kernel of that shape)."""
    p, geo = build(gpu, "general", Q, "hyperFS", qextra)
    po, _ = build(oracle, "general", Q, "hyperFS", qextra)
    lv, c = p.fine, COEFS[1]
    nl = p.lsize(lv)
    x = np.random.default_rng(5).uniform(-1, 1, nl)
    X, Y, Xo, Yo = gpu.vector(nl).set_array(x), gpu.vector(nl), oracle.vector(nl).set_array(x), oracle.vector(nl)
    po.apply_jacobian(lv, Xo, Yo)
    free = po.levels[lv].mask == 0
    want = Yo.to_numpy() + np.where(free, MassOperator(po, lv, c, portable=True).apply_host(x), 0.0)
    op = p.levels[lv].opJacob
    op.set_mass_term(c)
    op.apply(X, Y)
    qf = "HyperFSdF" + ("+derived" if km.derived_state(Q) else "")
    assert op.kernel_name == mass_name(Q - qextra, Q, qf, geo)
    close(Y.to_numpy(), want, f"Q={Q} qextra={qextra} vs the oracle")
    op.set_mass_term(0.0)
    p.destroy(); po.destroy()


# ------------------------------------------------------------------------------------------------------------------------------
# the other properties, on a few small problems: (mesh case, Q, physics)
# ------------------------------------------------------------------------------------------------------------------------------
SMALL = [("general", 3, "hyperSS"), ("swept", 5, "hyperFS"), ("affine", 6, "hyperFS"), ("general", 2, "linElas")]
SMALL_IDS = [f"{m}-Q{q}-{ph}" for m, q, ph in SMALL]


def level_vectors(ceed, p, lv, seed=21):
    nl = p.lsize(lv)
    x = np.random.default_rng(seed + lv).uniform(-1, 1, nl)
    return x, ceed.vector(nl).set_array(x), ceed.vector(nl)


@pytest.mark.parametrize("meshname,Q,physics", SMALL, ids=SMALL_IDS)
def test_cleared_term_gives_the_bits_and_the_kernel_of_an_operator_without_one(gpu, meshname, Q, physics):
    p, geo = build(gpu, meshname, Q, physics)
    for lv, level in enumerate(p.levels):
        op = level.opJacob
        x, X, Y = level_vectors(gpu, p, lv)
        op.apply(X, Y)
        before, name = Y.to_numpy(), op.kernel_name
        assert "+mass" not in name
        op.set_mass_term(COEFS[1])
        op.apply(X, Y)
        assert "+mass" in op.kernel_name and not np.array_equal(Y.to_numpy(), before)
        op.set_mass_term(0.0)
        Y.set_value(-1.0)
        op.apply(X, Y)
        assert np.array_equal(Y.to_numpy(), before) and op.kernel_name == name
    p.destroy()


def cheb_both(p, lv, arrs, b_form, assign_x):
    """(apply then step, CeedXOperatorApplyChebyshev) {x, d} of one step on level lv.  b_form: "b" -- the solver's step, the residual
    recomputed from b with c2 != 0 and not stored; "b first" -- a first step (c2 = 0), r stored; "r" -- the recurrence r -= A d."""
    c, L, op = p.ceed, p.ceed.L, p.levels[lv].opJacob
    n = p.lsize(lv)
    c1, c2 = C.c_double(0.37), C.c_double(0.0 if b_form == "b first" else 0.21)
    out = []
    for fused in (False, True):
        v = {k: c.vector(n).set_array(arrs[k]) for k in ("x", "d", "r", "b", "dinv")}
        t = c.vector(n).set_value(-3.0)
        src = v["d"] if b_form == "r" else v["x"]
        r = None if b_form == "b" else v["r"].h
        b = None if b_form == "r" else v["b"].h
        if fused:
            L.chk(L.lib.CeedXOperatorApplyChebyshev(op.h, src.h, t.h, v["x"].h, v["d"].h, r, b, v["dinv"].h, c1, c2, int(assign_x)))
        else:
            op.apply(src, t)
            if b_form == "b":
                L.chk(L.lib.CeedXVectorChebyshevStep(v["x"].h, v["d"].h, None, v["b"].h, t.h, v["dinv"].h, c1, c2, int(assign_x)))
            elif b_form == "b first":
                L.chk(L.lib.CeedXVectorChebyshevStart(v["x"].h, v["d"].h, v["r"].h, v["b"].h, t.h, v["dinv"].h, c1, int(assign_x)))
            else:
                L.chk(L.lib.CeedXVectorChebyshevUpdate(v["x"].h, v["d"].h, v["r"].h, t.h, v["dinv"].h, c1, c2, int(assign_x)))
        out.append({k: v[k].to_numpy() for k in ("x", "d", "r")})
        for w in list(v.values()) + [t]:
            w.destroy()
    return out


@pytest.mark.parametrize("meshname,Q,physics", SMALL, ids=SMALL_IDS)
def test_epilogue_forms_with_a_term_give_the_bits_of_apply_then_step(product_lib, meshname, Q, physics):
    gpu = ceed_with_env(product_lib, {"CEED_MI355X_ASSEMBLE": "serial"})
    p, _ = build(gpu, meshname, Q, physics)
    L = gpu.L
    for lv, level in enumerate(p.levels):
        op = level.opJacob
        arrs = _arrays(p, lv, 100 + lv)
        plain = cheb_both(p, lv, arrs, "b", False)[1]
        op.set_mass_term(COEFS[1])
        for b_form in ("b", "b first", "r"):
            for assign_x in (False, True):
                a, b = cheb_both(p, lv, arrs, b_form, assign_x)
                for k in ("x", "d", "r"):
                    assert np.array_equal(a[k], b[k]), (lv, b_form, assign_x, k, np.abs(a[k] - b[k]).max())
                assert "+mass" in op.kernel_name
        assert not np.array_equal(cheb_both(p, lv, arrs, "b", False)[1]["x"], plain["x"])       # the term is in the step
        nl = p.lsize(lv)
        X, B, T, W1, W2 = (gpu.vector(nl).set_array(arrs["x"]), gpu.vector(nl).set_array(arrs["b"]), gpu.vector(nl), gpu.vector(nl), gpu.vector(nl))
        op.apply(X, T)
        L.chk(L.lib.CeedXVectorWAXPBY(W1.h, C.c_double(1.0), B.h, C.c_double(-1.0), T.h))
        T.set_value(9.0)
        op.apply_residual(X, T, B, W2)
        assert np.array_equal(W1.to_numpy(), W2.to_numpy()) and "+mass" in op.kernel_name, lv
        op.set_mass_term(0.0)
        op.apply_residual(X, T, B, W2)
        assert not np.array_equal(W1.to_numpy(), W2.to_numpy())
    p.destroy()


@pytest.mark.parametrize("meshname,Q,physics", SMALL, ids=SMALL_IDS)
def test_apply_add_with_a_term_leaves_the_masked_rows_alone(gpu, meshname, Q, physics):
    p, _ = build(gpu, meshname, Q, physics)
    for lv, level in enumerate(p.levels):
        op = level.opJacob
        x, X, Y = level_vectors(gpu, p, lv)
        y0 = np.random.default_rng(3).uniform(-1, 1, x.size)
        op.set_mass_term(COEFS[1])
        op.apply(X, Y)
        ax = Y.to_numpy()
        Y.set_array(y0.copy())
        op.apply_add(X, Y)
        got = Y.to_numpy()
        masked = level.mask != 0
        assert masked.any() and np.array_equal(got[masked], y0[masked])
        assert "+mass" in op.kernel_name
        close(got[~masked], (y0 + ax)[~masked], f"{meshname} Q={Q} level {lv}: y0 + (K + c M) x")
        op.set_mass_term(0.0)
    p.destroy()


@pytest.mark.parametrize("mk,degree,physics", [(lambda: nb.distorted_box(9, 7, 5), 1, "linElas"), (lambda: hollow_cylinder_mesh(4, 24, 16), 4, "hyperFS")],
                         ids=["box p1", "cyl1536 p4"])
def test_pipelined_form_with_a_term_gives_the_bits_of_the_serial_form(product_lib, mk, degree, physics):
    """Reached as tests/test_numbering_gpu.py reaches it (the switches of test_gpu_parity.pipelined_assembly_equals_serial_assembly):
    three segments whatever the mesh size."""
    gated = ceed_with_env(product_lib, {"CEED_MI355X_PIPE_MIN_ROUNDS": "0", "CEED_MI355X_PIPE_SEGMENTS": "3", "CEED_MI355X_ASSEMBLE": "pipelined"})
    serial = ceed_with_env(product_lib, {"CEED_MI355X_ASSEMBLE": "serial"})
    mesh = mk()
    probs = [SolidProblem(c, mesh, degree, physics, nu=NU, E=E_MOD, bc_sides=[sorted(mesh.side_sets)[0]], multigrid="none") for c in (gated, serial)]
    n = probs[0].lsize()
    u0 = probs[0].smooth_state(0.1)
    vecs = [(c.vector(n), c.vector(n)) for c in (gated, serial)]
    for (X, Y), p in zip(vecs, probs):
        X.set_array(u0); p.form_residual(X, Y)
        p.levels[p.fine].opJacob.set_mass_term(COEFS[1])
    rng = np.random.default_rng(11)
    for it in range(4):
        x = rng.uniform(-1, 1, n)
        outs = []
        for (X, Y), p in zip(vecs, probs):
            X.set_array(x)
            p.apply_jacobian(p.fine, X, Y)
            if it == 2:
                p.apply_jacobian(p.fine, X, Y)
            outs.append(Y.to_numpy())
        assert np.array_equal(outs[0], outs[1]), it
    ops = [p.levels[p.fine].opJacob for p in probs]
    assert ops[0].kernel_name == ops[1].kernel_name and "+mass" in ops[0].kernel_name
    info = [op.launch_info() for op in ops]
    assert info[1]["segments"] == 1 and info[0]["segments"] == 3 and info[0]["streams"] == 2 and info[0]["assemble_launches"] == 3
    for p in probs:
        p.destroy()


@pytest.mark.parametrize("meshname,Q,physics", SMALL[:3], ids=SMALL_IDS[:3])
def test_recorded_apply_replays_the_eager_bits_and_keeps_its_coefficient(gpu, meshname, Q, physics):
    p, _ = build(gpu, meshname, Q, physics)
    lv = p.fine
    op = p.levels[lv].opJacob
    x, X, Y = level_vectors(gpu, p, lv)
    Yg = gpu.vector(x.size)
    c_old, c_new = COEFS[1], 3.0 * COEFS[1]
    op.set_mass_term(c_old)
    op.apply(X, Y)                                   # one eager apply before the recording
    eager_old = Y.to_numpy()
    g = gpu.capture(lambda: op.apply(X, Yg))
    Yg.set_value(-7.0)
    g.launch()
    assert np.array_equal(Yg.to_numpy(), eager_old)
    op.set_mass_term(c_new)
    op.apply(X, Y)
    eager_new = Y.to_numpy()
    assert not np.array_equal(eager_new, eager_old)
    Yg.set_value(-7.0); Yg.device_pointer()
    g.launch()
    assert np.array_equal(Yg.to_numpy(), eager_old)  # the recording keeps the coefficient it was made with
    g.destroy()
    op.set_mass_term(0.0)
    p.destroy()


NUMBERED = {"cyl p3 fs": (lambda: hollow_cylinder_mesh(2, 6, 2), 3, "hyperFS", [998]),
            "box p4 fs": (lambda: nb.distorted_box(3, 2, 3, seed=2, amp=0.2), 4, "hyperFS", [1])}


@pytest.mark.parametrize("numbering", ["permuted", "gaps"])
@pytest.mark.parametrize("case", list(NUMBERED))
def test_apply_with_a_term_under_a_numbering(monkeypatch, gpu, case, numbering):
    """`permuted`: the direct stores of the element-interior nodes stay on; `gaps` (entries no element holds): the map has no full
    cover.  Against two passes under the same numbering (1e-10) and, mapped back, the BITS of the default numbering: nothing the
    kernel adds depends on what a node is called."""
    mk, degree, physics, bc = NUMBERED[case]
    mesh = mk()
    res = {}
    for which, numb in (("default", nb.default), (numbering, nb.NUMBERINGS[numbering])):
        p = nb.problem_under(monkeypatch, numb, gpu, mesh, degree, physics, bc)
        dms = [lv.dofmap for lv in p.levels]
        if which == "default":
            u_def = nb.to_default(p.smooth_state(0.1), dms[-1])
        n = p.lsize()
        Xs, Ys = gpu.vector(n).set_array(nb.from_default(u_def, dms[-1], nb.UNREAD)), gpu.vector(n)
        p.form_residual(Xs, Ys)
        out = []
        for lv, level in enumerate(p.levels):
            dm, nl = dms[lv], p.lsize(lv)
            xd = np.random.default_rng(31 + lv).uniform(-1, 1, 3 * dm.new.size)
            X, Y = gpu.vector(nl).set_array(nb.from_default(xd, dm, nb.UNREAD)), gpu.vector(nl).set_value(nb.PRESET)
            op = level.opJacob
            op.set_mass_term(COEFS[1])
            op.apply(X, Y)
            got = Y.to_numpy()
            assert "+mass" in op.kernel_name
            held = nb.referenced(dm)
            assert np.all(got[~held] == 0.0)
            Y2 = gpu.vector(nl)
            two_pass(p, lv, COEFS[1], X, Y2)
            close(got[held], Y2.to_numpy()[held], f"{case} {which} level {lv} vs two passes")
            out.append(nb.to_default(got, dm))
        res[which] = out
        if which != "default" and numbering == "gaps":
            assert not all(nb.referenced(dm).all() for dm in dms)
        p.destroy()
    for lv, (a, b) in enumerate(zip(res["default"], res[numbering])):
        assert np.array_equal(a, b), (lv, np.abs(a - b).max())


@pytest.mark.parametrize("meshname,Q,physics", SMALL, ids=SMALL_IDS)
def test_diagonals_ignore_the_term(gpu, meshname, Q, physics):
    p, _ = build(gpu, meshname, Q, physics)
    for lv, level in enumerate(p.levels):
        nl = p.lsize(lv)
        D, B = gpu.vector(nl), gpu.vector(3 * nl)
        p.get_diag(lv, D); p.get_pointblock_diag(lv, B)
        d0, b0 = D.to_numpy(), B.to_numpy()
        level.opJacob.set_mass_term(COEFS[2])
        D.set_value(5.0); B.set_value(5.0)
        p.get_diag(lv, D); p.get_pointblock_diag(lv, B)
        assert np.array_equal(D.to_numpy(), d0) and np.array_equal(B.to_numpy(), b0) and np.abs(d0).max() > 0
        level.opJacob.set_mass_term(0.0)
    p.destroy()


def test_refusals(product_lib):
    gpu = ceed_with_env(product_lib, {})             # a Ceed of its own: the halo below needs a (one-rank) communicator
    p, _ = build(gpu, "two", 3, "hyperFS")
    with pytest.raises(cd.CeedError, match="a mass term belongs to a Jacobian operator"):
        p.opApply.set_mass_term(1.0)                                     # the residual operator
    m = MassOperator(p, p.fine, 1.0)
    with pytest.raises(cd.CeedError, match="a mass term belongs to a Jacobian operator"):
        m.op.set_mass_term(1.0)                                          # another kernel family
    with pytest.raises(cd.CeedError, match="a mass term belongs to a Jacobian operator"):
        m.op.mass_term_available()
    m.destroy()
    op = p.levels[p.fine].opJacob
    with pytest.raises(cd.CeedError, match="must be finite"):
        op.set_mass_term(float("nan"))
    # a halo with a neighbour: refused while the term is set, accepted again without
    n = p.lsize()
    X, Y = gpu.vector(n).set_array(np.ones(n)), gpu.vector(n)
    idx = np.array([0], dtype=np.int32)
    h = C.c_void_p()
    ident = C.create_string_buffer(128)
    gpu.L.chk(gpu.L.lib.CeedXCommGetUniqueId(gpu.h, ident))
    gpu.L.chk(gpu.L.lib.CeedXCommInit(gpu.h, C.c_int(1), C.c_int(0), C.c_char_p(ident.raw)))
    gpu.L.chk(gpu.L.lib.CeedXHaloCreate(gpu.h, 1, (C.c_int * 1)(0), (C.c_int * 1)(1), (C.POINTER(C.c_int) * 1)(idx.ctypes.data_as(C.POINTER(C.c_int))), C.byref(h)))
    op.set_mass_term(1.0)
    with pytest.raises(cd.CeedError, match="CeedXOperatorApplyWithHalo: the operator carries a mass term"):
        op.apply_with_halo(X, Y, h)
    with pytest.raises(cd.CeedError, match="CeedXOperatorApplyWithHalo: the operator carries a mass term"):
        op.apply_with_halo(X, Y, None)                                   # no halo at all: refused too, not a silent K + c M
    op.set_mass_term(0.0)
    op.apply_with_halo(X, Y, None)                                       # without a term and a halo: the plain apply
    assert "+mass" not in op.kernel_name
    gpu.L.chk(gpu.L.lib.CeedXHaloDestroy(C.byref(h)))
    p.destroy()
    # a (P, Q) without a kernel: Q = 8 keeps the two-pass form
    p8 = SolidProblem(gpu, box_mesh(1, 1, 1), 7, "linElas", nu=NU, E=E_MOD, bc_sides=[1], multigrid="none")
    op8 = p8.levels[p8.fine].opJacob
    assert not op8.mass_term_available()
    with pytest.raises(cd.CeedError, match="no fused kernel with the mass term is instantiated for P=8 Q=8"):
        op8.set_mass_term(1.0)
    op8.set_mass_term(0.0)                                               # clearing is always allowed
    p8.destroy()
