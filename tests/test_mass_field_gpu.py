"""The mass operator with a density field on the device (QFunction "MassField": k_mass's modes with a field, csrc/kernels_mass.hip,
ceed_op_mass.cpp) against its portable NumPy form (mass.py): every instantiated (P, Q) with a nodal and a per-element density, the
component-wise Dirichlet masks, caller numberings, a composite, graph recording with the density rewritten in place, and every
refusal of the lowering.  Bound: 1e-12 of the largest entry, DESIGN.md 2's bound for device against portable."""
import ctypes as C

import numpy as np
import pytest

from _numbering import NUMBERINGS, distorted_box
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd import solid
from ceedpetscsolid_amd.mass import DensityField, MassOperator
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem

pytestmark = pytest.mark.gpu

PAIRS = [(P, Q) for P in range(2, 9) for Q in range(P, 9)]          # the 28 pairs of CPS_DIAG_PQ
TOL = 1e-12
COEF = 1.75
SENTINEL = -3.25


def make(gpu, mesh, P, Q, bc=(1,)):
    return SolidProblem(gpu, mesh, P - 1, "linElas", nu=0.3, E=1.0, multigrid="none", qextra=Q - P, bc_sides=list(bc))


def nodal_rho(X):
    """In [0.5, 2] on the (slightly distorted) unit cube, and at the origin, where the nodes no element holds of a numbering lie."""
    return 0.5 + 1.5 * (0.5 * X[:, 0] + 0.3 * X[:, 1] ** 2 + 0.2 * X[:, 2]).clip(0.0, 1.0)


def fields(ne):
    return {"nodal": DensityField.nodal(nodal_rho),
            "per_element": DensityField.per_element(0.5 + 1.5 * np.random.default_rng(5).uniform(0, 1, ne))}


def err(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("P,Q", PAIRS)
def test_every_pair_against_the_portable_form(gpu, P, Q):
    """A distorted 3 x 7 x 1 box: 21 elements leave the last workgroup partial at every packing (21 mod 16, 8, 4, 2 are non-zero), the
    smallest shape at which the `live` guard and the looped x and y passes can go wrong.  Side set 1 clamped."""
    prob = make(gpu, distorted_box(3, 7, 1), P, Q)
    assert len(PAIRS) == 28
    n = prob.lsize()
    mask = prob.levels[0].mask != 0
    assert mask.any() and not mask.all()
    rng = np.random.default_rng(100 * P + Q)
    x, y0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    X = gpu.vector(n).set_array(x)
    for kind, f in fields(21).items():
        dev, ref = MassOperator(prob, 0, COEF, density=f), MassOperator(prob, 0, COEF, density=f, portable=True)
        assert not dev.portable and ref.portable
        rho = dev.rho
        assert 0.5 <= rho.min() and rho.max() <= 2.0 and rho.max() - rho.min() > 0.5
        want = np.where(mask, 0.0, ref.apply_host(x))
        Y = gpu.vector(n).set_value(5.0)
        dev.apply(X, Y)
        assert dev.kernel_name == f"mass_field<{P},{Q}>"
        e1 = err(Y.to_numpy(), want)
        Y.set_array(y0)
        dev.apply_add(X, Y)
        assert dev.kernel_name == f"mass_field<{P},{Q}>"
        e2 = err(Y.to_numpy(), y0 + want)
        assert np.array_equal(Y.to_numpy()[mask], y0[mask])
        D = gpu.vector(n).set_value(5.0)
        dev.diagonal(D)
        assert dev.kernel_name == f"mass_field_diag<{P},{Q}>"
        d = D.to_numpy()
        e3 = err(d, ref.diagonal_host())
        D.set_value(5.0)
        dev.lumped(D)
        assert dev.kernel_name == f"mass_field<{P},{Q}>"
        e4 = err(D.to_numpy(), ref.lumped_host())
        print(f"mass_field<{P},{Q}> {kind}: apply {e1:.2e}  apply_add {e2:.2e}  diagonal {e3:.2e}  lumped {e4:.2e}")
        assert e1 <= TOL and e2 <= TOL and e3 <= TOL and e4 <= TOL
        assert np.all(d[mask] == 0.0) and np.all(d[~mask] > 0.0) and np.all(D.to_numpy()[mask] == 0.0)
        dev.destroy()
    prob.destroy()


@pytest.mark.parametrize("mode", [2, 3])
def test_all_eight_component_mask_patterns(gpu, mode):
    """Node n carries pattern n % 8 (bit c: component c constrained): every pattern on nodes shared by 1, 2 and 4 elements."""
    P, Q = 3, 4
    prob = make(gpu, distorted_box(3, 7, 1), P, Q, bc=())
    n = prob.lsize()
    pat = np.arange(n // 3) % 8
    mask = ((pat[:, None] >> np.arange(3)[None, :]) & 1).astype(bool).reshape(-1)
    assert len(set(pat.tolist())) == 8
    rng = np.random.default_rng(mode)
    x = rng.uniform(-1, 1, n)
    X = gpu.vector(n).set_array(x)
    for kind, f in fields(21).items():
        dev, ref = MassOperator(prob, 0, COEF, density=f, mask_mode=mode), MassOperator(prob, 0, COEF, density=f, portable=True, mask_mode=mode)
        dev.mask = ref.mask = mask
        dev.op.set_dirichlet_mask_mode(mask.astype(np.uint8), None, mode)
        want = np.where(mask, 0.0, ref.apply_host(x))
        other = np.where(mask, 0.0, ref.apply_host(x, mask_mode=5 - mode))
        assert err(other, want) > 1e-3                                          # the two modes differ on this input
        Y = gpu.vector(n).set_value(5.0)
        dev.apply(X, Y)
        assert dev.kernel_name == f"mass_field<{P},{Q}>"
        assert err(Y.to_numpy(), want) <= TOL and np.all(Y.to_numpy()[mask] == 0.0)
        D = gpu.vector(n).set_value(5.0)
        dev.diagonal(D)
        assert err(D.to_numpy(), ref.diagonal_host()) <= TOL and np.all(D.to_numpy()[mask] == 0.0) and np.all(D.to_numpy()[~mask] > 0.0)
        dev.lumped(D)
        assert err(D.to_numpy(), ref.lumped_host()) <= TOL and np.all(D.to_numpy()[mask] == 0.0)
        dev.destroy()
    prob.destroy()


@pytest.mark.parametrize("numbering", ["permuted", "gaps"])
def test_caller_numberings(gpu, monkeypatch, numbering):
    """rho goes through its own restriction on the level's nodes, whatever their numbers; entries no element holds stay zero."""
    monkeypatch.setattr(solid, "build_dofmap", NUMBERINGS[numbering])
    P, Q = 3, 3
    prob = make(gpu, distorted_box(3, 7, 1), P, Q)
    n = prob.lsize()
    mask = prob.levels[0].mask != 0
    x = np.random.default_rng(9).uniform(-1, 1, n)
    X = gpu.vector(n).set_array(x)
    for kind, f in fields(21).items():
        dev, ref = MassOperator(prob, 0, COEF, density=f), MassOperator(prob, 0, COEF, density=f, portable=True)
        Y = gpu.vector(n).set_value(5.0)
        dev.apply(X, Y)
        assert dev.kernel_name == f"mass_field<{P},{Q}>"
        assert err(Y.to_numpy(), np.where(mask, 0.0, ref.apply_host(x))) <= TOL
        D = gpu.vector(n).set_value(5.0)
        dev.diagonal(D)
        assert err(D.to_numpy(), ref.diagonal_host()) <= TOL
        dev.destroy()
    prob.destroy()


def test_element_discontinuous_restriction_of_the_caller(gpu):
    """x through the caller's element-discontinuous restriction, rho still through its own on the level's nodes."""
    prob = make(gpu, distorted_box(3, 7, 1), 3, 4)
    ne, P3 = 21, 27
    eoff = (np.arange(ne * P3, dtype=np.int64) * 3).astype(np.int32)
    rstr = gpu.elem_restriction(ne, P3, 3, 1, 3 * ne * P3, eoff)
    n = 3 * ne * P3
    x = np.random.default_rng(7).uniform(-1, 1, n)
    X, Y = gpu.vector(n).set_array(x), gpu.vector(n)
    for kind, f in fields(ne).items():
        dev = MassOperator(prob, 0, COEF, rstr=rstr, offsets=eoff, density=f)
        ref = MassOperator(prob, 0, COEF, portable=True, rstr=rstr, offsets=eoff, density=f)
        dev.apply(X, Y)
        assert dev.kernel_name == "mass_field<3,4>"
        assert err(Y.to_numpy(), ref.apply_host(x)) <= TOL
        dev.destroy()
    rstr.destroy(); prob.destroy()


def test_apply_add_leaves_masked_rows_and_the_tail_alone(gpu):
    prob = make(gpu, distorted_box(3, 7, 1), 4, 5, bc=(1, 6))
    n = prob.lsize()
    mask = prob.levels[0].mask != 0
    m = MassOperator(prob, 0, COEF, density=fields(21)["nodal"])
    x = np.random.default_rng(13).uniform(-1, 1, n)
    X, Y1, Y2 = gpu.vector(n).set_array(x), gpu.vector(n), gpu.vector(n)
    m.apply(X, Y1); m.apply(X, Y2)
    assert np.array_equal(Y1.to_numpy(), Y2.to_numpy()) and np.abs(Y1.to_numpy()).max() > 0
    long = gpu.vector(n + 7).set_value(SENTINEL)
    m.apply_add(X, long)
    v = long.to_numpy()
    assert np.all(v[:n][mask] == SENTINEL) and np.all(v[n:] == SENTINEL)
    assert np.array_equal(v[:n][~mask], (SENTINEL + Y1.to_numpy())[~mask])
    long.set_value(SENTINEL)
    m.apply(X, long)                                                        # overwrite: masked rows and the tail are zero
    v = long.to_numpy()
    assert np.all(v[:n][mask] == 0.0) and np.all(v[n:] == 0.0) and np.array_equal(v[:n], Y1.to_numpy())
    m.set_coef(2 * COEF)                                                    # the context is re-read at every apply
    m.apply(X, Y2)
    assert np.array_equal(Y2.to_numpy(), 2.0 * Y1.to_numpy())
    m.destroy(); prob.destroy()


def test_composite_of_jacobian_and_mass_field_is_the_separate_sum(gpu):
    prob = make(gpu, distorted_box(3, 2, 2), 3, 3)
    L, n = gpu.L, prob.lsize()
    m = MassOperator(prob, 0, COEF, density=fields(12)["per_element"])
    opJ = prob.levels[0].opJacob
    comp = C.c_void_p()
    L.chk(L.lib.CeedCompositeOperatorCreate(gpu.h, C.byref(comp)))
    L.chk(L.lib.CeedCompositeOperatorAddSub(comp, opJ.h))
    L.chk(L.lib.CeedCompositeOperatorAddSub(comp, m.op.h))
    rng = np.random.default_rng(11)
    x, y0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    X, Y, Z = gpu.vector(n).set_array(x), gpu.vector(n).set_array(y0), gpu.vector(n).set_array(y0)
    L.chk(L.lib.CeedOperatorApplyAdd(comp, X.h, Y.h, C.c_void_p(L.REQUEST_IMMEDIATE)))
    opJ.apply_add(X, Z)
    m.apply_add(X, Z)
    assert m.kernel_name == "mass_field<3,3>"
    assert np.array_equal(Y.to_numpy(), Z.to_numpy())
    L.chk(L.lib.CeedOperatorApply(comp, X.h, Y.h, C.c_void_p(L.REQUEST_IMMEDIATE)))
    Z.set_value(0.0)
    opJ.apply_add(X, Z)
    m.apply_add(X, Z)
    assert np.array_equal(Y.to_numpy(), Z.to_numpy())
    ref = MassOperator(prob, 0, COEF, density=fields(12)["per_element"], portable=True)
    K = gpu.vector(n)
    opJ.apply(X, K)
    mask = prob.levels[0].mask != 0
    assert err(Y.to_numpy(), K.to_numpy() + np.where(mask, 0.0, ref.apply_host(x))) <= 1e-10      # (K's own parity bound)
    L.lib.CeedOperatorDestroy(C.byref(comp))
    m.destroy(); prob.destroy()


def test_without_a_density_the_kernel_is_the_one_it_was(gpu):
    prob = make(gpu, distorted_box(3, 7, 1), 3, 4)
    n = prob.lsize()
    m = MassOperator(prob, 0, COEF)
    X, Y = gpu.vector(n).set_value(0.5), gpu.vector(n)
    m.apply(X, Y)
    assert m.kernel_name == "mass<3,4>" and m.rho_vec is None
    m.diagonal(Y)
    assert m.kernel_name == "mass_diag<3,4>"
    m.destroy(); prob.destroy()


# ---- the lowering: one valid graph and one defective twin per check of op_plan, on a 2 x 1 x 1 box at P = 2, Q = 2 -------------------
@pytest.fixture(scope="module")
def box(gpu):
    prob = make(gpu, box_mesh(2, 1, 1), 2, 2, bc=(6,))
    lv = prob.levels[0]
    off = np.asarray(lv.dofmap.offsets(), dtype=np.int32)
    nodes = off // 3
    nn = prob.lsize() // 3
    fine = np.array([[(2 * e + a) + 5 * b + 15 * k for k in range(3) for b in range(3) for a in range(3)] for e in (0, 1)], dtype=np.int32)
    s = dict(prob=prob, lv=lv, n=prob.lsize(),
             ru=lv.Erestrictu, bu=lv.basisu, rq=lv.Erestrictqdi, qdata=lv.qdata,
             rr=gpu.elem_restriction(2, 8, 1, 1, nn, nodes), br=gpu.basis_lagrange(3, 1, 2, 2, cd.GAUSS),
             rho=gpu.vector(nn).set_value(2.0), rho_short=gpu.vector(nn - 1).set_value(2.0),
             rr_nc3=gpu.elem_restriction(2, 8, 3, 1, prob.lsize(), off),
             rr_ne1=gpu.elem_restriction(1, 8, 1, 1, nn, nodes.reshape(-1)[:8]),
             rr_27=gpu.elem_restriction(2, 27, 1, 1, 45, fine),
             rr_strided=gpu.strided_restriction(2, 8, 1, 16),
             br_q3=gpu.basis_lagrange(3, 1, 2, 3, cd.GAUSS), br_p3=gpu.basis_lagrange(3, 1, 3, 2, cd.GAUSS),
             br_lobatto=gpu.basis_lagrange(3, 1, 2, 2, cd.GAUSS_LOBATTO),
             b32=gpu.basis_lagrange(3, 3, 3, 2, cd.GAUSS), b32r=gpu.basis_lagrange(3, 1, 3, 2, cd.GAUSS),
             r27=gpu.elem_restriction(2, 27, 3, 1, 135, fine * 3),
             rq_nc9=gpu.strided_restriction(2, 8, 9, 144),
             qdata_short=gpu.vector(159).set_value(0.125))
    yield s
    prob.destroy()


def graph(gpu, s, ru="ru", bu="bu", rr="rr", br="br", rho="rho", rq="rq", qdata="qdata", ctx=(COEF,), u_mode=cd.EVAL_INTERP, u_size=3,
          rho_mode=cd.EVAL_INTERP, rho_size=1, q_size=10, v_mode=cd.EVAL_INTERP, no_rho=False, name="MassField"):
    qf = gpu.qfunction(name, source=f"qfunctions/mass.h:{name}")
    qf.add_input("u", u_size, u_mode)
    if not no_rho:
        qf.add_input("rho", rho_size, rho_mode)
    qf.add_input("qdata", q_size, cd.EVAL_NONE).add_output("v", 3, v_mode)
    if ctx is not None:
        qf.set_context(list(ctx))
    op = gpu.operator(qf)
    op.set_field("u", s[ru], s[bu], "active")
    if not no_rho:
        op.set_field("rho", s[rr], s[br] if br else None, s[rho] if rho != "active" else "active")
    op.set_field("qdata", s[rq], None, s[qdata])
    op.set_field("v", s[ru], s[bu], "active")
    return op


def apply_once(gpu, s, op, n=None):
    X = gpu.vector(n or s["n"]).set_value(0.5)
    Y = gpu.vector(n or s["n"]).set_value(SENTINEL)
    try:
        op.apply(X, Y)
    except cd.CeedError:
        assert np.all(Y.to_numpy() == SENTINEL), "a refused apply wrote into its output"
        raise
    return Y.to_numpy()


def test_valid_graph_is_lowered_to_the_field_kernel(gpu, box):
    assert gpu.has_qfunction("MassField") and gpu.has_qfunction("qfunctions/mass.h:MassField") and gpu.has_qfunction("Mass")
    op = graph(gpu, box)
    y = apply_once(gpu, box, op)
    assert op.kernel_name == "mass_field<2,2>"
    # u = 0.5, rho = 2 everywhere: the sum of M u over all rows = c * 2 * 0.5 * volume per component (nothing masked: no mask set)
    assert abs(y.reshape(-1, 3)[:, 0].sum() - COEF * 2.0 * 0.5 * 1.0) < 1e-12
    D = gpu.vector(box["n"])
    op.assemble_diagonal(D)
    assert op.kernel_name == "mass_field_diag<2,2>"
    with pytest.raises(cd.CeedError, match="point-block diagonal assembly is not provided for the mass operator"):
        op.assemble_pointblock_diagonal(gpu.vector(3 * box["n"]))


DEFECTS = [
    (dict(no_rho=True), "MassField takes (u, rho, qdata) -> v"),
    (dict(u_mode=cd.EVAL_GRAD, u_size=9), "MassField eval modes must be INTERP(3) active, INTERP(1), NONE(10) -> INTERP(3) active"),
    (dict(rho_mode=cd.EVAL_NONE), "MassField eval modes must be"),
    (dict(rho_size=3), "MassField eval modes must be"),
    (dict(q_size=9, rq="rq_nc9"), "MassField eval modes must be"),
    (dict(v_mode=cd.EVAL_NONE), "MassField eval modes must be"),
    (dict(rho="active"), "rho must be a passive field with a vector of its own, not the active one"),
    (dict(rr="rr_nc3"), "rho must be on an offsets restriction with 1 component"),
    (dict(rr="rr_strided"), "rho must be on an offsets restriction with 1 component"),
    (dict(rr="rr_ne1"), "rho's restriction must have the element count of u's"),
    (dict(rr="rr_27"), "rho's restriction must have the element size P^3 of u's"),
    (dict(br="br_q3"), "rho's basis must have u's P, Q and interp table"),
    (dict(br="br_p3"), "rho's basis must have u's P, Q and interp table"),
    (dict(br="br_lobatto"), "rho's basis must have u's P, Q and interp table"),
    (dict(br=None), "rho's basis must have u's P, Q and interp table"),
    (dict(ru="r27", bu="b32", rr="rr_27", br="b32r"), "the mass kernel needs P <= Q"),
    (dict(rho="rho_short"), "rho vector shorter than its restriction's L-size"),
    (dict(ctx=None), "needs its context"),
    (dict(qdata="qdata_short"), "qdata vector too short"),
]


@pytest.mark.parametrize("defect,message", DEFECTS, ids=[m[:40] + "/" + ",".join(d) for d, m in DEFECTS])
def test_defective_twin_is_refused_before_anything_is_queued(gpu, box, defect, message):
    op = graph(gpu, box, **defect)
    with pytest.raises(cd.CeedError) as ei:
        apply_once(gpu, box, op, 135 if defect.get("ru") == "r27" else None)
    assert message in str(ei.value), str(ei.value)
    assert "outside the kernel families" in str(ei.value) or message.startswith(("needs", "qdata vector", "rho vector"))


def test_in_place_and_short_vectors_are_refused(gpu, box):
    n = box["n"]
    op = graph(gpu, box)
    v = gpu.vector(n).set_value(SENTINEL)
    with pytest.raises(cd.CeedError, match="in-place"):
        op.apply(v, v)
    assert np.all(v.to_numpy() == SENTINEL)
    with pytest.raises(cd.CeedError, match="shorter than the restriction's L-size"):
        op.apply(gpu.vector(n - 1).set_value(0.0), v)
    with pytest.raises(cd.CeedError, match="diagonal vector too short"):
        op.assemble_diagonal(gpu.vector(n - 1))
    assert np.all(v.to_numpy() == SENTINEL)


def test_recording_sees_a_density_rewritten_in_place(gpu):
    """A first apply while recording is refused with build_csr's message; after one eager apply the operator records, and the replay
    reads the density behind the recorded address: new values give the new result."""
    P, Q = 3, 4
    prob = make(gpu, distorted_box(3, 7, 1), P, Q)
    n = prob.lsize()
    f = fields(21)["nodal"]
    off = np.asarray(prob.levels[0].dofmap.offsets(), dtype=np.int32)
    fresh = gpu.elem_restriction(21, P ** 3, 3, 1, n, off)                  # a restriction no operator has applied: no transpose map yet
    m = MassOperator(prob, 0, COEF, density=f, rstr=fresh, offsets=off)
    ref = MassOperator(prob, 0, COEF, density=f, rstr=fresh, offsets=off, portable=True)
    x = np.random.default_rng(17).uniform(-1, 1, n)
    X, Y = gpu.vector(n).set_array(x), gpu.vector(n).set_value(0.0)
    X.device_pointer(); Y.device_pointer(); m.rho_vec.device_pointer()      # on the device before anything is recorded
    with pytest.raises(cd.CeedError, match="apply the operator once before recording"):
        gpu.capture(lambda: m.apply(X, Y))
    m.apply(X, Y)
    eager = Y.to_numpy().copy()
    assert err(eager, ref.apply_host(x)) <= TOL
    g = gpu.capture(lambda: m.apply(X, Y))
    Y.set_value(0.0); Y.device_pointer()
    g.launch()
    assert np.array_equal(Y.to_numpy(), eager)
    addr = m.rho_vec.device_pointer()
    new = m.rho[::-1].copy() * 1.5
    m.set_density_values(new); ref.set_density_values(new)
    assert m.rho_vec.device_pointer() == addr
    Y.set_value(0.0); Y.device_pointer()
    g.launch()
    got = Y.to_numpy()
    assert err(got, ref.apply_host(x)) <= TOL and err(got, eager) > 1e-2
    m.apply(X, Y)                                                           # ... and they are the bits of an eager apply
    assert np.array_equal(Y.to_numpy(), got)
    g.destroy(); m.destroy(); fresh.destroy(); prob.destroy()
