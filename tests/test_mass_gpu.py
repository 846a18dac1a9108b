"""The mass operator family on the device (csrc/kernels_mass.hip, ceed_op_mass.cpp) against its portable NumPy form (mass.py): every
instantiated (P, Q), the element-discontinuous restriction, a composite with the Jacobian, bits and mask, and the refusals of the
lowering and of the entry points.  The bound of the comparisons is the project's operator parity bound, 1e-10 of max |y|."""
import ctypes as C

import numpy as np
import pytest

from _numbering import distorted_box
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mass import MassOperator
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.solid import SolidProblem

pytestmark = pytest.mark.gpu

PAIRS = [(P, Q) for P in range(2, 9) for Q in range(P, 9)]          # the 28 pairs of CPS_DIAG_PQ
TOL = 1e-10
COEF = 1.75
WORST = {}                                                          # Q -> worst relative error seen (printed by the last test)


def make(gpu, mesh, P, Q, bc=(1,)):
    return SolidProblem(gpu, mesh, P - 1, "linElas", nu=0.3, E=1.0, multigrid="none", qextra=Q - P, bc_sides=list(bc))


def close(a, b, Q=None):
    err = np.abs(a - b).max() / np.abs(b).max()
    if Q is not None:
        WORST[Q] = max(WORST.get(Q, 0.0), err)
    return err


@pytest.mark.parametrize("P,Q", PAIRS)
def test_apply_add_and_diagonal_against_the_portable_form(gpu, P, Q):
    """27 distorted elements (no multiple of 2, 4, 8 or 16: every packing has a partial last group), nodes shared by 2, 4 and 8
    elements, side set 1 clamped."""
    prob = make(gpu, distorted_box(3, 3, 3), P, Q)
    assert len(PAIRS) == 28
    n = prob.lsize()
    mask = prob.levels[0].mask != 0
    assert mask.any() and not mask.all()
    dev, ref = MassOperator(prob, 0, COEF), MassOperator(prob, 0, COEF, portable=True)
    assert not dev.portable and ref.portable
    rng = np.random.default_rng(100 * P + Q)
    x, y0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    X, Y = gpu.vector(n).set_array(x), gpu.vector(n).set_value(5.0)
    want = np.where(mask, 0.0, ref.apply_host(x))
    dev.apply(X, Y)
    assert dev.kernel_name == f"mass<{P},{Q}>"
    e1 = close(Y.to_numpy(), want, Q)
    Y.set_array(y0)
    dev.apply_add(X, Y)
    assert dev.kernel_name == f"mass<{P},{Q}>"
    e2 = close(Y.to_numpy(), y0 + want, Q)
    assert np.array_equal(Y.to_numpy()[mask], y0[mask])
    D = gpu.vector(n).set_value(5.0)
    dev.diagonal(D)
    assert dev.kernel_name == f"mass_diag<{P},{Q}>"
    d = D.to_numpy()
    e3 = close(d, ref.diagonal_host(), Q)
    print(f"mass<{P},{Q}>: apply {e1:.2e}  apply_add {e2:.2e}  diagonal {e3:.2e}")
    assert e1 <= TOL and e2 <= TOL and e3 <= TOL
    assert np.all(d[mask] == 0.0) and np.all(d[~mask] > 0.0)
    dev.destroy(); prob.destroy()


def test_worst_error_per_Q():
    print("worst relative error against the portable form per Q:", {q: f"{e:.2e}" for q, e in sorted(WORST.items())})
    assert all(e <= TOL for e in WORST.values())


def test_element_discontinuous_restriction(gpu):
    prob = make(gpu, distorted_box(3, 3, 3), 3, 4)
    ne, P3 = 27, 27
    eoff = (np.arange(ne * P3, dtype=np.int64) * 3).astype(np.int32)
    rstr = gpu.elem_restriction(ne, P3, 3, 1, 3 * ne * P3, eoff)
    dev = MassOperator(prob, 0, COEF, rstr=rstr, offsets=eoff)
    ref = MassOperator(prob, 0, COEF, portable=True, rstr=rstr, offsets=eoff)
    n = 3 * ne * P3
    x = np.random.default_rng(7).uniform(-1, 1, n)
    X, Y = gpu.vector(n).set_array(x), gpu.vector(n)
    dev.apply(X, Y)
    assert dev.kernel_name == "mass<3,4>"
    assert close(Y.to_numpy(), ref.apply_host(x)) <= TOL
    dev.destroy(); rstr.destroy(); prob.destroy()


def test_composite_of_jacobian_and_mass_is_the_separate_sum(gpu):
    prob = make(gpu, distorted_box(3, 2, 2), 3, 3)
    L, n = gpu.L, prob.lsize()
    m = MassOperator(prob, 0, COEF)
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
    assert np.array_equal(Y.to_numpy(), Z.to_numpy())
    ref = MassOperator(prob, 0, COEF, portable=True)                      # ... and it IS K x + M x
    K = gpu.vector(n)
    opJ.apply(X, K)
    mask = prob.levels[0].mask != 0
    want = K.to_numpy() + np.where(mask, 0.0, ref.apply_host(x))
    assert close(Y.to_numpy(), y0 + want) <= TOL
    L.chk(L.lib.CeedOperatorApply(comp, X.h, Y.h, C.c_void_p(L.REQUEST_IMMEDIATE)))
    Z.set_value(0.0)
    opJ.apply_add(X, Z)
    m.apply_add(X, Z)
    assert np.array_equal(Y.to_numpy(), Z.to_numpy())
    L.lib.CeedOperatorDestroy(C.byref(comp))
    m.destroy(); prob.destroy()


def test_bits_mask_and_tail(gpu):
    prob = make(gpu, distorted_box(3, 3, 3), 4, 5, bc=(1, 6))
    n = prob.lsize()
    mask = prob.levels[0].mask != 0
    m = MassOperator(prob, 0, COEF)
    x = np.random.default_rng(13).uniform(-1, 1, n)
    X, Y1, Y2 = gpu.vector(n).set_array(x), gpu.vector(n), gpu.vector(n)
    m.apply(X, Y1); m.apply(X, Y2)
    assert np.array_equal(Y1.to_numpy(), Y2.to_numpy()) and np.abs(Y1.to_numpy()).max() > 0
    assert np.all(Y1.to_numpy()[mask] == 0.0)
    x0 = np.where(mask, 0.0, x)                                             # masked input reads as zero
    m.apply(gpu.vector(n).set_array(x0), Y2)
    assert np.array_equal(Y1.to_numpy(), Y2.to_numpy())
    long = gpu.vector(n + 7).set_value(-3.25)                               # the sentinel: masked rows and the tail beyond the L-size
    m.apply_add(X, long)
    v = long.to_numpy()
    assert np.all(v[:n][mask] == -3.25) and np.all(v[n:] == -3.25)
    assert np.array_equal(v[:n][~mask], (-3.25 + Y1.to_numpy())[~mask])
    m2 = MassOperator(prob, 0, COEF, mask_mode=2)                           # the residual's form reads the boundary values
    m2.apply(X, Y2)
    ref2 = MassOperator(prob, 0, COEF, portable=True, mask_mode=2)
    assert close(Y2.to_numpy(), np.where(mask, 0.0, ref2.apply_host(x))) <= TOL
    assert np.abs(Y2.to_numpy() - Y1.to_numpy()).max() > 1e-4
    m.set_coef(2 * COEF)                                                    # the context is re-read at every apply
    m.apply(X, Y2)
    assert np.array_equal(Y2.to_numpy(), 2.0 * Y1.to_numpy())
    m.destroy(); m2.destroy(); prob.destroy()


# ---- the lowering: one valid graph and one defective twin per check of op_plan, on a 2 x 1 x 1 box at P = 2, Q = 2 -------------------
@pytest.fixture(scope="module")
def box(gpu):
    prob = make(gpu, box_mesh(2, 1, 1), 2, 2, bc=(6,))
    lv = prob.levels[0]
    off = np.asarray(lv.dofmap.offsets(), dtype=np.int32)
    fine = np.array([[(2 * e + a) + 5 * b + 15 * k for k in range(3) for b in range(3) for a in range(3)] for e in (0, 1)], dtype=np.int32)
    s = dict(prob=prob, lv=lv, n=prob.lsize(),
             ru=lv.Erestrictu, bu=lv.basisu, rq=lv.Erestrictqdi, qdata=lv.qdata,
             ru_twin=gpu.elem_restriction(2, 8, 3, 1, prob.lsize(), off),
             bu_twin=gpu.basis_lagrange(3, 3, 2, 2, cd.GAUSS),
             r_nc1=gpu.elem_restriction(2, 8, 1, 1, prob.lsize() // 3, off // 3),
             r_strided=gpu.strided_restriction(2, 8, 3, 48),
             b32=gpu.basis_lagrange(3, 3, 3, 2, cd.GAUSS),
             r27=gpu.elem_restriction(2, 27, 3, 1, 135, fine * 3),
             rq_ne1=gpu.strided_restriction(1, 8, 10, 80),
             rq_nc9=gpu.strided_restriction(2, 8, 9, 144),
             rq_off=gpu.elem_restriction(2, 8, 10, 1, 160, np.arange(16, dtype=np.int32) * 10),
             qdata_short=gpu.vector(159).set_value(0.125))
    yield s
    prob.destroy()


def graph(gpu, s, ru_in="ru", ru_out="ru", b_in="bu", b_out="bu", rq="rq", qdata="qdata", ctx=(COEF,), u_mode=cd.EVAL_INTERP,
          v_mode=cd.EVAL_INTERP, u_size=3, q_size=10, extra_input=False, passive_u=False):
    qf = gpu.qfunction("Mass", source="qfunctions/mass.h:Mass")
    qf.add_input("u", u_size, u_mode).add_input("qdata", q_size, cd.EVAL_NONE)
    if extra_input:
        qf.add_input("more", 3, cd.EVAL_INTERP)
    qf.add_output("v", 3, v_mode)
    if ctx is not None:
        qf.set_context(list(ctx))
    op = gpu.operator(qf)
    op.set_field("u", s[ru_in], s[b_in], s["qdata"] if passive_u else "active")
    op.set_field("qdata", s[rq], None, s[qdata] if qdata else "active")
    if extra_input:
        op.set_field("more", s[ru_in], s[b_in], "active")
    op.set_field("v", s[ru_out], s[b_out], "active")
    return op


def apply_once(gpu, s, op, nin=None, nout=None):
    X = gpu.vector(nin or s["n"]).set_value(0.5)
    Y = gpu.vector(nout or s["n"])
    op.apply(X, Y)
    return Y.to_numpy()


def test_valid_graph_is_lowered_to_the_mass_kernel(gpu, box):
    assert gpu.has_qfunction("Mass") and gpu.has_qfunction("qfunctions/mass.h:Mass") and not gpu.has_qfunction("NoSuchQFunction")
    op = graph(gpu, box)
    y = apply_once(gpu, box, op)
    assert op.kernel_name == "mass<2,2>"
    # u = 0.5 everywhere: sum of M u over all rows = c * 0.5 * volume per component
    assert abs(y.reshape(-1, 3)[:, 0].sum() - COEF * 0.5 * 1.0) < 1e-12


DEFECTS = [
    (dict(u_mode=cd.EVAL_GRAD, u_size=9), "Mass eval modes must be INTERP(3) active, NONE(10) -> INTERP(3) active"),
    (dict(v_mode=cd.EVAL_NONE), "Mass eval modes must be"),
    (dict(q_size=9, rq="rq_nc9"), "Mass eval modes must be"),
    (dict(passive_u=True), "Mass eval modes must be"),
    (dict(extra_input=True), "Mass takes (u, qdata) -> v"),
    (dict(ru_out="ru_twin"), "active input and output must share one offsets restriction and one basis"),
    (dict(b_out="bu_twin"), "active input and output must share one offsets restriction and one basis"),
    (dict(ru_in="r_strided", ru_out="r_strided"), "active input and output must share one offsets restriction and one basis"),
    (dict(ru_in="r_nc1", ru_out="r_nc1"), "active fields must be 3 interlaced components"),
    (dict(b_in="b32", b_out="b32"), "restriction element size is not P^3"),
    (dict(rq="rq_ne1"), "qdata must be a strided 10 x Q^3 field"),
    (dict(rq="rq_off"), "qdata must be a strided 10 x Q^3 field"),
    (dict(ru_in="r27", ru_out="r27", b_in="b32", b_out="b32"), "the mass kernel needs P <= Q"),
    (dict(ctx=None), "needs its context"),
    (dict(qdata="qdata_short"), "qdata vector too short"),
    (dict(qdata=None), "qdata needs a passive vector"),
]


@pytest.mark.parametrize("defect,message", DEFECTS, ids=[m[:40] + "/" + ",".join(d) for d, m in DEFECTS])
def test_defective_twin_is_refused(gpu, box, defect, message):
    op = graph(gpu, box, **defect)
    n = 135 if defect.get("ru_in") == "r27" else None
    with pytest.raises(cd.CeedError) as ei:
        apply_once(gpu, box, op, n, n)
    assert message in str(ei.value), str(ei.value)
    assert "outside the kernel families" in str(ei.value) or message.startswith(("needs", "qdata vector", "qdata needs"))


def test_entry_point_refusals(gpu, box):
    s, n = box, box["n"]
    op = graph(gpu, s)
    v = [gpu.vector(n).set_value(0.25) for _ in range(6)]
    for call in (lambda: op.apply_chebyshev(v[0], v[1], v[2], v[3], None, v[4], v[5], 1.0, 0.0),
                 lambda: op.apply_residual(v[0], v[1], v[2], v[3]),
                 lambda: op.apply_state(v[0]),
                 lambda: op.set_overlap_split(1, np.zeros(n, dtype=np.uint8)),
                 lambda: op.apply_phase(v[0], v[1], 0)):
        with pytest.raises(cd.CeedError, match="is provided for the"):
            call()
    with pytest.raises(cd.CeedError, match="point-block diagonal assembly is not provided for the mass operator"):
        op.assemble_pointblock_diagonal(gpu.vector(3 * n))
    with pytest.raises(cd.CeedError, match="diagonal vector too short"):
        op.assemble_diagonal(gpu.vector(n - 1))
    with pytest.raises(cd.CeedError, match="shorter than the restriction's L-size"):
        op.apply(gpu.vector(n - 1).set_value(0.0), v[1])
    with pytest.raises(cd.CeedError, match="in-place"):
        op.apply(v[0], v[0])


def test_first_apply_during_capture_is_refused_then_replays_to_the_eager_bits(gpu, box):
    s, n = box, box["n"]
    off = np.asarray(s["lv"].dofmap.offsets(), dtype=np.int32)
    s2 = dict(s, ru=gpu.elem_restriction(2, 8, 3, 1, n, off))               # a restriction no operator has applied: no transpose map yet
    op = graph(gpu, s2)
    op.set_dirichlet_mask_mode(s["lv"].mask, None, 3)
    x = np.random.default_rng(17).uniform(-1, 1, n)
    X, Y = gpu.vector(n).set_array(x), gpu.vector(n).set_value(0.0)
    X.device_pointer(); Y.device_pointer()                                  # on the device before anything is recorded
    with pytest.raises(cd.CeedError, match="apply the operator once before recording"):
        gpu.capture(lambda: op.apply(X, Y))
    op.apply(X, Y)
    eager = Y.to_numpy().copy()
    assert np.abs(eager).max() > 0
    g = gpu.capture(lambda: op.apply(X, Y))
    Y.set_value(0.0)
    g.launch()
    assert np.array_equal(Y.to_numpy(), eager)
    g.destroy()
