"""Thermal loads on the device (QFunctions "ThermalForce", "ThermalTangent", "{LinElas,HyperSS,HyperFS}StressThermal": k_stress's modes with
a temperature field, csrc/kernels_stress.hip, ceed_op_thermal.cpp) against their portable NumPy forms (thermal.py, postprocess.py): every
instantiated (P, Q) in the four modes and the three models, the Dirichlet mask modes, graph recording with the temperature rewritten in
place, every refusal of the lowering, the force-free expansions of tests/test_thermal.py and the three solvers against the CPU oracle.
Bounds: 1e-12 of the largest entry for the loads (DESIGN.md 2's bound for device against portable), 1e-10 for the stress modes (the
Stress tests' bound) and for device against oracle solves."""
import numpy as np
import pytest

import test_thermal as tt
from _numbering import distorted_box
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.dynamics import ExplicitDynamics, NewmarkPMG
from ceedpetscsolid_amd.mesh import box_mesh
from ceedpetscsolid_amd.postprocess import Stress
from ceedpetscsolid_amd.solid import SolidProblem
from ceedpetscsolid_amd.solver import NewtonPMG
from ceedpetscsolid_amd.thermal import ThermalLoad

pytestmark = pytest.mark.gpu

PAIRS = [(P, Q) for P in range(2, 9) for Q in range(P, 9)]          # the 28 pairs of CPS_DIAG_PQ
MODELS = ("linElas", "hyperSS", "hyperFS")
TOL, STRESS_TOL = 1e-12, 1e-10
ALPHA = 2e-3
SENTINEL = -3.25
EPB = {2: 16, 3: 8, 4: 4, 5: 2, 6: 2, 7: 1, 8: 1}                    # elements per workgroup (kernel_line_pass.hpp, MassGeom)


def make(gpu, mesh, P, Q, name, bc=(1,)):
    return SolidProblem(gpu, mesh, P - 1, name, nu=0.3, E=1.5, multigrid="none", qextra=Q - P, bc_sides=list(bc))


def theta_field(X):
    return 30.0 * (1.0 + 0.5 * X[:, 0] - 0.4 * X[:, 1] ** 2 + 0.3 * X[:, 2])


def state(prob, seed):
    """A smooth displacement with its boundary values, a little noise on top (det F stays near 1 at every P), and a variation."""
    n = prob.lsize()
    rng = np.random.default_rng(seed)
    return prob.smooth_state(0.05) + 1e-4 * rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)


def err(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def pair_against_portable(gpu, mesh, P, Q):
    worst = {"force": 0.0, "tangent": 0.0, "points": 0.0, "nodal": 0.0}
    for name in MODELS:
        prob = make(gpu, mesh, P, Q, name)
        n = prob.lsize()
        mask = prob.levels[0].mask != 0
        assert mask.any() and not mask.all()
        u, dx = state(prob, 100 * P + Q)
        dev, ref = ThermalLoad(prob, 0, ALPHA, theta_field, name), ThermalLoad(prob, 0, ALPHA, theta_field, name, portable=True)
        assert not dev.portable and ref.portable and np.ptp(dev.theta) > 5.0
        U, D, Y = gpu.vector(n).set_array(u), gpu.vector(n).set_array(dx), gpu.vector(n).set_value(5.0)
        dev.force(U, Y)
        assert dev.kernel_name["force"] == f"thermal_force<P={P},Q={Q}>"
        want = np.where(mask, 0.0, ref.force_host(u))
        worst["force"] = max(worst["force"], err(Y.to_numpy(), want))
        assert np.all(Y.to_numpy()[mask] == 0.0)
        if name == "hyperFS":
            Y.set_value(5.0)
            dev.tangent(U, D, Y)
            assert dev.kernel_name["tangent"] == f"thermal_tangent<P={P},Q={Q}>"
            worst["tangent"] = err(Y.to_numpy(), np.where(mask, 0.0, ref.tangent_host(u, dx)))
            assert np.all(Y.to_numpy()[mask] == 0.0)
        sd, sr = Stress(prob, name, thermal=dev), Stress(prob, name, thermal=ref, portable=True)
        assert not sd.portable
        pts, nod = sd.points(U), sd.nodal(U)
        assert sd.kernel_names == {"points": f"stress<P={P},Q={Q},points+thermal>", "nodal": f"stress<P={P},Q={Q},nodal+thermal>"}
        x = U.to_numpy()
        worst["points"] = max(worst["points"], err(pts, sr.points_host(x)))
        sums = sr.nodal_sums_host(x)
        worst["nodal"] = max(worst["nodal"], err(nod, sums[:, :6] / sums[:, 6:7]))
        plain = Stress(prob, name)
        assert err(plain.points(U), pts) > 1e-3                                  # the thermal term is there
        for o in (sd, sr, plain, dev, ref):
            o.destroy()
        prob.destroy()
    return worst


@pytest.mark.parametrize("P,Q", PAIRS)
def test_every_pair_mode_and_model_against_the_portable_form(gpu, P, Q):
    """A distorted 3 x 1 x 1 box: 3 elements are a multiple of no EPB above 1, so the last workgroup has dead element slots; the pairs
    with more than 3 elements per workgroup also run a strip of 5.  Side set 1 clamped."""
    assert len(PAIRS) == 28
    meshes = [distorted_box(3, 1, 1)] + ([distorted_box(5, 1, 1)] if EPB[Q] > 3 else [])
    for mesh in meshes:
        w = pair_against_portable(gpu, mesh, P, Q)
        print(f"<P={P},Q={Q}> {mesh.nelem} elements: force {w['force']:.2e}  tangent {w['tangent']:.2e} (bound {TOL:.0e})  "
              f"points {w['points']:.2e}  nodal {w['nodal']:.2e} (bound {STRESS_TOL:.0e})")
        assert w["force"] <= TOL and w["tangent"] <= TOL and w["points"] <= STRESS_TOL and w["nodal"] <= STRESS_TOL


@pytest.mark.parametrize("mode", [2, 3])
def test_mask_modes_and_apply_add(gpu, mode):
    """Node n carries pattern n % 8 (bit c: component c constrained): constrained rows of force and tangent are exactly zero; the
    tangent reads constrained entries of dx as zero in mode 3 and as they are in mode 2; ApplyAdd adds and leaves masked rows alone."""
    P, Q = 3, 4
    prob = make(gpu, distorted_box(3, 2, 1), P, Q, "hyperFS", bc=())
    n = prob.lsize()
    pat = np.arange(n // 3) % 8
    mask = ((pat[:, None] >> np.arange(3)[None, :]) & 1).astype(bool).reshape(-1)
    u, dx = state(prob, mode)
    dev, ref = ThermalLoad(prob, 0, ALPHA, theta_field, "hyperFS"), ThermalLoad(prob, 0, ALPHA, theta_field, "hyperFS", portable=True)
    dev.mask = ref.mask = mask
    m8 = mask.astype(np.uint8)
    dev.op_force.set_dirichlet_mask_mode(m8, None, 2)
    dev.op_tangent.set_dirichlet_mask_mode(m8, None, mode)
    U, D = gpu.vector(n).set_array(u), gpu.vector(n).set_array(dx)
    y0 = np.random.default_rng(5).uniform(-1, 1, n)
    for what, apply, want in (("force", lambda y, add: dev.force(U, y, add=add), ref.force_host(u)),
                              ("tangent", lambda y, add: dev.tangent(U, D, y, add=add), ref.tangent_host(u, dx, mask_in=mode == 3))):
        want = np.where(mask, 0.0, want)
        Y = gpu.vector(n).set_value(5.0)
        apply(Y, False)
        assert err(Y.to_numpy(), want) <= TOL and np.all(Y.to_numpy()[mask] == 0.0), what
        Y.set_array(y0)
        apply(Y, True)
        assert err(Y.to_numpy(), y0 + want) <= TOL and np.array_equal(Y.to_numpy()[mask], y0[mask]), what
    other = np.where(mask, 0.0, ref.tangent_host(u, dx, mask_in=mode != 3))
    assert err(other, np.where(mask, 0.0, ref.tangent_host(u, dx, mask_in=mode == 3))) > 1e-3      # the two modes differ on this input
    long = gpu.vector(n + 7).set_value(SENTINEL)
    dev.force(U, long)                                                             # overwrite: masked rows and the tail are zero
    v = long.to_numpy()
    assert np.all(v[:n][mask] == 0.0) and np.all(v[n:] == 0.0)
    long.set_value(SENTINEL)
    dev.force(U, long, add=True)
    v = long.to_numpy()
    assert np.all(v[:n][mask] == SENTINEL) and np.all(v[n:] == SENTINEL)
    dev.destroy(); ref.destroy(); prob.destroy()


def test_recording_sees_a_temperature_rewritten_in_place(gpu):
    """After one eager apply the operators record, and the replay reads the temperature behind the recorded address: theta is the
    active input of the force and a passive field of the tangent."""
    P, Q = 3, 4
    prob = make(gpu, distorted_box(3, 2, 1), P, Q, "hyperFS")
    n = prob.lsize()
    mask = prob.levels[0].mask != 0
    dev, ref = ThermalLoad(prob, 0, ALPHA, theta_field, "hyperFS"), ThermalLoad(prob, 0, ALPHA, theta_field, "hyperFS", portable=True)
    u, dx = state(prob, 17)
    U, D, Yf, Yt = gpu.vector(n).set_array(u), gpu.vector(n).set_array(dx), gpu.vector(n).set_value(0.0), gpu.vector(n).set_value(0.0)
    dev.force(U, Yf); dev.tangent(U, D, Yt)                                  # eager: the transpose map, the row flags, the state
    eager_f, eager_t = Yf.to_numpy().copy(), Yt.to_numpy().copy()
    for v in (D, Yf, Yt, dev.theta_vec, dev.state):
        v.device_pointer()                                                   # on the device before anything is recorded
    g = gpu.capture(lambda: (dev.op_force.apply(dev.theta_vec, Yf), dev.op_tangent.apply(D, Yt)))
    Yf.set_value(0.0); Yt.set_value(0.0); Yf.device_pointer(); Yt.device_pointer()
    g.launch()
    assert np.array_equal(Yf.to_numpy(), eager_f) and np.array_equal(Yt.to_numpy(), eager_t)
    addr = dev.theta_vec.device_pointer()
    new = dev.theta[::-1].copy() * 1.5
    dev.set_theta_values(new); ref.set_theta_values(new)
    assert dev.theta_vec.device_pointer() == addr
    Yf.set_value(0.0); Yt.set_value(0.0); Yf.device_pointer(); Yt.device_pointer()
    g.launch()
    gf, gt = Yf.to_numpy().copy(), Yt.to_numpy().copy()
    assert err(gf, np.where(mask, 0.0, ref.force_host(u))) <= TOL and err(gf, eager_f) > 1e-2
    assert err(gt, np.where(mask, 0.0, ref.tangent_host(u, dx))) <= TOL and err(gt, eager_t) > 1e-2
    dev.force(U, Yf); dev.tangent(U, D, Yt)                                  # ... and they are the bits of an eager apply
    assert np.array_equal(Yf.to_numpy(), gf) and np.array_equal(Yt.to_numpy(), gt)
    g.destroy(); dev.destroy(); ref.destroy(); prob.destroy()


def test_without_a_field_the_kernels_are_the_ones_they_were(gpu):
    prob = make(gpu, distorted_box(3, 1, 1), 3, 4, "hyperFS")
    U = gpu.vector(prob.lsize()).set_array(prob.smooth_state(0.05))
    st = Stress(prob, "hyperFS")
    st.points(U); st.nodal(U)
    assert st.thermal is None and st.kernel_names == {"points": "stress<P=3,Q=4,points>", "nodal": "stress<P=3,Q=4,nodal>"}
    st.destroy(); prob.destroy()


# ---- the lowering: one valid graph and one defective twin per check, on a 2 x 1 x 1 box at P = 2, Q = 2 ------------------------------------
@pytest.fixture(scope="module")
def box(gpu):
    prob = make(gpu, box_mesh(2, 1, 1), 2, 2, "hyperFS", bc=(6,))
    lv = prob.levels[0]
    off = np.asarray(lv.dofmap.offsets(), dtype=np.int32)
    nodes = off // 3
    n = prob.lsize()
    nn = n // 3
    fine = np.array([[(2 * e + a) + 5 * b + 15 * k for k in range(3) for b in range(3) for a in range(3)] for e in (0, 1)], dtype=np.int32)
    s = dict(prob=prob, lv=lv, n=n, nn=nn, ru=lv.Erestrictu, bu=lv.basisu, rq=lv.Erestrictqdi, qdata=lv.qdata,
             rt=gpu.elem_restriction(2, 8, 1, 1, nn, nodes), bt=gpu.basis_lagrange(3, 1, 2, 2, cd.GAUSS),
             theta=gpu.vector(nn).set_value(20.0), theta_short=gpu.vector(nn - 1).set_value(20.0),
             u=gpu.vector(n).set_array(prob.smooth_state(0.05)), u_short=gpu.vector(n - 1).set_value(0.0),
             rt_nc3=gpu.elem_restriction(2, 8, 3, 1, n, off), rt_strided=gpu.strided_restriction(2, 8, 1, 16),
             rt_ne1=gpu.elem_restriction(1, 8, 1, 1, nn, nodes.reshape(-1)[:8]), rt_27=gpu.elem_restriction(2, 27, 1, 1, 45, fine),
             bt_q3=gpu.basis_lagrange(3, 1, 2, 3, cd.GAUSS), bt_lobatto=gpu.basis_lagrange(3, 1, 2, 2, cd.GAUSS_LOBATTO),
             ru2=gpu.elem_restriction(2, 8, 3, 1, n, off), rq_nc9=gpu.strided_restriction(2, 8, 9, 144),
             qdata_short=gpu.vector(159).set_value(0.125),
             rs_pts=gpu.strided_restriction(2, 8, 6, 96))
    yield s
    prob.destroy()


CTX = (0.3, 1.5, ALPHA, 2.0)


def force_graph(gpu, s, rt="rt", bt="bt", rq="rq", qdata="qdata", du="u", ru_du="ru", ctx=CTX, t_size=1, t_mode=cd.EVAL_INTERP, q_size=10,
                v_mode=cd.EVAL_GRAD, no_du=False, du_vec=None):
    qf = gpu.qfunction("ThermalForce", source="qfunctions/thermal.h:ThermalForce")
    qf.add_input("theta", t_size, t_mode).add_input("qdata", q_size, cd.EVAL_NONE)
    if not no_du:
        qf.add_input("du", 9, cd.EVAL_GRAD)
    qf.add_output("dv", 9, v_mode)
    if ctx is not None:
        qf.set_context(list(ctx))
    op = gpu.operator(qf)
    op.set_field("theta", s[rt], s[bt] if bt else None, "active")
    op.set_field("qdata", s[rq], None, s[qdata])
    if not no_du:
        op.set_field("du", s[ru_du], s["bu"], "active" if du == "active" else s[du])
    op.set_field("dv", s["ru"], s["bu"], "active")
    return op


def tangent_graph(gpu, s, rt="rt", bt="bt", theta="theta", ctx=CTX, du="u"):
    qf = gpu.qfunction("ThermalTangent", source="qfunctions/thermal.h:ThermalTangent")
    qf.add_input("ddu", 9, cd.EVAL_GRAD).add_input("du", 9, cd.EVAL_GRAD).add_input("theta", 1, cd.EVAL_INTERP)
    qf.add_input("qdata", 10, cd.EVAL_NONE).add_output("dv", 9, cd.EVAL_GRAD)
    qf.set_context(list(ctx))
    op = gpu.operator(qf)
    op.set_field("ddu", s["ru"], s["bu"], "active")
    op.set_field("du", s["ru"], s["bu"], s[du])
    op.set_field("theta", s[rt], s[bt] if bt else None, "active" if theta == "active" else s[theta])
    op.set_field("qdata", s["rq"], None, s["qdata"])
    op.set_field("dv", s["ru"], s["bu"], "active")
    return op


def stress_graph(gpu, s, rt="rt", bt="bt", theta="theta", ctx=CTX[:3], name="HyperFSStressThermal", no_theta=False):
    qf = gpu.qfunction(name, source=f"qfunctions/hyperFS.h:{name}")
    qf.add_input("du", 9, cd.EVAL_GRAD)
    if not no_theta:
        qf.add_input("theta", 1, cd.EVAL_INTERP)
    qf.add_input("qdata", 10, cd.EVAL_NONE).add_output("stress", 6, cd.EVAL_NONE)
    qf.set_context(list(ctx))
    op = gpu.operator(qf)
    op.set_field("du", s["ru"], s["bu"], "active")
    if not no_theta:
        op.set_field("theta", s[rt], s[bt] if bt else None, s[theta])
    op.set_field("qdata", s["rq"], None, s["qdata"])
    op.set_field("stress", s["rs_pts"], None, "active")
    return op


def apply_once(gpu, s, op, vin, nout=None):
    Y = gpu.vector(nout or s["n"]).set_value(SENTINEL)
    try:
        op.apply(vin, Y)
    except cd.CeedError:
        assert np.all(Y.to_numpy() == SENTINEL), "a refused apply wrote into its output"
        raise
    return Y.to_numpy()


def test_valid_graphs_are_lowered_to_the_thermal_modes(gpu, box):
    for name in ("ThermalForce", "ThermalTangent", "LinElasStressThermal", "HyperSSStressThermal", "HyperFSStressThermal", "qfunctions/thermal.h:ThermalForce"):
        assert gpu.has_qfunction(name), name
    op = force_graph(gpu, box)
    y = apply_once(gpu, box, op, box["theta"])
    assert op.kernel_name == "thermal_force<P=2,Q=2>" and np.abs(y).max() > 0
    # a uniform theta in the small-strain model: the load sums to zero over all rows per component (div of a constant test function)
    op0 = force_graph(gpu, box, ctx=(0.3, 1.5, ALPHA, 0.0), no_du=True)
    y0 = apply_once(gpu, box, op0, box["theta"])
    assert np.abs(y0.reshape(-1, 3).sum(axis=0)).max() <= 1e-14 * np.abs(y0).max() and np.abs(y0).max() > 0
    assert op0.kernel_name == "thermal_force<P=2,Q=2>"
    ot = tangent_graph(gpu, box)
    apply_once(gpu, box, ot, gpu.vector(box["n"]).set_value(0.5))
    assert ot.kernel_name == "thermal_tangent<P=2,Q=2>"
    os_ = stress_graph(gpu, box)
    apply_once(gpu, box, os_, box["u"], 96)
    assert os_.kernel_name == "stress<P=2,Q=2,points+thermal>"
    for o in (op, ot):
        with pytest.raises(cd.CeedError, match="provided for the Jacobian operators"):
            o.assemble_diagonal(gpu.vector(box["n"]))
        with pytest.raises(cd.CeedError, match="provided for the Jacobian operators"):
            o.assemble_pointblock_diagonal(gpu.vector(3 * box["n"]))


FORCE_DEFECTS = [
    (dict(t_size=3), "theta must be a 1-component field through INTERP"),
    (dict(t_mode=cd.EVAL_NONE), "theta must be a 1-component field through INTERP"),
    (dict(q_size=9, rq="rq_nc9"), "ThermalForce eval modes must be"),
    (dict(v_mode=cd.EVAL_INTERP), "ThermalForce eval modes must be"),
    (dict(du="active"), "du must be a passive field with a vector of its own, not the active one"),
    (dict(ru_du="ru2"), "du must share dv's restriction and basis"),
    (dict(rt="rt_nc3"), "theta must be on an offsets restriction with 1 component"),
    (dict(rt="rt_strided"), "theta must be on an offsets restriction with 1 component"),
    (dict(rt="rt_ne1"), "theta's restriction must have the element count of u's"),
    (dict(rt="rt_27"), "theta's restriction must have the element size P^3 of u's"),
    (dict(bt="bt_q3"), "theta's basis must have u's P, Q and interp table"),
    (dict(bt="bt_lobatto"), "theta's basis must have u's P, Q and interp table"),
    (dict(bt=None), "theta's basis must have u's P, Q and interp table"),
    (dict(theta_in="theta_short"), "theta vector shorter than its restriction's L-size"),
    (dict(no_du=True), "ThermalForce with the finite-strain model (model 2) needs the displacement field du"),
    (dict(du="u_short"), "du vector shorter than the restriction's L-size"),
    (dict(ctx=None), "needs its context {nu, E, alpha, model}"),
    (dict(ctx=(0.3, 1.5, ALPHA, 3.0)), "the model in the context must be 0 (linElas), 1 (hyperSS) or 2 (hyperFS)"),
    (dict(qdata="qdata_short"), "qdata vector too short"),
]
RUN_TIME = ("theta vector", "ThermalForce with", "du vector", "needs its", "the model in", "qdata vector", "ThermalTangent is")


@pytest.mark.parametrize("defect,message", FORCE_DEFECTS, ids=[m[:40] + "/" + ",".join(d) for d, m in FORCE_DEFECTS])
def test_defective_force_graph_is_refused_before_anything_is_queued(gpu, box, defect, message):
    defect = dict(defect)
    vin = box[defect.pop("theta_in", "theta")]
    op = force_graph(gpu, box, **defect)
    with pytest.raises(cd.CeedError) as ei:
        apply_once(gpu, box, op, vin)
    assert message in str(ei.value), str(ei.value)
    assert "outside the kernel families" in str(ei.value) or message.startswith(RUN_TIME)


OTHER_DEFECTS = [
    ("tangent", dict(ctx=(0.3, 1.5, ALPHA, 0.0)), "ThermalTangent is the tangent of the finite-strain model alone (model 2)"),
    ("tangent", dict(ctx=(0.3, 1.5, ALPHA, 1.0)), "ThermalTangent is the tangent of the finite-strain model alone (model 2)"),
    ("tangent", dict(theta="active"), "theta must be a passive field with a vector of its own, not the active one"),
    ("tangent", dict(rt="rt_nc3"), "theta must be on an offsets restriction with 1 component"),
    ("tangent", dict(bt="bt_lobatto"), "theta's basis must have u's P, Q and interp table"),
    ("tangent", dict(theta="theta_short"), "theta vector shorter than its restriction's L-size"),
    ("tangent", dict(du="u_short"), "du vector shorter than the restriction's L-size"),
    ("stress", dict(no_theta=True), "stress with the thermal term takes (du, theta, qdata) -> stress"),
    ("stress", dict(rt="rt_nc3"), "theta must be on an offsets restriction with 1 component"),
    ("stress", dict(rt="rt_ne1"), "theta's restriction must have the element count of u's"),
    ("stress", dict(bt="bt_q3"), "theta's basis must have u's P, Q and interp table"),
    ("stress", dict(theta="theta_short"), "theta vector shorter than its restriction's L-size"),
    ("stress", dict(ctx=(0.3, 1.5)), "needs its context {nu, E, alpha}"),
]


@pytest.mark.parametrize("which,defect,message", OTHER_DEFECTS, ids=[w + "/" + m[:40] + "/" + ",".join(d) for w, d, m in OTHER_DEFECTS])
def test_defective_tangent_and_stress_graphs_are_refused(gpu, box, which, defect, message):
    if which == "tangent":
        op, vin, nout = tangent_graph(gpu, box, **defect), gpu.vector(box["n"]).set_value(0.5), None
    else:
        op, vin, nout = stress_graph(gpu, box, **defect), box["u"], 96
    with pytest.raises(cd.CeedError) as ei:
        apply_once(gpu, box, op, vin, nout)
    assert message in str(ei.value), str(ei.value)
    assert "outside the kernel families" in str(ei.value) or message.startswith(RUN_TIME)


def test_in_place_and_short_vectors_are_refused(gpu, box):
    n = box["n"]
    ot = tangent_graph(gpu, box)
    v = gpu.vector(n).set_value(SENTINEL)
    with pytest.raises(cd.CeedError, match="in-place"):
        ot.apply(v, v)
    with pytest.raises(cd.CeedError, match="in-place"):
        ot.apply(box["u"], v)                                                  # the state the operator reads
    with pytest.raises(cd.CeedError, match="shorter than the restriction's L-size"):
        ot.apply(gpu.vector(n - 1).set_value(0.0), v)
    with pytest.raises(cd.CeedError, match="shorter than the restriction's L-size"):
        force_graph(gpu, box).apply(box["theta"], gpu.vector(n - 1).set_value(SENTINEL))
    assert np.all(v.to_numpy() == SENTINEL)


# ---- the force-free expansions of the CPU tests on the device: their bounds x 10 ------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3])
def test_free_expansion_on_the_device(gpu, p):
    prob, u, theta = tt.free_expansion_case(gpu, p)
    e = tt.residual_error(gpu, prob, u, theta, "linElas")
    print(f"free expansion on the device, p = {p}: residual / F_int {e:.2e} (bound {10 * tt.FREE_TOL:.0e})")
    assert e <= 10 * tt.FREE_TOL
    prob.destroy()


@pytest.mark.parametrize("p", [2, 3])
def test_linear_field_on_the_device(gpu, p):
    prob, u, theta = tt.linear_field_case(gpu, p)
    e = tt.residual_error(gpu, prob, u, theta, "linElas")
    print(f"linear field on the device, p = {p}: residual / F_int {e:.2e} (bound {10 * tt.FREE_TOL:.0e})")
    assert e <= 10 * tt.FREE_TOL
    prob.destroy()


def test_hyperfs_free_expansion_on_the_device(gpu):
    prob, u, theta, beta = tt.hyperfs_case(gpu)
    e = tt.residual_error(gpu, prob, u, theta, "hyperFS")
    st = Stress(prob, "hyperFS", thermal=dict(alpha=tt.ALPHA, theta=theta))
    assert not st.portable
    se = np.abs(st.points(gpu.vector(prob.lsize()).set_array(u))).max() / (beta * theta)
    print(f"hyperFS free expansion on the device: residual / F_int {e:.2e}, stress / (beta theta) {se:.2e} (bounds {10 * tt.FREE_TOL:.0e})")
    assert e <= 10 * tt.FREE_TOL and se <= 10 * tt.FREE_TOL
    st.destroy(); prob.destroy()


# ---- the three solvers, device against oracle ---------------------------------------------------------------------------------------------
THERMAL = dict(alpha=ALPHA, theta=lambda X: 40.0 * (1.0 + X[:, 1]))


def dyn_bar(c, name):
    """The shape of tests/test_body_loads_gpu.py's dyn_bar."""
    return SolidProblem(c, box_mesh(3, 1, 1, lo=(0.0, -0.2, -0.2), hi=(2.0, 0.2, 0.2)), 2, name, nu=0.3, E=50.0, bc_sides=[6])


def test_static_hyperfs_solve_with_the_follower(gpu, oracle):
    out = {}
    for who, c in (("oracle", oracle), ("device", gpu)):
        prob = dyn_bar(c, "hyperFS")
        sol = NewtonPMG(prob, ksp_rtol=1e-13, snes_rtol=1e-12, thermal=THERMAL)
        assert sol.has_followers()
        sol.solve(num_increments=2)
        assert sol.stats.converged
        out[who] = sol.U.to_numpy()
        if who == "device":
            assert sol.thermal.kernel_name == {"force": "thermal_force<P=3,Q=3>", "tangent": "thermal_tangent<P=3,Q=3>"}
        sol.destroy(); prob.destroy()
    e = err(out["device"], out["oracle"])
    print(f"static hyperFS solve with a thermal follower: device against oracle {e:.2e}, |u| {np.abs(out['oracle']).max():.3e}")
    assert np.abs(out["oracle"]).max() > 1e-2 and e <= 1e-10


@pytest.mark.parametrize("name", ["linElas", "hyperFS"])
def test_one_newmark_step_with_a_thermal_load(gpu, oracle, name):
    out = {}
    for who, c in (("oracle", oracle), ("device", gpu)):
        prob = dyn_bar(c, name)
        v0 = 1e-2 * np.random.default_rng(1).uniform(-1, 1, prob.lsize())
        s = NewmarkPMG(prob, 2.0, 0.05, ksp_rtol=1e-14, snes_rtol=1e-13, thermal=THERMAL)
        s.set_initial(v0=v0)
        assert s.step().converged
        out[who] = (s.U.to_numpy(), s.vn.to_numpy(), s.an.to_numpy())
        if who == "device":
            assert s.thermal.kernel_name["force"] == "thermal_force<P=3,Q=3>"
        s.destroy(); prob.destroy()
    for what, d, o in zip("uva", out["device"], out["oracle"]):
        e = err(d, o)
        print(f"Newmark step with a thermal load, {name}, {what}: device against oracle {e:.2e}")
        assert e <= 1e-10


@pytest.mark.parametrize("name", ["linElas", "hyperFS"])
def test_twenty_explicit_steps_with_a_thermal_load(gpu, oracle, name):
    out = {}
    for who, c in (("oracle", oracle), ("device", gpu)):
        prob = dyn_bar(c, name)
        v0 = 1e-2 * np.random.default_rng(3).uniform(-1, 1, prob.lsize())
        e = ExplicitDynamics(prob, 2.0, dt=2e-3, thermal=THERMAL)
        plain_dt = ExplicitDynamics(prob, 2.0)
        assert e.stable_dt() == plain_dt.stable_dt()                         # no stiffness on the levels: the stable step is what it was
        plain_dt.destroy()
        e.set_initial(v0=v0)
        e.run(20)
        out[who] = (e.x.to_numpy(), e.vh.to_numpy())
        e.destroy(); prob.destroy()
    for what, d, o in zip(("x", "vh"), out["device"], out["oracle"]):
        er = err(d, o)
        print(f"20 explicit steps with a thermal load, {name}, {what}: device against oracle {er:.2e}")
        assert er <= 1e-10
