"""Stress recovery on the device (csrc/kernels_stress.hip, op_plan's PLAN_STRESS, postprocess.Stress) against its portable NumPy form:
every instantiated (P, Q) with the three models and both modes, bits, flags and boundary values, another numbering, the virtual work
against the device's residual, every refusal of the lowering, and the device reduction.  The bound of the comparisons is the project's
operator parity bound, 1e-10 of the largest |sigma| entry of the case."""
import numpy as np
import pytest

from _stress_common import MODELS, smooth_field, virtual_work
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.mesh import box_mesh, hollow_cylinder_mesh, scramble_mesh
from ceedpetscsolid_amd.postprocess import STRESS_QF, Stress
from ceedpetscsolid_amd.solid import SolidProblem

pytestmark = pytest.mark.gpu

PAIRS = [(P, Q) for P in range(2, 9) for Q in range(P, 9)]          # the 28 pairs of CPS_DIAG_PQ
TOL = 1e-10
WORST = {}                                                          # (model, mode) -> worst relative error seen (printed by the last sweep test)
SENTINEL = -3.25


def moved_box(nx, ny, nz, seed=3, amp=0.04):
    """box_mesh with its vertices moved off the affine grid"""
    m = box_mesh(nx, ny, nz)
    m.coords += amp / max(nx, ny, nz) * np.random.default_rng(seed).uniform(-1, 1, m.coords.shape)
    return m


def make(ceed, mesh, P, Q, model="linElas", **kw):
    return SolidProblem(ceed, mesh, P - 1, model, nu=0.3, E=1.0, multigrid="none", qextra=Q - P, **kw)


def compare(gpu, prob, P, Q, x=None, models=MODELS):
    """Device against portable, the three models and both modes on one problem (the Stress objects take their model themselves)."""
    dm = prob.levels[prob.fine].dofmap
    x = smooth_field(dm.node_coords, 0.02) if x is None else x
    X = gpu.vector(prob.lsize()).set_array(x)
    for model in models:
        dev, ref = Stress(prob, model), Stress(prob, model, portable=True)
        assert not dev.portable and ref.portable
        pts, nod = dev.points(X), dev.nodal(X)
        assert dev.kernel_names == {"points": f"stress<P={P},Q={Q},points>", "nodal": f"stress<P={P},Q={Q},nodal>"}
        wp, wn = ref.points(X), ref.nodal(X)
        scale = np.abs(wp).max()
        e_pts, e_nod = np.abs(pts - wp).max() / scale, np.abs(nod - wn).max() / scale
        e_vol = np.abs(dev.nodal_volume() - ref.nodal_volume()).max() / ref.nodal_volume().max()
        for mode, e in (("points", e_pts), ("nodal", max(e_nod, e_vol))):
            WORST[(model, mode)] = max(WORST.get((model, mode), 0.0), e)
        print(f"stress<P={P},Q={Q}> {model} on {prob.mesh.nelem} elements: points {e_pts:.2e}  nodal {e_nod:.2e}  volume {e_vol:.2e}")
        assert e_pts <= TOL and e_nod <= TOL and e_vol <= TOL
        dev.destroy(); ref.destroy()
    X.destroy()


@pytest.mark.parametrize("P,Q", PAIRS)
def test_sweep_against_the_portable_form(gpu, P, Q):
    """17 moved elements in a row (a multiple of no packing 16, 8, 4, 2: every grid has a partial last workgroup) and the 12 curved
    elements of the cylinder; a single element at three pairs."""
    assert len(PAIRS) == 28
    meshes = [moved_box(17, 1, 1), hollow_cylinder_mesh(1, 6, 2)]
    if (P, Q) in ((2, 2), (5, 5), (8, 8)):
        meshes.append(moved_box(1, 1, 1))
    for mesh in meshes:
        prob = make(gpu, mesh, P, Q)
        compare(gpu, prob, P, Q)
        prob.destroy()


def test_worst_error_per_family():
    print("worst error against the portable form, of max |sigma|:", {f"{m}/{k}": f"{e:.2e}" for (m, k), e in sorted(WORST.items())})
    assert len(WORST) == 6 and all(e <= TOL for e in WORST.values())


def test_overwrite_and_repeat(gpu):
    prob = make(gpu, moved_box(3, 2, 1), 3, 4, "hyperFS")
    X = gpu.vector(prob.lsize()).set_array(smooth_field(prob.levels[0].dofmap.node_coords, 0.02))
    st = Stress(prob, "hyperFS")
    out = []
    for _ in range(2):
        for v in (st.spts, st.snod):
            v.t.fill_(float("nan"))
            v.touched()
        out.append((st.points(X), st.nodal(X), st.nodal_volume()))
    for a, b in zip(*out):
        assert np.all(np.isfinite(a)) and np.abs(a).max() > 0 and np.array_equal(a, b)
    # a longer output vector: the points apply stores its [nelem][6][Q^3] entries and nothing else; the nodal sum, in overwrite mode,
    # zeroes a vector longer than the L-size first, and leaves it alone in add mode
    npts, nnod = st.spts.n, st.snod.n
    long = gpu.vector(npts + 5).set_value(SENTINEL)
    st.op_pts.apply(X, long)
    assert np.array_equal(long.to_numpy()[:npts], out[0][0].reshape(-1)) and np.all(long.to_numpy()[npts:] == SENTINEL)
    sums = gpu.vector(nnod)
    st.op_nod.apply(X, sums)
    long = gpu.vector(nnod + 5).set_value(SENTINEL)
    st.op_nod.apply(X, long)
    assert np.array_equal(long.to_numpy()[:nnod], sums.to_numpy()) and np.all(long.to_numpy()[nnod:] == 0.0)
    long.set_value(SENTINEL)
    st.op_nod.apply_add(X, long)
    assert np.array_equal(long.to_numpy()[:nnod], SENTINEL + sums.to_numpy()) and np.all(long.to_numpy()[nnod:] == SENTINEL)
    st.destroy(); prob.destroy()


def test_flags_are_stripped_and_boundary_values_are_read(gpu):
    """The same mesh with and without constraints on the same vector, whose constrained entries are not zero: bit for bit."""
    mesh = moved_box(3, 2, 2)
    res = []
    for bc in ([1, 6], None):
        prob = make(gpu, mesh, 3, 3, "hyperSS", bc_sides=bc)
        lv = prob.levels[0]
        x = smooth_field(lv.dofmap.node_coords, 0.02)
        if bc:
            assert (lv.mask != 0).any() and np.abs(x[lv.mask != 0]).min() > 0
        X = gpu.vector(prob.lsize()).set_array(x)
        Y = gpu.vector(prob.lsize())
        prob.form_residual(X, Y)                                   # the masked operators run first: their flagged offsets exist
        st = Stress(prob, "hyperSS")
        res.append((st.points(X), st.nodal(X)))
        st.destroy(); prob.destroy()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def test_scrambled_numbering(gpu):
    mesh = scramble_mesh(moved_box(3, 2, 2), seed=5, order=True, orient=True)
    prob = make(gpu, mesh, 4, 5)
    compare(gpu, prob, 4, 5)
    prob.destroy()


@pytest.mark.parametrize("model", MODELS)
def test_virtual_work_of_the_device_stress_is_the_device_residual(gpu, model):
    prob = make(gpu, hollow_cylinder_mesh(1, 6, 2), 3, 4, model, bc_sides=[998])
    lv = prob.levels[0]
    n = prob.lsize()
    x = smooth_field(lv.dofmap.node_coords, 0.01)
    X, R = gpu.vector(n).set_array(x), gpu.vector(n)
    prob.form_residual(X, R)
    r = R.to_numpy()
    st = Stress(prob, model)
    vw = virtual_work(Stress(prob, model, portable=True), x, st.points(X))
    free = lv.mask == 0
    err = np.abs(vw - r)[free].max() / np.abs(r).max()
    print(f"{model}: |virtual work of the device stress - device residual| / max |residual| = {err:.2e}")
    assert err <= TOL
    st.destroy(); prob.destroy()


def test_max_von_mises_is_the_host_reduction_of_nodal(gpu):
    prob = make(gpu, hollow_cylinder_mesh(1, 6, 2), 3, 3, "hyperFS")
    X = gpu.vector(prob.lsize()).set_array(smooth_field(prob.levels[0].dofmap.node_coords, 0.01))
    st = Stress(prob, "hyperFS")
    t = st.nodal(X, numpy=False)
    assert t.device.type == "cuda" and st.points(X, numpy=False).device.type == "cuda"
    vm = Stress.von_mises(st.nodal(X))
    value, node = st.max_von_mises(X)
    assert value == vm.max() and node == int(vm.argmax()) and value > 0
    st.destroy(); prob.destroy()


# ---- the lowering: one valid graph per mode and one defective twin per check, on a 2 x 1 x 1 box at P = 2, Q = 2 ---------------------
@pytest.fixture(scope="module")
def box(gpu):
    prob = make(gpu, box_mesh(2, 1, 1), 2, 2)
    lv = prob.levels[0]
    off = np.asarray(lv.dofmap.offsets(), dtype=np.int32)
    node = (off // 3).reshape(-1)
    nn = lv.dofmap.nnodes
    assert nn == 12
    fine = np.array([[(2 * e + a) + 5 * b + 15 * k for k in range(3) for b in range(3) for a in range(3)] for e in (0, 1)], dtype=np.int32)
    s = dict(prob=prob, lv=lv, n=prob.lsize(), nn=nn,
             ru=lv.Erestrictu, bu=lv.basisu, rq=lv.Erestrictqdi, qdata=lv.qdata,
             rp=gpu.strided_restriction(2, 8, 6, 96),
             rn=gpu.elem_restriction(2, 8, 7, 1, 7 * nn, node * 7), bn=gpu.basis_lagrange(3, 7, 2, 2, cd.GAUSS),
             r_nc1=gpu.elem_restriction(2, 8, 1, 1, nn, node),
             b32=gpu.basis_lagrange(3, 3, 3, 2, cd.GAUSS), r27=gpu.elem_restriction(2, 27, 3, 1, 135, fine * 3),
             rq_nc9=gpu.strided_restriction(2, 8, 9, 144), rq_ne1=gpu.strided_restriction(1, 8, 10, 80),
             rp_nc5=gpu.strided_restriction(2, 8, 5, 80), rp_ne1=gpu.strided_restriction(1, 8, 6, 48),
             rp_es27=gpu.strided_restriction(2, 27, 6, 324),
             rp_off=gpu.elem_restriction(2, 8, 6, 1, 6 * nn, node * 6),
             rn_nc6=gpu.elem_restriction(2, 8, 6, 1, 6 * nn, node * 6), rn_cs=gpu.elem_restriction(2, 8, 7, nn, 7 * nn, node),
             rn_ne1=gpu.elem_restriction(1, 8, 7, 1, 7 * nn, node[:8] * 7), rn_es27=gpu.elem_restriction(2, 27, 7, 1, 7 * 45, fine * 7),
             rn_strided=gpu.strided_restriction(2, 8, 7, 112),
             bn_p3=gpu.basis_lagrange(3, 7, 3, 2, cd.GAUSS), bn_q3=gpu.basis_lagrange(3, 7, 2, 3, cd.GAUSS),
             bn_gll=gpu.basis_lagrange(3, 7, 2, 2, cd.GAUSS_LOBATTO),
             qdata_short=gpu.vector(159).set_value(0.125), passive=gpu.vector(7 * 45).set_value(0.0))
    yield s
    prob.destroy()


def graph(gpu, s, nodal, name="HyperFSStress", ru="ru", bu="bu", rq="rq", qdata="qdata", ro=None, bo="default", ctx=(0.3, 1.0),
          du_mode=cd.EVAL_GRAD, du_size=9, q_size=10, o_mode=None, o_size=None, extra_input=False, passive_du=False, passive_out=False):
    qf = gpu.qfunction(name, source=f"qfunctions/{STRESS_QF['hyperFS'][0]}:{name}")
    qf.add_input("du", du_size, du_mode).add_input("qdata", q_size, cd.EVAL_NONE)
    if extra_input:
        qf.add_input("more", 3, cd.EVAL_INTERP)
    qf.add_output("stress", o_size or (7 if nodal else 6), o_mode if o_mode is not None else (cd.EVAL_INTERP if nodal else cd.EVAL_NONE))
    if ctx is not None:
        qf.set_context(list(ctx))
    op = gpu.operator(qf)
    op.set_field("du", s[ru], s[bu], s["passive"] if passive_du else "active")
    op.set_field("qdata", s[rq], None, s[qdata] if qdata else "active")
    if extra_input:
        op.set_field("more", s[ru], s[bu], "active")
    basis = (s["bn"] if nodal else None) if bo == "default" else (s[bo] if bo else None)
    op.set_field("stress", s[ro or ("rn" if nodal else "rp")], basis, s["passive"] if passive_out else "active")
    return op


def apply_once(gpu, s, op, nodal, nin=None, nout=None, add=False):
    X = gpu.vector(nin or s["n"]).set_array(np.linspace(0.0, 0.05, nin or s["n"]))
    Y = gpu.vector(nout or (7 * s["nn"] if nodal else 96)).set_value(SENTINEL)
    try:
        (op.apply_add if add else op.apply)(X, Y)
    except cd.CeedError:
        assert np.all(Y.to_numpy() == SENTINEL)           # refused before anything is queued
        raise
    return Y.to_numpy()


def test_names_and_valid_graphs(gpu, box):
    for name in ("LinElasStress", "HyperSSStress", "HyperFSStress"):
        assert gpu.has_qfunction(name) and gpu.has_qfunction(f"qfunctions/x.h:{name}")
    assert not gpu.has_qfunction("Stress")
    for nodal, kname in ((False, "stress<P=2,Q=2,points>"), (True, "stress<P=2,Q=2,nodal>")):
        op = graph(gpu, box, nodal)
        y = apply_once(gpu, box, op, nodal)
        assert op.kernel_name == kname and np.all(np.isfinite(y)) and np.all(y != SENTINEL)
    assert abs(y.reshape(-1, 7)[:, 6].sum() - 1.0) < 1e-13          # the nodal volumes sum to the box's


P, N = False, True
DEFECTS = [
    (P, dict(extra_input=True), "stress takes (du, qdata) -> stress"),
    (P, dict(du_mode=cd.EVAL_INTERP, du_size=3), "stress eval modes must be GRAD(9), NONE(10) -> NONE(6) at the points or INTERP(7) at the nodes"),
    (P, dict(q_size=9, rq="rq_nc9"), "stress eval modes must be"),
    (P, dict(o_size=5, ro="rp_nc5"), "stress eval modes must be"),
    (N, dict(o_size=6, ro="rn_nc6"), "stress eval modes must be"),
    (P, dict(o_mode=cd.EVAL_INTERP), "stress eval modes must be"),
    (P, dict(passive_du=True), "du must be the active input of a stress operator"),
    (N, dict(passive_out=True), "stress must be the active output"),
    (P, dict(ru="r_nc1"), "displacement field"),
    (P, dict(bu="b32"), "restriction element size is not P^3"),
    (P, dict(rq="rq_ne1"), "qdata must be strided 10 x Q^3"),
    (P, dict(ru="r27", bu="b32"), "the stress kernel needs P <= Q"),
    (P, dict(ro="rp_nc5"), "stress at the points must be a strided 6 x Q^3 field"),
    (P, dict(ro="rp_ne1"), "stress at the points must be a strided 6 x Q^3 field"),
    (P, dict(ro="rp_es27"), "stress at the points must be a strided 6 x Q^3 field"),
    (P, dict(ro="rp_off"), "stress at the points must be a strided 6 x Q^3 field"),
    (P, dict(bo="bn"), "stress at the points is collocated"),
    (N, dict(ro="rn_nc6"), "nodal stress must be an offsets restriction with 7 interlaced components"),
    (N, dict(ro="rn_cs"), "nodal stress must be an offsets restriction with 7 interlaced components"),
    (N, dict(ro="rn_ne1"), "nodal stress must be an offsets restriction with 7 interlaced components"),
    (N, dict(ro="rn_es27"), "nodal stress must be an offsets restriction with 7 interlaced components"),
    (N, dict(ro="rn_strided"), "nodal stress must be an offsets restriction with 7 interlaced components"),
    (N, dict(bo="bn_p3"), "nodal stress basis must have the displacement basis's P, Q and interp table"),
    (N, dict(bo="bn_q3"), "nodal stress basis must have"),
    (N, dict(bo="bn_gll"), "nodal stress basis must have"),
    (N, dict(bo=None), "nodal stress basis must have"),
    (P, dict(ctx=None), "needs its Physics context"),
    (N, dict(qdata="qdata_short"), "qdata vector too short"),
    (P, dict(qdata=None), "qdata needs a passive vector"),
]


@pytest.mark.parametrize("nodal,defect,message", DEFECTS, ids=[("nodal/" if n else "points/") + m[:36] + "/" + ",".join(f"{k}={v}" for k, v in d.items()) for n, d, m in DEFECTS])
def test_defective_twin_is_refused(gpu, box, nodal, defect, message):
    op = graph(gpu, box, nodal, **defect)
    nin = 135 if defect.get("ru") == "r27" else None
    with pytest.raises(cd.CeedError) as ei:
        apply_once(gpu, box, op, nodal, nin, 7 * 45 if nodal else None)
    assert message in str(ei.value), str(ei.value)
    assert "outside the kernel families" in str(ei.value) or message.startswith(("needs", "qdata vector", "qdata needs"))


def test_vector_refusals(gpu, box):
    s = box
    for nodal, nout in ((P, 95), (N, 7 * s["nn"] - 1)):
        op = graph(gpu, s, nodal)
        with pytest.raises(cd.CeedError, match="stress vector too short"):
            apply_once(gpu, s, op, nodal, nout=nout)
        with pytest.raises(cd.CeedError, match="displacement vector too short"):
            apply_once(gpu, s, op, nodal, nin=s["n"] - 1)
        v = gpu.vector(7 * 45).set_value(0.0)
        with pytest.raises(cd.CeedError, match="in-place"):
            op.apply(v, v)
    with pytest.raises(cd.CeedError, match="stored, not summed"):
        apply_once(gpu, s, graph(gpu, s, P), P, add=True)
    op = graph(gpu, s, N)
    with pytest.raises(cd.CeedError, match="is provided for the"):
        op.apply_state(gpu.vector(s["n"]).set_value(0.0))
    with pytest.raises(cd.CeedError, match="takes no Dirichlet mask"):
        op.set_dirichlet_mask(np.zeros(s["n"], dtype=np.uint8) + 1)


def test_first_nodal_apply_during_capture_is_refused_then_replays_to_the_eager_bits(gpu, box):
    s = box
    node = (np.asarray(s["lv"].dofmap.offsets(), dtype=np.int32) // 3).reshape(-1)
    s2 = dict(s, rn=gpu.elem_restriction(2, 8, 7, 1, 7 * s["nn"], node * 7))        # a restriction no operator has applied: no transpose map yet
    op = graph(gpu, s2, N)
    X, Y = gpu.vector(s["n"]).set_array(np.linspace(0.0, 0.05, s["n"])), gpu.vector(7 * s["nn"]).set_value(SENTINEL)
    X.device_pointer(); Y.device_pointer()                                          # on the device before anything is recorded
    with pytest.raises(cd.CeedError, match="apply the operator once before recording"):
        gpu.capture(lambda: op.apply(X, Y))
    assert np.all(Y.to_numpy() == SENTINEL)
    op.apply(X, Y)
    eager = Y.to_numpy().copy()
    assert np.abs(eager).max() > 0
    Y.device_pointer()
    g = gpu.capture(lambda: op.apply(X, Y))
    Y.set_value(0.0)
    g.launch()
    assert np.array_equal(Y.to_numpy(), eager)
    g.destroy()
