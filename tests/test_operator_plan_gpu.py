"""The refusals of the operator lowering (csrc/ceed_operator.cpp, op_plan) and of the operator entry points: "no fallback: a graph outside
the kernel families is a loud error" (DESIGN 1), pinned message by message.

Every graph is built through ceed.py on a 2 x 1 x 1 box at P = 2, Q = 2 (the transfers: P_c = 2, P_f = 3).  Per kernel family one valid
graph is applied once -- the family accepts it -- and each defective twin differs from it in ONE thing and must raise CeedError with the
message of the check that thing violates: every distinct message of op_plan, and every disjunct of its shape checks (strided or not,
ncomp, compstride, elemsize, collocated basis or not, nelem of every family's qdata, missing / superfluous state field, field order).
A refused graph launches nothing.  Neither does an energy, diagnostic or forcing operator whose qdata VECTOR is shorter than its elements
need (apply_energy / apply_coord, ceed_op_other.cpp).  Then the refusals the entry points make themselves (masks, overlap split, diagonals, epilogue applies,
split-phase applies, the state kernel; composite operators), and one replay of a recorded apply whose Dirichlet flag arrays were replaced
under it (the operator's device arrays leave through ceed_retire), and a forcing operator whose FIRST apply is recorded: refused, its output
restriction's transpose map being built on the host; after one eager apply the recording replays to the bits of the eager result.

Two branches of op_plan the binding cannot reach are left out:
  * "the basis tables are not centro-symmetric": every basis comes from CeedBasisCreateTensorH1Lagrange, whose tables are;
  * "no kernel family": every QFunction name CeedQFunctionCreateInterior resolves belongs to one of the families (an unknown name is
    refused at creation, test_gpu_parity.py::test_unsupported_graphs_fail_loudly)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from ceedpetscsolid_amd import ceed as cd

pytestmark = pytest.mark.gpu

NONE, INTERP, GRAD, WEIGHT = cd.EVAL_NONE, cd.EVAL_INTERP, cd.EVAL_GRAD, cd.EVAL_WEIGHT
PHYS = [0.3, 1.0]


@pytest.fixture(scope="module")
def o(gpu):
    """The restrictions, bases and vectors of the valid graphs, and the defective stand-ins of each."""
    c = gpu
    # the eight nodes of an element in the tensor order of the bases (x fastest)
    cells = np.array([[(e + a) + 3 * b + 6 * k for k in (0, 1) for b in (0, 1) for a in (0, 1)] for e in (0, 1)], dtype=np.int32)
    fine = np.array([[(2 * e + a) + 5 * b + 15 * k for k in range(3) for b in range(3) for a in range(3)] for e in (0, 1)], dtype=np.int32)
    coords = np.array([[i, j, k] for k in (0, 1) for j in (0, 1) for i in (0, 1, 2)], dtype=np.float64)
    s = SimpleNamespace(c=c, L=c.L)
    # --- the valid pieces
    s.ru = c.elem_restriction(2, 8, 3, 1, 36, cells * 3)                # displacement, P = 2
    s.rx = c.elem_restriction(2, 8, 3, 1, 36, cells * 3)                # coordinates (trilinear)
    s.rf = c.elem_restriction(2, 27, 3, 1, 135, fine * 3)               # the transfers' fine side, P_f = 3
    s.rq = c.strided_restriction(2, 8, 10, 160)                         # qdata at Q = 2
    s.rs = c.strided_restriction(2, 8, 9, 144)                          # stored state at Q = 2
    s.re = c.elem_restriction(2, 8, 1, 1, 12, cells)                    # energy: one value per node
    s.rd = c.elem_restriction(2, 8, 8, 1, 96, cells * 8)                # diagnostic: eight values per node / point
    s.bu = c.basis_lagrange(3, 3, 2, 2, cd.GAUSS)
    s.bx = c.basis_lagrange(3, 3, 2, 2, cd.GAUSS)
    s.be = c.basis_lagrange(3, 1, 2, 2, cd.GAUSS)
    s.bd = c.basis_lagrange(3, 3, 2, 2, cd.GAUSS_LOBATTO)               # diagnostic: points = nodes
    s.bcf = c.basis_lagrange(3, 3, 2, 3, cd.GAUSS_LOBATTO)              # coarse nodes -> fine nodes
    s.x = c.vector(36).set_array(coords.reshape(-1))
    s.qdata, s.gradu = c.vector(160), c.vector(144).set_value(0.0)
    s.u = c.vector(36).set_array(np.linspace(-0.01, 0.01, 36))
    # --- the stand-ins: each wrong in one property
    s.ru_twin = c.elem_restriction(2, 8, 3, 1, 36, cells * 3)           # a restriction of its own
    s.ru_strided = c.strided_restriction(2, 8, 3, 48)                   # not an offsets restriction
    s.ru_nc1 = s.re                                                     # ncomp 1
    s.ru_cs = c.elem_restriction(2, 8, 3, 12, 36, cells)                # compstride 12
    s.ru_ne1 = c.elem_restriction(1, 8, 3, 1, 36, cells[:1] * 3)        # one element
    s.rd_cs = c.elem_restriction(2, 8, 8, 12, 96, cells)                # diagnostic with compstride 12
    s.bu_twin = c.basis_lagrange(3, 3, 2, 2, cd.GAUSS)                  # a basis of its own
    s.b32 = c.basis_lagrange(3, 3, 3, 2, cd.GAUSS)                      # P = 3: elemsize 8 is not P^3, coordinates not trilinear
    s.b23 = c.basis_lagrange(3, 3, 2, 3, cd.GAUSS)                      # Q = 3: qdata / state at Q = 2 do not fit
    s.be23 = c.basis_lagrange(3, 1, 2, 3, cd.GAUSS)
    s.rq_off = c.elem_restriction(2, 8, 10, 1, 160, np.arange(16, dtype=np.int32) * 10)   # qdata through offsets
    s.rq_e27 = c.strided_restriction(2, 27, 10, 540)
    s.rq_nc9 = s.rs
    s.rq_ne1 = c.strided_restriction(1, 8, 10, 80)
    s.rs_off = c.elem_restriction(2, 8, 9, 1, 144, np.arange(16, dtype=np.int32) * 9)
    s.rs_e27 = c.strided_restriction(2, 27, 9, 486)
    s.rs_nc10 = s.rq
    s.qdata_short = c.vector(159).set_value(0.125)                      # one entry short of 2 elements x 10 x Q^3
    return s


# ---------------------------------------------------------------------------------------------------------------------------------
# Graphs as data: {qf, ctx, ins, outs}; a field is [name, size, eval mode, restriction, basis, vector].  The restriction / basis entries
# are attribute names of the fixture (None: the NONE / COLLOCATED sentinel), the vector "active", None or an attribute name.
# ---------------------------------------------------------------------------------------------------------------------------------
def g_setup_geo():
    return dict(qf="SetupGeo", ctx=None, vin="x", vout="qdata",
                ins=[["dx", 9, GRAD, "rx", "bx", "active"], ["weight", 1, WEIGHT, None, "bx", None]],
                outs=[["qdata", 10, NONE, "rq", None, "active"]])


def g_jacobian(qf="HyperFSdF"):
    ins = [["deltadu", 9, GRAD, "ru", "bu", "active"], ["qdata", 10, NONE, "rq", None, "qdata"]]
    if qf != "LinElasdF":
        ins.append(["gradu", 9, NONE, "rs", None, "gradu"])
    return dict(qf=qf, ctx=PHYS, vin="u", vout=36, ins=ins, outs=[["deltadv", 9, GRAD, "ru", "bu", "active"]])


def g_residual():
    return dict(qf="HyperFSF", ctx=PHYS, vin="u", vout=36,
                ins=[["du", 9, GRAD, "ru", "bu", "active"], ["qdata", 10, NONE, "rq", None, "qdata"]],
                outs=[["dv", 9, GRAD, "ru", "bu", "active"], ["gradu", 9, NONE, "rs", "bu", "gradu"]])


def g_prolong():
    return dict(identity=(3, INTERP, NONE), vin="u", vout=135,
                ins=[["input", 3, INTERP, "ru", "bcf", "active"]], outs=[["output", 3, NONE, "rf", None, "active"]])


def g_restrict():
    return dict(identity=(3, NONE, INTERP), vin=135, vout=36,
                ins=[["input", 3, NONE, "rf", None, "active"]], outs=[["output", 3, INTERP, "ru", "bcf", "active"]])


def g_energy():
    return dict(qf="LinElasEnergy", ctx=PHYS, vin="u", vout=12,
                ins=[["du", 9, GRAD, "ru", "bu", "active"], ["qdata", 10, NONE, "rq", None, "qdata"]],
                outs=[["energy", 1, INTERP, "re", "be", "active"]])


def g_diagnostic():
    return dict(qf="LinElasDiagnostic", ctx=PHYS, vin="u", vout=96,
                ins=[["u", 3, INTERP, "ru", "bd", "active"], ["du", 9, GRAD, "ru", "bd", "active"], ["qdata", 10, NONE, "rq", None, "qdata"]],
                outs=[["diagnostic", 8, NONE, "rd", None, "active"]])


def g_force():
    return dict(qf="SetupConstantForce", ctx=[0.0, 0.0, -1.0], vin="x", vout=36,
                ins=[["x", 3, INTERP, "rx", "bx", "active"], ["qdata", 10, NONE, "rq", None, "qdata"]],
                outs=[["force", 3, INTERP, "ru", "bu", "active"]])


def g_true():
    return dict(qf="MMSTrueSoln", ctx=None, vin="x", vout=36,
                ins=[["x", 3, INTERP, "rx", "bx", "active"]], outs=[["true_soln", 3, NONE, "ru", None, "active"]])


GRAPHS = {"setup_geo": g_setup_geo, "jacobian": g_jacobian, "jacobian_linelas": lambda: g_jacobian("LinElasdF"), "residual": g_residual,
          "prolong": g_prolong, "restrict": g_restrict, "energy": g_energy, "diagnostic": g_diagnostic, "force": g_force, "true": g_true}

SIZE, MODE, RSTR, BASIS, VEC = 1, 2, 3, 4, 5


def put(side, i, what, value):
    """the defect: field i of `side` gets `value` for its size / mode / restriction / basis / vector"""
    def f(g):
        g[side][i][what] = value
    return f


def both(*fs):
    def f(g):
        for x in fs:
            x(g)
    return f


def swap(side, i, j):
    def f(g):
        g[side][i], g[side][j] = g[side][j], g[side][i]
    return f


def add(side, field):
    return lambda g: g[side].append(list(field))


def drop(side, i):
    return lambda g: g[side].pop(i)


def unset(side, i):
    return lambda g: g[side][i].append("unset")


def build(o, g):
    """(operator, QFunction) of graph `g`"""
    c = o.c
    if "identity" in g:
        qf = c.qfunction_identity(*g["identity"])
    else:
        qf = c.qfunction(g["qf"])
        for f in g["ins"]:
            qf.add_input(f[0], f[1], f[2])
        for f in g["outs"]:
            qf.add_output(f[0], f[1], f[2])
        if g["ctx"] is not None:
            qf.set_context(g["ctx"])
    op = c.operator(qf)
    for f in g["ins"] + g["outs"]:
        if f[-1] == "unset":
            continue
        vec = f[VEC] if f[VEC] in ("active", None) else getattr(o, f[VEC])
        op.set_field(f[0], getattr(o, f[RSTR]) if f[RSTR] else None, getattr(o, f[BASIS]) if f[BASIS] else None, vec)
    return op, qf


def vectors(o, g):
    return tuple(getattr(o, v) if isinstance(v, str) else o.c.vector(v).set_value(0.0) for v in (g["vin"], g["vout"]))


@pytest.fixture(scope="module")
def qdata(o):
    """the geometric factors every other valid graph reads: the SetupGeo graph, applied"""
    g = g_setup_geo()
    op, qf = build(o, g)
    op.apply(*vectors(o, g))
    assert op.kernel_name.startswith("setup_geo<Q=2>")
    assert np.allclose(o.qdata.to_numpy().reshape(2, 10, 8)[:, 0], 0.125)      # unit cubes, two points per direction: w det J = 1 / 8
    return o.qdata


@pytest.mark.parametrize("name", list(GRAPHS))
def test_the_valid_graph_of_each_family_is_accepted(o, qdata, name):
    g = GRAPHS[name]()
    op, qf = build(o, g)
    vin, vout = vectors(o, g)
    op.apply(vin, vout)
    assert op.kernel_name and np.all(np.isfinite(vout.to_numpy()))
    op.destroy(); qf.destroy()


FUSED_ACTIVE = "active input and output must share one offsets restriction and one basis"
FUSED_QDATA = "qdata must be a strided 10 x Q\\^3 field"
QDATA = "qdata must be strided 10 x Q\\^3"
TRILINEAR = "coordinates must be trilinear \\(P=2\\), 3 interlaced components"
OUTSIDE = "outside the kernel families of /gpu/hip/mi355x: "

# (valid graph, the one defect, the message of the check it violates)
REFUSED = [
    ("jacobian", unset("ins", 1), "operator field 'qdata' not set"),
    ("jacobian", unset("outs", 0), "operator field 'deltadv' not set"),
    # --- the residual / Jacobian family
    ("jacobian", put("ins", 1, MODE, INTERP), OUTSIDE + "unexpected input field"),
    ("jacobian", put("ins", 0, VEC, "u"), OUTSIDE + "unexpected input field"),                 # GRAD, but not the active vector
    ("jacobian", put("outs", 0, MODE, INTERP), OUTSIDE + "unexpected output field"),
    ("jacobian", swap("ins", 0, 1), OUTSIDE + "inputs must be \\(GRAD active, NONE qdata\\[, NONE state\\]\\)"),
    ("jacobian", swap("ins", 1, 2), OUTSIDE + "inputs must be \\(GRAD active"),               # the state before qdata
    ("jacobian", drop("ins", 2), OUTSIDE + "stored-state fields do not match the QFunction"),                              # missing
    ("jacobian_linelas", add("ins", ["gradu", 9, NONE, "rs", None, "gradu"]), OUTSIDE + "stored-state fields do not match"),   # superfluous
    ("jacobian", add("outs", ["gradu_out", 9, NONE, "rs", None, "gradu"]), OUTSIDE + "stored-state fields do not match"),
    ("residual", drop("outs", 1), OUTSIDE + "stored-state fields do not match"),
    ("residual", swap("outs", 0, 1), OUTSIDE + "stored-state fields do not match"),           # the active output is not the first
    ("jacobian", both(put("ins", 0, RSTR, "ru_strided"), put("outs", 0, RSTR, "ru_strided")), OUTSIDE + FUSED_ACTIVE),
    ("jacobian", put("outs", 0, RSTR, "ru_twin"), OUTSIDE + FUSED_ACTIVE),
    ("jacobian", put("outs", 0, BASIS, "bu_twin"), OUTSIDE + FUSED_ACTIVE),
    ("jacobian", both(put("ins", 0, BASIS, None), put("outs", 0, BASIS, None)), OUTSIDE + FUSED_ACTIVE),
    ("jacobian", both(put("ins", 0, RSTR, "ru_nc1"), put("outs", 0, RSTR, "ru_nc1")), OUTSIDE + "active fields must be 3 interlaced components"),
    ("jacobian", both(put("ins", 0, RSTR, "ru_cs"), put("outs", 0, RSTR, "ru_cs")), OUTSIDE + "active fields must be 3 interlaced components"),
    ("jacobian", both(put("ins", 0, BASIS, "b32"), put("outs", 0, BASIS, "b32")), OUTSIDE + "restriction element size is not P\\^3"),
    ("jacobian", put("ins", 1, RSTR, "rq_off"), OUTSIDE + FUSED_QDATA),
    ("jacobian", put("ins", 1, RSTR, "rq_e27"), OUTSIDE + FUSED_QDATA),
    ("jacobian", put("ins", 1, RSTR, "rq_nc9"), OUTSIDE + FUSED_QDATA),
    ("jacobian", put("ins", 1, RSTR, "rq_ne1"), OUTSIDE + FUSED_QDATA),
    ("jacobian", put("ins", 1, RSTR, None), OUTSIDE + FUSED_QDATA),
    ("jacobian", put("ins", 2, RSTR, "rs_off"), OUTSIDE + "state input must be strided 9 x Q\\^3"),
    ("jacobian", put("ins", 2, RSTR, "rs_e27"), OUTSIDE + "state input must be strided 9 x Q\\^3"),
    ("jacobian", put("ins", 2, RSTR, "rs_nc10"), OUTSIDE + "state input must be strided 9 x Q\\^3"),
    ("residual", put("outs", 1, RSTR, "rs_off"), OUTSIDE + "state output must be strided 9 x Q\\^3"),
    ("residual", put("outs", 1, RSTR, "rs_e27"), OUTSIDE + "state output must be strided 9 x Q\\^3"),
    ("residual", put("outs", 1, RSTR, "rs_nc10"), OUTSIDE + "state output must be strided 9 x Q\\^3"),
    # --- SetupGeo
    ("setup_geo", add("ins", ["more", 1, NONE, "rq", None, None]), OUTSIDE + "SetupGeo takes \\(dx, weight\\) -> qdata"),
    ("setup_geo", put("ins", 0, MODE, INTERP), OUTSIDE + "SetupGeo eval modes must be GRAD, WEIGHT -> NONE"),
    ("setup_geo", put("outs", 0, MODE, INTERP), OUTSIDE + "SetupGeo eval modes must be GRAD, WEIGHT -> NONE"),
    ("setup_geo", put("ins", 0, RSTR, "ru_strided"), OUTSIDE + TRILINEAR + " \\(setuplibceed.c:279,339\\)"),
    ("setup_geo", put("ins", 0, RSTR, "rf"), OUTSIDE + TRILINEAR),                             # elemsize 27
    ("setup_geo", put("ins", 0, RSTR, "ru_nc1"), OUTSIDE + TRILINEAR),
    ("setup_geo", put("ins", 0, RSTR, "ru_cs"), OUTSIDE + TRILINEAR),
    ("setup_geo", put("ins", 0, BASIS, None), OUTSIDE + TRILINEAR),
    ("setup_geo", put("ins", 0, BASIS, "b32"), OUTSIDE + TRILINEAR),
    ("setup_geo", put("outs", 0, RSTR, "rq_off"), OUTSIDE + QDATA),
    ("setup_geo", put("outs", 0, RSTR, "rq_nc9"), OUTSIDE + QDATA),
    ("setup_geo", put("outs", 0, RSTR, "rq_e27"), OUTSIDE + QDATA),
    # --- the transfers
    ("prolong", lambda g: g.update(identity=(1, INTERP, NONE)), OUTSIDE + "identity transfer operators carry 3 components"),
    ("prolong", put("ins", 0, RSTR, "ru_strided"), OUTSIDE + "transfer needs offsets restrictions on both sides"),
    ("prolong", put("outs", 0, RSTR, "ru_strided"), OUTSIDE + "transfer needs offsets restrictions on both sides"),
    ("prolong", put("ins", 0, RSTR, "ru_ne1"), OUTSIDE + "transfer needs offsets restrictions on both sides"),
    ("prolong", put("ins", 0, RSTR, "ru_nc1"), OUTSIDE + "3 interlaced components expected"),
    ("restrict", put("outs", 0, RSTR, "ru_nc1"), OUTSIDE + "3 interlaced components expected"),
    ("prolong", put("ins", 0, RSTR, "ru_cs"), OUTSIDE + "3 interlaced components expected"),
    ("restrict", put("outs", 0, RSTR, "ru_cs"), OUTSIDE + "3 interlaced components expected"),
    ("prolong", put("ins", 0, RSTR, "rf"), OUTSIDE + "prolongation sizes"),
    ("prolong", put("outs", 0, RSTR, "ru"), OUTSIDE + "prolongation sizes"),
    ("restrict", put("outs", 0, RSTR, "rf"), OUTSIDE + "restriction sizes"),
    ("restrict", put("ins", 0, RSTR, "ru"), OUTSIDE + "restriction sizes"),
    ("prolong", lambda g: g.update(identity=(3, INTERP, INTERP)), OUTSIDE + "identity operator is neither INTERP->NONE nor NONE->INTERP"),
    ("prolong", put("ins", 0, BASIS, None), OUTSIDE + "identity operator is neither"),
    ("restrict", put("ins", 0, BASIS, "bcf"), OUTSIDE + "identity operator is neither"),
    # --- the energy operator
    ("energy", add("ins", ["more", 1, NONE, "rq", None, None]), OUTSIDE + "energy takes \\(du, qdata\\) -> energy"),
    ("energy", put("ins", 1, SIZE, 9), OUTSIDE + "energy eval modes must be GRAD\\(9\\), NONE\\(10\\) -> INTERP\\(1\\)"),
    ("energy", put("ins", 0, RSTR, "ru_strided"), OUTSIDE + "displacement field"),
    ("energy", put("ins", 0, RSTR, "ru_nc1"), OUTSIDE + "displacement field"),
    ("energy", put("ins", 0, RSTR, "ru_cs"), OUTSIDE + "displacement field"),
    ("energy", put("ins", 0, BASIS, None), OUTSIDE + "displacement field"),
    ("energy", put("ins", 0, BASIS, "b32"), OUTSIDE + "restriction element size is not P\\^3"),
    ("energy", put("ins", 1, RSTR, "rq_off"), OUTSIDE + QDATA),
    ("energy", put("ins", 1, RSTR, "rq_nc9"), OUTSIDE + QDATA),
    ("energy", put("ins", 1, RSTR, "rq_e27"), OUTSIDE + QDATA),
    ("energy", put("outs", 0, RSTR, "ru"), OUTSIDE + "energy field must be a 1-component field on the displacement's nodes and points"),
    ("energy", put("outs", 0, BASIS, "be23"), OUTSIDE + "energy field must be a 1-component field"),
    # --- the diagnostic operator
    ("diagnostic", drop("ins", 0), OUTSIDE + "diagnostic takes \\(u, du, qdata\\) -> diagnostic"),
    ("diagnostic", put("outs", 0, SIZE, 3), OUTSIDE + "diagnostic eval modes must be INTERP\\(3\\), GRAD\\(9\\), NONE\\(10\\) -> NONE\\(8\\)"),
    ("diagnostic", put("ins", 1, BASIS, "bu_twin"), OUTSIDE + "u and du must be the same active field"),
    ("diagnostic", put("ins", 1, VEC, "u"), OUTSIDE + "u and du must be the same active field"),
    ("diagnostic", both(put("ins", 0, RSTR, "ru_strided"), put("ins", 1, RSTR, "ru_strided")), OUTSIDE + "displacement field"),
    ("diagnostic", both(put("ins", 0, RSTR, "ru_cs"), put("ins", 1, RSTR, "ru_cs")), OUTSIDE + "displacement field"),
    ("diagnostic", both(put("ins", 0, BASIS, None), put("ins", 1, BASIS, None)), OUTSIDE + "displacement field"),
    ("diagnostic", both(put("ins", 0, BASIS, "b32"), put("ins", 1, BASIS, "b32")), OUTSIDE + "restriction element size is not P\\^3"),
    ("diagnostic", put("ins", 2, RSTR, "rq_off"), OUTSIDE + QDATA),
    ("diagnostic", put("ins", 2, RSTR, "rq_e27"), OUTSIDE + QDATA),
    ("diagnostic", put("outs", 0, RSTR, "ru"), OUTSIDE + "diagnostic field must be 8 interlaced components collocated with the points"),
    ("diagnostic", put("outs", 0, RSTR, "rd_cs"), OUTSIDE + "diagnostic field must be 8 interlaced components"),
    ("diagnostic", put("outs", 0, BASIS, "bd"), OUTSIDE + "diagnostic field must be 8 interlaced components"),
    # --- the coordinate operators
    ("force", drop("ins", 1), OUTSIDE + "expected \\(x\\[, qdata\\]\\) -> one output"),
    ("true", add("ins", ["qdata", 10, NONE, "rq", None, "qdata"]), OUTSIDE + "expected \\(x\\[, qdata\\]\\) -> one output"),
    ("force", put("ins", 0, MODE, GRAD), OUTSIDE + "x must be 3 components, INTERP"),
    ("true", put("outs", 0, SIZE, 1), OUTSIDE + "x must be 3 components, INTERP"),
    ("force", put("ins", 0, RSTR, "ru_strided"), OUTSIDE + TRILINEAR),
    ("force", put("ins", 0, RSTR, "rf"), OUTSIDE + TRILINEAR),
    ("force", put("ins", 0, RSTR, "ru_nc1"), OUTSIDE + TRILINEAR),
    ("true", put("ins", 0, RSTR, "ru_cs"), OUTSIDE + TRILINEAR),
    ("true", put("ins", 0, BASIS, None), OUTSIDE + TRILINEAR),
    ("true", put("ins", 0, BASIS, "b32"), OUTSIDE + TRILINEAR),
    ("force", put("outs", 0, RSTR, "ru_strided"), OUTSIDE + "output must be an offsets restriction with 3 interlaced components"),
    ("force", put("outs", 0, RSTR, "ru_ne1"), OUTSIDE + "output must be an offsets restriction with 3 interlaced components"),
    ("true", put("outs", 0, RSTR, "ru_cs"), OUTSIDE + "output must be an offsets restriction with 3 interlaced components"),
    ("force", put("ins", 1, MODE, INTERP), OUTSIDE + "forcing takes qdata NONE and gives force INTERP"),
    ("force", put("outs", 0, MODE, NONE), OUTSIDE + "forcing takes qdata NONE and gives force INTERP"),
    ("force", put("ins", 1, RSTR, "rq_off"), OUTSIDE + QDATA),
    ("force", put("ins", 1, RSTR, "rq_nc9"), OUTSIDE + QDATA),
    ("force", put("ins", 1, RSTR, "rq_e27"), OUTSIDE + QDATA),
    ("force", put("outs", 0, BASIS, None), OUTSIDE + "force basis must share the quadrature of the coordinate basis"),
    ("force", put("outs", 0, BASIS, "b23"), OUTSIDE + "force basis must share the quadrature"),
    ("force", put("outs", 0, BASIS, "b32"), OUTSIDE + "force basis must share the quadrature"),
    ("true", put("outs", 0, MODE, INTERP), OUTSIDE + "true solution is collocated on the points of the coordinate basis"),
    ("true", put("outs", 0, BASIS, "bu"), OUTSIDE + "true solution is collocated on the points"),
    ("true", put("outs", 0, RSTR, "rf"), OUTSIDE + "true solution is collocated on the points"),
    # --- qdata of fewer elements than the active field (behind the rest: the ids above stay what they were)
    ("energy", put("ins", 1, RSTR, "rq_ne1"), OUTSIDE + QDATA),
    ("diagnostic", put("ins", 2, RSTR, "rq_ne1"), OUTSIDE + QDATA),
    ("force", put("ins", 1, RSTR, "rq_ne1"), OUTSIDE + QDATA),
]


@pytest.mark.parametrize("i", range(len(REFUSED)), ids=[f"{i}-{r[0]}" for i, r in enumerate(REFUSED)])
def test_a_graph_with_one_defect_is_refused_with_the_message_of_its_check(o, qdata, i):
    name, defect, message = REFUSED[i]
    g = GRAPHS[name]()
    defect(g)
    op, qf = build(o, g)
    vin, vout = vectors(o, g)
    before = vout.to_numpy()
    with pytest.raises(cd.CeedError, match=message):
        op.apply(vin, vout)
    assert np.array_equal(vout.to_numpy(), before)          # nothing was launched
    op.destroy(); qf.destroy()


# (valid graph, its qdata input): the kernels read nelem * 10 * Q^3 entries of the passive vector, whatever its length
SHORT_QDATA = [("energy", 1), ("diagnostic", 2), ("force", 1)]


@pytest.mark.parametrize("name,i", SHORT_QDATA, ids=[n for n, _ in SHORT_QDATA])
def test_a_qdata_vector_shorter_than_the_elements_need_is_refused(o, qdata, name, i):
    g = GRAPHS[name]()
    put("ins", i, VEC, "qdata_short")(g)                    # the graph is the valid one: op_plan accepts it
    op, qf = build(o, g)
    vin, vout = vectors(o, g)
    vout.set_value(-7.0)
    with pytest.raises(cd.CeedError, match="qdata vector too short"):
        op.apply(vin, vout)
    assert np.all(vout.to_numpy() == -7.0)                  # refused before the output was zeroed: nothing was launched
    with pytest.raises(cd.CeedError, match="qdata vector too short"):
        op.apply_add(vin, vout)
    assert np.all(vout.to_numpy() == -7.0)
    op.destroy(); qf.destroy()


def _refused(L, message, rc):
    with pytest.raises(cd.CeedError, match=message):
        L.chk(rc)


def test_the_entry_points_refuse_the_operators_they_are_not_provided_for(o, qdata):
    L, lib, c = o.L, o.L.lib, o.c
    ops = {k: build(o, GRAPHS[k]())[0] for k in ("setup_geo", "jacobian", "residual", "prolong")}
    X, Y, T, W = (c.vector(36).set_value(0.0) for _ in range(4))
    D, B9 = c.vector(36).set_value(0.0), c.vector(108)
    mask = np.zeros(36, dtype=np.uint8)
    with pytest.raises(cd.CeedError, match="this operator takes no Dirichlet mask"):
        ops["setup_geo"].set_dirichlet_mask(mask)
    with pytest.raises(cd.CeedError, match="overlap split is provided for the residual / Jacobian operators"):
        ops["prolong"].set_overlap_split(1, mask)
    res, jac = ops["residual"], ops["jacobian"]
    with pytest.raises(cd.CeedError, match="diagonal assembly is provided for the Jacobian operators"):
        res.assemble_diagonal(D)
    with pytest.raises(cd.CeedError, match="point-block diagonal assembly is provided for the Jacobian operators"):
        res.assemble_pointblock_diagonal(B9)
    _refused(L, "CeedXOperatorApplyResidual is provided for the Jacobian operators", lib.CeedXOperatorApplyResidual(res.h, X.h, T.h, Y.h, W.h))
    _refused(L, "CeedXOperatorApplyChebyshev is provided for the Jacobian operators",
             lib.CeedXOperatorApplyChebyshev(res.h, X.h, T.h, Y.h, W.h, None, D.h, D.h, C.c_double(1.0), C.c_double(0.0), 0))
    with pytest.raises(cd.CeedError, match="split-phase apply needs CeedXOperatorSetOverlapSplit and overwrite mode"):
        res.apply_phase(X, Y, 0)                             # a residual operator has split phases too, once the split is set
    with pytest.raises(cd.CeedError, match="split-phase apply"):
        jac.apply_phase(X, Y, 2)
    with pytest.raises(cd.CeedError, match="split-phase apply"):
        ops["prolong"].apply_phase(X, Y, 0)
    with pytest.raises(cd.CeedError, match="CeedXOperatorApplyState is provided for the residual operators"):
        jac.apply_state(X)
    assert np.all(W.to_numpy() == 0.0) and np.all(D.to_numpy() == 0.0)
    for op in ops.values():
        op.destroy()


def test_a_composite_operator_is_refused_by_every_entry_point_but_the_apply(o, qdata):
    L, lib, c = o.L, o.L.lib, o.c
    jac = build(o, g_jacobian())[0]
    comp, imm = C.c_void_p(), C.c_void_p(o.L.REQUEST_IMMEDIATE)
    L.chk(lib.CeedCompositeOperatorCreate(c.h, C.byref(comp)))
    L.chk(lib.CeedCompositeOperatorAddSub(comp, jac.h))
    X, Y, T, W = (c.vector(36).set_value(0.0) for _ in range(4))
    mask = np.zeros(36, dtype=np.uint8)
    pm = mask.ctypes.data_as(C.POINTER(C.c_ubyte))
    _refused(L, "not a composite operator", lib.CeedCompositeOperatorAddSub(jac.h, jac.h))
    _refused(L, "cannot set a field on a composite operator", lib.CeedOperatorSetField(comp, b"qdata", o.rq.h, C.c_void_p(L.BASIS_COLLOCATED), o.qdata.h))
    _refused(L, "set the mask on the sub-operators", lib.CeedXOperatorSetDirichletMask(comp, cd.MEM_HOST, pm, cd.c_int(36)))
    _refused(L, "sub-operators", lib.CeedXOperatorSetOverlapSplit(comp, cd.c_int(1), pm, cd.c_int(36)))
    _refused(L, "composite operator", lib.CeedOperatorLinearAssembleDiagonal(comp, Y.h, imm))
    _refused(L, "composite operator", lib.CeedOperatorLinearAssemblePointBlockDiagonal(comp, c.vector(108).h, imm))
    _refused(L, "composite operator", lib.CeedXOperatorApplyState(comp, X.h))
    _refused(L, "composite operator", lib.CeedXOperatorApplyPhase(comp, X.h, Y.h, C.c_int(0)))
    _refused(L, "composite operator", lib.CeedXOperatorApplyWithHalo(comp, X.h, Y.h, None))
    _refused(L, "composite operator", lib.CeedXOperatorApplyResidual(comp, X.h, T.h, Y.h, W.h))
    _refused(L, "composite operator", lib.CeedXOperatorApplyChebyshev(comp, X.h, T.h, Y.h, W.h, None, T.h, T.h, C.c_double(1.0), C.c_double(0.0), 0))
    # the apply itself is provided: the sum of the sub-operators' applies
    X.set_array(np.linspace(-1, 1, 36))
    L.chk(lib.CeedOperatorApply(comp, X.h, Y.h, imm))
    jac.apply(X, W)
    assert np.allclose(Y.to_numpy(), W.to_numpy(), rtol=1e-13, atol=0.0) and np.any(W.to_numpy() != 0.0)
    L.chk(lib.CeedOperatorDestroy(C.byref(comp)))
    jac.destroy()


def test_a_recorded_apply_replays_after_its_mask_was_set_again(o, qdata):
    """The flagged offsets and the node flags a recorded apply reads are parked, not freed, when the mask is set again while the graph
    lives: the replay gives the bits of the eager apply, before and after the new arrays exist."""
    c = o.c
    op = build(o, g_jacobian())[0]
    mask = np.zeros(36, dtype=np.uint8)
    mask[:12] = 1                                            # four nodes, all components
    X, Y = c.vector(36).set_array(np.linspace(-1, 1, 36)), c.vector(36)
    op.set_dirichlet_mask(mask)
    op.apply(X, Y)
    eager = Y.to_numpy()
    assert np.any(eager[12:] != 0.0)
    graph = c.capture(lambda: op.apply(X, Y))
    try:
        op.set_dirichlet_mask(mask)                          # new arrays, same content; the old ones are what the graph reads
        Y.set_value(-7.0)
        graph.launch()
        assert np.array_equal(Y.to_numpy(), eager)
        op.apply(X, Y)                                       # the new arrays come into being
        assert np.array_equal(Y.to_numpy(), eager)
        Y.set_value(-7.0)
        graph.launch()
        assert np.array_equal(Y.to_numpy(), eager)
    finally:
        graph.destroy()
    op.destroy()


FIRST_APPLY = "first apply of an operator during graph capture: its restriction's transpose map is built on the host; apply the operator once before recording"


def _force_on_a_fresh_restriction(o):
    """the valid forcing graph with an output restriction of its own: no operator has built its transpose map"""
    cells = np.array([[(e + a) + 3 * b + 6 * k for k in (0, 1) for b in (0, 1) for a in (0, 1)] for e in (0, 1)], dtype=np.int32)
    o.ru_fresh = o.c.elem_restriction(2, 8, 3, 1, 36, cells * 3)
    g = g_force()
    put("outs", 0, RSTR, "ru_fresh")(g)
    return build(o, g)[0], o.c.vector(36)


def test_a_first_apply_of_a_forcing_operator_is_refused_while_recording(o, qdata):
    op, Y = _force_on_a_fresh_restriction(o)
    Y.set_value(-7.0)
    with pytest.raises(cd.CeedError, match=FIRST_APPLY):
        o.c.capture(lambda: op.apply(o.x, Y))
    assert np.all(Y.to_numpy() == -7.0)                      # nothing was recorded or launched
    op.apply(o.x, Y)                                         # the Ceed records no longer: an eager apply goes through
    assert np.any(Y.to_numpy() != 0.0)
    op.destroy()


def test_a_forcing_operator_applied_once_records_and_replays_to_the_bit(o, qdata):
    op, Y = _force_on_a_fresh_restriction(o)
    op.apply(o.x, Y)
    eager = Y.to_numpy()
    assert np.any(eager != 0.0)
    graph = o.c.capture(lambda: op.apply(o.x, Y))
    try:
        for _ in range(2):
            Y.set_value(-7.0)
            graph.launch()
            assert np.array_equal(Y.to_numpy(), eager)
    finally:
        graph.destroy()
    op.destroy()
