#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY -- generate tests/golden/qfunctions.npz and tests/golden/qfunctions_edges.npz.

Runs the REFERENCE's own QFunctions (qfunctions/*.h compiled where they lie into
oracle/_ref/libref_qfunctions.so by oracle/Makefile) on seeded inputs and stores
inputs + outputs as plain data.  Needs /root/reference, so it only runs in the
build container; the fixture it writes is committed and travels to the GPU box.

    python oracle/gen_golden.py            # rewrites both fixtures
    python oracle/gen_golden.py edges      # rewrites tests/golden/qfunctions_edges.npz alone (or: qfunctions)

qfunctions.npz holds every QFunction at ONE material, {nu, E} = {0.3, 2.5}, and strains of 0.02.  qfunctions_edges.npz pins the
physics away from there: 15 materials (EDGE_NUS x EDGE_ES, the leading index of every output in the order of edge_groups()) on one shared
set of points whose physical gradients sit closely on both
sides of both range shifts of the finite-strain log series, at 30 % and at 1e-7 (make_edge_inputs); it must stay no larger than
qfunctions.npz, which is why the points are few and shared between the materials.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
QF = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.POINTER(C.c_double)))


def load_table(path, getter):
    lib = C.CDLL(path)
    fn = getattr(lib, getter)
    fn.restype = C.c_void_p
    fn.argtypes = [C.c_char_p]
    return lib, lambda name: QF(fn(name.encode()))


def call_qf(f, ctx, Q, ins, out_sizes):
    ins = [np.ascontiguousarray(a, dtype=np.float64) for a in ins]
    outs = [np.zeros((s, Q)) for s in out_sizes]
    pin = (C.POINTER(C.c_double) * len(ins))(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in ins])
    pout = (C.POINTER(C.c_double) * len(outs))(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in outs])
    ctxa = np.ascontiguousarray(ctx, dtype=np.float64)
    rc = f(ctxa.ctypes.data_as(C.c_void_p), Q, pin, pout)
    assert rc == 0
    return outs


def make_inputs(seed=20261003, Q=96):
    rng = np.random.default_rng(seed)
    # distorted element Jacobians J[d][c] = d x_c / d xi_d (common.h:51, 62-70)
    J = np.zeros((3, 3, Q))
    for i in range(Q):
        h = rng.uniform(0.05, 0.6, size=3)
        A = np.diag(h) + 0.15 * h.mean() * rng.uniform(-1, 1, size=(3, 3))
        J[:, :, i] = A.T
    w = rng.uniform(0.01, 0.3, size=(1, Q))
    # reference-space displacement gradients, |grad u| up to ~0.3 after mapping
    ug = rng.uniform(-1, 1, size=(9, Q)) * 0.02
    dug = rng.uniform(-1, 1, size=(9, Q))
    x = rng.uniform(-0.5, 1.0, size=(3, Q))
    return dict(J=J.reshape(9, Q), w=w, ug=ug, dug=dug, x=x)


EDGE_NUS = (-0.3, 0.0, 0.3, 0.49, 0.4999)
EDGE_ES = (1e-3, 2.5, 2e11)
EDGE_STRETCHES = (-0.25, -0.06, -0.05, 0.059, 0.06, 0.3)     # (1 + s)^6 - 1 on both sides of sqrt(2)/2 - 1 and of sqrt(2) - 1
EDGE_PER_STRETCH, EDGE_LARGE, EDGE_TINY = 2, 1, 2
# the QFunctions of a group: name -> (inputs, sizes of the outputs, their keys); the stored state does not depend on the material and
# is kept once ("gradu": HyperSSF and HyperFSF store the same physical gradient, asserted when the fixture is written)
EDGE_CASES = {
    "LinElasF": (("ug", "SetupGeo.qdata"), (9,), ("LinElasF.dv",)),
    "LinElasdF": (("dug", "SetupGeo.qdata"), (9,), ("LinElasdF.dv",)),
    "HyperSSF": (("ug", "SetupGeo.qdata"), (9, 9), ("HyperSSF.dv", None)),
    "HyperSSdF": (("dug", "SetupGeo.qdata", "gradu"), (9,), ("HyperSSdF.dv",)),
    "HyperFSF": (("ug", "SetupGeo.qdata"), (9, 9), ("HyperFSF.dv", None)),
    "HyperFSdF": (("dug", "SetupGeo.qdata", "gradu"), (9,), ("HyperFSdF.dv",)),
    "LinElasEnergy": (("ug", "SetupGeo.qdata"), (1,), ("LinElasEnergy.energy",)),
    "HyperSSEnergy": (("ug", "SetupGeo.qdata"), (1,), ("HyperSSEnergy.energy",)),
    "HyperFSEnergy": (("ug", "SetupGeo.qdata"), (1,), ("HyperFSEnergy.energy",)),
}


def edge_groups():
    return [(f"nu{nu}_E{E:g}", nu, E) for nu in EDGE_NUS for E in EDGE_ES]


def make_edge_inputs(seed=20261018):
    """Element Jacobians with all nine entries non-zero, and the PHYSICAL gradients wanted at each point: s I + 0.01 random for every s
    of EDGE_STRETCHES (tr e = 3 s for the small-strain model), random of amplitude 0.3, random of amplitude 1e-7."""
    kinds = [f"s={s}" for s in EDGE_STRETCHES for _ in range(EDGE_PER_STRETCH)] + ["large"] * EDGE_LARGE + ["tiny"] * EDGE_TINY
    Q = len(kinds)
    rng = np.random.default_rng(seed)
    J = np.zeros((3, 3, Q))
    for i in range(Q):
        h = rng.uniform(0.05, 0.6, size=3)
        J[:, :, i] = (np.diag(h) + 0.15 * h.mean() * rng.uniform(-1, 1, size=(3, 3))).T
    w = rng.uniform(0.01, 0.3, size=(1, Q))
    g = np.zeros((Q, 3, 3))
    for i, kind in enumerate(kinds):
        R = rng.uniform(-1, 1, size=(3, 3))
        g[i] = float(kind[2:]) * np.eye(3) + 0.01 * R if kind.startswith("s=") else (0.3 if kind == "large" else 1e-7) * R
    dug = rng.uniform(-1, 1, size=(9, Q))
    return dict(J=J.reshape(9, Q), w=w, dug=dug, kind=np.array(kinds)), g


def write_edges(ref):
    out, g = make_edge_inputs()
    Q = g.shape[0]
    (qdata,) = call_qf(ref("SetupGeo"), np.zeros(2), Q, [out["J"], out["w"]], [10])
    out["SetupGeo.qdata"] = qdata
    ug = np.zeros((9, Q))
    for i in range(Q):                               # g[c][k] = sum_m du[c][m] dXdx[m][k];  ug[d * 3 + c] = du[c][d]
        ug[:, i] = (g[i] @ np.linalg.inv(qdata[1:, i].reshape(3, 3))).T.reshape(9)
    out["ug"] = ug
    out["nus"], out["Es"] = np.array(EDGE_NUS), np.array(EDGE_ES)
    groups = edge_groups()
    for k, (group, nu, E) in enumerate(groups):      # one array per output, [group][component][point]: fewer, larger members
        phys = np.array([nu, E])
        for name, (ins, sizes, keys) in EDGE_CASES.items():
            for key, o in zip(keys, call_qf(ref(name), phys, Q, [out[i] for i in ins], sizes)):
                if key is None:                      # the stored state: the same bits from either model and under every material
                    assert np.array_equal(out.setdefault("gradu", o), o)
                else:
                    out.setdefault(key, np.zeros((len(groups),) + o.shape))[k] = o
    gu = out["gradu"].T.reshape(Q, 3, 3)
    assert np.abs(gu - g).max() < 1e-14
    x = np.linalg.det(np.eye(3) + gu) ** 2 - 1
    print("det C - 1:", {k: np.round(x[out["kind"] == k], 4).tolist() for k in dict.fromkeys(out["kind"])})
    dst = os.path.join(ROOT, "tests", "golden", "qfunctions_edges.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes;", len(out), "arrays of", Q, "points; qfunctions.npz is",
          os.path.getsize(os.path.join(ROOT, "tests", "golden", "qfunctions.npz")))


def main():
    ref_path = os.path.join(HERE, "_ref", "libref_qfunctions.so")
    if not os.path.exists(ref_path):
        sys.exit("oracle/_ref/libref_qfunctions.so missing: run `make -C oracle` in the build container")
    _, ref = load_table(ref_path, "RefGetQFunction")
    which = sys.argv[1:] or ["qfunctions", "edges"]
    if "edges" in which:
        write_edges(ref)
    if "qfunctions" in which:
        write_qfunctions(ref)


def write_qfunctions(ref):
    d = make_inputs()
    Q = d["w"].shape[1]
    out = {k: v for k, v in d.items()}
    phys = np.array([0.3, 2.5])  # {nu, E}
    out["phys"] = phys
    force_dir = np.array([0.1, -1.0, 0.25])
    out["force_dir"] = force_dir

    (qdata,) = call_qf(ref("SetupGeo"), phys, Q, [d["J"], d["w"]], [10])
    out["SetupGeo.qdata"] = qdata
    # scale the reference gradient so the physical gradient is O(0.1..0.3)
    ug = d["ug"]
    # points that force both range-shift branches of log1p_series_shifted
    # (hyperFS.h:49-55): physical grad u = -0.2 I  and  +0.2 I
    for i, s in ((0, -0.2), (1, 0.2), (2, -0.28), (3, 0.41)):
        dXdx = qdata[1:, i].reshape(3, 3)
        du = s * np.linalg.inv(dXdx)  # gradu[j][k] = sum_m du[j][m] dXdx[m][k] = s*delta
        # ug[(d*3+c)] = du[c][d]
        ug[:, i] = du.T.reshape(9)
    out["ug"] = ug

    for name in ("LinElasF", "LinElasdF"):
        (dv,) = call_qf(ref(name), phys, Q, [ug if name.endswith("sF") else d["dug"], qdata], [9])
        out[f"{name}.dv"] = dv
    for fam in ("HyperSS", "HyperFS"):
        dv, gradu = call_qf(ref(fam + "F"), phys, Q, [ug, qdata], [9, 9])
        out[f"{fam}F.dv"], out[f"{fam}F.gradu"] = dv, gradu
        (ddv,) = call_qf(ref(fam + "dF"), phys, Q, [d["dug"], qdata, gradu], [9])
        out[f"{fam}dF.dv"] = ddv
    for fam in ("LinElas", "HyperSS", "HyperFS"):   # strain energy density x w detJ (post-processing operator opEnergy)
        (en,) = call_qf(ref(fam + "Energy"), phys, Q, [ug, qdata], [1])
        out[f"{fam}Energy.energy"] = en
        (dg,) = call_qf(ref(fam + "Diagnostic"), phys, Q, [d["x"], ug, qdata], [8])   # u := the sample coordinates
        out[f"{fam}Diagnostic.diagnostic"] = dg
    (f1,) = call_qf(ref("SetupConstantForce"), force_dir, Q, [d["x"], qdata], [3])
    out["SetupConstantForce.force"] = f1
    (f2,) = call_qf(ref("SetupMMSForce"), phys, Q, [d["x"], qdata], [3])
    out["SetupMMSForce.force"] = f2
    (ts,) = call_qf(ref("MMSTrueSoln"), phys, Q, [d["x"]], [3])
    out["MMSTrueSoln.true_soln"] = ts

    dst = os.path.join(ROOT, "tests", "golden", "qfunctions.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
