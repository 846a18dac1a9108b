"""The device kernels a default build instantiates, restated as data, and the plan of problem builds that launches every one of them.

The dispatch tables of csrc (kernels_fused_inst.hip CPS_CASE / CPS_LEVEL, kernel_diag_sf.hpp CPS_DIAG_PQ, kernels_transfer.hip CPS_TR, kernels_geometry.hip CPS_SG,
kernels_state.hip CPS_ST) are the product; this module is their second statement.  test_kernel_inventory.py holds the two against each
other on the code objects of the build (both directions), and holds the plan below against the matrix; test_kernel_matrix_gpu.py runs
the plan.  Whoever adds or drops an instantiation has to change the matrix here, and the sweep follows.

A kernel is a tuple:
  ("fused", P, Q, qf, geo)                k_fused_pencil<P, Q, QF, GEO>; qf one of FUSED_QF, geo 0 qdata read, 1 recomputed per point,
                                          2 affine elements, 3 swept elements
  ("diag", P, Q, qf)                      k_diag_sf<P, Q, QF>; k_pbdiag_sf<P, Q, QF> is instantiated for the same set (pbdiag_of_symbol)
  ("transfer", Pc, Pf, prolong, weighted) k_transfer<Pc, Pf, PROLONG, WEIGHTED>
  ("state", Pf, Qc)                       k_state_at_points<Pf, Qc>
  ("setup_geo", Q)                        k_setup_geo<Q>
"""
import re
from collections import namedtuple

QS = range(2, 9)                     # points per direction (MAXN1D = 8)
# QFKind of kernels.hpp -> the text of the dispatch tables (and of tools/isa_guard.py)
FUSED_QF = {2: "LinElas", 3: "HyperSSF", 4: "HyperSSdF", 5: "HyperFSF", 6: "HyperFSdF", 17: "HyperFSdF+derived"}
DIAG_QF = {2: "LinElas", 4: "HyperSSdF", 6: "HyperFSdF"}
GEO_TEXT = {0: "qdata read", 1: "dXdx recomputed per point", 2: "affine elements: dXdx per element",
            3: "swept elements: 2 x 2 dXdx recomputed per point"}       # CeedXOperatorGetKernelName
PHYSICS = {"linElas": ("LinElas", "LinElas"), "hyperSS": ("HyperSSF", "HyperSSdF"), "hyperFS": ("HyperFSF", "HyperFSdF")}   # residual, Jacobian


def derived_state(Q):                # kernels.hpp, pencil_derived_state
    return Q >= 6


def group_elems(Q):                  # kernels.hpp, pencil_group_elems: elements per wave of the fused kernel
    return 8 if Q <= 2 else (4 if Q <= 4 else (2 if Q == 5 else 1))


def fused_kernels():
    out = set()
    for Q in QS:
        for P in range(2, Q + 1):
            qfs = ["LinElas", "HyperSSdF", "HyperFSdF"]
            if derived_state(Q):
                qfs.append("HyperFSdF+derived")
            if Q - P <= 2:           # the fine level: P = Q, and P = Q - 1, Q - 2 under -qextra 1, 2
                qfs += ["HyperSSF", "HyperFSF"]
            out |= {("fused", P, Q, qf, geo) for qf in qfs for geo in range(4)}
    return out


def diag_kernels():
    return {("diag", P, Q, qf) for Q in QS for P in range(2, Q + 1) for qf in DIAG_QF.values()}


# adjacent levels of the uniform ladders (P, P + 1), of the logarithmic ones (degrees 1, 2, 4, p), and the two-level ladders (1, 3), (1, 4)
TRANSFER_PAIRS = [(2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (3, 5), (5, 7), (5, 8), (2, 4), (2, 5)]


def transfer_kernels():
    return {("transfer", c, f, pro, w) for c, f in TRANSFER_PAIRS for pro in (True, False) for w in (True, False)}


# fine P_f = 3 .. 8 x the Q_c = P_c + qextra <= 8 of a level below it (P_c < P_f, qextra <= 2)
STATE_PAIRS = [(Pf, Qc) for Pf in range(3, 9) for Qc in range(2, min(Pf + 1, 8) + 1)]


def state_kernels():
    return {("state", Pf, Qc) for Pf, Qc in STATE_PAIRS}


def setup_geo_kernels():
    return {("setup_geo", Q) for Q in QS}


FAMILIES = {"fused": fused_kernels, "diag": diag_kernels, "transfer": transfer_kernels, "state": state_kernels, "setup_geo": setup_geo_kernels}


def matrix():
    return {fam: make() for fam, make in FAMILIES.items()}


_MANGLED = [
    (re.compile(r"\d+k_fused_pencilILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE"), lambda m: ("fused", int(m[1]), int(m[2]), FUSED_QF.get(int(m[3]), int(m[3])), int(m[4]))),
    (re.compile(r"\d+k_diag_sfILi(\d+)ELi(\d+)ELi(\d+)EE"), lambda m: ("diag", int(m[1]), int(m[2]), DIAG_QF.get(int(m[3]), int(m[3])))),
    (re.compile(r"\d+k_transferILi(\d+)ELi(\d+)ELb(\d)ELb(\d)EE"), lambda m: ("transfer", int(m[1]), int(m[2]), m[3] == "1", m[4] == "1")),
    (re.compile(r"\d+k_state_at_pointsILi(\d+)ELi(\d+)EE"), lambda m: ("state", int(m[1]), int(m[2]))),
    (re.compile(r"\d+k_setup_geoILi(\d+)EE"), lambda m: ("setup_geo", int(m[1]))),
]


def kernel_of_symbol(mangled):
    """The kernel tuple of a mangled name of the five families (the template arguments are in the name), else None."""
    for rx, make in _MANGLED:
        m = rx.search(mangled)
        if m:
            return make(m)
    return None


_MANGLED_PBDIAG = re.compile(r"\d+k_pbdiag_sfILi(\d+)ELi(\d+)ELi(\d+)EE")


def pbdiag_of_symbol(mangled):
    """The ("diag", P, Q, qf) shape of a mangled k_pbdiag_sf<P, Q, QF>, else None: the point-block diagonal is no family of its own, it is
    built for the shapes of the scalar one (one list in csrc, CPS_DIAG_PQ)."""
    m = _MANGLED_PBDIAG.search(mangled)
    return ("diag", int(m[1]), int(m[2]), DIAG_QF.get(int(m[3]), int(m[3]))) if m else None


def show(k):
    fam = k[0]
    if fam == "fused":
        return f"k_fused_pencil<P={k[1]},Q={k[2]},{k[3]},geo={k[4]}>"
    if fam == "diag":
        return f"k_diag_sf<P={k[1]},Q={k[2]},{k[3]}>"
    if fam == "transfer":
        return f"k_transfer<Pc={k[1]},Pf={k[2]},{'prolong' if k[3] else 'restrict'},{'weighted' if k[4] else 'plain'}>"
    if fam == "state":
        return f"k_state_at_points<Pf={k[1]},Qc={k[2]}>"
    return f"k_setup_geo<Q={k[1]}>"


# ---------------------------------------------------------------------------------------------------------------------------------
# The plan of the GPU sweep
# ---------------------------------------------------------------------------------------------------------------------------------
# geometry case -> (mesh of the build, GEO template argument its fused kernels must report, switches of the Ceed it is built on)
GEOMETRIES = {
    "general": ("general", 1, ()),
    "stored": ("general", 0, ("CEED_MI355X_GEO",)),
    "affine": ("affine", 2, ()),
    "swept0": ("swept0", 3, ()),
    "swept1": ("swept1", 3, ()),
    "swept2": ("swept2", 3, ()),
}
# the form a geometry case is compared with on the device: (switches of the other Ceed, GEO it must report there)
COMPARE = {"general": (("CEED_MI355X_GEO",), 0), "affine": (("CEED_MI355X_AFFINE",), 1),
           "swept0": (("CEED_MI355X_SWEPT",), 1), "swept1": (("CEED_MI355X_SWEPT",), 1), "swept2": (("CEED_MI355X_SWEPT",), 1)}

# One problem build: SolidProblem(degree = Q - 1 - qextra, multigrid="uniform", qextra) on the case's mesh.  `derived` False: the Ceed also has
# CEED_MI355X_DERIVED=0 (hyperFS at Q >= 6 only: the one route to the plain HyperFSdF there).
Build = namedtuple("Build", "Q qextra physics geometry derived")


def build_id(b):
    return f"Q{b.Q}-qextra{b.qextra}-{b.physics}-{b.geometry}" + ("" if b.derived else "-plain_tangent")


def build_degree(b):
    return b.Q - 1 - b.qextra


def build_switches(b):
    """The CEED_MI355X_* switches set to 0 in the Ceed of this build (sorted tuple; () is the default Ceed)."""
    return tuple(sorted(GEOMETRIES[b.geometry][2] + (() if b.derived else ("CEED_MI355X_DERIVED",))))


def jacobian_qf(b):
    qf = PHYSICS[b.physics][1]
    return qf + "+derived" if qf == "HyperFSdF" and b.derived and derived_state(b.Q) else qf


def build_kernels(b):
    """Every kernel of the five families the sweep launches in build `b` (weighted transfers and the state kernels have tests of their own)."""
    geo, Pfine = GEOMETRIES[b.geometry][1], build_degree(b) + 1
    ks = {("setup_geo", b.Q), ("fused", Pfine, b.Q, PHYSICS[b.physics][0], geo)}
    for P in range(2, Pfine + 1):
        ks.add(("fused", P, b.Q, jacobian_qf(b), geo))
        ks.add(("diag", P, b.Q, PHYSICS[b.physics][1]))
        if P > 2:
            ks |= {("transfer", P - 1, P, pro, False) for pro in (True, False)}
    return ks


def fused_name(P, Q, qf, geo):
    """What kernel_name reports after a fused apply."""
    return f"fused_grad<P={P},Q={Q},{qf}>/pencil [{GEO_TEXT[geo]}]"


def plan():
    out = []
    for Q in QS:                                        # ascending Q: a first launch that goes wrong ends the run at the smallest shape
        for qextra in (0, 1, 2):
            if Q - 1 - qextra < 1:
                continue
            for physics in PHYSICS:
                for g in GEOMETRIES:
                    out.append(Build(Q, qextra, physics, g, True))
                    if physics == "hyperFS" and derived_state(Q) and qextra == 0:
                        out.append(Build(Q, qextra, physics, g, False))
    return out


# ladders of the transfer tests: (degree, multigrid or the two-level ladder [1, degree]) -> every pair of TRANSFER_PAIRS
TRANSFER_LADDERS = [(7, "uniform"), (6, "logarithmic"), (7, "logarithmic"), (3, "two-level"), (4, "two-level")]


def ladder_pairs(degree, kind):
    if kind == "uniform":
        degs = list(range(1, degree + 1))
    elif kind == "two-level":
        degs = [1, degree]
    else:
        degs, d = [degree], 1
        while d < degree:
            degs.insert(-1, d); d *= 2
    return [(a + 1, b + 1) for a, b in zip(degs[:-1], degs[1:])]


def planned_kernels():
    """Family -> the kernels the GPU tests of the matrix launch: the sweep's builds, the transfer ladders (plain and weighted), all state pairs."""
    ks = set()
    for b in plan():
        ks |= build_kernels(b)
    for degree, kind in TRANSFER_LADDERS:
        ks |= {("transfer", c, f, pro, w) for c, f in ladder_pairs(degree, kind) for pro in (True, False) for w in (True, False)}
    ks |= state_kernels()
    return {fam: {k for k in ks if k[0] == fam} for fam in FAMILIES}
