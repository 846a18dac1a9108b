"""The mass term of the Jacobian operators, the parts that need no GPU: dynamics.NewmarkPMG(fused_mass=) on the CPU oracle (which lacks
the entry points: "auto" keeps two passes with the bits of False, True raises), the kernels with the term in the code objects of the
build against the shipped (P, Q, QF, GEO) set, and the two entry points in include/ceed.h and the product library."""
import glob
import os
import re
import tempfile

import numpy as np
import pytest

import _kernel_matrix as km
import _newmark_dense as nd
from _mass_common import RHO
from ceedpetscsolid_amd import ceed as cd
from ceedpetscsolid_amd.dynamics import NewmarkPMG
from conftest import ROOT
from test_kernel_inventory import BUILD, COUNTS, _isa_guard

NAMES = ["CeedXOperatorSetMassTerm", "CeedXOperatorMassTermAvailable"]
MASS_QMAX = 7                                      # kernels.hpp FUSED_MASS_QMAX: Q = 8 keeps the two-pass form
_MASS = re.compile(r"\d+k_fused_pencil_massILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE")


# ---------------------------------------------------------------- 1. the oracle: two passes
def test_oracle_lacks_the_entry_points_auto_takes_two_passes_with_the_bits_of_false(oracle):
    assert not any(oracle.L.has(s) for s in NAMES)
    runs = {}
    for fused in (False, "auto"):
        prob, sol = nd.hyperfs_solver(oracle, 2, 2, None, fused_mass=fused)
        assert sol._mass_in_op == [] and all(sol._fused_op(lv) is None for lv in range(sol.nlev))
        assert not prob.levels[prob.fine].opJacob.mass_term_available()
        runs[fused] = [v.to_numpy() for v in (sol.xn, sol.vn, sol.an)]
        nd.teardown(sol, prob)
    for a, b in zip(runs[False], runs["auto"]):
        assert np.array_equal(a, b) and np.abs(a).max() > 0


def test_oracle_refuses_fused_mass_true_and_leaves_the_problem_usable(oracle):
    prob, sol = nd.hyperfs_solver(oracle, 2, 1, None)
    sol.destroy()
    with pytest.raises(ValueError, match="no fused Jacobian kernel with the mass term for level"):
        NewmarkPMG(prob, RHO, nd.DT_FS, fused_mass=True)
    with pytest.raises(ValueError, match="fused_mass must be"):
        NewmarkPMG(prob, RHO, nd.DT_FS, fused_mass=1.5)
    with pytest.raises(cd.CeedError, match="CeedXOperatorSetMassTerm"):
        prob.levels[prob.fine].opJacob.set_mass_term(1.0)
    sol = NewmarkPMG(prob, RHO, nd.DT_FS, fused_mass="auto")          # the problem is still whole
    sol.set_initial()
    assert sol.step().converged
    nd.teardown(sol, prob)


# ---------------------------------------------------------------- 2. the code objects of the build
def shipped_mass_kernels():
    """(P, Q, qf, geo) of every kernel with the term: the Jacobian functors of the fused family up to Q = MASS_QMAX."""
    jac = {"LinElas", "HyperSSdF", "HyperFSdF", "HyperFSdF+derived"}
    return {k[1:] for k in km.fused_kernels() if k[3] in jac and k[2] <= MASS_QMAX}


@pytest.fixture(scope="module")
def symbols():
    objs = sorted(glob.glob(os.path.join(BUILD, "*.o")))
    if not objs:
        pytest.fail("no objects under csrc/build: run __graft_entry__.build() (a missing build must not hide a broken inventory)")
    guard = _isa_guard()
    mass, old = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for obj in objs:
            with open(obj, "rb") as f:
                if b".hip_fatbin" not in f.read():
                    continue
            for mangled in guard.kernel_meta(guard.code_object(obj, tmp)):
                m = _MASS.search(mangled)
                if m:
                    mass.append((os.path.basename(obj), (int(m[1]), int(m[2]), km.FUSED_QF.get(int(m[3]), int(m[3])), int(m[4]))))
                k = km.kernel_of_symbol(mangled)
                if k is not None:
                    old.append((os.path.basename(obj), k))
    return mass, old


def test_build_holds_the_mass_kernels_of_exactly_the_shipped_set(symbols):
    mass, _ = symbols
    have = [k for _, k in mass]
    assert len(have) == len(set(have)), "a kernel with the mass term is defined in two objects"
    want = shipped_mass_kernels()
    missing, extra = sorted(want - set(have)), sorted(set(have) - want)
    assert not missing and not extra, f"shipped but not built: {missing}; built but not shipped: {extra}"
    assert len(want) == 296
    assert all(obj.startswith("fusedm_q") for obj, _ in mass), "the kernels with the term live in objects of their own"


def test_the_five_families_are_what_they_were(symbols):
    """No kernel of the old families was added or lost, none moved into an object of the kernels with the term, and no mangled name of
    the new entry is read as one of the old family (tests/_kernel_matrix.py, tools/isa_guard.py)."""
    _, old = symbols
    found = {}
    for obj, k in old:
        assert not obj.startswith("fusedm_q"), (obj, km.show(k))
        found.setdefault(k[0], set()).add(k)
    assert {fam: len(ks) for fam, ks in found.items()} == COUNTS
    assert found == km.matrix()
    name = "_ZN3cps19k_fused_pencil_massILi5ELi7ELi6ELi3EEEvNS_11BasisTablesENS_13FusedGradArgsE"
    assert km.kernel_of_symbol(name) is None and _MASS.search(name)
    short, q, eo = _isa_guard().short_name(name)
    assert short == "k_fused_pencil_mass<P=5,Q=7,HyperFSdF,geo=3,eo=1>" and q == 7 and eo == 1
    assert _isa_guard().short_name(name.replace("19k_fused_pencil_mass", "14k_fused_pencil"))[0] == "k_fused_pencil<P=5,Q=7,HyperFSdF,geo=3,eo=1>"


def test_isa_summary_lists_the_mass_kernels_under_the_contract():
    path = os.path.join(BUILD, "isa_summary.txt")
    if not os.path.exists(path):
        pytest.fail("no ISA summary under csrc/build: run __graft_entry__.build()")
    rows = [l.rstrip("\n").split("\t") for l in open(path)]
    hdr = rows[0]
    mass = [dict(zip(hdr, r)) for r in rows[1:] if r[0].startswith("k_fused_pencil_mass<")]
    assert len(mass) == 296
    for r in mass:
        assert int(r["scratch_B"]) == 0 and int(r["vspill"]) == 0 and int(r["s_barrier"]) == 0 and int(r["lds2/128"]) == 0 and int(r["scratch_ins"]) == 0, r
        assert int(r["vgpr"]) <= 256, r
    assert "VIOLATIONS: none" in open(path).read()


# ---------------------------------------------------------------- 3. header and exports
def test_header_declares_the_entry_points_optional_and_the_product_exports_them(oracle_lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ceed.h")).read(), flags=re.S)
    optional = re.findall(r"CEED_EXTERN_OPTIONAL\s+int\s+(Ceed[A-Za-z0-9_]+)\s*\(", txt)
    required = re.findall(r"CEED_EXTERN\s+int\s+(Ceed[A-Za-z0-9_]+)\s*\(", txt)
    for s in NAMES:
        assert s in optional and s not in required and s in cd.CeedLib.OPTIONAL and s not in cd.CeedLib.FUNCTIONS
    assert not oracle_lib.missing_symbols(optional=False)
    if not os.path.exists(cd.PRODUCT_LIB):
        pytest.fail("product library not built: run __graft_entry__.build()")
    lib = cd.CeedLib(cd.PRODUCT_LIB)
    assert not [s for s in NAMES if not lib.has(s)]
    assert not lib.missing_symbols()
