"""The kernels in the code objects of the build against the matrix of tests/_kernel_matrix.py, both directions, and the plan of the GPU
sweep (test_kernel_matrix_gpu.py) against the same matrix: an instantiation nobody launches, or a launch of something that is not
built, fails here on the CPU.  The names are read the way tools/isa_guard.py reads them: the .hip_fatbin section, unbundled for gfx950,
the .name fields of the code object's metadata note (the mangled names carry the template arguments)."""
import glob
import importlib.util
import os
import tempfile

import pytest

import _kernel_matrix as km
from conftest import ROOT

BUILD = os.path.join(ROOT, "ceedpetscsolid_amd", "csrc", "build")
COUNTS = {"fused": 552, "diag": 84, "transfer": 44, "state": 32, "setup_geo": 7}


def _isa_guard():
    spec = importlib.util.spec_from_file_location("isa_guard", os.path.join(ROOT, "tools", "isa_guard.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
    return mod


@pytest.fixture(scope="module")
def built():
    """Family -> kernels found in build/*.o.  Skips only where nothing was ever built; with objects present every failure to read them is
    a failure of the test."""
    objs = sorted(glob.glob(os.path.join(BUILD, "*.o")))
    if not objs:
        pytest.skip("no objects under csrc/build: this checkout was never built")
    guard = _isa_guard()
    found = {fam: set() for fam in km.FAMILIES}
    found["pbdiag"] = set()                                   # the shapes of k_pbdiag_sf: no family of its own (km.pbdiag_of_symbol)
    with tempfile.TemporaryDirectory() as tmp:
        for obj in objs:
            with open(obj, "rb") as f:
                if b".hip_fatbin" not in f.read():
                    continue                                  # host-only object: no device code to look at
            names = guard.kernel_meta(guard.code_object(obj, tmp))
            assert names, f"{obj} has a .hip_fatbin section but no kernel was read out of it"
            for mangled in names:
                k = km.kernel_of_symbol(mangled)
                if k is not None:
                    assert k not in found[k[0]], f"{km.show(k)} is defined in two objects"
                    found[k[0]].add(k)
                k = km.pbdiag_of_symbol(mangled)
                if k is not None:
                    assert k not in found["pbdiag"], f"k_pbdiag_sf of {km.show(k)} is defined in two objects"
                    found["pbdiag"].add(k)
    return found


def _diff(have, want):
    return sorted(km.show(k) for k in want - have), sorted(km.show(k) for k in have - want)


@pytest.mark.parametrize("family", list(km.FAMILIES))
def test_build_holds_exactly_the_matrix(built, family):
    missing, extra = _diff(built[family], km.matrix()[family])
    assert not missing and not extra, f"{family}: in the matrix but not built: {missing}; built but not in the matrix: {extra}"


def test_point_block_diagonal_is_built_for_the_shapes_of_the_scalar_one(built):
    """k_pbdiag_sf<P,Q,QF> against matrix()["diag"]: a level with a scalar diagonal and no blocks (or the reverse) fails at solve time."""
    missing, extra = _diff(built["pbdiag"], km.matrix()["diag"])
    assert len(built["pbdiag"]) == COUNTS["diag"] and not missing and not extra, \
        f"k_pbdiag_sf: shapes of k_diag_sf without blocks: {missing}; blocks without a scalar diagonal: {extra}"


@pytest.mark.parametrize("family", list(km.FAMILIES))
def test_plan_launches_exactly_the_matrix(family):
    unlaunched, unknown = _diff(km.planned_kernels()[family], km.matrix()[family])
    assert not unlaunched and not unknown, f"{family}: instantiated but in no build of the plan: {unlaunched}; planned but not instantiated: {unknown}"


def test_matrix_counts_of_a_default_build():
    """The sizes of the five families (the code-object metadata of a default build): a change of the matrix is a change of these."""
    assert {fam: len(ks) for fam, ks in km.matrix().items()} == COUNTS


def test_symbol_parser_reads_the_template_arguments():
    assert km.kernel_of_symbol("_ZN3cps14k_fused_pencilILi5ELi7ELi6ELi3EEEvNS_11BasisTablesENS_13FusedGradArgsE") == ("fused", 5, 7, "HyperFSdF", 3)
    assert km.kernel_of_symbol("_ZN3cps14k_fused_pencilILi8ELi8ELi17ELi0EEEvNS_11BasisTablesENS_13FusedGradArgsE") == ("fused", 8, 8, "HyperFSdF+derived", 0)
    assert km.kernel_of_symbol("_ZN3cps17k_state_at_pointsILi3ELi2EEEvNS_11BasisTablesENS_9StateArgsE") == ("state", 3, 2)
    assert km.kernel_of_symbol("_ZN3cps10k_transferILi2ELi3ELb1ELb0EEEvNS_11BasisTablesENS_12TransferArgsE") == ("transfer", 2, 3, True, False)
    assert km.kernel_of_symbol("_ZN3cps9k_diag_sfILi2ELi8ELi4EEEvNS_11BasisTablesENS_8DiagArgsE") == ("diag", 2, 8, "HyperSSdF")
    assert km.kernel_of_symbol("_ZN3cps11k_setup_geoILi8EEEvNS_11BasisTablesENS_12SetupGeoArgsE") == ("setup_geo", 8)
    assert km.kernel_of_symbol("_ZN3cps10k_assembleEPKjS1_S1_PKhPKdPdii") is None
    assert km.kernel_of_symbol("_ZN3cps11k_pbdiag_sfILi2ELi8ELi4EEEvNS_11BasisTablesENS_8DiagArgsE") is None
    assert km.pbdiag_of_symbol("_ZN3cps11k_pbdiag_sfILi2ELi8ELi4EEEvNS_11BasisTablesENS_8DiagArgsE") == ("diag", 2, 8, "HyperSSdF")
    assert km.pbdiag_of_symbol("_ZN3cps9k_diag_sfILi2ELi8ELi4EEEvNS_11BasisTablesENS_8DiagArgsE") is None
