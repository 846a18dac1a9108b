"""The entry points of include/ceed_surface_field.h in the binding: parsed like include/ceed.h's, declared on every library that exports
them, and called with the declared number of arguments (what test_support_binding.py holds for include/ceed_support.h)."""
import ast
import ctypes as C
import glob
import os
import re

import pytest

from ceedpetscsolid_amd import ceed as cd
from conftest import ROOT

NAMES = ["CeedXSurfaceLoadApplyFieldAdd", "CeedXSurfaceLoadApplyFieldTangentAdd", "CeedXSurfaceLoadApplyHydrostaticAdd",
         "CeedXSurfaceLoadApplyHydrostaticTangentAdd"]


def test_parse_equals_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(cd.SURFACE_FIELD_HEADER).read(), flags=re.S)
    txt = re.sub(r"(?m)^\s*#.*$", "", txt)
    assert re.findall(r"CEED_EXTERN\s[^;(]*?(\w+)\s*\(", txt) == []                        # all optional
    assert re.findall(r"CEED_EXTERN_OPTIONAL\s[^;(]*?(\w+)\s*\(", txt) == NAMES == cd.CeedLib.SURFACE_FIELD == list(cd.SURFACE_FIELD_PROTOTYPES.functions)
    P = cd.SURFACE_FIELD_PROTOTYPES.functions
    assert all(p.optional and p.restype is C.c_int for p in P.values())
    assert not set(P) & (set(cd.PROTOTYPES.functions) | set(cd.CONTACT_PROTOTYPES.functions) | set(cd.SUPPORT_PROTOTYPES.functions))
    for name, p in P.items():                                                               # the arity against a count of the commas
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1).strip()
        assert len(p.argtypes) == args.count(",") + 1, name
    H, D = cd._Handle, C.c_double
    assert P["CeedXSurfaceLoadApplyFieldAdd"].argtypes == (H, C.c_int, H, D, H, H, H)
    assert P["CeedXSurfaceLoadApplyFieldTangentAdd"].argtypes == (H, H, D, H, H, H, H)
    assert P["CeedXSurfaceLoadApplyHydrostaticAdd"].argtypes == (H, D, D, C.POINTER(D), D, H, H, H)
    assert P["CeedXSurfaceLoadApplyHydrostaticTangentAdd"].argtypes == (H, D, D, C.POINTER(D), D, H, H, H, H)
    # include/ceed.h keeps the list of entry points it had
    assert not [n for n in cd.PROTOTYPES.functions if "Field" in n and n.startswith("CeedXSurfaceLoad") or "Hydrostatic" in n]


@pytest.mark.parametrize("which", ["oracle", "product"])
def test_libraries_carry_the_parsed_prototypes(which, oracle_lib):
    if which == "product" and not os.path.exists(cd.PRODUCT_LIB):
        pytest.fail("product library not built: run __graft_entry__.build()")
    lib = oracle_lib if which == "oracle" else cd.CeedLib(cd.PRODUCT_LIB)
    for name, p in cd.SURFACE_FIELD_PROTOTYPES.functions.items():
        if which == "oracle":
            assert not lib.has(name) and not hasattr(lib, name), name                       # the oracle takes the portable form
            continue
        raw, twin = getattr(lib.lib, name), getattr(lib, name)
        assert raw is not twin and raw.errcheck is None and twin.errcheck is lib.errcheck, name
        for f in (raw, twin):
            assert tuple(f.argtypes) == p.argtypes and f.restype is C.c_int, name
    assert not lib.missing_symbols(optional=which == "product")


def test_missing_symbols_counts_the_entry_points(oracle_lib):
    assert set(NAMES) <= set(oracle_lib.missing_symbols()) and not set(NAMES) & set(oracle_lib.missing_symbols(optional=False))


def test_every_call_site_passes_the_declared_number_of_arguments():
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "ceedpetscsolid_amd", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py"))):
        for node in ast.walk(ast.parse(open(path).read())):
            if not isinstance(node, ast.Call):
                continue
            f, args = node.func, node.args
            if isinstance(f, ast.Attribute) and f.attr in cd.SURFACE_FIELD_PROTOTYPES.functions:
                found[f.attr] = found.get(f.attr, 0) + 1
                assert len(args) == len(cd.SURFACE_FIELD_PROTOTYPES.functions[f.attr].argtypes), (path, node.lineno, f.attr)
                assert os.path.basename(path) == "ceed.py", (path, f.attr)
    assert found == {n: 1 for n in NAMES}                                                   # each entry point is called once, in ceed.py
