"""The table of the plain device kernels (tests/_plain_kernels.py) against the build, the sources and the test modules, on the CPU:
every kernel of the code objects that no family of _kernel_matrix claims is in the table and every entry of the table is built; every
cap the table restates still stands verbatim in the file it names; every capped kernel names a GPU test that exists and whose largest
stated size exceeds one grid.  The names are read as the `built` fixture of test_kernel_inventory.py reads them: the .name fields of the
code objects' metadata and nothing else of the code objects."""
import glob
import importlib
import os
import tempfile

import pytest

import _kernel_matrix as km
import _plain_kernels as pk
from conftest import ROOT
from test_kernel_inventory import BUILD, _isa_guard


@pytest.fixture(scope="module")
def built_plain():
    """kernel name -> number of instantiations found in build/*.o, for the kernels no family claims.  Skips only where nothing was ever
    built."""
    objs = sorted(glob.glob(os.path.join(BUILD, "*.o")))
    if not objs:
        pytest.skip("no objects under csrc/build: this checkout was never built")
    guard = _isa_guard()
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in objs:
            with open(obj, "rb") as f:
                if b".hip_fatbin" not in f.read():
                    continue
            names = guard.kernel_meta(guard.code_object(obj, tmp))
            assert names, f"{obj} has a .hip_fatbin section but no kernel was read out of it"
            for mangled in names:
                if km.kernel_of_symbol(mangled) is None and km.pbdiag_of_symbol(mangled) is None:
                    name = pk.plain_name_of_symbol(mangled)
                    assert name, f"{mangled} in {obj}: not a kernel of the cps namespace"
                    found[name] = found.get(name, 0) + 1
    return found


def inventory_diff(found, table):
    """(built but in no table, in the table but not built)"""
    return sorted(set(found) - set(table)), sorted(set(table) - set(found))


def test_build_holds_exactly_the_table(built_plain):
    extra, missing = inventory_diff(built_plain, pk.BY_NAME)
    assert not extra and not missing, f"built but in neither a family nor the table of plain kernels: {extra}; in the table but not built: {missing}"


def test_the_check_fails_in_both_directions(built_plain):
    """An entry taken out of the table and an entry no build holds are both reported."""
    table = dict(pk.BY_NAME)
    gone = table.pop("k_pb_mult")
    assert inventory_diff(built_plain, table) == (["k_pb_mult"], [])
    table["k_pb_mult"], table["k_no_such_kernel"] = gone, gone
    assert inventory_diff(built_plain, table) == ([], ["k_no_such_kernel"])


def test_table_is_well_formed():
    assert len(pk.BY_NAME) == len(pk.KERNELS), "a kernel stands in the table twice"
    for k in pk.KERNELS:
        assert k.launch in pk.CAPS or k.launch in pk.UNCAPPED, (k.name, k.launch)
        src = read(k.file)
        assert f"void {k.name}(" in src, f"{k.name} is not defined in {k.file}"


def read(rel):
    with open(os.path.join(ROOT, rel)) as f:
        return f.read()


@pytest.mark.parametrize("form", list(pk.CAPS))
def test_every_cap_stands_verbatim_in_its_file(form):
    cap = pk.CAPS[form]
    src = read(cap.file)
    for expr in cap.exprs:
        assert expr in src, f"{form}: `{expr}` no longer stands in {cap.file}: the cap changed, so the table and the sizes of its tests do"


def test_cap_constants_and_items():
    for rel, text in pk.CAP_CONSTANTS:
        assert text in read(rel), f"`{text}` no longer stands in {rel}"
    items = {form: cap.items for form, cap in pk.CAPS.items()}
    assert items == {"stream": 524288, "grid_for": 1048576, "assemble unpack": 262144, "assemble_epi interior": 1048576, "spgemm dense": 8192,
                     "spgemm row": 32768, "spgemm plain": 65536, "block gram": 65536, "block combine": 1048576}


def gpu_test_of(node_id):
    module, name = node_id.split("::")
    fn = getattr(importlib.import_module(module), name, None)
    assert callable(fn), f"{node_id}: no such test"
    mod = importlib.import_module(module)
    marks = getattr(mod, "pytestmark", None)
    marks = [marks] if marks is not None and not isinstance(marks, (list, tuple)) else list(marks or [])
    marks += list(getattr(fn, "pytestmark", []))
    assert any(m.name == "gpu" for m in marks), f"{node_id} is not a GPU test"
    return fn


def largest_size(k):
    kind = k.sizes[0]
    if kind == "attr":
        value = getattr(importlib.import_module(k.sizes[1]), k.sizes[2])
        sizes = [value] if isinstance(value, int) else list(value)
        assert sizes and all(isinstance(s, int) for s in sizes), (k.name, k.sizes)
        return max(sizes)
    assert kind == "text", (k.name, k.sizes)
    _, rel, snippet, value = k.sizes
    assert snippet in read(rel), f"{k.name}: `{snippet}` no longer stands in {rel}"
    return value


@pytest.mark.parametrize("name", [k.name for k in pk.KERNELS])
def test_every_capped_kernel_is_run_past_one_grid(name):
    k = pk.BY_NAME[name]
    for node_id in k.tests:
        gpu_test_of(node_id)
    if k.launch in pk.UNCAPPED:
        assert k.sizes is None and k.reach is None
        return
    G = pk.CAPS[k.launch].items
    if k.reach is not None:                     # a cap that no caller reaches: the limits stand in the sources, and nothing larger is claimed
        limit, pins = k.reach
        assert limit < G and (pins or name in pk.NO_CALLER), name
        for rel, text in pins:
            assert text in read(rel), f"{name}: `{text}` no longer stands in {rel}: the kernel may be reachable past one grid now"
        if name in pk.NO_CALLER:
            callers = [f for f in glob.glob(os.path.join(ROOT, pk.CSRC, "*.cpp")) if pk.NO_CALLER[name] + "(" in open(f).read()]
            assert not callers and not k.tests, f"{pk.NO_CALLER[name]} has a caller now: {callers}"
        else:
            assert k.tests and largest_size(k) == limit, name
        return
    assert k.tests, f"{name} is launched on a capped grid ({k.launch}) and names no test"
    assert largest_size(k) > G, f"{name}: the largest size its tests state, {largest_size(k)}, does not exceed one grid of {G} items"


def test_vectorised_references_of_the_lap_tests_equal_the_loops():
    """ordered_transpose and ordered_sums of test_grid_laps_gpu against the loops they restate: expected_transpose of
    test_restriction_transpose_gpu on its 2 x 2 x 2 layouts, coo_expected of test_linalg_kernels on its pattern."""
    import numpy as np
    import test_grid_laps_gpu as laps
    import test_restriction_transpose_gpu as rt
    from test_linalg_kernels import coo_expected, coo_pattern, coo_values
    rng = np.random.default_rng(1)
    for case in rt.CASES:
        lay = rt.layout(*case)
        E, y0 = rng.uniform(-1, 1, lay[0] * lay[1] * lay[2]), rng.uniform(-1, 1, lay[4])
        assert np.array_equal(rt.expected_transpose(lay, E, y0), laps.ordered_transpose(lay, E, y0)), case
    rowptr, cols, slot, unit, unmapped = coo_pattern(rng)
    v = coo_values(rng, slot.size)
    exp = coo_expected(cols.size, slot, v, rowptr, cols, np.zeros(0, dtype=np.int64))
    assert np.array_equal(exp, laps.ordered_sums(slot[slot >= 0], v[slot >= 0], cols.size))
