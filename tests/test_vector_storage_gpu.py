"""The storage of a CeedVector against its model (tests/_vector_model.py) on the device: every pair of the sixteen operations and
every triple that touches both sides, from the fresh state, from a borrowed host array and from a borrowed device tensor, 50 seeded
walks of 30 operations, at the lengths 0, 1 and 257; the two refusals of a mirror transfer during a recording; and what a replayed recording rests on -- a
vector's device address survives host-side writes."""
import ctypes as C
import functools

import numpy as np
import pytest

import _vector_model as vm
from ceedpetscsolid_amd import ceed as cd

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 257]
HOST_ACCESS = "host access to a device vector during graph capture"
UPLOAD = "host-to-device vector upload during graph capture"


ON_DEVICE = set(vm.DEVICE_MEMORY_OPS + vm.LIBRARY_OPS)      # the operations that touch the device mirror; the others the host's


@functools.lru_cache(maxsize=None)
def triples(start):
    """The sweep of all 16^3 triples measured 8.9 s on the MI355X over the nine cases below (0.45 s to 1.47 s each), so the triples
    are thinned to those with at least one device and one host operation -- a mirror goes stale only between the two sides -- and
    every PAIR is kept."""
    return [s for s in vm.sequences(start, True, 3) if 0 < sum(op in ON_DEVICE for op in s) < 3]


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("start", list(vm.STARTS))
def test_every_triple_of_operations_across_the_two_sides(gpu, start, n):
    w, wdata = vm.operand(gpu, n)
    seqs = triples(start)
    assert len(seqs) > 2200                              # 16^3 - 9^3 - 7^3, less those that read a vector whose sole copy was taken
    for ops in seqs:
        vm.run_sequence(gpu, n, True, start, ops, w, wdata, every=True)
    w.destroy()


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("start", list(vm.STARTS))
def test_every_pair_of_operations(gpu, start, n):
    """Checked after every operation, and at the end only: the reads of a check leave both mirrors valid, and without them the
    second operation meets the state the first one left."""
    w, wdata = vm.operand(gpu, n)
    pairs = vm.sequences(start, True, 2)
    assert len(pairs) > 200
    for every in (True, False):
        for ops in pairs:
            vm.run_sequence(gpu, n, True, start, ops, w, wdata, every=every)
    w.destroy()


@pytest.mark.parametrize("n", LENGTHS)
def test_seeded_walks(gpu, n):
    w, wdata = vm.operand(gpu, n)
    for seed in range(50):
        vm.run_sequence(gpu, n, True, "fresh", vm.walk(seed, True), w, wdata, every=True)
        vm.run_sequence(gpu, n, True, "fresh", vm.walk(seed, True), w, wdata, every=False)
    w.destroy()


def device_address(v):
    p = cd.c_scalar_p()
    v.L.CeedVectorGetArrayRead(v.h, cd.MEM_DEVICE, C.byref(p))
    addr = C.cast(p, C.c_void_p).value
    v.L.CeedVectorRestoreArrayRead(v.h, C.byref(p))
    return addr


# ---- during a recording ---------------------------------------------------------------------------------------------------------
def records_and_runs_normally(gpu, n=257):
    x = gpu.vector(n).set_array(np.arange(1.0, n + 1))
    y = gpu.vector(n).set_value(-7.0)
    gpu.L.CeedVectorSyncArray(x.h, cd.MEM_DEVICE)
    y.axpby(2.0, x, 0.0)                                 # eager
    assert vm.same_bits(y.to_numpy(), 2.0 * np.arange(1.0, n + 1))
    g = gpu.capture(lambda: y.axpby(-1.0, x, 0.0))
    try:
        y.set_value(-7.0)
        g.launch()
        assert vm.same_bits(y.to_numpy(), -np.arange(1.0, n + 1) + 0.0)
    finally:
        g.destroy()
    x.destroy(); y.destroy()


def test_a_host_read_of_a_device_vector_is_refused_while_recording(gpu):
    v = gpu.vector(257).set_value(2.5)                   # the valid copy is on the device
    with pytest.raises(cd.CeedError, match=HOST_ACCESS):
        gpu.capture(lambda: v.to_numpy())
    assert np.all(v.to_numpy() == 2.5)                   # the Ceed records no longer: the read goes through
    records_and_runs_normally(gpu)
    v.destroy()


def test_an_upload_of_a_host_vector_is_refused_while_recording(gpu):
    n = 257
    data = np.linspace(-1, 1, n)
    x = gpu.vector(n).set_array(data)                    # the valid copy is on the host
    y = gpu.vector(n).set_value(-7.0)
    with pytest.raises(cd.CeedError, match=UPLOAD):
        gpu.capture(lambda: y.axpby(2.0, x, 0.0))
    assert np.all(y.to_numpy() == -7.0)                  # nothing was recorded or launched
    y.axpby(2.0, x, 0.0)
    assert vm.same_bits(y.to_numpy(), 2.0 * data + 0.0)
    records_and_runs_normally(gpu)
    x.destroy(); y.destroy()


@pytest.mark.parametrize("n", [257, 2048 * 256 + 1])
def test_set_value_records_and_replays(gpu, n):
    """Zero (a fill kernel while recording, a memset otherwise), minus zero and a non-zero value."""
    vals = (0.0, -0.0, 2.5)
    vs = [gpu.vector(n).set_value(9.0) for _ in vals]
    g = gpu.capture(lambda: [v.set_value(val) for v, val in zip(vs, vals)])
    try:
        for _ in range(2):
            for v in vs:
                v.set_value(9.0)
            g.launch()
            for v, val in zip(vs, vals):
                assert vm.same_bits(v.to_numpy(), np.full(n, val)), val
    finally:
        g.destroy()
    records_and_runs_normally(gpu)
    for v in vs:
        v.destroy()


# ---- what replays rest on -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257])
def test_a_replay_reads_what_a_host_side_write_put_behind_the_same_device_address(gpu, n):
    """tools/graph_replay_check.py refills its inputs with set_array between replays: the recording holds the device address, so
    set_array + SyncArray(DEVICE) must put the new values behind that very address."""
    L = gpu.L
    old, new = vm.values(n, 2), vm.values(n, 3)
    x, y = gpu.vector(n).set_array(old), gpu.vector(n).set_value(-7.0)
    L.CeedVectorSyncArray(x.h, cd.MEM_DEVICE)
    ax, ay = device_address(x), device_address(y)
    g = gpu.capture(lambda: y.axpby(2.0, x, 0.0))
    try:
        with np.errstate(all="ignore"):
            for data in (old, new, old):
                x.set_array(data)
                L.CeedVectorSyncArray(x.h, cd.MEM_DEVICE)
                assert device_address(x) == ax
                y.set_value(-7.0)
                g.launch()
                assert vm.same_bits(y.to_numpy(), 2.0 * data + 0.0)
                assert device_address(y) == ay
            p = cd.c_scalar_p()                             # a write through GetArray(HOST) is a host-side write as well
            L.CeedVectorGetArray(x.h, cd.MEM_HOST, C.byref(p))
            np.ctypeslib.as_array(p, shape=(n,))[:] = new
            L.CeedVectorRestoreArray(x.h, C.byref(p))
            L.CeedVectorSyncArray(x.h, cd.MEM_DEVICE)
            assert device_address(x) == ax
            y.set_value(-7.0)
            g.launch()
            assert vm.same_bits(y.to_numpy(), 2.0 * new + 0.0)
    finally:
        g.destroy()
    x.destroy(); y.destroy()
