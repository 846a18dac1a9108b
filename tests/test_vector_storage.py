"""The storage of a CeedVector against its model (tests/_vector_model.py), host-only subset, on the CPU oracle: every sequence of
three operations from the fresh state and from a borrowed host array, 50 seeded walks, at the lengths 0, 1 and 257; the oracle's
refusal of every device-memory call; and what ``Vector.set_array(copy=False)`` accepts."""
import ctypes as C
import functools

import numpy as np
import pytest

import _vector_model as vm
from ceedpetscsolid_amd import ceed as cd

LENGTHS = [0, 1, 257]


@functools.lru_cache(maxsize=None)
def triples(start, device):
    return vm.sequences(start, device, 3)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("start", ["fresh", "host_borrowed"])
def test_every_triple_of_host_operations_on_oracle(oracle, start, n):
    w, wdata = vm.operand(oracle, n)
    seqs = triples(start, False)
    assert len(seqs) > 800                               # 11^3 less those that read a vector whose sole copy was taken
    for every in (True, False):
        for ops in seqs:
            vm.run_sequence(oracle, n, False, start, ops, w, wdata, every=every)
    w.destroy()


@pytest.mark.parametrize("n", LENGTHS)
def test_seeded_walks_on_oracle(oracle, n):
    w, wdata = vm.operand(oracle, n)
    for seed in range(50):
        vm.run_sequence(oracle, n, False, "fresh", vm.walk(seed, False), w, wdata)
    w.destroy()


def test_the_model_itself():
    """The generator leaves out exactly the reads of a taken sole copy, and the walks are reproducible."""
    assert ("set_host_copy", "take_host", "read_host") not in triples("fresh", False)
    assert ("set_host_copy", "take_host", "set_value") in triples("fresh", False)
    assert ("take_host", "take_host", "read_host") in triples("fresh", False)          # never written: still reads as zeros
    assert ("sync_dev", "take_host", "dot") in triples("host_borrowed", True)          # the device mirror holds the value
    assert ("take_host", "dot", "dot") not in triples("host_borrowed", True)
    assert len(triples("fresh", True)) > 3000 and len(vm.OPS) == 16
    assert vm.walk(3, True) == vm.walk(3, True) and len(vm.walk(3, True)) == 30
    assert {op for s in range(50) for op in vm.walk(s, True)} == set(vm.OPS)


@pytest.mark.parametrize("n", LENGTHS)
def test_device_memory_calls_are_refused_by_the_oracle_and_leave_the_value(oracle, n):
    L = oracle.L
    data = vm.values(n, 1)
    v = oracle.vector(n).set_array(data)
    buf = vm.HostBuffer(data)                            # (an address to pass: the oracle must not touch it)
    p = cd.c_scalar_p()
    calls = [lambda: L.CeedVectorSetArray(v.h, cd.MEM_DEVICE, cd.USE_POINTER, buf.pointer()),
             lambda: L.CeedVectorSetArray(v.h, cd.MEM_DEVICE, cd.COPY_VALUES, buf.pointer()),
             lambda: L.CeedVectorTakeArray(v.h, cd.MEM_DEVICE, C.byref(p)),
             lambda: L.CeedVectorGetArrayRead(v.h, cd.MEM_DEVICE, C.byref(p)),
             lambda: L.CeedVectorGetArray(v.h, cd.MEM_DEVICE, C.byref(p)),
             lambda: L.CeedVectorSyncArray(v.h, cd.MEM_DEVICE)]
    for call in calls:
        with pytest.raises(cd.CeedError, match="no device memory"):
            call()
        assert not p
        assert vm.same_bits(v.to_numpy(), data)
        assert cd.out_value(L.CeedVectorGetLength, C.c_int32, v.h) == n
    assert vm.same_bits(buf.full, buf.snapshot()) and vm.same_bits(buf.window, data)
    v.destroy()


# ---- Vector.set_array(copy=False) borrows the caller's array or refuses ------------------------------------------------------------
def test_set_array_without_a_copy_writes_the_callers_array(oracle):
    n = 6
    x = oracle.vector(n).set_array(np.arange(1.0, n + 1))
    a = np.full(n, 3.0)
    v = oracle.vector(n).set_array(a, copy=False)
    v.axpby(2.0, x, 1.0)
    v.take_array()
    assert np.array_equal(a, 2.0 * np.arange(1.0, n + 1) + 3.0)
    e = np.zeros(0)
    oracle.vector(0).set_array(e, copy=False).take_array()


@pytest.mark.parametrize("what", ["float32", "strided", "read_only", "wrong_size", "list", "fortran_2d", "int64"])
def test_set_array_without_a_copy_refuses_what_it_would_have_to_convert(oracle, what):
    n = 6
    arr = {"float32": np.full(n, 3.0, dtype=np.float32), "strided": np.full(2 * n, 3.0)[::2], "read_only": np.full(n, 3.0),
           "wrong_size": np.full(n + 1, 3.0), "list": [3.0] * n, "fortran_2d": np.asfortranarray(np.full((2, 3), 3.0)),
           "int64": np.full(n, 3, dtype=np.int64)}[what]
    if what == "read_only":
        arr.setflags(write=False)
    before = np.array(arr, copy=True)
    x = oracle.vector(n).set_array(np.arange(1.0, n + 1))
    v = oracle.vector(n).set_array(np.full(n, 7.0))
    with pytest.raises(ValueError, match="copy=False"):
        v.set_array(arr, copy=False)
    assert np.array_equal(v.to_numpy(), np.full(n, 7.0))   # the vector is as it was, and so is the argument
    v.axpby(2.0, x, 1.0)
    assert np.array_equal(np.asarray(arr), before)
    # with a copy the same argument is converted, as before
    if what != "wrong_size":
        assert np.array_equal(oracle.vector(n).set_array(arr).to_numpy(), np.full(n, 3.0))
