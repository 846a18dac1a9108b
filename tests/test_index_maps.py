"""The index arithmetic of set-up (csrc/index_maps.hpp) on the host alone: the stand-alone program index_maps_host.cpp is built with g++
under the address and undefined-behaviour sanitizers and run as a child process.  On boxes of 1, 2 and 3 elements per side at P = 2, 3, 5
(and a 6 x 6 x 6 box at P = 3 for the pipelined map) it checks the properties the device kernels rely on: every E-vector position in
exactly one row, its node's, contributors in element order; priority rows first; the interior nodes; the segments of the pipelined map
and its rows, each behind its last contributor; the Dirichlet flags; the owner map; the pack fold and the arrival lists of a halo.  On
the same boxes under masks whose nodes carry all eight component patterns, flagged_offsets, row_flag_bits, owner_map and the rows
pack_fold folds a halo into are held against loops over the L-vector entries: one mask byte, one flag bit.  Any sanitizer report or
failed check fails it."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ceedpetscsolid_amd", "csrc")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_index_maps_under_sanitizers(tmp_path):
    exe = str(tmp_path / "index_maps_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",     # the runtimes inside the program: nothing about them depends on how it is started
           "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-isystem", ROCM_INCLUDE, os.path.join(HERE, "index_maps_host.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "index_maps_host ok" in run.stdout
    assert "component patterns ok" in run.stdout      # flags, row flags, owner map and pack fold under masks of all eight node patterns
    for word in ("Sanitizer", "runtime error", "FAIL"):     # the sanitizers and the program's own checks stayed silent
        assert word not in run.stderr, run.stderr
