"""The index arithmetic of a surface load (csrc/index_maps.hpp as csrc/ceed_surface.cpp calls it) on the host alone: the stand-alone
program surface_maps_host.cpp is built with g++ under the address and undefined-behaviour sanitizers and run as a child process.  Patches
of 1 x 1 ... 2 x 3 faces at P = 2, 5, 8 under a numbering with gaps: the face offsets with and without a mask (a load without a mask
must not read one), the faces' transpose map (every E position in exactly one row, contributors in face order, the valences of a
patch) and the mask in row order; the empty load.  Any sanitizer report or failed check fails it."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ceedpetscsolid_amd", "csrc")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_surface_maps_under_sanitizers(tmp_path):
    exe = str(tmp_path / "surface_maps_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",     # the runtimes inside the program: nothing about them depends on how it is started
           "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-isystem", ROCM_INCLUDE, os.path.join(HERE, "surface_maps_host.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "surface_maps_host ok" in run.stdout
    for word in ("Sanitizer", "runtime error", "FAIL"):     # the sanitizers and the program's own checks stayed silent
        assert word not in run.stderr, run.stderr
