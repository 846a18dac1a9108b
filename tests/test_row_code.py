"""The stencil coder of the transpose maps (csrc/row_code.hpp) on the host alone: the stand-alone program row_code_host.cpp is built with
g++ under the address and undefined-behaviour sanitizers and run as a child process.  It encodes and decodes the maps of 2 x 2 x 2 and
3 x 3 x 3 boxes at P = 2, 3, 5 (whole and shell maps), a 12-contributor row, a row that is not ascending, empty maps, and the same
boxes under table limits of 4 and 0; the decoded (rowptr, cols) must be the map, and any sanitizer report fails it."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ceedpetscsolid_amd", "csrc")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_row_code_round_trip_under_sanitizers(tmp_path):
    exe = str(tmp_path / "row_code_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",     # the runtimes inside the program: nothing about them depends on how it is started
           "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-isystem", ROCM_INCLUDE, os.path.join(HERE, "row_code_host.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "row_code_host ok" in run.stdout
    for word in ("Sanitizer", "runtime error", "FAIL"):     # the sanitizers and the program's own checks stayed silent
        assert word not in run.stderr, run.stderr
