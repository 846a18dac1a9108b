"""DevArray, the owner of every device array of the host layer (csrc/dev_array.hpp), exercised on the host alone: the stand-alone
program dev_array_host.cpp is built with g++ under the address and undefined-behaviour sanitizers, against malloc-backed stand-ins of
the three HIP calls the header uses (no HIP runtime is linked), and run as a child process.  It checks sizes 0 / 1 / 1000, moves,
re-upload, parking under a live graph and an allocation failing at each of an object's three arrays; any leak, double free or
sanitizer report fails it."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ceedpetscsolid_amd", "csrc")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_dev_array_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "dev_array_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",     # the runtimes inside the program: nothing about them depends on how it is started
           "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-isystem", ROCM_INCLUDE, os.path.join(HERE, "dev_array_host.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "dev_array_host ok" in run.stdout
    for word in ("Sanitizer", "runtime error", "FAIL"):     # the sanitizers and the program's own checks stayed silent
        assert word not in run.stderr, run.stderr
