"""The range and overlap arithmetic of the block-vector entry points (csrc/block_args.hpp) on the host alone: the stand-alone program
block_args_host.cpp is built with g++ under the address and undefined-behaviour sanitizers and run as a child process."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ceedpetscsolid_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_block_args_under_sanitizers(tmp_path):
    exe = str(tmp_path / "block_args_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan",     # the runtimes inside the program: nothing about them depends on how it is started
           "-I", CSRC, os.path.join(HERE, "block_args_host.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "block_args_host ok" in run.stdout
    for word in ("Sanitizer", "runtime error", "FAIL"):     # the sanitizers and the program's own checks stayed silent
        assert word not in run.stderr, run.stderr
