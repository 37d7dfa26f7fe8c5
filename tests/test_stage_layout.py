"""The host entries' staging layout (distilp_amd/csrc/halda_stage.hpp) on the CPU: tests/stage_layout.cpp
includes the header's pure part alone (no HIP), is built with the host compiler under AddressSanitizer and
UBSan as a stand-alone program, and run. A missing compiler fails the test."""

import shutil
import subprocess

from .conftest import REPO

HIPCC = "/opt/rocm/bin/hipcc"


def test_stage_layout_arithmetic(tmp_path):
    exe = tmp_path / "stage_layout"
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", f"-I{REPO / 'include'}", f"-I{REPO / 'distilp_amd' / 'csrc'}",
             str(REPO / "tests" / "stage_layout.cpp"), "-o", str(exe)]
    gxx = shutil.which("g++")
    if gxx:
        cmd = [gxx] + flags
    else:
        assert shutil.which(HIPCC), "no host C++ compiler: neither g++ nor hipcc was found"
        cmd = [HIPCC] + flags  # a .cpp source: compiled as plain C++, host only
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "stage layout ok" in ran.stdout
