"""The pure parts of libhalda's launch bookkeeping (distilp_amd/csrc/halda_launch.hpp) on the CPU: the launch
record's slots against the five booleans it replaced, the families' path ranges and messages, the scoped path
override and result_slice. tests/launch_record.cpp includes that header and the public ones alone (no HIP), is
built with the host compiler under AddressSanitizer and UBSan as a stand-alone program, and run. A missing
compiler fails the test."""

import shutil
import subprocess

from .conftest import REPO

HIPCC = "/opt/rocm/bin/hipcc"


def test_launch_record_slots_knobs_and_slices(tmp_path):
    exe = tmp_path / "launch_record"
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", f"-I{REPO / 'include'}", f"-I{REPO / 'distilp_amd' / 'csrc'}",
             str(REPO / "tests" / "launch_record.cpp"), "-o", str(exe)]
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
    assert "launch record ok" in ran.stdout
