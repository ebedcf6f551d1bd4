"""The wave-uniform bookkeeping of trace_kernel_v2's path bank (csrc/pt_path_bank.h) against a simulated work feed, on the
CPU under AddressSanitizer and UBSan: every work item handed out exactly once, slots in range, termination
(tests/native/path_bank_check.cpp).  The GPU half is tests/test_path_bank.py."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_path_bank_bookkeeping(tmp_path):
    exe = tmp_path / "path_bank_check"
    src = os.path.join(REPO, "tests", "native", "path_bank_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(REPO, "pathtracer_cuda_interactive_amd", "csrc"), src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
