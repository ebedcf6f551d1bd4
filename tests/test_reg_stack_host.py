"""The register traversal stack of trace_kernel_v2 (csrc/pt_reg_stack.h) on the CPU under AddressSanitizer and UBSan: push and
pop against an array stack, the done value of an empty word, and the predicate that admits a launch
(tests/native/reg_stack_check.cpp).  The GPU half is tests/test_reg_stack.py."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reg_stack_operations(tmp_path):
    exe = tmp_path / "reg_stack_check"
    src = os.path.join(REPO, "tests", "native", "reg_stack_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(REPO, "pathtracer_cuda_interactive_amd", "csrc"), src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
