"""What the path bank carries of a work item's index (csrc/pt_path_index.h: the scratch-buffer slot and the 64-bit PCG increment
in three words per slot) against plain divisions over a simulated work feed, on the CPU under AddressSanitizer and UBSan:
short fills, empty bands, chunk ends, both item orders, row selections, streams beyond 32 bits
(tests/native/bank_index_check.cpp).  The GPU half is tests/test_bank_index.py."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bank_index_words(tmp_path):
    exe = tmp_path / "bank_index_check"
    src = os.path.join(REPO, "tests", "native", "bank_index_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(REPO, "pathtracer_cuda_interactive_amd", "csrc"), src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
