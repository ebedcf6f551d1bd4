"""The host twins of pt_gradient_pixels and pt_temporal_gradient_sparse (csrc/pt_gradient.h: the functions pt_gradient_pixels_host
and pt_temporal_gradient_sparse_host run) on the smallest frames where a tile, a tap, a clamp or a list entry can go wrong, on the
CPU under AddressSanitizer and UBSan with exactly-sized buffers (tests/native/gradient_sparse_check.cpp).  The GPU halves are the
corner-case tests of test_gradient_sparse.py."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sparse_gradient_rules_stay_inside_their_buffers(tmp_path):
    exe = tmp_path / "gradient_sparse_check"
    src = os.path.join(REPO, "tests", "native", "gradient_sparse_check.cpp")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    "-I", os.path.join(REPO, "pathtracer_cuda_interactive_amd", "csrc"), src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
