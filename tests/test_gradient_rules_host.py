"""The host twins of pt_temporal_gradient and pt_temporal_accumulate_adaptive (csrc/pt_gradient.h, csrc/pt_temporal.h: the
functions pt_temporal_gradient_host and pt_temporal_accumulate_adaptive_host run) on the smallest frames where a tile, a tap or
a map index can go wrong, on the CPU under AddressSanitizer and UBSan with exactly-sized buffers
(tests/native/gradient_rules_check.cpp).  The GPU halves are the corner-case tests of test_temporal_gradient.py and
test_temporal_adaptive.py."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gradient_rules_stay_inside_their_buffers(tmp_path):
    exe = tmp_path / "gradient_rules_check"
    src = os.path.join(REPO, "tests", "native", "gradient_rules_check.cpp")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    "-I", os.path.join(REPO, "pathtracer_cuda_interactive_amd", "csrc"), src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
