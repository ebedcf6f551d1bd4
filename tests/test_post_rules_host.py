"""The host twins of the four image-space stages (csrc/pt_denoise.h, csrc/pt_temporal.h: the functions pt_denoise_host,
pt_denoise_variance_host, pt_temporal_accumulate_host and pt_temporal_accumulate_moments_host run) on the smallest frames where
the clipping of a tap can go wrong, on the CPU under AddressSanitizer and UBSan with exactly-sized buffers
(tests/native/post_rules_check.cpp).  The GPU halves are the corner-case tests of test_denoise.py, test_denoise_variance.py,
test_temporal.py and test_temporal_moments.py."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_post_rules_stay_inside_their_buffers(tmp_path):
    exe = tmp_path / "post_rules_check"
    src = os.path.join(REPO, "tests", "native", "post_rules_check.cpp")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    "-I", os.path.join(REPO, "pathtracer_cuda_interactive_amd", "csrc"), src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
