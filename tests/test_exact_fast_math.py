"""The exact short sequences of csrc/pt_math.h (rcp_exact, div_pi_exact, sqrt_exact) against the IEEE expressions
they replace on the hot path (1.0f / x, x / kPi, sqrtf(x)): bit for bit on all 2^32 fp32 inputs.
The device check runs each primitive as compiled for gfx950; div_pi_exact's fast path uses only IEEE * and fma, so it
is also checked on the CPU."""
import os
import subprocess

import pytest

from pathtracer_cuda_interactive_amd import PT_EXACT_DIV_PI, PT_EXACT_RAW_RCP, PT_EXACT_RCP, PT_EXACT_SQRT
from pathtracer_cuda_interactive_amd import device as dev

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 1 << 28


@pytest.mark.gpu
@pytest.mark.parametrize("op,name", [(PT_EXACT_RCP, "rcp_exact"), (PT_EXACT_DIV_PI, "div_pi_exact"),
                                     (PT_EXACT_SQRT, "sqrt_exact")])
def test_device_primitive_is_exact_on_every_input(op, name):
    total, first = 0, -1
    for begin in range(0, 1 << 32, CHUNK):
        bad, f = dev.debug_exact_math(op, begin, CHUNK)
        total += bad
        if bad and first < 0:
            first = f
    assert total == 0, f"{name}: {total} inputs differ from the IEEE result, first bit pattern 0x{first:08x}"


@pytest.mark.gpu
def test_device_check_sees_a_difference():
    """Control: the bare v_rcp_f32 is not correctly rounded, so the same check must report mismatches and point at one
    of them.  A range past 2^32 is refused."""
    bad, first = dev.debug_exact_math(PT_EXACT_RAW_RCP, 0, 1 << 32)
    assert bad > 0 and first >= 0
    assert dev.debug_exact_math(PT_EXACT_RAW_RCP, first, 1)[0] == 1
    assert dev.debug_exact_math(PT_EXACT_RCP, first, 1) == (0, -1)
    assert dev.debug_exact_math(PT_EXACT_RCP, first, 0) == (0, -1)
    with pytest.raises(dev.PtError):
        dev.debug_exact_math(PT_EXACT_RCP, (1 << 32) - 4, 8)


def test_div_pi_fast_path_is_exact_on_every_input(tmp_path):
    exe = tmp_path / "div_pi_check"
    src = os.path.join(REPO, "tests", "native", "div_pi_check.cpp")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(rocm, "include"),
                    "-I", os.path.join(REPO, "pathtracer_cuda_interactive_amd", "csrc"), src, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    assert "mismatches 0 " in r.stdout
