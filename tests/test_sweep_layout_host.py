"""The tables a sweep launch stages in place of the octant node tables (csrc/pt_sweep_layout.h: box tables per octant, chained
slot records, the hit word) on the CPU under AddressSanitizer and UBSan (tests/native/sweep_layout_check.cpp).  The GPU half is
tests/test_sweep_layout.py."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sweep_layout") / "sweep_layout_check"
    src = os.path.join(REPO, "tests", "native", "sweep_layout_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(REPO, "pathtracer_cuda_interactive_amd", "csrc"), src, "-o", str(exe)], check=True)
    return str(exe)


def test_box_tables_chains_and_hit_words(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sweep_layout_check: ok" in r.stdout
