"""The box sweep's skip table (csrc/pt_sweep_skip.h) on the CPU under AddressSanitizer and UBSan
(tests/native/sweep_skip_check.cpp): the lemma that a triangle in the origin's axis-aligned plane is never kept, with the
library's own leaf-test arithmetic; the table against a brute-force grouping by (axis, float-equal c) in every order a launch
sweeps in, with the existing tables' bytes unchanged; and the kernel's rule — hit groups minus the skip word — over 2048 bounces
per scene: only tests the plain loop rejects are lost, the closest hit is bit-equal.  The scenes: fixed ones inside the checker,
cbox, and those of tests/sweep_pairs_cases.py and tests/sweep_skip_cases.py (which tests/test_sweep_skip.py renders on the GPU)."""
import os
import subprocess

import pytest
from conftest import load_scene
from sweep_pairs_cases import CASES as PAIR_CASES
from sweep_skip_cases import CASES, triangles

from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sweep_skip") / "sweep_skip_check"
    src = os.path.join(REPO, "tests", "native", "sweep_skip_check.cpp")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    "-I", os.path.join(REPO, "pathtracer_cuda_interactive_amd", "csrc"), src, "-o", str(exe)], check=True)
    return str(exe)


def counts_of(checker, tris, path):
    """The checker's line for a scene's triangles: groups, skip_groups, planes, skipped_tests, tests, on_plane, bounces."""
    tris.tofile(path)
    r = subprocess.run([checker, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sweep_skip_check: ok" in r.stdout
    w = r.stdout.split()
    assert [w[0], w[2], w[4], w[6], w[8], w[10], w[12]] == ["groups", "skip_groups", "planes", "skipped_tests", "of", "on_plane", "of"], r.stdout
    return {"groups": int(w[1]), "skip_groups": int(w[3]), "planes": int(w[5]), "skipped": int(w[7]), "tests": int(w[9]),
            "on_plane": int(w[11]), "bounces": int(w[13])}


def test_lemma_and_fixed_scenes(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "none kept" in r.stdout and "sweep_skip_check: ok" in r.stdout


def test_cbox(checker, tmp_path):
    """cbox: 25 groups, 15 of them flat on an axis (walls, floor, ceiling, light, block tops).  The ceiling and the light are
    different planes (548.8 and 548.7)."""
    _, d = load_scene("cbox")
    c = counts_of(checker, triangles(d), tmp_path / "cbox.bin")
    print(c)
    assert c["groups"] == 25 and c["skip_groups"] == 15
    assert c["skipped"] > 0 and c["on_plane"] > 0


@pytest.mark.parametrize("name", sorted(PAIR_CASES))
def test_scene_of_the_pairs(checker, tmp_path, name):
    make = PAIR_CASES[name][0]
    c = counts_of(checker, triangles(make().finalize(PT_BVH_SORT_REFERENCE)), tmp_path / (name + ".bin"))
    print(name, c)
    if name in ("flat", "full", "signed_zero", "flat_on_two_axes"):
        assert c["skip_groups"] > 0 and c["skipped"] > 0
    if name in ("share", "general"):
        assert c["skip_groups"] == 0 and c["skipped"] == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_scene_of_the_gpu_half(checker, tmp_path, name):
    make, want = CASES[name]
    c = counts_of(checker, triangles(make().finalize(PT_BVH_SORT_REFERENCE)), tmp_path / (name + ".bin"))
    print(name, c)
    assert {k: c[k] for k in want} == want
