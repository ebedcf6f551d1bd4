"""The box sweep's groups paired by shared axis intervals and its box tables in class order (csrc/pt_sweep_pairs.h) on the CPU
under AddressSanitizer and UBSan (tests/native/sweep_pairs_check.cpp): fixed and random sets of boxes, the leaf boxes of cbox,
and those of the scenes the GPU half (tests/test_sweep_pairs.py) renders."""
import os
import subprocess

import numpy as np
import pytest
from conftest import load_scene
from sweep_pairs_cases import CASES, GROUPS, triangle_boxes

from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sweep_pairs") / "sweep_pairs_check"
    src = os.path.join(REPO, "tests", "native", "sweep_pairs_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "pathtracer_cuda_interactive_amd", "csrc"), src, "-o", str(exe)],
                   check=True)
    return str(exe)


def classes_of(checker, boxes, path, min_sharing=0):
    boxes.tofile(path)
    r = subprocess.run([checker, str(path), str(min_sharing)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    w = r.stdout.split()
    assert [w[0], w[2], w[6], w[10], w[12]] == ["groups", "flat", "share", "general", "single"], r.stdout
    info = {"groups": int(w[1]), "sweep_general_pairs": int(w[11]), "single": int(w[13])}
    for k, a in enumerate("xyz"):
        info["sweep_flat_pairs_" + a], info["sweep_share_pairs_" + a] = int(w[3 + k]), int(w[7 + k])
    info["sweep_flat_pairs"] = sum(info["sweep_flat_pairs_" + a] for a in "xyz")
    info["sweep_share_pairs"] = sum(info["sweep_share_pairs_" + a] for a in "xyz")
    return info


def test_fixed_and_random_sets(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sweep_pairs_check: ok" in r.stdout


def test_cbox_has_at_least_10_sharing_pairs(checker, tmp_path):
    """cbox's 25 distinct leaf boxes have 8 distinct y intervals, 12 of the boxes flat on y: under every order of the groups
    (8 random trees) at least 10 of the 12 pairs share an interval."""
    _, d = load_scene("cbox")
    info = classes_of(checker, triangle_boxes(d), tmp_path / "cbox_boxes.bin", min_sharing=10)
    print(info)
    assert info["groups"] == 25 and info["single"] == 1
    assert info["sweep_flat_pairs"] + info["sweep_share_pairs"] >= 10
    assert info["sweep_flat_pairs"] >= 4


@pytest.mark.parametrize("name", sorted(CASES))
def test_scene_of_the_gpu_half(checker, tmp_path, name):
    make, above_zero, zero = CASES[name]
    boxes = triangle_boxes(make().finalize(PT_BVH_SORT_REFERENCE))
    assert 16 <= len(boxes) <= 32
    if name == "signed_zero":
        flat_z = boxes[(boxes[:, 2] == 0) & (boxes[:, 5] == 0)]
        assert sorted(np.signbit(flat_z[:, 2]).tolist()) == [False, False, True, True], "the scene lost its -0.0 on the way"
    info = classes_of(checker, boxes, tmp_path / (name + ".bin"))
    print(name, info)
    assert info["groups"] == GROUPS[name]
    for k in above_zero:
        assert info[k] > 0, (k, info)
    for k in zero:
        assert info[k] == 0, (k, info)
