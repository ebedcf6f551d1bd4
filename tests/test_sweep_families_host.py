"""The box sweep's PAIR2 records in front of the pair classes (csrc/pt_sweep_families.h) on the CPU under AddressSanitizer and
UBSan (tests/native/sweep_families_check.cpp): fixed and random sets of boxes, the leaf boxes of cbox, and those of the scenes
the GPU half (tests/test_sweep_families.py) renders.  The count model's sum for cbox is pinned here: at most 353, against
377 .. 381 for the pair classes."""
import os
import subprocess

import numpy as np
import pytest
from conftest import load_scene
from sweep_families_cases import CASES
from sweep_pairs_cases import triangle_boxes

from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sweep_families") / "sweep_families_check"
    src = os.path.join(REPO, "tests", "native", "sweep_families_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "pathtracer_cuda_interactive_amd", "csrc"), src, "-o", str(exe)],
                   check=True)
    return str(exe)


def classes_of(checker, boxes, path):
    """The info keys a launch would report for these leaf boxes, from the checker's line for mode "on" (first tree), and the
    model's sums of both modes (the largest over 8 random trees)."""
    boxes.tofile(path)
    r = subprocess.run([checker, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    w = r.stdout.split()
    assert [w[0], w[2], w[5], w[18], w[22], w[26], w[28]] == ["groups", "model", "pair2", "flat", "share", "general", "single"], r.stdout
    pair2 = np.array(w[6:18], int).reshape(3, 4)           # [u][fb + 2 fc]
    flat, share = np.array(w[19:22], int), np.array(w[23:26], int)
    info = {"groups": int(w[1]), "sweep_valu_model": int(w[3]), "model_pairs": int(w[4]),
            "sweep_pair2_records": int(pair2.sum()), "sweep_general_pairs": int(w[27]), "single": int(w[29])}
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        # a PAIR2 counts under each axis it shares (a is the lower shared axis where u > a, the upper one where u < a)
        for is_flat, key in ((1, "sweep_flat_pairs_"), (0, "sweep_share_pairs_")):
            n = (flat if is_flat else share)[a]
            for u in (b, c):
                for fl in range(4):
                    bit = fl & 1 if a == min(x for x in range(3) if x != u) else (fl >> 1) & 1
                    n += pair2[u][fl] if bit == is_flat else 0
            info[key + "xyz"[a]] = int(n)
    return info


def test_fixed_and_random_sets(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sweep_families_check: ok" in r.stdout


def test_cbox_model_counts(checker, tmp_path):
    """cbox's 25 leaf boxes under 8 random trees: six pairs share two axes.  The model's sum: at most 353, not above the pair
    classes' own."""
    _, d = load_scene("cbox")
    info = classes_of(checker, triangle_boxes(d), tmp_path / "cbox_boxes.bin")
    print(info)
    assert info["groups"] == 25 and info["single"] == 1
    assert info["sweep_valu_model"] <= 353
    assert info["sweep_valu_model"] <= info["model_pairs"] <= 381
    assert info["sweep_pair2_records"] >= 5


@pytest.mark.parametrize("name", sorted(CASES))
def test_scene_of_the_gpu_half(checker, tmp_path, name):
    make, groups, want = CASES[name]
    boxes = triangle_boxes(make().finalize(PT_BVH_SORT_REFERENCE))
    assert 16 <= len(boxes) <= 32
    if name == "signed_zero":
        flat_z = boxes[(boxes[:, 2] == 0) & (boxes[:, 5] == 0)]
        assert sorted(np.signbit(flat_z[:, 2]).tolist()) == [False] * 3 + [True] * 3, "the scene lost its -0.0 on the way"
        assert (np.signbit(flat_z[:, 2]) == np.signbit(flat_z[:, 5])).all()
    info = classes_of(checker, boxes, tmp_path / (name + ".bin"))
    print(name, info)
    assert info["groups"] == groups
    assert {k: info[k] for k in want} == want
