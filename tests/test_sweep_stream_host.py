"""The sweep kernel's record stream (csrc/pt_kernels.h: SweepWindow) as a CPU model under AddressSanitizer and UBSan
(tests/native/sweep_stream_check.cpp): every body receives exactly its record's bytes from the window the body before it read,
the furthest byte read is sweep_stream_end's (csrc/pt_sweep_families.h) and lies inside the staged region, the hit words are the
plain loop's.  Fixed sets (every class alone, every ordered pair of classes), random sets, the leaf boxes of cbox, and those of
the scenes the GPU half (tests/test_sweep_stream.py) renders, whose classes are pinned here."""
import os
import subprocess

import pytest
from conftest import load_scene
from sweep_pairs_cases import triangle_boxes
from sweep_stream_cases import GENERAL, N_CLASSES, SINGLE, TRANSITIONS, octants_of_the_views

from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sweep_stream") / "sweep_stream_check"
    src = os.path.join(REPO, "tests", "native", "sweep_stream_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "pathtracer_cuda_interactive_amd", "csrc"), src, "-o", str(exe)],
                   check=True)
    return str(exe)


def stream_of(checker, boxes, path, trees=8):
    """The checker's line for these leaf boxes: groups, the model's sum, the stream's end and the staged bytes, and the records
    per class, the 20 classes in table order."""
    boxes.tofile(path)
    r = subprocess.run([checker, str(path), str(trees)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    w = r.stdout.split()
    assert [w[0], w[2], w[4], w[6], w[8], w[21], w[25], w[29], w[31]] == \
        ["groups", "model", "stream_end", "staged", "pair2", "flat", "share", "general", "single"], r.stdout
    classes = [int(x) for x in w[9:21] + w[22:25] + w[26:29] + [w[30], w[32]]]
    return {"groups": int(w[1]), "sweep_valu_model": int(w[3]), "stream_end": int(w[5]), "staged": int(w[7]), "classes": classes,
            "sweep_pair2_records": sum(classes[:12]), "sweep_general_pairs": classes[GENERAL], "single": classes[SINGLE]}


def test_fixed_and_random_sets(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sweep_stream_check: ok" in r.stdout


def test_cbox(checker, tmp_path):
    """cbox's 25 leaf boxes under 8 random trees: PAIR2 records, sharing pairs and the single in one stream."""
    _, d = load_scene("cbox")
    s = stream_of(checker, triangle_boxes(d), tmp_path / "cbox_boxes.bin")
    print(s)
    assert s["groups"] == 25 and s["single"] == 1 and s["sweep_pair2_records"] >= 5
    assert s["stream_end"] <= s["staged"]


def test_scenes_of_the_gpu_half(checker, tmp_path):
    """Each of the 190 scenes holds one record of each of the two classes its name says and nothing else, in groups of equal boxes."""
    for name, (a, b, make, groups, per, want) in TRANSITIONS.items():
        boxes = triangle_boxes(make().finalize(PT_BVH_SORT_REFERENCE))
        assert 16 <= len(boxes) == groups * per <= 32, name
        s = stream_of(checker, boxes, tmp_path / "boxes.bin", trees=1)
        assert s["groups"] == groups, (name, s)
        assert s["classes"] == [int(c in (a, b)) for c in range(N_CLASSES)], (name, s)
        assert {k: s[k] for k in want} == want, (name, s)
        assert s["stream_end"] <= s["staged"], (name, s)


def test_views_look_into_every_octant():
    """Pixel centres, several per octant (the renderers jitter inside the pixel): octant 7, whose table is the last, among them."""
    n = octants_of_the_views()
    print(n)
    assert (n >= 4).all(), n
