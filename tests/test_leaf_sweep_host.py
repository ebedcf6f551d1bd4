"""The group table and candidate mask of the leaf sweep (csrc/pt_leaf_sweep.h) on the CPU under AddressSanitizer and UBSan
(tests/native/leaf_sweep_check.cpp), and the table of the headline scene.  The GPU half is tests/test_leaf_sweep.py."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest
from conftest import load_scene

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("leaf_sweep") / "leaf_sweep_check"
    src = os.path.join(REPO, "tests", "native", "leaf_sweep_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(REPO, "pathtracer_cuda_interactive_amd", "csrc"), src, "-o", str(exe)], check=True)
    return str(exe)


def test_group_table_and_mask_operations(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_cbox_has_25_groups_13_of_them_pairs(checker, tmp_path):
    """The leaf boxes of cbox (the boxes of the caller's leaves: the internal tree is built over the same ones): 38 triangles,
    25 distinct boxes, 13 shared by the two triangles of a quad and 12 of one triangle each."""
    from pathtracer_cuda_interactive_amd import device as dev
    _, d = load_scene("cbox")
    nodes = np.frombuffer((C.c_char * (d.num_nodes * dev.NODE_DTYPE.itemsize)).from_address(C.addressof(d.nodes.contents)),
                          dtype=dev.NODE_DTYPE)
    leaves = nodes[nodes["prim"] >= 0]
    assert len(leaves) == d.num_shapes == 38
    boxes = np.zeros((38, 6), np.float32)
    boxes[leaves["prim"], :3] = leaves["bmin"]
    boxes[leaves["prim"], 3:] = leaves["bmax"]
    path = tmp_path / "cbox_boxes.bin"
    boxes.tofile(path)
    r = subprocess.run([checker, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert words[0] == "groups" and words[2] == "sizes", r.stdout
    sizes = [int(w) for w in words[3:]]
    assert int(words[1]) == len(sizes) == 25, r.stdout
    assert Counter(sizes) == {2: 13, 1: 12}, r.stdout
