"""The refit plan and the level-by-level refit of csrc/pt_scene_refit.hip, restated in numpy (no GPU) and checked against
pt_host_refit_bvh.

The device keeps inner nodes only; a node carries the boxes of its two CHILDREN, so the box of node k lives in k's parent, in
child slot parent * 2 + side.  The plan (parent_slot, leaf_slot, nodes sorted by depth) is made from the array's own left /
right references; the refit writes the leaf boxes into their slots and then, deepest level first, every node's union of its
two child boxes into its own slot.  Each level is one vectorised step here, as it is one launch there: the steps of one level
must not depend on one another."""
import ctypes as C

import numpy as np
import pytest
from conftest import load_scene, random_scene

from pathtracer_cuda_interactive_amd import PT_SHAPE_SPHERE, host
from pathtracer_cuda_interactive_amd import device as dev
from pathtracer_cuda_interactive_amd.standins import mesh_arrays


def pool(desc):
    return np.frombuffer(C.string_at(desc.nodes, desc.num_nodes * host.NODE_DTYPE.itemsize), dtype=host.NODE_DTYPE).copy()


def inner_only(desc, seed):
    """The caller's pool as the device holds it: inner nodes only, the root first, the rest in a shuffled order; child
    references are inner indices or ~prim.  Boxes are left out: the refit has to make every one of them."""
    nodes = pool(desc)
    inner = [int(k) for k in np.flatnonzero(nodes["prim"] == -1) if k != desc.root]
    np.random.default_rng(seed).shuffle(inner)
    inner = [desc.root] + inner
    ident = {k: i for i, k in enumerate(inner)}
    ref = lambda k: ident[int(k)] if nodes["prim"][k] == -1 else ~int(nodes["prim"][k])
    child = np.array([[ref(nodes["left"][k]), ref(nodes["right"][k])] for k in inner], np.int64)
    return child, inner


def plan(child, n_prims):
    n = len(child)
    parent_slot, leaf_slot = np.full(n, -1, np.int64), np.full(n_prims, -1, np.int64)
    for side in (0, 1):
        c = child[:, side]
        k = np.arange(n)
        parent_slot[c[c >= 0]] = 2 * k[c >= 0] + side
        leaf_slot[~c[c < 0]] = 2 * k[c < 0] + side
    assert (leaf_slot >= 0).all() and (parent_slot[1:] >= 0).all() and parent_slot[0] == -1
    depth, v = np.zeros(n, np.int64), np.arange(n)
    while (v != 0).any():                                   # a walk to the root per node
        up = v != 0
        depth[up] += 1
        v[up] = parent_slot[v[up]] >> 1
    order = np.argsort(depth, kind="stable")
    level_begin = np.searchsorted(depth[order], np.arange(depth.max() + 2))
    return parent_slot, leaf_slot, order, level_begin


def leaf_boxes(d):
    out = np.zeros((d.num_shapes, 6), np.float32)
    meshes = {}
    for i in range(d.num_shapes):
        s = d.shapes[i]
        if s.type == PT_SHAPE_SPHERE:
            c, r = np.array(s.center[:], np.float32), np.float32(s.radius)
            out[i, :3], out[i, 3:] = c - r, c + r
        else:
            P, I, _ = meshes.setdefault(s.mesh_index, mesh_arrays(d, s.mesh_index))
            p0, p1, p2 = (P[v] for v in I[s.face_index])
            lo = np.where(p0 < p1, p0, p1)
            hi = np.where(p0 > p1, p0, p1)
            out[i, :3], out[i, 3:] = np.where(lo < p2, lo, p2), np.where(hi > p2, hi, p2)
    return out


def refit(child, n_prims, boxes):
    """slots[node * 2 + side] = the box of that child, [min xyz, max xyz]."""
    parent_slot, leaf_slot, order, level_begin = plan(child, n_prims)
    slots = np.full((2 * len(child), 6), np.nan, np.float32)
    slots[leaf_slot] = boxes
    for d in range(len(level_begin) - 2, 0, -1):
        ks = order[level_begin[d]:level_begin[d + 1]]
        a, b = slots[2 * ks], slots[2 * ks + 1]
        assert not np.isnan(a).any() and not np.isnan(b).any(), "a level read a box that no deeper level has written"
        slots[parent_slot[ks]] = np.concatenate([np.where(a[:, :3] < b[:, :3], a[:, :3], b[:, :3]),
                                                 np.where(a[:, 3:] > b[:, 3:], a[:, 3:], b[:, 3:])], axis=1)
    return slots


@pytest.mark.parametrize("name", ["cbox", "random7", "teapot"])
def test_plan_and_level_refit_reproduce_the_host_refit(name):
    d0 = random_scene(7).finalize() if name == "random7" else load_scene(name)[1]
    P, _, _ = mesh_arrays(d0, d0.num_meshes - 1)
    edits = {d0.num_meshes - 1: ((P * np.float32(0.8) + np.array([0.3, -0.5, 0.7], np.float32)).astype(np.float32), None)}
    spheres = {i: ((0.2, 0.6, 0.5), 0.55) for i in range(d0.num_shapes) if d0.shapes[i].type == PT_SHAPE_SPHERE}
    d1 = dev.edited_desc(d0, meshes=edits, spheres=dict(list(spheres.items())[:1]) or None)
    want = pool(host.refit_bvh(d1))
    child, inner = inner_only(d1, seed=3)
    slots = refit(child, d1.num_shapes, leaf_boxes(d1))
    assert not np.isnan(slots).any()
    for side, field in ((0, "left"), (1, "right")):
        kids = want[field][inner]
        assert np.array_equal(slots[side::2, :3], want["bmin"][kids]) and np.array_equal(slots[side::2, 3:], want["bmax"][kids])
    assert not np.array_equal(want["bmin"], pool(d0)["bmin"])
