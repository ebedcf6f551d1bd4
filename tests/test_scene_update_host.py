"""Host half of pt_scene_update (no GPU): pt_host_refit_bvh keeps a node pool's topology and makes every box anew,
pt_host_compute_normals exposes the normals add_mesh computes, and pt_scene_update refuses bad arguments before it touches HIP."""
import ctypes as C
import os

import numpy as np
import pytest
from conftest import DATA, load_scene, random_scene

from pathtracer_cuda_interactive_amd import PT_ERR_INVALID_ARG, PT_MAT_DIFFUSE, PT_SHAPE_SPHERE, HostScene, host
from pathtracer_cuda_interactive_amd import device as dev
from pathtracer_cuda_interactive_amd.standins import mesh_arrays


def pool(desc):
    """The node pool of a desc as a structured array (copy)."""
    return np.frombuffer(C.string_at(desc.nodes, desc.num_nodes * host.NODE_DTYPE.itemsize), dtype=host.NODE_DTYPE).copy()


def scene(name):
    if name.startswith("random"):
        hs = random_scene(int(name[6:]))
        return hs.finalize()
    return load_scene(name)[1]


@pytest.mark.parametrize("name", ["cbox", "teapot", "scene4", "single_triangle", "random1", "random2", "random3"])
def test_refit_of_an_unedited_scene_returns_the_pool_byte_for_byte(name):
    d = scene(name)
    got = host.refit_bvh(d)
    assert got.num_nodes == d.num_nodes and got.root == d.root
    assert pool(got).tobytes() == pool(d).tobytes()


def numpy_refit(d):
    """The rule restated: leaf box = shape box, inner box = union of the two children's, children before parents; min and max
    as np.where(a < b, a, b) / np.where(a > b, a, b) with the left child's value as a."""
    nodes = pool(d)
    order, todo = [], [d.root]
    while todo:
        k = todo.pop()
        order.append(k)
        if nodes["prim"][k] == -1:
            todo += [int(nodes["left"][k]), int(nodes["right"][k])]
    for k in reversed(order):
        prim = int(nodes["prim"][k])
        if prim != -1:
            s = d.shapes[prim]
            if s.type == PT_SHAPE_SPHERE:
                c, r = np.array(s.center[:], np.float32), np.float32(s.radius)
                lo, hi = c - r, c + r
            else:
                P, I, _ = mesh_arrays(d, s.mesh_index)
                p0, p1, p2 = (P[v] for v in I[s.face_index])
                lo = np.where(p0 < p1, p0, p1); lo = np.where(lo < p2, lo, p2)
                hi = np.where(p0 > p1, p0, p1); hi = np.where(hi > p2, hi, p2)
        else:
            a, b = nodes[nodes["left"][k]], nodes[nodes["right"][k]]
            lo = np.where(a["bmin"] < b["bmin"], a["bmin"], b["bmin"])
            hi = np.where(a["bmax"] > b["bmax"], a["bmax"], b["bmax"])
        nodes["bmin"][k], nodes["bmax"][k] = lo, hi
    return nodes


def test_refit_of_an_edited_scene_equals_the_numpy_restatement():
    hs = random_scene(7)
    d = hs.finalize()
    P, _, _ = mesh_arrays(d, 0)
    moved = (P * np.float32(0.8) + np.array([0.5, -0.3, 0.6], np.float32)).astype(np.float32)
    sphere = next(i for i in range(d.num_shapes) if d.shapes[i].type == PT_SHAPE_SPHERE)
    d1 = dev.edited_desc(d, meshes={0: (moved, None)}, spheres={sphere: ((0.9, 0.4, -0.7), 0.33)})
    before, got, want = pool(d), pool(host.refit_bvh(d1)), numpy_refit(d1)
    assert got.tobytes() == want.tobytes()
    for f in ("left", "right", "prim"):
        assert np.array_equal(got[f], before[f])
    # the edit did move boxes, the sphere's leaf among them
    assert (got["bmin"] != before["bmin"]).any()
    leaf = int(np.flatnonzero(got["prim"] == sphere)[0])
    assert np.array_equal(got["bmin"][leaf], np.array([0.9, 0.4, -0.7], np.float32) - np.float32(0.33))
    assert not np.array_equal(before["bmin"][leaf], got["bmin"][leaf])


def read_obj(path):
    """v / f lines of a normal-free OBJ; polygons as the fan (0, 1, 2), (0, 2, 3), ... the host loader makes."""
    V, F = [], []
    for line in open(path):
        t = line.split()
        if t and t[0] == "v":
            V.append([float(x) for x in t[1:4]])
        elif t and t[0] == "f":
            idx = [int(x.split("/")[0]) - 1 for x in t[1:]]
            F += [[idx[0], idx[k], idx[k + 1]] for k in range(1, len(idx) - 1)]
    return np.array(V, np.float32), np.array(F, np.int32)


def random_mesh(seed, n_tris=200):
    rng = np.random.default_rng(seed)
    P = (rng.random((120, 3)) * 2 - 1).astype(np.float32)
    I = rng.integers(0, 120, (n_tris, 3)).astype(np.int32)
    I[5] = (3, 3, 9)                                    # a degenerate face: contributes nothing
    return P, I


@pytest.mark.parametrize("mesh", ["pyramid", "random"])
def test_compute_normals_equals_what_add_mesh_stored(mesh):
    P, I = read_obj(os.path.join(DATA, "pyramid.obj")) if mesh == "pyramid" else random_mesh(3)
    assert I.shape == ((6, 3) if mesh == "pyramid" else (200, 3))
    hs = HostScene()
    hs.add_mesh(P, I, hs.add_material(PT_MAT_DIFFUSE, (0.5, 0.5, 0.5)))
    d = hs.finalize()
    _, _, stored = mesh_arrays(d, 0)
    got = host.compute_normals(P, I)
    assert got.dtype == np.float32 and got.shape == P.shape and got.tobytes() == stored.tobytes()


def test_update_refuses_bad_arguments_before_any_hip_call():
    _, d = load_scene("cbox")
    lib = dev.lib()
    # a handle that is never dereferenced: every one of these is refused on the arguments alone
    bogus = C.c_void_p(16)
    cases = [(None, C.byref(d), 1, "scene"), (bogus, None, 1, "description"), (bogus, C.byref(d), 0, "flags"),
             (bogus, C.byref(d), 8, "flags"), (bogus, C.byref(d), 1 | 8, "flags")]
    for scene, desc, flags, word in cases:
        assert lib.pt_scene_update(scene, desc, flags) == PT_ERR_INVALID_ARG
        assert word in lib.pt_last_error().decode()
