"""pt_scene_create's refusals: status, pt_last_error text and — where a description carries two defects — which one is reported.

A table in the style of scene_update_cases.py's section C: each row is a mutation of a valid description, the status and the
exact text.  The rows cover every refusal that csrc/pt_scene_life.hip's validate_and_build and convert_tree can give (all but
"tie tables on the device failed", which no description provokes).  After every refusal *out is null and a valid create succeeds.

Shapes: the smallest on which each path can go wrong — one shape (the root is a leaf), two triangles, 17 shapes (from 16 up an
internal tree is built), 66 triangles on a chain (one level deeper than the traversal stack) for the host path; 4,096 shapes
(kDeviceSweepMin: records and trees are made on the device) for the device path, which must say what the host path says; the
test takes PT_SWEEP_BUILD out of the environment and asserts that the device made the valid scene's trees.  Two of the host path's
tree defects have no device row: the device validation (pt_scene_prep.hip: relay_tree_device) counts the references to every node
of the pool, reachable or not, so the pool that is one cycle and the root that is a leaf both read there as "BVH node referenced
twice" — what the host path says of them, "BVH is not a tree (cycle)" and "primitive not covered by any leaf", it says only
because it walks from the root.  That difference is the library's as it stands; this table pins what the two paths share.

The creates that succeed without an internal tree are pinned too: info fast_tree and pt_scene_rebuild's refusal with its reason."""
import ctypes as C

import numpy as np
import pytest
import scene_update_cases as suc

from pathtracer_cuda_interactive_amd import (PT_ERR_BAD_SCENE, PT_ERR_INVALID_ARG, PT_ERR_UNSUPPORTED, PT_LIGHT_DIFFUSE_AREA, PT_OK,
                                             host)
from pathtracer_cuda_interactive_amd import device as dev
from pathtracer_cuda_interactive_amd.ctypes_defs import PtLight, PtMaterial, PtMesh, PtSceneDesc

BAD = PT_ERR_BAD_SCENE
NO_SHAPES = "scene has no shapes"
NODE_COUNT = "BVH must have 2*num_shapes-1 nodes (bvh.cu:16-54)"
ROOT = "BVH root out of range"
NO_MATERIALS = "scene has no materials"
MESH_ARRAY = "bad mesh array"
LIGHT_ARRAY = "bad light array"
MATERIAL_TYPE = "unknown material type (scene.h:410 asserts)"
EMPTY_MESH = "empty mesh"
NO_NORMALS = "mesh without vertex normals (required, SURVEY H5a)"
MESH_MATERIAL = "mesh material id out of range"
SPHERE_MATERIAL, MESH_INDEX, FACE_INDEX, VERTEX_INDEX, SHAPE_TYPE = suc.ID_ERRORS
LEAF_PRIM = "leaf primitive id out of range"
CYCLE = "BVH is not a tree (cycle)"
NODE_TWICE = "BVH node referenced twice"
CHILD_RANGE = "BVH child index out of range"
PRIM_TWICE = "primitive referenced by two leaves"
PRIM_MISSING = "primitive not covered by any leaf"
TOO_DEEP = "BVH deeper than the traversal stack (reference cap 64, scene.h:251)"
AREA_LIGHT = "area light refers to a shape that does not exist"
REBUILD_REFUSED = "pt_scene_rebuild: the handle holds no tie tables, pt_scene_create kept no internal tree: "


# ---- valid descriptions -----------------------------------------------------------------------------------------------------

def scene(n_tris, n_spheres):
    """(desc, pool): suc.make_scene's triangles in two meshes (the second emissive) and spheres, on the host pipeline's tree."""
    d = suc.make_scene(n_tris, n_spheres, seed=n_tris + n_spheres).finalize()
    assert d.num_shapes == n_tris + n_spheres
    return d, pool(d)


def pool(d):
    return np.frombuffer(C.string_at(d.nodes, d.num_nodes * host.NODE_DTYPE.itemsize), dtype=host.NODE_DTYPE).copy()


def copy_of(d, **fields):
    d2 = PtSceneDesc()
    C.memmove(C.byref(d2), C.byref(d), C.sizeof(PtSceneDesc))
    d2._keep = [d]
    for k, v in fields.items():
        setattr(d2, k, v)
        d2._keep.append(v)
    return d2


def array_of(ctype, ptr, n):
    arr = (ctype * n)()
    C.memmove(arr, ptr, C.sizeof(arr))
    return arr


# ---- mutations: each takes a valid desc and returns a broken copy ------------------------------------------------------------

def fields(**kw):
    return lambda d: copy_of(d, **{k: (v(d) if callable(v) else v) for k, v in kw.items()})


def material_type(d):
    mats = array_of(PtMaterial, d.materials, d.num_materials)
    mats[d.num_materials - 1].type = 99
    return copy_of(d, materials=mats)


def mesh_edit(**kw):
    def edit(d):
        meshes = array_of(PtMesh, d.meshes, d.num_meshes)
        for k, v in kw.items():
            setattr(meshes[d.num_meshes - 1], k, v(d) if callable(v) else v)
        return copy_of(d, meshes=meshes)
    return edit


def bad_id(msg):
    """One shape's id wrong (suc.bad_id_descs: the geometry moved as well, which a create does not mind)."""
    return lambda d: suc.bad_id_descs(d)[msg]


def area_light(d):
    lights = array_of(PtLight, d.lights, d.num_lights)
    k = next(k for k in range(d.num_lights) if lights[k].type == PT_LIGHT_DIFFUSE_AREA)
    lights[k].shape_id = d.num_shapes
    return copy_of(d, lights=lights)


def nodes_edit(edit):
    def apply(d):
        nodes = pool(d)
        edit(d, nodes)
        return suc.with_nodes(d, nodes, root=d.root)
    return apply


def inner_below_root(d, nodes):
    """An inner node other than the root whose two children are an inner node (left) and anything."""
    return next(int(k) for k in np.flatnonzero(nodes["prim"] == -1) if k != d.root and nodes["prim"][nodes["left"][k]] == -1)


def leaves(nodes):
    return np.flatnonzero(nodes["prim"] >= 0)


def _leaf_prim(d, nodes):
    nodes["prim"][leaves(nodes)[d.num_shapes // 2]] = d.num_shapes


def _cycle(d, nodes):                       # every node an inner node whose two children are the next node: node 0 comes round again
    nodes["prim"][:] = -1
    nodes["left"][:] = nodes["right"][:] = (np.arange(len(nodes)) + 1) % len(nodes)


def _node_twice(d, nodes):                  # one inner child twice, the other child orphaned
    k = inner_below_root(d, nodes)
    nodes["right"][k] = nodes["left"][k]


def _child_range(d, nodes):
    nodes["left"][inner_below_root(d, nodes)] = len(nodes)


def _prim_twice(d, nodes):                  # a primitive in two leaves, another in none
    lv = leaves(nodes)
    nodes["prim"][lv[1]] = nodes["prim"][lv[2]]


def root_is_leaf(d):                        # a tree of one leaf over two shapes
    return copy_of(d, root=int(leaves(pool(d))[0]))


def chain(d):
    """All of d's shapes on one chain: as many levels as shapes."""
    N = d.num_shapes
    return suc.with_nodes(d, suc.tree_from_widths([1] * (N - 1), list(range(N))))


def deep_tail(d):
    """A complete tree down to 1,024 nodes a level, then 56 narrow levels: 68 levels with the leaves', every walk to the root far
    shorter than the device validation's cycle bound."""
    N = d.num_shapes
    widths = [1 << k for k in range(11)] + [37] * 55
    return suc.with_nodes(d, suc.tree_from_widths(widths + [N - 1 - sum(widths)], list(range(N))))


def shrunk_inner_box(d):
    """A valid tree whose boxes do not nest: the children of one inner node stick out of it."""
    nodes = pool(d)
    k = inner_below_root(d, nodes)
    ctr = 0.5 * (nodes["bmin"][k] + nodes["bmax"][k])
    nodes["bmin"][k], nodes["bmax"][k] = ctr + 0.5 * (nodes["bmin"][k] - ctr), ctr + 0.5 * (nodes["bmax"][k] - ctr)
    return suc.with_nodes(d, nodes, root=d.root)


def both(first, second):
    return lambda d: second(first(d))


LEAF_PRIM_EDIT, CYCLE_EDIT, NODE_TWICE_EDIT = nodes_edit(_leaf_prim), nodes_edit(_cycle), nodes_edit(_node_twice)
CHILD_RANGE_EDIT, PRIM_TWICE_EDIT = nodes_edit(_child_range), nodes_edit(_prim_twice)

# scene -> (triangles, spheres)
SCENES = {"one": (1, 0), "two": (2, 0), "s17": (14, 3), "chain66": (66, 0), "g4096": (4090, 6)}

# (scene, what, mutation, status, text).  Order within validate_and_build: the description's counts and pointers, materials,
# meshes, the shapes' ids, the tree, the lights.
ROWS = [
    # the description as a whole
    ("two", "no shapes", fields(num_shapes=0), BAD, NO_SHAPES),
    ("two", "null shapes", fields(shapes=None), BAD, NO_SHAPES),
    ("two", "one node too many", fields(num_nodes=lambda d: d.num_nodes + 1), BAD, NODE_COUNT),
    ("two", "null nodes", fields(nodes=None), BAD, NODE_COUNT),
    ("two", "root -1", fields(root=-1), BAD, ROOT),
    ("two", "root = num_nodes", fields(root=lambda d: d.num_nodes), BAD, ROOT),
    ("two", "no materials", fields(num_materials=0), BAD, NO_MATERIALS),
    ("two", "null materials", fields(materials=None), BAD, NO_MATERIALS),
    ("two", "num_meshes -1", fields(num_meshes=-1), BAD, MESH_ARRAY),
    ("two", "null meshes", fields(meshes=None), BAD, MESH_ARRAY),
    ("two", "num_lights -1", fields(num_lights=-1), BAD, LIGHT_ARRAY),
    ("two", "null lights", fields(lights=None), BAD, LIGHT_ARRAY),
    ("two", "material type 99", material_type, BAD, MATERIAL_TYPE),
    ("two", "mesh without vertices", mesh_edit(num_vertices=0), BAD, EMPTY_MESH),
    ("two", "mesh without faces", mesh_edit(num_faces=0), BAD, EMPTY_MESH),
    ("two", "mesh without positions", mesh_edit(positions=None), BAD, EMPTY_MESH),
    ("two", "mesh without indices", mesh_edit(indices=None), BAD, EMPTY_MESH),
    ("two", "mesh without normals", mesh_edit(normals=None), BAD, NO_NORMALS),
    ("two", "mesh material id", mesh_edit(material_id=lambda d: d.num_materials), BAD, MESH_MATERIAL),
    # primitive records
    ("s17", "sphere material id", bad_id(SPHERE_MATERIAL), BAD, SPHERE_MATERIAL),
    ("s17", "mesh index", bad_id(MESH_INDEX), BAD, MESH_INDEX),
    ("s17", "face index", bad_id(FACE_INDEX), BAD, FACE_INDEX),
    ("s17", "vertex index", bad_id(VERTEX_INDEX), BAD, VERTEX_INDEX),
    ("s17", "shape type", bad_id(SHAPE_TYPE), BAD, SHAPE_TYPE),
    # the caller's tree
    ("one", "root leaf names shape 1 of 1", nodes_edit(lambda d, n: n["prim"].fill(1)), BAD, LEAF_PRIM),
    ("s17", "leaf names shape N", LEAF_PRIM_EDIT, BAD, LEAF_PRIM),
    ("two", "cycle through every node", CYCLE_EDIT, BAD, CYCLE),
    ("s17", "inner child twice", NODE_TWICE_EDIT, BAD, NODE_TWICE),
    ("s17", "child = num_nodes", CHILD_RANGE_EDIT, BAD, CHILD_RANGE),
    ("s17", "primitive in two leaves", PRIM_TWICE_EDIT, BAD, PRIM_TWICE),
    ("two", "root is a leaf", root_is_leaf, BAD, PRIM_MISSING),
    ("chain66", "66 levels", chain, BAD, TOO_DEEP),
    # shading tables
    ("two", "area light on shape N", area_light, BAD, AREA_LIGHT),
    # two defects: the earlier check speaks
    ("two", "no shapes + null materials", both(fields(num_shapes=0), fields(materials=None)), BAD, NO_SHAPES),
    ("two", "null nodes + root -1", both(fields(nodes=None), fields(root=-1)), BAD, NODE_COUNT),
    ("two", "root -1 + material type", both(fields(root=-1), material_type), BAD, ROOT),
    ("two", "null lights + material type", both(fields(lights=None), material_type), BAD, LIGHT_ARRAY),
    ("two", "material type + empty mesh", both(material_type, mesh_edit(num_vertices=0)), BAD, MATERIAL_TYPE),
    ("two", "empty mesh without normals", mesh_edit(num_faces=0, normals=None), BAD, EMPTY_MESH),
    ("two", "no normals + mesh material id", mesh_edit(normals=None, material_id=-1), BAD, NO_NORMALS),
    ("s17", "mesh material id + sphere material id", both(bad_id(SPHERE_MATERIAL), mesh_edit(material_id=-1)), BAD, MESH_MATERIAL),
    ("s17", "vertex index + child = num_nodes", both(bad_id(VERTEX_INDEX), CHILD_RANGE_EDIT), BAD, VERTEX_INDEX),
    ("s17", "child = num_nodes + area light", both(CHILD_RANGE_EDIT, area_light), BAD, CHILD_RANGE),
    ("two", "cycle + area light", both(CYCLE_EDIT, area_light), BAD, CYCLE),
    # the device path: the host path's status and text for the same defect
    ("g4096", "null nodes", fields(nodes=None), BAD, NODE_COUNT),
    ("g4096", "mesh material id", mesh_edit(material_id=lambda d: d.num_materials), BAD, MESH_MATERIAL),
    ("g4096", "sphere material id", bad_id(SPHERE_MATERIAL), BAD, SPHERE_MATERIAL),
    ("g4096", "mesh index", bad_id(MESH_INDEX), BAD, MESH_INDEX),
    ("g4096", "face index", bad_id(FACE_INDEX), BAD, FACE_INDEX),
    ("g4096", "vertex index", bad_id(VERTEX_INDEX), BAD, VERTEX_INDEX),
    ("g4096", "shape type", bad_id(SHAPE_TYPE), BAD, SHAPE_TYPE),
    ("g4096", "leaf names shape N", LEAF_PRIM_EDIT, BAD, LEAF_PRIM),
    ("g4096", "inner child twice", NODE_TWICE_EDIT, BAD, NODE_TWICE),
    ("g4096", "child = num_nodes", CHILD_RANGE_EDIT, BAD, CHILD_RANGE),
    ("g4096", "primitive in two leaves", PRIM_TWICE_EDIT, BAD, PRIM_TWICE),
    ("g4096", "68 levels", deep_tail, BAD, TOO_DEEP),
    ("g4096", "area light on shape N", area_light, BAD, AREA_LIGHT),
    ("g4096", "vertex index + child = num_nodes", both(bad_id(VERTEX_INDEX), CHILD_RANGE_EDIT), BAD, VERTEX_INDEX),
    ("g4096", "child = num_nodes + area light", both(CHILD_RANGE_EDIT, area_light), BAD, CHILD_RANGE),
]


def create(d, out=True):
    """(status, pt_last_error, handle value) of one pt_scene_create; the handle starts out non-null."""
    h = C.c_void_p(0xdead)
    rc = dev.lib().pt_scene_create(C.byref(d) if d is not None else None, C.byref(h) if out else None)
    return rc, dev.lib().pt_last_error().decode(), h


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_refusals(name, monkeypatch):
    monkeypatch.delenv("PT_SWEEP_BUILD", raising=False)
    d, _ = scene(*SCENES[name])
    S = dev.DeviceScene(d)
    try:
        assert S.info("sweep_on_device") == (1 if name == "g4096" else 0), "which path prepares this scene"
    finally:
        S.close()
    assert d.num_lights > 0 or name == "one"
    rows = [r for r in ROWS if r[0] == name]
    assert rows
    for _, what, mutate, status, text in rows:
        rc, msg, h = create(mutate(d))
        print(f"{name}: {what}: status {rc}, {msg!r}")
        assert (rc, msg) == (status, text), (name, what)
        assert h.value is None, (name, what, "*out is not null")
        rc, msg, h = create(d)
        assert rc == PT_OK and h.value, (name, what, "the valid create that follows", rc, msg)
        assert dev.lib().pt_scene_destroy(h) == PT_OK


@pytest.mark.gpu
def test_null_arguments():
    d, _ = scene(*SCENES["two"])
    rc, msg, h = create(None)
    assert (rc, msg, h.value) == (PT_ERR_INVALID_ARG, "null scene description", None)
    rc, msg, _ = create(d, out=False)
    assert (rc, msg) == (PT_ERR_INVALID_ARG, "null output pointer")
    rc, msg, _ = create(fields(num_shapes=0)(d), out=False)             # two defects: the output pointer is looked at first
    assert (rc, msg) == (PT_ERR_INVALID_ARG, "null output pointer")


@pytest.mark.gpu
def test_creates_that_keep_no_internal_tree():
    d17, _ = scene(*SCENES["s17"])
    d15, _ = scene(12, 3)
    own_tree, _ = dev.build_bvh_sweep(d17)                             # the caller hands in the sweep tree itself: nothing to gain
    cases = [("15 shapes", d15, "fewer than 16 shapes"),
             ("boxes do not nest", shrunk_inner_box(d17), "the caller's boxes do not nest"),
             ("probe lost", own_tree, "the sweep tree lost the probe on an LDS-resident scene")]
    for what, d, why in cases:
        S = dev.DeviceScene(d)
        try:
            assert S.info("fast_tree") == 0, what
            rc = dev.lib().pt_scene_rebuild(S._h, 0)
            msg = dev.lib().pt_last_error().decode()
            print(f"{what}: status {rc}, {msg!r}")
            assert (rc, msg) == (PT_ERR_UNSUPPORTED, REBUILD_REFUSED + why), what
            assert S.info("rebuilds") == 0 and S.info("fast_tree") == 0
        finally:
            S.close()
