"""Input makers for tests/test_scene_update_contract.py, in plain numpy (no GPU): caller's trees of a chosen shape, the scenes
they stand over, and the edits pt_scene_update's contract allows beyond moved vertices (include/pt_api.h, PT_UPDATE_GEOMETRY).

Everything here is made once per name, shared between the tests that need it and left unchanged."""
import ctypes as C
import functools

import numpy as np
from test_scene_update_plan import inner_only, plan

from pathtracer_cuda_interactive_amd import (PT_MAT_DIFFUSE, PT_MAT_MIRROR, PT_MAT_PHONG, PT_MAT_PLASTIC, PT_SHAPE_SPHERE,
                                             PT_SHAPE_TRIANGLE, PT_TRAVERSAL_EXACT, HostScene, host)
from pathtracer_cuda_interactive_amd import device as dev
from pathtracer_cuda_interactive_amd.ctypes_defs import PtBvhNode, PtSceneDesc, PtShape
from pathtracer_cuda_interactive_amd.standins import mesh_arrays

# csrc/pt_scene_refit.hip, restated: a level of at most K_NARROW nodes is "narrow"; a tree of at most K_WHOLE_TREE_NODES inner
# nodes whose levels are all narrow is refitted by one launch
K_NARROW = 1024
K_WHOLE_TREE_NODES = 4096

W, H, SPP = 64, 48, 2
SHAPE_DT = np.dtype([("type", "<i4"), ("material_id", "<i4"), ("area_light_id", "<i4"), ("center", "<f4", 3), ("radius", "<f4"),
                     ("face_index", "<i4"), ("mesh_index", "<i4")])
assert SHAPE_DT.itemsize == C.sizeof(PtShape)

NONE, ONE_LAUNCH, LEVELS_AND_TOP, TOP_ALONE = "none", "one launch", "levels + top", "top alone"
# info "refit_shape0" / "refit_shape1" (include/pt_api.h)
REFIT_SHAPE = {0: NONE, 1: ONE_LAUNCH, 2: LEVELS_AND_TOP, 3: TOP_ALONE}


# ---- trees ------------------------------------------------------------------------------------------------------------------

def tree_from_widths(widths, leaf_prims):
    """The node pool (host.NODE_DTYPE, boxes zero, root 0) of a binary tree with widths[d] inner nodes at depth d over
    len(leaf_prims) = sum(widths) + 1 leaves.  Inner nodes come first, level by level; the inner nodes of level d + 1 hang from
    those of level d in order: one under each parent as its LEFT child, what is left over as the RIGHT child of the first
    parents.  Every other child is a leaf; the leaves take leaf_prims in depth-first order, left subtree first."""
    widths = [int(w) for w in widths]
    n_inner, N = sum(widths), sum(widths) + 1
    assert len(leaf_prims) == N and sorted(leaf_prims) == list(range(N))
    nodes = np.zeros(2 * N - 1, dtype=host.NODE_DTYPE)
    nodes["left"], nodes["right"], nodes["prim"] = -1, -1, -1
    if N == 1:
        nodes["prim"][0] = leaf_prims[0]
        return nodes
    assert widths[0] == 1 and all(1 <= b <= 2 * a for a, b in zip(widths, widths[1:]))
    begin = np.concatenate([[0], np.cumsum(widths)])
    child = np.full((n_inner, 2), -1, np.int64)
    for d in range(len(widths) - 1):
        w, wn = widths[d], widths[d + 1]
        first = min(w, wn)
        child[begin[d]:begin[d] + first, 0] = begin[d + 1] + np.arange(first)
        child[begin[d]:begin[d] + wn - first, 1] = begin[d + 1] + first + np.arange(wn - first)
    leaf, todo = 0, [(0, 1), (0, 0)]
    while todo:
        k, side = todo.pop()
        c = child[k, side]
        if c < 0:
            c = n_inner + leaf
            nodes["prim"][c] = leaf_prims[leaf]
            leaf += 1
        else:
            todo += [(c, 1), (c, 0)]
        nodes["right" if side else "left"][k] = c
    assert leaf == N
    return nodes


def with_nodes(d, nodes, root=0):
    d2 = PtSceneDesc()
    C.memmove(C.byref(d2), C.byref(d), C.sizeof(PtSceneDesc))
    nodes = np.ascontiguousarray(nodes)
    d2.nodes = nodes.ctypes.data_as(C.POINTER(PtBvhNode))
    d2.num_nodes, d2.root = len(nodes), int(root)
    d2._keep = (nodes, d)
    return d2


def level_widths(desc):
    """Inner nodes per depth of desc's tree, through test_scene_update_plan's restatement of the device's plan."""
    if desc.num_shapes < 2:
        return []
    child, _ = inner_only(desc, seed=1)
    level_begin = plan(child, desc.num_shapes)[3]
    return [int(w) for w in np.diff(level_begin)]


def classify(widths):
    """Which launches ptf::refit_tree makes for a tree of these level widths (ptf::plan_build's rule)."""
    if not widths:
        return NONE
    levels = len(widths)
    top = 0
    while top + 1 < levels and widths[top + 1] <= K_NARROW:
        top += 1
    if top == levels - 1 and sum(widths) <= K_WHOLE_TREE_NODES:
        return ONE_LAUNCH
    return TOP_ALONE if top == levels - 1 else LEVELS_AND_TOP


def tree_depth(desc):
    """Levels of desc's tree, the leaves' counting (pt_scene_create accepts up to 64)."""
    return len(level_widths(desc)) + 1


# ---- scenes -----------------------------------------------------------------------------------------------------------------

def shape_table(d):
    return np.frombuffer(C.string_at(d.shapes, d.num_shapes * SHAPE_DT.itemsize), dtype=SHAPE_DT).copy()


def as_shapes(table):
    table = np.ascontiguousarray(table, dtype=SHAPE_DT)
    return (PtShape * len(table)).from_buffer_copy(table.tobytes())


def mesh_table(d):
    """desc's meshes in edited_desc's mesh_list form."""
    return [mesh_arrays(d, m) + (d.meshes[m].material_id, d.meshes[m].area_light_id) for m in range(d.num_meshes)]


def centroids(d):
    shp = shape_table(d)
    c = shp["center"].astype(np.float64)
    for m in range(d.num_meshes):
        P, I, _ = mesh_arrays(d, m)
        sel = (shp["type"] == PT_SHAPE_TRIANGLE) & (shp["mesh_index"] == m)
        c[sel] = P[I[shp["face_index"][sel]]].astype(np.float64).mean(axis=1)
    return c


def make_scene(n_tris, n_spheres, seed, n_meshes=2, diffuse_only=False, emissive_sphere=True):
    """Small random triangles in n_meshes meshes (the last one emissive) and a few spheres, seen by conftest.random_scene's
    camera.  The triangles shrink with their number so that a ray meets a handful of them."""
    rng = np.random.default_rng(seed)
    hs = HostScene()
    hs.set_camera((0, 0.5, 4.0), (0, 0, 0), (0, 1, 0), 50.0, W, H, SPP)
    hs.set_background((0.4, 0.5, 0.6))
    kinds = [PT_MAT_DIFFUSE] * 4 if diffuse_only else [PT_MAT_DIFFUSE, PT_MAT_MIRROR, PT_MAT_PLASTIC, PT_MAT_PHONG]
    mats = [hs.add_material(kinds[0], rng.random(3) * 0.8 + 0.1), hs.add_material(kinds[1], rng.random(3) * 0.5 + 0.5),
            hs.add_material(kinds[2], rng.random(3) * 0.8 + 0.1, eta=1.5), hs.add_material(kinds[3], rng.random(3) * 0.8 + 0.1, exponent=20.0)]
    size = min(1.5, 4.0 * max(n_tris + n_spheres, 1) ** (-1.0 / 3.0))
    if n_tris:
        # a handful of shapes stay near the middle of the frame, where the camera sees them
        c = ((rng.random((n_tris, 1, 3)) * 4 - 2) * min(1.0, (n_tris + n_spheres) / 16)).astype(np.float32)
        P = (c + (rng.random((n_tris, 3, 3)) - 0.5).astype(np.float32) * np.float32(size)).astype(np.float32)
        n_meshes = min(n_meshes, n_tris)
        cuts = [n_tris * k // n_meshes for k in range(n_meshes + 1)]
        for k in range(n_meshes):
            Pk = P[cuts[k]:cuts[k + 1]].reshape(-1, 3)
            hs.add_mesh(Pk, np.arange(len(Pk), dtype=np.int32).reshape(-1, 3), mats[k % 4],
                        radiance=(3.0, 2.5, 2.0) if k == n_meshes - 1 and n_meshes > 1 else None)
    for k in range(n_spheres):
        hs.add_sphere(rng.random(3) * 3 - 1.5, (0.2 + float(rng.random()) * 0.5) * min(1.0, 2 * size), mats[(k + 1) % 4],
                      radiance=(4.0, 4.0, 1.0) if (emissive_sphere and k == 0) else None)
    return hs


def params_of(hs, seed=11):
    p = hs.render_params(W, H, SPP, seed=seed)
    p.traversal = PT_TRAVERSAL_EXACT
    return p


def moved_geometry(d, step=1):
    """Every mesh wobbled with its normals computed anew, every sphere moved and resized."""
    e = dev.wobbled_desc(d, step, amp=0.03) if d.num_meshes else d
    shp = shape_table(d)
    spheres = {int(i): (shp["center"][i] + np.float32(0.15 * step) * np.array([1, -0.5, 0.7], np.float32), float(shp["radius"][i]) * (1 - 0.2 * step))
               for i in np.flatnonzero(shp["type"] == PT_SHAPE_SPHERE)}
    return dev.edited_desc(e, spheres=spheres) if spheres else e


def scene_rays(n, seed):
    """Random rays from in and around the box the scenes fill towards points inside it."""
    rng = np.random.default_rng(seed)
    lo, hi = np.full(3, -2.5), np.full(3, 2.5)
    o = lo + (hi - lo) * (rng.random((n, 3)) * 1.6 - 0.3)
    dirs = lo + (hi - lo) * rng.random((n, 3)) - o
    dirs /= np.maximum(np.linalg.norm(dirs, axis=1, keepdims=True), 1e-20)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = o, dirs, 1e-4, np.inf
    return rays


# ---- A: refit regimes -------------------------------------------------------------------------------------------------------

def _complete(last):
    return [1 << k for k in range(last.bit_length())] if last & (last - 1) == 0 else None


TOP_1024 = _complete(1024)                                   # 2047 nodes, levels 0 .. 10
# name -> (triangles, spheres, level widths of the caller's tree, the regime it aims at)
REGIME_INPUTS = {
    "n1": (1, 0, [], NONE),
    "n2": (1, 1, [1], ONE_LAUNCH),                           # levels == 1
    "n3": (3, 0, [1, 1], ONE_LAUNCH),                        # levels == 2
    "chain65": (62, 3, [1, 2] + [1] * 61, ONE_LAUNCH),       # 64 levels with the leaves': the deepest tree pt_scene_create takes
    "complete2048": (2044, 4, TOP_1024, ONE_LAUNCH),         # the widest level is exactly K_NARROW
    "chains4097": (4093, 4, TOP_1024 + [1024, 1024, 1], ONE_LAUNCH),        # exactly K_WHOLE_TREE_NODES inner nodes
    "chains4098": (4094, 4, TOP_1024 + [1024, 1024, 2], TOP_ALONE),         # one node more, every level narrow
    "chains5120": (5116, 4, TOP_1024 + [1024, 1024, 1024], TOP_ALONE),      # every level below the top exactly K_NARROW wide
    "heap4097": (4093, 4, _complete(2048) + [1], LEVELS_AND_TOP),           # 4096 nodes, level 11 is 2048 wide
    "bulge3106": (3102, 4, TOP_1024 + [1025, 30, 3], LEVELS_AND_TOP),       # a wide level between narrow ones
}


@functools.lru_cache(maxsize=None)
def regime_input(name):
    """(hs, d0, d1, d1r, params): the scene on a caller's tree of the listed level widths with host.refit_bvh's boxes, its edit
    (moved_geometry) and the edit's fresh-create twin.  The leaves take the shapes sorted along x: slabs, a tree the internal
    one beats easily."""
    n_tris, n_spheres, widths, _ = REGIME_INPUTS[name]
    hs = make_scene(n_tris, n_spheres, seed=100 + n_tris)
    d = hs.finalize()
    assert d.num_shapes == n_tris + n_spheres == sum(widths) + 1
    order = [int(i) for i in np.argsort(centroids(d)[:, 0], kind="stable")]
    d0 = host.refit_bvh(with_nodes(d, tree_from_widths(widths, order)))
    d1 = moved_geometry(d0)
    return hs, d0, d1, host.refit_bvh(d1), params_of(hs)


@functools.lru_cache(maxsize=None)
def sweep_widths(name):
    """Level widths of the library's internal tree over regime_input(name)'s leaf boxes (dev.build_bvh_sweep, host code)."""
    d0 = regime_input(name)[1]
    return level_widths(dev.build_bvh_sweep(d0)[0]) if d0.num_shapes >= 2 else []


# ---- B: what a geometry update may change -----------------------------------------------------------------------------------

B_SCENES = {"lds": (36, 3), "global": (4180, 20)}             # name -> (triangles in three meshes, spheres)


@functools.lru_cache(maxsize=None)
def b_scene(name, diffuse_only):
    n_tris, n_spheres = B_SCENES[name]
    hs = make_scene(n_tris, n_spheres, seed=7 + n_tris, n_meshes=3, diffuse_only=diffuse_only, emissive_sphere=False)
    return hs, hs.finalize(), params_of(hs)


def _tri_rows(shp):
    return np.flatnonzero(shp["type"] == PT_SHAPE_TRIANGLE)


def _sphere_rows(shp):
    return np.flatnonzero(shp["type"] == PT_SHAPE_SPHERE)


def spheres_to_triangles(d, rows, shp=None):
    """The listed sphere shapes become (second uses of) faces of mesh 0."""
    shp = shape_table(d) if shp is None else shp.copy()
    for j, i in enumerate(rows):
        assert shp["type"][i] == PT_SHAPE_SPHERE
        shp[i] = (PT_SHAPE_TRIANGLE, -1, -1, (0, 0, 0), 0, (3 * j + 1) % d.meshes[0].num_faces, 0)
    return shp


def triangles_to_spheres(d, rows, shp=None):
    """The listed triangle shapes become spheres around their centroids, with materials in turn and no emission."""
    shp = shape_table(d) if shp is None else shp.copy()
    c = centroids(d)
    r = 0.5 * min(1.0, 4.0 * d.num_shapes ** (-1.0 / 3.0))
    for j, i in enumerate(rows):
        assert shp["type"][i] == PT_SHAPE_TRIANGLE
        shp[i] = (PT_SHAPE_SPHERE, j % d.num_materials, -1, tuple(c[i].astype(np.float32)), r * (0.5 + 0.1 * (j % 5)), -1, -1)
    return shp


def edit_types(d):
    """A few shapes change type: every other sphere becomes a triangle, some non-emissive triangles become spheres."""
    shp = shape_table(d)
    tris = [i for i in _tri_rows(shp) if d.meshes[int(shp["mesh_index"][i])].area_light_id < 0]
    shp = spheres_to_triangles(d, _sphere_rows(shp)[::2], shp)
    shp = triangles_to_spheres(d, tris[2::max(len(tris) // 7, 1)][:7], shp)
    return dev.edited_desc(moved_geometry(d), shapes=as_shapes(shp))


def edit_no_sphere(d):
    """The last sphere goes: every sphere becomes a triangle."""
    shp = shape_table(d)
    return dev.edited_desc(d, shapes=as_shapes(spheres_to_triangles(d, _sphere_rows(shp), shp)))


def edit_merged(d):
    """The three meshes merged into one (mesh 0's ids): the same triangles from one vertex pool."""
    tab, shp = mesh_table(d), shape_table(d)
    vbase = np.cumsum([0] + [len(t[0]) for t in tab])
    fbase = np.cumsum([0] + [len(t[1]) for t in tab])
    merged = (np.concatenate([t[0] for t in tab]), np.concatenate([t[1] + vbase[m] for m, t in enumerate(tab)]).astype(np.int32),
              np.concatenate([t[2] for t in tab]), tab[0][3], tab[0][4])
    tri = _tri_rows(shp)
    shp["face_index"][tri] += fbase[shp["mesh_index"][tri]].astype(np.int32)
    shp["mesh_index"][tri] = 0
    return dev.edited_desc(d, shapes=as_shapes(shp), mesh_list=[merged])


def edit_split(d, n_meshes=70):
    """The same triangles in n_meshes meshes (above 64: prims_device's staging branch; the LDS-resident scene has 36 triangles
    and so gets 36 meshes of one); triangle k of the scene goes to mesh k % n_meshes, and mesh m takes the ids of mesh m % 3 —
    ids move too."""
    tab, shp = mesh_table(d), shape_table(d)
    tri = _tri_rows(shp)
    n_meshes = min(n_meshes, len(tri))
    parts = [([], [], []) for _ in range(n_meshes)]
    for k, i in enumerate(tri):
        P, I, Nn = tab[int(shp["mesh_index"][i])][:3]
        f = I[int(shp["face_index"][i])]
        part = parts[k % n_meshes]
        shp["mesh_index"][i], shp["face_index"][i] = k % n_meshes, len(part[1])
        part[1].append(3 * len(part[1]) + np.arange(3))
        part[0].append(P[f])
        part[2].append(Nn[f])
    mesh_list = [(np.concatenate(p[0]), np.array(p[1], np.int32), np.concatenate(p[2]), tab[m % 3][3], tab[m % 3][4]) for m, p in enumerate(parts)]
    return dev.edited_desc(d, shapes=as_shapes(shp), mesh_list=mesh_list)


def edit_ids(d):
    """Ids alone: mesh 0 takes another material, the emissive mesh stops emitting and mesh 1 emits in its place, the first sphere
    takes another material and the emissive mesh's light.  Geometry and the lights table stay."""
    tab, shp = mesh_table(d), shape_table(d)
    lit = [m for m, t in enumerate(tab) if t[4] >= 0]
    assert lit == [2] and d.num_lights > 0
    light = tab[2][4]
    tab[0] = tab[0][:3] + ((tab[0][3] + 1) % d.num_materials, tab[0][4])
    tab[1] = tab[1][:3] + (tab[1][3], light)
    tab[2] = tab[2][:3] + (tab[2][3], -1)
    s = _sphere_rows(shp)[0]
    shp["material_id"][s] = (shp["material_id"][s] + 2) % d.num_materials
    shp["area_light_id"][s] = light
    return dev.edited_desc(d, shapes=as_shapes(shp), mesh_list=tab)


def edit_rewired(d):
    """The same vertices, the faces rewired: face f of every mesh takes its third corner from face f + 1."""
    tab = mesh_table(d)
    for m, t in enumerate(tab):
        I = t[1].copy()
        I[:, 2] = np.roll(t[1][:, 2], -1)
        tab[m] = (t[0], I) + t[2:]
    return dev.edited_desc(d, mesh_list=tab)


def edit_emitter_moved(d):
    """The emissive mesh moved and scaled, everything else wobbled: next-event estimation must aim at the new place."""
    e = moved_geometry(d)
    P, _, _ = mesh_arrays(d, 2)
    return dev.edited_desc(e, meshes={2: ((P * np.float32(0.7) + np.array([0.4, 0.3, -0.2], np.float32)).astype(np.float32), None)})


B_EDITS = {"types": edit_types, "no_sphere": edit_no_sphere, "merged": edit_merged, "split70": edit_split, "ids": edit_ids,
           "rewired": edit_rewired, "emitter_moved": edit_emitter_moved}


@functools.lru_cache(maxsize=None)
def b_edit(name, diffuse_only, edit):
    """(edited desc, its fresh-create twin)."""
    d1 = B_EDITS[edit](b_scene(name, diffuse_only)[1])
    return d1, host.refit_bvh(d1)


@functools.lru_cache(maxsize=None)
def sphere_scene(n):
    """n small spheres and not a single mesh; (hs, d0, d1 = every sphere moved and resized, a desc with num_meshes == 0 and a
    null mesh pointer, d1r, params)."""
    hs = make_scene(0, n, seed=n)
    d0 = hs.finalize()
    assert d0.num_meshes == 0
    d1 = dev.edited_desc(moved_geometry(d0), mesh_list=[])
    return hs, d0, d1, host.refit_bvh(d1), params_of(hs)


# ---- C: descs an update must refuse -----------------------------------------------------------------------------------------

ID_ERRORS = ("sphere material id out of range", "triangle mesh index out of range", "triangle face index out of range",
             "vertex index out of range", "unknown shape type")


def bad_id_descs(d):
    """message -> a desc with moved geometry (so that a half-applied update would show) and ONE id wrong, in the order of
    ID_ERRORS: the messages pt_scene_create's host loop gives."""
    e = moved_geometry(d, step=2)
    shp = shape_table(e)
    i = int(_tri_rows(shp)[len(_tri_rows(shp)) // 2])
    m, f = int(shp["mesh_index"][i]), int(shp["face_index"][i])
    out = {}
    for msg, row in zip(ID_ERRORS, [(PT_SHAPE_SPHERE, e.num_materials, -1, (0, 0, 0), 0.1, -1, -1), (PT_SHAPE_TRIANGLE, -1, -1, (0, 0, 0), 0, 0, e.num_meshes),
                                    (PT_SHAPE_TRIANGLE, -1, -1, (0, 0, 0), 0, e.meshes[m].num_faces, m), None, (7, 0, -1, (0, 0, 0), 0.1, f, m)]):
        if row is None:
            tab = mesh_table(e)
            I = tab[m][1].copy()
            I[f, 1] = len(tab[m][0])                          # one past the last vertex
            tab[m] = (tab[m][0], I) + tab[m][2:]
            out[msg] = dev.edited_desc(e, mesh_list=tab)
        else:
            s = shp.copy()
            s[i] = row
            out[msg] = dev.edited_desc(e, shapes=as_shapes(s))
    return out


def not_finite_descs(d):
    """Descs whose shape i is a sphere that has no finite box: centre + radius overflows, or the radius is no number."""
    e = moved_geometry(d, step=2)
    shp = shape_table(e)
    i = d.num_shapes // 2
    out = {}
    for what, (c, r) in {"centre + radius overflows": ((3e38, 0, 0), 3e38), "radius inf": ((0, 0, 0), np.inf), "radius nan": ((0, 0, 0), np.nan)}.items():
        s = shp.copy()
        s[i] = (PT_SHAPE_SPHERE, 0, -1, c, r, -1, -1)
        assert what != "centre + radius overflows" or (np.isfinite(s["center"][i]).all() and np.isfinite(s["radius"][i]))
        out[what] = dev.edited_desc(e, shapes=as_shapes(s))
    return out


def unused_nan_desc(d):
    """Moved geometry, and mesh 0 grown by one vertex that is NaN in position and normal and that no face uses."""
    e = moved_geometry(d, step=2)
    tab = mesh_table(e)
    nan = np.full((1, 3), np.nan, np.float32)
    tab[0] = (np.concatenate([tab[0][0], nan]), tab[0][1], np.concatenate([tab[0][2], nan])) + tab[0][3:]
    return dev.edited_desc(e, mesh_list=tab)


# ---- D: the two record makers ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def many_meshes_scene():
    """About 4200 shapes: 70 meshes (every fifth emissive), 20 spheres (one emissive), all four materials."""
    rng = np.random.default_rng(70)
    hs = make_scene(0, 0, seed=70)
    n_tris = 4180
    size = np.float32(4.0 * n_tris ** (-1.0 / 3.0))
    c = (rng.random((n_tris, 1, 3)) * 4 - 2).astype(np.float32)
    P = (c + (rng.random((n_tris, 3, 3)) - 0.5).astype(np.float32) * size).astype(np.float32)
    for k in range(70):
        Pk = P[k::70].reshape(-1, 3)
        hs.add_mesh(Pk, np.arange(len(Pk), dtype=np.int32).reshape(-1, 3), k % 4, radiance=(3.0, 2.5, 2.0) if k % 5 == 0 else None)
    for k in range(20):
        hs.add_sphere(rng.random(3) * 3 - 1.5, 0.1 + float(rng.random()) * 0.2, k % 4, radiance=(4.0, 4.0, 1.0) if k == 0 else None)
    return hs, hs.finalize(), params_of(hs)
