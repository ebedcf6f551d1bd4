"""Inputs of the pt_scene_rebuild tests (test_scene_rebuild_host.py, test_scene_rebuild.py) and of the tree-cost tests
(test_tree_cost_cases_host.py, test_tree_cost_states.py; second half of this file), made once and left unchanged.

grid_case(n): n^3 cubes of edge 0.4 on a unit grid, one mesh of 12 triangles per cube, one group per cube.  The shuffle
translates cube i to the cell np.random.default_rng(1).permutation(n^3)[i]: objects that move independently, the animation
a refitted tree copes with worst.  n = 2, 3, 7: 96, 324 and 4,116 shapes — an LDS-resident scene, one in global
memory built on the host, and the smallest that takes the device build path.

cbox_case(): the Cornell box with its two blocks (meshes 6 and 7) translated only; a pure translation keeps the two triangles
of a face on one box, so the sweep groups keep their number."""
import math

import numpy as np
from conftest import load_scene

from pathtracer_cuda_interactive_amd import PT_TRAVERSAL_EXACT, host, standins
from pathtracer_cuda_interactive_amd import device as dev

W, H, SPP, RAYS = 64, 48, 4, 20000
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
GRIDS = (2, 3, 7)

grid_scene, shuffle_matrices = standins.grid_scene, standins.grid_shuffle_matrices


def box_rays(d, n, seed):
    """Random rays from in and around the root box of `d` towards points inside it."""
    root = d.nodes[d.root]
    lo, hi = np.array(root.bmin[:], np.float64), np.array(root.bmax[:], np.float64)
    rng = np.random.default_rng(seed)
    o = lo + (hi - lo) * (rng.random((n, 3)) * 1.6 - 0.3)
    dirs = lo + (hi - lo) * rng.random((n, 3)) - o
    dirs /= np.maximum(np.linalg.norm(dirs, axis=1, keepdims=True), 1e-20)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = o, dirs, 1e-4, np.inf
    return rays


_cases = {}


def _finish(name, hs, d0, ids, M1, M2, seed=11):
    p = hs.render_params(W, H, SPP, seed=seed)
    p.traversal = PT_TRAVERSAL_EXACT
    d1r = host.refit_bvh(dev.transform_desc_host(d0, ids, M1))
    d2r = host.refit_bvh(dev.transform_desc_host(d0, ids, M2))
    _cases[name] = dict(name=name, hs=hs, d0=d0, ids=ids, M1=M1, M2=M2, d1r=d1r, d2r=d2r, p=p, rays=box_rays(d1r, RAYS, 5))
    return _cases[name]


def grid_case(n):
    """d0: the grid at rest; M1: the shuffle; M2: another shuffle; d1r / d2r: the moved scenes on pt_host_refit_bvh's pool."""
    name = f"grid{n}"
    if name not in _cases:
        hs = grid_scene(n)
        d0 = hs.finalize()
        ids, G = dev.groups_by_object(d0)
        assert G == n ** 3 and d0.num_shapes == 12 * n ** 3
        _finish(name, hs, d0, ids, shuffle_matrices(n, 1), shuffle_matrices(n, 2))
    return _cases[name]


def cbox_case():
    if "cbox" not in _cases:
        hs, d0 = load_scene("cbox")
        ids, G = dev.groups_by_object(d0)
        M1, M2 = np.stack([IDENTITY] * G), np.stack([IDENTITY] * G)
        M1[6, :, 3], M1[7, :, 3] = (60.0, 0.0, -40.0), (-50.0, 30.0, 45.0)
        M2[6, :, 3], M2[7, :, 3] = (-30.0, 20.0, 25.0), (35.0, 0.0, -60.0)
        # The blocks stand on the floor: a path that hits both at one t continues from whichever the tree's visit order names.
        # conftest.assert_work_counters runs the oracle on the sweep tree with that tree's own ties, so its counts are the
        # device's only for frames without such a path.  Seed 9 is the first for which the oracle traces the same segments on
        # the caller's tree and on the sweep tree at rest, under M1 and under M2 (checked on the CPU, no device involved).
        _finish("cbox", hs, d0, ids, M1, M2, seed=9)
    return _cases["cbox"]


def case(name):
    return cbox_case() if name == "cbox" else grid_case(int(name[4:]))


def pool(d):
    """desc's node pool as a structured array (a copy)."""
    import ctypes as C
    return np.frombuffer(C.string_at(d.nodes, d.num_nodes * host.NODE_DTYPE.itemsize), dtype=host.NODE_DTYPE).copy()


def desc_with_nodes(desc, nodes):
    """A copy of `desc` on the pool `nodes` (same root)."""
    import ctypes as C

    from pathtracer_cuda_interactive_amd.ctypes_defs import PtBvhNode, PtSceneDesc
    d2 = PtSceneDesc()
    C.memmove(C.byref(d2), C.byref(desc), C.sizeof(PtSceneDesc))
    d2.nodes = nodes.ctypes.data_as(C.POINTER(PtBvhNode))
    d2._keep = (nodes, desc)
    return d2


def box_areas(nodes):
    """fp64 area of every node's box: e = (double)max - (double)min, a = 2 ((ex ey + ey ez) + ez ex)."""
    e = nodes["bmax"].astype(np.float64) - nodes["bmin"].astype(np.float64)
    return 2.0 * ((e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2]) + e[:, 2] * e[:, 0])


def inner_terms(d):
    """The terms of desc's tree cost in pool index order: the areas of the inner nodes below the root."""
    nodes = pool(d)
    keep = nodes["prim"] == -1
    keep[d.root] = False
    return box_areas(nodes)[keep]


def sum_bound(m):
    """Relative error bound of ANY order of an fp64 sum of m positive terms: (m - 1) u / (1 - (m - 1) u), u = 2^-53."""
    g = (m - 1) * 2.0 ** -53
    return g / (1.0 - g)


# ---- inputs of test_tree_cost_states.py (checked without a GPU by test_tree_cost_cases_host.py) ----------------------------------

# Shape counts of the equal-sphere scenes, by what the cost kernels do with N - 1 node records: 1..5 records (one thread's four
# and its tail), 255..257 (one wave's 256), 1023..1025 (one partial against two), 2048 / 2049 (two against three), and the shape
# counts either side of the threshold between host and device scene preparation.  N = 1 and 2: no inner node below the root.
EQUAL_SIZES = (1, 2, 3, 4, 5, 6, 256, 257, 258, 1024, 1025, 1026, 2049, 2050, 4095, 4096, 4097)
COST_KEYS = ("tree_cost0_bits", "tree_cost1_bits", "tree_cost0_permille", "tree_cost1_permille")
UNMEASURED = [0, 0, 1000, 1000]


def f64(bits):
    return float(np.array([bits], np.int64).view(np.float64)[0])


def bits64(x):
    return int(np.array([x], np.float64).view(np.int64)[0])


def scaling(s, groups=1):
    """[groups, 3, 4]: s * I and no translation.  For s a power of two every coordinate, radius and box scales exactly."""
    return np.stack([IDENTITY * np.float32(s)] * groups)


def equal_spheres(n):
    """(HostScene, desc) of n spheres of radius 0.5 about the origin: every box of any tree over them is [-0.5, 0.5]^3, of
    area 6.0 exactly, so the tree's cost is the integer 6 (n - 2) in any order of summation."""
    name = f"equal{n}"
    if name not in _cases:
        from pathtracer_cuda_interactive_amd import PT_MAT_DIFFUSE, HostScene
        hs = HostScene()
        hs.set_camera((0, 0.5, 4.0), (0, 0, 0), (0, 1, 0), 50.0, W, H, SPP)
        hs.set_background((0.4, 0.5, 0.6))
        m = hs.add_material(PT_MAT_DIFFUSE, (0.6, 0.6, 0.5))
        for _ in range(n):
            hs.add_sphere((0.0, 0.0, 0.0), 0.5, m)
        _cases[name] = (hs, hs.finalize())
    return _cases[name]


SCALED = ("random1025", "random1030", "grid7", "bunny")


def scaled_case(name):
    """dict(d0, ids, G) with ONE group holding every shape, for transforms by s * I: two mixed scenes of 1,025 and 1,030 shapes
    (1,024 and 1,029 records: a partial's tail of 0 and of 5), grid7, and bunny — 288,094 shapes, 563 partials, the only case
    whose partials take cost_total_kernel round its loop three times."""
    key = "scaled " + name
    if key not in _cases:
        if name.startswith("random"):
            n = int(name[6:])
            from conftest import random_scene
            hs = random_scene(n, n_tris=n - 6, n_spheres=5)
            d0 = hs.finalize()
        elif name == "bunny":
            hs, d0 = load_scene("bunny")
        else:
            c = case(name)
            hs, d0 = c["hs"], c["d0"]
        _cases[key] = dict(name=name, hs=hs, d0=d0, ids=np.zeros(d0.num_shapes, np.int32), G=1)
    return _cases[key]


ROUTES = ("grid3", "scene4", "mixed")


def route_case(name):
    """dict(d0, ids, G, M, M2, d1, d2, p): a scene, one group per object, two sets of matrices and the descs they stand for
    (dev.transform_desc_host) — what pt_scene_transform makes on the device and what pt_scene_update is handed.  grid3: the
    shuffle; scene4: 30 spheres, each moved and scaled on its own; mixed: two meshes and six spheres, rotated, scaled, moved."""
    key = "route " + name
    if key not in _cases:
        if name == "grid3":
            c = grid_case(3)
            hs, d0, ids, M, M2 = c["hs"], c["d0"], c["ids"], c["M1"], c["M2"]
            G = M.shape[0]
        else:
            if name == "scene4":
                hs, d0 = load_scene("scene4")
            else:
                from conftest import random_scene
                hs = random_scene(31, n_tris=70, n_spheres=5)
                d0 = hs.finalize()
            ids, G = dev.groups_by_object(d0)
            rng = np.random.default_rng(17)

            def matrices():
                out = []
                for _ in range(G):
                    out.append(dev.rigid_matrix(rng.standard_normal(3), float(rng.uniform(-60, 60)), centre=rng.uniform(-1, 1, 3),
                                                scale=float(rng.uniform(0.7, 1.4)), translate=rng.uniform(-0.5, 0.5, 3)))
                return np.stack(out)
            M, M2 = matrices(), matrices()
        p = hs.render_params(W, H, SPP, seed=11)
        p.traversal = PT_TRAVERSAL_EXACT
        _cases[key] = dict(name=name, hs=hs, d0=d0, ids=ids, G=G, M=M, M2=M2, d1=dev.transform_desc_host(d0, ids, M),
                           d2=dev.transform_desc_host(d0, ids, M2), p=p)
    return _cases[key]


def host_cost0(d):
    """(exact, m): math.fsum of the terms of the caller's tree refitted to desc `d` on the host, and their number."""
    terms = inner_terms(host.refit_bvh(d))
    return math.fsum(terms), terms.size


def not_nested_desc():
    """grid3 on a pool in which some inner boxes are shrunk about their centres, so that their children stick out: a caller's
    tree whose boxes do not nest (test_fast_tree.py), for which pt_scene_create keeps no internal tree."""
    if "not nested" not in _cases:
        c = grid_case(3)
        nodes = pool(c["d0"])
        inner = [int(k) for k in np.flatnonzero(nodes["prim"] < 0) if int(k) != int(c["d0"].root)]
        for k in inner[::7]:
            ctr = 0.5 * (nodes["bmin"][k] + nodes["bmax"][k])
            nodes["bmin"][k] = ctr + 0.6 * (nodes["bmin"][k] - ctr)
            nodes["bmax"][k] = ctr + 0.6 * (nodes["bmax"][k] - ctr)
        _cases["not nested"] = desc_with_nodes(c["d0"], nodes)
    return _cases["not nested"]


NO_TREE = ("scene1", "not nested")


def no_tree_case(name):
    """dict(d0, ids, G, M, d1): a handle for which pt_scene_create keeps no internal tree — scene1 (4 shapes, fewer than 16) and
    grid3 on boxes that do not nest — with one group per object and matrices that move every one of them."""
    key = "no tree " + name
    if key not in _cases:
        if name == "scene1":
            _, d0 = load_scene("scene1")
            ids, G = dev.groups_by_object(d0)
            M = np.stack([dev.rigid_matrix((0, 1, 0), 10.0 * (g + 1), scale=1.0 + 0.125 * g, translate=(0.1 * g, 0.0, -0.05 * g)) for g in range(G)])
        else:
            c = grid_case(3)
            d0, ids, M = not_nested_desc(), c["ids"], c["M1"]
            G = M.shape[0]
        _cases[key] = dict(name=name, d0=d0, ids=ids, G=G, M=M, d1=dev.transform_desc_host(d0, ids, M))
    return _cases[key]


def same_tree_case():
    """dict(d0, ids, G, M, d1r, p): grid3 on the library's own sweep tree as the caller's tree, ONE group, doubled.  The sweep
    tree of the doubled boxes is the doubled sweep tree, node for node (checked on the host): a rebuild's candidate is the tree
    the handle holds, visits as many nodes, and is not adopted — while the cost has risen to exactly 4000 permille."""
    if "same tree" not in _cases:
        c = grid_case(3)
        ds, _ = dev.build_bvh_sweep(c["d0"])
        ids, M = np.zeros(ds.num_shapes, np.int32), scaling(2.0)
        _cases["same tree"] = dict(name="same tree", d0=ds, ids=ids, G=1, M=M, d1r=host.refit_bvh(dev.transform_desc_host(ds, ids, M)), p=c["p"])
    return _cases["same tree"]


def with_a_nan_vertex(d):
    """A copy of desc `d` whose first mesh has one vertex coordinate NaN: an update pt_scene_update refuses (PT_ERR_UNSUPPORTED)
    after it has staged the records, once a reference measurement may already be enqueued."""
    P, _, _ = standins.mesh_arrays(d, 0)
    Q = P.copy()
    Q[Q.shape[0] // 2, 1] = np.nan
    return dev.edited_desc(d, meshes={0: (Q, None)})


def singular(G):
    """[G, 3, 4] matrices, the second of determinant 0: a transform pt_scene_transform refuses (PT_ERR_INVALID_ARG)."""
    M = np.stack([IDENTITY] * G)
    M[1, :, :3] = [[1, 2, 3], [2, 4, 6], [0, 0, 1]]
    return M


def reshaded(d):
    """A copy of desc `d` with another background: a shading-only update."""
    return dev.edited_desc(d, background=(0.1, 0.7, 0.3))
