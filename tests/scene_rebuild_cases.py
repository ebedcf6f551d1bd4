"""Inputs of the pt_scene_rebuild tests (test_scene_rebuild_host.py, test_scene_rebuild.py), made once and left unchanged.

grid_case(n): n^3 cubes of edge 0.4 on a unit grid, one mesh of 12 triangles per cube, one group per cube.  The shuffle
translates cube i to the cell np.random.default_rng(1).permutation(n^3)[i]: objects that move independently, the animation
a refitted tree copes with worst.  n = 2, 3, 7: 96, 324 and 4,116 shapes — an LDS-resident scene, one in global
memory built on the host, and the smallest that takes the device build path.

cbox_case(): the Cornell box with its two blocks (meshes 6 and 7) translated only; a pure translation keeps the two triangles
of a face on one box, so the sweep groups keep their number."""
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
