"""pt_bvh_build_device (csrc/pt_bvh_build.hip) against tests/bvh_build_reference.py: the device-built tree must be the reference
tree node for node — ints, root and depth exactly, boxes by value (the sign of a zero is not part of the contract, see the
reference's docstring) — at the sizes where the builder changes path (wave, block, padded range-tree size P and P + 1, a
second trip of the centroid-bounds grid-stride loop) and on inputs that leave only the tie rules, the clamps or the depth cap
to decide.  The CPU tests check the reference itself and that every input has the property it is there for."""
import ctypes as C
import functools

import numpy as np
import pytest
from bvh_build_reference import (LBVH, SAH, assert_same_tree, build_reference, centroid_codes, inorder_prims, lbvh_cut,
                                 morton_order, sah_cut, sah_max_depth)
from conftest import assert_bit_equal
from test_device_bvh import check_tree, host_leaf_boxes

from pathtracer_cuda_interactive_amd import (PT_ERR_BAD_SCENE, PT_MAT_DIFFUSE, PT_MAT_MIRROR, PT_MAT_PHONG, PT_MAT_PLASTIC, HostScene,
                                             PtError)
from pathtracer_cuda_interactive_amd import device as dev
from pathtracer_cuda_interactive_amd.ctypes_defs import PtBvhNode, PtSceneDesc

METHODS = {"lbvh": LBVH, "sah": SAH}
assert (dev.PT_BVH_DEVICE_LBVH, dev.PT_BVH_DEVICE_SAH) == (LBVH, SAH)
SIZES = (2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
MAX_RENDER_DEPTH = 64                      # pt_scene_create accepts a caller's tree of up to 64 levels (leaves count 1)
BIG_FIRST_TRIP = 1024 * 256                # centroid_bounds_kernel launches at most 1024 blocks of 256: ids beyond take a second trip
BIG_N = BIG_FIRST_TRIP + 300


def _new_scene(lookfrom=(0, 0.5, 4.0), lookat=(0, 0, 0), vfov=50.0):
    hs = HostScene()
    hs.set_camera(lookfrom, lookat, (0, 1, 0), vfov, 16, 12, 1)
    hs.set_background((0.4, 0.5, 0.6))
    mats = [hs.add_material(PT_MAT_DIFFUSE, (0.7, 0.6, 0.5)), hs.add_material(PT_MAT_MIRROR, (0.9, 0.9, 0.9)),
            hs.add_material(PT_MAT_PLASTIC, (0.3, 0.6, 0.4), eta=1.5), hs.add_material(PT_MAT_PHONG, (0.5, 0.4, 0.7), exponent=20.0)]
    return hs, mats


def _add_triangles(hs, P, material, radiance=None):
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    hs.add_mesh(P, np.arange(len(P), dtype=np.int32).reshape(-1, 3), material, radiance=radiance)


def _mixed(n):
    """Triangles and a few spheres as in conftest.random_scene; from 63 primitives up with the far ground sphere — the outlier
    that stretches the centroid bounds by two orders of magnitude, which the 21-bit grid exists for."""
    rng = np.random.default_rng(1000 + n)
    hs, mats = _new_scene()
    n_spheres = 1 if n < 63 else 5                                  # the ground sphere included
    n_tris = n - n_spheres
    c = (rng.random((n_tris, 1, 3)) * 4 - 2).astype(np.float32)
    _add_triangles(hs, c + (rng.random((n_tris, 3, 3)) - 0.5).astype(np.float32) * 1.5, mats[n % 4], radiance=(3.0, 2.5, 2.0))
    for k in range(n_spheres - (n >= 63)):
        hs.add_sphere(rng.random(3) * 3 - 1.5, 0.2 + float(rng.random()) * 0.5, mats[k % 4])
    if n >= 63:
        hs.add_sphere((0, -101.5, 0), 100.0, mats[0])
    return hs


def _coincident():
    hs, mats = _new_scene()
    tri = np.float32([[-1, -0.5, 0], [1, -0.5, 0.25], [0, 1, -0.25]])
    hs.add_mesh(tri, np.tile(np.int32([0, 1, 2]), (300, 1)), mats[0])
    return hs


def _planar():
    """Flat triangles in the plane z = 0.25: every centroid has that z — one axis of zero extent."""
    rng = np.random.default_rng(7)
    hs, mats = _new_scene()
    P = (rng.random((90, 3, 3)) * 3 - 1.5).astype(np.float32)
    P[:, :, 2] = 0.25
    _add_triangles(hs, P, mats[0], radiance=(2.0, 2.0, 2.0))
    return hs


def _collinear():
    """Spheres along x, every value a small dyadic number so that (hi + lo) * 0.5 is the centre exactly: two axes of zero extent."""
    rng = np.random.default_rng(8)
    hs, mats = _new_scene()
    for k in range(70):
        hs.add_sphere((float(rng.integers(-2048, 2048)) / 1024, 0.5, 0.25), float(rng.integers(1, 16)) / 64, mats[k % 4])
    return hs


def _ties():
    """Spheres of several radii centred on the points of a 4 x 4 x 4 lattice: 64 distinct codes among 600 primitives."""
    rng = np.random.default_rng(9)
    hs, mats = _new_scene(lookfrom=(1.5, 2.0, 12.0), lookat=(1.5, 1.5, 1.5), vfov=35.0)
    for k in range(600):
        hs.add_sphere(rng.integers(0, 4, 3).astype(float), float(rng.integers(1, 5)) / 16, mats[k % 4])
    return hs


def _overflow():
    """Triangles some 1e20 across: every surface area, and so every SAH cost, is +inf."""
    rng = np.random.default_rng(10)
    hs, mats = _new_scene()
    c =(rng.random((80, 1, 3)) * 2 - 1) * 1e20
    _add_triangles(hs, c + (rng.random((80, 3, 3)) - 0.5) * 2e20, mats[0])
    return hs


def _tiny():
    """Centres 1 + k ulps, k in 0..3 per axis, radius 1/16 (all sums exact): centroid bounds three ulps wide."""
    rng = np.random.default_rng(11)
    hs, mats = _new_scene(lookfrom=(1, 1, 1.5), lookat=(1, 1, 1))
    K = rng.integers(0, 4, (40, 3))
    K[:2] = [[0, 0, 0], [3, 3, 3]]
    for k in range(40):
        hs.add_sphere(tuple(1.0 + K[k] * 2.0 ** -23), 1.0 / 16, mats[k % 4])
    return hs


CHAIN_CODES = [0] + [1 << m for m in range(63)] + [(1 << 63) - 1]


def _chain(copies_at_origin):
    """Spheres of radius 2^-22 whose sorted codes are 0, 2^0, 2^1, ..., 2^62 and 2^63 - 1: every LBVH cut peels one leaf off the top."""
    hs, mats = _new_scene(lookfrom=(3e-6, 2e-6, 5e-6), lookat=(0, 0, 2.4e-7), vfov=30.0)
    r = 2.0 ** -22
    for _ in range(copies_at_origin):
        hs.add_sphere((0, 0, 0), r, mats[0])
    hs.add_sphere((1, 1, 1), r, mats[1])
    for m in range(63):
        centre = [0.0, 0.0, 0.0]
        centre[2 - m % 3] = 2.0 ** (m // 3) * 2.0 ** -21
        hs.add_sphere(centre, r, mats[m % 4])
    return hs


LOWBITS_BASE = np.array([0x0AAAAA, 0x155555, 0x0CCCCC]) & ~0x3FF


def _lowbits_cells():
    rng = np.random.default_rng(13)
    return np.concatenate([[[0, 0, 0]], LOWBITS_BASE + rng.integers(0, 1024, (300, 3))])


def _lowbits():
    """Spheres of radius 2^-22 centred on cells k * 2^-21 of the unit cube (spanned by the origin and the far corner) that
    agree in their upper 11 bits per axis: the LOW bits of the code decide the order, which no scattered input ever asks of them."""
    centre = (LOWBITS_BASE + 512) * 2.0 ** -21
    hs, mats = _new_scene(lookfrom=tuple(centre + [0, 0, 1.2e-3]), lookat=tuple(centre), vfov=30.0)
    hs.add_sphere((1, 1, 1), 2.0 ** -22, mats[0])
    for k, cell in enumerate(_lowbits_cells()):
        hs.add_sphere(tuple(cell * 2.0 ** -21), 2.0 ** -22, mats[k % 4])
    return hs


def _big():
    """One mesh of BIG_N small triangles: the first 262,144 inside the unit cube, the last 300 around it — the first six of those
    at the very ends of each axis, so only ids that the bounds kernel's second grid-stride trip reads set the centroid bounds."""
    rng = np.random.default_rng(12)
    hs, mats = _new_scene()
    c = rng.random((BIG_N, 1, 3))
    c[BIG_FIRST_TRIP:] = c[BIG_FIRST_TRIP:] * 2 - 0.5
    for axis in range(3):
        c[BIG_FIRST_TRIP + 2 * axis, 0, axis] = -1.0
        c[BIG_FIRST_TRIP + 2 * axis + 1, 0, axis] = 2.0
    _add_triangles(hs, c + (rng.random((BIG_N, 3, 3)) - 0.5) * 0.004, mats[0])
    return hs


BUILDERS = {**{f"n{n}": functools.partial(_mixed, n) for n in SIZES},
            "coincident": _coincident, "planar": _planar, "collinear": _collinear, "ties": _ties, "overflow": _overflow,
            "tiny": _tiny, "lowbits": _lowbits, "chain64": functools.partial(_chain, 1), "chain_dups": functools.partial(_chain, 4)}
CASES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """(HostScene, desc, (lo, hi) primitive boxes by id) — built once, shared and left unchanged."""
    hs = _big() if name == "big" else BUILDERS[name]()
    d = hs.finalize()
    lo, hi = host_leaf_boxes(hs)
    lo.setflags(write=False), hi.setflags(write=False)
    return hs, d, (lo, hi)


@functools.lru_cache(maxsize=None)
def reference(name, method):
    nodes, root, depth = build_reference(*case(name)[2], METHODS[method])
    nodes.setflags(write=False)
    return nodes, root, depth


def desc_with_tree(d, nodes, root):
    d2 = PtSceneDesc()
    C.memmove(C.byref(d2), C.byref(d), C.sizeof(PtSceneDesc))
    nodes = np.ascontiguousarray(nodes)
    d2.nodes = nodes.ctypes.data_as(C.POINTER(PtBvhNode))
    d2.num_nodes = len(nodes)
    d2.root = int(root)
    d2._keep = (nodes, d)
    return d2


def centroid_extent(lo, hi):
    c = (hi + lo) * np.float32(0.5)
    return c.max(axis=0) - c.min(axis=0)


# ---- without a GPU: the reference itself, and the inputs' properties ---------------------------------------------------------

def test_morton_codes_of_known_cells():
    """Per-axis cells (x, y, z) of the unit cube's corners and of single bits: x is the highest bit of each triple."""
    lo = np.float32([[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0, 0], [0, 0, 2.0 ** -21], [0, 2.0 ** -20, 0]])
    want = [0, (1 << 63) - 1, int("100" * 21, 2), int("010" * 21, 2), int("001" * 21, 2), 1 << 62, 1, 1 << 4]
    assert centroid_codes(lo, lo).tolist() == want
    order, codes = morton_order(lo[[1, 0, 0, 4]], lo[[1, 0, 0, 4]])
    assert order.tolist() == [1, 2, 3, 0] and codes.tolist() == sorted(codes.tolist())       # equal codes stay in id order


@pytest.mark.parametrize("method", sorted(METHODS))
@pytest.mark.parametrize("name", CASES)
def test_reference_tree_is_a_valid_cover_in_morton_order(name, method):
    _, d, boxes = case(name)
    nodes, root, depth = reference(name, method)
    n = d.num_shapes
    assert n == len(boxes[0]) and (int(name[1:]) == n if name[1:].isdigit() else True)
    assert check_tree(nodes, root, n, boxes) == depth                     # a level-by-level walk finds the same depth
    order, codes = morton_order(*boxes)
    assert np.array_equal(inorder_prims(nodes, root), order)
    assert root == (n if method == "lbvh" else 2 * n - 2)
    if method == "lbvh":
        assert np.array_equal(nodes["prim"][:n], order)
    else:
        assert depth <= sah_max_depth(n)


def test_inputs_have_the_properties_they_are_there_for():
    for n in SIZES:
        if n >= 63:                                                        # the far ground sphere: most of the scene in few cells
            lo, hi = case(f"n{n}")[2]
            assert centroid_extent(lo, hi)[1] > 90 and np.median(np.abs((hi + lo)[:, 1])) < 4
    # coincident: one code; LBVH balanced over the positions; SAH: every cost ties, the lowest cut wins down to the cap
    lo, hi = case("coincident")[2]
    assert len(lo) == 300 and len(np.unique(centroid_codes(lo, hi))) == 1
    assert reference("coincident", "lbvh")[2] == 9 + 1
    nodes, root, depth = reference("coincident", "sah")
    assert depth == sah_max_depth(300) == 14
    chain = 0
    while nodes["prim"][nodes["left"][root]] >= 0:                         # a single leaf peeled off on the left, level after level
        root, chain = nodes["right"][root], chain + 1
    assert chain == 4                                                      # 5 + ceil(log2 296) reaches 14: median cuts from there
    # planar / collinear: one / two axes of zero extent
    assert (centroid_extent(*case("planar")[2]) > 0).tolist() == [True, True, False]
    assert (centroid_extent(*case("collinear")[2]) > 0).tolist() == [True, False, False]
    # ties: runs of equal codes across sorted positions 64 and 256 (a wave's and a block's edge)
    _, codes = morton_order(*case("ties")[2])
    assert len(codes) == 600 and len(np.unique(codes)) == 64
    assert codes[63] == codes[64] and codes[255] == codes[256]
    # overflow: every cost of the root is +inf, and the tie rule cuts at the lowest position
    lo, hi = case("overflow")[2]
    order, _ = morton_order(lo, hi)
    ext = hi - lo
    with np.errstate(over="ignore"):
        assert np.isinf(ext[:, 0] * ext[:, 1] + ext[:, 1] * ext[:, 2] + ext[:, 0] * ext[:, 2]).all() and np.isfinite(ext).all()
    assert sah_cut(lo[order], hi[order], 0, len(lo), 1, sah_max_depth(len(lo))) == 1
    # tiny: centroid bounds exactly three ulps of 1.0 wide
    assert centroid_extent(*case("tiny")[2]).tolist() == [3 * 2.0 ** -23] * 3
    # lowbits: every centroid sits on its cell exactly (codes == the cells' bits interleaved by plain Python integers), and
    # neighbours in the order of the cluster agree in every bit above the low 30 of 63
    lo, hi = case("lowbits")[2]
    cells = [(2 ** 21 - 1,) * 3] + _lowbits_cells().tolist()
    want = [sum(((c[a] >> b) & 1) << (3 * b + 2 - a) for b in range(21) for a in range(3)) for c in cells]
    assert centroid_codes(lo, hi).tolist() == want
    _, codes = morton_order(lo, hi)
    assert (np.bitwise_xor(codes[1:-2], codes[2:-1]) < np.uint64(1 << 30)).all()
    # chains: the codes are single bits; depth 64 exactly — the deepest tree pt_scene_create accepts — and beyond
    _, codes = morton_order(*case("chain64")[2])
    assert codes.tolist() == CHAIN_CODES
    assert reference("chain64", "lbvh")[2] == MAX_RENDER_DEPTH
    _, codes = morton_order(*case("chain_dups")[2])
    assert codes.tolist() == [0] * 3 + CHAIN_CODES
    assert reference("chain_dups", "lbvh")[2] == 66
    assert reference("chain_dups", "sah")[2] <= sah_max_depth(68) == 12


def test_the_oracle_traverses_the_64_level_chain_without_overflowing_its_stack(oracle):
    """The reference's traversal stack holds 64 entries (scene.h:251): on the reference LBVH tree of the chain the oracle must get
    through every level (stack_overflow counts the rays it abandons), and rays must actually reach the bottom of the chain."""
    hs, d, _ = case("chain64")
    nodes, root, _ = reference("chain64", "lbvh")
    img, cnt = oracle.render(desc_with_tree(d, nodes, root), hs.render_params(16, 12, 1, seed=9))
    assert cnt.stack_overflow == 0 and cnt.leaf_sphere > 0 and np.isfinite(img).all()
    assert cnt.inner_pops > 20 * cnt.paths                                  # the camera sits inside most of the chain's boxes


@pytest.mark.parametrize("name", [c for c in CASES if c != "chain_dups"])
def test_the_oracle_image_of_every_rendered_input_is_finite(oracle, name):
    """The GPU test compares images bit for bit; a NaN's sign and payload are not part of any contract, so no input may
    produce one (the overflowing triangles least of all)."""
    hs, d, _ = case(name)
    nodes, root, _ = reference(name, "sah")
    img, cnt = oracle.render(desc_with_tree(d, nodes, root), hs.render_params(16, 12, 1, seed=9))
    assert np.isfinite(img).all() and cnt.stack_overflow == 0


def test_big_input_sets_its_centroid_bounds_beyond_the_first_grid_trip():
    lo, hi = case("big")[2]
    assert len(lo) == BIG_N > BIG_FIRST_TRIP
    c = (hi + lo) * np.float32(0.5)
    first, rest = c[:BIG_FIRST_TRIP], c[BIG_FIRST_TRIP:]
    assert (rest.min(axis=0) < first.min(axis=0) - 0.5).all() and (rest.max(axis=0) > first.max(axis=0) + 0.5).all()
    # with the bounds of the first trip alone the order would be another one: the test can see the difference
    assert not np.array_equal(morton_order(lo, hi)[0][:1000], morton_order(lo[:BIG_FIRST_TRIP], hi[:BIG_FIRST_TRIP])[0][:1000])


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("method", sorted(METHODS))
@pytest.mark.parametrize("name", CASES)
def test_device_tree_is_the_reference_tree(oracle, name, method):
    """The device tree equals the reference tree; the device renders on it what the oracle renders on it, on the handed-in tree
    (fast_tree 0) and on the library's internal one (1).  A tree deeper than 64 levels is returned with its true depth and
    refused by pt_scene_create (host code, before any launch) — the depth contract of pt_bvh_build_device in pt_api.h."""
    hs, d, boxes = case(name)
    want = reference(name, method)
    d2, info = dev.build_bvh_device(d, METHODS[method])
    assert_same_tree(want, (info["nodes"], info["root"], info["depth"]), f"{name} {method}")
    if info["depth"] > MAX_RENDER_DEPTH:
        with pytest.raises(PtError) as e:
            dev.DeviceScene(d2).close()
        assert e.value.status == PT_ERR_BAD_SCENE and "deeper than the traversal stack" in str(e.value)
        return
    p = hs.render_params(16, 12, 1, seed=9)
    img_want, _ = oracle.render(d2, p)
    ds = dev.DeviceScene(d2)
    try:
        assert ds.info("bvh_depth") == info["depth"]
        for fast_tree in (0, 1):
            ds.set_option("fast_tree", fast_tree)
            assert_bit_equal(ds.render(p), img_want, f"{name} {method} fast_tree={fast_tree}")
    finally:
        ds.close()


def _assert_top_levels(nodes, root, boxes, method, levels):
    """The cuts and boxes of the top `levels` levels against the reference's per-node rules (the whole recursive reference would
    take too long at this size)."""
    n = len(boxes[0])
    order, codes = morton_order(*boxes)
    slo, shi = boxes[0][order], boxes[1][order]
    max_depth = sah_max_depth(n)
    todo = [(root, 0, n, 0)]                                               # slot, [first, end), first output slot (SAH)
    for level in range(1, levels + 1):
        nxt = []
        for slot, first, end, base in todo:
            if method == LBVH:
                m = lbvh_cut(codes, first, end - 1) + 1
                kids = (m - 1 if m - first == 1 else n + m - 1, m if end - m == 1 else n + m)
            else:
                m = sah_cut(slo, shi, first, end, level, max_depth)
                kids = (base + 2 * (m - first) - 2, base + 2 * (m - first) - 1 + 2 * (end - m) - 2)
            nd = nodes[slot]
            assert (nd["left"], nd["right"], nd["prim"]) == (*kids, -1), f"level {level} [{first}, {end}): cut {m}, device node {nd}"
            assert np.array_equal(nd["bmin"], slo[first:end].min(axis=0)) and np.array_equal(nd["bmax"], shi[first:end].max(axis=0))
            for kid, a, b, kbase in ((kids[0], first, m, base), (kids[1], m, end, base + 2 * (m - first) - 1)):
                if b - a > 1:
                    nxt.append((kid, a, b, kbase))
        todo = nxt


@pytest.mark.gpu
@pytest.mark.parametrize("method", sorted(METHODS))
def test_device_tree_beyond_one_pass_of_the_bounds_grid(method):
    """n > 262,144: the primitives that set the centroid bounds are read only on the second trip of centroid_bounds_kernel's
    grid-stride loop; bounds that miss them give another Morton order."""
    _, d, boxes = case("big")
    order, _ = morton_order(*boxes)
    d2, info = dev.build_bvh_device(d, METHODS[method])
    nodes, root = info["nodes"], info["root"]
    depth = check_tree(nodes, root, BIG_N, boxes)
    assert depth == info["depth"]
    if method == "lbvh":
        assert root == BIG_N and np.array_equal(nodes["prim"][:BIG_N], order)
        assert np.array_equal(nodes["bmin"][root], boxes[0].min(axis=0)) and np.array_equal(nodes["bmax"][root], boxes[1].max(axis=0))
    else:
        assert root == 2 * BIG_N - 2 and np.array_equal(inorder_prims(nodes, root), order)
        assert 19 <= depth <= sah_max_depth(BIG_N) == 24
    _assert_top_levels(nodes, root, boxes, METHODS[method], levels=6)
