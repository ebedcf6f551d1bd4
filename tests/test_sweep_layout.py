"""The sweep kernel on its own tables (csrc/pt_sweep_layout.h): a sweep launch stages one box table per octant and one chained
slot record per primitive where the tree kernel stages the octant node tables, keeps one hit bit per group and tests a group's
primitives along the chain of its records.  None of it may show: every frame here equals the oracle's and the same handle's
frame with option "leaf_sweep" 0 bit for bit, with equal work counters.  Every frame traces more segments than paths, so a frame
of background alone cannot pass.  The layout itself is checked on the CPU by tests/test_sweep_layout_host.py.

What a scene needs to sweep is unchanged (tests/test_leaf_sweep.py): an internal tree (16 primitives and more), the register
stack, the octant tables (at most 48 inner nodes) and at most 32 groups.  The shapes of the layout that lie outside of that —
two primitives, four triangles alone, 64 primitives in 32 pairs — are rendered too and must keep the tree; inside it the same
shapes appear as part of a larger scene."""
import numpy as np
import pytest
from conftest import assert_bit_equal, load_scene
from test_leaf_sweep import grown_quads_scene, render_with, tie_scene
from test_reg_stack import poor_tree, quads_scene

from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE, PT_MAT_DIFFUSE, HostScene
from pathtracer_cuda_interactive_amd import device as dev


@pytest.fixture(scope="module")
def cbox():
    hs, d = load_scene("cbox")
    ds = dev.DeviceScene(d)
    yield hs, d, ds
    ds.close()


def check_frame(oracle, d, ds, p, what, want_sweep):
    """One frame with the sweep allowed and one on the tree, both against the oracle."""
    want, cnt = oracle.render(d, p)
    img1, c1, i1 = render_with(ds, p)
    img0, c0, i0 = render_with(ds, p, leaf_sweep=0)
    print(what, "leaf_sweep", i1["leaf_sweep"], "sweep_boxes", ds.info("sweep_boxes"), "paths", c1.paths, "segments", c1.segments)
    assert (i1["leaf_sweep"], i0["leaf_sweep"]) == (want_sweep, 0), what
    assert i1["lds_bytes"] == i0["lds_bytes"] and i1["trace_variant"] == i0["trace_variant"] and i1["reg_stack"] == i0["reg_stack"], what
    assert_bit_equal(img1, want, what + ": against the oracle")
    assert_bit_equal(img1, img0, what + ": sweep against tree")
    assert (c1.paths, c1.segments) == (c0.paths, c0.segments) == (cnt.paths, cnt.segments), what
    assert c1.segments > c1.paths, what + ": no path went beyond its camera segment"
    return img1


def check_scene(oracle, hs, what, want_sweep, want_boxes, tree_seed=1, size=(24, 16, 2)):
    d = poor_tree(hs.finalize(PT_BVH_SORT_REFERENCE), tree_seed)      # a poor caller's tree: scene creation keeps its internal tree
    ds = dev.DeviceScene(d)
    try:
        assert ds.info("sweep_boxes") == want_boxes, what
        check_frame(oracle, d, ds, hs.render_params(*size, seed=50 + tree_seed), what, want_sweep)
    finally:
        ds.close()


@pytest.mark.gpu
def test_first_frame_cbox_8x4(oracle, cbox):
    """8 x 4 at 1 spp: 32 paths for the 256 lanes of the one block; 25 groups, an odd count (12 pairs and the tail)."""
    hs, d, ds = cbox
    assert ds.info("sweep_boxes") == 25
    p = hs.render_params(8, 4, 1, seed=3)
    check_frame(oracle, d, ds, p, "cbox 8x4x1", 1)
    assert ds.counters().paths == 32


@pytest.mark.gpu
@pytest.mark.parametrize("minw", [5, 6])
def test_cbox_both_instantiations(oracle, cbox, minw):
    hs, d, ds = cbox
    ds.set_option("v2_minw", minw)
    try:
        check_frame(oracle, d, ds, hs.render_params(64, 48, 8, seed=21), f"cbox 64x48x8 minw {minw}", 1)
    finally:
        ds.set_option("v2_minw", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [31, 32])
def test_odd_and_even_group_counts_at_the_top(oracle, n):
    """n triangles in n groups of one: 31 ends on the tail iteration, 32 fills the hit word to its last bit."""
    check_scene(oracle, grown_quads_scene(n, 1), f"{n} grown triangles", 1, n, tree_seed=n)


def with_one_quad(n):
    """n single triangles and one quad behind them: n + 1 groups, one of them of two primitives (the only chain of two)."""
    hs = grown_quads_scene(n, 1)
    z, s = -0.5 * 1.5 ** n, 0.4 * 1.5 ** n
    P = np.array([[-s, -s, z], [s, -s, z], [s, s, z], [-s, s, z]], np.float32)
    hs.add_mesh(P, np.array([[0, 1, 2], [0, 2, 3]], np.int32), hs.add_material(PT_MAT_DIFFUSE, (0.2, 0.7, 0.3)))
    return hs


@pytest.mark.gpu
def test_one_group_of_two(oracle):
    check_scene(oracle, with_one_quad(16), "16 triangles and one quad", 1, 17, tree_seed=3)


def folded_quad_scene():
    """quads_scene(7) and, in front of it, a square folded along both of its diagonals: four different triangles that each
    hold three corners of the square, so all four have the square's box and make one group, a chain of four.  The corners
    lie at two depths, so no two of the four are coplanar."""
    hs = quads_scene(7)
    m = hs.add_material(PT_MAT_DIFFUSE, (0.1, 0.2, 0.9))
    P = np.array([[-1, -1, 0.5], [1, -1, 0.3], [1, 1, 0.5], [-1, 1, 0.3]], np.float32)
    hs.add_mesh(P, np.array([[0, 1, 2], [0, 2, 3], [0, 1, 3], [1, 2, 3]], np.int32), m)
    return hs


@pytest.mark.gpu
def test_four_triangles_with_one_box(oracle):
    check_scene(oracle, folded_quad_scene(), "7 quads and a folded square", 1, 8, tree_seed=2)


@pytest.mark.gpu
def test_48_primitives_in_24_pairs(oracle):
    """The largest scene of pairs a launch admits (octant tables exist up to 48 inner nodes): slots 24 .. 47 are all successors."""
    check_scene(oracle, grown_quads_scene(24), "24 grown quads", 1, 24, tree_seed=24)


def tiny_scene(tris):
    hs = HostScene()
    hs.set_camera((0.1, 0.05, 4.0), (0.1, 0.05, 0.0), (0, 1, 0), 40.0, 24, 16, 2)
    hs.set_background((0.4, 0.5, 0.6))
    m = hs.add_material(PT_MAT_DIFFUSE, (0.7, 0.6, 0.2))
    P = np.array([[-1, -1, 0.5], [1, -1, 0.3], [1, 1, 0.5], [-1, 1, 0.3], [-1.5, -1.5, -1], [1.5, -1.5, -1], [1.5, 1.5, -1]], np.float32)
    hs.add_mesh(P, np.array(tris, np.int32), m)
    return hs


@pytest.mark.gpu
@pytest.mark.parametrize("what,tris,boxes", [
    ("one group of two", [[0, 1, 2], [0, 2, 3]], 0),
    ("two primitives in two groups", [[0, 1, 2], [4, 5, 6]], 0),
    ("four triangles with one box", [[0, 1, 2], [0, 2, 3], [0, 1, 3], [1, 2, 3]], 0),
])
def test_scenes_without_an_internal_tree_keep_the_tree(oracle, what, tris, boxes):
    """The layout's smallest shapes as whole scenes: below 16 primitives scene creation builds no internal tree, so there is no
    group table and the launch walks the caller's tree."""
    check_scene(oracle, tiny_scene(tris), what, 0, boxes)


@pytest.mark.gpu
def test_64_primitives_in_32_pairs_keep_the_tree(oracle):
    """32 groups of two fill the hit word and the link's slot range (tests/native/sweep_layout_check.cpp walks them); on the
    device 63 inner nodes are over the limit of the octant tables, so the handle holds the groups and the launch keeps the tree."""
    check_scene(oracle, grown_quads_scene(32), "32 grown quads", 0, 32, tree_seed=32)


@pytest.mark.gpu
def test_coincident_quads_tie_scene(oracle):
    """tests/test_leaf_sweep.py's twin quads under two caller's trees that order the twins differently: the four triangles of the
    twins are one chain, tested in ascending order whatever the caller's tree says; the tie branch alone settles who wins."""
    hs = tie_scene()
    d0 = hs.finalize(PT_BVH_SORT_REFERENCE)
    p = hs.render_params(24, 16, 2, seed=9)
    frames = []
    for seed in (1, 2, 3, 4, 5, 6):
        d = poor_tree(d0, seed)
        want, _ = oracle.render(d, p)
        if frames and np.array_equal(frames[0][1], want):
            continue
        frames.append((d, want))
        if len(frames) == 2:
            break
    assert len(frames) == 2, "no two caller's trees that order the twins differently"
    for k, (d, _) in enumerate(frames):
        ds = dev.DeviceScene(d)
        try:
            assert ds.info("sweep_boxes") == 8
            check_frame(oracle, d, ds, p, f"twin quads, tree {k}", 1)
        finally:
            ds.close()


@pytest.mark.gpu
def test_rays_with_a_zero_direction_component(oracle, cbox):
    """A camera flattened into the horizontal plane through its origin: every camera ray has direction.y == 0, so its 1/d is not
    finite and the segment is rerun on the caller's tree; the bounces after it are swept."""
    hs, d, ds = cbox
    p = hs.render_params(96, 72, 4, seed=2)
    for k in range(3):
        p.cam_vertical[k] = 0.0
    p.cam_top_left[1] = p.cam_origin[1]
    p.cam_horizontal[1] = 0.0
    _, _, i_stats = render_with(ds, p, stats=1)                    # the counting frame runs the tree kernel on the same rays
    reruns = ds.info("redo_segments")
    print("redo_segments", reruns)
    assert i_stats["leaf_sweep"] == 0 and reruns > 0
    check_frame(oracle, d, ds, p, "cbox 96x72x4, flat camera", 1)
    assert reruns >= ds.counters().paths


@pytest.mark.gpu
def test_geometry_update_drops_the_tables(oracle):
    hs, d = load_scene("cbox")
    p = hs.render_params(64, 48, 4, seed=21)
    ds = dev.DeviceScene(d)
    try:
        check_frame(oracle, d, ds, p, "cbox before the update", 1)
        ds.update(dev.edited_desc(d))
        assert ds.info("sweep_boxes") == 0
        check_frame(oracle, d, ds, p, "cbox after a geometry update", 0)
        assert ds.info("reg_stack") == 1
    finally:
        ds.close()


@pytest.mark.gpu
def test_progressive_frames_in_flight(oracle, cbox):
    """pt_render_accumulate, 4 frames of 2 spp with two frames in flight, each staging the handle's tables."""
    import torch
    hs, d, ds = cbox
    assert ds.info("frames_in_flight") == 2
    W, H = 64, 48
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    want = None
    for k in range(4):
        p = hs.render_params(W, H, 2, seed=31)
        p.sample_offset, p.stream_stride = 2 * k, 8
        ds.accumulate_into(p, acc.data_ptr(), stream)
        assert ds.info("leaf_sweep") == 1, f"frame {k}"
        part, cnt = oracle.render(d, p, accumulate=True)
        assert cnt.segments > cnt.paths
        want = part if k == 0 else (want + part).astype(np.float32)
    torch.cuda.synchronize()
    assert_bit_equal(acc.cpu().numpy(), want, "4 accumulated frames of 2 spp")
    ds.set_option("leaf_sweep", 0)
    try:
        acc0 = torch.zeros_like(acc)
        for k in range(4):
            p = hs.render_params(W, H, 2, seed=31)
            p.sample_offset, p.stream_stride = 2 * k, 8
            ds.accumulate_into(p, acc0.data_ptr(), stream)
            assert ds.info("leaf_sweep") == 0, f"frame {k} on the tree"
        torch.cuda.synchronize()
    finally:
        ds.set_option("leaf_sweep", 1)
    assert_bit_equal(acc.cpu().numpy(), acc0.cpu().numpy(), "accumulated frames: sweep against tree")
