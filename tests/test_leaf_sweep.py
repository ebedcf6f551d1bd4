"""The leaf sweep of trace_kernel_v2_sweep (csrc/pt_leaf_sweep.h, csrc/pt_trace_sweep_body.h): small scenes find the leaves a
segment tests by one test per distinct leaf box instead of a tree walk.  Exact traversal tests a leaf iff the ray hits the leaf's
own box, so the frame must equal the oracle's and the tree kernel's bit for bit, with equal work counters, and the launch must
report the variant, register-stack flag and LDS plan of the tree kernel it stands in for; info "leaf_sweep" alone tells them
apart.  Launches the predicate does not admit keep the tree.  The table builder and the mask operations are checked on the CPU
by tests/test_leaf_sweep_host.py."""
import numpy as np
import pytest
from conftest import assert_bit_equal, load_scene
from test_reg_stack import poor_tree, quads_scene
from trace_variants import Variant

from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE, PT_MAT_DIFFUSE, PT_TRAVERSAL_PRUNED, HostScene
from pathtracer_cuda_interactive_amd import device as dev

REG_BIT = 1 << 13
MAX_BOXES = 32               # csrc/pt_leaf_sweep.h: kSweepMaxBoxes
W, H, SPP = 64, 48, 8
DEFAULTS = {"leaf_sweep": 1, "reg_stack": 1, "octants": 1, "stats": 0, "fast_tree": 1, "v2_minw": 0}


@pytest.fixture(scope="module")
def cbox():
    hs, d = load_scene("cbox")
    ds = dev.DeviceScene(d)
    yield hs, d, ds
    ds.close()


_oracle_cache = {}


def oracle_frame(oracle, d, p):
    key = (p.width, p.height, p.spp, p.seed)
    if key not in _oracle_cache:
        _oracle_cache[key] = oracle.render(d, p)
    return _oracle_cache[key]


def render_with(ds, p, **opts):
    """(image, counters, {info}) of one frame under `opts`, options restored."""
    for k, v in opts.items():
        ds.set_option(k, v)
    try:
        img = ds.render(p)
        return img, ds.counters(), {k: ds.info(k) for k in ("leaf_sweep", "reg_stack", "path_bank", "lds_bytes", "trace_variant")}
    finally:
        for k in opts:
            ds.set_option(k, DEFAULTS[k])


@pytest.mark.gpu
def test_fewer_work_items_than_lanes(oracle, cbox):
    """8 x 4 at 1 spp: 32 paths for the 256 lanes of the one block.  Lanes that never receive a path hold an empty candidate
    mask and leave."""
    hs, d, ds = cbox
    assert ds.info("sweep_boxes") == 25
    p = hs.render_params(8, 4, 1, seed=3)
    want, cnt = oracle.render(d, p)
    img, c, info = render_with(ds, p)
    assert info["leaf_sweep"] == 1 and info["reg_stack"] == 1 and info["trace_variant"] & REG_BIT
    assert_bit_equal(img, want, "cbox 8x4x1")
    assert (c.paths, c.segments) == (cnt.paths, cnt.segments) and c.paths == 32


@pytest.mark.gpu
@pytest.mark.parametrize("minw", [5, 6])
def test_cbox_equals_oracle_and_tree(oracle, cbox, minw):
    """cbox 64 x 48 at 8 spp: the sweep's frame against the oracle's and the tree kernel's; the launch reports the tree kernel's
    variant and LDS plan."""
    hs, d, ds = cbox
    p = hs.render_params(W, H, SPP, seed=21)
    want, cnt = oracle_frame(oracle, d, p)
    what = f"cbox minw {minw}"
    img1, c1, i1 = render_with(ds, p, v2_minw=minw)
    img0, c0, i0 = render_with(ds, p, v2_minw=minw, leaf_sweep=0)
    assert (i1["leaf_sweep"], i0["leaf_sweep"]) == (1, 0), what
    assert i1["trace_variant"] == i0["trace_variant"] == Variant(2, 2, 0, 0, 2, 0, 0, 0, 40, 162, minw).code | REG_BIT, what
    assert i1["lds_bytes"] == i0["lds_bytes"] and i1["reg_stack"] == i0["reg_stack"] == 1 and i1["path_bank"] == i0["path_bank"] == 1, what
    assert_bit_equal(img1, want, what + ": against the oracle")
    assert_bit_equal(img1, img0, what + ": sweep against tree")
    assert (c1.paths, c1.segments) == (c0.paths, c0.segments) == (cnt.paths, cnt.segments), what


def grown_quads_scene(n, tris_per_quad=2):
    """n parallel quads (or their first triangles alone), each 1.5 times as large and as far away as the one before: the
    internal tree peels them off one by one, so its stack stays short however many there are, and the register stack admits
    scenes of more than 32 primitives."""
    hs = HostScene()
    hs.set_camera((0.1, 0.05, 4.0), (0.1, 0.05, 0.0), (0, 1, 0), 40.0, 24, 16, 2)
    hs.set_background((0.4, 0.5, 0.6))
    mats = [hs.add_material(PT_MAT_DIFFUSE, (0.7, 0.6 - 0.02 * k, 0.2 + 0.03 * k)) for k in range(3)]
    for k in range(n):
        z, s = -0.5 * 1.5 ** k, 0.4 * 1.5 ** k
        P = np.array([[-s, -s, z], [s, -s, z], [s, s, z], [-s, s, z]], np.float32)
        hs.add_mesh(P, np.array([[0, 1, 2], [0, 2, 3]][:tris_per_quad], np.int32), mats[k % 3],
                    radiance=(3.0, 2.5, 2.0) if k == n - 1 else None)
    return hs


def boundary_row(oracle, hs, tag, seed):
    d = poor_tree(hs.finalize(PT_BVH_SORT_REFERENCE), seed)       # a poor caller's tree: scene creation keeps its internal tree
    ds = dev.DeviceScene(d)
    try:
        p = hs.render_params(24, 16, 2, seed=40 + seed)
        want, cnt = oracle.render(d, p)
        img = ds.render(p)
        c = ds.counters()
        reg, sweep, boxes, res = ds.info("reg_stack"), ds.info("leaf_sweep"), ds.info("sweep_boxes"), ds.info("residency")
    finally:
        ds.close()
    what = f"{tag}: {d.num_shapes} primitives, residency {res}, reg_stack {reg}, leaf_sweep {sweep}, sweep_boxes {boxes}"
    print(what)
    return what, img, want, (c.paths, c.segments), (cnt.paths, cnt.segments), d.num_shapes, reg, sweep, boxes, res


@pytest.mark.gpu
def test_group_count_boundary(oracle):
    """Which scenes sweep: every launch the register stack admits whose scene is staged with its octant tables (residency 2)
    and has at most 64 primitives in at most 32 groups.
      - 8 .. 20 quads of tests/test_reg_stack.py (16 .. 40 triangles, a quad's two triangles share a box): up to 15 quads the
        register stack, and with it the sweep; beyond, the tree needs a fifth stack entry and both are off;
      - 16, 17, 20 and 24 grown quads: the register stack admits them, 34 .. 48 primitives use the high word of the mask;
      - 25, 31 and 32 grown quads: a table, but eight octant tables of 49 nodes and more are over their LDS limit (residency 1);
      - 33 grown quads are 66 primitives: no table (sweep_boxes 0);
      - 32 grown triangles are 32 groups of one: the most a launch admits; 33 and 40 are a table that no launch takes."""
    rows = [boundary_row(oracle, quads_scene(n), f"{n} quads", n) + (n,) for n in range(8, 21)]
    rows += [boundary_row(oracle, grown_quads_scene(n), f"{n} grown quads", n) + (n if n <= 32 else 0,)
             for n in (16, 17, 20, 24, 25, 31, 32, 33)]
    rows += [boundary_row(oracle, grown_quads_scene(n, 1), f"{n} grown triangles", n) + (n,) for n in (32, 33, 40)]
    for what, img, want, got_c, want_c, prims, reg, sweep, boxes, res, want_boxes in rows:
        assert_bit_equal(img, want, what)
        assert got_c == want_c, what
        assert boxes == want_boxes, what
        assert sweep == (reg if 1 <= boxes <= MAX_BOXES and res == 2 else 0), what
    swept = [r[5] for r in rows if r[7]]
    assert max(swept) == 48 and len([n for n in swept if n > 32]) >= 3, f"swept scenes of more than 32 primitives: {swept}"
    assert max(r[8] for r in rows if r[7]) == MAX_BOXES, "a swept scene with as many groups as a launch admits"
    kept = [r[0] for r in rows if not r[7]]
    assert any(r[6] == 0 for r in rows), f"a scene on the LDS stack: {kept}"
    assert any(r[6] == 1 and r[9] == 2 and r[8] > MAX_BOXES for r in rows), f"a scene with too many groups: {kept}"
    assert any(r[6] == 1 and r[9] == 1 and r[8] > 0 for r in rows), f"a scene without octant tables: {kept}"


def tie_scene():
    """quads_scene(8) with its nearest quad added a second time in another colour: four triangles in one group, each pair of
    copies hit at equal t.  Which copy a pixel shows is settled by the visit order of the caller's tree alone."""
    hs = quads_scene(8)
    twin = hs.add_material(PT_MAT_DIFFUSE, (0.1, 0.2, 0.9))
    z = -0.4 * 0                                       # quads_scene's own expression: -0.0, and +0 would be another box
    P = np.array([[-1, -1, z], [1, -1, z], [1, 1, z], [-1, 1, z]], np.float32)
    hs.add_mesh(P, np.array([[0, 1, 2], [0, 2, 3]], np.int32), twin)
    return hs


@pytest.mark.gpu
def test_ties_are_settled_in_the_callers_order(oracle):
    """The same 18 triangles under two caller's trees.  The internal tree and the group table are made from the leaf boxes and
    do not know the caller's tree; the tie branch of the leaf test is the one place of a sweep frame that reads it (reruns give
    the caller's answer either way).  The oracle's two frames differ, and the sweep matches each: the branch is reached."""
    hs = tie_scene()
    d0 = hs.finalize(PT_BVH_SORT_REFERENCE)
    p = hs.render_params(24, 16, 2, seed=9)
    frames = []
    for seed in (1, 2, 3, 4, 5, 6):
        d = poor_tree(d0, seed)
        want, cnt = oracle.render(d, p)
        if frames and np.array_equal(frames[0][1], want):
            continue
        frames.append((d, want, cnt))
        if len(frames) == 2:
            break
    assert len(frames) == 2, "no two caller's trees that order the twins differently"
    for d, want, cnt in frames:
        ds = dev.DeviceScene(d)
        try:
            img = ds.render(p)
            c = ds.counters()
            assert ds.info("leaf_sweep") == 1 and ds.info("sweep_boxes") == 8
        finally:
            ds.close()
        assert_bit_equal(img, want, "twin quads")
        assert (c.paths, c.segments) == (cnt.paths, cnt.segments)


@pytest.mark.gpu
def test_rays_with_a_zero_direction_component_are_rerun(oracle, cbox):
    """A frame large enough to hold rays whose 1/d is not finite (about 20 per million segments on cbox): the counting frame, which
    runs the tree kernel on the same rays, reports them; the sweep frame equals the oracle's."""
    hs, d, ds = cbox
    p = hs.render_params(320, 240, 4, seed=2)
    want, cnt = oracle.render(d, p)
    _, _, i_stats = render_with(ds, p, stats=1)
    reruns = ds.info("redo_segments")
    print("redo_segments", reruns)
    assert i_stats["leaf_sweep"] == 0 and reruns > 0
    img, c, info = render_with(ds, p)
    assert info["leaf_sweep"] == 1
    assert_bit_equal(img, want, "cbox 320x240x4")
    assert (c.paths, c.segments) == (cnt.paths, cnt.segments)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["pruned", "stats", "one_table", "callers_tree", "reg_stack_off"])
def test_not_eligible_keeps_the_tree(oracle, cbox, how):
    hs, d, ds = cbox
    p = hs.render_params(W, H, SPP, seed=21)
    want, cnt = oracle_frame(oracle, d, p)
    opts = {"pruned": {}, "stats": {"stats": 1}, "one_table": {"octants": 0}, "callers_tree": {"fast_tree": 0},
            "reg_stack_off": {"reg_stack": 0}}[how]
    if how == "pruned":
        p.traversal = PT_TRAVERSAL_PRUNED
    img, c, info = render_with(ds, p, **opts)
    assert info["leaf_sweep"] == 0, how
    assert_bit_equal(img, want, how)
    assert (c.paths, c.segments) == (cnt.paths, cnt.segments) or how == "pruned", how


@pytest.mark.gpu
def test_scene_in_global_memory_keeps_the_tree(oracle):
    hs, d = load_scene("bunny")
    ds = dev.DeviceScene(d)
    try:
        p = hs.render_params(32, 24, 1, seed=5)
        want, _ = oracle.render(d, p)
        img = ds.render(p)
        assert ds.info("leaf_sweep") == 0 and ds.info("sweep_boxes") == 0
    finally:
        ds.close()
    assert_bit_equal(img, want, "bunny 32x24x1")


@pytest.mark.gpu
def test_geometry_update_returns_to_the_tree(oracle):
    """After pt_scene_update with new geometry the leaf boxes of a group need not be equal any more: the handle keeps to the tree
    (here the update hands in the geometry it had, so the frame is still cbox's)."""
    hs, d = load_scene("cbox")
    p = hs.render_params(W, H, SPP, seed=21)
    want, cnt = oracle_frame(oracle, d, p)
    ds = dev.DeviceScene(d)
    try:
        ds.render(p)
        assert ds.info("leaf_sweep") == 1
        ds.update(dev.edited_desc(d))
        img = ds.render(p)
        c = ds.counters()
        assert ds.info("leaf_sweep") == 0 and ds.info("sweep_boxes") == 0 and ds.info("reg_stack") == 1
    finally:
        ds.close()
    assert_bit_equal(img, want, "cbox after a geometry update")
    assert (c.paths, c.segments) == (cnt.paths, cnt.segments)


@pytest.mark.gpu
def test_progressive_frames_in_flight(oracle, cbox):
    """pt_render_accumulate, 4 frames of 2 spp with two frames in flight: the accumulated image against the oracle's."""
    import torch
    hs, d, ds = cbox
    assert ds.info("frames_in_flight") == 2
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    want = None
    for k in range(4):
        p = hs.render_params(W, H, 2, seed=31)
        p.sample_offset, p.stream_stride = 2 * k, 8
        ds.accumulate_into(p, acc.data_ptr(), stream)
        assert ds.info("leaf_sweep") == 1, f"frame {k}"
        part, _ = oracle.render(d, p, accumulate=True)
        want = part if k == 0 else (want + part).astype(np.float32)
    torch.cuda.synchronize()
    assert_bit_equal(acc.cpu().numpy(), want, "4 accumulated frames of 2 spp")
