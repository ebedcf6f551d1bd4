"""The sweep kernel's skip word (csrc/pt_sweep_skip.h, option "sweep_self_skip"): a bounce that starts on an axis-aligned plane
does not test that plane's triangles.  None of it may show: every frame here equals the oracle's bit for bit, with equal path and
segment counts, under option 1 (default) and 0, and the two frames of a handle equal each other.  The info keys
"sweep_skip_groups" and "sweep_skip_planes" prove that a table was in the launch.  The lemma, the tables and the kernel's rule
are checked on the CPU by tests/test_sweep_skip_host.py, on the same scenes (tests/sweep_skip_cases.py)."""
import pytest
from conftest import assert_bit_equal, load_scene
from sweep_skip_cases import CASES
from test_reg_stack import poor_tree

from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE
from pathtracer_cuda_interactive_amd import device as dev


def frame(ds, p, skip):
    """(image, (paths, segments), leaf_sweep, (skip_groups, skip_planes)) of one frame under option "sweep_self_skip" = skip."""
    ds.set_option("sweep_self_skip", skip)
    try:
        info = (ds.info("sweep_skip_groups"), ds.info("sweep_skip_planes"))
        img = ds.render(p)
        c = ds.counters()
        return img, (c.paths, c.segments), ds.info("leaf_sweep"), info
    finally:
        ds.set_option("sweep_self_skip", 1)


def check_frame(oracle, d, ds, p, what, swept=1, bounces=True):
    """One frame with the skip word and one without: both the oracle's.  Returns (skip_groups, skip_planes) of the first."""
    want, cnt = oracle.render(d, p)
    img1, c1, s1, info1 = frame(ds, p, 1)
    print(what, "groups", ds.info("sweep_boxes"), "skip groups / planes", info1, "paths", c1[0], "segments", c1[1])
    assert s1 == swept, what
    assert_bit_equal(img1, want, what + ": option 1 against the oracle")
    assert c1 == (cnt.paths, cnt.segments), what
    assert (c1[1] > c1[0]) == bounces, what
    img0, c0, s0, info0 = frame(ds, p, 0)
    assert s0 == swept and info0 == (0, 0), what
    assert_bit_equal(img0, want, what + ": option 0 against the oracle")
    assert c0 == c1, what
    return info1


@pytest.fixture(scope="module")
def cbox():
    hs, d = load_scene("cbox")
    ds = dev.DeviceScene(d)
    yield hs, d, ds
    ds.close()


@pytest.mark.gpu
def test_first_frame_cbox_8x4(oracle, cbox):
    """8 x 4 at 1 spp: 32 paths for the 256 lanes of the one block.  15 of cbox's 25 groups lie flat in 7 planes."""
    hs, d, ds = cbox
    assert ds.info("sweep_boxes") == 25
    info = check_frame(oracle, d, ds, hs.render_params(8, 4, 1, seed=3), "cbox 8x4x1")
    assert ds.counters().paths == 32
    assert info == (15, 7)


@pytest.mark.gpu
def test_cbox_64x48x8(oracle, cbox):
    hs, d, ds = cbox
    assert check_frame(oracle, d, ds, hs.render_params(64, 48, 8, seed=21), "cbox 64x48x8") == (15, 7)


@pytest.mark.gpu
def test_cbox_under_the_other_tables(oracle, cbox):
    """The mask is in the bit order of the table the launch sweeps: the pair classes alone, and the groups' own order."""
    hs, d, ds = cbox
    for opts in ({"sweep_families": 0}, {"sweep_pairs": 0}):
        for k, v in opts.items():
            ds.set_option(k, v)
        try:
            assert check_frame(oracle, d, ds, hs.render_params(16, 16, 4, seed=8), "cbox %r" % (opts,)) == (15, 7)
        finally:
            for k in opts:
                ds.set_option(k, 1)


@pytest.mark.gpu
def test_max_depth_1(oracle, cbox):
    """Nothing bounces: every segment is a camera ray, whose skip word is zero."""
    hs, d, ds = cbox
    p = hs.render_params(16, 16, 4, seed=9)
    p.max_depth = 1
    check_frame(oracle, d, ds, p, "cbox max_depth 1", bounces=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_scene(oracle, name):
    """The scenes of tests/sweep_skip_cases.py at their own 16 x 16 or 16 x 8, under a poor caller's tree so that scene creation
    keeps its own: a floor under a rotated block, a coplanar split wall, a plane at 0 with vertices at -0.0, a room at cbox's
    coordinates (origins that miss the plane by an ulp), 31 and 32 groups."""
    make, want = CASES[name]
    hs = make()
    d = poor_tree(hs.finalize(PT_BVH_SORT_REFERENCE), 3)
    ds = dev.DeviceScene(d)
    try:
        info = check_frame(oracle, d, ds, hs.render_params(seed=60), name)
        if "skip_groups" in want:
            assert info == (want["skip_groups"], want["planes"]), name
        assert info[0] > 0, name
    finally:
        ds.close()


@pytest.mark.gpu
def test_rebuild_then_update(oracle):
    """pt_scene_rebuild makes the skip table anew with the sweep's tables; pt_scene_update drops it with them, and the tree
    kernel renders.  (A handle of its own: the update is for good.)"""
    hs, d = load_scene("cbox")
    ds = dev.DeviceScene(d)
    try:
        ds.rebuild()
        if ds.info("sweep_boxes"):
            assert check_frame(oracle, d, ds, hs.render_params(64, 48, 8, seed=21), "cbox after a rebuild") == (15, 7)
        ds.update(d)
        assert ds.info("sweep_boxes") == 0 and ds.info("sweep_skip_groups") == 0
        want, cnt = oracle.render(d, hs.render_params(16, 16, 4, seed=12))
        for skip in (1, 0):
            img, c, swept, info = frame(ds, hs.render_params(16, 16, 4, seed=12), skip)
            assert swept == 0 and info == (0, 0)
            assert_bit_equal(img, want, "cbox after an update, option %d" % skip)
            assert c == (cnt.paths, cnt.segments)
    finally:
        ds.close()


@pytest.mark.gpu
def test_option_is_checked(cbox):
    _, _, ds = cbox
    for bad in (-1, 2):
        with pytest.raises(dev.PtError):
            ds.set_option("sweep_self_skip", bad)
    assert ds.info("sweep_skip_groups") == 15
