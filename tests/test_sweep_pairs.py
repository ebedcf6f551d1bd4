"""The sweep kernel's pair classes (csrc/pt_sweep_pairs.h): pairs of groups whose boxes share an axis interval compute that
axis's slab products once (SHARE), a shared flat interval once in all (SHARE_FLAT).  None of it may show: every frame here
equals the oracle's bit for bit, and the same handle's frame with option "sweep_pairs" 0 (the tables in the groups' own order,
every pair general) and with "leaf_sweep" 0 (the tree).  The info keys "sweep_share_pairs", "sweep_flat_pairs" (with _x, _y,
_z) and "sweep_general_pairs" prove that the class a scene is made for was in the launch.  The pairing and the tables are
checked on the CPU by tests/test_sweep_pairs_host.py, on the same scenes (tests/sweep_pairs_cases.py)."""
import pytest
from conftest import assert_bit_equal, load_scene
from sweep_pairs_cases import CASES, GROUPS
from test_reg_stack import poor_tree

from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE
from pathtracer_cuda_interactive_amd import device as dev

CLASS_KEYS = ["sweep_share_pairs", "sweep_flat_pairs", "sweep_general_pairs"] + \
             [k + a for k in ("sweep_share_pairs", "sweep_flat_pairs") for a in ("_x", "_y", "_z")]


def frame(ds, p, **opts):
    """(image, (paths, segments), leaf_sweep, {class counts}) of one frame under `opts`, options back at their defaults after it."""
    for k, v in opts.items():
        ds.set_option(k, v)
    try:
        classes = {k: ds.info(k) for k in CLASS_KEYS}
        img = ds.render(p)
        c = ds.counters()
        return img, (c.paths, c.segments), ds.info("leaf_sweep"), classes
    finally:
        for k in opts:
            ds.set_option(k, 1)


def check_frame(oracle, d, ds, p, what):
    """One frame with the pair classes, one with every pair general, one on the tree: all three the oracle's.  Returns the classes."""
    want, cnt = oracle.render(d, p)
    img, c, sweep, classes = frame(ds, p)
    img_general, c_general, sweep_general, classes_general = frame(ds, p, sweep_pairs=0)
    img_tree, c_tree, sweep_tree, _ = frame(ds, p, leaf_sweep=0)
    groups = ds.info("sweep_boxes")
    print(what, "groups", groups, classes, "paths", c[0], "segments", c[1])
    assert (sweep, sweep_general, sweep_tree) == (1, 1, 0), what
    assert_bit_equal(img, want, what + ": against the oracle")
    assert_bit_equal(img, img_general, what + ": pair classes against general pairs")
    assert_bit_equal(img, img_tree, what + ": sweep against tree")
    assert c == c_general == c_tree == (cnt.paths, cnt.segments), what
    assert c[1] > c[0], what + ": no path went beyond its camera segment"
    assert 2 * (classes["sweep_share_pairs"] + classes["sweep_flat_pairs"] + classes["sweep_general_pairs"]) + groups % 2 == groups, what
    assert classes_general == dict({k: 0 for k in CLASS_KEYS}, sweep_general_pairs=groups // 2), what
    return classes


@pytest.fixture(scope="module")
def cbox():
    hs, d = load_scene("cbox")
    ds = dev.DeviceScene(d)
    yield hs, d, ds
    ds.close()


@pytest.mark.gpu
def test_first_frame_cbox_8x4(oracle, cbox):
    """8 x 4 at 1 spp: 32 paths for the 256 lanes of the one block.  cbox's 25 groups: 11 sharing pairs, a general pair, the tail."""
    hs, d, ds = cbox
    assert ds.info("sweep_boxes") == 25
    classes = check_frame(oracle, d, ds, hs.render_params(8, 4, 1, seed=3), "cbox 8x4x1")
    assert ds.counters().paths == 32
    assert classes["sweep_share_pairs"] + classes["sweep_flat_pairs"] >= 10
    assert classes["sweep_flat_pairs_y"] >= 4 and classes["sweep_share_pairs_y"] >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_scene_of_one_class(oracle, name):
    """16 x 8 at 2 spp on the scenes of tests/sweep_pairs_cases.py, under a poor caller's tree so that scene creation keeps its own."""
    make, above_zero, zero = CASES[name]
    hs = make()
    d = poor_tree(hs.finalize(PT_BVH_SORT_REFERENCE), 3)
    ds = dev.DeviceScene(d)
    try:
        assert ds.info("sweep_boxes") == GROUPS[name], name
        classes = check_frame(oracle, d, ds, hs.render_params(16, 8, 2, seed=60), name)
        for k in above_zero:
            assert classes[k] > 0, (name, k, classes)
        for k in zero:
            assert classes[k] == 0, (name, k, classes)
    finally:
        ds.close()


@pytest.mark.gpu
def test_cbox_64x48x8(oracle, cbox):
    hs, d, ds = cbox
    check_frame(oracle, d, ds, hs.render_params(64, 48, 8, seed=21), "cbox 64x48x8")


@pytest.mark.gpu
def test_option_is_checked(cbox):
    _, _, ds = cbox
    with pytest.raises(dev.PtError):
        ds.set_option("sweep_pairs", 2)
    with pytest.raises(dev.PtError):
        ds.info("sweep_share_pairs_w")
