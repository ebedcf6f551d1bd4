"""The sweep kernel's PAIR2 records (csrc/pt_sweep_families.h): two boxes with the same interval on two axes compute both axes
once.  None of it may show: every frame here equals the oracle's bit for bit, and the same handle's frame with option
"sweep_families" 0 (the pair classes alone), "sweep_pairs" 0 (every pair general) and "leaf_sweep" 0 (the tree), with equal path
and segment counts.  The info keys "sweep_pair2_records", "sweep_valu_model" and the pair keys prove that the class a scene is
made for was in the launch.  The placement and the tables are checked on the CPU by tests/test_sweep_families_host.py, on the
same scenes (tests/sweep_families_cases.py)."""
import pytest
from conftest import assert_bit_equal, load_scene
from sweep_families_cases import CASES
from test_reg_stack import poor_tree

from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE
from pathtracer_cuda_interactive_amd import device as dev

KEYS = ["sweep_pair2_records", "sweep_valu_model", "sweep_general_pairs", "sweep_share_pairs", "sweep_flat_pairs"] + \
       [k + a for k in ("sweep_share_pairs", "sweep_flat_pairs") for a in ("_x", "_y", "_z")]
DEFAULTS = {"sweep_families": 1, "sweep_pairs": 1, "leaf_sweep": 1}


def frame(ds, p, **opts):
    """(image, (paths, segments), leaf_sweep, {info}) of one frame under `opts`, options back at their defaults after it."""
    for k, v in opts.items():
        ds.set_option(k, v)
    try:
        info = {k: ds.info(k) for k in KEYS}
        img = ds.render(p)
        c = ds.counters()
        return img, (c.paths, c.segments), ds.info("leaf_sweep"), info
    finally:
        for k in opts:
            ds.set_option(k, DEFAULTS[k])


def check_frame(oracle, d, ds, p, what):
    """One frame with the PAIR2 records, and one each without them, with every pair general and on the tree: all
    four the oracle's.  Returns the info of the first."""
    want, cnt = oracle.render(d, p)
    groups = ds.info("sweep_boxes")
    img, c, sweep, info = frame(ds, p)
    print(what, "groups", groups, info, "paths", c[0], "segments", c[1])
    assert sweep == 1, what
    assert_bit_equal(img, want, what + ": against the oracle")
    assert c == (cnt.paths, cnt.segments), what
    assert c[1] > c[0], what + ": no path went beyond its camera segment"
    for opts, swept in (({"sweep_families": 0}, 1), ({"sweep_pairs": 0}, 1), ({"leaf_sweep": 0}, 0)):
        img_o, c_o, sweep_o, info_o = frame(ds, p, **opts)
        assert sweep_o == swept, (what, opts)
        assert_bit_equal(img, img_o, what + ": families against %r" % (opts,))
        assert c_o == c, (what, opts)
        if opts == {"sweep_families": 0}:
            assert info_o["sweep_pair2_records"] == 0, what
            assert info["sweep_valu_model"] <= info_o["sweep_valu_model"], what
        if opts == {"sweep_pairs": 0}:
            assert info_o == dict({k: 0 for k in KEYS}, sweep_general_pairs=groups // 2, sweep_valu_model=35 * (groups // 2) + 17 * (groups % 2)), what
    # every group is in one record: a PAIR2 and a pair hold two, the single one
    assert 2 * (info["sweep_share_pairs"] + info["sweep_flat_pairs"] + info["sweep_general_pairs"]) + groups % 2 == groups, what
    return info


@pytest.fixture(scope="module")
def cbox():
    hs, d = load_scene("cbox")
    ds = dev.DeviceScene(d)
    yield hs, d, ds
    ds.close()


@pytest.mark.gpu
def test_first_frame_cbox_8x4(oracle, cbox):
    """8 x 4 at 1 spp: 32 paths for the 256 lanes of the one block.  cbox's 25 groups: six PAIR2 records, 353 or fewer VALU by the
    model where the pair classes alone come to 377 .. 381."""
    hs, d, ds = cbox
    assert ds.info("sweep_boxes") == 25
    info = check_frame(oracle, d, ds, hs.render_params(8, 4, 1, seed=3), "cbox 8x4x1")
    assert ds.counters().paths == 32
    assert info["sweep_pair2_records"] >= 5
    assert info["sweep_valu_model"] <= 353


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_scene_of_one_class(oracle, name):
    """16 x 8 at 2 spp on the scenes of tests/sweep_families_cases.py, under a poor caller's tree so that scene creation keeps its own."""
    make, groups, want = CASES[name]
    hs = make()
    d = poor_tree(hs.finalize(PT_BVH_SORT_REFERENCE), 3)
    ds = dev.DeviceScene(d)
    try:
        assert ds.info("sweep_boxes") == groups, name
        info = check_frame(oracle, d, ds, hs.render_params(16, 8, 2, seed=60), name)
        assert {k: info[k] for k in want} == want, (name, info)
    finally:
        ds.close()


@pytest.mark.gpu
def test_cbox_64x48x8(oracle, cbox):
    hs, d, ds = cbox
    check_frame(oracle, d, ds, hs.render_params(64, 48, 8, seed=21), "cbox 64x48x8")


@pytest.mark.gpu
def test_rebuild_places_the_records_again(oracle, cbox):
    """pt_scene_rebuild makes the sweep's tables anew: the families are in the launch after it as before it."""
    hs, d, ds = cbox
    ds.rebuild()
    if ds.info("sweep_boxes"):
        info = check_frame(oracle, d, ds, hs.render_params(16, 8, 2, seed=5), "cbox after a rebuild")
        assert info["sweep_valu_model"] <= 353


@pytest.mark.gpu
def test_option_is_checked(cbox):
    _, _, ds = cbox
    for bad in (-1, 2):
        with pytest.raises(dev.PtError):
            ds.set_option("sweep_families", bad)
    assert ds.info("sweep_pair2_records") >= 5
