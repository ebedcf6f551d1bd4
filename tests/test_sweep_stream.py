"""The sweep kernel's record stream (csrc/pt_kernels.h: SweepWindow, csrc/pt_trace_sweep_body.h step (3)): every body of the box
sweep works on four 8-byte pairs that the body BEFORE it read, whatever class that was, the first of them read in front of the
reciprocals from the octant the direction's sign bits name, and the last body of a phase reads 32 bytes it does not use.  None of
it may show: every frame here equals the oracle's bit for bit, and the same handle's frame with option "sweep_families" 0,
"sweep_pairs" 0 (one class, the general pairs: the stream in its plainest form) and "leaf_sweep" 0 (the tree), with equal path and
segment counts.  The stream itself — which bytes each body receives, the furthest byte read — is checked on the CPU by
tests/test_sweep_stream_host.py on the same scenes (tests/sweep_stream_cases.py)."""
import pytest
from conftest import assert_bit_equal, load_scene
from sweep_families_cases import CASES as FAMILY_CASES
from sweep_stream_cases import NOTHING_TO_HIT, TRANSITIONS, VIEWS, interleaved_tree, octants_of_the_views, view_params
from test_reg_stack import poor_tree
from test_sweep_families import check_frame, frame
from test_sweep_hit_word import cubes_scene

from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE
from pathtracer_cuda_interactive_amd import device as dev


@pytest.fixture(scope="module")
def cbox():
    hs, d = load_scene("cbox")
    ds = dev.DeviceScene(d)
    yield hs, d, ds
    ds.close()


@pytest.mark.gpu
def test_first_frame_cbox_8x4(oracle, cbox):
    """8 x 4 at 1 spp: 32 paths for the 256 lanes of the one block.  cbox's table has PAIR2 records of four classes, a
    SHARE_FLAT and SHARE pairs and the single: the stream crosses seven loops."""
    hs, d, ds = cbox
    assert ds.info("sweep_boxes") == 25
    info = check_frame(oracle, d, ds, hs.render_params(8, 4, 1, seed=3), "cbox 8x4x1")
    assert ds.counters().paths == 32
    assert info["sweep_pair2_records"] >= 5 and info["sweep_general_pairs"] == 0


@pytest.mark.gpu
def test_cbox_64x48x8(oracle, cbox):
    hs, d, ds = cbox
    check_frame(oracle, d, ds, hs.render_params(64, 48, 8, seed=22), "cbox 64x48x8")


@pytest.mark.gpu
def test_cbox_after_rebuild(oracle, cbox):
    """pt_scene_rebuild makes the tables anew and checks the stream's bound again."""
    hs, d, ds = cbox
    ds.rebuild()
    assert ds.info("sweep_boxes") == 25
    check_frame(oracle, d, ds, hs.render_params(16, 8, 2, seed=6), "cbox after a rebuild")


@pytest.mark.gpu
@pytest.mark.parametrize("groups", [2, 3])
def test_few_groups(oracle, groups):
    """2 groups (two cubes in a row share their y and z intervals: one PAIR2_x): the body that starts the stream is the one that
    ends it.  3: the pair's body fetches the single."""
    hs = cubes_scene(groups)
    d = poor_tree(hs.finalize(PT_BVH_SORT_REFERENCE), groups)
    ds = dev.DeviceScene(d)
    try:
        assert ds.info("sweep_boxes") == groups
        info = check_frame(oracle, d, ds, hs.render_params(16, 16, 2, seed=40 + groups), f"{groups} cubes")
        assert info["sweep_pair2_records"] == 1 and info["sweep_valu_model"] == 27 + 17 * (groups - 2)
    finally:
        ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["groups_31", "groups_32", "signed_zero", "flat_on_two_axes"])
def test_scene_of_the_families(oracle, name):
    """31 groups (fifteen PAIR2 and the single) and 32 (sixteen PAIR2, nothing behind the last: its body reads past the table);
    -0.0 against +0.0; boxes flat on two axes."""
    make, groups, want = FAMILY_CASES[name]
    hs = make()
    d = poor_tree(hs.finalize(PT_BVH_SORT_REFERENCE), 3)
    ds = dev.DeviceScene(d)
    try:
        assert ds.info("sweep_boxes") == groups, name
        info = check_frame(oracle, d, ds, hs.render_params(16, 8, 2, seed=61), name)
        assert {k: info[k] for k in want} == want, (name, info)
    finally:
        ds.close()


def frames_agree(oracle, d, ds, p, what):
    """check_frame of tests/test_sweep_families.py without its demand that some path of THIS frame goes on behind its camera
    segment (a view may face a record that has no area): the frame equals the oracle's, and the same handle's with
    sweep_families 0, sweep_pairs 0 and leaf_sweep 0, bit for bit, with equal path and segment counts.  Returns (info, counts)."""
    want, cnt = oracle.render(d, p)
    img, c, sweep, info = frame(ds, p)
    assert sweep == 1, what
    assert_bit_equal(img, want, what + ": against the oracle")
    assert c == (cnt.paths, cnt.segments), what
    for opts, swept in (({"sweep_families": 0}, 1), ({"sweep_pairs": 0}, 1), ({"leaf_sweep": 0}, 0)):
        img_o, c_o, sweep_o, _ = frame(ds, p, **opts)
        assert sweep_o == swept, (what, opts)
        assert_bit_equal(img, img_o, what + ": the stream of the families against %r" % (opts,))
        assert c_o == c, (what, opts)
    return info, c


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TRANSITIONS))
def test_class_transition(oracle, name):
    """One record of each of two classes in one table, for every ordered pair of the 20 classes, seen from between the two
    records at 16 x 16 x 4 along a space diagonal and back: camera rays of all eight octants (octant 7, whose table is the last
    and whose read past the end is the furthest, among them), and some path goes on behind its camera segment unless neither
    record has an area."""
    a, b, make, groups, per, want = TRANSITIONS[name]
    d = interleaved_tree(make().finalize(PT_BVH_SORT_REFERENCE), groups, per)
    ds = dev.DeviceScene(d)
    try:
        assert ds.info("sweep_boxes") == groups, name
        paths = segments = 0
        for k in range(len(VIEWS)):
            info, c = frames_agree(oracle, d, ds, view_params(k), f"{name}, view {k}")
            assert {key: info[key] for key in want} == want, (name, info)
            paths, segments = paths + c[0], segments + c[1]
        assert (segments > paths) == ((a, b) not in NOTHING_TO_HIT), (name, paths, segments)
    finally:
        ds.close()


def test_views_reach_every_octant():
    assert (octants_of_the_views() >= 4).all()
