"""The hit word of the sweep kernel (csrc/pt_trace_sweep_body.h): the box sweep shifts one bit per group into a register,
h = 2 * h + hit, as a compare and one add-with-carry, two groups per iteration and the last of an odd count alone.  Scenes of
1, 2, 3, 31 and 32 groups cover the odd tail alone, a single pair, a pair and the tail, and the full word with bit 31 set; the
cameras make the camera rays hit the box of one group alone (each end of the table among them), of all groups, and of none.
Every 16 x 16 frame at 2 spp equals the oracle's bit for bit with equal work counters, and the launch must be a sweep launch
(all but the scene of one group: test_few_groups).

A scene sweeps only with an internal tree (16 primitives and more), so the scenes of few groups hold many triangles per box:
the triangles on three corners of a cube that do not share a face have the cube's box, all of them.  31 and 32 groups are the
grown triangles of tests/test_leaf_sweep.py, one behind the other: a camera between two of them looks at one end of the row."""
import itertools

import numpy as np
import pytest
from conftest import assert_bit_equal
from test_leaf_sweep import grown_quads_scene, render_with
from test_reg_stack import poor_tree

from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE, PT_MAT_DIFFUSE, HostScene
from pathtracer_cuda_interactive_amd import device as dev

pytestmark = pytest.mark.gpu

CORNERS = np.array(list(itertools.product((0.0, 1.0), repeat=3)), np.float32)
# corner triples that touch all six faces of the cube: their triangle's box is the cube
FULL_BOX = [t for t in itertools.combinations(range(8), 3)
            if all(CORNERS[list(t), a].min() == 0.0 and CORNERS[list(t), a].max() == 1.0 for a in range(3))]
SPACING = 3.0


def cubes_scene(groups):
    """`groups` unit cubes in a row along x, each holding ceil(16 / groups) triangles that have the cube's box."""
    per = -(-16 // groups)
    hs = HostScene()
    hs.set_camera((0.5, 0.5, 6.0), (0.5, 0.5, 0.5), (0, 1, 0), 20.0, 16, 16, 2)
    hs.set_background((0.4, 0.5, 0.6))
    for g in range(groups):
        m = hs.add_material(PT_MAT_DIFFUSE, (0.7 - 0.2 * g, 0.3 + 0.2 * g, 0.2 + 0.1 * g))
        P = CORNERS + np.array([SPACING * g, 0, 0], np.float32)
        I = np.array(FULL_BOX[5 * g: 5 * g + per], np.int32)
        hs.add_mesh(P.astype(np.float32), I, m, radiance=(3.0, 2.5, 2.0) if g == groups - 1 else None)
    return hs


def cube_views(groups):
    """name -> (eye, target, fov): one cube alone for each cube, all of them along the row, none."""
    views = {f"cube {g} alone": ((SPACING * g + 0.5, 0.5, 6.0), (SPACING * g + 0.5, 0.5, 0.5), 12.0) for g in range(groups)}
    views["all along the row"] = ((-4.0, 0.45, 0.55), (0.5, 0.5, 0.5), 4.0)
    views["none"] = ((0.5, 0.5, 6.0), (0.5, 0.5, 12.0), 20.0)
    return views


def grown_views(n):
    """The grown triangles stand at z = -0.5 * 1.5^k with half-width 0.4 * 1.5^k.  From the first scene's camera every ray near
    the axis passes through all boxes; from between the two nearest, looking back, through the first alone; from between the
    two farthest, looking on, through the last alone."""
    z = [-0.5 * 1.5 ** k for k in range(n)]
    return {
        "all": ((0.1, 0.05, 4.0), (0.1, 0.05, 0.0), 2.0),
        "the nearest alone": ((0.1, -0.05, 0.5 * (z[0] + z[1])), (0.1, -0.05, 0.0), 20.0),
        "the farthest alone": ((0.1, 0.05, 0.5 * (z[n - 2] + z[n - 1])), (0.1, 0.05, 2.0 * z[n - 1]), 20.0),
        "none": ((0.1, 0.05, 4.0), (0.1, 0.05, 8.0), 20.0),
    }


def check_views(oracle, hs, groups, views, what, tree_seed, want_sweep=1):
    d = poor_tree(hs.finalize(PT_BVH_SORT_REFERENCE), tree_seed)      # a poor caller's tree: scene creation keeps its internal tree
    ds = dev.DeviceScene(d)
    try:
        assert ds.info("sweep_boxes") == (groups if want_sweep else 0), what
        deeper = 0
        for k, (name, (eye, target, fov)) in enumerate(views.items()):
            cam = HostScene()                                         # a camera of its own: the scene's desc stays as finalized
            cam.set_camera(eye, target, (0, 1, 0), fov, 16, 16, 2)
            p = cam.render_params(16, 16, 2, seed=90 + k)
            want, cnt = oracle.render(d, p)
            img, c, info = render_with(ds, p)
            print(what, name, "paths", c.paths, "segments", c.segments)
            assert info["leaf_sweep"] == want_sweep, f"{what}, {name}"
            assert_bit_equal(img, want, f"{what}, {name}")
            assert (c.paths, c.segments) == (cnt.paths, cnt.segments), f"{what}, {name}"
            if name == "none":
                assert c.segments == c.paths, f"{what}: a camera ray of the view 'none' hit something"
            else:
                deeper += c.segments > c.paths
        assert deeper == len(views) - 1, f"{what}: a view whose camera rays hit nothing"
    finally:
        ds.close()


@pytest.mark.parametrize("groups", [1, 2, 3])
def test_few_groups(oracle, groups):
    """One group cannot sweep: where every leaf has the same box, every inner node of every tree over them has it too, so no tree
    visits fewer boxes than the caller's, scene creation keeps no internal tree (it wants 10 % fewer visits) and the handle
    holds no table.  The frames of that scene are checked all the same, on the tree; a group count of 1 is not reachable on
    the device, and the tail alone after no pair is what 3 and 31 groups run after their pairs."""
    check_views(oracle, cubes_scene(groups), groups, cube_views(groups), f"{groups} cubes", tree_seed=groups,
                want_sweep=0 if groups == 1 else 1)


@pytest.mark.parametrize("n", [31, 32])
def test_the_full_word(oracle, n):
    check_views(oracle, grown_quads_scene(n, 1), n, grown_views(n), f"{n} grown triangles", tree_seed=n)
