"""Scenes for the box sweep's skip table (csrc/pt_sweep_skip.h), shared by tests/test_sweep_skip_host.py (their triangles
through tests/native/sweep_skip_check.cpp) and tests/test_sweep_skip.py (their frames on the GPU).

Every scene has 16 .. 32 triangles (tests/sweep_pairs_cases.py says why).  CASES maps a name to (constructor, {count of the
host checker: value}); the counts are groups, skip_groups (groups with a mask) and planes (distinct axis and coordinate)."""
import numpy as np
from sweep_pairs_cases import QUAD, _loose_triangles, _panel, _scene, flat_scene

from pathtracer_cuda_interactive_amd import PT_MAT_DIFFUSE, HostScene
from pathtracer_cuda_interactive_amd import device as dev

LIGHT = (3.0, 2.5, 2.0)


def triangles(desc):
    """[N][9] float32: p0 p1 p2 of every shape of a scene of triangles, by primitive."""
    sh = dev.shape_table(desc)
    out = np.zeros((desc.num_shapes, 9), np.float32)
    for k, s in enumerate(sh):
        m = desc.meshes[int(s["mesh_index"])]
        idx = np.ctypeslib.as_array(m.indices, shape=(m.num_faces, 3))[int(s["face_index"])]
        pos = np.ctypeslib.as_array(m.positions, shape=(m.num_vertices, 3))
        out[k] = pos[idx].reshape(9)
    return out


def _block(hs, mat, centre, half, height, angle):
    """A block turned about y by `angle`, standing on y = 0: four upright faces whose boxes are flat on no axis, and its top."""
    cs, sn = np.cos(angle), np.sin(angle)
    corners = [(centre[0] + cs * x - sn * z, centre[1] + sn * x + cs * z) for x, z in ((-half, -half), (half, -half), (half, half), (-half, half))]
    for k in range(4):
        (x0, z0), (x1, z1) = corners[k], corners[(k + 1) % 4]
        hs.add_mesh(np.array([[x0, 0, z0], [x1, 0, z1], [x1, height, z1], [x0, height, z0]], np.float32), QUAD, mat)
    hs.add_mesh(np.array([[x, height, z] for x, z in corners], np.float32), QUAD, mat)


def floor_block_scene():
    """A floor quad under a rotated block, a back wall and a light above: bounces off the floor skip the floor alone, bounces
    off the block's sides skip nothing."""
    hs, mats = _scene(eye=(0.1, 1.1, 3.2), look=(0.0, 0.4, 0.0))
    _panel(hs, mats[0], 1, 0.0, (-2.0, -2.0), (2.0, 2.0))
    _panel(hs, mats[1], 2, -2.0, (-2.0, 0.0), (2.0, 2.5))
    _block(hs, mats[2], (0.1, -0.2), 0.6, 0.9, 0.35)
    _panel(hs, mats[3], 1, 2.4, (-0.7, -0.9), (0.8, 0.6), radiance=LIGHT)
    return hs


def zero_plane_scene():
    """A floor in the plane y = 0 whose vertices are +0.0 and -0.0 in turn, and a second quad in y = -0.0 beside it: one plane.
    12 loose triangles above them."""
    hs, mats = _scene(eye=(0.13, 1.4, 2.6), look=(0.0, 0.0, 0.0))
    P = np.array([[-2.0, 0.0, -2.0], [0.1, -0.0, -2.0], [0.1, 0.0, 1.8], [-2.0, -0.0, 1.8]], np.float32)
    hs.add_mesh(P, QUAD, mats[0])
    _panel(hs, mats[1], 1, np.float32(-0.0), (0.3, -1.7), (2.1, 1.6))
    _loose_triangles(hs, mats, 12, seed=17)
    return hs


def room_scene():
    """A room of cbox's size and coordinates, open towards the camera: planes at 548.8, 559.2 and 556.0, where a bounce's origin
    misses the plane's coordinate by an ulp a few times in a hundred, and at 0, where it never does.  A light just under the
    ceiling and four loose triangles inside."""
    hs = HostScene()
    hs.set_camera((278.0, 273.0, -800.0), (278.0, 273.0, 0.0), (0, 1, 0), 39.0, 16, 16, 4)
    hs.set_background((0.0, 0.0, 0.0))
    mats = [hs.add_material(PT_MAT_DIFFUSE, (0.7, 0.6 - 0.05 * k, 0.3 + 0.1 * k)) for k in range(4)]
    _panel(hs, mats[0], 1, 0.0, (0.0, 0.0), (556.0, 559.2))
    _panel(hs, mats[0], 1, 548.8, (0.0, 0.0), (556.0, 559.2))
    _panel(hs, mats[1], 2, 559.2, (0.0, 0.0), (556.0, 548.8))
    _panel(hs, mats[2], 0, 0.0, (0.0, 0.0), (548.8, 559.2))
    _panel(hs, mats[3], 0, 556.0, (0.0, 0.0), (548.8, 559.2))
    _panel(hs, mats[0], 1, 548.7, (213.0, 227.0), (343.0, 332.0), radiance=(17.0, 12.0, 4.0))
    rng = np.random.default_rng(23)
    for k in range(4):
        P = (np.array([150.0 + 80.0 * k, 120.0 + 60.0 * k, 200.0 + 50.0 * k]) + rng.uniform(-90.0, 90.0, (3, 3))).astype(np.float32)
        hs.add_mesh(P, np.array([[0, 1, 2]], np.int32), mats[k])
    return hs


def planes_scene(groups):
    """`groups` groups, 31 or 32: planes along the view axis, each 1.5 times as large and as far away as the one before, with
    two different triangles in each (one in the last where the count is odd).  The two triangles of a plane name each other."""
    hs = HostScene()
    hs.set_camera((0.1, 0.05, 4.0), (0.1, 0.05, 0.0), (0, 1, 0), 40.0, 16, 8, 2)
    hs.set_background((0.4, 0.5, 0.6))
    mats = [hs.add_material(PT_MAT_DIFFUSE, (0.7, 0.6 - 0.02 * k, 0.2 + 0.03 * k)) for k in range(3)]
    for k in range(16):
        z, s = -0.5 * 1.5 ** k, 0.4 * 1.5 ** k
        P = np.array([[-s, -s, z], [s, -s, z], [s, s, z], [-0.9 * s, -0.2 * s, z], [0.3 * s, 0.8 * s, z], [-0.7 * s, 0.9 * s, z]], np.float32)
        faces = [[0, 1, 2], [3, 4, 5]] if 2 * k + 2 <= groups else [[0, 1, 2]]
        hs.add_mesh(P, np.array(faces, np.int32), mats[k % 3], radiance=LIGHT if k == 15 else None)
    return hs


CASES = {
    "floor_block": (floor_block_scene, {"groups": 9, "skip_groups": 5, "planes": 4}),
    "split_wall": (flat_scene, {"groups": 12, "skip_groups": 12, "planes": 6}),
    "zero_plane": (zero_plane_scene, {"planes": 1}),
    "room": (room_scene, {"groups": 10, "skip_groups": 6, "planes": 6}),
    "planes31": (lambda: planes_scene(31), {"groups": 31, "skip_groups": 31, "planes": 16}),
    "planes32": (lambda: planes_scene(32), {"groups": 32, "skip_groups": 32, "planes": 16}),
}
