"""Scenes for the pair classes of the box sweep (csrc/pt_sweep_pairs.h), shared by tests/test_sweep_pairs_host.py (their leaf
boxes through tests/native/sweep_pairs_check.cpp) and tests/test_sweep_pairs.py (their frames on the GPU).

Every scene has 16 .. 32 triangles: scene creation builds an internal tree from 16 primitives on, a tree over fewer than 32
leaves never needs more than the register stack's four entries, and the octant tables exist up to 48 inner nodes.  A planar
quad is cut into two triangles with the quad's own box (one group); a "ramp" is a planar quad whose box is flat on no axis.
CASES maps a name to (constructor, the info keys that must be above zero, the info keys that must be zero)."""
import numpy as np

from pathtracer_cuda_interactive_amd import PT_MAT_DIFFUSE, HostScene

QUAD = np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def _scene(eye=(0.13, 0.07, 0.21), look=(0.2, 0.1, -1.0)):
    hs = HostScene()
    hs.set_camera(eye, look, (0, 1, 0), 75.0, 16, 8, 2)
    hs.set_background((0.4, 0.5, 0.6))
    mats = [hs.add_material(PT_MAT_DIFFUSE, (0.75, 0.6 - 0.05 * k, 0.25 + 0.06 * k)) for k in range(4)]
    return hs, mats


def _ramp(hs, mat, lo, hi, radiance=None):
    """The quad (lo.x, lo.y, lo.z) (hi.x, lo.y, lo.z) (hi.x, hi.y, hi.z) (lo.x, hi.y, hi.z): it rises in z as it goes up in y, so
    both of its triangles have the box lo .. hi."""
    P = np.array([[lo[0], lo[1], lo[2]], [hi[0], lo[1], lo[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], hi[2]]], np.float32)
    hs.add_mesh(P, QUAD, mat, radiance=radiance)


def _panel(hs, mat, axis, plane, lo, hi, radiance=None):
    """An axis-aligned quad in the plane `axis` = plane, from lo to hi on the two other axes (ascending)."""
    b, c = [a for a in range(3) if a != axis]
    P = np.zeros((4, 3), np.float32)
    P[:, axis] = plane
    P[:, b] = (lo[0], hi[0], hi[0], lo[0])
    P[:, c] = (lo[1], lo[1], hi[1], hi[1])
    hs.add_mesh(P, QUAD, mat, radiance=radiance)


def _uniq(k):
    """A small offset no two calls share: every interval that is not shared on purpose is distinct."""
    return 0.011 * k + 0.0007 * k * k


def share_scene():
    """(a) 12 ramps around the camera, two by two with the SAME interval on one axis and nothing else in common: two pairs each
    of SHARE_x, SHARE_y and SHARE_z."""
    hs, mats = _scene()
    n = 0
    for axis in range(3):
        for rep in range(2):
            s_lo, s_hi = -0.9 + 0.7 * rep + 0.05 * axis, -0.1 + 0.7 * rep + 0.09 * axis       # the shared interval
            for side in (-1.0, 1.0):
                n += 1
                b, c = [a for a in range(3) if a != axis]
                lo, hi = [0.0] * 3, [0.0] * 3
                lo[axis], hi[axis] = s_lo, s_hi
                # on the two other axes: to one side of the camera on b, spread along c, every bound unlike any other
                lo[b], hi[b] = (side * 2.0 - 0.5 + _uniq(n), side * 2.0 + 0.4 + _uniq(n + 20))
                lo[c], hi[c] = (-1.6 + 1.1 * rep + side * 0.3 + _uniq(n + 40), -0.7 + 1.1 * rep + side * 0.3 + _uniq(n + 60))
                _ramp(hs, mats[n % 4], lo, hi, radiance=(3.0, 2.5, 2.0) if n == 12 else None)
    return hs


def flat_scene():
    """(b) an open room: every wall, the floor and the ceiling are two panels of different sizes in one plane: two pairs each of
    SHARE_FLAT_x, SHARE_FLAT_y and SHARE_FLAT_z."""
    hs, mats = _scene()
    n = 0
    for axis in range(3):
        for plane in (-2.0, 2.0 + 0.25 * axis):
            for part in range(2):
                n += 1
                lo = (-1.9 + 2.0 * part + _uniq(n), -1.7 + _uniq(n + 20) + 0.3 * part)
                hi = (-0.2 + 2.0 * part + _uniq(n + 40), 1.5 + _uniq(n + 60) - 0.2 * part)
                _panel(hs, mats[n % 4], axis, plane, lo, hi, radiance=(3.0, 2.5, 2.0) if n == 6 else None)
    return hs


def _loose_triangles(hs, mats, count, seed, first=0):
    """`count` triangles scattered around the origin, every coordinate drawn on its own: no two boxes share a bound."""
    rng = np.random.default_rng(seed)
    for k in range(count):
        centre = rng.uniform(-1.0, 1.0, 3)
        centre *= (1.6 + 0.9 * rng.uniform()) / np.linalg.norm(centre)
        P = (centre + rng.uniform(-0.7, 0.7, (3, 3))).astype(np.float32)
        hs.add_mesh(P, np.array([[0, 1, 2]], np.int32), mats[(first + k) % 4], radiance=(3.0, 2.5, 2.0) if k == 0 and first == 0 else None)


def general_scene():
    """(c) 17 loose triangles: 17 groups, no two equal intervals, so 8 general pairs and the odd tail."""
    hs, mats = _scene()
    _loose_triangles(hs, mats, 17, seed=7)
    return hs


def full_scene():
    """(d) 32 groups, the most a launch admits: 16 planes along the view axis, each 1.5 times as large and as far away as the one
    before (the internal tree peels them off one by one, so its stack stays short), with two different triangles in each:
    16 pairs of SHARE_FLAT_z."""
    hs = HostScene()
    hs.set_camera((0.1, 0.05, 4.0), (0.1, 0.05, 0.0), (0, 1, 0), 40.0, 16, 8, 2)
    hs.set_background((0.4, 0.5, 0.6))
    mats = [hs.add_material(PT_MAT_DIFFUSE, (0.7, 0.6 - 0.02 * k, 0.2 + 0.03 * k)) for k in range(3)]
    for k in range(16):
        z, s = -0.5 * 1.5 ** k, 0.4 * 1.5 ** k
        P = np.array([[-s, -s, z], [s, -s, z], [s, s, z], [-0.9 * s, -0.2 * s, z], [0.3 * s, 0.8 * s, z], [-0.7 * s, 0.9 * s, z]], np.float32)
        hs.add_mesh(P, np.array([[0, 1, 2], [3, 4, 5]], np.int32), mats[k % 3], radiance=(3.0, 2.5, 2.0) if k == 15 else None)
    return hs


def signed_zero_scene():
    """(e) two quads side by side with the same y interval, one in the plane z = -0.0 and one in z = +0.0: different planes by
    their bits, so the pair is SHARE_y and never SHARE_FLAT_z.  14 loose triangles around them share nothing."""
    hs, mats = _scene(eye=(0.13, 0.07, 1.5))
    _panel(hs, mats[0], 2, np.float32(-0.0), (-1.9, -0.8), (-0.3, 0.9))
    _panel(hs, mats[1], 2, np.float32(0.0), (0.2, -0.8), (1.7, 0.9))
    _loose_triangles(hs, mats, 14, seed=11)
    return hs


def flat_on_two_axes_scene():
    """(f) a triangle of three points on a line along x: no area, a box flat on y and on z.  It lies in the plane y = -1 of a
    floor panel, so the two are a pair of SHARE_FLAT_y.  14 loose triangles around them share nothing."""
    hs, mats = _scene()
    _panel(hs, mats[0], 1, -1.0, (-1.8, -1.9), (1.6, 1.4))
    P = np.array([[-0.6, -1.0, -0.5], [0.1, -1.0, -0.5], [0.9, -1.0, -0.5]], np.float32)
    hs.add_mesh(P, np.array([[0, 1, 2]], np.int32), mats[1])
    _loose_triangles(hs, mats, 14, seed=13)
    return hs


X, Y, Z = "_x", "_y", "_z"
CASES = {
    "share": (share_scene, ["sweep_share_pairs" + a for a in (X, Y, Z)], ["sweep_flat_pairs"]),
    "flat": (flat_scene, ["sweep_flat_pairs" + a for a in (X, Y, Z)], []),
    "general": (general_scene, ["sweep_general_pairs"], ["sweep_share_pairs", "sweep_flat_pairs"]),
    "full": (full_scene, ["sweep_flat_pairs" + Z], []),
    "signed_zero": (signed_zero_scene, ["sweep_share_pairs" + Y], ["sweep_flat_pairs" + Z]),
    "flat_on_two_axes": (flat_on_two_axes_scene, ["sweep_flat_pairs" + Y], []),
}
# groups each scene has, and whether the count is odd (the single's tail)
GROUPS = {"share": 12, "flat": 12, "general": 17, "full": 32, "signed_zero": 16, "flat_on_two_axes": 16}


def triangle_boxes(desc):
    """[N][6] float32: min.xyz max.xyz of every leaf of the caller's tree, by primitive."""
    import ctypes as C

    from pathtracer_cuda_interactive_amd import device as dev
    nodes = np.frombuffer((C.c_char * (desc.num_nodes * dev.NODE_DTYPE.itemsize)).from_address(C.addressof(desc.nodes.contents)),
                          dtype=dev.NODE_DTYPE)
    leaves = nodes[nodes["prim"] >= 0]
    assert len(leaves) == desc.num_shapes
    boxes = np.zeros((desc.num_shapes, 6), np.float32)
    boxes[leaves["prim"], :3] = leaves["bmin"]
    boxes[leaves["prim"], 3:] = leaves["bmax"]
    return boxes
