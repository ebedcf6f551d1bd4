"""Scenes for the PAIR2 records of the box sweep (csrc/pt_sweep_families.h), shared by tests/test_sweep_families_host.py
(their leaf boxes through tests/native/sweep_families_check.cpp) and tests/test_sweep_families.py (their frames on the GPU).

Every scene has 16 .. 32 triangles, each its own group: a triangle is placed by the box it is to have, its corners on the box's
faces.  A PAIR2 is two triangles with the same interval on two axes (each flat or not).  CASES maps a name to (constructor,
groups, {info key: value} the launch must report under the default options).  The values follow from the count model of
pt_sweep_families.h: general pair 35, SHARE 31, SHARE_FLAT 29, single 17, PAIR2 27 / 25 / 23 with 0 / 1 / 2 flat axes."""
import numpy as np
from sweep_pairs_cases import _loose_triangles, _scene, _uniq

from pathtracer_cuda_interactive_amd import PT_MAT_DIFFUSE, HostScene

LIGHT = (3.0, 2.5, 2.0)


def _tri(hs, mat, lo, hi, radiance=None):
    """One triangle whose box is lo .. hi: two corners on opposite faces of x and z, the third on the upper y face."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    mid = np.where(lo == hi, lo, lo + (hi - lo) * np.float32(0.5)).astype(np.float32)        # a flat axis keeps its bits: -0.0 stays -0.0
    P = np.array([[lo[0], lo[1], hi[2]], [hi[0], lo[1], lo[2]], [mid[0], hi[1], mid[2]]], np.float32)
    hs.add_mesh(P, np.array([[0, 1, 2]], np.int32), mat, radiance=radiance)


def _pair2(hs, mats, r, u, flat_b, flat_c, centre):
    """Record r: two triangles with the same interval on both axes other than u (flat where asked), apart on u.  Every bound
    carries an offset of r's own, so nothing is shared by accident."""
    b, c = [a for a in range(3) if a != u]
    lo, hi = [0.0] * 3, [0.0] * 3
    lo[b] = centre[b] - 0.3 - _uniq(r)
    hi[b] = lo[b] if flat_b else centre[b] + 0.3 + _uniq(r + 13)
    lo[c] = centre[c] - 0.25 - _uniq(r + 27)
    hi[c] = lo[c] if flat_c else centre[c] + 0.25 + _uniq(r + 41)
    for side in range(2):
        lo[u] = centre[u] + (-0.36 - _uniq(r + 5) if side == 0 else 0.03 + _uniq(r + 9))
        hi[u] = centre[u] + (-0.04 + _uniq(r + 17) if side == 0 else 0.34 + _uniq(r + 23))
        _tri(hs, mats[(r + side) % 4], lo, hi, radiance=LIGHT if r == 0 and side == 0 else None)


def _grid(r):
    """A place in front of the camera for record r."""
    return [-1.5 + 1.0 * (r % 4), -0.8 + 0.8 * (r // 4), -2.0 - 0.1 * r]


def pair2_all_scene():
    """Every PAIR2 class once (trip count 1 in twelve loops): u = x, y, z, each flatness of the two shared axes; a box flat on
    two axes is among them (both shared axes flat: a segment).  Two loose triangles make a general pair."""
    hs, mats = _scene()
    for u in range(3):
        for fl in range(4):
            _pair2(hs, mats, 4 * u + fl, u, bool(fl & 1), bool(fl & 2), _grid(4 * u + fl))
    _loose_triangles(hs, mats, 2, seed=5, first=1)
    return hs


def pair2_back_edge_scene():
    """Three records of PAIR2_x (flat y, z), two of PAIR2_z (x, flat y), two of PAIR2_y (x, z): every loop that runs takes its
    back edge.  Three loose triangles: a general pair and the single."""
    hs, mats = _scene()
    for r, (u, fb, fc) in enumerate([(0, True, False)] * 3 + [(2, False, True)] * 2 + [(1, False, False)] * 2):
        _pair2(hs, mats, r, u, fb, fc, _grid(r))
    _loose_triangles(hs, mats, 3, seed=6, first=1)
    return hs


def no_pair2_scene():
    """The class is absent: three pairs that share one axis each (SHARE_x, SHARE_FLAT_y, SHARE_z) and 11 loose triangles; every
    PAIR2 loop is skipped by its word's branch."""
    hs, mats = _scene()
    for r, (axis, flat) in enumerate([(0, False), (1, True), (2, False)]):
        centre = _grid(r + 4)
        for side in range(2):
            lo = [centre[x] - 0.3 - _uniq(7 * r + side + 3 * x) + 0.7 * side * (x != axis) for x in range(3)]
            hi = [centre[x] + 0.3 + _uniq(7 * r + side + 40 + 3 * x) + 0.7 * side * (x != axis) for x in range(3)]
            lo[axis] = centre[axis] - 0.3 - _uniq(r + 90)
            hi[axis] = lo[axis] if flat else centre[axis] + 0.3 + _uniq(r + 95)
            _tri(hs, mats[(r + side) % 4], lo, hi, radiance=LIGHT if r == 0 and side == 0 else None)
    _loose_triangles(hs, mats, 11, seed=8, first=1)
    return hs


def _slabs(count):
    """`count` triangles, two to a slab along the view axis, each slab 1.5 times as large and as far away as the one before (the
    internal tree peels them off one by one, so its stack stays short); the two of a slab share their x and y intervals."""
    hs = HostScene()
    hs.set_camera((0.1, 0.05, 4.0), (0.1, 0.05, 0.0), (0, 1, 0), 40.0, 16, 8, 2)
    hs.set_background((0.4, 0.5, 0.6))
    mats = [hs.add_material(PT_MAT_DIFFUSE, (0.7, 0.6 - 0.02 * k, 0.2 + 0.03 * k)) for k in range(3)]
    for n in range(count):
        k, second = n // 2, n % 2
        z, s = -0.5 * 1.5 ** k, 0.4 * 1.5 ** k
        if second:
            lo, hi = [-s, -0.8 * s, z - 0.07 * s], [s, 0.8 * s, z - 0.01 * s]
        else:
            lo, hi = [-s, -0.8 * s, z - 0.2 * s], [s, 0.8 * s, z - 0.1 * s]
        _tri(hs, mats[k % 3], lo, hi, radiance=LIGHT if n == count - 1 else None)
    return hs


def groups_32_scene():
    """32 groups, the most a launch admits: sixteen PAIR2_z (x, y), the hit word full."""
    return _slabs(32)


def groups_31_scene():
    """31 groups: fifteen PAIR2_z (x, y) and the single."""
    return _slabs(31)


def signed_zero_scene():
    """Two triangles with the same x interval, one in the plane z = -0.0 and one in z = +0.0: different planes by their bits, so
    the two are a SHARE_x pair and never a PAIR2.  Four more in z = -0.0, +0.0, -0.0, +0.0 with nothing else in common: two
    SHARE_FLAT_z pairs, each inside its own plane.  Ten loose triangles share nothing."""
    hs, mats = _scene(eye=(0.13, 0.07, 1.5))
    for k, z in enumerate((np.float32(-0.0), np.float32(0.0))):
        _tri(hs, mats[k], [-1.6, -0.9 + 1.0 * k + _uniq(k), z], [-0.4, -0.1 + 1.0 * k + _uniq(k + 3), z])
    for k, z in enumerate((np.float32(-0.0), np.float32(0.0), np.float32(-0.0), np.float32(0.0))):
        _tri(hs, mats[k], [0.1 + 0.45 * k + _uniq(k + 6), -0.8 + 0.3 * k + _uniq(k + 11), z], [0.5 + 0.45 * k + _uniq(k + 16), -0.2 + 0.3 * k + _uniq(k + 21), z])
    _loose_triangles(hs, mats, 10, seed=11)
    return hs


def flat_on_two_axes_scene():
    """Two segments on one line along x (triangles without area, boxes flat on y and z): a PAIR2_x with both shared axes flat.
    A third segment on a line along z in the same plane y: it shares y alone and stays single.  13 loose triangles."""
    hs, mats = _scene()
    _tri(hs, mats[0], [-0.6, -1.0, -1.5], [0.1, -1.0, -1.5])
    _tri(hs, mats[1], [0.4, -1.0, -1.5], [1.3, -1.0, -1.5])
    _tri(hs, mats[2], [-1.1, -1.0, -2.4], [-1.1, -1.0, -1.7])
    _loose_triangles(hs, mats, 13, seed=13)
    return hs


P2, MODEL = "sweep_pair2_records", "sweep_valu_model"
CASES = {
    "pair2_all": (pair2_all_scene, 26, {P2: 12, MODEL: 3 * (27 + 25 + 25 + 23) + 35, "sweep_general_pairs": 1}),
    "pair2_back_edge": (pair2_back_edge_scene, 17, {P2: 7, MODEL: 5 * 25 + 2 * 27 + 35 + 17, "sweep_flat_pairs_y": 5, "sweep_share_pairs_z": 5,
                                                    "sweep_share_pairs_x": 4}),
    "no_pair2": (no_pair2_scene, 17, {P2: 0, MODEL: 31 + 29 + 31 + 5 * 35 + 17, "sweep_share_pairs_x": 1, "sweep_flat_pairs_y": 1, "sweep_share_pairs_z": 1}),
    "groups_32": (groups_32_scene, 32, {P2: 16, MODEL: 16 * 27, "sweep_share_pairs_x": 16, "sweep_share_pairs_y": 16}),
    "groups_31": (groups_31_scene, 31, {P2: 15, MODEL: 15 * 27 + 17}),
    "signed_zero": (signed_zero_scene, 16, {P2: 0, MODEL: 31 + 2 * 29 + 5 * 35, "sweep_share_pairs_x": 1, "sweep_flat_pairs_z": 2}),
    "flat_on_two_axes": (flat_on_two_axes_scene, 16, {P2: 1, MODEL: 23 + 7 * 35, "sweep_flat_pairs_y": 1, "sweep_flat_pairs_z": 1}),
}
