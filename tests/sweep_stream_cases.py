"""Scenes for the sweep kernel's record stream (csrc/pt_kernels.h: SweepWindow), shared by tests/test_sweep_stream_host.py (their
leaf boxes through tests/native/sweep_stream_check.cpp) and tests/test_sweep_stream.py (their frames on the GPU).

A body of the sweep reads the first 32 bytes of whichever record comes next, so what can go wrong is a TRANSITION: the last body of
one class fetching the first record of the next.  The sweep has 20 classes in table order — 0 .. 11 PAIR2_u(fb, fc) as
4 u + fb + 2 fc, 12 .. 14 SHARE_FLAT_x y z, 15 .. 17 SHARE_x y z, 18 the general pair, 19 the single — each class a loop body of
its own in the kernel.  TRANSITIONS holds one scene for every ordered pair a < b of them, 190 scenes, with ONE record of each of
the two classes and nothing else: a's body starts the stream's second read, b's body works on it.

A scene sweeps only with an internal tree (16 primitives and more), so a group is several different triangles with one and the
same box (4 of them, 6 where the scene has three groups).  The two records stand far apart, one in front of each of the two
views, and `interleaved_tree` gives the scene a caller's tree that is poor by construction, so scene creation keeps its own."""
import ctypes as C
import itertools

import numpy as np
from sweep_families_cases import LIGHT
from sweep_pairs_cases import _uniq

from pathtracer_cuda_interactive_amd import PT_MAT_DIFFUSE, HostScene

F = np.float32
EYE = (0.13, 0.07, 0.21)
DIAGONAL = (1.0, 0.9, 1.1)
REACH = 1.6                                   # the records stand at EYE +- REACH * DIAGONAL, boxes of about 0.5 .. 0.9
N_CLASSES, GENERAL, SINGLE = 20, 18, 19
MODEL = [27 - 2 * ((c & 1) + ((c >> 1) & 1)) for c in range(12)] + [29] * 3 + [31] * 3 + [35, 17]

CORNERS = np.array(list(itertools.product((0.0, 1.0), repeat=3)), F)
# corner triples that touch all six faces of a box: their triangle's box is the box
FULL_BOX = [t for t in itertools.combinations(range(8), 3)
            if all(CORNERS[list(t), a].min() == 0.0 and CORNERS[list(t), a].max() == 1.0 for a in range(3))]


def class_name(c):
    if c < 12:
        return "pair2_" + "xyz"[c // 4] + ("", "_flat_b", "_flat_c", "_flat_flat")[c % 4]
    return ("flat_x", "flat_y", "flat_z", "share_x", "share_y", "share_z", "general", "single")[c - 12]


def _group(hs, mat, lo, hi, count, radiance=None):
    """One group: `count` different triangles that all have the box lo .. hi (float32, used bit for bit).  A box flat on one axis
    is a rectangle: two neighbouring corners and a point on the opposite edge.  Flat on two: a segment, triangles without area."""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    flat = [a for a in range(3) if lo[a] == hi[a]]
    if len(flat) == 0:
        P = (lo + CORNERS * (hi - lo)).astype(F)
        P[CORNERS == 0.0] = np.broadcast_to(lo, P.shape)[CORNERS == 0.0]
        P[CORNERS == 1.0] = np.broadcast_to(hi, P.shape)[CORNERS == 1.0]
        idx = np.array([FULL_BOX[(3 * j) % len(FULL_BOX)] for j in range(count)], np.int32)
    elif len(flat) == 1:
        p, q = [a for a in range(3) if a != flat[0]]
        ring = [(lo[p], lo[q]), (hi[p], lo[q]), (hi[p], hi[q]), (lo[p], hi[q])]
        P = np.zeros((3 * count, 3), F)
        P[:, flat[0]] = lo[flat[0]]                                   # keeps its bits: -0.0 stays -0.0
        for j in range(count):
            i, t = j % 4, F(0.3) if j < 4 else F(0.7)
            a, b, c, d = (ring[(i + k) % 4] for k in range(4))
            third = (c[0] + (d[0] - c[0]) * t, c[1] + (d[1] - c[1]) * t)
            for k, pt in enumerate((a, b, third)):
                P[3 * j + k, p], P[3 * j + k, q] = pt
        idx = np.arange(3 * count, dtype=np.int32).reshape(count, 3)
    else:
        g = [a for a in range(3) if a not in flat][0]
        P = np.zeros((3 * count, 3), F)
        P[:] = lo
        for j in range(count):
            P[3 * j + 1, g] = hi[g]
            P[3 * j + 2, g] = lo[g] + (hi[g] - lo[g]) * F((j + 1) / (count + 1))
        idx = np.arange(3 * count, dtype=np.int32).reshape(count, 3)
    hs.add_mesh(P, idx, mat, radiance=radiance)


def record_boxes(cls, centre, k):
    """The boxes (lo, hi) of one record of class `cls` around `centre`: two, or one for the single.  Every bound that is not shared
    on purpose carries an offset of its own (k: the record's number in the scene)."""
    u = lambda i: _uniq(17 * k + i)
    c = centre
    if cls < 12:
        ax, fl = cls // 4, cls % 4
        b, cc = [a for a in range(3) if a != ax]
        lo, hi = [0.0] * 3, [0.0] * 3
        lo[b] = c[b] - 0.4 - u(0)
        hi[b] = lo[b] if fl & 1 else c[b] + 0.4 + u(1)
        lo[cc] = c[cc] - 0.35 - u(2)
        hi[cc] = lo[cc] if fl & 2 else c[cc] + 0.35 + u(3)
        out = []
        for side in range(2):
            lo[ax] = c[ax] + (-0.5 - u(4) if side == 0 else 0.05 + u(5))
            hi[ax] = c[ax] + (-0.06 + u(6) if side == 0 else 0.45 + u(7))
            out.append((list(lo), list(hi)))
        return out
    if cls < GENERAL:
        ax, flat = (cls - 12) % 3, cls < 15
        out = []
        for side in range(2):
            lo = [c[x] - 0.4 - u(side + 3 * x) + 0.45 * side * (x != ax) - 0.2 * (x != ax) for x in range(3)]
            hi = [c[x] + 0.3 + u(8 + side + 3 * x) + 0.45 * side * (x != ax) - 0.2 * (x != ax) for x in range(3)]
            lo[ax] = c[ax] - 0.4 - u(15)
            hi[ax] = lo[ax] if flat else c[ax] + 0.4 + u(16)
            out.append((lo, hi))
        return out
    out = []
    for side in range(2 if cls == GENERAL else 1):
        lo = [c[x] - 0.45 - u(side + 3 * x) + 0.4 * side for x in range(3)]
        hi = [c[x] + 0.05 + u(8 + side + 3 * x) + 0.4 * side for x in range(3)]
        out.append((lo, hi))
    return out


def transition(a, b):
    """(constructor, groups, triangles per group, info of the launch) of the scene with one record of class a in front of view 0
    and one of class b in front of view 1."""
    assert 0 <= a < b < N_CLASSES and a != SINGLE
    groups = 2 + (1 if b == SINGLE else 2)
    per = 4 if groups == 4 else 6

    def make():
        hs = HostScene()
        hs.set_camera(EYE, tuple(EYE[x] + DIAGONAL[x] for x in range(3)), (0, 1, 0), 135.0, 16, 16, 4)
        hs.set_background((0.4, 0.5, 0.6))
        mats = [hs.add_material(PT_MAT_DIFFUSE, (0.75, 0.6 - 0.05 * k, 0.25 + 0.06 * k)) for k in range(4)]
        n = 0
        for k, cls in enumerate((a, b)):
            side = 1.0 if k == 0 else -1.0
            centre = [EYE[x] + side * REACH * DIAGONAL[x] for x in range(3)]
            for lo, hi in record_boxes(cls, centre, k):
                _group(hs, mats[n % 4], lo, hi, per, radiance=LIGHT if n == 0 else None)
                n += 1
        return hs

    info = {"sweep_valu_model": MODEL[a] + MODEL[b], "sweep_pair2_records": int(a < 12) + int(b < 12),
            "sweep_general_pairs": int(a == GENERAL) + int(b == GENERAL)}
    return make, groups, per, info


TRANSITIONS = {f"{class_name(a)}__{class_name(b)}": (a, b) + transition(a, b)
               for a in range(N_CLASSES - 1) for b in range(a + 1, N_CLASSES)}
# neither record has a triangle with an area: every ray misses, no path goes on behind its camera segment
NOTHING_TO_HIT = {(a, b) for a in (3, 7, 11) for b in (3, 7, 11)}


def interleaved_tree(d, groups, per):
    """A copy of `d` whose caller's tree is poor by construction: the leaves in the order group 0, 1, .., group 0, 1, .. (the
    primitives were added group by group, `per` each) and paired up in that order, so every node above two leaves joins different
    groups and every node above four spans both records.  Valid and nested: every box is the union of its children's."""
    from pathtracer_cuda_interactive_amd import device as dev
    from pathtracer_cuda_interactive_amd.ctypes_defs import PtBvhNode, PtSceneDesc
    src = np.frombuffer((C.c_char * (d.num_nodes * dev.NODE_DTYPE.itemsize)).from_address(C.addressof(d.nodes.contents)),
                        dtype=dev.NODE_DTYPE)
    leaves = src[src["prim"] >= 0].copy()
    assert len(leaves) == d.num_shapes == groups * per
    leaves = leaves[np.argsort(leaves["prim"], kind="stable")]
    leaves = leaves[[g * per + j for j in range(per) for g in range(groups)]]
    out = []

    def build(lo, hi):                                 # post-order: the root is the last node
        if hi - lo == 1:
            out.append(leaves[lo])
            return len(out) - 1
        mid = (lo + hi) // 2
        l, r = build(lo, mid), build(mid, hi)
        node = np.zeros(1, dev.NODE_DTYPE)[0]
        node["bmin"] = np.minimum(out[l]["bmin"], out[r]["bmin"])
        node["bmax"] = np.maximum(out[l]["bmax"], out[r]["bmax"])
        node["left"], node["right"], node["prim"] = l, r, -1
        out.append(node)
        return len(out) - 1

    root = build(0, len(leaves))
    nodes = np.array(out, dtype=dev.NODE_DTYPE)
    d2 = PtSceneDesc()
    C.memmove(C.byref(d2), C.byref(d), C.sizeof(PtSceneDesc))
    d2.nodes = nodes.ctypes.data_as(C.POINTER(PtBvhNode))
    d2.num_nodes, d2.root = len(nodes), root
    d2._keep = (nodes, d)
    return d2


# two views from inside the scene, along a space diagonal and back, wide enough that their camera rays cover all eight octants
VIEWS = [(DIAGONAL, 135.0), (tuple(-x for x in DIAGONAL), 135.0)]


def view_params(k, width=16, height=16, spp=4, seed=70):
    """Render parameters of view k: a camera of its own, so the scene's description stays as finalized."""
    look, fov = VIEWS[k]
    cam = HostScene()
    cam.set_camera(EYE, tuple(EYE[a] + look[a] for a in range(3)), (0, 1, 0), fov, width, height, spp)
    return cam.render_params(width, height, spp, seed=seed + k)


def camera_ray_octants(p):
    """How many pixels of the frame have their CENTRE ray in each octant (bit a set: the direction's component a is negative, as
    the kernel takes it from the sign bits): [8] counts.  An approximation of the rays the renderers trace — they jitter the
    camera ray inside its pixel, and bounce rays come on top — which the oracle does not hand out; so the tests ask for several
    pixels per octant, not one."""
    u = (np.arange(p.width, dtype=F) + F(0.5)) / F(p.width)
    v = (np.arange(p.height, dtype=F) + F(0.5)) / F(p.height)
    tl, hz, vt, og = (np.array(list(a), dtype=F) for a in (p.cam_top_left, p.cam_horizontal, p.cam_vertical, p.cam_origin))
    d = ((tl + hz * u[None, :, None]) - vt * v[:, None, None]) - og
    neg = np.signbit(d)
    return np.bincount((neg[..., 0] * 1 + neg[..., 1] * 2 + neg[..., 2] * 4).reshape(-1), minlength=8)


def octants_of_the_views():
    return sum(camera_ray_octants(view_params(k)) for k in range(len(VIEWS)))
