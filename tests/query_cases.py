"""Ray makers for tests/test_query_states.py, in plain numpy (no GPU): rays of deliberately uneven cost for the query kernel's
hand-out, rays aimed at the shapes of a scene that random rays rarely meet, and rays whose interval ends sit on a hit.

Every maker is deterministic; the tests make each set once, share it and leave it unchanged."""
import numpy as np
from scene_update_cases import centroids, scene_rays, shape_table
from test_trace_rays import random_rays

from pathtracer_cuda_interactive_amd import PT_SHAPE_SPHERE
from pathtracer_cuda_interactive_amd.standins import mesh_arrays

F = np.float32
TFAR = F(3.0e38)


def root_box(d):
    """(lo, hi) of the caller's root node, float64."""
    root = d.nodes[d.root]
    return np.array(root.bmin[:], np.float64), np.array(root.bmax[:], np.float64)


def cheap_rays(d, n, seed):
    """Rays that start outside the scene's box and point away from it: they fail the root's slab test and cost one node."""
    rng = np.random.default_rng(seed)
    lo, hi = root_box(d)
    centre, half = 0.5 * (lo + hi), 0.5 * np.maximum(hi - lo, 1e-3)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = centre + u * (np.linalg.norm(half) * (1.5 + rng.random((n, 1))))
    rays = np.zeros((n, 8), F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = o, u, 1e-4, TFAR
    return rays


def long_rays(d, n, seed):
    """Rays from a corner region of the scene's box through its middle: they cross the whole scene."""
    rng = np.random.default_rng(seed)
    lo, hi = root_box(d)
    o = lo + (hi - lo) * 0.1 * rng.random((n, 3))
    u = 0.5 * (lo + hi) + (hi - lo) * 0.2 * (rng.random((n, 3)) - 0.5) - o
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rays = np.zeros((n, 8), F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = o, u, 1e-4, TFAR
    return rays


def uneven_rays(d, n=20000):
    """random_rays() interleaved index by index with cheap_rays(): odd indices random (its rays with a zero direction
    component sit there), even indices cheap.  Two odd indices of every aligned block of 64 are set apart: 33 is cheap as
    well, so that 33 of a block's 64 rays cost one node and the block's median is that cost whatever its random rays do; 17 is
    one of long_rays(), so that no block is cheap throughout on a scene the random rays mostly miss."""
    rays = random_rays(n).copy()
    cheap = cheap_rays(d, n, 23)
    k = np.arange(n)
    sel = (k % 2 == 0) | (k % 64 == 33)
    rays[sel] = cheap[sel]
    sel = k % 64 == 17
    rays[sel] = long_rays(d, n, 29)[sel]
    return rays


def block_spread(visits, block=64):
    """Per aligned block of `block` consecutive rays (the last, partial one included): (largest, median) node visits."""
    out = []
    for b in range(0, len(visits), block):
        v = visits[b:b + block].astype(np.float64)
        out.append((v.max(), np.median(v)))
    return np.array(out)


def aimed_rays(d, n, seed):
    """scene_rays() for the even indices; the odd ones start in the same places and are aimed at points on the shapes: the
    centroid of a shape chosen in turn, jittered by a fraction (a quarter, Gaussian) of that shape's extent."""
    rays = scene_rays(n, seed).copy()
    rng = np.random.default_rng(seed + 1000)
    shp = shape_table(d)
    c = centroids(d)
    ext = np.where(shp["type"] == PT_SHAPE_SPHERE, 2.0 * shp["radius"], 0.0).astype(np.float64)
    for m in range(d.num_meshes):
        P, I, _ = mesh_arrays(d, m)
        sel = np.flatnonzero((shp["type"] != PT_SHAPE_SPHERE) & (shp["mesh_index"] == m))
        tri = P[I[shp["face_index"][sel]]].astype(np.float64)
        ext[sel] = (tri.max(axis=1) - tri.min(axis=1)).max(axis=1)
    odd = np.arange(1, n, 2)
    shape = (odd // 2) % d.num_shapes
    target = c[shape] + rng.standard_normal((len(odd), 3)) * 0.25 * ext[shape, None]
    dirs = target - rays[odd, 0:3].astype(np.float64)
    dirs /= np.maximum(np.linalg.norm(dirs, axis=1, keepdims=True), 1e-20)
    rays[odd, 3:6] = dirs
    return rays


def interval_end_rays(rays, tuv, prim):
    """name -> copies of the hitting rays of `rays` with one end of the interval on the oracle's t or one float beside it."""
    hit = prim >= 0
    base, t = rays[hit], tuv[hit, 0].astype(F)
    out = {}
    for name, col, value in (("tfar_at_t", 7, t), ("tfar_above_t", 7, np.nextafter(t, F(np.inf))), ("tnear_at_t", 6, t),
                             ("tnear_below_t", 6, np.nextafter(t, F(-np.inf)))):
        r = base.copy()
        r[:, col] = value
        out[name] = r
    return out


def odd_interval_rays(d, rays, tuv, prim):
    """name -> rays: an empty interval (tnear > tfar around the hit, tnear == tfar on it and beside it), tnear = -1 from origins
    inside the scene's box, and the direction alone scaled by 1e-3 and 1e3 under tfar = 3e38."""
    hit = prim >= 0
    base, t = rays[hit], tuv[hit, 0].astype(F)
    out = {}
    r = base.copy()
    r[:, 6], r[:, 7] = t * F(1.5), t * F(0.5)
    out["tnear_above_tfar"] = r
    r = base.copy()
    r[:, 6] = r[:, 7] = t
    r[1::2, 6] = r[1::2, 7] = t[1::2] * F(0.5)
    out["tnear_is_tfar"] = r
    rng = np.random.default_rng(31)
    lo, hi = root_box(d)
    n = len(rays)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = np.zeros((n, 8), F)
    r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7] = lo + (hi - lo) * (0.1 + 0.8 * rng.random((n, 3))), u, -1.0, TFAR
    out["tnear_minus_one_inside"] = r
    for name, f in (("dir_by_1e-3", 1e-3), ("dir_by_1e3", 1e3)):
        r = rays.copy()
        r[:, 3:6] *= F(f)
        r[:, 7] = TFAR
        out[name] = r
    return out
