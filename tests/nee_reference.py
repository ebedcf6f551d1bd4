"""A plain fp64 direct-light integrator (numpy only) — the independent reference for PT_RENDER_NEE at max_depth = 1.

It shares nothing with the code under test but the scene description it reads and the four camera vectors: its own ray/sphere
and ray/triangle tests, its own BRDF values, its own visibility.  Per pixel it returns the mean over an S x S midpoint grid of
sub-pixel positions of

    miss            background
    hit at x, wi    Le(hit primitive) if it is a diffuse area light and dot(wi, n_shading) > 0
                    + sum over lights[] (n = shading normal turned towards wi):
                        point light      value(wi, wl) I / d^2  V
                        area light on P  integral over P of value(wi, wl(y)) Le [dot(-wl, n_s(y)) > 0] |dot(wl, n_g)| / d^2 V(x, y) dA(y)

    value           DIFFUSE rho max(n.wl, 0)/pi;  PLASTIC (1 - F(n.wi)) rho max(n.wl, 0)/pi, Schlick F from ((eta-1)/(eta+1))^2;
                    PHONG rho (e+1)/(2 pi) (r.wl)^e where r.wl > 0 and n.wl > 0 (no extra cosine);  MIRROR 0
    V(x, y)         1 iff no primitive but the emitter is hit at a parameter s of x + s (y - x) in (EPS, 1 - EPS), EPS = 1e-7:
                    an interval of this file's own, relative to the segment, wide enough for fp64 and far below any gap in a
                    scene of the tests (the estimator's own interval is absolute at the near end and 1e-4 relative at the far end)

Area integrals are equal-area midpoint rules: z x phi on a sphere, a uniform barycentric subdivision on a triangle.  Everything is
evaluated at two resolutions, the second doubling S and the light grids: the result is (T_fine, |T_fine - T_coarse|)."""
import numpy as np

SPHERE, TRIANGLE = 0, 1
DIFFUSE, MIRROR, PLASTIC, PHONG = 0, 1, 2, 3
POINT, AREA = 0, 1
EPS = 1e-7
PAIRS = 1 << 18           # point-light-sample pairs per numpy batch


def _f3(a):
    return np.array([a[0], a[1], a[2]], dtype=np.float64)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


class Scene:
    """The primitives, materials and lights of a pt_scene_desc as fp64 numpy values (the BVH is not read)."""

    def __init__(self, desc):
        self.background = _f3(desc.background)
        self.materials = [(m.type, _f3(m.reflectance), float(m.eta), float(m.exponent))
                          for m in (desc.materials[i] for i in range(desc.num_materials))]
        self.lights = []
        for i in range(desc.num_lights):
            l = desc.lights[i]
            self.lights.append((POINT, _f3(l.position), _f3(l.radiance)) if l.type == POINT else (AREA, int(l.shape_id), _f3(l.radiance)))
        self.prims = []
        for i in range(desc.num_shapes):
            s = desc.shapes[i]
            if s.type == SPHERE:
                lid, mat = s.area_light_id, s.material_id
                geo = (_f3(s.center), float(s.radius))
            else:
                m = desc.meshes[s.mesh_index]
                lid, mat = m.area_light_id, m.material_id
                idx = [m.indices[3 * s.face_index + k] for k in range(3)]
                P = np.array([[m.positions[3 * v + c] for c in range(3)] for v in idx], dtype=np.float64)
                N = np.array([[m.normals[3 * v + c] for c in range(3)] for v in idx], dtype=np.float64)
                geo = (P, N)
            le = None
            if 0 <= lid < desc.num_lights and desc.lights[lid].type == AREA:
                le = _f3(desc.lights[lid].radiance)
            self.prims.append((int(s.type), geo, int(mat), le))


def _sphere_roots(geo, o, d):
    """Both parameters s of o + s d on the sphere (nan where the line misses it); d need not be a unit vector."""
    c, r = geo
    oc = o - c
    a = (d * d).sum(-1)
    b = (oc * d).sum(-1)
    disc = b * b - a * ((oc * oc).sum(-1) - r * r)
    with np.errstate(invalid="ignore"):
        q = np.sqrt(disc)
    return (-b - q) / a, (-b + q) / a


def _triangle_param(geo, o, d):
    """Parameter s of o + s d in the triangle and its barycentrics (s = nan on a miss)."""
    P, _ = geo
    e1, e2 = P[1] - P[0], P[2] - P[0]
    pv = np.cross(d, e2)
    det = (pv * e1).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        tv = o - P[0]
        u = (tv * pv).sum(-1) * inv
        qv = np.cross(tv, e1)
        v = (d * qv).sum(-1) * inv
        s = (qv * e2).sum(-1) * inv
    ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
    return np.where(ok, s, np.nan), u, v


def closest_hit(sc, o, d):
    """(prim [N] or -1, s [N]) of the closest primitive along o + s d, s > EPS."""
    best = np.full(o.shape[0], np.inf)
    prim = np.full(o.shape[0], -1)
    for k, (kind, geo, _, _) in enumerate(sc.prims):
        if kind == SPHERE:
            s0, s1 = _sphere_roots(geo, o, d)
            s = np.where(s0 > EPS, s0, s1)
        else:
            s = _triangle_param(geo, o, d)[0]
        with np.errstate(invalid="ignore"):
            take = (s > EPS) & (s < best)
        best = np.where(take, s, best)
        prim = np.where(take, k, prim)
    return prim, best


def visible(sc, x, dv, skip):
    """V for the segments x + s dv, s in (EPS, 1 - EPS): x [n, 1, 3], dv [n, M, 3]; primitive `skip` (the emitter) is left out."""
    vis = np.ones(dv.shape[:2], dtype=bool)
    for k, (kind, geo, _, _) in enumerate(sc.prims):
        if k == skip:
            continue
        with np.errstate(invalid="ignore"):
            if kind == SPHERE:
                s0, s1 = _sphere_roots(geo, x, dv)
                vis &= ~(((s0 > EPS) & (s0 < 1 - EPS)) | ((s1 > EPS) & (s1 < 1 - EPS)))
            else:
                s = _triangle_param(geo, x, dv)[0]
                vis &= ~((s > EPS) & (s < 1 - EPS))
    return vis


def light_points(sc, prim, n):
    """Equal-area midpoint rule on an emitter: (y [M, 3], shading normal [M, 3], geometric normal [M, 3], dA)."""
    kind, geo, _, _ = sc.prims[prim]
    if kind == SPHERE:
        c, r = geo
        z = 1 - 2 * (np.arange(n) + 0.5) / n
        ph = 2 * np.pi * (np.arange(2 * n) + 0.5) / (2 * n)
        Z, PH = np.meshgrid(z, ph, indexing="ij")
        s = np.sqrt(1 - Z * Z)
        nx = np.stack([s * np.cos(PH), s * np.sin(PH), Z], -1).reshape(-1, 3)
        return c + r * nx, nx, nx, 4 * np.pi * r * r / nx.shape[0]
    P, N = geo
    pts = []
    for i in range(n):                      # n^2 congruent triangles: upright ones at (i, j), inverted ones between them
        for j in range(n - i):
            pts.append(((i + 1 / 3) / n, (j + 1 / 3) / n))
            if j < n - i - 1:
                pts.append(((i + 2 / 3) / n, (j + 2 / 3) / n))
    uv = np.array(pts)
    w = np.stack([1 - uv[:, 0] - uv[:, 1], uv[:, 0], uv[:, 1]], -1)
    cr = np.cross(P[1] - P[0], P[2] - P[0])
    area = 0.5 * np.linalg.norm(cr)
    ng = np.broadcast_to(cr / (2 * area), (w.shape[0], 3))
    return w @ P, _unit(w @ N), ng, area / w.shape[0]


def brdf_value(mat, n, wi, wl):
    """The scalar part of `value` (reflectance left out): n, wi [n, 1, 3], wl [n, M, 3] -> [n, M]."""
    kind, _, eta, e = mat
    cs = np.maximum((n * wl).sum(-1), 0.0)
    if kind == DIFFUSE:
        return cs / np.pi
    if kind == PLASTIC:
        f0 = ((eta - 1) / (eta + 1)) ** 2
        F = f0 + (1 - f0) * (1 - (n * wi).sum(-1)) ** 5
        return (1 - F) * cs / np.pi
    if kind == PHONG:
        r = 2 * (n * wi).sum(-1, keepdims=True) * n - wi
        rd = np.maximum((r * wl).sum(-1), 0.0)
        return np.where(cs > 0, (e + 1) / (2 * np.pi) * rd ** e, 0.0)
    return np.zeros(wl.shape[:2])


def radiance(sc, o, d, n_light):
    """Direct illumination along the rays o + s d: (L [N, 3], prim [N])."""
    prim, s = closest_hit(sc, o, d)
    L = np.where((prim < 0)[:, None], sc.background, 0.0)
    grids = {}
    for k in np.unique(prim[prim >= 0]):
        sel = np.nonzero(prim == k)[0]
        kind, geo, mat_id, le = sc.prims[k]
        mat = sc.materials[mat_id]
        x = o[sel] + d[sel] * s[sel, None]
        wi = -_unit(d[sel])
        if kind == SPHERE:
            n = (x - geo[0]) / geo[1]
        else:
            _, u, v = _triangle_param(geo, o[sel], d[sel])
            n = _unit(np.stack([1 - u - v, u, v], -1) @ geo[1])
        front = (wi * n).sum(-1) > 0
        out = np.zeros((sel.size, 3))
        if le is not None:
            out += np.where(front[:, None], le, 0.0)
        n = np.where(front[:, None], n, -n)
        if mat[0] != MIRROR:
            for light in sc.lights:
                if light[0] == POINT:
                    y, ns, ng, dA, skip = light[1][None], None, None, 1.0, -1
                else:
                    if light[1] not in grids:
                        grids[light[1]] = light_points(sc, light[1], n_light)
                    (y, ns, ng, dA), skip = grids[light[1]], light[1]
                    le_seen = sc.prims[skip][3]
                    if le_seen is None or (le_seen != light[2]).any():
                        raise ValueError("lights[] and the emitter's own light id disagree about its radiance")
                step = max(1, PAIRS // y.shape[0])
                for a in range(0, sel.size, step):
                    xs, ws, nn = x[a:a + step, None], wi[a:a + step, None], n[a:a + step, None]
                    dv = y[None] - xs
                    d2 = (dv * dv).sum(-1)
                    wl = dv / np.sqrt(d2)[..., None]
                    g = brdf_value(mat, nn, ws, wl) / d2
                    if ns is not None:
                        g = g * ((-(wl * ns[None]).sum(-1)) > 0) * np.abs((wl * ng[None]).sum(-1)) * dA
                    rows, cols = np.nonzero(g > 0)                      # visibility only where there is something to hide
                    g[rows, cols] *= visible(sc, xs[rows], dv[rows, cols][:, None], skip)[:, 0]
                    out[a:a + step] += mat[1] * light[2] * g.sum(-1)[:, None]
        L[sel] = out
    return L, prim


def camera_rays(cam, W, H, fx, fy, rows=None):
    """Rays through the film positions (i + fx, j + fy) of every pixel (of the listed rows): fx, fy [Q] -> o, d [rows * W * Q, 3]."""
    og, tl, hz, vt = np.asarray(cam, dtype=np.float64)
    jj, ii = np.meshgrid(np.arange(H) if rows is None else np.asarray(rows), np.arange(W), indexing="ij")
    u = (ii[..., None] + fx) / W
    v = (jj[..., None] + fy) / H
    d = tl + hz * u[..., None] - vt * v[..., None] - og
    return np.broadcast_to(og, d.shape).reshape(-1, 3), d.reshape(-1, 3)


def _frame(sc, cam, W, H, S, n_light, rows):
    sub = (np.arange(S) + 0.5) / S
    fy, fx = [a.ravel() for a in np.meshgrid(sub, sub, indexing="ij")]
    o, d = camera_rays(cam, W, H, fx, fy, rows)
    L, prim = radiance(sc, o, d, n_light)
    return L.reshape(-1, W, S * S, 3), prim.reshape(-1, W, S * S)


def direct_light(desc, cam, W, H, S=2, n_light=16, corner_light=False, rows=None):
    """(T_fine [H, W, 3], |T_fine - T_coarse| [H, W, 3], prim [H, W], dark [H, W], lit [H, W]): prim is the one primitive
    (-1: the background) that every sub-sample of the fine grid and the four corners of the pixel see, or -2 where they see more
    than one.  dark / lit: the radiance is zero / positive at every sub-sample, and with corner_light at the four corners too.
    With `rows`, only those rows of the frame."""
    sc = Scene(desc)
    coarse, _ = _frame(sc, cam, W, H, S, n_light, rows)
    fine, prim = _frame(sc, cam, W, H, 2 * S, 2 * n_light, rows)
    o, d = camera_rays(cam, W, H, np.array([0.0, 1.0, 0.0, 1.0]), np.array([0.0, 0.0, 1.0, 1.0]), rows)
    if corner_light:
        Lc, corner = radiance(sc, o, d, 2 * n_light)
        lum = np.concatenate([fine.max(-1), Lc.reshape(-1, W, 4, 3).max(-1)], axis=-1)
    else:
        corner, lum = closest_hit(sc, o, d)[0], fine.max(-1)
    seen = np.concatenate([prim, corner.reshape(-1, W, 4)], axis=-1)
    one = (seen == seen[..., :1]).all(-1)
    T = fine.mean(2)
    return T, np.abs(T - coarse.mean(2)), np.where(one, seen[..., 0], -2), (lum == 0).all(-1), (lum > 0).all(-1)


def t_quantile(dof, p):
    """c with P(|t_dof| > c) = p, by Simpson's rule on the t density and bisection."""
    import math
    k = math.exp(math.lgamma((dof + 1) / 2) - math.lgamma(dof / 2)) / math.sqrt(dof * math.pi)

    def inside(c, n=20000):
        t = np.linspace(0.0, c, n + 1)
        f = k * (1 + t * t / dof) ** (-(dof + 1) / 2)
        return 2 * (c / n) / 3 * (f[0] + f[-1] + 4 * f[1:-1:2].sum() + 2 * f[2:-1:2].sum())

    lo, hi = 0.0, 100.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if 1 - inside(mid) > p else (lo, mid)
    return 0.5 * (lo + hi)
