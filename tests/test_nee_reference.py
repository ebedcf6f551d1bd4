"""PT_RENDER_NEE against something that is not its own restatement ("What pins the light sample").

Direct-light cases: with max_depth = 1 a frame is emission at the camera hit plus one light sample, which tests/nee_reference.py
integrates by fp64 quadrature (T_fine, and |T_fine - T_coarse| as its own error).  Expectation cases: on a scene without specular
lobes and with a black background, NEE at max_depth = k and the plain estimator at k + 1 gather the same light.

Every statistical comparison is of K = 32 frames: mean and SE = std(ddof = 1) / sqrt(K) per pixel (direct light) or per 4 x 4 block
(expectation), and for the image mean.  The K seeds are fixed 62-bit numbers drawn once from numpy's generator, NOT s0 .. s0 + K - 1:
frames whose seeds differ by little are not independent (init_pcg32 adds the seed to the state one step before the first draw, so
the sub-pixel jitter of neighbouring seeds is a lattice), and under a point light, where that jitter is all the noise there is, K
consecutive seeds put the root-mean-square of (mean - T) / SE at 5.1 where independent frames give 1 (measured 0.89 with these seeds).

    direct light   |mean - T_fine| <= c SE + 2 |T_fine - T_coarse|, on the pixels whose sub-samples and corners see ONE primitive and
                   where |T_fine - T_coarse| <= c SE / 10; at least 80 % of a case's pixels must be such pixels
    expectation    |mean_A - mean_B| <= c sqrt(SE_A^2 + SE_B^2)

c is the two-sided Student-t quantile at K - 1 degrees of freedom for the level 0.01 / M, M the number of scalar comparisons this
file makes at that K (every channel of every pixel or block and of every image mean, CPU and device tests together, counted by
_count_comparisons from the case tables below):

    K = 32    M = 25848    c = 6.4076   (test_the_constants_in_this_docstring keeps this line true)

Seeds are fixed: c sets how small a defect is seen, not how often a test fails.  The mutation tests (oracle/pt_oracle.h, bits 16
upward) show that each named case does fail for the defect it is there for."""
import functools
import os

import numpy as np
import pytest
from conftest import GOLDEN, assert_bit_equal, bits

import nee_reference as nr
from pathtracer_cuda_interactive_amd import (PT_ERR_UNSUPPORTED, PT_MAT_DIFFUSE, PT_MAT_MIRROR, PT_MAT_PHONG, PT_MAT_PLASTIC,
                                             PT_RENDER_NEE, HostScene, PtError, camera_ray_data)

K = 32
SEEDS = [int(x) for x in np.random.default_rng(7000).integers(0, 1 << 62, 2 * K)]     # K for NEE, K for the plain estimator
GPU_SPP_FACTOR = 16          # device frames take 16 x the samples of the CPU frames
RHO = (0.6, 0.5, 0.4)
MATERIALS = {"diffuse": (PT_MAT_DIFFUSE, {}), "phong": (PT_MAT_PHONG, {"exponent": 10.0}), "plastic": (PT_MAT_PLASTIC, {"eta": 1.5})}
MUT_NO_NUM_LIGHTS, MUT_COS_SHADING, MUT_NO_LOBE_WEIGHT, MUT_BOTH_SIDES, MUT_COUNT_EMISSION, MUT_TFAR_FULL = 16, 32, 64, 128, 256, 512


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
# The receiver is the plane y = 0 seen from (0, +-3, 0) straight on: the frame shows |x|, |z| < 1.09 of it.  Its two triangles meet
# on x + z = 80, far outside the frame, so that no pixel straddles them.
# Point lights are added after every emitter: lights[] lists them last, and an emitter's own light id counts in the order of
# addition (the reference's quirk, SURVEY H5c, which both estimators keep), so only then do the two name the same radiance.

def _base(material="diffuse", below=False):
    hs = HostScene()
    hs.set_camera((0, -3 if below else 3, 0.001), (0, 0, 0), (0, 1, 0), 40.0, 16, 16, 1)
    hs.set_background((0, 0, 0))
    mtype, kw = MATERIALS[material]
    m = hs.add_material(mtype, RHO, **kw)
    P = np.float32([[-10, 0, -10], [90, 0, -10], [90, 0, 90], [-10, 0, 90]])
    hs.add_mesh(P, np.int32([[0, 3, 1], [1, 3, 2]]), m, normals=np.float32([[0, 1, 0]] * 4))
    return hs, hs.add_material(PT_MAT_DIFFUSE, (0, 0, 0))


POINT = ((0.5, 2.0, -0.25), (30.0, 20.0, 10.0))
SPHERE = ((2.5, 1.2, -0.25), 0.6, (3.0, 2.0, 1.0))
# a triangle beside the frame, sloping down and away: the side with the normal (-1, -1, 0) / sqrt 2 looks at the visible plane
TRI = np.float32([[1.4, 1.8, 0.6], [1.4, 1.8, -0.6], [2.4, 0.8, 0.0]])
TRI_N = np.float32([-1, -1, 0]) / np.sqrt(np.float32(2))
TRI_LE = (9.0, 12.0, 15.0)


def _rotated(n, axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    t = np.radians(deg)
    n = np.asarray(n, dtype=np.float64)
    return (n * np.cos(t) + np.cross(a, n) * np.sin(t) + a * a.dot(n) * (1 - np.cos(t))).astype(np.float32)


def _point(material):
    hs, _ = _base(material)
    hs.add_point_light(*POINT)
    return hs


def _sphere(material):
    hs, blk = _base(material)
    hs.add_sphere(SPHERE[0], SPHERE[1], blk, radiance=SPHERE[2])
    return hs


def _near_sphere():
    hs, blk = _base()
    hs.add_sphere((1.9, 0.72, 0.1), 0.6, blk, radiance=(3.0, 2.0, 1.0))          # lowest point 0.2 r above the plane
    return hs


def _triangle(normals):
    hs, blk = _base()
    hs.add_mesh(TRI, np.int32([[0, 1, 2]]), blk, normals=np.float32(normals), radiance=TRI_LE)
    return hs


def _tilted():
    return _triangle([_rotated(TRI_N, (0, 0, 1), 20), _rotated(TRI_N, (1, -1, 0), 35), _rotated(TRI_N, (1, -1, 1), -50)])


def _unequal_quad():
    hs, blk = _base("phong")
    o, eu, ev = np.float64([1.4, 1.8, 0.0]), np.float64([1.0, -1.0, 0.0]), np.float64([0.0, 0.0, 1.2])
    quad = [(0.0, -0.5), (-0.1, 0.0), (0.0, 0.5), (0.9, 0.0)]           # A, B, C, D: over the diagonal AC, heights 0.1 and 0.9
    P = np.float32([o + u * eu + v * ev for u, v in quad])
    hs.add_mesh(P, np.int32([[0, 1, 2], [0, 2, 3]]), blk, normals=np.float32([TRI_N] * 4), radiance=TRI_LE)
    return hs


def _three_kinds():
    hs, blk = _base("plastic")
    hs.add_sphere(SPHERE[0], SPHERE[1], blk, radiance=SPHERE[2])
    hs.add_mesh(TRI, np.int32([[0, 1, 2]]), blk, normals=np.float32([TRI_N] * 3), radiance=TRI_LE)
    hs.add_point_light((-0.4, 1.5, 0.5), (6.0, 9.0, 12.0))              # last: see _base
    return hs


OCCLUDER = ((1.8, 1.2, 0.0), 0.2)            # between the light at (3, 2, 0) and the middle of the frame, itself out of view


def _hard_shadow():
    hs, _ = _base()
    hs.add_point_light((3.0, 2.0, 0.0), (60.0, 40.0, 20.0))
    hs.add_sphere(OCCLUDER[0], OCCLUDER[1], hs.add_material(PT_MAT_DIFFUSE, (0.5, 0.5, 0.5)))
    return hs


def _penumbra():
    hs, blk = _base()
    hs.add_sphere((3.0, 2.0, 0.0), 0.3, blk, radiance=(30.0, 20.0, 10.0))
    hs.add_sphere(OCCLUDER[0], OCCLUDER[1], hs.add_material(PT_MAT_DIFFUSE, (0.5, 0.5, 0.5)))
    return hs


def _emitter_in_view():
    hs, blk = _base()
    hs.add_sphere((0.3, 0.8, -0.2), 0.45, blk, radiance=(3.0, 2.0, 1.0))
    return hs


def _back_face():
    hs, blk = _base(below=True)
    hs.add_sphere((2.5, -1.2, -0.25), 0.6, blk, radiance=SPHERE[2])
    hs.add_point_light((0.5, -2.0, -0.25), (30.0, 20.0, 10.0))
    return hs


# name -> (what it pins, builder, CPU spp, S and light grid of the coarse quadrature)
DIRECT = {
    "point-diffuse": ("nee_brdf of DIFFUSE, 1/d^2", lambda: _point("diffuse"), 256, 16, 1),
    "point-phong": ("nee_brdf of PHONG: no surface cosine in its value", lambda: _point("phong"), 256, 16, 1),
    "point-plastic": ("nee_brdf of PLASTIC: (1 - F) cancels against the lobe probability", lambda: _point("plastic"), 256, 16, 1),
    "sphere-diffuse": ("uniform sphere sampling, area -> solid angle", lambda: _sphere("diffuse"), 256, 1, 32),
    "sphere-phong": ("the same under a PHONG lobe", lambda: _sphere("phong"), 128, 8, 16),
    "sphere-plastic": ("the same under PLASTIC's diffuse lobe", lambda: _sphere("plastic"), 256, 1, 32),
    "near-sphere": ("the back half of a sphere light and grazing cosines", _near_sphere, 256, 1, 32),
    "triangle": ("uniform triangle sampling, area = |c| / 2", lambda: _triangle([TRI_N] * 3), 256, 2, 24),
    "tilted-normals": ("emitting side from the shading normal, cosine from the geometric one", _tilted, 256, 2, 24),
    "facing-away": ("an emitter that faces away lights nothing: all-zero bits", lambda: _triangle([-TRI_N] * 3), 64, 2, 16),
    "unequal-quad": ("one light per triangle, each weighted by its own area", _unequal_quad, 64, 8, 16),
    "three-kinds": ("the factor num_lights over lights of three kinds", _three_kinds, 256, 2, 32),
    "hard-shadow": ("the shadow ray of a point light: umbra all-zero bits, lit pixels the closed form", _hard_shadow, 256, 64, 1),
    "penumbra": ("V inside the area integral", _penumbra, 128, 1, 96),
    "emitter-in-view": ("emission at depth 0, no light sample through a black body", _emitter_in_view, 256, 2, 32),
    "back-face": ("the normal turned towards wi", _back_face, 256, 2, 32),
}
W = H = 16


def _expectation_scene(specular):
    hs = HostScene()
    hs.set_camera((0, 1.5, 5.0), (0, 0.6, 0), (0, 1, 0), 40.0, 32, 24, 1)
    hs.set_background((0, 0, 0))
    dif = hs.add_material(PT_MAT_DIFFUSE, (0.7, 0.6, 0.5))
    pho = hs.add_material(PT_MAT_PHONG, (0.6, 0.7, 0.5), exponent=8.0)
    pla = hs.add_material(PT_MAT_PLASTIC, (0.3, 0.5, 0.8), eta=1.5)
    mir = hs.add_material(PT_MAT_MIRROR, (0.9, 0.9, 0.9))
    blk = hs.add_material(PT_MAT_DIFFUSE, (0, 0, 0))
    P = np.float32([[-6, 0, -6], [6, 0, -6], [6, 0, 6], [-6, 0, 6]])
    hs.add_mesh(P, np.int32([[0, 2, 1], [0, 3, 2]]), dif, normals=np.float32([[0, 1, 0]] * 4))
    hs.add_sphere((-1.4, 0.6, 0), 0.6, pho)
    hs.add_sphere((0.0, 0.6, 0), 0.6, pla if specular else dif)
    hs.add_sphere((1.4, 0.6, 0), 0.6, mir if specular else pho)
    hs.add_sphere((0.5, 2.6, 0.5), 0.35, blk, radiance=(8.0, 6.0, 4.0))
    T = np.float32([[-2.5, 2.2, -1.0], [-1.5, 2.2, -1.0], [-2.0, 2.2, 0.0]])
    hs.add_mesh(T, np.int32([[0, 1, 2]]), blk, normals=np.float32([[0, -1, 0]] * 3), radiance=(5.0, 7.0, 9.0))
    return hs


def _mirror_scene():
    hs = HostScene()
    hs.set_camera((0, 3, 0.001), (0, 0, 0), (0, 1, 0), 40.0, 16, 16, 1)
    hs.set_background((0, 0, 0))
    mir = hs.add_material(PT_MAT_MIRROR, (0.9, 0.8, 0.7))
    P = np.float32([[-10, 0, -10], [90, 0, -10], [90, 0, 90], [-10, 0, 90]])
    hs.add_mesh(P, np.int32([[0, 3, 1], [1, 3, 2]]), mir, normals=np.float32([[0, 1, 0]] * 4))
    hs.add_sphere((0.5, 1.0, 0.3), 0.4, hs.add_material(PT_MAT_DIFFUSE, (0, 0, 0)), radiance=(3.0, 2.0, 1.0))
    return hs


# name -> (specular, NEE max_depth, plain max_depth, rr_depth, CPU spp)
EXPECTATION = {
    "depth-1": (0, 1, 2, 5, 256),
    "depth-2": (0, 2, 3, 5, 256),
    "depth-3": (0, 3, 4, 5, 256),
    "all-materials": (1, 50, 50, 5, 128),
}
EW, EH, BLOCK = 32, 24, 4


def _count_comparisons():
    direct = len(DIRECT) * (W * H * 3 + 3)
    expectation = len(EXPECTATION) * ((EW // BLOCK) * (EH // BLOCK) * 3 + 3)
    return 2 * (direct + expectation)                     # once on the oracle's frames, once on the device's


M = _count_comparisons()
C_T = nr.t_quantile(K - 1, 0.01 / M)


def test_the_constants_in_this_docstring():
    assert f"K = {K}    M = {M}    c = {C_T:.4f}" in __doc__
    # the quantile routine against values of the t table: two-sided 5 % at 10 and 1 % at 31 degrees of freedom, and the normal limit
    assert abs(nr.t_quantile(10, 0.05) - 2.228139) < 1e-5
    assert abs(nr.t_quantile(31, 0.01) - 2.744042) < 1e-5
    assert abs(nr.t_quantile(1e7, 0.05) - 1.959964) < 1e-5


# ---- shared, unchanged once made ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(name):
    hs = DIRECT[name][1]()
    return hs, hs.finalize()


def _compute_reference(name, rows=None):
    hs, d = _case(name)
    cam = camera_ray_data(hs.camera, W, H)
    return nr.direct_light(d, cam, W, H, S=DIRECT[name][3], n_light=DIRECT[name][4], corner_light=name == "hard-shadow", rows=rows)


RECORDED = os.path.join(GOLDEN, "nee_reference.npz")
FIELDS = ("T", "dT", "prim", "dark", "lit")


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(T_fine, |T_fine - T_coarse|, prim, dark, lit) of a direct-light case as recorded in tests/golden/nee_reference.npz: the fine
    quadratures take minutes together, so they are computed once (python tests/test_nee_reference.py writes the file) and
    test_the_recorded_quadrature_is_the_integrators holds the file to the integrator."""
    with np.load(RECORDED) as z:
        out = tuple(z[f"{name}/{f}"] for f in FIELDS)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _expectation(specular):
    hs = _expectation_scene(specular)
    return hs, hs.finalize()


def _params(hs, w, h, spp, seed, nee, max_depth=None, rr_depth=None):
    p = hs.render_params(w, h, spp, seed=seed)
    p.flags = PT_RENDER_NEE if nee else 0
    if max_depth is not None:
        p.max_depth = max_depth
    if rr_depth is not None:
        p.rr_depth = rr_depth
    return p


def _frames(render, hs, w, h, spp, nee, max_depth, rr_depth=None, first=0):
    return np.stack([render(_params(hs, w, h, spp, seed, nee, max_depth, rr_depth)) for seed in SEEDS[first:first + K]])


def _mean_se(x):
    x = x.astype(np.float64)
    return x.mean(0), x.std(0, ddof=1) / np.sqrt(x.shape[0])


def check_direct(name, frames, where):
    """The rule of the module docstring for one direct-light case; prints its figures, then asserts.  Returns them."""
    T, dT, prim, dark, lit = _reference(name)
    mean, se = _mean_se(frames)
    pure = prim != -2
    compared = pure[..., None] & (dT <= 0.1 * C_T * se)
    share = compared.all(-1).mean()
    dev = np.abs(mean - T) - 2 * dT
    noisy, exact = compared & (se > 0), compared & (se == 0)
    worst = (dev[noisy] / (C_T * se[noisy])).max() if noisy.any() else 0.0
    px = compared.all(-1)
    im = frames.astype(np.float64)[:, px].mean(1)                       # [K, 3]: the image mean over the compared pixels
    im_mean, im_se = im.mean(0), im.std(0, ddof=1) / np.sqrt(K)
    im_T, im_dT = T[px].mean(0), dT[px].mean(0)
    rel_se = (im_se / np.maximum(im_T, 1e-300)).max() if im_T.max() > 0 else 0.0
    im_dev = (np.abs(im_mean - im_T) - 2 * im_dT) / np.maximum(C_T * im_se, 1e-300) if im_se.max() > 0 else np.zeros(3)
    print(f"{where} {name}: compared {share:.3f} of the pixels, worst pixel {worst:.3f} c SE, image mean {im_dev.max():.3f} c SE, "
          f"relative SE of the image mean {rel_se:.2e}, bias of the image mean {((im_mean - im_T) / np.maximum(im_T, 1e-300)).max():+.2e}")
    assert share >= 0.8, f"{name}: only {share:.3f} of the pixels are compared"
    assert (dev[exact] <= 0).all(), f"{name}: a pixel without noise is off the quadrature"
    assert worst <= 1.0, f"{name}: a pixel is {worst:.2f} c SE off the quadrature"
    assert im_dev.max() <= 1.0, f"{name}: the image mean is {im_dev.max():.2f} c SE off the quadrature"
    return dict(share=share, worst=worst, image=im_dev.max(), rel_se=rel_se)


def check_exact_bits(name, frames):
    """The three assertions on bits: nothing lit by an emitter that faces away, nothing in the umbra, Le alone on the emitter."""
    T, dT, prim, dark, lit = _reference(name)
    prims = nr.Scene(_case(name)[1]).prims
    plane = np.isin(prim, [k for k, q in enumerate(prims) if q[0] == nr.TRIANGLE and q[3] is None])
    if name == "facing-away":
        assert (T == 0).all()
        assert not bits(frames).any(), "an emitter that faces away lit the plane"
    if name == "hard-shadow":
        umbra = dark & plane
        assert umbra.sum() >= 30 and (lit & plane).sum() >= 100, (umbra.sum(), (lit & plane).sum())
        assert not bits(frames[:, umbra]).any(), "light in the umbra"
        assert (frames[:, lit & plane] > 0).all()
    if name == "emitter-in-view":
        on = np.isin(prim, [k for k, q in enumerate(prims) if q[3] is not None])
        assert on.sum() >= 30, on.sum()
        want = np.broadcast_to(np.float32([3.0, 2.0, 1.0]), frames[:, on].shape)
        assert_bit_equal(frames[:, on], want, "pixels wholly on the emitter")


def check_expectation(name, a, b, where):
    blk = lambda x: x.astype(np.float64).reshape(K, EH // BLOCK, BLOCK, EW // BLOCK, BLOCK, 3).mean(axis=(2, 4))
    A, B = blk(a), blk(b)
    (ma, sa), (mb, sb) = _mean_se(A), _mean_se(B)
    # Student's t needs frame means that are roughly normal.  Where an estimator's block mean is exactly zero in most frames, its
    # light arrives as a few rare events (the edge of a PHONG lobe's support), K frames say nothing about its spread, and the block
    # is left out; such blocks must not carry more than a thousandth of the image, and the image mean below still counts them.
    valid = ((A > 0).sum(0) >= K // 2) & ((B > 0).sum(0) >= K // 2) | ~A.any(0) & ~B.any(0)       # ... or both see the background
    left_out = max(ma[~valid].sum() / ma.sum(), mb[~valid].sum() / mb.sum())
    z = np.where(valid, np.abs(ma - mb) / np.maximum(C_T * np.sqrt(sa ** 2 + sb ** 2), 1e-300), 0.0)
    (ia, ja), (ib, jb) = _mean_se(a.astype(np.float64).mean(axis=(1, 2))), _mean_se(b.astype(np.float64).mean(axis=(1, 2)))
    zi = np.abs(ia - ib) / (C_T * np.sqrt(ja ** 2 + jb ** 2))
    print(f"{where} {name}: {valid.mean():.3f} of the blocks compared (the others hold {left_out:.1e} of the image), "
          f"worst block {z.max():.3f} c SE, image mean {zi.max():.3f} c SE, relative SE of the image mean "
          f"{(ja / ia).max():.2e} (plain) {(jb / ib).max():.2e} (NEE), relative difference {((ib - ia) / ia).max():+.2e}")
    assert ia.min() > 0 and ib.min() > 0
    assert valid.mean() >= 0.8 and left_out <= 1e-3, (valid.mean(), left_out)
    assert z.max() <= 1.0, f"{name}: a block differs by {z.max():.2f} c SE"
    assert zi.max() <= 1.0, f"{name}: the image means differ by {zi.max():.2f} c SE"
    return dict(worst=z.max(), image=zi.max())


def _expectation_frames(render, name, nee_only=False):
    specular, kn, kp, rr, spp = EXPECTATION[name]
    hs, _ = _expectation(specular)
    b = _frames(render, hs, EW, EH, spp, True, kn, rr)
    a = None if nee_only else _frames(render, hs, EW, EH, spp, False, kp, rr, first=K)
    return a, b


# ---- the reference integrator itself ---------------------------------------------------------------------------------------------------

def test_the_integrator_reproduces_the_closed_form():
    """§6's arbiter: one diffuse plane under one point light is rho / pi I cos / d^2 — the formula tests/test_nee.py holds the
    estimator to — written out here once more, at the integrator's own sub-sample positions."""
    hs, d = _case("point-diffuse")
    T, dT, prim, _, _ = _reference("point-diffuse")
    og, tl, hz, vt = camera_ray_data(hs.camera, W, H).astype(np.float64)
    S = 2 * DIRECT["point-diffuse"][3]
    sub = (np.arange(S) + 0.5) / S
    jj, ii, sy, sx = np.meshgrid(np.arange(H), np.arange(W), sub, sub, indexing="ij")
    dirs = tl + hz * ((ii + sx) / W)[..., None] - vt * ((jj + sy) / H)[..., None] - og
    x = og + dirs * (-og[1] / dirs[..., 1])[..., None]
    L = np.float64(POINT[0]) - x
    d2 = (L ** 2).sum(-1)
    rho = np.float32(RHO).astype(np.float64)             # the scene holds float32 reflectances
    want = ((rho / np.pi) * np.float64(POINT[1]) * (L[..., 1] / np.sqrt(d2) / d2)[..., None]).mean(axis=(2, 3))
    assert (prim >= 0).all()
    np.testing.assert_allclose(T, want, rtol=1e-12)
    assert (dT <= 1e-5 * T).all()                        # the film's midpoint rule: h^2 / 24 of a smooth integrand, h = 1 / 16 pixel


@pytest.mark.parametrize("name", list(DIRECT))
def test_the_recorded_quadrature_is_the_integrators(name):
    """Two rows of every case computed anew (a row is computed on its own: the file's other rows are the same code on other rays);
    and the geometry alone, whatever the estimator does, leaves enough pixels that see one primitive."""
    rows = [3, 10]
    for f, a, b in zip(FIELDS, _compute_reference(name, rows), _reference(name)):
        if a.dtype == np.float64:
            np.testing.assert_allclose(a, b[rows], rtol=1e-9, atol=1e-15, err_msg=f"{name}/{f}")
        else:
            assert (a == b[rows]).all(), f"{name}/{f}"
    assert (_reference(name)[2] != -2).mean() >= 0.8


# ---- CPU: the oracle's frames ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle_direct(name, mutation=0):
    import oracle_binding as ob
    hs, d = _case(name)
    old = ob.lib().pt_oracle_set_mutation(mutation)
    try:
        out = _frames(lambda p: ob.render(d, p)[0], hs, W, H, DIRECT[name][2], True, 1)
    finally:
        ob.lib().pt_oracle_set_mutation(old)
    out.setflags(write=False)
    return out


def _oracle_expectation(name, mutation=0):
    import oracle_binding as ob
    d = _expectation(EXPECTATION[name][0])[1]
    plain = _expectation_frames(lambda p: ob.render(d, p)[0], name)[0] if mutation == 0 else _oracle_expectation(name)[0]
    old = ob.lib().pt_oracle_set_mutation(mutation)
    try:
        nee = _expectation_frames(lambda p: ob.render(d, p)[0], name, nee_only=True)[1]
    finally:
        ob.lib().pt_oracle_set_mutation(old)
    return plain, nee


_oracle_expectation = functools.lru_cache(maxsize=None)(_oracle_expectation)


@pytest.mark.parametrize("name", list(DIRECT))
def test_direct_light_matches_the_quadrature(oracle, name):
    frames = _oracle_direct(name)
    check_exact_bits(name, frames)
    check_direct(name, frames, "oracle")


@pytest.mark.parametrize("name", list(EXPECTATION))
def test_nee_gathers_what_the_plain_estimator_gathers(oracle, name):
    check_expectation(name, *_oracle_expectation(name), "oracle")


def _mirror_frames(render):
    hs = _mirror_scene()
    d = hs.finalize()
    return [render(d, _params(hs, 16, 16, 64, SEEDS[0], nee, 2)) for nee in (False, True)]


def test_a_mirror_draws_no_light_sample(oracle):
    """A MIRROR hit takes no light sample and draws nothing; the emitter's emission is added before its own light sample draws, and
    that sample dies on f = 0.  So NEE and the plain estimator walk the same paths: the frames are equal in every bit."""
    plain, nee = _mirror_frames(lambda d, p: oracle.render(d, p)[0])
    assert plain.max() > 0
    assert_bit_equal(nee, plain, "mirror plane showing an emitter")


# mutation -> the cases that must fail under it
MUTATIONS = {
    "NEE_NO_NUM_LIGHTS": (MUT_NO_NUM_LIGHTS, ("three-kinds",)),
    "NEE_COS_SHADING": (MUT_COS_SHADING, ("tilted-normals",)),
    "NEE_NO_LOBE_WEIGHT": (MUT_NO_LOBE_WEIGHT, ("point-plastic", "sphere-plastic")),
    "NEE_BOTH_SIDES": (MUT_BOTH_SIDES, ("facing-away",)),
    "NEE_COUNT_EMISSION": (MUT_COUNT_EMISSION, ("depth-2",)),
    "NEE_TFAR_FULL": (MUT_TFAR_FULL, ("triangle",)),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_the_cases_can_fail(oracle, mutation):
    """Each defect the cases are there for, switched on in the oracle, fails the case named for it (mask 0 passes them all: the
    tests above).  The mask is restored by the helpers that set it."""
    mask, cases = MUTATIONS[mutation]
    for name in cases:
        with pytest.raises(AssertionError):
            if name in DIRECT:
                frames = _oracle_direct(name, mask)
                check_exact_bits(name, frames)
                check_direct(name, frames, mutation)
            else:
                check_expectation(name, *_oracle_expectation(name, mask), mutation)
    assert oracle.lib().pt_oracle_set_mutation(0) == 0


# ---- device ------------------------------------------------------------------------------------------------------------------------------

def _device(d):
    from pathtracer_cuda_interactive_amd import device as dev
    return dev.DeviceScene(d)


def _every_kernel(ds, p, want, what):
    """Scene in LDS and in global memory, kernel 2 and kernel 1.  The light sample exists on kernel 2 only: kernel 1
    must refuse the flag, not render without it."""
    for fg in (0, 1):
        for kernel in (2, 1):
            ds.set_option("force_global", fg)
            ds.set_option("kernel", kernel)
            if kernel == 1 and p.flags & PT_RENDER_NEE:
                with pytest.raises(PtError) as e:
                    ds.render(p)
                assert e.value.status == PT_ERR_UNSUPPORTED
            else:
                assert_bit_equal(ds.render(p), want, f"{what}, force_global {fg}, kernel {kernel}")
    ds.set_option("force_global", 0)
    ds.set_option("kernel", 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DIRECT))
def test_device_direct_light(oracle, name):
    hs, d = _case(name)
    spp = DIRECT[name][2]
    p = _params(hs, W, H, spp, SEEDS[0], True, 1)
    ds = _device(d)
    try:
        _every_kernel(ds, p, oracle.render(d, p)[0], name)
        if name == "three-kinds":
            px = np.arange(W * H, dtype=np.int32)[::-3]
            assert_bit_equal(ds.render_pixels(p, px), ds.render(p).reshape(-1, 3)[px], name + " through pt_render_pixels")
        if name == "unequal-quad":
            q = p.copy()
            q.stream_stride = spp
            img, n, _ = ds.render_adaptive(p, 0.01, max_spp=spp)
            assert (n == spp).all()
            assert_bit_equal(img, ds.render(q), name + " through pt_render_adaptive")
        frames = _frames(ds.render, hs, W, H, GPU_SPP_FACTOR * spp, True, 1)
    finally:
        ds.close()
    check_exact_bits(name, frames)
    check_direct(name, frames, "device")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EXPECTATION))
def test_device_nee_gathers_what_the_plain_estimator_gathers(oracle, name):
    specular, kn, kp, rr, spp = EXPECTATION[name]
    hs, d = _expectation(specular)
    ds = _device(d)
    try:
        for nee, depth in ((True, kn), (False, kp)):
            p = _params(hs, EW, EH, spp, SEEDS[0], nee, depth, rr)
            _every_kernel(ds, p, oracle.render(d, p)[0], f"{name} NEE {nee}")
        factor = GPU_SPP_FACTOR
        b = _frames(ds.render, hs, EW, EH, factor * spp, True, kn, rr)
        a = _frames(ds.render, hs, EW, EH, factor * spp, False, kp, rr, first=K)
    finally:
        ds.close()
    check_expectation(name, a, b, "device")


@pytest.mark.gpu
def test_device_mirror_draws_no_light_sample(oracle):
    hs = _mirror_scene()
    d = hs.finalize()
    ds = _device(d)
    try:
        plain, nee = [ds.render(_params(hs, 16, 16, 64, SEEDS[0], flag, 2)) for flag in (False, True)]
        assert_bit_equal(nee, plain, "mirror plane showing an emitter")
        p = _params(hs, 16, 16, 64, SEEDS[0], True, 2)
        _every_kernel(ds, p, oracle.render(d, p)[0], "mirror plane")
    finally:
        ds.close()


if __name__ == "__main__":
    import sys
    rec = {}
    if sys.argv[1:]:                                      # only the named cases anew
        with np.load(RECORDED) as old:
            rec = {k: old[k] for k in old.files}
    for case in sys.argv[1:] or DIRECT:
        for field, value in zip(FIELDS, _compute_reference(case)):
            rec[f"{case}/{field}"] = value
        print(case, flush=True)
    np.savez_compressed(RECORDED, **rec)
