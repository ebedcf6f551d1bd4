"""pt_temporal_accumulate / pt_temporal_accumulate_host: a colour history carried along pt_render_guides' motion vectors
(include/pt_api.h).

The rule is specified down to the fp32 operation, so the library — host twin and device kernel alike — is pinned bit for bit
against the numpy restatement below (vectorised over the frame, one gather per tap, taps in the rule's order)."""
import ctypes
import os
import re

import numpy as np
import pytest
from conftest import REPO, assert_bit_equal
from test_aov import numpy_guides
from test_motion import case, numpy_motion

from pathtracer_cuda_interactive_amd import PT_ERR_INVALID_ARG, PT_TRAVERSAL_EXACT, PtError, host, temporal_accumulate_host
from pathtracer_cuda_interactive_amd import ctypes_defs as cd
from pathtracer_cuda_interactive_amd import device as dev

F = np.float32


def numpy_temporal(color, normal, motion, prev_depth, history=None, max_history=0, sigma_z=0.0, normal_min=0.9, scale=0.0,
                   stats=None):
    """The rule of pt_api.h in numpy fp32 (0 = the documented default of a field).  stats: a dict that receives how often each
    branch of the rule was taken."""
    color, normal, motion, prev_depth = (np.asarray(a, dtype=F) for a in (color, normal, motion, prev_depth))
    Hh, Ww = prev_depth.shape
    cap = F(max_history or 32)
    sz = F(sigma_z) if sigma_z else F(0.1)
    s = F(scale) if scale else F(1)
    nmin = F(normal_min)
    st = {} if stats is None else stats
    c = color * s
    if history is None:
        return c.astype(F), np.ones((Hh, Ww), dtype=F)
    hc, hn, hz, hl = (np.asarray(a, dtype=F) for a in history)
    with np.errstate(all="ignore"):
        x = motion[..., 0] - F(0.5)
        y = motion[..., 1] - F(0.5)
        valid = prev_depth != 0
        inside = (x >= F(-1)) & (x < F(Ww)) & (y >= F(-1)) & (y < F(Hh))
        ok = valid & inside
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = x - x0, y - y0
        ix, iy = np.where(ok, x0, 0).astype(np.int64), np.where(ok, y0, 0).astype(np.int64)
        acc = np.zeros((Hh, Ww, 3), dtype=F)
        lsum = np.zeros((Hh, Ww), dtype=F)
        wsum = np.zeros((Hh, Ww), dtype=F)
        tol = sz * prev_depth
        for dy in (0, 1):
            for dx in (0, 1):
                qx, qy = ix + dx, iy + dy
                inb = ok & (qx >= 0) & (qx < Ww) & (qy >= 0) & (qy < Hh)
                qxc, qyc = np.clip(qx, 0, Ww - 1), np.clip(qy, 0, Hh - 1)
                b = (fx if dx else F(1) - fx) * (fy if dy else F(1) - fy)
                l, z, n, col = hl[qyc, qxc], hz[qyc, qxc], hn[qyc, qxc], hc[qyc, qxc]
                t_len, t_z0 = l > 0, z != 0
                t_z = np.abs(z - prev_depth) <= tol
                t_n = (normal[..., 0] * n[..., 0] + normal[..., 1] * n[..., 1] + normal[..., 2] * n[..., 2]) >= nmin
                keep = inb & t_len & t_z0 & t_z & t_n
                acc = np.where(keep[..., None], acc + col * b[..., None], acc)
                lsum = np.where(keep, lsum + l * b, lsum)
                wsum = np.where(keep, wsum + b, wsum)
                st["clipped"] = st.get("clipped", 0) + int((ok & ~inb).sum())
                for key, t in (("len", t_len), ("z0", t_z0), ("z", t_z), ("n", t_n)):
                    others = [u for k2, u in (("len", t_len), ("z0", t_z0), ("z", t_z), ("n", t_n)) if k2 != key]
                    st["only_" + key] = st.get("only_" + key, 0) + int((inb & ~t & others[0] & others[1] & others[2]).sum())
        good = ok & (wsum > 0)
        r = F(1) / wsum
        h = acc * r[..., None]
        n = np.minimum(lsum * r + F(1), cap)
        out = np.where(good[..., None], h + (c - h) * (F(1) / n)[..., None], c)
        olen = np.where(good, n, F(1))
        st.update(invalid=int((~valid).sum()), outside=int((valid & ~inside).sum()), no_tap=int((ok & ~(wsum > 0)).sum()),
                  capped=int((good & (lsum * r + F(1) > cap)).sum()), fx0=int((ok & (fx == 0)).sum()),
                  left=int((valid & (x < -1)).sum()), right=int((valid & (x >= Ww)).sum()), top=int((valid & (y < -1)).sum()),
                  bottom=int((valid & (y >= Hh)).sum()))
    assert out.dtype == F and olen.dtype == F
    return out, olen


# ---- inputs -----------------------------------------------------------------------------------------------------------

def synthetic(seed, Hh, Ww):
    """A seeded frame pair in which every branch of the rule is taken: motion that leaves the window on each side, lands on
    exact pixel centres, straddles each frame edge; history taps that fail each of the four tests alone; invalid pixels."""
    rng = np.random.default_rng(seed)
    n_px = Hh * Ww

    def pick(share):
        return rng.random((Hh, Ww)) < share

    color = (rng.random((Hh, Ww, 3)) * 2).astype(F)
    hist_color = (rng.random((Hh, Ww, 3)) * 2).astype(F)
    normal = np.broadcast_to(np.array((0.6, 0.0, 0.8), dtype=F), (Hh, Ww, 3)).copy()
    hist_normal = normal.copy()
    hist_normal[pick(0.08)] = (0.8, 0.0, -0.6)                   # dot = 0
    tilt = pick(0.1)
    hist_normal[tilt] = (0.0, 0.6, 0.8)                          # dot = 0.64: passes normal_min 0.5, fails 0.9
    depth = (2.0 + rng.random((Hh, Ww)) * 0.05).astype(F)
    hist_depth = (2.0 + rng.random((Hh, Ww)) * 0.05).astype(F)
    hist_depth[pick(0.08)] = 0
    hist_depth[pick(0.08)] = 3.0                                 # off by more than sigma_z
    hist_len = rng.integers(1, 40, (Hh, Ww)).astype(F)
    hist_len[pick(0.05)] = 0
    hist_len[pick(0.03)] = -1
    j, i = np.meshgrid(np.arange(Hh), np.arange(Ww), indexing="ij")
    motion = np.stack([i + 0.5 + rng.uniform(-1.5, 1.5, (Hh, Ww)), j + 0.5 + rng.uniform(-1.5, 1.5, (Hh, Ww))], axis=-1).astype(F)
    centre = pick(0.15)
    motion[centre] = np.stack([i + 0.5, j + 0.5], axis=-1).astype(F)[centre]          # fx == fy == 0 exactly
    far = pick(0.12)
    k = rng.integers(0, 4, (Hh, Ww))
    motion[far & (k == 0), 0] = -0.75                            # x < -1
    motion[far & (k == 1), 0] = Ww + 0.5                         # x >= W
    motion[far & (k == 2), 1] = -3.0
    motion[far & (k == 3), 1] = Hh + 0.5
    edge = pick(0.08) & ~far
    motion[edge & (k == 0), 0] = -0.25                           # x in [-1, 0): the left tap column is outside
    motion[edge & (k == 1), 0] = Ww + 0.25                       # x in [W - 1, W): the right one
    motion[edge & (k == 2), 1] = 0.0
    motion[edge & (k == 3), 1] = Hh + 0.125
    depth[pick(0.07)] = 0                                        # invalid pixels
    block = (slice(0, max(1, Hh // 4)), slice(0, max(1, Ww // 4)))
    hist_len[block] = 0                                          # a corner whose taps are all skipped
    assert n_px > 0
    return color, normal, motion, depth, (hist_color, hist_normal, hist_depth, hist_len)


def corner_cases():
    """name -> (color, normal, motion, prev_depth, history, keywords)"""
    cases = {}
    cases["31x24, defaults"] = synthetic(1, 24, 31) + ({},)
    cases["3x2 frame"] = synthetic(2, 2, 3) + ({},)
    cases["67x5, normal_min 0.5"] = synthetic(3, 5, 67) + ({"normal_min": 0.5},)
    cases["max_history 1"] = synthetic(4, 24, 31) + ({"max_history": 1},)
    cases["max_history 8: the cap is reached"] = synthetic(5, 24, 31) + ({"max_history": 8},)
    cases["max_history 65536, sigma_z 0.001"] = synthetic(6, 24, 31) + ({"max_history": 65536, "sigma_z": 0.001},)
    cases["scale 1/3, sigma_z 1.5: every depth passes but 0"] = synthetic(7, 33, 40) + ({"scale": 1.0 / 3.0, "sigma_z": 1.5},)
    cases["normal_min -1"] = synthetic(8, 24, 31) + ({"normal_min": -1.0},)
    c, n, m, z, h = synthetic(9, 9, 11)
    cases["no history"] = (c, n, m, z, None, {"scale": 0.5})
    cases["history of length 0 everywhere"] = (c, n, m, z, (h[0], h[1], h[2], np.zeros_like(h[3])), {})
    cases["every pixel invalid"] = (c, n, m, np.zeros_like(z), h, {})
    c, n, m, z, h = synthetic(10, 1, 1)
    z[:] = 2.0
    for name, mv in (("the tap kept", (0.5, 0.5)), ("the window half outside", (0.25, 1.25))):
        motion = np.broadcast_to(np.array(mv, dtype=F), m.shape).copy()
        cases["1x1 frame, " + name] = (c, n, motion, z, (h[0], n.copy(), z.copy(), np.full_like(h[3], 3)), {})
    cases["65x5: one pixel past a 64x4 tile each way"] = synthetic(11, 5, 65) + ({},)
    return cases


CORNERS = corner_cases()


def test_the_corner_cases_reach_every_branch():
    total = {}
    for name, (c, n, m, z, h, kw) in CORNERS.items():
        st = {}
        numpy_temporal(c, n, m, z, h, stats=st, **kw)
        for k, v in st.items():
            total[k] = total.get(k, 0) + v
        if name == "history of length 0 everywhere":
            assert st["no_tap"] > 0
        if name.startswith("max_history 8"):
            assert st["capped"] > 0
    print(total)
    for k in ("invalid", "outside", "left", "right", "top", "bottom", "fx0", "clipped", "only_len", "only_z0", "only_z", "only_n",
              "no_tap", "capped"):
        assert total.get(k, 0) > 0, k


# ---- CPU --------------------------------------------------------------------------------------------------------------

def test_temporal_params_match_the_header():
    text = open(os.path.join(REPO, "include", "pt_api.h")).read()
    for struct, cls, size in (("pt_temporal_params", cd.PtTemporalParams, 24), ("pt_motion_params", cd.PtMotionParams, 52)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for _, decl in re.findall(r"(int32_t|float)\s+([a-z_0-9, \[\]]+);", body):
            names += [re.sub(r"\[\d+\]", "", n).strip() for n in decl.split(",")]
        assert names == [n for n, _ in cls._fields_], struct
        assert ctypes.sizeof(cls) == size


@pytest.mark.parametrize("name", list(CORNERS))
def test_host_twin_equals_the_numpy_rule(name):
    c, n, m, z, h, kw = CORNERS[name]
    want = numpy_temporal(c, n, m, z, h, **kw)
    got = temporal_accumulate_host(c, n, m, z, history=h, **kw)
    assert_bit_equal(got[0], want[0], name + " colour")
    assert_bit_equal(got[1], want[1], name + " length")
    buf = c.copy()                                               # out_color aliasing color
    out, length = temporal_accumulate_host(buf, n, m, z, history=h, out_color=buf, **kw)
    assert out is buf
    assert_bit_equal(buf, want[0], name + ", out_color = color")
    assert_bit_equal(length, want[1], name + ", out_color = color: length")


def _params(**kw):
    base = dict(width=8, height=6, max_history=0, sigma_z=0.0, normal_min=0.9, scale=0.0)
    base.update(kw)
    return cd.PtTemporalParams(*[base[n] for n, _ in cd.PtTemporalParams._fields_])


INVALID = [("width", dict(width=0)), ("height", dict(height=-1)), ("max_history", dict(max_history=-1)),
           ("max_history", dict(max_history=65537)), ("normal_min", dict(normal_min=1.5)), ("normal_min", dict(normal_min=-1.5)),
           ("normal_min", dict(normal_min=float("nan")))]
for _field in ("sigma_z", "scale"):
    INVALID += [(_field, {_field: v}) for v in (-1.0, float("nan"), float("inf"))]


def _buffers():
    """color, normal, motion, prev_depth, hist_color, hist_normal, hist_depth, hist_len, out_color, out_len of an 8x6 frame"""
    shapes = [(6, 8, 3), (6, 8, 3), (6, 8, 2), (6, 8), (6, 8, 3), (6, 8, 3), (6, 8), (6, 8), (6, 8, 3), (6, 8)]
    return [np.ones(s, dtype=F) for s in shapes]


def _call(fn, t, bufs, handle=None):
    ptrs = [None if b is None else b.ctypes.data_as(ctypes.c_void_p) for b in bufs]
    tp = None if t is None else ctypes.byref(t)
    return fn(tp, *ptrs) if handle is None else fn(handle, tp, *ptrs, 0, None)


def _argument_errors(fn, handle=None):
    lib = dev.lib()
    assert _call(fn, _params(), _buffers(), handle) == 0
    for field, kw in INVALID:
        assert _call(fn, _params(**kw), _buffers(), handle) == PT_ERR_INVALID_ARG, (field, kw)
        assert field in lib.pt_last_error().decode(), (field, lib.pt_last_error())
    assert _call(fn, None, _buffers(), handle) == PT_ERR_INVALID_ARG
    assert "pt_temporal_params" in lib.pt_last_error().decode()
    b = _buffers()
    b[8] = b[4]                                                  # out_color == hist_color
    assert _call(fn, _params(), b, handle) == PT_ERR_INVALID_ARG
    assert "out_color" in lib.pt_last_error().decode() and "hist_color" in lib.pt_last_error().decode()
    b = _buffers()
    b[9] = b[7]                                                  # out_len == hist_len
    assert _call(fn, _params(), b, handle) == PT_ERR_INVALID_ARG
    assert "out_len" in lib.pt_last_error().decode() and "hist_len" in lib.pt_last_error().decode()
    b = _buffers()
    b[8] = b[0]                                                  # out_color == color is allowed
    assert _call(fn, _params(), b, handle) == 0
    b = _buffers()
    b[4:8] = [None] * 4                                          # no history
    assert _call(fn, _params(), b, handle) == 0
    b[4] = np.ones((6, 8, 3), dtype=F)                           # ... but not a part of one
    assert _call(fn, _params(), b, handle) == PT_ERR_INVALID_ARG
    assert "hist_" in lib.pt_last_error().decode()
    for k in (0, 1, 2, 3, 8, 9):
        b = _buffers()
        b[k] = None
        assert _call(fn, _params(), b, handle) == PT_ERR_INVALID_ARG


def test_host_twin_rejects_bad_arguments():
    _argument_errors(dev.lib().pt_temporal_accumulate_host)
    with pytest.raises(PtError) as e:
        temporal_accumulate_host(*_buffers()[:4], sigma_z=-1.0)
    assert e.value.status == PT_ERR_INVALID_ARG and "sigma_z" in str(e.value)


def test_a_static_scene_converges_to_the_mean_of_its_frames():
    """Identity motion written by hand (exact pixel centres, so fx = fy = 0 and one tap of weight 1 is kept): the rule is the
    running mean h + (c - h) / n, and after 8 frames the history is 8 long and holds their arithmetic mean."""
    Hh, Ww = 20, 27
    rng = np.random.default_rng(12)
    frames = [(rng.random((Hh, Ww, 3)) * 2 + 0.1).astype(F) for _ in range(8)]
    normal = np.broadcast_to(np.array((0.0, 0.6, 0.8), dtype=F), (Hh, Ww, 3)).copy()
    depth = (1.0 + rng.random((Hh, Ww)) * 3).astype(F)
    j, i = np.meshgrid(np.arange(Hh), np.arange(Ww), indexing="ij")
    motion = np.stack([i + 0.5, j + 0.5], axis=-1).astype(F)
    hist = None
    for f in frames:
        out, length = temporal_accumulate_host(f, normal, motion, depth, history=hist, max_history=32)
        hist = (out, normal, depth, length)
    assert (length == 8).all()
    mean = np.mean(np.stack(frames).astype(np.float64), axis=0)
    rel = float(np.abs(out / mean - 1).max())
    print(f"8 static frames: max relative difference from their mean {rel:.3e}")
    assert rel <= 1e-5


# ---- an animated sequence, made once ------------------------------------------------------------------------------------

SEQ_W, SEQ_H, SEQ_FRAMES, SEQ_SPP = 96, 72, 6, 2
SEQ_MESH = 7                                                     # cbox: the box test_scene_update wobbles
SEQ_KW = dict(max_history=0, sigma_z=0.0, normal_min=0.9)        # tools/animate.py's defaults
# The camera moves by 2 % of the median hit distance per frame along (0.9, 0.35, -0.6): between one and two pixels per frame
# at 96x72.
SEQ_STEP = 0.02


def sequence_frames(oracle):
    """Per frame k: (render params, desc with a valid node pool, desc of the previous frame's geometry, previous params)."""
    hs, d0 = case("cbox")[:2]
    p0 = hs.render_params(SEQ_W, SEQ_H, SEQ_SPP, seed=3)
    p0.traversal = PT_TRAVERSAL_EXACT
    g = numpy_guides(oracle, d0, p0)
    step = np.array([0.9, 0.35, -0.6]) * SEQ_STEP * float(np.median(g["depth"][g["prim"] >= 0]))
    frames, d_prev, p_prev = [], d0, p0
    for k in range(SEQ_FRAMES):
        p = dev.translated_params(p0, step * k)
        p.seed = 3 + k
        d = d0 if k == 0 else dev.wobbled_desc(d0, k, meshes=[SEQ_MESH])
        frames.append((p, d if k == 0 else host.refit_bvh(d), d_prev, p_prev, d))
        d_prev, p_prev = d, p
    return frames


_reference = {}


def reference_sequence(oracle):
    """The sequence on the CPU — guides and motion by the numpy rules, accumulation by the host twin on zero colour (history
    lengths do not depend on colour): out_len and the hit mask of the last frame."""
    if not _reference:
        hist = None
        for p, d, d_prev, p_prev, _ in sequence_frames(oracle):
            g = numpy_guides(oracle, d, p)
            motion, pz, hit = numpy_motion(oracle, d, d_prev, p, p_prev)
            zero = np.zeros((SEQ_H, SEQ_W, 3), dtype=F)
            out, length = temporal_accumulate_host(zero, g["normal"], motion, pz, history=hist, **SEQ_KW)
            want = numpy_temporal(zero, g["normal"], motion, pz, hist, **SEQ_KW)
            assert_bit_equal(length, want[1], "host twin vs numpy on the sequence")
            hist = (out, g["normal"], g["depth"], length)
        _reference.update(length=length, hit=hit, share=float((length[hit] > 1).mean()))
    return _reference


# The share of hit pixels of the last frame whose history is longer than one frame, on the CPU (numpy guides and motion from
# the oracle's hits, host twin): 0.9998.  Pixels lose their history at silhouettes and at the frame's edge the camera moves towards.
SEQ_REFERENCE_SHARE = 0.9998


def test_history_survives_motion_on_the_cpu(oracle):
    ref = reference_sequence(oracle)
    print(f"reference share of hit pixels with a history: {ref['share']:.4f}; mean length {ref['length'][ref['hit']].mean():.2f}")
    assert ref["share"] > 0.8
    assert abs(ref["share"] - SEQ_REFERENCE_SHARE) < 5e-4, "SEQ_REFERENCE_SHARE and DESIGN.md §19 state the value"


# ---- GPU --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cbox_scene():
    ds = dev.DeviceScene(case("cbox")[1])
    yield ds
    ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CORNERS))
def test_device_filter_equals_host_and_numpy_on_corner_cases(cbox_scene, name):
    import torch
    c, n, m, z, h, kw = CORNERS[name]
    want = numpy_temporal(c, n, m, z, h, **kw)
    host_out = temporal_accumulate_host(c, n, m, z, history=h, **kw)
    got = cbox_scene.temporal_accumulate(c, n, m, z, history=h, **kw)
    for k, what in ((0, "colour"), (1, "length")):
        assert_bit_equal(got[k], host_out[k], f"{name} {what}: device vs host")
        assert_bit_equal(got[k], want[k], f"{name} {what}: device vs numpy")
    # device pointers, out_color aliasing color
    tc, tn, tm, tz = (torch.from_numpy(v).cuda() for v in (c, n, m, z))
    th = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in h] if h is not None else None
    tl = torch.full(z.shape, -7.0, device="cuda")
    cbox_scene.temporal_accumulate_into(z.shape[1], z.shape[0], tc.data_ptr(), tn.data_ptr(), tm.data_ptr(), tz.data_ptr(),
                                        [t.data_ptr() for t in th] if th else None, tc.data_ptr(), tl.data_ptr(), **kw)
    torch.cuda.synchronize()
    assert_bit_equal(tc.cpu().numpy(), want[0], name + " device pointers, out_color = color")
    assert_bit_equal(tl.cpu().numpy(), want[1], name + " device pointers: length")


@pytest.mark.gpu
def test_device_filter_rejects_bad_arguments(cbox_scene):
    _argument_errors(dev.lib().pt_temporal_accumulate, cbox_scene._h)
    ptrs = [b.ctypes.data_as(ctypes.c_void_p) for b in _buffers()]
    t = _params()
    assert dev.lib().pt_temporal_accumulate(None, ctypes.byref(t), *ptrs, 0, None) == PT_ERR_INVALID_ARG
    assert "null scene" in dev.lib().pt_last_error().decode()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cbox", "random7"])
def test_device_filter_on_rendered_frames_behind_an_async_render(oracle, name):
    """Three 2-spp frames with camera motion and one update in between.  Per frame: pt_render_async on a stream of the
    caller's and pt_temporal_accumulate right behind it on the same stream, no host sync in between; the result equals the
    blocking host-pointer form, the host twin and the numpy rule on the same inputs, bit for bit."""
    import torch
    from test_motion import camera_step
    hs, d0, d1 = case(name)[:3]
    Ww, Hh = 64, 48
    p0 = hs.render_params(Ww, Hh, 2, seed=5)
    step = camera_step(oracle, name, p0, scale=0.01)
    ds = dev.DeviceScene(d0)
    try:
        stream = torch.cuda.Stream()
        hist_np, hist_t, p_prev = None, None, p0
        for k in range(3):
            p = dev.translated_params(p0, step * k)
            p.seed = 5 + k
            if k == 2:
                ds.update(d1)
            g = ds.render_guides(p, p_prev, previous_geometry=True)
            tn, tm, tz = (torch.from_numpy(g[key]).cuda() for key in ("normal", "motion", "prev_depth"))
            color = torch.zeros((Hh, Ww, 3), device="cuda")
            out = torch.zeros((Hh, Ww, 3), device="cuda")
            length = torch.zeros((Hh, Ww), device="cuda")
            torch.cuda.synchronize()
            ds.render_into(p, color.data_ptr(), stream=stream.cuda_stream)
            ds.temporal_accumulate_into(Ww, Hh, color.data_ptr(), tn.data_ptr(), tm.data_ptr(), tz.data_ptr(),
                                        [t.data_ptr() for t in hist_t] if hist_t else None, out.data_ptr(), length.data_ptr(),
                                        stream=stream.cuda_stream)
            stream.synchronize()
            c = color.cpu().numpy()
            assert_bit_equal(c, ds.render(p), f"{name} frame {k}: the async render")
            want = numpy_temporal(c, g["normal"], g["motion"], g["prev_depth"], hist_np)
            twin = temporal_accumulate_host(c, g["normal"], g["motion"], g["prev_depth"], history=hist_np)
            blocking = ds.temporal_accumulate(c, g["normal"], g["motion"], g["prev_depth"], history=hist_np)
            for j, what in ((0, "colour"), (1, "length")):
                got = (out, length)[j].cpu().numpy()
                assert_bit_equal(got, want[j], f"{name} frame {k} {what}: stream form vs numpy")
                assert_bit_equal(got, twin[j], f"{name} frame {k} {what}: stream form vs host twin")
                assert_bit_equal(got, blocking[j], f"{name} frame {k} {what}: stream form vs blocking form")
            if k:
                share = float((want[1][g["prev_depth"] > 0] > 1).mean())
                print(f"{name} frame {k}: {share:.3f} of the valid pixels continue a history")
                assert share > 0.5
            hist_np = (want[0], g["normal"], g["depth"], want[1])
            hist_t = [out, tn, torch.from_numpy(g["depth"]).cuda(), length]
            p_prev = p
    finally:
        ds.close()


@pytest.mark.gpu
def test_render_and_aov_are_untouched_by_guides_and_accumulation():
    hs, d0, d1 = case("cbox")[:3]
    p = hs.render_params(64, 48, 4)
    prev = dev.translated_params(p, (1.0, 0.5, -0.5))
    ds = dev.DeviceScene(d0)
    try:
        for updated in (False, True):
            if updated:
                ds.update(d1)
            before, aov = ds.render(p), ds.render_aov(p)
            g = ds.render_guides(p, prev, previous_geometry=True)
            out, length = ds.temporal_accumulate(before, g["normal"], g["motion"], g["prev_depth"])
            out2, _ = ds.temporal_accumulate(before, g["normal"], g["motion"], g["prev_depth"], history=(out, g["normal"], g["depth"], length))
            assert np.isfinite(out2).all()
            assert_bit_equal(ds.render(p), before, f"pt_render after guides + accumulate, updated={updated}")
            after = ds.render_aov(p)
            assert np.array_equal(after["prim"], aov["prim"])
            for k in ("albedo", "normal", "depth"):
                assert_bit_equal(after[k], aov[k], f"pt_render_aov {k} after guides + accumulate, updated={updated}")
    finally:
        ds.close()


def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


_device_sequence = {}


def device_sequence(oracle):
    """The sequence on the device: pt_render at 2 spp, pt_render_guides, pt_temporal_accumulate per frame, through
    DeviceScene.update.  Returns the last frame's noisy colour, accumulated colour, history length, guides."""
    if not _device_sequence:
        frames = sequence_frames(oracle)
        ds = dev.DeviceScene(frames[0][1])
        try:
            hist = None
            for k, (p, _, _, p_prev, d_edit) in enumerate(frames):
                if k:
                    ds.update(d_edit)
                noisy = ds.render(p)
                g = ds.render_guides(p, p_prev, previous_geometry=True)
                out, length = ds.temporal_accumulate(noisy, g["normal"], g["motion"], g["prev_depth"], history=hist, **SEQ_KW)
                hist = (out, g["normal"], g["depth"], length)
            den = ds.denoise(out, g["albedo"], g["normal"], g["depth"])
        finally:
            ds.close()
        _device_sequence.update(noisy=noisy, out=out, length=length, g=g, denoised=den)
    return _device_sequence


@pytest.mark.gpu
def test_history_survives_motion(oracle):
    """cbox 96x72, 6 frames, the camera translating, one mesh wobbling through update: the share of the last frame's hit pixels
    that continue a history is the CPU reference's (SEQ_REFERENCE_SHARE = 0.9998, numpy rules + host twin) less at most 0.05 —
    so that the quality test below cannot pass on fallbacks."""
    ref = reference_sequence(oracle)
    seq = device_sequence(oracle)
    hit = seq["g"]["prim"] >= 0
    share = float((seq["length"][hit] > 1).mean())
    print(f"share of hit pixels with a history: device {share:.4f}, CPU reference {ref['share']:.4f}")
    assert share >= ref["share"] - 0.05
    assert_bit_equal(seq["length"], ref["length"], "history length: device sequence vs CPU sequence")


# RMSE(accumulated) / RMSE(noisy 2-spp last frame) against the oracle at 256 spp, measured on the MI355X: 0.2960 (RMSE 0.35809
# -> 0.10601); with pt_denoise applied after the accumulation 0.2360 (0.08452; for the record, not asserted).  The same
# sequence run on the CPU - oracle.render, the numpy guide and motion rules, the host twins of both filters - gives the same
# figures to every printed digit, as the bit-for-bit tests say it must.  profiles/r06_temporal_tests.log
MEASURED_RATIO = 0.2960
MEASURED_RATIO_DENOISED = 0.2360


@pytest.mark.gpu
def test_accumulation_removes_noise(oracle):
    """The last frame of the sequence against the oracle at 256 spp on the last frame's geometry (pool from host.refit_bvh):
    ratio = RMSE(accumulated) / RMSE(noisy 2-spp frame) <= 1.25 x MEASURED_RATIO (test_reference_images' margin for measured
    residuals); the ratio itself is below 0.75, test_filter_removes_noise's bar."""
    seq = device_sequence(oracle)
    p, d_last = sequence_frames(oracle)[-1][:2]
    q = p.copy()
    q.spp, q.seed = 256, 1984
    truth, _ = oracle.render(d_last, q)
    before, after, den = _rmse(seq["noisy"], truth), _rmse(seq["out"], truth), _rmse(seq["denoised"], truth)
    print(f"RMSE noisy {before:.5f}, accumulated {after:.5f}, ratio {after / before:.4f}; with pt_denoise behind it "
          f"{den:.5f}, ratio {den / before:.4f}")
    assert MEASURED_RATIO is not None and MEASURED_RATIO <= 0.75
    assert after / before <= 1.25 * MEASURED_RATIO
