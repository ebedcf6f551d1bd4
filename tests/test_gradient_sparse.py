"""pt_gradient_pixels / pt_temporal_gradient_sparse and their host twins: one re-traced pixel per tile of pt_temporal_gradient's
grid, at a per-frame pseudo-random position, in place of a re-traced row (include/pt_api.h).

Both rules are specified down to the uint32 / fp32 operation, so the library — host twins and device kernels alike — is pinned
bit for bit against the numpy restatements below.  The quality of the whole chain — pixel choice, the pixel-list re-trace, the
sparse gradient, adaptive accumulation — is measured on §21's three 10-frame sequences against the oracle at 256 spp."""
import ctypes

import numpy as np
import pytest
from conftest import assert_bit_equal, bits
from test_motion import case
from test_temporal import SEQ_KW
from test_temporal_adaptive import (MARGIN, Q_FRAMES, Q_RELIGHT_AT, SEQUENCES, _renders, _report, run_sequence, sequence_frames)
from test_temporal_gradient import H5, INVALID, SIZES, _params, scaled_lights, synthetic

from pathtracer_cuda_interactive_amd import (PT_ERR_INVALID_ARG, PtError, gradient_pixels_host, temporal_accumulate_adaptive_host,
                                             temporal_accumulate_moments_host, temporal_gradient_sparse_host)
from pathtracer_cuda_interactive_amd import ctypes_defs as cd
from pathtracer_cuda_interactive_amd import device as dev

F = np.float32
U = np.uint32
INT32_MIN = -2 ** 31


# ---- the rules in numpy ----------------------------------------------------------------------------------------------------

def numpy_pixels(Ww, Hh, seed, stride=0, stats=None):
    """pixels [TH * TW] int32 by the rule of pt_api.h: wrapping uint32 arithmetic on arrays (numpy wraps them silently)."""
    s = stride or 3
    _, TH, TW = dev.gradient_grid(Ww, Hh, s)
    t = np.arange(TH * TW, dtype=U)
    sigma = np.array([seed & 0xffffffff], dtype=U)
    v = t * U(747796405) + (sigma * U(2891336453) + U(1))
    w = ((v >> ((v >> U(28)) + U(4))) ^ v) * U(277803737)
    h = (w >> U(22)) ^ w
    assert v.dtype == U and w.dtype == U and h.dtype == U
    ox, oy = ((h & U(0xffff)) % U(s)).astype(np.int64), ((h >> U(16)) % U(s)).astype(np.int64)
    tx, ty = t.astype(np.int64) % TW, t.astype(np.int64) // TW
    x, y = np.minimum(s * tx + ox, Ww - 1), np.minimum(s * ty + oy, Hh - 1)
    if stats is not None:
        stats["x_clamped"] = stats.get("x_clamped", 0) + int((s * tx + ox > Ww - 1).sum())
        stats["y_clamped"] = stats.get("y_clamped", 0) + int((s * ty + oy > Hh - 1).sum())
    return (y * Ww + x).astype(np.int32)


def numpy_sparse(prev_color, pixels, resampled, stride=0, iterations=0, gain=0.0, norm_floor=0.0, x0_out=None):
    """lambda [TH, TW] by the rule of pt_api.h in numpy fp32: the sparse reduce, then pt_temporal_gradient's filter and final step
    (the taps in the rule's order, as test_temporal_gradient.numpy_gradient states them)."""
    prev_color, resampled = np.asarray(prev_color, dtype=F), np.asarray(resampled, dtype=F)
    Hh, Ww = prev_color.shape[:2]
    s = stride or 3
    iters = iterations or 3
    g = F(gain) if gain else F(2)
    floor = F(norm_floor) if norm_floor else F(1e-6)
    _, TH, TW = dev.gradient_grid(Ww, Hh, s)
    e = np.asarray(pixels, dtype=np.int64).reshape(TH * TW)
    assert resampled.shape == (TH * TW, 3)
    inside = (e >= 0) & (e < Ww * Hh)
    b = resampled
    a = np.where(inside[:, None], prev_color.reshape(-1, 3)[np.where(inside, e, 0)], b)
    x = np.concatenate([b - a, np.where(a < b, b, a)], axis=-1).reshape(TH, TW, 6)
    if x0_out is not None:
        x0_out.append(x.copy())
    ty, tx = np.meshgrid(np.arange(TH), np.arange(TW), indexing="ij")
    for k in range(iters):
        acc = np.zeros((TH, TW, 6), dtype=F)
        wsum = np.zeros((TH, TW), dtype=F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qx, qy = tx + dx * (1 << k), ty + dy * (1 << k)
                inb = (qx >= 0) & (qx < TW) & (qy >= 0) & (qy < TH)
                w = H5[dy + 2] * H5[dx + 2]
                q = x[np.clip(qy, 0, TH - 1), np.clip(qx, 0, TW - 1)]
                acc = np.where(inb[..., None], acc + q * w, acc)
                wsum = np.where(inb, wsum + w, wsum)
        x = acc * (F(1) / wsum)[..., None]
    d, m = x[..., :3], x[..., 3:]
    with np.errstate(all="ignore"):
        r = np.abs(d) / np.maximum(m, floor)
    r = np.maximum(np.maximum(r[..., 0], r[..., 1]), r[..., 2])
    lam = np.minimum(g * r, F(1))
    assert lam.dtype == F and lam.shape == (TH, TW)
    return lam


# ---- inputs ----------------------------------------------------------------------------------------------------------------

GRIDS = [(7, 3, 1), (7, 3, 2), (7, 3, 3), (67, 5, 3), (64, 9, 4), (16, 16, 16), (200, 13, 2)]   # W, H, stride
SEEDS = (0, 1, 0xffffffff)


def gathered(seed, Hh, Ww, stride, frame):
    """A previous frame, the list of frame number `frame` and the previous frame's changed version gathered at the list
    (test_temporal_gradient.synthetic at stride 1 changes a whole frame)."""
    prev, changed = synthetic(seed, Hh, Ww, 1)
    px = numpy_pixels(Ww, Hh, frame, stride)
    return prev, px, changed.reshape(-1, 3)[px].copy()


def corner_cases():
    """name -> (prev_color, pixels, resampled, keywords)"""
    cases = {}
    for k, (Ww, Hh, s) in enumerate(GRIDS):
        cases[f"{Ww}x{Hh}, stride {s}"] = gathered(k, Hh, Ww, s, SEEDS[k % 3]) + ({"stride": s},)
    cases["1 iteration"] = gathered(7, 24, 31, 3, 5) + ({"iterations": 1},)
    cases["8 iterations: the spacing exceeds the grid"] = gathered(8, 24, 31, 3, 6) + ({"iterations": 8},)
    cases["gain 0.5"] = gathered(9, 24, 31, 3, 7) + ({"gain": 0.5},)
    z = np.zeros((9, 11, 3), dtype=F)
    px = numpy_pixels(11, 9, 2)
    cases["a frame of zeros"] = (z, px, np.zeros((px.size, 3), dtype=F), {})
    cases["a frame of zeros against 1e-7: norm_floor decides"] = (z, px, np.full((px.size, 3), 1e-7, dtype=F), {})
    prev, px, res = gathered(12, 5, 67, 3, 9)
    px = px.copy()
    px[0::5], px[1::5], px[2::5] = -1, 67 * 5, INT32_MIN
    cases["67x5 with entries -1, W * H and INT32_MIN"] = (prev, px, res, {"stride": 3})
    return cases


CORNERS = corner_cases()


# ---- CPU: the pixel choice ---------------------------------------------------------------------------------------------------

def test_pixel_choice_equals_the_numpy_rule_and_stays_in_its_tile():
    st = {}
    for Ww, Hh, s in GRIDS:
        _, TH, TW = dev.gradient_grid(Ww, Hh, s)
        for seed in SEEDS:
            want = numpy_pixels(Ww, Hh, seed, s, stats=st)
            got = gradient_pixels_host(Ww, Hh, seed, stride=s)
            assert got.dtype == np.int32 and (got == want).all(), (Ww, Hh, s, seed)
            x, y = got % Ww, got // Ww
            t = np.arange(TH * TW)
            assert (got >= 0).all() and (got < Ww * Hh).all()
            assert (x // s == t % TW).all() and (y // s == t // TW).all(), (Ww, Hh, s, seed)
            if s == 1:                                           # the identity on the rows of the grid
                assert (got == t).all()
        assert len({tuple(gradient_pixels_host(Ww, Hh, k, stride=s)) for k in SEEDS}) == (3 if s > 1 else 1)
    print(st)
    assert st["x_clamped"] > 0 and st["y_clamped"] > 0           # both clamps are reached, counted not assumed


def test_the_default_stride_is_three():
    assert (gradient_pixels_host(96, 72, 4) == numpy_pixels(96, 72, 4, 3)).all()
    assert gradient_pixels_host(96, 72, 4).shape == (24 * 32,)


# ---- CPU: the sparse reduce and lambda --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CORNERS))
def test_host_twin_equals_the_numpy_rule(name):
    a, px, b, kw = CORNERS[name]
    assert_bit_equal(temporal_gradient_sparse_host(a, px, b, **kw), numpy_sparse(a, px, b, **kw), name)


@pytest.mark.parametrize("name", list(CORNERS))
def test_equal_inputs_give_plus_zero_everywhere(name):
    a, px, _, kw = CORNERS[name]
    Hh, Ww = a.shape[:2]
    same = a.reshape(-1, 3)[np.clip(px, 0, Ww * Hh - 1)]
    assert (bits(temporal_gradient_sparse_host(a, px, same, **kw)) == 0).all(), name
    assert (bits(numpy_sparse(a, px, same, **kw)) == 0).all(), name


def test_entries_outside_the_frame_give_d_plus_zero():
    """A tile whose entry is outside [0, W * H) compares its re-traced value with itself: d = +0, m = b, whatever prev_color
    holds; a list of such entries alone gives lambda == +0 at every tile."""
    a, px, b, kw = CORNERS["67x5 with entries -1, W * H and INT32_MIN"]
    x0 = []
    numpy_sparse(a, px, b, x0_out=x0, **kw)
    out = (px < 0) | (px >= 67 * 5)
    assert out.sum() >= 3 * (px.size // 5) and (~out).any()
    x0 = x0[0].reshape(-1, 6)
    assert (bits(x0[out, :3]) == 0).all() and (bits(x0[out, 3:]) == bits(b[out])).all()
    for entry in (-1, 67 * 5, INT32_MIN, 2 ** 31 - 1):
        lam = temporal_gradient_sparse_host(a, np.full(px.size, entry, dtype=np.int32), b, **kw)
        assert (bits(lam) == 0).all(), entry
    one = np.full((16, 16, 3), 0.5, dtype=F)                     # a single tile
    for entry in (-1, 256, INT32_MIN):
        lam = temporal_gradient_sparse_host(one, np.array([entry], dtype=np.int32), np.ones((1, 3), dtype=F), stride=16)
        assert lam.shape == (1, 1) and bits(lam)[0, 0] == 0


# ---- CPU: arguments and exports ------------------------------------------------------------------------------------------------

def _sparse_buffers():
    """prev_color, pixels, resampled, lambda_out of an 8x6 frame at the default stride (a 2x3 grid)"""
    return [np.ones((6, 8, 3), dtype=F), np.zeros(6, dtype=np.int32), np.ones((6, 3), dtype=F), np.ones((2, 3), dtype=F)]


def _call(fn, g, bufs, handle=None, seed=None):
    ptrs = [None if b is None else b.ctypes.data_as(ctypes.c_void_p) for b in bufs]
    gp = None if g is None else ctypes.byref(g)
    args = (gp,) + (() if seed is None else (ctypes.c_uint32(seed),)) + tuple(ptrs)
    return fn(*args) if handle is None else fn(handle, *args, 0, None)


def _argument_errors(fn, names, buffers, handle=None, seed=None):
    err = lambda: dev.lib().pt_last_error().decode()             # noqa: E731
    assert _call(fn, _params(), buffers(), handle, seed) == 0
    for field, kw in INVALID:
        assert _call(fn, _params(**kw), buffers(), handle, seed) == PT_ERR_INVALID_ARG, (field, kw)
        assert "pt_gradient_params." in err() and field in err(), (field, err())
    assert _call(fn, None, buffers(), handle, seed) == PT_ERR_INVALID_ARG and "pt_gradient_params" in err()
    for k, name in enumerate(names):
        b = buffers()
        b[k] = None
        assert _call(fn, _params(), b, handle, seed) == PT_ERR_INVALID_ARG and "null " + name in err(), (name, err())


SPARSE_NAMES = ("prev_color", "pixels", "resampled", "lambda_out")


def test_host_twins_reject_bad_arguments():
    _argument_errors(dev.lib().pt_temporal_gradient_sparse_host, SPARSE_NAMES, _sparse_buffers)
    _argument_errors(dev.lib().pt_gradient_pixels_host, ("pixels_out",), lambda: [np.zeros(6, dtype=np.int32)], seed=3)
    a, px, b, _ = _sparse_buffers()
    with pytest.raises(PtError) as e:
        temporal_gradient_sparse_host(a, px, b, gain=-1.0)
    assert e.value.status == PT_ERR_INVALID_ARG and "gain" in str(e.value)
    with pytest.raises(ValueError):
        temporal_gradient_sparse_host(a, px[:5], b)              # not one pixel per tile
    with pytest.raises(ValueError):
        temporal_gradient_sparse_host(a, px, np.ones((2, 8, 3), dtype=F))   # the rows of the other variant


def test_the_new_symbols_are_exported_and_declared():
    import pathtracer_cuda_interactive_amd as pkg
    new = {"pt_render_pixels", "pt_gradient_pixels", "pt_gradient_pixels_host", "pt_temporal_gradient_sparse",
           "pt_temporal_gradient_sparse_host"}
    assert new <= set(dev.EXPORTS) and new == set(cd.SPARSE_ARGTYPES)
    lib = dev.lib()
    for name in new:
        assert getattr(lib, name).argtypes == cd.SPARSE_ARGTYPES[name]
    for name in ("render_pixels", "render_pixels_into", "gradient_pixels_into", "temporal_gradient_sparse",
                 "temporal_gradient_sparse_into"):
        assert callable(getattr(dev.DeviceScene, name)), name
    assert pkg.gradient_pixels_host is gradient_pixels_host and pkg.temporal_gradient_sparse_host is temporal_gradient_sparse_host


# ---- oracle frames ------------------------------------------------------------------------------------------------------------

_frames = {}


def oracle_frames(oracle, name):
    """A 2-spp frame of the scene and the same frame after the lights changed."""
    if name not in _frames:
        hs, d0 = case(name)[:2]
        Ww, Hh = SIZES[name]
        p = hs.render_params(Ww, Hh, 2, seed=11)
        _frames[name] = (oracle.render(d0, p)[0], oracle.render(scaled_lights(d0), p)[0])
    return _frames[name]


@pytest.mark.parametrize("name", list(SIZES))
def test_an_unchanged_scene_gives_plus_zero(oracle, name):
    """A listed pixel holds the full frame's bits (pt_render_pixels' contract; on the CPU the full frame gathered at the list),
    so on an unchanged scene lambda is +0 at every tile, at every seed."""
    full, _ = oracle_frames(oracle, name)
    Ww, Hh = SIZES[name]
    for seed in (0, 7):
        px = gradient_pixels_host(Ww, Hh, seed)
        lam = temporal_gradient_sparse_host(full, px, full.reshape(-1, 3)[px])
        assert lam.shape == dev.gradient_grid(Ww, Hh)[1:] and (bits(lam) == 0).all()


@pytest.mark.parametrize("name", list(SIZES))
def test_host_twin_equals_the_numpy_rule_after_a_light_change(oracle, name):
    full, relit = oracle_frames(oracle, name)
    Ww, Hh = SIZES[name]
    px = gradient_pixels_host(Ww, Hh, 1)
    res = relit.reshape(-1, 3)[px]
    lam = temporal_gradient_sparse_host(full, px, res)
    assert_bit_equal(lam, numpy_sparse(full, px, res), name)
    print(f"{name}: sparse lambda after lights x (0.2, 0.5, 1.0): mean {lam.mean():.3f}, share saturated {(lam == 1).mean():.3f}, "
          f"share zero {(lam == 0).mean():.3f}")
    assert lam.mean() > 0.5                                      # the red channel lost 80 %: 2 x 0.8 saturates where light arrives


# ---- quality: §21's three 10-frame sequences with the sparse chain ------------------------------------------------------------

def chain_hooks(render_full, make_pixels, render_list, gradient):
    """run_sequence's `render` and `gradient` for the sparse chain.  run_sequence asks `render` for the row selection of the
    previous frame's parameters on the current scene; here that request makes the list of the current frame number (the seed)
    and re-traces the previous frame's parameters at it, and `gradient` receives (list, colours)."""
    def render(d, p):
        if p.row_stride > 1:
            q = p.copy()
            q.row_begin = q.row_end = q.row_stride = 0
            px = make_pixels(q.seed - 3 + 1)                     # sequence_frames: frame k renders with seed 3 + k
            return px, render_list(d, q, px)
        return render_full(d, p)

    def grad(prev_noisy, retrace):
        return gradient(prev_noisy, *retrace)
    return render, grad


_cpu = {}


def cpu_sequence(oracle, which):
    """Sequence a, b or c on the CPU: oracle.render (the re-trace: the full frame of the previous parameters on the current
    scene, gathered at the list), the numpy guide and motion rules, the host twins.  Full frames are shared with
    test_temporal_adaptive's sequences."""
    if which not in _cpu:
        from test_aov import numpy_guides
        from test_motion import numpy_motion
        spec = SEQUENCES[which]
        frames = sequence_frames(oracle, **spec)

        def cached(d, p, kind):
            k = p.seed - 3
            late = kind == "prev-full"                           # frame k's parameters on frame k + 1's scene
            key = (spec["moving"], spec["relight"] and k + late >= Q_RELIGHT_AT, k, kind)
            if key not in _renders:
                _renders[key] = oracle.render(d, p)[0]
            return _renders[key]

        render, grad = chain_hooks(lambda d, p: cached(d, p, "full"), lambda k: gradient_pixels_host(96, 72, k),
                                   lambda d, q, px: cached(d, q, "prev-full").reshape(-1, 3)[px], temporal_gradient_sparse_host)

        def guides(d, d_prev, p, p_prev):
            motion, pz, _ = numpy_motion(oracle, d, d_prev, p, p_prev)
            return numpy_guides(oracle, d, p), motion, pz

        def truth(k):
            p, d = frames[k][:2]
            q = p.copy()
            q.spp, q.seed = 256, 1984
            return oracle.render(d, q)[0]

        _cpu[which] = run_sequence(
            frames, render, guides, grad,
            lambda c, a, n, m, z, h: temporal_accumulate_moments_host(c, a, n, m, z, history=h, **SEQ_KW),
            lambda c, a, n, m, z, lam, h: temporal_accumulate_adaptive_host(c, a, n, m, z, lam, history=h, **SEQ_KW), truth)
    return _cpu[which]


# Measured on the CPU (oracle.render gathered at the list, numpy guide and motion rules, host twins; seed = frame number; tool
# defaults: stride 3, 3 iterations, gain 2): RMSE against the oracle at 256 spp.
#                                              noisy     plain     sparse adaptive
MEASURED_A_LAST = (0.12099, 0.26466, 0.05559)                    # frame 9: adaptive / plain 0.210
MEASURED_B_CHANGE = (0.11256, 0.34946, 0.10656)                  # frame 5, the frame of the change: adaptive / noisy 0.947
MEASURED_B_LAST = (0.10512, 0.18390, 0.03784)                    # frame 9: adaptive / plain 0.206
MEASURED_C_LAST = (0.33313, 0.09443, 0.11132)                    # frame 9: adaptive / noisy 0.334 (rows: 0.299; plain 0.283)


def test_a_still_scene_is_untouched_until_the_lights_change(oracle):
    """(a) §21's condition: before the change lambda is +0 and the adaptive outputs are the plain ones bit for bit; at frame 9
    the adaptive colour's RMSE is at most half the plain one's, and within 1.25 x the measured value."""
    seq = cpu_sequence(oracle, "a")
    for k in range(1, Q_RELIGHT_AT):
        assert (bits(seq[k]["lam"]) == 0).all(), k
    assert all(seq[k]["same"] for k in range(Q_RELIGHT_AT)), "adaptive vs plain through frame 4"
    print(f"sequence a frame {Q_RELIGHT_AT}: mean lambda {seq[Q_RELIGHT_AT]['lam'].mean():.3f}")
    assert not seq[Q_RELIGHT_AT]["same"] and seq[Q_RELIGHT_AT]["lam"].mean() > 0.5
    last = seq[-1]
    _report("a (sparse)", Q_FRAMES - 1, last)
    assert last["adaptive"] <= 0.5 * last["plain"]
    assert last["adaptive"] <= MARGIN * MEASURED_A_LAST[2]


def test_a_moving_scene_follows_the_light_change(oracle):
    """(b) §21's conditions: adaptive <= 1.25 x noisy in the frame of the change, at most half the plain RMSE at frame 9."""
    seq = cpu_sequence(oracle, "b")
    change, last = seq[Q_RELIGHT_AT], seq[-1]
    _report("b (sparse)", Q_RELIGHT_AT, change)
    _report("b (sparse)", Q_FRAMES - 1, last)
    assert change["adaptive"] <= 1.25 * change["noisy"]
    assert last["adaptive"] <= 0.5 * last["plain"]
    assert last["adaptive"] <= MARGIN * MEASURED_B_LAST[2]
    assert change["adaptive"] <= MARGIN * MEASURED_B_CHANGE[2]


def test_the_price_without_a_light_change(oracle):
    """(c) §21's condition: adaptive / noisy <= 0.75 with motion and no relight.  One pixel per tile is a noisier gradient than a
    row of three: the figure is dearer than the rows variant's and is printed beside the plain one."""
    last = cpu_sequence(oracle, "c")[-1]
    _report("c (sparse)", Q_FRAMES - 1, last)
    assert last["adaptive"] / last["noisy"] <= 0.75
    assert last["adaptive"] <= MARGIN * MEASURED_C_LAST[2]
    assert last["plain"] <= MARGIN * MEASURED_C_LAST[1]


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cbox_scene():
    ds = dev.DeviceScene(case("cbox")[1])
    yield ds
    ds.close()


@pytest.mark.gpu
def test_device_pixel_choice_equals_host_and_numpy(cbox_scene):
    """The host-pointer form, and the device-pointer form on a stream that is not the default one."""
    import torch
    stream = torch.cuda.Stream()
    for Ww, Hh, s in GRIDS:
        for seed in SEEDS:
            want = numpy_pixels(Ww, Hh, seed, s)
            assert (gradient_pixels_host(Ww, Hh, seed, stride=s) == want).all()
            assert (cbox_scene.gradient_pixels(Ww, Hh, seed, stride=s) == want).all(), (Ww, Hh, s, seed)
            out = torch.full((want.size,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            cbox_scene.gradient_pixels_into(Ww, Hh, seed, out.data_ptr(), stream=stream.cuda_stream, stride=s)
            stream.synchronize()
            assert (out.cpu().numpy() == want).all(), (Ww, Hh, s, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CORNERS))
def test_device_equals_host_and_numpy_on_corner_cases(cbox_scene, name):
    import torch
    a, px, b, kw = CORNERS[name]
    want = numpy_sparse(a, px, b, **kw)
    assert_bit_equal(temporal_gradient_sparse_host(a, px, b, **kw), want, name + ": host twin vs numpy")
    assert_bit_equal(cbox_scene.temporal_gradient_sparse(a, px, b, **kw), want, name + ": device, host pointers")
    stream = torch.cuda.Stream()
    ta, tp, tb = torch.from_numpy(a).cuda(), torch.from_numpy(px).cuda(), torch.from_numpy(b).cuda()
    out = torch.full(want.shape, -7.0, device="cuda")
    torch.cuda.synchronize()
    cbox_scene.temporal_gradient_sparse_into(a.shape[1], a.shape[0], ta.data_ptr(), tp.data_ptr(), tb.data_ptr(), out.data_ptr(),
                                             stream=stream.cuda_stream, **kw)
    stream.synchronize()
    assert_bit_equal(out.cpu().numpy(), want, name + ": device pointers on a stream")


@pytest.mark.gpu
def test_the_record_buffers_grow_and_shrink_with_the_frame(cbox_scene):
    """A small frame, a larger one, the small one again on one handle, interleaved with the rows variant that shares the
    buffers: each equals its numpy rule."""
    from test_temporal_gradient import numpy_gradient
    for seed, (Hh, Ww) in enumerate(((6, 9), (40, 130), (6, 9))):
        a, px, b = gathered(20 + seed, Hh, Ww, 3, seed)
        assert_bit_equal(cbox_scene.temporal_gradient_sparse(a, px, b), numpy_sparse(a, px, b), f"sparse {Ww}x{Hh}")
        assert (cbox_scene.gradient_pixels(Ww, Hh, seed) == px).all()
        a, rows = synthetic(30 + seed, Hh, Ww, 3)
        assert_bit_equal(cbox_scene.temporal_gradient(a, rows), numpy_gradient(a, rows), f"rows {Ww}x{Hh}")


@pytest.mark.gpu
def test_device_rejects_bad_arguments(cbox_scene):
    _argument_errors(dev.lib().pt_temporal_gradient_sparse, SPARSE_NAMES, _sparse_buffers, handle=cbox_scene._h)
    _argument_errors(dev.lib().pt_gradient_pixels, ("pixels_out",), lambda: [np.zeros(6, dtype=np.int32)], handle=cbox_scene._h, seed=3)
    none = ctypes.c_void_p(None)
    assert _call(dev.lib().pt_temporal_gradient_sparse, _params(), _sparse_buffers(), handle=none) == PT_ERR_INVALID_ARG
    assert "null scene" in dev.lib().pt_last_error().decode()
    assert _call(dev.lib().pt_gradient_pixels, _params(), [np.zeros(6, dtype=np.int32)], handle=none, seed=1) == PT_ERR_INVALID_ARG
    assert "null scene" in dev.lib().pt_last_error().decode()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cbox", "random7"])
def test_the_chain_on_one_stream_equals_the_host_twins(oracle, name):
    """§21's chain test with the sparse stages: three 2-spp frames with camera motion, a geometry update before frame 1 and a
    shading update before frame 2.  Per frame render_into, gradient_pixels_into, render_pixels_into with the previous parameters,
    temporal_gradient_sparse_into, render_guides_into (blocking, on the default stream, as the call is),
    temporal_accumulate_adaptive_into and denoise_variance_into on one stream with no host sync of ours in between; every result
    equals the host twins on the device-rendered inputs, bit for bit."""
    import torch
    from test_motion import camera_step

    from pathtracer_cuda_interactive_amd import denoise_variance_host
    hs, d0, d1 = case(name)[:3]
    Ww, Hh = (96, 72) if name == "cbox" else (64, 48)
    r0, TH, TW = dev.gradient_grid(Ww, Hh)
    p0 = hs.render_params(Ww, Hh, 2, seed=5)
    step = camera_step(oracle, name, p0, scale=0.01)
    ds = dev.DeviceScene(d0)
    try:
        stream = torch.cuda.Stream()
        s = stream.cuda_stream
        f3 = lambda: torch.zeros((Hh, Ww, 3), device="cuda")             # noqa: E731
        f1 = lambda: torch.zeros((Hh, Ww), device="cuda")                # noqa: E731
        sets = [dict(color=f3(), out=f3(), normal=f3(), depth=f1(), length=f1(), moments=torch.zeros((Hh, Ww, 2), device="cuda"))
                for _ in range(2)]
        albedo, den = f3(), f3()
        px_t = torch.zeros(TH * TW, dtype=torch.int32, device="cuda")
        res_t = torch.zeros((TH * TW, 3), device="cuda")
        motion, pz, lam_t = torch.zeros((Hh, Ww, 2), device="cuda"), f1(), torch.zeros((TH, TW), device="cuda")
        hist_np, p_prev, positive = None, p0, 0
        for k in range(3):
            p = dev.translated_params(p0, step * k)
            p.seed = 5 + k
            if k == 1:
                ds.update(d1)
            if k == 2:
                ds.update(scaled_lights(d1), geometry=False, shading=True)
            cur, old = sets[k & 1], sets[(k + 1) & 1]
            torch.cuda.synchronize()
            ds.render_into(p, cur["color"].data_ptr(), stream=s)
            if k:
                ds.gradient_pixels_into(Ww, Hh, k, px_t.data_ptr(), stream=s)
                ds.render_pixels_into(p_prev, px_t.data_ptr(), TH * TW, res_t.data_ptr(), stream=s)
                ds.temporal_gradient_sparse_into(Ww, Hh, old["color"].data_ptr(), px_t.data_ptr(), res_t.data_ptr(), lam_t.data_ptr(),
                                                 stream=s)
            ds.render_guides_into(p, p_prev, previous_geometry=True, albedo_ptr=albedo.data_ptr(), normal_ptr=cur["normal"].data_ptr(),
                                  depth_ptr=cur["depth"].data_ptr(), motion_ptr=motion.data_ptr(), prev_depth_ptr=pz.data_ptr())
            hist = [old[n].data_ptr() for n in ("out", "normal", "depth", "length", "moments")] if k else None
            ds.temporal_accumulate_adaptive_into(Ww, Hh, cur["color"].data_ptr(), albedo.data_ptr(), cur["normal"].data_ptr(),
                                                 motion.data_ptr(), pz.data_ptr(), hist, cur["out"].data_ptr(), cur["length"].data_ptr(),
                                                 cur["moments"].data_ptr(), lam_t.data_ptr(), stream=s)
            ds.denoise_variance_into(Ww, Hh, cur["out"].data_ptr(), albedo.data_ptr(), cur["normal"].data_ptr(), cur["depth"].data_ptr(),
                                     cur["moments"].data_ptr(), cur["length"].data_ptr(), den.data_ptr(), 0, stream=s)
            stream.synchronize()
            c, a, n, z, m, q = (t.cpu().numpy() for t in (cur["color"], albedo, cur["normal"], cur["depth"], motion, pz))
            assert_bit_equal(c, ds.render(p), f"{name} frame {k}: the async render")
            lam = np.zeros((TH, TW), dtype=F)
            if k:
                px, res = px_t.cpu().numpy(), res_t.cpu().numpy()
                assert (px == gradient_pixels_host(Ww, Hh, k)).all(), f"{name} frame {k}: the list vs host twin"
                assert_bit_equal(res, ds.render(p_prev).reshape(-1, 3)[px], f"{name} frame {k}: the async pixel-list render")
                lam = temporal_gradient_sparse_host(old["color"].cpu().numpy(), px, res)
                assert_bit_equal(lam_t.cpu().numpy(), lam, f"{name} frame {k}: lambda vs host twin")
                assert_bit_equal(lam, numpy_sparse(old["color"].cpu().numpy(), px, res), f"{name} frame {k}: lambda vs numpy")
                positive += int((lam > 0).sum())
            twin = temporal_accumulate_adaptive_host(c, a, n, m, q, lam, history=hist_np)
            for j, key in enumerate(("out", "length", "moments")):
                assert_bit_equal(cur[key].cpu().numpy(), twin[j], f"{name} frame {k} {key}: stream form vs host twin")
            assert_bit_equal(den.cpu().numpy(), denoise_variance_host(twin[0], a, n, z, twin[2], twin[1]), f"{name} frame {k}: denoised")
            hist_np = (twin[0], n, z, twin[1], twin[2])
            p_prev = p
        assert positive > 0, "the updates must show in lambda"
    finally:
        ds.close()


@pytest.mark.gpu
def test_a_still_scene_on_the_device():
    """The device pixel-list render equals the previous full render's pixels bit for bit, lambda is +0 at every tile, and the
    adaptive outputs are pt_temporal_accumulate_moments' bits."""
    hs, d0 = case("cbox")[:2]
    Ww, Hh = 96, 72
    ds = dev.DeviceScene(d0)
    try:
        p_prev = hs.render_params(Ww, Hh, 2, seed=5)
        p = p_prev.copy()
        p.seed = 6
        prev = ds.render(p_prev)
        px = ds.gradient_pixels(Ww, Hh, 1)
        res = ds.render_pixels(p_prev, px)
        assert_bit_equal(res, prev.reshape(-1, 3)[px], "the pixel-list render vs the pixels of the full render")
        lam = ds.temporal_gradient_sparse(prev, px, res)
        assert lam.shape == (24, 32) and (bits(lam) == 0).all()
        g0 = ds.render_guides(p_prev, p_prev)
        first = ds.temporal_accumulate_moments(prev, g0["albedo"], g0["normal"], g0["motion"], g0["prev_depth"], **SEQ_KW)
        hist = (first[0], g0["normal"], g0["depth"], first[1], first[2])
        noisy, g = ds.render(p), ds.render_guides(p, p_prev)
        plain = ds.temporal_accumulate_moments(noisy, g["albedo"], g["normal"], g["motion"], g["prev_depth"], history=hist, **SEQ_KW)
        adapt = ds.temporal_accumulate_adaptive(noisy, g["albedo"], g["normal"], g["motion"], g["prev_depth"], lam, history=hist, **SEQ_KW)
        assert (plain[1] > 1).mean() > 0.5
        for k, what in enumerate(("colour", "length", "moments")):
            assert_bit_equal(adapt[k], plain[k], what + ": adaptive with lambda +0 vs pt_temporal_accumulate_moments")
    finally:
        ds.close()


@pytest.mark.gpu
def test_sequence_b_on_the_device_gives_the_cpu_figures(oracle):
    """Sequence (b) with every stage on the device (blocking forms, through DeviceScene.update); the truth is the device's own
    256-spp render, which is the oracle's bit for bit.  The RMSE figures are the CPU's MEASURED_B_* to every printed digit."""
    frames = sequence_frames(oracle, **SEQUENCES["b"])
    ds = dev.DeviceScene(frames[0][1])
    try:
        def guides(d, d_prev, p, p_prev):
            g = ds.render_guides(p, p_prev, previous_geometry=True)
            return g, g["motion"], g["prev_depth"]

        def truth(k):
            q = frames[k][0].copy()
            q.spp, q.seed = 256, 1984
            return ds.render(q)

        def update(d_edit):
            ds.update(d_edit, geometry=True, shading=True)

        render, grad = chain_hooks(lambda d, p: ds.render(p), lambda k: ds.gradient_pixels(96, 72, k),
                                   lambda d, q, px: ds.render_pixels(q, px), ds.temporal_gradient_sparse)
        seq = run_sequence(
            frames, render, guides, grad,
            lambda c, a, n, m, z, h: ds.temporal_accumulate_moments(c, a, n, m, z, history=h, **SEQ_KW),
            lambda c, a, n, m, z, lam, h: ds.temporal_accumulate_adaptive(c, a, n, m, z, lam, history=h, **SEQ_KW), truth, update)
    finally:
        ds.close()
    for k, measured in ((Q_RELIGHT_AT, MEASURED_B_CHANGE), (Q_FRAMES - 1, MEASURED_B_LAST)):
        _report("b (sparse, device)", k, seq[k])
        for key, want in zip(("noisy", "plain", "adaptive"), measured):
            assert abs(seq[k][key] - want) < 5e-5, (k, key, seq[k][key], want)
