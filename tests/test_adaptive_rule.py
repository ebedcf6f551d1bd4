"""pt_render_adaptive's stopping rule on every pixel and parameter (include/pt_api.h), against tests/adaptive_reference.py.

Every case compares all three outputs on all pixels: spp_map equal, fb bit-equal, err_map inside the float32 interval the
reference derives from the true quantile (tests/test_adaptive_reference.py checks on the CPU that for every case here the
interval is one float and no pixel's count is in doubt).  "A NaN never stops" is not tested: no valid scene produces
non-finite radiance."""
import ctypes as C

import adaptive_cases as ac
import adaptive_reference as ar
import numpy as np
import pytest
import torch
from conftest import assert_bit_equal, bits

pytestmark = pytest.mark.gpu


def _open(scene, **opts):
    from pathtracer_cuda_interactive_amd import device as dev
    ds = dev.DeviceScene(ac.scene(scene)[1])
    for k, v in opts.items():
        ds.set_option(k, v)
    return ds


@pytest.fixture(scope="module")
def handles():
    """One handle per scene for the whole module: every case also runs behind whatever the cases before it left in the buffers."""
    open_ = {}

    def get(scene):
        if scene not in open_:
            open_[scene] = _open(scene)
        return open_[scene]
    yield get
    for ds in open_.values():
        ds.close()


def _kw(rule):
    return dict(max_error=rule.max_error, batch_spp=rule.batch, max_spp=rule.max_spp, p_value=rule.p_value,
                min_luminance=rule.min_luminance)


def _assert_outputs(got, E, what):
    fb, spp, err = got
    assert (spp.reshape(-1) == E.n).all(), (what, np.nonzero(spp.reshape(-1) != E.n)[0][:8])
    e = bits(err).reshape(-1)                      # non-negative floats order as their bits do; a NaN or a -0 falls outside
    bad = (e < bits(E.err_lo)) | (e > bits(E.err_hi))
    assert not bad.any(), (what, np.nonzero(bad)[0][:8], err.reshape(-1)[bad][:8], E.err_lo[bad][:8], E.err_hi[bad][:8])
    assert_bit_equal(fb.reshape(-1, 3), E.fb, f"{what}: fb")


def _assert_call(ds, got, E, what):
    """The outputs of the handle's last call, its path counter and its rounds."""
    _assert_outputs(got, E, what)
    assert ds.counters().paths == int(E.n.sum()), what
    assert ds.info("adaptive_rounds") == E.rounds, what


def _run_case(ds, oracle, frame, rule, what, scratch_bytes=None):
    p, E = ac.reference(oracle, frame, rule, scratch_bytes)
    got = ds.render_adaptive(p, **_kw(rule))
    _assert_call(ds, got, E, what)
    return got, E


# ---- 1: every pixel, every parameter --------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ac.SCENES)
@pytest.mark.parametrize("i", range(len(ac.RULES)))
def test_every_pixel_every_parameter(oracle, handles, scene, i):
    _run_case(handles(scene), oracle, ac.Frame(scene), ac.RULES[i], f"{scene} {ac.RULES[i]}")


@pytest.mark.parametrize("name", list(ac.VARIANTS))
def test_every_pixel_render_parameters(oracle, handles, name):
    """PT_RENDER_NEE, pruned traversal, the defaults batch_spp = max_spp = 0 at spp = 1, an explicit stream_stride of twice
    max_spp, a row selection."""
    frame, rule = ac.VARIANTS[name]
    if name == "pruned":
        return _pruned_case(handles(frame.scene), frame, rule)
    (_, spp, _), E = _run_case(handles(frame.scene), oracle, frame, rule, name)
    if name == "defaults":
        assert E.rounds > 1 and spp.min() > 1 and ar.checkpoints(*rule[:3]) == list(range(1, 33))
    if name == "rows":
        assert spp.shape == (len(range(*frame.rows)), frame.w)


def _pruned_case(ds, frame, rule):
    """The oracle never prunes, and a pruned frame may differ from the exact one by a rounding flip: the rule is
    compared on the samples the pruned kernel produced, pt_render at spp = 1 and sample_offset = k."""
    p = ac.params(frame, rule.spp)
    s = np.zeros((frame.w * frame.h, rule.max_spp, 3), np.float32)
    for k in range(rule.max_spp):
        q = p.copy()
        q.spp, q.sample_offset, q.stream_stride = 1, k, rule.max_spp
        s[:, k] = ds.render(q).reshape(-1, 3)
    E = ar.expected(s, *rule)
    assert E.decided.all() and (bits(E.err_lo) == bits(E.err_hi)).all() and len(np.unique(E.n)) >= 4
    _assert_call(ds, ds.render_adaptive(p, **_kw(rule)), E, "pruned")


# ---- 2: the edges of the rule ---------------------------------------------------------------------------------------------

def test_a_huge_max_error_stops_everyone_at_once(oracle, handles):
    frame, rule = ac.ALL_STOP
    (_, spp, err), E = _run_case(handles(frame.scene), oracle, frame, rule, "all stop")
    assert E.rounds == 1 and (spp == rule.spp).all() and (err <= np.float32(rule.max_error)).all()


def test_a_tiny_max_error_runs_everyone_to_max_spp(oracle, handles):
    frame, rule = ac.NONE_STOP
    (_, spp, err), E = _run_case(handles(frame.scene), oracle, frame, rule, "none stops")
    assert ((err > np.float32(rule.max_error)) == (spp == rule.max_spp)).all()
    assert (bits(err)[spp < rule.max_spp] == 0).all()           # what stopped early had a variance of exactly zero


@pytest.mark.parametrize("k", range(len(ac.BLACK)))
def test_black_pixels_stop_with_a_zero_error(oracle, handles, k):
    frame, rule = ac.BLACK[k]
    assert rule.min_luminance == 0
    (fb, spp, err), E = _run_case(handles(frame.scene), oracle, frame, rule, f"black {rule}")
    black = (ac.frame_samples(oracle, frame, rule.max_spp) == 0).all(axis=(1, 2)).reshape(spp.shape)
    first = [c for c in ar.checkpoints(*rule[:3]) if c > 1][0]
    assert black.sum() >= 100
    assert (spp[black] == first).all() and (bits(err)[black] == 0).all() and (bits(fb)[black] == 0).all()


# ---- 3: call forms --------------------------------------------------------------------------------------------------------

def _call(ds, p, rule, fb, spp, err, on_device):
    from pathtracer_cuda_interactive_amd import device as dev
    a = dev.DeviceScene.adaptive_params(**_kw(rule))
    rc = dev.lib().pt_render_adaptive(ds._h, C.byref(p), C.byref(a), C.c_void_p(fb), C.c_void_p(spp), C.c_void_p(err), on_device)
    assert rc == 0, rc


def test_call_forms_agree(oracle, handles):
    frame, rule = ac.FORMS
    ds = handles(frame.scene)
    p, E = ac.reference(oracle, frame, rule)
    want = ds.render_adaptive(p, **_kw(rule))
    _assert_outputs(want, E, "host pointers")
    shape = want[1].shape
    for with_spp in (True, False):
        for with_err in (True, False):
            what = f"spp_map {with_spp} err_map {with_err}"
            # host pointers
            fb = np.full(shape + (3,), -1.0, np.float32)
            spp = np.full(shape, -7, np.int32)
            err = np.full(shape, -1.0, np.float32)
            _call(ds, p, rule, fb.ctypes.data, spp.ctypes.data if with_spp else None, err.ctypes.data if with_err else None, 0)
            assert_bit_equal(fb, want[0], f"host, {what}: fb")
            assert (spp == (want[1] if with_spp else -7)).all(), what
            assert_bit_equal(err, want[2] if with_err else np.full(shape, -1.0, np.float32), f"host, {what}: err_map")
            # device pointers
            fb_d = torch.full(shape + (3,), -1.0, dtype=torch.float32, device="cuda")
            spp_d = torch.full(shape, -7, dtype=torch.int32, device="cuda")
            err_d = torch.full(shape, -1.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            if with_spp and with_err:
                ds.render_adaptive_into(p, fb_d.data_ptr(), spp_d.data_ptr(), err_d.data_ptr(), **_kw(rule))
            else:
                _call(ds, p, rule, fb_d.data_ptr(), spp_d.data_ptr() if with_spp else None, err_d.data_ptr() if with_err else None, 1)
            assert ds.counters().paths == int(E.n.sum()), what
            assert_bit_equal(fb_d.cpu().numpy(), want[0], f"device, {what}: fb")
            assert (spp_d.cpu().numpy() == (want[1] if with_spp else -7)).all(), what
            assert_bit_equal(err_d.cpu().numpy(), want[2] if with_err else np.full(shape, -1.0, np.float32), f"device, {what}: err_map")


# ---- 4: list sizes --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", ac.LIST_SIZES)
def test_list_of_k_pixels(oracle, handles, k):
    """Exactly k pixels continue after round 0: the wave-level compaction at 0, 1, one below / at / above a wave and a block.
    Twice on one handle: the list order is free and no output may depend on it."""
    rule = ac.list_case(oracle, k)
    ds = handles(ac.LIST_FRAME.scene)
    first, E = _run_case(ds, oracle, ac.LIST_FRAME, rule, f"k = {k}")
    assert int((E.n > rule.spp).sum()) == k and (E.rounds == 1) == (k == 0)
    again, _ = _run_case(ds, oracle, ac.LIST_FRAME, rule, f"k = {k}, again")
    for a, b in zip(first, again):
        assert (a.view(np.uint32) == b.view(np.uint32)).all(), k


@pytest.mark.parametrize("name", list(ac.SMALL_FRAMES))
def test_small_frames(oracle, handles, name):
    frame, rule = ac.SMALL_FRAMES[name]
    ds = handles(frame.scene)
    first, E = _run_case(ds, oracle, frame, rule, name)
    again, _ = _run_case(ds, oracle, frame, rule, name + ", again")
    for a, b in zip(first, again):
        assert (a.view(np.uint32) == b.view(np.uint32)).all(), name


# ---- 5: passes ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per_pixel", [True, False], ids=["one-sample-of-the-frame", "16-bytes"])
def test_passes_follow_the_shrinking_list(oracle, per_pixel):
    """scratch_bytes = 16 * npix: round 0 runs one sample per pass, later rounds more as the list shrinks; 16: one everywhere."""
    frame, rule = ac.PASSES
    scratch = 16 * frame.w * frame.h if per_pixel else 16
    ds = _open(frame.scene, scratch_bytes=scratch)
    try:
        _, E = _run_case(ds, oracle, frame, rule, f"scratch_bytes {scratch}", scratch)
        assert ds.info("passes") == E.passes
        assert E.passes > E.rounds
        if per_pixel:
            assert E.passes < ar.checkpoints(*rule[:3])[E.rounds - 1]
    finally:
        ds.close()


IN_FLIGHT = (640, 480, 128)          # width, height, spp of the frame an adaptive call runs behind

# ---- 6: one handle, many calls --------------------------------------------------------------------------------------------

def test_one_handle_many_calls(oracle):
    """Frames of 40 x 30, 8 x 4, 64 x 48 and 40 x 30 again under other parameters: the buffers grow and are reused, and no stale
    sum, moment or list entry may show; a plain render gives the same bits before and after."""
    scene = ac.SEQUENCE[0][0].scene
    d = ac.scene(scene)[1]
    q = ac.params(ac.Frame(scene, 56, 40), 6)
    want, _ = oracle.render(d, q)
    ds = _open(scene)
    try:
        assert_bit_equal(ds.render(q), want, "plain render before")
        for frame, rule in ac.SEQUENCE:
            assert frame.scene == scene
            _run_case(ds, oracle, frame, rule, f"{frame.w} x {frame.h} {rule}")
        assert_bit_equal(ds.render(q), want, "plain render after")
    finally:
        ds.close()


def test_behind_a_frame_in_flight(oracle):
    """An adaptive call entered directly behind a pt_render_async that is still running on a side stream, two frames in flight:
    both frames are right.  Everything the host computes comes before; the frame in flight (about 2 ms of GPU work, three times
    an adaptive call alone) is queried once, microseconds before the adaptive call is entered, and must still be running then.
    A query after the call shows nothing: the adaptive rounds get their compute units as that frame drains, and the call returns
    only some ten microseconds before the frame is done."""
    frame, rule = ac.OVERLAP
    d = ac.scene(frame.scene)[1]
    q = ac.params(ac.Frame(frame.scene, *IN_FLIGHT[:2]), IN_FLIGHT[2])
    p, E = ac.reference(oracle, frame, rule)                         # everything the host has to compute comes first
    kw = _kw(rule)
    ds = _open(frame.scene, frames_in_flight=2)
    try:
        want = ds.render(q)
        rows = ac.params(ac.Frame(frame.scene, *IN_FLIGHT[:2], rows=(0, IN_FLIGHT[1], IN_FLIGHT[1] // 2 - 1)), IN_FLIGHT[2])
        assert_bit_equal(want[::IN_FLIGHT[1] // 2 - 1], oracle.render(d, rows)[0], "the blocking frame, three rows of it")
        _assert_call(ds, ds.render_adaptive(p, **kw), E, "alone")
        stream = torch.cuda.Stream()
        out = torch.zeros(want.shape, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(2):
            ds.render_into(q, out.data_ptr(), stream=stream.cuda_stream)
            busy = not stream.query()
            got = ds.render_adaptive(p, **kw)
            _assert_call(ds, got, E, "behind a frame in flight")
            stream.synchronize()
            assert_bit_equal(out.cpu().numpy(), want, "the frame in flight")
            assert busy, "the side-stream frame had drained before the adaptive call was entered"
            out.zero_()
            torch.cuda.synchronize()
    finally:
        ds.close()
