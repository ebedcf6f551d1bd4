"""pt_trace_rays: closest-hit and any-hit queries for explicit rays on the lane-refilling query kernel (include/pt_api.h,
DESIGN.md §24).

Closest mode must write what pt_debug_intersect writes and what the CPU oracle's intersect returns, bit for bit, whatever the
grid: the tests run it on one block (every lane refills many times) and on the automatic grid.  Any mode is, by definition,
(closest prim >= 0) of the same ray."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
from conftest import GOLDEN, REPO, assert_bit_equal, load_scene
from test_aov import scene

from pathtracer_cuda_interactive_amd import (PT_ERR_INVALID_ARG, PT_QUERY_ANY, PT_QUERY_CLOSEST, PT_TRAVERSAL_DEFAULT, PT_TRAVERSAL_EXACT,
                                             PT_TRAVERSAL_PRUNED, _build)
from pathtracer_cuda_interactive_amd import device as dev

RAYS = sorted(glob.glob(os.path.join(GOLDEN, "rays", "*.npz")))
SCENES = ["bunny", "cbox", "scene1", "random1"]
N_RANDOM = 20000


# ---- CPU --------------------------------------------------------------------------------------------------------------

def test_library_and_binding_export_the_two_entry_points():
    lib = C.CDLL(_build.HIP_LIB)
    for name in ("pt_trace_rays", "pt_render_guides_async"):
        assert hasattr(lib, name), f"libpt_hip.so does not export {name}"
        assert name in dev.EXPORTS


def test_query_modes_match_the_header():
    text = open(os.path.join(REPO, "include", "pt_api.h")).read()
    m = re.search(r"enum\s*\{\s*PT_QUERY_CLOSEST\s*=\s*(\d+)\s*,\s*PT_QUERY_ANY\s*=\s*(\d+)\s*\}", text)
    assert m, "pt_api.h declares no PT_QUERY_* enum"
    assert (PT_QUERY_CLOSEST, PT_QUERY_ANY) == (int(m.group(1)), int(m.group(2))) == (0, 1)


# ---- rays and their reference, made once ----------------------------------------------------------------------------------

_ray_sets = {}


def random_rays(n=N_RANDOM):
    """test_many_random_rays_against_live_oracle's generator; then, so that the caller's-tree path runs inside refilling waves,
    every 16th ray gets one zero direction component and every other 16th is axis-aligned and aimed through its target."""
    rng = np.random.default_rng(5)
    o = (rng.standard_normal((n, 3)) * 2).astype(np.float32)
    t = (rng.standard_normal((n, 3)) * 0.7).astype(np.float32)
    dirs = t - o
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    dirs = dirs.astype(np.float32)
    k = np.arange(n)
    flat = np.nonzero(k % 16 == 3)[0]
    dirs[flat, flat % 3] = 0.0
    dirs[flat] /= np.linalg.norm(dirs[flat], axis=1, keepdims=True)
    axis = np.nonzero(k % 16 == 11)[0]
    a = np.zeros((len(axis), 3), dtype=np.float32)
    a[np.arange(len(axis)), axis % 3] = np.where((axis // 3) % 2 == 0, 1.0, -1.0)
    dirs[axis] = a
    o[axis] = t[axis] - 3.0 * a
    return np.concatenate([o, dirs, np.full((n, 1), 1e-4, np.float32), np.full((n, 1), 3.0e38, np.float32)], axis=1).astype(np.float32)


def ray_set(oracle, name):
    """(desc, rays [n, 8], the oracle's tuv, the oracle's prim) of a scene."""
    if name not in _ray_sets:
        _, d = scene(name)
        rays = random_rays()
        tuv, prim = oracle.intersect(d, rays)
        _ray_sets[name] = (d, rays, tuv, prim)
    return _ray_sets[name]


def test_the_ray_sets_hit_miss_and_hold_zero_components(oracle):
    for name in SCENES:
        _, rays, _, prim = ray_set(oracle, name)
        assert (prim >= 0).mean() > 0.05 and (prim < 0).mean() > 0.05, name
        zero = (rays[:, 3:6] == 0).any(axis=1)
        assert zero.sum() >= N_RANDOM // 10 and (prim[zero] >= 0).any(), name
        assert ((rays[:, 3:6] == 0).sum(axis=1) == 2).sum() >= N_RANDOM // 20


def any_rays(rays, tuv, prim):
    """Three copies: tfar as given, 0.5 t and 2 t of the closest hit (a miss keeps its tfar)."""
    hit = prim >= 0
    out = []
    for f in (None, 0.5, 2.0):
        r = rays.copy()
        if f is not None:
            r[hit, 7] = np.float32(f) * tuv[hit, 0]
        out.append(r)
    return np.concatenate(out, axis=0)


# ---- GPU --------------------------------------------------------------------------------------------------------------

def _open(d, **opts):
    ds = dev.DeviceScene(d)
    for key, v in opts.items():
        ds.set_option(key, v)
    return ds


@pytest.mark.gpu
@pytest.mark.parametrize("path", RAYS, ids=os.path.basename)
def test_closest_mode_reproduces_the_ray_kats(path):
    name = os.path.basename(path)[:-4]
    _, d = load_scene(name)
    z = np.load(path)
    for fast_tree in (1, 0):
        ds = _open(d, fast_tree=fast_tree)
        try:
            for trav in (PT_TRAVERSAL_EXACT, PT_TRAVERSAL_PRUNED):
                tuv, prim = ds.trace_rays(z["rays"], traversal=trav)
                what = f"{name} fast_tree={fast_tree} trav {trav}"
                assert (prim == z["prim"]).all(), f"{what}: {(prim != z['prim']).sum()} prims differ"
                assert_bit_equal(tuv, z["tuv"], what)
        finally:
            ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_random_rays_equal_the_oracle_and_debug_intersect(oracle, name):
    d, rays, tuv, prim = ray_set(oracle, name)
    for fast_tree in (1, 0):
        ds = _open(d, fast_tree=fast_tree)
        try:
            t_dbg, p_dbg = ds.intersect(rays)
            for blocks in (1, 0):
                ds.set_option("query_blocks", blocks)
                t2, p2 = ds.trace_rays(rays, traversal=PT_TRAVERSAL_DEFAULT)
                what = f"{name} fast_tree={fast_tree} query_blocks={blocks}"
                assert ds.info("query_grid") == 1 if blocks else ds.info("query_grid") >= 1
                assert (p2 == prim).all(), f"{what}: {(p2 != prim).sum()} prims differ from the oracle"
                assert_bit_equal(t2, tuv, what + " against the oracle")
                assert (p2 == p_dbg).all()
                assert_bit_equal(t2, t_dbg, what + " against pt_debug_intersect")
        finally:
            ds.close()


@pytest.mark.gpu
def test_prefixes_of_the_ray_list_and_untouched_tails(oracle):
    import torch
    d, rays, tuv, prim = ray_set(oracle, "bunny")
    ds = _open(d)
    try:
        chunk = ds.info("query_chunk")
        assert chunk >= 64 and chunk % 64 == 0
        total = 1000 + 8
        tuv, prim = ds.trace_rays(rays[:total])               # the full result (the oracle's: the test above)
        d_rays = torch.from_numpy(rays[:total]).cuda()
        for blocks in (1, 0):
            ds.set_option("query_blocks", blocks)
            for n in (0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 1000):
                t_out = torch.full((total, 3), -7.0, device="cuda")
                p_out = torch.full((total,), -7, device="cuda", dtype=torch.int32)
                ds.trace_rays_into(d_rays.data_ptr(), n, t_out.data_ptr(), p_out.data_ptr())
                torch.cuda.synchronize()
                t_np, p_np = t_out.cpu().numpy(), p_out.cpu().numpy()
                what = f"n={n} query_blocks={blocks}"
                assert (p_np[:n] == prim[:n]).all(), what
                assert_bit_equal(t_np[:n], tuv[:n], what)
                assert (p_np[n:] == -7).all() and (t_np[n:] == -7.0).all(), what + ": output past n was written"
    finally:
        ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_any_mode_is_closest_prim_nonnegative(oracle, name):
    d, rays, tuv, prim = ray_set(oracle, name)
    three = any_rays(rays, tuv, prim)
    # able to fail either way: the set holds both answers (CPU)
    _, p_or = oracle.intersect(d, three)
    assert (p_or >= 0).sum() > 100 and (p_or < 0).sum() > 100
    n = len(rays)
    assert ((p_or[:n] >= 0) & (p_or[n:2 * n] < 0)).sum() > 100, "halving tfar turns hits into misses"
    for fast_tree in (1, 0):
        ds = _open(d, fast_tree=fast_tree)
        try:
            for blocks in (1, 0):
                ds.set_option("query_blocks", blocks)
                _, p_closest = ds.trace_rays(three)
                hit = ds.trace_rays(three, mode=PT_QUERY_ANY)
                what = f"{name} fast_tree={fast_tree} query_blocks={blocks}"
                assert (p_closest == p_or).all(), what
                assert set(np.unique(hit)) <= {0, 1}
                assert np.array_equal(hit, (p_closest >= 0).astype(np.int32)), f"{what}: {(hit != (p_closest >= 0)).sum()} answers differ"
        finally:
            ds.close()


@pytest.mark.gpu
def test_device_pointers_follow_a_producer_on_a_side_stream(oracle):
    import torch
    d, rays, tuv, prim = ray_set(oracle, "bunny")
    n = len(rays)
    ds = _open(d)
    try:
        want_t, want_p = ds.trace_rays(rays)
        want_any = ds.trace_rays(rays, mode=PT_QUERY_ANY)
        src = torch.from_numpy(rays).cuda()
        work = torch.randn(2048, 2048, device="cuda")
        stream = torch.cuda.Stream()
        d_rays = torch.zeros_like(src)
        t_out = torch.full((n, 3), -7.0, device="cuda")
        p_out = torch.full((n,), -7, device="cuda", dtype=torch.int32)
        a_out = torch.full((n,), -7, device="cuda", dtype=torch.int32)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for _ in range(4):                               # the rays arrive late, behind other work of the stream
                work = work @ work * 1e-3
            d_rays.copy_(src)
            ds.trace_rays_into(d_rays.data_ptr(), n, t_out.data_ptr(), p_out.data_ptr(), stream=stream.cuda_stream)
            ds.trace_rays_into(d_rays.data_ptr(), n, 0, a_out.data_ptr(), mode=PT_QUERY_ANY, stream=stream.cuda_stream)
        stream.synchronize()
        assert (p_out.cpu().numpy() == want_p).all()
        assert_bit_equal(t_out.cpu().numpy(), want_t, "device pointers on a side stream")
        assert np.array_equal(a_out.cpu().numpy(), want_any)
    finally:
        ds.close()


@pytest.mark.gpu
def test_three_hundred_launches_on_two_streams(oracle):
    """More launches in flight than the handle has work counters: entries of the ring are reused across streams."""
    import torch
    d, rays, _, _ = ray_set(oracle, "bunny")
    n, launches = 2000, 300
    ds = _open(d)
    try:
        want_t, want_p = ds.trace_rays(rays[:n])
        d_rays = torch.from_numpy(rays[:n]).cuda()
        t_out = torch.full((launches, n, 3), -7.0, device="cuda")
        p_out = torch.full((launches, n), -7, device="cuda", dtype=torch.int32)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for k in range(launches):
            ds.trace_rays_into(d_rays.data_ptr(), n, t_out[k].data_ptr(), p_out[k].data_ptr(), stream=streams[k % 2].cuda_stream)
        for s in streams:
            s.synchronize()
        p_np, t_np = p_out.cpu().numpy(), t_out.cpu().numpy()
        assert (p_np == want_p[None]).all(), f"{(p_np != want_p[None]).any(axis=1).sum()} launches differ"
        assert_bit_equal(t_np, np.broadcast_to(want_t, t_np.shape), "300 launches on two streams")
    finally:
        ds.close()


@pytest.mark.gpu
def test_refusals_name_the_argument_and_leave_the_handle_alone(oracle):
    hs, d = load_scene("cbox")
    p = hs.render_params(64, 48, 2)
    _, rays, _, _ = ray_set(oracle, "cbox")
    rays = np.ascontiguousarray(rays[:64])
    tuv = np.full((64, 3), -7.0, dtype=np.float32)
    prim = np.full(64, -7, dtype=np.int32)
    R, T, P = (a.ctypes.data_as(C.c_void_p) for a in (rays, tuv, prim))
    ds = _open(d)
    try:
        before = ds.render(p)
        L = dev.lib()

        def call(r, n, mode, trav, t, q):
            return L.pt_trace_rays(ds._h, r, n, mode, trav, t, q, 0, None), L.pt_last_error().decode()

        for args, word in (((R, -1, PT_QUERY_CLOSEST, 0, T, P), " n "), ((R, (1 << 30) + 1, PT_QUERY_CLOSEST, 0, T, P), " n "),
                           ((None, 64, PT_QUERY_CLOSEST, 0, T, P), "rays"), ((R, 64, PT_QUERY_CLOSEST, 0, T, None), "out_prim"),
                           ((R, 64, PT_QUERY_ANY, 0, None, None), "out_prim"), ((R, 64, PT_QUERY_CLOSEST, 0, None, P), "out_tuv"),
                           ((R, 64, 2, 0, T, P), "mode"), ((R, 64, -1, 0, T, P), "mode"), ((R, 64, PT_QUERY_CLOSEST, 3, T, P), "traversal"),
                           ((R, 64, PT_QUERY_ANY, -1, None, P), "traversal")):
            rc, msg = call(*args)
            assert rc == PT_ERR_INVALID_ARG and "pt_trace_rays" in msg and word in msg, (args[1:4], rc, msg)
        assert (tuv == -7.0).all() and (prim == -7).all()
        # n == 0: PT_OK whatever the pointers, nothing written
        assert call(None, 0, PT_QUERY_CLOSEST, 0, None, None)[0] == 0
        assert call(R, 0, PT_QUERY_ANY, 0, T, P)[0] == 0
        assert (tuv == -7.0).all() and (prim == -7).all()
        # any mode takes a NULL out_tuv
        assert call(R, 64, PT_QUERY_ANY, 0, None, P)[0] == 0 and set(np.unique(prim)) <= {0, 1}
        assert_bit_equal(ds.render(p), before, "pt_render after refused pt_trace_rays calls")
    finally:
        ds.close()


@pytest.mark.gpu
def test_queries_leave_renders_counters_and_info_alone(oracle):
    d, rays, _, _ = ray_set(oracle, "cbox")
    hs, _ = load_scene("cbox")
    p = hs.render_params(64, 48, 4)
    ds = _open(d)
    try:
        before = ds.render(p)
        c0, v0, g0 = ds.counters(), ds.info("trace_variant"), ds.info("grid")
        ds.trace_rays(rays)
        ds.trace_rays(rays, mode=PT_QUERY_ANY, traversal=PT_TRAVERSAL_PRUNED)
        c1 = ds.counters()
        assert (c1.paths, c1.segments, c1.node_visits, c1.leaf_tests) == (c0.paths, c0.segments, c0.node_visits, c0.leaf_tests)
        assert ds.info("trace_variant") == v0 and ds.info("grid") == g0
        assert_bit_equal(ds.render(p), before, "pt_render after pt_trace_rays")
    finally:
        ds.close()
