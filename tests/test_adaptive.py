"""pt_render_adaptive: per-pixel sample counts from a noise target (include/pt_api.h).

A pixel that stops after n samples holds exactly what pt_render and the CPU oracle give it at spp = n with the same
stream stride, so every output is pinned against the oracle bit for bit; the stopping rule is recomputed in numpy."""
import ctypes
import os
import re
import socket
import subprocess
import sys

import adaptive_reference as ar
import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from adaptive_reference import checkpoints as _checkpoints
from conftest import REPO, SCENES, TESTS, assert_bit_equal, bits, load_scene, random_scene

from pathtracer_cuda_interactive_amd import (PT_BVH_SORT_REFERENCE, PT_ERR_INVALID_ARG, PT_RENDER_NEE, PT_TRAVERSAL_EXACT,
                                             PT_TRAVERSAL_PRUNED, PtError)
from pathtracer_cuda_interactive_amd import ctypes_defs as cd

# ---- CPU --------------------------------------------------------------------------------------------------------------

def test_adaptive_params_match_the_header():
    text = open(os.path.join(REPO, "include", "pt_api.h")).read()
    body = re.search(r"typedef struct pt_adaptive_params \{(.*?)\} pt_adaptive_params;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|float)\s+([a-z_]+)\s*;", body)
    assert [n for _, n in fields] == [n for n, _ in cd.PtAdaptiveParams._fields_]
    size = {"int32_t": 4, "float": 4}
    off = 0
    for (ty, name), (_, cty) in zip(fields, cd.PtAdaptiveParams._fields_):
        assert getattr(cd.PtAdaptiveParams, name).offset == off, name
        assert ctypes.sizeof(cty) == size[ty], name
        off += size[ty]
    assert ctypes.sizeof(cd.PtAdaptiveParams) == off == 20


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _band_value(j, W):
    """What a stub rank renders for image row j: rgb, spp (an integer, as float) and err — all distinct per pixel."""
    i = np.arange(W, dtype=np.float32)
    return np.stack([j * 1000.0 + i, j * 1000.0 + i + 0.25, -(j * 1000.0 + i), 4.0 * (1 + (j + i) % 16),
                     (j + 1) * 1e-3 + i * 1e-6], axis=1).astype(np.float32)


def _gather_worker(rank, world, port, H, W, out_path):
    for p in (REPO, TESTS):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from pathtracer_cuda_interactive_amd import distributed as D
    from pathtracer_cuda_interactive_amd.ctypes_defs import PtRenderParams
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        params = PtRenderParams()
        params.width, params.height, params.spp = W, H, 4

        def render_rows(q):
            assert (q.row_begin, q.row_stride) == (rank, world)
            rows = list(range(q.row_begin, q.height, q.row_stride))
            return torch.from_numpy(np.stack([_band_value(j, W) for j in rows]) if rows else np.zeros((0, W, 5), np.float32))
        frame = D.render_sharded(render_rows, params)
        if rank == 0:
            np.save(out_path, frame.numpy())
        else:
            assert frame is None
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,H", [(2, 6), (3, 7), (3, 9)])
def test_five_channel_bands_assemble(tmp_path, world, H):
    W = 5
    out = str(tmp_path / "frame.npy")
    mp.spawn(_gather_worker, args=(world, _free_port(), H, W, out), nprocs=world, join=True)
    got = np.load(out)
    want = np.stack([_band_value(j, W) for j in range(H)])
    assert got.shape == (H, W, 5)
    assert_bit_equal(got, want, "assembled rgb/spp/err")
    assert (got[..., 3].astype(np.int32) == want[..., 3]).all()


# ---- GPU --------------------------------------------------------------------------------------------------------------

def _scene(name):
    if name.startswith("random"):
        hs = random_scene(int(name[6:]))
        return hs, hs.finalize(PT_BVH_SORT_REFERENCE)
    return load_scene(name)


def _open(d, **opts):
    from pathtracer_cuda_interactive_amd import device as dev
    ds = dev.DeviceScene(d)
    for k, v in opts.items():
        ds.set_option(k, v)
    return ds


def _oracle_groups(oracle, d, p, spp_map, rows, max_spp):
    """The oracle's image at the selected rows `rows` (indices into the frame), each pixel rendered at its own spp_map."""
    out = np.zeros((len(rows), p.width, 3), np.float32)
    sub = spp_map[rows]
    for n in np.unique(sub):
        rr, ii = np.nonzero(sub == n)
        q = p.copy()
        q.spp, q.stream_stride, q.sample_offset = int(n), int(max_spp), 0
        xy = np.stack([ii, np.asarray(rows)[rr]], axis=1)
        img, _ = oracle.render_pixels(d, q, xy)
        out[rr, ii] = img
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cbox", "scene1", "bunny", "random1", "random2"])
def test_max_spp_equal_to_spp_is_pt_render(name):
    hs, d = _scene(name)
    ds = _open(d)
    try:
        for trav, flags in ((PT_TRAVERSAL_EXACT, 0), (PT_TRAVERSAL_PRUNED, 0), (PT_TRAVERSAL_EXACT, PT_RENDER_NEE)):
            p = hs.render_params(64, 48, 4)
            p.traversal, p.flags = trav, flags
            img, spp, err = ds.render_adaptive(p, 0.01, max_spp=4)
            q = p.copy()
            q.stream_stride = 4
            assert_bit_equal(img, ds.render(q), f"{name} traversal {trav} flags {flags}")
            assert (spp == 4).all()
            assert ds.info("adaptive_rounds") == 1
    finally:
        ds.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,w,h,rows", [("random3", 64, 48, None), ("scene1", 160, 120, None),
                                           ("cbox", 640, 480, [0, 97, 240, 333, 479]), ("bunny", 640, 480, [150, 260, 371])])
def test_bit_exact_against_the_oracle(oracle, name, w, h, rows):
    hs, d = _scene(name)
    p = hs.render_params(w, h, 4)
    ds = _open(d)
    try:
        img, spp, err = ds.render_adaptive(p, 0.3, batch_spp=4, max_spp=64)
        c = ds.counters()
    finally:
        ds.close()
    assert len(np.unique(spp)) >= 3, np.unique(spp)
    assert c.paths == int(spp.sum())
    rows = list(range(h)) if rows is None else rows
    want = _oracle_groups(oracle, d, p, spp, rows, 64)
    assert_bit_equal(img[rows], want, f"{name} {w}x{h} adaptive vs oracle")


@pytest.mark.gpu
def test_stopping_rule_matches_numpy(oracle):
    """Every pixel of the frame against tests/adaptive_reference.py, under the quantile of the p_value the library is handed:
    device.py's default 0.05 reaches it as float32(0.05)."""
    hs, d = load_scene("scene1")
    w, h, spp, batch, max_spp, max_error, min_lum = 160, 120, 4, 4, 64, 0.2, 0.01
    p = hs.render_params(w, h, spp)
    ds = _open(d)
    try:
        _, spp_map, err_map = ds.render_adaptive(p, max_error, batch_spp=batch, max_spp=max_spp, min_luminance=min_lum)
    finally:
        ds.close()
    E = ar.expected(ar.samples(oracle, d, p, max_spp, max_spp), spp, batch, max_spp, max_error, min_lum, np.float32(0.05))
    ok = E.decided
    # undecided needs an err within 1e-12 relative of max_error at one of 16 checkpoints of 19200 pixels: about 1e-6 expected
    assert (~ok).sum() <= 2
    got_n, got_e = spp_map.reshape(-1), bits(err_map).reshape(-1)
    assert (got_n[ok] == E.n[ok]).all(), np.nonzero(ok & (got_n != E.n))
    # err_map inside the float32 interval of the bracketed quantile (non-negative floats order as their bits do)
    assert ((got_e >= bits(E.err_lo)) & (got_e <= bits(E.err_hi)))[ok].all()
    assert len(np.unique(E.n)) >= 8


@pytest.mark.gpu
def test_invariants(oracle):
    hs, d = load_scene("scene1")
    w, h, spp, batch, max_spp, max_error = 160, 120, 4, 8, 60, 0.1
    p = hs.render_params(w, h, spp)
    ds = _open(d)
    try:
        img, spp_map, err_map = ds.render_adaptive(p, max_error, batch_spp=batch, max_spp=max_spp)
        c = ds.counters()
        rounds = ds.info("adaptive_rounds")
    finally:
        ds.close()
    cps = _checkpoints(spp, batch, max_spp)
    assert cps[-1] == 60 and cps[-2] == 52
    assert np.isin(spp_map, cps).all()
    assert (err_map[spp_map < max_spp] <= max_error).all()
    assert c.paths == int(spp_map.sum())
    assert rounds == cps.index(int(spp_map.max())) + 1
    assert c.kernel_ms > 0 and c.resolve_ms > 0
    # the background at the top of scene1: pixels whose first-round samples are all equal stop at the first checkpoint
    xy = np.stack([np.arange(w), np.zeros(w, np.int64)], axis=1)
    first = np.zeros((w, spp, 3), np.float32)
    for k in range(spp):
        q = p.copy()
        q.spp, q.sample_offset, q.stream_stride = 1, k, max_spp
        first[:, k], _ = oracle.render_pixels(d, q, xy)
    flat = (first == first[:, :1]).all(axis=(1, 2))
    assert flat.sum() >= w // 2
    assert (spp_map[0][flat] == spp).all()


@pytest.mark.gpu
def test_options_change_no_bit():
    hs, d = load_scene("scene1")
    p = hs.render_params(160, 120, 4)
    args = dict(max_error=0.15, batch_spp=4, max_spp=40)
    ds = _open(d)
    try:
        ref = ds.render_adaptive(p, **args)
        again = ds.render_adaptive(p, **args)
    finally:
        ds.close()
    for a, b in zip(ref, again):
        assert (a == b).all() if a.dtype == np.int32 else (a.view(np.uint32) == b.view(np.uint32)).all()
    assert len(np.unique(ref[1])) >= 3
    for opts in ({"kernel": 1}, {"kernel": 2}, {"kernel": 3}, {"item_order": 0}, {"item_order": 1}, {"xcd_regions": 1},
                 {"frames_in_flight": 1}, {"frames_in_flight": 3}, {"scratch_bytes": 160 * 120 * 16 * 2}):
        ds = _open(d, **opts)
        try:
            for _ in range(2):
                got = ds.render_adaptive(p, **args)
                assert_bit_equal(got[0], ref[0], f"fb {opts}")
                assert (got[1] == ref[1]).all(), opts
                assert_bit_equal(got[2], ref[2], f"err_map {opts}")
            if "scratch_bytes" in opts:
                assert ds.info("passes") > ds.info("adaptive_rounds")
        finally:
            ds.close()


@pytest.mark.gpu
def test_row_selection():
    hs, d = _scene("random5")
    p = hs.render_params(64, 48, 4)
    args = dict(max_error=0.25, batch_spp=4, max_spp=32)
    ds = _open(d)
    try:
        full = ds.render_adaptive(p, **args)
        for rb, re_, stride in ((0, 48, 3), (1, 48, 3), (2, 48, 3), (5, 30, 1), (7, 41, 4)):
            q = p.copy()
            q.row_begin, q.row_end, q.row_stride = rb, re_, stride
            part = ds.render_adaptive(q, **args)
            sel = list(range(rb, re_, stride))
            assert_bit_equal(part[0], full[0][sel], f"fb rows {rb}:{re_}:{stride}")
            assert (part[1] == full[1][sel]).all()
            assert_bit_equal(part[2], full[2][sel], f"err_map rows {rb}:{re_}:{stride}")
    finally:
        ds.close()


@pytest.mark.gpu
def test_bad_input():
    hs, d = load_scene("cbox")
    ds = _open(d)
    try:
        p = hs.render_params(32, 24, 4)
        bad = [dict(max_error=0.0), dict(max_error=-1.0), dict(max_error=float("nan")), dict(max_error=float("inf")),
               dict(max_error=0.1, p_value=1.0), dict(max_error=0.1, p_value=-0.5), dict(max_error=0.1, p_value=float("nan")),
               dict(max_error=0.1, max_spp=3), dict(max_error=0.1, max_spp=(1 << 20) + 1),
               dict(max_error=0.1, min_luminance=-1.0), dict(max_error=0.1, batch_spp=-1)]
        for kw in bad:
            with pytest.raises(PtError) as e:
                ds.render_adaptive(p, **kw)
            assert e.value.status == PT_ERR_INVALID_ARG, kw
        q = p.copy()
        q.sample_offset, q.stream_stride = 1, 1000
        with pytest.raises(PtError) as e:
            ds.render_adaptive(q, 0.1, max_spp=64)
        assert e.value.status == PT_ERR_INVALID_ARG
        q = p.copy()
        q.stream_stride = 63
        with pytest.raises(PtError) as e:
            ds.render_adaptive(q, 0.1, max_spp=64)
        assert e.value.status == PT_ERR_INVALID_ARG
        q.stream_stride = 64
        ds.render_adaptive(q, 0.1, max_spp=64)              # the smallest stride allowed
    finally:
        ds.close()


@pytest.mark.gpu
def test_cli_writes_image_and_spp_map(tmp_path):
    from pathtracer_cuda_interactive_amd import read_pfm
    out, smap = tmp_path / "a.pfm", tmp_path / "spp.pfm"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "render.py"), os.path.join(SCENES, "scene1.pts"),
                        "--width", "80", "--height", "60", "--spp", "4", "--adaptive", "0.05", "--max-spp", "64",
                        "-o", str(out), "--spp-map", str(smap)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rounds" in r.stdout
    hs, d = load_scene("scene1")
    p = hs.render_params(80, 60, 4)
    ds = _open(d)
    try:
        img, spp, _ = ds.render_adaptive(p, 0.05, max_spp=64)
    finally:
        ds.close()
    m = read_pfm(str(smap))
    assert m.shape == (60, 80, 3)
    assert (m == spp[..., None].astype(np.float32)).all()
    assert_bit_equal(read_pfm(str(out)), img, "CLI image")
