"""The index words of the path bank (csrc/pt_path_index.h: BankIndex): a bank fill keeps what start_path computed of each
item's index, its slot in the scratch buffer and its 64-bit PCG increment, and the hand-out moves those words to the lane that
takes the path in place of computing path_index there again.  A hand-out that moved the wrong slot's words would show as swapped
or repeated samples, so every frame here equals the oracle's bit for bit with equal work counters.

The kernels: cbox takes the sweep kernel, which always carries the words; with "leaf_sweep" 0 it takes trace_kernel_v2_reg and
with "reg_stack" 0 plain trace_kernel_v2 with the bank, both of which carry them at 5 blocks per CU ("v2_minw" 5) and keep the
computing hand-out at 6 (csrc/pt_kernels.h: bank_index_on); the random triangles of tests/test_path_bank.py are a second
LDS-resident scene, on whichever bank kernel scene creation gives them.  The words themselves are checked on the CPU by
tests/test_bank_index_host.py."""
import numpy as np
import pytest
from conftest import assert_bit_equal, load_scene
from test_path_bank import diffuse_triangles, oracle_frame
from trace_variants import Variant

from pathtracer_cuda_interactive_amd import device as dev

pytestmark = pytest.mark.gpu

DEFAULTS = {"leaf_sweep": 1, "reg_stack": 1, "v2_minw": 0, "chunk": 0, "item_order": 1, "xcd_regions": 0}

# name -> (scene, options that select the kernel, (leaf_sweep, reg_stack) the launch must report or None)
KERNELS = {
    "sweep": ("cbox", {}, (1, 1)),
    "reg5": ("cbox", {"leaf_sweep": 0, "v2_minw": 5}, (0, 1)),
    "reg6": ("cbox", {"leaf_sweep": 0, "v2_minw": 6}, (0, 1)),
    "lds_stack5": ("cbox", {"reg_stack": 0, "v2_minw": 5}, (0, 0)),
    "lds_stack6": ("cbox", {"reg_stack": 0, "v2_minw": 6}, (0, 0)),
    "tris5": ("tris", {"v2_minw": 5}, None),
}


@pytest.fixture(scope="module")
def scenes():
    out = {}
    hs, d = load_scene("cbox")
    out["cbox"] = (hs, d, dev.DeviceScene(d))
    hs = diffuse_triangles(5)
    d = hs.finalize()
    out["tris"] = (hs, d, dev.DeviceScene(d))
    yield out
    for _, _, ds in out.values():
        ds.close()


def frame(hs, w, h, spp, seed, offset=0, stride=0, rows=None):
    p = hs.render_params(w, h, spp, seed=seed)
    p.sample_offset, p.stream_stride = offset, stride
    if rows:
        p.row_begin, p.row_end, p.row_stride = rows
    return p


# what -> (width, height, spp, sample_offset, stream_stride, rows, feed options)
FRAMES = {
    "70x11x3: width no multiple of 64, a short last band": (70, 11, 3, 0, 0, None, {}),
    "7x5x1: a short bank fill, empty bands": (7, 5, 1, 0, 0, None, {}),
    "24x16x3 at sample offset 4, stream stride 16": (24, 16, 3, 4, 16, None, {}),
    "2048x2x1, stream stride 2^20: streams beyond 32 bits": (2048, 2, 1, 3, 1 << 20, None, {}),
    "40x31x2, rows 1::3": (40, 31, 2, 0, 0, (1, 31, 3), {}),
    "70x11x3, item order 0": (70, 11, 3, 0, 0, None, {"item_order": 0}),
    "70x11x3, item order 1": (70, 11, 3, 0, 0, None, {"item_order": 1}),
    "70x11x3, chunks of 64": (70, 11, 3, 0, 0, None, {"chunk": 64}),
    "24x16x3, chunks of 64, one band": (24, 16, 3, 0, 0, None, {"chunk": 64, "xcd_regions": 1}),
}


def render_under(ds, p, opts, want_info, what):
    for k, v in opts.items():
        ds.set_option(k, v)
    try:
        img = ds.render(p)
        c = ds.counters()
        assert ds.info("path_bank") == 1, what
        if want_info is not None:
            assert (ds.info("leaf_sweep"), ds.info("reg_stack")) == want_info, what
        if "v2_minw" in opts:
            assert Variant.decode(ds.info("trace_variant")).minw == opts["v2_minw"], what
    finally:
        for k in opts:
            ds.set_option(k, DEFAULTS[k])
    return img, c


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_frames_equal_the_oracle(oracle, scenes, kernel):
    name, kopts, want_info = KERNELS[kernel]
    hs, d, ds = scenes[name]
    for k, (what, (w, h, spp, off, stride, rows, fopts)) in enumerate(FRAMES.items()):
        p = frame(hs, w, h, spp, 60 + k, off, stride, rows)
        want, cnt = oracle_frame(oracle, name, d, p)
        img, c = render_under(ds, p, {**kopts, **fopts}, want_info, f"{kernel}: {what}")
        assert_bit_equal(img, want, f"{kernel}: {what}")
        assert (c.paths, c.segments) == (cnt.paths, cnt.segments), f"{kernel}: {what}"
        assert c.paths == p.num_rows() * w * spp, f"{kernel}: {what}"


@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("kernel", ["sweep", "reg5", "lds_stack5"])
def test_accumulated_frames(oracle, scenes, kernel, in_flight):
    """pt_render_accumulate over 3 frames of 2 spp at stream stride 2^20, one and two frames in flight, against the oracle's
    progressive sum."""
    import torch
    name, kopts, want_info = KERNELS[kernel]
    hs, d, ds = scenes[name]
    W, H = 70, 48
    was = ds.info("frames_in_flight")
    ds.set_option("frames_in_flight", in_flight)
    for k, v in kopts.items():
        ds.set_option(k, v)
    try:
        assert ds.info("frames_in_flight") == in_flight
        acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        want = None
        for k in range(3):
            p = frame(hs, W, H, 2, 77, 2 * k, 1 << 20)
            ds.accumulate_into(p, acc.data_ptr(), stream)
            assert ds.info("path_bank") == 1 and (ds.info("leaf_sweep"), ds.info("reg_stack")) == want_info, f"frame {k}"
            part, _ = oracle_frame(oracle, name, d, p, accumulate=True)
            want = part if k == 0 else (want + part).astype(np.float32)
        torch.cuda.synchronize()
    finally:
        for k in kopts:
            ds.set_option(k, DEFAULTS[k])
        ds.set_option("frames_in_flight", was)
    assert_bit_equal(acc.cpu().numpy(), want, f"{kernel}: 3 accumulated frames, {in_flight} in flight")
