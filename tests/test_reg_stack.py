"""The register traversal stack of trace_kernel_v2 (csrc/pt_reg_stack.h, csrc/pt_trace.h: RegStack; kernels trace_kernel_v2_reg):
small LDS-resident scenes traversed on the internal tree keep their four stack entries in one register instead of an LDS
column.  The nodes visited, the leaves tested and their order are the LDS stack's, so every frame must equal the oracle's and
the LDS-stack kernel's bit for bit, with equal work counters; launches the predicate does not admit must keep the LDS stack.
The operations alone are checked on the CPU by tests/test_reg_stack_host.py."""
import ctypes as C
import re

import numpy as np
import pytest
from conftest import assert_bit_equal, load_scene
from trace_variants import Variant, code_object_symbols

from pathtracer_cuda_interactive_amd import (PT_BVH_SORT_REFERENCE, PT_MAT_DIFFUSE, PT_TRAVERSAL_EXACT, PT_TRAVERSAL_PRUNED,
                                             HostScene, _build)
from pathtracer_cuda_interactive_amd import device as dev

REG_BIT = 1 << 13            # info "trace_variant" (include/pt_api.h)
W, H, SPP = 64, 48, 8


@pytest.fixture(scope="module")
def cbox():
    hs, d = load_scene("cbox")
    ds = dev.DeviceScene(d)
    yield hs, d, ds
    ds.close()


_oracle_cache = {}


def oracle_frame(oracle, d, p, **kw):
    key = (p.width, p.height, p.spp, p.seed, tuple(sorted(kw.items())))
    if key not in _oracle_cache:
        _oracle_cache[key] = oracle.render(d, p, **kw)
    return _oracle_cache[key]


def render_with(ds, p, **opts):
    """(image, counters, info reg_stack, info lds_bytes, info trace_variant) of one frame under `opts`, options restored."""
    defaults = {"reg_stack": 1, "octants": 1, "stats": 0, "fast_tree": 1, "kernel": 2, "v2_inner": 0, "v2_minw": 0}
    for k, v in opts.items():
        ds.set_option(k, v)
    try:
        img = ds.render(p)
        return img, ds.counters(), ds.info("reg_stack"), ds.info("lds_bytes"), ds.info("trace_variant")
    finally:
        for k in opts:
            ds.set_option(k, defaults[k])


@pytest.mark.gpu
def test_fewer_work_items_than_lanes(oracle, cbox):
    """8 x 4 at 1 spp: 32 paths for the 256 lanes of the one block.  Lanes that never receive a path must see an empty stack
    and leave."""
    hs, d, ds = cbox
    p = hs.render_params(8, 4, 1, seed=3)
    want, cnt = oracle.render(d, p)
    img, c, reg, _, var = render_with(ds, p)
    assert reg == 1 and var & REG_BIT
    assert_bit_equal(img, want, "cbox 8x4x1")
    assert (c.paths, c.segments) == (cnt.paths, cnt.segments) and c.paths == 32


@pytest.mark.gpu
@pytest.mark.parametrize("stats", [0, 1], ids=["plain", "stats"])
@pytest.mark.parametrize("octants", [1, 0], ids=["octants", "one_table"])
@pytest.mark.parametrize("traversal", [PT_TRAVERSAL_EXACT, PT_TRAVERSAL_PRUNED], ids=["exact", "pruned"])
def test_cbox_equals_oracle_and_lds_stack(oracle, cbox, traversal, octants, stats):
    """cbox 64 x 48 at 8 spp: the frame of the register stack against the oracle's and against the LDS stack's."""
    hs, d, ds = cbox
    p = hs.render_params(W, H, SPP, seed=21)
    want, cnt = oracle_frame(oracle, d, p)
    p.traversal = traversal
    what = f"cbox traversal {traversal} octants {octants} stats {stats}"
    img1, c1, reg1, lds1, var1 = render_with(ds, p, octants=octants, stats=stats)
    img0, c0, reg0, lds0, var0 = render_with(ds, p, octants=octants, stats=stats, reg_stack=0)
    assert (reg1, reg0) == (1, 0), what
    assert var1 == var0 | REG_BIT and not var0 & REG_BIT, what
    v = Variant.decode(var1)
    assert (v.family, v.res, v.prune, v.stats, v.spec, v.thresh, v.inner, v.minw) == \
        (2, 2 if octants else 1, int(traversal == PT_TRAVERSAL_PRUNED), stats, 2, 40, 162, 6), (what, str(v))
    # 4 waves x stack_entries 16-bit columns of 64 lanes less
    assert lds1 < lds0 and lds0 - lds1 == 4 * ds.info("stack_entries") * 64 * 2, (what, lds1, lds0)
    assert_bit_equal(img1, img0, what + ": register stack against LDS stack")
    assert_bit_equal(img1, want, what + ": against the oracle")
    assert (c1.paths, c1.segments) == (c0.paths, c0.segments), what
    if traversal == PT_TRAVERSAL_EXACT:
        assert (c1.paths, c1.segments) == (cnt.paths, cnt.segments), what
    if stats:
        assert c1.node_visits > 0 and c1.leaf_tests > 0, what
        assert (c1.node_visits, c1.leaf_tests) == (c0.node_visits, c0.leaf_tests), what


def quads_scene(n):
    """n parallel unit quads stacked along the view axis, seen head-on from the front: a ray through the middle enters the
    box of every triangle.  Diffuse materials, the last quad emissive."""
    hs = HostScene()
    hs.set_camera((0.1, 0.05, 4.0), (0.1, 0.05, 0.0), (0, 1, 0), 40.0, 24, 16, 2)
    hs.set_background((0.4, 0.5, 0.6))
    mats = [hs.add_material(PT_MAT_DIFFUSE, (0.7, 0.6 - 0.02 * k, 0.2 + 0.03 * k)) for k in range(3)]
    for k in range(n):
        z = -0.4 * k
        s = 1.0 + 0.05 * k                              # the farther quads stick out behind the nearer ones
        P = np.array([[-s, -s, z], [s, -s, z], [s, s, z], [-s, s, z]], np.float32)
        hs.add_mesh(P, np.array([[0, 1, 2], [0, 2, 3]], np.int32), mats[k % 3], radiance=(3.0, 2.5, 2.0) if k == n - 1 else None)
    return hs


def poor_tree(d, seed):
    """A copy of `d` whose caller's tree pairs the leaves up in random order: valid and nested (every box is the union of its
    children's), but poor, so that pt_scene_create keeps its internal tree."""
    from pathtracer_cuda_interactive_amd.ctypes_defs import PtBvhNode, PtSceneDesc
    src = np.frombuffer((C.c_char * (d.num_nodes * dev.NODE_DTYPE.itemsize)).from_address(C.addressof(d.nodes.contents)),
                        dtype=dev.NODE_DTYPE)
    leaves = src[src["prim"] >= 0].copy()
    assert len(leaves) == d.num_shapes
    leaves = leaves[np.random.default_rng(seed).permutation(len(leaves))]
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


@pytest.mark.gpu
def test_stack_depth_boundary(oracle):
    """8 .. 20 quads = 16 .. 40 triangles (scene creation keeps an internal tree from 16 primitives on): trees that need 4
    stack entries (5 with the sentinel) run on the register stack, trees that need 5 keep the LDS stack, and the range holds
    both."""
    seen, rows = {}, []
    for n in range(8, 21):
        hs = quads_scene(n)
        d = poor_tree(hs.finalize(PT_BVH_SORT_REFERENCE), n)       # a poor caller's tree: scene creation keeps its internal tree
        ds = dev.DeviceScene(d)
        try:
            p = hs.render_params(24, 16, 2, seed=40 + n)
            want, cnt = oracle.render(d, p)
            img = ds.render(p)
            c = ds.counters()
            entries, reg, on = ds.info("stack_entries"), ds.info("reg_stack"), ds.info("fast_tree_on")
        finally:
            ds.close()
        what = f"{n} quads: stack_entries {entries}, internal tree {on}, reg_stack {reg}"
        print(what)
        rows.append((what, img, want, (c.paths, c.segments), (cnt.paths, cnt.segments), entries, reg))
        seen.setdefault(entries, set()).add(reg)
    for what, img, want, got_c, want_c, entries, reg in rows:
        assert_bit_equal(img, want, what)
        assert got_c == want_c, what
        assert reg == (1 if entries <= 5 else 0), what
    assert seen.get(5) == {1} and seen.get(6) == {0}, f"the range must hold stack_entries 5 and 6: {seen}"


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [{"fast_tree": 0}, {"kernel": 1}, {"kernel": 3}, {"v2_inner": 4}], ids=str)
def test_not_eligible_keeps_the_lds_stack(oracle, cbox, opts):
    hs, d, ds = cbox
    p = hs.render_params(W, H, SPP, seed=21)
    want, cnt = oracle_frame(oracle, d, p)
    img, c, reg, _, var = render_with(ds, p, **opts)
    assert reg == 0 and not var & REG_BIT, opts
    assert_bit_equal(img, want, str(opts))
    assert (c.paths, c.segments) == (cnt.paths, cnt.segments), opts


@pytest.mark.gpu
def test_scene_in_global_memory_keeps_its_stack(oracle):
    hs, d = load_scene("bunny")
    ds = dev.DeviceScene(d)
    try:
        p = hs.render_params(32, 24, 1, seed=5)
        want, _ = oracle.render(d, p)
        img = ds.render(p)
        assert ds.info("lds_scene") == 0 and ds.info("reg_stack") == 0 and not ds.info("trace_variant") & REG_BIT
    finally:
        ds.close()
    assert_bit_equal(img, want, "bunny 32x24x1")


@pytest.mark.gpu
def test_progressive_frames_in_flight(oracle, cbox):
    """pt_render_accumulate, 4 frames of 2 spp with two frames in flight: the accumulated image against the oracle's."""
    import torch
    hs, d, ds = cbox
    assert ds.info("frames_in_flight") == 2
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    want = None
    for k in range(4):
        p = hs.render_params(W, H, 2, seed=31)
        p.sample_offset, p.stream_stride = 2 * k, 8
        ds.accumulate_into(p, acc.data_ptr(), stream)
        assert ds.info("reg_stack") == 1, f"frame {k}"
        part, _ = oracle.render(d, p, accumulate=True)
        want = part if k == 0 else (want + part).astype(np.float32)
    torch.cuda.synchronize()
    assert_bit_equal(acc.cpu().numpy(), want, "4 accumulated frames of 2 spp")


_REG_KERNEL = re.compile(r"trace_kernel_v2_regILi(\d+)ELb([01])ELb([01])ELi(\d+)EEEv")


def compiled_reg_kernels():
    """{(res, prune, stats, minw)} of the trace_kernel_v2_reg instantiations in the library's gfx950 code objects."""
    found = []
    for syms in code_object_symbols(_build.HIP_LIB):
        for s in syms:
            m = _REG_KERNEL.search(s)
            if m:
                found.append(tuple(int(x) for x in m.groups()))
    return found


def test_compiled_register_stack_kernels():
    """Exact / pruned x STATS x 5 / 6 waves per SIMD for both LDS residencies, each compiled once."""
    found = compiled_reg_kernels()
    assert len(found) == len(set(found)), found
    assert set(found) == {(r, pr, st, w) for r in (1, 2) for pr in (0, 1) for st in (0, 1) for w in (5, 6)}


@pytest.mark.gpu
def test_every_register_stack_kernel_matches_the_oracle(oracle, cbox):
    """Every compiled trace_kernel_v2_reg instantiation, launched once on cbox 24 x 16 at 3 spp: info "trace_variant" names it,
    the frame is the oracle's (and the LDS-stack kernel's of the same template arguments)."""
    hs, d, ds = cbox
    p = hs.render_params(24, 16, 3, seed=97)
    want, cnt = oracle.render(d, p)
    failures = []
    for res, prune, stats, minw in sorted(set(compiled_reg_kernels())):
        what = f"trace_kernel_v2_reg<{res}, {prune}, {stats}, {minw}>"
        p.traversal = PT_TRAVERSAL_PRUNED if prune else PT_TRAVERSAL_EXACT
        opts = {"octants": int(res == 2), "stats": stats, "v2_minw": minw}
        img1, c1, reg1, _, var1 = render_with(ds, p, **opts)
        img0, c0, reg0, _, var0 = render_with(ds, p, reg_stack=0, **opts)
        try:
            assert reg1 == 1 and reg0 == 0, what
            assert var1 == Variant(2, res, prune, stats, 2, 0, 0, 0, 40, 162, minw).code | REG_BIT, (what, hex(var1))
            assert var0 == var1 & ~REG_BIT, what
            assert_bit_equal(img1, want, what)
            assert_bit_equal(img1, img0, what + " against the LDS stack")
            assert (c1.paths, c1.segments) == (c0.paths, c0.segments), what
            if not prune:
                assert (c1.paths, c1.segments) == (cnt.paths, cnt.segments), what
            if stats:
                assert (c1.node_visits, c1.leaf_tests) == (c0.node_visits, c0.leaf_tests), what
        except AssertionError as e:
            failures.append(str(e).splitlines()[0])
    assert not failures, "\n".join(failures)
