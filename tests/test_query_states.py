"""pt_trace_rays and pt_render_guides_async in every state a handle can be in (include/pt_api.h, DESIGN.md §24, csrc/pt_query.h).

The query kernel has a scheduler of its own (static first ranges, one atomic work counter, the refill threshold "query_refill")
and builds its kernel argument block per call (tree_view), so it can be wrong on a few rays while every image looks right.
The tests here hold it to the CPU oracle, bit for bit, on the desc the handle currently stands for:

  A  the hand-out: every refill threshold x every kind of grid on rays of uneven cost, prefixes with untouched tails, guides;
  B  pruned traversal against pt_debug_intersect's;
  C  the ends of the open ray interval (tnear, tfar);
  D  every handle state: created (one shape .. the deepest tree), updated, updated back, after each kind of edit, transformed,
     between renders, across option changes;
  E  a query queued on a side stream answers for the geometry from before pt_scene_update / pt_scene_transform;
  F  ray and output pointers that are 4-byte aligned and no more.

Every ray set has a CPU test that states what makes its GPU test able to fail (hit and miss shares, the spread of cost inside
a block of 64 rays, the share of answers an edit changes, the interval-end conditions, the 64-block contention arithmetic)."""
import os
import re

import numpy as np
import pytest
import query_cases as qc
import test_scene_transform as tt
from conftest import REPO, assert_bit_equal
from scene_update_cases import B_EDITS, b_edit, b_scene, regime_input, scene_rays, tree_depth
from test_aov import numpy_guides, scene
from test_guides_async import AOV_KEYS, KEYS, assert_same, run_async
from test_motion import camera_step, moved
from test_motion import case as motion_case
from test_trace_rays import any_rays, ray_set

from pathtracer_cuda_interactive_amd import (PT_ERR_INVALID_ARG, PT_QUERY_ANY, PT_TRAVERSAL_EXACT, PT_TRAVERSAL_PRUNED, PtError, host)
from pathtracer_cuda_interactive_amd import device as dev

N = 20000
REFILLS = (1, 2, 16, 17, 63, 64)
BLOCKS = (1, 2, 3, 64, 0)
CSRC = os.path.join(REPO, "pathtracer_cuda_interactive_amd", "csrc")


def _constant(header, name):
    m = re.search(r"(?:constexpr int|#define)\s+" + name + r"\s*=?\s*(\d+)", open(os.path.join(CSRC, header)).read())
    assert m, f"{header} defines no {name}"
    return int(m.group(1))


QUERY_CHUNK = _constant("pt_query.h", "kQueryChunk")
BLOCK_THREADS = _constant("pt_kernels.h", "PT_BLOCK")
WAVES_PER_BLOCK = BLOCK_THREADS // 64

_made = {}


def once(key, make):
    """make() once per key; its arrays are shared between the tests and left unchanged."""
    if key not in _made:
        _made[key] = make()
        for a in _made[key] if isinstance(_made[key], tuple) else ():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _made[key]


def differ(a, b):
    """Rays whose (tuv, prim) answers differ in any bit."""
    return (a[1] != b[1]) | (a[0].view(np.uint32) != b[0].view(np.uint32)).any(axis=1)


# ---- the ray sets and their references ---------------------------------------------------------------------------------------

def uneven_set(oracle, name):
    """(desc, rays [N, 8], the oracle's tuv, prim, inner-node visits per ray) of bunny / cbox under query_cases.uneven_rays."""
    def make():
        _, d = scene(name)
        rays = qc.uneven_rays(d, N)
        tuv, prim = oracle.intersect(d, rays)
        return d, rays, tuv, prim, oracle.intersect_work(d, rays)[0]
    return once(("uneven", name), make)


def end_sets(oracle, name):
    """(desc, rays, tuv, prim of the base set, {variant: (rays, tuv, prim)}) for the interval ends of one scene."""
    def make():
        if name == "chain65":
            d = regime_input(name)[1]
            rays = qc.aimed_rays(d, 5000, 41)
            tuv, prim = oracle.intersect(d, rays)
        else:
            d, rays, tuv, prim = ray_set(oracle, name)
        out = {}
        for k, r in {**qc.interval_end_rays(rays, tuv, prim), **qc.odd_interval_rays(d, rays, tuv, prim)}.items():
            out[k] = (r,) + oracle.intersect(d, r)
        return d, rays, tuv, prim, out
    return once(("ends", name), make)


REGIMES = ["n1", "n2", "n3", "chain65", "complete2048", "heap4097"]
N_STATE = 5000


def regime_set(oracle, name):
    """(d0, d1, rays, the oracle's (tuv, prim) on d0, on d1r)."""
    def make():
        _, d0, d1, d1r, _ = regime_input(name)
        rays = qc.aimed_rays(d0, N_STATE, 41)
        return d0, d1, rays, oracle.intersect(d0, rays), oracle.intersect(d1r, rays)
    return once(("regime", name), make)


def edit_set(oracle, name):
    """(d0, rays, the oracle's answer on d0, {edit: (d1, d1r, the oracle's answer on d1r)}) of b_scene(name)."""
    def make():
        _, d0, _ = b_scene(name, False)
        rays = scene_rays(N_STATE, 43)
        edits = {}
        for e in B_EDITS:
            d1, d1r = b_edit(name, False, e)
            edits[e] = (d1, d1r, oracle.intersect(d1r, rays))
        return d0, rays, oracle.intersect(d0, rays), edits
    return once(("edits", name), make)


def transform_set(oracle, name):
    """(d0, ids, [(matrices, the desc they stand for, the oracle's answer on it)] for identity, M1, M2, rays)."""
    def make():
        d0, ids, M1, M2 = tt.case(name)[:4]
        rays = tt.scene_rays(d0, name, N_STATE, 9)
        steps = []
        for M in (np.stack([tt.IDENTITY] * M1.shape[0]), M1, M2):
            d = host.refit_bvh(dev.transform_desc_host(d0, ids, M))
            steps.append((M, d, oracle.intersect(d, rays)))
        return d0, ids, steps, rays
    return once(("transform", name), make)


def stream_set(oracle, kind):
    """(d0, the edit's argument, rays, the oracle's answer before, after) for the two stream-order cases."""
    def make():
        if kind == "update":
            d0, rays, before, edits = edit_set(oracle, "global")
            d1, _, after = edits["emitter_moved"]
            return d0, d1, rays, before, after
        d0, ids, steps, rays = transform_set(oracle, "random7")
        return d0, (ids, steps[1][0]), rays, oracle.intersect(d0, rays), steps[1][2]
    return once(("stream", kind), make)


# ---- CPU: what makes the GPU tests able to fail ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["bunny", "cbox"])
def test_uneven_rays_spread_the_cost_inside_every_block_of_64(oracle, name):
    """Measured spread (largest / median inner-node visits per aligned block of 64 rays, the smallest over the 313 blocks):
    bunny 144, cbox 21; the median is 1 node everywhere — 33 rays of a block fail the root's box."""
    d, rays, _, prim, visits = uneven_set(oracle, name)
    assert len(rays) == N
    spread = qc.block_spread(visits)
    print(name, "largest / median per block: min", (spread[:, 0] / spread[:, 1]).min(), "median of medians", np.median(spread[:, 1]))
    assert (spread[:, 1] >= 1).all()
    assert (spread[:, 0] >= 8 * spread[:, 1]).all(), "a block of 64 rays holds no ray 8 times as expensive as its median"
    lo, hi = qc.root_box(d)
    o, u = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    for b in range(0, N, 64):
        ob, ub = o[b:b + 64], u[b:b + 64]
        away = (((ob > hi) & (ub > 0)) | ((ob < lo) & (ub < 0))).any(axis=1)        # outside on an axis and leaving on it
        assert away.mean() >= 0.25 and (visits[b:b + 64][away] == 1).all()
    assert (prim >= 0).mean() > 0.05 and (prim[1::2] >= 0).sum() > 1000
    zero = (rays[:, 3:6] == 0).any(axis=1)
    assert zero.sum() >= N // 40 and (prim[zero] >= 0).any(), "rays for the caller's-tree lanes"


def test_at_64_blocks_256_waves_contend_for_the_counter():
    """The grids of the matrix: 1, 2, 3 and 64 blocks leave indices beyond the waves' first ranges, the automatic grid none."""
    first_ranges = {b: b * WAVES_PER_BLOCK * QUERY_CHUNK for b in (1, 2, 3, 64)}
    assert (WAVES_PER_BLOCK, QUERY_CHUNK) == (4, 64)
    assert first_ranges[64] == 16384 < N and 64 * WAVES_PER_BLOCK == 256
    assert (N - first_ranges[64]) // QUERY_CHUNK >= 56, "ranges left for the counter"
    assert all(r < N for r in first_ranges.values())
    by_work = (N + BLOCK_THREADS - 1) // BLOCK_THREADS
    assert by_work == 79 and by_work * WAVES_PER_BLOCK * QUERY_CHUNK >= N, "the automatic grid is the static case"
    # the prefix sizes of the sentinel test against their grids: static at n <= first ranges, else contended
    assert {n: n > first_ranges[3] for n in PREFIXES} == {1: False, 63: False, 65: False, 4095: True, 4097: True, 16385: True}
    assert 16385 > first_ranges[64]


@pytest.mark.parametrize("name", ["bunny", "cbox", "random1", "chain65"])
def test_interval_end_sets_change_answers_as_stated(oracle, name):
    d, rays, tuv, prim, sets = end_sets(oracle, name)
    hp = prim[prim >= 0]
    assert len(hp) >= 1000
    share = {k: ((p < 0).mean(), (p == hp).mean() if len(p) == len(hp) else None, (p >= 0).mean()) for k, (_, _, p) in sets.items()}
    print(name, share)
    assert share["tfar_at_t"][0] >= 0.95, "tfar = t is outside the open interval"
    assert share["tfar_above_t"][1] >= 0.95 and share["tnear_below_t"][1] >= 0.95
    assert_bit_equal(sets["tfar_above_t"][1][sets["tfar_above_t"][2] == hp], tuv[prim >= 0][sets["tfar_above_t"][2] == hp], "the same hit")
    other = (sets["tnear_at_t"][2] >= 0) & (sets["tnear_at_t"][2] != hp)
    assert other.sum() >= 100, "tnear = t: rays that go on to another primitive"
    again = sets["tnear_at_t"][2] >= 0
    if name in ("bunny", "cbox"):
        # triangles alone are hit: tnear = t is outside the interval.  (On random1 and chain65 most hits are on spheres, and the
        # reference's sphere test, which the oracle restates, keeps a root at t == tnear: 78 % of random1's rays return the
        # same hit at the same t.  The oracle decides; the GPU tests hold both kinds to it.)
        assert (sets["tnear_at_t"][1][again, 0] > tuv[prim >= 0][again, 0]).all(), "tnear = t is outside the open interval"
        assert (sets["tnear_at_t"][2] != hp).all()
    else:
        assert (sets["tnear_at_t"][1][again, 0] >= tuv[prim >= 0][again, 0]).all()
    assert share["tnear_above_tfar"][2] == 0 and share["tnear_is_tfar"][2] == 0, "an empty interval holds no hit"
    for k in ("tnear_minus_one_inside", "dir_by_1e-3", "dir_by_1e3"):
        assert 0.05 <= share[k][2] <= 0.95, k
    # a scaled direction scales t (and so what tnear cuts off): most rays keep their primitive at a t a thousand times smaller
    same = (sets["dir_by_1e3"][2] == prim) & (prim >= 0)
    assert same.sum() > 0.9 * (prim >= 0).sum() and np.median(tuv[same, 0] / sets["dir_by_1e3"][1][same, 0]) == pytest.approx(1e3, rel=1e-3)


@pytest.mark.parametrize("name", REGIMES)
def test_regime_rays_hit_miss_and_see_the_edit(oracle, name):
    d0, d1, rays, at0, at1 = regime_set(oracle, name)
    for tuv, prim in (at0, at1):
        assert (prim >= 0).mean() >= 0.05 and (prim < 0).mean() >= 0.05, name
    changed = differ(at0, at1)
    print(name, "hits", (at0[1] >= 0).mean(), (at1[1] >= 0).mean(), "answers the edit changes", changed.mean())
    assert changed.mean() >= 0.02 and changed.sum() >= 1
    if name == "chain65":
        assert tree_depth(d0) == 64, "the deepest tree pt_scene_create accepts"
        assert WAVES_PER_BLOCK * 64 * 64 * 4 == 64 * 1024, "64 entries per lane are exactly 64 KiB of LDS per block"


@pytest.mark.parametrize("name", ["lds", "global"])
def test_edit_rays_hit_miss_and_see_the_edits(oracle, name):
    d0, rays, before, edits = edit_set(oracle, name)
    assert (before[1] >= 0).mean() >= 0.05 and (before[1] < 0).mean() >= 0.05
    for e, (_, _, after) in edits.items():
        share = differ(before, after).mean()
        print(name, e, "hits", (after[1] >= 0).mean(), "answers the edit changes", share)
        assert (after[1] >= 0).mean() >= 0.05 and (after[1] < 0).mean() >= 0.05
        if e in ("merged", "split70", "ids"):
            assert share == 0, "these edits keep every shape where it is"
        else:
            assert share >= 0.02, e


@pytest.mark.parametrize("name", tt.SCENES)
def test_transform_rays_hit_miss_and_see_the_motion(oracle, name):
    d0, ids, steps, rays = transform_set(oracle, name)
    at0 = oracle.intersect(d0, rays)
    assert not differ(at0, steps[0][2]).any(), "the identity moves nothing"
    for _, _, (_, prim) in steps:                              # (cbox is a closed room: 2.5 % of its rays miss)
        assert (prim >= 0).sum() >= 100 and (prim < 0).sum() >= 100
    share = differ(at0, steps[1][2]).mean(), differ(steps[1][2], steps[2][2]).mean()
    print(name, "answers M1 changes", share[0], "answers M2 changes after M1", share[1])
    assert min(share) >= 0.02


@pytest.mark.parametrize("kind", ["update", "transform"])
def test_stream_order_rays_tell_the_old_geometry_from_the_new(oracle, kind):
    _, _, rays, before, after = stream_set(oracle, kind)
    changed = differ(before, after)
    print(kind, "answers that differ", changed.mean(), "any-mode answers that differ", ((before[1] >= 0) != (after[1] >= 0)).mean())
    assert changed.mean() >= 0.02 and ((before[1] >= 0) != (after[1] >= 0)).mean() >= 0.02


# ---- GPU: helpers -----------------------------------------------------------------------------------------------------------

class opened:
    """A DeviceScene with the given options, closed on the way out."""

    def __init__(self, d, **opts):
        self.d, self.opts = d, opts

    def __enter__(self):
        self.ds = dev.DeviceScene(self.d)
        for key, v in self.opts.items():
            self.ds.set_option(key, v)
        return self.ds

    def __exit__(self, *exc):
        self.ds.close()


def schedule(ds, refill, blocks):
    ds.set_option("query_refill", refill)
    ds.set_option("query_blocks", blocks)


def assert_closest(ds, rays, want, what, traversal=PT_TRAVERSAL_EXACT):
    tuv, prim = ds.trace_rays(rays, traversal=traversal)
    bad = np.flatnonzero(prim != want[1])
    assert bad.size == 0, f"{what}: {bad.size} of {len(prim)} prims differ, first at {bad[:4]}: {prim[bad[:4]]} vs {want[1][bad[:4]]}"
    assert_bit_equal(tuv, want[0], what)
    return tuv, prim


def assert_any(ds, rays, want_prim, what, traversal=PT_TRAVERSAL_EXACT):
    hit = ds.trace_rays(rays, mode=PT_QUERY_ANY, traversal=traversal)
    bad = np.flatnonzero(hit != (want_prim >= 0))
    assert bad.size == 0, f"{what} any mode: {bad.size} of {len(hit)} answers differ, first at {bad[:4]}: {hit[bad[:4]]} vs prim {want_prim[bad[:4]]}"
    return hit


STATE_SCHEDULES = ((0, 0), (1, 2))


def assert_state(ds, rays, want, what, schedules=STATE_SCHEDULES, debug=False):
    """Closest and any mode against the oracle's answer `want` on both trees, at the default scheduler and a forced one;
    debug: against pt_debug_intersect on the same handle as well.  Leaves the options as they were found (defaults)."""
    for fast in (1, 0):
        ds.set_option("fast_tree", fast)
        if debug:
            dbg = ds.intersect(rays)
            assert not differ(dbg, want).any(), f"{what} fast_tree={fast}: pt_debug_intersect and the oracle disagree"
        for refill, blocks in schedules:
            schedule(ds, refill, blocks)
            w = f"{what} fast_tree={fast} query_refill={refill} query_blocks={blocks}"
            assert_closest(ds, rays, want, w)
            assert_any(ds, rays, want[1], w)
    schedule(ds, 0, 0)
    ds.set_option("fast_tree", 1)


# ---- A: the hand-out --------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bunny", "cbox"])
def test_every_refill_threshold_on_every_grid(oracle, name):
    d, rays, tuv, prim, _ = uneven_set(oracle, name)
    with opened(d) as ds:
        assert ds.info("query_chunk") == QUERY_CHUNK
        # at 64 blocks the first ranges end at 16,384: 256 waves share the counter for the rest
        assert 64 * WAVES_PER_BLOCK * ds.info("query_chunk") == 16384 < N
        for fast in (1, 0):
            ds.set_option("fast_tree", fast)
            for refill in REFILLS:
                for blocks in BLOCKS:
                    schedule(ds, refill, blocks)
                    what = f"{name} fast_tree={fast} query_refill={refill} query_blocks={blocks}"
                    assert_closest(ds, rays, (tuv, prim), what)
                    grid = ds.info("query_grid")
                    if blocks:
                        assert grid == blocks, what
                    else:                                     # one ray per lane, on a device of 79 CUs or more
                        assert grid == (N + BLOCK_THREADS - 1) // BLOCK_THREADS or grid >= ds.info("num_cus"), what
                    assert_any(ds, rays, prim, what)
                    assert ds.info("query_grid") == grid


PREFIXES = (1, 63, 65, 4095, 4097, 16385)


@pytest.mark.gpu
def test_prefixes_are_written_exactly_where_they_should_be(oracle):
    import torch
    d, rays, tuv, prim, _ = uneven_set(oracle, "bunny")
    total = max(PREFIXES) + 8
    d_rays = torch.from_numpy(rays[:total].copy()).cuda()
    with opened(d) as ds:
        for refill, blocks in ((1, 3), (64, 3), (17, 64)):
            schedule(ds, refill, blocks)
            for n in PREFIXES:
                t_out = torch.full((total, 3), -7.0, device="cuda")
                p_out = torch.full((total,), -7, device="cuda", dtype=torch.int32)
                a_out = torch.full((total,), -7, device="cuda", dtype=torch.int32)
                ds.trace_rays_into(d_rays.data_ptr(), n, t_out.data_ptr(), p_out.data_ptr())
                ds.trace_rays_into(d_rays.data_ptr(), n, 0, a_out.data_ptr(), mode=PT_QUERY_ANY)
                torch.cuda.synchronize()
                t_np, p_np, a_np = t_out.cpu().numpy(), p_out.cpu().numpy(), a_out.cpu().numpy()
                what = f"n={n} query_refill={refill} query_blocks={blocks}"
                unwritten = np.flatnonzero(p_np[:n] == -7)
                assert unwritten.size == 0, f"{what}: {unwritten.size} results of [0, n) were never written, first at {unwritten[:4]}"
                assert (p_np[:n] == prim[:n]).all(), what
                assert_bit_equal(t_np[:n], tuv[:n], what)
                assert np.array_equal(a_np[:n], (prim[:n] >= 0).astype(np.int32)), what + " any mode"
                assert (p_np[n:] == -7).all() and (t_np[n:] == -7.0).all() and (a_np[n:] == -7).all(), what + ": output past n was written"


@pytest.mark.gpu
def test_query_refill_takes_0_to_64_and_0_is_the_default(oracle):
    d, rays, tuv, prim, _ = uneven_set(oracle, "cbox")
    with opened(d, query_blocks=2) as ds:
        default = assert_closest(ds, rays, (tuv, prim), "the default threshold")
        ds.set_option("query_refill", 64)
        for bad in (65, -1):
            with pytest.raises(PtError) as e:
                ds.set_option("query_refill", bad)
            assert e.value.status == PT_ERR_INVALID_ARG and "query_refill" in str(e.value)
        assert not differ(assert_closest(ds, rays, (tuv, prim), "query_refill=64 after the refusals"), default).any()
        ds.set_option("query_refill", 0)
        assert not differ(assert_closest(ds, rays, (tuv, prim), "query_refill=0"), default).any()
        assert_any(ds, rays, prim, "query_refill=0")


def _frames(oracle):
    hs, d = scene("cbox")
    p = hs.render_params(61, 37, 1)
    p.row_begin, p.row_end, p.row_stride = 2, 37, 2
    yield "cbox 61x37 rows (2, 37, 2)", d, p, moved(p, camera_step(oracle, "cbox", p))
    hs, d = scene("bunny")
    p = hs.render_params(64, 48, 1)
    yield "bunny 64x48", d, p, moved(p, np.array([0.02, 0.01, -0.015]))


@pytest.mark.gpu
def test_guides_on_the_refilling_kernel_at_every_threshold(oracle):
    for name, d, p, prev in _frames(oracle):
        want_np = numpy_guides(oracle, d, p)
        with opened(d, query_guides=1) as ds:
            want, want_aov = ds.render_guides(p, prev), ds.render_aov(p)
            for refill in (1, 17, 64):
                for blocks in (0, 2, 3):
                    schedule(ds, refill, blocks)
                    what = f"{name} query_refill={refill} query_blocks={blocks}"
                    got = run_async(ds, p, prev)
                    assert ds.info("query_guides") == 1 and (ds.info("query_grid") == blocks or not blocks)
                    assert_same(got, want, KEYS, what)
                    assert_same(got, want_np, AOV_KEYS, what + ", numpy")
                    got = run_async(ds, p, None)
                    assert_same(got, want_aov, AOV_KEYS, what + ", no motion")
                    assert_same(got, want_np, AOV_KEYS, what + ", no motion, numpy")
                    assert (got["motion"] == -7).all() and (got["prev_depth"] == -7).all()


# ---- B: pruned traversal ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bunny", "cbox"])
def test_pruned_closest_mode_is_pruned_debug_intersect(oracle, name):
    """intersect_kernel and query_kernel run the same step functions for every class of ray: inner_step<PRUNE> and leaf_step
    with ties on the tree a render traverses, and — on a handle that traverses its internal tree — exact steps on the caller's
    tree for a ray whose 1/d is not finite, in both.  That class is held to the exact answer here as well."""
    d, rays, tuv, prim, _ = uneven_set(oracle, name)
    zero = (rays[:, 3:6] == 0).any(axis=1)
    with opened(d) as ds:
        for fast in (1, 0):
            ds.set_option("fast_tree", fast)
            want = ds.intersect(rays, PT_TRAVERSAL_PRUNED)
            flips = int((want[1] != prim).sum())
            print(f"{name} fast_tree={fast}: pruned prim ids that differ from the oracle's: {flips}")
            assert flips <= max(3, N // 20000)
            for refill, blocks in ((16, 0), (1, 1), (64, 3)):
                schedule(ds, refill, blocks)
                what = f"{name} pruned fast_tree={fast} query_refill={refill} query_blocks={blocks}"
                got = assert_closest(ds, rays, want, what, traversal=PT_TRAVERSAL_PRUNED)
                if fast and ds.info("fast_tree"):
                    assert not differ((got[0][zero], got[1][zero]), (tuv[zero], prim[zero])).any(), what + ": rays on the caller's tree are exact"
                assert_any(ds, rays, prim, what, traversal=PT_TRAVERSAL_PRUNED)


# ---- C: interval ends -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bunny", "cbox", "random1", "chain65"])
def test_the_interval_is_open_at_both_ends(oracle, name):
    d, _, _, _, sets = end_sets(oracle, name)
    with opened(d) as ds:
        for fast in (1, 0):
            ds.set_option("fast_tree", fast)
            for refill, blocks in ((0, 0), (1, 3)):
                schedule(ds, refill, blocks)
                for k, (rays, tuv, prim) in sets.items():
                    what = f"{name} {k} fast_tree={fast} query_refill={refill} query_blocks={blocks}"
                    if (refill, blocks) == (0, 0):
                        dbg = ds.intersect(rays)
                        assert not differ(dbg, (tuv, prim)).any(), what + ": pt_debug_intersect and the oracle disagree"
                    assert_closest(ds, rays, (tuv, prim), what)
                    assert_any(ds, rays, prim, what)


# ---- D: every handle state --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", REGIMES)
def test_created_updated_and_updated_back(oracle, name):
    d0, d1, rays, at0, at1 = regime_set(oracle, name)
    with opened(d0) as ds:
        if name == "chain65":
            # the deepest stack the library allows: 64 entries per lane, 64 KiB of LDS per block of four waves, on either tree
            ds.set_option("fast_tree", 0)
            assert ds.info("bvh_depth") == 64 and ds.info("stack_entries") == 64
            assert WAVES_PER_BLOCK * ds.info("stack_entries") * 64 * 4 == 64 * 1024
            ds.set_option("fast_tree", 1)
        assert_state(ds, rays, at0, name + " created")
        first = ds.trace_rays(rays), ds.trace_rays(rays, mode=PT_QUERY_ANY)
        ds.update(d1)
        assert_state(ds, rays, at1, name + " after update(d1)", debug=True)
        ds.update(d0)
        assert_state(ds, rays, at0, name + " back at d0")
        again = ds.trace_rays(rays), ds.trace_rays(rays, mode=PT_QUERY_ANY)
        assert not differ(first[0], again[0]).any() and np.array_equal(first[1], again[1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lds", "global"])
def test_after_each_kind_of_edit(oracle, name):
    d0, rays, before, edits = edit_set(oracle, name)
    _, _, p = b_scene(name, False)
    with opened(d0) as ds:
        assert ds.info("residency") == (2 if name == "lds" else 3)
        assert_state(ds, rays, before, name + " created")
        aov0 = ds.render_aov(p)
        for e, (d1, d1r, after) in edits.items():
            ds.update(d1)
            what = f"{name} after {e}"
            assert_state(ds, rays, after, what, debug=True)
            # the guide planes of the refilling kernel follow the blocking call (whose contract: a fresh create of d1r)
            ds.set_option("query_guides", 1)
            want = ds.render_aov(p)
            for refill, blocks in STATE_SCHEDULES:
                schedule(ds, refill, blocks)
                got = run_async(ds, p, None)
                assert ds.info("query_guides") == 1
                assert_same(got, want, AOV_KEYS, f"{what} guides query_refill={refill} query_blocks={blocks}")
            schedule(ds, 0, 0)
            ds.set_option("query_guides", 0)
            if e == "ids":
                assert not differ(ds.trace_rays(rays), before).any(), "ids alone: the same hits"
                assert np.array_equal(want["prim"], aov0["prim"]) and not np.array_equal(want["albedo"], aov0["albedo"])
                assert_same(want, numpy_guides(oracle, d1r, p), AOV_KEYS, what + " guides, numpy")
        ds.update(d0)
        assert_state(ds, rays, before, name + " back at d0")


@pytest.mark.gpu
@pytest.mark.parametrize("name", tt.SCENES)
def test_after_set_groups_and_transform(oracle, name):
    d0, ids, steps, rays = transform_set(oracle, name)
    p = tt.case(name)[7].copy()
    p.spp = 1
    prev_cam = dev.translated_params(p, np.array([0.02, -0.01, 0.03]) * (550.0 if name == "cbox" else 60.0 if name == "teapot" else 3.0))
    with opened(d0) as ds:
        ds.set_groups(ids, steps[0][0].shape[0])
        assert_state(ds, rays, steps[0][2], name + " after set_groups")
        for k, (M, _, want) in enumerate(steps):
            ds.transform(M)
            what = f"{name} after transform {k}"
            assert_state(ds, rays, want, what, debug=True)
            assert ds.info("prev_geometry") == 1
            ds.set_option("query_guides", 1)
            for previous in (True, False):
                blocking = ds.render_guides(p, prev_cam, previous_geometry=previous)
                for refill, blocks in STATE_SCHEDULES:
                    schedule(ds, refill, blocks)
                    got = run_async(ds, p, prev_cam, previous_geometry=previous)
                    assert ds.info("query_guides") == 1
                    assert_same(got, blocking, KEYS, f"{what} guides previous_geometry={previous} query_refill={refill} query_blocks={blocks}")
            schedule(ds, 0, 0)
            ds.set_option("query_guides", 0)


@pytest.mark.gpu
def test_queries_between_renders_after_an_update(oracle):
    """query, render, query under the other traversal, render_aov, query: the exact queries and every any-mode answer are equal,
    the pruned closest query is pt_debug_intersect's pruned answer (of the handle that never ran the query kernel) and within
    the project's bound of the exact one; the renders are those of that other handle."""
    hs, d0, d1, d1r = motion_case("cbox")[:4]
    p = hs.render_params(64, 48, 4)
    rays = ray_set(oracle, "cbox")[1][:N_STATE]
    want = oracle.intersect(d1r, rays)
    assert (want[1] >= 0).mean() >= 0.05 and (want[1] < 0).mean() >= 0.05
    with opened(d0) as A, opened(d0) as B:
        A.update(d1)
        B.update(d1)
        q1 = assert_closest(A, rays, want, "before the render"), assert_any(A, rays, want[1], "before the render")
        img = A.render(p)
        q2 = A.trace_rays(rays, traversal=PT_TRAVERSAL_PRUNED), assert_any(A, rays, want[1], "pruned, after the render", PT_TRAVERSAL_PRUNED)
        aov = A.render_aov(p)
        q3 = assert_closest(A, rays, want, "after render_aov"), assert_any(A, rays, want[1], "after render_aov")
        assert not differ(q1[0], q3[0]).any() and np.array_equal(q1[1], q2[1]) and np.array_equal(q1[1], q3[1])
        assert not differ(q2[0], B.intersect(rays, PT_TRAVERSAL_PRUNED)).any(), "the pruned query against pt_debug_intersect's"
        assert (q2[0][1] != want[1]).sum() <= max(3, len(rays) // 20000)
        assert_bit_equal(img, B.render(p), "pt_render between queries")
        assert_same(aov, B.render_aov(p), AOV_KEYS, "pt_render_aov between queries")


@pytest.mark.gpu
def test_option_changes_between_queries(oracle):
    d, rays, tuv, prim = ray_set(oracle, "bunny")
    three = any_rays(rays[:6000], tuv[:6000], prim[:6000])
    want = once(("options", "bunny"), lambda: oracle.intersect(d, three))
    hs, _ = scene("bunny")
    p = hs.render_params(64, 48, 1)
    prev = moved(p, np.array([0.02, 0.01, -0.015]))
    # "blocks_per_cu" feeds the automatic grid only where the rays outnumber one block per CU: the same rays, several times over
    many = np.resize(three, (4 * len(three), 8))
    want_many = np.resize(want[0], (len(many), 3)), np.resize(want[1], len(many))
    with opened(d) as ds:
        guides = ds.render_guides(p, prev)
        for fast in (1, 0, 1):
            ds.set_option("fast_tree", fast)
            assert_closest(ds, three, want, f"fast_tree={fast}")
            assert_any(ds, three, want[1], f"fast_tree={fast}")
            ds.set_option("query_guides", 1)
            assert_same(run_async(ds, p, prev), guides, KEYS, f"guides fast_tree={fast}")
            ds.set_option("query_guides", 0)
        assert len(many) > ds.info("num_cus") * BLOCK_THREADS
        grids = []
        for bpc in (0, 1, 0):
            ds.set_option("blocks_per_cu", bpc)
            assert_closest(ds, many, want_many, f"blocks_per_cu={bpc}")
            grids.append(ds.info("query_grid"))
            assert_any(ds, many, want_many[1], f"blocks_per_cu={bpc}")
            assert ds.info("query_grid") == grids[-1]
        print("query_grid under blocks_per_cu 0, 1, 0:", grids)
        assert grids[1] == ds.info("num_cus") and grids[0] == grids[2] != grids[1]
        for kernel in (0, 1, 2):
            ds.set_option("query_guides", kernel)
            assert_same(run_async(ds, p, prev), guides, KEYS, f"query_guides={kernel}")
            assert ds.info("query_guides") == (1 if kernel == 1 else 0)
            assert_closest(ds, three, want, f"query_guides={kernel}")
            assert_any(ds, three, want[1], f"query_guides={kernel}")


# ---- E: stream order against update and transform --------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["update", "transform"])
def test_a_queued_query_answers_for_the_geometry_before_the_edit(oracle, kind):
    """pt_scene_update and pt_scene_transform synchronise the device before they write: queries enqueued on a side stream
    behind other work, then the edit from the host at once, then the same queries again.  The edit swaps buffers and frees
    none, so a missing synchronisation shows as answers for the wrong geometry."""
    import torch
    d0, arg, rays, before, after = stream_set(oracle, kind)
    n = len(rays)
    with opened(d0) as ds:
        if kind == "transform":
            ds.set_groups(arg[0], arg[1].shape[0])
        src = torch.from_numpy(rays.copy()).cuda()
        work = torch.randn(4096, 4096, device="cuda")
        stream = torch.cuda.Stream()
        d_rays = torch.zeros_like(src)
        out = [(torch.full((n, 3), -7.0, device="cuda"), torch.full((n,), -7, device="cuda", dtype=torch.int32),
                torch.full((n,), -7, device="cuda", dtype=torch.int32)) for _ in range(2)]
        work = work @ work * (1.0 / 4096)                            # (the library behind @ is loaded before the clock matters)
        torch.cuda.synchronize()

        def enqueue(t_out, p_out, a_out):
            ds.trace_rays_into(d_rays.data_ptr(), n, t_out.data_ptr(), p_out.data_ptr(), stream=stream.cuda_stream)
            ds.trace_rays_into(d_rays.data_ptr(), n, 0, a_out.data_ptr(), mode=PT_QUERY_ANY, stream=stream.cuda_stream)

        with torch.cuda.stream(stream):
            for _ in range(6):                                       # the rays arrive late, behind other work of the stream
                work = work @ work * (1.0 / 4096)
            d_rays.copy_(src)
            enqueue(*out[0])
        queued = not stream.query()
        if kind == "update":
            ds.update(arg)
        else:
            ds.transform(arg[1])
        enqueue(*out[1])
        stream.synchronize()
        print(kind, "the first queries were still queued when the edit was called:", queued)
        for (t_out, p_out, a_out), want, what in ((out[0], before, "queued before the edit"), (out[1], after, "enqueued after the edit")):
            got = t_out.cpu().numpy(), p_out.cpu().numpy()
            bad = differ(got, want)
            assert not bad.any(), f"{kind}, {what}: {bad.sum()} of {n} answers are not the oracle's for that geometry"
            assert np.array_equal(a_out.cpu().numpy(), (want[1] >= 0).astype(np.int32)), f"{kind}, {what}, any mode"


# ---- F: pointer alignment ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_rays_and_outputs_at_four_byte_alignment(oracle):
    import torch
    d, rays, tuv, prim, _ = uneven_set(oracle, "bunny")
    n = 1000
    with opened(d) as ds:
        for refill, blocks in ((0, 0), (1, 2)):
            schedule(ds, refill, blocks)
            aligned = ds.trace_rays(rays[:n]), ds.trace_rays(rays[:n], mode=PT_QUERY_ANY)
            assert not differ(aligned[0], (tuv[:n], prim[:n])).any()
            r = torch.zeros(8 * n + 1, device="cuda")
            r[1:] = torch.from_numpy(rays[:n].copy()).cuda().reshape(-1)
            t_out = torch.full((3 * n + 2,), -7.0, device="cuda")
            p_out = torch.full((n + 2,), -7, device="cuda", dtype=torch.int32)
            a_out = torch.full((n + 2,), -7, device="cuda", dtype=torch.int32)
            assert r.data_ptr() % 16 == 0 and t_out.data_ptr() % 16 == 0 and p_out.data_ptr() % 16 == 0
            ds.trace_rays_into(r.data_ptr() + 4, n, t_out.data_ptr() + 4, p_out.data_ptr() + 4)
            ds.trace_rays_into(r.data_ptr() + 4, n, 0, a_out.data_ptr() + 4, mode=PT_QUERY_ANY)
            torch.cuda.synchronize()
            t_np, p_np, a_np = t_out.cpu().numpy(), p_out.cpu().numpy(), a_out.cpu().numpy()
            what = f"base + 4 bytes, query_refill={refill} query_blocks={blocks}"
            assert np.array_equal(p_np[1:-1], aligned[0][1]) and np.array_equal(a_np[1:-1], aligned[1]), what
            assert_bit_equal(t_np[1:-1].reshape(n, 3), aligned[0][0], what)
            assert p_np[0] == p_np[-1] == a_np[0] == a_np[-1] == -7 and t_np[0] == t_np[-1] == -7.0, what + ": a neighbour was written"
