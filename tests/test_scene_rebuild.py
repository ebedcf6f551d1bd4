"""pt_scene_rebuild: a fresh internal tree on a live handle, the tree-cost telemetry and the rebuild policy.

The statement under test: a handle that was transformed and then rebuilt IS a freshly created handle of the moved scene — frame
for frame through every entry point, node visit for node visit, info key for info key — that has kept its records, groups and
options.  Inputs: scene_rebuild_cases.py (the shuffled grids of 96, 324 and 4,116 shapes; the Cornell box with its blocks
translated)."""
import math

import numpy as np
import pytest
import scene_rebuild_cases as rc
from conftest import assert_bit_equal, assert_work_counters, load_scene

from pathtracer_cuda_interactive_amd import (PT_ERR_INVALID_ARG, PT_ERR_UNSUPPORTED, PT_QUERY_ANY, PT_QUERY_CLOSEST, PT_RENDER_NEE,
                                             PT_TRAVERSAL_EXACT, PT_TRAVERSAL_PRUNED, PtError, host)
from pathtracer_cuda_interactive_amd import device as dev

NAMES = ["grid2", "grid3", "grid7", "cbox"]
INFO = ("fast_tree", "fast_tree_is_callers", "fast_tree_depth", "stack_entries", "fast_tree_cost_permille", "residency", "top_nodes",
        "sweep_boxes", "sweep_on_device")
COST_KEYS = ("tree_cost0_bits", "tree_cost1_bits", "tree_cost0_permille", "tree_cost1_permille")


class closing:
    def __init__(self, *scenes):
        self.scenes = scenes

    def __enter__(self):
        return self.scenes

    def __exit__(self, *exc):
        for s in self.scenes:
            s.close()


def moved(c, M):
    """A handle of the rest scene with its groups set and transformed by M."""
    S = dev.DeviceScene(c["d0"])
    S.set_groups(c["ids"], M.shape[0])
    S.transform(M)
    return S


def frames(S, p, rays):
    """Everything the statement covers, as a dict of arrays: frames under exact and pruned traversal on both trees, next-event
    estimation, the four guide buffers, the ray queries, the adaptive sample counts."""
    out = {}
    for fast in (0, 1):
        S.set_option("fast_tree", fast)
        for trav in (PT_TRAVERSAL_EXACT, PT_TRAVERSAL_PRUNED):
            out[f"frame fast_tree={fast} traversal={trav}"] = S.render(p, traversal=trav)
    q = p.copy()
    q.flags = PT_RENDER_NEE
    out["frame nee"] = S.render(q)
    for k, v in S.render_aov(p).items():
        out["aov " + k] = v
    tuv, prim = S.trace_rays(rays, PT_QUERY_CLOSEST)
    out["closest tuv"], out["closest prim"], out["any"] = tuv, prim, S.trace_rays(rays, PT_QUERY_ANY)
    out["spp_map"] = S.render_adaptive(p, 0.05, batch_spp=2, max_spp=8)[1]
    return out


def assert_same_frames(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if a[k].dtype == np.float32:
            assert_bit_equal(a[k], b[k], f"{what}: {k}")
        else:
            assert np.array_equal(a[k], b[k]), f"{what}: {k}"


def work(S, p):
    """(node_visits, leaf_tests, redo_segments) of an exact STATS render on the internal tree; the counters object as well."""
    S.set_option("stats", 1)
    S.set_option("fast_tree", 1)
    S.render(p, traversal=PT_TRAVERSAL_EXACT)
    c = S.counters()
    w = (c.node_visits, c.leaf_tests, S.info("redo_segments"))
    S.set_option("stats", 0)
    return w, c


def info(S, p, keys=INFO):
    """The compared info keys, and what a plain render then ran on."""
    S.set_option("fast_tree", 1)
    out = {k: S.info(k) for k in keys}
    S.render(p, traversal=PT_TRAVERSAL_EXACT)
    out["leaf_sweep"], out["reg_stack"] = S.info("leaf_sweep"), S.info("reg_stack")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_a_rebuilt_handle_equals_a_fresh_create(oracle, name):
    c = rc.case(name)
    p, rays = c["p"], c["rays"]
    with closing(moved(c, c["M1"]), dev.DeviceScene(c["d1r"])) as (A, F):
        (visits_before, _, _), _ = work(A, p)
        assert A.info("rebuilds") == 0
        adopted = A.rebuild()
        assert (A.info("rebuilds"), A.info("rebuild_adopted")) == (1, int(adopted))
        assert A.info("rebuild_us0") >= A.info("rebuild_us1") > 0
        assert adopted == bool(F.info("fast_tree") and not F.info("fast_tree_is_callers"))
        assert A.info("rebuild_cost_permille") == F.info("fast_tree_cost_permille")
        assert_same_frames(frames(A, p, rays), frames(F, p, rays), name)
        wa, ca = work(A, p)
        wf, _ = work(F, p)
        print(f"{name}: node_visits before the rebuild {visits_before}, after {wa[0]}, fresh create {wf[0]}")
        assert wa == wf
        _, cnt = oracle.render(c["d1r"], p)
        A.set_option("stats", 1)
        assert_work_counters(A, ca, cnt, oracle, c["d1r"], p, name)
        A.set_option("stats", 0)
        assert info(A, p) == info(F, p)
        if name in ("grid3", "grid7"):
            assert visits_before > wa[0]
        assert A.info("sweep_on_device") == (1 if name == "grid7" else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_a_rebuilt_handle_goes_on_living(name):
    c = rc.case(name)
    p, rays = c["p"], c["rays"]
    G = c["M1"].shape[0]
    with closing(moved(c, c["M1"]), moved(c, c["M1"]), dev.DeviceScene(c["d2r"]), dev.DeviceScene(c["d0"])) as (A, B, F2, D0):
        state = (A.info("prev_geometry"), A.info("rest_geometry"), A.info("groups"), A.info("transforms"))
        assert state == (1, 1, G, 1)
        A.rebuild()
        assert (A.info("prev_geometry"), A.info("rest_geometry"), A.info("groups"), A.info("transforms")) == state
        A.transform(c["M2"])
        assert A.info("refit_shape1") != 0 and A.info("transform_us3") == 0, "the new tree's plan was made by the rebuild"
        B.transform(c["M2"])
        fa = frames(A, p, rays)
        assert_same_frames(fa, frames(B, p, rays), name + " vs a handle that never rebuilt")
        assert_same_frames(fa, frames(F2, p, rays), name + " vs a fresh create")
        A.transform(np.stack([rc.IDENTITY] * G))
        assert_same_frames(frames(A, p, rays), frames(D0, p, rays), name + " back at rest vs a never-updated handle")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grid3", "cbox"])
def test_motion_vectors_carry_on_across_a_rebuild(name):
    c = rc.case(name)
    p = c["p"]
    root = c["d0"].nodes[c["d0"].root]
    size = float(max(root.bmax[k] - root.bmin[k] for k in range(3)))
    prev_cam = dev.translated_params(p, np.array([0.02, -0.01, 0.03]) * size)
    with closing(moved(c, c["M1"]), moved(c, c["M1"])) as (A, B):
        A.transform(c["M2"])
        B.transform(c["M2"])
        A.rebuild()
        for previous in (True, False):
            a = A.render_guides(p, prev_cam, previous_geometry=previous)
            b = B.render_guides(p, prev_cam, previous_geometry=previous)
            assert np.array_equal(a["prim"], b["prim"])
            for k in ("albedo", "normal", "depth", "motion", "prev_depth"):
                assert_bit_equal(a[k], b[k], f"{name} previous_geometry={previous} {k}")


@pytest.mark.gpu
def test_the_box_sweep_comes_back():
    c = rc.cbox_case()
    p = c["p"]
    reached = {}
    for which in ("M1", "M2"):
        with closing(moved(c, c[which]), dev.DeviceScene(c["d1r" if which == "M1" else "d2r"])) as (A, F):
            assert A.info("sweep_boxes") == 0
            A.render(p)
            assert A.info("leaf_sweep") == 0
            A.rebuild()
            assert A.info("sweep_boxes") == F.info("sweep_boxes")
            img = A.render(p)
            assert_bit_equal(img, F.render(p), "cbox " + which)
            assert A.info("leaf_sweep") == F.info("leaf_sweep")
            reached[which] = (A.info("sweep_boxes"), A.info("leaf_sweep"))
    print("cbox (sweep_boxes, leaf_sweep) after the rebuild:", reached)
    assert any(v[1] == 1 for v in reached.values())


def inflated(d, factor):
    """desc on a pool whose every box is scaled about one centre: caller's boxes that are not the shapes' exact boxes and
    still nest (the map is monotone per axis, rounding included)."""
    nodes = rc.pool(d)
    ctr = 0.5 * (nodes["bmin"][d.root] + nodes["bmax"][d.root])
    nodes["bmin"] = ctr + np.float32(factor) * (nodes["bmin"] - ctr)
    nodes["bmax"] = ctr + np.float32(factor) * (nodes["bmax"] - ctr)
    return rc.desc_with_nodes(d, nodes)


def idempotent_input(kind):
    if kind == "inflated":
        c = rc.grid_case(3)
        return inflated(c["d0"], 1.25), c["p"], c["rays"]
    hs, d = load_scene(kind)
    p = hs.render_params(rc.W, rc.H, rc.SPP, seed=11)
    p.traversal = PT_TRAVERSAL_EXACT
    return d, p, rc.box_rays(d, rc.RAYS, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cbox", "teapot", "inflated"])
def test_rebuilding_a_never_updated_handle_changes_nothing(kind):
    d, p, rays = idempotent_input(kind)
    with closing(dev.DeviceScene(d)) as (A,):
        assert A.info("fast_tree") == 1
        want, want_work, want_info = frames(A, p, rays), work(A, p)[0], info(A, p)
        for n in (1, 2):
            A.rebuild()
            assert A.info("rebuilds") == n
            assert_same_frames(frames(A, p, rays), want, f"{kind} after rebuild {n}")
            assert work(A, p)[0] == want_work, "the leaf boxes are the caller's, not the shapes'"
            assert info(A, p) == want_info


@pytest.mark.gpu
def test_a_candidate_that_does_not_win_is_not_adopted():
    hs, d0 = load_scene("teapot")
    d, _ = dev.build_bvh_sweep(d0)                            # the caller's tree = what the library builds itself
    p = hs.render_params(rc.W, rc.H, rc.SPP, seed=6)
    with closing(dev.DeviceScene(d)) as (A,):
        assert (A.info("fast_tree_is_callers"), A.info("fast_tree_cost_permille")) == (1, 1000)
        want, want_work = A.render(p), work(A, p)[0]
        assert A.rebuild() is False
        assert (A.info("rebuilds"), A.info("rebuild_adopted"), A.info("rebuild_cost_permille"), A.info("fast_tree_is_callers")) == (1, 0, 1000, 1)
        assert_bit_equal(A.render(p), want, "not adopted")
        assert work(A, p)[0] == want_work
    c = rc.grid_case(3)
    ds, _ = dev.build_bvh_sweep(c["d0"])
    with closing(dev.DeviceScene(ds), dev.DeviceScene(c["d1r"])) as (A, F):
        assert A.info("fast_tree_is_callers") == 1
        A.set_groups(c["ids"], c["M1"].shape[0])
        A.transform(c["M1"])
        assert A.rebuild() is True
        assert (A.info("rebuild_adopted"), A.info("fast_tree_is_callers")) == (1, 0)
        assert_bit_equal(A.render(c["p"]), F.render(c["p"]), "adopted over the caller's topology")


@pytest.mark.gpu
def test_refusals_leave_the_handle_as_it_was():
    c = rc.grid_case(3)
    nodes = rc.pool(c["d0"])
    inner = [int(k) for k in np.flatnonzero(nodes["prim"] < 0) if int(k) != int(c["d0"].root)]
    for k in inner[::7]:                               # shrink some inner boxes: their children now stick out
        ctr = 0.5 * (nodes["bmin"][k] + nodes["bmax"][k])
        nodes["bmin"][k] = ctr + 0.6 * (nodes["bmin"][k] - ctr)
        nodes["bmax"][k] = ctr + 0.6 * (nodes["bmax"][k] - ctr)
    hs1, d_small = load_scene("scene1")
    assert d_small.num_shapes == 4
    cases = [("flags", c["d0"], c["p"], 1, PT_ERR_INVALID_ARG, "flags"),
             ("four shapes", d_small, hs1.render_params(rc.W, rc.H, rc.SPP, seed=3), 0, PT_ERR_UNSUPPORTED, "16 shapes"),
             ("not nested", rc.desc_with_nodes(c["d0"], nodes), c["p"], 0, PT_ERR_UNSUPPORTED, "nest")]
    for what, d, p, flags, status, word in cases:
        with closing(dev.DeviceScene(d)) as (A,):
            want = A.render(p)
            assert A.info("fast_tree") == (1 if what == "flags" else 0)
            rc_ = dev.lib().pt_scene_rebuild(A._h, flags)
            msg = dev.lib().pt_last_error().decode()
            assert rc_ == status and word in msg, (what, rc_, msg)
            assert A.info("rebuilds") == 0
            assert_bit_equal(A.render(p), want, what)
    assert dev.lib().pt_scene_rebuild(None, 0) == PT_ERR_INVALID_ARG


def f64(bits):
    return float(np.array([bits], np.int64).view(np.float64)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grid3", "grid7", "cbox"])
def test_tree_cost_telemetry(name):
    c = rc.case(name)
    rest1, _ = dev.build_bvh_sweep(c["d0"])
    now1 = host.refit_bvh(dev.transform_desc_host(rest1, c["ids"], c["M1"]))
    fresh1, _ = dev.build_bvh_sweep(c["d1r"])
    terms = {"ref0": rc.inner_terms(c["d0"]), "now0": rc.inner_terms(c["d1r"]), "ref1": rc.inner_terms(rest1), "now1": rc.inner_terms(now1),
             "fresh1": rc.inner_terms(fresh1)}
    exact = {k: math.fsum(v) for k, v in terms.items()}

    def close_to(bits, k):
        got = f64(bits)
        print(f"{name} {k}: device {got!r}, fsum {exact[k]!r}")
        return abs(got - exact[k]) <= rc.sum_bound(terms[k].size) * exact[k]

    runs = []
    for _ in range(2):
        with closing(dev.DeviceScene(c["d0"])) as (A,):
            A.set_option("tree_cost", 1)
            assert [A.info(k) for k in COST_KEYS] == [0, 0, 1000, 1000], "before any refit"
            A.set_groups(c["ids"], c["M1"].shape[0])
            A.transform(c["M1"])
            got = [A.info(k) for k in COST_KEYS]
            runs.append(got)
            assert close_to(got[0], "now0") and close_to(got[1], "now1")
            for t in (0, 1):
                assert got[2 + t] == int(1000.0 * exact[f"now{t}"] / exact[f"ref{t}"] + 0.5), (t, got, exact)
            if name != "cbox":
                assert got[3] > 1500
            adopted = A.rebuild()
            assert adopted or name == "cbox"
            assert A.info("tree_cost1_permille") == 1000, "the reference follows a rebuild, adopted or not"
            assert close_to(A.info("tree_cost1_bits"), "fresh1") if adopted else A.info("tree_cost1_bits") == got[1]
            assert A.info("tree_cost0_bits") == got[0] and A.info("tree_cost0_permille") == got[2]
            A.set_option("tree_cost", 0)
            assert [A.info(k) for k in COST_KEYS] == [0, 0, 1000, 1000], "option off"
    assert runs[0] == runs[1], "the same bits on every run"
    with closing(moved(c, c["M1"])) as (A,):
        assert [A.info(k) for k in COST_KEYS] == [0, 0, 1000, 1000], "never switched on"


@pytest.mark.gpu
def test_rebuild_policy():
    c = rc.grid_case(7)
    p = c["p"]
    G = c["M1"].shape[0]
    with closing(dev.DeviceScene(c["d0"]), dev.DeviceScene(c["d1r"]), dev.DeviceScene(c["d0"])) as (A, F, I):
        with pytest.raises(PtError) as e:
            A.set_option("rebuild_at_permille", 1000)
        assert e.value.status == PT_ERR_INVALID_ARG
        A.set_option("rebuild_at_permille", 1500)
        A.set_groups(c["ids"], G)
        A.transform(c["M1"])
        assert (A.info("rebuilds"), A.info("rebuilds_auto"), A.info("rebuild_adopted")) == (1, 1, 1)
        assert A.info("tree_cost1_permille") == 1000
        assert work(A, p)[0] == work(F, p)[0]
        assert_bit_equal(A.render(p), F.render(p), "policy")
        A.transform(c["M1"])
        assert (A.info("rebuilds"), A.info("rebuilds_auto")) == (1, 1), "nothing drifted since the rebuild"
        I.set_option("rebuild_at_permille", 1500)
        I.set_groups(c["ids"], G)
        I.transform(np.stack([rc.IDENTITY] * G))
        assert (I.info("rebuilds"), I.info("rebuilds_auto"), I.info("tree_cost1_permille")) == (0, 0, 1000)


@pytest.mark.gpu
def test_sharded_renderer_rebuild_on_a_one_rank_group():
    from pathtracer_cuda_interactive_amd import distributed as D
    c = rc.grid_case(3)
    p = c["p"]
    R = D.ShardedRenderer(c["d0"])
    try:
        R.scene.set_groups(c["ids"], c["M1"].shape[0])
        R.scene.transform(c["M1"])
        before = R.render(p, rank=0, world=1).cpu().numpy().copy()
        assert R.rebuild() is True
        after = R.render(p, rank=0, world=1).cpu().numpy()
        assert_bit_equal(after, before, "the frame does not depend on the tree")
        assert R.scene.info("rebuilds") == 1
    finally:
        R.close()
    with closing(dev.DeviceScene(c["d1r"])) as (F,):
        assert_bit_equal(after, F.render(p), "vs a fresh create")
