"""pt_scene_update across what its contract allows (include/pt_api.h), beyond the moved vertices of
tests/test_scene_update.py: every launch shape of the device refit on caller's trees built for it, shapes that change type, a
mesh table that changes, ids and indices that change, refusals, and the two makers of primitive records against each other.

The statement is the header's: an updated handle renders, bit for bit and through every entry point, what a fresh
pt_scene_create of the new desc with host.refit_bvh's nodes renders.  Every comparison is bit-exact; the references are the CPU
oracle, a fresh create, and the numpy restatements of test_scene_update_plan.py (plan, refit) and test_motion.py (motion).
Inputs come from tests/scene_update_cases.py.

The refit's two constants (csrc/pt_scene_refit.hip) are restated in scene_update_cases: kNarrow = 1024 nodes per level,
kWholeTreeNodes = 4096 inner nodes.  The caller's trees of part A, by inner nodes per level (TOP = 1, 2, 4, ..., 1024: 2047 nodes):
  n1            one shape, no tree                                   no refit at all (n_trees == 0)
  n2, n3        [1], [1, 1]                                          one launch; levels == 1, levels == 2
  chain65       [1, 2, 1 x 61]: 64 levels with the leaves'           one launch; the deepest tree pt_scene_create accepts
  complete2048  TOP                                                  one launch; the widest level == kNarrow
  chains4097    TOP + [1024, 1024, 1]: 4096 nodes                    one launch; nodes == kWholeTreeNodes
  chains4098    TOP + [1024, 1024, 2]: 4097 nodes                    scatter + the single-workgroup launch, no level launch
  chains5120    TOP + [1024, 1024, 1024]: 5119 nodes                 the same, every level below the top == kNarrow
  heap4097      [1, 2, ..., 2048, 1]: 4096 nodes                     level launches + narrow top
  bulge3106     TOP + [1025, 30, 3]                                  one wide level between narrow ones"""
import ctypes as C

import numpy as np
import pytest
import scene_update_cases as cases
from conftest import assert_bit_equal
from scene_update_cases import (LEVELS_AND_TOP, NONE, ONE_LAUNCH, REFIT_SHAPE, REGIME_INPUTS, TOP_ALONE, classify, level_widths,
                                regime_input, sweep_widths)
from test_scene_update_plan import inner_only, leaf_boxes, pool, refit

from pathtracer_cuda_interactive_amd import (PT_ERR_BAD_SCENE, PT_ERR_INVALID_ARG, PT_ERR_UNSUPPORTED, PT_RENDER_NEE, PT_TRAVERSAL_EXACT,
                                             PT_TRAVERSAL_PRUNED, PtError, PtMaterial, host)
from pathtracer_cuda_interactive_amd import device as dev

A_NAMES = list(REGIME_INPUTS)
assert (cases.K_NARROW, cases.K_WHOLE_TREE_NODES) == (1024, 4096)               # csrc/pt_scene_refit.hip: kNarrow, kWholeTreeNodes
INFO_KEYS = ("fast_tree", "fast_tree_is_callers", "residency", "sweep_on_device", "refit_shape0", "refit_shape1")


# ---- CPU --------------------------------------------------------------------------------------------------------------------

def test_edited_desc_replaces_shape_list_and_mesh_table():
    hs, d, _ = cases.b_scene("lds", False)
    same = dev.edited_desc(d)
    assert (same.num_shapes, same.num_meshes, same.num_nodes) == (d.num_shapes, d.num_meshes, d.num_nodes)
    assert C.addressof(same.shapes.contents) == C.addressof(d.shapes.contents) and C.addressof(same.meshes.contents) == C.addressof(d.meshes.contents)
    shp = cases.shape_table(d)
    with pytest.raises(ValueError):
        dev.edited_desc(d, shapes=cases.as_shapes(shp[:-1]))
    with pytest.raises(ValueError):
        dev.edited_desc(d, shapes=list(cases.as_shapes(shp)) + [cases.as_shapes(shp)[0]])
    e = cases.edit_split(d)
    assert (e.num_meshes, e.num_shapes) == (36, d.num_shapes) and C.addressof(e.nodes.contents) == C.addressof(d.nodes.contents)
    # the same triangles and spheres: the leaf boxes are d's
    assert np.array_equal(leaf_boxes(e), leaf_boxes(d))
    assert np.array_equal(leaf_boxes(cases.edit_merged(d)), leaf_boxes(d))
    none = dev.edited_desc(cases.sphere_scene(40)[1], mesh_list=[])
    assert none.num_meshes == 0 and not none.meshes
    # `meshes` edits the table mesh_list gives, `spheres` the list `shapes` gives
    tab = cases.mesh_table(d)
    both = dev.edited_desc(d, mesh_list=tab[:1], meshes={0: (tab[0][0] + np.float32(1), None)})
    assert both.num_meshes == 1 and both.meshes[0].positions[0] == tab[0][0][0, 0] + np.float32(1)
    with pytest.raises(ValueError):
        dev.edited_desc(d, mesh_list=tab[:1], meshes={1: (tab[1][0], None)})
    s = int(np.flatnonzero(shp["type"] == 0)[0])
    with pytest.raises(ValueError):                            # after this replacement shape s is a triangle
        dev.edited_desc(d, shapes=cases.as_shapes(cases.spheres_to_triangles(d, [s])), spheres={s: ((0, 0, 0), 1.0)})


def test_the_trees_have_the_widths_the_table_states():
    for name, (n_tris, n_spheres, widths, aim) in REGIME_INPUTS.items():
        d0 = regime_input(name)[1]
        assert level_widths(d0) == widths, name
        assert classify(widths) == aim, name
    assert cases.tree_depth(regime_input("chain65")[1]) == 64
    w = REGIME_INPUTS["complete2048"][2]
    assert max(w) == cases.K_NARROW
    assert sum(REGIME_INPUTS["chains4097"][2]) == cases.K_WHOLE_TREE_NODES == sum(REGIME_INPUTS["chains4098"][2]) - 1
    assert set(REGIME_INPUTS["chains5120"][2][1 + 10:]) == {cases.K_NARROW} and sum(REGIME_INPUTS["chains5120"][2]) == 5119
    w = REGIME_INPUTS["bulge3106"][2]
    assert w[11] == cases.K_NARROW + 1 and max(w[:11] + w[12:]) <= cases.K_NARROW


def regime_classes():
    """name -> (class of the caller's tree, class of the library's internal tree over the same leaf boxes)."""
    return {name: (classify(level_widths(regime_input(name)[1])), classify(sweep_widths(name))) for name in A_NAMES}


def assert_coverage(classes):
    callers = {c for c, _ in classes.values()}
    assert callers == {NONE, ONE_LAUNCH, LEVELS_AND_TOP, TOP_ALONE}, classes
    assert any(i == LEVELS_AND_TOP for _, i in classes.values()), classes
    # the mixed path of update_scene: one of a handle's two trees done by one launch, the other not
    assert any(i is not None and NONE not in (c, i) and (c == ONE_LAUNCH) != (i == ONE_LAUNCH) for c, i in classes.values()), classes


def test_the_inputs_reach_every_refit_shape_and_the_mixed_path():
    classes = regime_classes()
    print({name: (c, i, sweep_widths(name)) for name, (c, i) in classes.items()})
    assert_coverage(classes)


@pytest.mark.parametrize("name", A_NAMES)
def test_host_refit_of_every_edited_input_is_the_numpy_refit(name):
    d1 = regime_input(name)[2]
    want = pool(host.refit_bvh(d1))
    boxes = leaf_boxes(d1)
    leaves = want["prim"] >= 0
    assert np.array_equal(want["bmin"][leaves], boxes[want["prim"][leaves], :3]) and np.array_equal(want["bmax"][leaves], boxes[want["prim"][leaves], 3:])
    assert not np.array_equal(boxes, leaf_boxes(regime_input(name)[1])), "the edit moves every box"
    if d1.num_shapes < 2:
        return
    child, inner = inner_only(d1, seed=3)
    slots = refit(child, d1.num_shapes, boxes)
    assert not np.isnan(slots).any()
    for side, field in ((0, "left"), (1, "right")):
        kids = want[field][inner]
        assert np.array_equal(slots[side::2, :3], want["bmin"][kids]) and np.array_equal(slots[side::2, 3:], want["bmax"][kids])


# ---- GPU: shared comparisons ------------------------------------------------------------------------------------------------

_oracle_frames = {}
RAYS = cases.scene_rays(4000, 5)
RAYS.setflags(write=False)


def oracle_frame(oracle, key, d, p):
    """The oracle's (image, counters) of one desc and frame: rendered once, shared, left unchanged."""
    key = (key, p.flags, p.seed)
    if key not in _oracle_frames:
        _oracle_frames[key] = oracle.render(d, p)
        _oracle_frames[key][0].setflags(write=False)
    return _oracle_frames[key]


def with_nee(p):
    q = p.copy()
    q.flags = PT_RENDER_NEE
    return q


def infos(S):
    return {k: S.info(k) for k in INFO_KEYS}


def assert_same_outputs(oracle, S, F, p, dr, key, what, rays=RAYS):
    """Frames under both traversals on both trees, pt_debug_intersect and the AOV buffers of handle S against handle F, a fresh
    create of `dr`; exact frames against the oracle's of `dr` as well."""
    want = oracle_frame(oracle, key, dr, p)[0]
    for fast in (1, 0):
        S.set_option("fast_tree", fast)
        F.set_option("fast_tree", fast)
        for trav in (PT_TRAVERSAL_EXACT, PT_TRAVERSAL_PRUNED):
            w = f"{what} fast_tree={fast} traversal={trav}"
            img = S.render(p, traversal=trav)
            assert_bit_equal(img, F.render(p, traversal=trav), w + " vs fresh create")
            if trav == PT_TRAVERSAL_EXACT:
                assert_bit_equal(img, want, w + " vs oracle")
            tuv, prim = S.intersect(rays, trav)
            tuv_f, prim_f = F.intersect(rays, trav)
            assert np.array_equal(prim, prim_f), w + " intersect"
            assert_bit_equal(tuv, tuv_f, w + " intersect")
        a, b = S.render_aov(p), F.render_aov(p)
        assert np.array_equal(a["prim"], b["prim"]), f"{what} fast_tree={fast} aov prim"
        for k in ("albedo", "normal", "depth"):
            assert_bit_equal(a[k], b[k], f"{what} fast_tree={fast} aov {k}")
    S.set_option("fast_tree", 1)
    F.set_option("fast_tree", 1)
    return prim


def assert_same_entry_points(oracle, S, F, p, dr, key, what):
    """The other ways to a frame: pt_render_adaptive, pt_render_accumulate over two calls, option kernel = 3, next-event estimation."""
    import torch
    a, b = S.render_adaptive(p, 0.3, batch_spp=2, max_spp=8), F.render_adaptive(p, 0.3, batch_spp=2, max_spp=8)
    assert np.array_equal(a[1], b[1]), what + " adaptive spp_map"
    assert a[1].min() >= p.spp and a[1].max() <= 8 and len(np.unique(a[1])) > 1, "the noise target stops some pixels early, not all"
    assert_bit_equal(a[0], b[0], what + " adaptive image")
    assert_bit_equal(a[2], b[2], what + " adaptive err_map")
    acc = [torch.zeros((p.height, p.width, 3), dtype=torch.float32, device="cuda") for _ in range(2)]
    total = None
    for off in (0, p.spp):
        q = p.copy()
        q.sample_offset, q.stream_stride = off, 2 * p.spp
        for ds, buf in zip((S, F), acc):
            ds.accumulate_into(q, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        part = oracle.render(dr, q, accumulate=True)[0]
        total = part if total is None else (total + part).astype(np.float32)
    got = acc[0].cpu().numpy()
    assert_bit_equal(got, acc[1].cpu().numpy(), what + " accumulate vs fresh create")
    assert_bit_equal(got, total, what + " accumulate vs oracle")
    want = oracle_frame(oracle, key, dr, p)[0]
    for ds in (S, F):
        ds.set_option("kernel", 3)
    try:
        img = S.render(p)
        assert_bit_equal(img, F.render(p), what + " kernel 3 vs fresh create")
        assert_bit_equal(img, want, what + " kernel 3 vs oracle")
        assert S.info("kernel") == F.info("kernel") == 3 and S.info("trace_variant") == F.info("trace_variant")
    finally:
        for ds in (S, F):
            ds.set_option("kernel", 2)
    q = with_nee(p)
    img = S.render(q)
    assert not np.array_equal(img, want), "next-event estimation changes the estimator"
    assert_bit_equal(img, F.render(q), what + " NEE vs fresh create")
    assert_bit_equal(img, oracle_frame(oracle, key, dr, q)[0], what + " NEE vs oracle")
    assert S.info("trace_variant") == F.info("trace_variant")


def assert_exact_boxes(S, p, want, cnt, what):
    """test_scene_update's counter pin on the caller's tree: the oracle's inner pops and leaf tests exactly, which boxes that
    are conservative but not tight would exceed while rendering the same image.  Leaves the handle with stats on."""
    S.set_option("stats", 1)
    S.set_option("fast_tree", 0)
    assert_bit_equal(S.render(p), want, what + " caller's tree, stats build")
    c = S.counters()
    assert (c.paths, c.segments) == (cnt.paths, cnt.segments), what
    assert c.node_visits == cnt.inner_pops, (what, c.node_visits, cnt.inner_pops)
    assert c.leaf_tests == cnt.leaf_tri + cnt.leaf_sphere, (what, c.leaf_tests, cnt.leaf_tri + cnt.leaf_sphere)
    S.set_option("fast_tree", 1)


def assert_same_work(S, Z, p, what):
    """Both handles render the same frame visiting the same number of nodes and leaves, on either tree (stats on)."""
    for fast in (1, 0):
        S.set_option("fast_tree", fast)
        Z.set_option("fast_tree", fast)
        assert S.info("fast_tree_on") == Z.info("fast_tree_on")
        assert_bit_equal(S.render(p), Z.render(p), f"{what} fast_tree={fast}")
        cs, cz = S.counters(), Z.counters()
        assert (cs.paths, cs.segments, cs.node_visits, cs.leaf_tests) == (cz.paths, cz.segments, cz.node_visits, cz.leaf_tests), (what, fast)
    S.set_option("fast_tree", 1)
    Z.set_option("fast_tree", 1)


class handles:
    """DeviceScenes of the listed descs, closed on the way out."""

    def __init__(self, *descs):
        self.descs = descs

    def __enter__(self):
        self.open = []
        try:
            for d in self.descs:
                self.open.append(dev.DeviceScene(d))
        except Exception:
            self.__exit__()
            raise
        return self.open

    def __exit__(self, *exc):
        for ds in self.open:
            ds.close()


def expected_shapes(name, info):
    """(refit_shape0, refit_shape1) a handle of regime input `name` must report after a geometry update, from the numpy plan."""
    d0 = regime_input(name)[1]
    own = classify(level_widths(d0))
    if not info["fast_tree"] or own == NONE:
        return own, NONE
    return own, own if info["fast_tree_is_callers"] else classify(sweep_widths(name))


# ---- A: refit regimes -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", A_NAMES)
def test_update_on_a_callers_tree_of_every_refit_shape(oracle, name):
    hs, d0, d1, d1r, p = regime_input(name)
    want, cnt = oracle_frame(oracle, ("A", name), d1r, p)
    with handles(d0, d1r, d0) as (S, F, Z):
        before = S.render(p)
        assert (S.info("refit_shape0"), S.info("refit_shape1")) == (0, 0)
        S.update(d1)
        info = infos(S)
        print(name, info)
        assert tuple(REFIT_SHAPE[info[k]] for k in ("refit_shape0", "refit_shape1")) == expected_shapes(name, info), info
        assert REFIT_SHAPE[info["refit_shape0"]] == REGIME_INPUTS[name][3]
        assert not np.array_equal(before, want), "the edit does not show in the image"
        prim = assert_same_outputs(oracle, S, F, p, d1r, ("A", name), name)
        assert (prim >= 0).sum() > (100 if d0.num_shapes > 3 else 0)
        assert_exact_boxes(S, p, want, cnt, name)
        # back to d0: the frames and the work of a handle that was never updated
        S.update(d0)
        assert S.info("updates") == 2 and S.info("update_us3") == 0
        Z.set_option("stats", 1)
        assert_same_work(S, Z, p, name + " back at d0")


@pytest.mark.gpu
def test_the_handles_report_every_refit_shape_and_the_mixed_path():
    report = {}
    for name in A_NAMES:
        _, d0, d1, _, _ = regime_input(name)
        with handles(d0) as (S,):
            S.update(d1)
            report[name] = infos(S)
            assert tuple(REFIT_SHAPE[report[name][k]] for k in ("refit_shape0", "refit_shape1")) == expected_shapes(name, report[name]), (name, report[name])
    print(report)
    # an internal tree counts where the handle kept the sweep tree; its shape is what the handle reports
    classes = {name: (REFIT_SHAPE[i["refit_shape0"]], REFIT_SHAPE[i["refit_shape1"]] if i["fast_tree"] and not i["fast_tree_is_callers"] else None)
               for name, i in report.items()}
    assert_coverage(classes)


# ---- B: what a geometry update may change -----------------------------------------------------------------------------------

B_CASES = [(s, dif) for s in ("lds", "global") for dif in (True, False)]
B_IDS = [f"{s}-{'diffuse' if dif else 'mixed'}" for s, dif in B_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("edit", ["types", "merged", "split70", "ids", "rewired", "emitter_moved"])
@pytest.mark.parametrize("scene,diffuse_only", B_CASES, ids=B_IDS)
def test_update_to_another_shape_list_mesh_table_ids_or_indices(oracle, scene, diffuse_only, edit):
    hs, d0, p = cases.b_scene(scene, diffuse_only)
    d1, d1r = cases.b_edit(scene, diffuse_only, edit)
    key = ("B", scene, diffuse_only, edit)
    what = f"{scene} diffuse_only={diffuse_only} {edit}"
    want, cnt = oracle_frame(oracle, key, d1r, p)
    with handles(d0, d1r) as (S, F):
        before = S.render(p)
        assert S.info("residency") == (2 if scene == "lds" else 3)
        S.update(d1)
        print(what, infos(S))
        assert not np.array_equal(before, want), "the edit does not show in the image"
        assert_same_outputs(oracle, S, F, p, d1r, key, what)
        assert_same_entry_points(oracle, S, F, p, d1r, key, what)
        if edit == "types":
            from test_motion import moved, numpy_motion
            q = hs.render_params(cases.W, cases.H, 1)
            prev = moved(q, (0.1, 0.04, -0.07))
            m_want = numpy_motion(oracle, d1r, d0, q, prev)
            cur, old = cases.shape_table(d1)["type"], cases.shape_table(d0)["type"]
            g = S.render_guides(q, prev, previous_geometry=True)
            changed = (g["prim"] >= 0) & (cur[np.maximum(g["prim"], 0)] != old[np.maximum(g["prim"], 0)])
            assert changed.sum() > 0 and (g["prev_depth"][changed] == 0).all(), "a pixel whose record changed type is invalid"
            assert_bit_equal(g["motion"], m_want[0], what + " motion")
            assert_bit_equal(g["prev_depth"], m_want[1], what + " prev_depth")
        assert_exact_boxes(S, p, want, cnt, what)


@pytest.mark.gpu
@pytest.mark.parametrize("scene,diffuse_only", B_CASES, ids=B_IDS)
def test_the_last_sphere_goes_and_comes_back(oracle, scene, diffuse_only):
    from trace_variants import Variant
    hs, d0, p = cases.b_scene(scene, diffuse_only)
    d1, d1r = cases.b_edit(scene, diffuse_only, "no_sphere")
    key = ("B", scene, diffuse_only, "no_sphere")
    what = f"{scene} diffuse_only={diffuse_only}"
    with handles(d0, d1r, d0) as (S, F, Z):
        S.render(p)
        with_spheres = (S.info("trace_variant"), S.info("path_bank"))
        assert Variant.decode(with_spheres[0]).spec == 0 and with_spheres[1] == 0
        S.update(d1)
        S.render(p)
        without = (S.info("trace_variant"), S.info("path_bank"))
        F.render(p)
        print(what, str(Variant.decode(with_spheres[0])), "->", str(Variant.decode(without[0])), "path_bank", without[1])
        assert without[0] != with_spheres[0] and Variant.decode(without[0]).spec == (2 if diffuse_only else 1)
        assert without == (F.info("trace_variant"), F.info("path_bank"))
        if scene == "lds" and diffuse_only:
            assert without[1] == 1
        assert_same_outputs(oracle, S, F, p, d1r, key, what + " without spheres")
        assert_same_entry_points(oracle, S, F, p, d1r, key, what + " without spheres")
        S.update(d0)
        S.render(p)
        assert (S.info("trace_variant"), S.info("path_bank")) == with_spheres
        assert_same_outputs(oracle, S, Z, p, d0, ("B", scene, diffuse_only, "d0"), what + " spheres back")
        assert_same_entry_points(oracle, S, Z, p, d0, ("B", scene, diffuse_only, "d0"), what + " spheres back")


@pytest.mark.gpu
def test_a_scene_of_spheres_without_a_single_mesh(oracle):
    # as an update, on the host's record loop's side of the create threshold ...
    hs, d0, d1, d1r, p = cases.sphere_scene(40)
    with handles(d0, d1r) as (S, F):
        S.update(d1)
        assert_same_outputs(oracle, S, F, p, d1r, ("spheres", 40), "40 spheres")
        assert_same_entry_points(oracle, S, F, p, d1r, ("spheres", 40), "40 spheres")
    # ... and as a create from 4096 shapes up, where prims_kernel makes the records; then updated as well
    hs, d0, d1, d1r, p = cases.sphere_scene(4096)
    with handles(d0, d1r) as (S, F):
        assert S.info("sweep_on_device") == 1
        assert_bit_equal(S.render(p), oracle_frame(oracle, ("spheres", 4096, 0), d0, p)[0], "4096 spheres, created")
        S.update(d1)
        assert_same_outputs(oracle, S, F, p, d1r, ("spheres", 4096), "4096 spheres")


# ---- C: refusals ------------------------------------------------------------------------------------------------------------

def raw_update_status(S, desc, flags):
    rc = dev.lib().pt_scene_update(S._h, C.byref(desc), flags)
    return rc, dev.lib().pt_last_error().decode()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n1", "complete2048", "heap4097"])
def test_a_refused_update_leaves_the_handle_as_it_was(oracle, name):
    hs, d0, d1, d1r, p = regime_input(name)
    want = oracle_frame(oracle, ("A", name), d1r, p)[0]
    with handles(d0, d1r) as (S, F):
        S.update(d1)
        frames = {}
        for fast in (1, 0):
            S.set_option("fast_tree", fast)
            frames[fast] = S.render(p)
            assert_bit_equal(frames[fast], want, f"before, fast_tree={fast}")

        def refused(desc, status, word, flags=1):
            rc, msg = raw_update_status(S, desc, flags)
            assert rc == status and word in msg, (rc, msg, word)
            assert S.info("updates") == 1
            for fast in (1, 0):
                S.set_option("fast_tree", fast)
                assert_bit_equal(S.render(p), frames[fast], f"after the refused update ({word}), fast_tree={fast}")

        for msg, bad in cases.bad_id_descs(d0).items():
            refused(bad, PT_ERR_BAD_SCENE, msg)
        for what, bad in cases.not_finite_descs(d0).items():
            refused(bad, PT_ERR_UNSUPPORTED, "not finite")
        # counts that must be create's, through the C API itself (edited_desc refuses to make such a desc)
        short = dev.edited_desc(d1)
        short.num_shapes = d0.num_shapes + 1
        refused(short, PT_ERR_INVALID_ARG, "num_shapes")
        if d0.num_shapes > 1:
            short.num_shapes = d0.num_shapes - 1
            refused(short, PT_ERR_INVALID_ARG, "num_shapes")
        mats = [PtMaterial.from_buffer_copy(d0.materials[m]) for m in range(d0.num_materials)]
        other = dev.edited_desc(d1, materials=mats)
        other.num_materials = d0.num_materials - 1
        refused(other, PT_ERR_INVALID_ARG, "num_materials", flags=3)
        refused(other, PT_ERR_INVALID_ARG, "num_materials", flags=2)
        other = dev.edited_desc(d1)
        other.num_lights = d0.num_lights + 1
        refused(other, PT_ERR_INVALID_ARG, "num_lights", flags=3)
        # a NaN that no shape uses is no reason to refuse: accepted, and rendered like the fresh create
        ok = cases.unused_nan_desc(d0)
        okr = host.refit_bvh(ok)
        S.update(ok)
        assert S.info("updates") == 2
        with handles(okr) as (G,):
            assert_same_outputs(oracle, S, G, p, okr, ("C", name, "unused nan"), name + " unused NaN vertex")
        # and the handle still takes a good update
        S.update(d1)
        assert S.info("updates") == 3
        assert_same_outputs(oracle, S, F, p, d1r, ("A", name), name + " a good update after the refusals")


@pytest.mark.gpu
def test_a_big_create_refuses_bad_ids_as_the_host_loop_does(monkeypatch):
    d0 = regime_input("heap4097")[1]
    assert d0.num_shapes >= 4096
    for msg, bad in cases.bad_id_descs(d0).items():
        got = {}
        for build in ("device", "host"):
            if build == "host":
                monkeypatch.setenv("PT_SWEEP_BUILD", "host")
            else:
                monkeypatch.delenv("PT_SWEEP_BUILD", raising=False)
            with pytest.raises(PtError) as e:
                dev.DeviceScene(bad).close()
            got[build] = (e.value.status, str(e.value))
        assert got["device"] == got["host"] and got["host"][0] == PT_ERR_BAD_SCENE and msg in got["host"][1], (msg, got)
    monkeypatch.delenv("PT_SWEEP_BUILD", raising=False)
    with handles(d0) as (S,):
        assert S.info("sweep_on_device") == 1, "a good create of this size takes the device path"


# ---- D: the two record makers agree -----------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_device_and_host_record_makers_agree_on_a_scene_of_70_meshes(oracle, monkeypatch):
    from test_aov import numpy_guides
    hs, d, p = cases.many_meshes_scene()
    assert d.num_shapes >= 4096 and d.num_meshes == 70 and d.num_lights > 1
    assert {d.materials[m].type for m in range(d.num_materials)} == {0, 1, 2, 3}
    monkeypatch.delenv("PT_SWEEP_BUILD", raising=False)
    D = dev.DeviceScene(d)
    monkeypatch.setenv("PT_SWEEP_BUILD", "host")
    Hh = dev.DeviceScene(d)
    monkeypatch.delenv("PT_SWEEP_BUILD", raising=False)
    try:
        assert (D.info("sweep_on_device"), Hh.info("sweep_on_device")) == (1, 0)
        rays = cases.scene_rays(20000, 9)
        prim = assert_same_outputs(oracle, D, Hh, p, d, ("D",), "device records vs host records", rays=rays)
        tuv, prim = D.intersect(rays, PT_TRAVERSAL_EXACT)
        tuv_o, prim_o = oracle.intersect(d, rays)
        assert (prim >= 0).sum() > 2000 and np.array_equal(prim, prim_o)
        assert_bit_equal(tuv, tuv_o, "intersect vs oracle")
        a, g = D.render_aov(p), numpy_guides(oracle, d, p)
        assert np.array_equal(a["prim"], g["prim"])
        for k in ("albedo", "normal", "depth"):
            assert_bit_equal(a[k], g[k], "aov vs numpy " + k)
        q = with_nee(p)
        img = D.render(q)
        assert_bit_equal(img, Hh.render(q), "NEE, device records vs host records")
        assert_bit_equal(img, oracle_frame(oracle, ("D",), d, q)[0], "NEE vs oracle")
    finally:
        D.close()
        Hh.close()
