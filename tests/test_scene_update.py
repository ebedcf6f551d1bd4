"""pt_scene_update: new geometry / shading on a live handle, both trees refitted on the device (csrc/pt_scene_refit.hip).

The statement under test: both trees keep their topology and get exact new boxes, so an updated handle renders,
bit for bit, what a fresh pt_scene_create renders for the edited desc with the host's refitted pool (host.refit_bvh) — through
every entry point, on the caller's tree and on the internal one.  The work counters on the caller's tree pin the boxes
themselves: a refit that is merely conservative renders the same image but visits more nodes than the oracle does."""
import numpy as np
import pytest
from conftest import assert_bit_equal, load_scene, random_scene

from pathtracer_cuda_interactive_amd import (PT_ERR_BAD_SCENE, PT_ERR_INVALID_ARG, PT_ERR_UNSUPPORTED, PT_MAT_DIFFUSE, PT_MAT_MIRROR,
                                             PT_RENDER_NEE, PT_SHAPE_SPHERE, PT_TRAVERSAL_EXACT, PT_TRAVERSAL_PRUNED, PtError,
                                             PtLight, PtMaterial, host)
from pathtracer_cuda_interactive_amd import device as dev
from pathtracer_cuda_interactive_amd.standins import mesh_arrays

SCENES = ["cbox", "random7", "teapot"]
# (mesh that is scaled by 0.8 and moved, mesh that wobbles); cbox's mesh 0 is its light and stays where it is
EDITED_MESHES = {"cbox": (6, 7), "random7": (0, 1), "teapot": (1, 0)}
W, H = 64, 48


def wobble(P, phase, amp):
    """A smooth per-vertex displacement, large against the triangles it moves."""
    P = P.astype(np.float32)
    off = np.stack([np.sin(3.1 * P[:, 1] + phase), np.cos(2.3 * P[:, 2] + phase), np.sin(2.7 * P[:, 0] - phase)], axis=1)
    return (P + np.float32(amp) * off.astype(np.float32)).astype(np.float32)


def edit(d, name, variant):
    """variant 1 / 2: two different edits of the same kind."""
    scaled, wobbled = EDITED_MESHES[name]
    shift = np.array([(0.3, -0.5, 0.7), (-0.6, 0.4, 0.3)][variant - 1], np.float32)
    P, _, _ = mesh_arrays(d, scaled)
    Q, I, _ = mesh_arrays(d, wobbled)
    size = float((Q.max(axis=0) - Q.min(axis=0)).max())
    Q = wobble(Q, 0.4 * variant, 0.05 * size)
    meshes = {scaled: ((P * np.float32(0.8) + shift).astype(np.float32), None),
              wobbled: (Q, host.compute_normals(Q, I))}
    spheres = None
    if name == "random7":
        ids = [i for i in range(d.num_shapes) if d.shapes[i].type == PT_SHAPE_SPHERE][:2]
        spheres = {ids[0]: ((1.2 - variant, 0.6, 0.5 * variant), 0.55), ids[1]: ((-0.8, 0.2 * variant, 0.9), 0.15)}
    return dev.edited_desc(d, meshes=meshes, spheres=spheres)


_cases = {}


def case(name, oracle):
    """(d0, d1, d1r, d2, params, oracle image and counters of d1r, exact traversal), made once per scene and left unchanged."""
    if name not in _cases:
        if name == "random7":
            hs = random_scene(7)
            d0 = hs.finalize()
        else:
            hs, d0 = load_scene(name)
        d1, d2 = edit(d0, name, 1), edit(d0, name, 2)
        d1r = host.refit_bvh(d1)
        p = hs.render_params(W, H, 2 if name == "teapot" else 4, seed=11)
        p.traversal = PT_TRAVERSAL_EXACT
        want, cnt = oracle.render(d1r, p)
        _cases[name] = (d0, d1, d1r, d2, p, want, cnt)
    return _cases[name]


def scene_rays(d, name, n, seed):
    """Random rays from in and around the scene's bounding box (random7: without its ground sphere) at points inside it."""
    if name == "random7":
        lo, hi = np.full(3, -3.0), np.full(3, 3.0)
    else:
        root = d.nodes[d.root]
        lo, hi = np.array(root.bmin[:], np.float64), np.array(root.bmax[:], np.float64)
    rng = np.random.default_rng(seed)
    o = lo + (hi - lo) * (rng.random((n, 3)) * 1.6 - 0.3)
    dirs = lo + (hi - lo) * rng.random((n, 3)) - o
    dirs /= np.maximum(np.linalg.norm(dirs, axis=1, keepdims=True), 1e-20)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = o, dirs, 1e-4, np.inf
    return rays


@pytest.mark.gpu
def test_the_scenes_cover_both_refit_shapes_and_both_kinds_of_tree(oracle):
    infos = {}
    for name in SCENES:
        d0, d1 = case(name, oracle)[:2]
        S = dev.DeviceScene(d0)
        try:
            S.update(d1)
            infos[name] = {k: S.info(k) for k in ("fast_tree", "fast_tree_is_callers", "residency", "updates", "num_inner_nodes")}
        finally:
            S.close()
    print(infos)
    assert any(i["fast_tree"] == 1 and i["fast_tree_is_callers"] == 0 for i in infos.values()), infos
    assert any(i["residency"] == 2 for i in infos.values()), infos
    assert any(i["residency"] == 3 for i in infos.values()), infos
    assert all(i["updates"] == 1 for i in infos.values())


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_renders_after_an_update_match_a_fresh_create(oracle, name):
    d0, d1, d1r, _, p, want, _ = case(name, oracle)
    rays = scene_rays(d1r, name, 20000, 5)
    S, F = dev.DeviceScene(d0), dev.DeviceScene(d1r)
    try:
        before = S.render(p)
        S.update(d1)
        assert not np.array_equal(before, want), "the edit does not show in the image"
        for fast in (1, 0):
            S.set_option("fast_tree", fast)
            F.set_option("fast_tree", fast)
            for trav in (PT_TRAVERSAL_EXACT, PT_TRAVERSAL_PRUNED):
                what = f"{name} fast_tree={fast} traversal={trav}"
                img = S.render(p, traversal=trav)
                assert_bit_equal(img, F.render(p, traversal=trav), what + " vs fresh create")
                if trav == PT_TRAVERSAL_EXACT:
                    assert_bit_equal(img, want, what + " vs oracle")
                tuv, prim = S.intersect(rays, trav)
                tuv_f, prim_f = F.intersect(rays, trav)
                assert np.array_equal(prim, prim_f), what
                assert_bit_equal(tuv, tuv_f, what + " intersect")
            a, b = S.render_aov(p), F.render_aov(p)
            assert np.array_equal(a["prim"], b["prim"])
            for k in ("albedo", "normal", "depth"):
                assert_bit_equal(a[k], b[k], f"{name} fast_tree={fast} aov {k}")
        assert (prim >= 0).sum() > 2000
        if name == "cbox":
            q = p.copy()
            q.flags = PT_RENDER_NEE
            S.set_option("fast_tree", 1)
            F.set_option("fast_tree", 1)
            assert_bit_equal(S.render(q), F.render(q), "next-event estimation")
    finally:
        S.close()
        F.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_work_counters_after_an_update_equal_the_oracles_on_the_refitted_tree(oracle, name):
    d0, d1, d1r, _, p, want, cnt = case(name, oracle)
    S = dev.DeviceScene(d0)
    try:
        S.set_option("stats", 1)
        on = S.info("fast_tree_on")
        assert on == S.info("fast_tree")
        S.update(d1)
        # the handle goes on rendering on the tree it rendered on before
        assert (S.info("fast_tree"), S.info("fast_tree_on")) == (on, on)
        assert_bit_equal(S.render(p), want, "fast tree")
        assert S.info("fast_tree_on") == on
        c = S.counters()
        assert (c.paths, c.segments) == (cnt.paths, cnt.segments)
        fast_visits = c.node_visits
        S.set_option("fast_tree", 0)
        assert S.info("fast_tree_on") == 0
        assert_bit_equal(S.render(p), want, "caller's tree")
        c = S.counters()
        assert (c.paths, c.segments) == (cnt.paths, cnt.segments)
        if on and not S.info("fast_tree_is_callers"):
            assert fast_visits != c.node_visits, "another topology visits another number of nodes"
        # exact boxes, not merely conservative ones: the same nodes visited, the same leaves tested
        assert c.node_visits == cnt.inner_pops, (c.node_visits, cnt.inner_pops)
        assert c.leaf_tests == cnt.leaf_tri + cnt.leaf_sphere, (c.leaf_tests, cnt.leaf_tri + cnt.leaf_sphere)
    finally:
        S.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cbox", "teapot"])
def test_repeated_updates_return_to_the_first_image(oracle, name):
    d0, d1, d1r, d2, p, want, _ = case(name, oracle)
    S, F = dev.DeviceScene(d0), dev.DeviceScene(d0)
    try:
        S.set_option("stats", 1)
        F.set_option("stats", 1)
        first = F.render(p)
        assert S.info("updates") == 0 and S.info("update_us3") == 0
        S.update(d1)
        assert S.info("updates") == 1 and S.info("update_us3") > 0 and S.info("update_us0") >= S.info("update_us3")
        assert_bit_equal(S.render(p), want, "d1")
        S.update(d2)
        assert S.info("updates") == 2 and S.info("update_us3") == 0
        mid = S.render(p)
        assert not np.array_equal(mid, want) and not np.array_equal(mid, first)
        S.update(d0)
        assert S.info("updates") == 3 and S.info("update_us3") == 0
        for fast in (1, 0):
            S.set_option("fast_tree", fast)
            F.set_option("fast_tree", fast)
            assert S.info("fast_tree_on") == F.info("fast_tree_on") == (fast and F.info("fast_tree"))
            assert_bit_equal(S.render(p), F.render(p), f"back at d0, fast_tree={fast}")
            # the same topology with exact boxes, on the internal tree as on the caller's: the same nodes and leaves visited
            cs, cf = S.counters(), F.counters()
            assert (cs.node_visits, cs.leaf_tests) == (cf.node_visits, cf.leaf_tests), fast
    finally:
        S.close()
        F.close()


@pytest.mark.gpu
def test_shading_only_update_changes_the_kernel_specialisation(oracle):
    d0, _, _, _, p, _, _ = case("cbox", oracle)
    assert all(d0.materials[m].type == PT_MAT_DIFFUSE for m in range(d0.num_materials))
    mats = [PtMaterial.from_buffer_copy(d0.materials[m]) for m in range(d0.num_materials)]
    mats[0].type = PT_MAT_MIRROR                          # the two boxes
    lights = [PtLight.from_buffer_copy(d0.lights[k]) for k in range(d0.num_lights)]
    for lt in lights:
        lt.radiance[:] = [9.0, 3.0, 1.0]
    ds = dev.edited_desc(d0, materials=mats, lights=lights, background=(0.1, 0.7, 0.2))
    want, cnt = oracle.render(ds, p)
    S, F = dev.DeviceScene(d0), dev.DeviceScene(ds)
    try:
        S.set_option("stats", 1)
        before = S.render(p)
        variant = S.info("trace_variant")
        S.update(ds, geometry=False, shading=True)
        img = S.render(p)
        assert S.info("trace_variant") != variant and S.info("update_us3") == 0
        assert not np.array_equal(img, before)
        assert_bit_equal(img, F.render(p), "vs fresh create")
        assert_bit_equal(img, want, "vs oracle")
        c = S.counters()
        assert (c.paths, c.segments) == (cnt.paths, cnt.segments)
    finally:
        S.close()
        F.close()


@pytest.mark.gpu
def test_update_waits_for_the_frames_in_flight(oracle):
    import torch
    d0, d1, _, _, p, want, _ = case("teapot", oracle)
    S = dev.DeviceScene(d0)
    try:
        want0 = S.render(p)
        stream = torch.cuda.Stream()
        outs = [torch.zeros(H, W, 3, dtype=torch.float32, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        for o in outs:
            S.render_into(p, o.data_ptr(), stream=stream.cuda_stream)
        S.update(d1)                                      # no host sync between the enqueues and this call
        later = S.render(p)
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            assert_bit_equal(o.cpu().numpy(), want0, f"frame {k} enqueued before the update")
        assert_bit_equal(later, want, "render after the update")
    finally:
        S.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cbox", "teapot"])
def test_a_failed_update_leaves_the_handle_as_it_was(oracle, name):
    d0, d1, _, _, p, want, _ = case(name, oracle)
    scaled, wobbled = EDITED_MESHES[name]
    S = dev.DeviceScene(d0)
    try:
        S.update(d1)
        assert_bit_equal(S.render(p), want, "before")

        def refused(desc, status, word):
            with pytest.raises(PtError) as e:
                S.update(desc)
            assert e.value.status == status and word in str(e.value), str(e.value)
            assert S.info("updates") == 1
            for fast in (1, 0):
                S.set_option("fast_tree", fast)
                assert_bit_equal(S.render(p), want, f"after the refused update, fast_tree={fast}")

        short = dev.edited_desc(d0)
        short.num_shapes = d0.num_shapes - 1
        refused(short, PT_ERR_INVALID_ARG, "num_shapes")
        # the edits below start from d2-like geometry, so that a half-applied update would show
        P, I, _ = mesh_arrays(d0, wobbled)
        Q = wobble(P, 2.0, 0.1 * float((P.max(axis=0) - P.min(axis=0)).max()))
        bad_index = dev.edited_desc(d0, meshes={wobbled: (Q, None)})
        J = I.copy()
        J[len(J) // 2, 1] = len(P)                        # one past the last vertex
        bad_index.meshes[wobbled].indices = J.ctypes.data_as(type(bad_index.meshes[wobbled].indices))
        bad_index._keep.append(J)
        refused(bad_index, PT_ERR_BAD_SCENE, "vertex index out of range")
        # `a < b ? a : b` keeps a NaN in its second argument only, so min(min(p0, p1), p2) is finite unless the NaN sits in p2:
        # a NaN coordinate is refused wherever it sits, by the box (last corner) or by the record itself (the other two)
        v = I[len(I) // 3, 0]
        Q[v, 1] = np.nan
        for corner in (0, 1, 2):
            J = I.copy()
            for f in np.nonzero((I == v).any(axis=1))[0]:
                J[f] = np.roll(I[f], corner - int(np.argmax(I[f] == v)))
            assert (J[(J == v).any(axis=1)][:, corner] == v).all()
            nan_desc = dev.edited_desc(d0, meshes={wobbled: (Q, None)})
            nan_desc.meshes[wobbled].indices = J.ctypes.data_as(type(nan_desc.meshes[wobbled].indices))
            nan_desc._keep.append(J)
            refused(nan_desc, PT_ERR_UNSUPPORTED, "not finite")
        # and the handle still takes a good update
        S.update(d0)
        assert S.info("updates") == 2
    finally:
        S.close()
