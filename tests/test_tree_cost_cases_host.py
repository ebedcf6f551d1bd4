"""The inputs of test_tree_cost_states.py, checked without a GPU (scene_rebuild_cases.py, second half): the identities those
tests assert of the device hold of the host twins of the same scenes, so a failure there is the device's."""
import numpy as np
import pytest
import scene_rebuild_cases as rc

from pathtracer_cuda_interactive_amd import host
from pathtracer_cuda_interactive_amd import device as dev


def boxes(d):
    nodes = rc.pool(d)
    return nodes["bmin"], nodes["bmax"]


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_sizes_sit_on_both_sides_of_every_boundary_of_the_cost_kernels():
    records = {n - 1 for n in rc.EQUAL_SIZES}
    assert {1, 2, 3, 4, 5} <= records, "one thread's four records and its tail"
    for edge in (256, 1024, 2048):
        assert {edge, edge + 1} <= records, edge
    assert {255, 1023} <= records
    assert {4095, 4096, 4097} <= set(rc.EQUAL_SIZES), "host against device scene preparation"
    assert {1, 2} <= set(rc.EQUAL_SIZES)
    assert [rc.scaled_case(n)["d0"].num_shapes for n in ("random1025", "random1030")] == [1025, 1030]


@pytest.mark.parametrize("n", rc.EQUAL_SIZES)
def test_equal_spheres_cost_six_per_inner_node(host_lib, n):
    _, d = rc.equal_spheres(n)
    assert d.num_shapes == n and d.num_nodes == 2 * n - 1
    lo, hi = boxes(d)
    assert (lo == np.float32(-0.5)).all() and (hi == np.float32(0.5)).all()
    assert host.tree_cost(d) == 6.0 * max(n - 2, 0)
    r = host.refit_bvh(d)                                     # what an update with the same desc refits the handle to
    assert same_bits(boxes(r)[0], lo) and same_bits(boxes(r)[1], hi)
    assert host.tree_cost(r) == 6.0 * max(n - 2, 0)
    if n >= 16:
        s, _ = dev.build_bvh_sweep(d)                         # the internal tree, where one is kept
        assert host.tree_cost(s) == 6.0 * (n - 2)


@pytest.mark.parametrize("name", rc.SCALED)
def test_scaling_by_a_power_of_two_scales_every_box_exactly(host_lib, name):
    c = rc.scaled_case(name)
    d0, ids = c["d0"], c["ids"]
    lo0, hi0 = boxes(d0)
    one = host.refit_bvh(dev.transform_desc_host(d0, ids, rc.scaling(1.0)))
    lo1, hi1 = boxes(one)
    leaf = rc.pool(d0)["prim"] >= 0
    # the reference of a handle is the cost of the boxes as built: permille 4000 needs them to be the boxes of a refit
    assert same_bits(lo1, lo0) and same_bits(hi1, hi0), "the boxes as built are the boxes a refit makes"
    for s in (2.0, 0.5):
        sc = host.refit_bvh(dev.transform_desc_host(d0, ids, rc.scaling(s)))
        lo, hi = boxes(sc)
        assert same_bits(lo[leaf], np.float32(s) * lo1[leaf]) and same_bits(hi[leaf], np.float32(s) * hi1[leaf]), f"leaf boxes x {s}"
        assert same_bits(lo, np.float32(s) * lo1) and same_bits(hi, np.float32(s) * hi1), f"every box x {s}"
        assert host.tree_cost(sc) == s * s * host.tree_cost(one), "and so the cost, in a fixed order, by s^2 exactly"
    assert np.isfinite(lo1).all() and (np.abs(lo1[lo1 != 0]) > 2.0 ** -100).all(), "nowhere near overflow or underflow"


@pytest.mark.parametrize("name", rc.ROUTES)
def test_route_cases_move_every_tree(host_lib, name):
    c = rc.route_case(name)
    d0 = c["d0"]
    assert c["ids"].size == d0.num_shapes and c["M"].shape == (c["G"], 3, 4)
    assert d0.num_shapes >= 16, "large enough for an internal tree"
    costs = [host.tree_cost(host.refit_bvh(d)) for d in (d0, c["d1"], c["d2"])]
    assert len(set(costs)) == 3, "three different costs: a reference taken from the wrong boxes shows"
    exact, m = rc.host_cost0(c["d1"])
    assert m == d0.num_shapes - 2 and abs(costs[1] - exact) <= rc.sum_bound(m) * exact
    if name == "scene4":
        assert d0.num_shapes == 30 and d0.num_meshes == 0
    if name == "mixed":
        sh = dev.shape_table(d0)
        assert 0 < int((sh["type"] == sh["type"][0]).sum()) < d0.num_shapes, "triangles and spheres"


@pytest.mark.parametrize("name", rc.NO_TREE)
def test_no_tree_cases(host_lib, name):
    c = rc.no_tree_case(name)
    d0 = c["d0"]
    if name == "scene1":
        assert d0.num_shapes < 16
    else:
        nodes = rc.pool(d0)
        out = 0
        for k in np.flatnonzero(nodes["prim"] < 0):
            if int(k) == int(d0.root):
                continue
            for ch in (nodes["left"][k], nodes["right"][k]):
                out += int((nodes["bmin"][ch] < nodes["bmin"][k]).any() or (nodes["bmax"][ch] > nodes["bmax"][k]).any())
        assert out > 0, "some child sticks out of its parent"
    assert host.tree_cost(host.refit_bvh(c["d1"])) != host.tree_cost(host.refit_bvh(d0))


def test_the_refused_inputs_are_what_they_say(host_lib):
    c = rc.route_case("grid3")
    bad = rc.with_a_nan_vertex(c["d1"])
    from pathtracer_cuda_interactive_amd import standins
    P, I, _ = standins.mesh_arrays(bad, 0)
    assert np.isnan(P).sum() == 1 and np.isin(np.argwhere(np.isnan(P))[0, 0], I), "one NaN, in a vertex some face uses"
    S = rc.singular(c["G"])
    assert np.linalg.det(S[1, :, :3].astype(np.float64)) == 0.0 and np.linalg.det(S[0, :, :3].astype(np.float64)) == 1.0
    assert tuple(rc.reshaded(c["d0"]).background) != tuple(c["d0"].background)


def test_the_sweep_tree_of_the_doubled_grid_is_the_doubled_sweep_tree(host_lib):
    c = rc.same_tree_case()
    fresh, _ = dev.build_bvh_sweep(c["d1r"])
    a, b = rc.pool(c["d1r"]), rc.pool(fresh)
    assert fresh.root == c["d1r"].root and all(np.array_equal(a[k], b[k]) for k in ("left", "right", "prim")), "the candidate is the tree held"
    assert same_bits(a["bmin"], b["bmin"]) and same_bits(a["bmax"], b["bmax"])
    assert host.tree_cost(c["d1r"]) == 4.0 * host.tree_cost(c["d0"])


def test_the_cornell_box_drifts_past_the_lowest_threshold(host_lib):
    """The policy test at the lowest threshold runs cbox under M1 with "rebuild_at_permille" 1001: the internal tree's cost must
    have risen by more than rounding can hide (the device adds the same terms in another order)."""
    c = rc.cbox_case()
    rest1, _ = dev.build_bvh_sweep(c["d0"])
    now1 = host.refit_bvh(dev.transform_desc_host(rest1, c["ids"], c["M1"]))
    permille = 1000.0 * host.tree_cost(now1) / host.tree_cost(rest1)
    print("cbox under M1: host permille of the internal tree", permille)
    assert permille >= 1002.0
