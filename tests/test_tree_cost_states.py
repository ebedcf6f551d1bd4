"""Tree-cost telemetry and the rebuild policy in every state a handle can be in (include/pt_api.h, pt_scene_rebuild: "When to call
it"; csrc/pt_tree_cost.hip and adopt_staged, collect_costs, rebuild_scene, rebuild_by_policy of pt_scene_life.hip).

The order in which the device adds a tree's records is not visible from outside, so the cost kernels are pinned by identities
that hold in ANY order of summation and fail on a wrong set of terms: equal boxes of area 6 (the cost is an integer, exact
whatever the order) and scaling by a power of two (every term and every partial sum scales exactly).  Everything else compares a
handle with a twin that reached the same state by another route, bit for bit.  Inputs: scene_rebuild_cases.py, checked without a
GPU by test_tree_cost_cases_host.py."""
import math

import numpy as np
import pytest
import scene_rebuild_cases as rc
from conftest import assert_bit_equal

from pathtracer_cuda_interactive_amd import PT_ERR_INVALID_ARG, PT_ERR_UNSUPPORTED, PT_TRAVERSAL_EXACT, PtError, host
from pathtracer_cuda_interactive_amd import device as dev

KEYS, UNMEASURED = rc.COST_KEYS, rc.UNMEASURED


class closing:
    def __init__(self, *scenes):
        self.scenes = scenes

    def __enter__(self):
        return self.scenes

    def __exit__(self, *exc):
        for s in self.scenes:
            s.close()


def work(S, p):
    """(node_visits, leaf_tests, redo_segments) of an exact STATS render on the internal tree."""
    S.set_option("stats", 1)
    S.set_option("fast_tree", 1)
    S.render(p, traversal=PT_TRAVERSAL_EXACT)
    c = S.counters()
    w = (c.node_visits, c.leaf_tests, S.info("redo_segments"))
    S.set_option("stats", 0)
    return w


def keys(S):
    return [S.info(k) for k in KEYS]


def counts(S):
    return S.info("rebuilds"), S.info("rebuilds_auto")


def handle(c, d=None, **options):
    """A handle of c's rest scene (or of `d`) with c's groups set and the options given."""
    S = dev.DeviceScene(c["d0"] if d is None else d)
    S.set_groups(c["ids"], c["G"])
    for k, v in options.items():
        S.set_option(k, v)
    return S


def refused(call, status):
    with pytest.raises(PtError) as e:
        call()
    assert e.value.status == status, str(e.value)


# ---- A: the cost kernels ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", rc.EQUAL_SIZES)
def test_equal_boxes_cost_exactly_six_per_inner_node(n):
    _, d = rc.equal_spheres(n)
    want = rc.bits64(6.0 * (n - 2)) if n > 2 else 0
    with closing(dev.DeviceScene(d)) as (A,):
        if n > 1:
            assert A.info("num_inner_nodes") == n - 1, "one record per inner node"
        A.set_option("tree_cost", 1)
        assert keys(A) == UNMEASURED
        A.update(d, geometry=True)
        got, fast = keys(A), A.info("fast_tree")
        print(f"n={n}: fast_tree {fast}, keys {got}, cost0 {rc.f64(got[0])!r}, cost1 {rc.f64(got[1])!r}, want {6.0 * max(n - 2, 0)!r}")
        assert got[0] == want, f"tree 0 of {n} equal boxes: {rc.f64(got[0])!r}, not {6.0 * max(n - 2, 0)!r}"
        assert got[1] == (want if fast else 0), f"tree 1 of {n} equal boxes with fast_tree = {fast}: {rc.f64(got[1])!r}"
        assert got[2:] == [1000, 1000]
        A.update(d, geometry=True)
        assert keys(A) == got, "and again"


@pytest.mark.gpu
@pytest.mark.parametrize("name", rc.SCALED)
def test_scaling_by_two_is_exact_and_the_absolute_value_is_the_hosts(name):
    c = rc.scaled_case(name)
    d0 = c["d0"]
    with closing(handle(c, tree_cost=1), handle(c, tree_cost=1)) as (A, B):
        A.transform(rc.scaling(1.0))
        a = keys(A)
        assert A.info("fast_tree") == 1 and a[0] != 0 and a[1] != 0
        assert a[2:] == [1000, 1000], "the boxes as built are the boxes a refit makes"
        for s, permille in ((2.0, 4000), (0.5, 250), (1.0, 1000)):
            B.transform(rc.scaling(s))
            b = keys(B)
            for t in (0, 1):
                print(f"{name} x {s} tree {t}: {rc.f64(b[t])!r} against {s * s} * {rc.f64(a[t])!r}, permille {b[2 + t]}")
                assert b[t] == rc.bits64(s * s * rc.f64(a[t])), f"tree {t} x {s}: {rc.f64(b[t])!r}, not {s * s} * {rc.f64(a[t])!r}"
                assert b[2 + t] == permille, (t, s, b)
        # A3: the absolute value, within the bound of any order of summation
        exact, m = rc.host_cost0(d0)
        got = rc.f64(a[0])
        print(f"{name} tree 0: device {got!r}, fsum {exact!r}, {m} terms, host in pool order {host.tree_cost(host.refit_bvh(d0))!r}")
        assert m == d0.num_shapes - 2 and abs(got - exact) <= rc.sum_bound(m) * exact


# ---- B: every route into a refit measures the same thing -------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", rc.ROUTES)
def test_transform_and_update_measure_the_same(name):
    c = rc.route_case(name)
    with closing(handle(c, tree_cost=1), handle(c, tree_cost=1), handle(c, tree_cost=1)) as (T, U, V):
        T.transform(c["M"])
        U.update(c["d1"])
        t, u = keys(T), keys(U)
        print(f"{name}: transform {t}, update {u}, fast_tree {T.info('fast_tree')}")
        assert t == u
        assert T.info("fast_tree") == 1 and t[1] != 0 and t[2] != 1000 and t[3] != 1000
        exact, m = rc.host_cost0(c["d1"])
        assert abs(rc.f64(t[0]) - exact) <= rc.sum_bound(m) * exact, (rc.f64(t[0]), exact)
        ref = math.fsum(rc.inner_terms(c["d0"]))
        assert abs(t[2] - 1000.0 * exact / ref) <= 0.5 + 1e-6, "the reference is the cost of the boxes as built"
        # a second refit keeps the reference, by either route
        T.transform(c["M2"])
        U.update(c["d2"])
        assert keys(T) == keys(U)
        exact2, _ = rc.host_cost0(c["d2"])
        assert abs(rc.f64(T.info("tree_cost0_bits")) - exact2) <= rc.sum_bound(m) * exact2
        # a shading-only update measures nothing and takes no reference ...
        V.update(rc.reshaded(c["d0"]), geometry=False, shading=True)
        assert keys(V) == UNMEASURED
        V.update(c["d1"])
        assert keys(V) == u, "... the next geometry update takes it from the boxes as built"
        V.update(rc.reshaded(c["d1"]), geometry=False, shading=True)
        assert keys(V) == u, "and one after a measurement changes no key"
        V.update(rc.reshaded(c["d2"]), geometry=True, shading=True)
        assert keys(V) == keys(U)


@pytest.mark.gpu
@pytest.mark.parametrize("name", rc.NO_TREE)
def test_handles_without_an_internal_tree(name):
    c = rc.no_tree_case(name)
    with closing(handle(c, tree_cost=1), handle(c, rebuild_at_permille=1001)) as (T, U):
        assert T.info("fast_tree") == 0
        T.transform(c["M"])
        U.update(c["d1"])
        t, u = keys(T), keys(U)
        print(f"{name}: transform {t}, update under a policy {u}")
        assert t == u
        assert t[0] != 0 and t[1] == 0 and t[3] == 1000
        exact, m = rc.host_cost0(c["d1"])
        assert abs(rc.f64(t[0]) - exact) <= rc.sum_bound(m) * exact
        assert counts(U) == (0, 0), "a policy with no internal tree to rebuild does nothing"
        assert U.info("updates") == 1
        U.transform(c["M"])
        assert counts(U) == (0, 0) and U.info("tree_cost1_permille") == 1000


@pytest.mark.gpu
def test_refused_calls_leave_the_telemetry_as_it_was():
    c = rc.route_case("grid3")
    nan1, sing = rc.with_a_nan_vertex(c["d1"]), rc.singular(c["G"])
    with closing(handle(c, tree_cost=1), handle(c, tree_cost=1), handle(c), handle(c)) as (A, W, R, RW):
        def both_refused(S):
            before = keys(S), counts(S), S.info("rebuild_adopted")
            refused(lambda: S.update(nan1), PT_ERR_UNSUPPORTED)
            assert (keys(S), counts(S), S.info("rebuild_adopted")) == before, "after the refused update"
            refused(lambda: S.transform(sing), PT_ERR_INVALID_ARG)
            assert (keys(S), counts(S), S.info("rebuild_adopted")) == before, "after the refused transform"
        # before any reference exists: the refused update had enqueued one
        both_refused(A)
        assert keys(A) == UNMEASURED
        A.transform(c["M"])
        W.transform(c["M"])
        assert keys(A) == keys(W), "the keys of a handle that never saw the refused calls"
        # after a measured refit
        both_refused(A)
        A.transform(c["M2"])
        W.transform(c["M2"])
        assert keys(A) == keys(W)
        # what a refused update enqueued is not collected by a later call: the tree it measured is replaced in between
        for S in (R, RW):
            S.transform(c["M"])
            S.set_option("tree_cost", 1)
        refused(lambda: R.update(nan1), PT_ERR_UNSUPPORTED)
        assert R.rebuild() is True and RW.rebuild() is True
        R.update(rc.reshaded(c["d0"]), geometry=False, shading=True)
        print("after a refused update, a rebuild and a shading-only update", keys(R), "twin", keys(RW))
        assert keys(R) == keys(RW) and keys(R)[2:] == [1000, 1000]
        R.transform(c["M2"])
        RW.transform(c["M2"])
        assert keys(R) == keys(RW), "tree 1's reference is the rebuilt tree's"


# ---- C: the option's life cycle --------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_switching_the_telemetry_off_forgets_the_boxes_it_measured():
    c = rc.route_case("grid3")
    M1, M2 = c["M"], c["M2"]
    with closing(handle(c, tree_cost=1), handle(c)) as (A, W):
        A.transform(M1)
        assert keys(A) != UNMEASURED
        A.set_option("tree_cost", 0)
        assert keys(A) == UNMEASURED
        A.transform(M2)                                  # unmeasured
        A.set_option("tree_cost", 1)
        assert keys(A) == UNMEASURED, "the costs of boxes that no longer exist"
        A.transform(M1)
        W.transform(M2)
        W.set_option("tree_cost", 1)
        W.transform(M1)
        print("A", keys(A), "twin", keys(W))
        assert keys(A) == keys(W), "the reference is the cost of the M2 boxes"
        assert keys(A)[2] != 1000 and keys(A)[3] != 1000


@pytest.mark.gpu
def test_switching_the_telemetry_off_forgets_the_tree_it_measured():
    c = rc.route_case("grid3")
    M1, M2 = c["M"], c["M2"]
    with closing(handle(c, tree_cost=1), handle(c)) as (A, W):
        A.transform(M1)
        A.set_option("tree_cost", 0)
        assert A.rebuild() is True
        A.set_option("tree_cost", 1)
        assert keys(A) == UNMEASURED
        A.transform(M2)
        W.transform(M1)
        assert W.rebuild() is True
        W.set_option("tree_cost", 1)
        W.transform(M2)
        print("A", keys(A), "twin", keys(W))
        assert keys(A) == keys(W), "nothing of the replaced tree remains"
        # a rebuild that is not adopted, with the telemetry off, writes no reference either: the tree is fresh for the M2 boxes
        for S in (A, W):
            S.set_option("tree_cost", 0)
        adopted = A.rebuild(), W.rebuild()
        assert adopted[0] == adopted[1]
        for S in (A, W):
            S.set_option("tree_cost", 1)
            assert keys(S) == UNMEASURED
            S.transform(M1)
        assert keys(A) == keys(W)


@pytest.mark.gpu
def test_either_option_switches_the_telemetry_on():
    c = rc.route_case("grid3")
    with closing(handle(c), handle(c, tree_cost=1)) as (A, W):
        W.transform(c["M"])
        want = keys(W)
        A.set_option("rebuild_at_permille", 1_000_000)       # never reached
        A.transform(c["M"])
        assert keys(A) == want and counts(A) == (0, 0), "the policy alone implies the telemetry"
        A.set_option("rebuild_at_permille", 0)
        assert keys(A) == UNMEASURED, "both options 0: off"
        A.set_option("tree_cost", 1)
        A.set_option("rebuild_at_permille", 1_000_000)
        A.transform(c["M"])
        measured = keys(A)
        assert measured[:2] == want[:2] and measured[2:] == [1000, 1000], "the reference: the M boxes, which the handle held"
        A.set_option("rebuild_at_permille", 0)
        assert keys(A) == measured, "tree_cost 1 keeps it on"
        A.set_option("tree_cost", 0)
        A.set_option("rebuild_at_permille", 1_000_000)
        assert keys(A) == UNMEASURED, "off and on again"


@pytest.mark.gpu
def test_option_values_that_are_refused_change_nothing():
    c = rc.route_case("grid3")
    with closing(handle(c, tree_cost=1), handle(c, rebuild_at_permille=1_000_000), handle(c)) as (A, B, Z):
        A.transform(c["M"])
        B.transform(c["M"])
        want = keys(A)
        assert keys(B) == want
        for S in (A, B, Z):
            before = keys(S)
            for key, value in (("tree_cost", 2), ("tree_cost", -1), ("rebuild_at_permille", 1), ("rebuild_at_permille", 1000), ("rebuild_at_permille", -5)):
                refused(lambda: S.set_option(key, value), PT_ERR_INVALID_ARG)
                assert keys(S) == before, (key, value)
        # the options stand as they were: A and B still measure, Z still does not, and no policy has appeared
        for S in (A, B, Z):
            S.transform(c["M2"])
        assert keys(A) == keys(B) != want and keys(Z) == UNMEASURED
        assert [counts(S) for S in (A, B, Z)] == [(0, 0)] * 3


# ---- D: the policy -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_the_threshold_is_at_or_above():
    c = rc.scaled_case("grid7")
    with closing(handle(c, rebuild_at_permille=4000), handle(c, rebuild_at_permille=4001)) as (A, B):
        for S in (A, B):
            S.transform(rc.scaling(2.0))
        print("at 4000:", counts(A), keys(A), "at 4001:", counts(B), keys(B))
        assert counts(B) == (0, 0) and B.info("tree_cost1_permille") == 4000
        assert counts(A) == (1, 1) and A.info("tree_cost1_permille") == 1000
        assert A.info("tree_cost0_permille") == 4000 and A.info("tree_cost0_bits") == B.info("tree_cost0_bits")
        for S in (A, B):
            S.transform(rc.scaling(2.0))
        assert counts(A) == (1, 1) and counts(B) == (0, 0), "the same transform again: nothing drifted"


@pytest.mark.gpu
def test_the_policy_at_the_lowest_threshold_on_the_cornell_box():
    """cbox under M1 with "rebuild_at_permille" 1001, the lowest there is.  Measured on an MI355X: tree_cost1_permille 1007 without a
    policy (the host twin says 1006.56), so the policy fires; the candidate's probe ratio is 661 and it is ADOPTED — as a fresh
    create of the moved scene keeps its sweep tree — so this is not a candidate that loses (the next test has one)."""
    c = rc.cbox_case()
    p = c["p"]
    with closing(dev.DeviceScene(c["d0"]), dev.DeviceScene(c["d1r"]), dev.DeviceScene(c["d0"])) as (A, F, W):
        G = c["M1"].shape[0]
        for S in (A, W):
            S.set_groups(c["ids"], G)
        W.set_option("tree_cost", 1)
        W.transform(c["M1"])
        drift = W.info("tree_cost1_permille")
        print("cbox under M1: tree_cost1_permille without a policy", drift, "keys", keys(W))
        assert drift >= 1001
        A.set_option("rebuild_at_permille", 1001)
        A.transform(c["M1"])
        print("with the policy:", counts(A), A.info("rebuild_adopted"), A.info("rebuild_cost_permille"), keys(A))
        wins = int(F.info("fast_tree") and not F.info("fast_tree_is_callers"))       # pt_scene_create's rule on the same boxes
        assert (*counts(A), A.info("rebuild_adopted")) == (1, 1, wins)
        assert A.info("rebuild_cost_permille") == F.info("fast_tree_cost_permille")
        assert A.info("tree_cost1_permille") == 1000 and A.info("tree_cost0_bits") == W.info("tree_cost0_bits")
        A.transform(c["M1"])
        assert counts(A) == (1, 1), "a repeat does not rebuild"
        assert_bit_equal(A.render(p), F.render(p), "cbox after a policy's rebuild")


@pytest.mark.gpu
def test_a_policy_rebuild_whose_candidate_loses():
    """grid3 on the library's own sweep tree, doubled (rc.same_tree_case): the cost is at exactly 4000 permille, the candidate is the
    tree the handle holds and cannot win."""
    c = rc.same_tree_case()
    p = c["p"]
    with closing(handle(c, rebuild_at_permille=1001), dev.DeviceScene(c["d1r"]), handle(c, tree_cost=1)) as (A, F, W):
        assert A.info("fast_tree_is_callers") == 1
        W.transform(c["M"])
        w = keys(W)
        assert w[2:] == [4000, 4000]
        A.transform(c["M"])
        print("with the policy:", counts(A), A.info("rebuild_adopted"), A.info("rebuild_cost_permille"), keys(A))
        assert (*counts(A), A.info("rebuild_adopted")) == (1, 1, 0)
        assert keys(A) == [w[0], w[1], 4000, 1000], "the current cost became tree 1's reference; nothing else changed"
        assert A.info("fast_tree_is_callers") == 1
        A.transform(c["M"])
        assert counts(A) == (1, 1) and keys(A) == [w[0], w[1], 4000, 1000], "a repeat does not rebuild"
        assert_bit_equal(A.render(p), F.render(p), "a candidate that lost")
        A.transform(rc.scaling(4.0))
        assert counts(A) == (2, 2) and A.info("rebuild_adopted") == 0, "and the next drift is measured from there: 4000 again"


@pytest.mark.gpu
def test_the_policy_through_an_update():
    c = rc.grid_case(7)
    p = c["p"]
    G = c["M1"].shape[0]
    d1 = dev.transform_desc_host(c["d0"], c["ids"], c["M1"])
    root = c["d0"].nodes[c["d0"].root]
    size = float(max(root.bmax[k] - root.bmin[k] for k in range(3)))
    prev_cam = dev.translated_params(p, np.array([0.02, -0.01, 0.03]) * size)
    with closing(dev.DeviceScene(c["d0"]), dev.DeviceScene(c["d1r"]), dev.DeviceScene(c["d0"]), dev.DeviceScene(c["d0"])) as (A, F, I, B):
        A.set_option("rebuild_at_permille", 1500)
        A.update(d1)
        assert (*counts(A), A.info("rebuild_adopted")) == (1, 1, 1)
        assert A.info("tree_cost1_permille") == 1000
        assert 0 < A.info("rebuild_us0") <= A.info("update_us0"), "the rebuild ran inside the update"
        assert work(A, p) == work(F, p)
        assert_bit_equal(A.render(p), F.render(p), "policy through pt_scene_update")
        B.update(d1)
        a = A.render_guides(p, prev_cam, previous_geometry=True)
        b = B.render_guides(p, prev_cam, previous_geometry=True)
        assert np.array_equal(a["prim"], b["prim"])
        for k in ("albedo", "normal", "depth", "motion", "prev_depth"):
            assert_bit_equal(a[k], b[k], f"previous_geometry across an automatic rebuild: {k}")
        A.update(d1)
        assert counts(A) == (1, 1), "nothing drifted since the rebuild"
        I.set_option("rebuild_at_permille", 1500)
        I.update(c["d0"])
        assert (*counts(I), I.info("tree_cost1_permille")) == (0, 0, 1000)
        I.set_groups(c["ids"], G)
        I.transform(c["M1"])
        assert counts(I) == (1, 1), "and by a transform after an update on the same handle"
