"""Every trace-kernel instantiation compiled into libpt_hip.so, launched once and checked against the CPU oracle.

The compiled set is read from the library's gfx950 code object (tests/trace_variants.py).  A planner maps each instantiation
to the scene, options, traversal and entry point that make choose_trace / find_trace of csrc/pt_api.hip launch it; info
"trace_variant" confirms that they did.  The CPU tests fail when an instantiation exists that the planner cannot reach, or
when the compiled set is not the one listed in tests/golden/trace_kernels.txt."""
import ctypes as C
import os
from collections import Counter

import adaptive_reference
import numpy as np
import pytest
from conftest import assert_bit_equal, assert_work_counters, random_scene
from trace_variants import Variant, compiled_trace_variants, parse_kernel_name

from pathtracer_cuda_interactive_amd import (PT_BVH_SORT_REFERENCE, PT_MAT_DIFFUSE, PT_MAT_MIRROR, PT_MAT_PHONG, PT_MAT_PLASTIC,
                                             PT_RENDER_NEE, PT_TRAVERSAL_EXACT, PT_TRAVERSAL_PRUNED, HostScene, _build)

W, H, SPP = 24, 16, 3
A_SPP, A_BATCH, A_MAX, A_ERROR, A_MIN_LUM = 2, 2, 4, 0.05, 0.01     # adaptive calls: checkpoints 2 and 4, two rounds
TINY, BIG = 32, 320        # primitives: 8 octant tables of 31 inner nodes fit 24 KB; 320 x 160 B is over the 36 KB LDS limit

OPTION_DEFAULTS = {"kernel": 2, "force_global": 0, "octants": 1, "top_cache": 1, "fast_tree": 1, "specialize": 1, "stats": 0,
                   "v2_thresh": 0, "v2_inner": 0, "v2_minw": 0}
# the automatic (v2_thresh, v2_inner) of kernel 2 by residency and tree, and of NEE kernels (choose_trace / v2_schedule)
AUTO_SCHEDULE = {0: {"internal": (32, 1231), "callers": (32, 4)}, 3: {"internal": (32, 1231), "callers": (32, 4)},
                 1: {"internal": (40, 162), "callers": (40, 162)}, 2: {"internal": (40, 162), "callers": (40, 162)}}
NEE_SCHEDULE = {0: (32, 4), 3: (32, 4), 1: (40, 162), 2: (40, 162)}


class Unreachable(Exception):
    pass


def plan(v):
    """How to make a render launch instantiation `v`: {scene: (size, content), options, traversal, nee, adaptive, tree}.
    Residency: 2 tiny scene with octant tables, 1 tiny scene without, 0 force_global, 3 a scene over the LDS limit with the
    top-of-tree cache.  SPEC: 2 triangles with diffuse materials only, 1 triangles with other materials too, 0 a scene with
    spheres (STATS kernels) or the mixed triangles with "specialize" off.  Raises Unreachable."""
    res = v.res
    if v.family == 1:
        res, kernel = (1 if v.res else 0), 1
        if v.nee or v.spec or v.postpone or v.thresh or v.inner or v.minw:
            raise Unreachable("trace_kernel has no such template argument")
    elif v.family == 3:
        kernel = 3
        if v.prune or v.nee or v.list:
            raise Unreachable("kernel 3 serves exact traversal without NEE outside adaptive rounds only")
    elif v.family == 2:
        kernel = 2
        if v.postpone:
            raise Unreachable("trace_kernel_v2 has no POSTPONE")
    else:
        raise Unreachable(f"unknown family {v.family}")
    opts = dict(OPTION_DEFAULTS, kernel=kernel, stats=int(v.stats), force_global=int(res == 0), octants=int(res == 2))
    size = "big" if res == 3 else "tiny"
    if v.spec == 2:
        content = "diffuse"
    elif v.spec == 1:
        content = "mixed"
    elif v.stats:
        content = "spheres"
    else:
        content, opts["specialize"] = "mixed", 0
    sched = (v.thresh, v.inner)
    tree, adaptive = "internal", bool(v.list)
    if v.family == 1:
        tree = "callers"                               # kernel 1 always traverses the caller's tree
    elif v.family == 3:
        if res in (1, 2):
            if v.postpone:
                raise Unreachable("leaves are set aside only by scenes in global memory")
        elif not v.postpone:
            tree = "callers"
    elif v.list and v.nee:
        if v.prune or v.spec == 1 or v.minw != 6 or sched != NEE_SCHEDULE[res]:
            raise Unreachable("adaptive NEE rounds run the automatic NEE schedule, exact, SPEC 0 / 2")
    elif v.list:
        if v.minw != 6:
            raise Unreachable("adaptive rounds run MINW 6")
        trees = [t for t in ("internal", "callers") if AUTO_SCHEDULE[res][t] == sched]
        if not trees:
            raise Unreachable("adaptive rounds run the automatic schedule of the residency and tree")
        tree = trees[0]
    elif v.nee:
        if v.prune or v.spec == 1 or v.minw != 6 or sched != NEE_SCHEDULE[res]:
            raise Unreachable("NEE runs the automatic schedule of the residency, exact, SPEC 0 / 2")
    else:
        opts.update(v2_thresh=v.thresh, v2_inner=v.inner, v2_minw=v.minw)
        # leaves set aside need the internal tree; the others alternate between the two trees
        tree = "internal" if (v.inner >= 1000 or v.stats) else "callers"
    opts["fast_tree"] = int(tree == "internal")
    return {"scene": (size, content), "options": opts, "traversal": PT_TRAVERSAL_PRUNED if v.prune else PT_TRAVERSAL_EXACT,
            "nee": bool(v.nee), "adaptive": adaptive, "tree": tree}


def _compiled():
    found = compiled_trace_variants(_build.HIP_LIB)
    return [v for v, _ in found]


def test_trace_kernel_names_parse():
    v = parse_kernel_name("_ZN3ptk15trace_kernel_v2ILi3ELb1ELb0ELi40ELin6ELi5ELi2ELb1ELb0EEEvN3ptl8SceneDevE.kd"[:-3])
    assert v == Variant(2, 3, 1, 0, 2, 1, 0, 0, 40, -6, 5)
    assert Variant.decode(v.code) == v and v.code == 2 | 3 << 4 | 1 << 6 | 2 << 8 | 1 << 10 | 40 << 16 | 0xFFFA << 24 | 5 << 40
    assert parse_kernel_name("_ZN3ptk14trace_kernel_qILi0ELb1ELi1ELb1EEEvN3ptl8SceneDevE") == Variant(3, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0)
    assert parse_kernel_name("_ZN3ptk12trace_kernelILb1ELb0ELb1ELb1EEEvN3ptl8SceneDevE") == Variant(1, 1, 0, 1, 0, 0, 1, 0, 0, 0, 0)
    assert parse_kernel_name("_ZN3ptk13resolve_kernelEPK15HIP_vector_typeIfLj4EEPf") is None


def test_every_compiled_trace_kernel_is_reachable():
    """The code object's trace kernels: a non-empty set without duplicates, each of them reachable through the public API."""
    variants = _compiled()
    assert variants, "no trace kernel found in the gfx950 code object"
    dup = [str(v) for v, n in Counter(variants).items() if n > 1]
    assert not dup, f"compiled more than once: {dup}"
    unreachable = []
    for v in variants:
        try:
            plan(v)
        except Unreachable as e:
            unreachable.append(f"{v}: {e}")
    assert not unreachable, "no way to launch:\n" + "\n".join(unreachable)
    fam = Counter(v.family for v in variants)
    print(f"{len(variants)} trace-kernel instantiations compiled: trace_kernel {fam[1]}, trace_kernel_v2 {fam[2]}, "
          f"trace_kernel_q {fam[3]}")


# tests/golden/trace_kernels.txt: the sorted mangled names of every kernel of the gfx950 code objects whose name contains
# "trace_kernel".  The matrix above and below iterates over what is compiled, so only this list notices an instantiation that
# the dispatcher of csrc/pt_api.hip stopped naming (or names in addition).  A pull request that adds or removes a kernel on
# purpose regenerates it from its own build:
#   python -c "import sys; sys.path.insert(0, 'tests'); from trace_variants import code_object_symbols as s;
#              from pathtracer_cuda_interactive_amd import _build as b;
#              print('\n'.join(sorted(n for co in s(b.HIP_LIB) for n in co if 'trace_kernel' in n)))" > tests/golden/trace_kernels.txt
def test_compiled_trace_kernels_are_the_listed_set():
    from trace_variants import code_object_symbols
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trace_kernels.txt")) as f:
        listed = f.read().split()
    assert listed == sorted(set(listed)), "tests/golden/trace_kernels.txt is not a sorted list of distinct names"
    built = [n for co in code_object_symbols(_build.HIP_LIB) for n in co if "trace_kernel" in n]
    missing, extra = sorted(set(listed) - set(built)), sorted(set(built) - set(listed))
    print(f"{len(built)} trace kernels built, {len(listed)} listed; missing {len(missing)}, extra {len(extra)}")
    for name in missing:
        print("missing:", name)
    for name in extra:
        print("extra:", name)
    assert not missing and not extra, f"{len(missing)} listed kernels are not built, {len(extra)} built kernels are not listed"
    assert len(built) == len(listed), "a trace kernel is compiled into more than one code object"


# ---- GPU --------------------------------------------------------------------------------------------------------------

def _poor_tree(d, seed):
    """A copy of `d` whose caller's tree pairs the leaves up in random order: valid and nested (every box is the union of its
    children's), but poor, so that pt_scene_create keeps its internal tree for every scene of this module."""
    from pathtracer_cuda_interactive_amd.device import NODE_DTYPE
    from pathtracer_cuda_interactive_amd.ctypes_defs import PtBvhNode, PtSceneDesc
    src = np.frombuffer((C.c_char * (d.num_nodes * NODE_DTYPE.itemsize)).from_address(C.addressof(d.nodes.contents)),
                        dtype=NODE_DTYPE)
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
        node = np.zeros(1, NODE_DTYPE)[0]
        node["bmin"] = np.minimum(out[l]["bmin"], out[r]["bmin"])
        node["bmax"] = np.maximum(out[l]["bmax"], out[r]["bmax"])
        node["left"], node["right"], node["prim"] = l, r, -1
        out.append(node)
        return len(out) - 1

    root = build(0, len(leaves))
    nodes = np.array(out, dtype=NODE_DTYPE)
    d2 = PtSceneDesc()
    C.memmove(C.byref(d2), C.byref(d), C.sizeof(PtSceneDesc))
    d2.nodes = nodes.ctypes.data_as(C.POINTER(PtBvhNode))
    d2.num_nodes, d2.root = len(nodes), root
    d2._keep = (nodes, d)
    return d2


def _triangle_scene(seed, n_prims, diffuse_only):
    """Triangles only: a floor of two and a soup of random ones in four meshes, one of them emissive."""
    rng = np.random.default_rng(seed)
    hs = HostScene()
    hs.set_camera((0, 0.5, 4.0), (0, 0, 0), (0, 1, 0), 50.0, W, H, SPP)
    hs.set_background((0.4, 0.5, 0.6))
    kinds = [PT_MAT_DIFFUSE] * 4 if diffuse_only else [PT_MAT_DIFFUSE, PT_MAT_MIRROR, PT_MAT_PLASTIC, PT_MAT_PHONG]
    mats = [hs.add_material(k, rng.random(3) * 0.8 + 0.1, eta=1.3 + float(rng.random()) * 0.5,
                            exponent=float(rng.integers(2, 80))) for k in kinds]
    floor = np.array([[-6, -1.5, -6], [6, -1.5, -6], [6, -1.5, 6], [-6, -1.5, 6]], np.float32)
    hs.add_mesh(floor, np.array([[0, 2, 1], [0, 3, 2]], np.int32), mats[0])
    n = n_prims - 2
    c = (rng.random((n, 1, 3)) * 4 - 2).astype(np.float32)
    P = (c + (rng.random((n, 3, 3)) - 0.5).astype(np.float32) * 1.2).reshape(-1, 3).astype(np.float32)
    cuts = [0, n // 4, n // 2, 3 * n // 4, n]
    for k in range(4):
        m = cuts[k + 1] - cuts[k]
        hs.add_mesh(P[cuts[k] * 3: cuts[k + 1] * 3], np.arange(m * 3, dtype=np.int32).reshape(-1, 3), mats[k],
                    radiance=(3.0, 2.5, 2.0) if k == 3 else None)
    return hs


SCENE_SEEDS = {("tiny", "spheres"): 11, ("tiny", "mixed"): 12, ("tiny", "diffuse"): 13,
               ("big", "spheres"): 21, ("big", "mixed"): 22, ("big", "diffuse"): 23}


def _make_scene(size, content):
    seed = SCENE_SEEDS[(size, content)]
    n = TINY if size == "tiny" else BIG
    if content == "spheres":
        hs = random_scene(seed, n_tris=n - 5, n_spheres=4)          # + the ground sphere; an emissive mesh and sphere
    else:
        hs = _triangle_scene(seed, n, content == "diffuse")
    d = hs.finalize(PT_BVH_SORT_REFERENCE)
    assert d.num_shapes == n
    return hs, _poor_tree(d, seed)


def _pruned_bound(img, want, what):
    """test_device_matches_live_oracle's bound for pruned traversal against the exact image."""
    diff_px = int((np.abs(img - want).max(axis=2) > 0).sum())
    assert diff_px <= 2, f"{what}: {diff_px} pixels differ from the exact oracle image"
    assert abs(float(img.mean()) - float(want.mean())) < 1e-3 * max(float(want.mean()), 1e-6), what


@pytest.mark.gpu
def test_every_compiled_trace_kernel_matches_the_oracle(oracle):
    from test_adaptive import _oracle_groups
    from pathtracer_cuda_interactive_amd import device as dev

    compiled = sorted(set(_compiled()), key=lambda v: (plan(v)["scene"], v))
    scenes, exact, samples, pruned = {}, {}, {}, {}
    ran, failures = set(), []
    try:
        for v in compiled:
            pl = plan(v)
            key = pl["scene"]
            if key not in scenes:
                hs, d = _make_scene(*key)
                ds = dev.DeviceScene(d)
                scenes[key] = (hs, d, ds)
                assert ds.info("fast_tree") == 1 and ds.info("fast_tree_is_callers") == 0, f"{key}: no internal tree"
            hs, d, ds = scenes[key]
            for k, val in pl["options"].items():
                ds.set_option(k, val)
            if pl["options"]["kernel"] >= 2:
                assert ds.info("fast_tree_on") == (pl["tree"] == "internal"), (str(v), pl["tree"])
            flags = PT_RENDER_NEE if pl["nee"] else 0
            p = hs.render_params(W, H, A_SPP if pl["adaptive"] else SPP, seed=97)
            p.traversal, p.flags = pl["traversal"], flags
            if pl["adaptive"]:
                img, spp, _ = ds.render_adaptive(p, A_ERROR, batch_spp=A_BATCH, max_spp=A_MAX, min_luminance=A_MIN_LUM)
                rounds = ds.info("adaptive_rounds")
            else:
                img, spp, rounds = ds.render(p), None, 0
            c = ds.counters()
            got = ds.info("trace_variant")
            ran.add(Variant.decode(got))
            what = f"{v} on {key} ({pl['tree']} tree)"
            try:
                assert got == v.code, f"{what}: launched {Variant.decode(got)}"
                if pl["adaptive"]:
                    assert rounds == 2, f"{what}: {rounds} adaptive rounds"
                    assert c.paths == int(spp.sum()), what
                if pl["traversal"] == PT_TRAVERSAL_EXACT:
                    if pl["adaptive"]:
                        _check_adaptive(oracle, d, p, img, spp, samples, key, flags, what, _oracle_groups)
                    else:
                        if (key, flags) not in exact:
                            exact[(key, flags)] = oracle.render(d, p)
                        want, cnt = exact[(key, flags)]
                        assert_bit_equal(img, want, what)
                        if v.stats and pl["nee"]:
                            assert (c.paths, c.segments) == (cnt.paths, cnt.segments), what    # shadow rays are no segments
                        elif v.stats:
                            assert_work_counters(ds, c, cnt, oracle, d, p, what)
                else:
                    # no oracle for pruned traversal: every kernel that prunes on the same tree renders the same bits,
                    # within the bound of test_device_matches_live_oracle of the exact image
                    group = (key, pl["adaptive"], pl["tree"])
                    if group not in pruned:
                        pruned[group] = (v, img, spp)
                    v0, img0, spp0 = pruned[group]
                    assert_bit_equal(img, img0, f"{what} against {v0}")
                    if pl["adaptive"]:
                        assert (spp == spp0).all(), f"{what}: spp_map differs from {v0}'s"
                        want = _oracle_groups(oracle, d, _with_spp(p, A_SPP, traversal=PT_TRAVERSAL_EXACT), spp,
                                              list(range(H)), A_MAX)
                    else:
                        if (key, 0) not in exact:
                            exact[(key, 0)] = oracle.render(d, _with_spp(p, SPP, traversal=PT_TRAVERSAL_EXACT))
                        want = exact[(key, 0)][0]
                    _pruned_bound(img, want, what)
            except AssertionError as e:
                failures.append(str(e).splitlines()[0])
    finally:
        for _, _, ds in scenes.values():
            ds.close()
    missing = sorted(set(compiled) - ran)
    print(f"trace-kernel matrix: {len(set(compiled) & ran)}/{len(compiled)} compiled instantiations ran")
    assert not failures, f"{len(failures)} instantiations failed:\n" + "\n".join(failures)
    assert not missing, "never launched:\n" + "\n".join(map(str, missing))


@pytest.mark.gpu
def test_a_schedule_without_a_kernel_fails_and_leaves_the_handle_as_it_was():
    """v2_thresh names an instantiation; 41 names none: the render fails with PT_ERR_INVALID_ARG, and once the option is back
    at 0 the handle renders the same bits with the same kernel as before the failure."""
    from pathtracer_cuda_interactive_amd import PT_ERR_INVALID_ARG, PtError
    from pathtracer_cuda_interactive_amd import device as dev
    hs, d = _make_scene("tiny", "diffuse")
    p = hs.render_params(W, H, SPP, seed=97)
    ds = dev.DeviceScene(d)
    try:
        before, variant = ds.render(p), ds.info("trace_variant")
        assert Variant.decode(variant).family == 2
        ds.set_option("v2_thresh", 41)
        with pytest.raises(PtError) as e:
            ds.render(p)
        assert e.value.status == PT_ERR_INVALID_ARG
        assert "no kernel variant compiled for these v2_thresh / v2_inner options" in str(e.value)
        ds.set_option("v2_thresh", 0)
        assert_bit_equal(ds.render(p), before, "the frame after the failed render")
        assert ds.info("trace_variant") == variant
    finally:
        ds.close()


def _with_spp(p, spp, traversal=None):
    q = p.copy()
    q.spp = spp
    if traversal is not None:
        q.traversal = traversal
    return q


def _check_adaptive(oracle, d, p, img, spp, samples, key, flags, what, oracle_groups):
    """An exact adaptive call: spp_map as the stopping rule gives it on the oracle's samples, the image as the oracle's at
    each pixel's own sample count."""
    if (key, flags) not in samples:
        jj, ii = np.mgrid[0:H, 0:W]
        xy = np.stack([ii.reshape(-1), jj.reshape(-1)], axis=1)
        s = np.zeros((W * H, A_MAX, 3), np.float32)
        for k in range(A_MAX):
            q = p.copy()
            q.spp, q.sample_offset, q.stream_stride = 1, k, A_MAX
            s[:, k], _ = oracle.render_pixels(d, q, xy)
        # render_adaptive's default p_value reaches the library as float32(0.05)
        samples[(key, flags)] = adaptive_reference.expected(s, A_SPP, A_BATCH, A_MAX, A_ERROR, A_MIN_LUM, np.float32(0.05))
    E = samples[(key, flags)]
    n_ref, ok = E.n, E.decided                         # pixels whose count the bracketed quantile leaves no doubt about
    assert ok.sum() >= 0.95 * ok.size, what
    got = spp.reshape(-1)
    assert (got[ok] == n_ref[ok]).all(), f"{what}: spp_map differs from the stopping rule at {np.nonzero(got[ok] != n_ref[ok])[0][:5]}"
    assert_bit_equal(img, oracle_groups(oracle, d, p, spp, list(range(H)), A_MAX), what)
