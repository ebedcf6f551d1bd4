"""Tier 0 of the pinning chain: host pipeline, oracle and HIP kernels against recordings of what THE REFERENCE'S OWN
CODE computed — a host build of its unmodified sources (oracle/ref_build/), run by tests/golden/make_reference_recordings.py
over the 14 shipped scenes and the inputs of tests/data/ref_cases/.  The recordings are data under tests/golden/ref/; these tests
need neither the reference nor the probe binaries, except the live leg, which rebuilds the recordings where both exist.

Every comparison is on bit patterns (assert_bit_equal, array equality, SHA-256): no tolerance appears in this file.
Non-finite radiance is outside what is pinned: the generator asserts that no recorded frame holds a NaN or an inf (so the
reference's ternary max / min and the IEEE maxNum / minNum of the deterministic flavour cannot part on these inputs)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
from conftest import GOLDEN, assert_bit_equal, load_scene

sys.path.insert(0, GOLDEN)
import make_reference_recordings as gen  # noqa: E402

from pathtracer_cuda_interactive_amd import (PT_BVH_SORT_REFERENCE, PT_LIGHT_DIFFUSE_AREA, PT_MAT_MIRROR, PT_SHAPE_SPHERE,  # noqa: E402
                                             PT_TRAVERSAL_EXACT, PT_TRAVERSAL_PRUNED, HostScene, PtError)

REC_DIR = os.path.join(GOLDEN, "ref")
CASES = gen.case_names()

# Inputs the reference refuses and our parser loads: named, documented extensions.  Anything else the reference
# rejects, our parser must reject as well.
OURS_ACCEPTS_MORE = {
    "ascii_ply": "ASCII PLY: the reference's bundled PLY reader hands the list-element read its write offset as the buffer size "
                 "(tinyply.h, the ASCII branch of the list reader), so its destination-size check throws 'unexpected EOF' on the "
                 "first face of ANY ascii file - whatever the index type or the property set; the binary form of the same "
                 "mesh loads.  Our reader takes both.",
    "mixed": "tests/data/mixed.xml holds tests/data/tri_ascii.ply: the same ASCII PLY rejection",
}

_recs = {}


def rec(name):
    if name not in _recs:
        with np.load(os.path.join(REC_DIR, name + ".npz")) as z:
            _recs[name] = {k: z[k] for k in z.files}
    return _recs[name]


def accepted(name):
    return str(rec(name)["reference"]) == "accepts"


ACCEPTED = [c for c in CASES if os.path.exists(os.path.join(REC_DIR, c + ".npz")) and accepted(c)]
_ours = {}


def ours(name):
    """(HostScene, desc) of a case as OUR pipeline builds it: the XML for inputs of our own, the .pts fixture for shipped scenes."""
    if name in gen.SHIPPED:
        return load_scene(name)
    if name not in _ours:
        hs = HostScene.load(gen.case_xml(name))
        _ours[name] = (hs, hs.finalize(PT_BVH_SORT_REFERENCE))
    return _ours[name]


def _records(ptr, n, dtype):
    import ctypes as C
    return np.frombuffer(C.string_at(ptr, n * dtype.itemsize), dtype=dtype) if n else np.zeros(0, dtype=dtype)


SHAPE_DT = np.dtype([("type", "<i4"), ("material_id", "<i4"), ("area_light_id", "<i4"), ("center", "<f4", 3), ("radius", "<f4"),
                     ("face_index", "<i4"), ("mesh_index", "<i4")])
MAT_DT = np.dtype([("type", "<i4"), ("reflectance", "<f4", 3), ("eta", "<f4"), ("exponent", "<f4")])
LIGHT_DT = np.dtype([("type", "<i4"), ("shape_id", "<i4"), ("radiance", "<f4", 3), ("position", "<f4", 3)])
NODE_DT = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("left", "<i4"), ("right", "<i4"), ("prim", "<i4")])


def ours_dump(hs, d, w, h):
    """Our flattened scene in the layout of the probe's `dump` (oracle/ref_build/ref_probe.cpp)."""
    out = {}
    sh = _records(d.shapes, d.num_shapes, SHAPE_DT)
    sph = sh["type"] == PT_SHAPE_SPHERE
    ids = np.full((d.num_shapes, 5), -1, dtype=np.int32)
    ids[:, 0] = sh["type"]
    ids[sph, 1], ids[sph, 2] = sh["material_id"][sph], sh["area_light_id"][sph]
    ids[~sph, 3], ids[~sph, 4] = sh["face_index"][~sph], sh["mesh_index"][~sph]
    out["shape_ids"] = ids
    sf = np.zeros((d.num_shapes, 4), dtype=np.float32)
    sf[sph, :3], sf[sph, 3] = sh["center"][sph], sh["radius"][sph]
    out["shape_sphere"] = sf
    mh = np.zeros((d.num_meshes, 4), dtype=np.int32)
    for k in range(d.num_meshes):
        m = d.meshes[k]
        mh[k] = (m.material_id, m.area_light_id, m.num_vertices, m.num_faces)
        out[f"mesh{k}_positions"] = np.ctypeslib.as_array(m.positions, shape=(m.num_vertices, 3)).copy()
        out[f"mesh{k}_normals"] = np.ctypeslib.as_array(m.normals, shape=(m.num_vertices, 3)).copy()
        out[f"mesh{k}_indices"] = np.ctypeslib.as_array(m.indices, shape=(m.num_faces, 3)).copy()
    out["mesh_header"] = mh
    mt = _records(d.materials, d.num_materials, MAT_DT)
    out["material_type"] = mt["type"].astype(np.int32)
    mp = np.zeros((d.num_materials, 5), dtype=np.float32)
    mp[:, :3] = mt["reflectance"]
    mp[:, 3] = np.where(mt["type"] == 2, mt["eta"], np.float32(0))           # a field the type does not have is 0 in the dump
    mp[:, 4] = np.where(mt["type"] == 3, mt["exponent"], np.float32(0))
    out["material_params"] = mp
    lt = _records(d.lights, d.num_lights, LIGHT_DT)
    area = lt["type"] == PT_LIGHT_DIFFUSE_AREA
    out["light_ids"] = np.stack([lt["type"], np.where(area, lt["shape_id"], -1)], axis=1).astype(np.int32).reshape(-1, 2)
    lp = np.zeros((d.num_lights, 6), dtype=np.float32)
    lp[:, :3] = lt["radiance"]
    lp[~area, 3:] = lt["position"][~area]
    out["light_params"] = lp
    nd = _records(d.nodes, d.num_nodes, NODE_DT)
    out["node_box"] = np.concatenate([nd["bmin"], nd["bmax"]], axis=1).astype(np.float32)
    out["node_ids"] = np.stack([nd["left"], nd["right"], nd["prim"]], axis=1).astype(np.int32)
    out["root"] = np.array([d.root, d.num_nodes, hs.bvh_depth], dtype=np.int32)
    out["background"] = np.array(d.background, dtype=np.float32)
    cam = hs.camera
    out["camera"] = np.array([*cam.lookfrom, *cam.lookat, *cam.up, cam.vfov], dtype=np.float32)
    out["film"] = np.array([cam.width, cam.height, cam.spp], dtype=np.int32)
    p = hs.render_params(w, h, 1)
    out["camera_ray_data"] = np.array([p.cam_origin, p.cam_top_left, p.cam_horizontal, p.cam_vertical], dtype=np.float32)
    out["camera_ray_data_film"] = np.array([w, h], dtype=np.int32)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and a.tobytes() == b.tobytes()


def compare_dump(name, mine, want_full=None, recording=None):
    """mine (ours_dump) against a full dump (dict of arrays) or a recording (arrays or hashes per key)."""
    if want_full is not None:
        keys = {k: ("full", v) for k, v in want_full.items()}
    else:
        keys = {k[len("dump_"):]: ("full", v) for k, v in recording.items() if k.startswith("dump_")}
        keys.update({k[len("dumpsha_"):]: ("sha", str(v)) for k, v in recording.items() if k.startswith("dumpsha_")})
    assert keys, name
    assert sorted(mine) == sorted(keys), f"{name}: arrays {sorted(set(mine) ^ set(keys))} on one side only"
    bad = []
    for k, (kind, want) in sorted(keys.items()):
        got = mine[k]
        if kind == "sha":
            if tuple(recording["dumpshape_" + k]) != got.shape or gen.hashed(got) != want:
                bad.append(f"{k}: shape {got.shape} vs {tuple(recording['dumpshape_' + k])}, SHA-256 differs")
        elif not same_bits(got, want):
            if got.shape != want.shape:
                bad.append(f"{k}: shape {got.shape} vs {want.shape}")
            else:
                w = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
                bad.append(f"{k}: {len(w)} of {got.size} words differ, first at {tuple(w[0])}: ours {got[tuple(w[0])]!r} vs "
                           f"reference {want[tuple(w[0])]!r}")
    assert not bad, f"{name}: host pipeline != reference Scene:\n  " + "\n  ".join(bad)


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_every_case_is_recorded():
    assert sorted(os.path.splitext(f)[0] for f in os.listdir(REC_DIR) if f.endswith(".npz")) == sorted(CASES)
    assert len(gen.SHIPPED) == 14 and all(accepted(c) for c in gen.SHIPPED)
    for c in ACCEPTED:
        r = rec(c)
        for f in ("frame_libm_per_pixel", "frame_libm_per_sample", "frame_det_per_sample"):
            w, h, _ = r["size"]
            assert r[f].shape == (h, w, 3) and r[f].dtype == np.float32 and np.isfinite(r[f]).all(), (c, f)
        assert r["rays"].shape == (gen.N_RAYS, 8) and r["hit"].shape == (gen.N_RAYS, 7)
        assert os.path.getsize(os.path.join(REC_DIR, c + ".npz")) < 256 * 1024


@pytest.mark.parametrize("name", [c for c in CASES if c not in ACCEPTED])
def test_inputs_the_reference_rejects(name):
    """What the reference refuses, we refuse too - or it is a named extension."""
    r = rec(name)
    assert str(r["reference"]) == "rejects" and str(r["message"])
    if name in OURS_ACCEPTS_MORE:
        assert "unexpected EOF" in str(r["message"])
        hs = HostScene.load(gen.case_xml(name))          # the extension is real: ours loads it
        assert hs.finalize(PT_BVH_SORT_REFERENCE).num_shapes > 0
    else:
        with pytest.raises(PtError):
            HostScene.load(gen.case_xml(name))


def test_named_extensions_are_rejected_by_the_reference():
    assert sorted(OURS_ACCEPTS_MORE) == sorted(c for c in CASES if c not in ACCEPTED)


@pytest.mark.parametrize("name", ACCEPTED)
def test_host_pipeline_equals_reference_scene(name):
    """1. shapes, mesh arrays, materials, lights, every BVH node, root, background and the camera vectors, bit for bit."""
    hs, d = ours(name)
    w, h, _ = rec(name)["size"]
    compare_dump(name, ours_dump(hs, d, int(w), int(h)), recording=rec(name))


_renders = {}


def oracle_render(oracle, name, math_mode, rng_mode):
    key = (name, math_mode, rng_mode)
    if key not in _renders:
        hs, d = ours(name)
        w, h, spp = (int(v) for v in rec(name)["size"])
        _renders[key] = oracle.render(d, hs.render_params(w, h, spp, seed=gen.SEED), math_mode=math_mode, rng_mode=rng_mode)
    return _renders[key]


@pytest.mark.parametrize("name", ACCEPTED)
def test_oracle_frames_equal_reference_frames(oracle, name):
    """2a. both flavours of the oracle against the frame the matching build of the reference rendered."""
    r = rec(name)
    for key, mm, rm in (("frame_libm_per_pixel", oracle.MATH_LIBM, oracle.RNG_PER_PIXEL),
                        ("frame_libm_per_sample", oracle.MATH_LIBM, oracle.RNG_PER_SAMPLE),
                        ("frame_det_per_sample", oracle.MATH_DET, oracle.RNG_PER_SAMPLE)):
        assert_bit_equal(oracle_render(oracle, name, mm, rm)[0], r[key], f"{name} {key}")


def centre_rays(r):
    n = r["centre_dir"].shape[0]
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, :3], rays[:, 3:6], rays[:, 6], rays[:, 7] = r["centre_origin"], r["centre_dir"], 0.0, np.inf
    return rays


def check_hits(what, hit, ids, want_hit, want_ids):
    valid = want_ids[:, 0] == 1
    assert np.array_equal(ids[:, 0] >= 0, valid), f"{what}: {int(((ids[:, 0] >= 0) != valid).sum())} rays hit on one side only"
    assert_bit_equal(hit[:, 0], want_hit[:, 0], what + " distance")
    assert_bit_equal(hit[:, 1:4], want_hit[:, 1:4], what + " position")
    assert_bit_equal(hit[:, 4:7], want_hit[:, 4:7], what + " shading normal")
    assert np.array_equal(ids[:, 1:], want_ids[:, 1:]), what + " material / area-light ids"


@pytest.mark.parametrize("name", ACCEPTED)
def test_oracle_hits_equal_reference_intersect(oracle, name):
    """2b. 1,024 explicit rays and the pixel-centre rays: valid, distance, position, shading normal, material and light id."""
    r = rec(name)
    _, d = ours(name)
    for mm in (oracle.MATH_LIBM, oracle.MATH_DET):
        hit, ids = oracle.intersect_full(d, r["rays"], math_mode=mm)
        check_hits(f"{name} rays math={mm}", hit, ids, r["hit"], r["hit_ids"])
        hit, ids = oracle.intersect_full(d, centre_rays(r), math_mode=mm)
        check_hits(f"{name} pixel centres math={mm}", hit, ids, r["centre_hit"], r["centre_ids"])
        # the short accessor the device tests use agrees with the long one
        tuv, prim = oracle.intersect(d, r["rays"], math_mode=mm)
        hit, ids = oracle.intersect_full(d, r["rays"], math_mode=mm)
        assert np.array_equal(prim, ids[:, 0]) and same_bits(tuv[:, 0], hit[:, 0])


# mutation -> cases whose frames run through the mutated code (diffuse surfaces; paths longer than 5 bounces; Schlick's term)
MUTATIONS = {
    "PT_ORACLE_MUT_DIFFUSE_NO_INV_PI": (1, ("cbox", "scene1", "meshes")),
    "PT_ORACLE_MUT_RR_NO_WEIGHT": (2, ("inside_sphere", "cbox", "mirrors")),
    "PT_ORACLE_MUT_SCHLICK_POW4": (4, ("plastic", "mirrors", "scene1")),
    # the UNBIASED control: a bit-exact pin rejects it too.  The floor shows only where a path is more than 5 bounces deep with a
    # throughput above 0.5: the closed bright sphere (nothing ends by a miss) and the closed-in box
    "PT_ORACLE_MUT_RR_FLOOR_QUARTER": (8, ("inside_sphere", "cbox")),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_the_pin_can_fail(oracle, mutation):
    """3. With one term of the estimator changed, the cases that use it no longer match their recording."""
    bits, cases = MUTATIONS[mutation]
    lib = oracle.lib()
    for name in cases:
        hs, d = ours(name)
        w, h, spp = (int(v) for v in rec(name)["size"])
        want = rec(name)["frame_det_per_sample"]
        assert_bit_equal(oracle_render(oracle, name, oracle.MATH_DET, oracle.RNG_PER_SAMPLE)[0], want, name)
        old = lib.pt_oracle_set_mutation(bits)
        try:
            img, _ = oracle.render(d, hs.render_params(w, h, spp, seed=gen.SEED))
        finally:
            lib.pt_oracle_set_mutation(old)
        assert not same_bits(img, want), f"{mutation}: {name} still matches the reference's frame"


def test_case_list_covers_what_a_restatement_can_get_wrong(oracle):
    """4. Keeps the case list from quietly shrinking: from the recorded dumps, rays and the oracle's counters."""
    on_sphere, on_mesh, light_kinds = set(), set(), set()
    behind = zero_component = term_rr = 0
    for name in ACCEPTED:
        r = rec(name)
        if "dump_shape_ids" in r:
            sid, mt = r["dump_shape_ids"], r["dump_material_type"]
            on_sphere |= {int(mt[m]) for m in sid[sid[:, 0] == 0, 1] if m >= 0}
            used = np.unique(sid[sid[:, 0] == 1, 4])
            on_mesh |= {int(mt[m]) for m in r["dump_mesh_header"][used, 0] if m >= 0}
            light_kinds |= {int(t) for t in r["dump_light_ids"][:, 0]}
        for dirs, hit, ids in ((r["rays"][:, 3:6], r["hit"], r["hit_ids"]), (r["centre_dir"], r["centre_hit"], r["centre_ids"])):
            lit = (ids[:, 0] == 1) & (ids[:, 2] >= 0)
            behind += int((lit & ((-dirs * hit[:, 4:7]).sum(axis=1) < 0)).sum())
            zero_component += int(((dirs == 0).any(axis=1) & (ids[:, 0] == 1)).sum())
        term_rr += oracle_render(oracle, name, oracle.MATH_DET, oracle.RNG_PER_SAMPLE)[1].term_rr
    assert on_sphere == {0, 1, 2, 3} and on_mesh == {0, 1, 2, 3}, (on_sphere, on_mesh)
    assert light_kinds == {0, 1}
    assert behind > 0, "no emitter is hit from its back side"
    assert term_rr > 0
    assert zero_component > 0, "no ray with a zero direction component hits anything"
    # a tie on t: ties.obj holds every triangle of its unit quad twice; the twins differ in their normals only, so the recorded
    # shading normal says which one the reference's traversal kept
    r = rec("ties")
    P, I, N = r["dump_mesh0_positions"], r["dump_mesh0_indices"], r["dump_mesh0_normals"]
    tri = P[I].reshape(len(I), 9)
    twins = [(a, b) for a in range(len(I)) for b in range(a + 1, len(I)) if np.array_equal(tri[a], tri[b])]
    assert len(twins) == 2 and all(not np.array_equal(N[I[a]], N[I[b]]) for a, b in twins)
    _, d = ours("ties")
    _, prim = oracle.intersect(d, np.concatenate([r["rays"], centre_rays(r)]))
    mesh0 = np.flatnonzero((r["dump_shape_ids"][:, 0] == 1) & (r["dump_shape_ids"][:, 4] == 0))
    twin_prims = {int(mesh0[t]) for pair in twins for t in pair}
    assert sum(int(p) in twin_prims for p in prim) > 50, "hardly a ray ends on the coincident triangles"


def _live_leg_missing():
    miss = [p for p in (*gen.PROBES.values(), os.path.join(gen.REF_DEFAULT, "scenes")) if not os.path.exists(p)]
    return "live leg needs the reference's sources and both probe binaries (missing: %s)" % ", ".join(miss) if miss else ""


@pytest.mark.skipif(bool(_live_leg_missing()), reason=_live_leg_missing() or "-")
def test_live_recordings_come_back_byte_for_byte(tmp_path):
    """5a. Rerun the generator with the probes built from the reference: every committed recording comes back unchanged."""
    gen.generate(str(tmp_path))
    names = sorted(os.listdir(REC_DIR))
    assert names == sorted(os.listdir(tmp_path))
    bad = [n for n in names if open(os.path.join(REC_DIR, n), "rb").read() != open(os.path.join(tmp_path, n), "rb").read()]
    assert not bad, f"recordings that did not come back byte for byte: {bad}"


@pytest.mark.skipif(bool(_live_leg_missing()), reason=_live_leg_missing() or "-")
@pytest.mark.parametrize("name", list(gen.SHIPPED))
def test_live_shipped_xml_parses_like_the_reference(tmp_path, name):
    """5b. The only place the shipped XMLs are read: our parser on the XML itself against a fresh dump of the reference."""
    xml = gen.case_xml(name)
    hs = HostScene.load(xml)
    d = hs.finalize(PT_BVH_SORT_REFERENCE)
    w, h, _ = gen.case_size(name)
    compare_dump(name, ours_dump(hs, d, w, h), want_full=gen.probe("libm", "dump", xml, w, h, tmp=str(tmp_path)))


# ---------------------------------------------------------------------------------------------------------------- GPU

KERNELS, FAST_TREE, FORCE_GLOBAL = (1, 2, 3), (0, 1), (0, 1)
FRAMES_PER_CASE = len(KERNELS) * len(FAST_TREE) * len(FORCE_GLOBAL) + 2


@pytest.fixture(scope="module")
def dscene():
    from pathtracer_cuda_interactive_amd import device as dev
    cache = {}

    def get(name):
        if name not in cache:
            for s in cache.values():       # one resident scene at a time (bunny is the big one)
                s.close()
            cache.clear()
            cache[name] = dev.DeviceScene(ours(name)[1])
        return cache[name]
    yield get
    for s in cache.values():
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ACCEPTED)
def test_device_frame_equals_the_references_own_frame(dscene, name):
    """6. Exact traversal, kernels 1 / 2 / 3 x fast_tree x force_global, pt_render_accumulate in two calls and two row bands,
    each against the det/per_sample frame the reference's code rendered - directly, not through the oracle."""
    import torch
    hs, _ = ours(name)
    ds = dscene(name)
    want = rec(name)["frame_det_per_sample"]
    w, h, spp = (int(v) for v in rec(name)["size"])
    p = hs.render_params(w, h, spp, seed=gen.SEED)
    frames = 0
    try:
        for kernel in KERNELS:
            for fast in FAST_TREE:
                for fg in FORCE_GLOBAL:
                    ds.set_option("kernel", kernel)
                    ds.set_option("fast_tree", fast)
                    ds.set_option("force_global", fg)
                    img = ds.render(p, traversal=PT_TRAVERSAL_EXACT)
                    assert_bit_equal(img, want, f"{name} kernel={kernel} fast_tree={fast} force_global={fg}")
                    frames += 1
    finally:
        ds.set_option("kernel", 2)
        ds.set_option("fast_tree", 1)
        ds.set_option("force_global", 0)
    # render_progressive: all samples but the last, then the last (the reference's sum runs in sample order), scaled as main.cu:50
    acc = torch.full((h, w, 3), 77.0, dtype=torch.float32, device="cuda")
    for off, n in ([(0, spp - 1), (spp - 1, 1)] if spp > 1 else [(0, 1)]):
        q = hs.render_params(w, h, n, seed=gen.SEED)
        q.sample_offset, q.stream_stride, q.traversal = off, spp, PT_TRAVERSAL_EXACT
        ds.accumulate_into(q, acc.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    inv = np.float32(1.0) / np.float32(spp)
    assert_bit_equal(acc.cpu().numpy() * inv, want, f"{name} pt_render_accumulate")
    bands = []
    for rb, re in ((0, h // 2 - 3), (h // 2 - 3, h)):
        q = p.copy()
        q.row_begin, q.row_end = rb, re
        bands.append(ds.render(q, traversal=PT_TRAVERSAL_EXACT))
    assert_bit_equal(np.concatenate(bands, axis=0), want, f"{name} two row bands")
    assert frames + 2 == FRAMES_PER_CASE


def _prim_ids(d, prim):
    """material and area-light id of a shape id, as the reference's Intersection reports them (-1, -1 on a miss)."""
    sh = _records(d.shapes, d.num_shapes, SHAPE_DT)
    mh = np.array([(d.meshes[k].material_id, d.meshes[k].area_light_id) for k in range(d.num_meshes)], dtype=np.int32).reshape(-1, 2)
    sph = sh["type"] == PT_SHAPE_SPHERE
    mat = np.where(sph, sh["material_id"], mh[np.where(sph, 0, sh["mesh_index"]), 0] if len(mh) else -1)
    light = np.where(sph, sh["area_light_id"], mh[np.where(sph, 0, sh["mesh_index"]), 1] if len(mh) else -1)
    hit = prim >= 0
    safe = np.where(hit, prim, 0)
    return np.where(hit, mat[safe], -1), np.where(hit, light[safe], -1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ACCEPTED)
def test_device_hits_and_first_hit_buffers_equal_reference_intersect(dscene, name):
    """7. pt_debug_intersect (exact and pruned) against the recorded hits; pt_render_aov's depth / normal / primitive / albedo
    against the reference's intersect() for the pixel-centre rays."""
    r = rec(name)
    hs, d = ours(name)
    ds = dscene(name)
    valid = r["hit_ids"][:, 0] == 1
    for trav in (PT_TRAVERSAL_EXACT, PT_TRAVERSAL_PRUNED):
        tuv, prim = ds.intersect(r["rays"], traversal=trav)
        assert np.array_equal(prim >= 0, valid), f"{name} traversal={trav}"
        assert_bit_equal(np.where(valid, tuv[:, 0], 0), r["hit"][:, 0], f"{name} traversal={trav} distance")
        mat, light = _prim_ids(d, prim)
        assert np.array_equal(mat, r["hit_ids"][:, 1]) and np.array_equal(light, r["hit_ids"][:, 2]), f"{name} traversal={trav} ids"
    cw, ch = (int(v) for v in r["centre_size"])
    cvalid = (r["centre_ids"][:, 0] == 1).reshape(ch, cw)
    for fast in FAST_TREE:
        ds.set_option("fast_tree", fast)
        try:
            aov = ds.render_aov(hs.render_params(cw, ch, 1), traversal=PT_TRAVERSAL_EXACT)
        finally:
            ds.set_option("fast_tree", 1)
        what = f"{name} aov fast_tree={fast}"
        assert np.array_equal(aov["prim"] >= 0, cvalid), what
        assert_bit_equal(aov["depth"], r["centre_hit"][:, 0].reshape(ch, cw), what + " depth")
        # the renderer's turn of the normal towards the ray (radiance.cuh:45-47): dot(-dir, n) < 0, summed left to right in fp32
        n, dirs = r["centre_hit"][:, 4:7], r["centre_dir"]
        dot = ((-dirs[:, 0] * n[:, 0]) + (-dirs[:, 1] * n[:, 1])) + (-dirs[:, 2] * n[:, 2])
        turned = np.where((dot < 0)[:, None], -n, n).astype(np.float32)
        turned[~cvalid.reshape(-1)] = 0.0
        assert_bit_equal(aov["normal"], turned.reshape(ch, cw, 3), what + " normal")
        mat, light = _prim_ids(d, aov["prim"].reshape(-1))
        assert np.array_equal(mat, r["centre_ids"][:, 1]) and np.array_equal(light, r["centre_ids"][:, 2]), what + " ids"
        # albedo: the hit material's reflectance, (1,1,1) for a mirror, 0 on a miss and where the first segment adds emission
        mt = _records(d.materials, d.num_materials, MAT_DT)
        lt = _records(d.lights, d.num_lights, LIGHT_DT)
        hitm = cvalid.reshape(-1)
        alb = np.zeros((cw * ch, 3), dtype=np.float32)
        alb[hitm] = np.where((mt["type"][mat[hitm]] == PT_MAT_MIRROR)[:, None], np.float32(1), mt["reflectance"][mat[hitm]])
        in_range = hitm & (light >= 0) & (light < d.num_lights)
        emits = np.zeros(cw * ch, dtype=bool)
        emits[in_range] = (lt["type"][light[in_range]] == PT_LIGHT_DIFFUSE_AREA) & (dot[in_range] > 0)
        alb[emits] = 0.0
        assert_bit_equal(aov["albedo"], alb.reshape(ch, cw, 3), what + " albedo")


with open(os.path.join(REC_DIR, "bench_frames.json")) as _f:
    BENCH_FRAMES = json.load(_f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(gen.BENCH_FRAMES))
def test_benchmarked_frame_equals_the_references_frame(oracle, dscene, name):
    """8. The three single-GPU BASELINE.json configs, set up as bench.py sets them up (seed 1984, default options, exact
    traversal): SHA-256, mean and max of the whole frame against what the reference's code rendered."""
    want = BENCH_FRAMES[name]
    assert (want["width"], want["height"], want["spp"]) == gen.BENCH_FRAMES[name]
    hs, d = ours(name)
    p = hs.render_params(want["width"], want["height"], want["spp"], seed=want["seed"])
    p.traversal = PT_TRAVERSAL_EXACT
    img = dscene(name).render(p)
    got = {"sha256": hashlib.sha256(img.tobytes()).hexdigest(), "mean": float(img.mean(dtype=np.float64)), "max": float(img.max())}
    print(f"{name} {want['width']}x{want['height']} spp={want['spp']}: {got}")
    if got["sha256"] != want["sha256"]:
        # the recording is a hash: the oracle (equal to the reference on every recorded case) can say where the frames part
        ref, _ = oracle.render(d, p)
        bad = np.argwhere((img.view(np.uint32) != ref.view(np.uint32)).any(axis=2))
        where = f"first pixel that differs from the oracle: (x={bad[0][1]}, y={bad[0][0]}) device {img[tuple(bad[0])]} oracle " \
                f"{ref[tuple(bad[0])]}, {len(bad)} pixels" if len(bad) else "the device equals the oracle: the oracle differs from the reference here"
        raise AssertionError(f"{name}: SHA-256 {got['sha256']} != {want['sha256']}; {where}")
    assert got["mean"] == want["mean"] and got["max"] == want["max"]
