"""Host half of pt_scene_transform (no GPU): pt_transform_geometry_host / pt_transform_sphere_host are csrc/pt_transform.h
compiled for the host, the rule the device kernel runs.  They equal a numpy fp32 restatement bit for bit, refuse what the rule
refuses, and transform_desc_host — the desc a transformed handle stands for — applies every matrix to the rest pose."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import REPO, load_scene, random_scene

from pathtracer_cuda_interactive_amd import PT_ERR_INVALID_ARG, PT_ERR_UNSUPPORTED, PT_SHAPE_SPHERE, PtError, PtTransform, host
from pathtracer_cuda_interactive_amd import device as dev
from pathtracer_cuda_interactive_amd.standins import mesh_arrays

f32 = np.float32


def np_point(M, P):
    """x' = ((m0 x + m1 y) + m2 z) + m3 in fp32, every product and sum rounded on its own."""
    M, P = M.astype(f32), P.astype(f32)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], axis=1)


def np_cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=f32)


def np_normal_matrix(M):
    M = M.astype(f32)
    r0, r1, r2 = M[0, :3], M[1, :3], M[2, :3]
    c = np.stack([np_cross(r1, r2), np_cross(r2, r0), np_cross(r0, r1)])
    det = (r0[0] * c[0, 0] + r0[1] * c[0, 1]) + r0[2] * c[0, 2]
    return (-c if det < 0 else c), det


def np_normal(M, N):
    c, _ = np_normal_matrix(M)
    N = N.astype(f32)
    x, y, z = N[:, 0], N[:, 1], N[:, 2]
    return np.stack([(c[r, 0] * x + c[r, 1] * y) + c[r, 2] * z for r in range(3)], axis=1)


def np_radius(M, r):
    M = M.astype(f32)
    return f32(r) * np.sqrt((M[0, 0] * M[0, 0] + M[1, 0] * M[1, 0]) + M[2, 0] * M[2, 0])


def matrices():
    rng = np.random.default_rng(3)
    out = {f"random{k}": (rng.standard_normal((3, 4)) * (0.1, 1.0, 30.0)[k % 3]).astype(f32) for k in range(6)}
    out["rotation"] = dev.rigid_matrix((1.0, 2.0, -0.5), 37.0, centre=(0.3, -1.0, 2.0))
    out["mirror"] = np.array([[-1, 0, 0, 0.25], [0, 1, 0, 0], [0, 0, 1, -0.5]], f32)
    out["scale"] = np.array([[2.5, 0, 0, 0], [0, 0.3, 0, 1], [0, 0, -1.25, 0]], f32)
    out["translation"] = np.array([[1, 0, 0, 0.1], [0, 1, 0, -7.5], [0, 0, 1, 1e-3]], f32)
    return out


MATRICES = matrices()


def same_bits(a, b):
    return np.ascontiguousarray(a, f32).tobytes() == np.ascontiguousarray(b, f32).tobytes()


def test_pt_transform_is_48_bytes_and_matches_the_header():
    assert C.sizeof(PtTransform) == 48 and PtTransform._fields_[0][0] == "m"
    text = open(os.path.join(REPO, "include", "pt_api.h")).read()
    m = re.search(r"typedef struct pt_transform \{ float m\[(\d+)\]; \} pt_transform;", text)
    assert m and int(m.group(1)) * 4 == C.sizeof(PtTransform)


@pytest.mark.parametrize("name", sorted(MATRICES))
def test_host_twin_equals_the_numpy_restatement(name):
    M = MATRICES[name]
    rng = np.random.default_rng(11)
    P = (rng.standard_normal((1000, 3)) * 5).astype(f32)
    N = rng.standard_normal((1000, 3)).astype(f32)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    Po, No = dev.transform_geometry_host(M, P, N)
    assert same_bits(Po, np_point(M, P)), name
    assert same_bits(No, np_normal(M, N)), name
    P_only, none = dev.transform_geometry_host(M, P)
    assert none is None and same_bits(P_only, Po)
    for k in range(20):
        c, r = P[k], f32(0.05 + k)
        co, ro = dev.transform_sphere_host(M, c, r)
        assert same_bits(co, np_point(M, c[None])[0]) and same_bits(ro, np_radius(M, r)), (name, k)
    _, det = np_normal_matrix(M)
    if name == "mirror":
        assert det < 0 and same_bits(No, N * np.array([-1, 1, 1], f32))     # cofactors (1, -1, -1), negated: the reflected normal
    if name == "translation":
        assert same_bits(No, N)
    if name == "rotation":
        assert np.abs(np.linalg.norm(No, axis=1) - 1).max() < 1e-5 and np.abs(Po - (P @ M[:, :3].T + M[:, 3])).max() < 1e-4


def test_in_place_transform_is_allowed():
    M = MATRICES["rotation"]
    P = np.arange(30, dtype=f32).reshape(10, 3)
    want, _ = dev.transform_geometry_host(M, P)
    t = PtTransform((C.c_float * 12)(*M.reshape(-1).tolist()))
    ptr = P.ctypes.data_as(C.c_void_p)
    assert dev.lib().pt_transform_geometry_host(C.byref(t), 10, ptr, None, ptr, None) == 0
    assert same_bits(P, want)


def test_refused_transforms_name_the_entry():
    P = np.ones((4, 3), f32)
    singular = np.array([[1, 2, 3, 0], [2, 4, 6, 0], [0, 0, 1, 0]], f32)
    nan = MATRICES["rotation"].copy(); nan[1, 2] = np.nan
    inf = MATRICES["rotation"].copy(); inf[2, 3] = np.inf
    for M, word in ((singular, "singular"), (np.zeros((3, 4), f32), "singular"), (nan, "m[6]"), (inf, "m[11]")):
        for call in (lambda: dev.transform_geometry_host(M, P), lambda: dev.transform_sphere_host(M, P[0], 1.0)):
            with pytest.raises(PtError) as e:
                call()
            assert e.value.status == PT_ERR_INVALID_ARG and word in str(e.value), str(e.value)
    # finite entries whose cofactors overflow: every normal would be infinite
    with pytest.raises(PtError) as e:
        dev.transform_geometry_host(dev.rigid_matrix((0, 1, 0), 0.0, scale=1e30), P)
    assert e.value.status == PT_ERR_UNSUPPORTED and "normal matrix" in str(e.value), str(e.value)
    big, _ = dev.transform_geometry_host(dev.rigid_matrix((0, 1, 0), 0.0, scale=1e18), P, P)
    assert np.isfinite(big).all()


def test_null_arguments_are_refused():
    lib = dev.lib()
    t = PtTransform((C.c_float * 12)(*MATRICES["rotation"].reshape(-1).tolist()))
    P = np.ones((4, 3), f32)
    p = P.ctypes.data_as(C.c_void_p)
    fp = P.ctypes.data_as(C.POINTER(C.c_float))
    r = C.c_float()
    for args in ((None, 4, p, None, p, None), (C.byref(t), 4, None, None, p, None), (C.byref(t), 4, p, None, None, None),
                 (C.byref(t), 4, p, p, p, None), (C.byref(t), 4, p, None, p, p), (C.byref(t), -1, p, None, p, None)):
        assert lib.pt_transform_geometry_host(*args) == PT_ERR_INVALID_ARG
        assert "pt_transform_geometry_host" in lib.pt_last_error().decode()
    for args in ((None, fp, 1.0, fp, C.byref(r)), (C.byref(t), None, 1.0, fp, C.byref(r)), (C.byref(t), fp, 1.0, None, C.byref(r)),
                 (C.byref(t), fp, 1.0, fp, None)):
        assert lib.pt_transform_sphere_host(*args) == PT_ERR_INVALID_ARG
    # the scene entry points refuse a null handle, and a null array, before they touch HIP
    ids = np.zeros(4, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.pt_scene_set_groups(None, ids, 1) == PT_ERR_INVALID_ARG
    assert lib.pt_scene_set_groups(C.c_void_p(16), None, 1) == PT_ERR_INVALID_ARG
    assert lib.pt_scene_set_groups(C.c_void_p(16), ids, -1) == PT_ERR_INVALID_ARG
    assert lib.pt_scene_set_groups(C.c_void_p(16), ids, (1 << 20) + 1) == PT_ERR_INVALID_ARG
    assert "num_groups" in lib.pt_last_error().decode()
    assert lib.pt_scene_transform(None, C.byref(t), 1) == PT_ERR_INVALID_ARG


def rest_desc():
    return random_scene(7).finalize()


def spin(d, deg):
    """One matrix per object of `d` (groups_by_object): each mesh about its centroid, each sphere about the origin."""
    ids, G = dev.groups_by_object(d)
    M = np.empty((G, 3, 4), f32)
    for g in range(G):
        c = mesh_arrays(d, g)[0].astype(np.float64).mean(axis=0) if g < d.num_meshes else (0.0, 0.0, 0.0)
        M[g] = dev.rigid_matrix((0.2, 1.0, 0.1), deg * (1 + g % 3), centre=c)
    return ids, M


def geometry_bytes(d):
    out = [dev.shape_table(d).tobytes()]
    for m in range(d.num_meshes):
        out += [a.tobytes() for a in mesh_arrays(d, m)]
    return b"".join(out)


def test_groups_by_object_numbers_meshes_then_spheres():
    d = rest_desc()
    ids, G = dev.groups_by_object(d)
    sh = dev.shape_table(d)
    sphere = sh["type"] == PT_SHAPE_SPHERE
    assert G == d.num_meshes + int(sphere.sum()) and ids.dtype == np.int32
    assert np.array_equal(ids[~sphere], sh["mesh_index"][~sphere])
    assert np.array_equal(ids[sphere], d.num_meshes + np.arange(int(sphere.sum())))


def test_transform_desc_host_applies_every_matrix_to_the_rest_pose():
    """Absolute, not cumulative: rotating by theta and then by -theta gives rest x R(-theta), not rest — transform_desc_host
    reads nothing but the rest desc and the matrices of the call, so nothing composes and nothing drifts."""
    d = rest_desc()
    ids, M1 = spin(d, 20.0)
    _, M2 = spin(d, -20.0)
    first = dev.transform_desc_host(d, ids, M1)
    second = dev.transform_desc_host(d, ids, M2)
    again = dev.transform_desc_host(d, ids, M1)
    assert geometry_bytes(first) == geometry_bytes(again)
    assert geometry_bytes(second) != geometry_bytes(d) and geometry_bytes(second) != geometry_bytes(first)
    # second is rest under R(-theta), mesh by mesh and sphere by sphere
    sh, sh2 = dev.shape_table(d), dev.shape_table(second)
    for m in range(d.num_meshes):
        P, I, N = mesh_arrays(d, m)
        P2, I2, N2 = mesh_arrays(second, m)
        assert np.array_equal(I, I2) and same_bits(P2, np_point(M2[m], P)) and same_bits(N2, np_normal(M2[m], N))
    for i in np.flatnonzero(sh["type"] == PT_SHAPE_SPHERE):
        assert same_bits(sh2["center"][i], np_point(M2[ids[i]], sh["center"][i][None])[0])
        assert same_bits(sh2["radius"][i], np_radius(M2[ids[i]], sh["radius"][i]))
    # the rest desc is left alone
    assert geometry_bytes(d) == geometry_bytes(rest_desc())


def test_transform_desc_host_with_groups_per_shape_splits_shared_vertices():
    _, d = load_scene("cbox")
    rng = np.random.default_rng(5)
    G = 5
    ids = rng.integers(-1, G, d.num_shapes).astype(np.int32)
    M = np.stack([dev.rigid_matrix(rng.standard_normal(3), 10.0 * (g + 1), centre=(278, 273, 280)) for g in range(G)])
    d2 = dev.transform_desc_host(d, ids, M)
    sh = dev.shape_table(d)
    assert dev.shape_table(d2).tobytes() == sh.tobytes()
    for i in range(d.num_shapes):
        P, I, N = mesh_arrays(d, sh["mesh_index"][i])
        P2, I2, N2 = mesh_arrays(d2, sh["mesh_index"][i])
        v, v2 = I[sh["face_index"][i]], I2[sh["face_index"][i]]
        if ids[i] < 0:
            assert same_bits(P2[v2], P[v]) and same_bits(N2[v2], N[v])
        else:
            assert same_bits(P2[v2], np_point(M[ids[i]], P[v])) and same_bits(N2[v2], np_normal(M[ids[i]], N[v]))
    with pytest.raises(ValueError):
        dev.transform_desc_host(d, ids[:-1], M)
    with pytest.raises(ValueError):
        dev.transform_desc_host(d, np.full(d.num_shapes, G, np.int32), M)


def test_refit_of_a_host_transformed_cbox_gives_nested_finite_boxes():
    """The pool the GPU tests' fresh-create comparison uses."""
    _, d = load_scene("cbox")
    ids, G = dev.groups_by_object(d)
    M = np.stack([dev.rigid_matrix((0, 1, 0), 15.0 + 5 * g, centre=mesh_arrays(d, g)[0].mean(axis=0)) if g >= 6
                  else dev.rigid_matrix((0, 1, 0), 0.0) for g in range(G)])
    d1 = dev.transform_desc_host(d, ids, M)
    r = host.refit_bvh(d1)
    nodes = np.frombuffer(C.string_at(r.nodes, r.num_nodes * host.NODE_DTYPE.itemsize), dtype=host.NODE_DTYPE)
    before = np.frombuffer(C.string_at(d.nodes, d.num_nodes * host.NODE_DTYPE.itemsize), dtype=host.NODE_DTYPE)
    assert r.num_nodes == d.num_nodes and r.root == d.root
    for f in ("left", "right", "prim"):
        assert np.array_equal(nodes[f], before[f])
    assert np.isfinite(nodes["bmin"]).all() and np.isfinite(nodes["bmax"]).all()
    assert (nodes["bmin"] != before["bmin"]).any()
    inner = np.flatnonzero(nodes["prim"] == -1)
    for side in ("left", "right"):
        c = nodes[nodes[side][inner]]
        assert (c["bmin"] >= nodes["bmin"][inner]).all() and (c["bmax"] <= nodes["bmax"][inner]).all()
    # every leaf box is its triangle's box under the matrix
    sh = dev.shape_table(d1)
    for k in np.flatnonzero(nodes["prim"] != -1)[:40]:
        s = sh[nodes["prim"][k]]
        P, I, _ = mesh_arrays(d1, s["mesh_index"])
        tri = P[I[s["face_index"]]]
        assert same_bits(nodes["bmin"][k], tri.min(axis=0)) and same_bits(nodes["bmax"][k], tri.max(axis=0))
