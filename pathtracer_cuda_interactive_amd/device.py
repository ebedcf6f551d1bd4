"""Device library bindings (libpt_hip.so): the C ABI of include/pt_api.h.

There is NO CPU fallback: if the HIP library is missing or no GPU is present the
calls raise (PT_ERR_NO_DEVICE) — the product never routes through the oracle.
"""
import ctypes as C
import os

import numpy as np

from . import _build
from .ctypes_defs import (PT_MOTION_GEOMETRY_CURRENT, PT_MOTION_GEOMETRY_PREVIOUS, PT_OK, PT_QUERY_ANY, PT_QUERY_CLOSEST, PT_SHAPE_SPHERE,
                          PT_TRAVERSAL_DEFAULT, PT_UPDATE_GEOMETRY, PT_UPDATE_SHADING, QUERY_ARGTYPES, SPARSE_ARGTYPES, PtAdaptiveParams, PtBvhNode, PtCounters, PtDenoiseParams, PtError,
                          PtGradientParams, PtGuideBuffers, PtLight, PtMaterial, PtMesh, PtMotionParams, PtRenderParams, PtSceneDesc, PtShape,
                          PtTemporalIo, PtTemporalParams, PtTransform, PtVdenoiseParams)
from .host import NODE_DTYPE  # noqa: F401  (one definition; callers also read it from here)

_lib = None

EXPORTS = [
    "pt_api_version", "pt_last_error", "pt_scene_create", "pt_scene_destroy", "pt_render", "pt_render_async",
    "pt_render_accumulate", "pt_get_counters", "pt_scene_set_option", "pt_scene_get_info", "pt_debug_math",
    "pt_debug_intersect", "pt_debug_math_host", "pt_bvh_build_device", "pt_bvh_build_sweep", "pt_get_frame_times", "pt_bvh_build_sweep_device",
    "pt_debug_exact_math", "pt_render_adaptive", "pt_render_aov", "pt_denoise", "pt_denoise_host", "pt_scene_update",
    "pt_render_guides", "pt_temporal_accumulate", "pt_temporal_accumulate_host",
    "pt_temporal_accumulate_moments", "pt_temporal_accumulate_moments_host", "pt_denoise_variance", "pt_denoise_variance_host",
    "pt_temporal_gradient", "pt_temporal_gradient_host", "pt_temporal_accumulate_adaptive", "pt_temporal_accumulate_adaptive_host",
    "pt_render_pixels", "pt_gradient_pixels", "pt_gradient_pixels_host", "pt_temporal_gradient_sparse", "pt_temporal_gradient_sparse_host",
    "pt_scene_set_groups", "pt_scene_transform", "pt_transform_geometry_host", "pt_transform_sphere_host",
    "pt_trace_rays", "pt_render_guides_async", "pt_scene_rebuild",
]


def lib():
    global _lib
    if _lib is None:
        path = _build.HIP_LIB
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: build it with `python -m pathtracer_cuda_interactive_amd._build` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        L = C.CDLL(path)
        vp, fp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)
        L.pt_api_version.restype = C.c_int
        L.pt_last_error.restype = C.c_char_p
        L.pt_scene_create.argtypes = [C.POINTER(PtSceneDesc), C.POINTER(vp)]
        L.pt_scene_destroy.argtypes = [vp]
        L.pt_scene_update.argtypes = [vp, C.POINTER(PtSceneDesc), C.c_int]
        L.pt_scene_rebuild.argtypes = [vp, C.c_int]
        L.pt_scene_set_groups.argtypes = [vp, ip, C.c_int32]
        L.pt_scene_transform.argtypes = [vp, C.POINTER(PtTransform), C.c_int32]
        L.pt_transform_geometry_host.argtypes = [C.POINTER(PtTransform), C.c_int32, vp, vp, vp, vp]
        L.pt_transform_sphere_host.argtypes = [C.POINTER(PtTransform), fp, C.c_float, fp, fp]
        L.pt_render.argtypes = [vp, C.POINTER(PtRenderParams), vp, C.c_int]
        L.pt_render_async.argtypes = [vp, C.POINTER(PtRenderParams), vp, vp]
        L.pt_render_accumulate.argtypes = [vp, C.POINTER(PtRenderParams), vp, vp]
        L.pt_render_adaptive.argtypes = [vp, C.POINTER(PtRenderParams), C.POINTER(PtAdaptiveParams), vp, vp, vp, C.c_int]
        L.pt_render_aov.argtypes = [vp, C.POINTER(PtRenderParams), vp, vp, vp, vp, C.c_int]
        L.pt_denoise.argtypes = [vp, C.POINTER(PtDenoiseParams), vp, vp, vp, vp, vp, C.c_int, vp]
        L.pt_denoise_host.argtypes = [C.POINTER(PtDenoiseParams), vp, vp, vp, vp, vp]
        L.pt_render_guides.argtypes = [vp, C.POINTER(PtRenderParams), C.POINTER(PtMotionParams), C.POINTER(PtGuideBuffers), C.c_int]
        L.pt_temporal_accumulate.argtypes = [vp, C.POINTER(PtTemporalParams)] + [vp] * 10 + [C.c_int, vp]
        L.pt_temporal_accumulate_host.argtypes = [C.POINTER(PtTemporalParams)] + [vp] * 10
        L.pt_temporal_accumulate_moments.argtypes = [vp, C.POINTER(PtTemporalParams), C.c_float, C.POINTER(PtTemporalIo), C.c_int, vp]
        L.pt_temporal_accumulate_moments_host.argtypes = [C.POINTER(PtTemporalParams), C.c_float, C.POINTER(PtTemporalIo)]
        L.pt_denoise_variance.argtypes = [vp, C.POINTER(PtVdenoiseParams)] + [vp] * 8 + [C.c_int, vp]
        L.pt_denoise_variance_host.argtypes = [C.POINTER(PtVdenoiseParams)] + [vp] * 8
        L.pt_temporal_gradient.argtypes = [vp, C.POINTER(PtGradientParams), vp, vp, vp, C.c_int, vp]
        L.pt_temporal_gradient_host.argtypes = [C.POINTER(PtGradientParams), vp, vp, vp]
        for name, argtypes in list(SPARSE_ARGTYPES.items()) + list(QUERY_ARGTYPES.items()):
            getattr(L, name).argtypes = argtypes
        L.pt_temporal_accumulate_adaptive.argtypes = [vp, C.POINTER(PtTemporalParams), C.c_float, C.POINTER(PtTemporalIo), vp, C.c_int32,
                                                      C.c_int, vp]
        L.pt_temporal_accumulate_adaptive_host.argtypes = [C.POINTER(PtTemporalParams), C.c_float, C.POINTER(PtTemporalIo), vp, C.c_int32]
        L.pt_get_counters.argtypes = [vp, C.POINTER(PtCounters)]
        L.pt_get_frame_times.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.pt_scene_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
        L.pt_scene_get_info.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
        L.pt_debug_math.argtypes = [C.c_int, fp, fp, fp, fp, C.c_int]
        L.pt_debug_intersect.argtypes = [vp, fp, C.c_int, C.c_int, fp, ip]
        L.pt_debug_math_host.argtypes = [C.c_int, fp, fp, fp, fp, C.c_int]
        L.pt_debug_exact_math.argtypes = [C.c_int, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]
        L.pt_bvh_build_device.argtypes = [C.POINTER(PtSceneDesc), C.c_int, C.POINTER(PtBvhNode), ip, ip, C.POINTER(C.c_double)]
        L.pt_bvh_build_sweep.argtypes = [C.POINTER(PtSceneDesc), C.POINTER(PtBvhNode), ip, ip, C.POINTER(C.c_double)]
        L.pt_bvh_build_sweep_device.argtypes = [C.POINTER(PtSceneDesc), C.POINTER(PtBvhNode), ip, ip, C.POINTER(C.c_double)]
        _lib = L
    return _lib


def _check(rc):
    if rc != PT_OK:
        raise PtError(rc, lib().pt_last_error().decode())


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class DeviceScene:
    """A scene resident on the current HIP device (pt_scene*)."""

    def __init__(self, desc):
        h = C.c_void_p()
        _check(lib().pt_scene_create(C.byref(desc), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().pt_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, desc, geometry=True, shading=False):
        """pt_scene_update: new geometry (shapes and meshes of `desc`) and / or new shading values (materials, lights, background)
        on this handle; both trees keep their topology and are refitted on the device.  Blocking.  `desc` must have the
        shape count the handle was created with (see edited_desc); its nodes are ignored."""
        flags = (PT_UPDATE_GEOMETRY if geometry else 0) | (PT_UPDATE_SHADING if shading else 0)
        _check(lib().pt_scene_update(self._h, C.byref(desc), flags))

    def set_groups(self, ids, num_groups):
        """pt_scene_set_groups: the group of every shape (ids [num_shapes] int32, -1 = never moves) for transform."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        _check(lib().pt_scene_set_groups(self._h, ids.ctypes.data_as(C.POINTER(C.c_int32)), int(num_groups)))

    def transform(self, matrices):
        """pt_scene_transform: the rest geometry under one row-major 3x4 matrix per group (matrices [num_groups, 3, 4]); the
        records are made on the device and both trees refitted.  Absolute, not cumulative.  Blocking."""
        M = _matrices(matrices)
        _check(lib().pt_scene_transform(self._h, M.ctypes.data_as(C.POINTER(PtTransform)), M.shape[0]))

    def rebuild(self):
        """pt_scene_rebuild: a fresh internal tree over the leaf boxes the handle holds now, adopted where it visits at least 10 %
        fewer nodes than the caller's tree; records, groups, options and frame slots carry on.  Blocking.  Returns whether the
        tree was adopted (info "rebuild_adopted")."""
        _check(lib().pt_scene_rebuild(self._h, 0))
        return bool(self.info("rebuild_adopted"))

    def set_option(self, key, value):
        _check(lib().pt_scene_set_option(self._h, key.encode(), int(value)))

    def info(self, key):
        v = C.c_int64()
        _check(lib().pt_scene_get_info(self._h, key.encode(), C.byref(v)))
        return v.value

    def render(self, params, traversal=None):
        """Blocking render into a new host array [rows, W, 3] float32."""
        p = params.copy()
        if traversal is not None:
            p.traversal = traversal
        img = np.empty((p.num_rows(), p.width, 3), dtype=np.float32)
        _check(lib().pt_render(self._h, C.byref(p), img.ctypes.data_as(C.c_void_p), 0))
        return img

    def render_into(self, params, dev_ptr, stream=None, traversal=None):
        """Asynchronous render into device memory (e.g. a torch tensor's data_ptr()) on a HIP stream."""
        p = params.copy()
        if traversal is not None:
            p.traversal = traversal
        _check(lib().pt_render_async(self._h, C.byref(p), C.c_void_p(dev_ptr), C.c_void_p(stream or 0)))

    @staticmethod
    def adaptive_params(max_error, batch_spp=0, max_spp=0, p_value=0.05, min_luminance=0.01):
        return PtAdaptiveParams(int(batch_spp), int(max_spp), float(max_error), float(p_value), float(min_luminance))

    def render_adaptive(self, params, max_error, batch_spp=0, max_spp=0, p_value=0.05, min_luminance=0.01, traversal=None):
        """Blocking adaptive render (pt_render_adaptive): returns host arrays (image [rows, W, 3] float32,
        spp_map [rows, W] int32, err_map [rows, W] float32)."""
        p = params.copy()
        if traversal is not None:
            p.traversal = traversal
        a = self.adaptive_params(max_error, batch_spp, max_spp, p_value, min_luminance)
        img = np.empty((p.num_rows(), p.width, 3), dtype=np.float32)
        spp = np.empty((p.num_rows(), p.width), dtype=np.int32)
        err = np.empty((p.num_rows(), p.width), dtype=np.float32)
        _check(lib().pt_render_adaptive(self._h, C.byref(p), C.byref(a), img.ctypes.data_as(C.c_void_p),
                                        spp.ctypes.data_as(C.c_void_p), err.ctypes.data_as(C.c_void_p), 0))
        return img, spp, err

    def render_adaptive_into(self, params, fb_ptr, spp_ptr, err_ptr, max_error, batch_spp=0, max_spp=0, p_value=0.05,
                             min_luminance=0.01, traversal=None):
        """Adaptive render into device memory (fb [rows, W, 3] float32, spp_map [rows, W] int32, err_map [rows, W] float32;
        spp_ptr / err_ptr may be 0).  Blocking: it runs on the default stream and returns when the frame is done."""
        p = params.copy()
        if traversal is not None:
            p.traversal = traversal
        a = self.adaptive_params(max_error, batch_spp, max_spp, p_value, min_luminance)
        _check(lib().pt_render_adaptive(self._h, C.byref(p), C.byref(a), C.c_void_p(fb_ptr), C.c_void_p(spp_ptr or 0),
                                        C.c_void_p(err_ptr or 0), 1))

    def render_aov(self, params, traversal=None, albedo=True, normal=True, depth=True, prim=True):
        """Guide buffers of the first hit (pt_render_aov), one ray through every selected pixel's centre: a dict of host arrays
        "albedo" / "normal" [rows, W, 3] float32, "depth" [rows, W] float32, "prim" [rows, W] int32 (those asked for)."""
        p = params.copy()
        if traversal is not None:
            p.traversal = traversal
        rows, W = p.num_rows(), p.width
        out = {}
        if albedo:
            out["albedo"] = np.empty((rows, W, 3), dtype=np.float32)
        if normal:
            out["normal"] = np.empty((rows, W, 3), dtype=np.float32)
        if depth:
            out["depth"] = np.empty((rows, W), dtype=np.float32)
        if prim:
            out["prim"] = np.empty((rows, W), dtype=np.int32)
        ptr = [out[k].ctypes.data_as(C.c_void_p) if k in out else None for k in ("albedo", "normal", "depth", "prim")]
        _check(lib().pt_render_aov(self._h, C.byref(p), ptr[0], ptr[1], ptr[2], ptr[3], 0))
        return out

    def render_aov_into(self, params, albedo_ptr=0, normal_ptr=0, depth_ptr=0, prim_ptr=0, traversal=None):
        """pt_render_aov into device memory (albedo / normal [rows, W, 3] float32, depth [rows, W] float32, prim [rows, W]
        int32; a pointer of 0 skips that buffer).  Blocking: it runs on the default stream and returns when the buffers are written."""
        p = params.copy()
        if traversal is not None:
            p.traversal = traversal
        _check(lib().pt_render_aov(self._h, C.byref(p), C.c_void_p(albedo_ptr or 0), C.c_void_p(normal_ptr or 0),
                                   C.c_void_p(depth_ptr or 0), C.c_void_p(prim_ptr or 0), 1))

    def denoise(self, color, albedo, normal, depth, **kw):
        """pt_denoise on host arrays (color, albedo, normal [H, W, 3], depth [H, W], float32): the filtered frame as a new
        array.  Keywords: the fields of pt_denoise_params (denoise_params)."""
        color, albedo, normal, depth, d = _denoise_args(color, albedo, normal, depth, kw)
        out = np.empty_like(color)
        _check(lib().pt_denoise(self._h, C.byref(d), *_ptrs([color, albedo, normal, depth, out]), 0, None))
        return out

    def denoise_into(self, width, height, color_ptr, albedo_ptr, normal_ptr, depth_ptr, out_ptr, stream=None, **kw):
        """pt_denoise on device memory, enqueued on a HIP stream without a host sync (out_ptr may be color_ptr)."""
        d = denoise_params(width, height, **kw)
        _check(lib().pt_denoise(self._h, C.byref(d), C.c_void_p(color_ptr), C.c_void_p(albedo_ptr), C.c_void_p(normal_ptr),
                                C.c_void_p(depth_ptr), C.c_void_p(out_ptr), 1, C.c_void_p(stream or 0)))

    def render_guides(self, params, prev_camera, previous_geometry=False, traversal=None, albedo=True, normal=True, depth=True,
                      prim=True, motion=True, prev_depth=True):
        """pt_render_guides: render_aov's buffers plus "motion" [rows, W, 2] and "prev_depth" [rows, W] float32 (those asked
        for), as a dict of host arrays.  prev_camera: the previous frame's PtRenderParams (its camera is read) or a
        PtMotionParams; previous_geometry: the surface points are followed into the records from before the last update."""
        p = params.copy()
        if traversal is not None:
            p.traversal = traversal
        rows, W = p.num_rows(), p.width
        shapes = {"albedo": ((rows, W, 3), np.float32), "normal": ((rows, W, 3), np.float32), "depth": ((rows, W), np.float32),
                  "prim": ((rows, W), np.int32), "motion": ((rows, W, 2), np.float32), "prev_depth": ((rows, W), np.float32)}
        want = {"albedo": albedo, "normal": normal, "depth": depth, "prim": prim, "motion": motion, "prev_depth": prev_depth}
        out = {k: np.empty(*shapes[k]) for k in shapes if want[k]}
        g = PtGuideBuffers(*(out[k].ctypes.data if k in out else None for k in shapes))
        m = motion_params(prev_camera, previous_geometry)
        _check(lib().pt_render_guides(self._h, C.byref(p), C.byref(m), C.byref(g), 0))
        return out

    def render_guides_into(self, params, prev_camera, previous_geometry=False, albedo_ptr=0, normal_ptr=0, depth_ptr=0, prim_ptr=0,
                           motion_ptr=0, prev_depth_ptr=0, traversal=None):
        """pt_render_guides into device memory (a pointer of 0 skips that buffer).  Blocking, on the default stream."""
        p = params.copy()
        if traversal is not None:
            p.traversal = traversal
        g = PtGuideBuffers(*(ptr or None for ptr in (albedo_ptr, normal_ptr, depth_ptr, prim_ptr, motion_ptr, prev_depth_ptr)))
        m = motion_params(prev_camera, previous_geometry)
        _check(lib().pt_render_guides(self._h, C.byref(p), C.byref(m), C.byref(g), 1))

    def render_guides_async_into(self, params, prev_camera=None, previous_geometry=False, albedo_ptr=0, normal_ptr=0, depth_ptr=0,
                                 prim_ptr=0, motion_ptr=0, prev_depth_ptr=0, stream=None, traversal=None):
        """pt_render_guides_async: render_guides_into's buffers and bits, enqueued on a HIP stream without a host sync.
        prev_camera None: pt_render_aov's four buffers only (no motion parameters are passed)."""
        p = params.copy()
        if traversal is not None:
            p.traversal = traversal
        g = PtGuideBuffers(*(ptr or None for ptr in (albedo_ptr, normal_ptr, depth_ptr, prim_ptr, motion_ptr, prev_depth_ptr)))
        m = C.byref(motion_params(prev_camera, previous_geometry)) if prev_camera is not None else None
        _check(lib().pt_render_guides_async(self._h, C.byref(p), m, C.byref(g), C.c_void_p(stream or 0)))

    def trace_rays(self, rays, mode=PT_QUERY_CLOSEST, traversal=PT_TRAVERSAL_DEFAULT):
        """pt_trace_rays on a host array of rays [n, 8] ({org, dir, tnear, tfar}).  Blocking.  PT_QUERY_CLOSEST: (tuv [n, 3]
        float32, prim [n] int32), what intersect() returns; PT_QUERY_ANY: hit [n] int32, 1 where the ray hits anything."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = rays.shape[0]
        prim = np.zeros(n, dtype=np.int32)
        tuv = np.zeros((n, 3), dtype=np.float32) if mode == PT_QUERY_CLOSEST else None
        _check(lib().pt_trace_rays(self._h, *_ptrs([rays]), n, int(mode), int(traversal), *_ptrs([tuv, prim]), 0, None))
        return (tuv, prim) if mode == PT_QUERY_CLOSEST else prim

    def trace_rays_into(self, rays_ptr, n, tuv_ptr, prim_ptr, mode=PT_QUERY_CLOSEST, traversal=PT_TRAVERSAL_DEFAULT, stream=None):
        """pt_trace_rays on device memory (rays_ptr: [n, 8] float32, tuv_ptr: [n, 3] float32 or 0 with PT_QUERY_ANY, prim_ptr: [n]
        int32), enqueued on a HIP stream without a host sync.  The rays must stay valid until the stream has passed the call."""
        _check(lib().pt_trace_rays(self._h, C.c_void_p(rays_ptr or 0), int(n), int(mode), int(traversal), C.c_void_p(tuv_ptr or 0),
                                   C.c_void_p(prim_ptr or 0), 1, C.c_void_p(stream or 0)))

    def temporal_accumulate(self, color, normal, motion, prev_depth, history=None, **kw):
        """pt_temporal_accumulate on host arrays: (out_color [H, W, 3], out_len [H, W]) as new arrays.  history: None or
        (hist_color, hist_normal, hist_depth, hist_len) of the previous frame.  Keywords: the fields of pt_temporal_params."""
        args, t = _temporal_args(color, normal, motion, prev_depth, history, kw)
        out_color, out_len = np.empty_like(args[0]), np.empty_like(args[3])
        _check(lib().pt_temporal_accumulate(self._h, C.byref(t), *_ptrs(args + [out_color, out_len]), 0, None))
        return out_color, out_len

    def temporal_accumulate_into(self, width, height, color_ptr, normal_ptr, motion_ptr, prev_depth_ptr, hist_ptrs, out_color_ptr,
                                 out_len_ptr, stream=None, **kw):
        """pt_temporal_accumulate on device memory, enqueued on a HIP stream without a host sync.  hist_ptrs: None or the four
        pointers (hist_color, hist_normal, hist_depth, hist_len); out_color_ptr may be color_ptr."""
        t = temporal_params(width, height, **kw)
        hist = [C.c_void_p(q) for q in hist_ptrs] if hist_ptrs else [None] * 4
        _check(lib().pt_temporal_accumulate(self._h, C.byref(t), C.c_void_p(color_ptr), C.c_void_p(normal_ptr), C.c_void_p(motion_ptr),
                                            C.c_void_p(prev_depth_ptr), *hist, C.c_void_p(out_color_ptr), C.c_void_p(out_len_ptr), 1,
                                            C.c_void_p(stream or 0)))

    def temporal_accumulate_moments(self, color, albedo, normal, motion, prev_depth, history=None, albedo_floor=0.0, **kw):
        """pt_temporal_accumulate_moments on host arrays: (out_color [H, W, 3], out_len [H, W], out_moments [H, W, 2]) as new
        arrays.  history: None or (hist_color, hist_normal, hist_depth, hist_len, hist_moments) of the previous frame.
        Keywords: the fields of pt_temporal_params."""
        args, t = _temporal_moments_args(color, albedo, normal, motion, prev_depth, history, kw)
        outs = [np.empty_like(args[0]), np.empty_like(args[4]), np.empty_like(args[3])]
        io = PtTemporalIo(*_ptrs(args + outs))
        _check(lib().pt_temporal_accumulate_moments(self._h, C.byref(t), float(albedo_floor), C.byref(io), 0, None))
        return tuple(outs)

    def temporal_accumulate_moments_into(self, width, height, color_ptr, albedo_ptr, normal_ptr, motion_ptr, prev_depth_ptr, hist_ptrs,
                                         out_color_ptr, out_len_ptr, out_moments_ptr, stream=None, albedo_floor=0.0, **kw):
        """pt_temporal_accumulate_moments on device memory, enqueued on a HIP stream without a host sync.  hist_ptrs: None or the
        five pointers (hist_color, hist_normal, hist_depth, hist_len, hist_moments); out_color_ptr may be color_ptr."""
        t = temporal_params(width, height, **kw)
        io = PtTemporalIo(color_ptr, albedo_ptr, normal_ptr, motion_ptr, prev_depth_ptr, *(hist_ptrs if hist_ptrs else [None] * 5),
                          out_color_ptr, out_len_ptr, out_moments_ptr)
        _check(lib().pt_temporal_accumulate_moments(self._h, C.byref(t), float(albedo_floor), C.byref(io), 1, C.c_void_p(stream or 0)))

    def temporal_gradient(self, prev_color, resampled, **kw):
        """pt_temporal_gradient on host arrays (prev_color [H, W, 3]: the previous frame's noisy render; resampled [TH, W, 3]: the
        render of gradient_rows_params(previous parameters, stride) on the current scene): lambda [TH, TW] as a new array.
        Keywords: the fields of pt_gradient_params (gradient_params)."""
        prev_color, resampled, g, shape = _gradient_args(prev_color, resampled, kw)
        out = np.empty(shape, dtype=np.float32)
        _check(lib().pt_temporal_gradient(self._h, C.byref(g), *_ptrs([prev_color, resampled, out]), 0, None))
        return out

    def temporal_gradient_into(self, width, height, prev_color_ptr, resampled_ptr, lambda_ptr, stream=None, **kw):
        """pt_temporal_gradient on device memory, enqueued on a HIP stream without a host sync (lambda_ptr: [TH, TW] float32, the
        shape gradient_grid gives)."""
        g = gradient_params(width, height, **kw)
        _check(lib().pt_temporal_gradient(self._h, C.byref(g), C.c_void_p(prev_color_ptr), C.c_void_p(resampled_ptr),
                                          C.c_void_p(lambda_ptr), 1, C.c_void_p(stream or 0)))

    def render_pixels(self, params, pixels, traversal=None):
        """pt_render_pixels on a host list of pixel indices (j * width + i, any order, duplicates allowed): their colours as a new
        [n, 3] float32 array, each the bits a full render(params) gives that pixel.  Blocking."""
        p = params.copy()
        if traversal is not None:
            p.traversal = traversal
        pixels = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1)
        out = np.empty((pixels.size, 3), dtype=np.float32)
        _check(lib().pt_render_pixels(self._h, C.byref(p), *_ptrs([pixels]), pixels.size, *_ptrs([out]), 0, None))
        return out

    def render_pixels_into(self, params, pixels_ptr, n, out_ptr, stream=None, traversal=None):
        """pt_render_pixels on device memory (pixels_ptr: n int32, out_ptr: [n, 3] float32), enqueued on a HIP stream without a
        host sync.  The list must stay valid until the stream has passed the call."""
        p = params.copy()
        if traversal is not None:
            p.traversal = traversal
        _check(lib().pt_render_pixels(self._h, C.byref(p), C.c_void_p(pixels_ptr or 0), int(n), C.c_void_p(out_ptr or 0), 1,
                                      C.c_void_p(stream or 0)))

    def gradient_pixels(self, width, height, seed, **kw):
        """pt_gradient_pixels through the handle's staging memory: the list [TH * TW] int32 as a new host array (the bits of
        gradient_pixels_host).  Keywords: the fields of pt_gradient_params."""
        g = gradient_params(width, height, **kw)
        _, TH, TW = gradient_grid(width, height, g.stride)
        out = np.empty(TH * TW, dtype=np.int32)
        _check(lib().pt_gradient_pixels(self._h, C.byref(g), int(seed) & 0xffffffff, *_ptrs([out]), 0, None))
        return out

    def gradient_pixels_into(self, width, height, seed, pixels_ptr, stream=None, **kw):
        """pt_gradient_pixels into device memory ([TH * TW] int32, the grid gradient_grid gives), enqueued on a HIP stream
        without a host sync."""
        g = gradient_params(width, height, **kw)
        _check(lib().pt_gradient_pixels(self._h, C.byref(g), int(seed) & 0xffffffff, C.c_void_p(pixels_ptr), 1, C.c_void_p(stream or 0)))

    def temporal_gradient_sparse(self, prev_color, pixels, resampled, **kw):
        """pt_temporal_gradient_sparse on host arrays (prev_color [H, W, 3]; pixels [TH * TW] int32 of gradient_pixels; resampled
        [TH * TW, 3]: render_pixels of the previous parameters and that list on the current scene): lambda [TH, TW] as a new array."""
        prev_color, pixels, resampled, g, shape = _gradient_sparse_args(prev_color, pixels, resampled, kw)
        out = np.empty(shape, dtype=np.float32)
        _check(lib().pt_temporal_gradient_sparse(self._h, C.byref(g), *_ptrs([prev_color, pixels, resampled, out]), 0, None))
        return out

    def temporal_gradient_sparse_into(self, width, height, prev_color_ptr, pixels_ptr, resampled_ptr, lambda_ptr, stream=None, **kw):
        """pt_temporal_gradient_sparse on device memory, enqueued on a HIP stream without a host sync."""
        g = gradient_params(width, height, **kw)
        _check(lib().pt_temporal_gradient_sparse(self._h, C.byref(g), C.c_void_p(prev_color_ptr), C.c_void_p(pixels_ptr),
                                                 C.c_void_p(resampled_ptr), C.c_void_p(lambda_ptr), 1, C.c_void_p(stream or 0)))

    def temporal_accumulate_adaptive(self, color, albedo, normal, motion, prev_depth, lam, history=None, stride=0, albedo_floor=0.0,
                                     **kw):
        """pt_temporal_accumulate_adaptive on host arrays: temporal_accumulate_moments with the map `lam` [TH, TW] of
        temporal_gradient at `stride`.  Returns (out_color, out_len, out_moments) as new arrays."""
        args, t = _temporal_moments_args(color, albedo, normal, motion, prev_depth, history, kw)
        lam = _lambda_arg(lam, args[4].shape, stride)
        outs = [np.empty_like(args[0]), np.empty_like(args[4]), np.empty_like(args[3])]
        io = PtTemporalIo(*_ptrs(args + outs))
        _check(lib().pt_temporal_accumulate_adaptive(self._h, C.byref(t), float(albedo_floor), C.byref(io), *_ptrs([lam]), int(stride),
                                                     0, None))
        return tuple(outs)

    def temporal_accumulate_adaptive_into(self, width, height, color_ptr, albedo_ptr, normal_ptr, motion_ptr, prev_depth_ptr, hist_ptrs,
                                          out_color_ptr, out_len_ptr, out_moments_ptr, lambda_ptr, stride=0, stream=None,
                                          albedo_floor=0.0, **kw):
        """pt_temporal_accumulate_adaptive on device memory, enqueued on a HIP stream without a host sync: the arguments of
        temporal_accumulate_moments_into, and the map temporal_gradient_into wrote with the same stride."""
        t = temporal_params(width, height, **kw)
        io = PtTemporalIo(color_ptr, albedo_ptr, normal_ptr, motion_ptr, prev_depth_ptr, *(hist_ptrs if hist_ptrs else [None] * 5),
                          out_color_ptr, out_len_ptr, out_moments_ptr)
        _check(lib().pt_temporal_accumulate_adaptive(self._h, C.byref(t), float(albedo_floor), C.byref(io), C.c_void_p(lambda_ptr),
                                                     int(stride), 1, C.c_void_p(stream or 0)))

    def denoise_variance(self, color, albedo, normal, depth, moments, hist_len, variance=False, **kw):
        """pt_denoise_variance on host arrays (moments [H, W, 2] and hist_len [H, W] from temporal_accumulate_moments): the
        filtered frame as a new array, or (frame, variance [H, W]) with variance=True.  Keywords: the fields of
        pt_vdenoise_params (vdenoise_params)."""
        arrays, d = _vdenoise_args(color, albedo, normal, depth, moments, hist_len, kw)
        out = np.empty_like(arrays[0])
        var = np.empty_like(arrays[3]) if variance else None
        _check(lib().pt_denoise_variance(self._h, C.byref(d), *_ptrs(arrays + [out, var]), 0, None))
        return (out, var) if variance else out

    def denoise_variance_into(self, width, height, color_ptr, albedo_ptr, normal_ptr, depth_ptr, moments_ptr, hist_len_ptr, out_ptr,
                              out_variance_ptr=0, stream=None, **kw):
        """pt_denoise_variance on device memory, enqueued on a HIP stream without a host sync (out_ptr may be color_ptr;
        out_variance_ptr 0 = not wanted)."""
        d = vdenoise_params(width, height, **kw)
        _check(lib().pt_denoise_variance(self._h, C.byref(d), *(C.c_void_p(q) for q in (color_ptr, albedo_ptr, normal_ptr, depth_ptr,
                                                                                      moments_ptr, hist_len_ptr, out_ptr)),
                                         C.c_void_p(out_variance_ptr or 0), 1, C.c_void_p(stream or 0)))

    def accumulate_into(self, params, dev_ptr, stream=None):
        _check(lib().pt_render_accumulate(self._h, C.byref(params), C.c_void_p(dev_ptr), C.c_void_p(stream or 0)))

    def counters(self):
        c = PtCounters()
        _check(lib().pt_get_counters(self._h, C.byref(c)))
        return c

    def frame_times(self, max_frames):
        """(kernel_ms[], resolve_ms[]) of the last render calls, oldest first (option "timing_frames" sets how many are kept)."""
        k = (C.c_double * max(max_frames, 1))()
        r = (C.c_double * max(max_frames, 1))()
        n = C.c_int()
        _check(lib().pt_get_frame_times(self._h, int(max_frames), k, r, C.byref(n)))
        return np.array(k[: n.value]), np.array(r[: n.value])

    def intersect(self, rays, traversal=PT_TRAVERSAL_DEFAULT):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        tuv = np.zeros((rays.shape[0], 3), dtype=np.float32)
        prim = np.zeros(rays.shape[0], dtype=np.int32)
        _check(lib().pt_debug_intersect(self._h, _fp(rays), rays.shape[0], traversal, _fp(tuv),
                                        prim.ctypes.data_as(C.POINTER(C.c_int32))))
        return tuv, prim


def _ptrs(arrays):
    """The c_void_p of each array of a list; None stays None (a null pointer)."""
    return [a.ctypes.data_as(C.c_void_p) if a is not None else None for a in arrays]


def _out_like(out, like, what):
    """`out` if given, else a new array like `like`; it must be a contiguous float32 array of `like`'s shape."""
    if out is None:
        return np.empty_like(like)
    if out.dtype != np.float32 or out.shape != like.shape or not out.flags.c_contiguous:
        raise ValueError(what + " must be a contiguous [H, W, 3] float32 array")
    return out


def denoise_params(width, height, iterations=0, normal_power_log2=7, sigma_z=0.0, sigma_c=0.0, scale=0.0, albedo_floor=0.0):
    """pt_denoise_params; 0 = the library's default (5 iterations, sigma_z 0.05, no colour term, scale 1, albedo_floor 0.01)."""
    return PtDenoiseParams(int(width), int(height), int(iterations), int(normal_power_log2), float(sigma_z), float(sigma_c),
                           float(scale), float(albedo_floor))


def _denoise_args(color, albedo, normal, depth, kw):
    color, albedo, normal = (np.ascontiguousarray(a, dtype=np.float32) for a in (color, albedo, normal))
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    H, W = depth.shape
    if not (color.shape == albedo.shape == normal.shape == (H, W, 3)):
        raise ValueError("denoise: color, albedo, normal must be [H, W, 3] and depth [H, W]")
    return color, albedo, normal, depth, denoise_params(W, H, **kw)


def denoise_host(color, albedo, normal, depth, out=None, **kw):
    """pt_denoise_host: the filter of pt_denoise run by the host half of the library (no GPU needed).  out: an [H, W, 3]
    float32 array to write (it may be `color` itself); default a new one."""
    color, albedo, normal, depth, d = _denoise_args(color, albedo, normal, depth, kw)
    out = _out_like(out, color, "denoise_host: out")
    _check(lib().pt_denoise_host(C.byref(d), *_ptrs([color, albedo, normal, depth, out])))
    return out


def motion_params(prev_camera, previous_geometry=False):
    """pt_motion_params from the previous frame's PtRenderParams (or a PtMotionParams, whose camera is taken over)."""
    m = PtMotionParams()
    for f in ("origin", "top_left", "horizontal", "vertical"):
        src = getattr(prev_camera, "prev_cam_" + f) if isinstance(prev_camera, PtMotionParams) else getattr(prev_camera, "cam_" + f)
        getattr(m, "prev_cam_" + f)[:] = src[:]
    m.geometry = PT_MOTION_GEOMETRY_PREVIOUS if previous_geometry else PT_MOTION_GEOMETRY_CURRENT
    return m


def temporal_params(width, height, max_history=0, sigma_z=0.0, normal_min=0.9, scale=0.0):
    """pt_temporal_params; 0 = the library's default (32 frames, sigma_z 0.1, scale 1); normal_min is used as given."""
    return PtTemporalParams(int(width), int(height), int(max_history), float(sigma_z), float(normal_min), float(scale))


def _temporal_args(color, normal, motion, prev_depth, history, kw):
    color, normal, motion, prev_depth = (np.ascontiguousarray(a, dtype=np.float32) for a in (color, normal, motion, prev_depth))
    H, W = prev_depth.shape
    if not (color.shape == normal.shape == (H, W, 3) and motion.shape == (H, W, 2)):
        raise ValueError("temporal_accumulate: color, normal must be [H, W, 3], motion [H, W, 2] and prev_depth [H, W]")
    hist = [None] * 4
    if history is not None:
        hist = [np.ascontiguousarray(a, dtype=np.float32) for a in history]
        if [a.shape for a in hist] != [(H, W, 3), (H, W, 3), (H, W), (H, W)]:
            raise ValueError("temporal_accumulate: history must be (color [H, W, 3], normal [H, W, 3], depth [H, W], len [H, W])")
    return [color, normal, motion, prev_depth] + hist, temporal_params(W, H, **kw)


def temporal_accumulate_host(color, normal, motion, prev_depth, history=None, out_color=None, **kw):
    """pt_temporal_accumulate_host: the rule of pt_temporal_accumulate run by the host half of the library (no GPU needed).
    Returns (out_color, out_len); out_color: an [H, W, 3] float32 array to write (it may be `color` itself), default a new one."""
    args, t = _temporal_args(color, normal, motion, prev_depth, history, kw)
    out_color = _out_like(out_color, args[0], "temporal_accumulate_host: out_color")
    out_len = np.empty_like(args[3])
    _check(lib().pt_temporal_accumulate_host(C.byref(t), *_ptrs(args + [out_color, out_len])))
    return out_color, out_len


def _temporal_moments_args(color, albedo, normal, motion, prev_depth, history, kw):
    if history is not None and len(history) != 5:
        raise ValueError("temporal_accumulate_moments: history must be (color, normal, depth, len, moments [H, W, 2])")
    (color, normal, motion, prev_depth, *hist), t = _temporal_args(color, normal, motion, prev_depth,
                                                                   None if history is None else list(history)[:4], kw)
    albedo = np.ascontiguousarray(albedo, dtype=np.float32)
    if albedo.shape != color.shape:
        raise ValueError("temporal_accumulate_moments: albedo must be [H, W, 3]")
    hist_moments = None
    if history is not None:
        hist_moments = np.ascontiguousarray(history[4], dtype=np.float32)
        if hist_moments.shape != motion.shape:
            raise ValueError("temporal_accumulate_moments: the history's moments must be [H, W, 2]")
    return [color, albedo, normal, motion, prev_depth, *hist, hist_moments], t


def temporal_accumulate_moments_host(color, albedo, normal, motion, prev_depth, history=None, out_color=None, albedo_floor=0.0, **kw):
    """pt_temporal_accumulate_moments_host: the rule of pt_temporal_accumulate_moments run by the host half of the library (no
    GPU needed).  Returns (out_color, out_len, out_moments); out_color: an [H, W, 3] float32 array to write (it may be `color`
    itself), default a new one."""
    args, t = _temporal_moments_args(color, albedo, normal, motion, prev_depth, history, kw)
    out_color = _out_like(out_color, args[0], "temporal_accumulate_moments_host: out_color")
    outs = [out_color, np.empty_like(args[4]), np.empty_like(args[3])]
    io = PtTemporalIo(*_ptrs(args + outs))
    _check(lib().pt_temporal_accumulate_moments_host(C.byref(t), float(albedo_floor), C.byref(io)))
    return tuple(outs)


def gradient_params(width, height, stride=0, iterations=0, gain=0.0, norm_floor=0.0):
    """pt_gradient_params; 0 = the library's default (stride 3, 3 iterations, gain 2, norm_floor 1e-6)."""
    return PtGradientParams(int(width), int(height), int(stride), int(iterations), float(gain), float(norm_floor))


def gradient_grid(width, height, stride=0):
    """(r0, TH, TW) of pt_temporal_gradient's tile grid: the first sampled row and the shape of the lambda map."""
    s = int(stride) or 3
    r0 = s // 2
    if not 1 <= s <= 16 or height <= r0:
        raise ValueError("gradient_grid: stride must be 0 or 1..16 and height > stride // 2")
    return r0, (height - r0 + s - 1) // s, (width + s - 1) // s


def gradient_rows_params(prev_params, stride=0):
    """A copy of the previous frame's PtRenderParams with the row selection pt_temporal_gradient's `resampled` is rendered with:
    row_begin = stride // 2, row_end = height, row_stride = stride (0 = the default, 3)."""
    q = prev_params.copy()
    r0, _, _ = gradient_grid(q.width, q.height, stride)
    q.row_begin, q.row_end, q.row_stride = r0, q.height, int(stride) or 3
    return q


def _gradient_args(prev_color, resampled, kw):
    prev_color, resampled = (np.ascontiguousarray(a, dtype=np.float32) for a in (prev_color, resampled))
    if prev_color.ndim != 3 or prev_color.shape[2] != 3:
        raise ValueError("temporal_gradient: prev_color must be [H, W, 3]")
    H, W = prev_color.shape[:2]
    g = gradient_params(W, H, **kw)
    _, TH, TW = gradient_grid(W, H, g.stride)
    if resampled.shape != (TH, W, 3):
        raise ValueError(f"temporal_gradient: resampled must be [{TH}, {W}, 3] (the rows of gradient_rows_params)")
    return prev_color, resampled, g, (TH, TW)


def temporal_gradient_host(prev_color, resampled, **kw):
    """pt_temporal_gradient_host: the rule of pt_temporal_gradient run by the host half of the library (no GPU needed).  Returns
    lambda [TH, TW]."""
    prev_color, resampled, g, shape = _gradient_args(prev_color, resampled, kw)
    out = np.empty(shape, dtype=np.float32)
    _check(lib().pt_temporal_gradient_host(C.byref(g), *_ptrs([prev_color, resampled, out])))
    return out


def gradient_pixels_host(width, height, seed, **kw):
    """pt_gradient_pixels_host: the pixel of every tile of the gradient grid at `seed` (no GPU needed), [TH * TW] int32."""
    g = gradient_params(width, height, **kw)
    _, TH, TW = gradient_grid(width, height, g.stride)
    out = np.empty(TH * TW, dtype=np.int32)
    _check(lib().pt_gradient_pixels_host(C.byref(g), int(seed) & 0xffffffff, *_ptrs([out])))
    return out


def _gradient_sparse_args(prev_color, pixels, resampled, kw):
    prev_color, resampled = (np.ascontiguousarray(a, dtype=np.float32) for a in (prev_color, resampled))
    pixels = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1)
    if prev_color.ndim != 3 or prev_color.shape[2] != 3:
        raise ValueError("temporal_gradient_sparse: prev_color must be [H, W, 3]")
    H, W = prev_color.shape[:2]
    g = gradient_params(W, H, **kw)
    _, TH, TW = gradient_grid(W, H, g.stride)
    if pixels.size != TH * TW or resampled.shape != (TH * TW, 3):
        raise ValueError(f"temporal_gradient_sparse: pixels must be [{TH * TW}] and resampled [{TH * TW}, 3] (one pixel per tile)")
    return prev_color, pixels, resampled, g, (TH, TW)


def temporal_gradient_sparse_host(prev_color, pixels, resampled, **kw):
    """pt_temporal_gradient_sparse_host: the rule of pt_temporal_gradient_sparse run by the host half of the library (no GPU
    needed).  Returns lambda [TH, TW]."""
    prev_color, pixels, resampled, g, shape = _gradient_sparse_args(prev_color, pixels, resampled, kw)
    out = np.empty(shape, dtype=np.float32)
    _check(lib().pt_temporal_gradient_sparse_host(C.byref(g), *_ptrs([prev_color, pixels, resampled, out])))
    return out


def _lambda_arg(lam, frame_shape, stride):
    lam = np.ascontiguousarray(lam, dtype=np.float32)
    H, W = frame_shape
    try:
        shape = gradient_grid(W, H, stride)[1:]
    except ValueError:
        return lam                                                # a stride or frame the library rejects, naming it
    if lam.shape != shape:
        raise ValueError("temporal_accumulate_adaptive: lam must be the [TH, TW] map of temporal_gradient at this stride")
    return lam


def temporal_accumulate_adaptive_host(color, albedo, normal, motion, prev_depth, lam, history=None, stride=0, out_color=None,
                                      albedo_floor=0.0, **kw):
    """pt_temporal_accumulate_adaptive_host: the rule of pt_temporal_accumulate_adaptive run by the host half of the library (no
    GPU needed).  Returns (out_color, out_len, out_moments); out_color as in temporal_accumulate_moments_host."""
    args, t = _temporal_moments_args(color, albedo, normal, motion, prev_depth, history, kw)
    lam = _lambda_arg(lam, args[4].shape, stride)
    out_color = _out_like(out_color, args[0], "temporal_accumulate_adaptive_host: out_color")
    outs = [out_color, np.empty_like(args[4]), np.empty_like(args[3])]
    io = PtTemporalIo(*_ptrs(args + outs))
    _check(lib().pt_temporal_accumulate_adaptive_host(C.byref(t), float(albedo_floor), C.byref(io), *_ptrs([lam]), int(stride)))
    return tuple(outs)


def vdenoise_params(width, height, iterations=0, normal_power_log2=7, sigma_z=0.0, sigma_l=0.0, scale=0.0, albedo_floor=0.0,
                    min_history=0, var_floor=0.0):
    """pt_vdenoise_params; 0 = the library's default (5 iterations, sigma_z 0.05, sigma_l 4, scale 1, albedo_floor 0.01,
    min_history 4, var_floor 1e-10)."""
    return PtVdenoiseParams(int(width), int(height), int(iterations), int(normal_power_log2), float(sigma_z), float(sigma_l),
                            float(scale), float(albedo_floor), int(min_history), float(var_floor))


def _vdenoise_args(color, albedo, normal, depth, moments, hist_len, kw):
    color, albedo, normal, depth = _denoise_args(color, albedo, normal, depth, {})[:4]
    moments, hist_len = (np.ascontiguousarray(a, dtype=np.float32) for a in (moments, hist_len))
    H, W = depth.shape
    if moments.shape != (H, W, 2) or hist_len.shape != (H, W):
        raise ValueError("denoise_variance: moments must be [H, W, 2] and hist_len [H, W]")
    return [color, albedo, normal, depth, moments, hist_len], vdenoise_params(W, H, **kw)


def denoise_variance_host(color, albedo, normal, depth, moments, hist_len, out=None, variance=False, **kw):
    """pt_denoise_variance_host: the filter of pt_denoise_variance run by the host half of the library (no GPU needed).  out: an
    [H, W, 3] float32 array to write (it may be `color` itself); default a new one.  variance=True: (out, variance [H, W])."""
    arrays, d = _vdenoise_args(color, albedo, normal, depth, moments, hist_len, kw)
    out = _out_like(out, arrays[0], "denoise_variance_host: out")
    var = np.empty_like(arrays[3]) if variance else None
    _check(lib().pt_denoise_variance_host(C.byref(d), *_ptrs(arrays + [out, var])))
    return (out, var) if variance else out


def debug_math(op, x, y=None, host=False):
    """op 0: sincos, 1: powf, 2: pcg32 (stream/seed = bit patterns of x/y).  host=True runs the host build of pt_math.h."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = x if y is None else np.ascontiguousarray(y, dtype=np.float32)
    o0 = np.zeros_like(x)
    o1 = np.zeros_like(x)
    fn = lib().pt_debug_math_host if host else lib().pt_debug_math
    _check(fn(op, _fp(x), _fp(y), _fp(o0), _fp(o1), x.size))
    return o0, o1


def debug_exact_math(op, begin=0, count=1 << 32):
    """pt_debug_exact_math: the device's exact short sequence `op` (PT_EXACT_RCP / _DIV_PI / _SQRT, or the control
    PT_EXACT_RAW_RCP) against the IEEE expression it replaces on the fp32 bit patterns begin .. begin + count - 1.
    Returns (mismatches, first mismatching bit pattern or -1)."""
    bad, first = C.c_uint64(), C.c_int64()
    _check(lib().pt_debug_exact_math(op, begin, count, C.byref(bad), C.byref(first)))
    return bad.value, first.value


def build_bvh_sweep(desc, on_device=False):
    """The library's internal-tree builder over the leaf boxes of `desc`'s tree: pt_bvh_build_sweep (host code, runs without a
    GPU) or, on_device=True, pt_bvh_build_sweep_device — the same tree byte for byte.  Returns (desc2, info) like build_bvh_device."""
    n_nodes = 2 * desc.num_shapes - 1
    nodes = np.zeros(max(n_nodes, 1), dtype=NODE_DTYPE)
    root, depth, ms = C.c_int32(), C.c_int32(), C.c_double()
    fn = lib().pt_bvh_build_sweep_device if on_device else lib().pt_bvh_build_sweep
    _check(fn(C.byref(desc), nodes.ctypes.data_as(C.POINTER(PtBvhNode)), C.byref(root), C.byref(depth),
                                    C.byref(ms)))
    d2 = PtSceneDesc()
    C.memmove(C.byref(d2), C.byref(desc), C.sizeof(PtSceneDesc))
    d2.nodes = nodes.ctypes.data_as(C.POINTER(PtBvhNode))
    d2.num_nodes = n_nodes
    d2.root = root.value
    d2._keep = (nodes, desc)
    return d2, {"root": root.value, "depth": depth.value, "build_ms": ms.value, "nodes": nodes}


def edited_desc(desc, meshes=None, spheres=None, materials=None, lights=None, background=None, shapes=None, mesh_list=None):
    """A copy of `desc` with some of its arrays replaced, for DeviceScene.update and host.refit_bvh.
      meshes      {mesh_index: (positions [V, 3], normals [V, 3] or None = keep the mesh's normals)}
      spheres     {shape_id: (center, radius)}
      materials   a sequence of PtMaterial, as many as desc has       lights   the same with PtLight
      background  (r, g, b)
      shapes      a sequence of PtShape that replaces the whole shape list; as many as desc has (ValueError otherwise)
      mesh_list   a sequence of (positions [V, 3], indices [F, 3], normals [V, 3], material_id, area_light_id) that replaces the
                  whole mesh table; its length may differ from desc's, and may be 0
    Every argument defaults to "unchanged".  `meshes` edits the table `mesh_list` gives (or desc's), `spheres` the list `shapes`
    gives (or desc's).  The node pool is desc's — topology is what an update keeps — and whatever is not replaced is shared
    with `desc`; the copy keeps the new arrays, and `desc`, alive."""
    d2 = PtSceneDesc()
    C.memmove(C.byref(d2), C.byref(desc), C.sizeof(PtSceneDesc))
    keep = [desc]
    if mesh_list is not None:
        mesh_list = list(mesh_list)
        arr = (PtMesh * max(len(mesh_list), 1))()
        for m, (pos, idx, nrm, material_id, area_light_id) in enumerate(mesh_list):
            P = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
            I = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1, 3)
            Nn = np.ascontiguousarray(nrm, dtype=np.float32).reshape(-1, 3)
            if Nn.shape != P.shape:
                raise ValueError("normals must match positions")
            arr[m] = PtMesh(int(material_id), int(area_light_id), P.shape[0], I.shape[0], _fp(P),
                            I.ctypes.data_as(C.POINTER(C.c_int32)), _fp(Nn))
            keep += [P, I, Nn]
        d2.meshes = arr if mesh_list else None
        d2.num_meshes = len(mesh_list)
        keep.append(arr)
    if shapes is not None:
        shapes = list(shapes)
        if len(shapes) != desc.num_shapes:
            raise ValueError(f"shapes: the count must stay {desc.num_shapes}")
        arr = (PtShape * desc.num_shapes)(*shapes)
        d2.shapes = arr
        keep.append(arr)
    if meshes:
        arr = (PtMesh * d2.num_meshes)()
        C.memmove(arr, d2.meshes, C.sizeof(arr))
        for m, (pos, nrm) in meshes.items():
            if not 0 <= m < d2.num_meshes:
                raise ValueError(f"mesh index {m} out of range")
            P = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
            if P.shape[0] != arr[m].num_vertices:
                raise ValueError(f"mesh {m} has {arr[m].num_vertices} vertices, got {P.shape[0]}")
            arr[m].positions = _fp(P)
            keep.append(P)
            if nrm is not None:
                Nn = np.ascontiguousarray(nrm, dtype=np.float32).reshape(-1, 3)
                if Nn.shape != P.shape:
                    raise ValueError("normals must match positions")
                arr[m].normals = _fp(Nn)
                keep.append(Nn)
        d2.meshes = arr
        keep.append(arr)
    if spheres:
        arr = (PtShape * desc.num_shapes)()
        C.memmove(arr, d2.shapes, C.sizeof(arr))
        for i, (center, radius) in spheres.items():
            if not 0 <= i < desc.num_shapes or arr[i].type != PT_SHAPE_SPHERE:
                raise ValueError(f"shape {i} is not a sphere")
            arr[i].center[:] = [float(x) for x in center]
            arr[i].radius = float(radius)
        d2.shapes = arr
        keep.append(arr)
    for name, ctype, seq in (("materials", PtMaterial, materials), ("lights", PtLight, lights)):
        if seq is not None:
            seq = list(seq)
            if len(seq) != getattr(desc, "num_" + name):
                raise ValueError(f"{name}: the count must stay {getattr(desc, 'num_' + name)}")
            arr = (ctype * max(len(seq), 1))(*seq)
            setattr(d2, name, arr)
            keep.append(arr)
    if background is not None:
        d2.background[:] = [float(x) for x in background]
    d2._keep = keep
    return d2


def _matrices(matrices):
    M = np.ascontiguousarray(matrices, dtype=np.float32)
    if M.ndim == 2 and M.shape == (3, 4):
        M = M[None]
    if M.ndim != 3 or M.shape[1:] != (3, 4):
        raise ValueError("matrices must be [num_groups, 3, 4]")
    return M


SHAPE_DTYPE = np.dtype([("type", "<i4"), ("material_id", "<i4"), ("area_light_id", "<i4"), ("center", "<f4", 3), ("radius", "<f4"),
                        ("face_index", "<i4"), ("mesh_index", "<i4")])


def shape_table(desc):
    """desc's shapes as a structured numpy array (a copy)."""
    assert SHAPE_DTYPE.itemsize == C.sizeof(PtShape)
    raw = C.string_at(C.addressof(desc.shapes.contents), desc.num_shapes * C.sizeof(PtShape))
    return np.frombuffer(raw, dtype=SHAPE_DTYPE).copy()


def groups_by_object(desc):
    """One group per object of `desc`: a triangle's group is its mesh_index, sphere k (the k-th sphere in shape order) gets
    num_meshes + k.  Returns (ids [num_shapes] int32, num_groups)."""
    sh = shape_table(desc)
    sphere = sh["type"] == PT_SHAPE_SPHERE
    ids = sh["mesh_index"].astype(np.int32)
    ids[sphere] = desc.num_meshes + np.arange(int(sphere.sum()), dtype=np.int32)
    return ids, desc.num_meshes + int(sphere.sum())


def rigid_matrix(axis, degrees, centre=(0.0, 0.0, 0.0), scale=1.0, translate=(0.0, 0.0, 0.0)):
    """A row-major 3x4 float32 matrix: rotation by `degrees` about the unit vector along `axis` through `centre`, a uniform
    `scale` about the same point, then a translation."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    t = np.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = (np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)) * scale
    c = np.asarray(centre, dtype=np.float64)
    M = np.empty((3, 4))
    M[:, :3] = R
    M[:, 3] = c - R @ c + np.asarray(translate, dtype=np.float64)
    return M.astype(np.float32)


def transform_geometry_host(matrix, positions, normals=None):
    """pt_transform_geometry_host: positions [n, 3] (and normals [n, 3]) under one 3x4 matrix, by the host half of the library
    (no GPU needed).  Returns (positions', normals' or None) as new arrays."""
    M = _matrices(matrix)[0]
    P = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    Nn = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    if Nn is not None and Nn.shape != P.shape:
        raise ValueError("normals must match positions")
    Po = np.empty_like(P)
    No = None if Nn is None else np.empty_like(Nn)
    _check(lib().pt_transform_geometry_host(M.ctypes.data_as(C.POINTER(PtTransform)), P.shape[0], *_ptrs([P, Nn, Po, No])))
    return Po, No


def transform_sphere_host(matrix, center, radius):
    """pt_transform_sphere_host: (centre' [3] float32, radius' as np.float32) of a sphere under one 3x4 matrix (no GPU needed)."""
    M = _matrices(matrix)[0]
    c = np.ascontiguousarray(center, dtype=np.float32).reshape(3)
    co, ro = np.empty(3, dtype=np.float32), np.empty(1, dtype=np.float32)
    _check(lib().pt_transform_sphere_host(M.ctypes.data_as(C.POINTER(PtTransform)), _fp(c), float(np.float32(radius)), _fp(co), _fp(ro)))
    return co, ro[0]


def transform_desc_host(desc, ids, matrices):
    """The desc DeviceScene.transform(matrices) stands for, made on the host: a copy of `desc` (edited_desc) in which every shape
    with a group id >= 0 is under its group's matrix, through pt_transform_geometry_host / pt_transform_sphere_host.  Transforms
    apply to `desc` — the rest pose — and never compose: transform_desc_host(desc, ids, M2) does not depend on an M1 applied
    before.  A mesh whose faces all share one group keeps its vertex table; one whose faces are spread over several groups
    gets a table of three vertices per face (a vertex shared by two groups has two images).  The node pool is desc's."""
    from .standins import mesh_arrays
    M = _matrices(matrices)
    ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    if ids.size != desc.num_shapes or (ids.size and (ids.min() < -1 or ids.max() >= M.shape[0])):
        raise ValueError("ids must hold one value in [-1, num_groups) per shape")
    sh = shape_table(desc)
    tri = sh["type"] != PT_SHAPE_SPHERE
    mesh_list = []
    for m in range(desc.num_meshes):
        P, I, Nn = mesh_arrays(desc, m)
        mine = np.nonzero(tri & (sh["mesh_index"] == m))[0]
        fg = np.full(I.shape[0], -1, dtype=np.int32)
        fg[sh["face_index"][mine]] = ids[mine]
        if (fg[sh["face_index"][mine]] != ids[mine]).any():
            raise ValueError(f"mesh {m}: a face is used by shapes of different groups")
        used = np.unique(ids[mine])
        if used.size == 1 and used[0] >= 0:
            P, Nn = transform_geometry_host(M[used[0]], P, Nn)
        elif used.size > 1:
            P, Nn = P[I].reshape(-1, 3), Nn[I].reshape(-1, 3)
            I = np.arange(P.shape[0], dtype=np.int32).reshape(-1, 3)
            order = np.argsort(fg, kind="stable")
            groups, first = np.unique(fg[order], return_index=True)
            for g, lo, hi in zip(groups, first, list(first[1:]) + [order.size]):
                if g >= 0:
                    v = (3 * order[lo:hi, None] + np.arange(3)).reshape(-1)
                    P[v], Nn[v] = transform_geometry_host(M[g], P[v], Nn[v])
        mesh_list.append((P, I, Nn, desc.meshes[m].material_id, desc.meshes[m].area_light_id))
    spheres = {}
    for i in np.nonzero(~tri & (ids >= 0))[0]:
        spheres[int(i)] = transform_sphere_host(M[ids[i]], sh["center"][i], sh["radius"][i])
    return edited_desc(desc, mesh_list=mesh_list, spheres=spheres)


def wobbled_desc(desc, step, meshes=None, amp=0.01):
    """A copy of `desc` (edited_desc) whose meshes — all of them, or those listed — are displaced by a smooth per-vertex wobble,
    amp * extent * sin(k . p + phase(step)) per axis, with the vertex normals computed anew: an animation to drive
    DeviceScene.update with (tools/animate.py).  step 0 is not the rest pose; the rest pose is `desc` itself."""
    from . import host
    from .standins import mesh_arrays
    edits = {}
    for m in (range(desc.num_meshes) if meshes is None else meshes):
        P, I, _ = mesh_arrays(desc, m)
        size = max(float((P.max(axis=0) - P.min(axis=0)).max()), 1e-6)
        ph = 0.37 * step
        off = np.stack([np.sin(5.0 / size * P[:, 1] + ph), np.cos(4.0 / size * P[:, 2] + ph), np.sin(6.0 / size * P[:, 0] - ph)], axis=1)
        Q = (P + np.float32(amp * size) * off.astype(np.float32)).astype(np.float32)
        edits[m] = (Q, host.compute_normals(Q, I))
    return edited_desc(desc, meshes=edits)


def translated_params(params, delta):
    """A copy of the render parameters with the camera moved by `delta` (origin and image plane alike), in fp32."""
    q = params.copy()
    for name in ("cam_origin", "cam_top_left"):
        v = np.array(list(getattr(params, name)), dtype=np.float32) + np.asarray(delta, dtype=np.float32)
        getattr(q, name)[:] = [float(x) for x in v]
    return q


PT_BVH_DEVICE_LBVH, PT_BVH_DEVICE_SAH = 0, 1


def build_bvh_device(desc, method=PT_BVH_DEVICE_SAH):
    """Builds the BVH of `desc`'s primitives on the GPU (pt_bvh_build_device).  Returns (desc2, info): desc2 is a copy of
    `desc` that points at the new node array (kept alive by desc2), info = {"root", "depth", "build_ms", "nodes"}."""
    n_nodes = 2 * desc.num_shapes - 1
    nodes = np.zeros(max(n_nodes, 1), dtype=NODE_DTYPE)
    root, depth, ms = C.c_int32(), C.c_int32(), C.c_double()
    _check(lib().pt_bvh_build_device(C.byref(desc), int(method), nodes.ctypes.data_as(C.POINTER(PtBvhNode)), C.byref(root),
                                     C.byref(depth), C.byref(ms)))
    d2 = PtSceneDesc()
    C.memmove(C.byref(d2), C.byref(desc), C.sizeof(PtSceneDesc))
    d2.nodes = nodes.ctypes.data_as(C.POINTER(PtBvhNode))
    d2.num_nodes = n_nodes
    d2.root = root.value
    d2._keep = (nodes, desc)          # the node array, and whatever keeps the other arrays of `desc` alive
    return d2, {"root": root.value, "depth": depth.value, "build_ms": ms.value, "nodes": nodes}
