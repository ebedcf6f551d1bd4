"""ctypes mirrors of the PODs in include/pt_api.h and include/pt_host.h.

Kept free of any library loading so both the product bindings (host.py, device.py)
and the test-only oracle binding (tests/oracle_binding.py) can share them.
"""
import ctypes as C

c_float3 = C.c_float * 3

PT_OK = 0
PT_ERR_INVALID_ARG, PT_ERR_BAD_SCENE, PT_ERR_DEVICE, PT_ERR_NO_DEVICE = 1, 2, 3, 4
PT_ERR_IO, PT_ERR_PARSE, PT_ERR_UNSUPPORTED = 5, 6, 7
PT_SHAPE_SPHERE, PT_SHAPE_TRIANGLE = 0, 1
PT_MAT_DIFFUSE, PT_MAT_MIRROR, PT_MAT_PLASTIC, PT_MAT_PHONG = 0, 1, 2, 3
PT_LIGHT_POINT, PT_LIGHT_DIFFUSE_AREA = 0, 1
PT_TRAVERSAL_DEFAULT, PT_TRAVERSAL_EXACT, PT_TRAVERSAL_PRUNED = 0, 1, 2
PT_BVH_SORT_TOTAL, PT_BVH_SORT_REFERENCE = 0, 1
PT_RENDER_NEE = 1
PT_UPDATE_GEOMETRY, PT_UPDATE_SHADING = 1, 2                                  # pt_scene_update flags
PT_EXACT_RCP, PT_EXACT_DIV_PI, PT_EXACT_SQRT, PT_EXACT_RAW_RCP = 0, 1, 2, 3   # pt_debug_exact_math ops

STATUS_NAMES = {
    0: "PT_OK", 1: "PT_ERR_INVALID_ARG", 2: "PT_ERR_BAD_SCENE", 3: "PT_ERR_DEVICE", 4: "PT_ERR_NO_DEVICE",
    5: "PT_ERR_IO", 6: "PT_ERR_PARSE", 7: "PT_ERR_UNSUPPORTED",
}


class PtShape(C.Structure):
    _fields_ = [("type", C.c_int32), ("material_id", C.c_int32), ("area_light_id", C.c_int32),
                ("center", c_float3), ("radius", C.c_float), ("face_index", C.c_int32), ("mesh_index", C.c_int32)]


class PtMesh(C.Structure):
    _fields_ = [("material_id", C.c_int32), ("area_light_id", C.c_int32), ("num_vertices", C.c_int32),
                ("num_faces", C.c_int32), ("positions", C.POINTER(C.c_float)), ("indices", C.POINTER(C.c_int32)),
                ("normals", C.POINTER(C.c_float))]


class PtMaterial(C.Structure):
    _fields_ = [("type", C.c_int32), ("reflectance", c_float3), ("eta", C.c_float), ("exponent", C.c_float)]


class PtLight(C.Structure):
    _fields_ = [("type", C.c_int32), ("shape_id", C.c_int32), ("radiance", c_float3), ("position", c_float3)]


class PtBvhNode(C.Structure):
    _fields_ = [("bmin", c_float3), ("bmax", c_float3), ("left", C.c_int32), ("right", C.c_int32), ("prim", C.c_int32)]


class PtSceneDesc(C.Structure):
    _fields_ = [("num_shapes", C.c_int32), ("shapes", C.POINTER(PtShape)),
                ("num_meshes", C.c_int32), ("meshes", C.POINTER(PtMesh)),
                ("num_materials", C.c_int32), ("materials", C.POINTER(PtMaterial)),
                ("num_lights", C.c_int32), ("lights", C.POINTER(PtLight)),
                ("num_nodes", C.c_int32), ("nodes", C.POINTER(PtBvhNode)),
                ("root", C.c_int32), ("background", c_float3)]


class PtRenderParams(C.Structure):
    _fields_ = [("cam_origin", c_float3), ("cam_top_left", c_float3), ("cam_horizontal", c_float3),
                ("cam_vertical", c_float3), ("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32),
                ("row_begin", C.c_int32), ("row_end", C.c_int32), ("row_stride", C.c_int32),
                ("seed", C.c_uint64), ("max_depth", C.c_int32), ("rr_depth", C.c_int32),
                ("sample_offset", C.c_int32), ("stream_stride", C.c_int32), ("traversal", C.c_int32),
                ("flags", C.c_int32)]

    def copy(self):
        out = PtRenderParams()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(PtRenderParams))
        return out

    def num_rows(self):
        rb, re = self.row_begin, self.row_end
        if rb == 0 and re == 0:
            re = self.height
        step = self.row_stride if self.row_stride > 1 else 1
        return len(range(rb, re, step))


class PtCounters(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("segments", C.c_uint64), ("node_visits", C.c_uint64),
                ("leaf_tests", C.c_uint64), ("kernel_ms", C.c_double), ("resolve_ms", C.c_double)]


class PtAdaptiveParams(C.Structure):
    """pt_adaptive_params (pt_api.h): per-pixel sample counts from a noise target (pt_render_adaptive)."""
    _fields_ = [("batch_spp", C.c_int32), ("max_spp", C.c_int32), ("max_error", C.c_float), ("p_value", C.c_float),
                ("min_luminance", C.c_float)]


class PtDenoiseParams(C.Structure):
    """pt_denoise_params (pt_api.h): edge-avoiding a-trous filter guided by albedo, normal and depth (pt_denoise)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32), ("normal_power_log2", C.c_int32),
                ("sigma_z", C.c_float), ("sigma_c", C.c_float), ("scale", C.c_float), ("albedo_floor", C.c_float)]


PT_MOTION_GEOMETRY_CURRENT, PT_MOTION_GEOMETRY_PREVIOUS = 0, 1                # pt_motion_params.geometry
PT_QUERY_CLOSEST, PT_QUERY_ANY = 0, 1                                         # pt_trace_rays modes


class PtTransform(C.Structure):
    """pt_transform (pt_api.h): a row-major 3x4 matrix, one per group of shapes (pt_scene_transform)."""
    _fields_ = [("m", C.c_float * 12)]


class PtMotionParams(C.Structure):
    """pt_motion_params (pt_api.h): the previous frame's camera and which record set holds its geometry (pt_render_guides)."""
    _fields_ = [("prev_cam_origin", c_float3), ("prev_cam_top_left", c_float3), ("prev_cam_horizontal", c_float3),
                ("prev_cam_vertical", c_float3), ("geometry", C.c_int32)]


class PtGuideBuffers(C.Structure):
    """pt_guide_buffers (pt_api.h): the six outputs of pt_render_guides, any of them NULL."""
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("prim", C.c_void_p),
                ("motion", C.c_void_p), ("prev_depth", C.c_void_p)]


class PtTemporalParams(C.Structure):
    """pt_temporal_params (pt_api.h): history length cap and the depth / normal tests of pt_temporal_accumulate."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("max_history", C.c_int32), ("sigma_z", C.c_float),
                ("normal_min", C.c_float), ("scale", C.c_float)]


class PtTemporalIo(C.Structure):
    """pt_temporal_io (pt_api.h): the buffers of pt_temporal_accumulate_moments; host or device addresses, None = NULL."""
    _fields_ = [(n, C.c_void_p) for n in ("color", "albedo", "normal", "motion", "prev_depth", "hist_color", "hist_normal",
                                          "hist_depth", "hist_len", "hist_moments", "out_color", "out_len", "out_moments")]


class PtVdenoiseParams(C.Structure):
    """pt_vdenoise_params (pt_api.h): the variance-guided a-trous filter (pt_denoise_variance)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("iterations", C.c_int32), ("normal_power_log2", C.c_int32),
                ("sigma_z", C.c_float), ("sigma_l", C.c_float), ("scale", C.c_float), ("albedo_floor", C.c_float),
                ("min_history", C.c_int32), ("var_floor", C.c_float)]


class PtGradientParams(C.Structure):
    """pt_gradient_params (pt_api.h): the tile grid, filter and gain of pt_temporal_gradient."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32), ("iterations", C.c_int32),
                ("gain", C.c_float), ("norm_floor", C.c_float)]


# Parameter lists of pt_render_pixels and the sparse gradient's entry points (pt_api.h), which device.lib() installs.
SPARSE_ARGTYPES = {
    "pt_render_pixels": [C.c_void_p, C.POINTER(PtRenderParams), C.c_void_p, C.c_int32, C.c_void_p, C.c_int, C.c_void_p],
    "pt_gradient_pixels": [C.c_void_p, C.POINTER(PtGradientParams), C.c_uint32, C.c_void_p, C.c_int, C.c_void_p],
    "pt_gradient_pixels_host": [C.POINTER(PtGradientParams), C.c_uint32, C.c_void_p],
    "pt_temporal_gradient_sparse": [C.c_void_p, C.POINTER(PtGradientParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_void_p],
    "pt_temporal_gradient_sparse_host": [C.POINTER(PtGradientParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
}

# ... and of the ray query and the asynchronous guide pass.
QUERY_ARGTYPES = {
    "pt_trace_rays": [C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "pt_render_guides_async": [C.c_void_p, C.POINTER(PtRenderParams), C.POINTER(PtMotionParams), C.POINTER(PtGuideBuffers), C.c_void_p],
}


class PtCamera(C.Structure):
    _fields_ = [("lookfrom", c_float3), ("lookat", c_float3), ("up", c_float3), ("vfov", C.c_float),
                ("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32)]


class PtError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status
