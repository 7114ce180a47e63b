"""ctypes declarations for librtmi.so (include/rtmi.h).

The library is built in-tree by `make -C a_dive_into_ray_tracing_amd/csrc`
(or `__graft_entry__.build()`) into a_dive_into_ray_tracing_amd/lib/.  There is
no fallback: if the library is missing, importing the bindings raises.
"""
import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTMI_LIBRARY") or os.path.join(PKG_DIR, "lib", "librtmi.so")

RT_OK = 0
ERRORS = {
    -1: "RT_EINVAL",
    -2: "RT_EHIP",
    -3: "RT_ENODEVICE",
    -4: "RT_EUNSUPPORTED",
    -5: "RT_ENOMEM",
    -6: "RT_ERCCL",
    -7: "RT_EIO",
    -8: "RT_ESTREAM",
}
RT_MAT_LAMBERTIAN, RT_MAT_METAL, RT_MAT_DIELECTRIC = 0, 1, 2

_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)


class RtScene(C.Structure):
    _fields_ = [("n", C.c_int32), ("center_radius", _dp), ("mat_kind", _ip), ("mat_params", _dp)]


class RtCamera(C.Structure):
    _fields_ = [(nm, C.c_double * 3) for nm in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w")] + [
        ("lens_radius", C.c_double)
    ]


class RtNwCamera(C.Structure):
    _fields_ = [("cam", RtCamera), ("time0", C.c_double), ("time1", C.c_double)]


class RtNwFlat(C.Structure):
    _fields_ = [(nm, C.c_int32) for nm in ("n_obj", "n_inst", "n_mat", "n_tex", "n_perlin", "n_image")] + [
        (nm, _fp) for nm in ("obj", "inst", "mat", "tex", "perlin_vec")
    ] + [("perlin_perm", _ip), ("image_desc", _ip), ("image_px", C.POINTER(C.c_uint8)), ("image_bytes", C.c_int64),
         ("background", C.c_float * 3)]


class RtNwAdaptStats(C.Structure):
    _fields_ = [("passes", C.c_int32), ("stopped", C.c_int32), ("total_samples", C.c_int64), ("pixels_at_max", C.c_int64),
                ("samples", C.c_int64), ("segments", C.c_int64),
                ("active", C.POINTER(C.c_int64)), ("cap", C.c_int32), ("pad", C.c_int32)]


class RtNwDenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("sigma_l", C.c_float), ("sigma_n", C.c_float), ("sigma_z", C.c_float),
                ("flags", C.c_uint32)]


NW_DENOISE_DEMODULATE, NW_DENOISE_NO_EDGES = 1, 2

NW_ADAPT_ON_PASS = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int64)  # rt_nw_adapt_on_pass


class RTError(RuntimeError):
    def __init__(self, what, code, msg):
        super().__init__(f"{what} failed: {ERRORS.get(code, code)}: {msg}")
        self.code = code


# every symbol include/rtmi.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "rt_last_error": (C.c_char_p, []),
    "rt_version": (C.c_int, []),
    "rt_camera_init": (C.c_int, [C.POINTER(RtCamera), _dp, _dp, _dp, C.c_double, C.c_double, C.c_double, C.c_double]),
    "rt_scene_random": (C.c_int, [C.c_uint32, _dp, _ip, _dp, C.c_int32, _ip]),
    "rt_scene_learn": (C.c_int, [_dp, _ip, _dp, C.c_int32, _ip]),
    "rt_write_ppm": (C.c_int, [C.c_char_p, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "rt_quantize": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]),
    "rt_write_pfm": (C.c_int, [C.c_char_p, _fp, C.c_int32, C.c_int32, C.c_int32]),
    "rt_scene_write": (C.c_int, [C.c_char_p, C.POINTER(RtScene)]),
    "rt_scene_read": (C.c_int, [C.c_char_p, _dp, _ip, _dp, C.c_int32, _ip]),
    "rt_device_count": (C.c_int, [_ip]),
    "rt_ctx_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "rt_ctx_destroy": (C.c_int, [C.c_void_p]),
    "rt_ctx_set_scene": (C.c_int, [C.c_void_p, C.POINTER(RtScene)]),
    "rt_ctx_set_tuning": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "rt_ctx_set_schedule": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "rt_ctx_set_overlap": (C.c_int, [C.c_void_p, C.c_int32]),
    "rt_ctx_set_kernel": (C.c_int, [C.c_void_p, C.c_int32]),
    "rt_ctx_set_accel": (C.c_int, [C.c_void_p, C.c_int32]),
    "rt_ctx_set_ordering": (C.c_int, [C.c_void_p, C.c_int32]),
    "rt_ctx_accel_info": (C.c_int, [C.c_void_p, _ip, _ip]),
    "rt_render": (C.c_int, [C.c_void_p, C.POINTER(RtCamera), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, _fp]),
    "rt_render_rows": (
        C.c_int,
        [C.c_void_p, C.POINTER(RtCamera)] + [C.c_int32] * 4 + [C.c_uint64] + [C.c_int32] * 3 + [C.c_void_p, C.c_void_p],
    ),
    "rt_ctx_synchronize": (C.c_int, [C.c_void_p]),
    "rt_ctx_last_segments": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "rt_accum_reset": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "rt_render_pass": (
        C.c_int,
        [C.c_void_p, C.POINTER(RtCamera)] + [C.c_int32] * 5 + [C.c_uint64] + [C.c_int32] * 3 + [C.c_void_p],
    ),
    "rt_accum_resolve": (C.c_int, [C.c_void_p, C.c_void_p, _fp, C.c_void_p]),
    "rt_accum_export": (C.c_int, [C.c_void_p, _lp, C.c_size_t, _ip]),
    "rt_accum_import": (C.c_int, [C.c_void_p, _lp, C.c_size_t, C.c_int32]),
    "rt_accum_save": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(RtScene), C.POINTER(RtCamera)] + [C.c_int32] * 4 + [C.c_uint64]),
    "rt_accum_load": (
        C.c_int,
        [C.c_void_p, C.c_char_p, C.POINTER(RtScene), C.POINTER(RtCamera)] + [C.c_int32] * 6 + [C.c_uint64, _ip],
    ),
    "rt_replay_worker": (C.c_int, [C.c_void_p, C.POINTER(RtCamera)] + [C.c_int32] * 5 + [_ip, _ip, _lp, _dp, _lp]),
    "rt_render_multi": (C.c_int, [C.POINTER(RtScene), C.POINTER(RtCamera)] + [C.c_int32] * 4 + [C.c_uint64, C.c_int32, _fp]),
    "rt_multi_create": (C.c_int, [C.POINTER(RtScene), C.c_int32, C.POINTER(C.c_void_p)]),
    "rt_multi_destroy": (C.c_int, [C.c_void_p]),
    "rt_multi_device_count": (C.c_int, [C.c_void_p, _ip]),
    "rt_multi_context": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "rt_multi_render": (C.c_int, [C.c_void_p, C.POINTER(RtCamera)] + [C.c_int32] * 4 + [C.c_uint64, _fp]),
    "rt_multi_last_timing": (C.c_int, [C.c_void_p, _fp, _fp]),
    "rt_multi_accum_reset": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "rt_multi_render_pass": (C.c_int, [C.c_void_p, C.POINTER(RtCamera)] + [C.c_int32] * 3 + [C.c_uint64]),
    "rt_multi_accum_resolve": (C.c_int, [C.c_void_p, _fp]),
    "rt_unpermute_rows": (C.c_int, [_fp] + [C.c_int32] * 4 + [_fp]),
    # include/rtmi_nw.h (Next-Week renderer)
    "rt_nw_camera_init": (C.c_int, [C.POINTER(RtNwCamera), _dp, _dp, _dp] + [C.c_double] * 6),
    "rt_nw_scene_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "rt_nw_scene_destroy": (C.c_int, [C.c_void_p]),
    "rt_nw_tex_solid": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "rt_nw_tex_checker": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "rt_nw_tex_noise": (C.c_int, [C.c_void_p, C.c_double, _fp, _ip]),
    "rt_nw_tex_image": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32]),
    "rt_nw_mat_lambertian": (C.c_int, [C.c_void_p, C.c_int32]),
    "rt_nw_mat_metal": (C.c_int, [C.c_void_p, C.c_int32, C.c_double]),
    "rt_nw_mat_dielectric": (C.c_int, [C.c_void_p, C.c_double]),
    "rt_nw_mat_diffuse_light": (C.c_int, [C.c_void_p, C.c_int32]),
    "rt_nw_mat_isotropic": (C.c_int, [C.c_void_p, C.c_int32]),
    "rt_nw_sphere": (C.c_int, [C.c_void_p, _dp, C.c_double, C.c_int32]),
    "rt_nw_moving_sphere": (C.c_int, [C.c_void_p, _dp, _dp, C.c_double, C.c_double, C.c_double, C.c_int32]),
    "rt_nw_rect": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_double] * 5 + [C.c_int32]),
    "rt_nw_box": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int32]),
    "rt_nw_triangle": (C.c_int, [C.c_void_p, _dp, _dp, _dp, C.c_int32]),
    "rt_nw_mesh": (C.c_int, [C.c_void_p, _dp, C.c_int32, _ip, C.c_int32, _dp, C.c_int32, _ip, C.c_int32]),
    "rt_nw_load_obj": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, _ip]),
    "rt_nw_scene_obj_stage": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_double, C.POINTER(RtNwCamera), _ip]),
    "rt_nw_mesh_attr": (C.c_int, [C.c_void_p, _dp, C.c_int32, _ip, C.c_int32, _dp, C.c_int32, _ip, _dp, C.c_int32, _ip,
                                  C.c_uint32, C.c_int32]),
    "rt_nw_load_obj_attr": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_uint32, _ip]),
    "rt_nw_scene_obj_stage_attr": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_uint32, C.POINTER(C.c_uint8), C.c_int32,
                                             C.c_int32, C.c_double, C.POINTER(RtNwCamera), _ip]),
    "rt_nw_scene_flat_attr": (C.c_int, [C.c_void_p, _ip, C.POINTER(_fp), C.POINTER(_ip)]),
    "rt_nw_scene_obj_stage_copies": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_uint32, C.POINTER(C.c_uint8), C.c_int32,
                                               C.c_int32, C.c_int32, C.c_double, C.POINTER(RtNwCamera), _ip]),
    "rt_nw_shared": (C.c_int, [C.c_void_p, C.c_int32]),
    "rt_nw_scene_instancing_stats": (C.c_int, [C.c_void_p, _ip]),
    "rt_nw_move": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, C.c_double, C.c_double]),
    "rt_nw_scene_flat_at": (C.c_int, [C.c_void_p, C.c_double, C.POINTER(RtNwFlat)]),
    "rt_nw_scene_motion_stats": (C.c_int, [C.c_void_p, _ip]),
    "rt_nw_scene_obj_stage_moving": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_uint32, C.POINTER(C.c_uint8), C.c_int32,
                                               C.c_int32, C.c_int32, _dp, C.c_double, C.POINTER(RtNwCamera), _ip]),
    "rt_nw_ctx_scene_tri": (C.c_int, [C.c_void_p, _ip]),
    "rt_nw_transform": (C.c_int, [C.c_void_p, C.c_int32, _dp]),
    "rt_nw_scene_affine_stats": (C.c_int, [C.c_void_p, _ip]),
    "rt_nw_scene_obj_stage_tumbled": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_uint32, C.POINTER(C.c_uint8), C.c_int32,
                                                C.c_int32, C.c_int32, _dp, C.c_double, C.POINTER(RtNwCamera), _ip]),
    "rt_nw_debug_trace_t": (C.c_int, [C.c_void_p, C.POINTER(RtNwCamera)] + [C.c_int32] * 3 + [C.c_uint64] + [C.c_int32] * 3 + [_fp, C.c_int32, _ip, _fp]),
    "rt_nw_debug_records": (C.c_int, [C.c_void_p, _fp, C.POINTER(C.c_uint64), C.c_int32, _ip, _fp, _fp, _ip]),
    "rt_nw_constant_medium": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_int32]),
    "rt_nw_medium_samples": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "rt_nw_group": (C.c_int, [C.c_void_p, _ip, C.c_int32]),
    "rt_nw_translate": (C.c_int, [C.c_void_p, C.c_int32, _dp]),
    "rt_nw_rotate_y": (C.c_int, [C.c_void_p, C.c_int32, C.c_double]),
    "rt_nw_world_add": (C.c_int, [C.c_void_p, C.c_int32]),
    "rt_nw_set_background": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "rt_nw_scene_preset": (
        C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_double, C.c_uint32, C.POINTER(RtNwCamera)]),
    "rt_nw_xorwow_uniforms": (C.c_int, [C.c_uint64, C.c_int32, _fp]),
    "rt_nw_scene_flat": (C.c_int, [C.c_void_p, C.POINTER(RtNwFlat)]),
    "rt_nw_ctx_create": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    "rt_nw_ctx_destroy": (C.c_int, [C.c_void_p]),
    "rt_nw_ctx_set_scene": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rt_nw_ctx_info": (C.c_int, [C.c_void_p, _ip, _ip]),
    "rt_nw_ctx_set_accel": (C.c_int, [C.c_void_p, C.c_int32]),
    "rt_nw_scene_grid_stats": (C.c_int, [C.c_void_p, _ip, _ip, _ip, _ip]),
    "rt_nw_debug_phases": (C.c_int, [C.POINTER(C.c_uint64)]),
    "rt_nw_debug_counters": (C.c_int, [C.POINTER(C.c_uint64)]),
    "rt_nw_ctx_accel_info": (C.c_int, [C.c_void_p, _ip, _ip, _ip, _ip]),
    "rt_nw_render": (C.c_int, [C.c_void_p, C.POINTER(RtNwCamera)] + [C.c_int32] * 4 + [C.c_uint64, _fp]),
    "rt_nw_render_rows": (
        C.c_int,
        [C.c_void_p, C.POINTER(RtNwCamera)] + [C.c_int32] * 4 + [C.c_uint64] + [C.c_int32] * 3 + [C.c_void_p, C.c_void_p],
    ),
    "rt_ctx_last_schedule": (C.c_int, [C.c_void_p, _ip]),
    "rt_ctx_grid_info": (C.c_int, [C.c_void_p, _ip, _ip, _ip]),
    "rt_nw_ctx_last_segments": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "rt_nw_ctx_last_kernel": (C.c_int, [C.c_void_p, _ip]),
    "rt_nw_ctx_last_staging": (C.c_int, [C.c_void_p, _ip]),
    "rt_nw_debug_trace": (C.c_int, [C.c_void_p, C.POINTER(RtNwCamera)] + [C.c_int32] * 3 + [C.c_uint64] + [C.c_int32] * 3 + [_fp, C.c_int32, _ip]),
    "rt_nw_debug_hits": (C.c_int, [C.c_void_p, _fp, C.POINTER(C.c_uint64), C.c_int32, _ip, _fp, _ip]),
    # progressive passes of the Next-Week renderer
    "rt_nw_accum_reset": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "rt_nw_render_pass": (
        C.c_int,
        [C.c_void_p, C.POINTER(RtNwCamera)] + [C.c_int32] * 5 + [C.c_uint64] + [C.c_int32] * 3 + [C.c_void_p],
    ),
    "rt_nw_accum_resolve": (C.c_int, [C.c_void_p, C.c_void_p, _fp, C.c_void_p]),
    "rt_nw_accum_export": (C.c_int, [C.c_void_p, _lp, C.c_size_t, _ip]),
    "rt_nw_accum_import": (C.c_int, [C.c_void_p, _lp, C.c_size_t, C.c_int32]),
    "rt_nw_accum_save": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(RtNwCamera)] + [C.c_int32] * 4 + [C.c_uint64]),
    "rt_nw_accum_load": (
        C.c_int,
        [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(RtNwCamera)] + [C.c_int32] * 6 + [C.c_uint64, _ip],
    ),
    "rt_nw_accum_info": (C.c_int, [C.c_char_p, _ip, C.POINTER(C.c_uint64)]),
    "rt_nw_scene_hash": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    # adaptive sampling of the Next-Week renderer
    "rt_nw_adapt_reset": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "rt_nw_adapt_pass": (
        C.c_int,
        [C.c_void_p, C.POINTER(RtNwCamera)] + [C.c_int32] * 4 + [C.c_uint64] + [C.c_int32] * 3 + [C.POINTER(C.c_uint8), C.c_void_p],
    ),
    "rt_nw_adapt_export": (C.c_int, [C.c_void_p, _lp, C.POINTER(C.c_uint64), _ip, C.c_size_t]),
    "rt_nw_adapt_import": (C.c_int, [C.c_void_p, _lp, C.POINTER(C.c_uint64), _ip, C.c_size_t]),
    "rt_nw_adapt_resolve": (C.c_int, [C.c_void_p, C.c_void_p, _fp, C.c_void_p]),
    "rt_nw_adapt_criterion": (
        C.c_int,
        [_lp, C.POINTER(C.c_uint64), _ip] + [C.c_int32] * 4 + [C.c_double, C.c_double, C.c_int32, C.POINTER(C.c_uint8), _dp, _lp],
    ),
    "rt_nw_render_adaptive": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.POINTER(RtNwCamera)] + [C.c_int32] * 5 + [C.c_double, C.c_double, C.c_int32, C.c_int32,
                                                                             C.c_uint64, C.c_char_p, C.c_double, _fp, _ip, _dp,
                                                                             C.POINTER(RtNwAdaptStats), NW_ADAPT_ON_PASS,
                                                                             C.c_void_p],
    ),
    "rt_nw_adapt_save": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(RtNwCamera)] + [C.c_int32] * 4 + [C.c_uint64]),
    "rt_nw_adapt_load": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(RtNwCamera)] + [C.c_int32] * 6 + [C.c_uint64]),
    "rt_nw_adapt_info": (C.c_int, [C.c_char_p, _ip, C.POINTER(C.c_uint64)]),
    # denoising of the Next-Week renderer
    "rt_nw_render_features": (C.c_int, [C.c_void_p, C.POINTER(RtNwCamera)] + [C.c_int32] * 3 + [C.c_uint64, C.c_void_p, _fp, C.c_void_p]),
    "rt_nw_adapt_variance": (C.c_int, [_lp, C.POINTER(C.c_uint64), _ip, C.c_int32, C.c_int32, _fp]),
    "rt_nw_denoise_params_default": (C.c_int, [C.POINTER(RtNwDenoiseParams)]),
    "rt_nw_denoise_params_check": (C.c_int, [C.POINTER(RtNwDenoiseParams)]),
    "rt_nw_denoise": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtNwDenoiseParams),
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "rt_nw_denoise_host": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _fp, _fp, _fp, C.POINTER(RtNwDenoiseParams), _fp, _fp]),
    "rt_nw_render_denoised": (
        C.c_int,
        [C.c_void_p, C.c_void_p, C.POINTER(RtNwCamera)] + [C.c_int32] * 5 + [C.c_double, C.c_double, C.c_int32, C.c_int32,
                                                                             C.c_uint64, C.c_char_p, C.c_double, _fp, _ip, _dp,
                                                                             C.POINTER(RtNwAdaptStats), NW_ADAPT_ON_PASS,
                                                                             C.c_void_p, C.c_int32, C.POINTER(RtNwDenoiseParams), _fp],
    ),
}

_lib = None


def load():
    """Load librtmi.so once; raises if it has not been built."""
    global _lib
    if _lib is None:
        # One HIP runtime per process: torch's wheel bundles libamdhip64 /
        # libhsa-runtime64 / librccl under the same SONAMEs as /opt/rocm.  If
        # torch is importable, load it first so librtmi.so binds to the copy
        # already in the process (device pointers and streams are then shared
        # with torch); loading ours first would leave torch a second runtime.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"librtmi.so not built at {LIB_PATH}: run `make -C a_dive_into_ray_tracing_amd/csrc`")
        L = C.CDLL(LIB_PATH)
        override = bool(os.environ.get("RTMI_LIBRARY"))  # an A/B build of an older tree may lack newer symbols
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name, None)
            if fn is None:
                if override:
                    continue
                raise ImportError(f"{LIB_PATH} does not export {name} (rebuild it)")
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what):
    if rc != RT_OK:
        raise RTError(what, rc, load().rt_last_error().decode(errors="replace"))
    return rc
