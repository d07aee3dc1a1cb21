"""gsrt -- Python host mirror of the C ABI in include/gsrt.h (ctypes over gsrt/libgsrt.so).

Mirrors the reference's scene / camera / dispatch / frame-dump interface for the Gaussian render path
(SURVEY.md §8b): `Scene.from_params` ~ Assets::Scene packing (Scene.cpp:16-182), `Scene.from_model` ~
Model::CreateGauss (Model.cpp:550-564), `Scene.build_bvh` ~ the TLAS build, `Scene.render` ~
vkCmdTraceRaysKHR(W,H,1) over GaussTracing.rgen, `dump_ppm` ~ VulkanRayTracing::image_store.

Errors raise GsrtError carrying the C status. The native library is required: importing this module
without a built libgsrt.so raises ImportError (there is no CPU fallback in the product path).
"""
from __future__ import annotations

import ctypes
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSRT_LIB_PATH") or os.path.join(_HERE, "libgsrt.so")  # override: A/B builds

OK, E_ARG, E_OOM, E_DEVICE, E_IO, E_STATE, E_COMM = 0, -1, -2, -3, -4, -5, -6
PAGE_GAUSSIANS = 4096  # GSRT_PAGE_GAUSSIANS
MODE_REF, MODE_COR = 0, 1
FLAG_LUT, FLAG_STATS, FLAG_OUT_DUMP8, FLAG_DEPTH, FLAG_FEATURES = 0x100, 0x200, 0x400, 0x800, 0x1000
FLAG_FEATURE_GRAD = 0x2000
FLAG_SH_GRAD = 0x4000
FLAG_OPACITY_GRAD = 0x8000
FLAG_SPLAT_GRAD = 0x20000
FLAG_SPLAT_DEPTH_GRAD = 0x80000
MAX_FEATURES = 16  # GSRT_MAX_FEATURES
DUMP8_ESCAPE = 1 << 30  # GSRT_DUMP8_ESCAPE
SYNTH_COR, SYNTH_REF, SYNTH_NEEDLE = 0, 1, 2

UBO_DTYPE = np.dtype([
    ("model_view", "<f4", 16), ("projection", "<f4", 16),
    ("model_view_inverse", "<f4", 16), ("projection_inverse", "<f4", 16),
    ("light_position", "<f4", 3), ("light_radius", "<f4"), ("aperture", "<f4"),
    ("focus_distance", "<f4"), ("heatmap_scale", "<f4"),
    ("total_samples", "<u4"), ("samples", "<u4"), ("bounces", "<u4"), ("shadows", "<u4"),
    ("random_seed", "<u4"), ("width", "<u4"), ("height", "<u4"), ("has_sky", "<u4"),
    ("show_heatmap", "<u4"),
])
RAYSTATE_DTYPE = np.dtype([("trans", "<f4"), ("depth", "<f4"), ("gauss_num", "<i4"),
                           ("gauss_num_raw", "<i4"), ("k", "<f4", (8, 2))])
ESCAPE_DTYPE = np.dtype([("pixel", "<u4"), ("r", "<f4"), ("g", "<f4"), ("b", "<f4")])  # gsrt_dump8_escape
assert UBO_DTYPE.itemsize == 320 and RAYSTATE_DTYPE.itemsize == 80 and ESCAPE_DTYPE.itemsize == 16

# every symbol include/gsrt.h (the drop-in ABI) and include/gsrt_test.h (test and measurement hooks) declare (tests check
# the library exports all of them)
EXPORTS = [
    "gsrt_status_string", "gsrt_abi_version", "gsrt_create", "gsrt_destroy", "gsrt_last_error",
    "gsrt_synchronize", "gsrt_stream", "gsrt_prep_stream", "gsrt_update_stream", "gsrt_slot_streams", "gsrt_scene_from_params", "gsrt_scene_from_model",
    "gsrt_scene_download", "gsrt_scene_size", "gsrt_destroy_scene", "gsrt_camera_from_modelview",
    "gsrt_camera_from_file", "gsrt_lookat", "gsrt_build_bvh", "gsrt_refit_bvh", "gsrt_scene_update", "gsrt_scene_attach",
    "gsrt_scene_detach", "gsrt_bvh_info",
    "gsrt_bvh_download", "gsrt_render", "gsrt_render_async", "gsrt_framebuffer", "gsrt_last_stats",
    "gsrt_comm_unique_id", "gsrt_comm_init", "gsrt_comm_stream", "gsrt_render_sharded", "gsrt_render_sharded_async",
    "gsrt_dump_ppm", "gsrt_reference_ppm_name", "gsrt_dump_image_binary", "gsrt_synth_cloud",
    "gsrt_timing", "gsrt_timing_read", "gsrt_tile_plan", "gsrt_render_sharded_emulated",
    "gsrt_debug_counters", "gsrt_debug_counters_hi", "gsrt_exp_lut", "gsrt_debug_exp_lut", "gsrt_ply_info",
    "gsrt_ply_read", "gsrt_scene_from_ply", "gsrt_dump_rgba_text", "gsrt_scene_add_mesh", "gsrt_scene_mesh_triangles",
    "gsrt_sphere_mesh", "gsrt_scene_stream_pages", "gsrt_scene_pages", "gsrt_host_register", "gsrt_host_unregister",
    "gsrt_vs_stats", "gsrt_dump_vs_stats", "gsrt_tile_pack_host", "gsrt_tile_unpack_host",
    "gsrt_timing_read_exchange", "gsrt_comm_size", "gsrt_debug_gathered", "gsrt_tile_bands", "gsrt_timing_kernel_only",
    "gsrt_set_bands", "gsrt_last_bands", "gsrt_row_costs", "gsrt_dump8_read", "gsrt_dump8_encode", "gsrt_dump8_ppm",
    "gsrt_render_sharded_emulated_dump8", "gsrt_debug_share_costs", "gsrt_debug_row_profile", "gsrt_debug_streams", "gsrt_deal_units", "gsrt_dump8_layout",
    "gsrt_tile_pack_dump8_host", "gsrt_tile_unpack_dump8_host", "gsrt_timing_stride", "gsrt_partition_hash",
    "gsrt_decide_bands", "gsrt_render_depth", "gsrt_render_depth_async", "gsrt_depth_buffer", "gsrt_dump_pfm",
    "gsrt_scene_set_features", "gsrt_scene_features", "gsrt_render_features", "gsrt_render_features_async",
    "gsrt_feature_buffer", "gsrt_render_feature_grad", "gsrt_render_feature_grad_async", "gsrt_group_order",
    "gsrt_unit_order", "gsrt_scene_set_sh", "gsrt_render_sh_grad", "gsrt_render_sh_grad_async",
    "gsrt_render_opacity_grad", "gsrt_render_opacity_grad_async", "gsrt_debug_frame_refusal",
    "gsrt_render_splat_grad", "gsrt_render_splat_grad_async", "gsrt_splat_grad_to_model", "gsrt_splat_grad_to_model_async",
    "gsrt_debug_frame_refusal_kind", "gsrt_render_splat_depth_grad", "gsrt_render_splat_depth_grad_async",
    "gsrt_splat_depth_grad_to_model", "gsrt_splat_depth_grad_to_model_async", "gsrt_debug_frame_refusal_any",
    "gsrt_density_stats_add", "gsrt_density_stats_add_async", "gsrt_densify_count", "gsrt_densify", "gsrt_densify_async",
    "gsrt_image_loss", "gsrt_image_loss_async", "gsrt_image_loss_window", "gsrt_frame_loss", "gsrt_frame_loss_async",
    "gsrt_adam_scalars", "gsrt_model_step", "gsrt_model_step_async", "gsrt_model_activate", "gsrt_model_activate_async",
    "gsrt_model_deactivate", "gsrt_model_deactivate_async", "gsrt_model_opacity_reset", "gsrt_model_opacity_reset_async",
    "gsrt_pose_grad", "gsrt_pose_grad_async", "gsrt_pose_twist", "gsrt_ubo_apply_twist", "gsrt_debug_pose_grad_layout",
    "gsrt_normal_noise", "gsrt_normal_noise_async", "gsrt_debug_philox", "gsrt_model_remap", "gsrt_model_remap_async",
    "gsrt_ply_write", "gsrt_lr_expon", "gsrt_trainer_create", "gsrt_trainer_destroy", "gsrt_trainer_step",
    "gsrt_trainer_densify", "gsrt_trainer_opacity_reset", "gsrt_trainer_rebuild_bvh", "gsrt_trainer_scene",
    "gsrt_trainer_info", "gsrt_trainer_state", "gsrt_trainer_download", "gsrt_view_stats_add", "gsrt_view_stats_add_async",
    "gsrt_densify_screen", "gsrt_densify_screen_async", "gsrt_densify_screen_count", "gsrt_model_step_degree",
    "gsrt_model_step_degree_async", "gsrt_trainer_densify_screen", "gsrt_trainer_set_sh_degree", "gsrt_trainer_sh_degree",
    "gsrt_trainer_radii",
]


class GsrtError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"gsrt status {status}: {msg}")
        self.status = status


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"gsrt native library not built: {LIB_PATH} (run __graft_entry__.build() or make)")
    L = ctypes.CDLL(LIB_PATH)
    P, u32, i32, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_float
    PP = ctypes.POINTER(ctypes.c_void_p)
    sig = {
        "gsrt_status_string": ([i32], ctypes.c_char_p),
        "gsrt_abi_version": ([], i32),
        "gsrt_create": ([PP, i32], i32),
        "gsrt_destroy": ([P], None),
        "gsrt_last_error": ([P], ctypes.c_char_p),
        "gsrt_synchronize": ([P], i32),
        "gsrt_stream": ([P], P),
        "gsrt_prep_stream": ([P], P),
        "gsrt_update_stream": ([P], P),
        "gsrt_slot_streams": ([P], i32),
        "gsrt_scene_from_params": ([P, P, P, u32, P, PP], i32),
        "gsrt_scene_from_model": ([P, P, P, P, P, P, u32, PP], i32),
        "gsrt_scene_download": ([P, P, P], i32),
        "gsrt_scene_size": ([P], u32),
        "gsrt_destroy_scene": ([P], None),
        "gsrt_camera_from_modelview": ([P, f32, u32, u32, f32, u32, u32, P], i32),
        "gsrt_camera_from_file": ([ctypes.c_char_p, f32, u32, u32, f32, u32, u32, P], i32),
        "gsrt_lookat": ([P, P, P, P], i32),
        "gsrt_build_bvh": ([P], i32),
        "gsrt_refit_bvh": ([P, P], i32),
        "gsrt_scene_update": ([P, P, P], i32),
        "gsrt_scene_attach": ([P, P, P], i32),
        "gsrt_scene_detach": ([P], i32),
        "gsrt_ply_info": ([ctypes.c_char_p, P, P], i32),
        "gsrt_ply_read": ([ctypes.c_char_p, P, P, P, P, P], i32),
        "gsrt_scene_from_ply": ([P, ctypes.c_char_p, i32, PP], i32),
        "gsrt_dump_rgba_text": ([ctypes.c_char_p, P, u32, u32], i32),
        "gsrt_bvh_info": ([P, P, P, P], i32),
        "gsrt_bvh_download": ([P, P, P, P], i32),
        "gsrt_render": ([P, P, u32, u32, P, P], i32),
        "gsrt_render_async": ([P, P, u32, u32, P, P], i32),
        "gsrt_framebuffer": ([P], P),
        "gsrt_last_stats": ([P, P, P], i32),
        "gsrt_comm_unique_id": ([P], i32),
        "gsrt_comm_init": ([P, P, i32, i32], i32),
        "gsrt_comm_stream": ([P], P),
        "gsrt_render_sharded": ([P, P, u32, u32, P], i32),
        "gsrt_render_sharded_async": ([P, P, u32, u32], i32),
        "gsrt_dump_ppm": ([ctypes.c_char_p, P, u32, u32], i32),
        "gsrt_reference_ppm_name": ([ctypes.c_char_p, ctypes.c_size_t], i32),
        "gsrt_dump_image_binary": ([ctypes.c_char_p, P, u32, u32], i32),
        "gsrt_synth_cloud": ([u32, u32, u32, i32, P, P, P, P, P], i32),
        "gsrt_timing": ([P, u32], i32),
        "gsrt_timing_read": ([P, P, P, u32, P], i32),
        "gsrt_timing_read_exchange": ([P, P, u32, P], i32),
        "gsrt_timing_kernel_only": ([P, i32], i32),
        "gsrt_comm_size": ([P, P, P], i32),
        "gsrt_debug_gathered": ([P, P, ctypes.c_size_t], i32),
        "gsrt_tile_bands": ([P, u32, i32, P, P], i32),
        "gsrt_set_bands": ([P, i32, P], i32),
        "gsrt_last_bands": ([P, P, u32, P], i32),
        "gsrt_row_costs": ([P, P, u32, P], i32),
        "gsrt_tile_plan": ([P, u32, i32, i32, P], i32),
        "gsrt_debug_counters": ([P, P], i32),
        "gsrt_debug_counters_hi": ([P, P], i32),
        "gsrt_exp_lut": ([P], i32),
        "gsrt_debug_exp_lut": ([P, P], i32),
        "gsrt_render_sharded_emulated": ([P, P, u32, i32, P, P], i32),
        "gsrt_scene_add_mesh": ([P, P, u32, P, u32], i32),
        "gsrt_scene_mesh_triangles": ([P], u32),
        "gsrt_sphere_mesh": ([P, f32, P, P], i32),
        "gsrt_scene_stream_pages": ([P, P, P, P, u32], i32),
        "gsrt_scene_pages": ([P], u32),
        "gsrt_host_register": ([P, P, ctypes.c_size_t], i32),
        "gsrt_host_unregister": ([P, P], i32),
        "gsrt_vs_stats": ([P, P], i32),
        "gsrt_tile_pack_host": ([P, u32, i32, i32, P, P, P], i32),
        "gsrt_tile_unpack_host": ([P, u32, i32, P, P, P], i32),
        "gsrt_dump_vs_stats": ([P, ctypes.c_char_p], i32),
        "gsrt_dump8_read": ([P, P, P, u32, P], i32),
        "gsrt_dump8_encode": ([P, ctypes.c_size_t, P, P, u32, P], i32),
        "gsrt_dump8_ppm": ([ctypes.c_char_p, P, u32, u32, P, u32], i32),
        "gsrt_render_sharded_emulated_dump8": ([P, P, u32, i32, P, P, P, u32, P], i32),
        "gsrt_dump8_layout": ([P, u32, i32, P, P], i32),
        "gsrt_timing_stride": ([P, u32], i32),
        "gsrt_tile_pack_dump8_host": ([P, u32, i32, i32, P, P, P], i32),
        "gsrt_tile_unpack_dump8_host": ([P, u32, i32, P, P, P, P, u32, P], i32),
        "gsrt_debug_share_costs": ([P, i32], i32),
        "gsrt_partition_hash": ([P, u32, i32, P, i32, P], i32),
        "gsrt_decide_bands": ([P, u32, i32, P, i32, P, u32, P], i32),
        "gsrt_debug_row_profile": ([P, P, u32, P], i32),
        "gsrt_debug_streams": ([P, P, P], i32),
        "gsrt_deal_units": ([P, P, u32, P], i32),
        "gsrt_group_order": ([u32, u32, u32, u32, u32, u32, P, P], i32),
        "gsrt_unit_order": ([u32, u32, u32, u32, P], i32),
        "gsrt_render_depth": ([P, P, u32, u32, P, P], i32),
        "gsrt_render_depth_async": ([P, P, u32, u32, P, P], i32),
        "gsrt_depth_buffer": ([P], P),
        "gsrt_dump_pfm": ([ctypes.c_char_p, P, u32, u32, u32], i32),
        "gsrt_scene_set_features": ([P, P, u32], i32),
        "gsrt_scene_features": ([P], u32),
        "gsrt_render_features": ([P, P, u32, u32, P, P], i32),
        "gsrt_render_features_async": ([P, P, u32, u32, P, P], i32),
        "gsrt_feature_buffer": ([P], P),
        "gsrt_render_feature_grad": ([P, P, u32, u32, P, u32, P, i32], i32),
        "gsrt_render_feature_grad_async": ([P, P, u32, u32, P, u32, P, i32], i32),
        "gsrt_scene_set_sh": ([P, P], i32),
        "gsrt_render_sh_grad": ([P, P, u32, u32, P, P, i32], i32),
        "gsrt_render_sh_grad_async": ([P, P, u32, u32, P, P, i32], i32),
        "gsrt_render_opacity_grad": ([P, P, u32, u32, P, P, i32], i32),
        "gsrt_render_opacity_grad_async": ([P, P, u32, u32, P, P, i32], i32),
        "gsrt_debug_frame_refusal": ([u32, u32, u32, i32, u32, i32, i32, ctypes.c_char_p, ctypes.c_size_t], i32),
        "gsrt_debug_frame_refusal_kind": ([u32, u32, u32, i32, u32, i32, i32, ctypes.c_char_p, ctypes.c_size_t], i32),
        "gsrt_debug_frame_refusal_any": ([u32, u32, u32, i32, u32, i32, i32, ctypes.c_char_p, ctypes.c_size_t], i32),
        "gsrt_render_splat_grad": ([P, P, u32, u32, P, P, i32], i32),
        "gsrt_render_splat_grad_async": ([P, P, u32, u32, P, P, i32], i32),
        "gsrt_splat_grad_to_model": ([P, P, P, P, P, i32], i32),
        "gsrt_splat_grad_to_model_async": ([P, P, P, P, P, i32], i32),
        "gsrt_render_splat_depth_grad": ([P, P, u32, u32, P, P, P, i32], i32),
        "gsrt_render_splat_depth_grad_async": ([P, P, u32, u32, P, P, P, i32], i32),
        "gsrt_splat_depth_grad_to_model": ([P, P, P, P, P, i32], i32),
        "gsrt_splat_depth_grad_to_model_async": ([P, P, P, P, P, i32], i32),
        "gsrt_density_stats_add": ([P, u32, u32, u32, P, P], i32),
        "gsrt_density_stats_add_async": ([P, u32, u32, u32, P, P], i32),
        "gsrt_densify_count": ([P, u32, P, P, P, P, P], i32),
        "gsrt_densify": ([P, P, u32, P, P, P, P, P, u32, P], i32),
        "gsrt_densify_async": ([P, P, u32, P, P, P, P, P, u32, P], i32),
        "gsrt_image_loss": ([P, u32, u32, P, P, u32, f32, P, P], i32),
        "gsrt_image_loss_async": ([P, u32, u32, P, P, u32, f32, P, P], i32),
        "gsrt_image_loss_window": ([P], i32),
        "gsrt_frame_loss": ([P, u32, u32, P, P, u32, P, P, P, P, P, P, P], i32),
        "gsrt_frame_loss_async": ([P, u32, u32, P, P, u32, P, P, P, P, P, P, P], i32),
        "gsrt_adam_scalars": ([P, P], i32),
        "gsrt_model_step": ([P, u32, P, P, P, P, P, P, P, P, P], i32),
        "gsrt_model_step_async": ([P, u32, P, P, P, P, P, P, P, P, P], i32),
        "gsrt_model_activate": ([P, u32, P, P, P, P], i32),
        "gsrt_model_activate_async": ([P, u32, P, P, P, P], i32),
        "gsrt_model_deactivate": ([P, u32, P, P], i32),
        "gsrt_model_deactivate_async": ([P, u32, P, P], i32),
        "gsrt_model_opacity_reset": ([P, u32, P, P, P, f32], i32),
        "gsrt_model_opacity_reset_async": ([P, u32, P, P, P, f32], i32),
        "gsrt_pose_grad": ([P, P, P, i32, P], i32),
        "gsrt_pose_grad_async": ([P, P, P, i32, P], i32),
        "gsrt_pose_twist": ([P, P, P], i32),
        "gsrt_ubo_apply_twist": ([P, P], i32),
        "gsrt_debug_pose_grad_layout": ([P], i32),
        "gsrt_normal_noise": ([P, ctypes.c_uint64, ctypes.c_uint64, u32, P], i32),
        "gsrt_normal_noise_async": ([P, ctypes.c_uint64, ctypes.c_uint64, u32, P], i32),
        "gsrt_debug_philox": ([ctypes.c_uint64, u32, ctypes.c_uint64, ctypes.c_uint64, P], i32),
        "gsrt_model_remap": ([P, u32, P, P, P], i32),
        "gsrt_model_remap_async": ([P, u32, P, P, P], i32),
        "gsrt_ply_write": ([ctypes.c_char_p, u32, P], i32),
        "gsrt_lr_expon": ([f32, f32, f32, u32, u32, u32, P], i32),
        "gsrt_trainer_create": ([P, P, u32, u32, PP], i32),
        "gsrt_trainer_destroy": ([P], None),
        "gsrt_trainer_step": ([P, P, u32, P, u32, P, P, P, P, P], i32),
        "gsrt_trainer_densify": ([P, P, ctypes.c_uint64, P], i32),
        "gsrt_trainer_opacity_reset": ([P, f32], i32),
        "gsrt_trainer_rebuild_bvh": ([P], i32),
        "gsrt_trainer_scene": ([P, PP], i32),
        "gsrt_trainer_info": ([P, P, P, P], i32),
        "gsrt_trainer_state": ([P, P, P, P, P, PP], i32),
        "gsrt_trainer_download": ([P, P, P], i32),
        "gsrt_view_stats_add": ([P, P, P, P, P], i32),
        "gsrt_view_stats_add_async": ([P, P, P, P, P], i32),
        "gsrt_densify_screen": ([P, P, u32, P, P, P, P, f32, P, P, u32, P], i32),
        "gsrt_densify_screen_async": ([P, P, u32, P, P, P, P, f32, P, P, u32, P], i32),
        "gsrt_densify_screen_count": ([P, u32, P, P, P, P, P, f32, P], i32),
        "gsrt_model_step_degree": ([P, u32, P, P, P, P, P, u32, P, P, P, P], i32),
        "gsrt_model_step_degree_async": ([P, u32, P, P, P, P, P, u32, P, P, P, P], i32),
        "gsrt_trainer_densify_screen": ([P, P, f32, ctypes.c_uint64, P], i32),
        "gsrt_trainer_set_sh_degree": ([P, u32], i32),
        "gsrt_trainer_sh_degree": ([P, P], i32),
        "gsrt_trainer_radii": ([P, PP], i32),
    }
    for name, (args, res) in sig.items():
        # an experiment build named by GSRT_LIB_PATH (an older revision under A/B) may predate a symbol; the
        # product library must export every one
        if os.environ.get("GSRT_LIB_PATH") and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    return L


lib = _load()


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _check(status: int, ctx=None):
    if status != OK:
        msg = lib.gsrt_status_string(status).decode()
        if ctx is not None and ctx.handle:
            detail = lib.gsrt_last_error(ctx.handle).decode()
            if detail:
                msg = f"{msg}: {detail}"
        raise GsrtError(status, msg)


def _f32(a, shape):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.reshape(shape)


def _rgba_grad(what, ubo, grad_image):
    """an RGBA frame's upstream gradient as (H, W, 4) float32, contiguous: an (H, W, 3) one gets a zero alpha gradient"""
    g = np.asarray(grad_image, np.float32)
    if g.ndim != 3 or g.shape[:2] != (int(ubo["height"][0]), int(ubo["width"][0])) or g.shape[2] not in (3, 4):
        raise GsrtError(E_ARG, f"{what}: an (H, W, 4) or (H, W, 3) array")
    if g.shape[2] == 3:
        g = np.concatenate([g, np.zeros(g.shape[:2] + (1,), np.float32)], axis=2)
    return np.ascontiguousarray(g)


# ---------------------------------------------------------------- camera (RayTracer.cpp:38-65)

def lookat(eye, center, up=(0.0, 1.0, 0.0)) -> np.ndarray:
    out = np.zeros(16, np.float32)
    e, c, u = _f32(eye, 3), _f32(center, 3), _f32(up, 3)  # keep the buffers alive across the call
    _check(lib.gsrt_lookat(_p(e), _p(c), _p(u), _p(out)))
    return out


def translate(x, y, z) -> np.ndarray:
    """glm::translate(mat4(1), vec3(x, y, z)), column-major."""
    m = np.eye(4, dtype=np.float32)
    m[3, :3] = (x, y, z)
    return m.reshape(16)


def camera_from_modelview(mv, fovy_deg, width, height, focus_distance=1.0, samples=1, bounces=16) -> np.ndarray:
    ubo = np.zeros(1, UBO_DTYPE)
    m = _f32(mv, 16)
    _check(lib.gsrt_camera_from_modelview(_p(m), fovy_deg, width, height, focus_distance,
                                          samples, bounces, _p(ubo)))
    return ubo


def pose_twist(model_view, grad_model_view) -> np.ndarray:
    """gsrt_pose_twist: the gradient (dL/dv, dL/dw), (6,) float32, in the tangent space of a left perturbation
    MV' = exp(xi^) MV, from model_view and Scene.pose_grad's result (16 floats each, column-major, or (4, 4) arrays holding
    the same 16 floats in that order)."""
    mv, g = np.asarray(model_view, np.float32), np.asarray(grad_model_view, np.float32)
    if mv.size != 16 or g.size != 16:
        raise GsrtError(E_ARG, "pose_twist: model_view and grad_model_view hold 16 floats each")
    mv, g = np.ascontiguousarray(mv).reshape(16), np.ascontiguousarray(g).reshape(16)
    out = np.zeros(6, np.float32)
    _check(lib.gsrt_pose_twist(_p(mv), _p(g), _p(out)))
    return out


def ubo_apply_twist(ubo, twist) -> np.ndarray:
    """gsrt_ubo_apply_twist on a copy of `ubo`: model_view <- exp(xi^) model_view, model_view_inverse <- model_view_inverse
    exp(-xi^) for the twist xi = (v, w), 6 floats. A zero twist returns an identical copy."""
    if not isinstance(ubo, np.ndarray) or ubo.dtype != UBO_DTYPE or ubo.size != 1:
        raise GsrtError(E_ARG, "ubo_apply_twist: ubo is one UBO_DTYPE record")
    t = np.asarray(twist, np.float32)
    if t.size != 6:
        raise GsrtError(E_ARG, "ubo_apply_twist: a twist holds 6 floats")
    t = np.ascontiguousarray(t).reshape(6)
    out = ubo.copy()
    _check(lib.gsrt_ubo_apply_twist(_p(out), _p(t)))
    return out


def pose_grad_layout():
    """(chunk, lanes) of gsrt_pose_grad's summation (gsrt_debug_pose_grad_layout): the Gaussians per first-stage partial
    and the second stage's lane count"""
    out = np.zeros(2, np.uint32)
    _check(lib.gsrt_debug_pose_grad_layout(_p(out)))
    return int(out[0]), int(out[1])


def camera_from_file(path, fovy_deg, width, height, focus_distance=1.0, samples=1, bounces=16) -> np.ndarray:
    ubo = np.zeros(1, UBO_DTYPE)
    _check(lib.gsrt_camera_from_file(os.fsencode(path), fovy_deg, width, height, focus_distance, samples,
                                     bounces, _p(ubo)))
    return ubo


# ---------------------------------------------------------------- frame dump / synthetic inputs

def dump_ppm(path, rgba):
    rgba = np.ascontiguousarray(rgba, np.float32)
    h, w = rgba.shape[:2]
    _check(lib.gsrt_dump_ppm(os.fsencode(path), _p(rgba), w, h))


def dump_pfm(path, img):
    """Portable float map of an (H, W) or (H, W, 1) image ("Pf") or an (H, W, 3) one ("PF"), e.g. a depth image:
    scale -1.0 (little-endian float32), rows bottom to top (gsrt_dump_pfm)"""
    img = np.ascontiguousarray(img, np.float32)
    if img.ndim not in (2, 3):
        raise GsrtError(E_ARG, "dump_pfm: an (H, W) or (H, W, channels) image")
    h, w = img.shape[:2]
    _check(lib.gsrt_dump_pfm(os.fsencode(path), _p(img), w, h, 1 if img.ndim == 2 else img.shape[2]))


def dump8_encode(rgba):
    """(codes[H, W] uint32, escapes ESCAPE_DTYPE) of an RGBA32F frame: what GSRT_FLAG_OUT_DUMP8 exchanges"""
    rgba = np.ascontiguousarray(rgba, np.float32)
    H, W = rgba.shape[:2]
    codes = np.zeros((H, W), np.uint32)
    n = np.zeros(1, np.uint32)
    _check(lib.gsrt_dump8_encode(_p(rgba), W * H, _p(codes), None, 0, _p(n)))
    esc = np.zeros(int(n[0]), ESCAPE_DTYPE)
    _check(lib.gsrt_dump8_encode(_p(rgba), W * H, _p(codes), _p(esc), esc.size, _p(n)))
    return codes, esc


def dump8_ppm(path, codes, esc):
    """the P3 PPM of a frame in dump codes + escapes (the bytes dump_ppm writes for the same frame)"""
    codes = np.ascontiguousarray(codes, np.uint32)
    esc = np.ascontiguousarray(esc, ESCAPE_DTYPE)
    H, W = codes.shape
    _check(lib.gsrt_dump8_ppm(os.fsencode(path), _p(codes), W, H, _p(esc) if esc.size else None, esc.size))


def dump_image_binary(path, rgba):
    rgba = np.ascontiguousarray(rgba, np.float32)
    h, w = rgba.shape[:2]
    _check(lib.gsrt_dump_image_binary(os.fsencode(path), _p(rgba), w, h))


def dump_rgba_text(path, rgba):
    """dump_image.sh text lines "[x, y] rgba(r, g, b)" (RayTracing.rgen:98)"""
    rgba = np.ascontiguousarray(rgba, np.float32)
    h, w = rgba.shape[:2]
    _check(lib.gsrt_dump_rgba_text(os.fsencode(path), _p(rgba), w, h))


def ply_info(path) -> dict:
    n = np.zeros(1, np.uint32)
    d = np.zeros(1, np.uint32)
    _check(lib.gsrt_ply_info(os.fsencode(path), _p(n), _p(d)))
    return {"n": int(n[0]), "sh_degree": int(d[0])}


def ply_read(path, with_sh=True):
    """3DGS .ply -> (center, rot_rxyz, scale, opacity, sh|None) in the gsrt_scene_from_model convention"""
    n = ply_info(path)["n"]
    c = np.zeros((n, 3), np.float32)
    r = np.zeros((n, 4), np.float32)
    s = np.zeros((n, 3), np.float32)
    o = np.zeros(n, np.float32)
    sh = np.zeros((n, 48), np.float32) if with_sh else None
    _check(lib.gsrt_ply_read(os.fsencode(path), _p(c), _p(r), _p(s), _p(o), _p(sh)))
    return c, r, s, o, sh


def reference_ppm_name() -> str:
    buf = ctypes.create_string_buffer(64)
    _check(lib.gsrt_reference_ppm_name(buf, 64))
    return buf.value.decode()


def exp_lut() -> np.ndarray:
    """The REF ExpLUT as the host library computes it (256 x {k, b})."""
    out = np.zeros(512, np.float32)
    _check(lib.gsrt_exp_lut(_p(out)))
    return out


def synth_cloud(kind, n, seed=42, with_sh=False):
    c = np.zeros((n, 3), np.float32)
    r = np.zeros((n, 4), np.float32)
    s = np.zeros((n, 3), np.float32)
    o = np.zeros(n, np.float32)
    sh = np.zeros((n, 16, 3), np.float32) if with_sh else None
    _check(lib.gsrt_synth_cloud(kind, n, seed, int(with_sh), _p(c), _p(r), _p(s), _p(o), _p(sh)))
    return c, r, s, o, sh


def sphere_mesh(center, radius):
    """Model::CreateSphere geometry (Model.cpp:566-629): vertices (561, 3) f32, indices (1024, 3) u32"""
    c = np.asarray(center, np.float32)
    v = np.zeros((561, 3), np.float32)
    i = np.zeros((1024, 3), np.uint32)
    _check(lib.gsrt_sphere_mesh(_p(c), float(radius), _p(v), _p(i)))
    return v, i


def tile_plan(ubo, mode=MODE_COR, nranks=1, rank=0) -> dict:
    """the frame's tiles under the even partition (gsrt_tile_plan)"""
    out = np.zeros(8, np.uint32)
    _check(lib.gsrt_tile_plan(_p(ubo), mode, nranks, rank, _p(out)))
    return dict(zip(["tile_w", "tile_h", "tiles_x", "tiles_y", "local_tiles", "spp_lanes", "row0", "stride"],
                    (int(v) for v in out)))


def _bands_arg(bands):
    return None if bands is None else np.ascontiguousarray(bands, np.uint32)


def tile_bands(ubo, nranks, row_cost=None, mode=MODE_COR) -> np.ndarray:
    """the partition's nranks + 1 tile-row boundaries the balancing rule cuts from a row cost profile (None: even)"""
    out = np.zeros(nranks + 1, np.uint32)
    rc = None if row_cost is None else np.ascontiguousarray(row_cost, np.uint32)
    _check(lib.gsrt_tile_bands(_p(ubo), mode, nranks, _p(rc), _p(out)))
    return out


def partition_hash(ubo, nranks, bands, pinned=False, mode=MODE_COR) -> int:
    """the partition hash a rank's cost profile carries for `bands` (gsrt_partition_hash)"""
    out = np.zeros(1, np.uint32)
    b = np.ascontiguousarray(bands, np.uint32)
    _check(lib.gsrt_partition_hash(_p(ubo), mode, nranks, _p(b), 1 if pinned else 0, _p(out)))
    return int(out[0])


def decide_bands(ubo, nranks, bands, profile, my_hash, pinned=False, mode=MODE_COR) -> np.ndarray:
    """the bands every rank adopts from an all-reduced profile (tiles_y row costs, then max(h), max(~h) of the ranks'
    partition hashes): gsrt_decide_bands, GsrtError(E_COMM) when the ranks' hashes differ"""
    out = np.zeros(nranks + 1, np.uint32)
    b = np.ascontiguousarray(bands, np.uint32)
    pr = np.ascontiguousarray(profile, np.uint32)
    _check(lib.gsrt_decide_bands(_p(ubo), mode, nranks, _p(b), 1 if pinned else 0, _p(pr), my_hash & 0xffffffff, _p(out)))
    return out


def deal_units(cost, centre=None) -> np.ndarray:
    """a rank share's render-unit deal over the 8 XCDs (gsrt_deal_units): perm[k * 8 + x] = XCD x's k-th unit"""
    c = np.ascontiguousarray(cost, np.float64)
    ctr = np.arange(c.size, dtype=np.uint32) if centre is None else np.ascontiguousarray(centre, np.uint32)
    out = np.zeros(c.size, np.uint32)
    _check(lib.gsrt_deal_units(_p(c), _p(ctr), c.size, _p(out)))
    return out


def group_order(groups_x, groups_y, fg, row0, row1, nranks):
    """k_group_list's dispatch order over groups_x x groups_y tile groups of fg x fg tiles (gsrt_group_order): (ord, own),
    the first own entries of ord being the groups with a tile row of the band [row0, row1)"""
    ord_ = np.zeros(groups_x * groups_y, np.uint32)
    own = ctypes.c_uint32(0)
    _check(lib.gsrt_group_order(groups_x, groups_y, fg, row0, row1, nranks, _p(ord_), ctypes.byref(own)))
    return ord_, int(own.value)


def unit_order(units, row0, row1, tiles_x) -> np.ndarray:
    """the centre-out order of a rank share's render units of 64 local tiles of the band [row0, row1) (gsrt_unit_order)"""
    out = np.zeros(units, np.uint32)
    _check(lib.gsrt_unit_order(units, row0, row1, tiles_x, _p(out)))
    return out


def tile_stride(ubo, nranks, bands=None, mode=MODE_COR) -> int:
    """the packed stride (the largest band's tile count) of a partition"""
    pl = tile_plan(ubo, mode, nranks, 0)
    if bands is None:
        return pl["stride"]
    return int(np.diff(np.asarray(bands, np.int64)).max()) * pl["tiles_x"]


def tile_pack(ubo, rgba, nranks, rank, mode=MODE_COR, bands=None) -> np.ndarray:
    """rank's tiles of an (H, W, 4) f32 frame in the packed layout of its sharded render (gsrt_tile_pack_host)"""
    pl = tile_plan(ubo, mode, nranks, rank)
    out = np.zeros((tile_stride(ubo, nranks, bands, mode), pl["tile_w"] * pl["tile_h"], 4), np.float32)
    src = np.ascontiguousarray(rgba, np.float32)
    b = _bands_arg(bands)
    _check(lib.gsrt_tile_pack_host(_p(ubo), mode, nranks, rank, _p(b), _p(src), _p(out)))
    return out


def tile_unpack(ubo, gathered, nranks, mode=MODE_COR, bands=None) -> np.ndarray:
    """the frame from all ranks' packed blocks (nranks, stride, tile_w * tile_h, 4), as k_unpack builds it"""
    W, H = int(ubo["width"][0]), int(ubo["height"][0])
    out = np.zeros((H, W, 4), np.float32)
    g = np.ascontiguousarray(gathered, np.float32)
    b = _bands_arg(bands)
    _check(lib.gsrt_tile_unpack_host(_p(ubo), mode, nranks, _p(b), _p(g), _p(out)))
    return out


def dump8_layout(ubo, nranks, bands=None, mode=MODE_COR) -> dict:
    """a rank's GSRT_FLAG_OUT_DUMP8 block: {"block": words, "codes": code words (the list header's offset),
    "cap": escape capacity} (gsrt_dump8_layout)"""
    out = np.zeros(3, np.uint64)
    b = _bands_arg(bands)
    _check(lib.gsrt_dump8_layout(_p(ubo), mode, nranks, _p(b), _p(out)))
    return dict(block=int(out[0]), codes=int(out[1]), cap=int(out[2]))


def tile_pack_dump8(ubo, rgba, nranks, rank, mode=MODE_COR, bands=None) -> np.ndarray:
    """rank's dump8 block (uint32 words) of an (H, W, 4) f32 frame, as its sharded render writes it
    (gsrt_tile_pack_dump8_host; raises when the frame's escapes overflow the block's list)"""
    L = dump8_layout(ubo, nranks, bands, mode)
    out = np.zeros(L["block"], np.uint32)
    src = np.ascontiguousarray(rgba, np.float32)
    b = _bands_arg(bands)
    _check(lib.gsrt_tile_pack_dump8_host(_p(ubo), mode, nranks, rank, _p(b), _p(src), _p(out)))
    return out


def tile_unpack_dump8(ubo, gathered, nranks, mode=MODE_COR, bands=None):
    """(codes[H, W] uint32, escapes in pixel order) from all ranks' dump8 blocks (nranks, block words), as rank 0
    unpacks them after the gather (gsrt_tile_unpack_dump8_host)"""
    W, H = int(ubo["width"][0]), int(ubo["height"][0])
    L = dump8_layout(ubo, nranks, bands, mode)
    codes = np.zeros((H, W), np.uint32)
    esc = np.zeros(L["cap"] * nranks, ESCAPE_DTYPE)
    n = np.zeros(1, np.uint32)
    g = np.ascontiguousarray(gathered, np.uint32)
    assert g.size == L["block"] * nranks
    b = _bands_arg(bands)
    _check(lib.gsrt_tile_unpack_dump8_host(_p(ubo), mode, nranks, _p(b), _p(g), _p(codes), _p(esc), esc.size, _p(n)))
    return codes, esc[: int(n[0])].copy()


def comm_unique_id() -> bytes:
    buf = np.zeros(128, np.uint8)
    _check(lib.gsrt_comm_unique_id(_p(buf)))
    return buf.tobytes()


# ---------------------------------------------------------------- adaptive density control

class ModelArrays(ctypes.Structure):
    """gsrt_model_arrays: addresses of a model's arrays in the gsrt_scene_from_model convention (0 / None: absent)"""
    _fields_ = [("center", ctypes.c_void_p), ("rot_rxyz", ctypes.c_void_p), ("scale", ctypes.c_void_p),
                ("opacity", ctypes.c_void_p), ("sh", ctypes.c_void_p), ("features", ctypes.c_void_p),
                ("feature_channels", ctypes.c_uint32)]


class DensifyParams(ctypes.Structure):
    """gsrt_densify_params"""
    _fields_ = [("grad_threshold", ctypes.c_float), ("split_scale", ctypes.c_float), ("min_opacity", ctypes.c_float),
                ("max_scale", ctypes.c_float), ("shrink", ctypes.c_float), ("reserved", ctypes.c_uint32 * 3)]


assert ctypes.sizeof(DensifyParams) == 32


def densify_params(grad_threshold, split_scale, min_opacity, max_scale=0.0, shrink=1.6) -> DensifyParams:
    """densify when the mean view-space gradient norm is >= grad_threshold: split when the largest scale is > split_scale,
    clone otherwise; prune unless opacity >= min_opacity, and when the largest scale is > max_scale (<= 0: no such test);
    a split child's scales are the parent's / shrink"""
    return DensifyParams(grad_threshold, split_scale, min_opacity, max_scale, shrink)


def _addr(a):
    return ctypes.c_void_p(a or None) if a is None or isinstance(a, int) else _p(a)


def density_stats_add(ctx, grad_splat, stats, width, height, n=None, asynchronous=False):
    """Add one view's densification statistic to stats (gsrt_density_stats_add): grad_splat the (n, 8) rows of
    Scene.splat_grad or Scene.splat_depth_grad for a width x height frame, stats an (n, 2) float32 array [sum, count],
    changed in place and returned: where any of a row's slots 0..5 is non-zero, sum += the norm of (row[0] width / 2,
    row[1] height / 2) and count += 1. Both numpy arrays, or both device addresses (int) with n given; asynchronous
    (device addresses only) enqueues on ctx.stream without waiting."""
    if isinstance(grad_splat, int) or isinstance(stats, int):
        if n is None:
            raise GsrtError(E_ARG, "density_stats_add: device addresses need n")
        fn = lib.gsrt_density_stats_add_async if asynchronous else lib.gsrt_density_stats_add
        _check(fn(ctx.handle, n, width, height, _addr(grad_splat), _addr(stats)), ctx)
        return stats
    if not (isinstance(stats, np.ndarray) and stats.dtype == np.float32 and stats.flags.c_contiguous and
            stats.ndim == 2 and stats.shape[1] == 2):
        raise GsrtError(E_ARG, "density_stats_add: stats is a C-contiguous (n, 2) float32 array, added to in place")
    rows = _f32(grad_splat, (stats.shape[0], 8))
    _check(lib.gsrt_density_stats_add(ctx.handle, stats.shape[0], width, height, _p(rows), _p(stats)), ctx)
    return stats


def view_stats_add(scene, ubo, grad_splat, stats, radii=None, asynchronous=False):
    """density_stats_add for a scene's Gaussians, with the largest screen radius beside it (gsrt_view_stats_add): stats
    (n, 2) gets exactly density_stats_add's bits for ubo's width and height; radii (n,), or None for the statistic alone,
    becomes max(radii, r) for every seen Gaussian the COR projection of ubo finds valid, r = ceil(3 sqrt(the larger
    eigenvalue of its 2-D covariance)) in pixels. All numpy float32 arrays changed in place, or all device addresses (int);
    asynchronous (device addresses only) enqueues on the ctx's stream without waiting. Returns (stats, radii)."""
    if isinstance(grad_splat, int) or isinstance(stats, int) or isinstance(radii, int):
        fn = lib.gsrt_view_stats_add_async if asynchronous else lib.gsrt_view_stats_add
        _check(fn(scene.handle, _p(ubo), _addr(grad_splat), _addr(stats), _addr(radii)), scene.ctx)
        return stats, radii
    n = scene.n
    for name, a, shape in (("stats", stats, (n, 2)), ("radii", radii, (n,))):
        if a is not None and not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous and
                                  a.shape == shape):
            raise GsrtError(E_ARG, f"view_stats_add: {name} is a C-contiguous float32 array of shape {shape}, changed in place")
    rows = _f32(grad_splat, (n, 8))
    _check(lib.gsrt_view_stats_add(scene.handle, _p(ubo), _p(rows), _p(stats), _p(radii)), scene.ctx)
    return stats, radii


def densify_count(ctx, scale, opacity, stats, params, n=None, radii=None, max_screen_radius=0.0) -> int:
    """the rows densify would write (gsrt_densify_count): scale (n, 3), opacity (n,), stats (n, 2) as numpy arrays or
    device addresses (int, with n given), params a DensifyParams. With radii (n,) (view_stats_add's) the screen-size prune
    takes part (gsrt_densify_screen_count): a Gaussian whose radius is > max_screen_radius (> 0) is pruned."""
    keep = []
    if n is None:
        n = np.asarray(opacity).reshape(-1).shape[0]

    def arg(x, shape):
        if x is None or isinstance(x, int):
            return _addr(x)
        keep.append(_f32(x, shape))
        return _p(keep[-1])
    out = ctypes.c_uint32(0)
    if radii is not None:
        _check(lib.gsrt_densify_screen_count(ctx.handle, n, arg(scale, (n, 3)), arg(opacity, (n,)), arg(stats, (n, 2)),
                                             ctypes.byref(params), arg(radii, (n,)), max_screen_radius, ctypes.byref(out)), ctx)
        return int(out.value)
    _check(lib.gsrt_densify_count(ctx.handle, n, arg(scale, (n, 3)), arg(opacity, (n,)), arg(stats, (n, 2)),
                                  ctypes.byref(params), ctypes.byref(out)), ctx)
    return int(out.value)


def densify(ctx, center, rot, scale, opacity, sh, stats, noise, params, features=None, *, n=None, feature_channels=0,
            out=None, origin=None, cap=None, d_n_out=None, radii=None, max_screen_radius=0.0):
    """Clone, split, prune or keep every Gaussian of a model and write the new one, in input order (gsrt_densify; the
    rule and the arithmetic are in gsrt.h). stats: (n, 2) from density_stats_add; noise: (n, 2, 3), the caller's normal
    draws for the two children of a split; params: a DensifyParams (densify_params).
    numpy arrays: center (n, 3), rot (n, 4), scale (n, 3), opacity (n,), sh (n, 16, 3) / (n, 48) or None, features
    (n, C) or None. Returns (center', rot', scale', opacity', sh' or None, features' or None, origin), each of n_out rows,
    sized with densify_count; origin[row] is g for Gaussian g itself and -1 - g for a row newly made from g.
    device addresses (int; sh / features 0 or None when absent): n, feature_channels, out = the six output addresses in
    the same order, origin and cap (rows of room) are needed. Blocks and returns n_out (GsrtError E_ARG when it exceeds
    cap: nothing was written then); with d_n_out, the device address of one uint32, the pass is only enqueued on
    ctx.stream (gsrt_densify_async) and None is returned.
    radii (n,) (view_stats_add's; a numpy array or a device address like the others) with max_screen_radius > 0: the
    screen-size prune (gsrt_densify_screen), a Gaussian whose radius is > max_screen_radius is pruned; radii=None is
    gsrt_densify itself."""
    screen = radii is not None
    if isinstance(center, int):
        if n is None or out is None or origin is None or cap is None:
            raise GsrtError(E_ARG, "densify: device addresses need n, out, origin and cap")
        a_in = ModelArrays(center, rot, scale, opacity, sh or None, features or None, feature_channels)
        a_out = ModelArrays(*[x or None for x in out], feature_channels)
        head = (ctx.handle, ctypes.byref(a_in), n, _addr(stats), _addr(noise), ctypes.byref(params))
        if screen:
            head += (_addr(radii), max_screen_radius)
        if d_n_out is not None:
            fn = lib.gsrt_densify_screen_async if screen else lib.gsrt_densify_async
            _check(fn(*head, ctypes.byref(a_out), _addr(origin), cap, _addr(d_n_out)), ctx)
            return None
        got = ctypes.c_uint32(0)
        fn = lib.gsrt_densify_screen if screen else lib.gsrt_densify
        _check(fn(*head, ctypes.byref(a_out), _addr(origin), cap, ctypes.byref(got)), ctx)
        return int(got.value)
    center = _f32(center, (-1, 3))
    n = center.shape[0]
    rot, scale, opacity = _f32(rot, (n, 4)), _f32(scale, (n, 3)), _f32(opacity, (n,))
    stats, noise = _f32(stats, (n, 2)), _f32(noise, (n, 2, 3))
    sh_shape = None if sh is None else np.asarray(sh).shape[1:]
    sh = None if sh is None else _f32(sh, (n, 48))
    features = None if features is None else _f32(features, (n, -1) if n else np.asarray(features).shape)
    fc = 0 if features is None else features.shape[1]
    radii = _f32(radii, (n,)) if screen else None
    rows = densify_count(ctx, scale, opacity, stats, params, radii=radii, max_screen_radius=max_screen_radius) if cap is None else cap
    o = [np.zeros((rows, 3), np.float32), np.zeros((rows, 4), np.float32), np.zeros((rows, 3), np.float32),
         np.zeros(rows, np.float32), None if sh is None else np.zeros((rows, 48), np.float32),
         None if features is None else np.zeros((rows, fc), np.float32)]
    org = np.zeros(rows, np.int32)
    a_in = ModelArrays(*[None if a is None else a.ctypes.data for a in (center, rot, scale, opacity, sh, features)], fc)
    a_out = ModelArrays(*[None if a is None else a.ctypes.data for a in o], fc)
    got = ctypes.c_uint32(0)
    head = (ctx.handle, ctypes.byref(a_in), n, _p(stats), _p(noise), ctypes.byref(params))
    if screen:
        head += (_p(radii), max_screen_radius)
    _check((lib.gsrt_densify_screen if screen else lib.gsrt_densify)(*head, ctypes.byref(a_out), _p(org), rows,
                                                                      ctypes.byref(got)), ctx)
    k = int(got.value)
    o = [None if a is None else a[:k] for a in o]
    if o[4] is not None:
        o[4] = o[4].reshape((k,) + tuple(sh_shape))
    return o[0], o[1], o[2], o[3], o[4], o[5], org[:k]


def image_loss_window() -> np.ndarray:
    """the 11 weights of image_loss's 1-D Gaussian window (sigma 1.5, sum 1) as float32 (gsrt_image_loss_window)"""
    out = np.zeros(11, np.float32)
    _check(lib.gsrt_image_loss_window(_p(out)))
    return out


def image_loss(ctx, rgba, target, lam=0.2, want_grad=True, *, width=None, height=None, target_channels=None, d_out=0,
               d_grad=0, asynchronous=False):
    """The photometric loss of a frame against a target image in one fused call (gsrt_image_loss; the formulas are in
    gsrt.h): loss = (1 - lam) l1 + lam (1 - ssim) with 3DGS's SSIM (11 x 11 Gaussian window, zero padding), and its
    gradient with respect to the frame.
    numpy arrays: rgba (H, W, 4) as Scene.render returns it, target (H, W, 3) or (H, W, 4). Returns (dict(loss=, l1=,
    ssim=, mse=), grad): grad is d loss / d rgba as (H, W, 4) float32 with a zero alpha slot, the grad_image that
    Scene.splat_grad, Scene.sh_grad and Scene.opacity_grad take, or None with want_grad=False.
    device addresses (int): width, height and target_channels are needed. With d_grad, the address of H x W x 4 floats,
    the gradient is written there (0: no gradient; want_grad is not read). Blocks and returns the dict. With d_out, the
    address of 4 floats, the scalars {loss, l1, ssim, mse} are written there instead and None is returned; then
    asynchronous=True only enqueues the call on ctx.stream (gsrt_image_loss_async) without waiting."""
    if isinstance(rgba, int) or isinstance(target, int):
        if width is None or height is None or target_channels is None:
            raise GsrtError(E_ARG, "image_loss: device addresses need width, height and target_channels")
        if asynchronous or d_out:
            _check(lib.gsrt_image_loss_async(ctx.handle, width, height, _addr(rgba), _addr(target), target_channels, lam,
                                             _addr(d_out), _addr(d_grad)), ctx)
            if not asynchronous:
                ctx.synchronize()
            return None
        out = np.zeros(4, np.float32)
        _check(lib.gsrt_image_loss(ctx.handle, width, height, _addr(rgba), _addr(target), target_channels, lam, _p(out),
                                   _addr(d_grad)), ctx)
        return dict(loss=float(out[0]), l1=float(out[1]), ssim=float(out[2]), mse=float(out[3]))
    x = np.ascontiguousarray(rgba, dtype=np.float32)
    y = np.ascontiguousarray(target, dtype=np.float32)
    if x.ndim != 3 or x.shape[2] != 4 or y.ndim != 3 or y.shape[:2] != x.shape[:2] or y.shape[2] not in (3, 4):
        raise GsrtError(E_ARG, "image_loss: rgba is an (H, W, 4) array and target an (H, W, 3) or (H, W, 4) one")
    out = np.zeros(4, np.float32)
    grad = np.zeros(x.shape, np.float32) if want_grad else None
    _check(lib.gsrt_image_loss(ctx.handle, x.shape[1], x.shape[0], _p(x), _p(y), y.shape[2], lam, _p(out), _p(grad)), ctx)
    return dict(loss=float(out[0]), l1=float(out[1]), ssim=float(out[2]), mse=float(out[3])), grad


LOSS_BACKGROUND = 1  # GSRT_LOSS_BACKGROUND
FRAME_LOSS_SCALARS = 6  # GSRT_FRAME_LOSS_SCALARS


class FrameLossParams(ctypes.Structure):
    """gsrt_frame_loss_params"""
    _fields_ = [("lam", ctypes.c_float), ("background", ctypes.c_float * 3), ("depth_weight", ctypes.c_float),
                ("alpha_min", ctypes.c_float), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


assert ctypes.sizeof(FrameLossParams) == 32


def frame_loss_params(lam=0.2, background=None, depth_weight=0.0, alpha_min=1.0 / 255.0, flags=None,
                      reserved=0) -> FrameLossParams:
    """a gsrt_frame_loss_params: lam the D-SSIM weight, background an (r, g, b) the frame is composited over (None: the
    frame as it is; otherwise LOSS_BACKGROUND is set), depth_weight the weight of the depth term, alpha_min the least
    alpha of a depth sample. flags / reserved: the struct's words as they are (flags None: from background). Nothing is
    checked here; frame_loss refuses what gsrt_frame_loss does."""
    bg = (0.0, 0.0, 0.0) if background is None else tuple(float(b) for b in background)
    if len(bg) != 3:
        raise GsrtError(E_ARG, "frame_loss_params: background is (r, g, b)")
    if flags is None:
        flags = 0 if background is None else LOSS_BACKGROUND
    return FrameLossParams(lam, (ctypes.c_float * 3)(*bg), depth_weight, alpha_min, flags, reserved)


def _frame_loss_refusal(P, width, height, channels, arrays, out, grads):
    """why gsrt_frame_loss would refuse these arguments, or None. arrays: addresses of (rgba, target, mask, depth,
    target_depth), 0 when absent; out: the scalars' address or 0; grads: (grad_image, grad_depth) addresses.
    The C call's own list (gsrt.h), checked here too so that a refusal needs no device."""
    rgba, target, mask, depth, target_depth = arrays
    gimg, gdepth = grads
    if not rgba or not target:
        return "rgba or target is NULL"
    if P is None:
        return "params is NULL"
    if not (1 <= width <= 32768 and 1 <= height <= 32768):
        return "width and height must be 1..32768"
    if channels not in (3, 4):
        return "target_channels must be 3 or 4"
    if not 0.0 <= P.lam <= 1.0:
        return "lam must be in [0, 1]"
    if P.flags & ~LOSS_BACKGROUND:
        return "an unknown flag"
    if P.reserved:
        return "reserved must be zero"
    if P.flags & LOSS_BACKGROUND and not all(np.isfinite(b) for b in P.background):
        return "background must be finite"
    if not P.depth_weight >= 0.0:
        return "depth_weight is negative or NaN"
    if not 0.0 < P.alpha_min <= 1.0:
        return "alpha_min must be in (0, 1]"
    if bool(depth) != bool(target_depth):
        return "depth and target_depth come together or not at all"
    if gdepth and (not depth or not gimg):
        return "grad_depth needs depth and grad_image"
    px = width * height
    ins = [(rgba, 16 * px), (target, 4 * channels * px), (mask, 4 * px), (depth, 4 * px), (target_depth, 4 * px)]
    outs = [(out, 4 * FRAME_LOSS_SCALARS), (gimg, 16 * px), (gdepth, 4 * px)]
    hit = lambda a, b: a[0] and b[0] and a[0] < b[0] + b[1] and b[0] < a[0] + a[1]  # noqa: E731
    for i, o in enumerate(outs):
        if any(hit(o, r) for r in ins) or any(hit(o, q) for q in outs[i + 1:]):
            return "an output overlaps an input or another output"
    return None


def frame_loss(ctx, rgba, target, *, mask=None, depth=None, target_depth=None, background=None, lam=0.2,
               depth_weight=0.0, alpha_min=1.0 / 255.0, want_grad=True, params=None, width=None, height=None,
               target_channels=None, d_out=0, d_grad=0, d_grad_depth=0, asynchronous=False):
    """The loss of a training frame in one fused call (gsrt_frame_loss; the formulas are in gsrt.h): image_loss of the
    frame composited over `background` ((r, g, b) or None) under the pixel weights `mask` ((H, W) or None), plus
    depth_weight times the mean over all pixels of mask |depth / alpha - target_depth|, taken where target_depth is
    finite and > 0 and alpha >= alpha_min. depth is the premultiplied (H, W) image of Scene.render_depth. params: a
    FrameLossParams used as it is, in place of background, lam, depth_weight and alpha_min.
    numpy arrays: returns (dict(loss=, l1=, ssim=, mse=, depth_l1=, depth_samples=), grad_image, grad_depth): the
    gradients with respect to rgba (H, W, 4; alpha slot included) and to depth (H, W; None without depth), which
    Scene.splat_grad and Scene.splat_depth_grad take as they are; both None with want_grad=False.
    device addresses (int, 0 / None for an absent mask, depth or target_depth): width, height and target_channels are
    needed; d_grad (H x W x 4 floats) and d_grad_depth (H x W floats) receive the gradients (0: none; want_grad is not
    read). Blocks and returns the dict. With d_out, the address of 6 floats, the scalars are written there and None is
    returned; then asynchronous=True only enqueues the call on ctx.stream (gsrt_frame_loss_async).
    Arrays and addresses cannot be mixed. Every refusal of the C call is raised here as GsrtError(E_ARG) first."""
    P = params if params is not None else frame_loss_params(lam, background, depth_weight, alpha_min)
    if not isinstance(P, FrameLossParams):
        raise GsrtError(E_ARG, "frame_loss: params is a FrameLossParams")
    given = [a for a in (rgba, target, mask, depth, target_depth) if a is not None]
    on_device = [isinstance(a, int) for a in given]
    if any(on_device):
        if not all(on_device):
            raise GsrtError(E_ARG, "frame_loss: host arrays and device addresses are mixed")
        if width is None or height is None or target_channels is None:
            raise GsrtError(E_ARG, "frame_loss: device addresses need width, height and target_channels")
        arrays = [int(a or 0) for a in (rgba, target, mask, depth, target_depth)]
        why = _frame_loss_refusal(P, width, height, target_channels, arrays, int(d_out or 0),
                                  (int(d_grad or 0), int(d_grad_depth or 0)))
        if why is None and (arrays[0] | int(d_grad or 0) | (arrays[1] if target_channels == 4 else 0)) % 16:
            why = "rgba, grad_image and a 4-channel target must be 16-byte aligned on the device"
        if why:
            raise GsrtError(E_ARG, "frame_loss: " + why)
        args = (width, height, _addr(arrays[0]), _addr(arrays[1]), target_channels, _addr(arrays[2]), _addr(arrays[3]),
                _addr(arrays[4]), ctypes.byref(P))
        if asynchronous or d_out:
            _check(lib.gsrt_frame_loss_async(ctx.handle, *args, _addr(d_out), _addr(d_grad), _addr(d_grad_depth)), ctx)
            if not asynchronous:
                ctx.synchronize()
            return None
        out = np.zeros(FRAME_LOSS_SCALARS, np.float32)
        _check(lib.gsrt_frame_loss(ctx.handle, *args, _p(out), _addr(d_grad), _addr(d_grad_depth)), ctx)
        return dict(zip(("loss", "l1", "ssim", "mse", "depth_l1", "depth_samples"), (float(v) for v in out)))
    if d_out or d_grad or d_grad_depth:
        raise GsrtError(E_ARG, "frame_loss: host arrays and device addresses are mixed")
    x = np.ascontiguousarray(rgba, dtype=np.float32)
    y = np.ascontiguousarray(target, dtype=np.float32)
    if x.ndim != 3 or x.shape[2] != 4 or y.ndim != 3 or y.shape[:2] != x.shape[:2] or y.shape[2] not in (3, 4):
        raise GsrtError(E_ARG, "frame_loss: rgba is an (H, W, 4) array and target an (H, W, 3) or (H, W, 4) one")
    planes = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (mask, depth, target_depth)]
    if any(a is not None and a.shape != x.shape[:2] for a in planes):
        raise GsrtError(E_ARG, "frame_loss: mask, depth and target_depth are (H, W) arrays")
    out = np.zeros(FRAME_LOSS_SCALARS, np.float32)
    grad = np.zeros(x.shape, np.float32) if want_grad else None
    gdepth = np.zeros(x.shape[:2], np.float32) if want_grad and planes[1] is not None else None
    addr = lambda a: 0 if a is None else a.ctypes.data  # noqa: E731
    why = _frame_loss_refusal(P, x.shape[1], x.shape[0], y.shape[2], [addr(x), addr(y)] + [addr(a) for a in planes],
                              addr(out), (addr(grad), addr(gdepth)))
    if why:
        raise GsrtError(E_ARG, "frame_loss: " + why)
    _check(lib.gsrt_frame_loss(ctx.handle, x.shape[1], x.shape[0], _p(x), _p(y), y.shape[2], _p(planes[0]), _p(planes[1]),
                               _p(planes[2]), ctypes.byref(P), _p(out), _p(grad), _p(gdepth)), ctx)
    return (dict(zip(("loss", "l1", "ssim", "mse", "depth_l1", "depth_samples"), (float(v) for v in out))), grad, gdepth)


# ---------------------------------------------------------------- the optimiser step

ADAM_SPARSE = 1  # GSRT_ADAM_SPARSE
ADAM_SCALARS = 10  # GSRT_ADAM_SCALARS


class AdamParams(ctypes.Structure):
    """gsrt_adam_params"""
    _fields_ = [("lr_center", ctypes.c_float), ("lr_rot", ctypes.c_float), ("lr_scale", ctypes.c_float),
                ("lr_opacity", ctypes.c_float), ("lr_sh_dc", ctypes.c_float), ("lr_sh_rest", ctypes.c_float),
                ("lr_features", ctypes.c_float), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float),
                ("eps", ctypes.c_float), ("step", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 4)]


class ModelGrads(ctypes.Structure):
    """gsrt_model_grads: addresses of the gradient tables as the library's backward writes them (0 / None: absent)"""
    _fields_ = [("center", ctypes.c_void_p), ("cov", ctypes.c_void_p), ("splat", ctypes.c_void_p),
                ("sh", ctypes.c_void_p), ("features", ctypes.c_void_p)]


assert ctypes.sizeof(AdamParams) == 64 and ctypes.sizeof(ModelGrads) == 40


def adam_params(lr_center=1.6e-4, lr_rot=1e-3, lr_scale=5e-3, lr_opacity=5e-2, lr_sh_dc=2.5e-3, lr_sh_rest=1.25e-4,
                lr_features=0.0, beta1=0.9, beta2=0.999, eps=1e-15, step=1, sparse=False) -> AdamParams:
    """a gsrt_adam_params; the defaults are 3DGS's rates (the caller schedules them: change lr_* and step per call). A
    rate of exactly 0 freezes its group; sparse: Gaussians no ray reached with a gradient keep raw, m and v (ADAM_SPARSE)"""
    return AdamParams(lr_center, lr_rot, lr_scale, lr_opacity, lr_sh_dc, lr_sh_rest, lr_features, beta1, beta2, eps, step,
                      ADAM_SPARSE if sparse else 0)


def adam_scalars(adam) -> np.ndarray:
    """the float32 scalars model_step's kernels use (gsrt_adam_scalars; no device needed): [1 - beta1, 1 - beta2,
    sqrt(1 - beta2^t), then lr / (1 - beta1^t) for center, rot, scale, opacity, sh_dc, sh_rest, features]"""
    out = np.zeros(ADAM_SCALARS, np.float32)
    _check(lib.gsrt_adam_scalars(ctypes.byref(adam), _p(out)))
    return out


_MODEL_SHAPES = ((3,), (4,), (3,), (), (48,), None)  # per Gaussian: center, rot, scale, opacity, sh, features (n, C)


def _model_set(what, arrays, n, writable):
    """(center, rot, scale, opacity, sh or None, features or None) as a ModelArrays. numpy arrays are passed by address
    (float32, C-contiguous; copies of other inputs are made only for arrays the call reads); ints are device addresses.
    Returns (struct, n, channels, keep-alive list, on the device?)."""
    arrays = tuple(arrays) + (None,) * (6 - len(arrays))
    dev = isinstance(arrays[0], int)
    keep, addr, fc = [], [], 0
    for a, shape in zip(arrays, _MODEL_SHAPES):
        if a is None or (isinstance(a, int) and a == 0):
            addr.append(None)
            continue
        if isinstance(a, int) != dev:
            raise GsrtError(E_ARG, f"{what}: numpy arrays or device addresses, not both")
        if dev:
            addr.append(a)
            continue
        if writable:
            if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous and a.flags.writeable):
                raise GsrtError(E_ARG, f"{what}: arrays changed in place are writable C-contiguous float32 arrays")
        else:
            a = np.ascontiguousarray(a, dtype=np.float32)
        if n is None:
            n = a.shape[0] if a.ndim else 1
        if shape is None:
            fc = a.size // n if n else (a.shape[1] if a.ndim == 2 else 0)
        want = n * (fc if shape is None else int(np.prod(shape, dtype=np.int64)))
        if a.size != want:
            raise GsrtError(E_ARG, f"{what}: an array of {a.size} floats where n = {n} needs {want}")
        keep.append(a)
        addr.append(a.ctypes.data)
    return addr, n, fc, keep, dev


def _new_model(n, src_addr, fc, sh_shape=(48,)):
    o = [np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32),
         None if src_addr[4] is None else np.zeros((n,) + tuple(sh_shape), np.float32),
         None if src_addr[5] is None else np.zeros((n, fc), np.float32)]
    return o


def model_step(ctx, raw, m, v, grads, adam, *, n=None, feature_channels=0, act=None, params_out=None, aabbs_out=None,
               grad_raw=None, want_act=True, want_grad_raw=False, asynchronous=False, sh_degree=3):
    """One optimiser step on the raw model (gsrt_model_step; the formulas are in gsrt.h): the gradient tables chained to the
    raw parameters, Adam, and the next frame's arrays. raw, m, v: (center (n, 3), rot (n, 4) unnormalised, log scale
    (n, 3), logit opacity (n,), sh (n, 48) / (n, 16, 3) or None, features (n, C) or None), the moments in the same layout,
    all updated in place. grads: (center (n, 3), cov (n, 6), splat (n, 8), sh or None, features or None) as Scene.model_grad,
    Scene.splat_grad, Scene.sh_grad and Scene.feature_grad return them. adam: an AdamParams (adam_params).
    numpy arrays: raw, m, v are writable C-contiguous float32 arrays. Returns dict(act=(center, rot, scale, opacity, sh,
    features) or None (want_act=False), params= (n, 12), aabbs= (n, 6) (as Scene.download returns them, for Scene.update), grad_raw= (n, 11)
    or None): act is the activated model, sh / features in it the stepped arrays themselves.
    device addresses (int; 0 or None when absent): n (and feature_channels) are needed; act = six addresses or None,
    params_out, aabbs_out, grad_raw addresses or None. Blocks and returns None; asynchronous=True only enqueues the call
    on ctx.stream (gsrt_model_step_async): synchronise before Scene.update / Scene.attach read params_out / aabbs_out.
    sh_degree (0..3): the active SH degree (gsrt_model_step_degree): the SH words from 3 (sh_degree + 1)^2 on keep their
    bits in raw, m and v; 3, the default, is gsrt_model_step itself."""
    r_addr, n, fc, k1, dev = _model_set("model_step: raw", raw, n, True)
    m_addr, _, fcm, k2, dev_m = _model_set("model_step: m", m, n, True)
    v_addr, _, fcv, k3, dev_v = _model_set("model_step: v", v, n, True)
    if n is None:
        raise GsrtError(E_ARG, "model_step: device addresses need n")
    grads = tuple(grads) + (None,) * (5 - len(grads))
    keep, g_addr = [], []
    for a, width in zip(grads, (3, 6, 8, 48, fc if not dev else feature_channels)):
        if a is None or (isinstance(a, int) and a == 0):
            g_addr.append(None)
        elif isinstance(a, int):
            g_addr.append(a)
        else:
            keep.append(_f32(a, (n, width)))
            g_addr.append(keep[-1].ctypes.data)
    if dev:
        fc = fcm = fcv = feature_channels
    s_raw, s_m, s_v = ModelArrays(*r_addr, fc), ModelArrays(*m_addr, fcm), ModelArrays(*v_addr, fcv)
    s_g = ModelGrads(*g_addr)
    if dev:
        s_act = None if act is None else ModelArrays(*[x or None for x in act], fc)
        head = (ctx.handle, n, ctypes.byref(s_raw), ctypes.byref(s_m), ctypes.byref(s_v), ctypes.byref(s_g), ctypes.byref(adam))
        if sh_degree != 3:
            fn = lib.gsrt_model_step_degree_async if asynchronous else lib.gsrt_model_step_degree
            head += (sh_degree,)
        else:
            fn = lib.gsrt_model_step_async if asynchronous else lib.gsrt_model_step
        _check(fn(*head, None if s_act is None else ctypes.byref(s_act), _addr(params_out), _addr(aabbs_out),
                  _addr(grad_raw)), ctx)
        return None
    out = _new_model(n, r_addr, fc) if want_act else None
    if out is not None:
        out[4], out[5] = (None if r_addr[4] is None else raw[4]), (None if r_addr[5] is None else raw[5])
        s_act = ModelArrays(*[None if a is None else a.ctypes.data for a in out], fc)
    params, aabbs = np.zeros((n, 12), np.float32), np.zeros((n, 6), np.float32)
    graw = np.zeros((n, 11), np.float32) if want_grad_raw else None
    head = (ctx.handle, n, ctypes.byref(s_raw), ctypes.byref(s_m), ctypes.byref(s_v), ctypes.byref(s_g), ctypes.byref(adam))
    fn = lib.gsrt_model_step
    if sh_degree != 3:
        fn, head = lib.gsrt_model_step_degree, head + (sh_degree,)
    _check(fn(*head, None if out is None else ctypes.byref(s_act), _p(params), _p(aabbs), _p(graw)), ctx)
    return dict(act=None if out is None else tuple(out), params=params, aabbs=aabbs, grad_raw=graw)


def model_activate(ctx, raw, *, n=None, feature_channels=0, act=None, params_out=None, aabbs_out=None, asynchronous=False):
    """The activation and packing of model_step alone (gsrt_model_activate), for step 0 and after a densify: raw =
    (center, rot, log scale, logit opacity, sh or None, features or None). numpy arrays: returns dict(act=(center, rot,
    scale, opacity, sh, features), params=, aabbs=); sh / features in act are copies. device addresses: n (and
    feature_channels) needed, act = six addresses or None, params_out / aabbs_out addresses or None; returns None."""
    r_addr, n, fc, keep, dev = _model_set("model_activate: raw", raw, n, False)
    if n is None:
        raise GsrtError(E_ARG, "model_activate: device addresses need n")
    if dev:
        fc = feature_channels
        s_raw = ModelArrays(*r_addr, fc)
        s_act = None if act is None else ModelArrays(*[x or None for x in act], fc)
        fn = lib.gsrt_model_activate_async if asynchronous else lib.gsrt_model_activate
        _check(fn(ctx.handle, n, ctypes.byref(s_raw), None if s_act is None else ctypes.byref(s_act), _addr(params_out),
                  _addr(aabbs_out)), ctx)
        return None
    s_raw = ModelArrays(*r_addr, fc)
    out = _new_model(n, r_addr, fc)
    s_act = ModelArrays(*[None if a is None else a.ctypes.data for a in out], fc)
    params, aabbs = np.zeros((n, 12), np.float32), np.zeros((n, 6), np.float32)
    _check(lib.gsrt_model_activate(ctx.handle, n, ctypes.byref(s_raw), ctypes.byref(s_act), _p(params), _p(aabbs)), ctx)
    return dict(act=tuple(out), params=params, aabbs=aabbs)


def model_deactivate(ctx, act, *, n=None, feature_channels=0, raw=None, asynchronous=False):
    """Activated to raw (gsrt_model_deactivate): what ply_read or densify return becomes the model model_step optimises;
    log scale = log(s), logit = log(o / (1 - o)), the rest copied. numpy arrays: returns (center, rot, log scale, logit,
    sh or None, features or None). device addresses: n (and feature_channels) and raw = six addresses are needed."""
    a_addr, n, fc, keep, dev = _model_set("model_deactivate: act", act, n, False)
    if n is None:
        raise GsrtError(E_ARG, "model_deactivate: device addresses need n")
    if dev:
        if raw is None:
            raise GsrtError(E_ARG, "model_deactivate: device addresses need raw")
        s_act, s_raw = ModelArrays(*a_addr, feature_channels), ModelArrays(*[x or None for x in raw], feature_channels)
        fn = lib.gsrt_model_deactivate_async if asynchronous else lib.gsrt_model_deactivate
        _check(fn(ctx.handle, n, ctypes.byref(s_act), ctypes.byref(s_raw)), ctx)
        return None
    out = _new_model(n, a_addr, fc)
    s_act = ModelArrays(*a_addr, fc)
    s_raw = ModelArrays(*[None if a is None else a.ctypes.data for a in out], fc)
    _check(lib.gsrt_model_deactivate(ctx.handle, n, ctypes.byref(s_act), ctypes.byref(s_raw)), ctx)
    return tuple(out)


def model_opacity_reset(ctx, logit, m, v, max_opacity=0.01, *, n=None, asynchronous=False):
    """3DGS's opacity reset on the raw model (gsrt_model_opacity_reset): logit = min(logit, log(max_opacity / (1 -
    max_opacity))) in place, both Adam moments of the opacities set to 0. Three writable float32 numpy arrays of n, or
    three device addresses with n given (asynchronous=True: enqueued on ctx.stream only)."""
    if isinstance(logit, int):
        if n is None:
            raise GsrtError(E_ARG, "model_opacity_reset: device addresses need n")
        fn = lib.gsrt_model_opacity_reset_async if asynchronous else lib.gsrt_model_opacity_reset
        _check(fn(ctx.handle, n, _addr(logit), _addr(m), _addr(v), max_opacity), ctx)
        return None
    for a in (logit, m, v):
        if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous and a.flags.writeable and
                a.size == logit.size):
            raise GsrtError(E_ARG, "model_opacity_reset: three writable C-contiguous float32 arrays of one size")
    _check(lib.gsrt_model_opacity_reset(ctx.handle, logit.size, _p(logit), _p(m), _p(v), max_opacity), ctx)
    return None


# ---------------------------------------------------------------- context / scene

class Context:
    """One gsrt_ctx per device (gsrt_create)."""

    def __init__(self, device: int = 0):
        h = ctypes.c_void_p()
        st = lib.gsrt_create(ctypes.byref(h), device)
        if st != OK:
            raise GsrtError(st, f"gsrt_create(device={device}) failed: {lib.gsrt_status_string(st).decode()}")
        self.handle = h
        self._scenes = weakref.WeakSet()

    def close(self):
        if getattr(self, "handle", None):
            for sc in list(self._scenes):
                sc.close()
            lib.gsrt_destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def synchronize(self):
        _check(lib.gsrt_synchronize(self.handle), self)

    @property
    def stream(self) -> int:
        return lib.gsrt_stream(self.handle) or 0

    @property
    def prep_stream(self) -> int:
        return lib.gsrt_prep_stream(self.handle) or 0

    @property
    def update_stream(self) -> int:
        """the stream of scene updates' copies (gsrt_update_stream): a GPU producer of an update's source fills it there"""
        return lib.gsrt_update_stream(self.handle) or 0

    def slot_streams(self) -> bool:
        """whether the last frame ran on slot streams (its prep and render kernels on its frame slot's stream)"""
        return bool(lib.gsrt_slot_streams(self.handle))

    @property
    def framebuffer_ptr(self) -> int:
        return lib.gsrt_framebuffer(self.handle) or 0

    def depth_ptr(self) -> int:
        """device address of the last frame's depth image (gsrt_depth_buffer); 0 when the last frame had none"""
        return lib.gsrt_depth_buffer(self.handle) or 0

    def features_ptr(self) -> int:
        """device address of the last frame's feature image (gsrt_feature_buffer); 0 when the last frame had none"""
        return lib.gsrt_feature_buffer(self.handle) or 0

    def last_stats(self, per_ray_shape=None):
        out = np.zeros(8, np.uint64)
        per = np.zeros(per_ray_shape + (4,), np.uint32) if per_ray_shape else None
        _check(lib.gsrt_last_stats(self.handle, _p(out), _p(per)), self)
        keys = ["rays", "candidates", "blended", "terminated", "tile_rounds", "restarts", "tiles", "max_tile_candidates"]
        d = {k: int(v) for k, v in zip(keys, out)}
        if per is not None:
            d["per_ray"] = per
        return d

    def vs_stats(self) -> dict:
        """vulkan-sim's rt_* statistics of the last REF render with FLAG_STATS (gsrt_vs_stats)"""
        out = np.zeros(8, np.uint64)
        _check(lib.gsrt_vs_stats(self.handle, _p(out)), self)
        keys = ["rt_n_total_rays", "rt_num_hits", "rt_max_tree_depth", "rt_max_nodes_per_ray", "rt_tot_nodes_per_ray",
                "overflowed_walks"]
        return {k: int(v) for k, v in zip(keys, out)}

    def dump_vs_stats(self, path):
        _check(lib.gsrt_dump_vs_stats(self.handle, os.fsencode(path)), self)

    def debug_counters(self):
        """The 32-word counter block of the last render (diagnostic; [16..] filled by GSRT_DIAG builds)."""
        out = np.zeros(32, np.uint64)
        _check(lib.gsrt_debug_counters(self.handle, _p(out[:16])), self)
        _check(lib.gsrt_debug_counters_hi(self.handle, _p(out[16:])), self)
        return out

    def device_exp_lut(self) -> np.ndarray:
        """The ExpLUT copy in HBM the REF kernels read (uploaded by gsrt_create)."""
        out = np.zeros(512, np.float32)
        _check(lib.gsrt_debug_exp_lut(self.handle, _p(out)), self)
        return out

    def timing(self, frames: int, kernel_only: bool = False, stride: int = 1):
        """Record HIP events around the next `frames` renders: the render kernel and (kernel_only False) the whole
        frame; with kernel_only the frame times read 0 and the timed frames carry two events each. stride > 1: only
        every stride-th frame is recorded (`frames` recorded frames, the others carry no events)."""
        _check(lib.gsrt_timing_kernel_only(self.handle, 1 if kernel_only else 0), self)
        _check(lib.gsrt_timing_stride(self.handle, stride), self)
        _check(lib.gsrt_timing(self.handle, frames), self)

    def timing_read(self, cap: int = 4096):
        k = np.zeros(cap, np.float32)
        f = np.zeros(cap, np.float32)
        n = np.zeros(1, np.uint32)
        _check(lib.gsrt_timing_read(self.handle, _p(k), _p(f), cap, _p(n)), self)
        return k[: int(n[0])].copy(), f[: int(n[0])].copy()

    def timing_read_exchange(self, cap: int = 4096):
        """per timed frame: the sharded exchange (gather + rank 0's unpack) on the comm stream, ms (0: no exchange)"""
        x = np.zeros(cap, np.float32)
        n = np.zeros(1, np.uint32)
        _check(lib.gsrt_timing_read_exchange(self.handle, _p(x), cap, _p(n)), self)
        return x[: int(n[0])].copy()

    def comm_size(self):
        """(ranks, rank) of the communicator as RCCL reports them; (1, 0) without comm_init"""
        n = np.zeros(1, np.int32)
        r = np.zeros(1, np.int32)
        _check(lib.gsrt_comm_size(self.handle, _p(n), _p(r)), self)
        return int(n[0]), int(r[0])

    def host_register(self, arr: np.ndarray):
        """page-lock a numpy array for asynchronous host-to-HBM streaming (gsrt_scene_stream_pages)"""
        _check(lib.gsrt_host_register(self.handle, ctypes.c_void_p(arr.ctypes.data), arr.nbytes), self)

    def host_unregister(self, arr: np.ndarray):
        _check(lib.gsrt_host_unregister(self.handle, ctypes.c_void_p(arr.ctypes.data)), self)

    def comm_init(self, uid: bytes, nranks: int, rank: int):
        buf = np.frombuffer(uid, np.uint8).copy()
        _check(lib.gsrt_comm_init(self.handle, _p(buf), nranks, rank), self)

    def debug_gathered(self, floats: int) -> np.ndarray:
        """rank 0's gather buffer after the last sharded frame (its first `floats` floats)"""
        out = np.zeros(floats, np.float32)
        _check(lib.gsrt_debug_gathered(self.handle, _p(out), floats), self)
        return out

    def comm_init_loopback(self):
        """A one-rank RCCL communicator that still takes the exchange path (packed buffers, ncclGather, k_unpack on
        the comm stream; GSRT_DEBUG_COMM_LOOPBACK). With GSRT_DEBUG_RANK_OF=N[:r] its sharded frames run rank r's
        share of an N-rank frame (the rank-share measurement)."""
        old = os.environ.get("GSRT_DEBUG_COMM_LOOPBACK")
        os.environ["GSRT_DEBUG_COMM_LOOPBACK"] = "1"
        try:
            self.comm_init(comm_unique_id(), 1, 0)
        finally:
            if old is None:
                del os.environ["GSRT_DEBUG_COMM_LOOPBACK"]
            else:
                os.environ["GSRT_DEBUG_COMM_LOOPBACK"] = old

    def set_bands(self, nranks: int, bands=None):
        """pin this ctx's sharded frames to a partition (nranks + 1 tile-row boundaries), or back to balancing (None)"""
        b = _bands_arg(bands)
        _check(lib.gsrt_set_bands(self.handle, nranks, _p(b)), self)

    def last_bands(self) -> np.ndarray:
        """the bands of the last sharded frame (empty before any)"""
        out = np.zeros(65, np.uint32)
        n = np.zeros(1, np.uint32)
        _check(lib.gsrt_last_bands(self.handle, _p(out), 65, _p(n)), self)
        return out[: int(n[0])].copy()

    def row_costs(self) -> np.ndarray:
        """the last whole COR frame's per-tile-row shading cost (the balancing profile)"""
        out = np.zeros(1 << 16, np.uint32)
        n = np.zeros(1, np.uint32)
        _check(lib.gsrt_row_costs(self.handle, _p(out), out.size, _p(n)), self)
        return out[: int(n[0])].copy()

    def dump8_read(self, width: int, height: int):
        """rank 0, after a FLAG_OUT_DUMP8 sharded frame: (codes[H, W], escapes in pixel order)"""
        codes = np.zeros((height, width), np.uint32)
        n = np.zeros(1, np.uint32)
        _check(lib.gsrt_dump8_read(self.handle, _p(codes), None, 0, _p(n)), self)
        esc = np.zeros(int(n[0]), ESCAPE_DTYPE)
        if esc.size:
            _check(lib.gsrt_dump8_read(self.handle, None, _p(esc), esc.size, _p(n)), self)
        return codes, esc

    def debug_share_costs(self, on: bool = True):
        """every sharded COR frame stores its tiles' costs (test hook; see debug_row_profile)"""
        _check(lib.gsrt_debug_share_costs(self.handle, 1 if on else 0), self)

    def debug_row_profile(self) -> np.ndarray:
        """the last cost-recording sharded frame's per-row costs over the frame's tile rows (this rank's band only)"""
        out = np.zeros(1 << 16, np.uint32)
        n = np.zeros(1, np.uint32)
        _check(lib.gsrt_debug_row_profile(self.handle, _p(out), out.size, _p(n)), self)
        return out[: int(n[0])].copy()

    @property
    def debug_streams(self) -> dict:
        """the context's streams by name, in creation order (gsrt_debug_streams; 0 = not created)"""
        out = (ctypes.c_void_p * 8)()
        n = ctypes.c_uint32()
        _check(lib.gsrt_debug_streams(self.handle, out, ctypes.byref(n)), self)
        names = ["render", "prep_hi0", "prep_lo0", "prep_hi1", "prep_lo1", "update", "comm"]
        return {k: int(out[i] or 0) for i, k in enumerate(names[: n.value])}

    @property
    def comm_stream(self) -> int:
        """the stream of sharded frames' gather + unpack (0: frames render straight into the framebuffer)"""
        return lib.gsrt_comm_stream(self.handle) or 0


class Scene:
    """gsrt_scene: Gaussians resident in HBM (params, AABBs, optional SH-3) + LBVH."""

    def __init__(self, ctx: Context, handle):
        self.ctx = ctx
        self.handle = handle
        ctx._scenes.add(self)

    @classmethod
    def from_ply(cls, ctx: Context, path, with_sh=True) -> "Scene":
        h = ctypes.c_void_p()
        _check(lib.gsrt_scene_from_ply(ctx.handle, os.fsencode(path), 1 if with_sh else 0, ctypes.byref(h)), ctx)
        return cls(ctx, h)

    @classmethod
    def from_params(cls, ctx: Context, params, aabbs, sh=None) -> "Scene":
        params = _f32(params, (-1, 12))
        n = params.shape[0]
        aabbs = _f32(aabbs, (n, 6))
        if sh is not None:
            sh = _f32(sh, (n, 48))
        h = ctypes.c_void_p()
        _check(lib.gsrt_scene_from_params(ctx.handle, _p(params), _p(aabbs), n, _p(sh), ctypes.byref(h)), ctx)
        return cls(ctx, h)

    @classmethod
    def from_model(cls, ctx: Context, center, rot, scale, opacity, sh=None) -> "Scene":
        center = _f32(center, (-1, 3))
        n = center.shape[0]
        rot, scale, opacity = _f32(rot, (n, 4)), _f32(scale, (n, 3)), _f32(opacity, (n,))
        if sh is not None:
            sh = _f32(sh, (n, 48))
        h = ctypes.c_void_p()
        _check(lib.gsrt_scene_from_model(ctx.handle, _p(center), _p(rot), _p(scale), _p(opacity), _p(sh), n,
                                         ctypes.byref(h)), ctx)
        return cls(ctx, h)

    @classmethod
    def from_model_device(cls, ctx: Context, n, d_center, d_rot, d_scale, d_opacity, d_sh=0) -> "Scene":
        """from_model of arrays that live on the device: addresses (int, e.g. a torch tensor's data_ptr()) of n x 3,
        n x 4, n x 3, n and, optionally, n x 48 floats, read without a host round trip (gsrt_scene_from_model with
        device sources). The arrays must hold their data when the call is made; it returns once they have been read."""
        h = ctypes.c_void_p()
        _check(lib.gsrt_scene_from_model(ctx.handle, _addr(d_center), _addr(d_rot), _addr(d_scale), _addr(d_opacity),
                                         _addr(d_sh or None), n, ctypes.byref(h)), ctx)
        return cls(ctx, h)

    @property
    def n(self) -> int:
        return lib.gsrt_scene_size(self.handle)

    @property
    def pages(self) -> int:
        return lib.gsrt_scene_pages(self.handle)

    def stream_pages(self, pages, params=None, aabbs=None):
        """copy the listed pages (GSRT_PAGE_GAUSSIANS Gaussians each) of the full-scene arrays params (n, 12) /
        aabbs (n, 6) into the scene: numpy arrays (page-lock them with Context.host_register for async copies)
        or device addresses (int)"""
        def arg(x, cols):
            if x is None:
                return None, None
            if isinstance(x, int):
                return ctypes.c_void_p(x), None
            a = _f32(x, (self.n, cols))
            return _p(a), a
        pp, kp = arg(params, 12)
        pa, ka = arg(aabbs, 6)
        ids = np.ascontiguousarray(pages, np.uint32).reshape(-1)
        _check(lib.gsrt_scene_stream_pages(self.handle, pp, pa, _p(ids), ids.size), self.ctx)
        del kp, ka

    def add_mesh(self, vertices, indices):
        """co-trace an indexed triangle mesh (REF frames): vertices (nv, 3), indices (nt, 3)"""
        v = _f32(vertices, (-1, 3))
        i = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
        _check(lib.gsrt_scene_add_mesh(self.handle, _p(v), v.shape[0], _p(i), i.shape[0]), self.ctx)

    @property
    def mesh_triangles(self) -> int:
        return lib.gsrt_scene_mesh_triangles(self.handle)

    def download(self):
        params = np.zeros((self.n, 12), np.float32)
        aabbs = np.zeros((self.n, 6), np.float32)
        _check(lib.gsrt_scene_download(self.handle, _p(params), _p(aabbs)), self.ctx)
        return params, aabbs

    def build_bvh(self):
        _check(lib.gsrt_build_bvh(self.handle), self.ctx)

    def refit_bvh(self, aabbs=None):
        """aabbs: numpy (n, 6), a device address (int, e.g. a torch tensor's data_ptr()), or None"""
        if isinstance(aabbs, int):
            _check(lib.gsrt_refit_bvh(self.handle, ctypes.c_void_p(aabbs)), self.ctx)
            return
        a = None if aabbs is None else _f32(aabbs, (self.n, 6))
        _check(lib.gsrt_refit_bvh(self.handle, _p(a)), self.ctx)

    def update(self, params=None, aabbs=None):
        """Replace GaussParam (n, 12) and/or AABB (n, 6) arrays: numpy arrays or device addresses (int)."""
        def arg(x, cols):
            if x is None:
                return None, None
            if isinstance(x, int):
                return ctypes.c_void_p(x), None
            a = _f32(x, (self.n, cols))
            return _p(a), a  # keep the array alive across the call
        pp, keep_p = arg(params, 12)
        pa, keep_a = arg(aabbs, 6)
        _check(lib.gsrt_scene_update(self.handle, pp, pa), self.ctx)
        del keep_p, keep_a

    def attach(self, params=None, aabbs=None):
        """Borrow device arrays (device addresses, int; None = unchanged): frames read them in place until detach()
        (gsrt_scene_attach). The caller keeps them allocated and unchanged until then."""
        _check(lib.gsrt_scene_attach(self.handle, None if params is None else ctypes.c_void_p(params),
                                     None if aabbs is None else ctypes.c_void_p(aabbs)), self.ctx)

    def detach(self):
        """copy borrowed arrays into the scene and wait for the frames that read them (gsrt_scene_detach)"""
        _check(lib.gsrt_scene_detach(self.handle), self.ctx)

    def bvh_info(self, depth=True):
        """n_internal, root_box (the BVH fitted to the current AABBs: a pending refit runs first) and, unless
        depth=False, max_depth (a host walk over the downloaded nodes)"""
        ni = np.zeros(1, np.uint32)
        box = np.zeros(6, np.float32)
        d = np.zeros(1, np.uint32)
        _check(lib.gsrt_bvh_info(self.handle, _p(ni), _p(box), _p(d) if depth else None), self.ctx)
        return {"n_internal": int(ni[0]), "root_box": box, "max_depth": int(d[0]) if depth else None}

    def bvh_download(self):
        n = self.n
        nodes = np.zeros((max(n - 1, 0), 16), np.uint32)
        gid = np.zeros(n, np.uint32)
        morton = np.zeros(n, np.uint32)
        _check(lib.gsrt_bvh_download(self.handle, _p(nodes) if n > 1 else None, _p(gid), _p(morton)), self.ctx)
        return nodes, gid, morton

    def render(self, ubo, mode=MODE_COR, k=0, raystate=False):
        """One frame to host memory: returns (rgba[H,W,4], raystate[H,W] or None)."""
        W, H = int(ubo["width"][0]), int(ubo["height"][0])
        rgba = np.zeros((H, W, 4), np.float32)
        rs = np.zeros((H, W), RAYSTATE_DTYPE) if raystate else None
        _check(lib.gsrt_render(self.handle, _p(ubo), mode, k, _p(rgba), _p(rs)), self.ctx)
        return rgba, rs

    def render_async(self, ubo, mode=MODE_COR, k=0, d_rgba: int = 0, d_raystate: int = 0):
        """Enqueue one frame on ctx.stream; outputs are device pointers (0 = keep in the framebuffer)."""
        _check(lib.gsrt_render_async(self.handle, _p(ubo), mode, k, d_rgba or None, d_raystate or None), self.ctx)

    def render_depth(self, ubo, mode=MODE_COR, k=0):
        """One COR frame with its expected depth (FLAG_DEPTH) to host memory: (rgba[H,W,4], depth[H,W]). depth is
        the premultiplied sum of z w over each ray's blended hits (z: the Gaussian centre's view depth), combined over
        the samples like the colour; divide by rgba[..., 3] for the normalised value (gsrt_render_depth)."""
        W, H = int(ubo["width"][0]), int(ubo["height"][0])
        rgba = np.zeros((H, W, 4), np.float32)
        depth = np.zeros((H, W), np.float32)
        _check(lib.gsrt_render_depth(self.handle, _p(ubo), mode, k, _p(rgba), _p(depth)), self.ctx)
        return rgba, depth

    def render_depth_async(self, ubo, mode=MODE_COR, k=0, d_rgba: int = 0, d_depth: int = 0):
        """Enqueue one depth frame on ctx.stream; outputs are device pointers (0 = keep in the ctx buffers:
        Context.framebuffer_ptr, Context.depth_ptr())."""
        _check(lib.gsrt_render_depth_async(self.handle, _p(ubo), mode, k, d_rgba or None, d_depth or None), self.ctx)

    def set_features(self, feat, channels=None):
        """The scene's feature table for render_features: an (n, C) float32 array, 1 <= C <= MAX_FEATURES, copied
        (a (n,) array is one channel), or a device address of n * channels floats; None removes it. Waits for every
        queued frame first (gsrt_scene_set_features)."""
        if feat is None:
            _check(lib.gsrt_scene_set_features(self.handle, None, 0), self.ctx)
            return
        if isinstance(feat, int):
            _check(lib.gsrt_scene_set_features(self.handle, ctypes.c_void_p(feat), channels or 0), self.ctx)
            return
        feat = np.ascontiguousarray(feat, np.float32)
        if feat.ndim == 1:
            feat = feat[:, None]
        if feat.ndim != 2 or feat.shape[0] != self.n:
            raise GsrtError(E_ARG, "set_features: an (n, channels) array")
        _check(lib.gsrt_scene_set_features(self.handle, _p(feat), feat.shape[1]), self.ctx)

    def features(self) -> int:
        """channels of the scene's feature table, 0 without one (gsrt_scene_features)"""
        return int(lib.gsrt_scene_features(self.handle))

    def render_features(self, ubo, mode=MODE_COR, k=0):
        """One feature frame (FLAG_FEATURES) to host memory: (rgba[H,W,4], feat[H,W,C]). feat[..., c] is the
        premultiplied sum of f_c w over each ray's blended hits, combined over the samples like the colour; rgba is the
        frame without SH rows (r = g = b = sum w, a = 1 - T): divide by it to normalise (gsrt_render_features)."""
        W, H = int(ubo["width"][0]), int(ubo["height"][0])
        rgba = np.zeros((H, W, 4), np.float32)
        feat = np.zeros((H, W, max(self.features(), 1)), np.float32)
        _check(lib.gsrt_render_features(self.handle, _p(ubo), mode, k, _p(rgba), _p(feat)), self.ctx)
        return rgba, feat

    def render_features_async(self, ubo, mode=MODE_COR, k=0, d_rgba: int = 0, d_feat: int = 0):
        """Enqueue one feature frame on ctx.stream; outputs are device pointers (0 = keep in the ctx buffers:
        Context.framebuffer_ptr, Context.features_ptr())."""
        _check(lib.gsrt_render_features_async(self.handle, _p(ubo), mode, k, d_rgba or None, d_feat or None), self.ctx)

    def feature_grad(self, ubo, grad_image, mode=MODE_COR, k=0):
        """The backward of a feature frame to the feature table (gsrt_render_feature_grad): grad_image is the upstream
        gradient of the feature image, (H, W, C) or (H, W) float32 with 1 <= C <= MAX_FEATURES; returns the (n, C)
        gradient table, grad[g, c] = sum of w * G[p, c] / ns over the hits of Gaussian g the frame blends. The sum's
        order is unspecified (float atomics): the last bits can differ from run to run. No feature table is needed."""
        W, H = int(ubo["width"][0]), int(ubo["height"][0])
        g = np.asarray(grad_image, np.float32)
        if g.ndim == 2:
            g = g[:, :, None]
        if g.ndim != 3 or g.shape[:2] != (H, W) or not 1 <= g.shape[2] <= MAX_FEATURES:
            raise GsrtError(E_ARG, "feature_grad: an (H, W, channels) or (H, W) array, 1 <= channels <= MAX_FEATURES")
        g = np.ascontiguousarray(g)
        out = np.zeros((self.n, g.shape[2]), np.float32)
        _check(lib.gsrt_render_feature_grad(self.handle, _p(ubo), mode, k, _p(g), g.shape[2], _p(out), 0), self.ctx)
        return out

    def feature_grad_async(self, ubo, d_grad_image: int, channels: int, d_grad_table: int, accumulate=False,
                           mode=MODE_COR, k=0):
        """Enqueue one gradient frame on ctx.stream: d_grad_image (W*H*channels floats) and d_grad_table (n*channels
        floats, ordinary device memory) are device addresses; accumulate adds to the table instead of writing it."""
        _check(lib.gsrt_render_feature_grad_async(self.handle, _p(ubo), mode, k, ctypes.c_void_p(d_grad_image or None),
                                                  channels, ctypes.c_void_p(d_grad_table or None),
                                                  1 if accumulate else 0), self.ctx)

    def contributions(self, ubo, mode=MODE_COR, k=0):
        """Each Gaussian's contribution to the view, (n,): its blend weight summed over the frame's pixels (the mean
        over a pixel's samples), i.e. feature_grad of an image of ones with one channel."""
        W, H = int(ubo["width"][0]), int(ubo["height"][0])
        return self.feature_grad(ubo, np.ones((H, W), np.float32), mode, k)[:, 0]

    def set_sh(self, sh):
        """Replace the scene's SH rows: an (n, 16, 3) or (n, 48) float32 array laid out [gauss][coef][rgb], copied, or a
        device address of n * 48 floats in that layout; None removes them (the scene then renders colour 1). Waits for
        every queued frame first (gsrt_scene_set_sh)."""
        if sh is None:
            _check(lib.gsrt_scene_set_sh(self.handle, None), self.ctx)
            return
        if isinstance(sh, int):
            _check(lib.gsrt_scene_set_sh(self.handle, ctypes.c_void_p(sh)), self.ctx)
            return
        sh = _f32(sh, (self.n, 48))
        _check(lib.gsrt_scene_set_sh(self.handle, _p(sh)), self.ctx)

    def sh_grad(self, ubo, grad_image, mode=MODE_COR, k=0):
        """The backward of a colour frame to the SH table (gsrt_render_sh_grad): grad_image is the upstream gradient of
        the RGBA frame, (H, W, 4) or (H, W, 3) float32 (alpha's gradient is ignored: alpha does not depend on SH); returns
        the (n, 16, 3) gradient of the table, grad[g, q, ch] = sum of w * Y_q * G[p, ch] / ns over the hits of Gaussian g
        whose channel ch the clamp at 0 let through. The sum's order is unspecified (float atomics)."""
        g = _rgba_grad("sh_grad", ubo, grad_image)
        out = np.zeros((self.n, 16, 3), np.float32)
        _check(lib.gsrt_render_sh_grad(self.handle, _p(ubo), mode, k, _p(g), _p(out), 0), self.ctx)
        return out

    def sh_grad_async(self, ubo, d_grad_image: int, d_grad_table: int, accumulate=False, mode=MODE_COR, k=0):
        """Enqueue one SH gradient frame on ctx.stream: d_grad_image (W*H*4 floats) and d_grad_table (n*48 floats,
        ordinary device memory) are device addresses; accumulate adds to the table instead of writing it."""
        _check(lib.gsrt_render_sh_grad_async(self.handle, _p(ubo), mode, k, ctypes.c_void_p(d_grad_image or None),
                                             ctypes.c_void_p(d_grad_table or None), 1 if accumulate else 0), self.ctx)

    def opacity_grad(self, ubo, grad_image, mode=MODE_COR, k=0):
        """The backward of a colour frame to the opacities (gsrt_render_opacity_grad): grad_image is the upstream
        gradient of the RGBA frame, (H, W, 4) float32, or (H, W, 3), padded with a zero alpha gradient; returns the (n,)
        gradient with respect to each Gaussian's opacity (the definition is in gsrt.h). A hit whose alpha the clamp at
        0.99 cut contributes +0. The sum's order is unspecified (float atomics)."""
        g = _rgba_grad("opacity_grad", ubo, grad_image)
        out = np.zeros(self.n, np.float32)
        _check(lib.gsrt_render_opacity_grad(self.handle, _p(ubo), mode, k, _p(g), _p(out), 0), self.ctx)
        return out

    def opacity_grad_async(self, ubo, d_grad_image: int, d_grad_table: int, accumulate=False, mode=MODE_COR, k=0):
        """Enqueue one opacity gradient frame on ctx.stream: d_grad_image (W*H*4 floats) and d_grad_table (n floats,
        ordinary device memory) are device addresses; accumulate adds to the table instead of writing it."""
        _check(lib.gsrt_render_opacity_grad_async(self.handle, _p(ubo), mode, k, ctypes.c_void_p(d_grad_image or None),
                                                  ctypes.c_void_p(d_grad_table or None), 1 if accumulate else 0), self.ctx)

    def splat_grad(self, ubo, grad_image, mode=MODE_COR, k=0):
        """The backward of a colour frame to each Gaussian's screen-space splat (gsrt_render_splat_grad): grad_image is
        the upstream gradient of the RGBA frame, (H, W, 4) float32, or (H, W, 3), padded with a zero alpha gradient;
        returns (n, 8): dL/d(ppx, ppy, A, B, C) of the pixel centre and the conic in slots 0..4, dL/d(opacity) in slot 5
        (opacity_grad's sum), +0 in slots 6 and 7. Slots 0 and 1 are the view-space positional gradient densification
        thresholds on. The sum's order is unspecified (float atomics). Not with FLAG_LUT."""
        g = _rgba_grad("splat_grad", ubo, grad_image)
        out = np.zeros((self.n, 8), np.float32)
        _check(lib.gsrt_render_splat_grad(self.handle, _p(ubo), mode, k, _p(g), _p(out), 0), self.ctx)
        return out

    def splat_grad_async(self, ubo, d_grad_image: int, d_grad_splat: int, accumulate=False, mode=MODE_COR, k=0):
        """Enqueue one splat gradient frame on ctx.stream: d_grad_image (W*H*4 floats) and d_grad_splat (n*8 floats,
        ordinary device memory) are device addresses; accumulate adds to the table instead of writing it."""
        _check(lib.gsrt_render_splat_grad_async(self.handle, _p(ubo), mode, k, ctypes.c_void_p(d_grad_image or None),
                                                ctypes.c_void_p(d_grad_splat or None), 1 if accumulate else 0), self.ctx)

    def splat_depth_grad(self, ubo, grad_image, grad_depth, mode=MODE_COR, k=0):
        """The backward of a depth frame, RGBA and expected depth together, to the splat rows
        (gsrt_render_splat_depth_grad): grad_image as for splat_grad, grad_depth the upstream gradient of the depth image,
        (H, W) float32. Returns (n, 8): slots 0..5 as splat_grad's with the depth's part in every hit's d, dL/d(view
        depth) in slot 6 (w * Gdepth / ns summed over the blended hits, clamped or not), +0 in slot 7. Not with FLAG_LUT."""
        g = _rgba_grad("splat_depth_grad", ubo, grad_image)
        gd = np.asarray(grad_depth, np.float32)
        if gd.shape != (int(ubo["height"][0]), int(ubo["width"][0])):
            raise GsrtError(E_ARG, "splat_depth_grad: grad_depth is an (H, W) array")
        gd = np.ascontiguousarray(gd)
        out = np.zeros((self.n, 8), np.float32)
        _check(lib.gsrt_render_splat_depth_grad(self.handle, _p(ubo), mode, k, _p(g), _p(gd), _p(out), 0), self.ctx)
        return out

    def splat_depth_grad_async(self, ubo, d_grad_image: int, d_grad_depth: int, d_grad_splat: int, accumulate=False,
                               mode=MODE_COR, k=0):
        """Enqueue one splat-depth gradient frame on ctx.stream: d_grad_image (W*H*4 floats), d_grad_depth (W*H floats)
        and d_grad_splat (n*8 floats, ordinary device memory) are device addresses; accumulate adds to the table."""
        _check(lib.gsrt_render_splat_depth_grad_async(self.handle, _p(ubo), mode, k, ctypes.c_void_p(d_grad_image or None),
                                                      ctypes.c_void_p(d_grad_depth or None),
                                                      ctypes.c_void_p(d_grad_splat or None), 1 if accumulate else 0),
               self.ctx)

    def model_grad(self, ubo, splat, depth=False):
        """The projection backwards (gsrt_splat_grad_to_model): splat is the (n, 8) table of splat_grad for the same ubo
        and scene parameters; returns (grad_center (n, 3), grad_cov (n, 6)), the covariance in cov3d's order xx, xy, xz,
        yy, yz, zz, an off-diagonal entry counted as the one variable it is. Deterministic. depth: the table is
        splat_depth_grad's and slot 6 is chained to the centre too (gsrt_splat_depth_grad_to_model)."""
        rows = _f32(splat, (self.n, 8))
        gc, gv = np.zeros((self.n, 3), np.float32), np.zeros((self.n, 6), np.float32)
        fn = lib.gsrt_splat_depth_grad_to_model if depth else lib.gsrt_splat_grad_to_model
        _check(fn(self.handle, _p(ubo), _p(rows), _p(gc), _p(gv), 0), self.ctx)
        return gc, gv

    def model_grad_async(self, ubo, d_grad_splat: int, d_grad_center: int, d_grad_cov: int, accumulate=False, depth=False):
        """Enqueue the projection's backward on ctx.stream: device addresses of n*8, n*3 and n*6 floats."""
        fn = lib.gsrt_splat_depth_grad_to_model_async if depth else lib.gsrt_splat_grad_to_model_async
        _check(fn(self.handle, _p(ubo), ctypes.c_void_p(d_grad_splat or None), ctypes.c_void_p(d_grad_center or None),
                  ctypes.c_void_p(d_grad_cov or None), 1 if accumulate else 0), self.ctx)

    def view_stats_add(self, ubo, grad_splat, stats, radii=None, asynchronous=False):
        """gsrt.view_stats_add of this scene: the densification statistic of the rows and the largest screen radius"""
        return view_stats_add(self, ubo, grad_splat, stats, radii, asynchronous)

    def pose_grad(self, ubo, rows, depth=False):
        """The camera's gradient (gsrt_pose_grad): rows is the (n, 8) table of splat_grad (depth=True: of splat_depth_grad)
        for the same ubo and scene parameters, a numpy array or a device address; returns (16,) float32, the partial
        derivative of the loss with respect to ubo.model_view in its own column-major layout (reshape(4, 4).T is the matrix),
        with model_view_inverse held fixed. Summed in double in a fixed order: deterministic."""
        out = np.zeros(16, np.float32)
        if isinstance(rows, (int, np.integer)):
            src = ctypes.c_void_p(int(rows) or None)
        else:
            rows = _f32(rows, (self.n, 8))
            src = _p(rows)
        _check(lib.gsrt_pose_grad(self.handle, _p(ubo), src, 1 if depth else 0, _p(out)), self.ctx)
        return out

    def pose_grad_async(self, ubo, d_grad_splat: int, d_grad_model_view: int, depth=False):
        """Enqueue the camera's gradient on ctx.stream: device addresses of n*8 and 16 floats."""
        _check(lib.gsrt_pose_grad_async(self.handle, _p(ubo), ctypes.c_void_p(d_grad_splat or None), 1 if depth else 0,
                                        ctypes.c_void_p(d_grad_model_view or None)), self.ctx)

    def geometry_grad(self, ubo, grad_image, mode=MODE_COR, k=0, grad_depth=None):
        """One splat gradient frame and the projection's backward: (grad_center (n, 3), grad_cov (n, 6), grad_opacity
        (n,)) of <grad_image, frame> with respect to the scene's parameters. grad_depth: the (H, W) upstream gradient of
        the depth image, for <grad_image, frame> + <grad_depth, depth> (splat_depth_grad and the depth chain)."""
        if grad_depth is None:
            rows = self.splat_grad(ubo, grad_image, mode, k)
            gc, gv = self.model_grad(ubo, rows)
        else:
            rows = self.splat_depth_grad(ubo, grad_image, grad_depth, mode, k)
            gc, gv = self.model_grad(ubo, rows, depth=True)
        return gc, gv, rows[:, 5].copy()

    def render_sharded(self, ubo, mode=MODE_COR, k=0, want_image=True):
        W, H = int(ubo["width"][0]), int(ubo["height"][0])
        rgba = np.zeros((H, W, 4), np.float32) if want_image and not (mode & FLAG_OUT_DUMP8) else None
        _check(lib.gsrt_render_sharded(self.handle, _p(ubo), mode, k, _p(rgba)), self.ctx)
        return rgba

    def render_sharded_emulated(self, ubo, nranks, mode=MODE_COR, bands=None):
        """All ranks' packed tiles on this device + the rank-0 unpack (everything but the RCCL transport)."""
        W, H = int(ubo["width"][0]), int(ubo["height"][0])
        rgba = np.zeros((H, W, 4), np.float32)
        b = _bands_arg(bands)
        _check(lib.gsrt_render_sharded_emulated(self.handle, _p(ubo), mode, nranks, _p(b), _p(rgba)), self.ctx)
        return rgba

    def render_sharded_emulated_dump8(self, ubo, nranks, mode=MODE_COR, bands=None):
        """render_sharded_emulated with FLAG_OUT_DUMP8 blocks: (codes[H, W], escapes in pixel order)"""
        W, H = int(ubo["width"][0]), int(ubo["height"][0])
        codes = np.zeros((H, W), np.uint32)
        b = _bands_arg(bands)
        n = np.zeros(1, np.uint32)
        # every rank's list at its capacity (gsrt_dump8_layout: the capacity follows the largest band)
        cap = int(dump8_layout(ubo, nranks, bands, mode)["cap"]) * nranks
        esc = np.zeros(cap, ESCAPE_DTYPE)
        _check(lib.gsrt_render_sharded_emulated_dump8(self.handle, _p(ubo), mode | FLAG_OUT_DUMP8, nranks, _p(b),
                                                      _p(codes), _p(esc), esc.size, _p(n)), self.ctx)
        if int(n[0]) > esc.size:
            raise GsrtError(E_STATE, f"dump8: {int(n[0])} escapes, room for {esc.size}")
        return codes, esc[: int(n[0])].copy()

    def render_sharded_async(self, ubo, mode=MODE_COR, k=0):
        _check(lib.gsrt_render_sharded_async(self.handle, _p(ubo), mode, k), self.ctx)

    def close(self):
        if getattr(self, "handle", None):
            lib.gsrt_destroy_scene(self.handle)
            self.handle = None

    def __del__(self):
        self.close()


# ---------------------------------------------------------------- the training session

def philox_words(seed, stream_id, first_block, blocks) -> np.ndarray:
    """the raw words of normal_noise's generator (gsrt_debug_philox; no device): (blocks, 4) uint32, Philox4x32-10 with
    the key (seed lo, seed hi) and the counters (j lo, j hi, stream_id, 0), j = first_block .. first_block + blocks - 1"""
    out = np.zeros((blocks, 4), np.uint32)
    _check(lib.gsrt_debug_philox(seed, stream_id, first_block, blocks, _p(out)))
    return out


def normal_noise(ctx, count, seed, stream_id=0, *, d_out=None, asynchronous=False):
    """count standard normal draws (gsrt_normal_noise; the arithmetic is in gsrt.h): value i is a pure function of (seed,
    stream_id, i). Returns a float32 array of count; with d_out, the device address of count floats, writes there and
    returns None (asynchronous=True: enqueued on ctx.stream only)."""
    if d_out is not None:
        fn = lib.gsrt_normal_noise_async if asynchronous else lib.gsrt_normal_noise
        _check(fn(ctx.handle, count, seed, stream_id, _addr(d_out)), ctx)
        return None
    out = np.zeros(count, np.float32)
    _check(lib.gsrt_normal_noise(ctx.handle, count, seed, stream_id, _p(out)), ctx)
    return out


def model_remap(ctx, origin, arrays, *, n_out=None, feature_channels=0, out=None, asynchronous=False):
    """The optimiser state across a densify (gsrt_model_remap): row i of every array of the result is row origin[i] of
    `arrays` = (center, rot, scale, opacity, sh or None, features or None), or zeros where origin[i] < 0; the contract
    of gsrt.autograd.remap_state for a whole model in one launch. numpy arrays: returns the new tuple. device addresses
    (int): origin an address too, n_out, out = six addresses (and feature_channels) are needed; returns None."""
    arrays = tuple(arrays) + (None,) * (6 - len(arrays))
    if isinstance(arrays[0], int):
        if n_out is None or out is None or not isinstance(origin, int):
            raise GsrtError(E_ARG, "model_remap: device addresses need origin as an address, n_out and out")
        s_in = ModelArrays(*[x or None for x in arrays], feature_channels)
        s_out = ModelArrays(*[x or None for x in out], feature_channels)
        fn = lib.gsrt_model_remap_async if asynchronous else lib.gsrt_model_remap
        _check(fn(ctx.handle, n_out, _addr(origin), ctypes.byref(s_in), ctypes.byref(s_out)), ctx)
        return None
    org = np.ascontiguousarray(origin, dtype=np.int32).reshape(-1)
    src = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
    n_in = src[0].shape[0]
    if org.size and int(org.max()) >= n_in:
        raise GsrtError(E_ARG, "model_remap: an origin entry is not a row of the arrays")
    fc = 0 if src[5] is None else (src[5].shape[1] if src[5].ndim == 2 else 0)
    k = org.size
    res = [None if a is None else np.zeros((k,) + a.shape[1:], np.float32) for a in src]
    s_in = ModelArrays(*[None if a is None else a.ctypes.data for a in src], fc)
    s_out = ModelArrays(*[None if a is None else a.ctypes.data for a in res], fc)
    _check(lib.gsrt_model_remap(ctx.handle, k, _p(org), ctypes.byref(s_in), ctypes.byref(s_out)), ctx)
    return tuple(res)


def ply_write(path, center, rot, log_scale, logit_opacity, sh=None):
    """Write the raw model (unnormalised quaternion, log scale, logit: what model_deactivate returns and model_step
    optimises) as a binary little-endian 3DGS .ply (gsrt_ply_write), every float as it is. sh: (n, 16, 3) / (n, 48) or
    None (then no f_dc / f_rest properties are written)."""
    center = _f32(center, (-1, 3))
    n = center.shape[0]
    rot, log_scale, logit_opacity = _f32(rot, (n, 4)), _f32(log_scale, (n, 3)), _f32(logit_opacity, (n,))
    sh = None if sh is None else _f32(sh, (n, 48))
    s_raw = ModelArrays(*[None if a is None else a.ctypes.data for a in (center, rot, log_scale, logit_opacity, sh)], None, 0)
    _check(lib.gsrt_ply_write(os.fsencode(path), n, ctypes.byref(s_raw)))


def lr_expon(lr_init, lr_final, step, max_steps, delay_mult=1.0, delay_steps=0) -> float:
    """3DGS's get_expon_lr_func at `step` (gsrt_lr_expon; host only): log-linear from lr_init to lr_final over max_steps,
    scaled by the delayed start when delay_steps > 0"""
    out = ctypes.c_float(0.0)
    _check(lib.gsrt_lr_expon(lr_init, lr_final, delay_mult, delay_steps, max_steps, step, ctypes.byref(out)))
    return float(out.value)


class _BorrowedScene(Scene):
    """a scene owned by a Trainer: every Scene method works, close() only forgets the handle"""

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.handle = handle

    def close(self):
        self.handle = None


class Trainer:
    """gsrt_trainer: a training run's state on the device (raw model, Adam moments, gradient tables, densification
    statistics, scene and BVH, step counter) and its iterations. model = (center, rot, scale, opacity, sh or None), the
    activated model as Scene.from_model takes it, numpy arrays or device addresses (then n is needed); capacity: the rows
    everything is allocated for (default n)."""

    def __init__(self, ctx: Context, model, capacity=None, *, n=None):
        addr, n, fc, keep, dev = _model_set("Trainer: model", model, n, False)
        if n is None:
            raise GsrtError(E_ARG, "Trainer: device addresses need n")
        s_model = ModelArrays(*addr, fc)
        h = ctypes.c_void_p()
        _check(lib.gsrt_trainer_create(ctx.handle, ctypes.byref(s_model), n, n if capacity is None else capacity,
                                       ctypes.byref(h)), ctx)
        self.ctx, self.handle, self.has_sh = ctx, h, addr[4] is not None
        ctx._scenes.add(self)  # closed with the context, before it

    def close(self):
        if getattr(self, "handle", None):
            lib.gsrt_trainer_destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def info(self) -> dict:
        n, cap, step = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(lib.gsrt_trainer_info(self.handle, ctypes.byref(n), ctypes.byref(cap), ctypes.byref(step)), self.ctx)
        return dict(n=int(n.value), capacity=int(cap.value), step=int(step.value))

    def step(self, ubo, target, adam, *, k=0, mask=None, target_depth=None, lam=0.2, params=None, target_channels=None,
             want_scalars=True):
        """One iteration against one view (gsrt_trainer_step). target: (H, W, 3) or (H, W, 4), mask / target_depth (H, W)
        or None, numpy arrays or device addresses (then target_channels is needed). adam: an AdamParams whose step is
        ignored. params: a FrameLossParams (default: frame_loss_params(lam)). Returns dict(loss=, l1=, ssim=, mse=,
        depth_l1=, depth_samples=), or None with want_scalars=False."""
        P = params if params is not None else frame_loss_params(lam)
        keep = []
        if isinstance(target, int):
            if target_channels is None:
                raise GsrtError(E_ARG, "Trainer.step: a device target needs target_channels")
            args = [_addr(target), target_channels, _addr(mask), _addr(target_depth)]
        else:
            y = np.ascontiguousarray(target, dtype=np.float32)
            h, w = int(ubo["height"][0]), int(ubo["width"][0])
            if y.ndim != 3 or y.shape[:2] != (h, w):
                raise GsrtError(E_ARG, "Trainer.step: target is an (H, W, 3) or (H, W, 4) array of the ubo's frame")
            planes = [a if a is None or isinstance(a, int) else _f32(a, (h, w)) for a in (mask, target_depth)]
            keep += [y] + planes
            args = [_p(y), y.shape[2] if target_channels is None else target_channels, _addr(planes[0]), _addr(planes[1])]
        out = np.zeros(FRAME_LOSS_SCALARS, np.float32) if want_scalars else None
        _check(lib.gsrt_trainer_step(self.handle, _p(ubo), k, args[0], args[1], args[2], args[3], ctypes.byref(P),
                                     ctypes.byref(adam), _p(out)), self.ctx)
        if out is None:
            return None
        return dict(zip(("loss", "l1", "ssim", "mse", "depth_l1", "depth_samples"), (float(v) for v in out)))

    @property
    def sh_degree(self) -> int:
        """the active SH degree of the following steps, 0..3 (gsrt_trainer_sh_degree / gsrt_trainer_set_sh_degree; 3 at
        creation): the SH words above it keep their bits, 3DGS's ramp-up when the caller raises it as it goes"""
        d = ctypes.c_uint32(0)
        _check(lib.gsrt_trainer_sh_degree(self.handle, ctypes.byref(d)), self.ctx)
        return int(d.value)

    @sh_degree.setter
    def sh_degree(self, d):
        if not 0 <= int(d) <= 0xFFFFFFFF:
            raise GsrtError(E_ARG, "Trainer.sh_degree: 0..3")
        _check(lib.gsrt_trainer_set_sh_degree(self.handle, int(d)), self.ctx)

    def radii(self) -> int:
        """the device address of the screen radii gathered since the last densify (gsrt_trainer_radii): n floats in use,
        borrowed until the next densify()"""
        p = ctypes.c_void_p()
        _check(lib.gsrt_trainer_radii(self.handle, ctypes.byref(p)), self.ctx)
        return int(p.value)

    def densify(self, params, seed=0, max_screen_radius=0.0) -> int:
        """clone, split and prune with the statistics gathered since the last densify (gsrt_trainer_densify; with
        max_screen_radius > 0 the screen-size prune too, gsrt_trainer_densify_screen: a Gaussian whose largest screen radius
        since the last densify is above it is pruned); returns the
        new n. GsrtError(E_ARG) with nothing changed when the new model exceeds the capacity. Scenes obtained from scene()
        earlier are dead after it."""
        got = ctypes.c_uint32(0)
        if max_screen_radius == 0.0:
            _check(lib.gsrt_trainer_densify(self.handle, ctypes.byref(params), seed, ctypes.byref(got)), self.ctx)
        else:
            _check(lib.gsrt_trainer_densify_screen(self.handle, ctypes.byref(params), max_screen_radius, seed,
                                                   ctypes.byref(got)), self.ctx)
        return int(got.value)

    def opacity_reset(self, max_opacity=0.01):
        _check(lib.gsrt_trainer_opacity_reset(self.handle, max_opacity), self.ctx)

    def rebuild_bvh(self):
        _check(lib.gsrt_trainer_rebuild_bvh(self.handle), self.ctx)

    def scene(self) -> Scene:
        """the trainer's scene, borrowed (evaluation views); dead after the next densify()"""
        h = ctypes.c_void_p()
        _check(lib.gsrt_trainer_scene(self.handle, ctypes.byref(h)), self.ctx)
        return _BorrowedScene(self.ctx, h)

    def state(self) -> dict:
        """device addresses (gsrt_trainer_state), borrowed until the next densify(): raw, m, v as (center, rot, scale,
        opacity, sh or None), grads as (center, cov, splat, sh or None), stats"""
        raw, m, v, g = ModelArrays(), ModelArrays(), ModelArrays(), ModelGrads()
        st = ctypes.c_void_p()
        _check(lib.gsrt_trainer_state(self.handle, ctypes.byref(raw), ctypes.byref(m), ctypes.byref(v), ctypes.byref(g),
                                      ctypes.byref(st)), self.ctx)
        five = lambda a: (a.center, a.rot_rxyz, a.scale, a.opacity, a.sh)  # noqa: E731
        return dict(raw=five(raw), m=five(m), v=five(v), grads=(g.center, g.cov, g.splat, g.sh), stats=st.value)

    def download(self, act=True):
        """(raw, act): the raw model and, with act, its activation, each (center (n, 3), rot (n, 4), scale (n, 3), opacity
        (n,), sh (n, 48) or None) as numpy arrays (gsrt_trainer_download)"""
        n = self.info()["n"]
        new = lambda: _new_model(n, [1, 1, 1, 1, 1 if self.has_sh else None, None], 0)[:5]  # noqa: E731
        raw, a = new(), (new() if act else None)
        s = lambda o: ModelArrays(*[None if x is None else x.ctypes.data for x in o], None, 0)  # noqa: E731
        s_raw, s_act = s(raw), (s(a) if act else None)
        _check(lib.gsrt_trainer_download(self.handle, ctypes.byref(s_raw), None if s_act is None else ctypes.byref(s_act)),
               self.ctx)
        return tuple(raw), (tuple(a) if act else None)
