"""ctypes binding of libdsnerf_hip.so (include/dsnerf.h) + thin torch-tensor plumbing.

PyTorch is used for device memory, streams and (elsewhere) torch.distributed only.  There is no
eager / CPU fallback: if the library is missing or a call fails, a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# DSNERF_LIB: another build of the same library (kernel-variant experiments, scripts/variants.sh)
LIB_PATH = os.environ.get("DSNERF_LIB") or os.path.join(_HERE, "libdsnerf_hip.so")
_lib = None

PARAM_ORDER = [
    "nerf.embedding.weight",
    "nerf.stage1.0.weight", "nerf.stage1.0.bias", "nerf.stage1.2.weight", "nerf.stage1.2.bias",
    "nerf.stage1.4.weight", "nerf.stage1.4.bias", "nerf.stage1.6.weight", "nerf.stage1.6.bias",
    "nerf.stage2.0.weight", "nerf.stage2.0.bias", "nerf.stage2.2.weight", "nerf.stage2.2.bias",
    "nerf.stage2.4.weight", "nerf.stage2.4.bias",
    "nerf.density_net.0.weight", "nerf.density_net.0.bias",
    "nerf.rgb_net.1.weight", "nerf.rgb_net.1.bias", "nerf.rgb_net.3.weight", "nerf.rgb_net.3.bias",
    "lighting_mlp.lights_encoding.0.weight", "lighting_mlp.lights_encoding.0.bias",
    "lighting_mlp.lights_encoding.2.weight", "lighting_mlp.lights_encoding.2.bias",
    "lighting_mlp.lights_encoding.4.weight", "lighting_mlp.lights_encoding.4.bias",
    "pose_mlp.0.weight", "pose_mlp.0.bias", "pose_mlp.2.weight", "pose_mlp.2.bias",
    "pose_mlp.4.weight", "pose_mlp.4.bias",
]

EXPORTS = [
    "dsn_abi_version", "dsn_last_error", "dsn_packed_param_bytes", "dsn_pack_params",
    "dsn_pack_params_host_image", "dsn_scene_bytes", "dsn_set_body", "dsn_set_frame", "dsn_set_frame_ex", "dsn_sample_gg",
    "dsn_sample_uniform", "dsn_warp", "dsn_field", "dsn_field_record_bytes",
    "dsn_field_forward", "dsn_field_reverse", "dsn_shade", "dsn_composite",
    "dsn_render_workspace_bytes", "dsn_render_rays", "dsn_grad_workspace_bytes", "dsn_render_rays_grad",
    "dsn_image_workspace_bytes", "dsn_image_scatter", "dsn_image_psnr", "dsn_debug_screen", "dsn_field_screen", "dsn_lbs_warp", "dsn_render_rays_train", "dsn_debug_nn_stats", "dsn_camera_rays",
    "dsn_pose_state_bytes", "dsn_set_pose", "dsn_light", "dsn_calibrate_workspace_bytes", "dsn_calibrate_screen",
    "dsn_set_screen_margin", "dsn_module_grad", "dsn_early_stop_eps", "dsn_calibrate_screen_frame",
    "dsn_early_stop_eps_scaled", "dsn_set_early_stop_colour_scale", "dsn_nn_header_offsets", "dsn_render_workspace_bytes_for",
    "dsn_render_workspace_record_capacity", "dsn_stop_slice_len", "dsn_stop_stats_slice_len", "dsn_early_stop_colour_headroom", "dsn_render_rays_ex",
    "dsn_render_rays_grad_ex", "dsn_render_rays_train_ex", "dsn_aux_create", "dsn_aux_destroy",
    "dsn_render_lights_scratch_bytes", "dsn_render_rays_lights", "dsn_image_ssim_workspace_bytes", "dsn_image_ssim",
    "dsn_density_grid_workspace_bytes", "dsn_density_grid", "dsn_mc_workspace_bytes", "dsn_mc_count", "dsn_mc_emit", "dsn_mc_table_host",
    "dsn_render_maps_scratch_bytes", "dsn_render_rays_maps", "dsn_composite_maps", "dsn_shade_factor",
    "dsn_raster_workspace_bytes", "dsn_raster_mesh", "dsn_raster_mesh_ex", "dsn_mc_normals", "dsn_raster_mesh_attr",
    "dsn_mesh_cc_workspace_bytes", "dsn_mesh_cc_label", "dsn_mesh_cc_emit", "dsn_mesh_cc_label_ex", "dsn_mesh_cc_emit_ex",
    "dsn_bound_mask", "dsn_train_rays_workspace_bytes", "dsn_train_rays",
    "dsn_mesh_bind_normals", "dsn_mesh_pose_workspace_bytes", "dsn_mesh_pose", "dsn_mesh_stretch",
    "dsn_mesh_simplify_workspace_bytes", "dsn_mesh_simplify_count", "dsn_mesh_simplify_emit", "dsn_mesh_simplify_cells",
    "dsn_mesh_simplify_count_ex", "dsn_mesh_simplify_emit_ex",
    "dsn_mesh_smooth_workspace_bytes", "dsn_mesh_smooth", "dsn_mesh_smooth_ex", "dsn_mesh_vertex_normals", "dsn_mesh_vertex_normals_ex",
    "dsn_mesh_dist_workspace_bytes", "dsn_mesh_dist_grid_host", "dsn_mesh_dist_build", "dsn_mesh_dist_query",
    "dsn_mesh_dist_reduce_workspace_bytes", "dsn_mesh_dist_reduce", "dsn_mesh_sample_workspace_bytes", "dsn_mesh_sample_surface",
    "dsn_train_loss_workspace_bytes", "dsn_train_loss", "dsn_train_loss_grad",
    "dsn_grid_hier_workspace_bytes", "dsn_grid_hier_mark", "dsn_grid_hier_list", "dsn_grid_hier_assemble",
    "dsn_density_points_workspace_bytes", "dsn_density_points",
    "dsn_adam_step", "dsn_adam_scalars_host", "dsn_train_draws",
    "dsn_body_shape", "dsn_body_pose_workspace_bytes", "dsn_body_pose",
    "dsn_grad_workspace_layout",
    "dsn_image_undistort", "dsn_image_morph", "dsn_image_resize", "dsn_image_prep",
    "dsn_lpips_packed_bytes", "dsn_lpips_pack", "dsn_lpips_workspace_bytes", "dsn_lpips_features", "dsn_lpips",
    "dsn_jpeg_max_bytes", "dsn_jpeg_workspace_bytes", "dsn_jpeg_header_host", "dsn_jpeg_coefficients", "dsn_jpeg_scan", "dsn_jpeg_encode",
    "dsn_jpeg_parse_host", "dsn_jpegd_workspace_bytes", "dsn_jpegd_workspace_coef", "dsn_jpegd_sync", "dsn_jpegd_coefficients",
    "dsn_jpegd_pixels", "dsn_jpeg_decode",
    "dsn_png_parse_host", "dsn_png_workspace_bytes", "dsn_png_workspace_layout", "dsn_png_decode",
    "dsn_png_encode_max_bytes", "dsn_png_encode_workspace_bytes", "dsn_png_deflate_max_bytes", "dsn_png_deflate_workspace_bytes",
    "dsn_png_filter", "dsn_png_adler", "dsn_png_deflate", "dsn_huff_lengths", "dsn_png_container", "dsn_png_encode",
]

SKIP_TRANSPARENT = 1
NN_EXHAUSTIVE = 2
FIELD_FP32 = 4
SAMPLE_UNIFORM = 8
DENSITY_SCREEN = 16           # opt-in since ABI 5 (was NO_SCREEN with the opposite meaning)
SCREEN_AUDIT = 32
EARLY_STOP, STOP_STATS = 64, 128
PHASE_GEOMETRY, PHASE_FIELD, PHASE_SHADE = 256, 512, 1024      # dsn_render_rays: enqueue only these parts of the frame (0 = all)
SHARE_CUS = 2048              # frames in flight: the persistent field kernels take 7/8 of the compute units (dsnerf.h)
CNT_STOP = 56                 # [56] samples left out by ray termination, [57] samples not shaded, [58] STOP_STATS: what early stop would leave out
CNT_BYTES = 8192              # bytes of the workspace's count area (256 diagnostic words + the slice histogram of STOP_STATS from word 256)
CNT_HIST = 256
CNT_COLOUR_MAX = 59           # largest |colour| the compositor of an eval frame weighed (float bits): the scale of the early-stop bound
EARLY_STOP_COLOUR_HEADROOM = 2.0   # the colour scale handed to the library = this x the largest colour seen so far (Renderer / bench.py)
EARLY_STOP_MIN_SKIPPED = 0.04  # Renderer / bench.py: share of the non-transparent samples early stop must leave out before the slicing pays (it costs ~0.5 ms = 3 % of a 512 x 512 x 64 frame when it leaves out nothing)
SCREEN_MARGIN_FLOOR, SCREEN_MARGIN_CAP = 0.002, 0.15      # = F16_SCREEN_FLOOR / F16_SCREEN_CAP of csrc/dsn_field16.hip
SCREEN_HEADROOM = 10.0        # = F16_SCREEN_HEADROOM: every calibration point is this factor in deviation away from a wrong drop
SCREEN_MIN_DROPPED = 0.35     # PackedParams.calibrate_screen: below this share of dropped calibration points the screen stays off
RAYS_ZJU, RAYS_H36M = 0, 1
TRAIN_RAYS_OK, TRAIN_RAYS_EMPTY_CLASS, TRAIN_RAYS_SHORT, TRAIN_RAYS_BAD_CAMERA = 0, 1, 2, 3     # dsn_train_rays' status (DSN_TRAIN_RAYS_*)
TRAIN_RAYS_MAX_ROUNDS, TRAIN_RAYS_MAX_RAYS = 64, 65536
SSIM_OK, SSIM_CROP_TOO_SMALL, SSIM_EMPTY_MASK = 0, 1, 2     # dsn_image_ssim's out_status (DSN_SSIM_*)
LOSS_L2, LOSS_SMOOTH_L1 = 0, 1      # dsn_train_loss' kind (DSN_LOSS_*)
LPIPS_NETS = {"alex": 0, "vgg": 1}                                          # DSN_LPIPS_ALEX / DSN_LPIPS_VGG
LPIPS_OK, LPIPS_TOO_SMALL, LPIPS_RANGE, LPIPS_NONFINITE = 0, 1, 2, 4        # dsn_lpips' out_status: an OR of DSN_LPIPS_*
LPIPS_RANGE_MAX, LPIPS_TILE_M = 32768.0, 64                                 # DSN_LPIPS_RANGE_MAX / DSN_LPIPS_TILE_M
LPIPS_WORKSPACE_CAP = 8 << 30       # lpips() / lpips_features() chunk their stacks so that one call's workspace stays below this
LOSS_SHARE = 256                    # rays per workgroup of dsn_train_loss' forward (DSN_LOSS_SHARE)
FRAME_FINE_ONLY = 1           # dsn_set_frame_ex: only the fine nearest-face level of the posed mesh (points beyond it: exhaustive sweep)
FRAME_LAZY_LISTS = 2          # dsn_set_frame_ex: grid geometry only - the frame that uses the level builds the lists of the cells it visits
LAZY_LISTS = 4096             # dsn_render_rays_ex: ... which is this flag (Scene.lazy says whether the scene's frame was set that way)
# int32 words of the render workspace the library leaves diagnostics in (include/dsnerf.h)
CNT_ACTIVE, CNT_POS, CNT_KEEP, CNT_AUDIT, CNT_RANGE = 0, 16, 32, 40, 48
CNT_SEL, CNT_LIT = 13, 14       # DSN_EARLY_STOP frames: slots of the reverse pass, shaded samples (DSN_CNT_SEL / DSN_CNT_LIT)


def lib():
    """Load the HIP library (raises if it has not been built: python dual-space-nerf_amd/build.py)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing - build it with `python dual-space-nerf_amd/build.py` "
                "(hipcc --offload-arch=gfx950). There is no fallback path.")
        L = C.CDLL(LIB_PATH)
        L.dsn_last_error.restype = C.c_char_p
        L.dsn_early_stop_eps.restype = C.c_float
        L.dsn_early_stop_eps_scaled.restype = C.c_float
        L.dsn_early_stop_colour_headroom.restype = C.c_float
        L.dsn_render_workspace_record_capacity.restype = C.c_int64
        L.dsn_render_workspace_record_capacity.argtypes = [C.c_int, C.c_int, C.c_size_t]
        L.dsn_render_workspace_bytes_for.argtypes = [C.c_int, C.c_int, C.c_float]
        for n in ("dsn_packed_param_bytes", "dsn_scene_bytes", "dsn_render_workspace_bytes", "dsn_render_workspace_bytes_for", "dsn_field_record_bytes",
                  "dsn_grad_workspace_bytes", "dsn_image_workspace_bytes", "dsn_pose_state_bytes",
                  "dsn_calibrate_workspace_bytes", "dsn_image_ssim_workspace_bytes"):
            getattr(L, n).restype = C.c_size_t
        L.dsn_render_lights_scratch_bytes.restype = C.c_size_t
        L.dsn_render_lights_scratch_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64]
        L.dsn_render_maps_scratch_bytes.restype = C.c_size_t
        L.dsn_render_maps_scratch_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64]
        L.dsn_density_grid_workspace_bytes.restype = C.c_size_t
        L.dsn_density_grid_workspace_bytes.argtypes = [C.c_int64]
        L.dsn_mc_workspace_bytes.restype = C.c_size_t
        L.dsn_mc_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.dsn_mc_table_host.argtypes = [C.c_void_p, C.c_size_t]
        L.dsn_density_grid.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]
        L.dsn_mc_count.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dsn_mc_emit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int,
                                  C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dsn_mc_normals.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int,
                                     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.dsn_raster_workspace_bytes.restype = C.c_size_t
        L.dsn_raster_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int]
        raster = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_int,
                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.dsn_raster_mesh.argtypes = raster + [C.c_void_p]
        L.dsn_raster_mesh_ex.argtypes = raster + [C.c_int, C.c_int, C.c_void_p]
        L.dsn_raster_mesh_attr.argtypes = raster + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dsn_mesh_cc_workspace_bytes.restype = C.c_size_t
        L.dsn_mesh_cc_workspace_bytes.argtypes = [C.c_int64, C.c_int64]
        cc_label = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        cc_emit = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dsn_mesh_cc_label.argtypes = cc_label + [C.c_void_p]
        L.dsn_mesh_cc_label_ex.argtypes = cc_label + [C.c_int, C.c_void_p]
        L.dsn_mesh_cc_emit.argtypes = cc_emit + [C.c_void_p]
        L.dsn_mesh_cc_emit_ex.argtypes = cc_emit + [C.c_int, C.c_void_p]
        L.dsn_bound_mask.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.dsn_train_rays_workspace_bytes.restype = C.c_size_t
        L.dsn_train_rays_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.dsn_train_rays.argtypes = ([C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_uint32]
                                     + [C.c_void_p] * 12 + [C.c_size_t, C.c_void_p])
        L.dsn_mesh_bind_normals.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.dsn_mesh_pose_workspace_bytes.restype = C.c_size_t
        L.dsn_mesh_pose_workspace_bytes.argtypes = [C.c_int, C.c_int]
        L.dsn_mesh_pose.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 5
        L.dsn_mesh_stretch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.dsn_mesh_simplify_workspace_bytes.restype = C.c_size_t
        L.dsn_mesh_simplify_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_void_p]
        sp_count = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        sp_emit = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                   C.c_void_p]
        L.dsn_mesh_simplify_count.argtypes = sp_count + [C.c_void_p]
        L.dsn_mesh_simplify_count_ex.argtypes = sp_count + [C.c_int, C.c_void_p]
        L.dsn_mesh_simplify_emit.argtypes = sp_emit + [C.c_void_p]
        L.dsn_mesh_simplify_emit_ex.argtypes = sp_emit + [C.c_int, C.c_void_p]
        L.dsn_mesh_simplify_cells.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.dsn_mesh_smooth_workspace_bytes.restype = C.c_size_t
        L.dsn_mesh_smooth_workspace_bytes.argtypes = [C.c_int64, C.c_int64]
        sm = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        sm_normals = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        L.dsn_mesh_smooth.argtypes = sm + [C.c_void_p]
        L.dsn_mesh_smooth_ex.argtypes = sm + [C.c_int, C.c_void_p]
        L.dsn_mesh_vertex_normals.argtypes = sm_normals + [C.c_void_p]
        L.dsn_mesh_vertex_normals_ex.argtypes = sm_normals + [C.c_int, C.c_void_p]
        L.dsn_mesh_dist_workspace_bytes.restype = C.c_size_t
        L.dsn_mesh_dist_workspace_bytes.argtypes = [C.c_int64, C.c_int64]
        L.dsn_mesh_dist_grid_host.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.dsn_mesh_dist_build.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.dsn_mesh_dist_query.argtypes = ([C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64]
                                          + [C.c_void_p] * 4)
        L.dsn_mesh_dist_reduce_workspace_bytes.restype = C.c_size_t
        L.dsn_mesh_dist_reduce_workspace_bytes.argtypes = [C.c_int64]
        L.dsn_mesh_dist_reduce.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.dsn_mesh_sample_workspace_bytes.restype = C.c_size_t
        L.dsn_mesh_sample_workspace_bytes.argtypes = [C.c_int64]
        L.dsn_mesh_sample_surface.argtypes = ([C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_int64, C.c_void_p, C.c_size_t]
                                              + [C.c_void_p] * 3)
        L.dsn_train_loss_workspace_bytes.restype = C.c_size_t
        L.dsn_train_loss_workspace_bytes.argtypes = [C.c_int64]
        L.dsn_train_loss.argtypes = [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 3
        L.dsn_train_loss_grad.argtypes = [C.c_void_p] * 6 + [C.c_int64, C.c_int] + [C.c_void_p] * 5
        L.dsn_grid_hier_workspace_bytes.restype = C.c_size_t
        L.dsn_grid_hier_workspace_bytes.argtypes = [C.c_int] * 4
        L.dsn_grid_hier_mark.argtypes = [C.c_void_p] + [C.c_int] * 8 + [C.c_float, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.dsn_grid_hier_list.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p]
        L.dsn_grid_hier_assemble.argtypes = ([C.c_void_p] + [C.c_int] * 7 + [C.c_float, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int64]
                                             + [C.c_void_p] * 3)
        L.dsn_density_points_workspace_bytes.restype = C.c_size_t
        L.dsn_density_points_workspace_bytes.argtypes = [C.c_int64]
        L.dsn_density_points.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]
        L.dsn_adam_step.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p] + [C.c_double] * 4 + [C.c_void_p, C.c_void_p]
        L.dsn_adam_scalars_host.argtypes = [C.c_double] * 6 + [C.c_void_p]
        L.dsn_train_draws.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 3
        L.dsn_body_shape.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        L.dsn_body_pose_workspace_bytes.restype = C.c_size_t
        L.dsn_body_pose_workspace_bytes.argtypes = [C.c_int, C.c_int]
        L.dsn_body_pose.argtypes = ([C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 6
                                    + [C.c_size_t, C.c_void_p])
        L.dsn_grad_workspace_layout.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.dsn_image_undistort.argtypes = [C.c_void_p] * 4 + [C.c_int] * 6 + [C.c_void_p]
        L.dsn_image_morph.argtypes = [C.c_void_p] * 2 + [C.c_int] * 5 + [C.c_void_p]
        L.dsn_image_resize.argtypes = [C.c_void_p] * 2 + [C.c_int] * 7 + [C.c_void_p]
        L.dsn_image_prep.argtypes = [C.c_void_p] * 4 + [C.c_int] * 7 + [C.c_void_p] * 5
        L.dsn_lpips_packed_bytes.restype = C.c_size_t
        L.dsn_lpips_packed_bytes.argtypes = [C.c_int]
        L.dsn_lpips_workspace_bytes.restype = C.c_size_t
        L.dsn_lpips_workspace_bytes.argtypes = [C.c_int] * 4
        L.dsn_lpips_pack.argtypes = [C.c_int] + [C.c_void_p] * 5
        L.dsn_lpips_features.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]
        L.dsn_lpips.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]
        L.dsn_jpeg_max_bytes.restype = C.c_size_t
        L.dsn_jpeg_max_bytes.argtypes = [C.c_int] * 3
        L.dsn_jpeg_workspace_bytes.restype = C.c_size_t
        L.dsn_jpeg_workspace_bytes.argtypes = [C.c_int] * 4
        L.dsn_jpeg_header_host.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p]
        L.dsn_jpeg_coefficients.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_float] + [C.c_void_p] * 3
        L.dsn_jpeg_scan.argtypes = [C.c_void_p] * 2 + [C.c_int] * 5 + [C.c_void_p, C.c_size_t] + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]
        L.dsn_jpeg_encode.argtypes = ([C.c_void_p] + [C.c_int] * 7 + [C.c_float] + [C.c_void_p, C.c_size_t] + [C.c_void_p] * 3
                                      + [C.c_size_t, C.c_void_p])
        L.dsn_jpeg_parse_host.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.dsn_jpegd_workspace_bytes.restype = C.c_size_t
        L.dsn_jpegd_workspace_bytes.argtypes = [C.c_int] * 4 + [C.c_size_t]
        L.dsn_jpegd_workspace_coef.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_size_t, C.c_void_p]
        L.dsn_jpegd_sync.argtypes = ([C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_size_t] + [C.c_int] * 3
                                     + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p])
        L.dsn_jpegd_coefficients.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_size_t, C.c_int] + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]
        L.dsn_jpegd_pixels.argtypes = ([C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_size_t] + [C.c_int] * 2 + [C.c_void_p] * 2
                                       + [C.c_size_t, C.c_void_p])
        L.dsn_jpeg_decode.argtypes = ([C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_size_t] + [C.c_int] * 4
                                      + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p])
        L.dsn_png_parse_host.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.dsn_png_workspace_bytes.restype = C.c_size_t
        L.dsn_png_workspace_bytes.argtypes = [C.c_int] * 5 + [C.c_size_t]
        L.dsn_png_workspace_layout.argtypes = [C.c_int] * 5 + [C.c_size_t, C.c_void_p]
        L.dsn_png_decode.argtypes = ([C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_size_t]
                                     + [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p])
        L.dsn_png_encode_max_bytes.restype = C.c_size_t
        L.dsn_png_encode_max_bytes.argtypes = [C.c_int] * 4
        L.dsn_png_encode_workspace_bytes.restype = C.c_size_t
        L.dsn_png_encode_workspace_bytes.argtypes = [C.c_int] * 5
        L.dsn_png_deflate_max_bytes.restype = C.c_size_t
        L.dsn_png_deflate_max_bytes.argtypes = [C.c_size_t, C.c_int]
        L.dsn_png_deflate_workspace_bytes.restype = C.c_size_t
        L.dsn_png_deflate_workspace_bytes.argtypes = [C.c_int, C.c_size_t, C.c_int]
        L.dsn_png_filter.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_float, C.c_int] + [C.c_void_p] * 3
        L.dsn_png_adler.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.dsn_png_deflate.argtypes = ([C.c_void_p, C.c_int, C.c_size_t] + [C.c_int] * 4 + [C.c_void_p, C.c_size_t] + [C.c_void_p] * 3
                                      + [C.c_size_t, C.c_void_p])
        L.dsn_huff_lengths.argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 2
        L.dsn_png_container.argtypes = ([C.c_void_p, C.c_size_t] + [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p, C.c_size_t]
                                        + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p])
        L.dsn_png_encode.argtypes = ([C.c_void_p] + [C.c_int] * 6 + [C.c_float] + [C.c_int] * 3 + [C.c_void_p, C.c_size_t] + [C.c_void_p] * 3
                                     + [C.c_size_t, C.c_void_p])
        if L.dsn_abi_version() != 8:
            raise RuntimeError(f"{LIB_PATH} has ABI version {L.dsn_abi_version()}, this binding needs 8 - rebuild it "
                               "(python dual-space-nerf_amd/build.py)")
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {lib().dsn_last_error().decode()}")


def cpu_quota_cores():
    """CPU bandwidth this process may use, in cores, from the cgroup (v2 cpu.max / v1 cpu.cfs_quota_us); None = unlimited / unknown.
    os.cpu_count() and the affinity mask do not see it: the GPU boxes show 256 hardware threads under a quota of 16 cores."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
        return None if q == "max" else float(q) / float(per)
    except Exception:
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
            q = int(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            per = int(f.read())
        return None if q <= 0 else q / float(per)
    except Exception:
        return None


_pool_warned = False


def fit_host_pool(keep=False):
    """Cap torch's intra-op pool at the cgroup's CPU quota (minus two cores for the thread that feeds the GPU and the HIP
    runtime's helper threads).  torch sizes its OpenMP pool from the hardware thread count (128-256 on the GPU boxes) whatever the
    quota (16 cores there): every torch CPU op of the CALLER (test.py:61-76 runs torch.clamp / psnr / .cpu() between frames) then
    wakes a team that burns the whole 100 ms quota period in a few milliseconds of busy-waiting at the pool's dock, the kernel
    freezes the container for the rest of the period, and a 19 ms frame takes 60-90 ms (scripts/h2h_guard_probe.py,
    profiles/r03a_h2h_guard.json: nr_throttled counts them; mean 36 ms in BENCH_r02).  No quota, pool already small, or
    DSN_HOST_POOL=keep / keep=True (Renderer(host_pool="keep")): nothing happens.  Lowering the caller's setting is said once, as a
    warning (it is process-global: it also applies to the caller's own CPU work).  Returns (threads before, threads now, quota)."""
    global _pool_warned
    before = torch.get_num_threads()
    quota = cpu_quota_cores()
    if keep or quota is None or os.environ.get("DSN_HOST_POOL", "") == "keep":
        return before, before, quota
    # one process per GPU: the quota is shared by the processes of this node (torchrun exports LOCAL_WORLD_SIZE)
    try:
        local_world = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))
    except ValueError:
        local_world = 1
    want = max(1, int(quota / local_world) - 2)
    if before > want:
        torch.set_num_threads(want)
        if not _pool_warned:
            _pool_warned = True
            import warnings
            warnings.warn(f"dsnerf_amd: torch.set_num_threads({want}) (was {before}): this process may use {quota:g} cores (cgroup quota"
                          f"{', shared by ' + str(local_world) + ' local ranks' if local_world > 1 else ''}) and a larger intra-op pool gets it "
                          "throttled while frames are in flight.  Renderer(host_pool=\"keep\") or DSN_HOST_POOL=keep leave the pool alone.")
    return before, torch.get_num_threads(), quota


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("dsnerf_amd needs a ROCm device (gfx950); no CPU fallback exists")


def _scratch(nbytes, device):
    """opaque device scratch for the library (scene blobs, workspaces): uninitialised, as the C ABI allows.  DSN_POISON_SCRATCH=1 (tests):
    every byte 0xFF - NaN floats, -1 integers - so that nothing can come to rely on a fresh allocation reading as zeros"""
    t = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    if os.environ.get("DSN_POISON_SCRATCH"):
        t.fill_(255)
    return t


def _output(shape, dtype, device):
    """an output tensor the library fills completely: uninitialised; DSN_POISON_SCRATCH=1 (tests): every byte 0xFF, as _scratch"""
    t = torch.empty(shape, dtype=dtype, device=device)
    if os.environ.get("DSN_POISON_SCRATCH"):
        t.view(torch.uint8).fill_(255)
    return t


def _ptr(t, dtype=None):
    if t is None:
        return C.c_void_p(0)
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensor required"
    if dtype is not None:
        assert t.dtype == dtype, (t.dtype, dtype)
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t, device):
    return t.to(device=device, dtype=torch.float32).contiguous()


class PackedParams:
    """MFMA-ordered device image of the 33 state_dict tensors (dsn_pack_params)."""

    def __init__(self, device):
        require_gpu()
        self.device = torch.device(device)
        self.buf = torch.zeros(lib().dsn_packed_param_bytes(), dtype=torch.uint8, device=self.device)
        self._versions = None
        self._keep = None
        self.generation = 0        # bumped by every re-pack: what calibrations / caches of derived state key on
        self.screen = None         # dict(deviation, margin, overflow_fraction, points, usable) once calibrate_screen() has run
        self.early_stop = None     # dict(skipped_fraction, usable) once a frame's DSN_STOP_STATS have been read (Renderer / bench.py)
        self.colour_scale = 1.0    # colour scale of the early-stop threshold in the packed image (set_early_stop_colour_scale)

    def update(self, state: dict, force=False):
        """state: name -> tensor (any device).  Re-packs only when a tensor changed (data pointer / version counter).
        Edits made through `param.data` do not bump the version counter: pass force=True (or call net.packed(force=True))
        after such an edit."""
        tensors = [state[k] for k in PARAM_ORDER]
        versions = tuple((t.data_ptr(), t._version) for t in tensors)
        if not force and versions == self._versions:
            return self
        dev = [_f32(t.detach(), self.device) for t in tensors]
        ptrs = (C.c_void_p * len(dev))(*[t.data_ptr() for t in dev])
        _check(lib().dsn_pack_params(ptrs, _ptr(self.buf), _stream()), "dsn_pack_params")
        self._keep = dev  # keep sources alive until the pack kernel has run (stream-ordered)
        self._repacked(versions)
        return self

    def _repacked(self, versions):
        self._versions = versions
        self.generation += 1
        self.screen = None         # the packed image carries the conservative default margin again
        self.early_stop = None
        self.colour_scale = 1.0    # (dsn_pack_params resets it)

    def note_repacked(self, tensors):
        """The image was rebuilt outside update() from the 33 `tensors` (PARAM_ORDER), as they are now - adam_step(..., packed=self)
        does that behind its update: update()'s bookkeeping, so that the next update() of the same tensors launches nothing."""
        assert len(tensors) == len(PARAM_ORDER)
        self._keep = None          # (the image was packed from the parameters themselves)
        self._repacked(tuple((t.data_ptr(), t._version) for t in tensors))
        return self

    def set_early_stop_colour_scale(self, scale: float):
        """colour scale c of DSN_EARLY_STOP's threshold eps(S, c) = min(2^-20, 1e-4 / (2 (S + 1) max(1, c))) for these parameters:
        frames stay within (S + 1) eps c' of the one-pass frame for colours up to c' - half of the 1e-4 bar, absolute, while c' <= c."""
        scale = max(1.0, float(scale))
        _check(lib().dsn_set_early_stop_colour_scale(_ptr(self.buf), C.c_float(scale), _stream()), "dsn_set_early_stop_colour_scale")
        self.colour_scale = scale
        return scale

    def screen_pays(self, early_stop_on: bool = False) -> bool:
        """Is the (calibrated) density screen worth running?  `usable` of calibrate_screen, except that with ray termination in use
        the share of samples it drops counts among the samples that are still evaluated: what termination leaves out is the dense
        interior, which the screen could never drop - dropped / (1 - skipped) >= SCREEN_MIN_DROPPED."""
        sc = self.screen
        if not sc:
            return False
        if not early_stop_on or not self.early_stop or sc.get("dropped_fraction") is None or not sc.get("safe"):
            return bool(sc["usable"])
        f = min(max(float(self.early_stop.get("skipped_fraction", 0.0)), 0.0), 0.99)
        return sc["dropped_fraction"] / (1.0 - f) >= SCREEN_MIN_DROPPED

    def calibrate_screen(self, scene: "Scene", n_points: int = 1 << 20, other_frames=(0, 125, 250, 375, 499), frame=None):
        """Measure the density screen's margin for THESE parameters (dsn_calibrate_screen; synchronises: meant to run once per
        checkpoint, Renderer does it lazily before the first eval-mode frame after the parameters changed): on the scene's
        current frame state with n_points points, and - the first layer's bias depends on the frame's embedding row - with the
        same pose under a spread of other frame codes (`other_frames`, n_points / 4 points each).  The margin leaves every point
        seen a factor 10 of headroom in deviation against a wrong drop (include/dsnerf.h: margin = 10 max(dev - rel / 10), at least
        0.002, +inf above 0.15).  Returns / stores dict(deviation, margin_statistic, margin, overflow_fraction, points,
        dropped_fraction, safe, usable); safe = False: the screen would need a margin above the cap; usable = safe and it
        drops enough samples to pay for itself.
        frame = (RenderWorkspace, R, S) of a frame whose geometry phase has run (render_rays(..., phases=PHASE_GEOMETRY)): the
        calibration points are then the canonical points of that frame's non-transparent samples (+ a 2 cm halo) instead of a cube
        around the canonical centroids - what Renderer and bench.py do: the margin and the share the screen drops are measured on what
        is rendered (dsn_calibrate_screen_frame)."""
        ws = _scratch(lib().dsn_calibrate_workspace_bytes(C.c_int64(n_points)), self.device)
        out = torch.zeros(8, dtype=torch.float32, device=self.device)

        def run(n):
            if frame is not None:       # (render workspace, R, S) of a frame whose geometry phase has run: calibrate on ITS points
                rws, R_, S_ = frame
                _check(lib().dsn_calibrate_screen_frame(_ptr(scene.buf), scene.V, scene.F, _ptr(self.buf), _ptr(rws.buf), int(R_), int(S_),
                                                        C.c_int64(n), _ptr(ws), _ptr(out), _stream()), "dsn_calibrate_screen_frame")
            else:
                _check(lib().dsn_calibrate_screen(_ptr(scene.buf), scene.V, scene.F, _ptr(self.buf), C.c_int64(n), _ptr(ws), _ptr(out),
                                                  _stream()), "dsn_calibrate_screen")
            return [float(v) for v in out.cpu()[:6]]

        state = getattr(scene, "_pose_args", None)          # (poses, frame_idx, zero_code, light_shift, rot, rot_center) of set_frame
        d = t = ovf = 0.0
        total = 0
        if state is not None and not state[2] and other_frames:
            poses, frame_idx, zero_code, ls, r, rc = state
            for f in other_frames:
                if f == frame_idx:
                    continue
                _set_pose(scene.buf, self, poses, None, f, zero_code, ls, r, rc, self.device)
                d2, _, ovf2, n2, _, t2 = run(max(n_points // 4, 1024))
                d, t, ovf, total = max(d, d2), max(t, t2), max(ovf, ovf2), total + n2
            _set_pose(scene.buf, self, poses, None, frame_idx, zero_code, ls, r, rc, self.device)      # back to the frame's own state
        if frame is not None:
            # ... and the cube around the canonical centroids under the frame's own state (the points of ONE frame - let alone
            # of its first chunk - are a sample of what a sequence visits; the margin is that of the joint set, never below the cube's)
            _frame, frame = frame, None
            d2, _, ovf2, n2, _, t2 = run(max(n_points // 4, 1024))
            d, t, ovf, total = max(d, d2), max(t, t2), max(ovf, ovf2), total + n2
            frame = _frame
        # the frame's own state last, with the other states' statistic carried in (out[7]): the margin it leaves in the packed image and
        # the share of points it counts as dropped are those of the joint set
        out[7:8].fill_(t)
        d1, m, ovf1, n1, dropped, t = run(n_points)
        d, ovf, total = max(d, d1), max(ovf, ovf1), total + n1
        safe = bool(m < float("inf"))
        # The screen costs ~0.3 of an accurate forward pass per sample (k_screen16 0.71 us vs k_field16<forward> 2.36 us per
        # thousand samples): it pays only if it drops more than that share.  A network that is dense everywhere near the
        # surface (every calibration point sigma > 0) is better off without it.
        self.screen = {"deviation": d, "margin_statistic": t, "margin": m, "overflow_fraction": ovf, "points": int(total),
                       "dropped_fraction": dropped, "safe": safe, "usable": safe and dropped >= SCREEN_MIN_DROPPED,
                       "points_from": "frame + centroid cube" if frame is not None else "centroid cube"}
        return self.screen

    def set_screen_margin(self, margin: float):
        _check(lib().dsn_set_screen_margin(_ptr(self.buf), C.c_float(margin), _stream()), "dsn_set_screen_margin")
        self.screen = {"deviation": None, "margin": float(margin), "overflow_fraction": None, "points": 0, "dropped_fraction": None,
                       "safe": None, "usable": margin < float("inf")}   # (a margin <= 0 is unsafe: tests use it to provoke the audit)
        return self.screen


class Scene:
    """Body model + per-frame state blob (dsn_set_body / dsn_set_frame)."""

    def __init__(self, canonical_vertex, faces, device):
        require_gpu()
        self.device = torch.device(device)
        canon = _f32(canonical_vertex.reshape(-1, 3), self.device)
        f = faces.to(device=self.device, dtype=torch.int32).contiguous()
        self.V, self.F = canon.shape[0], f.shape[0]
        self.buf = _scratch(lib().dsn_scene_bytes(self.V, self.F), self.device)
        _check(lib().dsn_set_body(_ptr(self.buf), _ptr(canon), _ptr(f), self.V, self.F, _stream()), "dsn_set_body")
        self._keep = (canon, f)
        self.frame_key = None
        # Nearest-face list levels that do not fit their (fixed) capacity are switched off by the build and every query falls through to
        # the next level / the exhaustive sweep - same index, 10-50x slower (silently).  The canonical mesh's levels are
        # built once: looked at here (one synchronisation at set-up); the posed mesh's are rebuilt per frame: their headers are copied
        # out asynchronously every NN_WATCH_EVERY-th frame and looked at when the next frame is set (nn_watch()).
        off = (C.c_size_t * 4)()
        _check(lib().dsn_nn_header_offsets(self.V, self.F, off), "dsn_nn_header_offsets")
        self._nn_off = [int(o) for o in off]
        self._nn_probe = None
        self._nn_host = None
        self._nn_frames = 0
        self.lazy = False              # the current frame was set with DSN_FRAME_LAZY_LISTS (render_rays then passes DSN_LAZY_LISTS)
        self.nn_overflow = {}          # level name -> (entries needed, capacity) of every overflow seen
        st = nn_stats(self)
        for name in ("canon_fine", "canon_coarse"):
            self._judge_level(name, st[name])

    NN_WATCH_EVERY = 16
    _NN_NAMES = ("world_fine", "world_coarse", "canon_fine", "canon_coarse")

    def _judge_level(self, name, rec):
        ncell, ok, total, cap = rec
        if cap <= 0:          # a level that was not built (fine-only frames leave the posed mesh's coarse level switched off)
            return
        if total > cap and name not in self.nn_overflow:
            import warnings
            warnings.warn(f"dsnerf_amd: the {name.replace('_', ' ')} nearest-face level of this mesh needs {total} list entries, its capacity is "
                          f"{cap}: the level is switched off and its queries take the next level / the exhaustive sweep over all {self.F} "
                          "centroids - same results, but the nearest-face search of every frame is several times slower "
                          "(Scene.nn_overflow; a mesh far denser than SMPL's 13 776 faces per body needs larger DSN capacities)")
        if total > cap:
            self.nn_overflow[name] = (int(total), int(cap))

    def nn_watch(self, wait=False):
        """look at the posed mesh's level headers an earlier frame left (no wait unless asked); returns the overflow record"""
        if self._nn_probe is not None:
            snap, ev = self._nn_probe
            if wait or ev.query():
                ev.synchronize()
                self._nn_probe = None
                w = snap.view(torch.int32)
                for i, name in enumerate(self._NN_NAMES[:2]):
                    self._judge_level(name, tuple(int(w[16 * i + k]) for k in (8, 9, 10, 11)))
        return self.nn_overflow

    def _watch_headers(self):
        """copy the posed mesh's two level headers out (asynchronously, into ONE persistent page-locked buffer: ADVICE r04 - a fresh
        pin_memory() per probe is a hipHostMalloc on the hot path) for nn_watch() to look at later"""
        if self._nn_host is None:
            self._nn_host = torch.empty(128, dtype=torch.uint8).pin_memory()
        host = self._nn_host
        for i in range(2):      # world fine / coarse headers, 64 bytes each
            host[64 * i:64 * i + 64].copy_(self.buf[self._nn_off[i]:self._nn_off[i] + 64], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._nn_probe = (host, ev)

    def set_frame(self, packed: PackedParams, xyz, poses, frame_idx: int, zero_code: bool = False,
                  light_shift=None, rot=None, rot_center=None, reuse: bool = False, fine_only: bool = False, lazy: bool = False):
        """reuse=True: skip the call when the scene already holds exactly this frame for these parameters (same tensors at
        the same versions) - used by the backward of a training step, which follows its own forward.
        fine_only=True (DSN_FRAME_FINE_ONLY): build only the fine nearest-face level of the posed mesh - enough for every sample
        of rays clipped to the body's bounds (what Renderer.render / render_view produce); points further than 0.12 m outside the
        posed centroids' box then take the exhaustive sweep (same index).
        lazy=True (DSN_FRAME_LAZY_LISTS, implies fine_only): only the fine grid is laid out; render_rays on this scene then builds
        the lists of the cells ITS samples visit (it passes DSN_LAZY_LISTS while Scene.lazy is set).  Stage calls on a lazily set
        scene (warp, lbs_warp, a training forward) stay exact but take the exhaustive sweep: set the frame without `lazy` for those."""
        vkey = lambda a: None if a is None else (a.data_ptr(), a._version, tuple(a.shape))
        key = (vkey(xyz), vkey(poses), int(frame_idx), bool(zero_code), vkey(light_shift), vkey(rot), vkey(rot_center),
               id(packed), packed._versions, bool(fine_only), bool(lazy))
        if reuse and key == self.frame_key:
            return self
        self.frame_key = key
        # (a lazily set frame's lists - and the header that says whether they fit - are completed by its render call: what the previous
        #  frame left is looked at here, before this frame overwrites it)
        self.nn_watch()
        if self.lazy and self._nn_probe is None and self._nn_frames % self.NN_WATCH_EVERY == 1:
            self._watch_headers()
        self.lazy = bool(lazy)
        xyz = _f32(xyz.reshape(-1, 3), self.device)
        assert xyz.shape[0] == self.V, "xyz must have the body model's vertex count"
        poses = _f32(poses.reshape(24, 3), self.device)
        ls = None if light_shift is None else _f32(light_shift.reshape(-1)[:3], self.device)
        r = None if rot is None else _f32(rot.reshape(-1)[:4], self.device)
        rc = None if rot_center is None else _f32(rot_center.reshape(-1)[:2], self.device)
        _check(lib().dsn_set_frame_ex(_ptr(self.buf), self.V, self.F, _ptr(packed.buf), _ptr(xyz), _ptr(poses),
                                      int(frame_idx), int(bool(zero_code)), _ptr(ls), _ptr(r), _ptr(rc),
                                      (FRAME_LAZY_LISTS | FRAME_FINE_ONLY) if lazy else (FRAME_FINE_ONLY if fine_only else 0), _stream()),
               "dsn_set_frame")
        self._keep_frame = (xyz, poses, ls, r, rc)
        self._pose_args = (poses, int(frame_idx), bool(zero_code), ls, r, rc)
        if not lazy and self._nn_probe is None and self._nn_frames % self.NN_WATCH_EVERY == 0:
            self._watch_headers()
        self._nn_frames += 1
        return self


def _set_pose(buf, packed, poses, pose_feat, frame_idx, zero_code, light_shift, rot, rot_center, device):
    f = lambda a, n: None if a is None else _f32(a.reshape(-1)[:n], device)
    po = None if poses is None else _f32(poses.reshape(24, 3), device)
    pf, ls, r, rc = f(pose_feat, 16), f(light_shift, 3), f(rot, 4), f(rot_center, 2)
    _check(lib().dsn_set_pose(_ptr(buf), _ptr(packed.buf), _ptr(po), _ptr(pf), int(frame_idx), int(bool(zero_code)), _ptr(ls),
                              _ptr(r), _ptr(rc), _stream()), "dsn_set_pose")
    return (po, pf, ls, r, rc)


def scene_set_pose(scene: Scene, packed: PackedParams, poses, frame_idx, zero_code=False, light_shift=None, rot=None,
                   rot_center=None, pose_feat=None):
    """pose code / embedding row / light edits of a scene, mesh untouched (dsn_set_pose)."""
    scene._keep_pose = _set_pose(scene.buf, packed, poses, pose_feat, frame_idx, zero_code, light_shift, rot, rot_center, scene.device)
    scene.frame_key = None     # no longer the state a set_frame(reuse=True) left
    scene._pose_args = None
    return scene


class PoseState:
    """Per-frame network state WITHOUT a body model (dsn_pose_state_bytes): all a density-only query or a stand-alone
    SpaceNet.forward needs.  Quacks like a Scene for `field()` (V = F = 0)."""

    def __init__(self, device):
        require_gpu()
        self.device = torch.device(device)
        self.V = self.F = 0
        self.buf = torch.zeros(lib().dsn_pose_state_bytes(), dtype=torch.uint8, device=self.device)

    def set_pose(self, packed: PackedParams, poses, frame_idx, zero_code=False, light_shift=None, rot=None, rot_center=None,
                 pose_feat=None):
        self._keep = _set_pose(self.buf, packed, poses, pose_feat, frame_idx, zero_code, light_shift, rot, rot_center, self.device)
        return self


def light(packed: PackedParams, normal, xyz_world, view_dir_world, essence, fp32=False):
    """model/spacenet.py:174-188 LightingMLP.forward as a pure function (dsn_light): [N,3] x 4 -> colour [N,3]."""
    dev = packed.device
    a = [_f32(t.reshape(-1, 3), dev) for t in (normal, xyz_world, view_dir_world, essence)]
    N = a[0].shape[0]
    assert all(t.shape[0] == N for t in a), "normal, xyz_world, view_dir_world and essence_feature must have one row per point"
    col = torch.empty(N, 3, dtype=torch.float32, device=dev)
    scratch = _scratch(lib().dsn_pose_state_bytes(), dev)
    _check(lib().dsn_light(_ptr(packed.buf), _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), C.c_int64(N), _ptr(col), _ptr(scratch),
                           FIELD_FP32 if fp32 else 0, _stream()), "dsn_light")
    return col


def nn_stats(scene: Scene):
    """Diagnostics (synchronising): dict level -> (ncell, ok, total, cap)."""
    out = (C.c_int32 * 16)()
    _check(lib().dsn_debug_nn_stats(_ptr(scene.buf), scene.V, scene.F, out, _stream()), "dsn_debug_nn_stats")
    names = ["world_fine", "world_coarse", "canon_fine", "canon_coarse"]
    return {n: tuple(out[4 * i:4 * i + 4]) for i, n in enumerate(names)}


# ------------------------------------------------------------------------------------------------
# stage calls (device tensors in, device tensors out)
# ------------------------------------------------------------------------------------------------
def sample(scene: Scene, ray_o, ray_d, near, far, S, t_vals, jitter=None, want_pts=True, gg=True):
    """near/far are updated in place (like utils/pts_utils.py:52-53)."""
    R = ray_o.shape[0]
    dev = scene.device
    z = torch.empty(R, S, dtype=torch.float32, device=dev)
    pts = torch.empty(R, S, 3, dtype=torch.float32, device=dev) if want_pts else None
    fn = lib().dsn_sample_gg if gg else lib().dsn_sample_uniform
    _check(fn(_ptr(scene.buf), scene.V, scene.F, _ptr(ray_o, torch.float32), _ptr(ray_d, torch.float32),
              _ptr(near, torch.float32), _ptr(far, torch.float32), R, S, _ptr(t_vals, torch.float32), _ptr(jitter),
              _ptr(z), _ptr(pts), _stream()), "dsn_sample")
    return pts, z


def warp(scene: Scene, pts, ray_d, S, want_dir=True, want_uvh=False, want_active=False, exhaustive=False):
    pts = pts.reshape(-1, 3)
    N = pts.shape[0]
    dev = scene.device
    out = {
        "face_idx": torch.empty(N, dtype=torch.int32, device=dev),
        "transparent": torch.empty(N, dtype=torch.uint8, device=dev),
        "x_c": torch.empty(N, 3, dtype=torch.float32, device=dev),
    }
    uv = h = rdc = lst = cnt = None
    if want_uvh:
        uv = out["uv"] = torch.empty(N, 2, dtype=torch.float32, device=dev)
        h = out["h"] = torch.empty(N, dtype=torch.float32, device=dev)
    if want_dir and ray_d is not None:
        rdc = out["ray_d_can"] = torch.empty(N, 3, dtype=torch.float32, device=dev)
    if want_active:
        lst = out["active_list"] = torch.empty(N, dtype=torch.int32, device=dev)
        cnt = out["active_count"] = torch.zeros(64, dtype=torch.int32, device=dev)
    _check(lib().dsn_warp(_ptr(scene.buf), scene.V, scene.F, _ptr(pts, torch.float32), _ptr(ray_d), C.c_int64(N), S,
                          _ptr(out["face_idx"]), _ptr(uv), _ptr(h), _ptr(out["transparent"]), _ptr(out["x_c"]),
                          _ptr(rdc), _ptr(lst), _ptr(cnt), NN_EXHAUSTIVE if exhaustive else 0, _stream()), "dsn_warp")
    return out


def field(scene: Scene, packed: PackedParams, x_c, want_essence=True, want_grad=True, active=None, fp32=False):
    x_c = x_c.reshape(-1, 3)
    N = x_c.shape[0]
    dev = scene.device
    sigma = torch.zeros(N, dtype=torch.float32, device=dev)
    ess = torch.zeros(N, 3, dtype=torch.float32, device=dev) if want_essence else None
    g = torch.zeros(N, 3, dtype=torch.float32, device=dev) if want_grad else None
    lst, cnt = (None, None) if active is None else active
    _check(lib().dsn_field(_ptr(scene.buf), scene.V, scene.F, _ptr(packed.buf), _ptr(x_c, torch.float32), C.c_int64(N),
                           _ptr(lst), _ptr(cnt), _ptr(sigma), _ptr(ess), _ptr(g), FIELD_FP32 if fp32 else 0, _stream()),
           "dsn_field")
    return sigma, ess, g


def field_forward(scene: Scene, packed: PackedParams, x_c, active=None):
    """sigma, essence for the listed points + the list of points with sigma > 0 (see dsn_field_forward)."""
    x_c = x_c.reshape(-1, 3)
    N = x_c.shape[0]
    dev = scene.device
    sigma = torch.zeros(N, dtype=torch.float32, device=dev)
    ess = torch.zeros(N, 3, dtype=torch.float32, device=dev)
    rec = _scratch(lib().dsn_field_record_bytes(C.c_int64(N)), dev)
    pos = torch.zeros(N, dtype=torch.int32, device=dev)
    pcnt = torch.zeros(1, dtype=torch.int32, device=dev)
    lst, cnt = (None, None) if active is None else active
    _check(lib().dsn_field_forward(_ptr(scene.buf), scene.V, scene.F, _ptr(packed.buf), _ptr(x_c, torch.float32), C.c_int64(N),
                                   _ptr(lst), _ptr(cnt), _ptr(sigma), _ptr(ess), _ptr(rec), _ptr(pos), _ptr(pcnt), _stream()),
           "dsn_field_forward")
    return sigma, ess, rec, (pos, pcnt)


def field_reverse(scene: Scene, packed: PackedParams, x_c, rec, pos, sigma, essence):
    """sigma / essence: the arrays field_forward returned (samples it flagged as outside the fp16 range are re-evaluated
    here in exact fp32, all three outputs)."""
    x_c = x_c.reshape(-1, 3)
    N = x_c.shape[0]
    g = torch.zeros(N, 3, dtype=torch.float32, device=scene.device)
    _check(lib().dsn_field_reverse(_ptr(scene.buf), scene.V, scene.F, _ptr(packed.buf), _ptr(x_c, torch.float32), C.c_int64(N),
                                   _ptr(pos[0]), _ptr(pos[1]), _ptr(rec), _ptr(g), _ptr(sigma, torch.float32),
                                   _ptr(essence, torch.float32), _stream()), "dsn_field_reverse")
    return g


DENSITY_GRID_SLAB_POINTS = 1 << 25      # default slab of dsn_density_grid: 32 M points (~1 GB of scratch), whole x-planes


def _axes_dev(axes, device):
    out = [(a if torch.is_tensor(a) else torch.from_numpy(__import__("numpy").asarray(a))).to(device=device, dtype=torch.float32)
           .reshape(-1).contiguous() for a in axes]
    assert len(out) == 3, "three axis arrays (x, y, z)"
    return out


def density_grid(scene: Scene, packed: PackedParams, axes, slab_points=None, fp32=False, exhaustive=False):
    """dsn_density_grid: the density volume [nx, ny, nz] (device float32) of the grid axes (x, y, z) for the scene's current frame
    (transparent points 0).  slab_points: scratch bound in points, rounded down to whole x-planes (default
    DENSITY_GRID_SLAB_POINTS, at least one plane)."""
    dev = scene.device
    x, y, z = _axes_dev(axes, dev)
    nx, ny, nz = x.numel(), y.numel(), z.numel()
    plane = ny * nz
    P = int(slab_points) if slab_points is not None else max(plane, min(DENSITY_GRID_SLAB_POINTS, nx * plane))
    vol = torch.empty(nx, ny, nz, dtype=torch.float32, device=dev)
    nbytes = lib().dsn_density_grid_workspace_bytes(P)
    ws = _scratch(max(nbytes, 1), dev)
    flags = (FIELD_FP32 if fp32 else 0) | (NN_EXHAUSTIVE if exhaustive else 0)
    _check(lib().dsn_density_grid(_ptr(scene.buf), scene.V, scene.F, _ptr(packed.buf), _ptr(x), nx, _ptr(y), ny, _ptr(z), nz, flags,
                                  _ptr(vol), P, _ptr(ws), nbytes, _stream()), "dsn_density_grid")
    return vol


MC_GRADIENT = {"descent": 0, "ascent": 1}
MC_MAX_TRI = 5               # DSN_MC_MAX_TRI


def mc_table():
    """the marching-cubes case table (host function): int32 [256, DSN_MC_TABLE_ROW] - count, then cube-edge triples (-1 padded)"""
    import numpy as np
    row = 1 + 3 * MC_MAX_TRI
    out = np.zeros((256, row), dtype=np.int32)
    _check(lib().dsn_mc_table_host(out.ctypes.data, out.size), "dsn_mc_table_host")
    return out


def marching_cubes(volume, axes, level, gradient_direction="descent", want_normals=False):
    """dsn_mc_count + dsn_mc_emit on a device volume [nx, ny, nz]: (verts [V,3] float32, faces [T,3] int32) device tensors, both empty
    where the level is not crossed.  One device->host read (the two counts).  want_normals: a third tensor, the unit vertex normals
    [V,3] float32 of dsn_mc_normals (verts and faces keep their bits)."""
    if gradient_direction not in MC_GRADIENT:
        raise ValueError('gradient_direction must be "descent" or "ascent"')
    vol = volume
    assert vol.is_cuda and vol.dtype == torch.float32 and vol.dim() == 3, "volume: device float32 [nx, ny, nz]"
    vol = vol.contiguous()
    dev = vol.device
    x, y, z = _axes_dev(axes, dev)
    nx, ny, nz = vol.shape
    assert (x.numel(), y.numel(), z.numel()) == (nx, ny, nz), "one axis value per grid point along each axis"
    ws = _scratch(max(lib().dsn_mc_workspace_bytes(nx, ny, nz), 1), dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    _check(lib().dsn_mc_count(_ptr(vol), nx, ny, nz, float(level), _ptr(ws), _ptr(counts), _stream()), "dsn_mc_count")
    V, T = (int(c) for c in counts.cpu())
    verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(T, 3, dtype=torch.int32, device=dev)
    _check(lib().dsn_mc_emit(_ptr(vol), nx, ny, nz, _ptr(x), _ptr(y), _ptr(z), float(level), MC_GRADIENT[gradient_direction], _ptr(ws),
                             V, T, _ptr(verts) if V else None, _ptr(faces) if T else None, _stream()), "dsn_mc_emit")
    if not want_normals:
        return verts, faces
    normals = torch.empty(V, 3, dtype=torch.float32, device=dev)
    _check(lib().dsn_mc_normals(_ptr(vol), nx, ny, nz, _ptr(x), _ptr(y), _ptr(z), float(level), MC_GRADIENT[gradient_direction], _ptr(ws),
                                V, _ptr(normals) if V else None, _stream()), "dsn_mc_normals")
    return verts, faces, normals


GRID_HIER_FACTORS = (2, 4, 8, 16)


def grid_hier_axes(axes, factor):
    """the coarse lattice of a grid (rule 1 of include/dsnerf.h's coarse-to-fine grid): per axis the int64 numpy array of the fine
    indices 0, c, 2c, ... < n, plus n - 1 if it is not among them.  `axes`: the three axis arrays, or their three lengths."""
    import numpy as np
    if factor not in GRID_HIER_FACTORS:
        raise ValueError(f"factor must be one of {GRID_HIER_FACTORS}")
    out = []
    for a in axes:
        n = int(a) if isinstance(a, (int, np.integer)) else len(a)
        if n < 2:
            raise ValueError("every grid axis needs at least 2 points")
        idx = list(range(0, n, factor))
        if idx[-1] != n - 1:
            idx.append(n - 1)
        out.append(np.asarray(idx, dtype=np.int64))
    return tuple(out)


def density_points(scene: Scene, packed: PackedParams, axes, index, slab_points=None, fp32=False, exhaustive=False):
    """dsn_density_points: values [m] float32 (device) = density_grid(scene, packed, axes).reshape(-1)[index[m]], bit for bit, for a
    device int32 list `index` of linear grid indices (i ny + j) nz + k in any order, duplicates allowed.  slab_points: scratch bound
    in points (default DENSITY_GRID_SLAB_POINTS, at most the list); the result does not depend on it."""
    dev = scene.device
    x, y, z = _axes_dev(axes, dev)
    nx, ny, nz = x.numel(), y.numel(), z.numel()
    index = index.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    M = index.numel()
    values = _output(M, torch.float32, dev)
    if M == 0:
        return values
    P = int(slab_points) if slab_points is not None else min(DENSITY_GRID_SLAB_POINTS, M)
    nbytes = lib().dsn_density_points_workspace_bytes(P)
    ws = _scratch(max(nbytes, 1), dev)
    flags = (FIELD_FP32 if fp32 else 0) | (NN_EXHAUSTIVE if exhaustive else 0)
    _check(lib().dsn_density_points(_ptr(scene.buf), scene.V, scene.F, _ptr(packed.buf), _ptr(x), nx, _ptr(y), ny, _ptr(z), nz,
                                    _ptr(index), M, flags, _ptr(values), P, _ptr(ws), nbytes, _stream()), "dsn_density_points")
    return values


def grid_hier_mark(coarse, shape, factor, dilate, level):
    """dsn_grid_hier_mark on a device coarse volume [mx, my, mz] of the grid `shape` = (nx, ny, nz): (workspace, counts) - counts a
    device int64 [3]: core cells, active cells, evaluated points."""
    assert coarse.is_cuda and coarse.dtype == torch.float32 and coarse.dim() == 3, "coarse: device float32 [mx, my, mz]"
    coarse = coarse.contiguous()
    nx, ny, nz = (int(n) for n in shape)
    nbytes = lib().dsn_grid_hier_workspace_bytes(nx, ny, nz, int(factor))
    ws = _scratch(max(nbytes, 1), coarse.device)
    counts = _output(3, torch.int64, coarse.device)
    mx, my, mz = coarse.shape
    _check(lib().dsn_grid_hier_mark(_ptr(coarse), mx, my, mz, nx, ny, nz, int(factor), int(dilate), float(level), _ptr(ws), nbytes,
                                    _ptr(counts), _stream()), "dsn_grid_hier_mark")
    return ws, counts


def grid_hier_list(ws, shape, factor, n_points):
    """dsn_grid_hier_list: the ascending device int32 list of the n_points evaluated points (n_points: counts[2] of grid_hier_mark)"""
    nx, ny, nz = (int(n) for n in shape)
    index = _output(int(n_points), torch.int32, ws.device)
    _check(lib().dsn_grid_hier_list(nx, ny, nz, int(factor), _ptr(ws), ws.numel(), int(n_points), _ptr(index) if n_points else None,
                                    _stream()), "dsn_grid_hier_list")
    return index


def grid_hier_assemble(coarse, shape, factor, level, ws, index, values):
    """dsn_grid_hier_assemble: (volume [nx, ny, nz] device float32 - the fill everywhere, then the listed values - and the device
    int64 [1] number of leaking edges)"""
    coarse = coarse.contiguous()
    nx, ny, nz = (int(n) for n in shape)
    mx, my, mz = coarse.shape
    M = index.numel()
    assert values.numel() == M and values.dtype == torch.float32 and index.dtype == torch.int32
    vol = _output((nx, ny, nz), torch.float32, coarse.device)
    leaks = _output(1, torch.int64, coarse.device)
    _check(lib().dsn_grid_hier_assemble(_ptr(coarse), mx, my, mz, nx, ny, nz, int(factor), float(level), _ptr(ws), ws.numel(),
                                        _ptr(index.contiguous()) if M else None, _ptr(values.contiguous()) if M else None, M, _ptr(vol),
                                        _ptr(leaks), _stream()), "dsn_grid_hier_assemble")
    return vol, leaks


def density_grid_hier(scene: Scene, packed: PackedParams, axes, level, factor=4, dilate=1, slab_points=None, fp32=False, evaluate=None):
    """The density volume of density_grid, evaluated coarse to fine (the rule of include/dsnerf.h): the density at the coarse lattice
    of grid_hier_axes(axes, factor), then only at the fine points in the closed boxes of the coarse cells the level crosses, dilated
    `dilate` times; every other point holds the coarse value at the lowest corner of its owner cell.  Returns (volume [nx, ny, nz]
    device float32, info) with info = {factor, dilate, coarse_shape, core_cells, active_cells, evaluated_points, points, leaks}.
    What info["leaks"] == 0 proves: every vertex and every normal marching_cubes(volume, ...) returns was computed from evaluated
    values only - where the volume also has the dense grid's inside mask, verts, faces and normals are the dense grid's, bit for bit.
    What it does not: a piece of surface wholly among unevaluated points (a floater smaller than a coarse cell, more than `dilate`
    cells from any coarse sign change) is neither seen nor counted.
    evaluate: a callable index (device int32 [m]) -> values (device float32 [m]) that replaces the field (scene and packed may then
    be None).  Listed coarse points are evaluated again (about 1 / factor^3 of the list; the bits are the same).  Two device->host
    reads (the counts, the leaks)."""
    dev = scene.device if scene is not None else torch.device("cuda", torch.cuda.current_device())
    x, y, z = _axes_dev(axes, dev)
    shape = (x.numel(), y.numel(), z.numel())
    if evaluate is None:
        def evaluate(index):
            return density_points(scene, packed, (x, y, z), index, slab_points=None if slab_points is None else min(int(slab_points), max(index.numel(), 1)),
                                  fp32=fp32)
    ix, iy, iz = (torch.from_numpy(a).to(dev) for a in grid_hier_axes(shape, factor))
    lin = ((ix[:, None, None] * shape[1] + iy[None, :, None]) * shape[2] + iz[None, None, :]).to(torch.int32)
    coarse = evaluate(lin.reshape(-1)).reshape(lin.shape).contiguous()
    ws, counts = grid_hier_mark(coarse, shape, factor, dilate, level)
    core, active, n_eval = (int(c) for c in counts.cpu())
    index = grid_hier_list(ws, shape, factor, n_eval)
    values = evaluate(index) if n_eval else torch.empty(0, dtype=torch.float32, device=dev)
    vol, leaks = grid_hier_assemble(coarse, shape, factor, level, ws, index, values)
    info = {"factor": int(factor), "dilate": int(dilate), "coarse_shape": tuple(coarse.shape), "core_cells": core, "active_cells": active,
            "evaluated_points": n_eval, "points": shape[0] * shape[1] * shape[2], "leaks": int(leaks.cpu())}
    return vol, info


MESH_CC_TILE = 1024          # DSN_MESH_CC_TILE: vertices / faces per tile of the compaction scans
CC_INIT, CC_UNITE, CC_FLATTEN, CC_SUMS, CC_SELECT, CC_COUNT, CC_EMIT_VERTS, CC_EMIT_FACES = 1, 2, 4, 8, 16, 32, 64, 128      # DSN_CC_*


def mesh_area_shift(lo, hi, n_faces):
    """area_shift of dsn_mesh_cc_label (the rule of include/dsnerf.h) from the bounding box lo [3], hi [3] of the vertices whose
    coordinates are all finite (None: there is none): 61 - bit_length(T) - e, clamped to +-60, e the frexp exponent of float32 D2"""
    import numpy as np
    e = 0
    if lo is not None:
        with np.errstate(over="ignore", invalid="ignore"):
            d = np.asarray(hi, np.float32) - np.asarray(lo, np.float32)
            d2 = np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        e = int(np.frexp(d2)[1]) if np.isfinite(d2) else 128
    return max(-60, min(60, 61 - int(n_faces).bit_length() - e))


def _mesh_cc_inputs(verts, faces):
    assert verts.is_cuda and faces.is_cuda, "verts and faces: device tensors"
    verts = verts.reshape(-1, 3).to(torch.float32).contiguous()
    faces = faces.reshape(-1, 3).to(torch.int32).contiguous()
    V, T = verts.shape[0], faces.shape[0]
    lo = hi = None
    if V:
        fin = torch.isfinite(verts).all(dim=1, keepdim=True)
        inf = torch.tensor(float("inf"), device=verts.device)
        box = torch.cat([torch.where(fin, verts, inf).amin(dim=0), torch.where(fin, verts, -inf).amax(dim=0)]).cpu().numpy()
        if box[0] <= box[3]:                       # (no finite vertex: +inf > -inf)
            lo, hi = box[:3], box[3:]
    return verts, faces, V, T, mesh_area_shift(lo, hi, T)


def _mesh_cc_label(verts, faces, V, T, shift, want_labels, phases=0, state=None):
    dev = verts.device
    nbytes = lib().dsn_mesh_cc_workspace_bytes(V, T)
    if nbytes == 0:
        raise RuntimeError("dsn_mesh_cc_label: the mesh must stay below 2^31 vertices and faces")
    if state is None:
        state = {"ws": _scratch(nbytes, dev), "counts": torch.empty(6, dtype=torch.int64, device=dev),
                 "labels": torch.empty(V, dtype=torch.int32, device=dev) if want_labels else None}
    labels = state["labels"]
    _check(lib().dsn_mesh_cc_label_ex(_ptr(verts) if V else None, _ptr(faces) if T else None, V, T, shift, _ptr(state["ws"]), nbytes,
                                      _ptr(labels) if labels is not None and V else None, _ptr(state["counts"]), int(phases), _stream()),
           "dsn_mesh_cc_label")
    return state, nbytes


def mesh_components(verts, faces):
    """dsn_mesh_cc_label (the rule of include/dsnerf.h) on a device mesh (verts [V,3] float32, faces [T,3] int32): the connected
    components under the shared-vertex-index rule.  Returns {"labels" [V] int32 on the device (a component's label is its smallest vertex
    index; -1: the vertex is in no valid face), "n_components", "winner" (the label of the component with the largest area, -1: none),
    "area" (the winner's, float), "faces_in_winner", "n_verts" / "n_faces" (of the winner), "area_shift", "area_sum" (the integer the
    area comes from)}.  One device->host read of the six counts behind one of the bounding box (six floats: the shift is a host
    argument of the call)."""
    require_gpu()
    verts, faces, V, T, shift = _mesh_cc_inputs(verts, faces)
    st, _ = _mesh_cc_label(verts, faces, V, T, shift, True)
    n, winner, nv, nf, s, fw = (int(c) for c in st["counts"].cpu())
    return {"labels": st["labels"], "n_components": n, "winner": winner, "area": math.ldexp(float(s), -shift - 1), "faces_in_winner": fw,
            "n_verts": nv, "n_faces": nf, "area_shift": shift, "area_sum": s}


def largest_component(verts, faces, want_source=True, info=None):
    """dsn_mesh_cc_label + dsn_mesh_cc_emit: the component of the mesh with the largest area (ties: the smaller label) as a mesh of its
    own - (verts' [V',3] float32, faces' [T',3] int32, source_vertex [V'] int32 or None) device tensors; vertices and faces keep their
    order and winding, source_vertex holds each kept vertex's old index (per-vertex arrays follow by a[source_vertex.long()]).  A mesh
    without a valid face gives three empty tensors.  One device->host read of the six counts, behind one of the bounding box.  info: a
    dict that receives n_components, winner, area, faces_in_winner and area_shift."""
    require_gpu()
    verts, faces, V, T, shift = _mesh_cc_inputs(verts, faces)
    dev = verts.device
    st, nbytes = _mesh_cc_label(verts, faces, V, T, shift, False)
    n, winner, nv, nf, s, fw = (int(c) for c in st["counts"].cpu())
    out_v = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    src = torch.empty(nv, dtype=torch.int32, device=dev) if want_source else None
    _check(lib().dsn_mesh_cc_emit(_ptr(verts) if V else None, _ptr(faces) if T else None, V, T, _ptr(st["ws"]), nbytes, nv, nf,
                                  _ptr(out_v) if nv else None, _ptr(out_f) if nf else None, _ptr(src) if want_source and nv else None,
                                  _stream()), "dsn_mesh_cc_emit")
    if info is not None:
        info.update(n_components=n, winner=winner, area=math.ldexp(float(s), -shift - 1), faces_in_winner=fw, area_shift=shift)
    return out_v, out_f, src


MESH_SIMPLIFY_MAX_G, MESH_SIMPLIFY_MAX_CLUSTERS = 4096, 1 << 21      # DSN_MESH_SIMPLIFY_MAX_G, 2^DSN_MESH_SIMPLIFY_MAX_LOG2
MESH_SIMPLIFY_TOO_MANY, MESH_SIMPLIFY_TABLE_FULL = 1, 2               # DSN_MESH_SIMPLIFY_*: the status word of the counts
SP_ZERO, SP_MARK, SP_RANK, SP_SUM, SP_PICK, SP_FACES, SP_KEEP, SP_EMIT_VERTS, SP_EMIT_FACES = 1, 2, 4, 8, 16, 32, 64, 128, 256      # DSN_SP_*
MESH_SIMPLIFY_COUNTS = ("n_clusters", "n_faces", "live_faces", "duplicates_dropped", "vertices_outside", "bad_index_faces", "status")


def _finite_box(verts):
    """(lo [3], hi [3]) float32 numpy over the vertices whose coordinates are all finite, or None (one device->host read of six floats)"""
    if verts.shape[0] == 0:
        return None
    fin = torch.isfinite(verts).all(dim=1, keepdim=True)
    inf = torch.tensor(float("inf"), device=verts.device)
    box = torch.cat([torch.where(fin, verts, inf).amin(dim=0), torch.where(fin, verts, -inf).amax(dim=0)]).cpu().numpy()
    return (box[:3], box[3:]) if box[0] <= box[3] else None


def mesh_simplify_grid(box, cell, origin=None, g=None):
    """(origin float32 [3], g [3] ints) of dsn_mesh_simplify_* from the finite bounding box `box` = (lo, hi) or None: origin defaults to
    lo (zeros without a finite vertex), g_a to floor((hi_a - origin_a) inv) + 1 in the rule's float32 operations, so that every
    finite vertex is inside"""
    import numpy as np
    f32 = np.float32
    if origin is None:
        origin = np.zeros(3, f32) if box is None else box[0]
    origin = np.ascontiguousarray(np.asarray(origin, f32).reshape(3))
    if g is None:
        if box is None:
            g = [1, 1, 1]
        else:
            with np.errstate(all="ignore"):
                tt = (np.asarray(box[1], f32) - origin) * (f32(1.0) / f32(cell))
            g = [max(int(np.floor(x)) + 1, 1) if np.isfinite(x) else MESH_SIMPLIFY_MAX_G + 1 for x in tt]
    g = [int(x) for x in g]
    if len(g) != 3:
        raise ValueError("mesh_simplify: g must hold three cell counts")
    return origin, g


def _mesh_simplify_check_grid(cell, origin, g):
    import numpy as np
    c = np.float32(cell)
    if not (np.isfinite(c) and c > 0 and np.isfinite(np.float32(1.0) / c)):
        raise ValueError(f"mesh_simplify: cell must be finite and > 0, got {cell!r}")
    if not np.isfinite(origin).all():
        raise ValueError("mesh_simplify: origin must be finite")
    if not all(1 <= x <= MESH_SIMPLIFY_MAX_G for x in g) or g[0] * g[1] * g[2] > (1 << 31):
        raise ValueError(f"mesh_simplify: the grid {g} is outside the limits (each count 1 ... {MESH_SIMPLIFY_MAX_G}, at most 2^31 cells): "
                         "choose a larger cell")
    return float(c), (C.c_int * 3)(*g)


def mesh_cell_count(verts, cell, origin=None, g=None, box=None):
    """dsn_mesh_simplify_cells: K, the number of grid cells the inside vertices of verts [V,3] (device float32) occupy - the vertex count
    mesh_simplify would return.  One device->host read of 8 bytes (behind one of the bounding box unless origin and g, or `box`, are
    given)."""
    require_gpu()
    assert verts.is_cuda, "verts: a device tensor"
    verts = verts.reshape(-1, 3).to(torch.float32).contiguous()
    V = verts.shape[0]
    if box is None and (origin is None or g is None):
        box = _finite_box(verts)
    origin, g = mesh_simplify_grid(box, cell, origin, g)
    c, g3 = _mesh_simplify_check_grid(cell, origin, g)
    nbytes = lib().dsn_mesh_simplify_workspace_bytes(V, 0, g3)
    if nbytes == 0:
        raise RuntimeError("dsn_mesh_simplify_cells: the mesh must stay below 2^31 vertices")
    ws = _scratch(nbytes, verts.device)
    out = torch.empty(1, dtype=torch.int64, device=verts.device)
    _check(lib().dsn_mesh_simplify_cells(_ptr(verts) if V else None, V, origin.ctypes.data, c, g3, _ptr(ws), nbytes, _ptr(out), _stream()),
           "dsn_mesh_simplify_cells")
    return int(out.cpu())


def mesh_simplify(verts, faces, cell, origin=None, g=None, info=None):
    """dsn_mesh_simplify_count + dsn_mesh_simplify_emit (the rule of include/dsnerf.h): vertex clustering on the grid of `cell`-sized
    cells at `origin` with g = (g0, g1, g2) cells, every cluster represented by the member nearest to the members' mean.  Device
    tensors in (verts [V,3] float32, faces [T,3] int32) and out: (verts' [K,3] float32, faces' [T',3] int32, cluster_source [K] int32,
    vertex_cluster [V] int32) - verts' = verts[cluster_source] bit for bit, so per-vertex arrays follow by a[cluster_source.long()];
    vertex_cluster holds the output vertex of every input vertex (-1: outside the grid).  origin defaults to the minimum over the
    vertices whose coordinates are all finite, g to what covers them (mesh_simplify_grid).  One device->host read of the seven counts,
    behind one of the bounding box where a default is taken.  More than 2^21 clusters: ValueError (choose a larger cell).  info: a
    dict that receives the counts (MESH_SIMPLIFY_COUNTS), cell, origin and g."""
    require_gpu()
    assert verts.is_cuda and faces.is_cuda, "verts and faces: device tensors"
    verts = verts.reshape(-1, 3).to(torch.float32).contiguous()
    faces = faces.reshape(-1, 3).to(torch.int32).contiguous()
    V, T = verts.shape[0], faces.shape[0]
    dev = verts.device
    box = _finite_box(verts) if origin is None or g is None else None
    origin, g = mesh_simplify_grid(box, cell, origin, g)
    c, g3 = _mesh_simplify_check_grid(cell, origin, g)
    nbytes = lib().dsn_mesh_simplify_workspace_bytes(V, T, g3)
    if nbytes == 0:
        raise RuntimeError("dsn_mesh_simplify_count: the mesh must stay below 2^31 vertices and faces")
    ws = _scratch(nbytes, dev)
    counts = torch.empty(7, dtype=torch.int64, device=dev)
    vc = torch.empty(V, dtype=torch.int32, device=dev)
    vp, fp = (_ptr(verts) if V else None), (_ptr(faces) if T else None)
    _check(lib().dsn_mesh_simplify_count(vp, fp, V, T, origin.ctypes.data, c, g3, _ptr(ws), nbytes, _ptr(vc) if V else None, _ptr(counts),
                                         _stream()), "dsn_mesh_simplify_count")
    n = [int(x) for x in counts.cpu()]
    if info is not None:
        info.update(dict(zip(MESH_SIMPLIFY_COUNTS, n)), cell=c, origin=origin.copy(), g=list(g))
    if n[6] & MESH_SIMPLIFY_TOO_MANY:
        raise ValueError(f"mesh_simplify: {n[0]} clusters, more than 2^21 = {MESH_SIMPLIFY_MAX_CLUSTERS}: choose a larger cell than {c:g}")
    if n[6]:
        raise RuntimeError(f"dsn_mesh_simplify_count: status {n[6]} (the duplicate table overflowed)")
    K, nf = n[0], n[1]
    out_v = torch.empty(K, 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    src = torch.empty(K, dtype=torch.int32, device=dev)
    _check(lib().dsn_mesh_simplify_emit(vp, fp, V, T, g3, _ptr(ws), nbytes, K, nf, _ptr(out_v) if K else None, _ptr(out_f) if nf else None,
                                        _ptr(src) if K else None, _stream()), "dsn_mesh_simplify_emit")
    return out_v, out_f, src, vc


MESH_TARGET_FACTOR = 1.0 + 2.0 ** -20      # the cell of n cells along the longest extent is a hair wider than extent / n: the far vertex stays in cell n - 1


def mesh_target_cell(box, n):
    """the cell of n cells along the longest finite extent of `box` = (lo, hi): float32(extent / n) (1 + 2^-20), every operation
    float32; 1 where the extent is 0 or there is no finite vertex"""
    import numpy as np
    f32 = np.float32
    if box is None:
        return 1.0
    ext = f32((np.asarray(box[1], f32) - np.asarray(box[0], f32)).max())
    if not (ext > 0 and np.isfinite(ext)):
        return 1.0
    c = f32(f32(ext / f32(n)) * f32(MESH_TARGET_FACTOR))
    return float(c) if (c > 0 and np.isfinite(c) and np.isfinite(f32(1.0) / c)) else 1.0


def mesh_target_search(verts, target_vertices, info=None):
    """The cell for at most `target_vertices` clusters: n = the number of cells along the longest finite extent, bisected in [1, 4096]
    for the largest n with K(n) <= target_vertices by mesh_cell_count - at most 12 probes, one 8-byte host read each.  K(n) is treated
    as monotone; it is not strictly so (a finer grid can by chance occupy fewer cells), so the n found is the bisection's, not
    necessarily the largest that fits.  A grid outside the library's limits counts as too many.  Returns the cell; info receives n and
    the probes."""
    N = int(target_vertices)
    if N < 1:
        raise ValueError("target_vertices must be at least 1")
    verts = verts.reshape(-1, 3).to(torch.float32).contiguous()
    box = _finite_box(verts)
    lo, hi, probes = 1, MESH_SIMPLIFY_MAX_G, []
    while lo < hi:
        mid = (lo + hi + 1) // 2
        probes.append(mid)
        c = mesh_target_cell(box, mid)
        o, g = mesh_simplify_grid(box, c)
        fits = all(1 <= x <= MESH_SIMPLIFY_MAX_G for x in g) and g[0] * g[1] * g[2] <= (1 << 31)
        if fits and mesh_cell_count(verts, c, o, g) <= N:
            lo = mid
        else:
            hi = mid - 1
    if info is not None:
        info.update(n=lo, probes=probes)
    return mesh_target_cell(box, lo)


MESH_SMOOTH_HEAVY, MESH_SMOOTH_MAX_STEPS, MESH_SMOOTH_MAX_EXP = 64, 4096, 900      # DSN_MESH_SMOOTH_*
SM_COUNT, SM_SCAN, SM_FILL, SM_STEP, SM_NORMALS = 1, 2, 4, 8, 16                    # DSN_SM_*
MESH_SMOOTH_COUNTS = ("contributing_faces", "skipped_faces", "vertices_moved", "max_faces_at_vertex")


def mesh_smooth_scale(box):
    """(origin float32 [3], k) of dsn_mesh_smooth from the finite bounding box `box` = (lo, hi) or None (the rule of include/dsnerf.h):
    origin = lo (zeros without a finite vertex), k = 27 - e with e the frexp exponent of the largest extent in double (0 when it is 0),
    so that the box maps to [0, 2^27)"""
    import numpy as np
    if box is None:
        return np.zeros(3, np.float32), 27
    lo, hi = np.asarray(box[0], np.float32).reshape(3), np.asarray(box[1], np.float32).reshape(3)
    D = float(np.max(hi.astype(np.float64) - lo.astype(np.float64)))
    e = int(np.frexp(D)[1]) if D > 0 else 0
    return np.ascontiguousarray(lo), 27 - e


def _mesh_smooth_check(factors, origin, scale_exp):
    import numpy as np
    f = np.ascontiguousarray(np.asarray(factors, np.float32).reshape(-1))
    if f.shape[0] > MESH_SMOOTH_MAX_STEPS:
        raise ValueError(f"mesh_smooth: {f.shape[0]} steps, more than {MESH_SMOOTH_MAX_STEPS}")
    if not np.isfinite(f).all():
        raise ValueError("mesh_smooth: every factor must be finite")
    origin = np.ascontiguousarray(np.asarray(origin, np.float32).reshape(3))
    if not np.isfinite(origin).all():
        raise ValueError("mesh_smooth: origin must be finite")
    k = int(scale_exp)
    if abs(k) > MESH_SMOOTH_MAX_EXP:
        raise ValueError(f"mesh_smooth: scale_exp {k} outside -{MESH_SMOOTH_MAX_EXP} ... {MESH_SMOOTH_MAX_EXP}")
    return f, origin, k


def mesh_smooth(verts, faces, factors, origin=None, scale_exp=None, info=None, phases=0, state=None):
    """dsn_mesh_smooth (the rule of include/dsnerf.h): one umbrella step per entry of `factors` (Taubin: lambda, mu, lambda, mu, ...;
    Laplacian: lambda, lambda, ...) on a device mesh (verts [V,3] float32, faces [T,3] int32).  Returns the moved vertices [V,3] float32
    on the device; faces, vertex count and order do not change.  origin / scale_exp default to mesh_smooth_scale of the vertices'
    finite bounding box (one device->host read of six floats; none when both are given).  info: a dict that receives the counts
    (MESH_SMOOTH_COUNTS: one device->host read of four int64, only then), origin, scale_exp and the factors.  phases / state: the
    measurement entry (scripts/bench_mesh_smooth.py; state = {"ws", "counts", "out"} reused between calls)."""
    require_gpu()
    assert verts.is_cuda and faces.is_cuda, "verts and faces: device tensors"
    verts = verts.reshape(-1, 3).to(torch.float32).contiguous()
    faces = faces.reshape(-1, 3).to(torch.int32).contiguous()
    V, T = verts.shape[0], faces.shape[0]
    dev = verts.device
    if origin is None or scale_exp is None:
        o, k = mesh_smooth_scale(_finite_box(verts))
        origin = o if origin is None else origin
        scale_exp = k if scale_exp is None else scale_exp
    f, origin, k = _mesh_smooth_check(factors, origin, scale_exp)
    nbytes = lib().dsn_mesh_smooth_workspace_bytes(V, T)
    if nbytes == 0:
        raise RuntimeError("dsn_mesh_smooth: the mesh must stay below 2^31 vertices and faces")
    if state is None:
        state = {"ws": _scratch(nbytes, dev), "counts": torch.empty(4, dtype=torch.int64, device=dev),
                 "out": torch.empty(V, 3, dtype=torch.float32, device=dev)}
    _check(lib().dsn_mesh_smooth_ex(_ptr(verts) if V else None, _ptr(faces) if T else None, V, T, origin.ctypes.data, k,
                                    f.ctypes.data if f.shape[0] else None, int(f.shape[0]), _ptr(state["ws"]), nbytes,
                                    _ptr(state["out"]) if V else None, _ptr(state["counts"]), int(phases), _stream()), "dsn_mesh_smooth")
    if info is not None:
        info.update(dict(zip(MESH_SMOOTH_COUNTS, (int(c) for c in state["counts"].cpu()))), origin=origin.copy(), scale_exp=k, factors=f.copy())
    return state["out"]


def mesh_vertex_normals(verts, faces, phases=0, state=None):
    """dsn_mesh_vertex_normals (the rule of include/dsnerf.h): area-weighted unit vertex normals [V,3] float32 from the faces of a device
    mesh, oriented by the winding; (0, 0, 0) at a vertex no face with finite corners uses.  One device->host read of the bounding box
    (six floats: the shift, mesh_area_shift's, is a host argument)."""
    require_gpu()
    verts, faces, V, T, shift = _mesh_cc_inputs(verts, faces)
    dev = verts.device
    nbytes = lib().dsn_mesh_smooth_workspace_bytes(V, T)
    if nbytes == 0:
        raise RuntimeError("dsn_mesh_vertex_normals: the mesh must stay below 2^31 vertices and faces")
    if state is None:
        state = {"ws": _scratch(nbytes, dev), "out": torch.empty(V, 3, dtype=torch.float32, device=dev)}
    _check(lib().dsn_mesh_vertex_normals_ex(_ptr(verts) if V else None, _ptr(faces) if T else None, V, T, shift, _ptr(state["ws"]), nbytes,
                                            _ptr(state["out"]) if V else None, int(phases), _stream()), "dsn_mesh_vertex_normals")
    return state["out"]


MESH_DIST_COUNTS = ("valid_faces", "listed_pairs", "level", "cells")
MESH_DIST_STATS = ("count", "nan_count", "sum_d", "sum_d2", "max_d", "argmax")


def mesh_dist_grid(n_faces, box):
    """(g [3] int, cell float32) of dsn_mesh_dist_build's level-0 grid for `n_faces` faces in the box (lo, hi): the host rule of
    include/dsnerf.h (dsn_mesh_dist_grid_host; no device work)"""
    import numpy as np
    b = np.ascontiguousarray(np.concatenate([np.asarray(box[0], np.float32).reshape(3), np.asarray(box[1], np.float32).reshape(3)]))
    g, cell = np.zeros(3, np.int32), np.zeros(1, np.float32)
    _check(lib().dsn_mesh_dist_grid_host(int(n_faces), b.ctypes.data, g.ctypes.data, cell.ctypes.data), "dsn_mesh_dist_grid_host")
    return g, cell[0]


def mesh_dist_build(verts, faces, box=None, check=True, state=None):
    """dsn_mesh_dist_build (include/dsnerf.h): the search grid over a device mesh (verts [V,3] float32, faces [T,3] int32) that
    mesh_dist_query answers from.  Returns the index: {"verts", "faces", "ws", "nbytes", "counts"} - the mesh as the library reads it, the
    workspace and the device counts (MESH_DIST_COUNTS).  box = (lo, hi): default the bounding box of the finite vertices (one
    device->host read of six floats).  check=True reads the counts (four int64) and raises ValueError for a target without a valid
    face; the numbers land under "info".  An empty mesh (no faces or no vertices) raises ValueError before any device work.
    state: an index of the same face count whose buffers are used again (scripts/bench_mesh_distance.py)."""
    import numpy as np
    require_gpu()
    assert verts.is_cuda and faces.is_cuda, "verts and faces: device tensors"
    verts = verts.reshape(-1, 3).to(torch.float32).contiguous()
    faces = faces.reshape(-1, 3).to(torch.int32).contiguous()
    V, T = verts.shape[0], faces.shape[0]
    if V == 0 or T == 0:
        raise ValueError("mesh_dist_build: an empty target (no faces or no vertices)")
    if box is None:
        box = _finite_box(verts)
        if box is None:
            raise ValueError("mesh_dist_build: the target has no finite vertex, so no valid face")
    b = np.ascontiguousarray(np.concatenate([np.asarray(box[0], np.float32).reshape(3), np.asarray(box[1], np.float32).reshape(3)]))
    nbytes = lib().dsn_mesh_dist_workspace_bytes(V, T)
    if nbytes == 0:
        raise RuntimeError("dsn_mesh_dist_build: the mesh must stay below 2^31 vertices and faces")
    if state is None:
        state = {"ws": _scratch(nbytes, verts.device), "counts": torch.empty(4, dtype=torch.int64, device=verts.device)}
    _check(lib().dsn_mesh_dist_build(_ptr(verts), _ptr(faces), V, T, b.ctypes.data, _ptr(state["ws"]), nbytes, _ptr(state["counts"]),
                                     _stream()), "dsn_mesh_dist_build")
    index = {"verts": verts, "faces": faces, "ws": state["ws"], "nbytes": nbytes, "counts": state["counts"], "box": b}
    if check:
        index["info"] = dict(zip(MESH_DIST_COUNTS, (int(c) for c in state["counts"].cpu())))
        if index["info"]["valid_faces"] == 0:
            raise ValueError("mesh_dist_build: the target has no valid face (indices in range, finite vertices)")
    return index


def mesh_dist_query(index, points, want_distance=True, want_face=True, want_point=True, out=None):
    """dsn_mesh_dist_query (include/dsnerf.h): for every row of `points` [n,3] (device) the nearest point of the mesh behind `index`
    (mesh_dist_build).  Returns {"dist2" [n] float32 - the SQUARED distance -, "face" [n] int32, "point" [n,3] float32} device tensors,
    None for what is not wanted.  A point that is not finite: NaN, -1, NaN.  n = 0 returns empty tensors without a launch.
    out: a dict of the same form whose tensors are filled (scripts/bench_mesh_distance.py)."""
    require_gpu()
    verts, faces = index["verts"], index["faces"]
    points = points.reshape(-1, 3).to(device=verts.device, dtype=torch.float32).contiguous()
    n = points.shape[0]
    dev = verts.device
    if out is None:
        out = {"dist2": _output((n,), torch.float32, dev) if want_distance else None,
               "face": _output((n,), torch.int32, dev) if want_face else None,
               "point": _output((n, 3), torch.float32, dev) if want_point else None}
    _check(lib().dsn_mesh_dist_query(_ptr(verts), _ptr(faces), verts.shape[0], faces.shape[0], _ptr(index["ws"]), index["nbytes"],
                                     _ptr(points) if n else None, n, _ptr(out["dist2"]) if n else None, _ptr(out["face"]) if n else None,
                                     _ptr(out["point"]) if n else None, _stream()), "dsn_mesh_dist_query")
    return out


def mesh_dist_reduce(dist2):
    """dsn_mesh_dist_reduce (include/dsnerf.h): six float64 on the device (MESH_DIST_STATS: count, NaN count, sum d, sum d^2, max d and
    the index of the maximum, -1 without an entry) from squared distances [n] float32, in a fixed order of additions."""
    require_gpu()
    assert dist2.is_cuda
    dist2 = dist2.reshape(-1).to(torch.float32).contiguous()
    n = dist2.shape[0]
    nbytes = lib().dsn_mesh_dist_reduce_workspace_bytes(n)
    ws = _scratch(nbytes, dist2.device)
    out = _output((6,), torch.float64, dist2.device)
    _check(lib().dsn_mesh_dist_reduce(_ptr(dist2) if n else None, n, _ptr(ws), nbytes, _ptr(out), _stream()), "dsn_mesh_dist_reduce")
    return out


def mesh_sample_surface(verts, faces, n, seed=0, want_points=True, want_face=True):
    """dsn_mesh_sample_surface (include/dsnerf.h): `n` area-weighted points on a device mesh, sample i a function of (seed, i) and the
    mesh alone.  Returns (points [n,3] float32, face [n] int32) device tensors (None for what is not wanted)."""
    require_gpu()
    assert verts.is_cuda and faces.is_cuda, "verts and faces: device tensors"
    verts = verts.reshape(-1, 3).to(torch.float32).contiguous()
    faces = faces.reshape(-1, 3).to(torch.int32).contiguous()
    V, T, n = verts.shape[0], faces.shape[0], int(n)
    if V == 0 or T == 0:
        raise ValueError("mesh_sample_surface: an empty mesh (no faces or no vertices)")
    if n < 0:
        raise ValueError("mesh_sample_surface: n must be >= 0")
    nbytes = lib().dsn_mesh_sample_workspace_bytes(T)
    if nbytes == 0:
        raise RuntimeError("dsn_mesh_sample_surface: the mesh must stay below 2^31 vertices and faces")
    ws = _scratch(nbytes, verts.device)
    pts = _output((n, 3), torch.float32, verts.device) if want_points else None
    face = _output((n,), torch.int32, verts.device) if want_face else None
    _check(lib().dsn_mesh_sample_surface(_ptr(verts), _ptr(faces), V, T, int(seed) & 0xFFFFFFFFFFFFFFFF, n, _ptr(ws), nbytes,
                                         _ptr(pts) if n else None, _ptr(face) if n else None, _stream()), "dsn_mesh_sample_surface")
    return pts, face


MESH_POSE_BAD_BINDING = 1    # DSN_MESH_POSE_BAD_BINDING: dsn_mesh_pose's status bit


def _body_faces(body_faces, device):
    return body_faces.to(device=device, dtype=torch.int32).reshape(-1, 3).contiguous()


def mesh_bind_normals(body_xyz, body_faces, face_idx, normals):
    """dsn_mesh_bind_normals (the rule of include/dsnerf.h): the covectors cov [N,3] of normals [N,3] at mesh vertices bound to faces
    face_idx [N] of the posed body (body_xyz [Vb,3], body_faces [Fb,3]) - what dsn_mesh_pose carries to another pose.  Device
    tensors in, a device tensor out."""
    require_gpu()
    dev = normals.device
    body_xyz = _f32(body_xyz, dev).reshape(-1, 3)
    body_faces = _body_faces(body_faces, dev)
    face_idx = face_idx.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    normals = _f32(normals, dev).reshape(-1, 3)
    N = face_idx.shape[0]
    if normals.shape[0] != N:
        raise ValueError(f"mesh_bind_normals: {normals.shape[0]} normals for {N} bound vertices")
    cov = torch.empty(N, 3, dtype=torch.float32, device=dev)
    _check(lib().dsn_mesh_bind_normals(_ptr(body_xyz), body_xyz.shape[0], _ptr(body_faces), body_faces.shape[0],
                                       _ptr(face_idx) if N else None, _ptr(normals) if N else None, N, _ptr(cov) if N else None, _stream()),
           "dsn_mesh_bind_normals")
    return cov


def mesh_pose(binding, body_faces, target_xyz):
    """dsn_mesh_pose (the rule of include/dsnerf.h): the bound vertices of `binding` ({"face_idx" [N] int32, "uv" [N,2], "h" [N],
    "cov" [N,3] or None / absent}: dsn_warp's record per vertex, mesh_bind_normals' covectors) under the bodies target_xyz [P,Vb,3] of
    the topology body_faces [Fb,3].  Returns {"verts" [P,N,3], "normals" [P,N,3] (None without cov),
    "status": an int32 device tensor whose word 0 has MESH_POSE_BAD_BINDING set when a face_idx lay outside [0, Fb) (NaN rows there;
    not read back here)}."""
    require_gpu()
    dev = binding["face_idx"].device
    target_xyz = _f32(target_xyz, dev)
    if target_xyz.dim() != 3 or target_xyz.shape[2] != 3:
        raise ValueError(f"mesh_pose: target_xyz must be [P,Vb,3], got {tuple(target_xyz.shape)}")
    P, Vb = target_xyz.shape[0], target_xyz.shape[1]
    body_faces = _body_faces(body_faces, dev)
    Fb = body_faces.shape[0]
    face_idx = binding["face_idx"].to(dtype=torch.int32).reshape(-1).contiguous()
    N = face_idx.shape[0]
    uv, h = _f32(binding["uv"], dev).reshape(-1, 2), _f32(binding["h"], dev).reshape(-1)
    cov = binding.get("cov")
    cov = None if cov is None else _f32(cov, dev).reshape(-1, 3)
    if uv.shape[0] != N or h.shape[0] != N or (cov is not None and cov.shape[0] != N):
        raise ValueError(f"mesh_pose: the binding's uv / h / cov do not have {N} rows")
    nbytes = lib().dsn_mesh_pose_workspace_bytes(P, Fb)
    if nbytes == 0:
        raise RuntimeError(f"dsn_mesh_pose: bad sizes (P = {P} poses of {Fb} body faces)")
    ws = _scratch(nbytes, dev)
    verts = torch.empty(P, N, 3, dtype=torch.float32, device=dev)
    normals = torch.empty(P, N, 3, dtype=torch.float32, device=dev) if cov is not None else None
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    n = bool(N)
    _check(lib().dsn_mesh_pose(_ptr(target_xyz), P, Vb, _ptr(body_faces), Fb, _ptr(face_idx) if n else None, _ptr(uv) if n else None,
                               _ptr(h) if n else None, _ptr(cov) if n else None, N, _ptr(verts) if n else None,
                               _ptr(normals) if n else None, _ptr(status), _ptr(ws), _stream()), "dsn_mesh_pose")
    return {"verts": verts, "normals": normals, "status": status}


BODY_PADS = {None: 0, "none": 0, "zju_train": 1, "zju_eval": 2, "h36m": 3}      # DSN_BODY_PAD_*
BODY_OUTPUTS = ("xyz", "xyz_smpl", "A", "bounds", "Rh_mat")


def body_parents(parents):
    """24 int32 parents in host memory (a ctypes array) from anything array-like; entry 0 is ignored by the library"""
    p = [int(x) for x in torch.as_tensor(parents).reshape(-1).tolist()]
    if len(p) != 24:
        raise ValueError(f"body model: parents must have 24 entries, got {len(p)}")
    p[0] = -1
    return (C.c_int32 * 24)(*p)


def body_shape(v_template, shapedirs=None, betas=None, J_regressor=None):
    """dsn_body_shape (the rule of include/dsnerf.h): v_template [V,3], shapedirs [V,3,B] and betas [B] (both or neither), a dense
    J_regressor [24,V] or None -> (v_shaped [V,3], joints [24,3] or None).  Device tensors in and out."""
    require_gpu()
    dev = v_template.device
    v_template = _f32(v_template, dev).reshape(-1, 3)
    V = v_template.shape[0]
    B = 0
    if (shapedirs is None) != (betas is None):
        raise ValueError("body_shape: shapedirs and betas go together")
    if betas is not None:
        betas = _f32(betas, dev).reshape(-1)
        B = betas.shape[0]
        shapedirs = _f32(shapedirs, dev)
        if shapedirs.numel() != V * 3 * B:
            raise ValueError(f"body_shape: shapedirs must be [V,3,B] = [{V},3,{B}], got {tuple(shapedirs.shape)}")
    if J_regressor is not None:
        J_regressor = _f32(J_regressor, dev)
        if tuple(J_regressor.shape) != (24, V):
            raise ValueError(f"body_shape: J_regressor must be [24,{V}], got {tuple(J_regressor.shape)}")
    v_shaped = _output((V, 3), torch.float32, dev)
    joints = _output((24, 3), torch.float32, dev) if J_regressor is not None else None
    _check(lib().dsn_body_shape(_ptr(v_template), _ptr(shapedirs) if B else None, _ptr(betas) if B else None, B, _ptr(J_regressor), V,
                                _ptr(v_shaped), _ptr(joints), _stream()), "dsn_body_shape")
    return v_shaped, joints


def body_pose(v_shaped, joints, parents, weights, posedirs, poses, Rh=None, Th=None, pad=None, want=("xyz", "A", "bounds"), workspace=None):
    """dsn_body_pose (the rule of include/dsnerf.h) for the P poses of `poses` [P,24,3] in ONE call: device tensors v_shaped [V,3], joints
    [24,3], weights [V,24], posedirs [207,3V] or None, Rh / Th [P,3] or None; `parents`: body_parents()' host array (or array-like).
    Returns a dict with the outputs named in `want` (BODY_OUTPUTS; "xyz" always).  P = 0: empty tensors, no launch."""
    require_gpu()
    dev = v_shaped.device
    if pad not in BODY_PADS:
        raise ValueError(f"body_pose: pad must be one of {sorted(k for k in BODY_PADS if k)} or None, got {pad!r}")
    unknown = set(want) - set(BODY_OUTPUTS)
    if unknown:
        raise ValueError(f"body_pose: unknown outputs {sorted(unknown)} (known: {BODY_OUTPUTS})")
    if not isinstance(parents, C.Array):
        parents = body_parents(parents)
    if v_shaped.dim() != 2 or v_shaped.shape[1] != 3 or v_shaped.shape[0] < 1:
        raise ValueError(f"body_pose: v_shaped must be [V,3], got {tuple(v_shaped.shape)}")
    V = v_shaped.shape[0]
    for name, t, shape in (("joints", joints, (24, 3)), ("weights", weights, (V, 24)), ("posedirs", posedirs, (207, 3 * V))):
        if t is None and name == "posedirs":
            continue
        if not torch.is_tensor(t) or tuple(t.shape) != shape:
            raise ValueError(f"body_pose: {name} must be a tensor [{shape[0]},{shape[1]}], got {tuple(t.shape) if torch.is_tensor(t) else type(t)}")
    for name, t in (("v_shaped", v_shaped), ("joints", joints), ("weights", weights), ("posedirs", posedirs)):
        if t is not None and (t.dtype != torch.float32 or t.device != dev or not t.is_contiguous()):
            raise ValueError(f"body_pose: {name} must be a contiguous float32 tensor on {dev}, got {t.dtype} on {t.device}")
    if poses.numel() % 72:
        raise ValueError(f"body_pose: poses must be [P,24,3], got {tuple(poses.shape)}")
    poses = _f32(poses, dev).reshape(-1, 24, 3)
    P = poses.shape[0]
    if Rh is not None:
        Rh = _f32(Rh, dev).reshape(-1, 3)
    if Th is not None:
        Th = _f32(Th, dev).reshape(-1, 3)
    if any(t is not None and t.shape[0] != P for t in (Rh, Th)):
        raise ValueError(f"body_pose: Rh / Th must have {P} rows like poses")
    shapes = {"xyz": (P, V, 3), "xyz_smpl": (P, V, 3), "A": (P, 24, 4, 4), "bounds": (P, 2, 3), "Rh_mat": (P, 3, 3)}
    out = {k: _output(shapes[k], torch.float32, dev) for k in BODY_OUTPUTS if k == "xyz" or k in want}
    nbytes = lib().dsn_body_pose_workspace_bytes(V, P)
    if P and nbytes == 0:
        raise RuntimeError(f"dsn_body_pose: bad sizes (V = {V}, P = {P})")
    if P and (workspace is None or workspace.numel() < nbytes):
        workspace = _scratch(nbytes, dev)
    o = lambda k: _ptr(out[k]) if (k in out and P) else None      # noqa: E731
    _check(lib().dsn_body_pose(_ptr(v_shaped, torch.float32), _ptr(joints, torch.float32), parents, _ptr(weights, torch.float32),
                               _ptr(posedirs), V, _ptr(poses) if P else None, _ptr(Rh), _ptr(Th), P, BODY_PADS[pad], o("xyz"), o("xyz_smpl"),
                               o("A"), o("bounds"), o("Rh_mat"), _ptr(workspace) if P else None, nbytes, _stream()), "dsn_body_pose")
    return out


def mesh_stretch(bind_verts, posed_verts, faces):
    """dsn_mesh_stretch (the rule of include/dsnerf.h): per pose and mesh face the largest ratio of a posed edge to the same edge of the
    mesh as it was bound - bind_verts [N,3], posed_verts [P,N,3], faces [T,3] int32 -> [P,T] float32 (device tensors); +inf for a face
    with an index outside [0, N), 1 for a face whose three bound edges have length 0."""
    require_gpu()
    dev = posed_verts.device
    bind_verts = _f32(bind_verts, dev).reshape(-1, 3)
    N = bind_verts.shape[0]
    posed_verts = _f32(posed_verts, dev)
    if posed_verts.dim() != 3 or tuple(posed_verts.shape[1:]) != (N, 3):
        raise ValueError(f"mesh_stretch: posed_verts must be [P,{N},3], got {tuple(posed_verts.shape)}")
    P = posed_verts.shape[0]
    faces = faces.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
    T = faces.shape[0]
    out = torch.empty(P, T, dtype=torch.float32, device=dev)
    _check(lib().dsn_mesh_stretch(_ptr(bind_verts) if N else None, _ptr(posed_verts) if N else None, P, N, _ptr(faces) if T else None, T,
                                  _ptr(out) if T else None, _stream()), "dsn_mesh_stretch")
    return out


RM_CLEAR, RM_PROJECT, RM_RASTER, RM_RASTER_BIG, RM_SHADE = 1, 2, 4, 8, 16      # DSN_RM_*: the kernels of dsn_raster_mesh_ex
RM_BIG_PIXELS = 16           # DSN_RM_BIG_PIXELS
RM_SMOOTH, RM_UNLIT = 1, 2   # DSN_RM_*: the mode word of dsn_raster_mesh_attr


def raster_camera(camera_pose, yfov, height, width):
    """(pose [3, 4] float32 numpy, fx, fy) of dsn_raster_mesh: the reference's camera pose (utils/visualizer.py:150-157) where none is
    given, and the NDC scales of pyrender's PerspectiveCamera(yfov, aspectRatio = width / height) rounded to float32"""
    import numpy as np
    if camera_pose is None:
        camera_pose = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 2.5], [0.0, 0.0, 0.0, 1.0]])
    if torch.is_tensor(camera_pose):
        camera_pose = camera_pose.detach().cpu().numpy()
    pose = np.ascontiguousarray(np.asarray(camera_pose, dtype=np.float64).reshape(4, 4)[:3], dtype=np.float32)
    fy = 1.0 / math.tan(0.5 * float(yfov))
    fx = fy * float(height) / float(width)
    return pose, float(np.float32(fx)), float(np.float32(fy))


def raster_mesh(verts, faces, camera_pose=None, yfov=math.pi / 3, height=1024, width=None, znear=0.05, intensity=30.0,
                inner=math.pi / 16, outer=math.pi / 6, base=0.3, fx=None, fy=None, phases=0, big_pixels=0, out=None,
                vertex_normals=None, vertex_colors=None, smooth=False, lit=True):
    """dsn_raster_mesh (utils/visualizer.py:144-168 render_mesh, the rule of include/dsnerf.h): the mesh (verts [V, 3] float32,
    faces [T, 3] int32, device tensors) seen by a pinhole camera at the camera-to-world pose `camera_pose` (4 x 4; default the
    reference's: the identity at (0, 0, 2.5)) under a spotlight riding with the camera.  Returns {"color" [H, W, 3] uint8 (255 where
    empty), "depth" [H, W] float32 (0 where empty), "face" [H, W] int32 (-1 where empty)} device tensors.  fx / fy: the NDC scales
    themselves instead of yfov and the aspect width / height.  phases / big_pixels / out: dsn_raster_mesh_ex's measurement switches
    (scripts/bench_render_mesh.py; `out` = a dict of an earlier call whose tensors and workspace are used again).
    vertex_normals / vertex_colors [V, 3] float32, smooth, lit=False: dsn_raster_mesh_attr - world-space vertex normals (shaded smooth
    with smooth=True) and vertex colours interpolated over every triangle; the colours take the grey base's place under the spotlight
    (lit) or are painted as they are (lit=False).  The dict then also holds "normal" [H, W, 3] float32 (the unit world normal of every
    pixel) and, with colours, "attr" [H, W, 3] float32 (the interpolated colour, not clamped), both 0 where empty.  Without any of
    the four the call is dsn_raster_mesh_ex's, bit for bit."""
    import numpy as np
    require_gpu()
    width = height if width is None else width
    H, W = int(height), int(width)
    assert verts.is_cuda and faces.is_cuda, "verts and faces: device tensors"
    dev = verts.device
    verts = verts.reshape(-1, 3).to(torch.float32).contiguous()
    faces = faces.reshape(-1, 3).to(torch.int32).contiguous()
    V, T = verts.shape[0], faces.shape[0]
    nbytes = lib().dsn_raster_workspace_bytes(V, T, H, W)
    if nbytes == 0:
        raise RuntimeError("dsn_raster_mesh: height and width must be 1 ... 16384 and the mesh below 2^31 vertices and faces")
    pose, fx0, fy0 = raster_camera(camera_pose, yfov, H, W)
    fx, fy = (fx0 if fx is None else float(fx)), (fy0 if fy is None else float(fy))
    light = np.array([intensity, math.cos(inner), math.cos(outer), base], dtype=np.float32)
    attr = vertex_normals is not None or vertex_colors is not None or smooth or not lit
    if smooth and vertex_normals is None:
        raise ValueError("raster_mesh: smooth=True needs vertex_normals")

    def per_vertex(a, what):
        if a is None:
            return None
        a = a.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        if a.shape[0] != V:
            raise ValueError(f"raster_mesh: {what} has {a.shape[0]} rows for {V} vertices")
        return a
    vn, vc = per_vertex(vertex_normals, "vertex_normals"), per_vertex(vertex_colors, "vertex_colors")
    if out is None:
        out = {"color": torch.empty(H, W, 3, dtype=torch.uint8, device=dev), "depth": torch.empty(H, W, dtype=torch.float32, device=dev),
               "face": torch.empty(H, W, dtype=torch.int32, device=dev), "_ws": _scratch(nbytes, dev)}
    if attr and "normal" not in out:
        out["normal"] = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    if vc is not None and "attr" not in out:
        out["attr"] = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    ws = out["_ws"]
    assert ws.numel() >= nbytes and out["face"].shape == (H, W)
    head = (_ptr(verts) if V else None, V, _ptr(faces) if T else None, T, pose.ctypes.data, fx, fy, float(znear), light.ctypes.data, H, W,
            _ptr(out["face"]), _ptr(out["depth"]), _ptr(out["color"]), _ptr(ws), nbytes, int(phases), int(big_pixels))
    if attr:
        mode = (RM_SMOOTH if smooth else 0) | (0 if lit else RM_UNLIT)
        _check(lib().dsn_raster_mesh_attr(*head, _ptr(vn) if V else None, _ptr(vc) if V else None, mode, _ptr(out["normal"]),
                                          _ptr(out["attr"]) if vc is not None else None, _stream()), "dsn_raster_mesh_attr")
    else:
        _check(lib().dsn_raster_mesh_ex(*head, _stream()), "dsn_raster_mesh")
    if phases or big_pixels:
        return out
    return {k: out[k] for k in ("color", "depth", "face", "normal", "attr") if k in out and (attr or k in ("color", "depth", "face"))}


def lbs_warp(scene: Scene, pts, smpl_weights, joint_transforms, bw_type="rigid_center", exhaustive=False):
    """dormant alternate (utils/render_utils.py:352-403 + utils/blend_utils.py:72-81): nearest-face blend weights and inverse
    LBS.  Returns dict(face_idx, weights [N,24], transparent, pts_zero [N,3])."""
    if bw_type not in ("rigid_center", "rigid_interp"):
        raise ValueError("unsupport value: bw_type")
    dev = scene.device
    pts = _f32(pts.reshape(-1, 3), dev)
    N = pts.shape[0]
    W = _f32(smpl_weights.reshape(-1, 24), dev)
    assert W.shape[0] == scene.V
    A = _f32(joint_transforms.reshape(24, 16), dev)
    out = {"face_idx": torch.empty(N, dtype=torch.int32, device=dev), "weights": torch.empty(N, 24, dtype=torch.float32, device=dev),
           "transparent": torch.empty(N, dtype=torch.uint8, device=dev), "pts_zero": torch.empty(N, 3, dtype=torch.float32, device=dev)}
    _check(lib().dsn_lbs_warp(_ptr(scene.buf), scene.V, scene.F, _ptr(pts), C.c_int64(N), _ptr(W), _ptr(A),
                              0 if bw_type == "rigid_center" else 1, _ptr(out["face_idx"]), _ptr(out["weights"]),
                              _ptr(out["transparent"]), _ptr(out["pts_zero"]), NN_EXHAUSTIVE if exhaustive else 0, _stream()),
           "dsn_lbs_warp")
    return out


def screen_debug(scene: Scene, packed: PackedParams, x_c):
    """plain-fp16 density and the magnitude of its terms for every point (dsn_debug_screen)."""
    x_c = x_c.reshape(-1, 3)
    N = x_c.shape[0]
    dev = scene.device
    sg = torch.zeros(N, dtype=torch.float32, device=dev)
    s1 = torch.zeros(N, dtype=torch.float32, device=dev)
    lst = torch.zeros(N, dtype=torch.int32, device=dev)
    cnt = torch.zeros(64, dtype=torch.int32, device=dev)
    _check(lib().dsn_debug_screen(_ptr(scene.buf), scene.V, scene.F, _ptr(packed.buf), _ptr(x_c, torch.float32), C.c_int64(N),
                                  _ptr(sg), _ptr(s1), _ptr(lst), _ptr(cnt), _stream()), "dsn_debug_screen")
    return sg, s1


def shade(scene: Scene, packed: PackedParams, x_c, grad, x_w, ray_d, essence, S, active=None, exhaustive=False, fp32=False,
          want_factor=False):
    """want_factor: the light factor ELU(lighting MLP) + 1 of every listed sample as a fourth value [N] (dsn_shade_factor; the other
    three keep their bits)"""
    x_c = x_c.reshape(-1, 3)
    N = x_c.shape[0]
    dev = scene.device
    idx = torch.zeros(N, dtype=torch.int32, device=dev)
    n_w = torch.zeros(N, 3, dtype=torch.float32, device=dev)
    col = torch.zeros(N, 3, dtype=torch.float32, device=dev)
    lst, cnt = (None, None) if active is None else active
    if want_factor:
        if fp32:
            raise ValueError("shade: want_factor needs the split-fp16 lighting kernel (fp32=False)")
        fac = torch.zeros(N, dtype=torch.float32, device=dev)
        _check(lib().dsn_shade_factor(_ptr(scene.buf), scene.V, scene.F, _ptr(packed.buf), _ptr(x_c, torch.float32),
                                      _ptr(grad.reshape(-1, 3), torch.float32), _ptr(x_w.reshape(-1, 3), torch.float32),
                                      _ptr(ray_d, torch.float32), _ptr(essence.reshape(-1, 3), torch.float32), C.c_int64(N), S,
                                      _ptr(lst), _ptr(cnt), _ptr(idx), _ptr(n_w), _ptr(col), _ptr(fac), NN_EXHAUSTIVE if exhaustive else 0,
                                      _stream()), "dsn_shade_factor")
        return idx, n_w, col, fac
    _check(lib().dsn_shade(_ptr(scene.buf), scene.V, scene.F, _ptr(packed.buf), _ptr(x_c, torch.float32),
                           _ptr(grad.reshape(-1, 3), torch.float32), _ptr(x_w.reshape(-1, 3), torch.float32),
                           _ptr(ray_d, torch.float32), _ptr(essence.reshape(-1, 3), torch.float32), C.c_int64(N), S,
                           _ptr(lst), _ptr(cnt), _ptr(idx), _ptr(n_w), _ptr(col), (NN_EXHAUSTIVE if exhaustive else 0) | (FIELD_FP32 if fp32 else 0),
                           _stream()), "dsn_shade")
    return idx, n_w, col


def composite(colour, sigma, transparent, z_vals, ray_d, noise=None):
    R, S = z_vals.shape
    dev = z_vals.device
    rgb = torch.empty(R, 3, dtype=torch.float32, device=dev)
    disp = torch.empty(R, dtype=torch.float32, device=dev)
    acc = torch.empty(R, dtype=torch.float32, device=dev)
    w = torch.empty(R, S, dtype=torch.float32, device=dev)
    dep = torch.empty(R, dtype=torch.float32, device=dev)
    _check(lib().dsn_composite(_ptr(colour.reshape(-1, 3), torch.float32), _ptr(sigma.reshape(-1), torch.float32),
                               _ptr(transparent), _ptr(z_vals, torch.float32), _ptr(ray_d, torch.float32), _ptr(noise),
                               R, S, _ptr(rgb), _ptr(disp), _ptr(acc), _ptr(w), _ptr(dep), _stream()), "dsn_composite")
    return rgb, disp, acc, w, dep


def composite_maps(essence, n_w, factor, sigma, transparent, z_vals, ray_d):
    """Stage entry of the decomposition maps (dsn_composite_maps): dense per-sample essence [N,3], world normals [N,3] and light factor
    [N] composited with the weights of (sigma, transparent, z_vals, ray_d).  Returns albedo [R,3], normal [R,3], shading [R], weights
    [R,S], max2 [2] (largest |essence|, largest factor weighed).  Any S."""
    R, S = z_vals.shape
    dev = z_vals.device
    alb = torch.empty(R, 3, dtype=torch.float32, device=dev)
    nrm = torch.empty(R, 3, dtype=torch.float32, device=dev)
    shd = torch.empty(R, dtype=torch.float32, device=dev)
    w = torch.empty(R, S, dtype=torch.float32, device=dev)
    mx = torch.empty(2, dtype=torch.float32, device=dev)
    _check(lib().dsn_composite_maps(_ptr(essence.reshape(-1, 3), torch.float32), _ptr(n_w.reshape(-1, 3), torch.float32),
                                    _ptr(factor.reshape(-1), torch.float32), _ptr(sigma.reshape(-1), torch.float32), _ptr(transparent),
                                    _ptr(z_vals, torch.float32), _ptr(ray_d, torch.float32), R, S, _ptr(alb), _ptr(nrm), _ptr(shd),
                                    _ptr(w), _ptr(mx), _stream()), "dsn_composite_maps")
    return alb, nrm, shd, w, mx


RECORD_FRACTION_DEFAULT = 0.125      # = DSN_RECORD_FRACTION_DEFAULT (csrc/dsn_api.hip)


class RenderWorkspace:
    """The caller-owned scratch of the fused path, grown on demand.  Its relu-record capacity is ITS OWN (ABI 6: the library reads the
    capacity from the size it is handed; rounds 3-4 kept one process-wide fraction that every workspace re-read at every call).
    `fraction` = share of a big frame's samples the records are sized for; fit_records() asks for more after a frame was seen to
    need it.  A larger request is applied at the START of the next frame only (begin_frame(), called by render_rays in front of a
    frame's geometry phase), never between the phase calls of one frame: the buffer a frame's geometry phase filled is the buffer
    its field and shading phases read."""

    def __init__(self, device, fraction: float = RECORD_FRACTION_DEFAULT):
        self.device = torch.device(device)
        self.buf = None
        self.cap = 0
        self.fraction = float(fraction)      # in force for the buffer
        self.want_fraction = float(fraction)      # asked for: applied by begin_frame()
        self._sized = None
        self.light_scratch = None                 # compact colours of render_rays_lights (grown on demand)

    def fit_records(self, positive_fraction: float, headroom: float = 1.25) -> float:
        """a frame put this share of its samples on the sigma > 0 list: make the record capacity cover `headroom` x that from the next
        frame on (samples beyond the capacity have their forward pass evaluated twice; Renderer / bench.py call this with their probe
        frame's count - with more headroom when the share is an ESTIMATE for sliced frames from a one-pass probe).  Never shrinks."""
        want = min(1.0, float(headroom) * float(positive_fraction))
        if want > self.want_fraction:
            self.want_fraction = want
        return self.want_fraction

    def begin_frame(self):
        self.fraction = max(self.fraction, self.want_fraction)

    def bytes_for(self, R, S):
        return lib().dsn_render_workspace_bytes_for(int(R), int(S), C.c_float(self.fraction))

    def record_capacity(self, R, S):
        """records the buffer holds for an R x S frame (what dsn_render_rays_ex will use)"""
        return int(lib().dsn_render_workspace_record_capacity(int(R), int(S), C.c_size_t(self.cap)))

    def get(self, R, S):
        need = self.bytes_for(R, S)
        if self.buf is None or self.cap < need:
            self.buf = _scratch(need, self.device)
            self.cap = need
        return self.buf


def _frame_outputs(R, S, dev, want_weights, K=None):
    """The output dict of render_rays (K given: render_rays_lights', "color" of shape [K, R, 3])."""
    out = {
        "color": torch.empty(*(() if K is None else (K,)), R, 3, dtype=torch.float32, device=dev),
        "disp_map": torch.empty(R, dtype=torch.float32, device=dev),
        "acc_map": torch.empty(R, dtype=torch.float32, device=dev),
        "depth_map": torch.empty(R, dtype=torch.float32, device=dev),
        "z_vals": torch.empty(R, S, dtype=torch.float32, device=dev),
    }
    if want_weights:
        out["weights"] = torch.empty(R, S, dtype=torch.float32, device=dev)
    return out


def _frame_flags(scene: Scene, skip_transparent=True, noise=None, exhaustive=False, fp32=False, uniform=False, screen=False,
                 audit=False, early_stop=False, stop_stats=False, phases=0, share_cus=False):
    """The DSN_* flag word of a frame (render_rays, render_rays_lights)."""
    flags = SKIP_TRANSPARENT if (skip_transparent and noise is None) else 0
    if exhaustive:
        flags |= NN_EXHAUSTIVE
    if fp32:
        flags |= FIELD_FP32
    if uniform:
        flags |= SAMPLE_UNIFORM
    if screen:
        flags |= DENSITY_SCREEN
        if audit:
            flags |= SCREEN_AUDIT
    if early_stop and (flags & SKIP_TRANSPARENT) and not fp32:
        flags |= EARLY_STOP
    if stop_stats:
        flags |= STOP_STATS
    flags |= int(phases) & (PHASE_GEOMETRY | PHASE_FIELD | PHASE_SHADE)
    if share_cus:
        flags |= SHARE_CUS
    if scene.lazy:               # (the training forward takes the flag too since round 6: dsn_render_rays_train's fused geometry)
        flags |= LAZY_LISTS
    return flags


def _slice_schedule(stop_schedule, flags):
    """stop_schedule (early stop only): slice lengths chosen from a probe frame's statistics (choose_stop_schedule) as the library's
    int32 array and its length; (None, 0) = uniform slices."""
    if stop_schedule is None or not (flags & EARLY_STOP):
        return None, 0
    return (C.c_int32 * len(stop_schedule))(*[int(x) for x in stop_schedule]), len(stop_schedule)


def render_rays(scene: Scene, packed: PackedParams, ws: RenderWorkspace, ray_o, ray_d, near, far, S, t_vals,
                jitter=None, noise=None, skip_transparent=True, want_weights=True, out=None, exhaustive=False,
                fp32=False, uniform=False, screen=False, train_cache=None, audit=False, early_stop=False, stop_stats=False, phases=0,
                share_cus=False, stop_schedule=None):
    """Whole hot path on R rays (can_render.py:137-168).  Returns dict of device tensors.
    phases: 0 = the whole frame; PHASE_GEOMETRY | PHASE_FIELD | PHASE_SHADE = only those parts, on the current stream (the caller
    orders the three calls of a frame with its own events and passes the same `out` / workspace to all of them: PhasePipeline).
    screen: DSN_DENSITY_SCREEN (opt-in: the plain-fp16 density screen in front of the accurate pass, margin as calibrated).
    early_stop: DSN_EARLY_STOP (eval mode: front-to-back slices, rays end once their transmittance is below eps(S, colour scale)).
    stop_stats: DSN_STOP_STATS (count what early stop would leave out; read ws word CNT_STOP + 2)."""
    R = ray_o.shape[0]
    if out is None:
        out = _frame_outputs(R, S, scene.device, want_weights)
    flags = _frame_flags(scene, skip_transparent, noise, exhaustive, fp32, uniform, screen, audit, early_stop, stop_stats, phases,
                         share_cus)
    if not phases or (int(phases) & PHASE_GEOMETRY):
        ws.begin_frame()          # (a larger record capacity asked for since the last frame: the buffer may be replaced HERE, only here)
    buf = ws.get(R, S)
    if train_cache is not None:      # training forward: dense, and everything its backward needs stays in train_cache
        flags &= ~SKIP_TRANSPARENT
        gbuf = train_cache.get(R, S)
        # (ABI 8: the far canonical search beside the field kernel on the backward's auxiliary stream)
        ax = train_cache.aux()
        _check(lib().dsn_render_rays_train_ex(_ptr(scene.buf), scene.V, scene.F, _ptr(packed.buf), _ptr(ray_o, torch.float32),
                                              _ptr(ray_d, torch.float32), _ptr(near, torch.float32), _ptr(far, torch.float32), R, S,
                                              _ptr(t_vals, torch.float32), _ptr(jitter), _ptr(noise), flags, _ptr(out["color"]),
                                              _ptr(out["disp_map"]), _ptr(out["acc_map"]), _ptr(out["depth_map"]),
                                              _ptr(out.get("weights")), _ptr(out["z_vals"]), _ptr(buf), _ptr(gbuf), _stream(),
                                              ax[0], ax[1], ax[2]),
               "dsn_render_rays_train")
        return out
    sched, n_sched = _slice_schedule(stop_schedule, flags)
    _check(lib().dsn_render_rays_ex(_ptr(scene.buf), scene.V, scene.F, _ptr(packed.buf), _ptr(ray_o, torch.float32),
                                    _ptr(ray_d, torch.float32), _ptr(near, torch.float32), _ptr(far, torch.float32), R, S,
                                    _ptr(t_vals, torch.float32), _ptr(jitter), _ptr(noise), flags, _ptr(out["color"]),
                                    _ptr(out["disp_map"]), _ptr(out["acc_map"]), _ptr(out["depth_map"]),
                                    _ptr(out.get("weights")), _ptr(out["z_vals"]), _ptr(buf), C.c_size_t(ws.cap), sched, n_sched, _stream()),
           "dsn_render_rays")
    return out


LIGHT_RECORD_FLOATS = 12            # = DSN_LIGHT_RECORD_FLOATS (include/dsnerf.h)
LIGHT_SCRATCH_BUDGET = 256 << 20    # render_rays_lights: bytes of compact colours a sweep keeps at most (lights are grouped to fit)


def light_records(lights, th_mean, device):
    """The light settings of a relighting sweep as the [K, 12] float32 records of dsn_render_rays_lights.  Each light is a dict with
    the optional keys `light_center` (world point, 3), `rot` (2 x 2) and `rot_center` (2): what DualSpaceNeRF.set_light_center /
    set_rot / set_rot_center would hold.  light_shift = light_center - th_mean, computed as DualSpaceNeRF.frame_args does (th_mean: the
    mean of the batch's Th, or Th itself: it is averaged here the same way); the rotation applies only with both `rot` and `rot_center` - one without the other is a ValueError
    (frame_args would silently ignore it)."""
    rows = []
    for i, lt in enumerate(lights):
        unknown = set(lt) - {"light_center", "rot", "rot_center"}
        if unknown:
            raise ValueError(f"light {i}: unknown keys {sorted(unknown)} (light_center, rot, rot_center)")
        rec_t = torch.zeros(LIGHT_RECORD_FLOATS, dtype=torch.float32)
        lc = lt.get("light_center")
        if lc is not None:
            lc = torch.as_tensor(lc)
            th = torch.as_tensor(th_mean).to(lc).reshape(-1, 3).mean(dim=0)
            rec_t[0] = 1.0
            rec_t[1:4] = (lc.reshape(-1)[:3] - th).to(torch.float32).cpu()
        rot, rc = lt.get("rot"), lt.get("rot_center")
        if (rot is None) != (rc is None):
            raise ValueError(f"light {i}: a rotation needs both `rot` and `rot_center`")
        if rot is not None:
            rec_t[4] = 1.0
            rec_t[5:9] = torch.as_tensor(rot).reshape(-1)[:4].to(torch.float32).cpu()
            rec_t[9:11] = torch.as_tensor(rc).reshape(-1)[:2].to(torch.float32).cpu()
        rows.append(rec_t)
    if not rows:
        raise ValueError("a relighting sweep needs at least one light")
    return torch.stack(rows).to(device)


def render_rays_lights(scene: Scene, packed: PackedParams, ws: RenderWorkspace, ray_o, ray_d, near, far, S, t_vals, lights,
                       skip_transparent=True, screen=False, audit=False, early_stop=False, stop_stats=False, stop_schedule=None,
                       uniform=False, want_weights=True, scratch_budget=None, fp32=False, scratch_bytes=None):
    """Relighting sweep (dsn_render_rays_lights): the eval-mode frame of render_rays(skip_transparent=True) under K light settings
    with one geometry / field / normal pass.  `lights`: [K, 12] device records (light_records).  Returns render_rays' dict with
    "color" of shape [K, R, 3]; disp / acc / depth / weights / z_vals do not depend on the light.  Synchronises once (the shading
    list's length sizes the groups of lights).  scratch_budget: bytes of compact colours at most (default LIGHT_SCRATCH_BUDGET; never
    less than one light's colours on a frame whose every sample is shaded).  scratch_bytes (tests): exactly this much scratch - the
    library fails when it does not hold one light's colours."""
    R = ray_o.shape[0]
    K = int(lights.shape[0])
    dev = scene.device
    lights = lights.to(device=dev, dtype=torch.float32).contiguous()
    assert lights.dim() == 2 and lights.shape[1] == LIGHT_RECORD_FLOATS, "lights: [K, 12] records (light_records)"
    if not skip_transparent:
        raise ValueError("render_rays_lights: eval mode with the transparent skip only")
    if fp32:
        raise ValueError("render_rays_lights: the exact-fp32 field is not supported (the sweep's lighting is the split-fp16 kernel's)")
    out = _frame_outputs(R, S, dev, want_weights, K)
    flags = _frame_flags(scene, uniform=uniform, screen=screen, audit=audit, early_stop=early_stop, stop_stats=stop_stats)
    ws.begin_frame()
    buf = ws.get(R, S)
    # compact colours: every light in one group when that fits the budget, else as many as fit - and always at least one light of the
    # largest possible shading list (every sample)
    budget = LIGHT_SCRATCH_BUDGET if scratch_budget is None else int(scratch_budget)
    L = lib()
    need = max(min(budget, L.dsn_render_lights_scratch_bytes(R, S, K, R * S)), L.dsn_render_lights_scratch_bytes(R, S, 1, R * S))
    if scratch_bytes is not None:
        need = int(scratch_bytes)
    ls = ws.light_scratch
    if ls is None or ls.numel() < need:
        ls = ws.light_scratch = _scratch(need, dev)
    sched, n_sched = _slice_schedule(stop_schedule, flags)
    _check(L.dsn_render_rays_lights(_ptr(scene.buf), scene.V, scene.F, _ptr(packed.buf), _ptr(ray_o, torch.float32),
                                    _ptr(ray_d, torch.float32), _ptr(near, torch.float32), _ptr(far, torch.float32), R, S,
                                    _ptr(t_vals, torch.float32), None, None, flags, _ptr(lights), K, _ptr(out["color"]),
                                    _ptr(out["disp_map"]), _ptr(out["acc_map"]), _ptr(out["depth_map"]), _ptr(out.get("weights")),
                                    _ptr(out["z_vals"]), _ptr(buf), C.c_size_t(ws.cap), _ptr(ls), C.c_size_t(min(ls.numel(), need)),
                                    sched, n_sched, _stream()),
           "dsn_render_rays_lights")
    return out


MAPS = ("albedo", "shading", "normal")


def maps_bound(S: int, eps: float, scale: float) -> float:
    """Early stop: the absolute distance of a sliced frame's map from its one-pass value, for per-sample values q with |q| <= scale on
    the one-pass shading list: (S + 1) (eps + 2^-22) scale (include/dsnerf.h, dsn_render_rays_maps)."""
    return (int(S) + 1) * (float(eps) + 2.0 ** -22) * float(scale)


def render_rays_maps(scene: Scene, packed: PackedParams, ws: RenderWorkspace, ray_o, ray_d, near, far, S, t_vals, lights,
                     maps=MAPS, want_color=True, want_max=True, skip_transparent=True, screen=False, audit=False, early_stop=False, stop_stats=False,
                     stop_schedule=None, uniform=False, want_weights=True, scratch_budget=None, fp32=False, scratch_bytes=None):
    """render_rays_lights that also composites the factors of the colour with the frame's weights (dsn_render_rays_maps): its dict
    plus "albedo" [R,3], "normal" [R,3] (world space, not renormalised), "shading" [K,R] for the names in `maps`, and "maps_max" [2]
    (device: the largest |essence| and the largest light factor that entered a sum; want_max=False: not asked for).
    want_color=False: no "color" (out_rgb = NULL).
    Everything else as render_rays_lights; the scratch holds 4 floats per shaded sample and light."""
    R = ray_o.shape[0]
    K = int(lights.shape[0])
    dev = scene.device
    lights = lights.to(device=dev, dtype=torch.float32).contiguous()
    assert lights.dim() == 2 and lights.shape[1] == LIGHT_RECORD_FLOATS, "lights: [K, 12] records (light_records)"
    maps = tuple(maps)
    unknown = [m for m in maps if m not in MAPS]
    if unknown:
        raise ValueError(f"render_rays_maps: unknown maps {unknown} (albedo, shading, normal)")
    if not skip_transparent:
        raise ValueError("render_rays_maps: eval mode with the transparent skip only")
    if fp32:
        raise ValueError("render_rays_maps: the exact-fp32 field is not supported (the sweep's lighting is the split-fp16 kernel's)")
    out = _frame_outputs(R, S, dev, want_weights, K)
    if not want_color:
        del out["color"]
    if "albedo" in maps:
        out["albedo"] = torch.empty(R, 3, dtype=torch.float32, device=dev)
    if "normal" in maps:
        out["normal"] = torch.empty(R, 3, dtype=torch.float32, device=dev)
    if "shading" in maps:
        out["shading"] = torch.empty(K, R, dtype=torch.float32, device=dev)
    if want_max:
        out["maps_max"] = torch.empty(2, dtype=torch.float32, device=dev)
    flags = _frame_flags(scene, uniform=uniform, screen=screen, audit=audit, early_stop=early_stop, stop_stats=stop_stats)
    ws.begin_frame()
    buf = ws.get(R, S)
    budget = LIGHT_SCRATCH_BUDGET if scratch_budget is None else int(scratch_budget)
    L = lib()
    need = max(min(budget, L.dsn_render_maps_scratch_bytes(R, S, K, R * S)), L.dsn_render_maps_scratch_bytes(R, S, 1, R * S))
    if scratch_bytes is not None:
        need = int(scratch_bytes)
    ls = ws.light_scratch
    if ls is None or ls.numel() < need:
        ls = ws.light_scratch = _scratch(need, dev)
    sched, n_sched = _slice_schedule(stop_schedule, flags)
    _check(L.dsn_render_rays_maps(_ptr(scene.buf), scene.V, scene.F, _ptr(packed.buf), _ptr(ray_o, torch.float32),
                                  _ptr(ray_d, torch.float32), _ptr(near, torch.float32), _ptr(far, torch.float32), R, S,
                                  _ptr(t_vals, torch.float32), None, None, flags, _ptr(lights), K, _ptr(out.get("color")),
                                  _ptr(out["disp_map"]), _ptr(out["acc_map"]), _ptr(out["depth_map"]), _ptr(out.get("weights")),
                                  _ptr(out["z_vals"]), _ptr(out.get("albedo")), _ptr(out.get("normal")), _ptr(out.get("shading")),
                                  _ptr(out.get("maps_max")), _ptr(buf), C.c_size_t(ws.cap), _ptr(ls), C.c_size_t(min(ls.numel(), need)),
                                  sched, n_sched, _stream()),
           "dsn_render_rays_maps")
    return out


class PhasePipeline:
    """Frames in flight BY PHASE (round 3): two HIP streams, one for the matrix-bound field kernels (density screen, field forward /
    reverse: 13 of a 512 x 512 x 64 frame's 17 ms, one persistent workgroup per compute unit) and one for everything else (per-frame
    list build, sampler, nearest-face search, warp of frame k + 1; normals, lighting, compositing of frame k - 1), which is sized to
    fit into the LDS and registers the field workgroups leave on every compute unit and runs BESIDE them.  With one stream per FRAME
    (round 2) the two frames' phases lock into step - both do geometry, then their field kernels take turns - and 2.3 ms of geometry
    per frame run with no field kernel beside them (profiles/r03b_overlap_two_frame_streams.txt).
    MEASURED (profiles/r03c_overlap_phase.txt, r03c_ab_*.json): no gain on the default frame (16.50 vs 16.26-16.45 ms), 2 % on the
    converged set (10.66 vs 10.90).  The GPU is busy 99.7 % of the frame in both schemes; beside a persistent field workgroup the small
    kernels run 5-10x longer (k_light16 0.40 -> 3.4 ms) and slow the field kernels by 8 %: the geometry is work the chip has to do,
    not latency to hide.  Kept as an option (bench.py --overlap phase) and as the test of the phase flags.

    submit(geometry_fn, field_fn, shade_fn): geometry_fn() is enqueued on the side stream at once, field_fn() on the field stream
    behind it, shade_fn() on the side stream behind field_fn - but one submit later, so that the side stream never waits for a
    field phase with the next frame's geometry queued behind the wait.  flush() enqueues the pending shading; join() makes the
    caller's current stream wait for everything.  The functions enqueue on torch's current stream."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.side = torch.cuda.Stream(device=self.device)
        self.field = torch.cuda.Stream(device=self.device)
        self.pending = None

    def submit(self, geometry_fn, field_fn, shade_fn):
        cur = torch.cuda.current_stream(self.device)
        self.side.wait_stream(cur)                      # inputs produced on the caller's stream
        with torch.cuda.stream(self.side):
            geometry_fn()
            e_g = torch.cuda.Event()
            e_g.record()
        with torch.cuda.stream(self.field):
            self.field.wait_event(e_g)
            field_fn()
            e_f = torch.cuda.Event()
            e_f.record()
        prev, self.pending = self.pending, (shade_fn, e_f)
        if prev is not None:
            self._shade(prev)

    def _shade(self, p):
        shade_fn, e_f = p
        with torch.cuda.stream(self.side):
            self.side.wait_event(e_f)
            shade_fn()

    def flush(self):
        if self.pending is not None:
            self._shade(self.pending)
            self.pending = None

    def join(self):
        self.flush()
        torch.cuda.current_stream(self.device).wait_stream(self.side)


def early_stop_eps(S: int, colour_scale: float = 1.0) -> float:
    """the termination / shading threshold of DSN_EARLY_STOP for rays of S samples and colours up to colour_scale:
    min(2^-20, 1e-4 / (2 (S + 1) max(1, colour_scale))) - the frame stays within (S + 1) eps x the largest colour of the one-pass
    frame (include/dsnerf.h), i.e. within 5e-5 absolute while the colours stay below the scale"""
    return float(lib().dsn_early_stop_eps_scaled(int(S), C.c_float(colour_scale)))


def stop_slice_len(R: int, S: int) -> int:
    """samples per uniform slice of DSN_EARLY_STOP for an R x S frame, from the library itself (dsn_stop_slice_len: what
    dsn_render_rays_ex and the DSN_STOP_STATS histogram use, the DSN_STOP_SLICE experiment override included)"""
    return int(lib().dsn_stop_slice_len(int(R), int(S)))


def read_stop_hist(ws, R: int, S: int):
    """(synchronises) the slice histogram a DSN_STOP_STATS frame left: numpy int64 [K + 1, K], hist[g][k] = non-transparent samples of
    uniform slice k on rays whose first slice with T < eps at its start is g (g = K: never)"""
    import numpy as np
    buf = ws if isinstance(ws, torch.Tensor) else ws.buf
    L = int(lib().dsn_stop_stats_slice_len(int(R), int(S)))      # (the histogram's own slice length: half the uniform slice where K <= 32 allows)
    K = (S + L - 1) // L
    c = buf[4 * CNT_HIST:4 * CNT_HIST + 4 * (K + 1) * K].view(torch.int32).cpu().numpy().astype(np.int64)
    return c.reshape(K + 1, K), L


def choose_stop_schedule(hist, L: int, S: int, round_samples: int = 128 * 224, launch_rounds: float = 0.3, quantise: bool = True,
                         round_weight: float = 0.5):
    """Slice lengths for dsn_render_rays_ex from a probe frame's histogram (read_stop_hist).  A slice that starts at uniform slice a
    and covers slices a .. b evaluates sum_k M[a][k], M[a][k] = samples of slice k on rays still alive at the start of a (sum over
    g > a of hist[g][k]).  Its forward launch runs in ROUNDS of the persistent grid - 128 samples per workgroup, round_samples per
    round (224 workgroups with frames in flight, DSN_SHARE_CUS) - so it costs ceil(samples / round_samples) rounds whatever its last
    round holds, plus about `launch_rounds` of a round for the small launches in front of it (transmittance, list filter).  Dynamic
    programming over the slice borders minimises the sum; slices stay within 64 samples.  round_weight (round 6's last session): the
    price of a slice is round_weight x its whole rounds + (1 - round_weight) x its plain sample count - the workgroups of the
    persistent grid fetch their tiles dynamically and the neighbours' kernels use what a last round leaves idle, so a started round
    does not cost a whole one: with 1.0 (rounds 5-6) a rank's eighth of the bench frame was cut into 2-4 slices and evaluated 20 % more
    samples than it had to; 0.5 measured best on the emulated partition (8 ranks 6.3 -> 6.5 x, the whole frame unchanged).
    quantise=False: round 4's model (samples +
    0.9 rounds per slice), which ignored the half-empty last round - 4 % on a whole 512 x 512 frame (12 rounds per slice), a third of
    the forward time of a rank's eighth of it (1.5 rounds per slice).
    Returns (list of lengths in samples, evaluated samples it predicts, evaluated samples of the uniform schedule)."""
    import numpy as np
    hist = np.asarray(hist, np.int64)
    K = hist.shape[1]
    M = np.zeros((K, K), np.int64)                       # M[a][k]: alive at the start of slice a
    for a in range(K):
        M[a] = hist[a + 1:].sum(0)
    rs = float(round_samples)
    alpha = float(round_weight)
    launch_rounds = float(launch_rounds)

    def cost(n):
        if not quantise:
            return 0.9 * 32768.0 + float(n)
        return (float(launch_rounds) + alpha * float(-(-int(n) // int(round_samples))) + (1.0 - alpha) * float(n) / rs) * rs

    best = [0.0] + [float("inf")] * K
    prev = [0] * (K + 1)
    for b in range(1, K + 1):
        for a in range(max(0, b - 64 // max(L, 1)), b):
            if (min(b * L, S) - a * L) > 64:
                continue
            c = best[a] + cost(M[a][a:b].sum())
            if c < best[b] or (c == best[b] and a > prev[b]):      # (ties: the later border - termination checked more often)
                best[b], prev[b] = c, a
    cuts, b = [], K
    while b > 0:
        cuts.append((prev[b], b))
        b = prev[b]
    cuts.reverse()
    lens = [min(b * L, S) - a * L for a, b in cuts]
    evaluated = int(sum(M[a][a:b].sum() for a, b in cuts))
    uniform = int(sum(M[k][k] for k in range(K)))
    return lens, evaluated, uniform


def read_stop_stats(ws):
    """(synchronises) dict(active, would_skip, skipped, unshaded, colour_max) of the last dsn_render_rays on this workspace (or of a
    copy of its first 256 bytes): non-transparent samples; what DSN_STOP_STATS counted (samples early stop would leave out); what
    DSN_EARLY_STOP left out / did not shade; the largest |colour| the frame's compositor weighed."""
    buf = ws if isinstance(ws, torch.Tensor) else ws.buf
    c = buf[:256].view(torch.int32).cpu()
    return {"active": int(c[CNT_ACTIVE]), "would_skip": int(c[CNT_STOP + 2]), "skipped": int(c[CNT_STOP]), "unshaded": int(c[CNT_STOP + 1]),
            "colour_max": float(c[CNT_COLOUR_MAX:CNT_COLOUR_MAX + 1].view(torch.float32)[0])}


class GradWorkspace:
    """Scratch of the training backward (grown on demand; 22 KB per sample)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.buf = None
        self._aux = None           # (aux stream, fork event, join event) of dsn_render_rays_grad_ex, made on first use

    def aux(self):
        """the second stream + two events the backward's independent chains use (DSN_TRAIN_AUX=0: none - one stream, as rounds 1-5)"""
        if os.environ.get("DSN_TRAIN_AUX", "1") == "0":
            return (None, None, None)
        if self._aux is None:
            h = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
            with torch.cuda.device(self.device):
                _check(lib().dsn_aux_create(C.byref(h[0]), C.byref(h[1]), C.byref(h[2])), "dsn_aux_create")
            self._aux = tuple(C.c_void_p(x.value) for x in h)
        return self._aux

    def __del__(self):
        a, self._aux = getattr(self, "_aux", None), None
        if a is not None:
            try:
                lib().dsn_aux_destroy(*a)
            except Exception:
                pass

    def get(self, R, S):
        need = lib().dsn_grad_workspace_bytes(int(R), int(S))
        if self.buf is None or self.buf.numel() < need:
            self.buf = None
            self.buf = _scratch(need, self.device)
        return self.buf


GRAD_CNT_RANGE = 303          # float word of the training workspace's last 4 KB (dsn_train.hip: w.small) that dsn_render_rays_grad uses as
                              # an int32 counter of samples whose tangent / adjoint pass left the fp16 range (their second-order /
                              # adjoint contributions are dropped from that step's weight gradients)


def grad_range_word(ws: "GradWorkspace", R, S):
    """1-element int32 device view of that counter for a backward over R x S samples (no synchronisation)"""
    need = lib().dsn_grad_workspace_bytes(int(R), int(S))
    off = need - 4096 + 4 * GRAD_CNT_RANGE
    return ws.buf[off:off + 4].view(torch.int32)


# the per-row arrays of the training workspace in the order of dsn_grad_workspace_layout (include/dsnerf.h: DSN_GRAD_WS_*):
# (name, dtype, columns; 0 columns = [N])
GRAD_WS_ARRAYS = [
    ("transparent", torch.uint8, 0), ("x_c", torch.float32, 3), ("sig", torch.float32, 0), ("ess", torch.float32, 3),
    ("g", torch.float32, 3), ("n_w", torch.float32, 3), ("xl", torch.float32, 9), ("hl1", torch.float32, 128),
    ("hl2", torch.float32, 128), ("pre", torch.float32, 0), ("wl", torch.float32, 0), ("col", torch.float32, 3),
    ("rr", torch.float32, 128), ("h6", torch.float32, 256),
    ("d_sig", torch.float32, 0), ("d_col", torch.float32, 3), ("d_ess", torch.float32, 3), ("d_pre", torch.float32, 0),
    ("d_hl2", torch.float32, 128), ("d_hl1", torch.float32, 128), ("d_xl", torch.float32, 9), ("d_rr", torch.float32, 128),
    ("u", torch.float32, 3), ("list1", torch.int32, 0), ("list2", torch.int32, 0), ("rowcnt", torch.int32, 0),
]


def grad_workspace_layout(R, S):
    """{array name: byte offset} of the training workspace of R x S samples, from the library's own carve (dsn_grad_workspace_layout)"""
    off = (C.c_int64 * len(GRAD_WS_ARRAYS))()
    _check(lib().dsn_grad_workspace_layout(int(R), int(S), off, len(GRAD_WS_ARRAYS)), "dsn_grad_workspace_layout")
    return {name: int(o) for (name, _, _), o in zip(GRAD_WS_ARRAYS, off)}


def grad_rows(ws: "GradWorkspace", R, S):
    """(synchronises) clones of the per-row arrays the last dsn_render_rays_grad over R x S samples left in this workspace, as a dict
    of device tensors: [N] or [N,k] by sample, `list1` / `list2` cut to their entries, `rowcnt` = the two counts.  Rows that are not on
    the lists hold stale values.  For tests and diagnostics: nothing in the product reads it."""
    N = int(R) * int(S)
    off = grad_workspace_layout(R, S)
    torch.cuda.synchronize(ws.buf.device)
    out = {}
    for name, dt, cols in GRAD_WS_ARRAYS:
        rows = 2 if name == "rowcnt" else N
        nbytes = rows * max(cols, 1) * torch.empty(0, dtype=dt).element_size()
        t = ws.buf[off[name]:off[name] + nbytes].view(dt)
        out[name] = (t.reshape(rows, cols) if cols else t).clone()
    n1, n2 = (int(v) for v in out["rowcnt"].cpu())
    out["list1"], out["list2"] = out["list1"][:n1], out["list2"][:n2]
    torch.cuda.synchronize(ws.buf.device)
    return out


def grad_row_counts(ws: "GradWorkspace", R, S):
    """(synchronises) (rows the last training forward evaluated, rows its backward propagated) of R x S samples: the forward skips
    transparent samples whose noise is <= 0 (alpha = 0 exactly), the backward every row whose cotangents are all zero (dsn_train.hip,
    Rows) - two int32 words of the workspace (dsn_grad_workspace_layout: rowcnt)"""
    off = grad_workspace_layout(R, S)["rowcnt"]
    c = ws.buf[off:off + 8].view(torch.int32).cpu()
    return int(c[0]), int(c[1])


def grad_range_overflow(ws: "GradWorkspace", R, S) -> int:
    """(synchronises) the counter's value after the last dsn_render_rays_grad on this workspace"""
    return int(grad_range_word(ws, R, S).item())


def render_rays_grad(scene: Scene, params, poses, frame_idx, zero_code, ray_o, ray_d, z_vals, noise, d_rgb, d_disp=None,
                     d_acc=None, d_depth=None, d_weights=None, ws: GradWorkspace = None, packed: PackedParams = None,
                     cached: bool = False):
    """Parameter gradients of render_rays' outputs (dsn_render_rays_grad; trainer.py:70-81 loss.backward()).
    params: the 33 tensors in PARAM_ORDER (name -> tensor dict or list).  Returns a list of 33 gradient tensors
    (float32, on the device, shaped like the parameters).  The scene's frame must be set with the same parameters."""
    dev = scene.device
    if isinstance(params, dict):
        params = [params[k] for k in PARAM_ORDER]
    prm = [_f32(p.detach(), dev) for p in params]
    if packed is None:       # MFMA image of the same parameters (the fused forward / reverse kernel streams it)
        packed = PackedParams(dev).update(dict(zip(PARAM_ORDER, prm)))
    grads = [torch.empty_like(p) for p in prm]
    pp = (C.c_void_p * 33)(*[p.data_ptr() for p in prm])
    gp = (C.c_void_p * 33)(*[g.data_ptr() for g in grads])
    R, S = z_vals.shape
    ws = ws or GradWorkspace(dev)
    buf = ws.get(R, S)
    poses = _f32(poses.reshape(24, 3), dev)
    f = lambda a: None if a is None else _f32(a, dev)
    args = [f(ray_o), f(ray_d), f(z_vals), f(noise), f(d_rgb), f(d_disp), f(d_acc), f(d_depth), f(d_weights)]
    ax = ws.aux()
    _check(lib().dsn_render_rays_grad_ex(_ptr(scene.buf), scene.V, scene.F, _ptr(packed.buf), pp, _ptr(poses), int(frame_idx), int(bool(zero_code)),
                                         _ptr(args[0]), _ptr(args[1]), _ptr(args[2]), _ptr(args[3]), int(R), int(S),
                                         _ptr(args[4]), _ptr(args[5]), _ptr(args[6]), _ptr(args[7]), _ptr(args[8]), gp,
                                         _ptr(buf), 1 if cached else 0, _stream(), ax[0], ax[1], ax[2]), "dsn_render_rays_grad")
    scene._keep_grad = (prm, args, poses, packed)
    return grads


def module_grad(scene: Scene, params, poses, frame_idx, zero_code, x_world, x_canon, view_dir, d_colour, d_sigma,
                ws: GradWorkspace = None, packed: PackedParams = None):
    """Parameter gradients of DualSpaceNeRF.forward's (colour, density) on explicit points (dsn_module_grad).  Returns the
    33 gradients in PARAM_ORDER (float32, device)."""
    dev = scene.device
    if isinstance(params, dict):
        params = [params[k] for k in PARAM_ORDER]
    prm = [_f32(p.detach(), dev) for p in params]
    if packed is None:
        packed = PackedParams(dev).update(dict(zip(PARAM_ORDER, prm)))
    grads = [torch.empty_like(p) for p in prm]
    pp = (C.c_void_p * 33)(*[p.data_ptr() for p in prm])
    gp = (C.c_void_p * 33)(*[g.data_ptr() for g in grads])
    xw, xc, vd = (_f32(t.reshape(-1, 3), dev) for t in (x_world, x_canon, view_dir))
    N = xw.shape[0]
    dc = _f32(d_colour.reshape(N, 3), dev)
    ds = _f32(d_sigma.reshape(N), dev)
    zeros = torch.zeros(N, dtype=torch.float32, device=dev)
    ws = ws or GradWorkspace(dev)
    buf = ws.get(N, 1)
    poses = _f32(poses.reshape(24, 3), dev)
    _check(lib().dsn_module_grad(_ptr(scene.buf), scene.V, scene.F, _ptr(packed.buf), pp, _ptr(poses), int(frame_idx),
                                 int(bool(zero_code)), _ptr(xw), _ptr(xc), _ptr(vd), _ptr(zeros), C.c_int64(N), _ptr(dc), _ptr(ds), gp,
                                 _ptr(buf), _stream()), "dsn_module_grad")
    scene._keep_grad = (prm, xw, xc, vd, dc, ds, zeros, poses, packed)
    return grads


def image_scatter(out: dict, mask_at_box, H, W, clamp=False):
    """post_process on the device (utils/render_utils.py:466-472): compacted per-ray outputs -> [H,W,*] images with
    zeros outside mask_at_box.  out: dict with color [R,3], disp_map, acc_map, depth_map [R] (device)."""
    dev = out["color"].device
    mask = mask_at_box.reshape(-1).to(device=dev, dtype=torch.uint8).contiguous()
    R = out["color"].shape[0]
    ws = _scratch(lib().dsn_image_workspace_bytes(H, W), dev)
    img = {k: _output((H, W, c), torch.float32, dev) for k, c in
           (("coarse_color", 3), ("coarse_disp", 1), ("coarse_acc", 1), ("coarse_depth", 1))}
    _check(lib().dsn_image_scatter(_ptr(out["color"], torch.float32), _ptr(out["disp_map"]), _ptr(out["acc_map"]),
                                   _ptr(out["depth_map"]), R, _ptr(mask), H, W, int(bool(clamp)), _ptr(img["coarse_color"]),
                                   _ptr(img["coarse_disp"]), _ptr(img["coarse_acc"]), _ptr(img["coarse_depth"]), _ptr(ws),
                                   _stream()), "dsn_image_scatter")
    return img


def image_scatter_maps(rgbs, scalars, mask_at_box, H, W):
    """image_scatter's kernel (dsn_image_scatter, unchanged) for other per-ray arrays: `rgbs` a list of [R,3], `scalars` a list of [R]
    device tensors -> ([H,W,3] images, [H,W,1] images), zeros outside mask_at_box.  One call carries one [R,3] and up to three [R]
    arrays (the colour / disp / acc / depth slots)."""
    rgbs, scalars = list(rgbs), list(scalars)
    if not rgbs and not scalars:
        return [], []
    dev = (rgbs + scalars)[0].device
    mask = mask_at_box.reshape(-1).to(device=dev, dtype=torch.uint8).contiguous()
    R = (rgbs + scalars)[0].shape[0]
    ws = _scratch(lib().dsn_image_workspace_bytes(H, W), dev)
    rgb_imgs = [_output((H, W, 3), torch.float32, dev) for _ in rgbs]
    sc_imgs = [_output((H, W, 1), torch.float32, dev) for _ in scalars]
    spare_src = spare_img = None
    i = j = 0
    while i < len(rgbs) or j < len(scalars):
        if i < len(rgbs):
            src, img = rgbs[i].contiguous(), rgb_imgs[i]
            i += 1
        else:      # (the kernel wants a colour with every call: a zero one into an image nobody reads)
            if spare_src is None:
                spare_src = torch.zeros(R, 3, dtype=torch.float32, device=dev)
                spare_img = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
            src, img = spare_src, spare_img
        three = [(scalars[k].contiguous(), sc_imgs[k]) for k in range(j, min(j + 3, len(scalars)))]
        j += len(three)
        three += [(None, None)] * (3 - len(three))
        _check(lib().dsn_image_scatter(_ptr(src, torch.float32), _ptr(three[0][0]), _ptr(three[1][0]), _ptr(three[2][0]), R, _ptr(mask),
                                       H, W, 0, _ptr(img), _ptr(three[0][1]), _ptr(three[1][1]), _ptr(three[2][1]), _ptr(ws),
                                       _stream()), "dsn_image_scatter")
    return rgb_imgs, sc_imgs


def image_psnr(img_rgb, gt, mask_at_box=None):
    """metrics.py:8-21 on the device: returns a float64 device tensor {mse_all, mse_masked, psnr_all, psnr_masked}."""
    dev = img_rgb.device
    H, W = img_rgb.shape[:2]
    gt = gt.reshape(H, W, 3).to(dev).contiguous()
    assert gt.dtype in (torch.float64, torch.float32)
    mask = None if mask_at_box is None else mask_at_box.reshape(-1).to(device=dev, dtype=torch.uint8).contiguous()
    ws = _scratch(lib().dsn_image_workspace_bytes(H, W), dev)
    out = _output((4,), torch.float64, dev)
    g64, g32 = (gt, None) if gt.dtype == torch.float64 else (None, gt)
    _check(lib().dsn_image_psnr(_ptr(img_rgb.contiguous(), torch.float32), _ptr(g64), _ptr(g32), _ptr(mask), H, W, _ptr(out),
                                _ptr(ws), _stream()), "dsn_image_psnr")
    return out


def image_ssim(img, gt, mask_at_box, clamp=False):
    """metrics.py:23-38 ssim_metric on the device (dsn_image_ssim): img [H,W,3] or [F,H,W,3] float32, gt of the same shape
    (float64 as the reference's batch["img"], or float32), mask_at_box [H,W] / [F,H,W] (or flattened pixels).  clamp=True
    clamps img to [0,1] first (test.py:62-63).  Returns device tensors (ssim float64 [F], rect int32 [F,4] = {x, y, w, h},
    status int32 [F]); no synchronisation.  A frame whose status is not SSIM_OK has no SSIM (NaN): skimage raises
    ValueError there - ssim_status_error() says why."""
    dev = img.device
    if img.dim() not in (3, 4) or img.shape[-1] != 3:
        raise ValueError(f"image_ssim: img must be [H,W,3] or [F,H,W,3], got {tuple(img.shape)}")
    img = img.reshape(-1, *img.shape[-3:])
    F, H, W, _ = img.shape
    gt = gt.to(dev).reshape(F, H, W, 3).contiguous()
    if gt.dtype not in (torch.float64, torch.float32):
        raise TypeError(f"image_ssim: gt must be float64 or float32, got {gt.dtype}")
    mask = mask_at_box.to(device=dev).reshape(F, H, W)
    mask = (mask != 0).to(torch.uint8).contiguous() if mask.dtype != torch.uint8 else mask.contiguous()
    ws = _scratch(lib().dsn_image_ssim_workspace_bytes(F, H, W), dev)
    ssim = torch.empty(F, dtype=torch.float64, device=dev)
    rect = torch.empty(F, 4, dtype=torch.int32, device=dev)
    status = torch.empty(F, dtype=torch.int32, device=dev)
    g64, g32 = (gt, None) if gt.dtype == torch.float64 else (None, gt)
    _check(lib().dsn_image_ssim(_ptr(img.contiguous(), torch.float32), _ptr(g64), _ptr(g32), _ptr(mask), F, H, W, int(bool(clamp)),
                                _ptr(ssim), _ptr(rect), _ptr(status), _ptr(ws), _stream()), "dsn_image_ssim")
    return ssim, rect, status


def ssim_status_error(status, rect):
    """The ValueError skimage's compare_ssim raises for a crop without a whole 7 x 7 window (host values of one frame)."""
    x, y, w, h = (int(v) for v in rect)
    what = "the mask is empty" if int(status) == SSIM_EMPTY_MASK else f"the mask's bounding rectangle is {w} x {h}"
    return ValueError(f"ssim: win_size exceeds image extent ({what}; SSIM needs at least 7 x 7)")


# ---- LPIPS (include/dsnerf.h "LPIPS"; csrc/dsn_lpips.hip) ----
LPIPS_CONV_SHAPES = {
    "alex": [(64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3)],
    "vgg": [(64, 3, 3, 3), (64, 64, 3, 3), (128, 64, 3, 3), (128, 128, 3, 3), (256, 128, 3, 3), (256, 256, 3, 3), (256, 256, 3, 3),
            (512, 256, 3, 3), (512, 512, 3, 3), (512, 512, 3, 3), (512, 512, 3, 3), (512, 512, 3, 3), (512, 512, 3, 3)],
}
LPIPS_TAP_CHANNELS = {"alex": (64, 192, 384, 256, 256), "vgg": (64, 128, 256, 512, 512)}
LPIPS_MIN_SIDE = {"alex": 31, "vgg": 16}


def lpips_tap_shapes(net, H, W):
    """[(C, h, w)] of the five taps of an H x W image (None below the net's smallest image)"""
    if H < LPIPS_MIN_SIDE[net] or W < LPIPS_MIN_SIDE[net]:
        return None
    if net == "alex":
        s = lambda n: (n + 4 - 11) // 4 + 1      # noqa: E731
        p = lambda n: (n - 3) // 2 + 1           # noqa: E731
        sides = [(s(H), s(W)), (p(s(H)), p(s(W)))] + [(p(p(s(H))), p(p(s(W))))] * 3
    else:
        sides = [(H >> k, W >> k) for k in range(5)]
    return [(c, h, w) for c, (h, w) in zip(LPIPS_TAP_CHANNELS[net], sides)]


def _lpips_net(net):
    if net not in LPIPS_NETS:
        raise ValueError(f"net must be 'alex' or 'vgg', got {net!r}")
    return LPIPS_NETS[net]


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def lpips_check_weights(net, conv, lin):
    """shape check of the canonical weight lists: conv = [(weight [Cout,Cin,k,k], bias [Cout]) ...] in layer order, lin = five [C_l]
    vectors (any shape with C_l elements); raises ValueError naming the tensor"""
    _lpips_net(net)
    shapes = LPIPS_CONV_SHAPES[net]
    if len(conv) != len(shapes) or len(lin) != 5:
        raise ValueError(f"lpips {net}: {len(shapes)} convolutions and 5 lin vectors expected, got {len(conv)} and {len(lin)}")
    for i, ((w, b), sh) in enumerate(zip(conv, shapes)):
        if tuple(w.shape) != sh:
            raise ValueError(f"lpips {net}: convolution {i} weight must be {sh}, got {tuple(w.shape)}")
        if tuple(b.shape) != (sh[0],):
            raise ValueError(f"lpips {net}: convolution {i} bias must be {(sh[0],)}, got {tuple(b.shape)}")
    for l, (w, c) in enumerate(zip(lin, LPIPS_TAP_CHANNELS[net])):
        if int(math.prod(w.shape)) != c:
            raise ValueError(f"lpips {net}: lin {l} must hold {c} weights, got {tuple(w.shape)}")


def lpips_pack(net, conv, lin, device):
    """dsn_lpips_pack: the canonical weight lists (lpips_check_weights) -> the packed device image (uint8 tensor)"""
    require_gpu()
    lpips_check_weights(net, conv, lin)
    dev = torch.device(device)
    cw = [_f32(torch.as_tensor(w), dev) for w, _ in conv]
    cb = [_f32(torch.as_tensor(b), dev) for _, b in conv]
    lw = [_f32(torch.as_tensor(w).reshape(-1), dev) for w in lin]
    packed = _scratch(lib().dsn_lpips_packed_bytes(_lpips_net(net)), dev)
    with torch.cuda.device(dev):
        _check(lib().dsn_lpips_pack(_lpips_net(net), _ptr_array(cw), _ptr_array(cb), _ptr_array(lw), _ptr(packed), _stream()), "dsn_lpips_pack")
        for t in cw + cb + lw:          # the kernels read them on the current stream after this function has dropped them
            t.record_stream(torch.cuda.current_stream())
    return packed


def _lpips_chunk(net, n_frames, H, W, per_frame=1):
    """frames per call so that the workspace stays below LPIPS_WORKSPACE_CAP (at least one)"""
    one = lib().dsn_lpips_workspace_bytes(_lpips_net(net), 1, H, W)
    if one == 0:
        raise ValueError(f"lpips: bad sizes ({n_frames} x {H} x {W})")
    most = max(1, min(n_frames, int(LPIPS_WORKSPACE_CAP // max(one, 1))))
    # (the workspace has a fixed part, so k frames need a little less than k times one frame's: take what really fits)
    while most < n_frames and lib().dsn_lpips_workspace_bytes(_lpips_net(net), most + 1, H, W) <= LPIPS_WORKSPACE_CAP:
        most += 1
    calls = -(-n_frames // most)
    return -(-n_frames // calls)          # even chunks: 16 frames under a cap of 15 go as 8 + 8


def lpips_features(net, packed, stack, rgb_pm1=False):
    """dsn_lpips_features: stack [n,H,W,3] float32 on the device -> (five float32 tensors [n,C,h,w], status int32 [n]); no
    synchronisation.  Below the net's smallest image the taps are empty tensors and every status is LPIPS_TOO_SMALL."""
    if stack.dim() != 4 or stack.shape[-1] != 3 or stack.dtype != torch.float32:
        raise ValueError(f"lpips_features: stack must be float32 [n,H,W,3], got {stack.dtype} {tuple(stack.shape)}")
    dev = stack.device
    stack = stack.contiguous()
    n, H, W, _ = stack.shape
    shapes = lpips_tap_shapes(net, H, W)
    status = _output((n,), torch.int32, dev)
    taps = [_output((n, c, h, w), torch.float32, dev) for c, h, w in shapes] if shapes else [torch.empty(n, c, 0, 0, device=dev)
                                                                                            for c in LPIPS_TAP_CHANNELS[net]]
    step = 2 * _lpips_chunk(net, (n + 1) // 2, H, W)
    nbytes = lib().dsn_lpips_workspace_bytes(_lpips_net(net), step // 2, H, W)
    ws = _scratch(nbytes, dev)
    dummy = [status] * 5
    for i in range(0, n, step):
        m = min(step, n - i)
        outs = [t[i:i + m] for t in taps] if shapes else dummy
        _check(lib().dsn_lpips_features(_ptr(packed), _lpips_net(net), _ptr(stack[i:i + m]), m, H, W, int(bool(rgb_pm1)), _ptr_array(outs),
                                        _ptr(status[i:i + m]), _ptr(ws), nbytes, _stream()), "dsn_lpips_features")
    return taps, status


def lpips(net, packed, img, gt, rgb_pm1=False):
    """dsn_lpips: img [F,H,W,3] (or [H,W,3]) float32 and gt of the same shape (float64 or float32) on the device -> (out float64 [F],
    layers float64 [F,5], status int32 [F]); no synchronisation.  A frame whose status is not LPIPS_OK is NaN."""
    if img.dim() not in (3, 4) or img.shape[-1] != 3 or img.dtype != torch.float32:
        raise ValueError(f"lpips: img must be float32 [H,W,3] or [F,H,W,3], got {img.dtype} {tuple(img.shape)}")
    dev = img.device
    img = img.reshape(-1, *img.shape[-3:]).contiguous()
    F, H, W, _ = img.shape
    gt = gt.to(dev).reshape(F, H, W, 3).contiguous()
    if gt.dtype not in (torch.float64, torch.float32):
        raise TypeError(f"lpips: gt must be float64 or float32, got {gt.dtype}")
    out = _output((F,), torch.float64, dev)
    layers = _output((F, 5), torch.float64, dev)
    status = _output((F,), torch.int32, dev)
    step = _lpips_chunk(net, F, H, W)
    nbytes = lib().dsn_lpips_workspace_bytes(_lpips_net(net), step, H, W)
    ws = _scratch(nbytes, dev)
    for i in range(0, F, step):
        m = min(step, F - i)
        g = gt[i:i + m]
        g64, g32 = (g, None) if g.dtype == torch.float64 else (None, g)
        _check(lib().dsn_lpips(_ptr(packed), _lpips_net(net), _ptr(img[i:i + m]), _ptr(g64), _ptr(g32), m, H, W, int(bool(rgb_pm1)),
                               _ptr(out[i:i + m]), _ptr(layers[i:i + m]), _ptr(status[i:i + m]), _ptr(ws), nbytes, _stream()), "dsn_lpips")
    return out, layers, status


def lpips_status_text(status):
    s = int(status)
    names = [n for bit, n in ((LPIPS_TOO_SMALL, "the image is below the net's smallest size"),
                              (LPIPS_RANGE, "an activation or weight left the split-fp16 range (|v| >= 32768)"),
                              (LPIPS_NONFINITE, "a pixel is NaN or infinite")) if s & bit]
    return "; ".join(names) if names else "ok"


def _loss_args(color, target, acc, occupancy, kind):
    """the device arrays of one loss call: (color [R,3] f32, target f32 | None, target f64 | None, acc [R] f32 | None, occupancy u8 |
    None, occupancy f32 | None, R, kind).  [1,R,3] / [1,R] shapes are reshaped, non-contiguous inputs copied."""
    if kind not in ("L2", "L1", LOSS_L2, LOSS_SMOOTH_L1):
        raise ValueError(f"kind must be 'L2' or 'L1' (Smooth-L1), got {kind!r}")
    kind = {"L2": LOSS_L2, "L1": LOSS_SMOOTH_L1}.get(kind, kind)
    dev = color.device
    if color.dtype != torch.float32 or color.shape[-1:] != (3,):
        raise TypeError(f"color must be float32 [R,3], got {color.dtype} {tuple(color.shape)}")
    color = color.reshape(-1, 3).contiguous()
    R = color.shape[0]
    target = target.to(dev).reshape(-1, 3).contiguous()
    if target.dtype not in (torch.float64, torch.float32):
        raise TypeError(f"target must be float64 or float32, got {target.dtype}")
    if target.shape[0] != R:
        raise ValueError(f"target has {target.shape[0]} rays, color {R}")
    t32, t64 = (target, None) if target.dtype == torch.float32 else (None, target)
    o8 = o32 = None
    if occupancy is not None:
        if acc is None:
            raise ValueError("the mask term (occupancy) needs acc")
        occupancy = occupancy.to(dev).reshape(-1)
        if occupancy.dtype == torch.bool:
            occupancy = occupancy.to(torch.uint8)
        if occupancy.dtype not in (torch.uint8, torch.float32):
            raise TypeError(f"occupancy must be uint8, bool or float32, got {occupancy.dtype}")
        if occupancy.numel() != R:
            raise ValueError(f"occupancy has {occupancy.numel()} rays, color {R}")
        occupancy = occupancy.contiguous()
        o8, o32 = (occupancy, None) if occupancy.dtype == torch.uint8 else (None, occupancy)
    if acc is not None:
        if acc.dtype != torch.float32 or acc.numel() != R:
            raise TypeError(f"acc must be float32 [{R}], got {acc.dtype} {tuple(acc.shape)}")
        acc = acc.reshape(-1)
    return color, t32, t64, acc, o8, o32, R, kind


def train_loss(color, target, acc=None, occupancy=None, kind="L2", overwrite_acc=True, workspace=None):
    """utils/loss.py's MSELoss ("L2") / SmoothL1Loss ("L1") with the LOSSwMask term when `occupancy` is given, and the trainer's
    mse / psnr of the same batch, on the device (dsn_train_loss, the rule of include/dsnerf.h).  color [R,3] float32, target [R,3]
    float32 or float64, acc [R] float32, occupancy [R] uint8 / bool / float32 ([1,R,...] shapes too).  overwrite_acc: acc reads 1
    where occupancy == 1 afterwards (the reference's in-place assignment; a non-contiguous acc is written back).  Returns 0-dim
    device tensors, nothing synchronises: "loss_rgb", "loss_mask" (float32, views of "losses_f32"), "mse", "psnr" (float64, views of
    "out4" = {loss_rgb, loss_mask, mse, psnr} in float64), and the "workspace" to hand to the next call."""
    require_gpu()
    color, t32, t64, acc_in, o8, o32, R, kind = _loss_args(color, target, acc, occupancy, kind)
    dev = color.device
    acc_c = None if acc_in is None else acc_in.contiguous()
    nbytes = lib().dsn_train_loss_workspace_bytes(R)
    ws = workspace if workspace is not None and workspace.numel() >= nbytes else _scratch(nbytes, dev)
    out4 = torch.empty(4, dtype=torch.float64, device=dev)
    mask_on = o8 is not None or o32 is not None
    # (R = 0: empty tensors have no address; the mask term is announced by a pointer the call never reads)
    p = (lambda t, dtype=None: _ptr(t, dtype)) if R else (lambda t, dtype=None: None if t is None else _ptr(ws))
    _check(lib().dsn_train_loss(p(color, torch.float32), p(t32), p(t64), p(acc_c), p(o8), p(o32), R, kind,
                                int(bool(overwrite_acc and mask_on)), _ptr(out4), _ptr(ws), _stream()), "dsn_train_loss")
    if overwrite_acc and mask_on and R and acc_c.data_ptr() != acc.data_ptr():
        acc.copy_(acc_c.reshape(acc.shape))
    f32 = out4[:2].to(torch.float32)
    return {"loss_rgb": f32[0], "loss_mask": f32[1], "mse": out4[2], "psnr": out4[3], "out4": out4, "losses_f32": f32, "workspace": ws}


def train_loss_grad(color, target, acc=None, occupancy=None, kind="L2", up_rgb=None, up_mask=None, want_acc=True):
    """The seeds of the backward (dsn_train_loss_grad): (g_color [R,3], g_acc [R] or None) = d(up_rgb loss_rgb + up_mask loss_mask) /
    d(color, acc).  up_rgb / up_mask: float32 device scalars (tensors; Python numbers are copied over), None = 0 for that term.
    g_acc is returned when acc is given and want_acc is set."""
    require_gpu()
    color, t32, t64, acc, o8, o32, R, kind = _loss_args(color, target, acc, occupancy, kind)
    dev = color.device
    acc = None if acc is None else acc.contiguous()

    def up(u):
        if u is None:
            return None
        u = torch.as_tensor(u, dtype=torch.float32) if not torch.is_tensor(u) else u
        return u.detach().to(device=dev, dtype=torch.float32).reshape(()).contiguous()

    up_rgb, up_mask = up(up_rgb), up(up_mask)
    g_color = torch.empty(R, 3, dtype=torch.float32, device=dev)
    g_acc = torch.empty(R, dtype=torch.float32, device=dev) if (want_acc and acc is not None) else None
    if R:
        _check(lib().dsn_train_loss_grad(_ptr(color, torch.float32), _ptr(t32), _ptr(t64), _ptr(acc), _ptr(o8), _ptr(o32), R, kind,
                                         _ptr(up_rgb), _ptr(up_mask), _ptr(g_color), _ptr(g_acc), _stream()), "dsn_train_loss_grad")
    return g_color, g_acc


ADAM_TABLE, ADAM_BLOCK = 48, 1024      # dsn_adam_step: segments per launch, elements per workgroup (DSN_ADAM_*)


def adam_scalars(lr, weight_decay, betas, eps, step):
    """the float32 host scalars of dsn_adam_step's rule, as the library computes them: dict(w1, w2, b2, eps, wd, ss, c2) of Python
    floats (dsn_adam_scalars_host; no device work)"""
    out = (C.c_float * 7)()
    _check(lib().dsn_adam_scalars_host(float(lr), float(weight_decay), float(betas[0]), float(betas[1]), float(eps), float(step), out),
           "dsn_adam_scalars_host")
    return dict(zip(("w1", "w2", "b2", "eps", "wd", "ss", "c2"), (float(v) for v in out)))


def adam_step(params, grads, exp_avgs, exp_avg_sqs, lrs, weight_decays, betas, eps, step, packed=None):
    """One Adam step of every tensor in one launch (dsn_adam_step, the rule of include/dsnerf.h; more than ADAM_TABLE tensors: one
    launch per table): params, exp_avgs and exp_avg_sqs are updated in place - through their storage, so the version counters do not
    move (the caller's business: optim.Adam bumps them).  Lists of equal length of contiguous float32 tensors on one GPU (views at
    any 4-byte offset included); a None in `grads` skips that tensor.  lrs / weight_decays: one number per tensor, or one for all.
    step: the count t of this step (1 for the first), one for all tensors.  packed: a PackedParams - the lists must then be the
    model's 33 tensors in PARAM_ORDER, and the image is rebuilt from the new parameters behind the update on the same stream
    (follow with packed.note_repacked(params) once the version counters are final).  Nothing synchronises."""
    require_gpu()
    count = len(params)
    if not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == count):
        raise ValueError("params, grads, exp_avgs and exp_avg_sqs must have one entry per tensor")
    lrs = [float(lrs)] * count if not hasattr(lrs, "__len__") else [float(x) for x in lrs]
    weight_decays = [float(weight_decays)] * count if not hasattr(weight_decays, "__len__") else [float(x) for x in weight_decays]
    if len(lrs) != count or len(weight_decays) != count:
        raise ValueError("lrs and weight_decays must have one entry per tensor (or be one number)")
    if packed is not None and count != len(PARAM_ORDER):
        raise ValueError(f"packed needs the model's {len(PARAM_ORDER)} tensors in PARAM_ORDER, got {count}")
    if count == 0:
        return
    dev = params[0].device
    ptrs = [[], [], [], []]
    ns = []
    for row in zip(params, grads, exp_avgs, exp_avg_sqs):
        p = row[0]
        for k, t in enumerate(row):
            if t is None and k == 1:
                ptrs[k].append(None)
                continue
            if t.dtype != torch.float32 or not t.is_cuda or t.device != dev or not t.is_contiguous() or t.numel() != p.numel():
                raise ValueError("adam_step: every tensor must be contiguous float32 on the parameters' GPU, with its parameter's size: "
                                 f"got {t.dtype} {tuple(t.shape)} on {t.device} (contiguous: {t.is_contiguous()}) for a parameter "
                                 f"{tuple(p.shape)} on {dev}")
            ptrs[k].append(t.data_ptr() or None)
        ns.append(p.numel())
    arr = [(C.c_void_p * count)(*col) for col in ptrs]
    with torch.cuda.device(dev):
        _check(lib().dsn_adam_step(arr[0], arr[1], arr[2], arr[3], (C.c_int64 * count)(*ns), count, (C.c_double * count)(*lrs),
                                   (C.c_double * count)(*weight_decays), float(betas[0]), float(betas[1]), float(eps), float(step),
                                   None if packed is None else _ptr(packed.buf), _stream()), "dsn_adam_step")


def train_draws(R, S, seed, step, ray_base=0, ray_ids=None, noise_std=1.0, want_jitter=True, want_noise=True, out=None, device=None):
    """The training step's stratified jitter and density noise drawn on the device (dsn_train_draws, the rule of include/dsnerf.h):
    (jitter, noise), float32 [R, S] device tensors, None for the one not wanted.  A value is a pure function of (seed, step, ray id,
    sample, kind): seed is taken modulo 2^64, step and ray_base modulo 2^32; ray_ids: int32 [R] on the device (ray r's id) instead
    of ray_base + r.  noise = the unit draw times noise_std in float32.  out = (jitter, noise): float32 [R, S] device tensors to
    fill instead of fresh ones (contiguous; a view at any 4-byte offset will do), None where not wanted.  One launch on the current
    stream; nothing is allocated on the host, copied or read back."""
    require_gpu()
    R, S = int(R), int(S)
    if R < 0 or S < 0:
        raise ValueError("train_draws: R and S must not be negative")
    if ray_ids is not None:
        if not (torch.is_tensor(ray_ids) and ray_ids.is_cuda and ray_ids.dtype == torch.int32 and ray_ids.is_contiguous()
                and ray_ids.numel() == R):
            raise ValueError("train_draws: ray_ids must be a contiguous int32 device tensor with one id per ray")
        dev = ray_ids.device
    else:
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    given = (None, None) if out is None else tuple(out)
    arrays = []
    for name, want, t in (("jitter", want_jitter, given[0]), ("noise", want_noise, given[1])):
        if not want:
            arrays.append(None)
        elif t is None:
            arrays.append(_output((R, S), torch.float32, dev))
        else:
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (R, S)):
                raise ValueError(f"train_draws: out's {name} must be a contiguous float32 device tensor [{R}, {S}]")
            dev = t.device if ray_ids is None else dev
            arrays.append(t)
    if any(a is not None and a.device != dev for a in arrays):
        raise ValueError("train_draws: ray_ids and the outputs must live on one device")
    if arrays[0] is None and arrays[1] is None:
        raise ValueError("train_draws: neither jitter nor noise is wanted")
    with torch.cuda.device(dev):
        _check(lib().dsn_train_draws(int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF, int(ray_base) & 0xFFFFFFFF,
                                     _ptr(ray_ids) if R else None, R, S, float(noise_std), _ptr(arrays[0]) if R * S else None,
                                     _ptr(arrays[1]) if R * S else None, _stream()), "dsn_train_draws")
    return arrays[0], arrays[1]


def camera_rays(K, R, T, bounds, H, W, device=None, convention="zju"):
    """Whole-image rays + box near/far on the device: convention "zju" = utils/rays_utils.py:16-30, :63-97, :176-184
    (un-normalised directions, padded box), "h36m" = utils/h36m_utils.py:14-28, :61-76, :162-176 (unit directions,
    float32 slab test).
    K, R [3,3], T [3] or [3,1], bounds [2,3]: anything convertible to float64 tensors.  Returns
    (ray_o [H*W,3], ray_d [H*W,3], near [H*W], far [H*W], mask_at_box [H*W] bool), all on the device, uncompacted."""
    require_gpu()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if convention not in ("zju", "h36m"):
        raise ValueError("convention must be 'zju' or 'h36m'")
    K, R, T, bounds = _camera_f64(K, R, T, bounds, dev)
    n = H * W
    ray_o = _output((n, 3), torch.float32, dev)
    ray_d = _output((n, 3), torch.float32, dev)
    near = _output((n,), torch.float32, dev)
    far = _output((n,), torch.float32, dev)
    mask = _output((n,), torch.uint8, dev)
    _check(lib().dsn_camera_rays(_ptr(K), _ptr(R), _ptr(T), _ptr(bounds), H, W, RAYS_H36M if convention == "h36m" else RAYS_ZJU,
                                 _ptr(ray_o), _ptr(ray_d), _ptr(near), _ptr(far), _ptr(mask), _stream()), "dsn_camera_rays")
    return ray_o, ray_d, near, far, mask.bool()


def _camera_f64(K, R, T, bounds, dev):
    f64 = lambda a: torch.as_tensor(a, dtype=torch.float64).reshape(-1).to(dev).contiguous()
    K, R, T, bounds = f64(K), f64(R), f64(T), f64(bounds)
    if (K.numel(), R.numel(), T.numel(), bounds.numel()) != (9, 9, 3, 6):
        raise ValueError("K, R must be [3,3], T [3] or [3,1], bounds [2,3]")
    return K, R, T, bounds


def bound_mask(K, R, T, bounds, H, W, device=None):
    """get_bound_2d_mask (utils/rays_utils.py:49-60) on the device by the rule of include/dsnerf.h: the union of the reference's six
    corner loops, exact integers - cv2.fillPoly's result without the outline pixels its line drawing adds.  Returns uint8 [H,W]
    (all zero for a camera with a box corner behind it)."""
    require_gpu()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    K, R, T, bounds = _camera_f64(K, R, T, bounds, dev)
    out = torch.empty(int(H), int(W), dtype=torch.uint8, device=dev)
    _check(lib().dsn_bound_mask(_ptr(K), _ptr(R), _ptr(T), _ptr(bounds), int(H), int(W), _ptr(out), _stream()), "dsn_bound_mask")
    return out


def train_rays(img, K, R, T, bounds, mask_a, nrays, seed, convention="zju", mask_b=None, occupancy_src=None, bound_mask_in=None,
               workspace=None):
    """A training batch drawn on the device (dsn_train_rays; my_sample_ray / sample_ray_h36m by the rule of include/dsnerf.h).
    img [H,W,3] float64 or float32, mask_a (zju: msk_cihp; h36m: msk) and the optional mask_b (h36m: msk_cihp), occupancy_src,
    bound_mask_in [H,W] uint8: device tensors (anything else is copied over).  Returns a dict of device tensors - ray_o, ray_d, rgb
    [n,3], near, far [n], coord [n,2] int64, mask_at_box [n] bool, occupancy [n] uint8 (None without occupancy_src), bound_mask [H,W]
    uint8, status and rounds (int32 scalars) - without synchronising: the caller reads status (TRAIN_RAYS_*) when it wants to know."""
    require_gpu()
    if convention not in ("zju", "h36m"):
        raise ValueError("convention must be 'zju' or 'h36m'")
    if not 0 <= int(seed) < 2 ** 32:
        raise ValueError("seed must be 0 ... 2^32 - 1")
    dev = img.device if isinstance(img, torch.Tensor) and img.is_cuda else torch.device("cuda", torch.cuda.current_device())
    img = torch.as_tensor(img).to(dev)
    if img.dim() != 3 or img.shape[2] != 3:
        raise ValueError(f"img must be [H,W,3], got {tuple(img.shape)}")
    if img.dtype not in (torch.float64, torch.float32):
        raise TypeError(f"img must be float64 or float32, got {img.dtype}")
    img = img.contiguous()
    H, W = int(img.shape[0]), int(img.shape[1])

    def u8(m, what):
        if m is None:
            return None
        m = torch.as_tensor(m).to(dev)
        if tuple(m.shape) != (H, W):
            raise ValueError(f"{what} must be [{H},{W}], got {tuple(m.shape)}")
        return (m if m.dtype == torch.uint8 else m.to(torch.uint8)).contiguous()

    mask_a, mask_b = u8(mask_a, "mask"), u8(mask_b, "mask_b")
    occupancy_src, bound_mask_in = u8(occupancy_src, "occupancy_src"), u8(bound_mask_in, "bound_mask")
    if mask_a is None or (convention == "h36m" and mask_b is None):
        raise ValueError("mask is required (h36m: mask_b = msk_cihp too)")
    n = int(nrays)
    K, R, T, bounds = _camera_f64(K, R, T, bounds, dev)
    nbytes = lib().dsn_train_rays_workspace_bytes(H, W, n)
    if nbytes == 0:
        raise ValueError(f"train_rays: nrays must be 1 ... {TRAIN_RAYS_MAX_RAYS} and H * W below 2^31 (got nrays = {n}, {H} x {W})")
    ws = workspace if workspace is not None and workspace.numel() >= nbytes else _scratch(nbytes, dev)
    e = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=dev)
    out = {"ray_o": e(n, 3), "ray_d": e(n, 3), "near": e(n), "far": e(n), "coord": e(n, 2, dtype=torch.int64), "rgb": e(n, 3),
           "occupancy": None if occupancy_src is None else e(n, dtype=torch.uint8), "mask_at_box": e(n, dtype=torch.uint8),
           "bound_mask": e(H, W, dtype=torch.uint8), "status": e((), dtype=torch.int32), "rounds": e((), dtype=torch.int32)}
    g64, g32 = (img, None) if img.dtype == torch.float64 else (None, img)
    _check(lib().dsn_train_rays(_ptr(K), _ptr(R), _ptr(T), _ptr(bounds), H, W, RAYS_H36M if convention == "h36m" else RAYS_ZJU,
                                _ptr(g64), _ptr(g32), _ptr(mask_a), _ptr(mask_b), _ptr(bound_mask_in), _ptr(occupancy_src), n,
                                int(seed), _ptr(out["ray_o"]), _ptr(out["ray_d"]), _ptr(out["near"]), _ptr(out["far"]),
                                _ptr(out["coord"]), _ptr(out["rgb"]), _ptr(out["occupancy"]), _ptr(out["mask_at_box"]),
                                _ptr(out["bound_mask"]), _ptr(out["status"]), _ptr(out["rounds"]), _ptr(ws), ws.numel(), _stream()),
           "dsn_train_rays")
    out["mask_at_box"] = out["mask_at_box"].bool()
    out["workspace"] = ws
    return out


# ---- the datasets' image preparation (dsn_image_undistort / _morph / _resize / _prep: the rule of include/dsnerf.h) ---------------------
PREP_U8, PREP_F32, PREP_F64 = 0, 1, 2          # DSN_PREP_*
PREP_DILATE, PREP_ERODE = 0, 1
PREP_NEAREST, PREP_AREA = 0, 1
PREP_TILE_W, PREP_TILE_H = 64, 16              # DSN_PREP_TILE_*: the full-resolution tile a workgroup owns
PREP_MAX_SIDE, PREP_MAX_BATCH = 32768, 65535


def _prep_image(what, x, dtypes, name="x"):
    """(N, H, W, channels) of a batch of images [N, H, W] or [N, H, W, 3]: a contiguous tensor of one of `dtypes`"""
    if not torch.is_tensor(x):
        raise ValueError(f"{what}: {name} must be a torch tensor, got {type(x).__name__}")
    if x.dtype not in dtypes:
        raise ValueError(f"{what}: {name} must be {' or '.join(str(d) for d in dtypes)}, got {x.dtype}")
    if x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[3] != 3):
        raise ValueError(f"{what}: {name} must be [N, H, W] or [N, H, W, 3], got {tuple(x.shape)}")
    N, H, W = (int(v) for v in x.shape[:3])
    if H < 1 or W < 1 or H > PREP_MAX_SIDE or W > PREP_MAX_SIDE or N > PREP_MAX_BATCH:
        raise ValueError(f"{what}: {name} has {N} images of {H} x {W}; sides 1 ... {PREP_MAX_SIDE}, at most {PREP_MAX_BATCH} images")
    if not x.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous")
    return N, H, W, (3 if x.dim() == 4 else 1)


def _prep_on_device(what, *tensors):
    require_gpu()
    dev = tensors[0].device
    for t in tensors:
        if not t.is_cuda or t.device != dev:
            raise ValueError(f"{what}: the images must be tensors on one ROCm device, got {t.device}")
    return dev


def prep_camera(what, K, D, N, device=None):
    """K [N, 3, 3] (or one [3, 3] for all N) and D [N, nd] (or one [nd]), nd = 4, 5 or 8, as the contiguous float64 arrays
    dsn_image_undistort and dsn_image_prep read.  Host arrays (numpy, lists, CPU tensors) are checked on the host and, with `device`,
    uploaded in one copy; device tensors are used where they are, after their skew entries have been read back for the check (N
    numbers: pass host cameras to avoid the wait).  A skew K[0, 1] other than 0 is refused: the rule has no such term."""
    Kt = torch.as_tensor(K).to(torch.float64)
    Dt = torch.as_tensor(D).to(torch.float64)
    if Kt.dim() == 2:
        Kt = Kt.unsqueeze(0).expand(N, -1, -1)
    if Dt.dim() == 1:
        Dt = Dt.unsqueeze(0).expand(N, -1)
    if tuple(Kt.shape) != (N, 3, 3):
        raise ValueError(f"{what}: K must be [3, 3] or [{N}, 3, 3], got {tuple(Kt.shape)}")
    if Dt.dim() != 2 or Dt.shape[0] != N or Dt.shape[1] not in (4, 5, 8):
        raise ValueError(f"{what}: D must be [nd] or [{N}, nd] with nd = 4, 5 or 8, got {tuple(Dt.shape)}")
    if N and bool((Kt[:, 0, 1] != 0).any()):
        raise ValueError(f"{what}: K has a skew term K[0, 1] other than 0, which the undistortion rule does not model")
    Kt, Dt = Kt.contiguous(), Dt.contiguous()
    if device is None:
        return Kt, Dt
    if not Kt.is_cuda and not Dt.is_cuda:          # the usual case: one upload for both
        both = torch.cat([Kt.reshape(-1), Dt.reshape(-1)]).to(device)
        return both[:9 * N].view(N, 3, 3), both[9 * N:].view(N, Dt.shape[1])
    return Kt.to(device), Dt.to(device)


def image_undistort(x, K, D):
    """dsn_image_undistort: x uint8 or float32 device tensor [N, H, W] or [N, H, W, 3]; K, D as prep_camera takes them -> the
    undistorted images, same shape and dtype.  N = 0: an empty tensor, no launch."""
    N, H, W, ch = _prep_image("image_undistort", x, (torch.uint8, torch.float32))
    Kd, Dd = prep_camera("image_undistort", K, D, N, x.device if x.is_cuda else None)          # (its checks need no device: they come first)
    dev = _prep_on_device("image_undistort", x)
    out = _output(tuple(x.shape), x.dtype, dev)
    with torch.cuda.device(dev):
        _check(lib().dsn_image_undistort(_ptr(x) if N else None, _ptr(out) if N else None, _ptr(Kd) if N else None, _ptr(Dd) if N else None,
                                         Dd.shape[1], N, H, W, ch, PREP_U8 if x.dtype == torch.uint8 else PREP_F32, _stream()),
               "dsn_image_undistort")
    return out


def image_morph(m, k, op):
    """dsn_image_morph: m uint8 device tensor [N, H, W], box k = 1 ... 15, op PREP_DILATE or PREP_ERODE -> uint8 [N, H, W]"""
    N, H, W, ch = _prep_image("image_morph", m, (torch.uint8,), "m")
    if ch != 1:
        raise ValueError(f"image_morph: m must be [N, H, W], got {tuple(m.shape)}")
    if int(k) != k or not 1 <= int(k) <= 15:
        raise ValueError(f"image_morph: k must be an integer 1 ... 15, got {k!r}")
    if op not in (PREP_DILATE, PREP_ERODE):
        raise ValueError(f"image_morph: op must be PREP_DILATE or PREP_ERODE, got {op!r}")
    dev = _prep_on_device("image_morph", m)
    out = _output(tuple(m.shape), torch.uint8, dev)
    with torch.cuda.device(dev):
        _check(lib().dsn_image_morph(_ptr(m) if N else None, _ptr(out) if N else None, N, H, W, int(k), op, _stream()), "dsn_image_morph")
    return out


def _prep_factor(what, c, H, W):
    if c not in (1, 2, 4):
        raise ValueError(f"{what}: the factor must be 1, 2 or 4, got {c!r}")
    if H % c or W % c:
        raise ValueError(f"{what}: {H} x {W} is not a multiple of the factor {c} (OpenCV's path for such sizes is another algorithm)")
    return int(c)


def image_resize(x, c, mode):
    """dsn_image_resize: x uint8 or float32 device tensor [N, H, W] or [N, H, W, 3], c = 1, 2 or 4 dividing H and W, mode PREP_AREA or
    PREP_NEAREST -> [N, H / c, W / c(, 3)] of x's dtype"""
    N, H, W, ch = _prep_image("image_resize", x, (torch.uint8, torch.float32))
    c = _prep_factor("image_resize", c, H, W)
    if mode not in (PREP_NEAREST, PREP_AREA):
        raise ValueError(f"image_resize: mode must be PREP_NEAREST or PREP_AREA, got {mode!r}")
    dev = _prep_on_device("image_resize", x)
    out = _output((N, H // c, W // c) + ((3,) if ch == 3 else ()), x.dtype, dev)
    with torch.cuda.device(dev):
        _check(lib().dsn_image_resize(_ptr(x) if N else None, _ptr(out) if N else None, N, H, W, ch,
                                      PREP_U8 if x.dtype == torch.uint8 else PREP_F32, c, mode, _stream()), "dsn_image_resize")
    return out


def image_prep(img_u8, msk_cihp, K, D, c=2, border=5, dtype=torch.float64, want_u8=False, want_masks=True):
    """dsn_image_prep, the fused ZJU item in one launch: img_u8 [N, H0, W0, 3] and msk_cihp [N, H0, W0] uint8 device tensors, K, D as
    prep_camera takes them -> (img [N, H, W, 3] of `dtype` (float64 or float32), img_u8 [N, H, W, 3] or None, msk_fg, msk_cihp
    [N, H, W] uint8 or None) with H = H0 / c, W = W0 / c."""
    N, H0, W0, ch = _prep_image("image_prep", img_u8, (torch.uint8,), "img_u8")
    if ch != 3:
        raise ValueError(f"image_prep: img_u8 must be [N, H0, W0, 3], got {tuple(img_u8.shape)}")
    Nm, Hm, Wm, chm = _prep_image("image_prep", msk_cihp, (torch.uint8,), "msk_cihp")
    if (Nm, Hm, Wm, chm) != (N, H0, W0, 1):
        raise ValueError(f"image_prep: msk_cihp must be [{N}, {H0}, {W0}], got {tuple(msk_cihp.shape)}")
    c = _prep_factor("image_prep", c, H0, W0)
    if int(border) != border or not 1 <= int(border) <= 15:
        raise ValueError(f"image_prep: border must be an integer 1 ... 15, got {border!r}")
    if dtype not in (torch.float64, torch.float32):
        raise ValueError(f"image_prep: dtype must be torch.float64 or torch.float32, got {dtype}")
    Kd, Dd = prep_camera("image_prep", K, D, N, img_u8.device if img_u8.is_cuda else None)
    dev = _prep_on_device("image_prep", img_u8, msk_cihp)
    H, W = H0 // c, W0 // c
    img = _output((N, H, W, 3), dtype, dev)
    u8 = _output((N, H, W, 3), torch.uint8, dev) if want_u8 else None
    fg = _output((N, H, W), torch.uint8, dev) if want_masks else None
    ci = _output((N, H, W), torch.uint8, dev) if want_masks else None
    p = lambda t: _ptr(t) if (t is not None and N) else None      # noqa: E731
    with torch.cuda.device(dev):
        _check(lib().dsn_image_prep(p(img_u8), p(msk_cihp), p(Kd), p(Dd), Dd.shape[1], N, H0, W0, c, int(border),
                                    PREP_F64 if dtype == torch.float64 else PREP_F32, p(img), p(u8), p(fg), p(ci), _stream()), "dsn_image_prep")
    return img, u8, fg, ci


# ---- baseline JPEG (dsn_jpeg_*: the rule of include/dsnerf.h) ----------------------------------------------------------------------------
JPEG_420, JPEG_444, JPEG_GRAY = 0, 1, 2          # DSN_JPEG_*
JPEG_U8, JPEG_F32 = 0, 1
JPEG_NONFINITE, JPEG_OVERFLOW = 1, 2
JPEG_MODES = {"420": JPEG_420, "444": JPEG_444, "gray": JPEG_GRAY, "grey": JPEG_GRAY}


def jpeg_mode(subsampling, channels):
    """the DSN_JPEG_* mode of an image with `channels` channels: one channel is always a one-component file"""
    if channels == 1:
        return JPEG_GRAY
    m = JPEG_MODES.get(str(subsampling))
    if m is None or m == JPEG_GRAY:
        raise ValueError(f"jpeg: subsampling of a three-channel image must be '420' or '444', got {subsampling!r}")
    return m


def jpeg_blocks(H, W, mode):
    """8 x 8 blocks of a frame's scan, dummy blocks included"""
    s = 16 if mode == JPEG_420 else 8
    return ((W + s - 1) // s) * ((H + s - 1) // s) * {JPEG_420: 6, JPEG_444: 3, JPEG_GRAY: 1}[mode]


def jpeg_max_bytes(H, W, mode):
    """dsn_jpeg_max_bytes: the capacity no frame of this size can exceed"""
    n = lib().dsn_jpeg_max_bytes(int(H), int(W), int(mode))
    if n == 0:
        raise ValueError(f"jpeg: {H} x {W} in mode {mode} is outside what dsn_jpeg_* takes (sides 1 ... 65535, blocks x 1664 below 2^31)")
    return int(n)


def jpeg_header(H, W, mode, quality):
    """dsn_jpeg_header_host: SOI ... SOS as bytes (host only, no device)"""
    buf = (C.c_uint8 * 640)()
    n = C.c_int(0)
    _check(lib().dsn_jpeg_header_host(int(H), int(W), int(mode), int(quality), buf, 640, C.byref(n)), "dsn_jpeg_header_host")
    return bytes(buf[:n.value])


def _jpeg_images(what, images):
    """(F, H, W, mode-independent channel count, dtype code) of a contiguous device stack [F, H, W] or [F, H, W, 3]"""
    if not torch.is_tensor(images) or images.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{what}: images must be a uint8 or float32 tensor")
    if images.dim() not in (3, 4) or (images.dim() == 4 and images.shape[3] != 3):
        raise ValueError(f"{what}: images must be [F, H, W] or [F, H, W, 3], got {tuple(images.shape)}")
    require_gpu()
    if not images.is_cuda or not images.is_contiguous():
        raise ValueError(f"{what}: images must be a contiguous tensor on a ROCm device")
    F, H, W = (int(v) for v in images.shape[:3])
    return F, H, W, (3 if images.dim() == 4 else 1), (JPEG_U8 if images.dtype == torch.uint8 else JPEG_F32)


def _jpeg_check_mode(what, mode, ch):
    if (mode == JPEG_GRAY) != (ch == 1) or mode not in (JPEG_420, JPEG_444, JPEG_GRAY):
        raise ValueError(f"{what}: mode {mode!r} does not fit images with {ch} channel(s)")


def jpeg_coefficients(images, mode, quality=95, rgb=False, scale=255.0):
    """dsn_jpeg_coefficients: -> (coef int16 [F, blocks, 64] in zigzag and scan order, status int32 [F]) on the device"""
    F, H, W, ch, dt = _jpeg_images("jpeg_coefficients", images)
    _jpeg_check_mode("jpeg_coefficients", mode, ch)
    dev = images.device
    coef = _output((F, jpeg_blocks(H, W, mode), 64), torch.int16, dev)
    status = _output((F,), torch.int32, dev)
    with torch.cuda.device(dev):
        _check(lib().dsn_jpeg_coefficients(_ptr(images) if F else None, dt, F, H, W, mode, int(quality), int(bool(rgb)), float(scale),
                                           _ptr(coef) if F else None, _ptr(status) if F else None, _stream()), "dsn_jpeg_coefficients")
    return coef, status


def jpeg_scan(coef, H, W, mode, quality=95, status_in=None, capacity=None, out=None):
    """dsn_jpeg_scan: coef int16 [F, blocks, 64] -> (out uint8 [F, capacity], lengths int32 [F], status int32 [F]) on the device.
    `out` (optional): a caller's uint8 [F, capacity] buffer, written only up to each frame's length."""
    if not torch.is_tensor(coef) or coef.dtype != torch.int16 or coef.dim() != 3 or coef.shape[2] != 64:
        raise ValueError("jpeg_scan: coef must be an int16 tensor [F, blocks, 64]")
    require_gpu()
    if not coef.is_cuda or not coef.is_contiguous():
        raise ValueError("jpeg_scan: coef must be a contiguous tensor on a ROCm device")
    F = int(coef.shape[0])
    if int(coef.shape[1]) != jpeg_blocks(H, W, mode):
        raise ValueError(f"jpeg_scan: {H} x {W} in mode {mode} has {jpeg_blocks(H, W, mode)} blocks, coef has {int(coef.shape[1])}")
    dev = coef.device
    if out is None:
        capacity = jpeg_max_bytes(H, W, mode) if capacity is None else int(capacity)
        out = _output((F, capacity), torch.uint8, dev)
    elif out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != F or not out.is_contiguous() or out.device != dev:
        raise ValueError("jpeg_scan: out must be a contiguous uint8 [F, capacity] tensor on coef's device")
    lengths = _output((F,), torch.int32, dev)
    status = _output((F,), torch.int32, dev)
    nws = lib().dsn_jpeg_workspace_bytes(max(F, 1), int(H), int(W), int(mode))
    ws = _scratch(nws, dev)
    with torch.cuda.device(dev):
        _check(lib().dsn_jpeg_scan(_ptr(coef) if F else None, _ptr(status_in) if (status_in is not None and F) else None, F, int(H), int(W),
                                   int(mode), int(quality), _ptr(out) if F else None, int(out.shape[1]), _ptr(lengths) if F else None,
                                   _ptr(status) if F else None, _ptr(ws), nws, _stream()), "dsn_jpeg_scan")
    return out, lengths, status


def jpeg_encode(images, mode, quality=95, rgb=False, scale=255.0, capacity=None, out=None, workspace=None):
    """dsn_jpeg_encode: images uint8 / float32 [F, H, W, 3] (JPEG_GRAY: [F, H, W]) on the device -> (out uint8 [F, capacity] whose row f
    starts with frame f's complete file, lengths int32 [F]: the bytes each file needs, status int32 [F]: OR of JPEG_NONFINITE /
    JPEG_OVERFLOW).  Nothing is copied back and nothing waits."""
    F, H, W, ch, dt = _jpeg_images("jpeg_encode", images)
    _jpeg_check_mode("jpeg_encode", mode, ch)
    dev = images.device
    if out is None:
        capacity = jpeg_max_bytes(H, W, mode) if capacity is None else int(capacity)
        out = _output((F, capacity), torch.uint8, dev)
    elif out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != F or not out.is_contiguous() or out.device != dev:
        raise ValueError("jpeg_encode: out must be a contiguous uint8 [F, capacity] tensor on the images' device")
    lengths = _output((F,), torch.int32, dev)
    status = _output((F,), torch.int32, dev)
    nws = lib().dsn_jpeg_workspace_bytes(max(F, 1), H, W, int(mode))
    if nws == 0:
        jpeg_max_bytes(H, W, mode)          # raises with the limits
    ws = _scratch(nws, dev) if workspace is None else workspace
    with torch.cuda.device(dev):
        _check(lib().dsn_jpeg_encode(_ptr(images) if F else None, dt, F, H, W, int(mode), int(quality), int(bool(rgb)), float(scale),
                                     _ptr(out) if F else None, int(out.shape[1]), _ptr(lengths) if F else None, _ptr(status) if F else None,
                                     _ptr(ws), int(ws.numel()), _stream()), "dsn_jpeg_encode")
    return out, lengths, status


# ---- baseline JPEG decoding (dsn_jpeg_parse_host, dsn_jpegd_*, dsn_jpeg_decode: the rule of include/dsnerf.h) -----------------------------
JPEGD_CORRUPT, JPEGD_PADDING, JPEGD_UNCONVERGED, JPEGD_UNMATCHED, JPEGD_OVERRUN, JPEGD_MARKER, JPEGD_COUNT = 1, 2, 4, 16, 32, 64, 128
JPEGD_REASONS = ["ok", "not_jpeg", "truncated", "progressive", "extended", "arithmetic", "precision", "sampling", "components", "table16",
                 "multiscan", "restart", "missing_table", "bad_table", "no_eoi", "bad_segment", "too_large"]          # DSN_JPEGD_* parse status
JPEGD_SUBSEQ_BITS = 512           # the default subsequence: the lowest median of 512 / 1024 / 2048 (profiles/jpeg_decode_bench.json)
JPEGD_ROUNDS = 16                 # rounds per launch group: the wrappers read the status words once per group


class JpegdHuff(C.Structure):
    _fields_ = [("bits", C.c_uint8 * 16), ("vals", C.c_uint8 * 256), ("lim", C.c_uint32 * 16), ("base", C.c_int32 * 16)]


class JpegdDesc(C.Structure):
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("mode", C.c_int32), ("ncomp", C.c_int32), ("scan_offset", C.c_int32),
                ("scan_length", C.c_int32), ("file_length", C.c_int32), ("reserved", C.c_int32), ("qsel", C.c_uint8 * 4),
                ("dcsel", C.c_uint8 * 4), ("acsel", C.c_uint8 * 4), ("pad", C.c_uint8 * 4), ("quant", (C.c_uint8 * 64) * 4),
                ("dc", JpegdHuff * 4), ("ac", JpegdHuff * 4)]


def jpeg_parse(data):
    """dsn_jpeg_parse_host: a file's bytes -> (JpegdDesc, parse status: an index into JPEGD_REASONS).  Host only, no device."""
    data = bytes(data)
    d, st = JpegdDesc(), C.c_int(0)
    _check(lib().dsn_jpeg_parse_host(data, len(data), C.byref(d), C.byref(st)), "dsn_jpeg_parse_host")
    return d, st.value


class JpegdBatch:
    """files of one (H, W, mode) on the device: the concatenated bytes (padded to 16), their offsets, the descriptor table"""

    def __init__(self, files, descs, device=None):
        require_gpu()
        if not files or len(files) != len(descs):
            raise ValueError("jpeg: a batch needs at least one file and one descriptor per file")
        self.F = len(files)
        self.H, self.W, self.mode = int(descs[0].H), int(descs[0].W), int(descs[0].mode)
        if any((int(d.H), int(d.W), int(d.mode)) != (self.H, self.W, self.mode) for d in descs):
            raise ValueError("jpeg: the files of one device call share H, W and mode (group them first)")
        self.max_scan = max(max(int(d.scan_length) for d in descs), 1)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        off = [0]
        for f in files:
            off.append(off[-1] + len(f))
        joined = bytearray(b"".join(bytes(f) for f in files))
        joined += bytes(-len(joined) % 16)          # the library reads 16 aligned bytes at a time, never past files_bytes
        self.files = torch.frombuffer(joined, dtype=torch.uint8).to(dev)
        self.offsets = torch.tensor(off, dtype=torch.int64).to(dev)
        self.desc = torch.frombuffer(bytearray(b"".join(bytes(d) for d in descs)), dtype=torch.uint8).to(dev)
        self.device = dev
        self.workspace_bytes = int(lib().dsn_jpegd_workspace_bytes(self.F, self.H, self.W, self.mode, self.max_scan))
        if self.workspace_bytes == 0:
            raise ValueError(f"jpeg: {self.F} frames of {self.H} x {self.W} in mode {self.mode} are outside what dsn_jpegd_* takes")
        self.blocks = jpeg_blocks(self.H, self.W, self.mode)

    def workspace(self):
        return _scratch(self.workspace_bytes, self.device)

    def geometry(self):
        return self.F, self.H, self.W, self.mode, self.max_scan


def _jpegd_bits(what, subseq_bits):
    b = JPEGD_SUBSEQ_BITS if subseq_bits is None else int(subseq_bits)
    if b < 128 or b > 4096 or b % 32:
        raise ValueError(f"{what}: subseq_bits must be a multiple of 32 from 128 to 4096, got {subseq_bits!r}")
    return b


def jpegd_sync(batch, workspace, subseq_bits=None, restart=True, rounds=JPEGD_ROUNDS):
    """dsn_jpegd_sync: `rounds` rounds (restart: unstuffing and round 0 first) on the state in `workspace` ->
    (converged int32 [F], rounds int32 [F]) on the device"""
    b = _jpegd_bits("jpegd_sync", subseq_bits)
    conv = _output((batch.F,), torch.int32, batch.device)
    rnd = _output((batch.F,), torch.int32, batch.device)
    with torch.cuda.device(batch.device):
        _check(lib().dsn_jpegd_sync(_ptr(batch.files), int(batch.files.numel()), _ptr(batch.offsets), _ptr(batch.desc), *batch.geometry(), b,
                                    int(bool(restart)), int(rounds), _ptr(conv), _ptr(rnd), _ptr(workspace), int(workspace.numel()),
                                    _stream()), "dsn_jpegd_sync")
    return conv, rnd


def jpegd_coefficients(batch, workspace, subseq_bits=None):
    """dsn_jpegd_coefficients: the converged state in `workspace` -> (coef int16 [F, blocks, 64] with DC values, status int32 [F])"""
    b = _jpegd_bits("jpegd_coefficients", subseq_bits)
    coef = _output((batch.F, batch.blocks, 64), torch.int16, batch.device)
    status = _output((batch.F,), torch.int32, batch.device)
    with torch.cuda.device(batch.device):
        _check(lib().dsn_jpegd_coefficients(_ptr(batch.desc), *batch.geometry(), b, _ptr(coef), _ptr(status), _ptr(workspace),
                                            int(workspace.numel()), _stream()), "dsn_jpegd_coefficients")
    return coef, status


def _jpegd_out(batch, gray):
    if gray and batch.mode != JPEG_GRAY:
        raise ValueError("jpeg: gray=True needs one-component files")
    return _output((batch.F, batch.H, batch.W) if gray else (batch.F, batch.H, batch.W, 3), torch.uint8, batch.device)


def jpegd_pixels(batch, coef, status, workspace, rgb=False, gray=False):
    """dsn_jpegd_pixels: coef int16 [F, blocks, 64], status int32 [F] or None -> uint8 [F, H, W, 3] (gray: [F, H, W]) on the device"""
    if not torch.is_tensor(coef) or coef.dtype != torch.int16 or tuple(coef.shape) != (batch.F, batch.blocks, 64) or not coef.is_contiguous():
        raise ValueError(f"jpegd_pixels: coef must be a contiguous int16 tensor [{batch.F}, {batch.blocks}, 64]")
    out = _jpegd_out(batch, gray)
    with torch.cuda.device(batch.device):
        _check(lib().dsn_jpegd_pixels(_ptr(coef), _ptr(status), _ptr(batch.desc), *batch.geometry(), int(bool(rgb)), int(bool(gray)),
                                      _ptr(out), _ptr(workspace), int(workspace.numel()), _stream()), "dsn_jpegd_pixels")
    return out


def jpegd_workspace_coef(batch, workspace):
    """the coefficients dsn_jpeg_decode left in `workspace`: an int16 [F, blocks, 64] view of it"""
    p = C.c_void_p(0)
    _check(lib().dsn_jpegd_workspace_coef(_ptr(workspace), *batch.geometry(), C.byref(p)), "dsn_jpegd_workspace_coef")
    at = int(p.value) - workspace.data_ptr()
    return workspace[at:at + batch.F * batch.blocks * 128].view(torch.int16).view(batch.F, batch.blocks, 64)


def jpeg_decode(batch, subseq_bits=None, rgb=False, gray=False, rounds=JPEGD_ROUNDS, workspace=None):
    """dsn_jpeg_decode, then - only if a frame came back UNCONVERGED - further groups of `rounds` rounds and the two closing steps:
    -> (out uint8 [F, H, W, 3] or [F, H, W], status int32 [F], rounds int32 [F], host copy of the status words).  One device->host
    copy of 2 F words per group."""
    b = _jpegd_bits("jpeg_decode", subseq_bits)
    ws = batch.workspace() if workspace is None else workspace
    out = _jpegd_out(batch, gray)
    both = _output((2, batch.F), torch.int32, batch.device)          # status, rounds
    with torch.cuda.device(batch.device):
        _check(lib().dsn_jpeg_decode(_ptr(batch.files), int(batch.files.numel()), _ptr(batch.offsets), _ptr(batch.desc), *batch.geometry(), b,
                                     int(rounds), int(bool(rgb)), int(bool(gray)), _ptr(out), _ptr(both[0]), _ptr(both[1]), _ptr(ws),
                                     int(ws.numel()), _stream()), "dsn_jpeg_decode")
    host = both.cpu().numpy()
    if (host[0] & JPEGD_UNCONVERGED).any():
        while True:
            conv, rnd = jpegd_sync(batch, ws, b, restart=False, rounds=rounds)
            if bool(torch.stack([conv, rnd]).cpu().numpy()[0].all()):
                break
        coef = jpegd_workspace_coef(batch, ws)
        with torch.cuda.device(batch.device):
            _check(lib().dsn_jpegd_coefficients(_ptr(batch.desc), *batch.geometry(), b, _ptr(coef), _ptr(both[0]), _ptr(ws), int(ws.numel()),
                                                _stream()), "dsn_jpegd_coefficients")
            _check(lib().dsn_jpegd_pixels(_ptr(coef), _ptr(both[0]), _ptr(batch.desc), *batch.geometry(), int(bool(rgb)), int(bool(gray)),
                                          _ptr(out), _ptr(ws), int(ws.numel()), _stream()), "dsn_jpegd_pixels")
        both[1].copy_(rnd)
        host = both.cpu().numpy()
    return out, both[0], both[1], host


# ---- PNG decoding (dsn_png_parse_host, dsn_png_workspace_*, dsn_png_decode: the rule of include/dsnerf.h) -----------------------------------
(PNG_EARLY_END, PNG_BLOCK_TYPE, PNG_STORED_LEN, PNG_BAD_CODES, PNG_NO_CODE, PNG_FAR_DISTANCE, PNG_TOO_MUCH, PNG_TOO_LITTLE, PNG_FILTER,
 PNG_ADLER) = (1 << k for k in range(10))
PNG_STATUS_NAMES = ["the stream ends early", "a reserved block type", "a stored block whose LEN and NLEN disagree",
                    "over-subscribed or unusable code lengths", "a code that matches nothing", "a distance that reaches before the output's start",
                    "more output than the image holds", "less output than the image needs", "a filter byte above 4", "an Adler-32 mismatch"]
PNG_REASONS = ["ok", "not_png", "truncated", "crc", "bad_ihdr", "interlace", "depth16", "no_ihdr", "no_idat", "no_plte", "zero_dim", "too_large",
               "zlib_method", "zlib_dict", "zlib_check"]          # DSN_PNG_* parse status
PNG_CHANNELS = {"bgr": 0, "rgb": 1, "native": 2}
PNG_GATHER, PNG_INFLATE, PNG_ADLER_STAGE, PNG_UNFILTER, PNG_PIXELS, PNG_ALL = 1, 2, 4, 8, 16, 31


class PngDesc(C.Structure):
    _fields_ = [("W", C.c_int32), ("H", C.c_int32), ("bits", C.c_int32), ("ctype", C.c_int32), ("channels", C.c_int32),
                ("row_bytes", C.c_int32), ("raw_bytes", C.c_int32), ("npal", C.c_int32), ("nseg", C.c_int32), ("zlen", C.c_int32),
                ("file_length", C.c_int32), ("reserved", C.c_int32 * 5), ("palette", (C.c_uint8 * 3) * 256)]


def png_status_text(status):
    return ", ".join(n for k, n in enumerate(PNG_STATUS_NAMES) if int(status) >> k & 1)


def png_parse(data, seg_capacity=64):
    """dsn_png_parse_host: a file's bytes -> (PngDesc, segments [(offset, length), ...], parse status: an index into PNG_REASONS).
    Host only, no device."""
    data = bytes(data)
    d, st = PngDesc(), C.c_int(0)
    while True:
        segs = (C.c_uint32 * (2 * seg_capacity))()
        _check(lib().dsn_png_parse_host(data, len(data), C.byref(d), segs, seg_capacity, C.byref(st)), "dsn_png_parse_host")
        if st.value != 0 or d.nseg <= seg_capacity:
            break
        seg_capacity = int(d.nseg)
    n = min(int(d.nseg), seg_capacity) if st.value == 0 else 0
    return d, [(int(segs[2 * k]), int(segs[2 * k + 1])) for k in range(n)], st.value


class PngBatch:
    """files of one (W, H, bits, ctype) on the device: the concatenated bytes, the IDAT segment table, the descriptor table"""

    def __init__(self, files, descs, segments, device=None):
        require_gpu()
        if not files or len(files) != len(descs) or len(files) != len(segments):
            raise ValueError("png: a batch needs at least one file, and a descriptor and a segment list per file")
        self.F = len(files)
        self.W, self.H, self.bits, self.ctype = (int(getattr(descs[0], k)) for k in ("W", "H", "bits", "ctype"))
        if any((int(d.W), int(d.H), int(d.bits), int(d.ctype)) != (self.W, self.H, self.bits, self.ctype) for d in descs):
            raise ValueError("png: the files of one device call share W, H, bit depth and colour type (group them first)")
        self.channels, self.row_bytes, self.raw_bytes = int(descs[0].channels), int(descs[0].row_bytes), int(descs[0].raw_bytes)
        self.max_stream = max(max(int(d.zlen) for d in descs), 1)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        table, first, base = [], [0], 0
        for f, seg in zip(files, segments):
            at = 0
            for o, n in seg:
                table.append((base + o, at, n))
                at += n
            first.append(len(table))
            base += len(f)
        joined = bytearray(b"".join(bytes(f) for f in files))
        self.files = torch.frombuffer(joined, dtype=torch.uint8).to(dev)
        self.segs = torch.tensor(table if table else [(0, 0, 0)], dtype=torch.int64).to(dev)
        self.n_segs = len(table)
        self.seg_first = torch.tensor(first, dtype=torch.int32).to(dev)
        self.desc = torch.frombuffer(bytearray(b"".join(bytes(d) for d in descs)), dtype=torch.uint8).to(dev)
        self.device = dev
        lay = (C.c_size_t * 8)()
        if lib().dsn_png_workspace_layout(self.F, self.W, self.H, self.bits, self.ctype, self.max_stream, lay) != 0:
            raise ValueError(f"png: {self.F} files of {self.W} x {self.H}, {self.bits} bits, colour type {self.ctype} are outside what "
                             "dsn_png_decode takes")
        self.layout = [int(v) for v in lay]
        self.workspace_bytes = self.layout[7]

    def workspace(self):
        return _scratch(self.workspace_bytes, self.device)

    def geometry(self):
        return self.F, self.W, self.H, self.bits, self.ctype, self.max_stream

    def out_shape(self, channels, first_channel):
        if first_channel:
            return (self.F, self.H, self.W)
        return (self.F, self.H, self.W, self.channels if channels == "native" else 3)

    def views(self, workspace):
        """what a decode left in `workspace`: (meta int32 [F, 8], streams uint8 [F, stride], raw uint8 [F, stride], rows uint8 [F, stride])"""
        m, s, ss, r, rs, w, ws, _ = self.layout
        F = self.F
        return (workspace[m:m + F * 32].view(torch.int32).view(F, 8), workspace[s:s + F * ss].view(F, ss), workspace[r:r + F * rs].view(F, rs),
                workspace[w:w + F * ws].view(F, ws))


def png_decode(batch, channels="bgr", first_channel=False, stages=PNG_ALL, workspace=None, out=None, status=None):
    """dsn_png_decode -> (out uint8 [F, H, W, C] or [F, H, W], status int32 [F]) on the device; no wait, no copy"""
    if channels not in PNG_CHANNELS:
        raise ValueError(f"png: channels must be 'bgr', 'rgb' or 'native', got {channels!r}")
    ws = batch.workspace() if workspace is None else workspace
    shape = batch.out_shape(channels, bool(first_channel))
    if out is None:
        out = _output(shape, torch.uint8, batch.device)
    elif tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"png_decode: out must be a contiguous uint8 tensor {shape}")
    if status is None:
        status = _output((batch.F,), torch.int32, batch.device)
    with torch.cuda.device(batch.device):
        _check(lib().dsn_png_decode(_ptr(batch.files), int(batch.files.numel()), _ptr(batch.segs), batch.n_segs, _ptr(batch.seg_first),
                                    _ptr(batch.desc), *batch.geometry(), PNG_CHANNELS[channels], int(bool(first_channel)), int(stages),
                                    _ptr(out), _ptr(status), _ptr(ws), int(ws.numel()), _stream()), "dsn_png_decode")
    return out, status


# ---- PNG encoding (dsn_png_filter / _adler / _deflate / _container / _encode, dsn_huff_lengths: the rule of include/dsnerf.h) --------------------
PNGE_GRAY, PNGE_COLOUR, PNGE_REPLICATE = 0, 1, 2          # DSN_PNGE_*
PNGE_ADAPTIVE = 5
PNGE_NONFINITE, PNGE_OVERFLOW = 1, 2
PNGE_CHUNK_MIN, PNGE_CHUNK_MAX, PNGE_CHUNK_DEFAULT = 256, 32768, 32768
PNGE_FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": PNGE_ADAPTIVE}


def pnge_filter(filter):
    """the DSN_PNGE filter number of "adaptive", a filter's name or 0 ... 4"""
    f = PNGE_FILTERS.get(filter, filter) if isinstance(filter, str) else filter
    if isinstance(f, bool) or not isinstance(f, int) or not 0 <= f <= PNGE_ADAPTIVE or (not isinstance(filter, str) and f == PNGE_ADAPTIVE):
        raise ValueError(f"png: filter must be 'adaptive', a filter's name or 0 ... 4, got {filter!r}")
    return f


def pnge_chunk(chunk):
    c = PNGE_CHUNK_DEFAULT if chunk is None else chunk
    if isinstance(c, bool) or int(c) != c or not PNGE_CHUNK_MIN <= int(c) <= PNGE_CHUNK_MAX or int(c) & (int(c) - 1):
        raise ValueError(f"png: chunk must be a power of two from {PNGE_CHUNK_MIN} to {PNGE_CHUNK_MAX}, got {chunk!r}")
    return int(c)


def pnge_mode(images, replicate):
    """the DSN_PNGE_* mode of a stack [F, H, W] or [F, H, W, 3]"""
    if images.dim() == 4:
        if replicate:
            raise ValueError("png: replicate=True takes one-channel images")
        return PNGE_COLOUR
    return PNGE_REPLICATE if replicate else PNGE_GRAY


def png_encode_max_bytes(W, H, channels, chunk=None):
    """dsn_png_encode_max_bytes: the capacity no file of this size can exceed (every chunk stored)"""
    n = lib().dsn_png_encode_max_bytes(int(W), int(H), int(channels), pnge_chunk(chunk))
    if n == 0:
        raise ValueError(f"png: {W} x {H} with {channels} channel(s) is outside what dsn_png_encode takes (sides 1 ... 16384, 1 or 3 channels)")
    return int(n)


def png_filter(images, mode, rgb=False, scale=255.0, filter=PNGE_ADAPTIVE):
    """dsn_png_filter: -> (raw uint8 [F, H (1 + row_bytes)], status int32 [F]) on the device"""
    F, H, W, ch, dt = _jpeg_images("png_filter", images)
    if (mode == PNGE_COLOUR) != (ch == 3) or mode not in (PNGE_GRAY, PNGE_COLOUR, PNGE_REPLICATE):
        raise ValueError(f"png_filter: mode {mode!r} does not fit images with {ch} channel(s)")
    dev = images.device
    raw = _output((F, H * (1 + W * (1 if mode == PNGE_GRAY else 3))), torch.uint8, dev)
    status = _output((F,), torch.int32, dev)
    with torch.cuda.device(dev):
        _check(lib().dsn_png_filter(_ptr(images) if F else None, dt, F, H, W, int(mode), int(bool(rgb)), float(scale), int(filter),
                                    _ptr(raw) if F else None, _ptr(status) if F else None, _stream()), "dsn_png_filter")
    return raw, status


def _pnge_raw(what, raw):
    if not torch.is_tensor(raw) or raw.dtype != torch.uint8 or raw.dim() != 2:
        raise ValueError(f"{what}: raw must be a uint8 tensor [F, n]")
    require_gpu()
    if not raw.is_cuda or not raw.is_contiguous():
        raise ValueError(f"{what}: raw must be a contiguous tensor on a ROCm device")
    return int(raw.shape[0]), int(raw.shape[1])


def png_adler(raw):
    """dsn_png_adler: raw uint8 [F, n] -> Adler-32 values int32 [F] (the bits of the uint32) on the device"""
    F, n = _pnge_raw("png_adler", raw)
    dev = raw.device
    out = _output((F,), torch.int32, dev)
    ws = _scratch(max(F, 1) * 8, dev)
    with torch.cuda.device(dev):
        _check(lib().dsn_png_adler(_ptr(raw) if F else None, F, n, _ptr(out) if F else None, _ptr(ws), int(ws.numel()), _stream()), "dsn_png_adler")
    return out


def png_deflate(raw, bpp, row_stride, chunk=None, stored_only=False, capacity=None, out=None):
    """dsn_png_deflate: raw uint8 [F, n] -> (out uint8 [F, capacity]: the deflate streams, lengths int32 [F], status int32 [F])"""
    F, n = _pnge_raw("png_deflate", raw)
    c = pnge_chunk(chunk)
    dev = raw.device
    if out is None:
        capacity = int(lib().dsn_png_deflate_max_bytes(n, c)) if capacity is None else int(capacity)
        out = _output((F, capacity), torch.uint8, dev)
    elif out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != F or not out.is_contiguous() or out.device != dev:
        raise ValueError("png_deflate: out must be a contiguous uint8 [F, capacity] tensor on raw's device")
    lengths = _output((F,), torch.int32, dev)
    status = _output((F,), torch.int32, dev)
    nws = lib().dsn_png_deflate_workspace_bytes(max(F, 1), n, c)
    if nws == 0:
        raise ValueError(f"png_deflate: {n} raw bytes per frame are outside what dsn_png_deflate takes (1 ... 2^30 + 2^15)")
    ws = _scratch(nws, dev)
    with torch.cuda.device(dev):
        _check(lib().dsn_png_deflate(_ptr(raw) if F else None, F, n, int(bpp), int(row_stride), c, int(bool(stored_only)),
                                     _ptr(out) if F else None, int(out.shape[1]), _ptr(lengths) if F else None, _ptr(status) if F else None,
                                     _ptr(ws), int(ws.numel()), _stream()), "dsn_png_deflate")
    return out, lengths, status


def huff_lengths(counts, limit):
    """dsn_huff_lengths: counts int32 [B, n] (non-negative) on the device -> code lengths uint8 [B, n]"""
    if not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 2:
        raise ValueError("huff_lengths: counts must be an int32 tensor [B, n]")
    require_gpu()
    if not counts.is_cuda or not counts.is_contiguous():
        raise ValueError("huff_lengths: counts must be a contiguous tensor on a ROCm device")
    B, n = int(counts.shape[0]), int(counts.shape[1])
    out = _output((B, n), torch.uint8, counts.device)
    with torch.cuda.device(counts.device):
        _check(lib().dsn_huff_lengths(_ptr(counts) if B else None, B, n, int(limit), _ptr(out) if B else None, _stream()), "dsn_huff_lengths")
    return out


def png_container(stream, lengths, adler, W, H, channels, status_in=None, capacity=None, out=None):
    """dsn_png_container: deflate streams uint8 [F, stride] with lengths int32 [F] and Adler-32 values int32 [F] -> (files uint8
    [F, capacity], lengths int32 [F], status int32 [F])"""
    F, stride = _pnge_raw("png_container", stream)
    dev = stream.device
    if out is None:
        capacity = 63 + stride if capacity is None else int(capacity)
        out = _output((F, capacity), torch.uint8, dev)
    out_lengths = _output((F,), torch.int32, dev)
    status = _output((F,), torch.int32, dev)
    ws = _scratch(max(F, 1) * 4, dev)
    with torch.cuda.device(dev):
        _check(lib().dsn_png_container(_ptr(stream) if F else None, stride, _ptr(lengths) if F else None, _ptr(adler) if F else None,
                                       _ptr(status_in) if (status_in is not None and F) else None, F, int(W), int(H), int(channels),
                                       _ptr(out) if F else None, int(out.shape[1]), _ptr(out_lengths) if F else None,
                                       _ptr(status) if F else None, _ptr(ws), int(ws.numel()), _stream()), "dsn_png_container")
    return out, out_lengths, status


def png_encode(images, mode, rgb=False, scale=255.0, filter=PNGE_ADAPTIVE, chunk=None, stored_only=False, capacity=None, out=None,
               workspace=None):
    """dsn_png_encode: images uint8 / float32 [F, H, W, 3] (PNGE_GRAY / PNGE_REPLICATE: [F, H, W]) on the device -> (out uint8
    [F, capacity] whose row f starts with frame f's complete file, lengths int32 [F]: the bytes each file needs, status int32 [F]: OR of
    PNGE_NONFINITE / PNGE_OVERFLOW).  Nothing is copied back and nothing waits."""
    F, H, W, ch, dt = _jpeg_images("png_encode", images)
    if (mode == PNGE_COLOUR) != (ch == 3) or mode not in (PNGE_GRAY, PNGE_COLOUR, PNGE_REPLICATE):
        raise ValueError(f"png_encode: mode {mode!r} does not fit images with {ch} channel(s)")
    c = pnge_chunk(chunk)
    dev = images.device
    if out is None:
        capacity = png_encode_max_bytes(W, H, 1 if mode == PNGE_GRAY else 3, c) if capacity is None else int(capacity)
        out = _output((F, capacity), torch.uint8, dev)
    elif out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != F or not out.is_contiguous() or out.device != dev:
        raise ValueError("png_encode: out must be a contiguous uint8 [F, capacity] tensor on the images' device")
    lengths = _output((F,), torch.int32, dev)
    status = _output((F,), torch.int32, dev)
    nws = lib().dsn_png_encode_workspace_bytes(max(F, 1), W, H, int(mode), c)
    if nws == 0:
        png_encode_max_bytes(W, H, 1 if mode == PNGE_GRAY else 3, c)          # raises with the limits
        raise ValueError(f"png_encode: F = {F} is above 16384")
    ws = _scratch(nws, dev) if workspace is None else workspace
    with torch.cuda.device(dev):
        _check(lib().dsn_png_encode(_ptr(images) if F else None, dt, F, H, W, int(mode), int(bool(rgb)), float(scale), int(filter), c,
                                    int(bool(stored_only)), _ptr(out) if F else None, int(out.shape[1]), _ptr(lengths) if F else None,
                                    _ptr(status) if F else None, _ptr(ws), int(ws.numel()), _stream()), "dsn_png_encode")
    return out, lengths, status
