// dsn_api.hip - the C ABI of libdsnerf_hip.so (include/dsnerf.h): argument checks, scene/workspace
// carving and kernel launches on the caller's stream.  No allocation, no synchronisation, no CPU
// fallback: every entry point only enqueues gfx950 kernels.
#include "../../include/dsnerf.h"
#include "dsn_common.h"
#include "dsn_kernels.h"
#include <climits>
#include <cmath>
#include <cstdlib>

#include <stdio.h>
#include <string.h>

static thread_local char g_err[512] = "";

static int dsn_fail(const char* fmt, const char* a = "", long long b = 0) {
    snprintf(g_err, sizeof(g_err), fmt, a, b);
    return 1;
}
static int dsn_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s: launch failed: %s", what, hipGetErrorString(e)); return 1; }
    return 0;
}
#define DSN_REQUIRE(cond, msg) do { if (!(cond)) return dsn_fail("%s", msg); } while (0)

thread_local int g_dsn_persistent_override = 0;
namespace {
struct DsnShareCus {      // DSN_SHARE_CUS for the duration of one dsn_render_rays call
    explicit DsnShareCus(bool on) {
        // (the persistent kernels take seven eighths of the compute units; other shares measured no different, docs/LAB_NOTEBOOK.md)
        if (on) { const int n = dsn_cu_count_raw(); g_dsn_persistent_override = std::max(8, (n * 7 / 8) / 8 * 8); }
    }
    ~DsnShareCus() { g_dsn_persistent_override = 0; }
};
}

struct DsnSceneHeader { int magic, V, F, has_body, has_frame; };
#define DSN_MAGIC 0x44534e31

extern "C" {

int dsn_abi_version(void) { return DSN_ABI_VERSION; }
const char* dsn_last_error(void) { return g_err; }

size_t dsn_packed_param_bytes(void) { return sizeof(float) * (size_t)OFF_END; }

int dsn_pack_params(const float* const* params33_host, void* packed, void* stream) {
    DSN_REQUIRE(params33_host && packed, "dsn_pack_params: null argument");
    for (int i = 0; i < DSN_NUM_PARAMS; ++i) DSN_REQUIRE(params33_host[i], "dsn_pack_params: null parameter pointer");
    dsn_launch_pack_params(params33_host, (float*)packed, (hipStream_t)stream);
    dsn_launch_set_screen_margin((float*)packed, DSN_SCREEN_MARGIN_DEFAULT, (hipStream_t)stream);   // until dsn_calibrate_screen has run
    dsn_launch_set_packed_scalar((float*)packed, 6, 1.0f, (hipStream_t)stream);      // colour scale of the early-stop threshold until measured
    return dsn_check_launch("dsn_pack_params");
}

// layout utility (no device work): the packed image of HOST parameter arrays, for tests / tooling
int dsn_pack_params_host_image(const float* const* params33_host, float* packed_host) {
    DSN_REQUIRE(params33_host && packed_host, "dsn_pack_params_host_image: null argument");
    dsn_pack_params_host(params33_host, packed_host);
    packed_host[OFF_SCAL + 5] = DSN_SCREEN_MARGIN_DEFAULT;
    packed_host[OFF_SCAL + 6] = 1.0f;
    return 0;
}

size_t dsn_scene_bytes(int V, int F) { return (V > 0 && F > 0) ? dsn_scene_size(V, F) : 0; }

int dsn_set_body(void* scene, const float* canon_vertex, const int32_t* faces, int V, int F, void* stream) {
    DSN_REQUIRE(scene && canon_vertex && faces && V > 0 && F > 0, "dsn_set_body: bad argument");
    hipStream_t st = (hipStream_t)stream;
    DsnSceneView s = dsn_scene_view(scene, V, F);
    DsnSceneHeader h = {DSN_MAGIC, V, F, 1, 0};
    // header lives in device memory too (sanity for later calls is done with the V/F the caller passes)
    if (hipMemcpyAsync(scene, &h, sizeof(h), hipMemcpyHostToDevice, st) != hipSuccess) return dsn_fail("%s", "dsn_set_body: header copy failed");
    if (hipMemcpyAsync(s.canon, canon_vertex, sizeof(float) * 3 * (size_t)V, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(s.faces, faces, sizeof(int32_t) * 3 * (size_t)F, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return dsn_fail("%s", "dsn_set_body: copy failed");
    dsn_launch_face_setup(s.canon, s.faces, F, s.face_canon, s.cent_canon, st);
    // canonical-space queries are x_c = face frame re-embedding with |h| <= 0.1 and uv in [-4,5]: wide pads
    // (fine level: pad 0.12 m - a non-transparent sample lies within |h| <= 0.1 m of its face, utils/render_utils.py:103-109, so its
    //  canonical point is inside; whatever is further out takes the coarse level / the sweep, same index)
    dsn_launch_build_nn(s.cent_canon, F, s.nn_canon, 0.12f, 0.7f, st, false, true);
    return dsn_check_launch("dsn_set_body");
}

int dsn_set_frame(void* scene, int V, int F, const void* packed, const float* xyz, const float* poses24x3, int frame_idx,
                  int zero_code, const float* light_shift3, const float* rot2x2, const float* rot_center2,
                  void* stream) {
    return dsn_set_frame_ex(scene, V, F, packed, xyz, poses24x3, frame_idx, zero_code, light_shift3, rot2x2, rot_center2, 0, stream);
}

int dsn_set_frame_ex(void* scene, int V, int F, const void* packed, const float* xyz, const float* poses24x3, int frame_idx,
                     int zero_code, const float* light_shift3, const float* rot2x2, const float* rot_center2, int flags,
                     void* stream) {
    DSN_REQUIRE(scene && packed && xyz && poses24x3, "dsn_set_frame_ex: null argument");
    DSN_REQUIRE(V > 0 && F > 0, "dsn_set_frame_ex: bad V/F");
    DSN_REQUIRE(frame_idx >= 0 && frame_idx < 500, "dsn_set_frame_ex: frame index outside the embedding table (maxFrame=500)");
    hipStream_t st = (hipStream_t)stream;
    DsnSceneView s = dsn_scene_view(scene, V, F);
    if (hipMemcpyAsync(s.xyz, xyz, sizeof(float) * 3 * (size_t)V, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return dsn_fail("%s", "dsn_set_frame_ex: copy failed");
    dsn_launch_face_setup(s.xyz, s.faces, F, s.face_world, s.cent_world, st);
    // world-space queries lie inside the (padded) body AABB the rays were clipped to; coarse level beyond
    dsn_launch_build_nn(s.cent_world, F, s.nn_world, 0.12f, 0.7f, st, (flags & DSN_FRAME_FINE_ONLY) != 0, false,
                        (flags & DSN_FRAME_LAZY_LISTS) != 0);
    dsn_launch_pose_setup((const float*)packed, poses24x3, frame_idx, zero_code, light_shift3, rot2x2, rot_center2,
                          s.frame, st);
    return dsn_check_launch("dsn_set_frame_ex");
}

size_t dsn_pose_state_bytes(void) { return dsn_pose_state_size(); }

int dsn_set_pose(void* scene_or_pose_state, const void* packed, const float* poses24x3, const float* pose_feat16, int frame_idx,
                 int zero_code, const float* light_shift3, const float* rot2x2, const float* rot_center2, void* stream) {
    DSN_REQUIRE(scene_or_pose_state && packed, "dsn_set_pose: null argument");
    DSN_REQUIRE(poses24x3 || pose_feat16, "dsn_set_pose: give poses (batch['poses'], pose_mlp is applied) or the 16 pose features");
    DSN_REQUIRE(frame_idx >= 0 && frame_idx < 500, "dsn_set_pose: frame index outside the embedding table (maxFrame=500)");
    // the per-frame state sits at the same offset in a scene blob and in a pose-only blob (dsn_common.h dsn_scene_view)
    DsnFrameState* fs = (DsnFrameState*)((char*)scene_or_pose_state + 256);
    dsn_launch_pose_setup((const float*)packed, poses24x3, frame_idx, zero_code, light_shift3, rot2x2, rot_center2, fs,
                          (hipStream_t)stream, pose_feat16);
    return dsn_check_launch("dsn_set_pose");
}

int dsn_sample_gg(const void* scene, int V, int F, const float* ray_o, const float* ray_d, float* near, float* far, int R, int S,
                  const float* t_vals, const float* jitter, float* z_vals, float* pts, void* stream) {
    DSN_REQUIRE(scene && ray_o && ray_d && near && far && t_vals && z_vals, "dsn_sample_gg: null argument");
    DSN_REQUIRE(R > 0 && S > 0, "dsn_sample_gg: empty ray batch");
    DSN_REQUIRE(V > 0 && F > 0, "dsn_sample_gg: bad V/F");
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    dsn_launch_sample_gg(s.xyz, V, ray_o, ray_d, near, far, R, S, t_vals, jitter, z_vals, pts, (hipStream_t)stream);
    return dsn_check_launch("dsn_sample_gg");
}

// utils/pts_utils.py:3-16 uniform_sampling alone (sample_points_mode == "uniform", can_render.py:42-51)
int dsn_sample_uniform(const void* scene, int V, int F, const float* ray_o, const float* ray_d, float* near, float* far,
                       int R, int S, const float* t_vals, const float* jitter, float* z_vals, float* pts, void* stream) {
    DSN_REQUIRE(ray_o && ray_d && near && far && t_vals && z_vals, "dsn_sample_uniform: null argument");
    DSN_REQUIRE(R > 0 && S > 0, "dsn_sample_uniform: empty ray batch");
    (void)scene; (void)V; (void)F;
    dsn_launch_sample_gg(nullptr, 0, ray_o, ray_d, near, far, R, S, t_vals, jitter, z_vals, pts, (hipStream_t)stream);
    return dsn_check_launch("dsn_sample_uniform");
}

int dsn_warp(const void* scene, int V, int F, const float* pts, const float* ray_d, int64_t N, int S, int32_t* face_idx, float* uv,
             float* h, uint8_t* transparent, float* x_c, float* ray_d_can, int32_t* active_list,
             int32_t* active_count, int flags, void* stream) {
    DSN_REQUIRE(scene && pts, "dsn_warp: null argument");
    DSN_REQUIRE(N > 0 && S > 0, "dsn_warp: empty point batch");
    DSN_REQUIRE((active_list == nullptr) == (active_count == nullptr), "dsn_warp: active_list and active_count go together");
    DSN_REQUIRE(V > 0 && F > 0, "dsn_warp: bad V/F");
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    dsn_launch_warp(s, pts, nullptr, ray_d, nullptr, N, S, face_idx, uv, h, transparent, x_c, ray_d_can, active_list,
                    active_count, (flags & DSN_NN_EXHAUSTIVE) != 0, (hipStream_t)stream);
    return dsn_check_launch("dsn_warp");
}

int dsn_lbs_warp(const void* scene, int V, int F, const float* pts, int64_t N, const float* smpl_weights,
                 const float* joint_transforms, int bw_type, int32_t* face_idx, float* weights, uint8_t* transparent,
                 float* pts_zero, int flags, void* stream) {
    DSN_REQUIRE(scene && pts && smpl_weights && joint_transforms, "dsn_lbs_warp: null argument");
    DSN_REQUIRE(N > 0 && V > 0 && F > 0, "dsn_lbs_warp: bad sizes");
    DSN_REQUIRE(bw_type == 0 || bw_type == 1, "dsn_lbs_warp: unsupport value: bw_type");   // the reference raises ValueError
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    dsn_launch_lbs_warp(s, pts, N, smpl_weights, joint_transforms, bw_type, face_idx, weights, transparent, pts_zero,
                        (flags & DSN_NN_EXHAUSTIVE) != 0, (hipStream_t)stream);
    return dsn_check_launch("dsn_lbs_warp");
}

int dsn_field(const void* scene, int V, int F, const void* packed, const float* x_c, int64_t N, const int32_t* active_list,
              const int32_t* active_count, float* sigma, float* essence, float* grad, int flags, void* stream) {
    DSN_REQUIRE(scene && packed && x_c && sigma, "dsn_field: null argument");
    DSN_REQUIRE(N > 0, "dsn_field: empty point batch");
    DSN_REQUIRE((active_list == nullptr) == (active_count == nullptr), "dsn_field: active_list and active_count go together");
    DSN_REQUIRE((V > 0 && F > 0) || (V == 0 && F == 0), "dsn_field: bad V/F (0/0 = pose-only state of dsn_pose_state_bytes())");
    DsnSceneView s = dsn_scene_view((void*)scene, V > 0 ? V : 1, F > 0 ? F : 1);     // only s.frame is used (fixed offset)
    // split-fp16 kernel for the full evaluation; the exact-fp32 kernel serves density-only / colour-only queries
    if (!(flags & DSN_FIELD_FP32) && essence && grad) {
        dsn_launch_field16((const float*)packed, s.frame, x_c, N, active_list, active_count, sigma, essence, grad,
                           (hipStream_t)stream);
        // range fallback: samples the split-fp16 kernel flagged (sigma = NaN) are re-evaluated in exact fp32
        dsn_launch_field_fix((const float*)packed, s.frame, x_c, N, active_list, active_count, sigma, essence, grad,
                             (hipStream_t)stream);
    } else
        dsn_launch_field((const float*)packed, s.frame, x_c, N, active_list, active_count, sigma, essence, grad,
                         (hipStream_t)stream);
    return dsn_check_launch("dsn_field");
}

size_t dsn_field_record_bytes(int64_t N) { return N > 0 ? dsn_align256(224 * (size_t)N) : 0; }

int dsn_field_forward(const void* scene, int V, int F, const void* packed, const float* x_c, int64_t N,
                      const int32_t* active_list, const int32_t* active_count, float* sigma, float* essence, void* records,
                      int32_t* pos_list, int32_t* pos_count, void* stream) {
    DSN_REQUIRE(scene && packed && x_c && sigma && essence && records && pos_list && pos_count, "dsn_field_forward: null argument");
    DSN_REQUIRE(N > 0, "dsn_field_forward: empty point batch");
    DSN_REQUIRE((active_list == nullptr) == (active_count == nullptr), "dsn_field_forward: active_list and active_count go together");
    DSN_REQUIRE(V > 0 && F > 0, "dsn_field_forward: bad V/F");
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    dsn_launch_field16_fwd((const float*)packed, s.frame, x_c, N, active_list, active_count, sigma, essence, records, pos_list,
                           pos_count, (hipStream_t)stream, N);
    return dsn_check_launch("dsn_field_forward");
}

int dsn_field_reverse(const void* scene, int V, int F, const void* packed, const float* x_c, int64_t N, const int32_t* pos_list,
                      const int32_t* pos_count, const void* records, float* grad, float* sigma, float* essence, void* stream) {
    DSN_REQUIRE(scene && packed && x_c && pos_list && pos_count && records && grad && sigma && essence, "dsn_field_reverse: null argument");
    DSN_REQUIRE(N > 0, "dsn_field_reverse: empty point batch");
    DSN_REQUIRE(V > 0 && F > 0, "dsn_field_reverse: bad V/F");
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    dsn_launch_field16_bwd((const float*)packed, s.frame, x_c, N, pos_list, pos_count, grad, records, (hipStream_t)stream, sigma, N);
    // range fallback for what dsn_field_forward or the reverse pass flagged (sigma = NaN): exact fp32, all three outputs
    dsn_launch_field_fix((const float*)packed, s.frame, x_c, N, pos_list, pos_count, sigma, essence, grad, (hipStream_t)stream);
    return dsn_check_launch("dsn_field_reverse");
}

// model/spacenet.py:174-188 LightingMLP.forward as a pure function of its four arguments
int dsn_light(const void* packed, const float* normal, const float* xyz_world, const float* view_dir_world,
              const float* essence, int64_t N, float* colour, void* zero_pose_state, int flags, void* stream) {
    DSN_REQUIRE(packed && normal && xyz_world && view_dir_world && essence && colour && zero_pose_state, "dsn_light: null argument");
    DSN_REQUIRE(N > 0, "dsn_light: empty point batch");
    hipStream_t st = (hipStream_t)stream;
    // the lighting kernels read the light-centre / rotation edits from a frame state; those belong to DualSpaceNeRF.forward
    // (:254-263), not to this function: run on a zeroed state
    if (hipMemsetAsync(zero_pose_state, 0, dsn_pose_state_size(), st) != hipSuccess) return dsn_fail("%s", "dsn_light: memset failed");
    const DsnFrameState* fs = (const DsnFrameState*)((const char*)zero_pose_state + 256);
    if (flags & DSN_FIELD_FP32)
        dsn_launch_light((const float*)packed, fs, normal, xyz_world, nullptr, view_dir_world, nullptr, essence, N, 1, nullptr, nullptr,
                         colour, st);
    else
        dsn_launch_light16((const float*)packed, fs, normal, xyz_world, nullptr, view_dir_world, nullptr, essence, N, 1, nullptr,
                           nullptr, colour, st);
    return dsn_check_launch("dsn_light");
}

size_t dsn_calibrate_workspace_bytes(int64_t n_points) { return n_points > 0 ? dsn_calibrate_workspace_size(n_points) : 0; }

int dsn_calibrate_screen(const void* scene, int V, int F, void* packed, int64_t n_points, void* workspace, float* out4, void* stream) {
    DSN_REQUIRE(scene && packed && workspace, "dsn_calibrate_screen: null argument");
    DSN_REQUIRE(V > 0 && F > 0 && n_points > 0, "dsn_calibrate_screen: bad sizes");
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    dsn_launch_calibrate_screen(s, (float*)packed, n_points, workspace, out4, (hipStream_t)stream);
    return dsn_check_launch("dsn_calibrate_screen");
}

int dsn_set_screen_margin(void* packed, float margin, void* stream) {
    DSN_REQUIRE(packed, "dsn_set_screen_margin: null argument");
    DSN_REQUIRE(margin == margin, "dsn_set_screen_margin: NaN margin");     // (+inf = keep every sample; <= 0 is unsafe, tests only)
    dsn_launch_set_screen_margin((float*)packed, margin, (hipStream_t)stream);
    return dsn_check_launch("dsn_set_screen_margin");
}

int dsn_set_early_stop_colour_scale(void* packed, float colour_scale, void* stream) {
    DSN_REQUIRE(packed, "dsn_set_early_stop_colour_scale: null argument");
    DSN_REQUIRE(colour_scale == colour_scale, "dsn_set_early_stop_colour_scale: NaN scale");
    dsn_launch_set_packed_scalar((float*)packed, 6, colour_scale, (hipStream_t)stream);
    return dsn_check_launch("dsn_set_early_stop_colour_scale");
}

int dsn_shade(const void* scene, int V, int F, const void* packed, const float* x_c, const float* grad, const float* x_w,
              const float* ray_d, const float* essence, int64_t N, int S, const int32_t* active_list,
              const int32_t* active_count, int32_t* face_idx_canon, float* n_w, float* colour, int flags, void* stream) {
    DSN_REQUIRE(scene && packed && x_c && grad && x_w && ray_d && essence && n_w && colour, "dsn_shade: null argument");
    DSN_REQUIRE(N > 0 && S > 0, "dsn_shade: empty point batch");
    DSN_REQUIRE((active_list == nullptr) == (active_count == nullptr), "dsn_shade: active_list and active_count go together");
    DSN_REQUIRE(V > 0 && F > 0, "dsn_shade: bad V/F");
    hipStream_t st = (hipStream_t)stream;
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    dsn_launch_normal(s, x_c, grad, N, active_list, active_count, face_idx_canon, n_w, (flags & DSN_NN_EXHAUSTIVE) != 0, st);
    if (flags & DSN_FIELD_FP32)
        dsn_launch_light((const float*)packed, s.frame, n_w, x_w, nullptr, ray_d, nullptr, essence, N, S, active_list,
                         active_count, colour, st);
    else
        dsn_launch_light16((const float*)packed, s.frame, n_w, x_w, nullptr, ray_d, nullptr, essence, N, S, active_list,
                           active_count, colour, st);
    return dsn_check_launch("dsn_shade");
}

int dsn_shade_factor(const void* scene, int V, int F, const void* packed, const float* x_c, const float* grad, const float* x_w,
                     const float* ray_d, const float* essence, int64_t N, int S, const int32_t* active_list,
                     const int32_t* active_count, int32_t* face_idx_canon, float* n_w, float* colour, float* factor, int flags,
                     void* stream) {
    DSN_REQUIRE(scene && packed && x_c && grad && x_w && ray_d && essence && n_w && colour && factor, "dsn_shade_factor: null argument");
    DSN_REQUIRE(N > 0 && S > 0, "dsn_shade_factor: empty point batch");
    DSN_REQUIRE((active_list == nullptr) == (active_count == nullptr), "dsn_shade_factor: active_list and active_count go together");
    DSN_REQUIRE(V > 0 && F > 0, "dsn_shade_factor: bad V/F");
    DSN_REQUIRE(!(flags & DSN_FIELD_FP32), "dsn_shade_factor: DSN_FIELD_FP32 is not supported (split-fp16 lighting only)");
    hipStream_t st = (hipStream_t)stream;
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    dsn_launch_normal(s, x_c, grad, N, active_list, active_count, face_idx_canon, n_w, (flags & DSN_NN_EXHAUSTIVE) != 0, st);
    dsn_launch_light16((const float*)packed, s.frame, n_w, x_w, nullptr, ray_d, nullptr, essence, N, S, active_list, active_count, colour, st,
                       nullptr, nullptr, nullptr, nullptr, factor);
    return dsn_check_launch("dsn_shade_factor");
}

int dsn_composite_maps(const float* essence, const float* n_w, const float* factor, const float* sigma, const uint8_t* transparent,
                       const float* z_vals, const float* ray_d, int R, int S, float* albedo_map, float* normal_map, float* shading_map,
                       float* weights, float* out_max, void* stream) {
    DSN_REQUIRE(sigma && z_vals && ray_d, "dsn_composite_maps: null argument");
    DSN_REQUIRE(R > 0 && S > 0, "dsn_composite_maps: empty ray batch");
    DSN_REQUIRE(albedo_map || normal_map || shading_map || weights || out_max, "dsn_composite_maps: no output asked for");
    DSN_REQUIRE((!albedo_map || essence) && (!normal_map || n_w) && (!shading_map || factor),
                "dsn_composite_maps: map requested without its source (albedo: essence, normal: n_w, shading: factor)");
    DSN_REQUIRE(!out_max || (essence && factor), "dsn_composite_maps: out_max needs essence and factor");
    hipStream_t st = (hipStream_t)stream;
    if (out_max && hipMemsetAsync(out_max, 0, 2 * sizeof(float), st) != hipSuccess)
        return dsn_fail("%s", "dsn_composite_maps: memset failed");
    DsnMapsArgs a = {};
    a.factors = factor; a.n_shaded = (int64_t)R * S; a.G = 1;
    a.essence = essence; a.n_w = n_w; a.sigma = sigma; a.transparent = transparent; a.z_vals = z_vals; a.ray_d = ray_d;
    a.R = R; a.S = S;
    a.albedo_map = albedo_map; a.normal_map = normal_map; a.shading_maps = shading_map; a.weights = weights;
    a.maps_max = (int32_t*)out_max;
    dsn_launch_composite_maps(a, st);
    return dsn_check_launch("dsn_composite_maps");
}

int dsn_composite(const float* colour, const float* sigma, const uint8_t* transparent, const float* z_vals,
                  const float* ray_d, const float* noise, int R, int S, float* rgb_map, float* disp_map,
                  float* acc_map, float* weights, float* depth_map, void* stream) {
    DSN_REQUIRE(colour && sigma && z_vals && ray_d && rgb_map && disp_map && acc_map && depth_map, "dsn_composite: null argument");
    DSN_REQUIRE(R > 0 && S > 0, "dsn_composite: empty ray batch");
    dsn_launch_composite(colour, sigma, transparent, z_vals, ray_d, noise, R, S, rgb_map, disp_map, acc_map, weights,
                         depth_map, (hipStream_t)stream);
    return dsn_check_launch("dsn_composite");
}

size_t dsn_image_workspace_bytes(int H, int W) { return (H > 0 && W > 0) ? dsn_image_workspace_size(H, W) : 0; }

int dsn_image_scatter(const float* rgb, const float* disp, const float* acc, const float* depth, int R, const uint8_t* mask_at_box,
                      int H, int W, int clamp_rgb, float* img_rgb, float* img_disp, float* img_acc, float* img_depth,
                      void* workspace, void* stream) {
    DSN_REQUIRE((rgb || R == 0) && mask_at_box && img_rgb && workspace, "dsn_image_scatter: null argument");
    DSN_REQUIRE(H > 0 && W > 0 && R >= 0, "dsn_image_scatter: bad sizes");
    DSN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "dsn_image_scatter: image too large");
    DSN_REQUIRE(R == 0 || ((!img_disp || disp) && (!img_acc || acc) && (!img_depth || depth)), "dsn_image_scatter: image requested without its source");
    dsn_launch_image_scatter(rgb, disp, acc, depth, R, mask_at_box, H, W, clamp_rgb, img_rgb, img_disp, img_acc, img_depth,
                             workspace, (hipStream_t)stream);
    return dsn_check_launch("dsn_image_scatter");
}

int dsn_image_psnr(const float* img_rgb, const double* gt_f64, const float* gt_f32, const uint8_t* mask_at_box, int H, int W,
                   double* out4, void* workspace, void* stream) {
    DSN_REQUIRE(img_rgb && out4 && workspace, "dsn_image_psnr: null argument");
    DSN_REQUIRE((gt_f64 != nullptr) != (gt_f32 != nullptr), "dsn_image_psnr: exactly one ground-truth pointer");
    DSN_REQUIRE(H > 0 && W > 0, "dsn_image_psnr: bad sizes");
    dsn_launch_image_psnr(img_rgb, gt_f64, gt_f32, mask_at_box, H, W, out4, workspace, (hipStream_t)stream);
    return dsn_check_launch("dsn_image_psnr");
}

static bool dsn_ssim_sizes_ok(int F, int H, int W) {
    return F > 0 && H > 0 && W > 0 && F <= 65535 && H <= 65535 && W <= 65535 && (int64_t)H * W < ((int64_t)1 << 31);
}

size_t dsn_image_ssim_workspace_bytes(int F, int H, int W) { return dsn_ssim_sizes_ok(F, H, W) ? dsn_image_ssim_workspace_size(F, H, W) : 0; }

int dsn_image_ssim(const float* img_rgb, const double* gt_f64, const float* gt_f32, const uint8_t* mask_at_box, int F, int H, int W,
                   int clamp_rgb, double* out_ssim, int32_t* out_rect, int32_t* out_status, void* workspace, void* stream) {
    DSN_REQUIRE(img_rgb && mask_at_box && out_ssim && out_rect && out_status && workspace, "dsn_image_ssim: null argument");
    DSN_REQUIRE((gt_f64 != nullptr) != (gt_f32 != nullptr), "dsn_image_ssim: exactly one ground-truth pointer");
    DSN_REQUIRE(dsn_ssim_sizes_ok(F, H, W), "dsn_image_ssim: bad sizes");
    dsn_launch_image_ssim(img_rgb, gt_f64, gt_f32, mask_at_box, F, H, W, clamp_rgb, out_ssim, out_rect, out_status, workspace,
                          (hipStream_t)stream);
    return dsn_check_launch("dsn_image_ssim");
}

// the trainer's loss (dsn_loss.hip).  R = 0 is a valid call: nothing is read, the means are NaN (the per-ray pointers may be null then)
#define DSN_LOSS_MAX_RAYS (((int64_t)1 << 31) - 1)
static bool dsn_loss_rays_ok(int64_t R) { return R >= 0 && R <= DSN_LOSS_MAX_RAYS; }

size_t dsn_train_loss_workspace_bytes(int64_t R) { return dsn_loss_rays_ok(R) ? dsn_train_loss_workspace_size(R) : 0; }

int dsn_train_loss(const float* color, const float* target_f32, const double* target_f64, float* acc, const uint8_t* occ_u8,
                   const float* occ_f32, int64_t R, int kind, int acc_overwrite, double* out4, void* workspace, void* stream) {
    DSN_REQUIRE(dsn_loss_rays_ok(R), "dsn_train_loss: R must be 0 ... 2^31 - 1");
    DSN_REQUIRE(kind == DSN_LOSS_L2 || kind == DSN_LOSS_SMOOTH_L1, "dsn_train_loss: unknown kind");
    DSN_REQUIRE(out4, "dsn_train_loss: null argument");
    DSN_REQUIRE(!(target_f32 && target_f64), "dsn_train_loss: exactly one target pointer");
    DSN_REQUIRE(!(occ_u8 && occ_f32), "dsn_train_loss: at most one occupancy pointer");
    if (R > 0) {
        DSN_REQUIRE(color && workspace, "dsn_train_loss: null argument");
        DSN_REQUIRE(target_f32 || target_f64, "dsn_train_loss: exactly one target pointer");
        DSN_REQUIRE(!(occ_u8 || occ_f32) || acc, "dsn_train_loss: the mask term needs acc");
    }
    dsn_launch_train_loss(color, target_f32, target_f64, acc, occ_u8, occ_f32, R, kind, acc_overwrite, out4, workspace, (hipStream_t)stream);
    return dsn_check_launch("dsn_train_loss");
}

int dsn_train_loss_grad(const float* color, const float* target_f32, const double* target_f64, const float* acc, const uint8_t* occ_u8,
                        const float* occ_f32, int64_t R, int kind, const float* up_rgb, const float* up_mask, float* g_color, float* g_acc,
                        void* stream) {
    DSN_REQUIRE(dsn_loss_rays_ok(R), "dsn_train_loss_grad: R must be 0 ... 2^31 - 1");
    DSN_REQUIRE(kind == DSN_LOSS_L2 || kind == DSN_LOSS_SMOOTH_L1, "dsn_train_loss_grad: unknown kind");
    DSN_REQUIRE(!(target_f32 && target_f64), "dsn_train_loss_grad: exactly one target pointer");
    DSN_REQUIRE(!(occ_u8 && occ_f32), "dsn_train_loss_grad: at most one occupancy pointer");
    if (R > 0) {
        DSN_REQUIRE(color && g_color, "dsn_train_loss_grad: null argument");
        DSN_REQUIRE(target_f32 || target_f64, "dsn_train_loss_grad: exactly one target pointer");
        DSN_REQUIRE(!(occ_u8 || occ_f32) || acc, "dsn_train_loss_grad: the mask term needs acc");
    }
    dsn_launch_train_loss_grad(color, target_f32, target_f64, acc, occ_u8, occ_f32, R, kind, up_rgb, up_mask, g_color, g_acc,
                               (hipStream_t)stream);
    return dsn_check_launch("dsn_train_loss_grad");
}

static bool dsn_adam_scalars_ok(double beta1, double beta2, double eps, double t) {
    return beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && std::isfinite(eps) && eps >= 0.0 && std::isfinite(t) && t >= 1.0;
}

int dsn_adam_scalars_host(double lr, double weight_decay, double beta1, double beta2, double eps, double t, float* out7_host) {
    DSN_REQUIRE(out7_host, "dsn_adam_scalars_host: null argument");
    DSN_REQUIRE(dsn_adam_scalars_ok(beta1, beta2, eps, t), "dsn_adam_scalars_host: betas must lie in [0, 1), eps be finite and >= 0, t be finite and >= 1");
    DSN_REQUIRE(std::isfinite(lr) && lr >= 0.0 && std::isfinite(weight_decay) && weight_decay >= 0.0,
                "dsn_adam_scalars_host: lr and weight_decay must be finite and >= 0");
    dsn_adam_scalars(lr, weight_decay, beta1, beta2, eps, t, out7_host);
    return 0;
}

int dsn_adam_step(float* const* params_host, const float* const* grads_host, float* const* exp_avgs_host, float* const* exp_avg_sqs_host,
                  const int64_t* n_host, int count, const double* lr_host, const double* weight_decay_host, double beta1, double beta2,
                  double eps, double t, void* packed, void* stream) {
    DSN_REQUIRE(count >= 0, "dsn_adam_step: count must not be negative");
    DSN_REQUIRE(count == 0 || (params_host && grads_host && exp_avgs_host && exp_avg_sqs_host && n_host && lr_host && weight_decay_host),
                "dsn_adam_step: null argument");
    DSN_REQUIRE(dsn_adam_scalars_ok(beta1, beta2, eps, t), "dsn_adam_step: betas must lie in [0, 1), eps be finite and >= 0, t be finite and >= 1");
    for (int i = 0; i < count; ++i) {
        DSN_REQUIRE(n_host[i] >= 0 && n_host[i] <= DSN_ADAM_MAX_N, "dsn_adam_step: a length must be 0 ... 2^33");
        DSN_REQUIRE(std::isfinite(lr_host[i]) && lr_host[i] >= 0.0 && std::isfinite(weight_decay_host[i]) && weight_decay_host[i] >= 0.0,
                    "dsn_adam_step: lr and weight_decay must be finite and >= 0");
        if (grads_host[i] && n_host[i] > 0)
            DSN_REQUIRE(params_host[i] && exp_avgs_host[i] && exp_avg_sqs_host[i], "dsn_adam_step: null tensor pointer");
    }
    if (packed) {
        DSN_REQUIRE(count == DSN_NUM_PARAMS, "dsn_adam_step: packed needs the model's 33 tensors");
        for (int i = 0; i < DSN_NUM_PARAMS; ++i)
            DSN_REQUIRE(params_host[i] && n_host[i] == DSN_PARAM_COUNT[i], "dsn_adam_step: packed needs the model's 33 tensors (a null parameter or another length)");
    }
    hipStream_t st = (hipStream_t)stream;
    dsn_launch_adam_step(params_host, grads_host, exp_avgs_host, exp_avg_sqs_host, n_host, count, lr_host, weight_decay_host, beta1, beta2,
                         eps, t, st);
    if (packed) {       // what dsn_pack_params enqueues, behind the update
        dsn_launch_pack_params(params_host, (float*)packed, st);
        dsn_launch_set_screen_margin((float*)packed, DSN_SCREEN_MARGIN_DEFAULT, st);
        dsn_launch_set_packed_scalar((float*)packed, 6, 1.0f, st);
    }
    return dsn_check_launch("dsn_adam_step");
}

int dsn_train_draws(uint64_t seed, uint32_t step, uint32_t ray_base, const int32_t* ray_ids, int R, int S, float noise_std, float* jitter,
                    float* noise, void* stream) {
    DSN_REQUIRE(R >= 0 && S >= 0, "dsn_train_draws: R and S must not be negative");
    DSN_REQUIRE((int64_t)R * S <= (int64_t)INT_MAX, "dsn_train_draws: R * S must not exceed INT_MAX");
    DSN_REQUIRE((((uintptr_t)ray_ids | (uintptr_t)jitter | (uintptr_t)noise) & 3) == 0, "dsn_train_draws: a pointer is not 4-byte aligned");
    if (R == 0 || S == 0) return 0;
    DSN_REQUIRE(jitter || noise, "dsn_train_draws: jitter and noise are both null");
    dsn_launch_train_draws(seed, step, ray_base, ray_ids, R, S, noise_std, jitter, noise, (hipStream_t)stream);
    return dsn_check_launch("dsn_train_draws");
}

int dsn_field_screen(const void* scene, int V, int F, const void* packed, const float* x_c, int64_t N, const int32_t* active_list,
                     const int32_t* active_count, float* sigma, int32_t* keep_list, int32_t* keep_count, void* stream) {
    DSN_REQUIRE(scene && packed && x_c && sigma && keep_list && keep_count, "dsn_field_screen: null argument");
    DSN_REQUIRE(N > 0 && V > 0 && F > 0, "dsn_field_screen: bad sizes");
    DSN_REQUIRE((active_list == nullptr) == (active_count == nullptr), "dsn_field_screen: active_list and active_count go together");
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    dsn_launch_screen16((const float*)packed, s.frame, x_c, N, active_list, active_count, sigma, keep_list, keep_count, nullptr,
                        nullptr, (hipStream_t)stream);
    return dsn_check_launch("dsn_field_screen");
}

int dsn_debug_screen(const void* scene, int V, int F, const void* packed, const float* x_c, int64_t N, float* sigma_screen,
                     float* s1, int32_t* scratch_list, int32_t* scratch_count, void* stream) {
    DSN_REQUIRE(scene && packed && x_c && sigma_screen && s1 && scratch_list && scratch_count, "dsn_debug_screen: null argument");
    DSN_REQUIRE(N > 0 && V > 0 && F > 0, "dsn_debug_screen: bad sizes");
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    if (hipMemsetAsync(scratch_count, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return dsn_fail("%s", "dsn_debug_screen: memset failed");
    dsn_launch_screen16((const float*)packed, s.frame, x_c, N, nullptr, nullptr, sigma_screen, scratch_list, scratch_count,
                        sigma_screen, s1, (hipStream_t)stream);
    return dsn_check_launch("dsn_debug_screen");
}

size_t dsn_grad_workspace_bytes(int R, int S) { return (R > 0 && S > 0) ? dsn_train_workspace_size((int64_t)R * S) : 0; }

// read-only view of the training workspace for tests and diagnostics (host function): see dsnerf.h
int dsn_grad_workspace_layout(int R, int S, int64_t* out_offsets_host, int n) {
    DSN_REQUIRE(out_offsets_host && R > 0 && S > 0, "dsn_grad_workspace_layout: bad argument");
    DSN_REQUIRE(dsn_train_workspace_layout((int64_t)R * S, out_offsets_host, n) == 0,
                "dsn_grad_workspace_layout: n is not DSN_GRAD_WS_COUNT");
    return 0;
}

int dsn_render_rays_grad(const void* scene, int V, int F, const void* packed, const float* const* params33_host, const float* poses24x3,
                         int frame_idx, int zero_code, const float* ray_o, const float* ray_d, const float* z_vals,
                         const float* noise, int R, int S, const float* d_rgb, const float* d_disp, const float* d_acc,
                         const float* d_depth, const float* d_weights, float* const* grads33_host, void* workspace,
                         int flags, void* stream) {
    return dsn_render_rays_grad_ex(scene, V, F, packed, params33_host, poses24x3, frame_idx, zero_code, ray_o, ray_d, z_vals, noise, R, S, d_rgb,
                                   d_disp, d_acc, d_depth, d_weights, grads33_host, workspace, flags, stream, nullptr, nullptr, nullptr);
}

int dsn_render_rays_grad_ex(const void* scene, int V, int F, const void* packed, const float* const* params33_host, const float* poses24x3,
                            int frame_idx, int zero_code, const float* ray_o, const float* ray_d, const float* z_vals,
                            const float* noise, int R, int S, const float* d_rgb, const float* d_disp, const float* d_acc,
                            const float* d_depth, const float* d_weights, float* const* grads33_host, void* workspace,
                            int flags, void* stream, void* aux_stream, void* ev_fork, void* ev_join) {
    DSN_REQUIRE(scene && packed && params33_host && poses24x3 && ray_o && ray_d && z_vals && d_rgb && grads33_host && workspace,
                "dsn_render_rays_grad: null argument");
    DSN_REQUIRE(R > 0 && S > 0 && V > 0 && F > 0, "dsn_render_rays_grad: bad sizes");
    DSN_REQUIRE(frame_idx >= 0 && frame_idx < 500, "dsn_render_rays_grad: frame index outside the embedding table");
    DSN_REQUIRE((aux_stream != nullptr) == (ev_fork != nullptr) && (aux_stream != nullptr) == (ev_join != nullptr),
                "dsn_render_rays_grad_ex: the auxiliary stream and its two events go together");
    DSN_REQUIRE(!aux_stream || aux_stream != stream, "dsn_render_rays_grad_ex: the auxiliary stream must not be the call's own stream");
    for (int i = 0; i < DSN_NUM_PARAMS; ++i)
        DSN_REQUIRE(params33_host[i] && grads33_host[i], "dsn_render_rays_grad: null parameter / gradient pointer");
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    const DsnTrainAux aux = {(hipStream_t)aux_stream, (hipEvent_t)ev_fork, (hipEvent_t)ev_join};
    const char* err = dsn_train_run(s, (const float*)packed, params33_host, poses24x3, frame_idx, zero_code, ray_o, ray_d, z_vals, noise, R, S, d_rgb,
                                    d_disp, d_acc, d_depth, d_weights, grads33_host, workspace, (hipStream_t)stream,
                                    (flags & DSN_GRAD_CACHED) != 0, nullptr, nullptr, nullptr, aux_stream ? &aux : nullptr);
    if (err) return dsn_fail("dsn_render_rays_grad: %s failed", err);
    return dsn_check_launch("dsn_render_rays_grad");
}

// the caller's auxiliary stream + fork / join events of dsn_render_rays_grad_ex, for callers without a HIP binding of their own
// (created and destroyed by the caller through these two; the library keeps no record of them)
int dsn_aux_create(void** aux_stream, void** ev_fork, void** ev_join) {
    DSN_REQUIRE(aux_stream && ev_fork && ev_join, "dsn_aux_create: null argument");
    hipStream_t st = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&a, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&b, hipEventDisableTiming) != hipSuccess) {
        if (st) (void)hipStreamDestroy(st);
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
        return dsn_fail("%s", "dsn_aux_create: hipStreamCreate / hipEventCreate failed");
    }
    *aux_stream = (void*)st; *ev_fork = (void*)a; *ev_join = (void*)b;
    return 0;
}
int dsn_aux_destroy(void* aux_stream, void* ev_fork, void* ev_join) {
    int bad = 0;
    if (aux_stream) bad |= hipStreamDestroy((hipStream_t)aux_stream) != hipSuccess;
    if (ev_fork) bad |= hipEventDestroy((hipEvent_t)ev_fork) != hipSuccess;
    if (ev_join) bad |= hipEventDestroy((hipEvent_t)ev_join) != hipSuccess;
    return bad ? dsn_fail("%s", "dsn_aux_destroy: destroy failed") : 0;
}

// backward of DualSpaceNeRF.forward on explicit points (model/spacenet.py:210-266): see dsnerf.h
int dsn_module_grad(const void* scene, int V, int F, const void* packed, const float* const* params33_host, const float* poses24x3,
                    int frame_idx, int zero_code, const float* x_world, const float* x_canon, const float* view_dir,
                    const float* zeros_n, int64_t N, const float* d_colour, const float* d_sigma, float* const* grads33_host,
                    void* workspace, void* stream) {
    DSN_REQUIRE(scene && packed && params33_host && poses24x3 && x_world && x_canon && view_dir && zeros_n && d_colour && d_sigma &&
                grads33_host && workspace, "dsn_module_grad: null argument");
    DSN_REQUIRE(N > 0 && N < ((int64_t)1 << 30) && V > 0 && F > 0, "dsn_module_grad: bad sizes");
    DSN_REQUIRE(frame_idx >= 0 && frame_idx < 500, "dsn_module_grad: frame index outside the embedding table");
    for (int i = 0; i < DSN_NUM_PARAMS; ++i)
        DSN_REQUIRE(params33_host[i] && grads33_host[i], "dsn_module_grad: null parameter / gradient pointer");
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    // N "rays" of ONE sample each: origin = the world point, direction = its view direction, z = 0
    const char* err = dsn_train_run(s, (const float*)packed, params33_host, poses24x3, frame_idx, zero_code, x_world, view_dir, zeros_n,
                                    nullptr, (int)N, 1, d_colour, nullptr, nullptr, nullptr, nullptr, grads33_host, workspace,
                                    (hipStream_t)stream, false, x_canon, d_colour, d_sigma);
    if (err) return dsn_fail("dsn_module_grad: %s failed", err);
    return dsn_check_launch("dsn_module_grad");
}

// diagnostics (synchronises the stream): {ncell, ok, total, cap} of world-fine, world-coarse, canon-fine,
// canon-coarse nearest-face levels -> out16_host
int dsn_debug_nn_stats(const void* scene, int V, int F, int32_t* out16_host, void* stream) {
    DSN_REQUIRE(scene && out16_host && V > 0 && F > 0, "dsn_debug_nn_stats: bad argument");
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    const DsnGrid* gs[4] = {s.nn_world.fine.g, s.nn_world.coarse.g, s.nn_canon.fine.g, s.nn_canon.coarse.g};
    for (int i = 0; i < 4; ++i) {
        DsnGrid h;
        if (hipMemcpyAsync(&h, gs[i], sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
            hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
            return dsn_fail("%s", "dsn_debug_nn_stats: copy failed");
        out16_host[4 * i + 0] = h.ncell; out16_host[4 * i + 1] = h.ok; out16_host[4 * i + 2] = h.total; out16_host[4 * i + 3] = h.cap;
    }
    return 0;
}

// where the four 64-byte level headers live inside a scene blob (host function): lets a caller copy them out asynchronously and
// watch for a level that did not fit its list capacity without the synchronisation dsn_debug_nn_stats implies
int dsn_nn_header_offsets(int V, int F, size_t* out4_host) {
    DSN_REQUIRE(out4_host && V > 0 && F > 0, "dsn_nn_header_offsets: bad argument");
    DsnSceneView s = dsn_scene_view(nullptr, V, F);
    const DsnGrid* gs[4] = {s.nn_world.fine.g, s.nn_world.coarse.g, s.nn_canon.fine.g, s.nn_canon.coarse.g};
    for (int i = 0; i < 4; ++i) out4_host[i] = (size_t)((const char*)gs[i] - (const char*)nullptr);
    return 0;
}

// utils/rays_utils.py:16-30 get_rays + :63-97 get_near_far, whole-image path (:176-184)
int dsn_camera_rays(const double* K3x3, const double* R3x3, const double* T3, const double* bounds2x3, int H, int W,
                    int convention, float* ray_o, float* ray_d, float* near, float* far, uint8_t* mask_at_box, void* stream) {
    DSN_REQUIRE(K3x3 && R3x3 && T3 && bounds2x3 && ray_o && ray_d && near && far && mask_at_box, "dsn_camera_rays: null argument");
    DSN_REQUIRE(H > 0 && W > 0, "dsn_camera_rays: empty image");
    // the kernels index ray_o[3 * p + c] with int: 3 * H * W must stay below 2^31
    DSN_REQUIRE((int64_t)H * W <= (int64_t)INT32_MAX / 3, "dsn_camera_rays: more than (2^31 - 1) / 3 pixels");
    DSN_REQUIRE(convention == DSN_RAYS_ZJU || convention == DSN_RAYS_H36M, "dsn_camera_rays: unknown convention");
    dsn_launch_camera_rays(K3x3, R3x3, T3, bounds2x3, H, W, ray_o, ray_d, near, far, mask_at_box, (hipStream_t)stream,
                           convention == DSN_RAYS_H36M);
    return dsn_check_launch("dsn_camera_rays");
}

// a training batch drawn on the device (utils/rays_utils.py:104-172, utils/h36m_utils.py:78-146; the rule is in dsnerf.h)
static bool dsn_image_size_ok(int H, int W) { return H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31); }

int dsn_bound_mask(const double* K3x3, const double* R3x3, const double* T3, const double* bounds2x3, int H, int W, uint8_t* mask_out,
                   void* stream) {
    DSN_REQUIRE(K3x3 && R3x3 && T3 && bounds2x3 && mask_out, "dsn_bound_mask: null argument");
    DSN_REQUIRE(H > 0 && W > 0, "dsn_bound_mask: empty image");
    DSN_REQUIRE(dsn_image_size_ok(H, W), "dsn_bound_mask: 2^31 or more pixels");
    dsn_launch_bound_mask(K3x3, R3x3, T3, bounds2x3, H, W, mask_out, (hipStream_t)stream);
    return dsn_check_launch("dsn_bound_mask");
}

size_t dsn_train_rays_workspace_bytes(int H, int W, int nrays) {
    if (!dsn_image_size_ok(H, W) || nrays < 1 || nrays > DSN_TRAIN_RAYS_MAX_RAYS) return 0;
    return dsn_train_rays_workspace_size((int64_t)H * W, nrays);
}

int dsn_train_rays(const double* K3x3, const double* R3x3, const double* T3, const double* bounds2x3, int H, int W, int convention,
                   const double* img_f64, const float* img_f32, const uint8_t* mask_a, const uint8_t* mask_b, const uint8_t* bound_mask_in,
                   const uint8_t* occupancy_src, int nrays, uint32_t seed, float* ray_o, float* ray_d, float* near, float* far,
                   int64_t* coord, float* rgb, uint8_t* occupancy, uint8_t* mask_at_box, uint8_t* bound_mask_out, int32_t* status,
                   int32_t* rounds, void* workspace, size_t workspace_bytes, void* stream) {
    DSN_REQUIRE(K3x3 && R3x3 && T3 && bounds2x3 && mask_a && ray_o && ray_d && near && far && coord && rgb && mask_at_box &&
                bound_mask_out && status && rounds && workspace, "dsn_train_rays: null argument");
    DSN_REQUIRE(H > 0 && W > 0, "dsn_train_rays: empty image");
    DSN_REQUIRE(dsn_image_size_ok(H, W), "dsn_train_rays: 2^31 or more pixels");
    DSN_REQUIRE(nrays >= 1 && nrays <= DSN_TRAIN_RAYS_MAX_RAYS, "dsn_train_rays: nrays must be 1 ... 65536");
    DSN_REQUIRE(convention == DSN_RAYS_ZJU || convention == DSN_RAYS_H36M, "dsn_train_rays: unknown convention");
    DSN_REQUIRE((img_f64 != nullptr) != (img_f32 != nullptr), "dsn_train_rays: exactly one of img_f64 / img_f32");
    DSN_REQUIRE(convention != DSN_RAYS_H36M || mask_b, "dsn_train_rays: DSN_RAYS_H36M needs mask_b (msk_cihp)");
    DSN_REQUIRE((occupancy != nullptr) == (occupancy_src != nullptr), "dsn_train_rays: occupancy and occupancy_src go together");
    DSN_REQUIRE(workspace_bytes >= dsn_train_rays_workspace_size((int64_t)H * W, nrays),
                "dsn_train_rays: workspace_bytes too small (dsn_train_rays_workspace_bytes)");
    DSN_REQUIRE(((uintptr_t)workspace & 15) == 0, "dsn_train_rays: workspace must be 16-byte aligned");
    DsnTrainRaysArgs a;
    a.K = K3x3; a.R = R3x3; a.T = T3; a.bounds = bounds2x3;
    a.H = H; a.W = W; a.convention = convention; a.nrays = nrays; a.seed = seed;
    a.img64 = img_f64; a.img32 = img_f32;
    a.mask_a = mask_a; a.mask_b = convention == DSN_RAYS_H36M ? mask_b : nullptr; a.bound_in = bound_mask_in; a.occ_src = occupancy_src;
    a.ray_o = ray_o; a.ray_d = ray_d; a.near = near; a.far = far; a.rgb = rgb; a.coord = coord;
    a.occupancy = occupancy; a.mask_at_box = mask_at_box; a.bound_out = bound_mask_out;
    a.status = status; a.rounds = rounds; a.workspace = workspace;
    dsn_launch_train_rays(a, (hipStream_t)stream);
    return dsn_check_launch("dsn_train_rays");
}

// workspace carve for the fused path
#define DSN_CELLMAJOR_MIN (1 << 20)   // below ~1 M samples the five extra launches cost more than they save (measured:
                                      // -0.12 ms at 128x128x32, +0.42 ms at 256x256x64)
#define DSN_TRAIN_FAR_SEARCH_MIN (1 << 15)   // train mode: batches from here on search their far canonical points cell-major
#define DSN_TRAIN_CELLMAJOR_MIN (1 << 18)    // train mode: batches from here on take the fused sampler + cell-major search + warp (round 6)
struct DsnWorkspace {
    int32_t* count;       // [128] (first word = number of active samples)
    int32_t* active;      // [N]
    uint8_t* transparent; // [N]
    float* z;             // [N] (used when the caller does not want z_vals)
    float* x_c;           // [N,3]
    float* sigma;         // [N]
    // Two 12 N-byte regions, adjacent, each used by two arrays IN PLACE (round 4; round 3 kept four arrays = 48 B per sample):
    //   G: d sigma / dx_c, overwritten sample by sample with the world normal made from it (k_normal reads its sample's gradient, then
    //      writes its normal); before the field phase the screen's keep list, after the slices the shading weights
    //   E: essence, overwritten sample by sample with the colour made from it (k_light16 / k_light write a tile's colours after they
    //      have read its essences; DSN_EARLY_STOP zeroes the "colour" of a sample it does not shade - its essence is dead by then)
    // and, during the geometry phase, together the 24 N bytes of the cell-major sort: cells (4 N) | ranks (4 N) | sorted records (16 N).
    float* essence;       // [N,3]  = E
    float* grad;          // [N,3]  = G
    float* n_w;           // [N,3]  = G
    float* colour;        // [N,3]  = E
    void* sort_scratch;   // 16 N bytes at G + 8 N (the sorted (point, id) records of the nearest-face search)
    int32_t* pos;         // [N]   samples with sigma > 0 (eval-mode split of the field kernel)
    void* masks;          // [rec_cap] x 224 B relu-mask records, indexed by the slot on the sigma > 0 list
    int64_t rec_cap;
    void* nn_small;       // per-cell scratch of the cell-major nearest-face search
    int32_t* keep;        // [N]   samples the density screen could not rule out
    int32_t* audit;       // [audit_cap] samples declared empty that DSN_SCREEN_AUDIT sends through the accurate pass anyway
    int audit_cap;
    void* T;              // [R] x 8 B  DSN_EARLY_STOP: (transmittance, slices it covers) of every ray (k_slice_alive)
    int32_t* slices;      // [R (S + 64)] the active list split by slice (slice k at k * R * L); later the shading list
    int32_t* alive;       // [N]   the current slice's samples on rays that are not finished
    size_t bytes;
};
// words of DsnWorkspace::count (device, int32): diagnostics the host mirror reads after a frame
#define DSN_CNT_ACTIVE 0      // non-transparent samples
#define DSN_CNT_POS 16        // samples with sigma > 0 (reverse pass, normals, lighting)
#define DSN_CNT_KEEP 32       // samples the density screen sent to the accurate pass
#define DSN_CNT_AUDIT 40      // DSN_SCREEN_AUDIT: audit candidates (runs past the capacity), [44] audited samples with accurate sigma > 0,
                              //                   [45] their max sigma (float bits), [46] samples audited (<= capacity)
#define DSN_CNT_RANGE 48      // dsn_render_rays_train: samples whose activations / adjoints left the fp16 range
#define DSN_CNT_FLAGGED 20    // eval mode: samples the split-fp16 passes flagged for the exact-fp32 fallback (k_field<fix> looks here first)
#define DSN_CNT_ALIVE_K 96    // DSN_EARLY_STOP: [96..127] live samples of slice k, [128..159] samples of slice k the screen kept (a counter
#define DSN_CNT_KEEP_K 128    //                 of its own per slice: no clearing launches inside the slice loop)
#define DSN_CNT_BYTES 8192     // 256 count words + (from word 256) the slice histogram of DSN_STOP_STATS: (K + 1) x K ints, K <= 32
#define DSN_CNT_HIST 256
#define DSN_CNT_SLICE 64      // DSN_EARLY_STOP: [64..95] active samples per slice (at most 32 slices), [12] alive in the current slice,
#define DSN_CNT_ALIVE 12      //                 [13] reverse-pass slots, [14] shaded samples
#define DSN_CNT_SEL 13
#define DSN_CNT_LIT 14
#define DSN_CNT_STOP 56       // [56] samples left out by ray termination, [57] samples not shaded (weight < eps), [58] DSN_STOP_STATS,
                              // [59] largest |colour| the compositor weighed (float bits; eval frames) - the scale of the early-stop bound
// (the DSN_EARLY_STOP threshold: dsn_stop_eps_scaled, dsn_common.h - it follows S and the colour scale kept in `packed`)
// samples per slice: 4 on big frames (finer termination: the converged set's 512 x 512 x 64 frame 10.32 -> 9.99 ms, w3 12.52 -> 12.22 with
// two frames in flight; profiles/r03_stop_slice_sweep.txt), 8 where the three launches per slice weigh more than the samples they save
static inline int dsn_slice_len(int R, int S) {
    const char* e = getenv("DSN_STOP_SLICE");      // experiments: samples per slice
    int L = e ? atoi(e) : ((int64_t)R * S >= ((int64_t)1 << 22) ? 4 : 8);
    if (L < 1) L = 8;
    if (L > 64) L = 64;
    return (S + L - 1) / L <= DSN_STOP_MAX_SLICES ? L : (S + DSN_STOP_MAX_SLICES - 1) / DSN_STOP_MAX_SLICES;
}
// samples per slice of the DSN_STOP_STATS histogram: HALF the uniform slice where that keeps K <= 32 - the schedule a caller cuts from the
// histogram (dsn_render_rays_ex) may put its borders there (round 6's last session: the bench frame's schedule from 2-sample statistics
// evaluates 1.3 % fewer samples than from 4-sample ones, -0.05 ms); the uniform slicing itself stays as it is (2-sample uniform slices
// measured worse: 32 launches)
static inline int dsn_stats_slice_len(int R, int S) {
    const int L = dsn_slice_len(R, S), half = L >= 2 ? L / 2 : L;
    return (S + half - 1) / half <= DSN_STOP_MAX_SLICES ? half : L;
}
// entries of the per-slice lists: K slices of R * L each (K L < S + L) for the slice length in use - round 3 reserved R (S + 64) for any
// length (8 bytes per sample at S = 64; now 4).  DSN_STOP_SLICE (experiments) changes L: set it before the workspace is sized.
static inline size_t dsn_slice_entries(size_t R, int S) {
    const int L = dsn_slice_len((int)std::min<size_t>(R, 0x7fffffff), S), K = (S + L - 1) / L;
    return R * (size_t)K * (size_t)L;
}
// Capacity of the relu-record array of a frame.  The records (224 B per sample) are what the reverse pass needs of the forward
// pass, only for samples with sigma > 0, so they are indexed by the slot on that list and sized for a FRACTION of the samples of a
// big frame.  The capacity is a property of the WORKSPACE (round 5; rounds 3-4 kept a process-wide fraction): the records are the
// LAST array of the carve, everything else has a place that depends on (R, S) alone, and the capacity is whatever the caller's
// workspace_bytes leave behind the fixed part - dsn_render_workspace_bytes_for(R, S, fraction) sizes it, dsn_render_rays_ex reads
// it back from the size it is handed.  The bench frame puts 11.6 % (hash-random parameters) / 14 % (converged parameters,
// front-to-back slices) of its samples there, a briefly trained solid 39 %: the host mirror's probe frame sizes each of its
// workspaces per checkpoint; samples beyond the capacity take the single-launch forward + reverse pass instead
// (dsn_launch_field16_from): same values, no records, ~10 % more time for them.
// DSN_RECORD_CAP (tests) lowers the capacity IN USE below what the workspace holds.
#define DSN_RECORD_FRACTION_DEFAULT 0.125f
static int64_t dsn_record_cap_for(int64_t N, float fraction) {
    const int64_t floor_ = (int64_t)1 << 21;
    if (N <= floor_) return N;
    if (!(fraction > 0.0f)) fraction = DSN_RECORD_FRACTION_DEFAULT;
    if (fraction > 1.0f) fraction = 1.0f;
    int64_t c = (int64_t)((double)N * (double)fraction);
    c = (c + 255) & ~(int64_t)255;
    return c < floor_ ? floor_ : (c > N ? N : c);
}
// rec_cap < 0: the fixed part only (w.bytes = where the records begin)
static DsnWorkspace dsn_carve(void* base, int R, int S, int64_t rec_cap) {
    DsnWorkspace w;
    size_t N = (size_t)R * S;
    char* p = (char*)base;
    w.count = (int32_t*)p;        p += DSN_CNT_BYTES;
    w.active = (int32_t*)p;       p += dsn_align256(4 * N);
    w.transparent = (uint8_t*)p;  p += dsn_align256(N);
    w.z = (float*)p;              p += dsn_align256(4 * N);
    w.x_c = (float*)p;            p += dsn_align256(12 * N);
    w.sigma = (float*)p;          p += dsn_align256(4 * N);
    w.grad = w.n_w = (float*)p;          p += 12 * N;                       // G (no padding between G and E: the sort spans both)
    w.essence = w.colour = (float*)p;    p += dsn_align256(12 * N + 256);   // E
    w.sort_scratch = (void*)((char*)w.grad + ((8 * N + 15) & ~(size_t)15));      // (16-byte aligned records; E carries 256 bytes of slack)
    w.pos = (int32_t*)p;          p += dsn_align256(4 * N);
    w.nn_small = (void*)p;        p += dsn_nn_sort_scratch_size((int64_t)N);
    // the density screen's keep list lives from the screen to the forward launch of a slice / frame: inside the field phase, where the
    // normal buffer is free (the geometry phase's sort is done with it, the early-stop shading weights and the normals come later)
    w.keep = (int32_t*)w.n_w;
    w.audit_cap = (int)(N / 32 + 1024);                                      // 1/128 of the empty samples are audited
    w.audit = (int32_t*)p;        p += dsn_align256(4 * (size_t)w.audit_cap);
    w.T = (void*)p;               p += dsn_align256(8 * (size_t)R);
    w.slices = (int32_t*)p;       p += dsn_align256(4 * dsn_slice_entries((size_t)R, S));
    w.alive = (int32_t*)p;        p += dsn_align256(4 * N);
    // the relu records LAST: nothing else moves with their capacity
    w.rec_cap = rec_cap < 0 ? 0 : rec_cap;
    w.masks = (void*)p;           p += dsn_align256(224 * (size_t)w.rec_cap);
    w.bytes = (size_t)(p - (char*)base);
    return w;
}
static size_t dsn_workspace_fixed_bytes(int R, int S) { return dsn_carve(nullptr, R, S, -1).bytes; }
// records a workspace of `bytes` bytes holds for an R x S frame (-1: not even the fixed part fits)
static int64_t dsn_record_cap_of(int R, int S, size_t bytes) {
    const size_t fixed = dsn_workspace_fixed_bytes(R, S);
    if (bytes < fixed) return -1;
    const int64_t N = (int64_t)R * S;
    int64_t c = (int64_t)((bytes - fixed) / 224);
    if (c > N) c = N;
    const char* e = getenv("DSN_RECORD_CAP");      // tests: a smaller capacity IN USE (provokes the overflow pass)
    if (e) { const long long v = atoll(e); c = v < 1 ? (c < 1 ? c : 1) : (v < c ? v : c); }
    return c;
}

size_t dsn_render_workspace_bytes_for(int R, int S, float record_fraction) {
    if (R <= 0 || S <= 0) return 0;
    return dsn_carve(nullptr, R, S, dsn_record_cap_for((int64_t)R * S, record_fraction)).bytes;
}
size_t dsn_render_workspace_bytes(int R, int S) { return dsn_render_workspace_bytes_for(R, S, DSN_RECORD_FRACTION_DEFAULT); }
int64_t dsn_render_workspace_record_capacity(int R, int S, size_t workspace_bytes) {
    if (R <= 0 || S <= 0) return -1;
    return dsn_record_cap_of(R, S, workspace_bytes ? workspace_bytes : dsn_render_workspace_bytes(R, S));
}

// samples per uniform slice of DSN_EARLY_STOP for an R x S frame (what dsn_render_rays_ex cuts and the DSN_STOP_STATS histogram counts)
int dsn_stop_slice_len(int R, int S) { return (R > 0 && S > 0) ? dsn_slice_len(R, S) : 0; }
// samples per slice of the DSN_STOP_STATS histogram (<= dsn_stop_slice_len: see dsn_stats_slice_len)
int dsn_stop_stats_slice_len(int R, int S) { return (R > 0 && S > 0) ? dsn_stats_slice_len(R, S) : 0; }

float dsn_early_stop_colour_headroom(void) { return DSN_STOP_COLOUR_HEADROOM; }
float dsn_early_stop_eps(int S) { return dsn_stop_eps_scaled(S > 0 ? S : 1, 1.0f); }
float dsn_early_stop_eps_scaled(int S, float colour_scale) { return dsn_stop_eps_scaled(S > 0 ? S : 1, colour_scale); }

// the same calibration on the points of a FRAME: see dsnerf.h
int dsn_calibrate_screen_frame(const void* scene, int V, int F, void* packed, const void* render_workspace, int R, int S,
                               int64_t n_points, void* workspace, float* out4, void* stream) {
    DSN_REQUIRE(scene && packed && workspace && render_workspace, "dsn_calibrate_screen_frame: null argument");
    DSN_REQUIRE(V > 0 && F > 0 && n_points > 0 && R > 0 && S > 0, "dsn_calibrate_screen_frame: bad sizes");
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    const DsnWorkspace w = dsn_carve((void*)render_workspace, R, S, -1);      // (the fixed part: x_c, the active list, the count words)
    dsn_launch_calibrate_screen(s, (float*)packed, n_points, workspace, out4, (hipStream_t)stream, w.x_c, w.active, w.count + DSN_CNT_ACTIVE);
    return dsn_check_launch("dsn_calibrate_screen_frame");
}


int dsn_render_rays(const void* scene, int V, int F, const void* packed, const float* ray_o, const float* ray_d, float* near,
                    float* far, int R, int S, const float* t_vals, const float* jitter, const float* noise,
                    int flags, float* out_rgb, float* out_disp, float* out_acc, float* out_depth,
                    float* out_weights, float* out_z, void* workspace, void* stream) {
    return dsn_render_rays_ex(scene, V, F, packed, ray_o, ray_d, near, far, R, S, t_vals, jitter, noise, flags, out_rgb, out_disp, out_acc,
                              out_depth, out_weights, out_z, workspace, 0, nullptr, 0, stream);
}

// dsn_render_rays_lights: what replaces the shading phase of a frame (NULL: the frame's own light, dsn_render_rays_ex)
struct DsnLightSweep {
    const DsnLightEdit* lights;      // [n_lights] (device)
    int n_lights;
    void* scratch;            // compact colours of a group of lights: [G][n_shaded][3] (maps: + the light factors [G][n_shaded])
    size_t scratch_bytes;
    const struct DsnMapsOut* maps;      // dsn_render_rays_maps: the decomposition maps beside the colours (NULL: the plain sweep)
};
// dsn_render_rays_maps: where the maps go (each may be NULL); out_rgb may be NULL too then
struct DsnMapsOut {
    float* albedo;      // [R,3]
    float* normal;      // [R,3]
    float* shading;     // [n_lights,R]
    float* max2;        // largest |essence|, largest light factor weighed (device)
};
static int dsn_render_frame(const void* scene, int V, int F, const void* packed, const float* ray_o, const float* ray_d, float* near,
                            float* far, int R, int S, const float* t_vals, const float* jitter, const float* noise,
                            int flags, float* out_rgb, float* out_disp, float* out_acc, float* out_depth,
                            float* out_weights, float* out_z, void* workspace, size_t workspace_bytes, const int32_t* slice_lengths_host,
                            int n_slices, void* stream, const DsnLightSweep* sweep);

int dsn_render_rays_ex(const void* scene, int V, int F, const void* packed, const float* ray_o, const float* ray_d, float* near,
                       float* far, int R, int S, const float* t_vals, const float* jitter, const float* noise,
                       int flags, float* out_rgb, float* out_disp, float* out_acc, float* out_depth,
                       float* out_weights, float* out_z, void* workspace, size_t workspace_bytes, const int32_t* slice_lengths_host,
                       int n_slices, void* stream) {
    return dsn_render_frame(scene, V, F, packed, ray_o, ray_d, near, far, R, S, t_vals, jitter, noise, flags, out_rgb, out_disp, out_acc,
                            out_depth, out_weights, out_z, workspace, workspace_bytes, slice_lengths_host, n_slices, stream, nullptr);
}

static_assert(DSN_LIGHT_RECORD_FLOATS == 12, "dsn_common.h and include/dsnerf.h disagree on the light record");

size_t dsn_render_lights_scratch_bytes(int R, int S, int n_lights, int64_t n_shaded) {
    if (R <= 0 || S <= 0 || n_lights < 1 || n_shaded < 0 || n_shaded > (int64_t)R * S) return 0;
    return dsn_align256(sizeof(float) * 3 * (size_t)n_lights * (size_t)std::max<int64_t>(n_shaded, 1));
}

int dsn_render_rays_lights(const void* scene, int V, int F, const void* packed, const float* ray_o, const float* ray_d, float* near,
                           float* far, int R, int S, const float* t_vals, const float* jitter, const float* noise, int flags,
                           const float* lights, int n_lights, float* out_rgb, float* out_disp, float* out_acc, float* out_depth,
                           float* out_weights, float* out_z, void* workspace, size_t workspace_bytes, void* light_scratch,
                           size_t light_scratch_bytes, const int32_t* slice_lengths_host, int n_slices, void* stream) {
    DSN_REQUIRE(R > 0 && S > 0, "dsn_render_rays_lights: empty ray batch");
    DSN_REQUIRE(scene && packed && ray_o && ray_d && near && far && t_vals && workspace && lights && light_scratch,
                "dsn_render_rays_lights: null argument");
    DSN_REQUIRE(out_rgb && out_disp && out_acc && out_depth, "dsn_render_rays_lights: null output");
    DSN_REQUIRE(n_lights >= 1, "dsn_render_rays_lights: n_lights must be at least 1");
    DSN_REQUIRE(!jitter && !noise, "dsn_render_rays_lights: eval mode only (no jitter, no noise)");
    DSN_REQUIRE(flags & DSN_SKIP_TRANSPARENT, "dsn_render_rays_lights: eval mode only (flags must hold DSN_SKIP_TRANSPARENT)");
    DSN_REQUIRE(!(flags & DSN_FIELD_FP32), "dsn_render_rays_lights: DSN_FIELD_FP32 is not supported (split-fp16 lighting only)");
    DSN_REQUIRE(!(flags & (DSN_PHASE_GEOMETRY | DSN_PHASE_FIELD | DSN_PHASE_SHADE)),
                "dsn_render_rays_lights: DSN_PHASE_* bits are not supported (one call renders the whole sweep)");
    DSN_REQUIRE(S == 64 || S == 128, "dsn_render_rays_lights: S must be 64 or 128 (the 16-lane compositor)");
    DSN_REQUIRE((((uintptr_t)workspace | (uintptr_t)out_weights | (uintptr_t)out_z) & 15) == 0,
                "dsn_render_rays_lights: workspace, out_weights and out_z must be 16-byte aligned");
    DSN_REQUIRE(light_scratch_bytes >= dsn_render_lights_scratch_bytes(R, S, 1, 0),
                "dsn_render_rays_lights: light_scratch is too small (dsn_render_lights_scratch_bytes)");
    const DsnLightSweep sweep = {reinterpret_cast<const DsnLightEdit*>(lights), n_lights, light_scratch, light_scratch_bytes, nullptr};
    return dsn_render_frame(scene, V, F, packed, ray_o, ray_d, near, far, R, S, t_vals, jitter, noise, flags, out_rgb, out_disp, out_acc,
                            out_depth, out_weights, out_z, workspace, workspace_bytes, slice_lengths_host, n_slices, stream, &sweep);
}

size_t dsn_render_maps_scratch_bytes(int R, int S, int n_lights, int64_t n_shaded) {
    if (R <= 0 || S <= 0 || n_lights < 1 || n_shaded < 0 || n_shaded > (int64_t)R * S) return 0;
    return dsn_align256(sizeof(float) * 4 * (size_t)n_lights * (size_t)std::max<int64_t>(n_shaded, 1));
}

int dsn_render_rays_maps(const void* scene, int V, int F, const void* packed, const float* ray_o, const float* ray_d, float* near,
                         float* far, int R, int S, const float* t_vals, const float* jitter, const float* noise, int flags,
                         const float* lights, int n_lights, float* out_rgb, float* out_disp, float* out_acc, float* out_depth,
                         float* out_weights, float* out_z, float* out_albedo, float* out_normal, float* out_shading, float* out_max,
                         void* workspace, size_t workspace_bytes, void* light_scratch, size_t light_scratch_bytes,
                         const int32_t* slice_lengths_host, int n_slices, void* stream) {
    DSN_REQUIRE(R > 0 && S > 0, "dsn_render_rays_maps: empty ray batch");
    DSN_REQUIRE(scene && packed && ray_o && ray_d && near && far && t_vals && workspace && lights && light_scratch,
                "dsn_render_rays_maps: null argument");
    DSN_REQUIRE(out_disp && out_acc && out_depth, "dsn_render_rays_maps: null output (out_rgb and the maps may be NULL, disp / acc / depth not)");
    DSN_REQUIRE(n_lights >= 1, "dsn_render_rays_maps: n_lights must be at least 1");
    DSN_REQUIRE(!jitter && !noise, "dsn_render_rays_maps: eval mode only (no jitter, no noise)");
    DSN_REQUIRE(flags & DSN_SKIP_TRANSPARENT, "dsn_render_rays_maps: eval mode only (flags must hold DSN_SKIP_TRANSPARENT)");
    DSN_REQUIRE(!(flags & DSN_FIELD_FP32), "dsn_render_rays_maps: DSN_FIELD_FP32 is not supported (split-fp16 lighting only)");
    DSN_REQUIRE(!(flags & (DSN_PHASE_GEOMETRY | DSN_PHASE_FIELD | DSN_PHASE_SHADE)),
                "dsn_render_rays_maps: DSN_PHASE_* bits are not supported (one call renders the whole sweep)");
    DSN_REQUIRE(S == 64 || S == 128, "dsn_render_rays_maps: S must be 64 or 128 (the 16-lane compositor)");
    DSN_REQUIRE((((uintptr_t)workspace | (uintptr_t)out_weights | (uintptr_t)out_z) & 15) == 0,
                "dsn_render_rays_maps: workspace, out_weights and out_z must be 16-byte aligned");
    DSN_REQUIRE(light_scratch_bytes >= dsn_render_maps_scratch_bytes(R, S, 1, 0),
                "dsn_render_rays_maps: light_scratch is too small (dsn_render_maps_scratch_bytes)");
    const DsnMapsOut maps = {out_albedo, out_normal, out_shading, out_max};
    const DsnLightSweep sweep = {reinterpret_cast<const DsnLightEdit*>(lights), n_lights, light_scratch, light_scratch_bytes, &maps};
    return dsn_render_frame(scene, V, F, packed, ray_o, ray_d, near, far, R, S, t_vals, jitter, noise, flags, out_rgb, out_disp, out_acc,
                            out_depth, out_weights, out_z, workspace, workspace_bytes, slice_lengths_host, n_slices, stream, &sweep);
}

static int dsn_render_frame(const void* scene, int V, int F, const void* packed, const float* ray_o, const float* ray_d, float* near,
                            float* far, int R, int S, const float* t_vals, const float* jitter, const float* noise,
                            int flags, float* out_rgb, float* out_disp, float* out_acc, float* out_depth,
                            float* out_weights, float* out_z, void* workspace, size_t workspace_bytes, const int32_t* slice_lengths_host,
                            int n_slices, void* stream, const DsnLightSweep* sweep) {
    DSN_REQUIRE(R > 0 && S > 0, "dsn_render_rays: empty ray batch");      // (first: empty tensors come with null pointers)
    // front-to-back schedule (DSN_EARLY_STOP): uniform slices by default, the caller's lengths otherwise
    int bounds[DSN_STOP_MAX_SLICES + 1];
    int K;
    const int L = dsn_slice_len(R, S);
    if (slice_lengths_host && n_slices > 0) {
        DSN_REQUIRE(n_slices <= DSN_STOP_MAX_SLICES, "dsn_render_rays_ex: more than 32 slices");
        int at = 0;
        for (int k = 0; k < n_slices; ++k) {
            DSN_REQUIRE(slice_lengths_host[k] >= 1 && slice_lengths_host[k] <= 64, "dsn_render_rays_ex: a slice holds 1 to 64 samples");
            bounds[k] = at;
            at += slice_lengths_host[k];
        }
        DSN_REQUIRE(at == S, "dsn_render_rays_ex: the slice lengths must add up to S");
        K = n_slices;
        bounds[K] = S;
    } else {
        K = (S + L - 1) / L;
        for (int k = 0; k <= K; ++k) bounds[k] = k * L < S ? k * L : S;
    }
    const bool custom_schedule = slice_lengths_host && n_slices > 0;
    DSN_REQUIRE(scene && packed && ray_o && ray_d && near && far && t_vals && workspace, "dsn_render_rays: null argument");
    DSN_REQUIRE((out_rgb || (sweep && sweep->maps)) && out_disp && out_acc && out_depth, "dsn_render_rays: null output");
    DSN_REQUIRE(V > 0 && F > 0, "dsn_render_rays: bad V/F");
    const bool skip = (flags & DSN_SKIP_TRANSPARENT) != 0;
    DSN_REQUIRE(!(skip && noise), "dsn_render_rays: DSN_SKIP_TRANSPARENT is only exact without noise (eval mode)");
    // rays of more than 32 x 64 samples: a uniform slice would hold more than the 64 samples k_advance_T covers per launch (ADVICE r04:
    // the transmittance was then only partly advanced - safe, but termination silently did nothing).  Such frames render in one pass.
    if (!custom_schedule && L > 64) flags &= ~DSN_EARLY_STOP;
    hipStream_t st = (hipStream_t)stream;
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    // the relu-record capacity is what the caller's workspace holds behind the fixed part (0 = sized by dsn_render_workspace_bytes)
    const int64_t rec_cap = dsn_record_cap_of(R, S, workspace_bytes ? workspace_bytes : dsn_render_workspace_bytes(R, S));
    DSN_REQUIRE(rec_cap >= 1, "dsn_render_rays_ex: workspace_bytes is smaller than the fixed part of the workspace + one record "
                              "(size it with dsn_render_workspace_bytes_for)");
    DsnWorkspace w = dsn_carve(workspace, R, S, rec_cap);
    const int64_t N = (int64_t)R * S;
    float* z = out_z ? out_z : w.z;
    const DsnShareCus share((flags & DSN_SHARE_CUS) != 0);
    // Phases (DSN_PHASE_*): none of the three bits = the whole frame on `stream`.  With bits set only those parts are enqueued, so
    // that a caller with several frames in flight can put the geometry / shading kernels of one frame on a stream of their own
    // BESIDE the matrix-bound field kernels of another (events between the calls are the caller's; the state that travels
    // between the phases lives in `workspace`).  Same arguments in all three calls.
    const int ph = flags & (DSN_PHASE_GEOMETRY | DSN_PHASE_FIELD | DSN_PHASE_SHADE);
    const bool do_geom = !ph || (ph & DSN_PHASE_GEOMETRY), do_field = !ph || (ph & DSN_PHASE_FIELD), do_shade = !ph || (ph & DSN_PHASE_SHADE);
    int32_t* list = skip ? w.active : nullptr;
    int32_t* cnt = skip ? w.count : nullptr;
    const bool exh = (flags & DSN_NN_EXHAUSTIVE) != 0;
    if (do_geom) {
    const char* cm_env = getenv("DSN_CELLMAJOR_MIN");      // test / tuning override
    const long long cellmajor_min = cm_env ? atoll(cm_env) : (long long)DSN_CELLMAJOR_MIN;
    const bool cellmajor = !exh && N >= (int64_t)cellmajor_min;
    const bool fused_nn = cellmajor && !getenv("DSN_NN_UNFUSED");
    const bool lazy = (flags & DSN_LAZY_LISTS) != 0;
    const bool clear_cells = fused_nn && dsn_clear_cells_on(lazy, skip);      // (read once: the list build and the search below agree)
    // a lazily set frame (DSN_FRAME_LAZY_LISTS) outside the fused cell-major path: every cell's lists, here, before anything reads them
    // (small ray batches, DSN_NN_UNFUSED, the exhaustive cross-check) - ONCE per frame: the device header says whether the level is
    // still lazy, the chunks after the first find it complete (round 5 rebuilt everything per call)
    if (lazy && !fused_nn) dsn_launch_build_nn_complete(s.cent_world, F, s.nn_world, st);
    if (fused_nn) {
        // the sampler classifies the samples by fine cell while it writes their z (the first step of the cell-major search)
        int32_t *counts = nullptr, *outside0 = nullptr;
        dsn_nn_cellmajor_begin(w.nn_small, &counts, &outside0, st);
        dsn_launch_sample_gg(s.xyz, (flags & DSN_SAMPLE_UNIFORM) ? 0 : V, ray_o, ray_d, near, far, R, S, t_vals, jitter, z, nullptr, st,
                             s.nn_world.fine.g, (int32_t*)w.grad, counts, outside0, (int32_t*)w.grad + N);      // (+ N: every sample's rank in its cell)
        // ... and a lazily set frame gets the lists of the cells that classification found samples in (counts > 0)
        // (eval mode, `skip`: the search below runs with lazy_canon - cells all of whose samples are transparent get no list and no scan)
        if (lazy) dsn_launch_build_nn_visited(s.cent_world, F, s.nn_world, counts, st, s.face_world, clear_cells);
    } else
        dsn_launch_sample_gg(s.xyz, (flags & DSN_SAMPLE_UNIFORM) ? 0 : V, ray_o, ray_d, near, far, R, S, t_vals, jitter, z, nullptr, st);
    if (skip) {
        if (hipMemsetAsync(w.count, 0, DSN_CNT_BYTES, st) != hipSuccess) return dsn_fail("%s", "dsn_render_rays: memset failed");
    }
    if (cellmajor) {
        // cell-major search: samples counting-sorted by fine cell, lists through the scalar cache, and the rest of the warp stage
        // fused behind the search (dsn_nn.hip, k_nns_search<WARP>).  Scratch: buffers that are not written before the field's
        // forward pass - G | E, 24 N bytes back to back (dsn_carve): cell ids (4 N) and ranks (4 N) at the start of G, the sorted
        // (point, id) records (16 N) behind them, into E (an essence / colour is read only where the density is positive: no clearing).
        // Samples outside the fine grid (none for rays clipped to the body's bounds) are left to a k_warp pass of their own.
        int32_t* g3 = (int32_t*)w.grad;
        if (!fused_nn) {      // (DSN_NN_UNFUSED, cross-check / A-B switch: round 2's form - search writes nn[], k_warp reads it)
            dsn_launch_nn_cellmajor(s.nn_world, nullptr, ray_o, ray_d, z, N, S, g3, w.sort_scratch, g3 + N, w.nn_small, st);
            dsn_launch_warp(s, nullptr, ray_o, ray_d, z, N, S, nullptr, nullptr, nullptr, w.transparent, w.x_c, nullptr, list, cnt, exh, st,
                            g3 + N, skip);
        } else {
            int32_t* outside = nullptr;
            dsn_launch_nn_cellmajor_warp(s.nn_world, ray_o, ray_d, z, N, S, g3, w.sort_scratch, w.nn_small, s.face_world, s.face_canon,
                                         w.transparent, w.x_c, list, cnt, skip, &outside, st, true, lazy, clear_cells);
            dsn_launch_warp(s, nullptr, ray_o, ray_d, z, N, S, nullptr, nullptr, nullptr, w.transparent, w.x_c, nullptr, list, cnt, exh, st,
                            nullptr, skip, g3, outside);
        }
    } else
        dsn_launch_warp(s, nullptr, ray_o, ray_d, z, N, S, nullptr, nullptr, nullptr, w.transparent, w.x_c, nullptr, list, cnt, exh, st,
                        nullptr, skip);
    if (skip) {
        // untouched (skipped) samples must hold density 0 for the compositor (cleared here, after the nearest-face search has
        // finished with its scratch); a colour is read only where the density is positive (k_composite, lazy_colour)
        if (hipMemsetAsync(w.sigma, 0, sizeof(float) * N, st) != hipSuccess)
            return dsn_fail("%s", "dsn_render_rays: memset failed");
    }
    }       // geometry phase
    if (do_field) {
    // (eval mode: the count words were cleared in the geometry phase; the split-fp16 passes count what they flag for k_field<fix>)
    int32_t* const fcnt = skip ? w.count + DSN_CNT_FLAGGED : nullptr;
    if (flags & DSN_FIELD_FP32)
        dsn_launch_field((const float*)packed, s.frame, w.x_c, N, list, cnt, w.sigma, w.essence, w.grad, st);
    else if (skip && (flags & DSN_EARLY_STOP)) {
        // eval mode, front to back: slices of L samples along the rays; a ray whose transmittance has fallen below eps is finished
        const bool screen = (flags & DSN_DENSITY_SCREEN) != 0;
        const bool audit = screen && (flags & DSN_SCREEN_AUDIT);
        int32_t* pcnt = w.count + DSN_CNT_POS;
        dsn_launch_slice_bucket(w.active, w.count + DSN_CNT_ACTIVE, N, S, R, bounds, K, w.slices, w.count + DSN_CNT_SLICE, st);
        dsn_launch_slice_T_init(w.T, R, st);
        // How the rays' transmittance follows the slices.  "ray" (default): one coalesced per-ray pass over slice k - 1 (k_advance_T,
        // 14 us) + the list filter (8 us).  "list" (DSN_STOP_ADVANCE=list): the filter advances the rays of its own entries (no
        // k_advance_T launch - what VERDICT r03 #4 asked for; measured: 45 us per slice, the per-entry gathers cost more than the
        // launch they save: frame 9.84 against 9.71 ms with three frames in flight, profiles/r04_stop_advance_ab.txt).  Same pairs,
        // same products, same lists either way.
        static const bool adv_env_ray = [] { const char* e = getenv("DSN_STOP_ADVANCE"); return !(e && e[0] == 'l'); }();
        const bool adv_per_ray = adv_env_ray || custom_schedule;      // (the list-fused form knows uniform slices only)
        const float* scal = (const float*)packed + OFF_SCAL;
        for (int k = 0; k < K; ++k) {
            const int s0 = bounds[k], s1 = bounds[k + 1];
            const int64_t Nk = (int64_t)R * (s1 - s0);
            const int32_t* sl = w.slices + (int64_t)R * s0;
            const int32_t* sc = w.count + DSN_CNT_SLICE + k;
            if (k > 0) {
                int32_t* acnt = w.count + DSN_CNT_ALIVE_K + k;
                // (advances the rays' transmittance over slice k - 1 on the way: no k_advance_T launch between the slices)
                if (adv_per_ray) dsn_launch_advance_T(w.sigma, w.transparent, z, ray_d, R, S, bounds[k - 1], s0, k, w.T, st);
                dsn_launch_slice_alive(sl, sc, Nk, S, L, k, w.T, w.sigma, w.transparent, z, ray_d, scal, w.alive, acnt, w.count + DSN_CNT_STOP, st,
                                       adv_per_ray);
                sl = w.alive;
                sc = acnt;
            }
            if (screen) {
                int32_t* kcnt = w.count + DSN_CNT_KEEP_K + k;
                dsn_launch_screen16((const float*)packed, s.frame, w.x_c, Nk, sl, sc, w.sigma, w.keep, kcnt, nullptr, nullptr, st,
                                    audit ? w.audit : nullptr, audit ? w.count + DSN_CNT_AUDIT : nullptr, w.audit_cap);
                sl = w.keep;
                sc = kcnt;
            }
            // (the sigma > 0 list and its relu records keep growing from slice to slice)
            dsn_launch_field16_fwd((const float*)packed, s.frame, w.x_c, Nk, sl, sc, w.sigma, w.essence, w.masks, w.pos, pcnt, st,
                                   w.rec_cap, fcnt);
            (void)s0;
        }
        // shading list: weights from the densities alone (the compositor without a colour and without per-ray outputs; flagged
        // densities are still NaN and keep their rays' samples); scratch = the normal buffer
        float* wq = w.n_w;
        dsn_launch_composite(nullptr, w.sigma, w.transparent, z, ray_d, nullptr, R, S, nullptr, nullptr, nullptr, wq, nullptr, st);
        int32_t* sel = w.alive;             // (dead by now; the list of non-transparent samples stays intact: dsn_calibrate_screen_frame)
        int32_t* lit = w.slices;
        dsn_launch_cull_lit(w.pos, pcnt, N, w.rec_cap, wq, w.sigma, S, scal, sel, w.count + DSN_CNT_SEL, lit, w.count + DSN_CNT_LIT,
                            w.count + DSN_CNT_STOP + 1, w.colour, st);
        dsn_launch_field16_bwd((const float*)packed, s.frame, w.x_c, N, w.pos, pcnt, w.grad, w.masks, st, w.sigma, w.rec_cap, sel,
                               w.count + DSN_CNT_SEL, fcnt);
        if (w.rec_cap < N)
            dsn_launch_field16_from((const float*)packed, s.frame, w.x_c, N, w.pos, pcnt, w.rec_cap, w.sigma, w.essence, w.grad, st, fcnt);
        dsn_launch_field_fix((const float*)packed, s.frame, w.x_c, N, w.pos, pcnt, w.sigma, w.essence, w.grad, st, fcnt);
        if (audit) dsn_launch_screen_audit(w.audit, w.count + DSN_CNT_AUDIT, w.audit_cap, w.sigma, w.count + DSN_CNT_AUDIT + 4, st);
        list = lit;
        cnt = w.count + DSN_CNT_LIT;
    } else if (skip) {
        // eval mode: forward for every non-transparent sample, then d sigma/dx, normals and lighting only where sigma > 0
        // (elsewhere alpha = 0 exactly and the colour is never used); count[16] = number of such samples
        int32_t* pcnt = w.count + DSN_CNT_POS;
        const bool screen = (flags & DSN_DENSITY_SCREEN) != 0;
        const bool audit = screen && (flags & DSN_SCREEN_AUDIT);
        if (screen) {
            // plain-fp16 screen: samples whose fp16 density is negative by the safety margin keep that (negative) density and leave the
            // list; count[32] = samples that go through the accurate pass
            int32_t* kcnt = w.count + DSN_CNT_KEEP;
            dsn_launch_screen16((const float*)packed, s.frame, w.x_c, N, list, cnt, w.sigma, w.keep, kcnt, nullptr, nullptr, st,
                                audit ? w.audit : nullptr, audit ? w.count + DSN_CNT_AUDIT : nullptr, w.audit_cap);
            list = w.keep;
            cnt = kcnt;
        }
        dsn_launch_field16_fwd((const float*)packed, s.frame, w.x_c, N, list, cnt, w.sigma, w.essence, w.masks, w.pos, pcnt, st,
                               w.rec_cap, fcnt);
        dsn_launch_field16_bwd((const float*)packed, s.frame, w.x_c, N, w.pos, pcnt, w.grad, w.masks, st, w.sigma, w.rec_cap, nullptr, nullptr,
                               fcnt);
        list = w.pos;
        cnt = pcnt;
        // samples of the sigma > 0 list beyond the record capacity (none on ordinary frames: the launch is N - cap empty
        // workgroups' worth of looking): forward + reverse in one launch, bit-identical values
        if (w.rec_cap < N)
            dsn_launch_field16_from((const float*)packed, s.frame, w.x_c, N, list, cnt, w.rec_cap, w.sigma, w.essence, w.grad, st, fcnt);
        // range fallback: whatever either pass flagged (sigma = NaN; such samples are on the sigma > 0 list) in exact fp32
        dsn_launch_field_fix((const float*)packed, s.frame, w.x_c, N, list, cnt, w.sigma, w.essence, w.grad, st, fcnt);
        if (audit) dsn_launch_screen_audit(w.audit, w.count + DSN_CNT_AUDIT, w.audit_cap, w.sigma, w.count + DSN_CNT_AUDIT + 4, st);
    } else {
        dsn_launch_field16((const float*)packed, s.frame, w.x_c, N, list, cnt, w.sigma, w.essence, w.grad, st);
        dsn_launch_field_fix((const float*)packed, s.frame, w.x_c, N, list, cnt, w.sigma, w.essence, w.grad, st);
    }
    }       // field phase
    // the list the shading kernels walk (what the field phase leaves; recomputed here so that a DSN_PHASE_SHADE call finds it)
    if (!(flags & DSN_FIELD_FP32) && skip) {
        if (flags & DSN_EARLY_STOP) { list = w.slices; cnt = w.count + DSN_CNT_LIT; }
        else { list = w.pos; cnt = w.count + DSN_CNT_POS; }
    }
    if (do_shade && sweep) {
    // Relighting sweep: the normals once, then per group of G lights the lighting MLP (k_light16_multi: colours by list slot in the
    // caller's scratch) and the compositor (k_composite16_multi: weights once per ray, then every light's sums).  The shading list's
    // length sizes G: one 4-byte read of its count word (the only synchronisation of the call).
    int32_t n_sh = 0;
    if (hipMemcpyAsync(&n_sh, cnt, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return dsn_fail("%s", "dsn_render_rays_lights: reading the shading list's length failed");
    // (maps: the light factors [G][n_shaded] behind the group's colours - 4 floats per shaded sample and light)
    const DsnMapsOut* const maps = sweep->maps;
    const char* const who = maps ? "dsn_render_rays_maps" : "dsn_render_rays_lights";
    const size_t per_light = sizeof(float) * (maps ? 4 : 3) * (size_t)n_sh;
    const int G = per_light == 0 ? sweep->n_lights : (int)std::min<size_t>((size_t)sweep->n_lights, sweep->scratch_bytes / per_light);
    if (G < 1)
        return maps ? dsn_fail("dsn_render_rays_maps: light_scratch is too small%s: one light's colours and factors need %lld bytes "
                               "(dsn_render_maps_scratch_bytes)", "", (long long)per_light)
                    : dsn_fail("dsn_render_rays_lights: light_scratch is too small%s: one light's colours need %lld bytes "
                               "(dsn_render_lights_scratch_bytes)", "", (long long)per_light);
    // the slot map takes the slice-filter list's buffer: dead after the field phase on both eval paths (early stop: its last
    // reader is the reverse pass's selection; one pass: never used)
    int32_t* slot = w.alive;
    if (!dsn_composite_multi_supported(S, z, w.sigma, out_weights, slot, w.transparent))
        return dsn_fail("%s", "dsn_render_rays_lights: unaligned arrays for the 16-lane compositor");
    dsn_launch_normal(s, w.x_c, w.grad, N, list, cnt, nullptr, w.n_w, exh, st);
    if (hipMemsetAsync(slot, 0xff, sizeof(int32_t) * (size_t)N, st) != hipSuccess)
        return dsn_fail("%s", "dsn_render_rays_lights: memset failed");
    dsn_launch_slot_map(list, cnt, n_sh, slot, st);
    float* colours = (float*)sweep->scratch;
    // Decomposition maps: the sweep's passes as they are - the lighting kernel also keeps its factor by slot, and the compositor
    // (k_composite16_maps: k_composite16_multi's sums, same bits) weighs the essence, the normal and the factors too.  The essence
    // array is still intact here (the sweep's colours live in the caller's scratch; on the one-light path the colour overwrites it).
    // Albedo, normal and the two maxima are written by the first group only, like disp / acc / depth / weights.
    if (maps && maps->max2 && hipMemsetAsync(maps->max2, 0, 2 * sizeof(float), st) != hipSuccess)
        return dsn_fail("%s", "dsn_render_rays_maps: memset failed");
    for (int g0 = 0; g0 < sweep->n_lights; g0 += G) {
        const int Gc = std::min(G, sweep->n_lights - g0);
        const bool first = g0 == 0;      // (the per-ray outputs that do not depend on the light: written once)
        if (maps) {
            float* factors = colours + (size_t)G * 3 * (size_t)n_sh;
            dsn_launch_light16_multi((const float*)packed, sweep->lights + g0, Gc, w.n_w, ray_o, ray_d, z,
                                     w.essence, n_sh, S, list, cnt, colours, st, factors);
            DsnMapsArgs a = {};
            a.slot_of = slot; a.colours = colours; a.factors = factors; a.n_shaded = n_sh; a.G = Gc;
            a.essence = w.essence; a.n_w = w.n_w; a.sigma = w.sigma; a.transparent = w.transparent; a.z_vals = z; a.ray_d = ray_d;
            a.R = R; a.S = S;
            a.rgb_maps = out_rgb ? out_rgb + (size_t)g0 * 3 * R : nullptr;
            a.shading_maps = maps->shading ? maps->shading + (size_t)g0 * R : nullptr;
            if (first) {
                a.albedo_map = maps->albedo; a.normal_map = maps->normal;
                a.disp_map = out_disp; a.acc_map = out_acc; a.weights = out_weights; a.depth_map = out_depth;
            }
            // (the largest factor is a maximum over every group; the largest |essence| is the same in all of them)
            a.maps_max = (int32_t*)maps->max2;
            a.colour_max = w.count + DSN_CNT_STOP + 3;
            dsn_launch_composite_maps(a, st);
            continue;
        }
        dsn_launch_light16_multi((const float*)packed, sweep->lights + g0, Gc, w.n_w, ray_o, ray_d, z,
                                 w.essence, n_sh, S, list, cnt, colours, st);
        dsn_launch_composite_multi(slot, colours, n_sh, Gc, w.sigma, w.transparent, z, ray_d, R, S, out_rgb + (size_t)g0 * 3 * R,
                                   first ? out_disp : nullptr, first ? out_acc : nullptr, first ? out_weights : nullptr,
                                   first ? out_depth : nullptr, w.count + DSN_CNT_STOP + 3, st);
    }
    if (flags & DSN_STOP_STATS)
        dsn_launch_stop_stats(w.sigma, w.transparent, z, ray_d, R, S, dsn_stats_slice_len(R, S), (const float*)packed + OFF_SCAL,
                              w.count + DSN_CNT_STOP + 2, st, w.count + DSN_CNT_HIST, w.count + DSN_CNT_STOP + 3, dsn_slice_len(R, S));
    return dsn_check_launch(who);
    }
    if (do_shade) {
    dsn_launch_normal(s, w.x_c, w.grad, N, list, cnt, nullptr, w.n_w, exh, st);
    if (flags & DSN_FIELD_FP32)
        dsn_launch_light((const float*)packed, s.frame, w.n_w, nullptr, ray_o, ray_d, z, w.essence, N, S, list, cnt, w.colour, st);
    else
        dsn_launch_light16((const float*)packed, s.frame, w.n_w, nullptr, ray_o, ray_d, z, w.essence, N, S, list, cnt, w.colour, st);
    dsn_launch_composite(w.colour, w.sigma, w.transparent, z, ray_d, noise, R, S, out_rgb, out_disp, out_acc,
                         out_weights, out_depth, st, skip, skip ? w.count + DSN_CNT_STOP + 3 : nullptr);
    if ((flags & DSN_STOP_STATS) && skip)
        dsn_launch_stop_stats(w.sigma, w.transparent, z, ray_d, R, S, dsn_stats_slice_len(R, S), (const float*)packed + OFF_SCAL,
                              w.count + DSN_CNT_STOP + 2, st, w.count + DSN_CNT_HIST, w.count + DSN_CNT_STOP + 3, dsn_slice_len(R, S));
    }       // shading phase
    return dsn_check_launch("dsn_render_rays");
}

int dsn_render_rays_train_ex(const void* scene, int V, int F, const void* packed, const float* ray_o, const float* ray_d, float* near,
                          float* far, int R, int S, const float* t_vals, const float* jitter, const float* noise, int flags,
                          float* out_rgb, float* out_disp, float* out_acc, float* out_depth, float* out_weights, float* out_z,
                          void* workspace, void* grad_workspace, void* stream, void* aux_stream, void* ev_fork, void* ev_join) {
    DSN_REQUIRE(R > 0 && S > 0, "dsn_render_rays_train: empty ray batch");
    DSN_REQUIRE(scene && packed && ray_o && ray_d && near && far && t_vals && workspace && grad_workspace,
                "dsn_render_rays_train: null argument");
    DSN_REQUIRE(out_rgb && out_disp && out_acc && out_depth, "dsn_render_rays_train: null output");
    DSN_REQUIRE(V > 0 && F > 0, "dsn_render_rays_train: bad V/F");
    DSN_REQUIRE(!(flags & (DSN_SKIP_TRANSPARENT | DSN_FIELD_FP32)), "dsn_render_rays_train: dense split-fp16 evaluation only");
    DSN_REQUIRE((aux_stream != nullptr) == (ev_fork != nullptr) && (aux_stream != nullptr) == (ev_join != nullptr),
                "dsn_render_rays_train_ex: the auxiliary stream and its two events go together");
    DSN_REQUIRE(!aux_stream || aux_stream != stream, "dsn_render_rays_train_ex: the auxiliary stream must not be the call's own stream");
    hipStream_t st = (hipStream_t)stream;
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    DsnWorkspace w = dsn_carve(workspace, R, S, -1);      // (train mode keeps its records in grad_workspace: the fixed part only)
    const int64_t N = (int64_t)R * S;
    const DsnTrainCache c = dsn_train_cache(grad_workspace, N);
    float* z = out_z ? out_z : w.z;
    const bool exh = (flags & DSN_NN_EXHAUSTIVE) != 0;
    // Geometry.  Round 6: batches of DSN_TRAIN_CELLMAJOR_MIN samples or more take the eval frames' fused path - the sampler classifies
    // the samples by fine cell, the cell-major search + warp run behind it (same index, same x_c, bit for bit: dsn_nn.hip) - and with
    // DSN_LAZY_LISTS on a lazily set frame (DSN_FRAME_LAZY_LISTS) the posed mesh's lists are built for the cells the batch visits
    // only: the per-step list build of every cell (0.48 ms of an 11.6 ms step at 8192 x 64) and the per-lane list walk of k_warp
    // (0.18 ms) were the two largest non-matrix items of the step.  Smaller batches: k_warp on every cell's lists (a lazily set
    // frame is completed first).  Every sample is warped (transparent samples with positive noise are evaluated: no lazy_canon).
    static const long long train_cm_min = [] { const char* e = getenv("DSN_TRAIN_CELLMAJOR_MIN"); return e ? atoll(e) : (long long)DSN_TRAIN_CELLMAJOR_MIN; }();
    const bool lazy = (flags & DSN_LAZY_LISTS) != 0;
    const bool fused = !exh && N >= (int64_t)train_cm_min && !getenv("DSN_NN_UNFUSED");
    if (lazy && !fused) dsn_launch_build_nn_complete(s.cent_world, F, s.nn_world, st);
    if (fused) {
        int32_t *counts = nullptr, *outside0 = nullptr, *outside = nullptr;
        int32_t* g3 = (int32_t*)w.grad;      // scratch: cells (4 N) | ranks (4 N) | sorted records (16 N) across G and E, as in dsn_render_rays_ex
        dsn_nn_cellmajor_begin(w.nn_small, &counts, &outside0, st);
        dsn_launch_sample_gg(s.xyz, (flags & DSN_SAMPLE_UNIFORM) ? 0 : V, ray_o, ray_d, near, far, R, S, t_vals, jitter, z, nullptr, st,
                             s.nn_world.fine.g, g3, counts, outside0, g3 + N);
        if (lazy) dsn_launch_build_nn_visited(s.cent_world, F, s.nn_world, counts, st);
        dsn_launch_nn_cellmajor_warp(s.nn_world, ray_o, ray_d, z, N, S, g3, w.sort_scratch, w.nn_small, s.face_world, s.face_canon,
                                     c.transparent, c.x_c, nullptr, nullptr, false, &outside, st, true, lazy);
        dsn_launch_warp(s, nullptr, ray_o, ray_d, z, N, S, nullptr, nullptr, nullptr, c.transparent, c.x_c, nullptr, nullptr, nullptr, exh, st,
                        nullptr, false, g3, outside);
    } else {
        dsn_launch_sample_gg(s.xyz, (flags & DSN_SAMPLE_UNIFORM) ? 0 : V, ray_o, ray_d, near, far, R, S, t_vals, jitter, z, nullptr, st);
        dsn_launch_warp(s, nullptr, ray_o, ray_d, z, N, S, nullptr, nullptr, nullptr, c.transparent, c.x_c, nullptr, nullptr, nullptr, exh, st);
    }
    // Rows the step evaluates: a transparent sample has its density forced to 0 (can_render.py:115-120), so with noise <= 0 its
    // alpha is exactly 0 (utils/nerf_net_utils.py:30-36: relu(0 + noise) = 0): neither its colour nor its density reaches an
    // output or receives a gradient.  Everything else - transparent samples with positive noise included, their colour is
    // weighted - goes through the networks.  (~30 % of a batch is skipped with raw_noise_std > 0, every transparent sample without.)
    dsn_train_forward_rows(c.transparent, noise, N, c.live, c.bcnt, c.list1, c.rowcnt, st);
    // (train mode has no exact-fp32 twin of the stored activations: samples outside the fp16 range are counted in count[48],
    //  which the host mirror checks - Renderer.range_overflow_count())
    if (hipMemsetAsync(w.count, 0, DSN_CNT_BYTES, st) != hipSuccess) return dsn_fail("%s", "dsn_render_rays_train: memset failed");
    // The canonical points of transparent samples (evaluated when their noise is positive) lie far from the body, outside the fine
    // grid: the coarse-level cell-major search finds their nearest face first (same lists, same index as k_normal's own walk;
    // scratch: buffers of the render workspace that train mode does not use) and k_normal takes it from there.  It reads the warp
    // stage's points and the row flags, nothing of the networks: with the caller's auxiliary stream (dsn_render_rays_train_ex) it is
    // enqueued BESIDE the field kernel - whose last round of row blocks leaves most compute units idle - and joined in front of the
    // normals; without one it follows the field kernel on `stream` as before.  (The matrix kernel owns its SIMDs, DESIGN 4.5: the
    // search's waves only ever run on compute units that hold none of its workgroups.)
    const int32_t* nn_far = nullptr;
    const char* far_env = getenv("DSN_TRAIN_FAR_SEARCH_MIN");      // test / tuning override (a huge value switches it off)
    const bool far_search = !exh && N >= (far_env ? atoll(far_env) : (long long)DSN_TRAIN_FAR_SEARCH_MIN);
    hipStream_t sf = st;
    const bool forked = far_search && aux_stream != nullptr;
    if (forked) {
        sf = (hipStream_t)aux_stream;
        if (hipEventRecord((hipEvent_t)ev_fork, st) != hipSuccess || hipStreamWaitEvent(sf, (hipEvent_t)ev_fork, 0) != hipSuccess)
            return dsn_fail("%s", "dsn_render_rays_train_ex: fork of the auxiliary stream failed");
    }
    auto search_far = [&]() {
        // (scratch of the segmented search, round 6: buffers the training forward does not use - the per-slice lists + the live list,
        //  8 N contiguous bytes, for the (distance, index) keys; the active list for the wave -> cell map and the scatter cursors)
        dsn_launch_nn_cellmajor_coarse(s.nn_canon, s.cent_canon, c.x_c, c.live, N, (int32_t*)w.grad, w.sort_scratch, w.pos, w.nn_small, sf,
                                       (void*)w.slices, F, w.active, N);
        nn_far = w.pos;
    };
    if (forked) search_far();
    // (skipped rows keep whatever their density slot held: the compositor masks transparent samples itself)
    dsn_launch_field16_train((const float*)packed, s.frame, c.x_c, N, c.sigma, c.essence, c.grad, c.h0, c.a0, c.rr, c.masks, st,
                             w.count + DSN_CNT_RANGE, c.list1, c.rowcnt);
    if (forked) {
        if (hipEventRecord((hipEvent_t)ev_join, sf) != hipSuccess || hipStreamWaitEvent(st, (hipEvent_t)ev_join, 0) != hipSuccess)
            return dsn_fail("%s", "dsn_render_rays_train_ex: join of the auxiliary stream failed");
    } else if (far_search) search_far();
    dsn_launch_normal(s, c.x_c, c.grad, N, c.list1, c.rowcnt, c.idx_c, c.n_w, exh, st, nn_far);
    dsn_launch_light16((const float*)packed, s.frame, c.n_w, nullptr, ray_o, ray_d, z, c.essence, N, S, c.list1, c.rowcnt, w.colour, st,
                       c.hl1, c.hl2, c.pre, w.count + DSN_CNT_RANGE);
    // (a colour is read only where relu(density + noise) > 0: skipped rows never are)
    dsn_launch_composite(w.colour, c.sigma, c.transparent, z, ray_d, noise, R, S, out_rgb, out_disp, out_acc, out_weights,
                         out_depth, st, true);
    return dsn_check_launch("dsn_render_rays_train");
}

int dsn_render_rays_train(const void* scene, int V, int F, const void* packed, const float* ray_o, const float* ray_d, float* near,
                          float* far, int R, int S, const float* t_vals, const float* jitter, const float* noise, int flags,
                          float* out_rgb, float* out_disp, float* out_acc, float* out_depth, float* out_weights, float* out_z,
                          void* workspace, void* grad_workspace, void* stream) {
    return dsn_render_rays_train_ex(scene, V, F, packed, ray_o, ray_d, near, far, R, S, t_vals, jitter, noise, flags, out_rgb, out_disp, out_acc,
                                    out_depth, out_weights, out_z, workspace, grad_workspace, stream, nullptr, nullptr, nullptr);
}

// ---- density grid + marching cubes (utils/visualizer.py Visualizer3D) ----
// density-grid scratch of a slab of P points: points 12 P | canonical points 12 P | active list 4 P | counters (256 B)
static size_t dsn_grid_ws(int64_t P) { return 2 * dsn_align256(12 * (size_t)P) + dsn_align256(4 * (size_t)P) + 256; }

size_t dsn_density_grid_workspace_bytes(int64_t slab_points) {
    return slab_points > 0 && slab_points < ((int64_t)1 << 31) ? dsn_grid_ws(slab_points) : 0;
}

int dsn_density_grid(const void* scene, int V, int F, const void* packed, const float* x, int nx, const float* y, int ny, const float* z,
                     int nz, int flags, float* volume, int64_t slab_points, void* workspace, size_t workspace_bytes, void* stream) {
    DSN_REQUIRE(scene && packed && x && y && z && volume && workspace, "dsn_density_grid: null argument");
    DSN_REQUIRE(V > 0 && F > 0, "dsn_density_grid: bad V/F");
    DSN_REQUIRE(nx > 0 && ny > 0 && nz > 0, "dsn_density_grid: empty grid axis");
    const int64_t plane = (int64_t)ny * nz, N = plane * nx;
    DSN_REQUIRE(N < ((int64_t)1 << 31), "dsn_density_grid: more than 2^31 - 1 grid points");
    DSN_REQUIRE(slab_points >= plane && slab_points < ((int64_t)1 << 31), "dsn_density_grid: slab_points must hold at least one x-plane (ny * nz points)");
    DSN_REQUIRE(workspace_bytes >= dsn_grid_ws(slab_points), "dsn_density_grid: workspace smaller than dsn_density_grid_workspace_bytes(slab_points)");
    DSN_REQUIRE((flags & ~(DSN_FIELD_FP32 | DSN_NN_EXHAUSTIVE)) == 0, "dsn_density_grid: flags other than DSN_FIELD_FP32 / DSN_NN_EXHAUSTIVE");
    hipStream_t st = (hipStream_t)stream;
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    char* p = (char*)workspace;
    float* pts = (float*)p;                      p += dsn_align256(12 * (size_t)slab_points);
    float* x_c = (float*)p;                      p += dsn_align256(12 * (size_t)slab_points);
    int32_t* list = (int32_t*)p;                 p += dsn_align256(4 * (size_t)slab_points);
    int32_t* cnt = (int32_t*)p;                  // [0] active points of the slab, [16] samples the split-fp16 kernel flagged
    const int per = (int)(slab_points / plane);
    for (int i0 = 0; i0 < nx; i0 += per) {
        const int np = nx - i0 < per ? nx - i0 : per;
        const int64_t Ns = (int64_t)np * plane;
        float* vs = volume + (int64_t)i0 * plane;
        if (hipMemsetAsync(cnt, 0, 256, st) != hipSuccess || hipMemsetAsync(vs, 0, sizeof(float) * (size_t)Ns, st) != hipSuccess)
            return dsn_fail("%s", "dsn_density_grid: memset failed");
        dsn_launch_grid_points(x, y, z, i0, ny, nz, Ns, pts, st);
        // utils/render_utils.py w2l_without_lbs: dsn_warp's kernel (transparent points stay off the list and keep density 0)
        dsn_launch_warp(s, pts, nullptr, nullptr, nullptr, Ns, 1, nullptr, nullptr, nullptr, nullptr, x_c, nullptr, list, cnt,
                        (flags & DSN_NN_EXHAUSTIVE) != 0, st);
        if (flags & DSN_FIELD_FP32)
            dsn_launch_field((const float*)packed, s.frame, x_c, Ns, list, cnt, vs, nullptr, nullptr, st);
        else {
            dsn_launch_field16_den((const float*)packed, s.frame, x_c, Ns, list, cnt, vs, st, cnt + 16);
            dsn_launch_field_fix((const float*)packed, s.frame, x_c, Ns, list, cnt, vs, nullptr, nullptr, st, cnt + 16);
        }
    }
    return dsn_check_launch("dsn_density_grid");
}

static bool dsn_mc_sizes_ok(int nx, int ny, int nz) {
    return nx >= 2 && ny >= 2 && nz >= 2 && (int64_t)nx * ny * nz < ((int64_t)1 << 31);
}

size_t dsn_mc_workspace_bytes(int nx, int ny, int nz) {
    return dsn_mc_sizes_ok(nx, ny, nz) ? dsn_mc_workspace_size((int64_t)nx * ny * nz) : 0;
}

int dsn_mc_count(const float* volume, int nx, int ny, int nz, float level, void* workspace, int64_t* out_counts2, void* stream) {
    DSN_REQUIRE(volume && workspace && out_counts2, "dsn_mc_count: null argument");
    DSN_REQUIRE(dsn_mc_sizes_ok(nx, ny, nz), "dsn_mc_count: bad grid size (every axis >= 2, fewer than 2^31 points)");
    DSN_REQUIRE(level == level, "dsn_mc_count: NaN level");
    dsn_launch_mc_count(volume, nx, ny, nz, level, workspace, out_counts2, (hipStream_t)stream);
    return dsn_check_launch("dsn_mc_count");
}

int dsn_mc_emit(const float* volume, int nx, int ny, int nz, const float* x, const float* y, const float* z, float level,
                int gradient_direction, const void* workspace, int64_t n_verts, int64_t n_faces, float* verts, int32_t* faces,
                void* stream) {
    DSN_REQUIRE(volume && x && y && z && workspace, "dsn_mc_emit: null argument");
    DSN_REQUIRE(dsn_mc_sizes_ok(nx, ny, nz), "dsn_mc_emit: bad grid size (every axis >= 2, fewer than 2^31 points)");
    DSN_REQUIRE(level == level, "dsn_mc_emit: NaN level");
    DSN_REQUIRE(gradient_direction == DSN_MC_DESCENT || gradient_direction == DSN_MC_ASCENT, "dsn_mc_emit: gradient_direction must be DSN_MC_DESCENT or DSN_MC_ASCENT");
    DSN_REQUIRE(n_verts >= 0 && n_faces >= 0, "dsn_mc_emit: negative count");
    DSN_REQUIRE(n_verts < ((int64_t)1 << 31), "dsn_mc_emit: 2^31 or more vertices do not fit int32 face indices");
    DSN_REQUIRE((n_verts == 0 || verts) && (n_faces == 0 || faces), "dsn_mc_emit: null output buffer");
    if (n_verts == 0 && n_faces == 0) return 0;
    dsn_launch_mc_emit(volume, nx, ny, nz, x, y, z, level, gradient_direction == DSN_MC_ASCENT, workspace, verts, n_verts, faces, n_faces,
                       (hipStream_t)stream);
    return dsn_check_launch("dsn_mc_emit");
}

int dsn_mc_normals(const float* volume, int nx, int ny, int nz, const float* x, const float* y, const float* z, float level,
                   int gradient_direction, const void* workspace, int64_t n_verts, float* normals, void* stream) {
    DSN_REQUIRE(volume && x && y && z && workspace, "dsn_mc_normals: null argument");
    DSN_REQUIRE(dsn_mc_sizes_ok(nx, ny, nz), "dsn_mc_normals: bad grid size (every axis >= 2, fewer than 2^31 points)");
    DSN_REQUIRE(level == level, "dsn_mc_normals: NaN level");
    DSN_REQUIRE(gradient_direction == DSN_MC_DESCENT || gradient_direction == DSN_MC_ASCENT, "dsn_mc_normals: gradient_direction must be DSN_MC_DESCENT or DSN_MC_ASCENT");
    DSN_REQUIRE(n_verts >= 0, "dsn_mc_normals: negative count");
    DSN_REQUIRE(n_verts == 0 || normals, "dsn_mc_normals: null output buffer");
    if (n_verts == 0) return 0;
    dsn_launch_mc_normals(volume, nx, ny, nz, x, y, z, level, gradient_direction == DSN_MC_ASCENT, workspace, normals, n_verts,
                          (hipStream_t)stream);
    return dsn_check_launch("dsn_mc_normals");
}

int dsn_mc_table_host(int32_t* out_host, size_t out_ints) {
    DSN_REQUIRE(out_host, "dsn_mc_table_host: null argument");
    DSN_REQUIRE(out_ints >= (size_t)256 * DSN_MC_TABLE_ROW, "dsn_mc_table_host: out_host holds fewer than 256 * DSN_MC_TABLE_ROW ints");
    dsn_mc_table_copy(out_host);
    return 0;
}

// ---- density grid, coarse to fine (the rule of include/dsnerf.h) ----
static int dsn_hier_shift(int factor) { return factor == 2 ? 1 : factor == 4 ? 2 : factor == 8 ? 3 : factor == 16 ? 4 : -1; }

size_t dsn_grid_hier_workspace_bytes(int nx, int ny, int nz, int factor) {
    return dsn_mc_sizes_ok(nx, ny, nz) && dsn_hier_shift(factor) > 0 ? dsn_grid_hier_workspace_size(nx, ny, nz, dsn_hier_shift(factor)) : 0;
}

static bool dsn_hier_coarse_ok(int nx, int ny, int nz, int sh, int mx, int my, int mz) {
    int m[3];
    dsn_grid_hier_coarse_shape(nx, ny, nz, sh, m);
    return m[0] == mx && m[1] == my && m[2] == mz;
}

int dsn_grid_hier_mark(const float* coarse, int mx, int my, int mz, int nx, int ny, int nz, int factor, int dilate, float level,
                       void* workspace, size_t workspace_bytes, int64_t* out_counts3, void* stream) {
    DSN_REQUIRE(coarse && workspace && out_counts3, "dsn_grid_hier_mark: null argument");
    DSN_REQUIRE(dsn_mc_sizes_ok(nx, ny, nz), "dsn_grid_hier_mark: bad grid size (every axis >= 2, fewer than 2^31 points)");
    const int sh = dsn_hier_shift(factor);
    DSN_REQUIRE(sh > 0, "dsn_grid_hier_mark: factor must be 2, 4, 8 or 16");
    DSN_REQUIRE(dilate >= 0, "dsn_grid_hier_mark: negative dilate");
    DSN_REQUIRE(level == level, "dsn_grid_hier_mark: NaN level");
    DSN_REQUIRE(dsn_hier_coarse_ok(nx, ny, nz, sh, mx, my, mz), "dsn_grid_hier_mark: coarse shape is not the grid's coarse lattice (ceil((n - 1) / factor) + 1 per axis)");
    DSN_REQUIRE(workspace_bytes >= dsn_grid_hier_workspace_size(nx, ny, nz, sh), "dsn_grid_hier_mark: workspace smaller than dsn_grid_hier_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out_counts3, 0, 3 * sizeof(int64_t), st) != hipSuccess) return dsn_fail("%s", "dsn_grid_hier_mark: memset failed");
    dsn_launch_grid_hier_mark(coarse, nx, ny, nz, sh, dilate, level, workspace, out_counts3, st);
    return dsn_check_launch("dsn_grid_hier_mark");
}

int dsn_grid_hier_list(int nx, int ny, int nz, int factor, const void* workspace, size_t workspace_bytes, int64_t n_points,
                       int32_t* point_index, void* stream) {
    DSN_REQUIRE(workspace, "dsn_grid_hier_list: null argument");
    DSN_REQUIRE(dsn_mc_sizes_ok(nx, ny, nz), "dsn_grid_hier_list: bad grid size (every axis >= 2, fewer than 2^31 points)");
    const int sh = dsn_hier_shift(factor);
    DSN_REQUIRE(sh > 0, "dsn_grid_hier_list: factor must be 2, 4, 8 or 16");
    DSN_REQUIRE(n_points >= 0 && n_points <= (int64_t)nx * ny * nz, "dsn_grid_hier_list: n_points outside 0 .. nx ny nz");
    DSN_REQUIRE(n_points == 0 || point_index, "dsn_grid_hier_list: null output buffer");
    DSN_REQUIRE(workspace_bytes >= dsn_grid_hier_workspace_size(nx, ny, nz, sh), "dsn_grid_hier_list: workspace smaller than dsn_grid_hier_workspace_bytes");
    if (n_points == 0) return 0;
    dsn_launch_grid_hier_list(nx, ny, nz, sh, workspace, point_index, n_points, (hipStream_t)stream);
    return dsn_check_launch("dsn_grid_hier_list");
}

int dsn_grid_hier_assemble(const float* coarse, int mx, int my, int mz, int nx, int ny, int nz, int factor, float level,
                           const void* workspace, size_t workspace_bytes, const int32_t* point_index, const float* values, int64_t n_points,
                           float* volume, int64_t* out_leaks, void* stream) {
    DSN_REQUIRE(coarse && workspace && volume && out_leaks, "dsn_grid_hier_assemble: null argument");
    DSN_REQUIRE(dsn_mc_sizes_ok(nx, ny, nz), "dsn_grid_hier_assemble: bad grid size (every axis >= 2, fewer than 2^31 points)");
    const int sh = dsn_hier_shift(factor);
    DSN_REQUIRE(sh > 0, "dsn_grid_hier_assemble: factor must be 2, 4, 8 or 16");
    DSN_REQUIRE(level == level, "dsn_grid_hier_assemble: NaN level");
    DSN_REQUIRE(dsn_hier_coarse_ok(nx, ny, nz, sh, mx, my, mz), "dsn_grid_hier_assemble: coarse shape is not the grid's coarse lattice (ceil((n - 1) / factor) + 1 per axis)");
    DSN_REQUIRE(n_points >= 0 && n_points <= (int64_t)nx * ny * nz, "dsn_grid_hier_assemble: n_points outside 0 .. nx ny nz");
    DSN_REQUIRE(n_points == 0 || (point_index && values), "dsn_grid_hier_assemble: null point list");
    DSN_REQUIRE(workspace_bytes >= dsn_grid_hier_workspace_size(nx, ny, nz, sh), "dsn_grid_hier_assemble: workspace smaller than dsn_grid_hier_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out_leaks, 0, sizeof(int64_t), st) != hipSuccess) return dsn_fail("%s", "dsn_grid_hier_assemble: memset failed");
    dsn_launch_grid_hier_assemble(coarse, nx, ny, nz, sh, level, workspace, point_index, values, n_points, volume, out_leaks, st);
    return dsn_check_launch("dsn_grid_hier_assemble");
}

size_t dsn_density_points_workspace_bytes(int64_t slab_points) {
    return slab_points > 0 && slab_points < ((int64_t)1 << 31) ? dsn_grid_ws(slab_points) : 0;
}

// dsn_density_grid's slab loop over a list of grid points instead of whole x-planes: the same warp and field launches
int dsn_density_points(const void* scene, int V, int F, const void* packed, const float* x, int nx, const float* y, int ny, const float* z,
                       int nz, const int32_t* point_index, int64_t n_points, int flags, float* values, int64_t slab_points, void* workspace,
                       size_t workspace_bytes, void* stream) {
    DSN_REQUIRE(scene && packed && x && y && z && workspace, "dsn_density_points: null argument");
    DSN_REQUIRE(V > 0 && F > 0, "dsn_density_points: bad V/F");
    DSN_REQUIRE(nx > 0 && ny > 0 && nz > 0, "dsn_density_points: empty grid axis");
    const int64_t N = (int64_t)nx * ny * nz;
    DSN_REQUIRE(N < ((int64_t)1 << 31), "dsn_density_points: more than 2^31 - 1 grid points");
    DSN_REQUIRE(n_points >= 0, "dsn_density_points: negative n_points");
    DSN_REQUIRE(n_points == 0 || (point_index && values), "dsn_density_points: null point list");
    DSN_REQUIRE(slab_points >= 1 && slab_points < ((int64_t)1 << 31), "dsn_density_points: slab_points must be 1 .. 2^31 - 1");
    DSN_REQUIRE(workspace_bytes >= dsn_grid_ws(slab_points), "dsn_density_points: workspace smaller than dsn_density_points_workspace_bytes(slab_points)");
    DSN_REQUIRE((flags & ~(DSN_FIELD_FP32 | DSN_NN_EXHAUSTIVE)) == 0, "dsn_density_points: flags other than DSN_FIELD_FP32 / DSN_NN_EXHAUSTIVE");
    hipStream_t st = (hipStream_t)stream;
    DsnSceneView s = dsn_scene_view((void*)scene, V, F);
    char* p = (char*)workspace;
    float* pts = (float*)p;                      p += dsn_align256(12 * (size_t)slab_points);
    float* x_c = (float*)p;                      p += dsn_align256(12 * (size_t)slab_points);
    int32_t* list = (int32_t*)p;                 p += dsn_align256(4 * (size_t)slab_points);
    int32_t* cnt = (int32_t*)p;                  // [0] active points of the slab, [16] samples the split-fp16 kernel flagged
    for (int64_t m0 = 0; m0 < n_points; m0 += slab_points) {
        const int64_t Ns = n_points - m0 < slab_points ? n_points - m0 : slab_points;
        float* vs = values + m0;
        if (hipMemsetAsync(cnt, 0, 256, st) != hipSuccess || hipMemsetAsync(vs, 0, sizeof(float) * (size_t)Ns, st) != hipSuccess)
            return dsn_fail("%s", "dsn_density_points: memset failed");
        dsn_launch_list_points(x, y, z, point_index + m0, ny, nz, N, Ns, pts, st);
        dsn_launch_warp(s, pts, nullptr, nullptr, nullptr, Ns, 1, nullptr, nullptr, nullptr, nullptr, x_c, nullptr, list, cnt,
                        (flags & DSN_NN_EXHAUSTIVE) != 0, st);
        if (flags & DSN_FIELD_FP32)
            dsn_launch_field((const float*)packed, s.frame, x_c, Ns, list, cnt, vs, nullptr, nullptr, st);
        else {
            dsn_launch_field16_den((const float*)packed, s.frame, x_c, Ns, list, cnt, vs, st, cnt + 16);
            dsn_launch_field_fix((const float*)packed, s.frame, x_c, Ns, list, cnt, vs, nullptr, nullptr, st, cnt + 16);
        }
        dsn_launch_points_invalid(point_index + m0, N, Ns, vs, st);
    }
    return dsn_check_launch("dsn_density_points");
}

static bool dsn_mesh_cc_sizes_ok(int64_t V, int64_t T) { return V >= 0 && T >= 0 && V < ((int64_t)1 << 31) && T < ((int64_t)1 << 31); }

size_t dsn_mesh_cc_workspace_bytes(int64_t n_verts, int64_t n_faces) {
    return dsn_mesh_cc_sizes_ok(n_verts, n_faces) ? dsn_mesh_cc_workspace_size(n_verts, n_faces) : 0;
}

int dsn_mesh_cc_label_ex(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, int area_shift, void* workspace,
                         size_t workspace_bytes, int32_t* labels_v, int64_t* out_counts6, int phases, void* stream) {
    DSN_REQUIRE(n_verts >= 0 && n_faces >= 0, "dsn_mesh_cc_label: negative count");
    DSN_REQUIRE(dsn_mesh_cc_sizes_ok(n_verts, n_faces), "dsn_mesh_cc_label: 2^31 or more vertices or faces");
    DSN_REQUIRE((n_verts == 0 || verts) && (n_faces == 0 || faces), "dsn_mesh_cc_label: null mesh");
    DSN_REQUIRE(workspace && out_counts6, "dsn_mesh_cc_label: null argument");
    DSN_REQUIRE(workspace_bytes >= dsn_mesh_cc_workspace_size(n_verts, n_faces), "dsn_mesh_cc_label: workspace_bytes too small (dsn_mesh_cc_workspace_bytes)");
    DSN_REQUIRE(((uintptr_t)workspace & 15) == 0, "dsn_mesh_cc_label: workspace must be 16-byte aligned");
    DSN_REQUIRE(area_shift >= -60 && area_shift <= 60, "dsn_mesh_cc_label: area_shift must be -60 ... 60");
    DSN_REQUIRE(phases >= 0 && phases < 256, "dsn_mesh_cc_label_ex: bad phases");
    dsn_launch_mesh_cc_label(verts, faces, n_verts, n_faces, std::ldexp(1.0, area_shift), workspace, labels_v, out_counts6,
                             phases ? phases : 255, (hipStream_t)stream);
    return dsn_check_launch("dsn_mesh_cc_label");
}

int dsn_mesh_cc_label(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, int area_shift, void* workspace,
                      size_t workspace_bytes, int32_t* labels_v, int64_t* out_counts6, void* stream) {
    return dsn_mesh_cc_label_ex(verts, faces, n_verts, n_faces, area_shift, workspace, workspace_bytes, labels_v, out_counts6, 0, stream);
}

int dsn_mesh_cc_emit_ex(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, void* workspace, size_t workspace_bytes,
                        int64_t out_n_verts, int64_t out_n_faces, float* out_verts, int32_t* out_faces, int32_t* source_vertex, int phases,
                        void* stream) {
    DSN_REQUIRE(n_verts >= 0 && n_faces >= 0 && out_n_verts >= 0 && out_n_faces >= 0, "dsn_mesh_cc_emit: negative count");
    DSN_REQUIRE(dsn_mesh_cc_sizes_ok(n_verts, n_faces), "dsn_mesh_cc_emit: 2^31 or more vertices or faces");
    DSN_REQUIRE(out_n_verts <= n_verts && out_n_faces <= n_faces, "dsn_mesh_cc_emit: more kept vertices or faces than the mesh has");
    DSN_REQUIRE((n_verts == 0 || verts) && (n_faces == 0 || faces), "dsn_mesh_cc_emit: null mesh");
    DSN_REQUIRE(workspace, "dsn_mesh_cc_emit: null argument");
    DSN_REQUIRE((out_n_verts == 0 || out_verts) && (out_n_faces == 0 || out_faces), "dsn_mesh_cc_emit: null output buffer");
    DSN_REQUIRE(workspace_bytes >= dsn_mesh_cc_workspace_size(n_verts, n_faces), "dsn_mesh_cc_emit: workspace_bytes too small (dsn_mesh_cc_workspace_bytes)");
    DSN_REQUIRE(((uintptr_t)workspace & 15) == 0, "dsn_mesh_cc_emit: workspace must be 16-byte aligned");
    DSN_REQUIRE(phases >= 0 && phases < 256, "dsn_mesh_cc_emit_ex: bad phases");
    if (out_n_verts == 0 && out_n_faces == 0) return 0;
    dsn_launch_mesh_cc_emit(verts, faces, n_verts, n_faces, workspace, out_verts, out_n_verts, out_faces, out_n_faces, source_vertex,
                            phases ? phases : 255, (hipStream_t)stream);
    return dsn_check_launch("dsn_mesh_cc_emit");
}

int dsn_mesh_cc_emit(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, void* workspace, size_t workspace_bytes,
                     int64_t out_n_verts, int64_t out_n_faces, float* out_verts, int32_t* out_faces, int32_t* source_vertex, void* stream) {
    return dsn_mesh_cc_emit_ex(verts, faces, n_verts, n_faces, workspace, workspace_bytes, out_n_verts, out_n_faces, out_verts, out_faces,
                               source_vertex, 0, stream);
}

// the grid of dsn_mesh_simplify_*: every g_a in [1, 4096], at most 2^31 cells, a finite origin, a finite cell > 0 whose inverse is finite
static bool dsn_mesh_simplify_grid_ok(const int* g) {
    if (!g) return false;
    for (int a = 0; a < 3; ++a)
        if (g[a] < 1 || g[a] > DSN_MESH_SIMPLIFY_MAX_G) return false;
    return (int64_t)g[0] * g[1] * g[2] <= ((int64_t)1 << 31);
}

size_t dsn_mesh_simplify_workspace_bytes(int64_t n_verts, int64_t n_faces, const int* g3_host) {
    return dsn_mesh_cc_sizes_ok(n_verts, n_faces) && dsn_mesh_simplify_grid_ok(g3_host) ? dsn_mesh_simplify_workspace_size(n_verts, n_faces, g3_host) : 0;
}

#define DSN_SIMPLIFY_REQUIRE_GRID(name)                                                                                                       \
    DSN_REQUIRE(origin_host && g3_host, name ": null argument");                                                                             \
    DSN_REQUIRE(dsn_mesh_simplify_grid_ok(g3_host), name ": every g must be 1 ... 4096 and g0 g1 g2 at most 2^31");                          \
    DSN_REQUIRE(std::isfinite(cell) && cell > 0.0f && std::isfinite(1.0f / cell), name ": cell must be finite and > 0");                     \
    DSN_REQUIRE(std::isfinite(origin_host[0]) && std::isfinite(origin_host[1]) && std::isfinite(origin_host[2]), name ": origin must be finite")

int dsn_mesh_simplify_count_ex(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const float* origin_host, float cell,
                               const int* g3_host, void* workspace, size_t workspace_bytes, int32_t* vertex_cluster, int64_t* out_counts7,
                               int phases, void* stream) {
    DSN_REQUIRE(n_verts >= 0 && n_faces >= 0, "dsn_mesh_simplify_count: negative count");
    DSN_REQUIRE(dsn_mesh_cc_sizes_ok(n_verts, n_faces), "dsn_mesh_simplify_count: 2^31 or more vertices or faces");
    DSN_REQUIRE((n_verts == 0 || verts) && (n_faces == 0 || faces), "dsn_mesh_simplify_count: null mesh");
    DSN_REQUIRE(workspace && out_counts7, "dsn_mesh_simplify_count: null argument");
    DSN_SIMPLIFY_REQUIRE_GRID("dsn_mesh_simplify_count");
    DSN_REQUIRE(workspace_bytes >= dsn_mesh_simplify_workspace_size(n_verts, n_faces, g3_host),
                "dsn_mesh_simplify_count: workspace_bytes too small (dsn_mesh_simplify_workspace_bytes)");
    DSN_REQUIRE(((uintptr_t)workspace & 15) == 0, "dsn_mesh_simplify_count: workspace must be 16-byte aligned");
    DSN_REQUIRE(phases >= 0 && phases < 128, "dsn_mesh_simplify_count_ex: bad phases");
    dsn_launch_mesh_simplify_count(verts, faces, n_verts, n_faces, origin_host, cell, g3_host, workspace, vertex_cluster, out_counts7,
                                   phases ? phases : 127, (hipStream_t)stream);
    return dsn_check_launch("dsn_mesh_simplify_count");
}

int dsn_mesh_simplify_count(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const float* origin_host, float cell,
                            const int* g3_host, void* workspace, size_t workspace_bytes, int32_t* vertex_cluster, int64_t* out_counts7,
                            void* stream) {
    return dsn_mesh_simplify_count_ex(verts, faces, n_verts, n_faces, origin_host, cell, g3_host, workspace, workspace_bytes, vertex_cluster,
                                      out_counts7, 0, stream);
}

int dsn_mesh_simplify_cells(const float* verts, int64_t n_verts, const float* origin_host, float cell, const int* g3_host, void* workspace,
                            size_t workspace_bytes, int64_t* out_K, void* stream) {
    DSN_REQUIRE(n_verts >= 0, "dsn_mesh_simplify_cells: negative count");
    DSN_REQUIRE(dsn_mesh_cc_sizes_ok(n_verts, 0), "dsn_mesh_simplify_cells: 2^31 or more vertices");
    DSN_REQUIRE(n_verts == 0 || verts, "dsn_mesh_simplify_cells: null mesh");
    DSN_REQUIRE(workspace && out_K, "dsn_mesh_simplify_cells: null argument");
    DSN_SIMPLIFY_REQUIRE_GRID("dsn_mesh_simplify_cells");
    DSN_REQUIRE(workspace_bytes >= dsn_mesh_simplify_workspace_size(n_verts, 0, g3_host),
                "dsn_mesh_simplify_cells: workspace_bytes too small (dsn_mesh_simplify_workspace_bytes with 0 faces)");
    DSN_REQUIRE(((uintptr_t)workspace & 15) == 0, "dsn_mesh_simplify_cells: workspace must be 16-byte aligned");
    dsn_launch_mesh_simplify_cells(verts, n_verts, origin_host, cell, g3_host, workspace, out_K, (hipStream_t)stream);
    return dsn_check_launch("dsn_mesh_simplify_cells");
}

int dsn_mesh_simplify_emit_ex(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const int* g3_host, void* workspace,
                              size_t workspace_bytes, int64_t out_n_verts, int64_t out_n_faces, float* out_verts, int32_t* out_faces,
                              int32_t* cluster_source, int phases, void* stream) {
    DSN_REQUIRE(n_verts >= 0 && n_faces >= 0 && out_n_verts >= 0 && out_n_faces >= 0, "dsn_mesh_simplify_emit: negative count");
    DSN_REQUIRE(dsn_mesh_cc_sizes_ok(n_verts, n_faces), "dsn_mesh_simplify_emit: 2^31 or more vertices or faces");
    DSN_REQUIRE(g3_host, "dsn_mesh_simplify_emit: null argument");
    DSN_REQUIRE(dsn_mesh_simplify_grid_ok(g3_host), "dsn_mesh_simplify_emit: every g must be 1 ... 4096 and g0 g1 g2 at most 2^31");
    DSN_REQUIRE(out_n_verts <= n_verts && out_n_verts <= (int64_t)g3_host[0] * g3_host[1] * g3_host[2] &&
                    out_n_verts <= ((int64_t)1 << DSN_MESH_SIMPLIFY_MAX_LOG2) && out_n_faces <= n_faces,
                "dsn_mesh_simplify_emit: more clusters or faces than dsn_mesh_simplify_count can have reported");
    DSN_REQUIRE((n_verts == 0 || verts) && (n_faces == 0 || faces), "dsn_mesh_simplify_emit: null mesh");
    DSN_REQUIRE(workspace, "dsn_mesh_simplify_emit: null argument");
    DSN_REQUIRE((out_n_verts == 0 || out_verts) && (out_n_faces == 0 || out_faces), "dsn_mesh_simplify_emit: null output buffer");
    DSN_REQUIRE(workspace_bytes >= dsn_mesh_simplify_workspace_size(n_verts, n_faces, g3_host),
                "dsn_mesh_simplify_emit: workspace_bytes too small (dsn_mesh_simplify_workspace_bytes)");
    DSN_REQUIRE(((uintptr_t)workspace & 15) == 0, "dsn_mesh_simplify_emit: workspace must be 16-byte aligned");
    DSN_REQUIRE(phases == 0 || (phases & ~(DSN_SP_EMIT_VERTS | DSN_SP_EMIT_FACES)) == 0, "dsn_mesh_simplify_emit_ex: bad phases");
    if (out_n_verts == 0 && out_n_faces == 0) return 0;
    dsn_launch_mesh_simplify_emit(verts, faces, n_verts, n_faces, g3_host, workspace, out_verts, out_n_verts, out_faces, out_n_faces,
                                  cluster_source, phases ? phases : (DSN_SP_EMIT_VERTS | DSN_SP_EMIT_FACES), (hipStream_t)stream);
    return dsn_check_launch("dsn_mesh_simplify_emit");
}

int dsn_mesh_simplify_emit(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const int* g3_host, void* workspace,
                           size_t workspace_bytes, int64_t out_n_verts, int64_t out_n_faces, float* out_verts, int32_t* out_faces,
                           int32_t* cluster_source, void* stream) {
    return dsn_mesh_simplify_emit_ex(verts, faces, n_verts, n_faces, g3_host, workspace, workspace_bytes, out_n_verts, out_n_faces, out_verts,
                                     out_faces, cluster_source, 0, stream);
}

size_t dsn_mesh_smooth_workspace_bytes(int64_t n_verts, int64_t n_faces) {
    return dsn_mesh_cc_sizes_ok(n_verts, n_faces) ? dsn_mesh_smooth_workspace_size(n_verts, n_faces) : 0;
}

// the byte ranges [a, a + n) and [b, b + n) share a byte
static bool dsn_ranges_overlap(const void* a, const void* b, size_t n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return n > 0 && (x < y ? y - x < n : x - y < n);
}

int dsn_mesh_smooth_ex(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const float* origin_host, int scale_exp,
                       const float* factors_host, int n_steps, void* workspace, size_t workspace_bytes, float* out_verts, int64_t* out_counts4,
                       int phases, void* stream) {
    DSN_REQUIRE(n_verts >= 0 && n_faces >= 0, "dsn_mesh_smooth: negative count");
    DSN_REQUIRE(dsn_mesh_cc_sizes_ok(n_verts, n_faces), "dsn_mesh_smooth: 2^31 or more vertices or faces");
    DSN_REQUIRE((n_verts == 0 || verts) && (n_faces == 0 || faces), "dsn_mesh_smooth: null mesh");
    DSN_REQUIRE(n_verts == 0 || out_verts, "dsn_mesh_smooth: null output buffer");
    DSN_REQUIRE(workspace && origin_host, "dsn_mesh_smooth: null argument");
    DSN_REQUIRE(n_steps >= 0 && n_steps <= DSN_MESH_SMOOTH_MAX_STEPS, "dsn_mesh_smooth: n_steps must be 0 ... 4096");
    DSN_REQUIRE(n_steps == 0 || factors_host, "dsn_mesh_smooth: null factors");
    DSN_REQUIRE(scale_exp >= -DSN_MESH_SMOOTH_MAX_EXP && scale_exp <= DSN_MESH_SMOOTH_MAX_EXP, "dsn_mesh_smooth: scale_exp must be -900 ... 900");
    for (int a = 0; a < 3; ++a) DSN_REQUIRE(std::isfinite(origin_host[a]), "dsn_mesh_smooth: the origin must be finite");
    for (int s = 0; s < n_steps; ++s) DSN_REQUIRE(std::isfinite(factors_host[s]), "dsn_mesh_smooth: every factor must be finite");
    DSN_REQUIRE(workspace_bytes >= dsn_mesh_smooth_workspace_size(n_verts, n_faces),
                "dsn_mesh_smooth: workspace_bytes too small (dsn_mesh_smooth_workspace_bytes)");
    DSN_REQUIRE(((uintptr_t)workspace & 15) == 0, "dsn_mesh_smooth: workspace must be 16-byte aligned");
    DSN_REQUIRE(!dsn_ranges_overlap(verts, out_verts, (size_t)12 * (size_t)n_verts), "dsn_mesh_smooth: out_verts must not overlap verts");
    DSN_REQUIRE(phases == 0 || (phases & ~(DSN_SM_COUNT | DSN_SM_SCAN | DSN_SM_FILL | DSN_SM_STEP)) == 0, "dsn_mesh_smooth_ex: bad phases");
    dsn_launch_mesh_smooth(verts, faces, n_verts, n_faces, origin_host, scale_exp, factors_host, n_steps, workspace, out_verts, out_counts4,
                           phases ? phases : (DSN_SM_COUNT | DSN_SM_SCAN | DSN_SM_FILL | DSN_SM_STEP), (hipStream_t)stream);
    return dsn_check_launch("dsn_mesh_smooth");
}

int dsn_mesh_smooth(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const float* origin_host, int scale_exp,
                    const float* factors_host, int n_steps, void* workspace, size_t workspace_bytes, float* out_verts, int64_t* out_counts4,
                    void* stream) {
    return dsn_mesh_smooth_ex(verts, faces, n_verts, n_faces, origin_host, scale_exp, factors_host, n_steps, workspace, workspace_bytes,
                              out_verts, out_counts4, 0, stream);
}

int dsn_mesh_vertex_normals_ex(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, int shift, void* workspace,
                               size_t workspace_bytes, float* out_normals, int phases, void* stream) {
    DSN_REQUIRE(n_verts >= 0 && n_faces >= 0, "dsn_mesh_vertex_normals: negative count");
    DSN_REQUIRE(dsn_mesh_cc_sizes_ok(n_verts, n_faces), "dsn_mesh_vertex_normals: 2^31 or more vertices or faces");
    DSN_REQUIRE((n_verts == 0 || verts) && (n_faces == 0 || faces), "dsn_mesh_vertex_normals: null mesh");
    DSN_REQUIRE(n_verts == 0 || out_normals, "dsn_mesh_vertex_normals: null output buffer");
    DSN_REQUIRE(workspace, "dsn_mesh_vertex_normals: null argument");
    DSN_REQUIRE(workspace_bytes >= dsn_mesh_smooth_workspace_size(n_verts, n_faces),
                "dsn_mesh_vertex_normals: workspace_bytes too small (dsn_mesh_smooth_workspace_bytes)");
    DSN_REQUIRE(((uintptr_t)workspace & 15) == 0, "dsn_mesh_vertex_normals: workspace must be 16-byte aligned");
    DSN_REQUIRE(!dsn_ranges_overlap(verts, out_normals, (size_t)12 * (size_t)n_verts), "dsn_mesh_vertex_normals: out_normals must not overlap verts");
    DSN_REQUIRE(shift >= -60 && shift <= 60, "dsn_mesh_vertex_normals: shift must be -60 ... 60");
    DSN_REQUIRE(phases == 0 || (phases & ~(DSN_SM_COUNT | DSN_SM_SCAN | DSN_SM_FILL | DSN_SM_NORMALS)) == 0, "dsn_mesh_vertex_normals_ex: bad phases");
    dsn_launch_mesh_vertex_normals(verts, faces, n_verts, n_faces, std::ldexp(1.0, shift), workspace, out_normals,
                                   phases ? phases : (DSN_SM_COUNT | DSN_SM_SCAN | DSN_SM_FILL | DSN_SM_NORMALS), (hipStream_t)stream);
    return dsn_check_launch("dsn_mesh_vertex_normals");
}

int dsn_mesh_vertex_normals(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, int shift, void* workspace,
                            size_t workspace_bytes, float* out_normals, void* stream) {
    return dsn_mesh_vertex_normals_ex(verts, faces, n_verts, n_faces, shift, workspace, workspace_bytes, out_normals, 0, stream);
}

// counts of the bound-mesh calls: every byte size fits size_t and every grid fits 2^31 - 1 workgroups of 256
static bool dsn_mesh_pose_sizes_ok(int64_t P, int64_t N) {
    return P >= 1 && N >= 0 && N < ((int64_t)1 << 38) && (uint64_t)N <= (uint64_t)SIZE_MAX / 12 / (uint64_t)P;
}

size_t dsn_mesh_pose_workspace_bytes(int P, int Fb) {
    return (P >= 1 && Fb >= 1 && (uint64_t)P * (uint64_t)Fb < ((uint64_t)1 << 38)) ? sizeof(DsnFaceRec) * (size_t)P * (size_t)Fb : 0;
}

int dsn_mesh_bind_normals(const float* body_xyz, int Vb, const int32_t* body_faces, int Fb, const int32_t* face_idx, const float* normals,
                          int64_t N, float* cov, void* stream) {
    DSN_REQUIRE(N >= 0, "dsn_mesh_bind_normals: negative count");
    DSN_REQUIRE(dsn_mesh_pose_sizes_ok(1, N), "dsn_mesh_bind_normals: too many vertices");
    DSN_REQUIRE(Vb > 0 && Fb > 0, "dsn_mesh_bind_normals: bad Vb/Fb");
    DSN_REQUIRE(body_xyz && body_faces, "dsn_mesh_bind_normals: null body");
    DSN_REQUIRE(N == 0 || (face_idx && normals && cov), "dsn_mesh_bind_normals: null argument");
    dsn_launch_mesh_bind_normals(body_xyz, Vb, body_faces, Fb, face_idx, normals, N, cov, (hipStream_t)stream);
    return dsn_check_launch("dsn_mesh_bind_normals");
}

int dsn_mesh_pose(const float* target_xyz, int P, int Vb, const int32_t* body_faces, int Fb, const int32_t* face_idx, const float* uv,
                  const float* h, const float* cov, int64_t N, float* out_verts, float* out_normals, int32_t* status, void* workspace,
                  void* stream) {
    DSN_REQUIRE(N >= 0, "dsn_mesh_pose: negative count");
    DSN_REQUIRE(P >= 1, "dsn_mesh_pose: P must be at least 1");
    DSN_REQUIRE(Vb > 0 && Fb > 0, "dsn_mesh_pose: bad Vb/Fb");
    DSN_REQUIRE(dsn_mesh_pose_sizes_ok(P, N) && dsn_mesh_pose_workspace_bytes(P, Fb) != 0 &&
                (uint64_t)Vb <= (uint64_t)SIZE_MAX / 12 / (uint64_t)P, "dsn_mesh_pose: counts too large");
    DSN_REQUIRE(target_xyz && body_faces && workspace, "dsn_mesh_pose: null argument");
    DSN_REQUIRE(((uintptr_t)workspace & 15) == 0, "dsn_mesh_pose: workspace must be 16-byte aligned");
    DSN_REQUIRE(N == 0 || (face_idx && uv && h && out_verts), "dsn_mesh_pose: null binding or output");
    DSN_REQUIRE(!out_normals || cov || N == 0, "dsn_mesh_pose: out_normals needs cov (null)");
    dsn_launch_mesh_pose(target_xyz, P, Vb, body_faces, Fb, face_idx, uv, h, cov, N, out_verts, out_normals, status, workspace,
                         (hipStream_t)stream);
    return dsn_check_launch("dsn_mesh_pose");
}

int dsn_mesh_stretch(const float* bind_verts, const float* posed_verts, int P, int64_t N, const int32_t* faces, int64_t T, float* stretch,
                     void* stream) {
    DSN_REQUIRE(N >= 0 && T >= 0, "dsn_mesh_stretch: negative count");
    DSN_REQUIRE(P >= 1, "dsn_mesh_stretch: P must be at least 1");
    DSN_REQUIRE(dsn_mesh_pose_sizes_ok(P, N) && dsn_mesh_pose_sizes_ok(P, T), "dsn_mesh_stretch: counts too large");
    DSN_REQUIRE(N == 0 || (bind_verts && posed_verts), "dsn_mesh_stretch: null vertices");
    DSN_REQUIRE(T == 0 || (faces && stretch), "dsn_mesh_stretch: null faces or output");
    dsn_launch_mesh_stretch(bind_verts, posed_verts, P, N, faces, T, stretch, (hipStream_t)stream);
    return dsn_check_launch("dsn_mesh_stretch");
}

// the body model: vertex counts whose [P, V, 3] byte sizes fit size_t, pose counts whose pose blocks fit the launch grid's y axis
static bool dsn_body_sizes_ok(int64_t V, int64_t P) {
    return V >= 1 && V <= ((int64_t)1 << 28) && P >= 0 && P <= ((int64_t)1 << 18) && (P == 0 || (uint64_t)V <= (uint64_t)SIZE_MAX / 12 / (uint64_t)P);
}

int dsn_body_shape(const float* v_template, const float* shapedirs, const float* betas, int B, const float* J_regressor, int V,
                   float* v_shaped, float* joints, void* stream) {
    DSN_REQUIRE(dsn_body_sizes_ok(V, 1), "dsn_body_shape: bad V");
    DSN_REQUIRE(B >= 0 && B <= 4096, "dsn_body_shape: bad B");
    DSN_REQUIRE(v_template && v_shaped, "dsn_body_shape: null v_template or v_shaped");
    DSN_REQUIRE(B == 0 || ((shapedirs == nullptr) == (betas == nullptr)), "dsn_body_shape: shapedirs and betas go together");
    DSN_REQUIRE((joints == nullptr) == (J_regressor == nullptr), "dsn_body_shape: joints and J_regressor go together");
    dsn_launch_body_shape(v_template, shapedirs, betas, B, J_regressor, V, v_shaped, joints, (hipStream_t)stream);
    return dsn_check_launch("dsn_body_shape");
}

size_t dsn_body_pose_workspace_bytes(int V, int P) {
    return (dsn_body_sizes_ok(V, P) && P >= 1) ? dsn_body_pose_workspace_size(V, P) : 0;
}

int dsn_body_pose(const float* v_shaped, const float* joints, const int32_t* parents_host, const float* weights, const float* posedirs, int V,
                  const float* poses, const float* Rh, const float* Th, int P, int pad_mode, float* xyz, float* xyz_smpl, float* A,
                  float* bounds, float* Rh_mat, void* workspace, size_t workspace_bytes, void* stream) {
    DSN_REQUIRE(V >= 1, "dsn_body_pose: V must be at least 1");
    DSN_REQUIRE(P >= 0, "dsn_body_pose: negative pose count");
    DSN_REQUIRE(dsn_body_sizes_ok(V, P), "dsn_body_pose: counts too large");
    DSN_REQUIRE(pad_mode >= DSN_BODY_PAD_NONE && pad_mode <= DSN_BODY_PAD_H36M, "dsn_body_pose: unknown pad_mode");
    DSN_REQUIRE(v_shaped && joints && parents_host && weights, "dsn_body_pose: null body model argument");
    for (int i = 1; i < 24; ++i)
        if (parents_host[i] < 0 || parents_host[i] >= i) return dsn_fail("dsn_body_pose: parents[%s%lld] is not an earlier joint", "", i);
    if (P == 0) return 0;      // an empty clip: nothing to write, no launch
    DSN_REQUIRE(poses && xyz, "dsn_body_pose: null poses or xyz");
    DSN_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0, "dsn_body_pose: workspace must be 256-byte aligned (null)");
    DSN_REQUIRE(workspace_bytes >= dsn_body_pose_workspace_size(V, P), "dsn_body_pose: workspace too small (dsn_body_pose_workspace_bytes)");
    dsn_launch_body_pose(v_shaped, joints, parents_host, weights, posedirs, V, poses, Rh, Th, P, pad_mode, xyz, xyz_smpl, A, bounds, Rh_mat,
                         workspace, (hipStream_t)stream);
    return dsn_check_launch("dsn_body_pose");
}

static bool dsn_raster_sizes_ok(int64_t V, int64_t T, int H, int W) {
    return V >= 0 && T >= 0 && V < ((int64_t)1 << 31) && T < ((int64_t)1 << 31) && H >= 1 && H <= 16384 && W >= 1 && W <= 16384;
}

size_t dsn_raster_workspace_bytes(int64_t n_verts, int64_t n_faces, int H, int W) {
    return dsn_raster_sizes_ok(n_verts, n_faces, H, W) ? dsn_raster_workspace_size(n_verts, n_faces, H, W) : 0;
}

// the checks and the launch of dsn_raster_mesh_ex and dsn_raster_mesh_attr (extra: the latter's two further outputs count as outputs)
static int dsn_raster_mesh_any(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cam_pose_host, float fx,
                               float fy, float znear, const float* light_host, int H, int W, int32_t* out_face, float* out_depth,
                               uint8_t* out_color, void* workspace, size_t workspace_bytes, int phases, int big_pixels,
                               const float* vertex_normals, const float* vertex_colors, int mode, float* out_normal, float* out_attr,
                               void* stream) {
    DSN_REQUIRE(n_verts >= 0 && n_faces >= 0, "dsn_raster_mesh: negative count");
    DSN_REQUIRE(H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "dsn_raster_mesh: H and W must be 1 ... 16384");
    DSN_REQUIRE(dsn_raster_sizes_ok(n_verts, n_faces, H, W), "dsn_raster_mesh: 2^31 or more vertices or faces");
    DSN_REQUIRE(cam_pose_host && light_host && workspace, "dsn_raster_mesh: null argument");
    DSN_REQUIRE((n_verts == 0 || verts) && (n_faces == 0 || faces), "dsn_raster_mesh: null mesh");
    DSN_REQUIRE(out_face || out_depth || out_color || out_normal || out_attr, "dsn_raster_mesh: no output (out_face, out_depth and out_color are all null)");
    DSN_REQUIRE(workspace_bytes >= dsn_raster_workspace_size(n_verts, n_faces, H, W), "dsn_raster_mesh: workspace_bytes too small (dsn_raster_workspace_bytes)");
    DSN_REQUIRE(((uintptr_t)workspace & 15) == 0, "dsn_raster_mesh: workspace must be 16-byte aligned");
    DSN_REQUIRE(std::isfinite(fx) && std::isfinite(fy) && std::isfinite(znear), "dsn_raster_mesh: fx, fy and znear must be finite");
    DSN_REQUIRE(znear > 0.0f, "dsn_raster_mesh: znear must be positive");
    for (int i = 0; i < 12; ++i) DSN_REQUIRE(std::isfinite(cam_pose_host[i]), "dsn_raster_mesh: cam_pose_host is not finite");
    for (int i = 0; i < 4; ++i) DSN_REQUIRE(std::isfinite(light_host[i]), "dsn_raster_mesh: light_host is not finite");
    DSN_REQUIRE(light_host[1] > light_host[2], "dsn_raster_mesh: light_host needs cos_inner > cos_outer");
    DSN_REQUIRE(phases >= 0 && phases < 32 && big_pixels >= 0, "dsn_raster_mesh_ex: bad phases or big_pixels");
    DSN_REQUIRE(mode >= 0 && mode <= (DSN_RM_SMOOTH | DSN_RM_UNLIT), "dsn_raster_mesh_attr: mode must be a combination of DSN_RM_SMOOTH and DSN_RM_UNLIT");
    DSN_REQUIRE(!(mode & DSN_RM_SMOOTH) || vertex_normals || n_verts == 0, "dsn_raster_mesh_attr: DSN_RM_SMOOTH needs vertex_normals (null)");
    DSN_REQUIRE(!out_attr || vertex_colors || n_verts == 0, "dsn_raster_mesh_attr: out_attr needs vertex_colors (null)");
    dsn_launch_raster_mesh_attr(verts, n_verts, faces, n_faces, cam_pose_host, fx, fy, znear, light_host, H, W, out_face, out_depth,
                                out_color, workspace, phases ? phases : 31, big_pixels ? big_pixels : DSN_RM_BIG_PIXELS, vertex_normals,
                                vertex_colors, mode, out_normal, out_attr, (hipStream_t)stream);
    return dsn_check_launch("dsn_raster_mesh");
}

int dsn_raster_mesh_ex(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cam_pose_host, float fx,
                       float fy, float znear, const float* light_host, int H, int W, int32_t* out_face, float* out_depth,
                       uint8_t* out_color, void* workspace, size_t workspace_bytes, int phases, int big_pixels, void* stream) {
    return dsn_raster_mesh_any(verts, n_verts, faces, n_faces, cam_pose_host, fx, fy, znear, light_host, H, W, out_face, out_depth, out_color,
                               workspace, workspace_bytes, phases, big_pixels, nullptr, nullptr, 0, nullptr, nullptr, stream);
}

int dsn_raster_mesh_attr(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cam_pose_host, float fx,
                         float fy, float znear, const float* light_host, int H, int W, int32_t* out_face, float* out_depth,
                         uint8_t* out_color, void* workspace, size_t workspace_bytes, int phases, int big_pixels,
                         const float* vertex_normals, const float* vertex_colors, int mode, float* out_normal, float* out_attr,
                         void* stream) {
    return dsn_raster_mesh_any(verts, n_verts, faces, n_faces, cam_pose_host, fx, fy, znear, light_host, H, W, out_face, out_depth, out_color,
                               workspace, workspace_bytes, phases, big_pixels, vertex_normals, vertex_colors, mode, out_normal, out_attr,
                               stream);
}

int dsn_raster_mesh(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cam_pose_host, float fx,
                    float fy, float znear, const float* light_host, int H, int W, int32_t* out_face, float* out_depth, uint8_t* out_color,
                    void* workspace, size_t workspace_bytes, void* stream) {
    return dsn_raster_mesh_ex(verts, n_verts, faces, n_faces, cam_pose_host, fx, fy, znear, light_host, H, W, out_face, out_depth,
                              out_color, workspace, workspace_bytes, 0, 0, stream);
}

// ---- the datasets' image preparation (dsn_prep.hip) ----
#define DSN_PREP_COMMON(name, N, H, W)                                                                        \
    DSN_REQUIRE((N) >= 0 && (N) <= 65535, name ": N must be 0 ... 65535");                                   \
    DSN_REQUIRE((H) > 0 && (W) > 0 && (H) <= DSN_PREP_MAX_SIDE && (W) <= DSN_PREP_MAX_SIDE, name ": H and W must be 1 ... 32768")

int dsn_image_undistort(const void* src, void* dst, const double* K, const double* D, int nd, int N, int H, int W, int channels, int dtype,
                        void* stream) {
    DSN_PREP_COMMON("dsn_image_undistort", N, H, W);
    DSN_REQUIRE(nd == 4 || nd == 5 || nd == 8, "dsn_image_undistort: nd must be 4, 5 or 8");
    DSN_REQUIRE(channels == 1 || channels == 3, "dsn_image_undistort: channels must be 1 or 3");
    DSN_REQUIRE(dtype == DSN_PREP_U8 || dtype == DSN_PREP_F32, "dsn_image_undistort: dtype must be DSN_PREP_U8 or DSN_PREP_F32");
    if (N == 0) return 0;
    DSN_REQUIRE(src && dst && K && D, "dsn_image_undistort: null argument");
    DSN_REQUIRE(src != dst, "dsn_image_undistort: src and dst must differ");
    dsn_launch_image_undistort(src, dst, K, D, nd, N, H, W, channels, dtype, (hipStream_t)stream);
    return dsn_check_launch("dsn_image_undistort");
}

int dsn_image_morph(const uint8_t* src, uint8_t* dst, int N, int H, int W, int k, int op, void* stream) {
    DSN_PREP_COMMON("dsn_image_morph", N, H, W);
    DSN_REQUIRE(k >= 1 && k <= 15, "dsn_image_morph: k must be 1 ... 15");
    DSN_REQUIRE(op == DSN_PREP_DILATE || op == DSN_PREP_ERODE, "dsn_image_morph: op must be DSN_PREP_DILATE or DSN_PREP_ERODE");
    if (N == 0) return 0;
    DSN_REQUIRE(src && dst, "dsn_image_morph: null argument");
    DSN_REQUIRE(src != dst, "dsn_image_morph: src and dst must differ");
    dsn_launch_image_morph(src, dst, N, H, W, k, op, (hipStream_t)stream);
    return dsn_check_launch("dsn_image_morph");
}

int dsn_image_resize(const void* src, void* dst, int N, int H, int W, int channels, int dtype, int c, int mode, void* stream) {
    DSN_PREP_COMMON("dsn_image_resize", N, H, W);
    DSN_REQUIRE(c == 1 || c == 2 || c == 4, "dsn_image_resize: c must be 1, 2 or 4");
    DSN_REQUIRE(H % c == 0 && W % c == 0, "dsn_image_resize: H and W must be multiples of c");
    DSN_REQUIRE(channels == 1 || channels == 3, "dsn_image_resize: channels must be 1 or 3");
    DSN_REQUIRE(dtype == DSN_PREP_U8 || dtype == DSN_PREP_F32, "dsn_image_resize: dtype must be DSN_PREP_U8 or DSN_PREP_F32");
    DSN_REQUIRE(mode == DSN_PREP_NEAREST || mode == DSN_PREP_AREA, "dsn_image_resize: mode must be DSN_PREP_NEAREST or DSN_PREP_AREA");
    if (N == 0) return 0;
    DSN_REQUIRE(src && dst, "dsn_image_resize: null argument");
    DSN_REQUIRE(src != dst, "dsn_image_resize: src and dst must differ");
    DSN_REQUIRE(dtype == DSN_PREP_U8 || (((uintptr_t)src | (uintptr_t)dst) & 3) == 0, "dsn_image_resize: a float32 pointer is not 4-byte aligned");
    dsn_launch_image_resize(src, dst, N, H, W, channels, dtype, c, mode, (hipStream_t)stream);
    return dsn_check_launch("dsn_image_resize");
}

int dsn_image_prep(const uint8_t* img, const uint8_t* msk_cihp, const double* K, const double* D, int nd, int N, int H0, int W0, int c,
                   int border, int out_dtype, void* out_img, uint8_t* out_img_u8, uint8_t* out_msk_fg, uint8_t* out_msk_cihp, void* stream) {
    DSN_PREP_COMMON("dsn_image_prep", N, H0, W0);
    DSN_REQUIRE(nd == 4 || nd == 5 || nd == 8, "dsn_image_prep: nd must be 4, 5 or 8");
    DSN_REQUIRE(c == 1 || c == 2 || c == 4, "dsn_image_prep: c must be 1, 2 or 4");
    DSN_REQUIRE(H0 % c == 0 && W0 % c == 0, "dsn_image_prep: H0 and W0 must be multiples of c");
    DSN_REQUIRE(border >= 1 && border <= 15, "dsn_image_prep: border must be 1 ... 15");
    DSN_REQUIRE(out_dtype == DSN_PREP_F64 || out_dtype == DSN_PREP_F32, "dsn_image_prep: out_dtype must be DSN_PREP_F64 or DSN_PREP_F32");
    if (N == 0) return 0;
    DSN_REQUIRE(img && msk_cihp && K && D && out_img, "dsn_image_prep: null argument");
    DSN_REQUIRE(((uintptr_t)out_img & (out_dtype == DSN_PREP_F64 ? 7 : 3)) == 0, "dsn_image_prep: out_img is not aligned to its element");
    dsn_launch_image_prep(img, msk_cihp, K, D, nd, N, H0, W0, c, border, out_dtype, out_img, out_img_u8, out_msk_fg, out_msk_cihp,
                          (hipStream_t)stream);
    return dsn_check_launch("dsn_image_prep");
}

// ---- LPIPS (csrc/dsn_lpips.hip) ----
static bool dsn_lpips_sizes_ok(int net, int n, int H, int W) {
    return (net == DSN_LPIPS_ALEX || net == DSN_LPIPS_VGG) && n >= 1 && n <= DSN_LPIPS_MAX_IMAGES / 2 && H >= 1 && W >= 1 &&
           H <= DSN_LPIPS_MAX_SIDE && W <= DSN_LPIPS_MAX_SIDE;
}
size_t dsn_lpips_packed_bytes(int net) { return net == DSN_LPIPS_ALEX || net == DSN_LPIPS_VGG ? dsn_lpips_packed_size(net) : 0; }
size_t dsn_lpips_workspace_bytes(int net, int F, int H, int W) {
    return dsn_lpips_sizes_ok(net, F, H, W) ? dsn_lpips_workspace_size(net, 2 * F, H, W) : 0;
}

int dsn_lpips_pack(int net, const float* const* conv_w, const float* const* conv_b, const float* const* lin_w, void* packed, void* stream) {
    DSN_REQUIRE(net == DSN_LPIPS_ALEX || net == DSN_LPIPS_VGG, "dsn_lpips_pack: net must be DSN_LPIPS_ALEX or DSN_LPIPS_VGG");
    DSN_REQUIRE(conv_w && conv_b && lin_w && packed, "dsn_lpips_pack: null argument");
    const int nconv = net == DSN_LPIPS_ALEX ? 5 : 13;
    for (int i = 0; i < nconv; ++i) DSN_REQUIRE(conv_w[i] && conv_b[i], "dsn_lpips_pack: null convolution tensor");
    for (int l = 0; l < 5; ++l) DSN_REQUIRE(lin_w[l], "dsn_lpips_pack: null lin tensor");
    DSN_REQUIRE(((uintptr_t)packed & 255) == 0, "dsn_lpips_pack: packed is not 256-byte aligned");
    if (dsn_launch_lpips_pack(net, conv_w, conv_b, lin_w, packed, (hipStream_t)stream)) return dsn_fail("%s", "dsn_lpips_pack: memset failed");
    return dsn_check_launch("dsn_lpips_pack");
}

int dsn_lpips_features(const void* packed, int net, const float* stack, int n, int H, int W, int rgb_pm1, float* const* out_taps5,
                       int32_t* out_status, void* workspace, size_t workspace_bytes, void* stream) {
    DSN_REQUIRE(packed && stack && out_taps5 && out_status && workspace, "dsn_lpips_features: null argument");
    DSN_REQUIRE((net == DSN_LPIPS_ALEX || net == DSN_LPIPS_VGG) && n >= 1 && n <= DSN_LPIPS_MAX_IMAGES && H >= 1 && W >= 1 &&
                    H <= DSN_LPIPS_MAX_SIDE && W <= DSN_LPIPS_MAX_SIDE, "dsn_lpips_features: bad sizes");
    for (int l = 0; l < 5; ++l) DSN_REQUIRE(out_taps5[l], "dsn_lpips_features: null tap pointer");
    DSN_REQUIRE((((uintptr_t)packed | (uintptr_t)workspace) & 255) == 0, "dsn_lpips_features: packed / workspace not 256-byte aligned");
    DSN_REQUIRE(workspace_bytes >= dsn_lpips_workspace_size(net, n, H, W), "dsn_lpips_features: workspace_bytes too small for n images");
    dsn_launch_lpips_features(packed, net, stack, n, H, W, rgb_pm1 != 0, out_taps5, out_status, workspace, (hipStream_t)stream);
    return dsn_check_launch("dsn_lpips_features");
}

int dsn_lpips(const void* packed, int net, const float* img, const double* gt_f64, const float* gt_f32, int F, int H, int W, int rgb_pm1,
              double* out, double* out_layers, int32_t* out_status, void* workspace, size_t workspace_bytes, void* stream) {
    DSN_REQUIRE(packed && img && out && out_layers && out_status && workspace, "dsn_lpips: null argument");
    DSN_REQUIRE((gt_f64 != nullptr) != (gt_f32 != nullptr), "dsn_lpips: exactly one ground-truth pointer");
    DSN_REQUIRE(dsn_lpips_sizes_ok(net, F, H, W), "dsn_lpips: bad sizes");
    DSN_REQUIRE((((uintptr_t)packed | (uintptr_t)workspace) & 255) == 0, "dsn_lpips: packed / workspace not 256-byte aligned");
    DSN_REQUIRE(workspace_bytes >= dsn_lpips_workspace_size(net, 2 * F, H, W), "dsn_lpips: workspace_bytes below dsn_lpips_workspace_bytes");
    dsn_launch_lpips(packed, net, img, gt_f64, gt_f32, F, H, W, rgb_pm1 != 0, out, out_layers, out_status, workspace, (hipStream_t)stream);
    return dsn_check_launch("dsn_lpips");
}

// ---- baseline JPEG (dsn_jpeg.hip) ----
#define DSN_JPEG_COMMON(name, F, H, W, mode, quality)                                                                          \
    DSN_REQUIRE((mode) == DSN_JPEG_420 || (mode) == DSN_JPEG_444 || (mode) == DSN_JPEG_GRAY, name ": mode must be DSN_JPEG_420, _444 or _GRAY"); \
    DSN_REQUIRE((quality) >= 1 && (quality) <= 100, name ": quality must be 1 ... 100");                                       \
    DSN_REQUIRE((F) >= 0 && (F) <= DSN_JPEG_MAX_FRAMES, name ": F must be 0 ... 65535");                                       \
    DSN_REQUIRE((H) >= 1 && (W) >= 1 && (H) <= 65535 && (W) <= 65535, name ": H and W must be 1 ... 65535");                   \
    int blocks = 0;                                                                                                            \
    DSN_REQUIRE(dsn_jpeg_blocks(H, W, mode, &blocks), name ": too many blocks for int32 bit offsets (blocks x 1664 must stay below 2^31)")

size_t dsn_jpeg_max_bytes(int H, int W, int mode) {
    int blocks = 0;
    if (!dsn_jpeg_blocks(H, W, mode, &blocks)) return 0;
    return dsn_jpeg_header_bytes(mode) + (size_t)blocks * (2 * DSN_JPEG_BLOCK_BYTES) + 2;
}

size_t dsn_jpeg_workspace_bytes(int F, int H, int W, int mode) { return dsn_jpeg_workspace_size(F, H, W, mode, true); }

int dsn_jpeg_header_host(int H, int W, int mode, int quality, uint8_t* out_host, int capacity, int* len) {
    DSN_JPEG_COMMON("dsn_jpeg_header_host", 0, H, W, mode, quality);
    DSN_REQUIRE(out_host && len, "dsn_jpeg_header_host: null argument");
    DSN_REQUIRE(capacity >= (int)dsn_jpeg_header_bytes(mode), "dsn_jpeg_header_host: capacity is below the header's length");
    *len = dsn_jpeg_write_header_host(H, W, mode, quality, out_host);
    return 0;
}

int dsn_jpeg_coefficients(const void* images, int dtype, int F, int H, int W, int mode, int quality, int rgb, float scale, int16_t* coef,
                          uint32_t* out_status, void* stream) {
    DSN_JPEG_COMMON("dsn_jpeg_coefficients", F, H, W, mode, quality);
    DSN_REQUIRE(dtype == DSN_JPEG_U8 || dtype == DSN_JPEG_F32, "dsn_jpeg_coefficients: dtype must be DSN_JPEG_U8 or DSN_JPEG_F32");
    if (F == 0) return 0;
    DSN_REQUIRE(images && coef && out_status, "dsn_jpeg_coefficients: null argument");
    DSN_REQUIRE(dtype == DSN_JPEG_U8 || ((uintptr_t)images & 3) == 0, "dsn_jpeg_coefficients: a float32 image is not 4-byte aligned");
    DSN_REQUIRE(((uintptr_t)coef & 1) == 0 && ((uintptr_t)out_status & 3) == 0, "dsn_jpeg_coefficients: coef or out_status is not aligned");
    dsn_launch_jpeg_coefficients(images, dtype, F, H, W, mode, quality, rgb != 0, scale, coef, out_status, (hipStream_t)stream);
    return dsn_check_launch("dsn_jpeg_coefficients");
}

int dsn_jpeg_scan(const int16_t* coef, const uint32_t* status_in, int F, int H, int W, int mode, int quality, uint8_t* out, size_t capacity,
                  int32_t* out_lengths, uint32_t* out_status, void* workspace, size_t workspace_bytes, void* stream) {
    DSN_JPEG_COMMON("dsn_jpeg_scan", F, H, W, mode, quality);
    if (F == 0) return 0;
    DSN_REQUIRE(coef && out && out_lengths && out_status && workspace, "dsn_jpeg_scan: null argument");
    DSN_REQUIRE(((uintptr_t)workspace & 255) == 0, "dsn_jpeg_scan: workspace must be 256-byte aligned");
    DSN_REQUIRE(workspace_bytes >= dsn_jpeg_workspace_size(F, H, W, mode, false), "dsn_jpeg_scan: workspace_bytes is too small");
    DSN_REQUIRE(status_in != out_status, "dsn_jpeg_scan: status_in and out_status must differ");
    DSN_REQUIRE((((uintptr_t)coef & 1) | ((uintptr_t)out_lengths & 3) | ((uintptr_t)out_status & 3) | ((uintptr_t)status_in & 3)) == 0,
                "dsn_jpeg_scan: a pointer is not aligned to its element");
    dsn_launch_jpeg_scan(coef, status_in, F, H, W, mode, quality, out, capacity, out_lengths, out_status, workspace, false, (hipStream_t)stream);
    return dsn_check_launch("dsn_jpeg_scan");
}

int dsn_jpeg_encode(const void* images, int dtype, int F, int H, int W, int mode, int quality, int rgb, float scale, uint8_t* out,
                    size_t capacity, int32_t* out_lengths, uint32_t* out_status, void* workspace, size_t workspace_bytes, void* stream) {
    DSN_JPEG_COMMON("dsn_jpeg_encode", F, H, W, mode, quality);
    DSN_REQUIRE(dtype == DSN_JPEG_U8 || dtype == DSN_JPEG_F32, "dsn_jpeg_encode: dtype must be DSN_JPEG_U8 or DSN_JPEG_F32");
    if (F == 0) return 0;
    DSN_REQUIRE(images && out && out_lengths && out_status && workspace, "dsn_jpeg_encode: null argument");
    DSN_REQUIRE(dtype == DSN_JPEG_U8 || ((uintptr_t)images & 3) == 0, "dsn_jpeg_encode: a float32 image is not 4-byte aligned");
    DSN_REQUIRE(((uintptr_t)workspace & 255) == 0, "dsn_jpeg_encode: workspace must be 256-byte aligned");
    DSN_REQUIRE(workspace_bytes >= dsn_jpeg_workspace_size(F, H, W, mode, true), "dsn_jpeg_encode: workspace_bytes is too small");
    DSN_REQUIRE((((uintptr_t)out_lengths & 3) | ((uintptr_t)out_status & 3)) == 0, "dsn_jpeg_encode: a pointer is not aligned to its element");
    dsn_launch_jpeg_encode(images, dtype, F, H, W, mode, quality, rgb != 0, scale, out, capacity, out_lengths, out_status, workspace,
                           (hipStream_t)stream);
    return dsn_check_launch("dsn_jpeg_encode");
}

// ---- baseline JPEG decoding (dsn_jpegd.hip) ----
#define DSN_JPEGD_COMMON(name, F, H, W, mode, max_scan)                                                                        \
    DSN_REQUIRE((mode) == DSN_JPEG_420 || (mode) == DSN_JPEG_444 || (mode) == DSN_JPEG_GRAY, name ": mode must be DSN_JPEG_420, _444 or _GRAY"); \
    DSN_REQUIRE((F) >= 0 && (F) <= DSN_JPEGD_MAX_FRAMES, name ": F must be 0 ... 16384");                                      \
    DSN_REQUIRE((H) >= 1 && (W) >= 1 && (H) <= 65535 && (W) <= 65535, name ": H and W must be 1 ... 65535");                   \
    DSN_REQUIRE(dsn_jpegd_workspace_size(1, H, W, mode, max_scan) != 0,                                                        \
                name ": too many blocks (blocks x 1664 must stay below 2^31) or max_scan_bytes above 2^27")
#define DSN_JPEGD_WORKSPACE(name, F, H, W, mode, max_scan)                                                                     \
    DSN_REQUIRE(((uintptr_t)workspace & 255) == 0, name ": workspace must be 256-byte aligned");                               \
    DSN_REQUIRE(workspace_bytes >= dsn_jpegd_workspace_size(F, H, W, mode, max_scan), name ": workspace_bytes is too small")
#define DSN_JPEGD_BITS(name, B)                                                                                                \
    DSN_REQUIRE((B) >= 128 && (B) <= 4096 && (B) % 32 == 0, name ": subseq_bits must be a multiple of 32 from 128 to 4096")

int dsn_jpeg_parse_host(const uint8_t* file_host, size_t bytes, dsn_jpegd_desc* desc_host, int* status) {
    DSN_REQUIRE(file_host && desc_host && status, "dsn_jpeg_parse_host: null argument");
    *status = dsn_jpegd_parse_host(file_host, bytes, desc_host);
    return 0;
}

size_t dsn_jpegd_workspace_bytes(int F, int H, int W, int mode, size_t max_scan_bytes) {
    return dsn_jpegd_workspace_size(F, H, W, mode, max_scan_bytes);
}

int dsn_jpegd_workspace_coef(void* workspace, int F, int H, int W, int mode, size_t max_scan_bytes, int16_t** coef) {
    DSN_JPEGD_COMMON("dsn_jpegd_workspace_coef", F, H, W, mode, max_scan_bytes);
    DSN_REQUIRE(workspace && coef && F >= 1, "dsn_jpegd_workspace_coef: null argument");
    *coef = dsn_jpegd_workspace_coef(workspace, F, H, W, mode, max_scan_bytes);
    return 0;
}

int dsn_jpegd_sync(const uint8_t* files, size_t files_bytes, const int64_t* offsets, const dsn_jpegd_desc* desc, int F, int H, int W,
                   int mode, size_t max_scan_bytes, int subseq_bits, int restart, int rounds, uint32_t* out_converged, int32_t* out_rounds,
                   void* workspace, size_t workspace_bytes, void* stream) {
    DSN_JPEGD_COMMON("dsn_jpegd_sync", F, H, W, mode, max_scan_bytes);
    DSN_JPEGD_BITS("dsn_jpegd_sync", subseq_bits);
    DSN_REQUIRE(rounds >= 0 && rounds <= 65536, "dsn_jpegd_sync: rounds must be 0 ... 65536");
    if (F == 0) return 0;
    DSN_REQUIRE(files && offsets && desc && workspace, "dsn_jpegd_sync: null argument");
    DSN_REQUIRE(((uintptr_t)files & 15) == 0 && files_bytes % 16 == 0, "dsn_jpegd_sync: files must be 16-byte aligned and files_bytes a multiple of 16");
    DSN_REQUIRE((((uintptr_t)offsets & 7) | ((uintptr_t)desc & 3) | ((uintptr_t)out_converged & 3) | ((uintptr_t)out_rounds & 3)) == 0,
                "dsn_jpegd_sync: a pointer is not aligned to its element");
    DSN_JPEGD_WORKSPACE("dsn_jpegd_sync", F, H, W, mode, max_scan_bytes);
    dsn_launch_jpegd_sync(files, files_bytes, offsets, desc, F, H, W, mode, max_scan_bytes, subseq_bits, restart != 0, rounds, out_converged,
                          out_rounds, workspace, (hipStream_t)stream);
    return dsn_check_launch("dsn_jpegd_sync");
}

int dsn_jpegd_coefficients(const dsn_jpegd_desc* desc, int F, int H, int W, int mode, size_t max_scan_bytes, int subseq_bits, int16_t* coef,
                           uint32_t* out_status, void* workspace, size_t workspace_bytes, void* stream) {
    DSN_JPEGD_COMMON("dsn_jpegd_coefficients", F, H, W, mode, max_scan_bytes);
    DSN_JPEGD_BITS("dsn_jpegd_coefficients", subseq_bits);
    if (F == 0) return 0;
    DSN_REQUIRE(desc && coef && out_status && workspace, "dsn_jpegd_coefficients: null argument");
    DSN_REQUIRE((((uintptr_t)coef & 15) | ((uintptr_t)desc & 3) | ((uintptr_t)out_status & 3)) == 0,
                "dsn_jpegd_coefficients: coef must be 16-byte aligned, desc and out_status 4-byte aligned");
    DSN_JPEGD_WORKSPACE("dsn_jpegd_coefficients", F, H, W, mode, max_scan_bytes);
    dsn_launch_jpegd_coefficients(desc, F, H, W, mode, max_scan_bytes, subseq_bits, coef, out_status, workspace, (hipStream_t)stream);
    return dsn_check_launch("dsn_jpegd_coefficients");
}

int dsn_jpegd_pixels(const int16_t* coef, const uint32_t* status, const dsn_jpegd_desc* desc, int F, int H, int W, int mode,
                     size_t max_scan_bytes, int rgb, int gray_out, uint8_t* out, void* workspace, size_t workspace_bytes, void* stream) {
    DSN_JPEGD_COMMON("dsn_jpegd_pixels", F, H, W, mode, max_scan_bytes);
    DSN_REQUIRE(!gray_out || mode == DSN_JPEG_GRAY, "dsn_jpegd_pixels: gray_out needs mode DSN_JPEG_GRAY");
    if (F == 0) return 0;
    DSN_REQUIRE(coef && desc && out && workspace, "dsn_jpegd_pixels: null argument");
    DSN_REQUIRE((((uintptr_t)coef & 15) | ((uintptr_t)desc & 3) | ((uintptr_t)status & 3)) == 0,
                "dsn_jpegd_pixels: coef must be 16-byte aligned, desc and status 4-byte aligned");
    DSN_JPEGD_WORKSPACE("dsn_jpegd_pixels", F, H, W, mode, max_scan_bytes);
    dsn_launch_jpegd_pixels(coef, status, desc, F, H, W, mode, max_scan_bytes, rgb != 0, gray_out != 0, out, workspace, (hipStream_t)stream);
    return dsn_check_launch("dsn_jpegd_pixels");
}

int dsn_jpeg_decode(const uint8_t* files, size_t files_bytes, const int64_t* offsets, const dsn_jpegd_desc* desc, int F, int H, int W,
                    int mode, size_t max_scan_bytes, int subseq_bits, int rounds, int rgb, int gray_out, uint8_t* out, uint32_t* out_status,
                    int32_t* out_rounds, void* workspace, size_t workspace_bytes, void* stream) {
    DSN_JPEGD_COMMON("dsn_jpeg_decode", F, H, W, mode, max_scan_bytes);
    DSN_JPEGD_BITS("dsn_jpeg_decode", subseq_bits);
    DSN_REQUIRE(rounds >= 1 && rounds <= 65536, "dsn_jpeg_decode: rounds must be 1 ... 65536");
    DSN_REQUIRE(!gray_out || mode == DSN_JPEG_GRAY, "dsn_jpeg_decode: gray_out needs mode DSN_JPEG_GRAY");
    if (F == 0) return 0;
    DSN_REQUIRE(files && offsets && desc && out && out_status && workspace, "dsn_jpeg_decode: null argument");
    DSN_REQUIRE(((uintptr_t)files & 15) == 0 && files_bytes % 16 == 0, "dsn_jpeg_decode: files must be 16-byte aligned and files_bytes a multiple of 16");
    DSN_REQUIRE((((uintptr_t)offsets & 7) | ((uintptr_t)desc & 3) | ((uintptr_t)out_status & 3) | ((uintptr_t)out_rounds & 3)) == 0,
                "dsn_jpeg_decode: a pointer is not aligned to its element");
    DSN_JPEGD_WORKSPACE("dsn_jpeg_decode", F, H, W, mode, max_scan_bytes);
    hipStream_t st = (hipStream_t)stream;
    int16_t* coef = dsn_jpegd_workspace_coef(workspace, F, H, W, mode, max_scan_bytes);
    dsn_launch_jpegd_sync(files, files_bytes, offsets, desc, F, H, W, mode, max_scan_bytes, subseq_bits, true, rounds, nullptr, out_rounds,
                          workspace, st);
    dsn_launch_jpegd_coefficients(desc, F, H, W, mode, max_scan_bytes, subseq_bits, coef, out_status, workspace, st);
    dsn_launch_jpegd_pixels(coef, out_status, desc, F, H, W, mode, max_scan_bytes, rgb != 0, gray_out != 0, out, workspace, st);
    return dsn_check_launch("dsn_jpeg_decode");
}

// ---- PNG decoding (dsn_png.hip) ----
int dsn_png_parse_host(const uint8_t* file_host, size_t bytes, dsn_png_desc* desc_host, uint32_t* segs_host, size_t seg_capacity, int* status) {
    DSN_REQUIRE(file_host && desc_host && status, "dsn_png_parse_host: null argument");
    DSN_REQUIRE(segs_host || seg_capacity == 0, "dsn_png_parse_host: segs_host is null but seg_capacity is not 0");
    *status = dsn_png_parse(file_host, bytes, desc_host, segs_host, seg_capacity);
    return 0;
}

size_t dsn_png_workspace_bytes(int F, int W, int H, int bits, int ctype, size_t max_stream_bytes) {
    return dsn_png_workspace_size(F, W, H, bits, ctype, max_stream_bytes, nullptr);
}

int dsn_png_workspace_layout(int F, int W, int H, int bits, int ctype, size_t max_stream_bytes, size_t* out8_host) {
    DSN_REQUIRE(out8_host, "dsn_png_workspace_layout: null argument");
    DSN_REQUIRE(dsn_png_workspace_size(F, W, H, bits, ctype, max_stream_bytes, out8_host) != 0,
                "dsn_png_workspace_layout: F must be 1 ... 16384, W and H 1 ... 16384, bits / ctype a pair the decoder takes, at most 2^30 raw "
                "bytes and max_stream_bytes at most 2^28");
    return 0;
}

int dsn_png_decode(const uint8_t* files, size_t files_bytes, const int64_t* segs, int n_segs, const int32_t* seg_first, const dsn_png_desc* desc,
                   int F, int W, int H, int bits, int ctype, size_t max_stream_bytes, int channels, int first_channel, int stages, uint8_t* out,
                   uint32_t* out_status, void* workspace, size_t workspace_bytes, void* stream) {
    DSN_REQUIRE(F >= 0 && F <= DSN_PNG_MAX_FILES, "dsn_png_decode: F must be 0 ... 16384");
    DSN_REQUIRE(dsn_png_workspace_size(1, W, H, bits, ctype, max_stream_bytes, nullptr) != 0,
                "dsn_png_decode: W and H must be 1 ... 16384, bits / ctype a pair the decoder takes, with at most 2^30 raw bytes, and "
                "max_stream_bytes at most 2^28");
    DSN_REQUIRE(channels == DSN_PNG_BGR || channels == DSN_PNG_RGB || channels == DSN_PNG_NATIVE,
                "dsn_png_decode: channels must be DSN_PNG_BGR, _RGB or _NATIVE");
    DSN_REQUIRE(stages >= 1 && stages <= DSN_PNG_STAGE_ALL, "dsn_png_decode: stages must be a non-empty set of DSN_PNG_STAGE_* bits");
    DSN_REQUIRE(n_segs >= 0, "dsn_png_decode: n_segs must not be negative");
    if (F == 0) return 0;
    DSN_REQUIRE(files && segs && seg_first && desc && workspace, "dsn_png_decode: null argument");
    DSN_REQUIRE(out || !(stages & DSN_PNG_STAGE_PIXELS), "dsn_png_decode: out is null");
    DSN_REQUIRE((((uintptr_t)segs & 7) | ((uintptr_t)seg_first & 3) | ((uintptr_t)desc & 3) | ((uintptr_t)out_status & 3)) == 0,
                "dsn_png_decode: a pointer is not aligned to its element");
    DSN_REQUIRE(((uintptr_t)workspace & 255) == 0, "dsn_png_decode: workspace must be 256-byte aligned");
    DSN_REQUIRE(workspace_bytes >= dsn_png_workspace_size(F, W, H, bits, ctype, max_stream_bytes, nullptr),
                "dsn_png_decode: workspace_bytes is too small");
    dsn_launch_png_decode(files, files_bytes, segs, n_segs, seg_first, desc, F, W, H, bits, ctype, max_stream_bytes, channels, first_channel != 0,
                          stages, out, out_status, workspace, (hipStream_t)stream);
    return dsn_check_launch("dsn_png_decode");
}

// ---- PNG encoding (dsn_pnge.hip) ----
#define DSN_PNGE_CHUNK(name, chunk)                                                                                            \
    DSN_REQUIRE((chunk) >= DSN_PNGE_CHUNK_MIN && (chunk) <= DSN_PNGE_CHUNK_MAX && ((chunk) & ((chunk) - 1)) == 0,              \
                name ": chunk must be a power of two from 256 to 32768")
#define DSN_PNGE_FRAMES(name, F) DSN_REQUIRE((F) >= 0 && (F) <= DSN_PNG_MAX_FILES, name ": F must be 0 ... 16384")

size_t dsn_png_encode_max_bytes(int W, int H, int channels, int chunk) {
    if (channels != 1 && channels != 3) return 0;
    const size_t n = dsn_pnge_raw_bytes(W, H, channels == 3 ? DSN_PNGE_COLOUR : DSN_PNGE_GRAY);
    const size_t z = n ? dsn_pnge_deflate_max(n, chunk) : 0;
    return z ? z + 63 : 0;
}

size_t dsn_png_encode_workspace_bytes(int F, int W, int H, int mode, int chunk) { return dsn_pnge_workspace_size(F, W, H, mode, chunk); }

size_t dsn_png_deflate_max_bytes(size_t n, int chunk) { return dsn_pnge_deflate_max(n, chunk); }

size_t dsn_png_deflate_workspace_bytes(int F, size_t n, int chunk) { return dsn_pnge_deflate_workspace_size(F, n, chunk); }

int dsn_png_filter(const void* images, int dtype, int F, int H, int W, int mode, int rgb, float scale, int filter, uint8_t* raw,
                   uint32_t* out_status, void* stream) {
    DSN_PNGE_FRAMES("dsn_png_filter", F);
    DSN_REQUIRE(dsn_pnge_raw_bytes(W, H, mode) != 0, "dsn_png_filter: W and H must be 1 ... 16384 and mode DSN_PNGE_GRAY, _COLOUR or _REPLICATE");
    DSN_REQUIRE(dtype == DSN_JPEG_U8 || dtype == DSN_JPEG_F32, "dsn_png_filter: dtype must be DSN_JPEG_U8 or DSN_JPEG_F32");
    DSN_REQUIRE(filter >= 0 && filter <= DSN_PNGE_ADAPTIVE, "dsn_png_filter: filter must be 0 ... 4 or DSN_PNGE_ADAPTIVE");
    if (F == 0) return 0;
    DSN_REQUIRE(images && raw && out_status, "dsn_png_filter: null argument");
    DSN_REQUIRE(dtype == DSN_JPEG_U8 || ((uintptr_t)images & 3) == 0, "dsn_png_filter: a float32 image is not 4-byte aligned");
    DSN_REQUIRE(((uintptr_t)out_status & 3) == 0, "dsn_png_filter: out_status is not 4-byte aligned");
    dsn_launch_png_filter(images, dtype, F, H, W, mode, rgb != 0, scale, filter, raw, out_status, (hipStream_t)stream);
    return dsn_check_launch("dsn_png_filter");
}

int dsn_png_adler(const uint8_t* raw, int F, size_t n, uint32_t* out_adler, void* workspace, size_t workspace_bytes, void* stream) {
    DSN_PNGE_FRAMES("dsn_png_adler", F);
    DSN_REQUIRE(dsn_pnge_deflate_max(n, DSN_PNGE_CHUNK_MAX) != 0, "dsn_png_adler: n must be 1 ... 2^30 + 2^15");
    if (F == 0) return 0;
    DSN_REQUIRE(raw && out_adler && workspace, "dsn_png_adler: null argument");
    DSN_REQUIRE((((uintptr_t)out_adler | (uintptr_t)workspace) & 3) == 0, "dsn_png_adler: out_adler or workspace is not 4-byte aligned");
    DSN_REQUIRE(workspace_bytes >= (size_t)F * 8, "dsn_png_adler: workspace_bytes is below 8 F");
    dsn_launch_png_adler(raw, F, n, out_adler, (uint32_t*)workspace, (hipStream_t)stream);
    return dsn_check_launch("dsn_png_adler");
}

int dsn_png_deflate(const uint8_t* raw, int F, size_t n, int bpp, int row_stride, int chunk, int stored_only, uint8_t* out, size_t capacity,
                    int32_t* out_lengths, uint32_t* out_status, void* workspace, size_t workspace_bytes, void* stream) {
    DSN_PNGE_FRAMES("dsn_png_deflate", F);
    DSN_PNGE_CHUNK("dsn_png_deflate", chunk);
    DSN_REQUIRE(dsn_pnge_deflate_max(n, chunk) != 0, "dsn_png_deflate: n must be 1 ... 2^30 + 2^15");
    DSN_REQUIRE(bpp >= 1 && bpp <= 8 && row_stride >= 1, "dsn_png_deflate: bpp must be 1 ... 8 and row_stride positive");
    if (F == 0) return 0;
    DSN_REQUIRE(raw && out && out_lengths && out_status && workspace, "dsn_png_deflate: null argument");
    DSN_REQUIRE((((uintptr_t)out_lengths | (uintptr_t)out_status) & 3) == 0, "dsn_png_deflate: a pointer is not aligned to its element");
    DSN_REQUIRE(((uintptr_t)workspace & 255) == 0, "dsn_png_deflate: workspace must be 256-byte aligned");
    DSN_REQUIRE(workspace_bytes >= dsn_pnge_deflate_workspace_size(F, n, chunk), "dsn_png_deflate: workspace_bytes is too small");
    dsn_launch_png_deflate(raw, F, n, bpp, row_stride, chunk, stored_only != 0, out, capacity, out_lengths, out_status, workspace,
                           (hipStream_t)stream);
    return dsn_check_launch("dsn_png_deflate");
}

int dsn_huff_lengths(const uint32_t* counts, int B, int n, int limit, uint8_t* lengths, void* stream) {
    DSN_REQUIRE(B >= 0 && B <= 65535, "dsn_huff_lengths: B must be 0 ... 65535");
    DSN_REQUIRE(limit >= 1 && limit <= 15, "dsn_huff_lengths: limit must be 1 ... 15");
    DSN_REQUIRE(n >= 2 && n <= 288 && n <= (1 << limit), "dsn_huff_lengths: n must be 2 ... 288 and at most 2^limit");
    if (B == 0) return 0;
    DSN_REQUIRE(counts && lengths, "dsn_huff_lengths: null argument");
    DSN_REQUIRE(((uintptr_t)counts & 3) == 0, "dsn_huff_lengths: counts is not 4-byte aligned");
    dsn_launch_huff_lengths(counts, B, n, limit, lengths, (hipStream_t)stream);
    return dsn_check_launch("dsn_huff_lengths");
}

int dsn_png_container(const uint8_t* stream_bytes, size_t stream_stride, const int32_t* stream_lengths, const uint32_t* adler,
                      const uint32_t* status_in, int F, int W, int H, int channels, uint8_t* out, size_t capacity, int32_t* out_lengths,
                      uint32_t* out_status, void* workspace, size_t workspace_bytes, void* stream) {
    DSN_PNGE_FRAMES("dsn_png_container", F);
    DSN_REQUIRE(channels == 1 || channels == 3, "dsn_png_container: channels must be 1 or 3");
    DSN_REQUIRE(dsn_pnge_raw_bytes(W, H, DSN_PNGE_GRAY) != 0, "dsn_png_container: W and H must be 1 ... 16384");
    DSN_REQUIRE(stream_stride >= 1 && stream_stride <= ((size_t)1 << 31) - 64, "dsn_png_container: stream_stride must be 1 ... 2^31 - 64");
    if (F == 0) return 0;
    DSN_REQUIRE(stream_bytes && stream_lengths && adler && out && out_lengths && out_status && workspace, "dsn_png_container: null argument");
    DSN_REQUIRE((((uintptr_t)stream_lengths | (uintptr_t)adler | (uintptr_t)status_in | (uintptr_t)out_lengths | (uintptr_t)out_status |
                  (uintptr_t)workspace) & 3) == 0, "dsn_png_container: a pointer is not aligned to its element");
    DSN_REQUIRE(status_in != out_status, "dsn_png_container: status_in and out_status must differ");
    DSN_REQUIRE(workspace_bytes >= (size_t)F * 4, "dsn_png_container: workspace_bytes is below 4 F");
    dsn_launch_png_container(stream_bytes, stream_stride, stream_lengths, adler, status_in, nullptr, F, W, H, channels, out, capacity,
                             out_lengths, out_status, (uint32_t*)workspace, (hipStream_t)stream);
    return dsn_check_launch("dsn_png_container");
}

int dsn_png_encode(const void* images, int dtype, int F, int H, int W, int mode, int rgb, float scale, int filter, int chunk, int stored_only,
                   uint8_t* out, size_t capacity, int32_t* out_lengths, uint32_t* out_status, void* workspace, size_t workspace_bytes,
                   void* stream) {
    DSN_PNGE_FRAMES("dsn_png_encode", F);
    DSN_PNGE_CHUNK("dsn_png_encode", chunk);
    DSN_REQUIRE(dsn_pnge_raw_bytes(W, H, mode) != 0, "dsn_png_encode: W and H must be 1 ... 16384 and mode DSN_PNGE_GRAY, _COLOUR or _REPLICATE");
    DSN_REQUIRE(dtype == DSN_JPEG_U8 || dtype == DSN_JPEG_F32, "dsn_png_encode: dtype must be DSN_JPEG_U8 or DSN_JPEG_F32");
    DSN_REQUIRE(filter >= 0 && filter <= DSN_PNGE_ADAPTIVE, "dsn_png_encode: filter must be 0 ... 4 or DSN_PNGE_ADAPTIVE");
    if (F == 0) return 0;
    DSN_REQUIRE(images && out && out_lengths && out_status && workspace, "dsn_png_encode: null argument");
    DSN_REQUIRE(dtype == DSN_JPEG_U8 || ((uintptr_t)images & 3) == 0, "dsn_png_encode: a float32 image is not 4-byte aligned");
    DSN_REQUIRE(((uintptr_t)workspace & 255) == 0, "dsn_png_encode: workspace must be 256-byte aligned");
    DSN_REQUIRE(workspace_bytes >= dsn_pnge_workspace_size(F, W, H, mode, chunk), "dsn_png_encode: workspace_bytes is too small");
    DSN_REQUIRE((((uintptr_t)out_lengths & 3) | ((uintptr_t)out_status & 3)) == 0, "dsn_png_encode: a pointer is not aligned to its element");
    dsn_launch_png_encode(images, dtype, F, H, W, mode, rgb != 0, scale, filter, chunk, stored_only != 0, out, capacity, out_lengths, out_status,
                          workspace, (hipStream_t)stream);
    return dsn_check_launch("dsn_png_encode");
}

// ---- the distance between meshes (dsn_meshdist.hip) ----
static bool dsn_mesh_dist_box_ok(const float* b) {
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(b[a]) || !std::isfinite(b[3 + a]) || b[a] > b[3 + a]) return false;
    return true;
}

size_t dsn_mesh_dist_workspace_bytes(int64_t n_verts, int64_t n_faces) {
    return dsn_mesh_cc_sizes_ok(n_verts, n_faces) && n_faces > 0 ? dsn_mesh_dist_workspace_size(n_faces) : 0;
}

int dsn_mesh_dist_grid_host(int64_t n_faces, const float* box_host, int* out_g3_host, float* out_cell_host) {
    DSN_REQUIRE(box_host && out_g3_host && out_cell_host, "dsn_mesh_dist_grid_host: null argument");
    DSN_REQUIRE(n_faces > 0 && n_faces < ((int64_t)1 << 31), "dsn_mesh_dist_grid_host: n_faces must be 1 ... 2^31 - 1");
    DSN_REQUIRE(dsn_mesh_dist_box_ok(box_host), "dsn_mesh_dist_grid_host: the box must be finite with lo <= hi");
    dsn_mesh_dist_grid_rule(n_faces, box_host, out_g3_host, out_cell_host);
    return 0;
}

int dsn_mesh_dist_build(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const float* box_host, void* workspace,
                        size_t workspace_bytes, int64_t* out_counts4, void* stream) {
    DSN_REQUIRE(n_verts >= 0 && n_faces >= 0, "dsn_mesh_dist_build: negative count");
    DSN_REQUIRE(dsn_mesh_cc_sizes_ok(n_verts, n_faces), "dsn_mesh_dist_build: 2^31 or more vertices or faces");
    DSN_REQUIRE(n_faces > 0 && n_verts > 0, "dsn_mesh_dist_build: an empty target (no faces or no vertices)");
    DSN_REQUIRE(verts && faces && box_host && workspace, "dsn_mesh_dist_build: null argument");
    DSN_REQUIRE(dsn_mesh_dist_box_ok(box_host), "dsn_mesh_dist_build: the box must be finite with lo <= hi");
    DSN_REQUIRE(workspace_bytes >= dsn_mesh_dist_workspace_size(n_faces), "dsn_mesh_dist_build: workspace_bytes too small (dsn_mesh_dist_workspace_bytes)");
    DSN_REQUIRE(((uintptr_t)workspace & 15) == 0, "dsn_mesh_dist_build: workspace must be 16-byte aligned");
    dsn_launch_mesh_dist_build(verts, faces, n_verts, n_faces, box_host, workspace, out_counts4, (hipStream_t)stream);
    return dsn_check_launch("dsn_mesh_dist_build");
}

int dsn_mesh_dist_query(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const void* workspace, size_t workspace_bytes,
                        const float* points, int64_t n_points, float* out_dist2, int32_t* out_face, float* out_point, void* stream) {
    DSN_REQUIRE(n_verts >= 0 && n_faces >= 0 && n_points >= 0, "dsn_mesh_dist_query: negative count");
    DSN_REQUIRE(dsn_mesh_cc_sizes_ok(n_verts, n_faces) && n_points < ((int64_t)1 << 31), "dsn_mesh_dist_query: 2^31 or more vertices, faces or points");
    DSN_REQUIRE(n_faces > 0 && n_verts > 0, "dsn_mesh_dist_query: an empty target (no faces or no vertices)");
    DSN_REQUIRE(verts && faces && workspace, "dsn_mesh_dist_query: null argument");
    DSN_REQUIRE(n_points == 0 || points, "dsn_mesh_dist_query: null points");
    DSN_REQUIRE(workspace_bytes >= dsn_mesh_dist_workspace_size(n_faces), "dsn_mesh_dist_query: workspace_bytes too small (dsn_mesh_dist_workspace_bytes)");
    DSN_REQUIRE(((uintptr_t)workspace & 15) == 0, "dsn_mesh_dist_query: workspace must be 16-byte aligned");
    dsn_launch_mesh_dist_query(verts, faces, n_verts, n_faces, workspace, points, n_points, out_dist2, out_face, out_point, (hipStream_t)stream);
    return dsn_check_launch("dsn_mesh_dist_query");
}

size_t dsn_mesh_dist_reduce_workspace_bytes(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31) ? dsn_mesh_dist_reduce_workspace_size(n) : 0; }

int dsn_mesh_dist_reduce(const float* dist2, int64_t n, void* workspace, size_t workspace_bytes, double* out_stats6, void* stream) {
    DSN_REQUIRE(n >= 0, "dsn_mesh_dist_reduce: negative count");
    DSN_REQUIRE(n < ((int64_t)1 << 31), "dsn_mesh_dist_reduce: 2^31 or more values");
    DSN_REQUIRE((n == 0 || dist2) && workspace && out_stats6, "dsn_mesh_dist_reduce: null argument");
    DSN_REQUIRE(workspace_bytes >= dsn_mesh_dist_reduce_workspace_size(n), "dsn_mesh_dist_reduce: workspace_bytes too small (dsn_mesh_dist_reduce_workspace_bytes)");
    DSN_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)out_stats6 & 7) == 0, "dsn_mesh_dist_reduce: workspace must be 16-byte, out_stats6 8-byte aligned");
    dsn_launch_mesh_dist_reduce(dist2, n, workspace, out_stats6, (hipStream_t)stream);
    return dsn_check_launch("dsn_mesh_dist_reduce");
}

size_t dsn_mesh_sample_workspace_bytes(int64_t n_faces) { return n_faces > 0 && n_faces < ((int64_t)1 << 31) ? dsn_mesh_sample_workspace_size(n_faces) : 0; }

int dsn_mesh_sample_surface(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, uint64_t seed, int64_t n_samples,
                            void* workspace, size_t workspace_bytes, float* out_points, int32_t* out_face, void* stream) {
    DSN_REQUIRE(n_verts >= 0 && n_faces >= 0 && n_samples >= 0, "dsn_mesh_sample_surface: negative count");
    DSN_REQUIRE(dsn_mesh_cc_sizes_ok(n_verts, n_faces) && n_samples < ((int64_t)1 << 31), "dsn_mesh_sample_surface: 2^31 or more vertices, faces or samples");
    DSN_REQUIRE(n_faces > 0 && n_verts > 0, "dsn_mesh_sample_surface: an empty mesh (no faces or no vertices)");
    DSN_REQUIRE(verts && faces && workspace, "dsn_mesh_sample_surface: null argument");
    DSN_REQUIRE(workspace_bytes >= dsn_mesh_sample_workspace_size(n_faces), "dsn_mesh_sample_surface: workspace_bytes too small (dsn_mesh_sample_workspace_bytes)");
    DSN_REQUIRE(((uintptr_t)workspace & 15) == 0, "dsn_mesh_sample_surface: workspace must be 16-byte aligned");
    dsn_launch_mesh_sample_surface(verts, faces, n_verts, n_faces, seed, n_samples, workspace, out_points, out_face, (hipStream_t)stream);
    return dsn_check_launch("dsn_mesh_sample_surface");
}

}  // extern "C"
