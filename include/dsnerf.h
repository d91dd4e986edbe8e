/*
 * dsnerf.h - C ABI of libdsnerf_hip.so: the MI355X (gfx950) implementation of the
 * Dual-Space-NeRF volume-rendering hot path.
 *
 * The reference (zyhbili/Dual-Space-NeRF) has no FFI layer: its boundary is the Python call
 * surface can_render.Renderer / model.spacenet.DualSpaceNeRF.  Each entry point below replaces
 * the device work behind one reference function (cited per function, paths relative to the
 * reference repo) and is what a ctypes binding inside that function would call; see
 * INTEGRATION.md for the stubs.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; float32 row-major,
 *     indices int32, masks uint8;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - `scene` is an opaque device blob (dsn_scene_bytes(V,F)); V and F are passed with it on every call
 *     (the library keeps no host-side state);
 *   - functions never allocate, never synchronise, never touch the host copy of any tensor:
 *     the caller owns every buffer (sizes from the *_bytes() helpers) and the ordering is the
 *     stream's;
 *   - return 0 on success; non-zero = error, message from dsn_last_error() (thread-local).
 *     There is no CPU fallback: if no gfx950 device / code object is available the call fails.
 */
#ifndef DSNERF_H
#define DSNERF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
#define DSN_EXPORT __attribute__((visibility("default")))
extern "C" {
#endif

#define DSN_ABI_VERSION 8
#define DSN_NUM_PARAMS 33 /* DualSpaceNeRF.state_dict(), model/spacenet.py:18-81,152-172,191-205 */

DSN_EXPORT int dsn_abi_version(void);
DSN_EXPORT const char* dsn_last_error(void);

/* ---- network parameters ------------------------------------------------------------------
 * params33_host: HOST array of 33 DEVICE pointers in state_dict order (nerf.embedding.weight,
 * nerf.stage1.{0,2,4,6}.{weight,bias}, nerf.stage2.{0,2,4}.{weight,bias}, nerf.density_net.0.*,
 * nerf.rgb_net.{1,3}.*, lighting_mlp.lights_encoding.{0,2,4}.*, pose_mlp.{0,2,4}.*), torch
 * Linear layout [out,in].  Replaces nn.Module parameter storage consumed by
 * model/spacenet.py:93-148,174-188,223-236; re-run after every optimizer step / load_state_dict. */
DSN_EXPORT size_t dsn_packed_param_bytes(void);
DSN_EXPORT int dsn_pack_params(const float* const* params33_host, void* packed, void* stream);

/* layout utility, no device work: writes the packed image of 33 HOST arrays into a HOST buffer of
 * dsn_packed_param_bytes() bytes (lets tools / tests inspect the MFMA operand layout without a GPU) */
DSN_EXPORT int dsn_pack_params_host_image(const float* const* params33_host, float* packed_host);

/* ---- body model + per-frame state ----------------------------------------------------------
 * dsn_set_body : can_render.py:382-406 Renderer.load_body_model (canonical_model["meshes"]).
 * dsn_set_frame: per-batch state: posed mesh batch["xyz"] (can_render.py:352-355), centroids
 *   (utils/render_utils.py:94), pose code batch_rod2quat+pose_mlp (model/spacenet.py:223-236,
 *   314-331), embedding row (model/spacenet.py:125-129; zero_code = `net.nerf.w is not None`),
 *   light-centre shift / rotation (model/spacenet.py:254-263; NULL = not set).
 *   light_shift3 = light_center - Th. */
DSN_EXPORT size_t dsn_scene_bytes(int V, int F);
DSN_EXPORT int dsn_set_body(void* scene, const float* canon_vertex, const int32_t* faces, int V, int F, void* stream);
DSN_EXPORT int dsn_set_frame(void* scene, int V, int F, const void* packed, const float* xyz, const float* poses24x3, int frame_idx,
                  int zero_code, const float* light_shift3, const float* rot2x2, const float* rot_center2,
                  void* stream);
/* dsn_set_frame with flags (ABI 3).  DSN_FRAME_FINE_ONLY: of the posed mesh's two nearest-face levels only the fine one is
 * built (it covers the posed centroids' bounding box + 0.12 m: every sample of a ray clipped to the body's bounds, which is
 * all Renderer.render / render_view ever produce, utils/rays_utils.py:63-97 + utils/pts_utils.py:18-58); points beyond it
 * take the exhaustive sweep instead of the coarse lists - the same index, slower for such points, 0.3 ms less per frame. */
#define DSN_FRAME_FINE_ONLY 1
/* DSN_FRAME_LAZY_LISTS (ABI 6; implies DSN_FRAME_FINE_ONLY): dsn_set_frame_ex only lays out the fine level's grid; the candidate
 * lists are built by the frame that uses them - dsn_render_rays[_ex] with DSN_LAZY_LISTS - and only for the cells its own samples
 * lie in (the sampler classifies the samples by cell while it writes them; the build sits between it and the search).  Same kernels,
 * same sweeps, same lists entry for entry as the full build, for fewer cells: the samples of a 512 x 512 frame visit 48 % of the
 * posed mesh's fine cells, a rank's contiguous eighth of a partitioned frame a tenth (0.44 ms of list build per frame -> 0.1).
 * Such a level answers NO other query (its header keeps ok = 0): dsn_warp / dsn_lbs_warp / dsn_render_rays_grad without
 * DSN_GRAD_CACHED on a lazily set frame take the exhaustive sweep - the same index, slowly; set the frame without the flag for
 * those.  dsn_render_rays_train takes DSN_LAZY_LISTS like dsn_render_rays[_ex] (round 6). */
#define DSN_FRAME_LAZY_LISTS 2
DSN_EXPORT int dsn_set_frame_ex(void* scene, int V, int F, const void* packed, const float* xyz, const float* poses24x3, int frame_idx,
                     int zero_code, const float* light_shift3, const float* rot2x2, const float* rot_center2, int flags,
                     void* stream);

/* Pose-only state: what a density-only query needs of a frame (DualSpaceNeRF.forward(density_only=True),
 * model/spacenet.py:223-241, used by Renderer.query_volume can_render.py:280-296 with a batch_info that holds only
 * 'poses') and what the stand-alone SpaceNet.forward(pos, rays, idx, density_only, pose_feats) consumes
 * (model/spacenet.py:93-131): embedding row `frame_idx` (zeroed when zero_code), the 16 pose features - either computed
 * from poses24x3 by batch_rod2quat + pose_mlp, or given explicitly as pose_feat16 (the pose_feats argument; one of the
 * two must be non-NULL, pose_feat16 wins) - and the light / rotation edits.  The target is a scene blob (its mesh is left
 * untouched) or a blob of dsn_pose_state_bytes() bytes, which dsn_field accepts with V = F = 0. */
DSN_EXPORT size_t dsn_pose_state_bytes(void);
DSN_EXPORT int dsn_set_pose(void* scene_or_pose_state, const void* packed, const float* poses24x3, const float* pose_feat16,
                 int frame_idx, int zero_code, const float* light_shift3, const float* rot2x2, const float* rot_center2,
                 void* stream);

/* ---- stage kernels -----------------------------------------------------------------------*/
/* utils/pts_utils.py:18-58 geometry_guided_ray_marching + :3-16 uniform_sampling.
 * near/far [R] are updated in place (reference :52-53).  t_vals [S] = torch.linspace(0,1,S);
 * jitter [R,S] = the torch.rand draw of :12 (NULL in eval).  pts [R,S,3] may be NULL. */
DSN_EXPORT int dsn_sample_gg(const void* scene, int V, int F, const float* ray_o, const float* ray_d, float* near, float* far, int R, int S,
                  const float* t_vals, const float* jitter, float* z_vals, float* pts, void* stream);

/* utils/pts_utils.py:3-16 uniform_sampling alone (cfg.MODEL.sample_points_mode == "uniform",
 * can_render.py:42-51): same arguments, near/far are not modified. */
DSN_EXPORT int dsn_sample_uniform(const void* scene, int V, int F, const float* ray_o, const float* ray_d, float* near, float* far,
                       int R, int S, const float* t_vals, const float* jitter, float* z_vals, float* pts, void* stream);

/* can_render.py:333-379 Renderer.w2l_without_lbs (+ utils/render_utils.py:84-109,
 * utils/geo_utils.py:96-113,138-156,181-200).  pts [N,3]; ray_d [N/S,3] per-ray directions
 * (NULL -> no ray_d_can).  Any output may be NULL.  active_list/active_count (optional): indices of
 * non-transparent points appended in unspecified order (count must be zeroed by the caller). */
DSN_EXPORT int dsn_warp(const void* scene, int V, int F, const float* pts, const float* ray_d, int64_t N, int S, int32_t* face_idx, float* uv,
             float* h, uint8_t* transparent, float* x_c, float* ray_d_can, int32_t* active_list,
             int32_t* active_count, int flags, void* stream);

/* Dormant alternate of the warp (nothing in the reference calls it any more, pinned at function level):
 * utils/render_utils.py:352-403 compute_nn_mesh - blend weights of each point from its nearest posed face (:112-164,
 * bw_type 0 = "rigid_center", 1 = "rigid_interp") and the transparency mask - followed by utils/blend_utils.py:72-81
 * ppts_to_pts, the inverse linear-blend skinning with those weights.  smpl_weights [V,24], joint_transforms [24,4,4]
 * row-major (device).  Outputs (any may be NULL): face_idx [N], weights [N,24], transparent [N], pts_zero [N,3].
 * flags: DSN_NN_EXHAUSTIVE. */
DSN_EXPORT int dsn_lbs_warp(const void* scene, int V, int F, const float* pts, int64_t N, const float* smpl_weights,
                 const float* joint_transforms, int bw_type, int32_t* face_idx, float* weights, uint8_t* transparent,
                 float* pts_zero, int flags, void* stream);

/* model/spacenet.py:93-148 SpaceNet.forward + :301-311 gradient(): sigma [N], essence [N,3],
 * grad = d sigma / d x_c [N,3].  If active_list != NULL only the listed points (count read from
 * active_count on the device) are evaluated and written; the rest are left untouched. */
DSN_EXPORT int dsn_field(const void* scene, int V, int F, const void* packed, const float* x_c, int64_t N, const int32_t* active_list,
              const int32_t* active_count, float* sigma, float* essence, float* grad, int flags, void* stream);

/* The same evaluation in two launches, for eval-mode rendering (what dsn_render_rays does under
 * DSN_SKIP_TRANSPARENT): dsn_field_forward writes sigma/essence for the listed points, appends the points with sigma > 0
 * to pos_list (pos_count zeroed by the caller) and keeps THEIR ReLU patterns in `records` (dsn_field_record_bytes(N) bytes;
 * record k belongs to pos_list[k]); dsn_field_reverse then writes grad = d sigma / d x_c for the points of
 * pos_list only - the others have alpha = 0 exactly (utils/nerf_net_utils.py:24-27: relu(sigma)), so their
 * normal and colour never reach a pixel.  Results are bit-identical to dsn_field's on the points both write. */
DSN_EXPORT size_t dsn_field_record_bytes(int64_t N);
DSN_EXPORT int dsn_field_forward(const void* scene, int V, int F, const void* packed, const float* x_c, int64_t N,
                      const int32_t* active_list, const int32_t* active_count, float* sigma, float* essence,
                      void* records, int32_t* pos_list, int32_t* pos_count, void* stream);
DSN_EXPORT int dsn_field_reverse(const void* scene, int V, int F, const void* packed, const float* x_c, int64_t N,
                      const int32_t* pos_list, const int32_t* pos_count, const void* records, float* grad, float* sigma,
                      float* essence, void* stream);
/* Range of the split-fp16 kernels.  Activations (|h| < 65000) and adjoints (|d sigma/dh| < 4e6) must fit fp16; every
 * split-fp16 kernel watches the values it splits, and a sample that leaves the range is FLAGGED: dsn_field_forward leaves
 * sigma = NaN for it and puts it on pos_list, dsn_field_reverse (which is why it takes sigma / essence, the arrays
 * dsn_field_forward wrote) and dsn_field / dsn_render_rays re-evaluate flagged samples with the exact-fp32 kernel before
 * they return.  Results for such samples are the exact-fp32 kernel's (DSN_FIELD_FP32), bit for bit. */

/* model/spacenet.py:174-188 LightingMLP.forward(normal, xyz_world, view_dir_world, essence_feature) as a pure function:
 * colour [N,3] = (ELU(lights_encoding([normal, xyz_world, view / |view|])) + 1) * essence.  All inputs [N,3] per point.
 * zero_pose_state: scratch of dsn_pose_state_bytes() bytes (cleared here).  flags: DSN_FIELD_FP32. */
DSN_EXPORT int dsn_light(const void* packed, const float* normal, const float* xyz_world, const float* view_dir_world,
              const float* essence, int64_t N, float* colour, void* zero_pose_state, int flags, void* stream);

/* model/spacenet.py:278-298 normal_local2world + :254-265 + :174-188 LightingMLP.forward.
 * x_w = world sample points [N,3], ray_d [N/S,3]; outputs face_idx_canon [N], n_w [N,3],
 * colour [N,3] (any may be NULL except colour). */
DSN_EXPORT int dsn_shade(const void* scene, int V, int F, const void* packed, const float* x_c, const float* grad, const float* x_w,
              const float* ray_d, const float* essence, int64_t N, int S, const int32_t* active_list,
              const int32_t* active_count, int32_t* face_idx_canon, float* n_w, float* colour, int flags, void* stream);

/* can_render.py:115-120 (transparent sigma-zeroing) + utils/nerf_net_utils.py:5-56 raw2outputs.
 * colour [R,S,3], sigma [R,S], transparent [R,S] (NULL = none), noise [R,S] = randn*raw_noise_std
 * (NULL in eval).  weights [R,S] may be NULL. */
DSN_EXPORT int dsn_composite(const float* colour, const float* sigma, const uint8_t* transparent, const float* z_vals,
                  const float* ray_d, const float* noise, int R, int S, float* rgb_map, float* disp_map,
                  float* acc_map, float* weights, float* depth_map, void* stream);

/* ---- "next" row: the step in front of the path -------------------------------
 * utils/rays_utils.py:16-30 get_rays + :63-97 get_near_far, as composed by my_sample_ray(nrays<=0) (:176-184):
 * K, R [3,3], T [3], bounds [2,3] (min xyz; max xyz) are float64 DEVICE arrays (the reference's numpy dtype).
 * Outputs for all H*W pixels (row-major): ray_o, ray_d [H*W,3], near, far [H*W] (0 where the ray does not cross the
 * box exactly twice), mask_at_box [H*W].  The caller compacts with the mask like the reference does (:181-183). */
#define DSN_RAYS_ZJU 0   /* utils/rays_utils.py:16-30,63-97: un-normalised directions, padded box, "exactly two faces" test in float64 */
#define DSN_RAYS_H36M 1  /* utils/h36m_utils.py:14-28,61-76 (get_rays_within_bounds :162-176): unit directions (normalised in
                          * float64), float32 slab test on the unpadded bounds with the +-1e-5 direction clamp; a NaN
                          * plane parameter is a miss, as numpy's minimum / max keep it.  H * W at most (2^31 - 1) / 3. */
DSN_EXPORT int dsn_camera_rays(const double* K3x3, const double* R3x3, const double* T3, const double* bounds2x3, int H, int W,
                    int convention, float* ray_o, float* ray_d, float* near, float* far, uint8_t* mask_at_box, void* stream);

/* ---- a training batch drawn on the device: utils/rays_utils.py:104-172 my_sample_ray (DSN_RAYS_ZJU) and
 * utils/h36m_utils.py:78-146 sample_ray_h36m (DSN_RAYS_H36M) from an image, its masks and the camera in device memory.
 * Not numpy's random stream and not cv2.fillPoly's outline pixels: the rule below, which tests/train_rays_restate.py restates in
 * numpy and tests/golden/train_rays.npz pins to the reference's own two functions (run with that fill and those draws).
 *
 * Box mask (get_bound_2d_mask): the eight corners of `bounds` in get_bound_corners' order (corner t: x = max where t & 4, y = max
 *   where t & 2, z = max where t & 1), cam = ((x R[c][0] + y R[c][1]) + z R[c][2]) + T[c], pix = (cam0 K[c][0] + cam1 K[c][1]) +
 *   cam2 K[c][2], (u, v) = round-half-even(pix0 / pix2, pix1 / pix2), all float64.  The mask is the union of the six loops as the
 *   reference writes them - {0,1,3,2} {4,5,7,6,5} {0,1,5,4} {2,3,7,6} {0,2,6,4} {1,3,7,5}, each closed from its last vertex to its
 *   first; the second keeps the reference's closing typo and is the triangle 5-7-6 plus the segment 4-5.  Pixel (x, y) belongs to a
 *   loop if it lies on one of its segments (cross product 0, inside the segment's box) or its winding number is non-zero (edge a->b
 *   counts +1 when ay <= y < by and cross > 0, -1 when by <= y < ay and cross < 0, cross = (bx-ax)(y-ay) - (by-ay)(x-ax)); exact
 *   64-bit integers.  NOT the convex hull of the rounded corners: corners round independently and the two differ by a few pixels.
 *   A corner with camera z <= 0, pix2 <= 0, a non-finite projection or |u|, |v| >= 2^29 is an argument error; K, R, T live on the
 *   device, so it is reported as status DSN_TRAIN_RAYS_BAD_CAMERA (dsn_bound_mask: an all-zero mask).  cv2.fillPoly additionally
 *   paints the outline pixels of its line drawing; a caller who needs those passes its own mask as bound_mask_in (values 0 / 1).
 * Classes, each listed in row-major pixel order (np.argwhere), b = (bound == 1):
 *   DSN_RAYS_ZJU  (mask_a = msk_cihp):                 body mask_a != 0;  face mask_a == 2;  random b;  rgb = img[coord]
 *   DSN_RAYS_H36M (mask_a = msk, mask_b = msk_cihp):   body b && mask_a == 1;  face mask_b == 2 (not cut by the box);
 *                                                      random b && mask_a != 100;  rgb = b ? img[coord] : 0 (h36m_utils.py:85-88)
 * Rounds, the reference's while loop: with rem rays missing, n_body = floor(rem 6 / 10), n_face = floor(rem 5 / 100) (= Python's
 *   int(rem * 0.6), int(rem * 0.05) for every rem <= 70000), n_rand = rem - n_body - n_face; the face draws are left out of the round
 *   when the face class is empty.  The drawn coordinates are body, face, random in slot order; each gets its ray and the
 *   convention's box test (dsn_camera_rays' per-pixel rule, bit for bit), the accepted ones are appended in order; the loop ends at
 *   rem == 0.  An empty body or random class: DSN_TRAIN_RAYS_EMPTY_CLASS (the reference raises ValueError, low >= high).  rem > 0
 *   after DSN_TRAIN_RAYS_MAX_ROUNDS rounds: DSN_TRAIN_RAYS_SHORT (the reference would loop for ever).
 * Draws: slot k (0-based, within its class) of class c (0 body, 1 face, 2 random) in round r (0-based) picks list entry
 *   (h(seed, r, c, k) * count_c) >> 32 (64-bit product), with the 32-bit counter hash
 *     mix(x): x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B; x ^= x >> 16
 *     h = mix(mix(seed + 0x9E3779B9 * (3 r + c)) ^ k)            (all modulo 2^32)
 *   a pure function of its arguments: the same call gives the same batch, bit for bit.
 * Outputs (device, n = nrays): ray_o, ray_d [n,3], near, far [n] float32 with the bits dsn_camera_rays writes for the pixel;
 *   coord [n,2] int64 (row, col); rgb [n,3] float32 from img_f64 or img_f32 ([H,W,3]; exactly one non-NULL); occupancy [n] uint8 =
 *   occupancy_src[coord] (both NULL or both given); mask_at_box [n] = 1; bound_mask_out [H,W] uint8 = the box mask (a copy of
 *   bound_mask_in when given) - the batch's mybound_mask; status (int32) and rounds (int32, rounds run).  With a status other than
 *   DSN_TRAIN_RAYS_OK the rows behind the accepted rays are zero (mask_at_box 0).
 * mask_b is required by DSN_RAYS_H36M and ignored by DSN_RAYS_ZJU.  Rejected by the return value: null arguments, H or W <= 0,
 * H W >= 2^31, nrays outside 1 ... DSN_TRAIN_RAYS_MAX_RAYS, an unknown convention, both or neither image pointer, occupancy
 * without occupancy_src (or the reverse), a workspace smaller than dsn_train_rays_workspace_bytes(H, W, nrays) (0 for bad sizes) or
 * not 16-byte aligned.  The workspace may hold anything on entry.  Kernels only: no allocation, no copy to the host, no
 * synchronisation; no atomics. */
#define DSN_TRAIN_RAYS_OK 0
#define DSN_TRAIN_RAYS_EMPTY_CLASS 1
#define DSN_TRAIN_RAYS_SHORT 2
#define DSN_TRAIN_RAYS_BAD_CAMERA 3
#define DSN_TRAIN_RAYS_MAX_ROUNDS 64
#define DSN_TRAIN_RAYS_MAX_RAYS 65536
DSN_EXPORT int dsn_bound_mask(const double* K3x3, const double* R3x3, const double* T3, const double* bounds2x3, int H, int W,
                              uint8_t* mask_out, void* stream);
DSN_EXPORT size_t dsn_train_rays_workspace_bytes(int H, int W, int nrays);
DSN_EXPORT int dsn_train_rays(const double* K3x3, const double* R3x3, const double* T3, const double* bounds2x3, int H, int W,
                              int convention, const double* img_f64, const float* img_f32, const uint8_t* mask_a, const uint8_t* mask_b,
                              const uint8_t* bound_mask_in, const uint8_t* occupancy_src, int nrays, uint32_t seed, float* ray_o,
                              float* ray_d, float* near, float* far, int64_t* coord, float* rgb, uint8_t* occupancy,
                              uint8_t* mask_at_box, uint8_t* bound_mask_out, int32_t* status, int32_t* rounds, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---- image epilogue on the device ----------------------------------------------------------
 * utils/render_utils.py:466-472 post_process: row k of the compacted per-ray outputs (rgb [R,3], disp/acc/depth [R],
 * the rays of the pixels where mask_at_box is set, in pixel order) goes to the k-th masked pixel of the [H,W] images;
 * all other pixels are zero.  clamp_rgb != 0 applies test.py:62-63's clamp to [0,1] to the colour image.
 * disp/acc/depth and their images may be NULL.  workspace: dsn_image_workspace_bytes(H,W). */
DSN_EXPORT size_t dsn_image_workspace_bytes(int H, int W);
DSN_EXPORT int dsn_image_scatter(const float* rgb, const float* disp, const float* acc, const float* depth, int R,
                      const uint8_t* mask_at_box, int H, int W, int clamp_rgb, float* img_rgb, float* img_disp,
                      float* img_acc, float* img_depth, void* workspace, void* stream);
/* metrics.py:8-21 mse / psnr of an [H,W,3] float32 image against the ground truth (float64 as in the reference's
 * batch["img"], or float32; exactly one of gt_f64 / gt_f32 non-NULL), over all pixels and over mask_at_box
 * (test.py:70-71).  out4 (device, float64) = {mse_all, mse_masked, psnr_all, psnr_masked}; mask may be NULL. */
DSN_EXPORT int dsn_image_psnr(const float* img_rgb, const double* gt_f64, const float* gt_f32, const uint8_t* mask_at_box,
                   int H, int W, double* out4, void* workspace, void* stream);
/* DSN image SSIM: metrics.py:23-38 ssim_metric (test.py:73-75), i.e. scikit-image 0.15 compare_ssim(multichannel=True) of
 * the float64 images that are zero outside mask_at_box, cropped to cv2.boundingRect(mask_at_box): per channel a 7 x 7 uniform
 * window, data range 2 (float64's dtype range), sample covariance (49/48), the mean of S over the crop without its 3-pixel
 * border; the mean over the three channels.  F frames of one size: img_rgb [F,H,W,3] float32 (clamp_rgb != 0 clamps it to
 * [0,1] first, as test.py:62-63), ground truth [F,H,W,3] (exactly one of gt_f64 / gt_f32 non-NULL), mask_at_box [F,H,W].
 * Out (device): out_ssim [F] float64, out_rect [F,4] int32 = {x, y, w, h} of the crop, out_status [F] int32 = DSN_SSIM_*.
 * A crop side below 7 has no SSIM (skimage raises "win_size exceeds image extent"): status != DSN_SSIM_OK and out_ssim = NaN.
 * A frame's result is the same bits on every call and in any batch.  workspace: dsn_image_ssim_workspace_bytes(F,H,W), any
 * contents. */
#define DSN_SSIM_OK 0
#define DSN_SSIM_CROP_TOO_SMALL 1   /* the bounding rectangle is narrower or lower than 7 pixels */
#define DSN_SSIM_EMPTY_MASK 2       /* no mask pixel set (cv2.boundingRect: 0 x 0) */
DSN_EXPORT size_t dsn_image_ssim_workspace_bytes(int F, int H, int W);
DSN_EXPORT int dsn_image_ssim(const float* img_rgb, const double* gt_f64, const float* gt_f32, const uint8_t* mask_at_box,
                   int F, int H, int W, int clamp_rgb, double* out_ssim, int32_t* out_rect, int32_t* out_status,
                   void* workspace, void* stream);

/* ---- the trainer's loss on the device (an addition within ABI 8: no existing entry point changes) -------------------------------------
 * utils/loss.py make_loss: MSELoss / SmoothL1Loss, each with the optional LOSSwMask term and its in-place acc_map[occupancy == 1] = 1,
 * and the psnr(coarse["color"], batch["rgb"]) trainer.py takes of the same tensors on every step - one pass over the batch forward, one
 * backward that writes the two seed arrays of dsn_render_rays_grad (d_rgb, d_acc).
 *   color [R,3] float32; the target [R,3] float32 or float64 (exactly one of target_f32 / target_f64 non-NULL, as dsn_image_psnr);
 *   acc [R] float32 or NULL; occupancy [R] uint8 or float32 (at most one of occ_u8 / occ_f32 non-NULL).  The mask term is on iff an
 *   occ_* pointer is given, and acc must be given then.  kind: DSN_LOSS_L2 or DSN_LOSS_SMOOTH_L1.
 * The rule, all in float64 (parentheses give the order of the products; the sums' order is fixed but not part of the rule):
 *   d = (double)color - (double)target, per element.
 *   term      L2: d d.   Smooth-L1 (torch's default beta = 1): 0.5 d d where |d| < 1, else |d| - 0.5.
 *   loss_rgb  = the mean of term over the 3R elements.
 *   mse       = the mean of d d over the 3R elements, in both kinds (what the trainer's psnr needs).
 *   psnr      = -10 log10(mse): +inf at mse = 0, as torch gives.
 *   mask term a' = 1 where occ == 1, else acc;  loss_mask = 0.1 (the mean over R of |a' - occ|).  occ keeps whatever value it has: it
 *             is not assumed to be 0 or 1.  acc_overwrite != 0: the kernel also stores 1.0f into acc where occ == 1 (the reference's
 *             side effect, in the same pass; acc is not written otherwise).
 *   out4 (device, float64) = {loss_rgb, loss_mask, mse, psnr}; loss_mask is 0 when the term is off.  NaN inputs propagate as in torch.
 *   R = 0 is a valid call: nothing is read (the per-ray pointers and the workspace may be NULL), loss_rgb, mse and - with the mask
 *   term on - loss_mask are NaN (the mean of nothing), and so is psnr.
 * dsn_train_loss_grad: the derivatives of the two losses with respect to color and acc, times their upstream gradients.
 *   up_rgb, up_mask: DEVICE float32 scalars, read by the kernel (no synchronisation, no multiply launches in the caller's autograd
 *   chain); a NULL pointer means 0 for that term.  s = 1.0 / (3R) and m = 0.1 / R are computed on the host in double.
 *   g_color[i] = (float)(((double)up_rgb s) e)  with  e = 2 d (L2);  e = d where |d| < 1, else sign(d) (Smooth-L1).
 *   g_acc[r]   = (float)(((double)up_mask m) sign(acc - occ)) where occ != 1, and exactly +0 where occ == 1; acc - occ in double.
 *   sign(x) = 1 for x > 0, -1 for x < 0, +0 for x == 0 (as torch's L1 backward), NaN for NaN.  acc is read only where occ != 1, so it
 *   does not matter whether the overwrite has happened.  g_acc may be NULL; with the mask term off a given g_acc is filled with zeros.
 *   One thread per element, one writer per word, no atomics.  R = 0 launches nothing.
 * Reduction of the forward: workgroup b sums rays [b DSN_LOSS_SHARE, (b + 1) DSN_LOSS_SHARE) - a function of R alone, not of the
 * device - into three fp64 partials in the workspace; a second one-workgroup launch adds the partials in index order.  No
 * floating-point atomics: every call returns the same bits, whatever the workspace (dsn_train_loss_workspace_bytes(R) bytes; 0 for
 * a bad R) held before.
 * Rejected (non-zero, dsn_last_error): R < 0 or 2^31 and more, a kind out of range, both target pointers - or, with R > 0, neither -,
 * both occupancy pointers, an occupancy pointer without acc, null color / out4 / workspace / g_color.  No allocation, no
 * synchronisation, all on `stream`. */
#define DSN_LOSS_L2 0
#define DSN_LOSS_SMOOTH_L1 1
#define DSN_LOSS_SHARE 256         /* rays per workgroup of the forward */
DSN_EXPORT size_t dsn_train_loss_workspace_bytes(int64_t R);
DSN_EXPORT int dsn_train_loss(const float* color, const float* target_f32, const double* target_f64, float* acc, const uint8_t* occ_u8,
                              const float* occ_f32, int64_t R, int kind, int acc_overwrite, double* out4, void* workspace, void* stream);
DSN_EXPORT int dsn_train_loss_grad(const float* color, const float* target_f32, const double* target_f64, const float* acc,
                                   const uint8_t* occ_u8, const float* occ_f32, int64_t R, int kind, const float* up_rgb,
                                   const float* up_mask, float* g_color, float* g_acc, void* stream);

/* ---- the optimizer step on the device (an addition within ABI 8: no existing entry point changes) ---------------------------------
 * solver/build.py:9-15 builds torch.optim.Adam and trainer.py:80 steps it: with the model's 33 small tensors a chain of multi-tensor
 * launches, and a re-pack of the MFMA image in front of the next render.  dsn_adam_step updates every tensor of the call in one launch
 * (a table of segments in the kernel arguments; more than DSN_ADAM_TABLE tensors with a gradient: one launch per table) and, given
 * `packed`, leaves the image of the new parameters behind it on the same stream.
 *   params_host, grads_host, exp_avgs_host, exp_avg_sqs_host: HOST arrays of `count` DEVICE pointers to float32 arrays of n_host[i]
 *   elements; 4-byte alignment is enough (a view into a larger buffer), 16-byte aligned tensors take 16-byte accesses.  A NULL
 *   gradient skips the tensor (torch skips parameters whose .grad is None): nothing of it is read or written, its other pointers may
 *   be NULL.  So does n_host[i] = 0.  lr_host, weight_decay_host: `count` doubles each (param groups differ).  beta1, beta2, eps
 *   and the step count t (1 for the first step, the same for every tensor of the call) are doubles.
 * The rule.  Host scalars, computed in double and rounded to float32 once each (dsn_adam_scalars_host returns them):
 *   w1 = f32(1 - beta1), w2 = f32(1 - beta2), b2 = f32(beta2), e = f32(eps), wd = f32(weight_decay),
 *   ss = f32(lr / (1 - pow(beta1, t))), c2 = f32(sqrt(1 - pow(beta2, t))).
 * Per element, float32, one IEEE rounding per operation, nothing fused, division and square root correctly rounded (parentheses give
 * the order):
 *   g' = g + wd p  where wd != 0, else g                    (L2 decay: the gradient, not the parameter, takes it)
 *   m' = m + w1 (g' - m)
 *   v' = b2 v + w2 (g' g')
 *   p' = p - ss (m' / (sqrt(v') / c2 + e))
 * and m', v', p' are stored.  This is torch/optim/adam.py's _single_tensor_adam operation for operation (add with alpha, lerp's
 * low-weight branch, mul_ then addcmul_, sqrt / div / add_, addcdiv_), so a numpy float32 restatement reproduces every bit
 * (tests/adam_restate.py).  Nothing is skipped or clamped: NaN and infinite gradients propagate as the rule says, g = 0 with v = 0
 * gives 0 / e.  lr = 0 (a frozen group): ss = 0, m' and v' advance and p' = p - 0 x quotient keeps p's bits wherever the quotient is
 * finite (the one exception IEEE makes: p = -0 with a negative quotient becomes +0).
 *   packed: NULL, or the image of dsn_packed_param_bytes() bytes; then the table must be the model's 33 tensors in state_dict order
 *   (count = DSN_NUM_PARAMS, the lengths of the model's tensors, no NULL parameter), and after the update the call enqueues what
 *   dsn_pack_params enqueues, on the new parameters: the image equals dsn_pack_params' of them, calibrations included (the screen's
 *   margin and the early-stop colour scale are back at their defaults).
 * Kernel: 256 threads, DSN_ADAM_BLOCK elements per workgroup, the grid the sum of the segments' workgroups (a launch also ends before
 * its grid would reach 2^24 workgroups: grid x 256 threads stays below the runtime's 2^32; sizes near that were not run); a workgroup finds its
 * segment by its index in the prefix of workgroup counts the table carries.  One writer per word, no atomics, no LDS: the same call
 * from the same state gives the same bits.  The device pointers are arguments: no process state is kept.  No allocation, no
 * synchronisation, all on `stream`.
 * Rejected before anything is enqueued: count < 0, null arrays with count > 0, a negative length or one above DSN_ADAM_MAX_N, a tensor with a
 * gradient and n > 0 whose p, m or v is NULL, t < 1 or not finite, a beta outside [0, 1), eps, a lr or a weight_decay that is
 * negative or not finite, `packed` with a table that is not the 33 tensors. */
#define DSN_ADAM_TABLE 48          /* segments per launch */
#define DSN_ADAM_BLOCK 1024        /* elements per workgroup */
#define DSN_ADAM_MAX_N ((int64_t)1 << 33)   /* elements per tensor */
DSN_EXPORT int dsn_adam_step(float* const* params_host, const float* const* grads_host, float* const* exp_avgs_host,
                             float* const* exp_avg_sqs_host, const int64_t* n_host, int count, const double* lr_host,
                             const double* weight_decay_host, double beta1, double beta2, double eps, double t, void* packed,
                             void* stream);
/* the rule's host scalars (no device work): out7_host = {w1, w2, b2, e, wd, ss, c2} */
DSN_EXPORT int dsn_adam_scalars_host(double lr, double weight_decay, double beta1, double beta2, double eps, double t, float* out7_host);

/* ---- the training step's random draws on the device (an addition within ABI 8: no existing entry point changes) ----------------------
 * can_render.py draws the stratified jitter (utils/pts_utils.py:12, torch.rand(1, R, S)) and the density noise
 * (utils/nerf_net_utils.py:31, torch.randn(R, S) * raw_noise_std) from the CPU default generator.  dsn_train_draws fills both arrays
 * in one launch from a counter-based generator: a draw is a pure function of (seed, step, ray id, sample, kind) - no generator state,
 * no host memory, no copy - so it does not depend on what else drew random numbers, on the order of the rays or on the rank that
 * holds a ray, and a resumed run repeats it from (seed, step) alone.  It is NOT the reference's stream: the values differ from
 * torch.rand / torch.randn's for every seed.
 * The rule.
 *   Generator: Philox4x32 with 10 rounds, multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85.  One
 *   round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to
 *       (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0))          hi / lo: the halves of the 64-bit product
 *   and then adds the increments to (k0, k1); the output is the counter after the tenth round.  Known answers (counter, key -> output):
 *       00000000 x 4, 00000000 x 2                                   -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *       ffffffff x 4, ffffffff x 2                                   -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *       243f6a88 85a308d3 13198a2e 03707344, a4093822 299f31d0       -> d16cfe09 94fdcceb 5001e420 24126ea1
 *   Addressing: key = (seed's low 32 bits, seed's high 32 bits); counter = (q, ray id, step, kind) with q = s / 4 the quad of samples
 *   along the ray, ray id = (uint32)ray_ids[r] where ray_ids is given, else ray_base + r modulo 2^32, kind = 0 for the jitter and 1
 *   for the noise.  The output words x0 .. x3 belong to the samples 4 q .. 4 q + 3; words past S are dropped.  A row therefore depends
 *   on its ray id only, and the first S columns are the same for every S.
 *   Jitter: u = (x >> 8) 2^-24 as float32 - exact, in [0, 1 - 2^-24], on torch.rand's float32 lattice.
 *   Noise: Box-Muller in float64 on the word pairs (x0, x1) and (x2, x3):
 *       u1 = (x0 + 1) 2^-32  (in (0, 1], exact),   u2 = x1 2^-32  (exact),   r = sqrt(-2 log(u1)),   t = 6.283185307179586 u2,
 *       z0 = r cos(t),   z1 = r sin(t)               one float64 rounding per operation, nothing fused,
 *   each z rounded to float32 once and then multiplied in float32 by noise_std (what the host path's mul_ does; noise_std = 0 leaves
 *   zeros that carry z's sign).  |z| <= sqrt(64 ln 2) = 6.66: with a finite noise_std nothing is NaN or infinite.  log, cos and sin are the
 *   device library's float64 functions: against another correct libm a float32 result can differ by one ulp where the float64 value
 *   falls next to a float32 rounding boundary (of the order of 1e-8 of the values); everything else is exact (tests/draws_restate.py).
 *   jitter, noise: float32 [R, S], either may be NULL (not drawn); 4-byte alignment is enough (a view into a larger buffer).
 *   ray_ids: int32 [R] or NULL.
 * Kernel: a thread owns one (ray, quad); 16-byte stores where S % 4 == 0 and the array is 16-byte aligned, scalar stores otherwise
 * (decided per array).  One writer per word, no atomics, no workspace, no synchronisation, all on `stream`.
 * R == 0 or S == 0: success, nothing is enqueued.  Rejected before anything is enqueued: R < 0, S < 0, R S > INT_MAX, a ray_ids, jitter
 * or noise pointer off the 4-byte grid, and - with R S > 0 - jitter and noise both NULL. */
DSN_EXPORT int dsn_train_draws(uint64_t seed, uint32_t step, uint32_t ray_base, const int32_t* ray_ids, int R, int S, float noise_std,
                               float* jitter, float* noise, void* stream);

/* The density screen as a stage (what dsn_render_rays runs first in eval mode): for the listed points (or all N) the
 * plain-fp16 trunk; points whose fp16 density is negative by the safety margin (calibrated for the parameters: dsn_calibrate_screen) get that negative value in sigma [N] and are dropped, the
 * others are appended to keep_list (keep_count zeroed by the caller) for dsn_field_forward. */
DSN_EXPORT int dsn_field_screen(const void* scene, int V, int F, const void* packed, const float* x_c, int64_t N,
                     const int32_t* active_list, const int32_t* active_count, float* sigma, int32_t* keep_list,
                     int32_t* keep_count, void* stream);

/* The screen's margin is a property of the PARAMETERS and travels in `packed`: dsn_pack_params writes the conservative default
 * (0.01); dsn_calibrate_screen measures it for the packed parameters and the scene's current frame state - n_points points
 * around the canonical surface, screen density sigma~ and magnitude S1 against the exact-fp32 density sigma.  With
 * dev = |sigma~ - sigma| / (S1 + 1) and rel = |sigma| / (S1 + 1) a sample is dropped wrongly iff sigma > 0 and dev > margin + rel, so
 * the margin leaves every calibration point a factor 10 of headroom in deviation:  margin = max(10 max(dev - rel / 10), 0.002), or
 * +inf (nothing is ever declared empty) when that exceeds 0.15 - and writes it into `packed`, all on the stream.
 * out (device, optional, 8 floats) = {largest deviation max(dev), margin, fraction of points the screen overflowed on, n_points,
 * fraction of the points the screen drops with that margin (the caller's cue whether the screen pays: it costs ~0.3 of an accurate
 * forward pass per sample), the statistic max(dev - rel / 10), 0, [7]}; out[7] is an INPUT: the statistic of earlier calls on other
 * frame states of the same parameters (0 = none), folded into the margin and the dropped share of this call.
 * dsn_set_screen_margin sets the margin by hand.  workspace: dsn_calibrate_workspace_bytes(n_points). */
DSN_EXPORT size_t dsn_calibrate_workspace_bytes(int64_t n_points);
/* The same calibration on the points that are being RENDERED (round 3): `render_workspace` holds a frame of R rays x S samples
 * behind the geometry phase of dsn_render_rays (DSN_PHASE_GEOMETRY with DSN_SKIP_TRANSPARENT - or a whole frame); the n_points
 * calibration points are the canonical points of its non-transparent samples, evenly spread over the list - as they are for the first
 * half of the set, moved by up to +-2 cm per axis for the second half.  The cube around the canonical centroids that
 * dsn_calibrate_screen draws from (+-0.15 m) reaches far outside the |h| <= 0.1 m shell a non-transparent sample can lie in
 * (utils/render_utils.py:103-109) and - for a trained field - outside everything the training ever saw; what is never rendered
 * should not set the margin, what is rendered must.  Same `out`, same workspace size.  A frame with fewer than 65 536 non-transparent
 * samples (a small ray batch, the first chunk of a chunked frame: a million points drawn from a handful of samples say nothing -
 * ADVICE r03) falls back to the cube; callers fold the cube's statistic in through out[7] in any case (the host mirror does).  The
 * frame's list of non-transparent samples (workspace words / `active`) survives a whole frame, DSN_EARLY_STOP included.  Declared
 * behind dsn_render_rays' flags. */
DSN_EXPORT int dsn_calibrate_screen(const void* scene, int V, int F, void* packed, int64_t n_points, void* workspace, float* out4,
                         void* stream);
DSN_EXPORT int dsn_set_screen_margin(void* packed, float margin, void* stream);

/* diagnostics of the density screen: the plain-fp16 density sigma~ [N] and the magnitude S1 [N] of its terms for
 * every point (no lists, nothing skipped) - lets tests measure the margin against dsn_field's sigma. */
DSN_EXPORT int dsn_debug_screen(const void* scene, int V, int F, const void* packed, const float* x_c, int64_t N,
                     float* sigma_screen, float* s1, int32_t* scratch_list, int32_t* scratch_count, void* stream);

/* ---- training backward: what loss.backward() computes in trainer.py:70-81 -----------------
 * Gradients of L w.r.t. the 33 parameters, given the cotangents of Renderer.render's outputs
 * (utils/loss.py:17-27 uses color and acc_map): d_rgb [R,3] (required), d_disp / d_acc / d_depth [R] and
 * d_weights [R,S] (optional, NULL = zero).  Inputs are what the forward call produced / consumed: z_vals [R,S] (the
 * sampler's output, jitter included), noise [R,S] or NULL, the frame set by dsn_set_frame with the same parameters
 * (frame_idx / zero_code / poses repeated here for the embedding and pose_mlp gradients).  params33_host / grads33_host
 * are HOST arrays of 33 device pointers in state_dict order with torch Linear layouts; every gradient is overwritten.
 * Includes the second-order path through d sigma/dx -> normal -> lighting (model/spacenet.py:251-265) as a forward
 * tangent pass.  `packed` = dsn_pack_params image of the same parameters.  Activations stay resident in `workspace`
 * (dsn_grad_workspace_bytes(R,S), 34 KB per sample). */
DSN_EXPORT size_t dsn_grad_workspace_bytes(int R, int S);
/* Read-only view of that workspace for tests and diagnostics (host function, nothing is launched): byte offsets of the per-row
 * arrays a dsn_render_rays_grad over R x S samples leaves there, N = R S rows each, indexed by sample.  None of them is overwritten
 * before the call returns; rows that are not on the lists hold stale values.  out_offsets_host: n = DSN_GRAD_WS_COUNT entries, in
 * this order (float32 unless said otherwise; [N,k] row-major):
 *   forward   0 transparent (uint8)  1 x_c [N,3]  2 sig  3 ess [N,3]  4 g = d sigma/dx [N,3]  5 n_w [N,3]  6 xl [N,9] = (n_w, x_w, view)
 *             7 hl1 [N,128]  8 hl2 [N,128] (after their ReLUs)  9 pre  10 wl = ELU(pre) + 1  11 col [N,3]  12 rr [N,128] (after ReLU)
 *             13 h[6] [N,256] (the trunk's last layer, after ReLU)
 *   backward  14 d_sig  15 d_col [N,3]  16 d_ess [N,3]  17 d_pre  18 d_hl2 [N,128]  19 d_hl1 [N,128]  20 d_xl [N,9]  21 d_rr [N,128]
 *             (18, 19, 21: behind the ReLU masks, i.e. cotangents of the layers' pre-activations)  22 u = dL/dg [N,3]
 *   lists     23 list1 (int32, rows the forward evaluated)  24 list2 (int32, rows with a non-zero cotangent; both ascending)
 *             25 rowcnt (int32 [2]: entries of list1, of list2)
 * Returns non-zero (dsn_last_error) when n is not DSN_GRAD_WS_COUNT or a size is not positive. */
#define DSN_GRAD_WS_COUNT 26
DSN_EXPORT int dsn_grad_workspace_layout(int R, int S, int64_t* out_offsets_host, int n);
/* Renderer.render in train mode (can_render.py:137-168 with net.training): dsn_render_rays (dense evaluation, jitter / noise
 * as given) that also leaves what its backward needs in `grad_workspace` (dsn_grad_workspace_bytes(R,S)): canonical points,
 * transparency, per-layer activations, sigma-adjoints, relu records, normals.  A following dsn_render_rays_grad on the same
 * inputs with DSN_GRAD_CACHED skips the recomputation of all of it. */
#define DSN_GRAD_CACHED 1
DSN_EXPORT int dsn_render_rays_train(const void* scene, int V, int F, const void* packed, const float* ray_o, const float* ray_d, float* near,
                    float* far, int R, int S, const float* t_vals, const float* jitter, const float* noise, int flags,
                    float* out_rgb, float* out_disp, float* out_acc, float* out_depth, float* out_weights, float* out_z,
                    void* workspace, void* grad_workspace, void* stream);
/* The same with the caller's auxiliary stream + fork / join events (ABI 8; the triple of dsn_render_rays_grad_ex below, all three or
 * none).  The nearest-face search of the batch's FAR canonical points (transparent samples with positive noise: six small kernels,
 * 0.25 ms at 8192 x 64) needs the warp stage's points only, not the networks: it is enqueued on aux_stream beside the field kernel,
 * whose last round of row blocks leaves most of the chip idle (2 844 blocks on 256 CUs at that batch), and joined in front of the
 * normals.  Same kernels, same arguments, same values; NULL triple = dsn_render_rays_train. */
DSN_EXPORT int dsn_render_rays_train_ex(const void* scene, int V, int F, const void* packed, const float* ray_o, const float* ray_d, float* near,
                    float* far, int R, int S, const float* t_vals, const float* jitter, const float* noise, int flags,
                    float* out_rgb, float* out_disp, float* out_acc, float* out_depth, float* out_weights, float* out_z,
                    void* workspace, void* grad_workspace, void* stream, void* aux_stream, void* ev_fork, void* ev_join);
DSN_EXPORT int dsn_render_rays_grad(const void* scene, int V, int F, const void* packed, const float* const* params33_host, const float* poses24x3,
                         int frame_idx, int zero_code, const float* ray_o, const float* ray_d, const float* z_vals,
                         const float* noise, int R, int S, const float* d_rgb, const float* d_disp, const float* d_acc,
                         const float* d_depth, const float* d_weights, float* const* grads33_host, void* workspace,
                         int flags, void* stream);
/* The same with a SECOND stream of the caller's (round 6).  Behind the adjoint of compositing the backward splits into two chains
 * that do not depend on each other - the lighting MLP's backward + the tangent pass, and the colour head's backward + the adjoint
 * pass (trainer.py:70-81 loss.backward() through model/spacenet.py:251-265 on one side, :136-147 on the other) - most of whose
 * kernels are too small to fill the chip.  With aux_stream / ev_fork / ev_join (a hipStream_t and two hipEvent_t, all three or none)
 * the second chain is enqueued on aux_stream between a fork and a join: everything the call enqueues is still ordered after what
 * `stream` held before the call and before what it gets afterwards, and nothing is synchronised on the host.  Same kernels, same
 * values.  dsn_aux_create / dsn_aux_destroy make and free such a triple for callers without a HIP binding of their own; they are
 * the caller's, the library keeps no record of them. */
DSN_EXPORT int dsn_render_rays_grad_ex(const void* scene, int V, int F, const void* packed, const float* const* params33_host, const float* poses24x3,
                         int frame_idx, int zero_code, const float* ray_o, const float* ray_d, const float* z_vals,
                         const float* noise, int R, int S, const float* d_rgb, const float* d_disp, const float* d_acc,
                         const float* d_depth, const float* d_weights, float* const* grads33_host, void* workspace,
                         int flags, void* stream, void* aux_stream, void* ev_fork, void* ev_join);
DSN_EXPORT int dsn_aux_create(void** aux_stream, void** ev_fork, void** ev_join);
DSN_EXPORT int dsn_aux_destroy(void* aux_stream, void* ev_fork, void* ev_join);

/* Backward of DualSpaceNeRF.forward(pos[N,6], rays[N,6], frame_idx, batch_info) (model/spacenet.py:210-266) on explicit
 * points, what autograd computes when a caller differentiates (colour, density) w.r.t. the parameters (can_render.py:97-134
 * render_rays / batchify_pts in train mode): x_world = pos[:, :3], x_canon = pos[:, 3:], view_dir = rays[:, :3],
 * d_colour [N,3] / d_sigma [N] the cotangents of the two outputs, zeros_n = N zero floats (device).  The scene holds the
 * frame (dsn_set_frame with the same parameters).  Every gradient is overwritten; inputs receive no gradient (they are
 * data in the reference too).  workspace: dsn_grad_workspace_bytes(N, 1). */
DSN_EXPORT int dsn_module_grad(const void* scene, int V, int F, const void* packed, const float* const* params33_host,
                    const float* poses24x3, int frame_idx, int zero_code, const float* x_world, const float* x_canon,
                    const float* view_dir, const float* zeros_n, int64_t N, const float* d_colour, const float* d_sigma,
                    float* const* grads33_host, void* workspace, void* stream);

/* ---- fused path: can_render.py:137-168 Renderer.render on R rays --------------------------
 * flags: DSN_SKIP_TRANSPARENT evaluates the networks only on non-transparent samples (exact in
 * eval mode: their sigma is forced to 0 and their colour is multiplied by weight 0; must not be
 * set when noise != NULL).  out_weights / out_z may be NULL. */
#define DSN_SKIP_TRANSPARENT 1
/* nearest-face search by exhaustive scan instead of the exact cell-candidate lists (same result by
 * construction; kept as the on-device cross-check of the lists).  Valid for dsn_warp, dsn_shade, dsn_render_rays. */
#define DSN_NN_EXHAUSTIVE 2
/* evaluate the field with exact-fp32 MFMA (v_mfma_f32_32x32x2_f32, bitwise an fp32 fma chain) instead of the
 * default split-fp16 scheme (3 x v_mfma_f32_32x32x16_f16 on hi/lo operand halves: fp32-equivalent accuracy at
 * 5.3x fewer matrix cycles).  Valid for dsn_field and dsn_render_rays. */
#define DSN_FIELD_FP32 4
/* cfg.MODEL.sample_points_mode == "uniform" (can_render.py:42-51): plain uniform_sampling between the given near/far
 * instead of the geometry-guided interval.  Valid for dsn_render_rays. */
#define DSN_SAMPLE_UNIFORM 8
/* eval-mode density screen, OPT-IN since ABI 5 (rounds 1-3: on unless DSN_NO_SCREEN = 16 was given - the bit now means the opposite):
 * with DSN_SKIP_TRANSPARENT and the split-fp16 field, dsn_render_rays first runs a plain-fp16 pass of the trunk and sends only the
 * samples whose fp16 density is not negative by a safety margin - sigma~ >= -margin (magnitude of its terms + 1) - through the
 * accurate pass; the others contribute exactly zero either way.  The margin is MEASURED for the parameters (dsn_calibrate_screen*:
 * a factor 10 of headroom on a million points; 0.01 until then) and can be audited per frame (DSN_SCREEN_AUDIT): frames come out
 * bit-identical with the screen on or off on everything tested, but that is a statistical statement about the calibration set, not
 * a bound - hence not the default under a "results identical" contract. */
#define DSN_DENSITY_SCREEN 16
/* audit of the density screen: a pseudo-random 1/128 of the samples it declares empty go through the accurate pass anyway
 * (the frame stays exact); afterwards int32 word 40 of `workspace` holds how many were audited, word 44 how many of those have
 * an accurate density > 0 (must be 0: such a sample would have been dropped wrongly) and word 45 the largest such density
 * (float bits). */
#define DSN_SCREEN_AUDIT 32
/* Front-to-back evaluation with ray termination (eval mode: needs DSN_SKIP_TRANSPARENT, split-fp16 field).  raw2outputs
 * (utils/nerf_net_utils.py:24-39) weighs sample i with alpha_i * T_i, T_i = prod_{j<i}(1 - alpha_j + 1e-10) non-increasing
 * along the ray: once T < eps (<= 2^-20) every later sample weighs less than eps and all of them together add less than eps to
 * acc_map (eps * colour to the pixel, eps * far to depth_map).  The frame is evaluated in slices of 8 samples along the rays
 * (S / 32 beyond 256 samples); after each slice T of every ray is advanced with the densities just computed, the next slice
 * leaves out the finished rays (their remaining samples keep density 0), and d sigma/dx, normals and lighting are computed only
 * for samples whose own weight is >= eps.  Worst case against the dense evaluation: the S samples not shaded add up to S eps and
 * the terminated tail to eps, i.e. (S + 1) eps x the largest colour component c, so eps follows S AND c:
 * eps(S, c) = min(2^-20, 1e-4 / (2 (S + 1) max(1, c))) keeps the worst case at half of the 1e-4 bar - ABSOLUTE - at any S for colours
 * up to c (1e-6 typical).  colour = (ELU + 1) x essence is unbounded (model/spacenet.py:174-188): c is a property of the loaded
 * parameters, kept in `packed` (1 after dsn_pack_params; dsn_set_early_stop_colour_scale sets it - the host mirror measures it: every
 * eval frame leaves the largest |colour| its compositor weighed in word 59 of `workspace`, float bits).  When no ray saturates,
 * weights / acc / depth keep their bits and only the colour moves (< eps x colour per unshaded sample).
 * int32 words 56 / 57 of `workspace`: samples left out by termination / samples not shaded. */
#define DSN_EARLY_STOP 64
/* the termination / shading threshold DSN_EARLY_STOP and DSN_STOP_STATS use for rays of S samples (host functions, no device work):
 * dsn_early_stop_eps(S) = dsn_early_stop_eps_scaled(S, 1) */
DSN_EXPORT float dsn_early_stop_eps(int S);
/* samples per uniform slice of an R x S frame: 4 on frames of >= 4 M samples, 8 below, S / 32 (rounded up) beyond 32 slices; rays of
 * more than 2048 samples (a slice would exceed 64 samples) render in one pass whatever the flag says */
DSN_EXPORT int dsn_stop_slice_len(int R, int S);
/* samples per slice of the DSN_STOP_STATS histogram (ABI 8: half the uniform slice where that keeps at most 32 slices - finer borders for
 * the schedule a caller cuts from it; the histogram is (K + 1) x K ints with K = ceil(S / this)) */
DSN_EXPORT int dsn_stop_stats_slice_len(int R, int S);
DSN_EXPORT float dsn_early_stop_eps_scaled(int S, float colour_scale);
/* the factor between the largest colour a frame weighed (word 59 of its workspace) and the colour scale a caller should set from it:
 * 2.  DSN_STOP_STATS applies it itself: its counts and histogram use the threshold for max(the scale in `packed`, 2 x the frame's own
 * largest colour) - the threshold the sliced frames decided by them will run with. */
DSN_EXPORT float dsn_early_stop_colour_headroom(void);
/* colour scale c of the early-stop threshold for THESE parameters (stream-ordered write into `packed`; values < 1 count as 1) */
DSN_EXPORT int dsn_set_early_stop_colour_scale(void* packed, float colour_scale, void* stream);
/* statistics for the caller's decision whether DSN_EARLY_STOP pays (a frame rendered WITHOUT it): word 58 of `workspace` =
 * non-transparent samples that lie in a slice whose ray had T < eps when the slice began (what DSN_EARLY_STOP would leave out;
 * compare with word 0, the non-transparent samples).  Slicing costs a few launches per slice, ~0.5 ms on a 512 x 512 x 64 frame. */
#define DSN_STOP_STATS 128
/* Phases of the fused path.  None of the three bits: the whole frame (all of the above) on `stream`.  With bits set
 * dsn_render_rays enqueues only those parts - DSN_PHASE_GEOMETRY: sampler, cell-major nearest-face search, warp, clears
 * (utils/pts_utils.py:18-58, can_render.py:333-379); DSN_PHASE_FIELD: density screen, canonical field forward / reverse, range
 * fallback, front-to-back slices (model/spacenet.py:93-148,301-311); DSN_PHASE_SHADE: normals, lighting MLP, compositing
 * (model/spacenet.py:278-298,174-188, utils/nerf_net_utils.py:5-56).  A caller with several frames in flight puts geometry and
 * shading of one frame on a stream of their own beside the matrix-bound field kernels of another (the field kernels occupy every
 * compute unit with one persistent workgroup; the geometry kernels are sized to fit into the LDS and registers they leave), with its
 * own events between the three calls; everything that travels between the phases lives in `workspace`.  Same arguments in all
 * three calls; dsn_set_frame belongs in front of the geometry phase, on its stream. */
#define DSN_PHASE_GEOMETRY 256
#define DSN_PHASE_FIELD 512
#define DSN_PHASE_SHADE 1024
/* Frames in flight.  The field kernels are persistent: one workgroup per compute unit walks the tiles of a launch.  With several
 * frames in flight on streams of their own, DSN_SHARE_CUS makes them take 7/8 of the compute units (a multiple of 8: one per XCD less
 * ... 28 of 32 per XCD on the MI355X) and leaves the rest to the neighbours' small kernels: -1.4 % per frame with three frames in
 * flight, +3 to +6 % for a frame that runs alone (profiles/r03_frames_in_flight.txt) - set it only when frames overlap.  Same values. */
#define DSN_SHARE_CUS 2048
/* the scene's frame was set with DSN_FRAME_LAZY_LISTS: this call's geometry phase completes the posed mesh's fine lists - for the
 * cells its samples visit (frames of >= 1 M samples: the cell-major search; those lists belong to THIS call: the next call with the
 * flag builds its own, the next call without it does not walk them), for every cell otherwise (once: the level is an ordinary,
 * fully built one afterwards and later calls find nothing to do).  Without the flag a lazily set frame still renders exactly (every
 * sample takes the exhaustive sweep - also after an earlier call with the flag); with the flag on a fully built level nothing is
 * rebuilt. */
#define DSN_LAZY_LISTS 4096
/* (The test override DSN_STOP_SLICE changes the workspace layout and is read at every call: set it before the workspace is sized
 *  and leave it alone while it is in use.) */
DSN_EXPORT size_t dsn_render_workspace_bytes(int R, int S);
/* The relu records the eval-mode reverse pass reads (224 B per sample with sigma > 0) are the largest item of the workspace.  Frames
 * of more than 2 M samples reserve them for a FRACTION of the samples (a frame of hash-random parameters puts 12 % of its samples
 * there, the converged checkpoint 14 % with front-to-back slices, a briefly trained solid 39 %); samples beyond the capacity are
 * evaluated by a single-launch forward + reverse pass: same values, but their forward pass runs twice.  The capacity is a property of
 * the WORKSPACE, not of the process (ABI 6; ABI 5 kept a process-wide fraction): the records are the last array of the workspace and
 * everything in front of them depends on (R, S) alone, so
 *   dsn_render_workspace_bytes_for(R, S, f)          bytes of a workspace with records for a fraction f of the samples (f <= 0 or
 *                                                    NaN: the default 1/8 = dsn_render_workspace_bytes(R, S); frames of <= 2 M
 *                                                    samples always get records for all of them);
 *   dsn_render_rays_ex(..., workspace, workspace_bytes, ...)
 *                                                    takes the capacity from the size it is handed (0 = "sized by
 *                                                    dsn_render_workspace_bytes(R, S)"); a size below the fixed part fails loudly;
 *   dsn_render_workspace_record_capacity(R, S, bytes) says what a workspace of that size holds (-1: too small).
 * A caller who has seen word 16 of a frame's workspace (samples with sigma > 0) come near the capacity gives ITS workspace more -
 * between frames; two workspaces of one process never size each other.  Host functions, no device work, no state. */
DSN_EXPORT size_t dsn_render_workspace_bytes_for(int R, int S, float record_fraction);
DSN_EXPORT int64_t dsn_render_workspace_record_capacity(int R, int S, size_t workspace_bytes);
DSN_EXPORT int dsn_calibrate_screen_frame(const void* scene, int V, int F, void* packed, const void* render_workspace, int R, int S,
                               int64_t n_points, void* workspace, float* out8, void* stream);
DSN_EXPORT int dsn_render_rays(const void* scene, int V, int F, const void* packed, const float* ray_o, const float* ray_d, float* near,
                    float* far, int R, int S, const float* t_vals, const float* jitter, const float* noise,
                    int flags, float* out_rgb, float* out_disp, float* out_acc, float* out_depth,
                    float* out_weights, float* out_z, void* workspace, void* stream);
/* The same with a SCHEDULE for DSN_EARLY_STOP: slice_lengths_host[0 .. n_slices) (host array, 1 .. 64 samples each, at most 32 slices,
 * adding up to S) instead of uniform slices of 4 / 8 samples.  A slice costs a launch of every field kernel whatever it holds (a
 * 512 x 512 frame's late slices hold 40-90 k samples, one to three rounds of the chip's 32 k-sample capacity), so where few rays end a
 * longer slice is cheaper than two short ones; termination is then checked less often there, i.e. MORE samples are evaluated: the
 * error bound of DSN_EARLY_STOP is unchanged.  The statistics to choose from: a DSN_STOP_STATS frame leaves, from int32 word 256 of
 * `workspace`, hist[g][k] (g = 0 .. K, k = 0 .. K - 1, K = ceil(S / L) uniform slices) = non-transparent samples of slice k on rays whose
 * first slice with T < eps at its start is g (g = K: never) - a group of slices that starts at slice a evaluates slice k >= a on the
 * rays with g > a.  NULL / 0 = uniform slices = dsn_render_rays.  (The host mirror picks the schedule by dynamic programming over
 * that histogram: _lib.choose_stop_schedule.)  workspace_bytes: see dsn_render_workspace_bytes_for. */
DSN_EXPORT int dsn_render_rays_ex(const void* scene, int V, int F, const void* packed, const float* ray_o, const float* ray_d, float* near,
                       float* far, int R, int S, const float* t_vals, const float* jitter, const float* noise,
                       int flags, float* out_rgb, float* out_disp, float* out_acc, float* out_depth,
                       float* out_weights, float* out_z, void* workspace, size_t workspace_bytes, const int32_t* slice_lengths_host,
                       int n_slices, void* stream);

/* ---- relighting sweep (an addition within ABI 8: no existing entry point changes) ------------------------------------------------
 * One eval-mode frame under n_lights light settings (the reference's vis_lighting.py renders every view under ten rotations of the
 * light): geometry, field, early stop, normals and compositing weights run ONCE, each light costs its lighting MLP and its rgb sums.
 * A light edit moves only the world position the lighting MLP sees (model/spacenet.py:254-265): every light's pixels have the bits of
 * dsn_render_rays_ex with that light in the scene's frame state (dsn_set_frame).  The light of the scene's frame state is NOT used.
 *   lights      device array of n_lights records of DSN_LIGHT_RECORD_FLOATS floats
 *               {has_light, light_shift[3], has_rot, rot[4] (row-major 2 x 2), rot_center[2], 0}: the world point x is first rotated
 *               about rot_center in xy when has_rot != 0, then shifted by light_shift when has_light != 0 (dsn_set_frame's arguments);
 *   out_rgb     [n_lights, R, 3]; out_disp / out_acc / out_depth / out_weights / out_z as in dsn_render_rays_ex (light-independent);
 *   light_scratch, light_scratch_bytes
 *               the compact colours of a group of G lights, [G][n_shaded][3] by slot on the shading list: G = as many lights as the
 *               scratch holds (at least one: otherwise the call fails).  n_shaded (<= R S) is known after the field phase: the call
 *               reads that one count word, i.e. it SYNCHRONISES `stream` once.
 * Eval mode only: flags must hold DSN_SKIP_TRANSPARENT; jitter, noise, DSN_FIELD_FP32 and DSN_PHASE_* are rejected; S must be 64 or
 * 128 and workspace / out_weights / out_z 16-byte aligned.  The early-stop guard word (int32 word 59 of `workspace`) holds the largest
 * |colour| weighed under ANY of the lights. */
#define DSN_LIGHT_RECORD_FLOATS 12
/* bytes of light_scratch for n_lights lights in one group on a frame of n_shaded shaded samples (0: bad sizes) */
DSN_EXPORT size_t dsn_render_lights_scratch_bytes(int R, int S, int n_lights, int64_t n_shaded);
DSN_EXPORT int dsn_render_rays_lights(const void* scene, int V, int F, const void* packed, const float* ray_o, const float* ray_d,
                           float* near, float* far, int R, int S, const float* t_vals, const float* jitter, const float* noise, int flags,
                           const float* lights, int n_lights, float* out_rgb, float* out_disp, float* out_acc, float* out_depth,
                           float* out_weights, float* out_z, void* workspace, size_t workspace_bytes, void* light_scratch,
                           size_t light_scratch_bytes, const int32_t* slice_lengths_host, int n_slices, void* stream);

/* ---- decomposition maps (an addition within ABI 8: no existing entry point changes) ------------------------------------------------
 * The model is a decomposition: a sample's colour is (ELU(lighting MLP) + 1) x essence (model/spacenet.py:174-188), the lighting MLP fed
 * by the world normal of normal_local2world (:278-298).  dsn_render_rays_maps is dsn_render_rays_lights that also composites the
 * factors one by one with the frame's own weights w_i (utils/nerf_net_utils.py:18-51; the bits of out_weights).  With e_i the essence
 * (SpaceNet.forward's rgbs, model/spacenet.py:141-147), n_i the unit world normal, L_{k,i} = ELU + 1 under light k (after the light
 * edit of :254-265), summed over the samples i of the frame's SHADING LIST (not transparent, sigma > 0 and - with DSN_EARLY_STOP - not
 * left out by ray termination or the weight cull):
 *   out_albedo  [R,3]           sum w_i e_i
 *   out_normal  [R,3]           sum w_i n_i      world space, NOT renormalised: the acc-weighted mean normal x acc
 *   out_shading [n_lights,R]    sum w_i L_{k,i}
 *   out_rgb     [n_lights,R,3]  sum w_i L_{k,i} e_i      dsn_render_rays_lights' out_rgb, bit for bit
 *   out_max     device, >= 2 floats: the largest |e| (any channel) and the largest L that entered a sum (NaN counts as +inf).
 * A sample off the list adds 0 to every map, as it adds colour 0 to the frame; in one pass (no DSN_EARLY_STOP) that is exact, since
 * such a sample has alpha = 0.  With DSN_EARLY_STOP a map with |q| <= Q on the one-pass list is within (S + 1) (eps + 2^-22) Q of its
 * one-pass value, eps = dsn_early_stop_eps_scaled(S, colour scale): at most S culled samples of weight < eps each and a terminated
 * tail of total weight < eps (1 + S 2^-23), plus the rounding of two float sums of S terms.  Q = 1 for the normal.  The sums run in
 * the compositor's order, whatever the grouping of the lights: every map is deterministic and independent of light_scratch_bytes.
 * Each of out_rgb / out_albedo / out_normal / out_shading / out_max may be NULL.  light_scratch holds 4 floats per shaded sample and
 * light (the colours and the factors of a group).  Restrictions, the single synchronisation, early stop, the density screen, its
 * audit and the slice schedule as for dsn_render_rays_lights; albedo, normal, disp, acc, depth and weights are written with the first
 * group of lights. */
DSN_EXPORT size_t dsn_render_maps_scratch_bytes(int R, int S, int n_lights, int64_t n_shaded);
DSN_EXPORT int dsn_render_rays_maps(const void* scene, int V, int F, const void* packed, const float* ray_o, const float* ray_d,
                         float* near, float* far, int R, int S, const float* t_vals, const float* jitter, const float* noise, int flags,
                         const float* lights, int n_lights, float* out_rgb, float* out_disp, float* out_acc, float* out_depth,
                         float* out_weights, float* out_z, float* out_albedo, float* out_normal, float* out_shading, float* out_max,
                         void* workspace, size_t workspace_bytes, void* light_scratch, size_t light_scratch_bytes,
                         const int32_t* slice_lengths_host, int n_slices, void* stream);
/* Stage entry (per-stage parity, like dsn_composite): the three maps of ONE light from dense per-sample arrays - essence [R S,3],
 * n_w [R S,3], factor [R S] (dsn_shade_factor), sigma [R S], transparent (optional, uint8 [R S]), z_vals [R,S], ray_d [R,3].  A sample
 * counts where it is not transparent and sigma > 0; the arrays are not read elsewhere.  Any S (S = 64 / 128 with 16-byte aligned
 * arrays: the 16-lane form of dsn_render_rays_maps; otherwise one wave per ray).  Outputs: albedo_map [R,3], normal_map [R,3],
 * shading_map [R], weights [R,S], out_max (device, 2 floats) - each may be NULL (a map needs its source array, out_max needs essence
 * and factor), not all of them. */
DSN_EXPORT int dsn_composite_maps(const float* essence, const float* n_w, const float* factor, const float* sigma, const uint8_t* transparent,
                       const float* z_vals, const float* ray_d, int R, int S, float* albedo_map, float* normal_map, float* shading_map,
                       float* weights, float* out_max, void* stream);
/* dsn_shade (normal_local2world + the split-fp16 lighting MLP) that also stores the light factor ELU + 1 of every listed sample in
 * factor [N]; n_w and colour have dsn_shade's bits.  DSN_FIELD_FP32 is rejected. */
DSN_EXPORT int dsn_shade_factor(const void* scene, int V, int F, const void* packed, const float* x_c, const float* grad, const float* x_w,
                     const float* ray_d, const float* essence, int64_t N, int S, const int32_t* active_list,
                     const int32_t* active_count, int32_t* face_idx_canon, float* n_w, float* colour, float* factor, int flags,
                     void* stream);

/* ---- density grid and iso-surface (an addition within ABI 8: no existing entry point changes) -------------------------------------
 * utils/visualizer.py:35-110 Visualizer3D.get_grid_pred_batch: the reference builds grid_pts on the host (get_grid, :170-236),
 * warps them with Renderer.w2l_without_lbs, evaluates Renderer.query_volume in 100 000-point chunks and sets transparent points to 0.
 * dsn_density_grid does all of it on the device for the scene's current frame (dsn_set_frame / dsn_set_pose: the frame code of the
 * density is the frame state's), from three float32 axis arrays x [nx], y [ny], z [nz]:
 *   volume [nx, ny, nz] float32, point n = (i ny + j) nz + k = (x[i], y[j], z[k]) (torch.meshgrid + vstack(...).T order);
 *   transparent points 0, the others sigma of the split-fp16 density-only kernel (bit-identical to dsn_field_forward's sigma where
 *   that does not flag; flagged points are re-evaluated by the exact-fp32 kernel).  DSN_FIELD_FP32: the exact-fp32 kernel for all,
 *   i.e. the bits of dsn_warp + dsn_field(density only) + zeroing.  DSN_NN_EXHAUSTIVE: the nearest-face cross-check.
 * The grid runs in slabs of whole x-planes of at most slab_points points (>= ny nz); the scratch `workspace` of
 * dsn_density_grid_workspace_bytes(slab_points) bytes does not grow with the grid, and the result does not depend on the slab size.
 * Grids of up to 2^31 - 1 points. */
DSN_EXPORT size_t dsn_density_grid_workspace_bytes(int64_t slab_points);
DSN_EXPORT int dsn_density_grid(const void* scene, int V, int F, const void* packed, const float* x, int nx, const float* y, int ny,
                                const float* z, int nz, int flags, float* volume, int64_t slab_points, void* workspace,
                                size_t workspace_bytes, void* stream);
/* utils/visualizer.py:112-142 get_mesh_from_grid (skimage.measure.marching_cubes): marching cubes over volume [nx, ny, nz] at the
 * grid's own coordinates (axes x, y, z as above; every axis >= 2 points, fewer than 2^31 points).  The rule, fixed so that a numpy
 * restatement reproduces it bit for bit:
 *   - inside = v > level (strict; NaN is outside);
 *   - one vertex per sign-changing grid edge (n, d): from point n to its neighbour along axis d (0 = x, 1 = y, 2 = z), edge id 3 n + d;
 *     t = (level - a) / (b - a) with a the value at n; the coordinate along d is ax[i] + t * (ax[i + 1] - ax[i]), the other two are the
 *     grid's (float32, no fused multiply-add);
 *   - vertices in ascending edge id; triangles in ascending cell index (i (ny - 1) + j) (nz - 1) + k, then in table order;
 *     vertex numbers int32 (2^31 or more vertices: the call fails);
 *   - DSN_MC_DESCENT (object = values above the level): each triangle's normal (v1 - v0) x (v2 - v0) points out of the object;
 *     DSN_MC_ASCENT (the reference visualizer's setting): every triangle reversed, (v2, v1, v0).
 * Cube numbering of the case table: corner c = dx + 2 dy + 4 dz (bit set = +1 along that axis); the case's bit c is set when corner c is
 * inside.  Edge e = 4 d + q runs along axis d; q = b1 + 2 b2 with b1, b2 the bits of its corners along the two other axes in increasing
 * order (d = 0: y, z; d = 1: x, z; d = 2: x, y).  Per case: on each cube face the sign-changing edges are paired (an ambiguous face -
 * diagonal corners inside - cuts each inside corner off on its own, so the two cells sharing a face cut the same segments); the
 * segments close into loops; each loop is fanned from its lowest-numbered edge, loops in order of that edge.
 * Two phases (the library never allocates): dsn_mc_count writes [n_verts, n_faces] (int64) to device memory and fills `workspace`
 * (dsn_mc_workspace_bytes, <= 8 bytes per grid point); the caller reads the counts, sizes verts [n_verts, 3] float32 and
 * faces [n_faces, 3] int32, and dsn_mc_emit fills them from the same workspace (no atomics: every call returns the same bits).
 * A level the volume does not cross gives 0 and 0 (the reference returns None). */
#define DSN_MC_DESCENT 0
#define DSN_MC_ASCENT 1
#define DSN_MC_MAX_TRI 5                              /* triangles per case, at most */
#define DSN_MC_TABLE_ROW (1 + 3 * DSN_MC_MAX_TRI)     /* int32 per case in dsn_mc_table_host: count, then edge triples (-1 padded) */
DSN_EXPORT size_t dsn_mc_workspace_bytes(int nx, int ny, int nz);
DSN_EXPORT int dsn_mc_count(const float* volume, int nx, int ny, int nz, float level, void* workspace, int64_t* out_counts2,
                            void* stream);
DSN_EXPORT int dsn_mc_emit(const float* volume, int nx, int ny, int nz, const float* x, const float* y, const float* z, float level,
                           int gradient_direction, const void* workspace, int64_t n_verts, int64_t n_faces, float* verts,
                           int32_t* faces, void* stream);
/* Vertex normals of the same mesh (skimage.measure.marching_cubes' third output; the reference's get_mesh_from_grid carries them to
 * trimesh.Trimesh(vertex_normals=...)): normals [n_verts, 3] float32 in dsn_mc_emit's vertex order, from the workspace dsn_mc_count
 * left (dsn_mc_emit may run before or after: neither writes it).  The rule, float32 throughout, no fused multiply-add, `/` and sqrt
 * correctly rounded, so that numpy reproduces it bit for bit (tests/mc_normals_restate.py):
 *   - gradient of the volume at a grid point along axis d, at index i of nd with coordinates ax: inside
 *     (v[i + 1] - v[i - 1]) / (ax[i + 1] - ax[i - 1]); at i = 0 (v[1] - v[0]) / (ax[1] - ax[0]); at i = nd - 1
 *     (v[nd - 1] - v[nd - 2]) / (ax[nd - 1] - ax[nd - 2]);
 *   - vertex of edge (n, d) between the points a = n and b = its neighbour along d: g = g_a + t (g_b - g_a) per component, with
 *     dsn_mc_emit's t = (level - v_a) / (v_b - v_a);
 *   - nn = sqrt((g0 g0 + g1 g1) + g2 g2); normal = (s g) / nn with s = -1 for DSN_MC_DESCENT (the object is where the values are
 *     higher: the normal points out of it, with that mode's (v1 - v0) x (v2 - v0)) and s = +1 for DSN_MC_ASCENT;
 *   - (0, 0, 0) unless 0 < nn < infinity (a zero gradient, NaN or infinite values among the neighbours).
 * skimage's fourth output (`values`) is not provided. */
DSN_EXPORT int dsn_mc_normals(const float* volume, int nx, int ny, int nz, const float* x, const float* y, const float* z, float level,
                              int gradient_direction, const void* workspace, int64_t n_verts, float* normals, void* stream);
/* the case table (host function, no device work): 256 rows of DSN_MC_TABLE_ROW int32 into a HOST array of out_ints >= 256 rows */
DSN_EXPORT int dsn_mc_table_host(int32_t* out_host, size_t out_ints);

/* ---- density grid, coarse to fine (an addition within ABI 8: no existing entry point changes) ---------------------------------------
 * The reference's visualizer carries a commented-out `from utils.mise import MISE` (multiresolution iso-surface extraction) it never
 * wired up.  Here: a two-level form with a certificate.  The density is evaluated on a coarse sub-lattice of the SAME grid, then only
 * at the fine points in and around the coarse cells the level crosses; every other point is filled so that it can neither create nor
 * move a vertex, and dsn_mc_count / dsn_mc_emit / dsn_mc_normals run unchanged on the assembled dense volume.  The rule, fixed so that
 * a numpy restatement (tests/grid_hier_restate.py) reproduces every output bit for bit - inputs: the fine grid nx, ny, nz (every axis
 * >= 2, fewer than 2^31 points), a level, a factor c in {2, 4, 8, 16} and a dilate r >= 0:
 *   1. Coarse lattice.  Per axis of n points the indices 0, c, 2c, ... < n, plus n - 1 if it is not among them: m = ceil((n - 1) / c) + 1
 *      coarse points, coarse point q = fine index min(q c, n - 1), m - 1 cells of which the last may be shorter.  Coarse points ARE fine
 *      points: coarse [mx, my, mz] holds the dense grid's values at those points, bit for bit (the density of a point depends on
 *      nothing but the point).
 *   2. Core cells.  A coarse cell whose eight corners are not all on the same side of the level, with marching cubes' inside =
 *      v > level (strict; NaN is outside).
 *   3. Active cells.  The core cells dilated r times over the 26-neighbourhood: a box maximum of radius r, clipped at the lattice's
 *      border.
 *   4. Evaluated points.  Every fine point in the closed index box of an active cell; their linear fine indices n = (i ny + j) nz + k
 *      as an ascending int32 list.
 *   5. Fill.  An unevaluated point gets the coarse value at the lowest corner of its owner cell - per axis the last coarse index <= the
 *      point's index, clamped to the last cell: min(i / c, m - 2).  Every cell that contains an unevaluated point is inactive, hence no
 *      core cell, hence has all corners on one side; neighbouring inactive cells share corners: no two filled points differ in side.
 *   6. Assembled volume [nx, ny, nz].  Evaluated points hold the caller's values (dsn_density_points': dsn_density_grid's bits at that
 *      point), all other points the fill.
 *   7. Leaks, the certificate.  Of the grid edges of the assembled volume whose ends differ in side, an edge is a leak when a filled
 *      point is among its two end points or among the in-grid +-1 neighbours of either end point along any of the three axes (the
 *      stencil of dsn_mc_normals).  `leaks` counts those edges, each once.
 * What this proves: where the assembled and the dense volume have the same inside mask everywhere and leaks == 0, dsn_mc_count,
 * dsn_mc_emit and dsn_mc_normals return the dense grid's vertices, faces and normals bit for bit (every value they read was evaluated).
 * What it does not: a piece of surface that lies wholly among unevaluated points - a floater smaller than a coarse cell, more than r
 * cells away from any coarse sign change - cannot be seen and is not counted; leaks == 0 says nothing about it.
 * Stages (the library never allocates; integer counters only, so the same call returns the same bits):
 *   dsn_grid_hier_mark     coarse volume -> core and active masks in `workspace` (dsn_grid_hier_workspace_bytes), out_counts3 (int64,
 *                          device): core cells, active cells, evaluated points;
 *   dsn_grid_hier_list     that workspace -> point_index [n_points] int32 ascending; the caller sizes it from out_counts3[2];
 *   dsn_density_points     values [m] = the dense grid's value at point_index [m] (below);
 *   dsn_grid_hier_assemble fill everywhere, then the scatter of the listed values -> volume; out_leaks (int64, device).  point_index
 *                          must be dsn_grid_hier_list's list of the same workspace (indices outside the grid are skipped). */
DSN_EXPORT size_t dsn_grid_hier_workspace_bytes(int nx, int ny, int nz, int factor);
DSN_EXPORT int dsn_grid_hier_mark(const float* coarse, int mx, int my, int mz, int nx, int ny, int nz, int factor, int dilate, float level,
                                  void* workspace, size_t workspace_bytes, int64_t* out_counts3, void* stream);
DSN_EXPORT int dsn_grid_hier_list(int nx, int ny, int nz, int factor, const void* workspace, size_t workspace_bytes, int64_t n_points,
                                  int32_t* point_index, void* stream);
DSN_EXPORT int dsn_grid_hier_assemble(const float* coarse, int mx, int my, int mz, int nx, int ny, int nz, int factor, float level,
                                      const void* workspace, size_t workspace_bytes, const int32_t* point_index, const float* values,
                                      int64_t n_points, float* volume, int64_t* out_leaks, void* stream);
/* The density of listed grid points: values [m] = dsn_density_grid's value at grid point point_index [m] = (i ny + j) nz + k of the
 * axes x, y, z, bit for bit (transparent points 0, flagged points re-evaluated by the exact-fp32 kernel; DSN_FIELD_FP32 and
 * DSN_NN_EXHAUSTIVE as there).  The list may be in any order and hold duplicates; an index outside the grid gives NaN.  The list runs
 * in slabs of at most slab_points (>= 1) points; the scratch `workspace` of dsn_density_points_workspace_bytes(slab_points) bytes does
 * not grow with the list, and the result does not depend on the slab size. */
DSN_EXPORT size_t dsn_density_points_workspace_bytes(int64_t slab_points);
DSN_EXPORT int dsn_density_points(const void* scene, int V, int F, const void* packed, const float* x, int nx, const float* y, int ny,
                                  const float* z, int nz, const int32_t* point_index, int64_t n_points, int flags, float* values,
                                  int64_t slab_points, void* workspace, size_t workspace_bytes, void* stream);

/* ---- mesh components (an addition within ABI 8: no existing entry point changes) ----------------------------------------------------
 * utils/visualizer.py:129-138, Visualizer3D(connected=True): the reference splits the mesh with trimesh and keeps the component with the
 * largest area.  Here: the connected components of an indexed mesh (verts [V, 3] float32, faces [T, 3] int32, device) and its largest
 * piece as a compacted mesh, by a rule fixed so that a numpy restatement (tests/mesh_cc_restate.py) reproduces every output bit for bit.
 *   Valid faces:  a face is valid when its three indices lie in [0, V).  Invalid faces belong to no component and are never emitted.  A
 *                 face with a repeated index is valid: it has area 0 and still connects.
 *   Connectivity: two valid faces are connected when they share a vertex INDEX (coincident positions under different indices do not
 *                 connect); a component is a class of the transitive closure.  trimesh's split joins faces that share an EDGE: on the
 *                 output of dsn_mc_emit the two rules give the same partition (every vertex's triangles form one edge-connected fan;
 *                 tests/test_mesh_cc_host.py), on arbitrary meshes they differ at pinch vertices - two pieces touching in one vertex
 *                 are ONE component here.
 *   Label:        a component's label is the smallest vertex index it contains, whatever the face order or the scheduling; a vertex used
 *                 by no valid face has label -1.
 *   Area:         per valid face (a, b, c), float32, no fused multiply-add: e1 = b - a, e2 = c - a; n = e1 x e2, each component two
 *                 rounded products and one subtraction (n0 = e1_1 e2_2 - e1_2 e2_1, ...); s = (n0 n0 + n1 n1) + n2 n2; d = sqrt(s), the
 *                 doubled area; a d that is not finite counts as 0.  The face adds q = floor(d 2^area_shift), formed exactly in double,
 *                 to its component's unsigned 64-bit sum: integer sums do not depend on the order the faces arrive in.  The caller
 *                 chooses the shift: area_shift = 61 - bit_length(T) - e, clamped to +-60, with e the frexp exponent of float32
 *                 D2 = (dx dx + dy dy) + dz dz over the extents of the bounding box of the vertices whose coordinates are all finite
 *                 (128 where D2 is not finite, 0 without such a vertex); no triangle with finite vertices has a doubled area above D2,
 *                 so the sums stay below 2^61.  (A q of 2^63 or more - no shift of this rule gives one - counts as 2^63.)  The area
 *                 of a component is sum 2^(-area_shift - 1).
 *   Winner:       the component with the largest sum; on equal sums the smaller label (the reference keeps the first component whose
 *                 area is strictly greater, in trimesh's unpinned component order).
 *   Filtered mesh: the winner's vertices in their original order; the winner's valid faces in their original order and winding, their
 *                 indices renumbered through the vertex map; source_vertex [V'] int32 = each kept vertex's old index (per-vertex arrays
 *                 follow by one gather).  A mesh that is one component without unused vertices comes back bit for bit.
 * Two phases, as dsn_mc_count / dsn_mc_emit (the library never allocates): dsn_mesh_cc_label fills `workspace`
 * (dsn_mesh_cc_workspace_bytes(V, T), 16-byte aligned; its earlier contents are not read), writes labels_v [V] int32 (may be NULL) and
 * out_counts: 6 int64 in device memory {components, winner label (-1: none), V', T', the winner's sum, the winner's face count}.  The caller
 * reads them, sizes out_verts [V', 3], out_faces [T', 3] and source_vertex [V'] (may be NULL), and dsn_mesh_cc_emit fills them from the
 * same workspace (rows beyond n_verts / n_faces are not written).  V = 0 or T = 0 is a valid call: all counts 0, the winner -1.
 * Kernels: a lock-free union-find over the vertex array, one thread per face (a root is only ever hooked under a smaller root by a
 * compare-and-swap, so parent[x] <= x always holds, every walk goes strictly downward and ends whatever value it reads, and no thread waits
 * for another; every access of that kernel is a relaxed agent-scope atomic), a launch that flattens every vertex to its root, 64-bit
 * integer atomic adds of the faces' areas aggregated per wave, a deterministic arg-max over the roots, and two scans over tiles of
 * DSN_MESH_CC_TILE vertices / faces that decide the output order (no atomics there).  Every call returns the same bits.  No allocation,
 * no synchronisation, all on `stream`.
 * Rejected: null verts with V > 0, null faces with T > 0, a null workspace or out_counts, negative sizes or 2^31 and more, a workspace
 * that is not 16-byte aligned or smaller than dsn_mesh_cc_workspace_bytes (0 for bad sizes), a shift outside +-60; by dsn_mesh_cc_emit
 * also null outputs with non-zero counts and counts above V / T. */
#define DSN_MESH_CC_TILE 1024
DSN_EXPORT size_t dsn_mesh_cc_workspace_bytes(int64_t n_verts, int64_t n_faces);
DSN_EXPORT int dsn_mesh_cc_label(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, int area_shift, void* workspace,
                                 size_t workspace_bytes, int32_t* labels_v, int64_t* out_counts6, void* stream);
DSN_EXPORT int dsn_mesh_cc_emit(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, void* workspace,
                                size_t workspace_bytes, int64_t out_n_verts, int64_t out_n_faces, float* out_verts, int32_t* out_faces,
                                int32_t* source_vertex, void* stream);
/* measurement (scripts/bench_mesh_cc.py): enqueue only these kernels (0 = all; one mesh and one workspace through the phases in order) */
#define DSN_CC_INIT 1
#define DSN_CC_UNITE 2
#define DSN_CC_FLATTEN 4
#define DSN_CC_SUMS 8
#define DSN_CC_SELECT 16
#define DSN_CC_COUNT 32
#define DSN_CC_EMIT_VERTS 64
#define DSN_CC_EMIT_FACES 128
DSN_EXPORT int dsn_mesh_cc_label_ex(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, int area_shift,
                                    void* workspace, size_t workspace_bytes, int32_t* labels_v, int64_t* out_counts6, int phases,
                                    void* stream);
DSN_EXPORT int dsn_mesh_cc_emit_ex(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, void* workspace,
                                   size_t workspace_bytes, int64_t out_n_verts, int64_t out_n_faces, float* out_verts, int32_t* out_faces,
                                   int32_t* source_vertex, int phases, void* stream);

/* ---- mesh simplification (an addition within ABI 8: no existing entry point changes) --------------------------------------------------
 * Vertex clustering with a picked representative: the output vertices are a SUBSET of the input vertices, so every per-vertex array
 * (normals, colours, the binding record of dsn_mesh_pose) follows by one gather through cluster_source, as through dsn_mesh_cc_emit's
 * source_vertex.  There is no counterpart in the reference (its users would decimate with trimesh or open3d on the host); the rule is
 * fixed so that a numpy restatement (tests/mesh_simplify_restate.py) reproduces every output bit for bit.  Integer sums and integer
 * atomics only: every call returns the same bits.
 *   Inputs:   verts [V, 3] float32, faces [T, 3] int32 (device); the grid: origin_host [3] float32 and g3_host [3] int in HOST memory
 *             (read before the call returns), cell float32 > 0; every g_a in [1, DSN_MESH_SIMPLIFY_MAX_G], g0 g1 g2 <= 2^31.
 *   Cell:     inv = 1.0f / cell (float32, once, on the host); t_a = (x_a - origin_a) inv, one float32 subtraction and one float32 product.
 *             A vertex is INSIDE when all three t_a are finite, >= 0 and < g_a (NaN and infinite coordinates are outside); its cell
 *             number is (i0 g1 + i1) g2 + i2 with i_a = floor(t_a).
 *   Clusters: the occupied cells numbered in ascending cell number; that number is the cluster index = the output vertex index, K their
 *             count.  vertex_cluster [V] int32: the cluster of every inside vertex, -1 for the others.  Inside vertices no face uses
 *             still occupy their cell.
 *   Representative: q_a = floor(double(t_a) 2^20) as a 64-bit integer (exact, below 2^32); per cluster s_a = the sum of q_a (below 2^63)
 *             and the member count n; m_a = double(s_a) / double(n), e_a = double(q_a) - m_a, d = (e0 e0 + e1 e1) + e2 e2 in IEEE double,
 *             one rounding per operation, nothing fused.  The representative minimises the 64-bit key
 *             (bits of float32(d)) << 32 | vertex index: nearest to the members' mean, ties to the smaller index.  cluster_source [K]
 *             int32 is its index; the output vertex is its three float32 words, copied.
 *   Faces:    a face is LIVE when its three indices lie in [0, V), all three vertices are inside and the three clusters differ.  Two live
 *             faces are DUPLICATES when their cluster triples agree as sets (any rotation or winding); of a set of duplicates only the
 *             face with the smallest input index is kept.  Kept faces come out in input order and input winding, indices replaced by
 *             clusters.  (Clustering can pinch a surface: no manifold repair is attempted.)
 *   Cap:      duplicate detection packs a sorted triple into 63 bits: K <= 2^DSN_MESH_SIMPLIFY_MAX_LOG2.  A larger K sets
 *             DSN_MESH_SIMPLIFY_TOO_MANY in the status: K, the vertices outside and vertex_cluster are still what the rule says, no face
 *             is looked at (the other counts are 0) and dsn_mesh_simplify_emit writes nothing - choose a larger cell.
 *   Counts:   out_counts7: 7 int64 in device memory {K, kept faces T', live faces, duplicates dropped, vertices outside, faces with an
 *             index outside [0, V), status}.
 * Two phases, as dsn_mesh_cc_label / dsn_mesh_cc_emit: dsn_mesh_simplify_count fills `workspace` (dsn_mesh_simplify_workspace_bytes(V, T,
 * g3), 16-byte aligned; its earlier contents are never read), writes vertex_cluster (may be NULL) and the counts; the caller reads them,
 * sizes out_verts [K, 3], out_faces [T', 3] and cluster_source [K] (may be NULL), and dsn_mesh_simplify_emit fills them from the same
 * workspace.  The library cannot read the counts without synchronising: emit rejects counts no call could have reported (above V, the
 * number of cells, the cap or T), never writes a row beyond K or T', and writes nothing at all while the status is not 0.
 * dsn_mesh_simplify_cells marks and counts the occupied cells only (out_K: one int64 in device memory; workspace:
 * dsn_mesh_simplify_workspace_bytes(V, 0, g3)): what a search for a cell size that gives a wanted K probes with.
 * Kernels: one thread per vertex sets its cell's bit in a bit grid (an atomic OR per run of equal cells in the wave), a popcount prefix
 * over the grid's words (the tile scan of the marching cubes, no atomics) ranks the cells, 64-bit integer atomic adds aggregated per
 * run of equal clusters in the wave form the sums, one 64-bit unsigned atomic minimum per run picks the representative; a live face claims
 * the slot of its sorted triple in a lock-free open-addressing table (capacity a power of two >= 2 T) by a 64-bit compare-and-swap and
 * leaves the minimum of its index there - the probe is bounded by the capacity (exhaustion, which that load rules out, sets
 * DSN_MESH_SIMPLIFY_TABLE_FULL), no thread waits for another - and a tile scan over the keep flags orders the output.  All atomics are
 * relaxed and agent scope, all 3 V and 3 T indexing is 64-bit.  V = 0 or T = 0 is a valid call.  No allocation, no synchronisation, all
 * on `stream`.
 * Rejected: null verts with V > 0, null faces with T > 0, a null origin, g3, workspace or counts, negative sizes or 2^31 and more, a g
 * outside its limits, a cell that is not finite or <= 0 (or whose float32 inverse is not finite), an origin that is not finite, a workspace
 * that is not 16-byte aligned or smaller than dsn_mesh_simplify_workspace_bytes (0 for bad sizes); by dsn_mesh_simplify_emit also null
 * outputs with non-zero counts. */
#define DSN_MESH_SIMPLIFY_MAX_G 4096
#define DSN_MESH_SIMPLIFY_MAX_LOG2 21
#define DSN_MESH_SIMPLIFY_TOO_MANY 1
#define DSN_MESH_SIMPLIFY_TABLE_FULL 2
DSN_EXPORT size_t dsn_mesh_simplify_workspace_bytes(int64_t n_verts, int64_t n_faces, const int* g3_host);
DSN_EXPORT int dsn_mesh_simplify_count(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const float* origin_host,
                                       float cell, const int* g3_host, void* workspace, size_t workspace_bytes, int32_t* vertex_cluster,
                                       int64_t* out_counts7, void* stream);
DSN_EXPORT int dsn_mesh_simplify_emit(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const int* g3_host,
                                      void* workspace, size_t workspace_bytes, int64_t out_n_verts, int64_t out_n_faces, float* out_verts,
                                      int32_t* out_faces, int32_t* cluster_source, void* stream);
DSN_EXPORT int dsn_mesh_simplify_cells(const float* verts, int64_t n_verts, const float* origin_host, float cell, const int* g3_host,
                                       void* workspace, size_t workspace_bytes, int64_t* out_K, void* stream);
/* measurement (scripts/bench_mesh_simplify.py): enqueue only these kernels (0 = all; one mesh and one workspace through the phases in order) */
#define DSN_SP_ZERO 1
#define DSN_SP_MARK 2
#define DSN_SP_RANK 4
#define DSN_SP_SUM 8
#define DSN_SP_PICK 16
#define DSN_SP_FACES 32
#define DSN_SP_KEEP 64
#define DSN_SP_EMIT_VERTS 128
#define DSN_SP_EMIT_FACES 256
DSN_EXPORT int dsn_mesh_simplify_count_ex(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const float* origin_host,
                                          float cell, const int* g3_host, void* workspace, size_t workspace_bytes, int32_t* vertex_cluster,
                                          int64_t* out_counts7, int phases, void* stream);
DSN_EXPORT int dsn_mesh_simplify_emit_ex(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const int* g3_host,
                                         void* workspace, size_t workspace_bytes, int64_t out_n_verts, int64_t out_n_faces, float* out_verts,
                                         int32_t* out_faces, int32_t* cluster_source, int phases, void* stream);

/* ---- mesh smoothing and normals from the faces (an addition within ABI 8: no existing entry point changes) ---------------------------
 * An iso-surface of a thresholded density grid is stair-stepped; the reference's users would call trimesh.smoothing.filter_taubin or
 * filter_laplacian on the host.  Here: umbrella steps on the device, and area-weighted vertex normals from the faces for meshes whose
 * marching-cubes normals are stale (smoothed, posed, loaded from a file).  There is no counterpart in the reference; both rules are fixed
 * so that a numpy restatement (tests/mesh_smooth_restate.py) reproduces every output bit for bit.  Integer sums only: every call returns
 * the same bits, whatever the order of the faces.
 * dsn_mesh_smooth:
 *   Inputs:   verts [V, 3] float32, faces [T, 3] int32 (device); origin_host [3] float32, scale_exp = k and factors_host [n_steps] float32
 *             in HOST memory (read before the call returns), 0 <= n_steps <= DSN_MESH_SMOOTH_MAX_STEPS, |k| <= DSN_MESH_SMOOTH_MAX_EXP.
 *             Output out_verts [V, 3] float32, which must not overlap verts.  Faces, vertex count and vertex order never change.
 *   Contributing face: its three indices lie in [0, V), are pairwise different, and all nine coordinates of its vertices IN THE INPUT are
 *             finite.  The set is fixed for the whole call; every other face is skipped.  n_i = 2 x the number of contributing faces at
 *             vertex i; a vertex with n_i = 0 (unused, not finite) is copied bit for bit.
 *   Weights:  every contributing face gives each of its corners the other two as neighbours: w_ij = the number of contributing faces that
 *             hold both i and j.  On a closed manifold every edge counts twice - the uniform umbrella operator of
 *             trimesh.smoothing.filter_laplacian - ; a BOUNDARY edge has weight 1, so a boundary vertex leans towards the interior.
 *   Scale:    the caller's: origin = the minimum of the vertices whose coordinates are all finite (zeros without one), D = the largest
 *             extent max_a double(hi_a) - double(lo_a), e = the frexp exponent of D (0 when D = 0), k = 27 - e: the box maps to [0, 2^27).
 *   Quantised coordinate, per step from that step's float32 positions: r = double(x_a) - double(origin_a); q = floor(r 2^k), formed in
 *             double and clamped to [-2^30, 2^30 - 1]; q = 0 where r is not finite.  (The clamp is eight extents away: only factors that
 *             make the iteration diverge reach it.)
 *   Step with factor f, every vertex with n_i > 0 and every axis: S = the signed 64-bit sum over the contributing faces (i, j, l) at i of
 *             (q_j - q_i) + (q_l - q_i)  (|S| <= 2 T (2^31 - 1) < 2^63);  delta = double(S) / double(n_i);  t = double(f) delta;
 *             u = t 2^-k (exact);  x' = float32(double(x) + u).  One IEEE rounding per operation, nothing fused.  All vertices of a step
 *             read the positions of the step before it.  The sum does not depend on the order of the faces or on their rotation, and a
 *             coordinate a vertex shares with all its neighbours keeps its bits.
 *   Modes:    Taubin smoothing is the factor sequence lambda, mu, lambda, mu, ... (mu < -lambda < 0), plain Laplacian lambda, lambda, ...
 *   Counts:   out_counts4 (may be NULL): 4 int64 in device memory {contributing faces, skipped faces, vertices with n_i > 0, the largest
 *             number of contributing faces at one vertex}.
 * dsn_mesh_vertex_normals: out_normals [V, 3] float32.
 *   A face counts when its indices lie in [0, V) and its nine coordinates are finite.  Its normal is dsn_mesh_cc_label's float32 cross
 *   product (e1 = b - a, e2 = c - a, each component two rounded products and one subtraction: a face with a repeated index gives exactly
 *   0); a component that is not finite counts as 0.  Every component adds floor(double(n_c) 2^shift), clamped to +-2^62, to a signed
 *   64-bit sum at each of the face's three vertices; `shift` is dsn_mesh_cc_label's area_shift, unchanged (it keeps T such terms below
 *   2^61).  With N = the three sums as doubles: L = sqrt((N0 N0 + N1 N1) + N2 N2), out_c = float32(N_c / L); L = 0, or a vertex in no
 *   such face: (0, 0, 0), which dsn_raster_mesh_attr already treats.  Area-weighted, oriented by the winding.
 * Kernels: once per call a vertex -> corner list (CSR): int32 atomic counts per vertex, one per run of equal vertices in the wave; the tile
 * scan of the simplification over tiles of DSN_MESH_CC_TILE vertices for the 64-bit offsets (3 T can pass 2^31); a fill through atomic
 * cursors (the order inside a row is arbitrary: rows are summed in integers).  An entry is 8 bytes: the face's two other corners in
 * winding order, the corner's number in the two sign bits.  Each step is one launch with one thread per vertex that gathers its row
 * from the positions of the step before and writes x' - no atomics; positions ping-pong between two buffers of the workspace.  A row
 * longer than DSN_MESH_SMOOTH_HEAVY entries is summed by its whole wave with a wave reduction.  The normals gather through the same
 * lists.  All atomics are relaxed and agent scope, all 3 V and 3 T indexing is 64-bit, everything read back from the workspace is
 * range-checked before it is used as an index.  V = 0, T = 0 and n_steps = 0 (a bit-for-bit copy) are valid calls.  No allocation, no
 * synchronisation, all on `stream`.  `workspace`: dsn_mesh_smooth_workspace_bytes(V, T) (0 for bad sizes) for both calls, 16-byte
 * aligned; its earlier contents are never read.
 * Rejected: null verts or out_verts / out_normals with V > 0, null faces with T > 0, a null workspace, a null origin, null factors with
 * n_steps > 0, negative sizes or 2^31 and more, n_steps or k outside their limits, factors or an origin that are not finite, a workspace
 * that is misaligned or too small, an output that overlaps verts, a shift outside +-60. */
#define DSN_MESH_SMOOTH_HEAVY 64
#define DSN_MESH_SMOOTH_MAX_STEPS 4096
#define DSN_MESH_SMOOTH_MAX_EXP 900
DSN_EXPORT size_t dsn_mesh_smooth_workspace_bytes(int64_t n_verts, int64_t n_faces);
DSN_EXPORT int dsn_mesh_smooth(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const float* origin_host,
                               int scale_exp, const float* factors_host, int n_steps, void* workspace, size_t workspace_bytes,
                               float* out_verts, int64_t* out_counts4, void* stream);
DSN_EXPORT int dsn_mesh_vertex_normals(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, int shift, void* workspace,
                                       size_t workspace_bytes, float* out_normals, void* stream);
/* measurement (scripts/bench_mesh_smooth.py): enqueue only these kernels (0 = all; one mesh and one workspace through the phases in order) */
#define DSN_SM_COUNT 1
#define DSN_SM_SCAN 2
#define DSN_SM_FILL 4
#define DSN_SM_STEP 8
#define DSN_SM_NORMALS 16
DSN_EXPORT int dsn_mesh_smooth_ex(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const float* origin_host,
                                  int scale_exp, const float* factors_host, int n_steps, void* workspace, size_t workspace_bytes,
                                  float* out_verts, int64_t* out_counts4, int phases, void* stream);
DSN_EXPORT int dsn_mesh_vertex_normals_ex(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, int shift,
                                          void* workspace, size_t workspace_bytes, float* out_normals, int phases, void* stream);

/* ---- the distance between two meshes (an addition within ABI 8: no existing entry point changes) ------------------------------------
 * How far did simplification, smoothing, a coarse extraction or a pose move the surface?  A user of the reference would take both meshes
 * to the host and call trimesh.proximity.closest_point or open3d's compute_point_cloud_distance.  Here: the exact nearest point on a
 * triangle mesh for a set of query points, a reduction of the distances to mean / rms / maximum, and area-weighted surface samples to
 * query from.  There is no counterpart in the reference; every rule is fixed so that a numpy restatement (tests/mesh_dist_restate.py)
 * reproduces every output bit for bit.  No float atomics: every call returns the same bits.
 * THE RULE (dsn_mesh_dist_query).  All float32, one IEEE rounding per operation, nothing fused; dot(x, y) = (x0 y0 + x1 y1) + x2 y2.
 *   Valid face: its three indices lie in [0, V) and its nine coordinates are finite.  Zero-area faces are valid.  Other faces take no part.
 *   Point and triangle (a, b, c), the seven-region closest point, in this order, the first region that applies:
 *     ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c (per component);
 *     d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);
 *     vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4 (two rounded products and one subtraction each);
 *     1. d1 <= 0 and d2 <= 0:                  q = a
 *     2. d3 >= 0 and d4 <= d3:                 q = b
 *     3. vc <= 0, d1 >= 0, d3 <= 0, D3 > 0:    v = d1 / D3,  q = a + v ab                    with D3 = d1 - d3
 *     4. d6 >= 0 and d5 <= d6:                 q = c
 *     5. vb <= 0, d2 >= 0, d6 <= 0, D5 > 0:    w = d2 / D5,  q = a + w ac                    with D5 = d2 - d6
 *     6. va <= 0, d4 - d3 >= 0, d5 - d6 >= 0, D6 > 0:  w = (d4 - d3) / D6,  q = b + w (c - b)  with D6 = (d4 - d3) + (d5 - d6)
 *     7. otherwise (the interior):             i = 1 / ((va + vb) + vc), v = vb i, w = vc i,  q = (a + ab v) + ac w
 *     The denominators D are the squared lengths of the edges in exact arithmetic: an edge of length zero has no region of its own
 *     (with a = b every point would otherwise land in region 3), its end points and the other two edges answer.  r = p - q, the
 *     squared distance is dot(r, r).  A triangle collapsed to a segment or a point falls into regions 1 - 6 in exact arithmetic.
 *   Result for p: the valid face with the smallest squared distance, ties to the LOWEST face index (a face wins with d < best, or
 *     d == best and a lower index; a NaN distance, which only overflow can produce, never wins): out_dist2 (float32), out_face (int32),
 *     out_point (that face's q, 3 float32).  Each output may be NULL.  No valid face: +inf, -1, NaN.  A query point with a coordinate
 *     that is not finite: NaN, -1, NaN.  The rule does not mention a grid: the answer is the brute-force answer.
 * THE GRID (dsn_mesh_dist_build) only decides which faces a query looks at.
 *   box_host [6] float32 in HOST memory: lo[3], hi[3], finite, lo <= hi, containing the vertices of the valid faces (the wrapper passes
 *     the bounding box of the finite vertices).  origin = lo.
 *   Level-0 grid (dsn_mesh_dist_grid_host, in double): ext_a = hi_a - lo_a, L = the largest; M = min(2 T + 64, 2^26) cells at most;
 *     n = the largest integer in [1, DSN_MESH_DIST_MAX_G] with prod_a min(n, floor(ext_a n / L) + 1) <= M;
 *     cell = float32((L / n) (1 + 2^-20)), inv = 1.0f / cell, g_a = min(n, floor(ext_a / cell) + 1).  L = 0, or a cell whose inverse is
 *     not finite: one cell.  So a surface of T triangles gets about 2 T cells, of which it occupies a few T^(2/3); the
 *     entry cap below keeps the lists short.
 *   Cell of a coordinate: floor(fl(fl(x - origin_a) inv)) clamped to [0, g_a - 1] - monotone in x.  A face is listed in every cell of the
 *     box its three vertices' cells span.
 *   Levels: level l merges 2^l level-0 cells per axis (index >> l).  The build counts the (face, cell) pairs of every level in 64-bit
 *     integers on the device and takes the finest level with at most E = min(8 T + 64, 2^31 - 1) pairs (the last level is one cell and
 *     always fits), so the workspace, dsn_mesh_dist_workspace_bytes(V, T), is a function of T alone, and one face that spans the box among
 *     many small ones cannot exhaust it.  Lists by count (integer atomics), exclusive scan (no atomics), fill (atomic cursors); the order
 *     inside a cell is arbitrary, the query resolves ties by index explicitly.
 *   out_counts4 (may be NULL): 4 int64 in device memory {valid faces, listed pairs, level, cells}.  T = 0 or V = 0 is rejected; a target
 *     without a valid face cannot be seen without synchronising: it reports 0 valid faces here (the wrapper raises) and every query
 *     against it returns +inf, -1.
 *   Query: the cell of the point clamped to the box, then the shells of growing Chebyshev radius r around it.  After shell r every face
 *     not yet seen lies beyond one of the six planes that bound the cube of radius r; lb = the smallest computed distance from p to those
 *     planes, over the sides where the grid goes on.  The search stops when no side goes on, or when
 *     lb' = fl(fl(lb - slack) (1 - 2^-16)) > 0 and fl(lb' lb') > best, with slack = S 2^-17 for S = the largest absolute coordinate
 *     of the box: 128 float32 epsilons of the coordinates, four times what the roundings of the cell function, the planes and the closest
 *     point can add up to (csrc/dsn_meshdist.hip: md_shell_stops), so a shell is skipped only where every face in it is provably farther
 *     in the COMPUTED distance.  A face listed in several cells may be evaluated more than once; that cannot change the result.
 *     A query far outside the box walks every shell: the cost of such a point is the number of cells.
 * dsn_mesh_dist_reduce: out_stats6 = 6 float64 in device memory {count, NaN count, sum d, sum d^2, max d, index of the max} from n squared
 *   distances x_i (float32): NaN entries are counted and left out; d_i = sqrt(double(x_i)), d_i^2 = double(x_i); the maximum is taken over
 *   x_i, the lowest index on ties (max d = 0, index -1 without an entry).  Order of the float64 sums: block k owns the
 *   DSN_MESH_DIST_REDUCE_TILE = 1024 values from 1024 k; its thread t adds the values 1024 k + t + 256 j for j = 0, 1, 2, 3 in that order
 *   (from 0.0), then the 256 thread sums are folded by s[t] += s[t + h] for h = 128, 64, ..., 1; a finishing block's thread t adds the
 *   block sums t, t + 256, ... in that order and folds the same way.  workspace: dsn_mesh_dist_reduce_workspace_bytes(n).
 * dsn_mesh_sample_surface: n points on the mesh, area-weighted; out_points [n, 3] float32, out_face [n] int32 (each may be NULL).
 *   Area of a valid face in float64: e = double(b) - double(a), f = double(c) - double(a), N = (e1 f2 - e2 f1, e2 f0 - e0 f2, e0 f1 - e1 f0),
 *     area = 0.5 sqrt((N0 N0 + N1 N1) + N2 N2); an invalid face has area 0.
 *   Prefix: faces in tiles of DSN_MESH_SAMPLE_TILE = 32, tiles in groups of 32.  in_tile[t] = the running sum of the areas from the tile's
 *     first face to t, in order from 0.0; in_group[k] = the running sum of the tiles' totals from the group's first tile to k; top[g] = the
 *     running sum of the groups' totals; cum[t] = top[g - 1] + (in_group[k - 1] + in_tile[t]) with 0.0 for a missing predecessor (k - 1 in
 *     the same group).  total = cum[T - 1].
 *   Sample i: (x0, x1, x2, x3) = Philox4x32-10 (the generator of dsn_train_draws) at counter (i, 0, 0, 2), key (seed low word, seed high
 *     word).  u0 = double(x0 2^20 + (x1 >> 12)) 2^-52; the face is the first t with cum[t] > fl(u0 total): a face of positive area.
 *     u = float32(x2 >> 8) 2^-24, v = float32(x3 >> 8) 2^-24; if fl(u + v) > 1: u = 1 - u, v = 1 - v.
 *     point = (a + u (b - a)) + v (c - a) per component in float32.  Sample i depends on (seed, i) and the mesh only, not on n.
 *     A mesh without area (total not > 0 or not finite): every point NaN, every face -1.
 *   workspace: dsn_mesh_sample_workspace_bytes(T).  T = 0 or V = 0 is rejected.
 * All kernels: no allocation, no synchronisation, all on `stream`; workspaces 16-byte aligned, their earlier contents are never read (a
 * query reads what the build wrote: a workspace no build has filled gives NaN, -1).  All 3 V, 3 T and 3 n indexing is 64-bit.
 * Rejected: null verts, faces, box or workspace, negative sizes or 2^31 and more, T = 0 or V = 0, a box that is not finite or has
 * lo > hi, a workspace that is misaligned or too small, null points with n > 0, null distances with n > 0, a null out_stats6. */
#define DSN_MESH_DIST_MAX_G 4096
#define DSN_MESH_DIST_REDUCE_TILE 1024
#define DSN_MESH_SAMPLE_TILE 32
DSN_EXPORT size_t dsn_mesh_dist_workspace_bytes(int64_t n_verts, int64_t n_faces);
DSN_EXPORT int dsn_mesh_dist_grid_host(int64_t n_faces, const float* box_host, int* out_g3_host, float* out_cell_host);
DSN_EXPORT int dsn_mesh_dist_build(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const float* box_host,
                                   void* workspace, size_t workspace_bytes, int64_t* out_counts4, void* stream);
DSN_EXPORT int dsn_mesh_dist_query(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, const void* workspace,
                                   size_t workspace_bytes, const float* points, int64_t n_points, float* out_dist2, int32_t* out_face,
                                   float* out_point, void* stream);
DSN_EXPORT size_t dsn_mesh_dist_reduce_workspace_bytes(int64_t n);
DSN_EXPORT int dsn_mesh_dist_reduce(const float* dist2, int64_t n, void* workspace, size_t workspace_bytes, double* out_stats6, void* stream);
DSN_EXPORT size_t dsn_mesh_sample_workspace_bytes(int64_t n_faces);
DSN_EXPORT int dsn_mesh_sample_surface(const float* verts, const int32_t* faces, int64_t n_verts, int64_t n_faces, uint64_t seed,
                                       int64_t n_samples, void* workspace, size_t workspace_bytes, float* out_points, int32_t* out_face,
                                       void* stream);

/* ---- a mesh bound to the body (an addition within ABI 8: no existing entry point changes) --------------------------------------------
 * novel_pose_vis.py and the novel-pose datasets animate one learned body by swapping batch["xyz"].  A mesh extracted in one pose follows
 * the body the same way: dsn_warp expresses a world point in the frame of its nearest posed face as (face, u, v, h) and evaluates that
 * record on the canonical mesh; evaluating it on the mesh of any other pose carries the point there.  The record is never clamped, so
 * the map is a bijection per face.  The rule is fixed so that a numpy restatement (tests/mesh_pose_restate.py) reproduces every output bit
 * for bit.  All float32, fused multiply-add only inside dsn_cross3 and dsn_norm3 (csrc/dsn_common.h), one rounding per operation otherwise.
 *   Binding:  vertex i of a mesh bound against posed body A (body_xyz [Vb, 3], body_faces [Fb, 3]) keeps exactly what dsn_warp returns for
 *             the point with A as the frame's mesh: face_idx[i], uv[i], h[i], transparent[i].  Nothing is clamped or replaced for
 *             transparent vertices: they are carried by the same formula, the mask is only reported.
 *   Position: under a target body B of the same topology, with r = dsn_make_face(B[f0], B[f1], B[f2]) of the bound face f, the position is
 *             dsn_map2face(u, v, h, r): per component ((m0 + u v20) + v v10) + h n, the operation order the warp uses for x_c.  With the
 *             canonical vertices as B this is dsn_warp's x_c, bit for bit.
 *   Normal:   transported as a covector of the face frame.  Bound (dsn_mesh_bind_normals) with the source face's v20, v10 and unit n_f:
 *             cov = (n . v20, n . v10, n . n_f), each (a0 b0 + a1 b1) + a2 b2.  Posed with the target face's w20, w10, c = w10 x w20
 *             (dsn_cross3, not normalised) and the record's unit n_t = c / |c|:
 *               m_k = (cov_0 (n_t x w10)_k + cov_1 (w20 x n_t)_k) + cov_2 c_k,   n' = dsn_normalize3(m) (eps 1e-12)
 *             the cross products by dsn_cross3.  Target = source returns normalize(n); a rigid motion of the body rotates n.  (The
 *             Gram-inverse form of the same covector loses three digits on sliver triangles; this form does not.)  A zero or NaN result is
 *             what dsn_normalize3 and NaN propagation give: nothing is patched.
 *   Stretch:  per mesh face t = (i0, i1, i2) and pose p the maximum over the edges (i0, i1), (i1, i2), (i2, i0) of
 *             dsn_div(dsn_norm3(e_posed), dsn_norm3(e_bind)), e = second vertex - first, e_bind from the vertices the mesh was bound with.
 *             An edge with |e_bind| == 0 is skipped; all three skipped: 1.  A NaN ratio stays (the value is NaN: every threshold test
 *             `stretch <= max` drops the face).  A face with an index outside [0, N): +inf.
 *   Bad bindings: a vertex whose face_idx lies outside [0, Fb) gets a NaN position and a NaN normal in every pose and sets
 *             DSN_MESH_POSE_BAD_BINDING in *status (an int32 in device memory the CALLER zeroes; an integer atomic OR, no host read is
 *             forced); dsn_mesh_bind_normals writes a NaN covector there.  A body face with a vertex index outside [0, Vb) gives a NaN
 *             record: NaN for the vertices bound to it.
 * dsn_mesh_pose: target_xyz [P, Vb, 3] (P bodies), the binding face_idx [N] int32, uv [N, 2], h [N], cov [N, 3] (NULL: no normals);
 * out_verts [P, N, 3], out_normals [P, N, 3] (NULL: none; needs cov), status (NULL: not reported); workspace:
 * dsn_mesh_pose_workspace_bytes(P, Fb) bytes (0 for bad sizes), 16-byte aligned, earlier contents not read - the call fills it with the
 * P x Fb face records (64 B each), one launch, and poses all vertices in a second: one thread per vertex, its 28-byte binding read once,
 * one record gather and 12 or 24 bytes of stores per pose.  P poses in one call give the bits of P calls.  No atomics on floats, every
 * output word has one writer: every call returns the same bits.  N = 0 is a valid call.  All P N 3 indexing is 64-bit.
 * dsn_mesh_stretch: bind_verts [N, 3], posed_verts [P, N, 3], faces [T, 3] int32 -> stretch [P, T].
 * Rejected: N < 0, T < 0, P < 1, Vb or Fb < 1, counts whose byte sizes overflow size_t (or 2^38 and more: the launch grids), null
 * required pointers (with N = 0 / T = 0 the per-vertex / per-face ones may be null), a workspace that is not 16-byte aligned,
 * out_normals without cov.  No allocation, no synchronisation, all on `stream`. */
#define DSN_MESH_POSE_BAD_BINDING 1
DSN_EXPORT int dsn_mesh_bind_normals(const float* body_xyz, int Vb, const int32_t* body_faces, int Fb, const int32_t* face_idx,
                                     const float* normals, int64_t N, float* cov, void* stream);
DSN_EXPORT size_t dsn_mesh_pose_workspace_bytes(int P, int Fb);
DSN_EXPORT int dsn_mesh_pose(const float* target_xyz, int P, int Vb, const int32_t* body_faces, int Fb, const int32_t* face_idx,
                             const float* uv, const float* h, const float* cov, int64_t N, float* out_verts, float* out_normals,
                             int32_t* status, void* workspace, void* stream);
DSN_EXPORT int dsn_mesh_stretch(const float* bind_verts, const float* posed_verts, int P, int64_t N, const int32_t* faces, int64_t T,
                                float* stretch, void* stream);

/* ---- the body model: SMPL parameters -> posed vertices for a whole clip (an addition within ABI 8: no existing entry point changes) ------
 * The reference reads the posed body's vertices from new_vertices/{i}.npy (tool/generate_novelpose_vertices.py writes them off-line with
 * EasyMocap's SMPL layer) and the Human3.6M datasets run utils/h36m_utils.get_rigid_transformation and get_bounds per item.  These two
 * calls make the same arrays on the device, P poses at a time: batch["xyz"], the datasets' pxyz, the joint_transforms of dsn_lbs_warp and
 * the bounds of dsn_camera_rays.  24 joints, as everywhere in this header.  The rule is fixed so that a numpy restatement
 * (tests/body_pose_restate.py) reproduces every output bit for bit, up to the float64 sin / cos / sqrt of the two platforms.
 * Parentheses give the order of operations; nothing is fused; "sum from 0" is s = 0, s = s + term in ascending index order.
 *   Shape (dsn_body_shape, float32): v_shaped[v,c] = v_template[v,c] + (sum from 0 over b of shapedirs[v,c,b] betas[b]); with shapedirs
 *             or betas NULL or B = 0: v_shaped = v_template.  joints[j,c] = sum from 0 over v of J_regressor[j,v] v_shaped[v,c] (dense
 *             regressor [24, V]; J_regressor and joints NULL together: the caller has the joints, the datasets ship joints.npy).
 *   Joint chain (float64 from the float32 inputs; utils/h36m_utils.py:210-264 batch_rodrigues + get_rigid_transformation, operation for
 *             operation):  per joint p = poses[j]:  q = p + 1e-8;  angle = sqrt((q0 q0 + q1 q1) + q2 q2);  r = p / angle;
 *             K = [0 -r2 r1; r2 0 -r0; -r1 r0 0];  (K K)_ij = (K_i0 K_0j + K_i1 K_1j) + K_i2 K_2j;
 *             R = (I + sin(angle) K) + (1 - cos(angle)) (K K).
 *             T_j = [R_j | t_j; 0 0 0 1] with t_0 = joints[0], t_j = joints[j] - joints[parents[j]];  G_0 = T_0,
 *             G_j = G_parents[j] T_j, every element ((a_r0 b_0c + a_r1 b_1c) + a_r2 b_2c) + a_r3 b_3c, all four rows;
 *             rel_r = ((G_r0 J_0 + G_r1 J_1) + G_r2 J_2) + G_r3 0 with J = joints[j];  A_j = G_j with column 3 replaced by G_r3 - rel_r
 *             (A = G [I | -J]), rounded to float32 once.  Rh_mat = the same R of Rh, rounded to float32 (Rh NULL: the identity).
 *   Pose feature: pf[9 (j - 1) + 3 r + c] = float32(R_j[r,c] - (r == c)), j = 1..23: 207 values.
 *   Vertex work (float32): v_posed[v,c] = v_shaped[v,c] + (sum from 0 over k = 0..206 of pf[k] posedirs[k, 3 v + c]) (posedirs NULL:
 *             v_posed = v_shaped);  T[e] = sum from 0 over j = 0..23 of weights[v,j] A_j[e], e over the 12 elements of rows 0-2;
 *             xyz_smpl_r = ((T_r0 v_0 + T_r1 v_1) + T_r2 v_2) + T_r3;   xyz_r = ((Rh_mat_r0 s_0 + Rh_mat_r1 s_1) + Rh_mat_r2 s_2) + Th_r
 *             with s = xyz_smpl (EasyMocap's vertices @ R.T + Th, the inverse of h36m_dataset.py:113; Th NULL: zeros).
 *   Bounds:   per pose and axis the exact minimum and maximum of xyz under the total order of the values with -0 below +0; an axis
 *             with a NaN coordinate anywhere in the pose: NaN for both.  Then the float32 padding of the datasets:
 *             DSN_BODY_PAD_ZJU_TRAIN min - 0.1f, max + 0.1f (zju_mocap_dataset.py:60-62); DSN_BODY_PAD_ZJU_EVAL z only, 0.05f (:64-65);
 *             DSN_BODY_PAD_H36M all axes, 0.05f (h36m_utils.py:372-379); DSN_BODY_PAD_NONE nothing.
 *   NaN:      nothing is patched.  A NaN in one pose's parameters reaches that pose's outputs only: no sum runs across poses.
 * dsn_body_shape: v_template [V,3], shapedirs [V,3,B], betas [B], J_regressor [24,V] -> v_shaped [V,3], joints [24,3] (all device).
 * dsn_body_pose: v_shaped [V,3], joints [24,3], weights [V,24], posedirs [207, 3V] or NULL, poses [P,24,3], Rh [P,3] or NULL, Th [P,3]
 * or NULL (device); parents_host: 24 int32 in HOST memory (the kinematic tree; entry 0 is ignored), read before the call returns.
 * Outputs (device; any but xyz may be NULL): xyz [P,V,3], xyz_smpl [P,V,3], A [P,24,4,4] row-major, bounds [P,2,3], Rh_mat [P,3,3].
 * workspace: dsn_body_pose_workspace_bytes(V, P) bytes (0 for bad sizes and for P = 0), 256-byte aligned, earlier contents not read;
 * after the call it begins with the pose features the call used, [P][208] float32 (207 and a zero), for whoever wants to look.
 * Three launches: the chain (one wave per pose), the vertex work (256 vertices x 8 poses per workgroup: a posedirs element is loaded
 * once per 8 poses), the bounds' final pass.  No atomics, one writer per output word, no sum whose order depends on the launch: P poses
 * in one call give the bits of P calls of one, wherever a pose sits in the call, and every call returns the same bits.
 * P = 0 is a valid call that launches nothing (poses, outputs and workspace may be NULL).  Rejected: V < 1, P < 0, V > 2^28, P > 2^18,
 * an unknown pad_mode, a parents_host[i] outside [0, i) for i >= 1, null required pointers, a small or misaligned workspace; for
 * dsn_body_shape B < 0 or > 4096, shapedirs without betas, joints without J_regressor or the reverse.  No allocation, no
 * synchronisation, all on `stream`. */
#define DSN_BODY_PAD_NONE 0
#define DSN_BODY_PAD_ZJU_TRAIN 1
#define DSN_BODY_PAD_ZJU_EVAL 2
#define DSN_BODY_PAD_H36M 3
DSN_EXPORT int dsn_body_shape(const float* v_template, const float* shapedirs, const float* betas, int B, const float* J_regressor, int V,
                              float* v_shaped, float* joints, void* stream);
DSN_EXPORT size_t dsn_body_pose_workspace_bytes(int V, int P);
DSN_EXPORT int dsn_body_pose(const float* v_shaped, const float* joints, const int32_t* parents_host, const float* weights,
                             const float* posedirs, int V, const float* poses, const float* Rh, const float* Th, int P, int pad_mode,
                             float* xyz, float* xyz_smpl, float* A, float* bounds, float* Rh_mat, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ---- mesh preview (an addition within ABI 8: no existing entry point changes) -------------------------------------------------------
 * utils/visualizer.py:144-168 Visualizer3D.render_mesh (pyrender: PerspectiveCamera(yfov = pi/3, aspect 1), a SpotLight of intensity 30
 * with cone angles pi/16 and pi/6 at the camera's pose, white background, no ambient light): a deterministic triangle rasteriser with
 * that camera and light.  It is NOT a pixel copy of pyrender (GL rasterisation and its PBR shader cannot be pinned); camera, light
 * geometry, image orientation (row 0 is the top, +x to the right), dtypes and background are pyrender's, and the rule below is fixed
 * so that a numpy restatement (tests/raster_restate.py) reproduces face and depth bit for bit.  All float32, no fused multiply-add,
 * `/` and sqrt correctly rounded; parentheses give the order of operations.
 *   verts [n_verts, 3] float32, faces [n_faces, 3] int32 (device); cam_pose_host: 12 floats in HOST memory, the rows of the
 *   camera-to-world pose [R | t] (camera looking down -z, y up); fx, fy: the NDC scales 1 / (aspect tan(yfov / 2)) and
 *   1 / tan(yfov / 2); light_host: 4 floats in HOST memory {intensity, cos_inner, cos_outer, base}.  Both host arrays are read
 *   before the call returns.
 * Vertex:   d = v - t;  c_k = (d0 R0k + d1 R1k) + d2 R2k;  w = -c_2;  xn = (fx c_0) / w, yn = (fy c_1) / w;
 *           px = (xn + 1) (W / 2), py = (1 - yn) (H / 2);  X = rint(px 256), Y = rint(py 256) (round-half-even, 1/256 px);
 *           valid when w > znear, px and py are finite and |X|, |Y| <= 2^24;  iw = 1 / w.
 * Triangle: dropped when a vertex index is outside [0, n_verts) (checked on the device), a vertex is invalid, or its signed integer
 *           area (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) is 0.  Two-sided: with a negative area vertices 1 and 2 are swapped (P = (v0, v2,
 *           v1)) and the area negated.  There is NO near-plane clipping: a triangle with a vertex at or behind znear is dropped whole.
 * Coverage: E_k(p) = (bx - ax)(py - ay) - (by - ay)(px - ax) in int64 with (a, b) = (P[k+1], P[k+2]) (indices mod 3), the edge opposite
 *           P[k].  The pixel centre p = (256 x + 128, 256 y + 128) is covered when every E_k > 0, or E_k = 0 on a top-left edge
 *           (by - ay < 0, or by = ay and bx > ax): a pixel on an edge two triangles share belongs to exactly one of them.
 * Depth:    l_k = float(E_k) / float(area);  q = (l_0 iw_0 + l_1 iw_1) + l_2 iw_2 (iw of P[k]);  z = 1 / q, the camera-space distance along
 *           -z.  Per pixel the smallest (z bits, face index) wins: nearest fragment, and on equal depth the lowest face index, whatever
 *           the order the triangles arrive in.  Every call returns the same bits.
 * Shade:    flat, two-sided, the diffuse term of a glTF punctual spotlight at the camera pointing down -z.
 *           xn = float(2 x + 1) / W - 1, yn = 1 - float(2 y + 1) / H;  p = ((xn z) / fx, (yn z) / fy, -z);
 *           r2 = (px px + py py) + z z, r = sqrt(r2);  s = clamp((z / r - cos_outer) / (cos_inner - cos_outer), 0, 1)^2;
 *           n = (c1 - c0) x (c2 - c0) from the camera coordinates of the face's vertices in the order given, each component
 *           a b - c d;  nn = sqrt((n0 n0 + n1 n1) + n2 n2);  ndl = |(n0 px + n1 py) - n2 z| / (nn r), or 0 when nn = 0;
 *           col = ((k s) ndl) / r2 with k = (base intensity) / float(pi);  level = floor(min(col, 1) 255 + 0.5) in all three channels.
 * Outputs (device; each may be NULL, not all): out_face [H, W] int32 (-1 empty), out_depth [H, W] float32 z (0 where empty, as
 * pyrender's depth), out_color [H, W, 3] uint8 (255 where empty).  A mesh with 0 faces gives the empty image.
 * Rejected: null required pointers, H or W outside 1 ... 16384, negative counts or 2^31 and more, a workspace smaller than
 * dsn_raster_workspace_bytes(n_verts, n_faces, H, W) (0 for bad sizes) or not 16-byte aligned, fx / fy / znear not finite, znear <= 0
 * (depth must be positive: its bits are ordered as integers), light values not finite or cos_inner <= cos_outer.
 * Kernels: a 64-bit visibility buffer (depth bits << 32 | face) cleared by the call, one thread per vertex, one thread per triangle
 * with one 64-bit unsigned atomic minimum per covered pixel; a triangle whose pixel bounding box holds more than
 * DSN_RM_BIG_PIXELS pixels is rasterised by a whole wave instead.  No allocation, no synchronisation, all on `stream`. */
#define DSN_RM_BIG_PIXELS 16      /* measured: scripts/bench_render_mesh.py, profiles/render_mesh_bench.json */
DSN_EXPORT size_t dsn_raster_workspace_bytes(int64_t n_verts, int64_t n_faces, int H, int W);
DSN_EXPORT int dsn_raster_mesh(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cam_pose_host,
                               float fx, float fy, float znear, const float* light_host, int H, int W, int32_t* out_face,
                               float* out_depth, uint8_t* out_color, void* workspace, size_t workspace_bytes, void* stream);
/* measurement (scripts/bench_render_mesh.py): enqueue only these kernels (0 = all; one mesh and one workspace through the phases of a
 * frame, in order), and the box size above which a triangle takes the wave form (0 = DSN_RM_BIG_PIXELS).  The image does not depend on
 * big_pixels. */
#define DSN_RM_CLEAR 1
#define DSN_RM_PROJECT 2
#define DSN_RM_RASTER 4
#define DSN_RM_RASTER_BIG 8
#define DSN_RM_SHADE 16
DSN_EXPORT int dsn_raster_mesh_ex(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cam_pose_host,
                                  float fx, float fy, float znear, const float* light_host, int H, int W, int32_t* out_face,
                                  float* out_depth, uint8_t* out_color, void* workspace, size_t workspace_bytes, int phases,
                                  int big_pixels, void* stream);
/* The preview with per-vertex attributes: dsn_raster_mesh_ex's arguments, then
 *   vertex_normals [n_verts, 3] float32, world space (NULL: none; required by DSN_RM_SMOOTH), e.g. dsn_mc_normals';
 *   vertex_colors  [n_verts, 3] float32 (NULL: none; required by out_attr), e.g. an albedo or a lit colour of the field;
 *   mode: DSN_RM_SMOOTH | DSN_RM_UNLIT (0: flat normals, lit);
 *   out_normal [H, W, 3] float32: the unit world normal the pixel was shaded with; out_attr [H, W, 3] float32: the interpolated
 *   colour, not clamped.  Both 0 where the pixel is empty; each may be NULL (one of the five outputs must not be).
 * Visibility is dsn_raster_mesh's own pass (the same kernels): face and depth have its bits.  Only the shade step differs; with P, l_k,
 * iw_k and z as defined for the depth:
 *   weights   b_k = (l_k iw_k) z (perspective-correct: they reproduce an affine function of the world position at the fragment);
 *   attribute a = (b_0 a_0 + b_1 a_1) + b_2 a_2 per component, a_k the value at P[k];
 *   normal    DSN_RM_SMOOTH: u = the attribute rule on the vertex normals, len = sqrt((u0 u0 + u1 u1) + u2 u2), world normal u / len,
 *             camera-space n_k = (m0 R0k + m1 R1k) + m2 R2k of m = u / len (as a vertex offset is rotated), nn = sqrt((n0 n0 + n1 n1) +
 *             n2 n2).  Falls back to the flat rule where (|m0| + |m1|) + |m2| of one of the three vertex normals is 0 or not finite, or
 *             len is 0 or not finite.  Flat: n and nn of dsn_raster_mesh's rule; world normal ((R_e0 n0 + R_e1 n1) + R_e2 n2) / nn, or 0
 *             unless 0 < nn < infinity.  Either way ndl = |(n0 px + n1 py) - n2 z| / (nn r), or 0 when nn = 0 (two-sided);
 *   colour    c_ch = the interpolated colour clamped to [0, 1] (c > 0 ? c : 0, then c < 1 ? c : 1: NaN is 0), or `base` in every channel
 *             without vertex_colors.  Lit: col_ch = min(((((c_ch intensity) / float(pi)) s) ndl) / r2, 1); DSN_RM_UNLIT: col_ch = c_ch
 *             (the colours as they are: e.g. the model's own lit colour painted on the mesh);  level = floor(col_ch 255 + 0.5).
 * Without attributes, mode 0: dsn_raster_mesh's image (and with out_normal and out_attr NULL too, its shade kernel).
 * The workspace is dsn_raster_workspace_bytes'.  Rejected: what dsn_raster_mesh_ex rejects, a mode outside 0 ... 3, DSN_RM_SMOOTH
 * without vertex_normals, out_attr without vertex_colors. */
#define DSN_RM_SMOOTH 1
#define DSN_RM_UNLIT 2
DSN_EXPORT int dsn_raster_mesh_attr(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* cam_pose_host,
                                    float fx, float fy, float znear, const float* light_host, int H, int W, int32_t* out_face,
                                    float* out_depth, uint8_t* out_color, void* workspace, size_t workspace_bytes, int phases,
                                    int big_pixels, const float* vertex_normals, const float* vertex_colors, int mode, float* out_normal,
                                    float* out_attr, void* stream);

/* ---- the datasets' image preparation on the device (an addition within ABI 8: no existing entry point changes) -------------------------
 * Between cv2.imread and the ray sampler the reference's datasets run OpenCV on the host (dataloader/zju_mocap_dataset.py:84-123,
 * :192-213; dataloader/h36m_dataset.py:88-93, :128-158, :182-184): cv2.undistort, cv2.dilate / cv2.erode with box kernels, an
 * INTER_AREA and INTER_NEAREST cv2.resize, / 255.  The four entry points below do that work on device arrays.  They follow the rule
 * written out here, which has the shape of OpenCV's fixed-point path (CV_16SC2 maps, INTER_BITS = 5) - cv2's own undistortion map
 * differs between its versions and SIMD paths, and its bits are NOT claimed.  tests/image_prep_restate.py restates the rule in numpy;
 * the kernels reproduce the restatement bit for bit.
 * The rule.
 *   1. Map.  Per image: K [3, 3] float64 row-major (fx = K[0], cx = K[2], fy = K[4], cy = K[5]; K[1], the skew, is not read - callers
 *      refuse a value other than 0) and D [nd] float64 = (k1, k2, p1, p2[, k3[, k4, k5, k6]]), nd = 4, 5 or 8, missing terms 0.  For the
 *      destination pixel (i, j) (row, column), directly from these inputs in float64, one rounding per operation, nothing fused and
 *      nothing carried from pixel to pixel:
 *          x = (j - cx) / fx          y = (i - cy) / fy          x2 = x x     y2 = y y     r2 = x2 + y2     t = (2 x) y
 *          kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2)
 *          xd = (x kr + p1 t) + p2 (r2 + 2 x2)          yd = (y kr + p1 (r2 + 2 y2)) + p2 t
 *          us = (fx xd + cx) 32       vs = (fy yd + cy) 32
 *      If us or vs is not finite or |us| >= 2^30 or |vs| >= 2^30 the pixel is an OUTSIDE pixel: every tap reads 0.  Otherwise
 *      iu = rint(us), iv = rint(vs) (halves to even), sx = iu >> 5, ax = iu & 31, sy = iv >> 5, ay = iv & 31 (arithmetic shifts).
 *   2. Taps.  s00 = src(sy, sx), s01 = src(sy, sx + 1), s10 = src(sy + 1, sx), s11 = src(sy + 1, sx + 1); a tap outside the image
 *      reads 0.  Integer weights w00 = (32 - ay)(32 - ax), w01 = (32 - ay) ax, w10 = ay (32 - ax), w11 = ay ax (their sum is 1024).
 *          uint8:    out = (s00 w00 + s01 w01 + s10 w10 + s11 w11 + 512) >> 10          (integers: no order)
 *          float32:  out = ((s00 f00 + s01 f01) + s10 f10) + s11 f11,  f = float32(w) / 1024 (exact), float32, nothing fused.
 *      Per channel, 1 or 3 interleaved channels.
 *   3. Box morphology on uint8 [H, W], k = 1 ... 15: dst(y, x) = max (DSN_PREP_DILATE) or min (DSN_PREP_ERODE) of src(y - a + dy,
 *      x - a + dx) over dy, dx = 0 ... k - 1 with the anchor a = k / 2 (integer division: an even box reaches k / 2 up and left and
 *      k - 1 - k / 2 down and right); pixels outside the image do not take part.
 *   4. Resize by c = 1, 2 or 4 (H and W multiples of c; output [H / c, W / c]).  DSN_PREP_NEAREST: dst(y, x) = src(c y, c x).
 *      DSN_PREP_AREA over the block src(c y .. c y + c - 1, c x .. c x + c - 1) per channel: uint8 with the integer block sum s:
 *      c = 2: (s + 2) >> 2 (half up); c = 4: s / 16 rounded half to even; float32: the block summed in row-major order in float32,
 *      times float32(1 / c^2).  c = 1 copies.
 *   5. The ZJU item (dsn_image_prep), in the reference's order: fg = (msk_cihp != 0) as 0 / 1; fg_u = undistort(fg) (rule 1-2, uint8:
 *      1 where the weights of the foreground taps reach 512); msk_fg = dilate(fg_u, border); im = undistort(img) msk_fg; im_small =
 *      area(im, c); msk_fg_small = nearest(msk_fg, c); msk_cihp_small = nearest(msk_cihp, c) - the RAW mask, not undistorted, as the
 *      reference has it; out_img = float64(im_small) / 255.0 (one float64 division), for DSN_PREP_F32 rounded to float32 once more.
 * Arrays: images [N, H, W] or [N, H, W, 3] (channels interleaved), contiguous; K [N, 3, 3], D [N, nd] float64, on the device.
 * Kernels (csrc/dsn_prep.hip): workgroups of 256 threads own tiles of DSN_PREP_TILE_W x DSN_PREP_TILE_H pixels at full resolution of
 * image blockIdx.z.  Morphology loads the tile with its halo into LDS and runs a row pass and a column pass.  dsn_image_prep is ONE
 * launch: map and foreground bit of tile and halo into LDS (the halo's map is recomputed by the neighbouring workgroups, the tile's
 * own is kept), the dilation from LDS, the image's taps times the mask, the c x c blocks from LDS, 16-byte stores of the float
 * rows and 4-byte stores of the uint8 rows wherever a row starts on that grid.  No atomics, no workspace, one writer per element: the
 * same bits every call; an image's outputs depend on that image's inputs only (a NaN in one K stays in its image, whose undistorted
 * outputs are 0).
 * N == 0: success, nothing is enqueued.  Rejected before anything is enqueued: N < 0 or > 65535, H or W outside 1 ... 32768, nd not
 * 4 / 5 / 8, channels not 1 / 3, k or border outside 1 ... 15, c not 1 / 2 / 4 or not dividing H and W, an unknown dtype / op / mode,
 * and - with N > 0 - a NULL required pointer or src == dst.  dsn_image_prep: out_img is required; out_img_u8 [N, H, W, 3] (im_small),
 * out_msk_fg and out_msk_cihp [N, H, W] may each be NULL. */
#define DSN_PREP_U8 0
#define DSN_PREP_F32 1
#define DSN_PREP_F64 2
#define DSN_PREP_DILATE 0
#define DSN_PREP_ERODE 1
#define DSN_PREP_NEAREST 0
#define DSN_PREP_AREA 1
#define DSN_PREP_TILE_W 64
#define DSN_PREP_TILE_H 16
#define DSN_PREP_MAX_SIDE 32768
DSN_EXPORT int dsn_image_undistort(const void* src, void* dst, const double* K, const double* D, int nd, int N, int H, int W,
                                   int channels, int dtype, void* stream);
DSN_EXPORT int dsn_image_morph(const uint8_t* src, uint8_t* dst, int N, int H, int W, int k, int op, void* stream);
DSN_EXPORT int dsn_image_resize(const void* src, void* dst, int N, int H, int W, int channels, int dtype, int c, int mode,
                                void* stream);
DSN_EXPORT int dsn_image_prep(const uint8_t* img, const uint8_t* msk_cihp, const double* K, const double* D, int nd, int N, int H0,
                              int W0, int c, int border, int out_dtype, void* out_img, uint8_t* out_img_u8, uint8_t* out_msk_fg,
                              uint8_t* out_msk_cihp, void* stream);

/* ---- LPIPS: test.py:18-23, 77-91's lpips_alex / lpips_vgg on the device (csrc/dsn_lpips.hip; additions within ABI 8) ----
 * The rule follows the `lpips` package v0.1, LPIPS(net = 'alex' | 'vgg', lpips = True, spatial = False) in eval mode, as test.py calls it.
 * PARITY WITH THE PACKAGE IS UNVERIFIED: neither lpips nor torchvision was available where this was written; the kernels are pinned to
 * the restatement of this rule (tests/lpips_restate.py), and tests/test_lpips_package.py compares with the package where it imports.
 *   Inputs.  Two stacks [F, H, W, 3] on the device: img float32, BGR in [0, 1], clamped by the caller (as for dsn_image_psnr); gt float64
 *      or float32, cast to float32 first (test.py:80's .float()).  Per pixel and channel, float32, one rounding per operation:
 *      x = 2 v - 1; the channel order reversed (flip(1): BGR -> RGB); then (x - shift) / scale with shift = (-.030, -.088, -.188),
 *      scale = (.458, .448, .450) for R, G, B.  rgb_pm1 != 0: the stacks are RGB in [-1, 1] already (the package's own call surface):
 *      no 2 v - 1, no flip.
 *   Backbones.  Convolutions with zero padding, bias, ReLU; output side floor((n + 2 p - k) / s) + 1; max pooling in floor mode,
 *      floor((n - k) / s) + 1.  DSN_LPIPS_ALEX: conv 3->64 k11 s4 p2, pool 3/2, conv 64->192 k5 p2, pool 3/2, conv 192->384 k3 p1, conv
 *      384->256 k3 p1, conv 256->256 k3 p1; taps behind each of the five ReLUs (64, 192, 384, 256, 256 channels).  DSN_LPIPS_VGG:
 *      torchvision VGG-16 `features`: 3 x 3 p1 convolutions of 64, 64 | 128, 128 | 256, 256, 256 | 512, 512, 512 | 512, 512, 512 channels
 *      with a 2/2 pool between the groups; taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (64, 128, 256, 512, 512 channels).
 *   Smallest image: 31 x 31 (alex), 16 x 16 (vgg); below it the package raises inside a pooling layer: DSN_LPIPS_TOO_SMALL and NaN.
 *   Head, per tap l: n = f / (sqrt(sum_c f^2) + 1e-10) per pixel (the eps outside the root: an all-zero vector gives 0);
 *      d_l = mean over the pixels of sum_c w_l[c] (n0 - n1)^2 with the tap's lin weights (1 x 1, no bias); the result is sum_l d_l.
 *      The head reads the float32 features and computes in float64: a wave per pixel, channels across its lanes, butterfly sums;
 *      a workgroup per share of the pixels (shares: a function of the tap's size alone), partials added in index order.
 *   Convolution arithmetic: fp32-equivalent on the split-fp16 scheme of csrc/dsn_field16.hip: every operand v = hi + lo 2^-12 (hi =
 *      fp16(v), lo = fp16((v - hi) 2^12): 22 significand bits), W.x = W_hi x_hi + 2^-12 (W_hi x_lo + W_lo x_hi) in three
 *      v_mfma_f32_32x32x16_f16 products with fp32 accumulation; implicit GEMM with M = output pixels of one image (tiles of
 *      DSN_LPIPS_TILE_M), N = output channels, k = (ky kw + kx) Cin + ci padded to 16; one kernel for all 18 shapes.
 *   Range.  The split covers |v| < DSN_LPIPS_RANGE_MAX = 32 768 (beyond it lo leaves fp16).  An activation outside it (NaN
 *      included) sets DSN_LPIPS_RANGE for its frame; a weight or bias outside it sets DSN_LPIPS_RANGE for every frame evaluated with
 *      that packed image; the frame's results are NaN.  There is no exact-fp32 fallback.  Values below 2^-36 in magnitude lose their lo part.
 *   Non-finite input: a NaN or infinite pixel sets DSN_LPIPS_NONFINITE for its frame (result NaN); other frames are not touched.
 *   Determinism: no float atomics (status bits are integer ORs); the same bits on every call; a frame gives the same bits alone or in
 *      any batch; d(a, b) and d(b, a) are bit-identical (both through the float32 path); identical images give exactly 0.0.
 * dsn_lpips_pack: conv_w / conv_b: HOST arrays of 5 (alex) or 13 (vgg) device pointers, float32 [Cout, Cin, k, k] / [Cout] in layer
 *   order; lin_w: host array of 5 device pointers, float32 [C_l].  packed: dsn_lpips_packed_bytes(net) bytes of device memory.
 * dsn_lpips_features: the five taps of stack [n, H, W, 3] float32 (interpreted as img is) as float32 [n, C_l, h_l, w_l] into the five
 *   device pointers of the host array out_taps5; out_status [n].  An image with a status has NaN taps (TOO_SMALL: taps untouched).
 * dsn_lpips: out [F], out_layers [F, 5] float64 (the d_l; they sum to out in index order), out_status [F] int32 (OR of DSN_LPIPS_*).
 * workspace: dsn_lpips_workspace_bytes(net, F, H, W) bytes (0 for bad sizes) serve F frames = 2 F images; it may hold anything on
 *   entry.  Kernels only: no allocation, no host copy, no synchronisation.  All device pointers 256-byte aligned where noted. */
#define DSN_LPIPS_ALEX 0
#define DSN_LPIPS_VGG 1
#define DSN_LPIPS_OK 0
#define DSN_LPIPS_TOO_SMALL 1
#define DSN_LPIPS_RANGE 2
#define DSN_LPIPS_NONFINITE 4
#define DSN_LPIPS_RANGE_MAX 32768.0f
#define DSN_LPIPS_TILE_M 64
#define DSN_LPIPS_MAX_SIDE 4096
#define DSN_LPIPS_MAX_IMAGES 65534
DSN_EXPORT size_t dsn_lpips_packed_bytes(int net);
DSN_EXPORT int dsn_lpips_pack(int net, const float* const* conv_w, const float* const* conv_b, const float* const* lin_w, void* packed,
                              void* stream);
DSN_EXPORT size_t dsn_lpips_workspace_bytes(int net, int F, int H, int W);
DSN_EXPORT int dsn_lpips_features(const void* packed, int net, const float* stack, int n, int H, int W, int rgb_pm1,
                                  float* const* out_taps5, int32_t* out_status, void* workspace, size_t workspace_bytes, void* stream);
DSN_EXPORT int dsn_lpips(const void* packed, int net, const float* img, const double* gt_f64, const float* gt_f32, int F, int H, int W,
                         int rgb_pm1, double* out, double* out_layers, int32_t* out_status, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---- Baseline JPEG on the device (csrc/dsn_jpeg.hip): the scripts' cv2.imwrite(path, img * 255) into a .jpg (validate.py:76-83,
 * novel_pose_vis.py:62-66, vis_lighting.py:62-65, test.py) from frames that are in HBM already.  The rule below is restated in
 * tests/jpeg_restate.py, which gives byte for byte the files Pillow writes through libjpeg-turbo (quality q, optimize=False, no
 * restart markers); cv2.imwrite's own bytes are not claimed.  Integer arithmetic and integer atomics only: the same bytes on every
 * call, and a frame gives the same file alone or in any batch.
 *   Levels.  uint8 input passes through.  float32 input v: t = v * scale in float32 (scale = 255 for the scripts), rounded to the
 *      nearest integer with ties to even, saturated to [0, 255]; NaN gives 0 (+inf 255, -inf 0).  A NaN or infinite value sets
 *      DSN_JPEG_NONFINITE for its frame; the file is still valid.  This is what cv2.imwrite is understood to do to a float image
 *      (convertTo(CV_8U)); unverified.  rgb = 0: the three channels are B, G, R (as cv2.imwrite reads them); rgb != 0: R, G, B.
 *   Modes.  DSN_JPEG_420: three components, luma sampled 2 x 2 (libjpeg's and cv2's default); DSN_JPEG_444: three components, all
 *      1 x 1; DSN_JPEG_GRAY: the image has ONE channel ([F, H, W]) and the file one component.  The other modes read [F, H, W, 3].
 *   Colour (JFIF YCbCr, 16-bit fixed point, >> arithmetic):
 *      Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *      Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *      Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
 *   MCUs in row-major order.  GRAY: one 8 x 8 block; 444: Y, Cb, Cr; 420: a 16 x 16 MCU of Y00, Y01, Y10, Y11, Cb, Cr (Yrc = block
 *      row r, column c).  MCU counts: ceil(W / 8) x ceil(H / 8), for 420 ceil(W / 16) x ceil(H / 16).
 *   Edges (libjpeg's rule).  GRAY / 444: every plane is replicated right and down to the MCU grid.  420: luma is replicated right
 *      and down to ceil(W / 8) 8 x ceil(H / 8) 8; luma blocks of the last MCU column / row beyond that are DUMMY blocks: all 63 AC
 *      coefficients zero, DC = the quantised DC of the block before it in the MCU's own order (resolved in order: a dummy block may
 *      follow a dummy block; Y00 is never one).  Chroma at 420: the Cb / Cr plane is replicated right to ceil(W / 16) 16 columns and,
 *      if H is odd, down by one row; out(y, x) = (p(2y, 2x) + p(2y, 2x + 1) + p(2y + 1, 2x) + p(2y + 1, 2x + 1) + bias) >> 2 with
 *      bias 1 on even and 2 on odd x; the last of the ceil(H / 2) downsampled rows is then replicated down to ceil(H / 16) 8 rows.
 *   DCT.  d = sample - 128, then the IJG slow-integer forward DCT: pass 1 along every row, pass 2 along every column of the result.
 *      CONST_BITS = 13, PASS1_BITS = 2, DESCALE(x, n) = (x + (1 << (n - 1))) >> n (arithmetic).  One pass over d0 ... d7:
 *        t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4
 *        t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2
 *        out0 = (t10 + t11) << 2 in pass 1, DESCALE(t10 + t11, 2) in pass 2;  out4 likewise from t10 - t11
 *        z1 = (t12 + t13) 4433;  out2 = DESCALE(z1 + t13 6270, n);  out6 = DESCALE(z1 - t12 15137, n);  n = 11 in pass 1, 15 in pass 2
 *        z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7, z5 = (z3 + z4) 9633
 *        t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299, z1 *= -7373, z2 *= -20995, z3 *= -16069, z4 *= -3196, z3 += z5, z4 += z5
 *        out7 = DESCALE(t4 + z1 + z3, n), out5 = DESCALE(t5 + z2 + z4, n), out3 = DESCALE(t6 + z2 + z3, n), out1 = DESCALE(t7 + z1 + z4, n)
 *      The result is 8 x the orthonormal DCT; every intermediate fits int32.  Error against the exact transform for samples in
 *      [-128, 127]: a constant is off by at most 2^-14 and an odd output adds four products.  Pass 1 (outputs at 4 x sqrt(8) x the 1-D
 *      transform): operands up to 256, 512, 512, 1024 give 4 x 2304 x 2^-14 = 0.57 units, the DESCALE 0.5: e1 <= 1.07.  Pass 2 carries
 *      e1 through rows of absolute sum <= sqrt(8), times sqrt(8) / 4: 2 e1 = 2.14 units of 8 x DCT; its own operands (up to 8192,
 *      16384, 16384, 32768) give 73728 x 2^-14 / 4 = 1.13 units, its DESCALE 0.5.  Sum 3.77 units: |integer / 8 - float64 DCT| <=
 *      DSN_JPEG_DCT_BAR = 0.5 levels; tests hold the restatement to this bar (random and extreme blocks measure 0.18).
 *   Quantisation.  Base tables of Annex K (luminance for Y, chrominance for Cb / Cr).  s = 5000 / q (integer division) for q < 50,
 *      else 200 - 2 q; entry = clamp((base s + 50) / 100, 1, 255), q = 1 ... 100.  With d = 8 entry: a = |c| + (d >> 1), quotient
 *      a / d by integer division, sign of c restored.
 *   Entropy coding.  Baseline Huffman, the four tables of Annex K (DC / AC luminance for Y, chrominance for Cb and Cr), one scan of
 *      interleaved MCUs, no restart markers.  DC: the difference to the previous block of the same component (dummy blocks
 *      included; predictors start at 0), coded as its size s = bits of |diff| followed by s amplitude bits.  AC in zigzag order: a
 *      non-zero coefficient after a run of r zeros writes r / 16 ZRL codes (0xF0), the code of ((r % 16) << 4 | s) and s amplitude
 *      bits; EOB (0x00) unless coefficient 63 is non-zero.  A negative value v is written as v + 2^s - 1.  Bits most significant first.
 *      The last byte is padded with 1-bits; every 0xFF byte of the scan, the padded one included, is followed by 0x00; then EOI.
 *      At q = 100 AC sizes stay <= 10 and DC-difference sizes <= 11: a block's scan is at most 1658 bits (20 for DC, 63 x 26 for AC).
 *   Header (what Pillow writes with optimize=False): SOI; APP0 "JFIF\0" 1.01, units 0, density 1 x 1, no thumbnail; one DQT segment per
 *      table (8-bit, zigzag order); SOF0 (8 bits, H, W, components 1 .. 3 with sampling 0x22 / 0x11, tables 0, 1, 1); one DHT segment
 *      per table in the order DC0, AC0, DC1, AC1 (GRAY: DC0, AC0); SOS (Ss 0, Se 63, Ah / Al 0).  623 bytes, GRAY 328.
 *   Kernels.  k_jpeg_coef: a workgroup per MCU, a wave per block, a lane per sample: levels, colour, edges, downsampling, the DCT
 *      in int32 through LDS, quantisation, dummy DCs -> int16 coef [F][block in scan order][64 in zigzag order].  k_jpeg_bits: a wave
 *      per block, a lane per coefficient: the non-zero mask is one ballot, a lane's run its distance to the previous set bit; its
 *      ZRLs, code and amplitude are one word of at most 59 bits -> the block's bit length.  The project's tile scan (per tile, then
 *      one workgroup over the tiles' totals, frames side by side) turns lengths into bit offsets.  k_jpeg_emit: the same words again,
 *      placed by a wave prefix sum, merged into the cleared unstuffed stream with 32-bit atomic OR.  k_jpeg_ffcount / tile scan /
 *      k_jpeg_stuff: 0xFF bytes per 16-byte chunk, their prefix, then the scatter behind the header with the inserted zeros, the
 *      1-padding of the last byte, EOI, the frame's length and status.  The header travels in the kernel arguments.
 *   Bounds.  dsn_jpeg_max_bytes = header + 416 bytes per block (208 with every byte stuffed) + 2.  `capacity` is the stride of `out`
 *      in bytes; a frame that needs more sets DSN_JPEG_OVERFLOW for that frame alone: nothing is written at or past the capacity,
 *      out_lengths still holds the needed length.  Bit offsets are int32: blocks x 1664 must stay below 2^31, H and W <= 65535 (the
 *      SOF0 fields): that admits every H W <= 2^24 pixels with H, W >= 16 in all modes (the entry points compute the block count).
 * images: [F, H, W, 3] (GRAY: [F, H, W]) contiguous, dtype DSN_JPEG_U8 or DSN_JPEG_F32.  coef: int16 [F, blocks, 64].  out: uint8
 * [F, capacity]; bytes past a frame's length are not touched.  out_lengths: int32 [F]; out_status: uint32 [F] (OR of DSN_JPEG_*).
 * dsn_jpeg_coefficients writes coef and out_status (NONFINITE).  dsn_jpeg_scan reads coef, ORs status_in [F] (may be null) into
 * out_status.  dsn_jpeg_encode is their composition bit for bit; its coef live in the workspace.  workspace:
 * dsn_jpeg_workspace_bytes(F, H, W, mode) bytes (0 for bad sizes), anything on entry, 256-byte aligned.  dsn_jpeg_header_host writes the
 * header into HOST memory and returns its length through *len (capacity >= DSN_JPEG_HEADER_MAX suffices).  No allocation, no
 * host copy, no synchronisation. */
#define DSN_JPEG_420 0
#define DSN_JPEG_444 1
#define DSN_JPEG_GRAY 2
#define DSN_JPEG_U8 0
#define DSN_JPEG_F32 1
#define DSN_JPEG_NONFINITE 1u
#define DSN_JPEG_OVERFLOW 2u
#define DSN_JPEG_HEADER_MAX 640
#define DSN_JPEG_BLOCK_BYTES 208          /* ceil(1658 / 8): the unstuffed stream's share per block */
#define DSN_JPEG_DCT_BAR 0.5
#define DSN_JPEG_MAX_FRAMES 65535
DSN_EXPORT size_t dsn_jpeg_max_bytes(int H, int W, int mode);
DSN_EXPORT size_t dsn_jpeg_workspace_bytes(int F, int H, int W, int mode);
DSN_EXPORT int dsn_jpeg_header_host(int H, int W, int mode, int quality, uint8_t* out_host, int capacity, int* len);
DSN_EXPORT int dsn_jpeg_coefficients(const void* images, int dtype, int F, int H, int W, int mode, int quality, int rgb, float scale,
                                     int16_t* coef, uint32_t* out_status, void* stream);
DSN_EXPORT int dsn_jpeg_scan(const int16_t* coef, const uint32_t* status_in, int F, int H, int W, int mode, int quality, uint8_t* out,
                             size_t capacity, int32_t* out_lengths, uint32_t* out_status, void* workspace, size_t workspace_bytes,
                             void* stream);
DSN_EXPORT int dsn_jpeg_encode(const void* images, int dtype, int F, int H, int W, int mode, int quality, int rgb, float scale,
                               uint8_t* out, size_t capacity, int32_t* out_lengths, uint32_t* out_status, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---- Baseline JPEG DECODING on the device (csrc/dsn_jpegd.hip): the datasets' cv2.imread(img_path) of a .jpg
 * (dataloader/zju_mocap_dataset.py:86, h36m_dataset.py:128, novel_poses_dataset.py:119): file bytes go up, the uint8 frame that
 * dsn_image_prep takes appears in HBM, a few status words come back.  The rule below is restated in tests/jpeg_decode_restate.py,
 * which gives pixel for pixel what Pillow decodes through libjpeg-turbo at its default settings (slow-integer IDCT, fancy
 * upsampling); cv2.imread's own pixels are not claimed.  Integer arithmetic only, no float atomics: the same bits on every call,
 * and a frame decodes the same alone or in any batch.
 *   Scope.  Baseline sequential files (SOF0), 8 bits, ONE interleaved scan, 1 component (DSN_JPEG_GRAY) or 3 components sampled
 *      4:4:4 (DSN_JPEG_444) or 4:2:0 (DSN_JPEG_420); quantisation (8-bit entries) and Huffman tables as the file gives them (DQT /
 *      DHT ids 0 ... 3); APPn and COM segments are skipped, so a three-component file is always taken as YCbCr.  Everything else is
 *      refused by dsn_jpeg_parse_host with a named status and reaches no kernel: DSN_JPEGD_PROGRESSIVE (SOF2), _EXTENDED (SOF1, 3,
 *      5 - 7), _ARITHMETIC (SOF9 - 15, DAC), _PRECISION (12-bit), _SAMPLING (4:2:2 and the rest), _COMPONENTS (2, 4), _TABLE16,
 *      _MULTISCAN (an SOS with fewer components than the frame), _RESTART (DRI with a non-zero interval), _MISSING_TABLE,
 *      _BAD_TABLE (code lengths that overflow, more than 256 symbols, a DC symbol above 15), _NO_EOI, _TRUNCATED, _BAD_SEGMENT,
 *      _NOT_JPEG, _TOO_LARGE (2^27 bytes and up, or more blocks than the encoder takes).
 *   Host part.  dsn_jpeg_parse_host reads the header and the file's last two bytes (EOI) and fills a dsn_jpegd_desc: H, W, mode,
 *      per-component selectors, the quantisation tables in the file's zigzag order, every Huffman table as bits / vals and in the
 *      decoders' form: lim[l - 1] = (first code that is NOT of length <= l) << (16 - l), base[l - 1] = (index of the first symbol of
 *      length l) - (its code); a 16-bit window v holds a code of length l = the smallest l with v < lim[l - 1], and the symbol is
 *      vals[(base[l - 1] + (v >> (16 - l))) & 255].  scan_offset / scan_length: the bytes between SOS and EOI.  A marker inside the
 *      scan is found by the device.  All frames of one device call share H, W and mode; tables may differ per frame.
 *   Unstuffing.  In the scan a 0x00 behind a 0xFF is dropped.  Any other byte behind a 0xFF, or a 0xFF as the scan's last byte, is a
 *      marker: DSN_JPEGD_MARKER.  The unstuffed scan of U bytes is 8 U bits, most significant bit first; bits past it read as 0.
 *   Symbols.  A decoder state is (bit position p, block k within the MCU, zigzag index z); the scan starts at (0, 0, 0).  One step
 *      at z = 0 reads a code of the block's component's DC table -> s = symbol & 15, then s bits v: the DC difference (v if its top
 *      bit is set, else v - 2^s + 1); z = 1.  At z > 0 it reads a code of the AC table -> r = symbol >> 4, s = symbol & 15, s bits:
 *      s = 0: r = 15 moves z on by 16, any other r ends the block; s > 0: z += r, the value is coefficient z, z += 1.  A z past 63
 *      ends the block; landing past 64 by a ZRL, or past 63 with a value (which is dropped), is DSN_JPEGD_OVERRUN.  At the end of a
 *      block k moves on (cyclically over the MCU's 1, 3 or 6 blocks) and z = 0.  A window that matches no code moves p on by one
 *      bit: DSN_JPEGD_UNMATCHED.  A symbol that needs bits past the scan's end is not decoded, and decoding ends there; so does a
 *      window without a code that has fewer than 16 bits left.
 *   Synchronisation (the parallel form).  The unstuffed scan is cut into subsequences of B bits (subseq_bits: a multiple of 32,
 *      128 ... 4096; S = max(1, ceil(8 U / B))).  Round 0: a thread per subsequence s decodes from (s B, 0, 0) until p >= (s + 1) B
 *      (or the scan's end) and records its entry, its exit state, the blocks it started and its error flags.  Round r: s takes the
 *      exit of s - 1 from the PREVIOUS round's buffer (two buffers, no race); equal to the entry it used: it copies its exit over;
 *      else it decodes again from there and raises the frame's "changed" word.  Subsequence 0 is right from the start and after
 *      round r subsequences 0 ... r are, so a round that changes nothing comes after at most S rounds, and the fixed point IS the
 *      serial decode.  That round counts: `rounds` is the number of rounds up to and including it (1 for S = 1).  Rounds after it
 *      return at once.  Streams usually re-synchronise within a subsequence or two; a scan without end-of-block codes (noise at
 *      quality 100) may need about S rounds.
 *   Emit.  The tile scan of the blocks started per subsequence gives each its first block index; every subsequence decodes once
 *      more from its true entry into the cleared int16 coef [F, blocks, 64] (zigzag and scan order), DC as differences; blocks at
 *      or past the geometry's count are dropped.  Per component an integer prefix sum over its blocks in scan order (tile scan
 *      again) turns differences into DC values (int32 sums, stored as int16).
 *      This last pass stops behind the frame's last block (the rounds, which do not know block indices, run on to the scan's end):
 *      what follows it is never decoded, as in libjpeg, and the error flags speak of the frame's own blocks only.
 *   Status.  DSN_JPEGD_COUNT: the scan ends before the geometry's last block is complete, or the descriptor's scan does not lie
 *      inside its file.  Any of _UNMATCHED, _OVERRUN, _MARKER, _COUNT sets DSN_JPEGD_CORRUPT.  DSN_JPEGD_PADDING (a warning, not an
 *      error): more than 7 bits are left behind the last block, or the bits left are not all 1.  DSN_JPEGD_UNCONVERGED: the rounds run so far did not reach the fixed point; nothing was emitted.
 *   Dequantisation and IDCT.  coefficient x table entry in int32, then libjpeg's jpeg_idct_islow in int32 (wrapping; a 64-bit
 *      libjpeg agrees whenever nothing overflows, which holds for every file an 8-bit encoder writes): pass 1 down every column,
 *      pass 2 along every row of the result, CONST_BITS = 13, PASS1_BITS = 2.  One pass over i0 ... i7:
 *        z1 = (i2 + i6) 4433, t2 = z1 - i6 15137, t3 = z1 + i2 6270, t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13
 *        t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2
 *        u0 = i7, u1 = i5, u2 = i3, u3 = i1, z1 = u0 + u3, z2 = u1 + u2, z3 = u0 + u2, z4 = u1 + u3, z5 = (z3 + z4) 9633
 *        u0 *= 2446, u1 *= 16819, u2 *= 25172, u3 *= 12299, z1 *= -7373, z2 *= -20995, z3 = z3 (-16069) + z5, z4 = z4 (-3196) + z5
 *        u0 += z1 + z3, u1 += z2 + z4, u2 += z2 + z3, u3 += z1 + z4
 *        out0, 7 = DESCALE(t10 +- u3, n), out1, 6 = DESCALE(t11 +- u2, n), out2, 5 = DESCALE(t12 +- u1, n), out3, 4 = DESCALE(t13 +- u0, n)
 *      with n = 11 in pass 1 and 18 in pass 2, DESCALE(x, n) = (x + (1 << (n - 1))) >> n (arithmetic).  No zero-column shortcut (it
 *      gives the same bits).  The sample is (result & 1023) read as a signed 10-bit number, + 128, clamped to [0, 255].
 *   Chroma at 4:2:0 (libjpeg's "fancy" h2v2 upsampling).  The chroma plane is ceil(W / 2) x ceil(H / 2); padding takes no part.
 *      Wider than 2 columns: for output row y, near = row y / 2, far = the row above (y even) or below (y odd), the first / last row
 *      standing in for a missing neighbour; c(j) = 3 near(j) + far(j).  Output column x, j = x / 2: x even: (3 c(j) + c(j - 1) + 8)
 *      >> 4, x odd: (3 c(j) + c(j + 1) + 7) >> 4, a missing neighbour replaced by c(j) itself ((4 c + 8) >> 4, (4 c + 7) >> 4).
 *      At most 2 columns wide (W <= 4): the sample of (y / 2, x / 2), as libjpeg's downsampled_width > 2 test has it.
 *   Colour (16-bit fixed point, >> arithmetic, clamped to [0, 255]):
 *      R = Y + ((91881 (Cr - 128) + 32768) >> 16),  B = Y + ((116130 (Cb - 128) + 32768) >> 16)
 *      G = Y + ((-22554 (Cb - 128) - 46802 (Cr - 128) + 32768) >> 16)
 *   Output.  uint8 [F, H, W, 3] in B, G, R order (rgb = 0: what cv2.imread returns; a one-component file is replicated) or R, G, B
 *      (rgb != 0); gray_out != 0 (DSN_JPEG_GRAY only): [F, H, W].  A frame whose status has DSN_JPEGD_CORRUPT or _UNCONVERGED gets
 *      all-zero pixels: every output byte is defined.
 *   Kernels.  k_jd_ffcount / tile scan / k_jd_unstuff: the mirror of the encoder's stuffing, 16 bytes of the scan per thread,
 *      fetched with two aligned 16-byte loads that are made only inside [0, files_bytes).  k_jd_round: a thread per subsequence,
 *      a workgroup's subsequences all of one frame, whose six resolved Huffman tables lie in LDS; a divergent per-lane bit reader
 *      whose every word index is checked against the frame's stream.  k_jd_verdict: the frames' round counters.  k_jd_emit: the
 *      same reader, writing.  k_jd_idct: a wave per 8 blocks, a lane per column, then per row, through LDS, 8 samples per store into
 *      the component planes at the MCU grid's size.  k_jd_colour: a thread per pixel.  No MFMA: DSN_OWN_SIMD does not apply.
 * files: uint8 [files_bytes], the frames' files one behind the other, 16-byte aligned, files_bytes a multiple of 16 (pad the tail);
 * offsets: int64 [F + 1], file f = [offsets[f], offsets[f + 1]); desc: dsn_jpegd_desc [F] in DEVICE memory.  Every read of a frame's
 * scan is clipped to its own file, to files_bytes and to max_scan_bytes (>= every frame's scan_length; it sizes the workspace).
 * dsn_jpegd_sync: restart != 0 unstuffs and runs round 0 as the first of `rounds`; restart = 0 runs `rounds` further rounds on the
 * state in the workspace (same subseq_bits).  out_converged uint32 [F] / out_rounds int32 [F] (either may be null).
 * dsn_jpegd_coefficients: emit + DC from the workspace's converged state -> coef int16 [F, blocks, 64] (16-byte aligned), out_status
 * uint32 [F].  dsn_jpegd_pixels: coef, status (may be null: all frames good) -> out.  dsn_jpeg_decode: sync (restart, `rounds`
 * rounds) + coefficients + pixels, bit for bit, its coef in the workspace; a frame that needs more rounds comes back
 * DSN_JPEGD_UNCONVERGED, and the caller goes on with dsn_jpegd_sync (restart = 0), dsn_jpegd_coefficients and dsn_jpegd_pixels on
 * the same workspace (dsn_jpegd_workspace_coef: where its coef lie).  workspace: dsn_jpegd_workspace_bytes(F, H, W, mode,
 * max_scan_bytes) bytes (0 for bad sizes), 256-byte aligned, anything on entry of a restart.  No allocation, no host copy, no
 * synchronisation.  dsn_jpeg_parse_host: HOST memory in and out; returns 0 and the DSN_JPEGD_* parse status through *status. */
#define DSN_JPEGD_CORRUPT 1u
#define DSN_JPEGD_PADDING 2u
#define DSN_JPEGD_UNCONVERGED 4u
#define DSN_JPEGD_UNMATCHED 16u
#define DSN_JPEGD_OVERRUN 32u
#define DSN_JPEGD_MARKER 64u
#define DSN_JPEGD_COUNT 128u
#define DSN_JPEGD_MAX_FRAMES 16384
#define DSN_JPEGD_OK 0            /* dsn_jpeg_parse_host's status */
#define DSN_JPEGD_NOT_JPEG 1
#define DSN_JPEGD_TRUNCATED 2
#define DSN_JPEGD_PROGRESSIVE 3
#define DSN_JPEGD_EXTENDED 4
#define DSN_JPEGD_ARITHMETIC 5
#define DSN_JPEGD_PRECISION 6
#define DSN_JPEGD_SAMPLING 7
#define DSN_JPEGD_COMPONENTS 8
#define DSN_JPEGD_TABLE16 9
#define DSN_JPEGD_MULTISCAN 10
#define DSN_JPEGD_RESTART 11
#define DSN_JPEGD_MISSING_TABLE 12
#define DSN_JPEGD_BAD_TABLE 13
#define DSN_JPEGD_NO_EOI 14
#define DSN_JPEGD_BAD_SEGMENT 15
#define DSN_JPEGD_TOO_LARGE 16
typedef struct dsn_jpegd_huff {
    uint8_t bits[16];             /* codes per length 1 ... 16 */
    uint8_t vals[256];            /* the symbols in code order, zeros behind them */
    uint32_t lim[16];
    int32_t base[16];
} dsn_jpegd_huff;
typedef struct dsn_jpegd_desc {
    int32_t H, W, mode, ncomp;
    int32_t scan_offset, scan_length, file_length, reserved;
    uint8_t qsel[4], dcsel[4], acsel[4], pad[4];          /* per component: table ids */
    uint8_t quant[4][64];         /* zigzag order */
    dsn_jpegd_huff dc[4], ac[4];
} dsn_jpegd_desc;
DSN_EXPORT int dsn_jpeg_parse_host(const uint8_t* file_host, size_t bytes, dsn_jpegd_desc* desc_host, int* status);
DSN_EXPORT size_t dsn_jpegd_workspace_bytes(int F, int H, int W, int mode, size_t max_scan_bytes);
DSN_EXPORT int dsn_jpegd_workspace_coef(void* workspace, int F, int H, int W, int mode, size_t max_scan_bytes, int16_t** coef);
DSN_EXPORT int dsn_jpegd_sync(const uint8_t* files, size_t files_bytes, const int64_t* offsets, const dsn_jpegd_desc* desc, int F, int H,
                              int W, int mode, size_t max_scan_bytes, int subseq_bits, int restart, int rounds, uint32_t* out_converged,
                              int32_t* out_rounds, void* workspace, size_t workspace_bytes, void* stream);
DSN_EXPORT int dsn_jpegd_coefficients(const dsn_jpegd_desc* desc, int F, int H, int W, int mode, size_t max_scan_bytes, int subseq_bits,
                                      int16_t* coef, uint32_t* out_status, void* workspace, size_t workspace_bytes, void* stream);
DSN_EXPORT int dsn_jpegd_pixels(const int16_t* coef, const uint32_t* status, const dsn_jpegd_desc* desc, int F, int H, int W, int mode,
                                size_t max_scan_bytes, int rgb, int gray_out, uint8_t* out, void* workspace, size_t workspace_bytes,
                                void* stream);
DSN_EXPORT int dsn_jpeg_decode(const uint8_t* files, size_t files_bytes, const int64_t* offsets, const dsn_jpegd_desc* desc, int F, int H,
                               int W, int mode, size_t max_scan_bytes, int subseq_bits, int rounds, int rgb, int gray_out, uint8_t* out,
                               uint32_t* out_status, int32_t* out_rounds, void* workspace, size_t workspace_bytes, void* stream);

/* ---- PNG DECODING on the device (csrc/dsn_png.hip): the datasets' label masks (mask_cihp/....png, read with cv2.imread at
 * dataloader/zju_mocap_dataset.py:197 and zju_novel_pose_dataset.py:195, with imageio.imread at h36m_dataset.py:81,
 * h36m_dataset_test.py:81 and novel_poses_dataset.py:70): file bytes go up, the uint8 mask that dsn_image_prep takes appears in HBM.
 * PNG is lossless: the pixels are the ones every decoder gives, and tests/png_decode_restate.py restates the rule below and is held
 * to Pillow.  Integer arithmetic only; the only atomics are 32-bit integer ORs / adds in LDS and ORs into the frames' status words:
 * the same bits on every call, and a file decodes the same alone or in any batch.
 *   Scope.  Non-interlaced files of colour type 0 (grey; 1, 2, 4, 8 bits), 2 (RGB, 8 bits), 3 (palette; 1, 2, 4, 8 bits), 4 (grey +
 *      alpha, 8 bits) and 6 (RGBA, 8 bits); any number of IDAT chunks of any length (zero included); ancillary chunks are skipped,
 *      wherever they stand (tRNS and gAMA are not applied).  Everything else is refused by dsn_png_parse_host with a named status
 *      and reaches no kernel.
 *   Host part.  dsn_png_parse_host checks the signature, walks the chunks (every read bounded by `bytes`), checks the CRC-32 of
 *      IHDR, PLTE, IDAT and IEND, and fills a dsn_png_desc: W, H, bits, ctype, channels, row_bytes = ceil(W bits channels / 8),
 *      raw_bytes = H (1 + row_bytes), the palette (R, G, B; entries the file does not give are 0), nseg and zlen = the IDAT payloads'
 *      total, and up to seg_capacity segments {offset of the payload in the file, its length} (nseg may exceed seg_capacity: call
 *      again with room for nseg).  Statuses: DSN_PNG_NOT_PNG, _TRUNCATED (a chunk that runs past the file, or no IEND), _CRC,
 *      _BAD_IHDR (a length other than 13, a colour type / depth pair PNG does not have, compression or filter method not 0, interlace
 *      above 1), _INTERLACE (Adam7), _DEPTH16, _NO_IHDR (the first chunk is not IHDR), _NO_IDAT (none, or fewer than 2 bytes in all),
 *      _NO_PLTE (type 3 without PLTE before the first IDAT, or a PLTE whose length is not 3 ... 768 in threes), _ZERO_DIM,
 *      _TOO_LARGE (a dimension above 16384, raw_bytes above 2^30, zlen above 2^28), _ZLIB_METHOD (the stream's first byte: method
 *      not 8 or a window above 32 K), _ZLIB_DICT (FDICT set), _ZLIB_CHECK ((CMF 256 + FLG) mod 31 != 0).
 *   Gather.  The IDAT payloads of file f, in order, form its zlib stream of zlen bytes; the device copy is followed by zeros up to
 *      the stream capacity.  A byte a segment table places outside files_bytes reads 0.
 *   Inflate (RFC 1951).  Bits are taken from the least significant bit of each byte on; bits at and past 8 zlen read 0.  p is the
 *      number of bits taken.  The deflate data start at p = 16.  Per block: 1 bit BFINAL, 2 bits BTYPE.
 *      BTYPE 0: p moves up to a byte boundary; LEN, NLEN (16 bits each); NLEN != ~LEN: DSN_PNG_STORED_LEN; the LEN bytes that follow
 *      are output (fewer than LEN left in the stream: DSN_PNG_EARLY_END).  BTYPE 1: the fixed code lengths (8 x 144, 9 x 112, 7 x 24,
 *      8 x 8 for literal/length symbols 0 ... 287; 32 distance codes of length 5).  BTYPE 2: HLIT + 257, HDIST + 1, HCLEN + 4 (5, 5, 4 bits); more than 286
 *      literal/length or 30 distance codes: DSN_PNG_BAD_CODES; the code-length code's lengths in the order 16 17 18 0 8 7 9 6 10 5
 *      11 4 12 3 13 2 14 1 15; then the lengths: 0 ... 15 as they are, 16 repeats the previous one 3 + 2 bits times (none before
 *      it: BAD_CODES), 17 gives 3 + 3 bits zeros, 18 gives 11 + 7 bits zeros; a repeat past HLIT + HDIST + 258 or a zero length for
 *      symbol 256: BAD_CODES.  BTYPE 3: DSN_PNG_BLOCK_TYPE.
 *      A set of code lengths is USABLE when it is complete (sum over symbols of 2^-len == 1), or - for the literal/length and the
 *      distance code only - when it has no code at all or one single code of length 1 (zlib's rule).  Over-subscribed or otherwise
 *      incomplete: BAD_CODES.  Codes are canonical: per length in ascending symbol order, the first code of length l =
 *      (first code of length l - 1 + its count) << 1; a code's bits arrive most significant first.
 *      Symbols: < 256 a literal; 256 ends the block; 257 ... 285 a length (base 3, 4, ... 258 with 0 ... 5 extra bits) followed by a
 *      distance code 0 ... 29 (base 1 ... 24577 with 0 ... 13 extra bits).  A window that is no code, length symbols 286 / 287 and
 *      distance symbols 30 / 31: DSN_PNG_NO_CODE.  A distance above the bytes output so far: DSN_PNG_FAR_DISTANCE.  Byte i of a match
 *      of distance d that starts at output position s is out[s - d + (i mod d)]: an overlapping match repeats its d bytes.
 *      After every group of reads (block header; stored header; a literal/length symbol with its extra bits; a distance symbol with
 *      its extra bits; each code-length symbol with its extra bits) p > 8 zlen is DSN_PNG_EARLY_END, and it is looked at before
 *      anything else the group could raise - except a window that is no code at all, which takes no bits and is NO_CODE.  Output that would pass raw_bytes is DSN_PNG_TOO_MUCH; nothing of that literal, match
 *      or stored block is written.  The first error ends the decoding of the file: exactly one of these bits is set then, and
 *      neither Adler-32 nor the filters are looked at.
 *      Behind the final block p moves up to a byte boundary and the next four bytes, most significant first, are the stored
 *      Adler-32 (fewer than four left: EARLY_END); what follows them inside IDAT is ignored.  Fewer than raw_bytes bytes output:
 *      DSN_PNG_TOO_LITTLE.  The window size the zlib header names is not enforced (as zlib does not, unless built strict).
 *      Every loop is bounded: each step takes at least one bit or ends the file, p never passes 8 zlen + 64, reads are masked to
 *      the stream's capacity, writes to raw_bytes.
 *   Adler-32 of the bytes output (n of them, d_0 ... d_(n-1)): a = (1 + sum d_i) mod 65521, b = (n + sum (n - i) d_i) mod 65521,
 *      value b 2^16 + a; computed for every file whose inflate ended without one of the errors above (TOO_LITTLE included); not the
 *      stored one: DSN_PNG_ADLER.
 *   Unfilter (files without a status bit so far).  Row r of the inflated bytes is a filter byte and row_bytes bytes; bpp = max(1,
 *      bits channels / 8); a = the unfiltered byte bpp to the left, b = the one above, c = the one above a (0 outside the image).
 *      0: x; 1: x + a; 2: x + b; 3: x + ((a + b) >> 1); 4: x + (a, b or c, whichever is nearest to a + b - c, ties in that order),
 *      mod 256.  A filter byte above 4: DSN_PNG_FILTER (the row is taken as filter 0).
 *   Pixels.  Samples of 1, 2, 4 bits are packed most significant first, rows padded to a byte.  Grey g of `bits` bits becomes
 *      g 255 / (2^bits - 1) (x 255, 85, 17, 1); a palette index i becomes palette[i].  channels = DSN_PNG_BGR: uint8 [F, H, W, 3] in
 *      B, G, R order - what cv2.imread(path) is understood to return: grey replicated, palette looked up, alpha dropped (UNVERIFIED
 *      against OpenCV); DSN_PNG_RGB: R, G, B; DSN_PNG_NATIVE: [F, H, W, channels] with the file's own samples: grey (scaled), R G B,
 *      the palette INDEX, grey + alpha, R G B A.  first_channel != 0: [F, H, W], channel 0 of the above, never three channels.
 *      A file with any status bit gets all-zero pixels: every output byte is defined.
 *   Kernels.  k_pn_gather: a thread per stream byte, its segment by bisection.  k_pn_inflate: ONE WAVE PER FILE (a stream is
 *      serial: matches reach back into its own output), the symbol loop wave-uniform; the 32 KiB window, the canonical tables (counts,
 *      symbols in code order) and a 10-bit / 8-bit direct lookup for short codes in LDS, built by all lanes (ballots give each symbol
 *      its rank); a match is read by all lanes from the window - sources lie before the match's start -, then written to window and
 *      output, workgroup barriers between.  k_pn_adler: a workgroup per file, 16 bytes per load, integer sums.  k_pn_unfilter: a wave
 *      per file, lane j on row r + j one pixel behind lane j - 1, the row above and its left neighbour arriving by wave shuffles.
 *      k_pn_pixels: a thread per pixel.  Decoding inside one stream in parallel (speculating on block boundaries) is not done.
 * files: uint8 [files_bytes], the files one behind the other; segs: int64 [S, 3] = {offset in `files`, position in its file's zlib
 * stream, length} for every IDAT segment, file after file (S = n_segs); seg_first: int32 [F + 1], file f's segments are [seg_first[f],
 * seg_first[f + 1]); desc: dsn_png_desc [F] in DEVICE memory.  All files of a call share W, H, bits and ctype; palettes and
 * streams differ.  max_stream_bytes >= every zlen; it sizes the workspace.  stages: DSN_PNG_STAGE_* bits, DSN_PNG_STAGE_ALL for a
 * decode; a later stage alone runs on what the earlier ones left in the workspace (timing, tests).  out: see Pixels; out_status
 * uint32 [F].  workspace: dsn_png_workspace_bytes(...) bytes (0 for sizes outside the scope), 256-byte aligned, anything on entry.
 * dsn_png_workspace_layout: byte offsets {meta, streams, stream stride, raw, raw stride, rows, rows stride, total} of a workspace;
 * meta is uint32 [F, 8] = {bytes output, status, stored Adler, computed Adler, p at the end, 0, 0, 0}; raw holds the inflated
 * bytes, rows the unfiltered rows [H, row_bytes].  No allocation, no host copy, no synchronisation.
 * dsn_png_parse_host: HOST memory in and out; returns 0 and the DSN_PNG_* parse status through *status. */
#define DSN_PNG_EARLY_END 1u
#define DSN_PNG_BLOCK_TYPE 2u
#define DSN_PNG_STORED_LEN 4u
#define DSN_PNG_BAD_CODES 8u
#define DSN_PNG_NO_CODE 16u
#define DSN_PNG_FAR_DISTANCE 32u
#define DSN_PNG_TOO_MUCH 64u
#define DSN_PNG_TOO_LITTLE 128u
#define DSN_PNG_FILTER 256u
#define DSN_PNG_ADLER 512u
#define DSN_PNG_MAX_FILES 16384
#define DSN_PNG_MAX_DIM 16384
#define DSN_PNG_BGR 0
#define DSN_PNG_RGB 1
#define DSN_PNG_NATIVE 2
#define DSN_PNG_STAGE_GATHER 1
#define DSN_PNG_STAGE_INFLATE 2
#define DSN_PNG_STAGE_ADLER 4
#define DSN_PNG_STAGE_UNFILTER 8
#define DSN_PNG_STAGE_PIXELS 16
#define DSN_PNG_STAGE_ALL 31
#define DSN_PNG_OK 0              /* dsn_png_parse_host's status */
#define DSN_PNG_NOT_PNG 1
#define DSN_PNG_TRUNCATED 2
#define DSN_PNG_CRC 3
#define DSN_PNG_BAD_IHDR 4
#define DSN_PNG_INTERLACE 5
#define DSN_PNG_DEPTH16 6
#define DSN_PNG_NO_IHDR 7
#define DSN_PNG_NO_IDAT 8
#define DSN_PNG_NO_PLTE 9
#define DSN_PNG_ZERO_DIM 10
#define DSN_PNG_TOO_LARGE 11
#define DSN_PNG_ZLIB_METHOD 12
#define DSN_PNG_ZLIB_DICT 13
#define DSN_PNG_ZLIB_CHECK 14
typedef struct dsn_png_desc {
    int32_t W, H, bits, ctype;
    int32_t channels, row_bytes, raw_bytes, npal;
    int32_t nseg, zlen, file_length, reserved[5];
    uint8_t palette[256][3];
} dsn_png_desc;
DSN_EXPORT int dsn_png_parse_host(const uint8_t* file_host, size_t bytes, dsn_png_desc* desc_host, uint32_t* segs_host, size_t seg_capacity,
                                  int* status);
DSN_EXPORT size_t dsn_png_workspace_bytes(int F, int W, int H, int bits, int ctype, size_t max_stream_bytes);
DSN_EXPORT int dsn_png_workspace_layout(int F, int W, int H, int bits, int ctype, size_t max_stream_bytes, size_t* out8_host);
DSN_EXPORT int dsn_png_decode(const uint8_t* files, size_t files_bytes, const int64_t* segs, int n_segs, const int32_t* seg_first,
                              const dsn_png_desc* desc, int F, int W, int H, int bits, int ctype, size_t max_stream_bytes, int channels,
                              int first_channel, int stages, uint8_t* out, uint32_t* out_status, void* workspace, size_t workspace_bytes,
                              void* stream);

/* ---- PNG ENCODING on the device (csrc/dsn_pnge.hip): test.py's five cv2.imwrite(....png) per evaluated frame (test.py:94-110: the
 * rendering, the ground truth, the two side by side, depth and acc maps repeated to three channels) from frames that are in HBM
 * already; the finished files are left in device memory.  The rule below is restated in tests/png_encode_restate.py; PNG is
 * lossless, so every decoder returns the levels.  cv2.imwrite's own bytes are not claimed (OpenCV is not installed where the tests
 * run).  Integer arithmetic and integer atomics only: the same bytes on every call, and a frame gives the same file alone or in any batch.
 *   Levels.  The JPEG encoder's rule (one shared definition, csrc/dsn_level.h): uint8 passes through; float32 v: v * scale in
 *      float32, nearest-even, saturated to [0, 255], NaN -> 0; a NaN or infinite value sets DSN_PNGE_NONFINITE for its frame, the file
 *      is still valid.  mode DSN_PNGE_COLOUR: images [F, H, W, 3] in B, G, R order (rgb != 0: R, G, B); the file stores R, G, B with
 *      colour type 2.  DSN_PNGE_GRAY: images [F, H, W], colour type 0.  DSN_PNGE_REPLICATE: images [F, H, W], colour type 2 with three
 *      equal channels that are never materialised (test.py's np.repeat(..., 3, axis=2)).  8 bits, no interlace.
 *   Filtering.  bpp = channels of the file, row_bytes = W bpp.  For byte x of a row: a = the byte bpp to the left, b = the one above,
 *      c = the one above a (0 outside the image); the filtered byte is x - {0, a, b, (a + b) >> 1, Paeth(a, b, c)} mod 256 for filters
 *      0 ... 4, Paeth = whichever of a, b, c is nearest to a + b - c, ties in that order.  filter = DSN_PNGE_ADAPTIVE: per row the filter
 *      with the smallest sum over the row of |filtered byte read as int8| (v < 128 ? v : 256 - v; libpng's heuristic), ties to the
 *      lower filter number; filter = 0 ... 4: that filter on every row.  The raw stream is H rows of the filter byte and row_bytes bytes.
 *   Adler-32 of the raw stream, as in the decoder's rule.
 *   Deflate in independent chunks.  The raw stream is cut into chunks of C bytes (chunk: a power of two, DSN_PNGE_CHUNK_MIN ...
 *      DSN_PNGE_CHUNK_MAX); nothing in a chunk refers to bytes before it.
 *      Matches.  At position p the candidate distances are {1, bpp, row_stride} (row_stride = 1 + row_bytes), duplicates and
 *      distances above 32768 dropped, and those with p - distance before the chunk start.  A candidate's length is the common prefix of
 *      the bytes at p and at p - distance, capped at 258 and at the chunk end.  The best candidate is the longest, ties to the smaller
 *      distance.  A best length below 3, or of 3 at a distance above 4096, makes p a literal.
 *      Parse.  Serial greedy from the chunk start: at a match emit (length, distance) and move on by the length, else emit the
 *      literal and move on by one.
 *      Histograms.  Literal/length symbols 0 ... 285 (lengths: RFC 1951's 29 codes with their extra bits) and distance symbols
 *      0 ... 29; symbol 256 counts once.
 *      Code lengths (limit 15; 7 for the code-length code).  If fewer than two symbols of an alphabet have a count, the lowest symbols
 *      without one get a count of 1 until two have (zlib's practice; every code is then complete).  The used symbols are sorted by
 *      (count, symbol).  Two-queue Huffman merging: the two smallest of the leaves' queue (sorted) and the internal nodes' queue (in
 *      order of creation) are merged, a leaf before an internal node of equal weight, an older internal node before a newer one.
 *      bl[l] = leaves of depth l, the deeper ones folded into bl[limit]; while sum bl[l] 2^(limit - l) exceeds 2^limit: bl[limit] -= 1,
 *      l = the deepest length below the limit with bl[l] > 0, bl[l] -= 1, bl[l + 1] += 2 (each turn lowers the sum by 1, so it ends at
 *      2^limit exactly).  Lengths are then handed out in sorted order, the rarest symbols the longest: bl[limit] symbols get `limit`,
 *      the next bl[limit - 1] get limit - 1, ...  (always, not only after a repair: symbols of equal count may swap depths against the
 *      tree, at the same cost).  Canonical codes as in RFC 1951 3.2.2.
 *      Header of a dynamic block.  HLIT = 257 + (index of the last used length code) at least 257, HDIST at least 1, trailing zero
 *      lengths dropped.  The literal/length lengths and the distance lengths are run-length coded SEPARATELY (no run crosses from one
 *      into the other), greedily: a run of r zeros: while r >= 11 one symbol 18 for min(r, 138); then r >= 3: one symbol 17; what is
 *      left (< 3) as explicit zeros.  A run of r equal non-zero lengths: the length itself once, then while r >= 3 one symbol 16 for
 *      min(r, 6), what is left (< 3) explicitly.  The code-length code comes from these symbols' counts; HCLEN drops trailing zeros in
 *      the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, at least 4.
 *      Block type.  Bits of the chunk as a stored block (8 + 32 + 8 bytes: a chunk starts on a byte boundary), with the fixed codes
 *      (3 + tokens + end of block) and with the dynamic ones (3 + header + tokens + end of block); the smallest wins, ties in that
 *      order.  stored_only != 0: every chunk is a stored block ([IMWRITE_PNG_COMPRESSION, 0]).
 *      Chunk end.  Every chunk but the last is followed by an empty stored block: 000, zero bits to the byte boundary, 00 00 FF FF;
 *      every chunk therefore occupies whole bytes.  Only the last chunk's block has BFINAL = 1; zero bits pad it to a byte.
 *   Container.  Signature; IHDR (W, H, 8, colour type 0 or 2, 0, 0, 0); ONE IDAT of 78 01, the chunks and the Adler-32 most significant
 *      byte first; IEND.  Every chunk's CRC-32 is computed on the device (IHDR's, the same for all frames, travels in the kernel
 *      arguments): table CRCs of 16-byte slices without conditioning, each moved to the end of the data by a multiplication with
 *      x^(8 n) mod the polynomial and XOR-ed together, the conditioning added as one more such term.  The file is 63 bytes + the
 *      deflate stream.
 *   Kernels.  k_pe_filter: a workgroup per row, integer sums.  k_pe_adler: sums mod 65521 per 64 KiB, integer adds per frame.
 *      k_pe_match: a thread per raw byte.  k_pe_codes: ONE WAVE PER CHUNK: the greedy parse 64 positions per turn with the next
 *      token's position as a wave-uniform carry (exactly the serial result), histograms by LDS atomics, the symbols' ranks by all
 *      lanes, the tree, the repair, the header and the costs by lane 0 out of LDS.  k_pe_emit: a workgroup per chunk: bit lengths,
 *      workgroup prefix sums, 32-bit atomic ORs into the chunk's cleared slot.  The project's tile scan turns the chunks' byte lengths
 *      into offsets; k_pe_compact moves the slots together; k_pe_cont_copy / _tail finish the file.
 *   Bounds.  dsn_png_encode_max_bytes = 63 + raw bytes + 10 per chunk - 5: every chunk stored.  `capacity` is the stride of `out` in
 *      bytes; a frame that needs more sets DSN_PNGE_OVERFLOW for that frame alone: nothing is written at or past the capacity,
 *      out_lengths still holds the needed length.  W, H <= 16384, F <= 16384.
 *   Not done: 16-bit, alpha, palette and Adam7 output; hash-chain matches and lazy matching; joining chunks at bit level without the
 *      empty stored block.
 * images: contiguous, dtype DSN_JPEG_U8 or DSN_JPEG_F32.  channels (of the file): 1 or 3.  out: uint8 [F, capacity], bytes past a frame's
 * length are not touched; out_lengths int32 [F]; out_status uint32 [F] (OR of DSN_PNGE_*).  dsn_png_filter: raw uint8 [F, H (1 + row_bytes)],
 * out_status (NONFINITE).  dsn_png_deflate: raw uint8 [F, n] (ANY bytes; bpp and row_stride only name the candidate distances) -> the
 * deflate stream without zlib header and Adler-32 in out [F, capacity], out_lengths, out_status (OVERFLOW); dsn_png_deflate_max_bytes(n,
 * chunk) never overflows.  dsn_huff_lengths: counts uint32 [B, n] (2 <= n <= 288, n <= 2^limit, limit 1 ... 15) -> lengths
 * uint8 [B, n].  dsn_png_adler: raw [F, n] -> out_adler uint32 [F]; workspace 8 F bytes.  dsn_png_container: stream
 * uint8 [F, stream_stride] with lengths int32 [F] (bytes past the stride are not read), adler uint32 [F], status_in uint32 [F] or null ->
 * the files; workspace 4 F bytes.  dsn_png_encode is filter, adler, deflate and container one after the other, bit for bit.
 * Workspaces: dsn_png_*_workspace_bytes (0 for sizes outside the scope), 256-byte aligned (dsn_png_adler / _container: 4-byte), anything on
 * entry.  No allocation, no host copy, no synchronisation. */
#define DSN_PNGE_GRAY 0
#define DSN_PNGE_COLOUR 1
#define DSN_PNGE_REPLICATE 2
#define DSN_PNGE_ADAPTIVE 5
#define DSN_PNGE_NONFINITE 1u
#define DSN_PNGE_OVERFLOW 2u
#define DSN_PNGE_CHUNK_MIN 256
#define DSN_PNGE_CHUNK_MAX 32768
#define DSN_PNGE_CHUNK_DEFAULT 32768
DSN_EXPORT size_t dsn_png_encode_max_bytes(int W, int H, int channels, int chunk);
DSN_EXPORT size_t dsn_png_encode_workspace_bytes(int F, int W, int H, int mode, int chunk);
DSN_EXPORT size_t dsn_png_deflate_max_bytes(size_t n, int chunk);
DSN_EXPORT size_t dsn_png_deflate_workspace_bytes(int F, size_t n, int chunk);
DSN_EXPORT int dsn_png_filter(const void* images, int dtype, int F, int H, int W, int mode, int rgb, float scale, int filter, uint8_t* raw,
                              uint32_t* out_status, void* stream);
DSN_EXPORT int dsn_png_adler(const uint8_t* raw, int F, size_t n, uint32_t* out_adler, void* workspace, size_t workspace_bytes, void* stream);
DSN_EXPORT int dsn_png_deflate(const uint8_t* raw, int F, size_t n, int bpp, int row_stride, int chunk, int stored_only, uint8_t* out,
                               size_t capacity, int32_t* out_lengths, uint32_t* out_status, void* workspace, size_t workspace_bytes,
                               void* stream);
DSN_EXPORT int dsn_huff_lengths(const uint32_t* counts, int B, int n, int limit, uint8_t* lengths, void* stream);
DSN_EXPORT int dsn_png_container(const uint8_t* stream_bytes, size_t stream_stride, const int32_t* stream_lengths, const uint32_t* adler,
                                 const uint32_t* status_in, int F, int W, int H, int channels, uint8_t* out, size_t capacity,
                                 int32_t* out_lengths, uint32_t* out_status, void* workspace, size_t workspace_bytes, void* stream);
DSN_EXPORT int dsn_png_encode(const void* images, int dtype, int F, int H, int W, int mode, int rgb, float scale, int filter, int chunk,
                              int stored_only, uint8_t* out, size_t capacity, int32_t* out_lengths, uint32_t* out_status, void* workspace,
                              size_t workspace_bytes, void* stream);

/* diagnostics, NOT for the hot path (synchronises `stream`): {ncell, ok, total entries, capacity} of the four
 * nearest-face list levels (world fine/coarse, canonical fine/coarse) into a HOST array of 16 int32. */
DSN_EXPORT int dsn_debug_nn_stats(const void* scene, int V, int F, int32_t* out16_host, void* stream);

/* byte offsets of the four 64-byte level headers inside a scene blob, in the order of dsn_debug_nn_stats (host function, no device
 * work).  Header layout (int32 words): [8] cells, [9] ok (1 = the level is in use; 0 = not built, or its lists did not fit the
 * capacity - queries then fall through to the next level / the exhaustive sweep: SAME index, 10-50x slower), [10] list entries
 * the level needs, [11] capacity.  The host mirror copies the posed mesh's headers out asynchronously every few frames and warns
 * when entries > capacity (a mesh whose tessellation the fixed capacities - 2000 F entries per level - do not cover). */
DSN_EXPORT int dsn_nn_header_offsets(int V, int F, size_t* out4_host);

/* diagnostics: after a DSN_SKIP_TRANSPARENT render, int32 word 0 of `workspace` holds the number of non-transparent
 * samples, word 32 the number the density screen sent to the accurate pass (field forward evaluated) and word 16 the number
 * of those with sigma > 0 (d sigma/dx, normal and lighting evaluated); after dsn_render_rays_train word 48 holds the number of
 * samples whose activations left the fp16 range (train mode has no exact fallback: must be 0) - device memory. */
#ifdef __cplusplus
}
#endif
#endif /* DSNERF_H */
