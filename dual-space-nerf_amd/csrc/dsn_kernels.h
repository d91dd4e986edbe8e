// dsn_kernels.h - host-side launcher prototypes shared by the .hip translation units and dsn_api.hip
#pragma once
#include "dsn_common.h"

// persistent-workgroup kernels launch one workgroup per compute unit (DSN_PERSISTENT_GROUPS overrides the count: experiments)
#include <algorithm>
#include <cstdlib>
// (DSN_SHARE_CUS: dsn_render_rays sets the number of persistent workgroups for the launches of ITS call on ITS thread)
extern thread_local int g_dsn_persistent_override;
inline int dsn_cu_count_raw();
inline int dsn_cu_count() { return g_dsn_persistent_override > 0 ? g_dsn_persistent_override : dsn_cu_count_raw(); }
inline int dsn_cu_count_raw() {
    static const int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        const char* e = getenv("DSN_PERSISTENT_GROUPS");
        if (e && atoi(e) > 0) v = atoi(e);
        return v;
    }();
    return n;
}

void dsn_launch_face_setup(const float* verts, const int32_t* faces, int F, DsnFaceRec* recs, float4* cent,
                           hipStream_t st);
void dsn_launch_pose_setup(const float* packed, const float* poses, int frame_idx, int zero_code,
                           const float* light_shift, const float* rot, const float* rot_center, DsnFrameState* fs,
                           hipStream_t st, const float* pose_feat16 = nullptr);
void dsn_launch_sample_gg(const float* xyz, int V, const float* ray_o, const float* ray_d, float* near, float* far,
                          int R, int S, const float* t_vals, const float* jitter, float* z_vals, float* pts,
                          hipStream_t st, const DsnGrid* cls_grid = nullptr, int32_t* cls_cell_of = nullptr,
                          int32_t* cls_counts = nullptr, int32_t* cls_outside = nullptr, int32_t* cls_rank_of = nullptr);
// scratch of the cell-major search that the sampler fills when it classifies on the way (cleared here): per-cell counters and
// the counter of samples outside the fine grid
void dsn_nn_cellmajor_begin(void* small, int32_t** counts, int32_t** outside, hipStream_t st);
void dsn_launch_warp(const DsnSceneView& s, const float* pts, const float* ray_o, const float* ray_d,
                     const float* z_vals, int64_t N, int S, int32_t* face_idx, float* uv, float* h,
                     uint8_t* transparent, float* x_c, float* ray_d_can, int32_t* active_list, int32_t* active_count,
                     bool exhaustive, hipStream_t st, const int32_t* nn_pre = nullptr, bool lazy_canon = false,
                     const int32_t* only_cell_of = nullptr, const int32_t* only_count = nullptr);
// dsn_nn.hip: cell-major exact search of the fine lists (nn [N]: index, or -1 where the fine grid does not cover)
size_t dsn_nn_sort_scratch_size(int64_t N);
// nn [N] <- exact nearest centroid for the (live) points outside the fine grid and inside the coarse one, -1 for all others
void dsn_launch_nn_cellmajor_coarse(const DsnNNView& v, const float4* cent, const float* pts, const uint8_t* live, int64_t N,
                                    int32_t* cell_of, void* sorted, int32_t* nn, void* small, hipStream_t st, void* keys8N = nullptr, int F = 0,
                                    int32_t* wave_scratch = nullptr, int64_t wave_scratch_ints = 0);
void dsn_launch_nn_cellmajor(const DsnNNView& v, const float* pts, const float* ray_o, const float* ray_d, const float* z_vals,
                             int64_t N, int S, int32_t* cell_of, void* sorted, int32_t* nn, void* small, hipStream_t st);
// the same search with the rest of the warp stage fused behind it (transparent, x_c, active list written by the search kernel);
// *outside <- device counter of the samples left alone (cell_of < 0): dsn_launch_warp(..., only_cell_of, only_count) takes those
void dsn_launch_nn_cellmajor_warp(const DsnNNView& v, const float* ray_o, const float* ray_d, const float* z_vals, int64_t N, int S,
                                  int32_t* cell_of, void* sorted, void* small, const DsnFaceRec* face_world, const DsnFaceRec* face_canon,
                                  uint8_t* transparent, float* x_c, int32_t* active_list, int32_t* active_count, bool lazy_canon,
                                  int32_t** outside, hipStream_t st, bool classified = false, bool lazy_call = false,
                                  bool clear_cells = false);
void dsn_launch_lbs_warp(const DsnSceneView& s, const float* pts, int64_t N, const float* smpl_w, const float* A, int bw_type,
                         int32_t* face_idx, float* weights, uint8_t* transparent, float* pts_zero, bool exhaustive, hipStream_t st);
void dsn_launch_normal(const DsnSceneView& s, const float* x_c, const float* grad, int64_t N,
                       const int32_t* active_list, const int32_t* active_count, int32_t* face_idx_canon, float* n_w,
                       bool exhaustive, hipStream_t st, const int32_t* nn_far = nullptr);
// dsn_nn.hip
void dsn_launch_build_nn(const float4* cent, int F, const DsnNNView& nn, float pad_fine, float pad_coarse, hipStream_t st,
                         bool fine_only = false, bool dense_fine = false, bool lazy = false);
// the lists of a lazy fine level for the cells with visited[cell] > 0 (no-op on a level that holds every cell's lists)
void dsn_launch_build_nn_visited(const float4* cent, int F, const DsnNNView& nn, const int32_t* visited, hipStream_t st,
                                 const DsnFaceRec* face_world = nullptr, bool clear_cells = false);
bool dsn_clear_cells_on(bool lazy_call, bool lazy_canon);      // the clear-cell flags of a lazily built level: written and read by this call?
// a lazily set fine level completed for every cell - decided on the device: no-op sweeps once the level is complete
void dsn_launch_build_nn_complete(const float4* cent, int F, const DsnNNView& nn, hipStream_t st);
void dsn_launch_composite(const float* colour, const float* sigma, const uint8_t* transparent, const float* z_vals,
                          const float* ray_d, const float* noise, int R, int S, float* rgb_map, float* disp_map,
                          float* acc_map, float* weights, float* depth_map, hipStream_t st, bool lazy_colour = false,
                          int32_t* colour_max = nullptr);
void dsn_launch_field16_fwd(const float* packed, const DsnFrameState* fs, const float* x_c, int64_t N,
                            const int32_t* active_list, const int32_t* active_count, float* sigma, float* essence,
                            void* masks, int32_t* pos_list, int32_t* pos_count, hipStream_t st, int64_t rec_cap,
                            int32_t* flag_count = nullptr);
// density only: k_field16's forward trunk and density head (sigma bit-identical to dsn_launch_field16_fwd's where that does not flag)
void dsn_launch_field16_den(const float* packed, const DsnFrameState* fs, const float* x_c, int64_t N,
                            const int32_t* active_list, const int32_t* active_count, float* sigma, hipStream_t st,
                            int32_t* flag_count = nullptr);
void dsn_launch_field16_from(const float* packed, const DsnFrameState* fs, const float* x_c, int64_t N, const int32_t* list,
                             const int32_t* count, int64_t slot_base, float* sigma, float* essence, float* grad, hipStream_t st,
                             int32_t* flag_count = nullptr);
void dsn_launch_field16_bwd(const float* packed, const DsnFrameState* fs, const float* x_c, int64_t N,
                            const int32_t* pos_list, const int32_t* pos_count, float* grad, const void* masks,
                            hipStream_t st, float* sigma, int64_t rec_cap, const int32_t* sel = nullptr,
                            const int32_t* sel_count = nullptr, int32_t* flag_count = nullptr);
void dsn_launch_screen16(const float* packed, const DsnFrameState* fs, const float* x_c, int64_t N, const int32_t* active_list,
                         const int32_t* active_count, float* sigma, int32_t* keep_list, int32_t* keep_count, float* dbg_sigma,
                         float* dbg_s1, hipStream_t st, int32_t* audit_list = nullptr, int32_t* audit_count = nullptr,
                         int audit_cap = 0);
void dsn_launch_screen_audit(const int32_t* audit_list, const int32_t* audit_count, int audit_cap, const float* sigma, int32_t* out,
                             hipStream_t st);
size_t dsn_calibrate_workspace_size(int64_t n);
void dsn_launch_calibrate_screen(const DsnSceneView& s, float* packed, int64_t n, void* workspace, float* out4, hipStream_t st,
                                 const float* frame_x_c = nullptr, const int32_t* frame_list = nullptr,
                                 const int32_t* frame_count = nullptr);
void dsn_launch_set_screen_margin(float* packed, float margin, hipStream_t st);
void dsn_launch_set_packed_scalar(float* packed, int word, float v, hipStream_t st);      // packed[OFF_SCAL + word] = v
void dsn_launch_light16(const float* packed, const DsnFrameState* fs, const float* n_w, const float* x_w,
                        const float* ray_o, const float* ray_d, const float* z_vals, const float* essence, int64_t N,
                        int S, const int32_t* active_list, const int32_t* active_count, float* colour, hipStream_t st,
                        float* tr_hl1 = nullptr, float* tr_hl2 = nullptr, float* tr_pre = nullptr, int32_t* range_count = nullptr,
                        float* factor = nullptr);      // factor [N] (dsn_shade_factor): the light factor ELU + 1 beside the colour
// relighting sweep (dsn_render_rays_lights): lighting MLP of G light records per pass over the shading list -> colours [G][count][3]
// by list slot; the list's slot of every sample (-1 elsewhere: the caller clears `slot`); the compositor of G lights through that map
void dsn_launch_light16_multi(const float* packed, const DsnLightEdit* lights, int G, const float* n_w, const float* ray_o, const float* ray_d,
                              const float* z_vals, const float* essence, int64_t max_count, int S, const int32_t* list,
                              const int32_t* list_count, float* colours, hipStream_t st,
                              float* factors = nullptr);      // factors [G][count] (dsn_render_rays_maps): ELU + 1 by list slot
void dsn_launch_slot_map(const int32_t* list, const int32_t* count, int64_t max_count, int32_t* slot, hipStream_t st);
bool dsn_composite_multi_supported(int S, const void* z_vals, const void* sigma, const void* weights, const void* slot_of,
                                   const void* transparent);
void dsn_launch_composite_multi(const int32_t* slot_of, const float* colours, int64_t n_shaded, int G, const float* sigma,
                                const uint8_t* transparent, const float* z_vals, const float* ray_d, int R, int S, float* rgb_maps,
                                float* disp_map, float* acc_map, float* weights, float* depth_map, int32_t* colour_max, hipStream_t st);
// decomposition maps (dsn_render_rays_maps, dsn_composite_maps): the compositor's weights over the essence, the world normal and the
// light factors of G lights.  slot_of == NULL: `factors` / `colours` are dense ([G][N], [G][N][3]) and every sample with sigma > 0
// counts as listed.  Every output pointer may be NULL; maps_max (2 words, float bits, cleared by the caller): largest |essence| and
// largest factor weighed.  Any S (one wave per ray where S is not 64 / 128 or an array is not 16-byte aligned).
struct DsnMapsArgs {
    const int32_t* slot_of; const float* colours; const float* factors; int64_t n_shaded; int G;
    const float* essence; const float* n_w; const float* sigma; const uint8_t* transparent; const float* z_vals; const float* ray_d;
    int R, S;
    float *rgb_maps, *albedo_map, *normal_map, *shading_maps, *disp_map, *acc_map, *weights, *depth_map;
    int32_t *colour_max, *maps_max;
};
void dsn_launch_composite_maps(const DsnMapsArgs& a, hipStream_t st);
void dsn_launch_camera_rays(const double* K, const double* R, const double* T, const double* bounds, int H, int W,
                            float* ray_o, float* ray_d, float* near, float* far, uint8_t* mask, hipStream_t st, int h36m = 0);
// dsn_sample.hip: a training batch drawn on the device (dsn_train_rays / dsn_bound_mask, the rule of include/dsnerf.h)
struct DsnTrainRaysArgs {
    const double *K, *R, *T, *bounds;
    int H, W, convention, nrays;
    uint32_t seed;
    const double* img64; const float* img32;
    const uint8_t *mask_a, *mask_b, *bound_in, *occ_src;
    float *ray_o, *ray_d, *near, *far, *rgb;
    int64_t* coord;
    uint8_t *occupancy, *mask_at_box, *bound_out;
    int32_t *status, *rounds;
    void* workspace;
};
size_t dsn_train_rays_workspace_size(int64_t hw, int nrays);
void dsn_launch_bound_mask(const double* K, const double* R, const double* T, const double* bounds, int H, int W, uint8_t* mask_out,
                           hipStream_t st);
void dsn_launch_train_rays(const DsnTrainRaysArgs& a, hipStream_t st);
// dsn_field.hip
void dsn_pack_params_host(const float* const* params33_host, float* packed_host);
void dsn_launch_pack_params(const float* const* params33_dev_array, float* packed, hipStream_t st);
void dsn_launch_field(const float* packed, const DsnFrameState* fs, const float* x_c, int64_t N,
                      const int32_t* active_list, const int32_t* active_count, float* sigma, float* essence,
                      float* grad, hipStream_t st);
// exact-fp32 re-evaluation of the listed samples whose sigma is NaN (range fallback of the split-fp16 kernels); flag_count
// (optional): what the split-fp16 launches counted while flagging - zero: the kernel leaves without looking
void dsn_launch_field_fix(const float* packed, const DsnFrameState* fs, const float* x_c, int64_t N,
                          const int32_t* active_list, const int32_t* active_count, float* sigma, float* essence,
                          float* grad, hipStream_t st, const int32_t* flag_count = nullptr);
void dsn_launch_field16(const float* packed, const DsnFrameState* fs, const float* x_c, int64_t N,
                        const int32_t* active_list, const int32_t* active_count, float* sigma, float* essence,
                        float* grad, hipStream_t st, int32_t* flag_count = nullptr);
void dsn_launch_light(const float* packed, const DsnFrameState* fs, const float* n_w, const float* x_w,
                      const float* ray_o, const float* ray_d, const float* z_vals, const float* essence, int64_t N,
                      int S, const int32_t* active_list, const int32_t* active_count, float* colour, hipStream_t st);

// dsn_train.hip: parameter gradients of Renderer.render / DualSpaceNeRF.forward (fused split-fp16 passes + in-tree fp32 / split-fp16
// weight-gradient and small-GEMM kernels; no library calls)
size_t dsn_train_workspace_size(int64_t N);
// where that workspace keeps its per-row arrays (byte offsets in the order of DSN_GRAD_WS_*, dsnerf.h); 0, or the number of entries if n is not it
int dsn_train_workspace_layout(int64_t N, int64_t* out, int n);
// the part of that workspace a training FORWARD fills for its backward (dsn_render_rays_train -> dsn_render_rays_grad)
struct DsnTrainCache {
    uint8_t* transparent; int32_t* idx_c; float *x_c, *sigma, *essence, *grad, *n_w, *h0, *a0, *rr; void* masks;
    float *hl1, *hl2, *pre;        // lighting MLP: hidden layers after ReLU [N,128] and the output pre-activation [N]
    uint8_t* live; int32_t *list1, *bcnt, *rowcnt;      // rows the forward evaluates: flags, ascending list, build scratch, [0] = their number
};
// rows the training forward has to evaluate: all but transparent samples whose noise is <= 0 (alpha = 0 exactly) -> list, *count
void dsn_train_forward_rows(const uint8_t* transparent, const float* noise, int64_t N, uint8_t* flag, int32_t* bcnt, int32_t* list,
                            int32_t* count, hipStream_t st);
DsnTrainCache dsn_train_cache(void* workspace, int64_t N);
void dsn_launch_field16_train(const float* packed, const DsnFrameState* fs, const float* x_c, int64_t N, float* sigma,
                              float* essence, float* grad, float* tr_h, float* tr_a, float* tr_rr, void* masks, hipStream_t st,
                              int32_t* range_count = nullptr, const int32_t* row_list = nullptr, const int32_t* row_count = nullptr);
void dsn_launch_adjoint16(const float* packed, int64_t N, const void* masks, const float* a_in, float* tr_a, float* gmax,
                          hipStream_t st, int32_t* range_count = nullptr, const int32_t* row_list = nullptr,
                          const int32_t* row_count = nullptr);
void dsn_launch_tangent16(const float* packed, const float* x_c, const float* u, int64_t N, const void* masks, float* tr_t,
                          float* gmax, hipStream_t st, int32_t* range_count, const int32_t* row_list, const int32_t* row_count,
                          float* colsum6);
// a second stream of the caller's for the training backward's two independent chains (dsn_render_rays_grad_ex): fork / join events
struct DsnTrainAux { hipStream_t stream; hipEvent_t fork, join; };
const char* dsn_train_run(const DsnSceneView& s, const float* packed, const float* const* params33, const float* poses, int frame_idx,
                          int zero_code,
                          const float* ray_o, const float* ray_d, const float* z_vals, const float* noise, int R, int S,
                          const float* d_rgb, const float* d_disp, const float* d_acc, const float* d_depth,
                          const float* d_weights, float* const* grads33, void* workspace, hipStream_t st, bool cached = false,
                          const float* ext_x_c = nullptr, const float* ext_d_col = nullptr, const float* ext_d_sig = nullptr,
                          const DsnTrainAux* aux = nullptr);

// dsn_image.hip: image epilogue on the device (post_process scatter, clamp, mse / psnr, ssim)
size_t dsn_image_workspace_size(int H, int W);
void dsn_launch_image_scatter(const float* rgb, const float* disp, const float* acc, const float* depth, int R,
                              const uint8_t* mask, int H, int W, int clamp_rgb, float* img_rgb, float* img_disp,
                              float* img_acc, float* img_depth, void* workspace, hipStream_t st);
void dsn_launch_image_psnr(const float* img_rgb, const double* gt64, const float* gt32, const uint8_t* mask, int H, int W,
                           double* out4, void* workspace, hipStream_t st);
size_t dsn_image_ssim_workspace_size(int F, int H, int W);
void dsn_launch_image_ssim(const float* img_rgb, const double* gt64, const float* gt32, const uint8_t* mask, int F, int H, int W,
                           int clamp_rgb, double* out_ssim, int32_t* out_rect, int32_t* out_status, void* workspace, hipStream_t st);
// dsn_lpips.hip: test.py's LPIPS distances (dsn_lpips_*; arguments checked by the entry points; N images = 2 F for the distance)
size_t dsn_lpips_packed_size(int net);
size_t dsn_lpips_workspace_size(int net, int N, int H, int W);
int dsn_lpips_min_side(int net);
int dsn_launch_lpips_pack(int net, const float* const* conv_w, const float* const* conv_b, const float* const* lin_w, void* packed,
                          hipStream_t st);
void dsn_launch_lpips_features(const void* packed, int net, const float* stack, int N, int H, int W, int rgb_pm1, float* const* out_taps,
                               int32_t* status, void* workspace, hipStream_t st);
void dsn_launch_lpips(const void* packed, int net, const float* img, const double* gt64, const float* gt32, int F, int H, int W, int rgb_pm1,
                      double* out, double* out_layers, int32_t* status, void* workspace, hipStream_t st);
// dsn_loss.hip: the trainer's loss and its two seed arrays (dsn_train_loss / dsn_train_loss_grad)
size_t dsn_train_loss_workspace_size(int64_t R);
void dsn_launch_train_loss(const float* color, const float* t32, const double* t64, float* acc, const uint8_t* o8, const float* o32,
                           int64_t R, int kind, int overwrite, double* out4, void* workspace, hipStream_t st);
void dsn_launch_train_loss_grad(const float* color, const float* t32, const double* t64, const float* acc, const uint8_t* o8,
                                const float* o32, int64_t R, int kind, const float* up_rgb, const float* up_mask, float* g_color,
                                float* g_acc, hipStream_t st);
// dsn_optim.hip: the optimizer step (dsn_adam_step): out7 = {w1, w2, b2, eps, wd, ss, c2}; the launcher returns its launch count
void dsn_adam_scalars(double lr, double weight_decay, double beta1, double beta2, double eps, double t, float* out7);
int dsn_launch_adam_step(float* const* params, const float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                         const int64_t* n, int count, const double* lr, const double* weight_decay, double beta1, double beta2, double eps,
                         double t, hipStream_t st);
// dsn_rng.hip: the training step's jitter and noise (dsn_train_draws; R, S > 0, R * S <= INT_MAX, not both arrays null)
void dsn_launch_train_draws(uint64_t seed, uint32_t step, uint32_t ray_base, const int32_t* ray_ids, int R, int S, float noise_std,
                            float* jitter, float* noise, hipStream_t st);
// dsn_prep.hip: the datasets' image preparation (dsn_image_undistort / _morph / _resize / _prep; arguments checked by the entry points)
void dsn_launch_image_undistort(const void* src, void* dst, const double* K, const double* D, int nd, int N, int H, int W, int channels,
                                int dtype, hipStream_t st);
void dsn_launch_image_morph(const uint8_t* src, uint8_t* dst, int N, int H, int W, int k, int op, hipStream_t st);
void dsn_launch_image_resize(const void* src, void* dst, int N, int H, int W, int channels, int dtype, int c, int mode, hipStream_t st);
void dsn_launch_image_prep(const uint8_t* img, const uint8_t* msk_cihp, const double* K, const double* D, int nd, int N, int H0, int W0, int c,
                           int border, int out_dtype, void* out_img, uint8_t* out_img_u8, uint8_t* out_msk_fg, uint8_t* out_msk_cihp,
                           hipStream_t st);
// dsn_jpeg.hip: baseline JPEG (dsn_jpeg_*; arguments checked by the entry points).  The workspace holds the coefficients first when
// `with_coef` / `ws_has_coef` (dsn_jpeg_encode), so that dsn_jpeg_scan carves the same layout behind them.
size_t dsn_jpeg_header_bytes(int mode);
bool dsn_jpeg_blocks(int H, int W, int mode, int* blocks);
size_t dsn_jpeg_workspace_size(int F, int H, int W, int mode, bool with_coef);
int dsn_jpeg_write_header_host(int H, int W, int mode, int quality, uint8_t* out);
void dsn_launch_jpeg_coefficients(const void* images, int dtype, int F, int H, int W, int mode, int quality, int rgb, float scale,
                                  int16_t* coef, uint32_t* status, hipStream_t st);
void dsn_launch_jpeg_scan(const int16_t* coef, const uint32_t* status_in, int F, int H, int W, int mode, int quality, uint8_t* out,
                          size_t capacity, int32_t* lengths, uint32_t* status, void* workspace, bool ws_has_coef, hipStream_t st);
void dsn_launch_jpeg_encode(const void* images, int dtype, int F, int H, int W, int mode, int quality, int rgb, float scale, uint8_t* out,
                            size_t capacity, int32_t* lengths, uint32_t* status, void* workspace, hipStream_t st);
void dsn_launch_jpeg_tile_scan(int* x, int n, int F, int* tot, hipStream_t st);
struct dsn_jpegd_desc;
// dsn_jpegd.hip: baseline JPEG decoding (dsn_jpeg_parse_host, dsn_jpegd_*, dsn_jpeg_decode; arguments checked by the entry points)
int dsn_jpegd_parse_host(const uint8_t* file, size_t bytes, dsn_jpegd_desc* out);
size_t dsn_jpegd_workspace_size(int F, int H, int W, int mode, size_t max_scan_bytes);
int16_t* dsn_jpegd_workspace_coef(void* workspace, int F, int H, int W, int mode, size_t max_scan_bytes);
void dsn_launch_jpegd_sync(const uint8_t* files, size_t files_bytes, const int64_t* offsets, const dsn_jpegd_desc* desc, int F, int H, int W,
                           int mode, size_t max_scan_bytes, int B, bool restart, int rounds, uint32_t* out_converged, int32_t* out_rounds,
                           void* workspace, hipStream_t st);
void dsn_launch_jpegd_coefficients(const dsn_jpegd_desc* desc, int F, int H, int W, int mode, size_t max_scan_bytes, int B, int16_t* coef,
                                   uint32_t* status, void* workspace, hipStream_t st);
void dsn_launch_jpegd_pixels(const int16_t* coef, const uint32_t* status, const dsn_jpegd_desc* desc, int F, int H, int W, int mode,
                             size_t max_scan_bytes, int rgb, int gray_out, uint8_t* out, void* workspace, hipStream_t st);

struct dsn_png_desc;
// dsn_png.hip: PNG decoding (dsn_png_parse_host, dsn_png_workspace_*, dsn_png_decode; arguments checked by the entry points)
int dsn_png_parse(const uint8_t* file, size_t bytes, dsn_png_desc* out, uint32_t* segs, size_t seg_capacity);
size_t dsn_png_workspace_size(int F, int W, int H, int bits, int ctype, size_t max_stream_bytes, size_t* out8);
void dsn_launch_png_decode(const uint8_t* files, size_t files_bytes, const int64_t* segs, int S, const int32_t* seg_first,
                           const dsn_png_desc* desc, int F, int W, int H, int bits, int ctype, size_t max_stream_bytes, int channels,
                           int first_channel, int stages, uint8_t* out, uint32_t* out_status, void* workspace, hipStream_t st);
// dsn_pnge.hip: PNG encoding (dsn_png_filter / _adler / _deflate / _container / _encode, dsn_huff_lengths; arguments checked by the entry
// points; the size functions return 0 for sizes outside the scope)
size_t dsn_pnge_raw_bytes(int W, int H, int mode);
size_t dsn_pnge_deflate_max(size_t n, int chunk);
size_t dsn_pnge_deflate_workspace_size(int F, size_t n, int chunk);
size_t dsn_pnge_workspace_size(int F, int W, int H, int mode, int chunk);
void dsn_launch_png_filter(const void* images, int dtype, int F, int H, int W, int mode, int rgb, float scale, int filter, uint8_t* raw,
                           uint32_t* status, hipStream_t st);
void dsn_launch_png_adler(const uint8_t* raw, int F, size_t n, uint32_t* adler, uint32_t* sums2, hipStream_t st);
void dsn_launch_png_deflate(const uint8_t* raw, int F, size_t n, int bpp, int row_stride, int chunk, int stored_only, uint8_t* out,
                            size_t capacity, int32_t* lengths, uint32_t* status, void* workspace, hipStream_t st);
void dsn_launch_huff_lengths(const uint32_t* counts, int B, int n, int limit, uint8_t* lengths, hipStream_t st);
void dsn_launch_png_container(const uint8_t* zs, size_t zstride, const int32_t* zlen, const uint32_t* adler, const uint32_t* status_a,
                              const uint32_t* status_b, int F, int W, int H, int channels, uint8_t* out, size_t capacity, int32_t* lengths,
                              uint32_t* status, uint32_t* crc_words, hipStream_t st);
void dsn_launch_png_encode(const void* images, int dtype, int F, int H, int W, int mode, int rgb, float scale, int filter, int chunk,
                           int stored_only, uint8_t* out, size_t capacity, int32_t* lengths, uint32_t* status, void* workspace, hipStream_t st);

// dsn_mesh.hip: density grid points and marching cubes (dsn_density_grid, dsn_mc_*)
void dsn_launch_grid_points(const float* x, const float* y, const float* z, int i0, int ny, int nz, int64_t n, float* pts, hipStream_t st);
size_t dsn_mc_workspace_size(int64_t N);
void dsn_launch_mc_count(const float* vol, int nx, int ny, int nz, float level, void* workspace, int64_t* out_counts, hipStream_t st);
void dsn_launch_mc_emit(const float* vol, int nx, int ny, int nz, const float* x, const float* y, const float* z, float level, int ascent,
                        const void* workspace, float* verts, int64_t vcap, int32_t* faces, int64_t fcap, hipStream_t st);
void dsn_launch_mc_normals(const float* vol, int nx, int ny, int nz, const float* x, const float* y, const float* z, float level, int ascent,
                           const void* workspace, float* normals, int64_t vcap, hipStream_t st);
void dsn_mc_table_copy(int32_t* out_host);
// dsn_mesh.hip: the density grid coarse to fine (dsn_grid_hier_*, dsn_density_points; sh = log2 of the factor; the counters an entry
// point hands in are zero on entry)
size_t dsn_grid_hier_workspace_size(int nx, int ny, int nz, int sh);
void dsn_grid_hier_coarse_shape(int nx, int ny, int nz, int sh, int* m3);
void dsn_launch_grid_hier_mark(const float* coarse, int nx, int ny, int nz, int sh, int dilate, float level, void* workspace,
                               int64_t* out_counts, hipStream_t st);
void dsn_launch_grid_hier_list(int nx, int ny, int nz, int sh, const void* workspace, int32_t* index, int64_t cap, hipStream_t st);
void dsn_launch_grid_hier_assemble(const float* coarse, int nx, int ny, int nz, int sh, float level, const void* workspace,
                                   const int32_t* index, const float* values, int64_t M, float* volume, int64_t* out_leaks, hipStream_t st);
void dsn_launch_list_points(const float* x, const float* y, const float* z, const int32_t* index, int ny, int nz, int64_t N, int64_t n,
                            float* pts, hipStream_t st);
void dsn_launch_points_invalid(const int32_t* index, int64_t N, int64_t n, float* values, hipStream_t st);
// dsn_mesh.hip: connected components and the largest piece of an indexed mesh (dsn_mesh_cc_*; scale = 2^area_shift; phases: DSN_CC_*)
size_t dsn_mesh_cc_workspace_size(int64_t V, int64_t T);
void dsn_launch_mesh_cc_label(const float* verts, const int32_t* faces, int64_t V, int64_t T, double scale, void* workspace, int32_t* labels_v,
                              int64_t* out_counts, int phases, hipStream_t st);
void dsn_launch_mesh_cc_emit(const float* verts, const int32_t* faces, int64_t V, int64_t T, void* workspace, float* out_verts, int64_t vcap,
                             int32_t* out_faces, int64_t fcap, int32_t* source_vertex, int phases, hipStream_t st);
// dsn_mesh.hip: vertex clustering with a picked representative (dsn_mesh_simplify_*; g: the grid's three cell counts; phases: DSN_SP_*)
size_t dsn_mesh_simplify_workspace_size(int64_t V, int64_t T, const int* g);
void dsn_launch_mesh_simplify_count(const float* verts, const int32_t* faces, int64_t V, int64_t T, const float* origin, float cell, const int* g,
                                    void* workspace, int32_t* vertex_cluster, int64_t* out_counts, int phases, hipStream_t st);
void dsn_launch_mesh_simplify_cells(const float* verts, int64_t V, const float* origin, float cell, const int* g, void* workspace, int64_t* out_K,
                                    hipStream_t st);
void dsn_launch_mesh_simplify_emit(const float* verts, const int32_t* faces, int64_t V, int64_t T, const int* g, void* workspace, float* out_verts,
                                   int64_t vcap, int32_t* out_faces, int64_t fcap, int32_t* cluster_source, int phases, hipStream_t st);
// dsn_mesh.hip: umbrella smoothing and vertex normals from the faces (dsn_mesh_smooth / dsn_mesh_vertex_normals; phases: DSN_SM_*)
size_t dsn_mesh_smooth_workspace_size(int64_t V, int64_t T);
void dsn_launch_mesh_smooth(const float* verts, const int32_t* faces, int64_t V, int64_t T, const float* origin, int k, const float* factors,
                            int n_steps, void* workspace, float* out_verts, int64_t* out_counts, int phases, hipStream_t st);
void dsn_launch_mesh_vertex_normals(const float* verts, const int32_t* faces, int64_t V, int64_t T, double scale, void* workspace,
                                    float* out_normals, int phases, hipStream_t st);
// dsn_mesh.hip: a mesh bound to the body (dsn_mesh_bind_normals / dsn_mesh_pose / dsn_mesh_stretch; workspace: DsnFaceRec [P, Fb])
void dsn_launch_mesh_bind_normals(const float* body, int Vb, const int32_t* bfaces, int Fb, const int32_t* face_idx, const float* normals,
                                  int64_t N, float* cov, hipStream_t st);
void dsn_launch_mesh_pose(const float* target, int P, int Vb, const int32_t* bfaces, int Fb, const int32_t* face_idx, const float* uv,
                          const float* h, const float* cov, int64_t N, float* out_verts, float* out_normals, int32_t* status, void* workspace,
                          hipStream_t st);
void dsn_launch_mesh_stretch(const float* bind, const float* posed, int P, int64_t N, const int32_t* faces, int64_t T, float* stretch,
                             hipStream_t st);
// dsn_body.hip: the SMPL forward pass (dsn_body_shape / dsn_body_pose; parents24: host memory, entries 1..23 already checked)
size_t dsn_body_pose_workspace_size(int V, int P);
void dsn_launch_body_shape(const float* v_template, const float* shapedirs, const float* betas, int B, const float* J_regressor, int V,
                           float* v_shaped, float* joints, hipStream_t st);
void dsn_launch_body_pose(const float* v_shaped, const float* joints, const int* parents24, const float* weights, const float* posedirs, int V,
                          const float* poses, const float* Rh, const float* Th, int P, int pad_mode, float* xyz, float* xyz_smpl, float* A,
                          float* bounds, float* Rh_mat, void* workspace, hipStream_t st);
// dsn_raster.hip: the mesh preview (dsn_raster_mesh)
size_t dsn_raster_workspace_size(int64_t V, int64_t T, int H, int W);
void dsn_launch_raster_mesh(const float* verts, int64_t V, const int32_t* faces, int64_t T, const float* pose12, float fx, float fy,
                            float znear, const float* light4, int H, int W, int32_t* out_face, float* out_depth, uint8_t* out_color,
                            void* workspace, int phases, int big_pixels, hipStream_t st);
// (all four null and mode 0: dsn_launch_raster_mesh)
void dsn_launch_raster_mesh_attr(const float* verts, int64_t V, const int32_t* faces, int64_t T, const float* pose12, float fx, float fy,
                                 float znear, const float* light4, int H, int W, int32_t* out_face, float* out_depth, uint8_t* out_color,
                                 void* workspace, int phases, int big_pixels, const float* vertex_normals, const float* vertex_colors,
                                 int mode, float* out_normal, float* out_attr, hipStream_t st);
// dsn_meshdist.hip: the nearest point on a triangle mesh (dsn_mesh_dist_*) and area-weighted surface samples (dsn_mesh_sample_surface)
size_t dsn_mesh_dist_workspace_size(int64_t T);
void dsn_mesh_dist_grid_rule(int64_t T, const float* box6, int* g0, float* cell0);
void dsn_launch_mesh_dist_build(const float* verts, const int32_t* faces, int64_t V, int64_t T, const float* box6, void* workspace,
                                int64_t* out_counts4, hipStream_t st);
void dsn_launch_mesh_dist_query(const float* verts, const int32_t* faces, int64_t V, int64_t T, const void* workspace, const float* points,
                                int64_t n, float* out_d2, int32_t* out_face, float* out_point, hipStream_t st);
size_t dsn_mesh_dist_reduce_workspace_size(int64_t n);
void dsn_launch_mesh_dist_reduce(const float* d2, int64_t n, void* workspace, double* out6, hipStream_t st);
size_t dsn_mesh_sample_workspace_size(int64_t T);
void dsn_launch_mesh_sample_surface(const float* verts, const int32_t* faces, int64_t V, int64_t T, uint64_t seed, int64_t n, void* workspace,
                                    float* out_points, int32_t* out_face, hipStream_t st);
// front-to-back slices with exact ray termination (dsn_geom.hip; DSN_EARLY_STOP in dsn_render_rays)
#define DSN_STOP_MAX_SLICES 32
// bounds[0 .. K]: slice k = samples [bounds[k], bounds[k + 1]) of every ray; its list starts at lists + R * bounds[k]
void dsn_launch_slice_bucket(const int32_t* active, const int32_t* active_count, int64_t N, int S, int R, const int* bounds, int K,
                             int32_t* lists, int32_t* counts, hipStream_t st);
// slice k >= 1: advances the rays' transmittance over the slices their pair does not cover yet and keeps the samples of live rays
// (Tk: [R] x 8 bytes, dsn_launch_slice_T_init; packed_scal = packed + OFF_SCAL: the threshold's colour scale lives there)
void dsn_launch_slice_alive(const int32_t* list, const int32_t* count, int64_t N, int S, int L, int k, void* Tk, const float* sigma,
                            const uint8_t* transparent, const float* z_vals, const float* ray_d, const float* packed_scal, int32_t* out,
                            int32_t* out_count, int32_t* stopped, hipStream_t st, bool pairs_current = false);
// the per-ray form of the advance (one coalesced pass over slice k - 1 of every ray; dsn_launch_slice_alive(..., pairs_current = true) behind it)
void dsn_launch_advance_T(const float* sigma, const uint8_t* transparent, const float* z_vals, const float* ray_d, int R, int S, int s0,
                          int s1, int k, void* Tk, hipStream_t st);
void dsn_launch_slice_T_init(void* Tk, int R, hipStream_t st);
void dsn_launch_fill_f32(float* p, int64_t n, float v, hipStream_t st);
void dsn_launch_cull_lit(const int32_t* pos, const int32_t* pos_count, int64_t N, int64_t rec_cap, const float* weight,
                         const float* sigma, int S, const float* packed_scal, int32_t* sel, int32_t* sel_count, int32_t* lit, int32_t* lit_count,
                         int32_t* culled, float* colour, hipStream_t st);
void dsn_launch_stop_stats(const float* sigma, const uint8_t* transparent, const float* z_vals, const float* ray_d, int R, int S, int L,
                           const float* packed_scal, int32_t* out, hipStream_t st, int32_t* hist = nullptr, const int32_t* colour_max = nullptr,
                           int Lu = 0);      // (Lu: the uniform slice length *out counts by; 0 = L)
