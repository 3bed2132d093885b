/*
 * gsr.h — C ABI of the MI355X (gfx950) differentiable Gaussian-splatting
 * rasterizer (libgsr.so).
 *
 * This is the drop-in boundary for the reference's hot path
 *   gaussian_renderer.render() -> GaussianRasterizer -> _C.rasterize_gaussians{,_backward}
 * The three entry points replace, one for one, the reference's C++ ABI
 *   CudaRasterizer::Rasterizer::forward / backward / markVisible
 *   (submodules/diff-gaussian-rasterization/cuda_rasterizer/rasterizer.h:21-129)
 * which its pybind layer binds as _C.rasterize_gaussians, _C.rasterize_gaussians_backward
 * and _C.mark_visible (DGR/ext.cpp:15-23, DGR/rasterize_points.cu:39-277).
 *
 * Differences from the reference ABI, all mechanical:
 *   - std::function<char*(size_t)> resize callbacks become (gsr_alloc_fn, ctx)
 *     pairs; a callback returns device memory of at least the requested size,
 *     valid until the backward of the same call has run (the reference keeps it
 *     alive in torch uint8 tensors saved by autograd, DGR/__init__.py:114-133).
 *     A NULL return makes the call fail with GSR_ERR_ALLOC.
 *   - every call takes the hipStream_t to launch on (the reference uses the
 *     legacy default stream); the forward synchronises that stream once, to read
 *     the instance count K (as the reference's cudaMemcpy does,
 *     rasterizer_impl.cu:384);
 *   - bool -> int, and a status code is returned (0 = success); the instance
 *     count is written to *num_rendered;
 *   - gradient outputs are fully written by the backward (no pre-zeroing
 *     needed); forward image outputs are written for every pixel
 *     (mdepth/normal are written as 0 when require_depth == 0).
 * All pointers are DEVICE pointers to contiguous fp32 / int32 arrays with the
 * reference's layouts: means3D [P,3], opacities [P,1], scales [P,3],
 * rotations [P,4] (r,x,y,z), shs [P,SHM,3], sg_axis [P,SGM,3],
 * sg_sharpness [P,SGM], sg_color [P,SGM,3], colors_precomp [P,3],
 * cov3D_precomp [P,6], viewmatrix/projmatrix [16] column-major, campos [3],
 * background [3]; images are planar [C,H,W].  Optional inputs may be NULL
 * (colors_precomp xor shs; scales+rotations xor cov3D_precomp).
 */
#ifndef GSR_H_INCLUDED
#define GSR_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum gsr_status {
    GSR_OK = 0,
    GSR_ERR_ARGS = 1,   /* invalid argument combination or shape */
    GSR_ERR_ALLOC = 2,  /* an allocation callback returned NULL */
    GSR_ERR_HIP = 3,    /* a HIP runtime / launch error (message: gsr_last_error) */
};

/* Replaces std::function<char*(size_t)> (rasterizer.h:30-33, rasterize_points.cu:27-37). */
typedef void* (*gsr_alloc_fn)(void* ctx, size_t bytes);
/* Host callback of gsr_rasterize_backward_ex after each Gaussian range [begin, end) of the
 * per-Gaussian backward has been queued on the call's stream. */
typedef void (*gsr_chunk_fn)(void* ctx, int begin, int end);

/*
 * Replaces CudaRasterizer::Rasterizer::forward (rasterizer.h:29-61,
 * rasterizer_impl.cu:285-448).  radii may be NULL (kept internally).
 */
int gsr_rasterize_forward(gsr_alloc_fn geom_alloc, void* geom_ctx, gsr_alloc_fn binning_alloc, void* binning_ctx,
                          gsr_alloc_fn image_alloc, void* image_ctx, gsr_alloc_fn tile_alloc, void* tile_ctx,
                          int P, int sh_degree, int SHM, int sg_degree, int SGM, const float* background, int width,
                          int height, const float* means3D, const float* colors_precomp, const float* opacities,
                          const float* scales, const float* rotations, const float* cov3D_precomp,
                          const float* shs, const float* sg_axis, const float* sg_sharpness, const float* sg_color,
                          float scale_modifier, const float* viewmatrix, const float* projmatrix,
                          const float* cam_pos, float tan_fovx, float tan_fovy, float kernel_size, int prefiltered,
                          float* out_color, float* out_mdepth, float* out_alpha, float* out_normal, int* radii,
                          int require_depth, int debug, void* stream, int* num_rendered);

/*
 * gsr_rasterize_forward with a fifth allocator for the forward-only scratch
 * (the depth-sort / scan temporaries and the tile-list building state: at 1M
 * Gaussians and 1080p about 0.25 GB that the reference keeps inside the saved
 * geometry / binning buffers until the backward).  scratch_alloc may be called
 * more than once per call; every block it returns must stay valid until the
 * call returns, and may be released then (stream-ordered: the kernels that use
 * it are queued on `stream`).  scratch_alloc == NULL is gsr_rasterize_forward.
 * The buffers the backward reads have the same layout either way.
 */
int gsr_rasterize_forward_ex(gsr_alloc_fn geom_alloc, void* geom_ctx, gsr_alloc_fn binning_alloc, void* binning_ctx,
                             gsr_alloc_fn image_alloc, void* image_ctx, gsr_alloc_fn tile_alloc, void* tile_ctx,
                             int P, int sh_degree, int SHM, int sg_degree, int SGM, const float* background, int width,
                             int height, const float* means3D, const float* colors_precomp, const float* opacities,
                             const float* scales, const float* rotations, const float* cov3D_precomp,
                             const float* shs, const float* sg_axis, const float* sg_sharpness, const float* sg_color,
                             float scale_modifier, const float* viewmatrix, const float* projmatrix,
                             const float* cam_pos, float tan_fovx, float tan_fovy, float kernel_size, int prefiltered,
                             float* out_color, float* out_mdepth, float* out_alpha, float* out_normal, int* radii,
                             int require_depth, int debug, void* stream, int* num_rendered,
                             gsr_alloc_fn scratch_alloc, void* scratch_ctx);

/*
 * Replaces CudaRasterizer::Rasterizer::backward (rasterizer.h:63-109,
 * rasterizer_impl.cu:452-592).  geom/binning/image/tile buffers are the ones
 * the forward obtained from its callbacks; R is the forward's num_rendered.
 * Output gradients (all fully overwritten): dL_dmean3D [P,3],
 * dL_dmean2D [P,3] (x, y, and the |.|-sum channel, render_backward.cu:1028),
 * dL_dcolor [P,3], dL_dopacity [P,1], dL_dscale [P,3], dL_drot [P,4],
 * dL_dcov3D [P,6], dL_dsh [P,SHM,3], dL_dsg_axis [P,SGM,3],
 * dL_dsg_sharpness [P,SGM], dL_dsg_color [P,SGM,3].
 * An upstream image gradient (dL_dpix, dL_dpix_mdepth, dL_dalphas,
 * dL_dpixel_normals) may be NULL for an output the loss does not use: it is
 * then zero (no reference equivalent; the autograd wrapper passes None
 * instead of materialising zero images).
 */
int gsr_rasterize_backward(gsr_alloc_fn geom_bwd_alloc, void* geom_bwd_ctx, int P, int sh_degree, int SHM,
                           int sg_degree, int SGM, int R, const float* background, int width, int height,
                           const float* means3D, const float* colors_precomp, const float* opacities,
                           const float* scales, const float* rotations, const float* cov3D_precomp,
                           const float* shs, const float* sg_axis, const float* sg_sharpness,
                           const float* sg_color, float scale_modifier, const float* viewmatrix,
                           const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                           float kernel_size, const int* radii, const float* alphas, const float* normalmap,
                           const float* mdepth, const void* geom_buffer, const void* binning_buffer,
                           const void* image_buffer, const void* tile_buffer, const float* dL_dpix,
                           const float* dL_dpix_mdepth, const float* dL_dalphas, const float* dL_dpixel_normals,
                           float* dL_dmean3D, float* dL_dmean2D, float* dL_dcolor, float* dL_dopacity,
                           float* dL_dscale, float* dL_drot, float* dL_dcov3D, float* dL_dsh, float* dL_dsg_axis,
                           float* dL_dsg_sharpness, float* dL_dsg_color, int require_depth, int debug,
                           void* stream);

/*
 * gsr_rasterize_backward with the per-Gaussian backward split into `chunks`
 * consecutive Gaussian ranges (no reference equivalent: the view-parallel
 * training step).  After each range's kernel is queued on
 * `stream`, on_chunk(chunk_ctx, begin, end) runs on the calling thread, so
 * the caller can post that range's gradient exchange on another stream while
 * the next range computes (gsr_dist.OverlappedViewGrads).  The ranges hold
 * ceil(ceil(P / chunks) / 256) * 256 Gaussians each (the last one fewer).  With dc_rows
 * non-NULL ([P][3] floats, SH colour path only) the kernel writes each
 * Gaussian's DC gradient row dL/dsh[:, 0, :] there and leaves dL_dsh and the
 * SG gradient rows unwritten: gsr_view_color_grads_chunked rebuilds them from
 * every view's DC rows.  chunks = 1, on_chunk = NULL, dc_rows = NULL is
 * gsr_rasterize_backward.
 */
int gsr_rasterize_backward_ex(gsr_alloc_fn geom_bwd_alloc, void* geom_bwd_ctx, int P, int sh_degree, int SHM,
                              int sg_degree, int SGM, int R, const float* background, int width, int height,
                              const float* means3D, const float* colors_precomp, const float* opacities,
                              const float* scales, const float* rotations, const float* cov3D_precomp,
                              const float* shs, const float* sg_axis, const float* sg_sharpness,
                              const float* sg_color, float scale_modifier, const float* viewmatrix,
                              const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                              float kernel_size, const int* radii, const float* alphas, const float* normalmap,
                              const float* mdepth, const void* geom_buffer, const void* binning_buffer,
                              const void* image_buffer, const void* tile_buffer, const float* dL_dpix,
                              const float* dL_dpix_mdepth, const float* dL_dalphas, const float* dL_dpixel_normals,
                              float* dL_dmean3D, float* dL_dmean2D, float* dL_dcolor, float* dL_dopacity,
                              float* dL_dscale, float* dL_drot, float* dL_dcov3D, float* dL_dsh, float* dL_dsg_axis,
                              float* dL_dsg_sharpness, float* dL_dsg_color, int require_depth, int debug,
                              int chunks, gsr_chunk_fn on_chunk, void* chunk_ctx, float* dc_rows, void* stream);

/*
 * The split SH layout of training (round 5): GaussianModel keeps the DC and
 * the higher-order SH coefficients as two tensors (_features_dc [P,1,3],
 * _features_rest [P,SHM-1,3]) and get_features concatenates them every call
 * (scene/gaussian_model.py:165-169: 192 MB at 1M Gaussians, and the
 * gradient's split in the backward).  These two entry points take them as
 * they are: `shs` is then the DC rows [P][3] and `shs_rest` the rest
 * [P][SHM-1][3] (SHM counts all coefficients, as before); the backward writes
 * dL_dsh [P][3] and dL_dsh_rest [P][SHM-1][3].  NULL shs_rest is exactly
 * the _ex call.  With dc_rows (the overlapped exchange, ABI 20) neither SH
 * gradient tensor is written: gsr_view_color_grads_chunked rebuilds both.
 */
int gsr_rasterize_forward_ex2(gsr_alloc_fn geom_alloc, void* geom_ctx, gsr_alloc_fn binning_alloc, void* binning_ctx,
                              gsr_alloc_fn image_alloc, void* image_ctx, gsr_alloc_fn tile_alloc, void* tile_ctx,
                              int P, int sh_degree, int SHM, int sg_degree, int SGM, const float* background,
                              int width, int height, const float* means3D, const float* colors_precomp,
                              const float* opacities, const float* scales, const float* rotations,
                              const float* cov3D_precomp, const float* shs, const float* sg_axis,
                              const float* sg_sharpness, const float* sg_color, float scale_modifier,
                              const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                              float tan_fovy, float kernel_size, int prefiltered, float* out_color, float* out_mdepth,
                              float* out_alpha, float* out_normal, int* radii, int require_depth, int debug,
                              void* stream, int* num_rendered, gsr_alloc_fn scratch_alloc, void* scratch_ctx,
                              const float* shs_rest);
int gsr_rasterize_backward_ex2(gsr_alloc_fn geom_bwd_alloc, void* geom_bwd_ctx, int P, int sh_degree, int SHM,
                               int sg_degree, int SGM, int R, const float* background, int width, int height,
                               const float* means3D, const float* colors_precomp, const float* opacities,
                               const float* scales, const float* rotations, const float* cov3D_precomp,
                               const float* shs, const float* sg_axis, const float* sg_sharpness,
                               const float* sg_color, float scale_modifier, const float* viewmatrix,
                               const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                               float kernel_size, const int* radii, const float* alphas, const float* normalmap,
                               const float* mdepth, const void* geom_buffer, const void* binning_buffer,
                               const void* image_buffer, const void* tile_buffer, const float* dL_dpix,
                               const float* dL_dpix_mdepth, const float* dL_dalphas, const float* dL_dpixel_normals,
                               float* dL_dmean3D, float* dL_dmean2D, float* dL_dcolor, float* dL_dopacity,
                               float* dL_dscale, float* dL_drot, float* dL_dcov3D, float* dL_dsh, float* dL_dsg_axis,
                               float* dL_dsg_sharpness, float* dL_dsg_color, int require_depth, int debug,
                               int chunks, gsr_chunk_fn on_chunk, void* chunk_ctx, float* dc_rows, void* stream,
                               const float* shs_rest, float* dL_dsh_rest);

/* The Gaussian range size gsr_rasterize_backward_ex uses for `chunks` ranges
 * of P Gaussians: ceil(ceil(P / chunks) / 256) * 256 (whole 256-Gaussian
 * workgroups; the last range holds the rest).  The range-major layout of the
 * gathered DC rows (gsr_view_color_grads_chunked) depends on it, so callers
 * take it from here.  -1 for P < 0 or chunks < 1.  Host only. */
int gsr_backward_chunk_size(int P, int chunks);

/* Replaces CudaRasterizer::Rasterizer::markVisible (rasterizer.h:21-27,
 * rasterizer_impl.cu:186-197): present[i] = (view-space z > 0.2). */
int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, void* stream);

/*
 * sample_depth: the median depth of the Gaussian field
 * at PN arbitrary world points seen from one camera — the multi-view
 * geometric-consistency term of the reference's training loss
 * (utils/loss_utils.py:160, gaussian_renderer/__init__.py:225-278).
 *
 * Replaces CudaRasterizer::Rasterizer::sampleDepth (rasterizer.h:170-195,
 * rasterizer_impl.cu:1042-1245), bound as _C.sample_rasterized_depth
 * (DGR/ext.cpp:21, rasterize_points.cu:459-553).  The six resize callbacks
 * are the reference's geometry, binning, point, point-binning, tile and
 * duplicated-tile buffers.  points3D [PN,3]; output [PN,3] is the
 * camera-space point (x, y, z) at the median depth along its ray and
 * inside [PN] (uint8) whether the median is defined; both are written for the
 * points that project into the image and left untouched for the others (the
 * reference zero-initialises them, so callers pass zeroed buffers).
 * kernel_size is whatever the caller passes: the reference's Python wrapper
 * passes 0.0 here (DGR/__init__.py:500-518) and the settings' value to the
 * backward.  Synchronises `stream` once (K, valid points, block count).
 * *num_points = points that project into the image, *num_duplicated_tiles =
 * the reference's count of 512-point blocks (both opaque to callers; the
 * backward ignores them).
 */
int gsr_sample_depth_forward(gsr_alloc_fn geom_alloc, void* geom_ctx, gsr_alloc_fn binning_alloc, void* binning_ctx,
                             gsr_alloc_fn point_alloc, void* point_ctx, gsr_alloc_fn point_binning_alloc,
                             void* point_binning_ctx, gsr_alloc_fn tile_alloc, void* tile_ctx,
                             gsr_alloc_fn dup_tile_alloc, void* dup_tile_ctx, int PN, int P, int width, int height,
                             const float* points3D, const float* means3D, const float* opacities,
                             const float* scales, float scale_modifier, const float* rotations,
                             const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                             const float* cam_pos, float tan_fovx, float tan_fovy, float kernel_size,
                             int prefiltered, float* output, uint8_t* inside, int debug, void* stream,
                             int* num_rendered, int* num_points, int* num_duplicated_tiles);

/* gsr_sample_depth_forward with the forward-only scratch allocator of
 * gsr_rasterize_forward_ex (same contract; the saved buffers keep their layout). */
int gsr_sample_depth_forward_ex(gsr_alloc_fn geom_alloc, void* geom_ctx, gsr_alloc_fn binning_alloc,
                                void* binning_ctx, gsr_alloc_fn point_alloc, void* point_ctx,
                                gsr_alloc_fn point_binning_alloc, void* point_binning_ctx, gsr_alloc_fn tile_alloc,
                                void* tile_ctx, gsr_alloc_fn dup_tile_alloc, void* dup_tile_ctx, int PN, int P,
                                int width, int height, const float* points3D, const float* means3D,
                                const float* opacities, const float* scales, float scale_modifier,
                                const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                                const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                                float kernel_size, int prefiltered, float* output, uint8_t* inside, int debug,
                                void* stream, int* num_rendered, int* num_points, int* num_duplicated_tiles,
                                gsr_alloc_fn scratch_alloc, void* scratch_ctx);

/*
 * integrate / evaluate_sdf: forward-only queries of the
 * Gaussian field at PN world points, used by the offline tetrahedral mesh
 * extraction (mesh_extract_tetrahedra.py:75, gaussian_renderer/__init__.py:
 * 101-222).  Same six resize callbacks, arguments and point binning as
 * gsr_sample_depth_forward; view2gaussian_precomp is accepted and ignored, as
 * in the reference.  Outputs are written for the points that project into
 * the image and left untouched for the others (callers pass zeroed buffers,
 * as the reference's torch::full(0)).  Synchronises `stream` once.
 *
 * gsr_integrate_forward replaces CudaRasterizer::Rasterizer::
 * evaluateTransmittance (rasterizer.h:111-138, rasterizer_impl.cu:594-815),
 * bound as _C.integrate_gaussians_to_points (DGR/rasterize_points.cu:279-366):
 * out_transmittance [PN] = the vacancy transmittance at each point's distance
 * from the camera (sample_forward.cu:55-169), inside [PN] = 1.
 *
 * gsr_evaluate_sdf_forward replaces Rasterizer::evaluateSDF (rasterizer.h:
 * 140-168, rasterizer_impl.cu:817-1040), bound as
 * _C.evaluate_sdf_from_signle_view (rasterize_points.cu:368-457):
 * out_depth [PN] = the median depth along the point's ray (+-0.8 first
 * window, 6 bisection passes, sample_forward.cu:171-427), out_sdf [PN] =
 * out_depth - |p_view|, inside [PN] = whether the median is defined.
 */
int gsr_integrate_forward(gsr_alloc_fn geom_alloc, void* geom_ctx, gsr_alloc_fn binning_alloc, void* binning_ctx,
                          gsr_alloc_fn point_alloc, void* point_ctx, gsr_alloc_fn point_binning_alloc,
                          void* point_binning_ctx, gsr_alloc_fn tile_alloc, void* tile_ctx,
                          gsr_alloc_fn dup_tile_alloc, void* dup_tile_ctx, int PN, int P, int width, int height,
                          const float* points3D, const float* means3D, const float* opacities, const float* scales,
                          float scale_modifier, const float* rotations, const float* cov3D_precomp,
                          const float* view2gaussian_precomp, const float* viewmatrix, const float* projmatrix,
                          const float* cam_pos, float tan_fovx, float tan_fovy, float kernel_size, int prefiltered,
                          float* out_transmittance, uint8_t* inside, int debug, void* stream, int* num_rendered);
int gsr_evaluate_sdf_forward(gsr_alloc_fn geom_alloc, void* geom_ctx, gsr_alloc_fn binning_alloc, void* binning_ctx,
                             gsr_alloc_fn point_alloc, void* point_ctx, gsr_alloc_fn point_binning_alloc,
                             void* point_binning_ctx, gsr_alloc_fn tile_alloc, void* tile_ctx,
                             gsr_alloc_fn dup_tile_alloc, void* dup_tile_ctx, int PN, int P, int width, int height,
                             const float* points3D, const float* means3D, const float* opacities,
                             const float* scales, float scale_modifier, const float* rotations,
                             const float* cov3D_precomp, const float* view2gaussian_precomp,
                             const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                             float tan_fovy, float kernel_size, int prefiltered, float* out_depth, float* out_sdf,
                             uint8_t* inside, int debug, void* stream, int* num_rendered);

/*
 * Replaces CudaRasterizer::Rasterizer::sampleDepthBackward (rasterizer.h:197-233,
 * rasterizer_impl.cu:1247-1394), bound as _C.sample_rasterized_depth_backward
 * (rasterize_points.cu:555-633).  The six buffers are the forward's; R, RN, TN
 * its three counts.  Gradients written: dL_dopacity [P,1], dL_dmean3D [P,3],
 * dL_dscale [P,3] + dL_drot [P,4] (scale/rotation path) or dL_dcov3D [P,6]
 * (precomputed covariance), all fully overwritten; dL_dpoints3D [PN,3] is
 * written for the points that project into the image only (callers pass a
 * zeroed buffer, as the reference's torch::zeros_like).
 */
int gsr_sample_depth_backward(gsr_alloc_fn geom_bwd_alloc, void* geom_bwd_ctx, int PN, int P, int RN, int R, int TN,
                              int width, int height, const float* points3D, const float* means3D,
                              const float* opacities, const float* scales, float scale_modifier,
                              const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                              const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                              float kernel_size, const void* geom_buffer, const void* binning_buffer,
                              const void* point_buffer, const void* point_binning_buffer, const void* tile_buffer,
                              const void* dup_tile_buffer, const uint8_t* inside, const float* dL_doutput,
                              float* dL_dopacity, float* dL_dmean3D, float* dL_dcov3D, float* dL_dscale,
                              float* dL_drot, float* dL_dpoints3D, int debug, void* stream);

/*
 * Training update.  One Adam step over up to 16
 * parameter groups in a single launch — torch.optim.Adam's update with its
 * rounding order (scene/gaussian_model.py:347-351 builds it with eps 1e-15;
 * train.py:259-261 steps it), every group at the same step count `step`
 * (>= 1, the value after increment) with its own learning rate.  Groups are
 * flat fp32 arrays of n elements; param, exp_avg and exp_avg_sq are updated
 * in place.
 */
typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    long long n;
    double lr;
} gsr_adam_group;
/* lr, betas and eps are doubles, like the Python floats torch combines them
 * in before rounding to fp32 (e.g. 1 - beta2). */
int gsr_adam_step(int n_groups, const gsr_adam_group* groups, double step, double beta1, double beta2, double eps,
                  void* stream);

/*
 * GaussianModel.add_densification_stats + the max_radii2D update
 * (scene/gaussian_model.py:818-821, train.py:236-237) for the P Gaussians
 * with radii > 0: max_radii2D = max(max_radii2D, radii), accum += |vgrad.xy|,
 * accum_abs += |vgrad.z|, denom += 1.  vgrad [P,3] is the viewspace-points
 * gradient (dL/dmeans2D of the backward); the four statistics are [P] fp32.
 */
int gsr_densify_stats(int P, const float* vgrad, const int* radii, float* max_radii2D, float* accum,
                      float* accum_abs, float* denom, void* stream);

/*
 * View-parallel training (no reference equivalent: the
 * reference trains one view per step on one GPU).  The SH / SG gradient rows
 * of a step summed over n_views views, rebuilt from each view's DC gradient
 * row and camera centre (view_grads.hip): per view the colour backward
 * (CR/render_backward.cu:56-191) makes every row a function of the
 * clamp-masked dL/dRGB = dL/dsh[:, 0, :] / SH_C0 and the view direction.
 * gathered: [n_views][P * 3 + 4] fp32, view v's dL/dsh[:, 0, :] (P x 3)
 * followed by its camera centre (3) and one pad float.  Outputs are
 * overwritten: dL_dsh [P, SHM, 3] (rows past (sh_degree + 1)^2 zero), and
 * when SGM > 0 dL_dsg_axis [P, SGM, 3], dL_dsg_sharpness [P, SGM],
 * dL_dsg_color [P, SGM, 3] (lobes past sg_degree zero); sg_degree <= 7.
 */
/*
 * gsr_view_color_grads for the layout gsr_dist.OverlappedViewGrads gathers
 * range by range: the Gaussians in ranges of `chunk` (the last shorter);
 * range [b, b + len) occupies gathered[3 n_views b, 3 n_views (b + len)) as
 * [n_views][len][3] DC rows; the camera centres are campos [n_views][4].
 * dL_dsh_rest (ABI 20; NULL: the one-tensor layout): the split SH layout of
 * gsr_rasterize_backward_ex2 — dL_dsh is then the DC rows [P, 1, 3] and
 * dL_dsh_rest the other SHM - 1 rows [P, SHM - 1, 3].
 */
int gsr_view_color_grads_chunked(int P, int sh_degree, int SHM, int sg_degree, int SGM, int n_views, int chunk,
                                 const float* gathered, const float* campos, const float* means3D,
                                 const float* sg_axis, const float* sg_sharpness, const float* sg_color,
                                 float* dL_dsh, float* dL_dsg_axis, float* dL_dsg_sharpness, float* dL_dsg_color,
                                 float* dL_dsh_rest, void* stream);

int gsr_view_color_grads(int P, int sh_degree, int SHM, int sg_degree, int SGM, int n_views, const float* gathered,
                         const float* means3D, const float* sg_axis, const float* sg_sharpness, const float* sg_color,
                         float* dL_dsh, float* dL_dsg_axis, float* dL_dsg_sharpness, float* dL_dsg_color,
                         void* stream);

/*
 * Multi-view photometric term: replaces WarpPatchNCC /
 * forward_mode_differentiation (submodules/warp-patch-ncc/warp_patch_ncc.cu:5-52,
 * cuda_warp_patch_ncc/warp_patch_ncc_impl.cu:18-302), bound as
 * warp_patch_ncc._C.warp_patch_ncc.  For P reference pixels uvs [P,2] (int32)
 * with depths [P], normals [P,3]: the NCC of the 7x7 half-step patch against
 * its homography warp into image_n, and d(NCC)/d(depth) [P],
 * d(NCC)/d(normal) [P,3]; valid [P] (uint8).  R [9] is the r-to-n rotation
 * as the reference's column-major float33, T [3]; images are [H,W] fp32
 * (grey).  Every output element is written.
 */
int gsr_warp_patch_ncc(int P, const float* depths, const float* normals, const int* uvs, const float* R,
                       const float* T, const float* image_r, const float* image_n, float fx_r, float fy_r,
                       float cx_r, float cy_r, float fx_n, float fy_n, float cx_n, float cy_n, int image_height_r,
                       int image_width_r, int image_height_n, int image_width_n, float* ncc, float* grad_depths,
                       float* grad_normals, uint8_t* valid, void* stream);

/*
 * GaussianModel's activation getters (the callers of the
 * rasterizer in training; scene/gaussian_model.py:146-212), one thread per
 * Gaussian.  scale/opacity with the 3D filter
 * (get_scaling_n_opacity_with_3D_filter): scaling [P,3] and opacity [P]
 * are the raw parameters, filter_3D [P]; scales [P,3] = sqrt(exp(s)^2 +
 * f^2), opacities [P] = sigmoid(o) * sqrt(prod exp(s)^2 / prod(exp(s)^2 +
 * f^2)).  The backward writes dL/dscaling, dL/dopacity for dL/dscales,
 * dL/dopacities (either may be NULL: zero).  normalize_rows: y = x /
 * max(|x|, 1e-12) per row of D (get_rotation's F.normalize) and its
 * backward.
 */
int gsr_scale_opacity_3d_filter(int P, const float* scaling, const float* opacity, const float* filter_3D,
                                float* scales, float* opacities, void* stream);
int gsr_scale_opacity_3d_filter_backward(int P, const float* scaling, const float* opacity, const float* filter_3D,
                                         const float* dL_dscales, const float* dL_dopacities, float* dL_dscaling,
                                         float* dL_dopacity, void* stream);
int gsr_normalize_rows(int n, int D, const float* x, float* y, void* stream);
int gsr_normalize_rows_backward(int n, int D, const float* x, const float* dL_dy, float* dL_dx, void* stream);

/*
 * PatchMatch multi-view loss, fused (the training
 * step's caller of sample_depth and warp_patch_ncc): replaces the torch body
 * of PatchMatch.__call__ (utils/loss_utils.py:140-267) around its two
 * extension calls, for one view of H x W pixels and its nearest view.
 *  - lift: points [H*W,3] = (median_depth * ray - T) @ M, ray = ((x - Cx) / Fx,
 *    (y - Cy) / Fy, 1) (:147-153; T = view.T, M = view.R^T, row-major);
 *    backward: dL/dmedian_depth [H*W] for dL/dpoints.
 *  - terms forward: from points_nearest [H*W,3] (sample_depth of the lifted
 *    points in the nearest view) and inside [H*W] (uint8): the reprojection
 *    into the view (point in view = tv + p @ Mv, Mv row-major), the pixel
 *    noise, the geometric mask (inside, both depths > 0.2, noise < noise_th,
 *    median depth > 0) and weight exp(-noise) (:160-221), and at the masked
 *    pixels the NCC (as gsr_warp_patch_ncc, R/T/intrinsics/images likewise) of
 *    the normalised normal [3,H*W] (:228-256).  out4 (device) = {geo_loss,
 *    ncc_loss, d_mask count, ncc_mask count}; a loss over an empty mask is 0
 *    (:223-224).  saved_* ([H*W] w, flags, gd; [H*W,3] gn) are for the
 *    backward.  One scratch allocation (16 B per 256 pixels); no host
 *    synchronisation.
 *  - terms backward: dL/d(points_nearest, median_depth, normal) for
 *    dL/d(geo_loss, ncc_loss) = dL_dloss2 (device, 2 floats).  Every output
 *    element is written.
 */
int gsr_patchmatch_lift(int H, int W, float Fx, float Fy, float Cx, float Cy, const float* T, const float* M,
                        const float* median_depth, float* points, void* stream);
int gsr_patchmatch_lift_backward(int H, int W, float Fx, float Fy, float Cx, float Cy, const float* M,
                                 const float* dL_dpoints, float* dL_dmedian_depth, void* stream);
int gsr_patchmatch_terms_forward(gsr_alloc_fn scratch_alloc, void* scratch_ctx, int H, int W,
                                 const float* median_depth, const float* normal, const float* points_nearest,
                                 const uint8_t* inside, const float* Mv, const float* tv, float Fx, float Fy, float Cx,
                                 float Cy, float noise_th, const float* R, const float* T, const float* image_r,
                                 const float* image_n, float fx_r, float fy_r, float cx_r, float cy_r, float fx_n,
                                 float fy_n, float cx_n, float cy_n, int image_height_n, int image_width_n,
                                 float* saved_w, uint8_t* saved_flags, float* saved_gd, float* saved_gn,
                                 float* out4, void* stream);
int gsr_patchmatch_terms_backward(int H, int W, const float* median_depth, const float* normal,
                                  const float* points_nearest, const uint8_t* inside, const float* Mv, const float* tv,
                                  float Fx, float Fy, float Cx, float Cy, float noise_th, const float* R,
                                  const float* T, const float* image_r, const float* image_n, float fx_r, float fy_r,
                                  float cx_r, float cy_r, float fx_n, float fy_n, float cx_n, float cy_n,
                                  int image_height_n, int image_width_n, const float* saved_w,
                                  const uint8_t* saved_flags, const float* saved_gd, const float* saved_gn,
                                  const float* out4, const float* dL_dloss2, float* dL_dpoints_nearest,
                                  float* dL_dmedian_depth, float* dL_dnormal, void* stream);

/*
 * D-SSIM term: replaces the external fused_ssim(img1,
 * img2, padding) that utils/loss_utils.py:48-49 calls (padding "valid") with
 * the SSIM of the reference's own _ssim (loss_utils.py:36-72): 11 x 11
 * Gaussian window, sigma 1.5, C1 = 1e-4, C2 = 9e-4, zero padding.  Images
 * are NC planes of H x W fp32 (e.g. [1,3,H,W]).  valid != 0 averages over
 * the positions whose window lies inside the image (needs H, W > 10).
 * *out_mean (device) receives the mean SSIM.  factors (device, 3*NC*H*W
 * floats, may be NULL when no gradient is wanted) receives what the backward
 * reads.  The backward writes dL/dimg1 (NC*H*W) for dL/dmean at dL_dmean
 * (device scalar).
 */
int gsr_fused_ssim_forward(gsr_alloc_fn scratch_alloc, void* scratch_ctx, int NC, int H, int W, int valid,
                           const float* img1, const float* img2, float* out_mean, float* factors, void* stream);
int gsr_fused_ssim_backward(int NC, int H, int W, int valid, const float* img1, const float* img2,
                            const float* factors, const float* dL_dmean, float* dL_dimg1, void* stream);

/*
 * Photometric loss, fused: the first term of the reference's training loss
 * as its geometry pipelines compute it (train.py:159-169, 189;
 * utils/loss_utils.py:90-123).  image, gt: [3,H,W] fp32.
 *   g_c = mask ? (mask[p] > 0.5 ? gt_c : bg_c) : gt_c   (mask [H,W], strict;
 *         bg [3], NULL = black)
 *   t_c = the appearance transform of the rendered image (gsr_app_model):
 *         NO x_c; GS E[c,3] + sum_k E[c,k] x_k (embedding [3,4]); PGSR
 *         e[1] + exp(e[0]) x_c (embedding [2]); GAIN gain_c[p] x_c inside the
 *         crop (gain [3,crop_h,crop_w] contiguous; the L1 over the crop only)
 *   out3 = {(1 - lambda) l1 + lambda (1 - ssim), l1 = mean|t - g|, ssim}
 * with ssim the "valid" mean SSIM of the raw image against g (the arithmetic
 * of gsr_fused_ssim_forward).  with_ssim == 0: the L1 alone (any H, W >= 1;
 * out3 = {l1, l1, 0}, lambda ignored).  out_gt (NULL or [3,H,W]) receives g.
 * factors (NULL or 3*3*H*W floats) and emb_sums (NULL, or 12 floats for GS, 2
 * for PGSR) receive what the backward reads; both NULL when no gradient is
 * wanted.  One stencil launch and one fixed-order reduction: two runs give
 * the same bits.  The backward is one launch: dL/dimage [3,H,W], and where
 * asked dL/dembedding (the embedding's shape) and dL/dgain (the gain's),
 * for dL/d out3[0] at dL_dloss (device scalar).
 * GSR_ERR_ARGS before any launch: unknown mode, a mode's buffer missing, a
 * crop outside the image, H or W <= 10 with the SSIM on.
 */
enum gsr_app_model { GSR_APP_NO = 0, GSR_APP_GS = 1, GSR_APP_PGSR = 2, GSR_APP_GAIN = 3 };
int gsr_photo_loss_forward(gsr_alloc_fn scratch_alloc, void* scratch_ctx, int H, int W, int mode, int with_ssim,
                           float lambda_dssim, const float* image, const float* gt, const float* mask,
                           const float* bg, const float* embedding, const float* gain, int crop_top, int crop_left,
                           int crop_h, int crop_w, float* out3, float* out_gt, float* factors, float* emb_sums,
                           void* stream);
int gsr_photo_loss_backward(int H, int W, int mode, int with_ssim, float lambda_dssim, const float* image,
                            const float* gt, const float* mask, const float* bg, const float* embedding,
                            const float* gain, int crop_top, int crop_left, int crop_h, int crop_w,
                            const float* factors, const float* emb_sums, const float* dL_dloss, float* dL_dimage,
                            float* dL_dembedding, float* dL_dgain, void* stream);

/*
 * Depth-normal consistency input: replaces the torch
 * function depth_to_normal (utils/graphics_utils.py:103-119).  depth [H,W];
 * forward: normal [3,H,W] (zero on the border), valid [H,W] uint8;
 * backward: dL/ddepth [H,W] for dL/dnormal [3,H,W].  Fx, Fy, Cx, Cy are the
 * camera's (scene/cameras.py).
 */
int gsr_depth_to_normal_forward(const float* depth, int H, int W, float Fx, float Fy, float Cx, float Cy,
                                float* normal, uint8_t* valid, void* stream);
int gsr_depth_to_normal_backward(const float* depth, int H, int W, float Fx, float Fy, float Cx, float Cy,
                                 const float* dL_dnormal, float* dL_ddepth, void* stream);

/*
 * Initial scales: replaces distCUDA2 / SimpleKNN::knn
 * (submodules/simple-knn/spatial.cu:15-25, simple_knn.cu:175-220), bound as
 * simple_knn._C.distCUDA2 (scene/gaussian_model.py:20, 323).  points [P,3]
 * fp32; mean_dists [P] = the mean of the squared distances to the 3 nearest
 * other points (inf / FLT_MAX-based values when P < 4, as the reference).
 * scratch_alloc is called once (about 48 B per point plus the sort's
 * temporary).  No host synchronisation.
 */
int gsr_knn_mean_dist(gsr_alloc_fn scratch_alloc, void* scratch_ctx, int P, const float* points, float* mean_dists,
                      void* stream);

/*
 * Marching tetrahedra (the mesh of the offline extraction,
 * mesh_extract_tetrahedra.py:128-132): replaces the torch function
 * utils/tetmesh.py:51-190 for one sdf.  tets [T,4] are vertex ids, int32
 * (tets_int64 == 0) or int64, 16-byte aligned; sdf [V] fp32; valid [V] uint8.
 * A vertex is positive when sdf > 0; a tet takes part when 1-3 of its
 * vertices are positive and all four are valid.  Outputs, allocated through
 * the callbacks once their sizes are known (not called for a size of 0):
 * edge_ids [E,2] int64, the undirected edges (a, b), a < b, with exactly one
 * positive end that belong to a participating tet, each once, in ascending
 * (a, b) order — the mesh vertices; faces [F,3] int64 indices into edge_ids,
 * in tet order (the reference lists one-triangle tets before two-triangle
 * tets chunk by chunk; winding and diagonals are the reference's).
 * scratch_alloc is called twice at most: V / 4 + T / 128 bytes before the
 * count, then 20 bytes per crossing-edge slot (3 or 4 per participating tet)
 * plus the radix sort's temporary; both blocks must stay valid until the
 * call returns (stream-ordered, as gsr_rasterize_forward_ex).  Limits:
 * V <= 2^31 - 1, T < 2^32, fewer than 2^32 slots.  A vertex id outside
 * [0, V) is found on the device, reads nothing, and fails the call with
 * GSR_ERR_ARGS; so do V <= 0 with T > 0 and a NULL input with a non-zero
 * size.  Synchronises `stream` twice (the slot count, then E), through the
 * forward's pinned readback slots.  stage_ms (host, 8 floats, may be NULL;
 * measurement only, adds synchronisation): the GPU milliseconds of the vertex
 * flags, count + scan, key emission, sort, ranks, edge and face stages, and 0.
 * The result is the same bits on every run.
 */
int gsr_marching_tetrahedra(gsr_alloc_fn edge_alloc, void* edge_ctx, gsr_alloc_fn face_alloc, void* face_ctx,
                            gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long T, long long V,
                            const void* tets, int tets_int64, const float* sdf, const uint8_t* valid,
                            long long* num_edges, long long* num_faces, float* stage_ms, void* stream);

/*
 * The sweep of the tetrahedral extraction around gsr_integrate_forward
 * (mesh_extract_tetrahedra.py:44-87 and :155-163).  Additive: the
 * ABI version is unchanged.  All buffers are device memory unless noted; the
 * three calls launch one kernel each on `stream`, need no scratch, read
 * nothing back and do not synchronise.  A size of 0 is a valid no-op, a
 * negative size or a NULL required buffer is GSR_ERR_ARGS and touches nothing.
 *
 * gsr_field_view_update folds one view into the running state of N points:
 * ok = inside and, with a mask, sample > 0.5; where ok, seen = 1 and weight =
 * alpha when alpha < weight (or alpha is NaN).  alpha [N] fp32 and inside [N]
 * (one byte per point, non-zero = set) are gsr_integrate_forward's outputs
 * (alpha = 1 - transmittance); weight [N] fp32 and seen [N] uint8 (0 or 1)
 * are updated in place, the caller starts them at 1 and 0.  mask [H,W] fp32 may
 * be NULL (no mask test; points, R, T and the camera numbers are then unused
 * and points, R, T may be NULL).  With a mask, for the points with inside set
 * only (so a point at or behind the near plane never divides): points [N,3]
 * fp32; R [9] and T [3] are HOST fp32, camera = points @ R + T with R
 * row-major; uv = c + s * (camera.xy / camera.z) with c = ((Cx 2 + 1) / W - 1,
 * (Cy 2 + 1) / H - 1) and s = (Fx 2 / W, Fy 2 / H) computed in float64 and
 * rounded to fp32; sample = the bilinear sample of the mask at uv as
 * torch.nn.functional.grid_sample takes it (align_corners=True, zeros
 * padding).  fp32 in the fixed operation order of DESIGN 6k without fused
 * multiply-add.  W, H < 1 with a mask is GSR_ERR_ARGS.
 *
 * gsr_field_finish ends a chunk: sdf [N] fp32 = 0.5 - (seen ? weight : 0),
 * valid [N] (one byte, 0 or 1) = seen.  sdf may be weight and valid may be
 * seen.
 *
 * gsr_field_bisect_step is one bisection step over E edges, in place:
 * left_points, right_points [E,3] fp32 (points_float64 == 0) or fp64,
 * left_sdf, right_sdf [E] fp32, mid_sdf [E] fp32 the field at
 * (left + right) * 0.5.  Where mid_sdf and left_sdf are both < 0 or both > 0
 * the midpoint and mid_sdf replace the left end, otherwise (a mid_sdf of
 * exactly 0 and NaN included) the right end; mid_points [E,3] (written only,
 * a buffer of its own) = the new (left + right) * 0.5: the next step's query
 * points and, after the last step, the vertices.
 */
int gsr_field_view_update(long long N, const float* points, const float* alpha, const uint8_t* inside, const float* R,
                          const float* T, double Fx, double Fy, double Cx, double Cy, int W, int H, const float* mask,
                          float* weight, uint8_t* seen, void* stream);
int gsr_field_finish(long long N, const float* weight, const uint8_t* seen, float* sdf, uint8_t* valid, void* stream);
int gsr_field_bisect_step(long long E, void* left_points, void* right_points, int points_float64, float* left_sdf,
                          float* right_sdf, const float* mid_sdf, void* mid_points, void* stream);

/*
 * Mesh clean-up (the reference's post_process_mesh,
 * mesh_extract_tetrahedra.py:18-40, which runs open3d on the CPU), in two
 * calls.
 *
 * gsr_mesh_clusters is open3d's cluster_connected_triangles: faces [F,3] are
 * vertex ids, int32 (faces_int64 == 0) or int64; vertices [V,3] fp32 may be
 * NULL (no areas; V is then only the bound of the ids, at most 2^31).  Two
 * triangles are adjacent when they share an undirected edge (min, max) of
 * vertex ids: a shared vertex alone does not connect, an edge of three or
 * more triangles connects them all, and the edges of index-degenerate
 * triangles count like any other.  Outputs: triangle_clusters [F] int64 (the
 * caller's buffer), the cluster of every triangle, clusters numbered in
 * ascending order of their lowest triangle index; *num_clusters = C; through
 * the callbacks once C is known (not called when F == 0):
 * cluster_n_triangles [C] int64 and, with vertices, cluster_area [C] float64
 * (0.5 |cross| per triangle, computed and summed in float64 in a fixed order).
 * scratch_alloc is called once: 64 bytes per triangle (72 with areas) plus
 * the radix sort's temporary; the block must stay valid until the call
 * returns (stream-ordered).  Limits: F < 2^31, V <= 2^31.  A vertex id
 * outside [0, V) is found on the device, reads nothing, and fails the call
 * with GSR_ERR_ARGS.  Synchronises `stream` once (C).  stage_ms (host, 8
 * floats, may be NULL; measurement only, adds synchronisation): the GPU
 * milliseconds of the key, sort, union, flatten, cluster-id, count and area
 * stages, and 0.  The result is the same bits on every run.
 *
 * gsr_mesh_filter removes, in this order, the triangles whose cluster has
 * fewer than *n_min triangles (n_min: one int64 in device memory, so a
 * threshold computed on the device needs no readback), the vertices no
 * remaining triangle references, and the remaining triangles with two equal
 * vertex ids (vertices orphaned only by this last step stay, as in open3d's
 * call order).  triangle_clusters [F] and cluster_n_triangles [C] are
 * gsr_mesh_clusters' outputs.  Outputs through the callbacks (not called for
 * a size of 0): vertices [V',3] fp32 and faces [F',3] int64, both in their
 * input order, winding kept.  scratch_alloc is called once (4 bytes per
 * vertex and per triangle plus a scan's temporary).  Limits: F, V < 2^31.
 * An id outside its range fails the call with GSR_ERR_ARGS.  Synchronises
 * `stream` once (V' and F').  The result is the same bits on every run.
 */
int gsr_mesh_clusters(gsr_alloc_fn count_alloc, void* count_ctx, gsr_alloc_fn area_alloc, void* area_ctx,
                      gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long F, long long V, const void* faces,
                      int faces_int64, const float* vertices, long long* triangle_clusters, long long* num_clusters,
                      float* stage_ms, void* stream);
int gsr_mesh_filter(gsr_alloc_fn vertex_alloc, void* vertex_ctx, gsr_alloc_fn face_alloc, void* face_ctx,
                    gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long F, long long V, long long C,
                    const float* vertices, const void* faces, int faces_int64, const long long* triangle_clusters,
                    const long long* cluster_n_triangles, const long long* n_min, long long* num_vertices,
                    long long* num_faces, void* stream);

/*
 * TSDF fusion and marching cubes (the open3d VoxelBlockGrid of the
 * reference's mesh_extract.py:63-85, which runs on the CPU).  Additive: the
 * ABI version is unchanged.  The contract is DESIGN §6h; it restates open3d's
 * behaviour from memory and claims no bit-parity with it.  Blocks are R^3
 * voxels (block_resolution R = 8 or 16); a voxel is linear in (z R + y) R + x;
 * a block's key is (x + 2^20) << 42 | (y + 2^20) << 21 | (z + 2^20).  The
 * caller owns the grid: tsdf / weight [capacity, R^3] fp32, colour
 * [capacity, R^3, 3] fp32 or NULL, and the index sorted_keys [num_blocks]
 * (ascending) with sorted_slots [num_blocks].  intrinsic (fx, fy, cx, cy) and
 * extrinsic (world -> camera, 4x4 row-major) are host fp32; all device
 * arithmetic is fp32.
 *
 * gsr_tsdf_touch: the blocks a depth image [H,W] touches.  Every pixel with
 * x % 4 == y % 4 == 0 and 0 < d = depth / depth_scale < depth_max gives four
 * samples o + t dir, t = t_min + k (t_max - t_min) / 3, t_min = max(d -
 * sdf_trunc, 0), t_max = min(d + sdf_trunc, depth_max), o = -R^T t the camera
 * centre, dir = R^T ((x - cx) / fx, (y - cy) / fy, 1); block =
 * floor(sample / block_size).  Output through coord_alloc (not called for 0):
 * the distinct blocks [n,3] int32, ascending by key.  A block beyond +-2^20
 * fails the call with GSR_ERR_ARGS.  scratch_alloc is called once (20 bytes
 * per sample plus the sort's temporary).  Synchronises `stream` once (n).
 *
 * gsr_tsdf_lookup: rank [n] int32 = the position of each of block_coords [n,3]
 * in sorted_keys, or -1.  No synchronisation.
 *
 * gsr_tsdf_integrate: one view into the listed blocks only (block_coords
 * [n,3] int32 with their slots [n] int32; a slot outside [0, capacity) is
 * skipped).  Per voxel: camera-space position of (block R + (x, y, z))
 * voxel_size; skipped when z_c <= 0, when the pixel (round(fx x_c / z_c + cx),
 * round(fy y_c / z_c + cy)) is outside the image, when d = depth / depth_scale
 * is not in (0, depth_max], or when d - z_c < -sdf_trunc; else the running
 * mean of min(d - z_c, sdf_trunc) / sdf_trunc (and of image [H,W,3]) with
 * weight + 1.  One thread owns a voxel; a block must not be listed twice.  No
 * synchronisation.
 *
 * gsr_tsdf_extract: marching cubes over the cubes whose 8 corners lie in
 * present blocks with weight > weight_threshold; inside is tsdf < 0.  One
 * vertex per crossed edge of an emitted cube, shared by the cubes around it,
 * at (p_a + t (p_b - p_a)) voxel_size, t = tsdf_a / (tsdf_a - tsdf_b), colour
 * likewise.  Vertices are ordered by (block in key order, voxel, axis),
 * triangles by (block, voxel, order in the case table of csrc/mc_table.h);
 * normals point to the positive side.  Outputs through the callbacks (not
 * called when there is no triangle): vertices [V,3] fp32, colours [V,3] fp32
 * (only with color), faces [F,3] int64.  scratch_alloc is called once (3.5
 * bytes per voxel).  Limit: fewer than (2^31 - 1) / 5 voxels.  Synchronises
 * `stream` once (V and F).  stage_ms (host, 8 floats, may be NULL;
 * measurement only, adds synchronisation): mark, count, vertices, faces.  The
 * result is the same bits on every run.
 */
int gsr_tsdf_touch(gsr_alloc_fn coord_alloc, void* coord_ctx, gsr_alloc_fn scratch_alloc, void* scratch_ctx,
                   const float* depth, int H, int W, const float* intrinsic, const float* extrinsic,
                   float depth_scale, float depth_max, float sdf_trunc, float block_size, long long* num_blocks,
                   void* stream);
int gsr_tsdf_lookup(long long n, const int* block_coords, long long num_blocks, const long long* sorted_keys,
                    int* rank, void* stream);
int gsr_tsdf_integrate(long long n, int block_resolution, const int* block_coords, const int* slots,
                       long long capacity, float voxel_size, float* tsdf, float* weight, float* color,
                       const float* depth, const float* image, int H, int W, const float* intrinsic,
                       const float* extrinsic, float depth_scale, float depth_max, float sdf_trunc, void* stream);
int gsr_tsdf_extract(gsr_alloc_fn vertex_alloc, void* vertex_ctx, gsr_alloc_fn color_alloc, void* color_ctx,
                     gsr_alloc_fn face_alloc, void* face_ctx, gsr_alloc_fn scratch_alloc, void* scratch_ctx,
                     long long num_blocks, int block_resolution, float voxel_size, float weight_threshold,
                     const long long* sorted_keys, const int* sorted_slots, const float* tsdf, const float* weight,
                     const float* color, long long* num_vertices, long long* num_faces, float* stage_ms,
                     void* stream);

/*
 * Point-cloud evaluation (the reference's dtu_eval/eval.py --mode mesh, which
 * runs numpy, a process pool and sklearn KD-trees on the CPU), in three calls.
 * All points are float64 [n,3]; the arithmetic is float64 without contraction,
 * in the reference's order.  Additive: the ABI version is unchanged.
 *
 * gsr_mesh_sample_points (eval.py:48-71): vertices [V,3] float64, faces [F,3]
 * int32 (faces_int64 == 0) or int64.  Output through point_alloc once its size
 * is known: points [V + S,3], the vertices first, then per triangle with
 * area2 = |v1 x v2| > 0, in triangle order, v1 k0 + v2 k1 + p0 for
 * k0 = (i + .5) / max(n1, 1e-7), k1 = (j + .5) / max(n2, 1e-7), k0 + k1 < 1,
 * 0 <= i <= n1 (outer), 0 <= j <= n2 (inner), n = floor(l / thr),
 * thr = density sqrt(l1 l2 / area2).  *num_points = V + S.  scratch_alloc is
 * called once (8 bytes per triangle plus a scan's temporary).  Limits:
 * F, V < 2^31, S < 2^38.  A vertex id outside [0, V) or a triangle whose
 * lattice is not finite fails the call with GSR_ERR_ARGS.  Synchronises
 * `stream` once (S).  stage_ms: count, scan, emit.
 *
 * gsr_points_downsample (eval.py:80-94 after the shuffle): points [N,3] in the
 * order the reference's loop walks them.  A point survives iff no earlier
 * surviving point has dx^2 + dy^2 + dz^2 <= radius^2 (exact duplicates
 * included): the sequential loop's result, computed in parallel rounds that run
 * until no point is undecided (*num_rounds, may be NULL; a chain of
 * dependencies costs a round per link).  Output through kept_alloc: the
 * positions of the survivors [M] int64, ascending; *num_kept = M.
 * scratch_alloc is called once (48 bytes per point plus the radix sort's
 * temporary).  Limits: N < 2^31, fewer than 2^31 cells of side radius along an
 * axis.  Synchronises `stream` once for the bounds, once per round and once
 * for M.  stage_ms: bounds, cell sort, rounds (host waits included), scan,
 * write.
 *
 * gsr_points_nearest: dist [Q] (the caller's buffer) = the Euclidean distance
 * from query [Q,3] to the nearest of ref [R,3] where that is < max_dist, else
 * +inf (all +inf when R == 0).  Exact within max_dist.  scratch_alloc is called
 * once (44 bytes per ref point, 20 per query, plus the sort's temporary).
 * Limits: Q, R < 2^31; ref must be finite.  Synchronises `stream` once (the
 * bounds of ref).  stage_ms: bounds, ref sort, query sort, search.
 *
 * stage_ms (host, 8 floats, may be NULL; measurement only, adds
 * synchronisation) as in gsr_marching_tetrahedra.  Every result is the same
 * bits on every run.
 */
int gsr_mesh_sample_points(gsr_alloc_fn point_alloc, void* point_ctx, gsr_alloc_fn scratch_alloc, void* scratch_ctx,
                           long long V, long long F, const double* vertices, const void* faces, int faces_int64,
                           double density, long long* num_points, float* stage_ms, void* stream);
int gsr_points_downsample(gsr_alloc_fn kept_alloc, void* kept_ctx, gsr_alloc_fn scratch_alloc, void* scratch_ctx,
                          long long N, const double* points, double radius, long long* num_kept,
                          long long* num_rounds, float* stage_ms, void* stream);
int gsr_points_nearest(gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long Q, const double* query, long long R,
                       const double* ref, double max_dist, double* dist, float* stage_ms, void* stream);

/*
 * Tanks and Temples F-score evaluation (the reference's eval_tnt/run.py, which
 * is open3d on the CPU): the device half, in seven calls.  All points are
 * float64 [n,3]; the arithmetic is float64 without contraction.  No float
 * atomic is used, so every result is the same bits on every run.  Additive: the
 * ABI version is unchanged.  A 4x4 `transform` is 16 host doubles, row-major;
 * only its first three rows are read: p' = ((r0 x + r1 y) + r2 z) + t.
 *
 * gsr_points_crop_polygon (open3d SelectionPolygonVolume::CropInPolygon):
 * `transform` (may be NULL) is applied first.  orthogonal_axis 0 / 1 / 2 = X /
 * Y / Z gives the axes (u, v, w) = (1,2,0) / (0,2,1) / (0,1,2).  A point is
 * dropped when p[w] < axis_min or p[w] > axis_max (both ends are kept).  For
 * every edge (i, j = i + 1 mod M) of polygon [M,3] (host) with
 * (b_i[v] < p[v] && b_j[v] >= p[v]) || (b_j[v] < p[v] && b_i[v] >= p[v]) the
 * node is b_i[u] + (p[v] - b_i[v]) / (b_j[v] - b_i[v]) * (b_j[u] - b_i[u]); the
 * point is kept iff the number of nodes strictly below p[u] is odd.  Outputs
 * once their size is known: kept_alloc the ascending int64 positions [K],
 * point_alloc the kept transformed points [K,3]; *num_kept = K.  scratch_alloc
 * is called once (4 bytes per point plus a scan's temporary).  Limits:
 * N < 2^31, M <= GSR_CROP_MAX_VERTICES (the polygon lives in LDS), else
 * GSR_ERR_ARGS.  Synchronises `stream` once (K).  stage_ms: flags and scan,
 * write.
 *
 * gsr_points_voxel_mean (open3d PointCloud::VoxelDownSample): origin =
 * min_bound - 0.5 voxel, cell = floor((p - origin) / voxel) per axis, one
 * output point per occupied cell = (the sum of its points in input order) /
 * count.  open3d emits in hash-map order, which is no contract; here the cells
 * come ascending in the packed key (cx, cy, cz), x most significant.  Outputs:
 * mean_alloc means [C,3] float64, count_alloc counts [C] int64, cell_alloc
 * cells [C,3] int64; *num_cells = C.  One lane walks one cell's run, however
 * long.  scratch_alloc is called once (20 bytes per point plus the radix
 * sort's temporary).  Limits: N < 2^31, a key of at most 64 bits, finite
 * points, voxel > 0, else GSR_ERR_ARGS.  Synchronises `stream` twice (bounds;
 * C).  stage_ms: bounds, keys, sort, heads and scan, emit.
 *
 * gsr_points_index_build / gsr_points_index_query: gsr_points_nearest in two
 * halves.  build does the ref half once (bounds, density-derived grid, cell
 * sort, gather) into `buffer`, a device block of the caller's of at least
 * gsr_points_index_bytes(R) bytes (36 per point plus alignment), and describes
 * it in *index (host).  There is no hidden state and nothing to free; the
 * index holds a copy of ref's coordinates, and is valid while `buffer` is.
 * query writes dist [Q] as gsr_points_nearest does (the same bits) and
 * nearest [Q] int64: the position in the original ref of the nearest point
 * with distance < max_dist, or -1 with +inf beyond.  Among equally near points
 * the lowest position wins.  build calls scratch_alloc once (8 bytes per ref
 * point plus the sort's temporary) and synchronises `stream` once (bounds);
 * query calls it once (20 bytes per query plus the sort's temporary) and does
 * not synchronise.  stage_ms: build bounds, ref sort; query query sort,
 * search.
 *
 * gsr_icp_accumulate: the sums of point-to-point ICP over the pairs
 * (src[i], ref[index[i]]) with index[i] >= 0; index [N] int64 in [-1, R).
 * pass 1 -> sums[8] (host) = n, sum |s - t|^2, sum s (3), sum t (3).  pass 2
 * takes means[6] (host; the caller's sum s / n, sum t / n) -> sums[10] =
 * sum (s - m_s)(t - m_t)^T (9, row-major), sum |s - m_s|^2.  A fixed-shape
 * tree reduction (a function of N alone).  scratch_alloc is called once
 * (about 45 KB).  Synchronises `stream` once per pass.  stage_ms: sums.
 *
 * gsr_points_transform: points [N,3] <- transform, in place.  stage_ms:
 * transform.
 */
#define GSR_CROP_MAX_VERTICES 1024
typedef struct gsr_point_index {
    long long R;         /* points indexed */
    void* buffer;        /* the caller's device block */
    double bounds_min[3], bounds_max[3];
    double cell_size;
    long long cells[3];  /* per axis */
    int key_bits[3];
} gsr_point_index;
int gsr_points_crop_polygon(gsr_alloc_fn kept_alloc, void* kept_ctx, gsr_alloc_fn point_alloc, void* point_ctx,
                            gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long N, const double* points,
                            const double* transform, int orthogonal_axis, double axis_min, double axis_max,
                            int num_vertices, const double* polygon, long long* num_kept, float* stage_ms,
                            void* stream);
int gsr_points_voxel_mean(gsr_alloc_fn mean_alloc, void* mean_ctx, gsr_alloc_fn count_alloc, void* count_ctx,
                          gsr_alloc_fn cell_alloc, void* cell_ctx, gsr_alloc_fn scratch_alloc, void* scratch_ctx,
                          long long N, const double* points, double voxel, long long* num_cells, float* stage_ms,
                          void* stream);
size_t gsr_points_index_bytes(long long R);
int gsr_points_index_build(gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long R, const double* ref, void* buffer,
                           size_t buffer_bytes, gsr_point_index* index, float* stage_ms, void* stream);
int gsr_points_index_query(gsr_alloc_fn scratch_alloc, void* scratch_ctx, const gsr_point_index* index, long long Q,
                           const double* query, double max_dist, double* dist, long long* nearest, float* stage_ms,
                           void* stream);
int gsr_icp_accumulate(gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long N, const double* src, long long R,
                       const double* ref, const long long* index, int pass, const double* means, double* sums,
                       float* stage_ms, void* stream);
int gsr_points_transform(long long N, double* points, const double* transform, float* stage_ms, void* stream);

/*
 * Tanks and Temples mesh culling (the reference's eval_tnt/cull_mesh.py, which
 * renders with pyrender / OpenGL): the depth map of a triangle mesh from one
 * pinhole view, and the per-vertex count of the views that see a vertex.
 * vertices [V,3] float32 and faces [F,3] int32 or int64 (faces_int64) are device
 * memory; w2c / w2cs are HOST float32, one row-major 3x4 world -> camera matrix
 * per view (x right, y down, z forward).
 *
 * gsr_mesh_depth: depth [H,W] float32 (device) = the smallest camera-space z in
 * [znear, zfar] at which the ray through the pixel centre (j + 0.5, i + 0.5)
 * meets a triangle, 0 where it meets none.  Both facings count, edges are
 * inclusive, degenerate triangles cover nothing, a triangle that crosses znear
 * or z = 0 contributes its part inside the slab.  float32 in a fixed operation
 * order without fused multiply-add; the winner per pixel is an
 * integer minimum, so the map is the same bits for any face order and on every
 * run.  stage_ms: clear, set-up and small triangles, unit scan, wave units,
 * finish.
 *
 * gsr_mesh_view_votes: counts [V] int32 (device) = the number of the n_views
 * views with 0 <= u <= W - 1, 0 <= v <= H - 1, z > 0 and (d <= 0 or z < d + eps),
 * where z = z_cam + 1e-8, (u, v) = K p_cam / z and d is the bilinear sample of
 * that view's depth map at (u, v) (integer coordinates are pixel indices, the
 * border repeated, empty pixels blended in as 0).  The views are rendered one
 * after another into one depth buffer on `stream`; nothing is read back
 * between them.  stage_ms: the same stages summed over the views, then the
 * vote.
 *
 * Both return GSR_ERR_ARGS unless 1 <= H, W <= 16384, fx, fy > 0,
 * 0 < znear <= zfar and every camera number (and eps) is finite.
 * Both call scratch_alloc once (4 bytes per pixel, 12 per triangle, the scan's
 * temporary) and synchronise `stream` once, at the end: a face that names a
 * vertex outside [0, V) is GSR_ERR_ARGS.  `counters` (host, optional, 4 words;
 * measurement only, it selects slower counting kernels): atomics issued, pixel
 * centres tested, triangles drawn by one lane, wave units.
 */
int gsr_mesh_depth(gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long V, const float* vertices, long long F,
                   const void* faces, int faces_int64, const float* w2c, int H, int W, float fx, float fy, float cx,
                   float cy, float znear, float zfar, float* depth, unsigned long long* counters, float* stage_ms,
                   void* stream);
int gsr_mesh_view_votes(gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long V, const float* vertices, long long F,
                        const void* faces, int faces_int64, int n_views, const float* w2cs, int H, int W, float fx,
                        float fy, float cx, float cy, float znear, float zfar, float eps, int* counts,
                        unsigned long long* counters, float* stage_ms, void* stream);

/*
 * Per-stage GPU timing (no reference equivalent; SURVEY §5 "tracing").  While
 * enabled, every kernel stage of the calls above is bracketed by two hipEvents
 * on the call's stream.  gsr_timing_collect() waits for the recorded events,
 * adds each stage's total milliseconds and launch count into the caller's
 * arrays (length GSR_NUM_STAGES, indexed by enum gsr_stage) and clears the
 * record.  Process-wide, thread-safe.
 */
enum gsr_stage {
    GSR_STAGE_PREPROCESS = 0,
    GSR_STAGE_SCAN,
    GSR_STAGE_EMIT_KEYS, /* (grids > 1024 tiles a side) instance emission for the tile-id sort */
    GSR_STAGE_SORT,      /* (grids > 1024 tiles a side) stable tile-id sort */
    GSR_STAGE_TILE_RANGES, /* (grids > 1024 tiles a side) */
    GSR_STAGE_RENDER_FWD,
    GSR_STAGE_BWD_CLEAR,
    GSR_STAGE_RENDER_BWD,
    GSR_STAGE_PREPROCESS_BWD,
    GSR_STAGE_DEPTH_ORDER, /* stable depth sort of the Gaussians (binning.hip) */
    GSR_STAGE_TILE_LISTS,  /* per-tile lists without an instance sort (tilelists.hip; grids <= 1024^2 tiles) */
    GSR_STAGE_SAMPLE_POINTS, /* sample_depth: point projection, per-tile point lists and chunks (sample.hip) */
    GSR_STAGE_SAMPLE_FWD,    /* sample_depth forward raster (render_fwd.hip, SAMPLE mode) */
    GSR_STAGE_SAMPLE_BWD,    /* sample_depth backward raster + point projection backward (sample.hip) */
    GSR_NUM_STAGES
};
int gsr_timing_enable(int on);
/* Restrict the timing to the stages whose bit (1 << enum gsr_stage) is set
 * (default: all).  Each recorded event costs the stream ~10 us of idle time,
 * so a throughput measurement times only the stage it reports. */
int gsr_timing_stage_mask(unsigned int mask);
int gsr_timing_collect(double* ms, int* launches);
const char* gsr_stage_name(int stage);

/*
 * Process-wide switches selecting the alternative kernel paths the parity
 * tests use as references for the default ones (all but GSR_OPT_NO_REFINE
 * give bit-identical results) and the forward's diagnostic counters.  Ids 0,
 * 2-4, 7 and 8 belonged to retired variants and diagnostics (a bisection
 * shortcut, bisection-pass and pre-pass timing switches, an unordered tile
 * launch, per-tile sort binning, a two-wave backward layout) and are rejected
 * with GSR_ERR_ARGS.
 */
/* GSR_OPT_BWD_NO_CACHE (A/B, default 0): the backward recomputes dT/dt_m at every
 * pixel in its pre-pass (render_backward.cu:835-880) instead of taking the
 * forward's cached value. */
/* GSR_OPT_ROCPRIM_DSORT (A/B, default 0): the depth order by rocPRIM's onesweep
 * radix sort instead of dsort.hip's (same order). */
/* GSR_OPT_PBWD_STAGE (A/B): the per-Gaussian backward's SH / SG-7 gradient rows
 * written through LDS as whole-wave stores (1) or per lane (2); 0 = the build's
 * default (GSR_PBWD_STAGE_DEFAULT). */
/* GSR_OPT_NO_REFINE (A/B, default 0): find the median depth with the reference's
 * five bisection passes only, instead of two passes plus the bracketed Halley
 * refinement (render_fwd.hip; results agree to ~1e-7 of the depth, not bitwise). */
enum gsr_option {
    GSR_OPT_RENDER_STATS = 1,
    GSR_OPT_NO_REFINE = 5,
    GSR_OPT_BWD_NO_CACHE = 6,
    GSR_OPT_ROCPRIM_DSORT = 9,
    GSR_OPT_PBWD_STAGE = 10
};
int gsr_set_option(int opt, int value);
/* Diagnostic counters of GSR_OPT_RENDER_STATS forward launches (20 values, see render_fwd.hip). */
int gsr_debug_render_stats(unsigned long long* out20, int reset);

/*
 * Introspection of a forward's opaque buffers (test hook, no reference
 * equivalent): copies the per-tile depth-ordered Gaussian list (R entries,
 * R = num_rendered) and the tile ranges (2 x tiles uint32, tiles =
 * ceil(W/16) * ceil(H/16)) to host memory; synchronises `stream`.
 */
int gsr_debug_binning(const void* binning_buffer, const void* tile_buffer, int R, int width, int height,
                      uint32_t* point_list_out, uint32_t* ranges_out, void* stream);

/*
 * Introspection of a forward's image buffer (test hook): the per-pixel last
 * contributor (1-based index into the pixel's tile list, which holds only the
 * instances that survive tile culling, see gsr_debug_binning), W x H uint32
 * row-major; synchronises `stream`.
 */
int gsr_debug_image(const void* image_buffer, int width, int height, uint32_t* n_contrib_out, void* stream);

/*
 * Introspection of a sample_depth forward's point buffer (test hook): the
 * per-point median depth along the ray and last contributor (index into the
 * culled per-tile list) for PN points; synchronises `stream`.
 */
int gsr_debug_sample_points(const void* point_buffer, int PN, float* median_depth_out, uint32_t* last_out,
                            void* stream);

/*
 * Introspection of a forward's tile buffer (test / measurement hook): the
 * per-tile max contributor (the last list position any pixel of the tile
 * blended, 1-based; the backward walks each tile's list up to it), one
 * uint32 per tile; synchronises `stream`.
 */
int gsr_debug_tile_stats(const void* tile_buffer, int width, int height, uint32_t* max_contrib_out, void* stream);

/*
 * The depth sort on the caller's keys (test hook, no reference equivalent;
 * additive to ABI 20).  All pointers but `stream` are device memory.
 */
/* host only: keys per dsort.hip workgroup tile for P keys (6144, or 12288 above 2,000,000); -1 for P < 0 */
int gsr_debug_depth_sort_tile_keys(int P);
/* bytes of `scratch` for P keys; -1 for P < 0 */
long long gsr_debug_depth_sort_bytes(int P);
/* order[P], keys_sorted[P] = the stable sort of keys[P] (values = index), by launch_depth_sort:
 * dsort.hip, or rocPRIM under GSR_OPT_ROCPRIM_DSORT.
 * prepared != 0: as the render path, with the state cleared up front (dsort_zero_region) and the
 * histograms from count_k_hist_kernel over a zeroed tiles_touched, then launch_depth_sort(..., true).
 * prepared == 0: the sort's own zero and histogram kernels.
 * P == 0 succeeds and writes nothing.  Stream-ordered, no host synchronisation. */
int gsr_debug_depth_sort(int P, const uint32_t* keys, uint32_t* keys_sorted, uint32_t* order,
                         void* scratch, int prepared, void* stream);

/*
 * The tile-list binning (csrc/tilelists.hip) for its tests (test hooks, no
 * reference equivalent; additive to ABI 20).
 */
/* host only: the structural constants of tilelists.hip, in this order: kRowSeg, kRowSegBig, kRowSegBigP,
 * kTileSeg, kRecSpans, kCoopCap, kEmitCapW, kEmitPlanes, kCoopMaxGx, kCoopBlocks, kTileBlocks, kScanTile,
 * kScanItems, kMaxGrid.  Writes the first min(n, 14) into out and returns their number (14); -1 for n < 0 or
 * a missing `out`. */
int gsr_debug_list_constants(int* out, int n);
/* bytes of `sums` for a bound of `cap` words; -1 for cap < 0 or cap >= 2^31 */
long long gsr_debug_scan_excl_bytes(long long cap);
/* launch_scan_excl alone: out[0, n) = the exclusive prefix sums (mod 2^32) of in[0, n) and out[n] = their total,
 * with n = n_dev ? mul * *n_dev (read on the device) : n_host; n <= cap, the host's bound, which sizes the
 * launch.  in: cap words, 16-byte aligned, of which only [0, n) are read; out: cap + 1 words, of which only
 * [0, n] are written; sums: gsr_debug_scan_excl_bytes(cap) bytes of scratch.  All pointers but `stream` are
 * device memory.  Stream-ordered, no host synchronisation. */
int gsr_debug_scan_excl(const uint32_t* in, uint32_t* out, long long cap, uint32_t n_host, const uint32_t* n_dev,
                        uint32_t mul, void* sums, void* stream);

/*
 * Densification (csrc/densify.hip): GaussianModel.densify_and_prune
 * (scene/gaussian_model.py:797-816 with its clone / split / prune helpers),
 * compute_3D_filter (:225-262) and reset_opacity (:521-539).  Additive to
 * ABI 20.
 *
 * gsr_densify_plan takes the statistics ([P] each), `_scaling` [P,3],
 * `_opacity` [P] and the scalars max_grad, min_opacity and
 * percent_dense * extent; on the device it forms grads = accum / denom (NaN
 * -> 0), ratio = mean(grads >= max_grad), Q = quantile(grads_abs, 1 - ratio)
 * (torch's linear rule in fp32, by radix select), the reference's clone /
 * split / opacity-prune decisions for every original point and the scans that
 * place every surviving or new point.  It synchronises `stream` once to read
 * counts = {C clones, S split selections (clones that are split again
 * included), points removed by the opacity prune, N final points}; Q (host,
 * may be NULL) receives the quantile.  `workspace` is device memory of
 * gsr_densify_workspace_bytes(P) bytes (-1: P out of range; P <= (2^31 - 1) / 5)
 * that the following gsr_densify_apply reads.
 *
 * gsr_densify_apply writes the new tensors: final layout [surviving originals
 * | surviving clones | surviving split children, copy 0 | copy 1], each in
 * source order.  `counts` as the plan returned them; `map` is device memory
 * of 3 N int32, filled when build_map is non-zero and read otherwise (a caller
 * that gathers one parameter per call, freeing each source as it goes to bound
 * the peak memory, builds it in the first call); `noise` [noise_rows, 3] standard-normal draws with
 * noise_rows == C + 2 S (clones take rows [0, C), the children of the k-th
 * selected point rows C + k and C + S + k); `rotation` [P,4] and `scaling`
 * [P,3] are the source `_rotation` and `_scaling` (read by GSR_DENSIFY_XYZ
 * descriptors only).  Each descriptor gathers
 * one [P, width] parameter (and its Adam moments, or neither) into [N, width]
 * outputs, every element written once: survivors keep parameter and moments,
 * new points copy the parameter with zero moments, except GSR_DENSIFY_XYZ
 * (new position R(q / |q|) (exp(s) * noise) + source position; the source of
 * a clone's child is the clone's new position) and GSR_DENSIFY_SCALING
 * (children: log(exp(s) / 1.6)).  Counts that are inconsistent, a noise buffer
 * of another size or an incomplete descriptor fail the call; counts that are
 * not those of the plan in `workspace` make the kernels write nothing.
 * The result is the same bits on every run.
 */
enum gsr_densify_role { GSR_DENSIFY_COPY = 0, GSR_DENSIFY_XYZ = 1, GSR_DENSIFY_SCALING = 2 };
typedef struct gsr_densify_param {
    const float* param;
    const float* exp_avg;
    const float* exp_avg_sq;
    float* param_out;
    float* exp_avg_out;
    float* exp_avg_sq_out;
    int width; /* floats per row */
    int role;  /* enum gsr_densify_role */
} gsr_densify_param;
long long gsr_densify_workspace_bytes(long long P);
int gsr_densify_plan(long long P, const float* xyz_gradient_accum, const float* xyz_gradient_accum_abs,
                     const float* denom, const float* scaling, const float* opacity, float max_grad,
                     float min_opacity, float pd_extent, void* workspace, long long* counts, float* Q, void* stream);
int gsr_densify_apply(long long P, const long long* counts, void* workspace, int32_t* map, int build_map,
                      const float* noise, long long noise_rows, const float* rotation, const float* scaling, int n_params,
                      const gsr_densify_param* params, void* stream);

/*
 * torch.quantile(values, q) with linear interpolation for n non-negative,
 * non-NaN fp32 values and a device scalar q in [0, 1]: rank = q (n - 1) in
 * fp32, the order statistics at floor and ceil of it by a radix select over
 * the bit patterns (no sort, no limit on n), then ATen's lerp.  `out` is a
 * device float; `workspace` device memory of gsr_quantile_workspace_bytes().
 */
long long gsr_quantile_workspace_bytes(void);
int gsr_quantile(long long n, const float* values, const float* q, float* out, void* workspace, void* stream);

/*
 * compute_3D_filter: `cameras` is device memory of n_cam records of 14
 * floats: R (3x3 row-major as the reference stores it, p_cam = p R + T), T,
 * image_width / Fx * 0.575, image_height / Fy * 0.575.  filter_3D [P]
 * receives (smallest depth over the cameras that see the point; for unseen
 * points the largest such depth) / max_focal * sqrt(0.2).  Fails with
 * GSR_ERR_ARGS when no camera sees any point (the reference raises there).
 * `scratch4`: 4 bytes of device memory.  Synchronises `stream` once.
 */
int gsr_filter_3d(long long P, const float* xyz, int n_cam, const float* cameras, float max_focal, float* filter_3D,
                  void* scratch4, void* stream);

/*
 * reset_opacity: opacity_out = inverse_sigmoid(min(sigmoid(o) coef, 0.01) / coef),
 * coef = sqrt(prod exp(s)^2 / prod (exp(s)^2 + filter_3D^2)); the two moment
 * outputs (both or neither) are zeroed.
 */
int gsr_reset_opacity(long long P, const float* scaling, const float* opacity, const float* filter_3D,
                      float* opacity_out, float* exp_avg_out, float* exp_avg_sq_out, void* stream);

/*
 * Image-quality evaluation (the reference's render.py -> metric.py, and the
 * test report of train.py:332-365).  Images are [N,C,H,W] fp32 planes.
 *
 * gsr_image_quantize8: the byte image torchvision's save_image hands to the
 * PNG writer, out [N,H,W,C] (4-byte aligned):
 *   byte = trunc(clamp(fl(fl(x * 255) + 0.5), 0, 255)),
 * the multiply and the add rounded separately in fp32 (never fused); NaN and
 * -inf give 0, +inf 255.
 *
 * gsr_image_metrics: out [N,3] float64 (device) receives per image
 * {l1, mse, ssim} of render against gt, each input read once.
 *   quantize != 0: both images go through the rule above and are compared as
 *     fl(byte / 255), what PIL and to_tensor read back; the sums are exact
 *     integers, l1 = S1 / (255 n), mse = S2 / (65025 n), n = C H W.
 *     render_bytes / gt_bytes (each NULL or [N,H,W,C], 4-byte aligned, C <= 4)
 *     receive the byte images from the same read.
 *   quantize == 0: both images are clamped to [0, 1], differences in fp32,
 *     sums in float64.
 *   with_ssim != 0: ssim is the mean of the reference's SSIM map (11 x 11
 *     Gaussian window, sigma 1.5, C1 = 1e-4, C2 = 9e-4) over the C (H-10)
 *     (W-10) windows inside that image, on the compared values; needs H, W
 *     >= 11.  Otherwise ssim = 0 and any H, W >= 1 is accepted.
 * Per-workgroup partials and a fixed-order finish per image: no atomics, an
 * image's numbers do not depend on the rest of the batch.  Asynchronous on
 * `stream`; PSNR = -10 log10(mse) is the caller's.
 */
int gsr_image_quantize8(long long N, int C, int H, int W, const float* image, uint8_t* out, void* stream);
int gsr_image_metrics(gsr_alloc_fn scratch_alloc, void* scratch_ctx, int N, int C, int H, int W, int quantize,
                      int with_ssim, const float* render, const float* gt, uint8_t* render_bytes, uint8_t* gt_bytes,
                      double* out, void* stream);

/*
 * View preparation (the reference's loadCam -> PILtoTorch -> Camera.__init__):
 * PIL.Image.resize's 8-bit bicubic resample, byte for byte, and the float
 * planes of the resized bytes.  Byte images are [N,H,W,C], C = 1..4.
 *
 * gsr_resample_ksize: the taps of one window, ceil(2 max(in/out, 1)) * 2 + 1.
 *
 * gsr_resample_coeffs (host only, float64): Pillow's table of one axis for
 * the bicubic filter (a = -0.5).  k [out_size][ksize] receives the weights
 * normalised to sum 1 and rounded to 22 fractional bits (0 past a window's
 * count), bounds [out_size][2] each window's (first input index, count).
 *
 * gsr_image_resample8: one pass along `axis` (1: W, 0: H) to `out_size`,
 *   out byte = clip8((2^21 + sum in byte * k) >> 22)  in int32.
 * `k` and `bounds` are DEVICE copies of that axis' table, k transposed to
 * tap-major [ksize][out_size].  `in` and `out` must not overlap.  A resize
 * is the pass along W, then the pass along H on its bytes; a pass that
 * keeps its size is not run.  No atomics: an image's bytes do not depend on
 * the batch.  Asynchronous on `stream`.
 *
 * gsr_view_planes: rgb [N,H,W,3] (and mask [N,H,W] or NULL) ->
 *   original [N,3,H,W] = fl(byte / 255), an IEEE divide;
 *   gray [N,1,H,W] = fl(fl(fl(0.299f r) + fl(0.587f g)) + fl(0.114f b));
 *   gt_mask [N,1,H,W] = fl(mask byte / 255) (ignored when mask is NULL),
 * one launch, asynchronous on `stream`.
 */
int gsr_resample_ksize(int in_size, int out_size);
int gsr_resample_coeffs(int in_size, int out_size, int32_t* k, int32_t* bounds);
int gsr_image_resample8(long long N, int H, int W, int C, int axis, int out_size, const uint8_t* in, uint8_t* out,
                        const int32_t* k, const int32_t* bounds, void* stream);
int gsr_view_planes(long long N, int H, int W, const uint8_t* rgb, const uint8_t* mask, float* original, float* gray,
                    float* gt_mask, void* stream);

/*
 * Model files (the reference's save_ply / load_ply, scene/gaussian_model.py:
 * 450-493 and 541-611): the vertex rows of point_cloud.ply packed from, and
 * unpacked into, the ten stored tensors
 *   xyz [P,3], features_dc [P,1,3], features_rest [P,M-1,3], opacity [P,1],
 *   scaling [P,3], rotation [P,4], sg_axis [P,G,3], sg_sharpness [P,G],
 *   sg_color [P,G,3], filter_3D [P,1]            (float32, contiguous).
 * A canonical row is A = gsr_model_row_floats(M, G) = 18 + 3 (M-1) + 7 G
 * float32 columns in save_ply's property order:
 *   x y z, nx ny nz (zeros), f_dc_0..2, f_rest_*, opacity, scale_0..2,
 *   rot_0..3, sg_axis_*, sg_sharpness_*, sg_color_*, filter_3D,
 * each block the plain flatten of its tensor's row except
 *   f_rest_{c (M-1) + k} = features_rest[p, k, c]   (transpose(1,2).flatten(1)).
 * Both kernels copy bits: NaN payloads, -0, infinities and denormals pass.
 *
 * gsr_model_row_floats (host only): A, or 0 for M outside [1, 2^20] or G
 * outside [0, 2^20].
 * gsr_model_block_rows (host only): the rows one workgroup of the pack kernel
 * owns for rows of A floats (a block seam falls every that many rows), or 0
 * when a single row does not fit its tile (A > 8192).
 *
 * gsr_model_unpack_block_rows (host only): the same for the unpack kernel and
 * file rows of `stride` bytes, or 0 when a row does not fit (stride > 32736).
 *
 * gsr_model_pack_rows: rows [P,A].  A tensor without columns (features_rest
 * at M = 1, the sg_* at G = 0) may be NULL.  One launch, no temporaries.
 *
 * gsr_model_unpack_rows: the inverse from file rows of `stride` bytes, any
 * positive number (not necessarily a multiple of 4), at `rows` (16-byte
 * aligned, P stride bytes; no byte outside them is read).  col_offset and
 * col_type are DEVICE tables of A entries: the byte offset of each canonical
 * column inside a file row, -1 for a column the file does not have (it reads
 * as 0), and its type, 0 = float32 (bits copied) or 1 = float64 (converted
 * round-to-nearest-even).  Columns nx ny nz are not stored anywhere; their
 * entries are ignored.  The tables are read back and checked before the
 * launch (the call waits for `stream` once): an offset below -1, a type other
 * than 0 or 1, or a column that ends past `stride` is GSR_ERR_ARGS.
 *
 * P = 0 is GSR_OK without a launch; a row too long for a tile is
 * GSR_ERR_ARGS.  Asynchronous on `stream` but for the table check.
 */
int gsr_model_row_floats(int M, int G);
int gsr_model_block_rows(int A);
int gsr_model_unpack_block_rows(long long stride);
int gsr_model_pack_rows(long long P, int M, int G, const float* xyz, const float* features_dc,
                        const float* features_rest, const float* opacity, const float* scaling, const float* rotation,
                        const float* sg_axis, const float* sg_sharpness, const float* sg_color, const float* filter_3D,
                        float* rows, void* stream);
int gsr_model_unpack_rows(long long P, int M, int G, long long stride, const uint8_t* rows, const int32_t* col_offset,
                          const int32_t* col_type, float* xyz, float* features_dc, float* features_rest,
                          float* opacity, float* scaling, float* rotation, float* sg_axis, float* sg_sharpness,
                          float* sg_color, float* filter_3D, void* stream);

/* Human-readable message for the last non-OK status on this thread. */
const char* gsr_last_error(void);

/* ABI version of this header (bumped on any signature or enum change). */
int gsr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GSR_H_INCLUDED */
