// api_train.hip — the C ABI (include/gsr.h) of the training step outside the rasteriser: the
// optimiser and densification statistics, the colour gradients over views, the multi-view terms
// (NCC, PatchMatch, SSIM, the fused photometric loss, depth to normal), the parameter getters, the nearest-neighbour distance
// and the device-side densify / prune, 3D filter and opacity reset.  Host orchestration only.
#include <vector>

#include "gsr_api_common.h"

using namespace gsr;

extern "C" {

int gsr_adam_step(int n_groups, const gsr_adam_group* groups, double step, double beta1, double beta2, double eps,
                  void* stream_ptr) {
    if (n_groups < 0 || n_groups > kMaxAdamGroups || (n_groups > 0 && !groups) || !(step >= 1.0))
        return fail(GSR_ERR_ARGS, "adam: 0..16 groups and step >= 1");
    AdamGroup g[kMaxAdamGroups];
    double lr[kMaxAdamGroups];
    for (int k = 0; k < n_groups; k++) {
        const gsr_adam_group& s = groups[k];
        if (s.n < 0 || (s.n > 0 && (!s.param || !s.grad || !s.exp_avg || !s.exp_avg_sq)))
            return fail(GSR_ERR_ARGS, "adam: missing group buffer");
        g[k].param = s.param;
        g[k].grad = s.grad;
        g[k].exp_avg = s.exp_avg;
        g[k].exp_avg_sq = s.exp_avg_sq;
        g[k].n = s.n;
        const uintptr_t bits = (uintptr_t)s.param | (uintptr_t)s.grad | (uintptr_t)s.exp_avg | (uintptr_t)s.exp_avg_sq;
        g[k].aligned = (bits & 15u) == 0;
        lr[k] = s.lr;
    }
    hipError_t e = launch_adam(n_groups, g, lr, step, beta1, beta2, eps, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "adam", e);
}

int gsr_densify_stats(int P, const float* vgrad, const int* radii, float* max_radii2D, float* accum,
                      float* accum_abs, float* denom, void* stream_ptr) {
    if (P < 0 || (P > 0 && (!vgrad || !radii || !max_radii2D || !accum || !accum_abs || !denom)))
        return fail(GSR_ERR_ARGS, "densify stats: invalid arguments");
    hipError_t e = launch_densify_stats(P, vgrad, radii, max_radii2D, accum, accum_abs, denom, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "densify stats", e);
}

int gsr_view_color_grads_chunked(int P, int sh_degree, int SHM, int sg_degree, int SGM, int n_views, int chunk,
                                 const float* gathered, const float* campos, const float* means3D,
                                 const float* sg_axis, const float* sg_sharpness, const float* sg_color,
                                 float* dL_dsh, float* dL_dsg_axis, float* dL_dsg_sharpness, float* dL_dsg_color,
                                 float* dL_dsh_rest, void* stream_ptr) {
    if (P < 0 || n_views < 1 || chunk < 1 || sh_degree < 0 || sh_degree > 3 ||
        SHM < (sh_degree + 1) * (sh_degree + 1) || SGM < 0 || sg_degree < 0 || sg_degree > 7 || sg_degree > SGM ||
        (dL_dsh_rest && SHM < 2))
        return fail(GSR_ERR_ARGS, "view colour grads: invalid arguments");
    if (P > 0 && (!gathered || !campos || !means3D || !dL_dsh ||
                  (SGM > 0 && (!dL_dsg_axis || !dL_dsg_sharpness || !dL_dsg_color)) ||
                  (sg_degree > 0 && (!sg_axis || !sg_sharpness || !sg_color))))
        return fail(GSR_ERR_ARGS, "view colour grads: missing buffer");
    hipError_t e = launch_view_color_grads(P, sh_degree, SHM, sg_degree, SGM, n_views, gathered, means3D, sg_axis,
                                           sg_sharpness, sg_color, dL_dsh, dL_dsg_axis, dL_dsg_sharpness,
                                           dL_dsg_color, (hipStream_t)stream_ptr, chunk, campos, dL_dsh_rest);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "view colour grads", e);
}

int gsr_view_color_grads(int P, int sh_degree, int SHM, int sg_degree, int SGM, int n_views, const float* gathered,
                         const float* means3D, const float* sg_axis, const float* sg_sharpness, const float* sg_color,
                         float* dL_dsh, float* dL_dsg_axis, float* dL_dsg_sharpness, float* dL_dsg_color,
                         void* stream_ptr) {
    if (P < 0 || n_views < 1 || sh_degree < 0 || sh_degree > 3 || SHM < (sh_degree + 1) * (sh_degree + 1) ||
        SGM < 0 || sg_degree < 0 || sg_degree > 7 || sg_degree > SGM)
        return fail(GSR_ERR_ARGS, "view colour grads: invalid arguments");
    if (P > 0 && (!gathered || !means3D || !dL_dsh ||
                  (SGM > 0 && (!dL_dsg_axis || !dL_dsg_sharpness || !dL_dsg_color)) ||
                  (sg_degree > 0 && (!sg_axis || !sg_sharpness || !sg_color))))
        return fail(GSR_ERR_ARGS, "view colour grads: missing buffer");
    hipError_t e = launch_view_color_grads(P, sh_degree, SHM, sg_degree, SGM, n_views, gathered, means3D, sg_axis,
                                           sg_sharpness, sg_color, dL_dsh, dL_dsg_axis, dL_dsg_sharpness,
                                           dL_dsg_color, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "view colour grads", e);
}

int gsr_warp_patch_ncc(int P, const float* depths, const float* normals, const int* uvs, const float* R,
                       const float* T, const float* image_r, const float* image_n, float fx_r, float fy_r,
                       float cx_r, float cy_r, float fx_n, float fy_n, float cx_n, float cy_n, int image_height_r,
                       int image_width_r, int image_height_n, int image_width_n, float* ncc, float* grad_depths,
                       float* grad_normals, uint8_t* valid, void* stream_ptr) {
    if (P < 0 || image_height_r <= 0 || image_width_r <= 0 || image_height_n <= 0 || image_width_n <= 0)
        return fail(GSR_ERR_ARGS, "warp_patch_ncc: invalid sizes");
    if (P > 0 && (!depths || !normals || !uvs || !R || !T || !image_r || !image_n || !ncc || !grad_depths ||
                  !grad_normals || !valid))
        return fail(GSR_ERR_ARGS, "warp_patch_ncc: missing buffer");
    NccParams q{P, depths, normals, uvs, R, T, image_r, image_n, fx_r, fy_r, cx_r, cy_r, fx_n, fy_n, cx_n, cy_n,
                image_height_r, image_width_r, image_height_n, image_width_n, ncc, grad_depths, grad_normals, valid};
    hipError_t e = launch_ncc(q, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "warp_patch_ncc", e);
}

int gsr_scale_opacity_3d_filter(int P, const float* scaling, const float* opacity, const float* filter_3D,
                                float* scales, float* opacities, void* stream_ptr) {
    if (P < 0 || (P > 0 && (!scaling || !opacity || !filter_3D || !scales || !opacities)))
        return fail(GSR_ERR_ARGS, "scale/opacity getter: invalid arguments");
    hipError_t e = launch_scale_opacity(P, scaling, opacity, filter_3D, scales, opacities, nullptr, nullptr, nullptr,
                                        nullptr, false, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "scale/opacity getter", e);
}

int gsr_scale_opacity_3d_filter_backward(int P, const float* scaling, const float* opacity, const float* filter_3D,
                                         const float* dL_dscales, const float* dL_dopacities, float* dL_dscaling,
                                         float* dL_dopacity, void* stream_ptr) {
    if (P < 0 || (P > 0 && (!scaling || !opacity || !filter_3D || !dL_dscaling || !dL_dopacity)))
        return fail(GSR_ERR_ARGS, "scale/opacity getter backward: invalid arguments");
    hipError_t e = launch_scale_opacity(P, scaling, opacity, filter_3D, nullptr, nullptr, dL_dscales, dL_dopacities,
                                        dL_dscaling, dL_dopacity, true, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "scale/opacity getter backward", e);
}

int gsr_normalize_rows(int n, int D, const float* x, float* y, void* stream_ptr) {
    if (n < 0 || D <= 0 || (n > 0 && (!x || !y))) return fail(GSR_ERR_ARGS, "normalize: invalid arguments");
    hipError_t e = launch_normalize_rows(n, D, x, nullptr, y, false, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "normalize", e);
}

int gsr_normalize_rows_backward(int n, int D, const float* x, const float* dL_dy, float* dL_dx, void* stream_ptr) {
    if (n < 0 || D <= 0 || (n > 0 && (!x || !dL_dy || !dL_dx)))
        return fail(GSR_ERR_ARGS, "normalize backward: invalid arguments");
    hipError_t e = launch_normalize_rows(n, D, x, dL_dy, dL_dx, true, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "normalize backward", e);
}

int gsr_patchmatch_lift(int H, int W, float Fx, float Fy, float Cx, float Cy, const float* T, const float* M,
                        const float* median_depth, float* points, void* stream_ptr) {
    if (H < 0 || W < 0 || (H * W > 0 && (!T || !M || !median_depth || !points)))
        return fail(GSR_ERR_ARGS, "patchmatch lift: invalid arguments");
    hipError_t e = launch_patchmatch_lift(false, H, W, Fx, Fy, Cx, Cy, T, M, median_depth, nullptr, points,
                                          (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "patchmatch lift", e);
}

int gsr_patchmatch_lift_backward(int H, int W, float Fx, float Fy, float Cx, float Cy, const float* M,
                                 const float* dL_dpoints, float* dL_dmedian_depth, void* stream_ptr) {
    if (H < 0 || W < 0 || (H * W > 0 && (!M || !dL_dpoints || !dL_dmedian_depth)))
        return fail(GSR_ERR_ARGS, "patchmatch lift backward: invalid arguments");
    hipError_t e = launch_patchmatch_lift(true, H, W, Fx, Fy, Cx, Cy, nullptr, M, nullptr, dL_dpoints,
                                          dL_dmedian_depth, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "patchmatch lift backward", e);
}

static const char* pm_check(int H, int W, const float* md, const float* normal, const float* pin,
                            const uint8_t* inside, const float* Mv, const float* tv, const float* R, const float* T,
                            const float* image_r, const float* image_n, int Hn, int Wn, const float* saved_w,
                            const uint8_t* saved_flags, const float* saved_gd, const float* saved_gn) {
    if (H <= 0 || W <= 0 || Hn <= 0 || Wn <= 0) return "patchmatch: invalid sizes";
    if (!md || !normal || !pin || !inside || !Mv || !tv || !R || !T || !image_r || !image_n || !saved_w ||
        !saved_flags || !saved_gd || !saved_gn)
        return "patchmatch: missing buffer";
    return nullptr;
}

int gsr_patchmatch_terms_forward(gsr_alloc_fn scratch_alloc, void* scratch_ctx, int H, int W,
                                 const float* median_depth, const float* normal, const float* points_nearest,
                                 const uint8_t* inside, const float* Mv, const float* tv, float Fx, float Fy, float Cx,
                                 float Cy, float noise_th, const float* R, const float* T, const float* image_r,
                                 const float* image_n, float fx_r, float fy_r, float cx_r, float cy_r, float fx_n,
                                 float fy_n, float cx_n, float cy_n, int image_height_n, int image_width_n,
                                 float* saved_w, uint8_t* saved_flags, float* saved_gd, float* saved_gn,
                                 float* out4, void* stream_ptr) {
    if (const char* m = pm_check(H, W, median_depth, normal, points_nearest, inside, Mv, tv, R, T, image_r, image_n,
                                 image_height_n, image_width_n, saved_w, saved_flags, saved_gd, saved_gn))
        return fail(GSR_ERR_ARGS, m);
    if (!out4 || !scratch_alloc) return fail(GSR_ERR_ARGS, "patchmatch: missing buffer");
    void* buf = scratch_alloc(scratch_ctx, patchmatch_partials(H, W) * sizeof(float) + 256);
    if (!buf) return fail(GSR_ERR_ALLOC, "patchmatch: scratch allocation failed");
    PatchMatchParams q{H, W, median_depth, normal, points_nearest, inside, Mv, tv, Fx, Fy, Cx, Cy, noise_th, R, T,
                       image_r, image_n, fx_r, fy_r, cx_r, cy_r, fx_n, fy_n, cx_n, cy_n, image_height_n,
                       image_width_n, saved_w, saved_flags, saved_gd, saved_gn};
    hipError_t e = launch_patchmatch_terms(q, reinterpret_cast<float*>(aligned_base(buf)), out4,
                                           (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "patchmatch terms", e);
}

int gsr_patchmatch_terms_backward(int H, int W, const float* median_depth, const float* normal,
                                  const float* points_nearest, const uint8_t* inside, const float* Mv, const float* tv,
                                  float Fx, float Fy, float Cx, float Cy, float noise_th, const float* R,
                                  const float* T, const float* image_r, const float* image_n, float fx_r, float fy_r,
                                  float cx_r, float cy_r, float fx_n, float fy_n, float cx_n, float cy_n,
                                  int image_height_n, int image_width_n, const float* saved_w,
                                  const uint8_t* saved_flags, const float* saved_gd, const float* saved_gn,
                                  const float* out4, const float* dL_dloss2, float* dL_dpoints_nearest,
                                  float* dL_dmedian_depth, float* dL_dnormal, void* stream_ptr) {
    if (const char* m = pm_check(H, W, median_depth, normal, points_nearest, inside, Mv, tv, R, T, image_r, image_n,
                                 image_height_n, image_width_n, saved_w, saved_flags, saved_gd, saved_gn))
        return fail(GSR_ERR_ARGS, m);
    if (!out4 || !dL_dloss2 || !dL_dpoints_nearest || !dL_dmedian_depth || !dL_dnormal)
        return fail(GSR_ERR_ARGS, "patchmatch backward: missing buffer");
    PatchMatchParams q{H, W, median_depth, normal, points_nearest, inside, Mv, tv, Fx, Fy, Cx, Cy, noise_th, R, T,
                       image_r, image_n, fx_r, fy_r, cx_r, cy_r, fx_n, fy_n, cx_n, cy_n, image_height_n,
                       image_width_n, const_cast<float*>(saved_w), const_cast<uint8_t*>(saved_flags),
                       const_cast<float*>(saved_gd), const_cast<float*>(saved_gn)};
    hipError_t e = launch_patchmatch_terms_bwd(q, out4, dL_dloss2, dL_dpoints_nearest, dL_dmedian_depth, dL_dnormal,
                                               (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "patchmatch terms backward", e);
}

int gsr_fused_ssim_forward(gsr_alloc_fn scratch_alloc, void* scratch_ctx, int NC, int H, int W, int valid,
                           const float* img1, const float* img2, float* out_mean, float* factors, void* stream_ptr) {
    if (NC <= 0 || H <= 0 || W <= 0 || (valid && (H <= 10 || W <= 10)))
        return fail(GSR_ERR_ARGS, "fused_ssim: invalid sizes (valid padding needs H, W > 10)");
    if (!img1 || !img2 || !out_mean || !scratch_alloc) return fail(GSR_ERR_ARGS, "fused_ssim: missing buffer");
    const size_t n = ssim_partials(NC, H, W);
    void* buf = scratch_alloc(scratch_ctx, n * sizeof(float) + 256);
    if (!buf) return fail(GSR_ERR_ALLOC, "fused_ssim: scratch allocation failed");
    float* partial = reinterpret_cast<float*>(aligned_base(buf));
    const size_t plane = (size_t)NC * H * W;
    hipError_t e = launch_ssim_fwd(NC, H, W, valid, img1, img2, factors, factors ? factors + plane : nullptr,
                                   factors ? factors + 2 * plane : nullptr, partial, out_mean, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "fused_ssim forward", e);
}

int gsr_fused_ssim_backward(int NC, int H, int W, int valid, const float* img1, const float* img2,
                            const float* factors, const float* dL_dmean, float* dL_dimg1, void* stream_ptr) {
    if (NC <= 0 || H <= 0 || W <= 0 || (valid && (H <= 10 || W <= 10)))
        return fail(GSR_ERR_ARGS, "fused_ssim: invalid sizes");
    if (!img1 || !img2 || !factors || !dL_dmean || !dL_dimg1) return fail(GSR_ERR_ARGS, "fused_ssim: missing buffer");
    const size_t plane = (size_t)NC * H * W;
    hipError_t e = launch_ssim_bwd(NC, H, W, valid, img1, img2, factors, factors + plane, factors + 2 * plane,
                                   dL_dmean, dL_dimg1, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "fused_ssim backward", e);
}

// the argument checks the two photometric-loss entry points share; nullptr when they pass
static const char* photo_check(int H, int W, int mode, int with_ssim, const float* image, const float* gt,
                               const float* embedding, const float* gain, int top, int left, int Hc, int Wc) {
    if (mode < kAppNo || mode > kAppGain) return "photo_loss: unknown appearance mode";
    if (H <= 0 || W <= 0 || (with_ssim && (H <= 10 || W <= 10)))
        return "photo_loss: invalid sizes (the SSIM needs H, W > 10)";
    if (!image || !gt) return "photo_loss: missing image";
    if ((mode == kAppGS || mode == kAppPGSR) && !embedding) return "photo_loss: this mode needs an embedding";
    if (mode == kAppGain) {
        if (!gain) return "photo_loss: the gain mode needs a gain plane";
        if (top < 0 || left < 0 || Hc < 1 || Wc < 1 || Hc > H - top || Wc > W - left)
            return "photo_loss: the crop lies outside the image";
    }
    return nullptr;
}

int gsr_photo_loss_forward(gsr_alloc_fn scratch_alloc, void* scratch_ctx, int H, int W, int mode, int with_ssim,
                           float lambda_dssim, const float* image, const float* gt, const float* mask,
                           const float* bg, const float* embedding, const float* gain, int crop_top, int crop_left,
                           int crop_h, int crop_w, float* out3, float* out_gt, float* factors, float* emb_sums,
                           void* stream_ptr) {
    if (const char* m = photo_check(H, W, mode, with_ssim, image, gt, embedding, gain, crop_top, crop_left, crop_h,
                                    crop_w))
        return fail(GSR_ERR_ARGS, m);
    if (!out3 || !scratch_alloc) return fail(GSR_ERR_ARGS, "photo_loss: missing buffer");
    void* buf = scratch_alloc(scratch_ctx, photo_loss_partials(H, W) * sizeof(float) + 256);
    if (!buf) return fail(GSR_ERR_ALLOC, "photo_loss: scratch allocation failed");
    float* partial = reinterpret_cast<float*>(aligned_base(buf));
    const size_t plane = (size_t)3 * H * W;
    if (!with_ssim) factors = nullptr;
    if (mode != kAppGS && mode != kAppPGSR) emb_sums = nullptr;
    const PhotoLossParams q{H, W, mode, with_ssim != 0, with_ssim ? lambda_dssim : 0.f, image, gt, mask, bg, embedding,
                            gain, crop_top, crop_left, crop_h, crop_w};
    hipError_t e = launch_photo_loss_fwd(q, out_gt, factors, factors ? factors + plane : nullptr,
                                         factors ? factors + 2 * plane : nullptr, partial, out3, emb_sums,
                                         (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "photo_loss forward", e);
}

int gsr_photo_loss_backward(int H, int W, int mode, int with_ssim, float lambda_dssim, const float* image,
                            const float* gt, const float* mask, const float* bg, const float* embedding,
                            const float* gain, int crop_top, int crop_left, int crop_h, int crop_w,
                            const float* factors, const float* emb_sums, const float* dL_dloss, float* dL_dimage,
                            float* dL_dembedding, float* dL_dgain, void* stream_ptr) {
    if (const char* m = photo_check(H, W, mode, with_ssim, image, gt, embedding, gain, crop_top, crop_left, crop_h,
                                    crop_w))
        return fail(GSR_ERR_ARGS, m);
    if (!dL_dloss || !dL_dimage || (with_ssim && !factors) || (dL_dembedding && !emb_sums))
        return fail(GSR_ERR_ARGS, "photo_loss backward: missing buffer");
    if (mode != kAppGS && mode != kAppPGSR) dL_dembedding = nullptr;
    const size_t plane = (size_t)3 * H * W;
    const PhotoLossParams q{H, W, mode, with_ssim != 0, with_ssim ? lambda_dssim : 0.f, image, gt, mask, bg, embedding,
                            gain, crop_top, crop_left, crop_h, crop_w};
    hipError_t e = launch_photo_loss_bwd(q, factors, with_ssim ? factors + plane : nullptr,
                                         with_ssim ? factors + 2 * plane : nullptr, emb_sums, dL_dloss, dL_dimage,
                                         dL_dembedding, dL_dgain, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "photo_loss backward", e);
}

int gsr_depth_to_normal_forward(const float* depth, int H, int W, float Fx, float Fy, float Cx, float Cy,
                                float* normal, uint8_t* valid, void* stream_ptr) {
    if (H < 0 || W < 0 || (H * W > 0 && (!depth || !normal || !valid)))
        return fail(GSR_ERR_ARGS, "depth_to_normal: invalid arguments");
    hipError_t e = launch_depth_normal(false, depth, H, W, Fx, Fy, Cx, Cy, nullptr, normal, valid,
                                       (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "depth_to_normal", e);
}

int gsr_depth_to_normal_backward(const float* depth, int H, int W, float Fx, float Fy, float Cx, float Cy,
                                 const float* dL_dnormal, float* dL_ddepth, void* stream_ptr) {
    if (H < 0 || W < 0 || (H * W > 0 && (!depth || !dL_dnormal || !dL_ddepth)))
        return fail(GSR_ERR_ARGS, "depth_to_normal backward: invalid arguments");
    hipError_t e = launch_depth_normal(true, depth, H, W, Fx, Fy, Cx, Cy, dL_dnormal, dL_ddepth, nullptr,
                                       (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "depth_to_normal backward", e);
}

int gsr_knn_mean_dist(gsr_alloc_fn scratch_alloc, void* scratch_ctx, int P, const float* points,
                      float* mean_dists, void* stream_ptr) {
    if (P < 0) return fail(GSR_ERR_ARGS, "distCUDA2: P < 0");
    if (P == 0) return GSR_OK;
    if (!points || !mean_dists || !scratch_alloc) return fail(GSR_ERR_ARGS, "distCUDA2: missing buffer");
    KnnState ks;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "distCUDA2: scratch allocation failed", carve_knn, P, ks))
        return rc;
    hipError_t e = launch_knn(P, points, ks, mean_dists, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "distCUDA2", e);
}

long long gsr_densify_workspace_bytes(long long P) {
    if (P < 1 || P > 0x7fffffffll / 5) return -1;
    return (long long)densify_workspace_bytes(P);
}

int gsr_densify_plan(long long P, const float* xyz_gradient_accum, const float* xyz_gradient_accum_abs,
                     const float* denom, const float* scaling, const float* opacity, float max_grad,
                     float min_opacity, float pd_extent, void* workspace, long long* counts, float* Q,
                     void* stream_ptr) {
    if (!counts) return fail(GSR_ERR_ARGS, "densify plan: missing count output");
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (P < 1) return fail(GSR_ERR_ARGS, "densify plan: no points");
    if (P > 0x7fffffffll / 5) return fail(GSR_ERR_ARGS, "densify plan: more than (2^31 - 1) / 5 points");
    if (!xyz_gradient_accum || !xyz_gradient_accum_abs || !denom || !scaling || !opacity || !workspace)
        return fail(GSR_ERR_ARGS, "densify plan: missing buffer");
    hipError_t e = launch_densify_plan(P, xyz_gradient_accum, xyz_gradient_accum_abs, denom, scaling, opacity, max_grad,
                                       min_opacity, pd_extent, workspace, counts, Q, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "densify plan", e);
}

int gsr_densify_apply(long long P, const long long* counts, void* workspace, int32_t* map, int build_map,
                      const float* noise, long long noise_rows, const float* rotation, const float* scaling, int n_params,
                      const gsr_densify_param* params, void* stream_ptr) {
    if (P < 1 || P > 0x7fffffffll / 5 || !counts || !workspace)
        return fail(GSR_ERR_ARGS, "densify apply: invalid arguments");
    const long long C = counts[0], S = counts[1], pruned = counts[2], N = counts[3];
    if (C < 0 || C > P || S < 0 || S > 2 * P || pruned < 0 || N < 0 || N != P + C + S - pruned)
        return fail(GSR_ERR_ARGS, "densify apply: counts are not those of a plan over P points");
    if (noise_rows != C + 2 * S)
        return fail(GSR_ERR_ARGS, "densify apply: the noise must have C + 2 S rows of 3");
    if (n_params < 0 || (n_params > 0 && !params)) return fail(GSR_ERR_ARGS, "densify apply: missing descriptors");
    if (N == 0) return GSR_OK;
    if (!map) return fail(GSR_ERR_ARGS, "densify apply: missing map buffer");
    std::vector<DensifyParam> d((size_t)n_params);
    for (int k = 0; k < n_params; k++) {
        const gsr_densify_param& s = params[k];
        if (s.width < 1 || !s.param || !s.param_out) return fail(GSR_ERR_ARGS, "densify apply: empty descriptor");
        if (s.role < kDensifyCopy || s.role > kDensifyScaling || (s.role != kDensifyCopy && s.width != 3))
            return fail(GSR_ERR_ARGS, "densify apply: xyz and scaling rows are 3 wide");
        if ((s.exp_avg != nullptr) != (s.exp_avg_sq != nullptr) ||
            (s.exp_avg && (!s.exp_avg_out || !s.exp_avg_sq_out)))
            return fail(GSR_ERR_ARGS, "densify apply: both moments and both outputs, or none");
        if (s.role == kDensifyXyz && noise_rows > 0 && (!noise || !rotation || !scaling))
            return fail(GSR_ERR_ARGS, "densify apply: new positions need noise, rotation and scaling");
        d[k] = DensifyParam{s.param, s.exp_avg, s.exp_avg_sq, s.param_out, s.exp_avg_out, s.exp_avg_sq_out, s.width,
                            s.role};
    }
    hipError_t e = launch_densify_apply(P, N, C, S, workspace, map, build_map != 0, noise, rotation, scaling, n_params, d.data(),
                                        (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "densify apply", e);
}

long long gsr_quantile_workspace_bytes(void) { return (long long)select_workspace_bytes(); }

int gsr_quantile(long long n, const float* values, const float* q, float* out, void* workspace, void* stream_ptr) {
    if (n < 1 || !values || !q || !out || !workspace) return fail(GSR_ERR_ARGS, "quantile: invalid arguments");
    hipError_t e = launch_radix_quantile(n, values, q, out, workspace, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "quantile", e);
}

int gsr_filter_3d(long long P, const float* xyz, int n_cam, const float* cameras, float max_focal, float* filter_3D,
                  void* scratch4, void* stream_ptr) {
    if (P < 1 || n_cam < 1 || !xyz || !cameras || !filter_3D || !scratch4 || !(max_focal > 0.f))
        return fail(GSR_ERR_ARGS, "filter_3d: invalid arguments");
    bool any = false;
    hipError_t e = launch_filter3d(P, xyz, n_cam, cameras, max_focal, filter_3D, (uint32_t*)scratch4, &any,
                                   (hipStream_t)stream_ptr);
    if (e != hipSuccess) return fail(GSR_ERR_HIP, "filter_3d", e);
    if (!any) return fail(GSR_ERR_ARGS, "filter_3d: no point is seen by any camera");
    return GSR_OK;
}

int gsr_reset_opacity(long long P, const float* scaling, const float* opacity, const float* filter_3D,
                      float* opacity_out, float* exp_avg_out, float* exp_avg_sq_out, void* stream_ptr) {
    if (P < 0 || (P > 0 && (!scaling || !opacity || !filter_3D || !opacity_out)) ||
        (exp_avg_out != nullptr) != (exp_avg_sq_out != nullptr))
        return fail(GSR_ERR_ARGS, "reset_opacity: invalid arguments");
    hipError_t e = launch_reset_opacity(P, scaling, opacity, filter_3D, opacity_out, exp_avg_out, exp_avg_sq_out,
                                        (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "reset_opacity", e);
}

}  // extern "C"
