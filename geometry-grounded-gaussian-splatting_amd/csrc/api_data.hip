// api_data.hip — the C ABI (include/gsr.h) of the view preparation (viewprep.hip): Pillow's coefficient
// table, the 8-bit resample pass and the float planes of a view.  Host orchestration only.
#include "gsr_api_common.h"

using namespace gsr;

// sizes of one axis: the table index t * out_size + xx and the launch grids stay far inside 32 bits
static constexpr int kMaxAxis = 1 << 20;

extern "C" {

int gsr_resample_ksize(int in_size, int out_size) {
    if (in_size <= 0 || out_size <= 0 || in_size > kMaxAxis || out_size > kMaxAxis) return 0;
    return resample_ksize(in_size, out_size);
}

int gsr_resample_coeffs(int in_size, int out_size, int32_t* k, int32_t* bounds) {
    if (in_size <= 0 || in_size > kMaxAxis) return fail(GSR_ERR_ARGS, "resample_coeffs: `in_size` must be in [1, 2^20]");
    if (out_size <= 0 || out_size > kMaxAxis)
        return fail(GSR_ERR_ARGS, "resample_coeffs: `out_size` must be in [1, 2^20]");
    if (!k || !bounds) return fail(GSR_ERR_ARGS, "resample_coeffs: missing buffer");
    resample_coeffs(in_size, out_size, k, bounds);
    return GSR_OK;
}

int gsr_image_resample8(long long N, int H, int W, int C, int axis, int out_size, const uint8_t* in, uint8_t* out,
                        const int32_t* k, const int32_t* bounds, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (N < 0 || H <= 0 || W <= 0 || H > kMaxAxis || W > kMaxAxis)
        return fail(GSR_ERR_ARGS, "image_resample8: `in` must be [N,H,W,C] with H, W in [1, 2^20]");
    if (C < 1 || C > 4) return fail(GSR_ERR_ARGS, "image_resample8: `C` must be 1, 2, 3 or 4");
    if (axis != 0 && axis != 1) return fail(GSR_ERR_ARGS, "image_resample8: `axis` must be 0 (H) or 1 (W)");
    if (out_size <= 0 || out_size > kMaxAxis) return fail(GSR_ERR_ARGS, "image_resample8: `out_size` must be in [1, 2^20]");
    if (N == 0) return GSR_OK;
    // rows of the W pass (N H) and (image, output row) pairs of the H pass are one grid dimension
    if ((double)N * H >= 2147483648.0 || (double)N * out_size >= 2147483648.0)
        return fail(GSR_ERR_ARGS, "image_resample8: 2^31 or more rows in one call");
    if (!in || !out || !k || !bounds) return fail(GSR_ERR_ARGS, "image_resample8: missing buffer");
    GSR_CHECK(launch_image_resample8(N, H, W, C, axis, out_size, in, out, k, bounds, stream), "image resample8");
    return GSR_OK;
}

int gsr_view_planes(long long N, int H, int W, const uint8_t* rgb, const uint8_t* mask, float* original, float* gray,
                    float* gt_mask, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (N < 0 || H <= 0 || W <= 0) return fail(GSR_ERR_ARGS, "view_planes: invalid sizes");
    if (N == 0) return GSR_OK;
    if ((double)N * H * W >= 274877906944.0) return fail(GSR_ERR_ARGS, "view_planes: 2^38 or more pixels");
    if (!rgb || !original || !gray) return fail(GSR_ERR_ARGS, "view_planes: missing buffer");
    if (mask && !gt_mask) return fail(GSR_ERR_ARGS, "view_planes: `mask` without `gt_mask`");
    GSR_CHECK(launch_view_planes(N, H, W, rgb, mask, original, gray, gt_mask, stream), "view planes");
    return GSR_OK;
}

}  // extern "C"
