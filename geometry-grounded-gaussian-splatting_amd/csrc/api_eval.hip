// api_eval.hip — the C ABI (include/gsr.h) of the DTU Chamfer evaluation (pointeval.hip): surface
// sampling, radius thinning and nearest point; and of the image-quality evaluation (imgmetric.hip):
// 8-bit quantisation, L1, MSE and per-image SSIM.  Host orchestration only.
#include <float.h>
#include <math.h>

#include "gsr_api_common.h"

using namespace gsr;

extern "C" {

int gsr_mesh_sample_points(gsr_alloc_fn point_alloc, void* point_ctx, gsr_alloc_fn scratch_alloc, void* scratch_ctx,
                           long long V, long long F, const double* vertices, const void* faces, int faces_int64,
                           double density, long long* num_points, float* stage_ms, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (!num_points) return fail(GSR_ERR_ARGS, "mesh_sample_points: missing count output");
    *num_points = 0;
    StageTimes times(stage_ms, stream);
    if (F < 0 || V < 0) return fail(GSR_ERR_ARGS, "mesh_sample_points: negative size");
    if (!(density > 0.0) || !(density < HUGE_VAL))
        return fail(GSR_ERR_ARGS, "mesh_sample_points: density must be positive and finite");
    if (F >= 0x80000000ll || V >= 0x80000000ll)
        return fail(GSR_ERR_ARGS, "mesh_sample_points: 2^31 or more triangles or vertices");
    if (F > 0 && V == 0) return fail(GSR_ERR_ARGS, "mesh_sample_points: faces without vertices");
    if ((V > 0 && !vertices) || (F > 0 && !faces)) return fail(GSR_ERR_ARGS, "mesh_sample_points: missing buffer");
    if (!point_alloc || !scratch_alloc) return fail(GSR_ERR_ARGS, "mesh_sample_points: missing allocator");
    if (V == 0) return GSR_OK;
    const bool is64 = faces_int64 != 0;

    unsigned long long S = 0;
    PointSampleState ss{};
    if (F > 0) {
        if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "mesh_sample_points: scratch allocation failed",
                                 carve_point_sample, F, ss))
            return rc;
        GSR_TIMED(times, 0, launch_sample_count(F, V, vertices, faces, is64, density, ss, stream), "sample count");
        GSR_TIMED(times, 1, launch_sample_scan(F, ss, stream), "sample scan");
        // the one readback: S (two words) and the bad flag
        Readback rb;
        GSR_CHECK(rb.begin(stream), "pinned readback buffer");
        GSR_CHECK(rb.copy(0, ss.offsets + F, sizeof(uint64_t)), "memcpy sample count");
        GSR_CHECK(rb.copy(2, ss.bad, sizeof(uint32_t)), "memcpy face flag");
        GSR_CHECK(rb.commit(), "event record");
        GSR_CHECK(rb.wait(), "event sync");
        if (rb[2])
            return fail(GSR_ERR_ARGS, "mesh_sample_points: a face names a vertex outside [0, V), or a triangle is "
                                      "not finite");
        S = (unsigned long long)rb[0] | (unsigned long long)rb[1] << 32;
        if (S >= (1ull << 38)) return fail(GSR_ERR_ARGS, "mesh_sample_points: 2^38 or more sampled points");
    }
    double* out = (double*)point_alloc(point_ctx, ((size_t)V + (size_t)S) * 3 * sizeof(double));
    if (!out) return fail(GSR_ERR_ALLOC, "mesh_sample_points: points allocation failed");
    // (stage 2 spans the vertex copy and the emit)
    GSR_CHECK(times.begin(2), "event");
    GSR_CHECK(hipMemcpyAsync(out, vertices, (size_t)V * 3 * sizeof(double), hipMemcpyDeviceToDevice, stream),
              "copy vertices");
    if (S > 0) GSR_CHECK(launch_sample_emit(F, V, S, vertices, faces, is64, density, ss, out, stream), "sample emit");
    GSR_CHECK(times.end(2), "event");
    GSR_CHECK(times.collect(), "stage times");
    *num_points = V + (long long)S;
    return GSR_OK;
}

int gsr_points_downsample(gsr_alloc_fn kept_alloc, void* kept_ctx, gsr_alloc_fn scratch_alloc, void* scratch_ctx,
                          long long N, const double* points, double radius, long long* num_kept,
                          long long* num_rounds, float* stage_ms, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (!num_kept) return fail(GSR_ERR_ARGS, "points_downsample: missing count output");
    *num_kept = 0;
    if (num_rounds) *num_rounds = 0;
    StageTimes times(stage_ms, stream);
    if (N < 0) return fail(GSR_ERR_ARGS, "points_downsample: negative size");
    if (!(radius > 0.0) || !(radius < HUGE_VAL))
        return fail(GSR_ERR_ARGS, "points_downsample: radius must be positive and finite");
    if (N == 0) return GSR_OK;
    if (N >= 0x80000000ll) return fail(GSR_ERR_ARGS, "points_downsample: 2^31 or more points");
    if (!points) return fail(GSR_ERR_ARGS, "points_downsample: missing buffer");
    if (!kept_alloc || !scratch_alloc) return fail(GSR_ERR_ARGS, "points_downsample: missing allocator");

    PointThinState ts;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "points_downsample: scratch allocation failed",
                             carve_point_thin, N, ts))
        return rc;
    GSR_TIMED(times, 0, launch_point_bounds(N, points, ts.partials, ts.bounds, stream), "point bounds");
    // first readback: the bounds, which size the grid
    double bounds[6];
    GSR_CHECK(hipMemcpyAsync(bounds, ts.bounds, sizeof(bounds), hipMemcpyDeviceToHost, stream), "memcpy bounds");
    GSR_CHECK(hipStreamSynchronize(stream), "stream sync");
    PointGrid grid;
    if (!point_thin_grid(bounds, radius, grid))
        return fail(GSR_ERR_ARGS, "points_downsample: points are not finite, or span 2^31 or more cells of side radius");
    GSR_TIMED(times, 1,
              launch_point_sort(N, points, grid, ts.keys, ts.keys_sorted, ts.order, ts.sx, ts.sy, ts.sz, ts.state,
                                ts.tmp, ts.tmp_bytes, stream),
              "point cell sort");

    Readback rb;
    GSR_CHECK(rb.begin(stream), "pinned readback buffer");
    // a round decides at least the lowest undecided rank, so N rounds are the most there can be
    long long rounds = 0;
    GSR_CHECK(times.begin(2), "event");  // (stage 2 spans the rounds)
    for (;;) {
        GSR_CHECK(launch_thin_round(ts, grid, radius, stream), "thinning round");
        rounds++;
        GSR_CHECK(rb.copy(0, ts.undecided, sizeof(uint32_t)), "memcpy undecided flag");
        GSR_CHECK(rb.commit(), "event record");
        GSR_CHECK(rb.wait(), "event sync");
        if (!rb[0]) break;
        if (rounds > N) return fail(GSR_ERR_HIP, "points_downsample: the rounds did not end");
    }
    GSR_CHECK(times.end(2), "event");
    GSR_TIMED(times, 3, launch_thin_plan(ts, stream), "thinning plan");
    GSR_CHECK(rb.copy(1, ts.flags + N, sizeof(uint32_t)), "memcpy kept count");
    GSR_CHECK(rb.commit(), "event record");
    GSR_CHECK(rb.wait(), "event sync");
    const long long M = rb[1];
    void* kept = kept_alloc(kept_ctx, (size_t)M * sizeof(long long));
    if (!kept) return fail(GSR_ERR_ALLOC, "points_downsample: kept allocation failed");
    GSR_TIMED(times, 4, launch_thin_write(ts, (long long*)kept, stream), "thinning write");
    GSR_CHECK(times.collect(), "stage times");
    *num_kept = M;
    if (num_rounds) *num_rounds = rounds;
    return GSR_OK;
}

int gsr_points_nearest(gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long Q, const double* query, long long R,
                       const double* ref, double max_dist, double* dist, float* stage_ms, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    StageTimes times(stage_ms, stream);
    if (Q < 0 || R < 0) return fail(GSR_ERR_ARGS, "points_nearest: negative size");
    if (!(max_dist > 0.0)) return fail(GSR_ERR_ARGS, "points_nearest: max_dist must be positive");
    if (Q == 0) return GSR_OK;
    if (Q >= 0x80000000ll || R >= 0x80000000ll) return fail(GSR_ERR_ARGS, "points_nearest: 2^31 or more points");
    if (!query || !dist || (R > 0 && !ref)) return fail(GSR_ERR_ARGS, "points_nearest: missing buffer");
    if (R == 0) {
        GSR_CHECK(launch_nearest_fill(Q, dist, stream), "nearest fill");
        return GSR_OK;
    }
    if (!scratch_alloc) return fail(GSR_ERR_ARGS, "points_nearest: missing allocator");

    PointNearestState ns;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "points_nearest: scratch allocation failed",
                             carve_point_nearest, Q, R, ns))
        return rc;
    GSR_TIMED(times, 0, launch_point_bounds(R, ref, ns.partials, ns.bounds, stream), "ref bounds");
    // the one readback: the bounds of ref, which size the grid
    double bounds[6];
    GSR_CHECK(hipMemcpyAsync(bounds, ns.bounds, sizeof(bounds), hipMemcpyDeviceToHost, stream), "memcpy bounds");
    GSR_CHECK(hipStreamSynchronize(stream), "stream sync");
    for (double b : bounds)
        if (!(b > -DBL_MAX && b < DBL_MAX)) return fail(GSR_ERR_ARGS, "points_nearest: ref is not finite");
    PointGrid grid;
    point_nearest_grid(bounds, R, grid);
    GSR_TIMED(times, 1,
              launch_point_sort(R, ref, grid, ns.rkeys, ns.rkeys_sorted, ns.rorder, ns.rx, ns.ry, ns.rz, nullptr,
                                ns.tmp, ns.tmp_bytes, stream),
              "ref cell sort");
    GSR_TIMED(times, 2, launch_nearest_qsort(Q, query, grid, ns, stream), "query sort");
    GSR_TIMED(times, 3, launch_nearest_search(Q, query, R, grid, ns, max_dist, dist, stream), "nearest search");
    GSR_CHECK(times.collect(), "stage times");
    return GSR_OK;
}

int gsr_image_quantize8(long long N, int C, int H, int W, const float* image, uint8_t* out, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (N < 0 || C <= 0 || H <= 0 || W <= 0) return fail(GSR_ERR_ARGS, "image_quantize8: invalid sizes");
    if (N == 0) return GSR_OK;
    if (!image || !out) return fail(GSR_ERR_ARGS, "image_quantize8: missing buffer");
    if ((double)N * C * H * W >= 1099511627776.0) return fail(GSR_ERR_ARGS, "image_quantize8: 2^40 or more values");
    if ((uintptr_t)out & 3) return fail(GSR_ERR_ARGS, "image_quantize8: `out` must be 4-byte aligned");
    GSR_CHECK(launch_image_quantize8(N, C, H, W, image, out, stream), "image quantize8");
    return GSR_OK;
}

int gsr_image_metrics(gsr_alloc_fn scratch_alloc, void* scratch_ctx, int N, int C, int H, int W, int quantize,
                      int with_ssim, const float* render, const float* gt, uint8_t* render_bytes, uint8_t* gt_bytes,
                      double* out, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (N < 0 || C <= 0 || H <= 0 || W <= 0) return fail(GSR_ERR_ARGS, "image_metrics: invalid sizes");
    if (with_ssim && (H < 11 || W < 11))
        return fail(GSR_ERR_ARGS, "image_metrics: SSIM needs H and W of at least 11 (no 11 x 11 window fits)");
    if (N == 0) return GSR_OK;
    if (N > 65535) return fail(GSR_ERR_ARGS, "image_metrics: more than 65535 images in one call");
    if ((double)C * H * W >= 2147483648.0) return fail(GSR_ERR_ARGS, "image_metrics: 2^31 or more values per image");
    if (!render || !gt || !out) return fail(GSR_ERR_ARGS, "image_metrics: missing buffer");
    if (!scratch_alloc) return fail(GSR_ERR_ARGS, "image_metrics: missing allocator");
    if (render_bytes || gt_bytes) {
        if (!quantize) return fail(GSR_ERR_ARGS, "image_metrics: byte images are written in quantised mode only");
        if (C > 4) return fail(GSR_ERR_ARGS, "image_metrics: byte images have at most 4 channels");
        if (((uintptr_t)render_bytes | (uintptr_t)gt_bytes) & 3)
            return fail(GSR_ERR_ARGS, "image_metrics: byte images must be 4-byte aligned");
    }
    ImageMetricsState st;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "image_metrics: scratch allocation failed",
                             carve_image_metrics, N, C, H, W, with_ssim, st))
        return rc;
    GSR_CHECK(launch_image_metrics(N, C, H, W, quantize, with_ssim, render, gt, render_bytes, gt_bytes, st, out,
                                   stream),
              "image metrics");
    return GSR_OK;
}

}  // extern "C"
