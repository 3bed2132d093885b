// api_tnt.hip — the C ABI (include/gsr.h) of the TnT F-score evaluation (tnteval.hip): polygon crop,
// voxel-mean grid, nearest-point index (build / query), ICP sums, in-place transform; and of the mesh
// culling that precedes it (meshraster.hip): triangle depth raster and view vote.  Host orchestration
// only.
#include <float.h>
#include <math.h>
#include <string.h>

#include "gsr_api_common.h"

using namespace gsr;

static_assert(GSR_CROP_MAX_VERTICES == kCropMaxVertices, "the header's vertex cap is the kernel's LDS array");

namespace {

bool finite_all(const double* v, int n) {
    for (int k = 0; k < n; k++)
        if (!(v[k] > -DBL_MAX && v[k] < DBL_MAX)) return false;
    return true;
}

PointGrid index_grid(const gsr_point_index& ix) {
    PointGrid g{};
    for (int k = 0; k < 3; k++) g.mn[k] = ix.bounds_min[k], g.mx[k] = ix.bounds_max[k], g.nc[k] = ix.cells[k];
    g.cs = ix.cell_size;
    g.bx = ix.key_bits[0], g.by = ix.key_bits[1], g.bz = ix.key_bits[2];
    g.hashed = 0;
    return g;
}

// Per-stage GPU times summed over the views of one call: StageTimes holds one event pair per stage, a
// loop over views needs one per stage and view.  Measurement only; with stage_ms NULL nothing is created.
class ViewStageTimes {
  public:
    ViewStageTimes(float* stage_ms, hipStream_t stream) : ms_(stage_ms), stream_(stream) {
        if (ms_)
            for (int k = 0; k < 8; k++) ms_[k] = 0.f;
    }
    ViewStageTimes(const ViewStageTimes&) = delete;
    ViewStageTimes& operator=(const ViewStageTimes&) = delete;
    hipError_t begin(int k) {
        if (!ms_) return hipSuccess;
        Span sp{k, nullptr, nullptr};
        hipError_t e = hipEventCreate(&sp.a);
        if (e == hipSuccess) e = hipEventCreate(&sp.b);
        spans_.push_back(sp);
        return e == hipSuccess ? hipEventRecord(sp.a, stream_) : e;
    }
    hipError_t end(int) { return ms_ ? hipEventRecord(spans_.back().b, stream_) : hipSuccess; }
    hipError_t collect() {
        if (!ms_) return hipSuccess;
        hipError_t e = hipStreamSynchronize(stream_);
        for (size_t k = 0; k < spans_.size() && e == hipSuccess; k++) {
            float t = 0.f;
            e = hipEventElapsedTime(&t, spans_[k].a, spans_[k].b);
            ms_[spans_[k].stage] += t;
        }
        return e;
    }
    ~ViewStageTimes() {
        for (auto& sp : spans_) {
            if (sp.a) (void)hipEventDestroy(sp.a);
            if (sp.b) (void)hipEventDestroy(sp.b);
        }
    }

  private:
    struct Span {
        int stage;
        hipEvent_t a, b;
    };
    float* ms_;
    hipStream_t stream_;
    std::vector<Span> spans_;
};

int raster_camera(const char* who, const float* w2c, int H, int W, float fx, float fy, float cx, float cy, float znear,
                  float zfar, RasterCamera& c) {
    if (H < 1 || W < 1 || H > 16384 || W > 16384) return fail(GSR_ERR_ARGS, who);
    const float v[6] = {fx, fy, cx, cy, znear, zfar};
    for (float x : v)
        if (!(x > -FLT_MAX && x < FLT_MAX)) return fail(GSR_ERR_ARGS, who);
    if (!(fx > 0.f && fy > 0.f && znear > 0.f && zfar >= znear)) return fail(GSR_ERR_ARGS, who);
    if (w2c) memcpy(c.m, w2c, sizeof(c.m));
    c.fx = fx, c.fy = fy, c.cx = cx, c.cy = cy, c.znear = znear, c.zfar = zfar, c.W = W, c.H = H;
    return GSR_OK;
}

// the stages of one view's depth map into s.depth (stages 0-3 of `times`)
template <class Times>
int raster_view(Times& times, const RasterCamera& c, long long V, const float* vertices, long long F, const void* faces,
                bool is64, bool count, const MeshRasterState& s, hipStream_t stream) {
    GSR_TIMED(times, 0, launch_raster_clear(c, s, stream), "depth clear");
    if (F == 0) return GSR_OK;
    GSR_TIMED(times, 1, launch_raster_setup(c, V, F, vertices, faces, is64, count, s, stream), "raster set-up");
    GSR_TIMED(times, 2, launch_raster_scan(F, s, stream), "unit scan");
    GSR_TIMED(times, 3, launch_raster_units(c, V, F, vertices, faces, is64, count, s, stream), "raster units");
    return GSR_OK;
}

// the one readback of a raster call: the vertex id flag, and the counters when asked for
int raster_readback(const char* who, const MeshRasterState& s, unsigned long long* counters, hipStream_t stream) {
    Readback rb;
    GSR_CHECK(rb.begin(stream), "pinned readback buffer");
    GSR_CHECK(rb.copy(0, s.bad, sizeof(uint32_t)), "memcpy vertex id flag");
    GSR_CHECK(rb.commit(), "event record");
    if (counters)
        GSR_CHECK(hipMemcpyAsync(counters, s.counters, kRasterCounters * sizeof(unsigned long long),
                                 hipMemcpyDeviceToHost, stream),
                  "memcpy counters");
    GSR_CHECK(rb.wait(), "event sync");
    if (counters) GSR_CHECK(hipStreamSynchronize(stream), "stream sync");
    if (rb[0]) return fail(GSR_ERR_ARGS, who);
    return GSR_OK;
}

}  // namespace

extern "C" {

int gsr_points_crop_polygon(gsr_alloc_fn kept_alloc, void* kept_ctx, gsr_alloc_fn point_alloc, void* point_ctx,
                            gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long N, const double* points,
                            const double* transform, int orthogonal_axis, double axis_min, double axis_max,
                            int num_vertices, const double* polygon, long long* num_kept, float* stage_ms,
                            void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (!num_kept) return fail(GSR_ERR_ARGS, "points_crop_polygon: missing count output");
    *num_kept = 0;
    StageTimes times(stage_ms, stream);
    if (N < 0) return fail(GSR_ERR_ARGS, "points_crop_polygon: negative size");
    if (orthogonal_axis < 0 || orthogonal_axis > 2)
        return fail(GSR_ERR_ARGS, "points_crop_polygon: orthogonal_axis must be 0 (X), 1 (Y) or 2 (Z)");
    if (num_vertices < 0 || num_vertices > GSR_CROP_MAX_VERTICES)
        return fail(GSR_ERR_ARGS, "points_crop_polygon: more polygon vertices than GSR_CROP_MAX_VERTICES");
    if (num_vertices > 0 && !polygon) return fail(GSR_ERR_ARGS, "points_crop_polygon: missing polygon");
    if (N >= 0x80000000ll) return fail(GSR_ERR_ARGS, "points_crop_polygon: 2^31 or more points");
    if (N == 0) return GSR_OK;
    if (!points) return fail(GSR_ERR_ARGS, "points_crop_polygon: missing buffer");
    if (!kept_alloc || !point_alloc || !scratch_alloc)
        return fail(GSR_ERR_ARGS, "points_crop_polygon: missing allocator");

    CropParams p{};
    static const int axes[3][3] = {{1, 2, 0}, {0, 2, 1}, {0, 1, 2}};
    p.u = axes[orthogonal_axis][0], p.v = axes[orthogonal_axis][1], p.w = axes[orthogonal_axis][2];
    p.axis_min = axis_min, p.axis_max = axis_max, p.M = num_vertices;
    p.has_T = transform ? 1 : 0;
    if (transform) memcpy(p.T, transform, sizeof(p.T));

    CropState cs;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "points_crop_polygon: scratch allocation failed", carve_crop,
                             N, num_vertices, cs))
        return rc;
    if (num_vertices > 0)
        GSR_CHECK(hipMemcpyAsync(cs.poly, polygon, (size_t)num_vertices * 3 * sizeof(double), hipMemcpyHostToDevice,
                                 stream),
                  "copy polygon");
    GSR_TIMED(times, 0, launch_crop_plan(N, points, p, cs, stream), "crop flags and scan");
    // the one readback: the number kept
    Readback rb;
    GSR_CHECK(rb.begin(stream), "pinned readback buffer");
    GSR_CHECK(rb.copy(0, cs.flags + N, sizeof(uint32_t)), "memcpy kept count");
    GSR_CHECK(rb.commit(), "event record");
    GSR_CHECK(rb.wait(), "event sync");
    const long long M = rb[0];
    void* kept = kept_alloc(kept_ctx, (size_t)M * sizeof(long long));
    void* out = point_alloc(point_ctx, (size_t)M * 3 * sizeof(double));
    if (!kept || !out) return fail(GSR_ERR_ALLOC, "points_crop_polygon: output allocation failed");
    GSR_TIMED(times, 1, launch_crop_write(N, points, p, cs, (long long*)kept, (double*)out, stream), "crop write");
    GSR_CHECK(times.collect(), "stage times");
    *num_kept = M;
    return GSR_OK;
}

int gsr_points_voxel_mean(gsr_alloc_fn mean_alloc, void* mean_ctx, gsr_alloc_fn count_alloc, void* count_ctx,
                          gsr_alloc_fn cell_alloc, void* cell_ctx, gsr_alloc_fn scratch_alloc, void* scratch_ctx,
                          long long N, const double* points, double voxel, long long* num_cells, float* stage_ms,
                          void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (!num_cells) return fail(GSR_ERR_ARGS, "points_voxel_mean: missing count output");
    *num_cells = 0;
    StageTimes times(stage_ms, stream);
    if (N < 0) return fail(GSR_ERR_ARGS, "points_voxel_mean: negative size");
    if (!(voxel > 0.0) || !(voxel < HUGE_VAL))
        return fail(GSR_ERR_ARGS, "points_voxel_mean: voxel must be positive and finite");
    if (N == 0) return GSR_OK;
    if (N >= 0x80000000ll) return fail(GSR_ERR_ARGS, "points_voxel_mean: 2^31 or more points");
    if (!points) return fail(GSR_ERR_ARGS, "points_voxel_mean: missing buffer");
    if (!mean_alloc || !count_alloc || !cell_alloc || !scratch_alloc)
        return fail(GSR_ERR_ARGS, "points_voxel_mean: missing allocator");

    VoxelState vs;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "points_voxel_mean: scratch allocation failed", carve_voxel,
                             N, vs))
        return rc;
    GSR_TIMED(times, 0, launch_point_bounds(N, points, vs.partials, vs.bounds, stream), "point bounds");
    // first readback: the bounds, which place the grid and size the key
    double bounds[6];
    GSR_CHECK(hipMemcpyAsync(bounds, vs.bounds, sizeof(bounds), hipMemcpyDeviceToHost, stream), "memcpy bounds");
    GSR_CHECK(hipStreamSynchronize(stream), "stream sync");
    if (!finite_all(bounds, 6)) return fail(GSR_ERR_ARGS, "points_voxel_mean: points are not finite");
    VoxelGrid g{};
    g.voxel = voxel;
    int bits[3];
    for (int k = 0; k < 3; k++) {
        g.origin[k] = bounds[k] - 0.5 * voxel;
        const double cells = floor((bounds[3 + k] - g.origin[k]) / voxel) + 1.0;
        if (!(cells >= 1.0 && cells < 4611686018427387904.0))
            return fail(GSR_ERR_ARGS, "points_voxel_mean: the extent spans 2^62 or more voxels along an axis");
        bits[k] = 0;
        while (bits[k] < 63 && (double)(1ull << bits[k]) < cells) bits[k]++;
    }
    if (bits[0] + bits[1] + bits[2] > 64)
        return fail(GSR_ERR_ARGS, "points_voxel_mean: the voxel key needs more than 64 bits");
    g.by = bits[1], g.bz = bits[2];
    const unsigned key_bits = (unsigned)(bits[0] + bits[1] + bits[2] > 0 ? bits[0] + bits[1] + bits[2] : 1);
    GSR_TIMED(times, 1, launch_voxel_keys(N, points, g, vs, stream), "voxel keys");
    GSR_TIMED(times, 2, launch_voxel_sort(N, key_bits, vs, stream), "voxel sort");
    GSR_TIMED(times, 3, launch_voxel_plan(N, vs, stream), "voxel heads and scan");
    // second readback: the number of cells and the non-finite flag
    Readback rb;
    GSR_CHECK(rb.begin(stream), "pinned readback buffer");
    GSR_CHECK(rb.copy(0, vs.flags + N, sizeof(uint32_t)), "memcpy cell count");
    GSR_CHECK(rb.copy(1, vs.bad, sizeof(uint32_t)), "memcpy point flag");
    GSR_CHECK(rb.commit(), "event record");
    GSR_CHECK(rb.wait(), "event sync");
    if (rb[1]) return fail(GSR_ERR_ARGS, "points_voxel_mean: a point is not finite");
    const long long M = rb[0];
    void* means = mean_alloc(mean_ctx, (size_t)M * 3 * sizeof(double));
    void* counts = count_alloc(count_ctx, (size_t)M * sizeof(long long));
    void* cells = cell_alloc(cell_ctx, (size_t)M * 3 * sizeof(long long));
    if (!means || !counts || !cells) return fail(GSR_ERR_ALLOC, "points_voxel_mean: output allocation failed");
    GSR_TIMED(times, 4,
              launch_voxel_emit(N, points, g, vs, (double*)means, (long long*)counts, (long long*)cells, stream),
              "voxel emit");
    GSR_CHECK(times.collect(), "stage times");
    *num_cells = M;
    return GSR_OK;
}

size_t gsr_points_index_bytes(long long R) {
    if (R < 0 || R >= 0x80000000ll) return 0;
    PointIndexView v;
    return carve_point_index(nullptr, R, v);
}

int gsr_points_index_build(gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long R, const double* ref, void* buffer,
                           size_t buffer_bytes, gsr_point_index* index, float* stage_ms, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    StageTimes times(stage_ms, stream);
    if (!index) return fail(GSR_ERR_ARGS, "points_index_build: missing index description");
    memset(index, 0, sizeof(*index));
    if (R < 0) return fail(GSR_ERR_ARGS, "points_index_build: negative size");
    if (R >= 0x80000000ll) return fail(GSR_ERR_ARGS, "points_index_build: 2^31 or more points");
    if (R == 0) return GSR_OK;  // an index of nothing: every query answers +inf / -1
    if (!ref || !buffer) return fail(GSR_ERR_ARGS, "points_index_build: missing buffer");
    if (buffer_bytes < gsr_points_index_bytes(R))
        return fail(GSR_ERR_ARGS, "points_index_build: buffer smaller than gsr_points_index_bytes(R)");
    if (!scratch_alloc) return fail(GSR_ERR_ARGS, "points_index_build: missing allocator");

    PointIndexView v;
    carve_point_index(aligned_base(buffer), R, v);
    PointIndexBuildState bs;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "points_index_build: scratch allocation failed",
                             carve_point_index_build, R, bs))
        return rc;
    GSR_TIMED(times, 0, launch_point_bounds(R, ref, bs.partials, bs.bounds, stream), "ref bounds");
    // the one readback: the bounds of ref, which size the grid
    double bounds[6];
    GSR_CHECK(hipMemcpyAsync(bounds, bs.bounds, sizeof(bounds), hipMemcpyDeviceToHost, stream), "memcpy bounds");
    GSR_CHECK(hipStreamSynchronize(stream), "stream sync");
    if (!finite_all(bounds, 6)) return fail(GSR_ERR_ARGS, "points_index_build: ref is not finite");
    PointGrid grid;
    point_nearest_grid(bounds, R, grid);
    GSR_TIMED(times, 1,
              launch_point_sort(R, ref, grid, bs.keys, v.keys, v.order, v.x, v.y, v.z, nullptr, bs.tmp, bs.tmp_bytes,
                                stream),
              "ref cell sort");
    GSR_CHECK(times.collect(), "stage times");
    index->R = R;
    index->buffer = buffer;
    for (int k = 0; k < 3; k++)
        index->bounds_min[k] = grid.mn[k], index->bounds_max[k] = grid.mx[k], index->cells[k] = grid.nc[k];
    index->cell_size = grid.cs;
    index->key_bits[0] = grid.bx, index->key_bits[1] = grid.by, index->key_bits[2] = grid.bz;
    return GSR_OK;
}

int gsr_points_index_query(gsr_alloc_fn scratch_alloc, void* scratch_ctx, const gsr_point_index* index, long long Q,
                           const double* query, double max_dist, double* dist, long long* nearest, float* stage_ms,
                           void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    StageTimes times(stage_ms, stream);
    if (!index) return fail(GSR_ERR_ARGS, "points_index_query: missing index");
    if (Q < 0) return fail(GSR_ERR_ARGS, "points_index_query: negative size");
    if (!(max_dist > 0.0)) return fail(GSR_ERR_ARGS, "points_index_query: max_dist must be positive");
    if (Q == 0) return GSR_OK;
    if (Q >= 0x80000000ll) return fail(GSR_ERR_ARGS, "points_index_query: 2^31 or more points");
    if (!query || !dist || !nearest) return fail(GSR_ERR_ARGS, "points_index_query: missing buffer");
    const long long R = index->R;
    if (R == 0) {
        GSR_CHECK(launch_index_fill(Q, dist, nearest, stream), "index fill");
        return GSR_OK;
    }
    if (R < 0 || R >= 0x80000000ll || !index->buffer || !(index->cell_size > 0.0) || index->cells[0] < 1 ||
        index->cells[1] < 1 || index->cells[2] < 1 || index->cells[0] > 2097152 || index->cells[1] > 2097152 ||
        index->cells[2] > 2097152)
        return fail(GSR_ERR_ARGS, "points_index_query: not an index that gsr_points_index_build wrote");
    if (!scratch_alloc) return fail(GSR_ERR_ARGS, "points_index_query: missing allocator");

    PointIndexView v;
    carve_point_index(aligned_base(index->buffer), R, v);
    const PointGrid grid = index_grid(*index);
    PointNearestState ns;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "points_index_query: scratch allocation failed",
                             carve_point_query, Q, ns))
        return rc;
    GSR_TIMED(times, 0, launch_nearest_qsort(Q, query, grid, ns, stream), "query sort");
    GSR_TIMED(times, 1, launch_index_search(Q, query, R, grid, v, ns, max_dist, dist, nearest, stream),
              "indexed search");
    GSR_CHECK(times.collect(), "stage times");
    return GSR_OK;
}

int gsr_icp_accumulate(gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long N, const double* src, long long R,
                       const double* ref, const long long* index, int pass, const double* means, double* sums,
                       float* stage_ms, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    StageTimes times(stage_ms, stream);
    if (pass != 1 && pass != 2) return fail(GSR_ERR_ARGS, "icp_accumulate: pass must be 1 or 2");
    const int K = pass == 1 ? 8 : 10;
    if (!sums) return fail(GSR_ERR_ARGS, "icp_accumulate: missing output");
    for (int k = 0; k < K; k++) sums[k] = 0.0;
    if (N < 0 || R < 0) return fail(GSR_ERR_ARGS, "icp_accumulate: negative size");
    if (pass == 2 && !means) return fail(GSR_ERR_ARGS, "icp_accumulate: pass 2 needs the two means");
    if (N == 0) return GSR_OK;
    if (N >= 0x80000000ll || R >= 0x80000000ll) return fail(GSR_ERR_ARGS, "icp_accumulate: 2^31 or more points");
    if (!src || !index || (R > 0 && !ref)) return fail(GSR_ERR_ARGS, "icp_accumulate: missing buffer");
    if (!scratch_alloc) return fail(GSR_ERR_ARGS, "icp_accumulate: missing allocator");

    IcpState is;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "icp_accumulate: scratch allocation failed", carve_icp, is))
        return rc;
    GSR_TIMED(times, 0, launch_icp_accumulate(pass, N, src, R, ref, index, means, is, stream), "icp sums");
    // the one readback: the sums and the bad-index count
    double host[kIcpMaxSums + 1];
    GSR_CHECK(hipMemcpyAsync(host, is.sums, sizeof(host), hipMemcpyDeviceToHost, stream), "memcpy sums");
    GSR_CHECK(hipStreamSynchronize(stream), "stream sync");
    if (host[K] != 0.0) return fail(GSR_ERR_ARGS, "icp_accumulate: an index lies outside [-1, R)");
    for (int k = 0; k < K; k++) sums[k] = host[k];
    GSR_CHECK(times.collect(), "stage times");
    return GSR_OK;
}

int gsr_points_transform(long long N, double* points, const double* transform, float* stage_ms, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    StageTimes times(stage_ms, stream);
    if (N < 0) return fail(GSR_ERR_ARGS, "points_transform: negative size");
    if (!transform) return fail(GSR_ERR_ARGS, "points_transform: missing transform");
    if (N == 0) return GSR_OK;
    if (N >= 0x80000000ll) return fail(GSR_ERR_ARGS, "points_transform: 2^31 or more points");
    if (!points) return fail(GSR_ERR_ARGS, "points_transform: missing buffer");
    GSR_TIMED(times, 0, launch_points_transform(N, points, transform, stream), "transform");
    GSR_CHECK(times.collect(), "stage times");
    return GSR_OK;
}

int gsr_mesh_depth(gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long V, const float* vertices, long long F,
                   const void* faces, int faces_int64, const float* w2c, int H, int W, float fx, float fy, float cx,
                   float cy, float znear, float zfar, float* depth, unsigned long long* counters, float* stage_ms,
                   void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    StageTimes times(stage_ms, stream);
    if (counters)
        for (int k = 0; k < kRasterCounters; k++) counters[k] = 0;
    if (V < 0 || F < 0) return fail(GSR_ERR_ARGS, "mesh_depth: negative size");
    if (V >= 0x80000000ll || F >= 0x80000000ll) return fail(GSR_ERR_ARGS, "mesh_depth: 2^31 or more elements");
    RasterCamera c{};
    if (!w2c || !depth) return fail(GSR_ERR_ARGS, "mesh_depth: missing buffer");
    if (int rc = raster_camera("mesh_depth: image size, intrinsics or depth range out of range", w2c, H, W, fx, fy, cx,
                               cy, znear, zfar, c))
        return rc;
    if (F == 0) {
        GSR_CHECK(hipMemsetAsync(depth, 0, (size_t)H * (size_t)W * sizeof(float), stream), "depth clear");
        return GSR_OK;
    }
    if (!faces || (V > 0 && !vertices)) return fail(GSR_ERR_ARGS, "mesh_depth: missing buffer");
    if (!scratch_alloc) return fail(GSR_ERR_ARGS, "mesh_depth: missing allocator");
    MeshRasterState s;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "mesh_depth: scratch allocation failed", carve_mesh_raster, F,
                             H, W, s))
        return rc;
    GSR_CHECK(launch_raster_reset(s, stream), "raster reset");
    if (int rc = raster_view(times, c, V, vertices, F, faces, faces_int64 != 0, counters != nullptr, s, stream))
        return rc;
    GSR_TIMED(times, 4, launch_raster_finish(c, s, depth, stream), "depth finish");
    if (int rc = raster_readback("mesh_depth: a face names a vertex outside [0, V)", s, counters, stream)) return rc;
    GSR_CHECK(times.collect(), "stage times");
    return GSR_OK;
}

int gsr_mesh_view_votes(gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long V, const float* vertices, long long F,
                        const void* faces, int faces_int64, int n_views, const float* w2cs, int H, int W, float fx,
                        float fy, float cx, float cy, float znear, float zfar, float eps, int* counts,
                        unsigned long long* counters, float* stage_ms, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    ViewStageTimes times(stage_ms, stream);
    if (counters)
        for (int k = 0; k < kRasterCounters; k++) counters[k] = 0;
    if (V < 0 || F < 0 || n_views < 0) return fail(GSR_ERR_ARGS, "mesh_view_votes: negative size");
    if (V >= 0x80000000ll || F >= 0x80000000ll)
        return fail(GSR_ERR_ARGS, "mesh_view_votes: 2^31 or more elements");
    RasterCamera c{};
    if (int rc = raster_camera("mesh_view_votes: image size, intrinsics or depth range out of range", nullptr, H, W,
                               fx, fy, cx, cy, znear, zfar, c))
        return rc;
    if (!(eps > -FLT_MAX && eps < FLT_MAX)) return fail(GSR_ERR_ARGS, "mesh_view_votes: eps must be finite");
    if (V == 0 && F == 0) return GSR_OK;
    if ((V > 0 && (!vertices || !counts)) || (F > 0 && !faces) || (n_views > 0 && !w2cs))
        return fail(GSR_ERR_ARGS, "mesh_view_votes: missing buffer");
    if (V > 0) GSR_CHECK(hipMemsetAsync(counts, 0, (size_t)V * sizeof(int), stream), "count clear");
    if (n_views == 0) return GSR_OK;
    if (!scratch_alloc) return fail(GSR_ERR_ARGS, "mesh_view_votes: missing allocator");
    MeshRasterState s;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "mesh_view_votes: scratch allocation failed",
                             carve_mesh_raster, F, H, W, s))
        return rc;
    GSR_CHECK(launch_raster_reset(s, stream), "raster reset");
    // every view on the stream, one depth buffer, nothing read back in between
    for (int k = 0; k < n_views; k++) {
        memcpy(c.m, w2cs + 12 * (size_t)k, sizeof(c.m));
        if (int rc = raster_view(times, c, V, vertices, F, faces, faces_int64 != 0, counters != nullptr, s, stream))
            return rc;
        if (V > 0) GSR_TIMED(times, 4, launch_view_vote(c, eps, V, vertices, s, counts, stream), "view vote");
    }
    if (int rc = raster_readback("mesh_view_votes: a face names a vertex outside [0, V)", s, counters, stream))
        return rc;
    GSR_CHECK(times.collect(), "stage times");
    return GSR_OK;
}

}  // extern "C"
