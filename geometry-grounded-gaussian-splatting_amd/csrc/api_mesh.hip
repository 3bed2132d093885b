// api_mesh.hip — the C ABI (include/gsr.h) of the mesh path: marching tetrahedra (tetmesh.hip), the
// extraction sweep around `integrate` (fieldsweep.hip), the mesh clean-up (meshclean.hip) and TSDF
// fusion with marching cubes (tsdf.hip).  Host orchestration only: each call sizes its outputs from
// counts it reads back through one pinned slot (Readback); the sweep's three entries read nothing back.
#include "gsr_api_common.h"

using namespace gsr;

extern "C" {

int gsr_marching_tetrahedra(gsr_alloc_fn edge_alloc, void* edge_ctx, gsr_alloc_fn face_alloc, void* face_ctx,
                            gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long T, long long V,
                            const void* tets, int tets_int64, const float* sdf, const uint8_t* valid,
                            long long* num_edges, long long* num_faces, float* stage_ms, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (!num_edges || !num_faces) return fail(GSR_ERR_ARGS, "marching_tetrahedra: missing count outputs");
    *num_edges = *num_faces = 0;
    StageTimes times(stage_ms, stream);
    if (T < 0 || V < 0) return fail(GSR_ERR_ARGS, "marching_tetrahedra: negative size");
    if (T == 0) return GSR_OK;
    if (V <= 0) return fail(GSR_ERR_ARGS, "marching_tetrahedra: tets without vertices (V <= 0)");
    if (!tets || !sdf || !valid) return fail(GSR_ERR_ARGS, "marching_tetrahedra: missing input");
    if (!edge_alloc || !face_alloc || !scratch_alloc) return fail(GSR_ERR_ARGS, "marching_tetrahedra: missing allocator");
    if (reinterpret_cast<uintptr_t>(tets) % 16) return fail(GSR_ERR_ARGS, "marching_tetrahedra: tets must be 16-byte aligned");
    if (V > 0x7fffffffll || T > 0xffffffffll)
        return fail(GSR_ERR_ARGS, "marching_tetrahedra: more than 2^31 - 1 vertices or 2^32 - 1 tets");
    const bool is64 = tets_int64 != 0;

    TetCountState cs;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "marching_tetrahedra: scratch allocation failed",
                             carve_tet_count, V, T, cs))
        return rc;
    GSR_TIMED(times, 0, launch_tet_flags(V, sdf, valid, cs, stream), "tet vertex flags");
    GSR_TIMED(times, 1, launch_tet_count(T, V, tets, is64, cs, stream), "tet count");

    // first readback: the totals of one- and two-triangle tets and the bad-id flag
    Readback rb;
    GSR_CHECK(rb.begin(stream), "pinned readback buffer");
    GSR_CHECK(rb.copy(0, cs.partials + cs.nblocks, sizeof(uint64_t)), "memcpy tet counts");
    GSR_CHECK(rb.copy(2, cs.bad, sizeof(uint32_t)), "memcpy vertex id flag");
    GSR_CHECK(rb.commit(), "event record");
    GSR_CHECK(rb.wait(), "event sync");
    if (rb[2]) return fail(GSR_ERR_ARGS, "marching_tetrahedra: a tet names a vertex outside [0, V)");
    const uint64_t n1 = rb[0], n2 = rb[1];
    const uint64_t S = 3 * n1 + 4 * n2, F = n1 + 2 * n2;
    if (S == 0) {
        GSR_CHECK(times.collect(), "stage times");
        return GSR_OK;
    }
    if (S > 0xffffffffull) return fail(GSR_ERR_ARGS, "marching_tetrahedra: more than 2^32 - 1 crossing-edge slots");

    TetEdgeState es;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "marching_tetrahedra: scratch allocation failed",
                             carve_tet_edges, (size_t)S, tet_key_bits(V), es))
        return rc;
    GSR_TIMED(times, 2, launch_tet_emit(T, V, tets, is64, cs, es, stream), "tet edge keys");
    GSR_TIMED(times, 3, launch_tet_sort(es, stream), "tet edge sort");
    GSR_TIMED(times, 4, launch_tet_ranks(es, stream), "tet edge ranks");

    // second readback: E, the number of distinct keys
    GSR_CHECK(rb.copy(3, es.heads + (S - 1), sizeof(uint32_t)), "memcpy edge count");
    GSR_CHECK(rb.commit(), "event record");
    GSR_CHECK(rb.wait(), "event sync");
    const uint64_t E = rb[3];
    void* edge_ids = edge_alloc(edge_ctx, (size_t)E * 2 * sizeof(long long));
    if (!edge_ids) return fail(GSR_ERR_ALLOC, "marching_tetrahedra: edge_ids allocation failed");
    void* faces = face_alloc(face_ctx, (size_t)F * 3 * sizeof(long long));
    if (!faces) return fail(GSR_ERR_ALLOC, "marching_tetrahedra: faces allocation failed");
    GSR_TIMED(times, 5, launch_tet_edges(es, (long long*)edge_ids, stream), "tet edges");
    GSR_TIMED(times, 6, launch_tet_faces(T, V, tets, is64, cs, es, (long long*)faces, stream), "tet faces");
    GSR_CHECK(times.collect(), "stage times");
    *num_edges = (long long)E;
    *num_faces = (long long)F;
    return GSR_OK;
}

int gsr_field_view_update(long long N, const float* points, const float* alpha, const uint8_t* inside, const float* R,
                          const float* T, double Fx, double Fy, double Cx, double Cy, int W, int H, const float* mask,
                          float* weight, uint8_t* seen, void* stream_ptr) {
    if (N < 0 || N > kFieldMaxN) return fail(GSR_ERR_ARGS, "field_view_update: invalid size");
    if (mask && (W < 1 || H < 1)) return fail(GSR_ERR_ARGS, "field_view_update: a mask needs W, H >= 1");
    if (N == 0) return GSR_OK;
    if (!alpha || !inside || !weight || !seen) return fail(GSR_ERR_ARGS, "field_view_update: missing buffer");
    if (mask && (!points || !R || !T)) return fail(GSR_ERR_ARGS, "field_view_update: a mask needs points, R and T");
    FieldView v{};
    if (mask) {
        for (int k = 0; k < 9; k++) v.r[k] = R[k];
        for (int k = 0; k < 3; k++) v.t[k] = T[k];
        // the reference's constants: float64 on the host, then rounded (mesh_extract_tetrahedra.py:50-57)
        v.c[0] = (float)((Cx * 2.0 + 1.0) / W - 1.0), v.c[1] = (float)((Cy * 2.0 + 1.0) / H - 1.0);
        v.s[0] = (float)(Fx * 2.0 / W), v.s[1] = (float)(Fy * 2.0 / H);
        v.W = W, v.H = H;
    }
    hipError_t e = launch_field_view_update(v, N, points, alpha, inside, mask, weight, seen, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "field view update", e);
}

int gsr_field_finish(long long N, const float* weight, const uint8_t* seen, float* sdf, uint8_t* valid,
                     void* stream_ptr) {
    if (N < 0 || N > kFieldMaxN) return fail(GSR_ERR_ARGS, "field_finish: invalid size");
    if (N == 0) return GSR_OK;
    if (!weight || !seen || !sdf || !valid) return fail(GSR_ERR_ARGS, "field_finish: missing buffer");
    hipError_t e = launch_field_finish(N, weight, seen, sdf, valid, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "field finish", e);
}

int gsr_field_bisect_step(long long E, void* left_points, void* right_points, int points_float64, float* left_sdf,
                          float* right_sdf, const float* mid_sdf, void* mid_points, void* stream_ptr) {
    if (E < 0 || E > kFieldMaxN) return fail(GSR_ERR_ARGS, "field_bisect_step: invalid size");
    if (E == 0) return GSR_OK;
    if (!left_points || !right_points || !left_sdf || !right_sdf || !mid_sdf || !mid_points)
        return fail(GSR_ERR_ARGS, "field_bisect_step: missing buffer");
    hipError_t e = launch_field_bisect(E, left_points, right_points, points_float64 != 0, left_sdf, right_sdf, mid_sdf,
                                       mid_points, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "field bisect step", e);
}

int gsr_mesh_clusters(gsr_alloc_fn count_alloc, void* count_ctx, gsr_alloc_fn area_alloc, void* area_ctx,
                      gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long F, long long V, const void* faces,
                      int faces_int64, const float* vertices, long long* triangle_clusters, long long* num_clusters,
                      float* stage_ms, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (!num_clusters) return fail(GSR_ERR_ARGS, "mesh_clusters: missing count output");
    *num_clusters = 0;
    StageTimes times(stage_ms, stream);
    if (F < 0 || V < 0) return fail(GSR_ERR_ARGS, "mesh_clusters: negative size");
    if (F == 0) return GSR_OK;
    if (F >= 0x80000000ll || V > 0x80000000ll)
        return fail(GSR_ERR_ARGS, "mesh_clusters: 2^31 or more triangles, or more than 2^31 vertices");
    if (V == 0) return fail(GSR_ERR_ARGS, "mesh_clusters: faces without vertices (V <= 0)");
    if (!faces || !triangle_clusters) return fail(GSR_ERR_ARGS, "mesh_clusters: missing buffer");
    if (!count_alloc || !scratch_alloc || (vertices && !area_alloc))
        return fail(GSR_ERR_ARGS, "mesh_clusters: missing allocator");
    const bool is64 = faces_int64 != 0, area = vertices != nullptr;

    MeshClusterState cs;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "mesh_clusters: scratch allocation failed",
                             carve_mesh_clusters, F, V, area, cs))
        return rc;
    GSR_TIMED(times, 0, launch_clean_keys(V, faces, is64, cs, stream), "mesh edge keys");
    GSR_TIMED(times, 1, launch_clean_sort(cs, stream), "mesh edge sort");
    GSR_TIMED(times, 2, launch_clean_union(cs, stream), "mesh union");
    GSR_TIMED(times, 3, launch_clean_flatten(cs, stream), "mesh flatten");
    GSR_TIMED(times, 4, launch_clean_ids(cs, stream), "mesh cluster ids");

    // the one readback: C and the bad-id flag
    Readback rb;
    GSR_CHECK(rb.begin(stream), "pinned readback buffer");
    GSR_CHECK(rb.copy(0, cs.cid + F, sizeof(uint32_t)), "memcpy cluster count");
    GSR_CHECK(rb.copy(1, cs.flags + cs.rounds + 1, sizeof(uint32_t)), "memcpy vertex id flag");
    GSR_CHECK(rb.commit(), "event record");
    GSR_CHECK(rb.wait(), "event sync");
    if (rb[1]) return fail(GSR_ERR_ARGS, "mesh_clusters: a face names a vertex outside [0, V)");
    const long long C = rb[0];
    void* counts = count_alloc(count_ctx, (size_t)C * sizeof(long long));
    if (!counts) return fail(GSR_ERR_ALLOC, "mesh_clusters: cluster_n_triangles allocation failed");
    void* areas = area ? area_alloc(area_ctx, (size_t)C * sizeof(double)) : nullptr;
    if (area && !areas) return fail(GSR_ERR_ALLOC, "mesh_clusters: cluster_area allocation failed");
    GSR_TIMED(times, 5, launch_clean_counts(cs, triangle_clusters, (long long*)counts, stream), "mesh cluster counts");
    if (area)
        GSR_TIMED(times, 6, launch_clean_area(C, faces, is64, vertices, cs, (double*)areas, stream),
                  "mesh cluster areas");
    GSR_CHECK(times.collect(), "stage times");
    *num_clusters = C;
    return GSR_OK;
}

int gsr_mesh_filter(gsr_alloc_fn vertex_alloc, void* vertex_ctx, gsr_alloc_fn face_alloc, void* face_ctx,
                    gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long F, long long V, long long C,
                    const float* vertices, const void* faces, int faces_int64, const long long* triangle_clusters,
                    const long long* cluster_n_triangles, const long long* n_min, long long* num_vertices,
                    long long* num_faces, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (!num_vertices || !num_faces) return fail(GSR_ERR_ARGS, "mesh_filter: missing count outputs");
    *num_vertices = *num_faces = 0;
    if (F < 0 || V < 0 || C < 0) return fail(GSR_ERR_ARGS, "mesh_filter: negative size");
    if (F == 0) return GSR_OK;  // no triangle references a vertex
    if (F >= 0x80000000ll || V >= 0x80000000ll)
        return fail(GSR_ERR_ARGS, "mesh_filter: 2^31 or more triangles or vertices");
    if (V == 0 || C == 0) return fail(GSR_ERR_ARGS, "mesh_filter: faces without vertices or clusters");
    if (!vertices || !faces || !triangle_clusters || !cluster_n_triangles || !n_min)
        return fail(GSR_ERR_ARGS, "mesh_filter: missing buffer");
    if (!vertex_alloc || !face_alloc || !scratch_alloc) return fail(GSR_ERR_ARGS, "mesh_filter: missing allocator");
    const bool is64 = faces_int64 != 0;

    MeshFilterState fs;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "mesh_filter: scratch allocation failed", carve_mesh_filter,
                             F, V, fs))
        return rc;
    GSR_CHECK(launch_filter_plan(F, V, C, faces, is64, triangle_clusters, cluster_n_triangles, n_min, fs, stream),
              "mesh filter plan");

    // the one readback: V', F' and the bad-id flag
    Readback rb;
    GSR_CHECK(rb.begin(stream), "pinned readback buffer");
    GSR_CHECK(rb.copy(0, fs.vmap + V, sizeof(uint32_t)), "memcpy vertex count");
    GSR_CHECK(rb.copy(1, fs.fmap + F, sizeof(uint32_t)), "memcpy face count");
    GSR_CHECK(rb.copy(2, fs.bad, sizeof(uint32_t)), "memcpy id flag");
    GSR_CHECK(rb.commit(), "event record");
    GSR_CHECK(rb.wait(), "event sync");
    if (rb[2])
        return fail(GSR_ERR_ARGS, "mesh_filter: a face names a vertex outside [0, V) or a cluster outside [0, C)");
    const long long Vn = rb[0], Fn = rb[1];
    void* vout = Vn ? vertex_alloc(vertex_ctx, (size_t)Vn * 3 * sizeof(float)) : nullptr;
    if (Vn && !vout) return fail(GSR_ERR_ALLOC, "mesh_filter: vertices allocation failed");
    void* fout = Fn ? face_alloc(face_ctx, (size_t)Fn * 3 * sizeof(long long)) : nullptr;
    if (Fn && !fout) return fail(GSR_ERR_ALLOC, "mesh_filter: faces allocation failed");
    GSR_CHECK(launch_filter_gather(F, V, vertices, faces, is64, fs, (float*)vout, (long long*)fout, stream),
              "mesh filter gather");
    *num_vertices = Vn;
    *num_faces = Fn;
    return GSR_OK;
}

static const char* tsdf_camera(const float* intrinsic, const float* extrinsic, TsdfCamera& cam) {
    if (!intrinsic || !extrinsic) return "missing camera";
    cam.fx = intrinsic[0], cam.fy = intrinsic[1], cam.cx = intrinsic[2], cam.cy = intrinsic[3];
    if (!(cam.fx > 0.f) || !(cam.fy > 0.f)) return "focal lengths must be positive";
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) cam.e[r][c] = extrinsic[4 * r + c];
    return nullptr;
}

int gsr_tsdf_touch(gsr_alloc_fn coord_alloc, void* coord_ctx, gsr_alloc_fn scratch_alloc, void* scratch_ctx,
                   const float* depth, int H, int W, const float* intrinsic, const float* extrinsic,
                   float depth_scale, float depth_max, float sdf_trunc, float block_size, long long* num_blocks,
                   void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (!num_blocks) return fail(GSR_ERR_ARGS, "tsdf_touch: missing count output");
    *num_blocks = 0;
    if (H <= 0 || W <= 0 || !depth) return fail(GSR_ERR_ARGS, "tsdf_touch: missing depth image");
    if ((long long)H * W > 0x40000000ll) return fail(GSR_ERR_ARGS, "tsdf_touch: more than 2^30 pixels");
    if (!(depth_scale > 0.f) || !(depth_max > 0.f) || !(sdf_trunc > 0.f) || !(block_size > 0.f))
        return fail(GSR_ERR_ARGS, "tsdf_touch: depth_scale, depth_max, sdf_trunc and block_size must be positive");
    if (!coord_alloc || !scratch_alloc) return fail(GSR_ERR_ARGS, "tsdf_touch: missing allocator");
    TsdfCamera cam;
    if (const char* msg = tsdf_camera(intrinsic, extrinsic, cam)) return fail(GSR_ERR_ARGS, msg);

    TsdfTouchState ts;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "tsdf_touch: scratch allocation failed", carve_tsdf_touch, H,
                             W, ts))
        return rc;
    GSR_CHECK(launch_tsdf_touch(H, W, depth, cam, depth_scale, depth_max, sdf_trunc, block_size, ts, stream),
              "tsdf touch");

    // the one readback: the number of blocks and the out-of-range flag
    Readback rb;
    GSR_CHECK(rb.begin(stream), "pinned readback buffer");
    GSR_CHECK(rb.copy(0, ts.heads + ts.n, sizeof(uint32_t)), "memcpy block count");
    GSR_CHECK(rb.copy(1, ts.bad, sizeof(uint32_t)), "memcpy range flag");
    GSR_CHECK(rb.commit(), "event record");
    GSR_CHECK(rb.wait(), "event sync");
    if (rb[1]) return fail(GSR_ERR_ARGS, "tsdf_touch: a sample falls in a block beyond +-2^20");
    const long long n = rb[0];
    if (n == 0) return GSR_OK;
    void* coords = coord_alloc(coord_ctx, (size_t)n * 3 * sizeof(int));
    if (!coords) return fail(GSR_ERR_ALLOC, "tsdf_touch: block coordinate allocation failed");
    GSR_CHECK(launch_tsdf_touch_write(ts, (int*)coords, stream), "tsdf touch write");
    *num_blocks = n;
    return GSR_OK;
}

int gsr_tsdf_lookup(long long n, const int* block_coords, long long num_blocks, const long long* sorted_keys,
                    int* rank, void* stream_ptr) {
    if (n < 0 || num_blocks < 0 || num_blocks > 0x7fffffffll) return fail(GSR_ERR_ARGS, "tsdf_lookup: invalid size");
    if (n == 0) return GSR_OK;
    if (!block_coords || !rank || (num_blocks > 0 && !sorted_keys))
        return fail(GSR_ERR_ARGS, "tsdf_lookup: missing buffer");
    hipError_t e = launch_tsdf_lookup(n, block_coords, (int)num_blocks, (const uint64_t*)sorted_keys, rank,
                                      (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "tsdf lookup", e);
}

int gsr_tsdf_integrate(long long n, int block_resolution, const int* block_coords, const int* slots,
                       long long capacity, float voxel_size, float* tsdf, float* weight, float* color,
                       const float* depth, const float* image, int H, int W, const float* intrinsic,
                       const float* extrinsic, float depth_scale, float depth_max, float sdf_trunc,
                       void* stream_ptr) {
    if (n < 0 || n > 0x7fffffffll || capacity < 0 || capacity > 0x7fffffffll)
        return fail(GSR_ERR_ARGS, "tsdf_integrate: invalid size");
    if (block_resolution != 8 && block_resolution != 16)
        return fail(GSR_ERR_ARGS, "tsdf_integrate: block_resolution must be 8 or 16");
    if (H <= 0 || W <= 0 || !depth) return fail(GSR_ERR_ARGS, "tsdf_integrate: missing depth image");
    if ((long long)H * W > 0x40000000ll) return fail(GSR_ERR_ARGS, "tsdf_integrate: more than 2^30 pixels");
    if (!(voxel_size > 0.f) || !(depth_scale > 0.f) || !(depth_max > 0.f) || !(sdf_trunc > 0.f))
        return fail(GSR_ERR_ARGS, "tsdf_integrate: voxel_size, depth_scale, depth_max and sdf_trunc must be positive");
    if ((color != nullptr) != (image != nullptr))
        return fail(GSR_ERR_ARGS, "tsdf_integrate: a colour grid needs a colour image and the reverse");
    TsdfCamera cam;
    if (const char* msg = tsdf_camera(intrinsic, extrinsic, cam)) return fail(GSR_ERR_ARGS, msg);
    if (n == 0) return GSR_OK;
    if (!block_coords || !slots || !tsdf || !weight) return fail(GSR_ERR_ARGS, "tsdf_integrate: missing buffer");
    hipError_t e = launch_tsdf_integrate((int)n, block_resolution, block_coords, slots, capacity, voxel_size, tsdf,
                                         weight, color, depth, image, H, W, cam, depth_scale, depth_max, sdf_trunc,
                                         (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "tsdf integrate", e);
}

int gsr_tsdf_extract(gsr_alloc_fn vertex_alloc, void* vertex_ctx, gsr_alloc_fn color_alloc, void* color_ctx,
                     gsr_alloc_fn face_alloc, void* face_ctx, gsr_alloc_fn scratch_alloc, void* scratch_ctx,
                     long long num_blocks, int block_resolution, float voxel_size, float weight_threshold,
                     const long long* sorted_keys, const int* sorted_slots, const float* tsdf, const float* weight,
                     const float* color, long long* num_vertices, long long* num_faces, float* stage_ms,
                     void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (!num_vertices || !num_faces) return fail(GSR_ERR_ARGS, "tsdf_extract: missing count outputs");
    *num_vertices = *num_faces = 0;
    StageTimes times(stage_ms, stream);
    if (num_blocks < 0) return fail(GSR_ERR_ARGS, "tsdf_extract: negative size");
    if (block_resolution != 8 && block_resolution != 16)
        return fail(GSR_ERR_ARGS, "tsdf_extract: block_resolution must be 8 or 16");
    if (!(voxel_size > 0.f)) return fail(GSR_ERR_ARGS, "tsdf_extract: voxel_size must be positive");
    if (num_blocks == 0) return GSR_OK;
    // 5 triangles per voxel at most: the per-block totals stay below 2^32 over all blocks
    if (num_blocks * block_resolution * block_resolution * block_resolution > 0x7fffffffll / 5)
        return fail(GSR_ERR_ARGS, "tsdf_extract: more than (2^31 - 1) / 5 voxels");
    if (!sorted_keys || !sorted_slots || !tsdf || !weight) return fail(GSR_ERR_ARGS, "tsdf_extract: missing buffer");
    if (!vertex_alloc || !face_alloc || !scratch_alloc || (color && !color_alloc))
        return fail(GSR_ERR_ARGS, "tsdf_extract: missing allocator");
    const uint64_t* keys = (const uint64_t*)sorted_keys;

    TsdfExtractState es;
    if (int rc = carve_alloc(scratch_alloc, scratch_ctx, "tsdf_extract: scratch allocation failed",
                             carve_tsdf_extract, (int)num_blocks, block_resolution, es))
        return rc;
    GSR_TIMED(times, 0, launch_mc_mark(keys, sorted_slots, tsdf, weight, weight_threshold, es, stream),
              "marching cubes mark");
    GSR_TIMED(times, 1, launch_mc_count(es, stream), "marching cubes count");

    // the one readback: V and F
    Readback rb;
    GSR_CHECK(rb.begin(stream), "pinned readback buffer");
    GSR_CHECK(rb.copy(0, es.vbase + num_blocks, sizeof(uint32_t)), "memcpy vertex count");
    GSR_CHECK(rb.copy(1, es.fbase + num_blocks, sizeof(uint32_t)), "memcpy face count");
    GSR_CHECK(rb.commit(), "event record");
    GSR_CHECK(rb.wait(), "event sync");
    const long long V = rb[0], F = rb[1];
    if (F == 0) {  // a vertex exists only on an emitted cube's crossed edge, and such a cube has a triangle
        GSR_CHECK(times.collect(), "stage times");
        return GSR_OK;
    }
    void* vout = vertex_alloc(vertex_ctx, (size_t)V * 3 * sizeof(float));
    if (!vout) return fail(GSR_ERR_ALLOC, "tsdf_extract: vertices allocation failed");
    void* cout = color ? color_alloc(color_ctx, (size_t)V * 3 * sizeof(float)) : nullptr;
    if (color && !cout) return fail(GSR_ERR_ALLOC, "tsdf_extract: colours allocation failed");
    void* fout = face_alloc(face_ctx, (size_t)F * 3 * sizeof(long long));
    if (!fout) return fail(GSR_ERR_ALLOC, "tsdf_extract: faces allocation failed");
    GSR_TIMED(times, 2,
              launch_mc_vertices(keys, sorted_slots, tsdf, color, voxel_size, es, (float*)vout, (float*)cout, stream),
              "marching cubes vertices");
    GSR_TIMED(times, 3, launch_mc_faces(keys, es, (long long*)fout, stream), "marching cubes faces");
    GSR_CHECK(times.collect(), "stage times");
    *num_vertices = V;
    *num_faces = F;
    return GSR_OK;
}

}  // extern "C"
