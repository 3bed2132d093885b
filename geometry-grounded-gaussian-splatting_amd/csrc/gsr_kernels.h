// gsr_kernels.h — internal launch interface between the C-ABI host code
// (gsr_api.hip for the rasteriser, api_train.hip, api_mesh.hip, api_eval.hip) and
// the kernels.  Not part of the public ABI (include/gsr.h).
#pragma once

#include "gsr_common.h"

namespace gsr {

// Run-time switches for A/B variants of one kernel in one process
// (gsr_set_option in include/gsr.h); defaults are the shipped paths.
// ids 0, 7 and 8 belonged to retired A/B variants (bisection shortcut, per-tile
// sort binning, two-wave backward); gsr_set_option rejects them
enum Option : int { kOptRenderStats = 1, kOptNoRefine = 5, kOptBwdNoCache = 6, kOptRocprimDsort = 9, kOptPbwdStage = 10, kNumOptions = 11 };
inline bool option_retired(int opt) { return opt == 0 || (opt >= 2 && opt <= 4) || opt == 7 || opt == 8; }
int option(int which);
hipError_t read_render_stats(unsigned long long* out, bool reset);

struct FwdParams {
    int P, D, SHM, SGD, SGM, W, H;
    const float* background;
    const float* means3D;
    const float* colors_precomp;
    const float* opacities;
    const float* scales;
    const float* rotations;
    const float* cov3D_precomp;
    const float* shs;
    const float* sg_axis;
    const float* sg_sharpness;
    const float* sg_color;
    const float* shs_rest = nullptr;  // split SH rows: shs holds [P][3] DC rows, shs_rest [P][SHM-1][3]
    float scale_modifier;
    const float* view;
    const float* proj;
    const float* campos;
    float tan_fovx, tan_fovy, focal_x, focal_y, kernel_size;
    uint32_t grid_x, grid_y;
    bool require_depth;
    bool no_color;   // sample_depth: preprocess skips the colour (rasterizer_impl.cu:1080)
    float cull_pad;  // tile-culling pad in pixels (tiles.h): 0 render, 0.5 sample_depth
};

struct BwdParams {
    FwdParams f;
    int R;
    const int* radii;
    const float* alphas;
    const float* normalmap;
    const float* mdepth;
    const float* dL_dpix;
    const float* dL_dmdepth;
    const float* dL_dalpha;
    const float* dL_dnormal;
    float* dL_dmean3D;
    float* dL_dmean2D;
    float* dL_dcolor;
    float* dL_dopacity;
    float* dL_dscale;
    float* dL_drot;
    float* dL_dcov3D;
    float* dL_dsh;
    float* dL_dsg_axis;
    float* dL_dsg_sharpness;
    float* dL_dsg_color;
    float* dL_dsh_rest = nullptr;  // split SH rows (f.shs_rest): dL_dsh [P][3], dL_dsh_rest [P][SHM-1][3]
};

// preprocess_fwd.hip
hipError_t launch_preprocess_fwd(const FwdParams& p, const GeomState& gs, int* radii, hipStream_t stream);

// binning.hip
size_t scan_temp_bytes(int P);
size_t depth_sort_temp_bytes(int P);
size_t sort_temp_bytes(int K, int tile_bits);
hipError_t launch_depth_sort(const GeomState& gs, int P, bool prepared, hipStream_t stream);
// dsort.hip
size_t dsort_temp_bytes(int P);
int dsort_tile_keys(int P);
void dsort_zero_region(void* base, int P, uint32_t** first, size_t* words);
// K into gs.offsets_K and, with `hist`, the depth-key digit histograms (both zeroed by the preprocess)
hipError_t launch_count_k_hist(const GeomState& gs, int P, bool hist, hipStream_t stream);
// `prepared`: state zeroed and histograms counted by the two kernels above
hipError_t launch_dsort(const GeomState& gs, int P, bool prepared, hipStream_t stream);
hipError_t launch_live_counts(const FwdParams& p, const GeomState& gs, const int* radii, hipStream_t stream);
hipError_t launch_scan(const GeomState& gs, int P, hipStream_t stream);
hipError_t launch_emit_keys(const FwdParams& p, const GeomState& gs, const int* radii, const BinningState& bs,
                            hipStream_t stream);
hipError_t launch_sort(const BinningState& bs, int K, int tile_bits, hipStream_t stream);
hipError_t launch_tile_ranges(const BinningState& bs, int K, const TileState& ts, int tiles, hipStream_t stream);

// tilelists.hip
bool list_binning(uint32_t gx, uint32_t gy);
ListLayout list_layout(int P, int K, uint32_t gx, uint32_t gy);
size_t reduce_temp_bytes(int P);
hipError_t launch_list_binning(const FwdParams& p, const GeomState& gs, const int* radii, const BinningState& bs,
                               const TileState& ts, int K, hipStream_t stream);
// the device-sized exclusive scan of the counting passes: in[0, n) into out[0, n], n = n_dev ? mul * *n_dev : n_host,
// cap >= n the host's bound; `sums` holds scan_sums_count(cap) words (gsr_debug_scan_excl runs it alone)
uint32_t scan_sums_count(size_t cap);
hipError_t launch_scan_excl(const uint32_t* in, uint32_t* out, size_t cap, uint32_t n_host, const uint32_t* n_dev,
                            uint32_t mul, uint32_t* sums, hipStream_t stream);
// the file's structural constants (gsr_debug_list_constants): writes min(n, count) of them, returns count
int list_constants(int* out, int n);


// render_fwd.hip
hipError_t launch_render_fwd(const FwdParams& p, const GeomState& gs, const BinningState& bs, const ImageState& is,
                             const TileState& ts, float* out_color, float* out_alpha, float* out_normal,
                             float* out_mdepth, hipStream_t stream);

// render_bwd.hip
hipError_t launch_render_bwd(const BwdParams& b, const GeomState& gs, const BinningState& bs, const ImageState& is,
                             const TileState& ts, const BwdState& ws, hipStream_t stream);

// preprocess_bwd.hip
// Gaussians [begin, end) (end < 0: all P); dc_rows non-null: factored view-parallel mode
// (preprocess_bwd.hip PreprocessBwdArgs::dc_rows)
hipError_t launch_preprocess_bwd(const BwdParams& b, const GeomState& gs, const BwdState& ws, hipStream_t stream,
                                 int begin = 0, int end = -1, float* dc_rows = nullptr);

// render_fwd.hip: the forward raster in SAMPLE mode (median depth at points)
// point queries answered by the forward raster in SAMPLE mode
enum { kQuerySample = 0, kQueryIntegrate = 1, kQuerySDF = 2 };
// sample_depth: out0 = points [PN][3]; integrate: out0 = transmittance [PN];
// evaluate_sdf: out0 = median depth [PN], out1 = sdf [PN]
hipError_t launch_point_fwd(int query, const FwdParams& p, const GeomState& gs, const BinningState& bs,
                            const TileState& ts, const PointState& ps, const PointBinState& pb, const SampleTiles& st,
                            const ChunkState& cs, uint32_t num_chunks, float* out0, float* out1, uint8_t* out_inside,
                            hipStream_t stream);

// sample.hip
hipError_t launch_sample_points(const FwdParams& p, int PN, const float* points3D, const PointState& ps,
                                const PointBinState& pb, const SampleTiles& st, hipStream_t stream);
hipError_t launch_sample_setup(int PN, uint32_t tiles, const PointBinState& pb, const SampleTiles& st,
                               hipStream_t stream);
struct SampleBwdParams {
    FwdParams f;
    int PN;
    const float* points3D;
    const uint8_t* inside;
    const float* dL_doutput;
    float* dL_dpoints3D;
};
hipError_t launch_sample_bwd(const SampleBwdParams& b, const GeomState& gs, const BinningState& bs,
                             const TileState& ts, const PointState& ps, const PointBinState& pb,
                             const SampleTiles& st, const ChunkState& cs, const BwdState& ws, hipStream_t stream);

// optim.hip: multi-tensor Adam step and densification statistics
constexpr int kMaxAdamGroups = 16;
struct AdamGroup {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    long long n;
    int aligned;  // all four pointers 16-B aligned: float4 path
};
hipError_t launch_adam(int n_groups, const AdamGroup* groups, const double* lr, double step, double beta1,
                       double beta2, double eps, hipStream_t stream);
// view_grads.hip: a view-parallel step's SH / SG gradients from the gathered DC rows
hipError_t launch_view_color_grads(int P, int D, int SHM, int SGD, int SGM, int n_views, const float* gathered,
                                   const float* means3D, const float* sg_axis, const float* sg_sharpness,
                                   const float* sg_color, float* dL_dsh, float* dL_dsg_axis, float* dL_dsg_sharpness,
                                   float* dL_dsg_color, hipStream_t stream, int chunk = 0,
                                   const float* campos = nullptr, float* dL_dsh_rest = nullptr);
hipError_t launch_densify_stats(int P, const float* vgrad, const int* radii, float* max_radii2D, float* accum,
                                float* accum_abs, float* denom, hipStream_t stream);

// ncc.hip: warp-patch NCC with forward-mode gradients
struct NccParams {
    int P;
    const float* depths;
    const float* normals;
    const int* uvs;
    const float* R;
    const float* T;
    const float* image_r;
    const float* image_n;
    float fx_r, fy_r, cx_r, cy_r, fx_n, fy_n, cx_n, cy_n;
    int Hr, Wr, Hn, Wn;
    float* ncc;
    float* grad_depths;
    float* grad_normals;
    uint8_t* valid;
};
hipError_t launch_ncc(const NccParams& q, hipStream_t stream);

// optim.hip: the activation getters of training (gsr_scale_opacity_3d_filter*, gsr_normalize_rows*)
hipError_t launch_scale_opacity(int P, const float* s, const float* o, const float* f, float* scales, float* opac,
                                const float* gS, const float* gO, float* ds, float* dop, bool backward,
                                hipStream_t stream);
hipError_t launch_normalize_rows(int n, int D, const float* x, const float* gy, float* out, bool backward,
                                 hipStream_t stream);

// ncc.hip: the fused PatchMatch terms of training (gsr_patchmatch_*)
struct PatchMatchParams {
    int H, W;               // the view (reference image of the NCC)
    const float* md;        // [H*W]
    const float* normal;    // [3, H*W]
    const float* pin;       // [H*W, 3]
    const uint8_t* inside;  // [H*W]
    const float* Mv;        // [9] row-major
    const float* tv;        // [3]
    float Fx, Fy, Cx, Cy;
    float noise_th;
    const float* R;  // [9] NCC rotation (the reference's column-major float33), T [3]
    const float* T;
    const float* image_r;
    const float* image_n;
    float fx_r, fy_r, cx_r, cy_r, fx_n, fy_n, cx_n, cy_n;
    int Hn, Wn;
    float* w;
    uint8_t* flags;
    float* gd;
    float* gn;
};
size_t patchmatch_partials(int H, int W);
hipError_t launch_patchmatch_terms(const PatchMatchParams& q, float* partial, float* out, hipStream_t stream);
hipError_t launch_patchmatch_terms_bwd(const PatchMatchParams& q, const float* out, const float* dL_dloss,
                                       float* dL_dpin, float* dL_dmd, float* dL_dnormal, hipStream_t stream);
hipError_t launch_patchmatch_lift(bool backward, int H, int W, float Fx, float Fy, float Cx, float Cy, const float* T,
                                  const float* M, const float* md, const float* gpts, float* out, hipStream_t stream);

// ssim.hip: fused SSIM forward / backward
size_t ssim_partials(int NC, int H, int W);
hipError_t launch_ssim_fwd(int NC, int H, int W, int valid, const float* img1, const float* img2, float* fA,
                           float* fB, float* fC, float* partial, float* out, hipStream_t stream);
hipError_t launch_ssim_bwd(int NC, int H, int W, int valid, const float* img1, const float* img2, const float* fA,
                           const float* fB, const float* fC, const float* dL_dloss, float* dL_dimg1,
                           hipStream_t stream);

// photoloss.hip: the photometric loss (mask composite, appearance transform, L1 and D-SSIM) fused
enum { kAppNo = 0, kAppGS = 1, kAppPGSR = 2, kAppGain = 3 };  // gsr_app_model (include/gsr.h)
struct PhotoLossParams {
    int H, W, mode, ssim;
    float lambda;
    const float *img, *gt, *mask, *bg, *emb, *gain;
    int top, left, Hc, Wc;
};
size_t photo_loss_partials(int H, int W);
hipError_t launch_photo_loss_fwd(const PhotoLossParams& q, float* out_gt, float* fA, float* fB, float* fC,
                                 float* partial, float* out3, float* emb_sums, hipStream_t stream);
hipError_t launch_photo_loss_bwd(const PhotoLossParams& q, const float* fA, const float* fB, const float* fC,
                                 const float* emb_sums, const float* dL_dloss, float* dL_dimg, float* dL_demb,
                                 float* dL_dgain, hipStream_t stream);

// depth_normal.hip: normal map of a depth map and its backward
hipError_t launch_depth_normal(bool backward, const float* depth, int H, int W, float Fx, float Fy, float Cx, float Cy,
                               const float* g, float* out, uint8_t* valid, hipStream_t stream);

// mark visible
hipError_t launch_near_violation(int P, const float* means3D, const float* view, uint32_t* flag,
                                 hipStream_t stream);
hipError_t launch_mark_visible(int P, const float* means3D, const float* view, uint8_t* present,
                               hipStream_t stream);

// distCUDA2 (knn.hip): scratch carved from one caller buffer
struct KnnState {
    float* partials;
    float* bounds;
    uint32_t* codes;
    uint32_t* codes_sorted;
    uint32_t* order;
    float4* sorted;
    float4* boxes;
    char* sort_tmp;
    size_t sort_tmp_bytes;
};
size_t carve_knn(void* base, int P, KnnState& s);
hipError_t launch_knn(int P, const float* pts, const KnnState& s, float* mean_dists, hipStream_t stream);

// marching tetrahedra (tetmesh.hip).  Two scratch buffers: the first is sized by V and T alone
// (V / 4 bytes of vertex flags, 8 bytes per 1024 tets), the second by the number S of crossing-edge
// slots, known after the count (20 bytes per slot plus the sort's temporary).
struct TetCountState {
    long long nblocks;   // ceil(T / 1024)
    uint32_t* flags;     // 2 bits per vertex: sdf > 0, valid
    uint64_t* partials;  // [nblocks + 1] (one-triangle | two-triangle << 32) tets per block, then their exclusive scan
    uint32_t* bad;       // set when a tet names a vertex outside [0, V)
    void* scan_tmp;
    size_t scan_tmp_bytes;
};
struct TetEdgeState {
    size_t S;
    int bits;                // key = a << bits | b
    uint64_t* keys;          // [S] in slot order
    uint64_t* keys_sorted;   // [S]
    uint32_t* slots_sorted;  // [S] the slot of each sorted key
    uint32_t* heads;         // [S] (over keys) head flags, then the 1-based rank of each sorted key
    uint32_t* rank;          // [S] (over keys) the mesh vertex of each slot
    void* tmp;
    size_t tmp_bytes;
};
int tet_key_bits(long long V);
size_t carve_tet_count(void* base, long long V, long long T, TetCountState& s);
size_t carve_tet_edges(void* base, size_t S, int bits, TetEdgeState& s);
hipError_t launch_tet_flags(long long V, const float* sdf, const uint8_t* valid, const TetCountState& s,
                            hipStream_t stream);
hipError_t launch_tet_count(long long T, long long V, const void* tets, bool is64, const TetCountState& s,
                            hipStream_t stream);
hipError_t launch_tet_emit(long long T, long long V, const void* tets, bool is64, const TetCountState& s,
                           const TetEdgeState& es, hipStream_t stream);
hipError_t launch_tet_sort(const TetEdgeState& es, hipStream_t stream);
hipError_t launch_tet_ranks(const TetEdgeState& es, hipStream_t stream);
hipError_t launch_tet_edges(const TetEdgeState& es, long long* edge_ids, hipStream_t stream);
hipError_t launch_tet_faces(long long T, long long V, const void* tets, bool is64, const TetCountState& s,
                            const TetEdgeState& es, long long* faces, hipStream_t stream);

// mesh clean-up (meshclean.hip).  gsr_mesh_clusters: one scratch buffer sized by F alone (64 bytes per
// triangle, 8 more with areas, plus the sort's temporary); arrays that are dead by then are reused.
struct MeshClusterState {
    long long F;
    int bits;                // key = a << bits | b
    int rounds;              // ceil(log2 F) pointer-jumping rounds
    uint64_t* keys;          // [3 F] slot 3 t + e: edge e of triangle t
    uint64_t* keys_sorted;   // [3 F]
    uint32_t* slots_sorted;  // [3 F]
    uint32_t* parent;        // [F] the union-find forest, parent[x] <= x
    uint32_t* flags;         // [rounds] a round moved a parent, [rounds + 1] a face names a vertex outside [0, V)
    uint32_t* cid;           // [F + 1] (over keys) root flags, then their exclusive scan: cid[F] = C
    uint32_t* root_count;    // [F] (over keys) triangles per root
    uint32_t* label32;       // [F] (over keys_sorted) cluster id per triangle
    uint32_t* label_sorted;  // [F] (over keys_sorted)
    uint32_t* seg;           // [C + 1] (over keys_sorted) first sorted position of every cluster
    double* tri_area;        // [F] (over slots_sorted)
    double* area_sorted;     // [F] only with areas
    void* tmp;
    size_t tmp_bytes;
};
struct MeshFilterState {
    uint32_t* vmap;  // [V + 1] used flags, then their exclusive scan: the new vertex ids, vmap[V] = V'
    uint32_t* fmap;  // [F + 1] the same for the triangles that stay
    uint32_t* bad;
    void* tmp;
    size_t tmp_bytes;
};
size_t carve_mesh_clusters(void* base, long long F, long long V, bool area, MeshClusterState& s);
size_t carve_mesh_filter(void* base, long long F, long long V, MeshFilterState& s);
hipError_t launch_clean_keys(long long V, const void* faces, bool is64, const MeshClusterState& s,
                             hipStream_t stream);
hipError_t launch_clean_sort(const MeshClusterState& s, hipStream_t stream);
hipError_t launch_clean_union(const MeshClusterState& s, hipStream_t stream);
hipError_t launch_clean_flatten(const MeshClusterState& s, hipStream_t stream);
hipError_t launch_clean_ids(const MeshClusterState& s, hipStream_t stream);
hipError_t launch_clean_counts(const MeshClusterState& s, long long* triangle_clusters, long long* cluster_n,
                               hipStream_t stream);
hipError_t launch_clean_area(long long C, const void* faces, bool is64, const float* vertices,
                             const MeshClusterState& s, double* cluster_area, hipStream_t stream);
hipError_t launch_filter_plan(long long F, long long V, long long C, const void* faces, bool is64,
                              const long long* clusters, const long long* cluster_n, const long long* n_min,
                              const MeshFilterState& s, hipStream_t stream);
hipError_t launch_filter_gather(long long F, long long V, const float* vertices, const void* faces, bool is64,
                                const MeshFilterState& s, float* vertices_out, long long* faces_out,
                                hipStream_t stream);

// TSDF fusion and marching cubes (tsdf.hip).  Touch: 20 bytes per sample (4 per stride-4 pixel) plus
// the sort's temporary.  Extract: 3.5 bytes per voxel (case, 4 mask bits, vertex offset) and 8 per block.
struct TsdfCamera {  // by value into the kernels
    float fx, fy, cx, cy;
    float e[3][4];  // the first three rows of the world -> camera matrix
};
struct TsdfTouchState {
    int gw, gh;             // stride-4 lattice
    long long n;            // 4 gw gh samples
    uint64_t* keys;         // [n] packed block keys, all ones where there is no sample
    uint64_t* keys_sorted;  // [n]
    uint32_t* heads;        // [n + 1] run heads, then their exclusive scan: heads[n] = the number of blocks
    uint32_t* bad;          // a sample beyond +-2^20 blocks
    void* tmp;
    size_t tmp_bytes;
};
struct TsdfExtractState {
    int nb, R;
    uint8_t* cases;     // [nb R^3] the case of every emitted cube, 0 otherwise
    uint32_t* masks;    // [nb R^3 / 8] 4 bits per voxel: its x, y, z edge carries a vertex
    uint16_t* voffset;  // [nb R^3] vertices of the block before the voxel's
    uint32_t* vbase;    // [nb + 1] vertices per block, then their exclusive scan
    uint32_t* fbase;    // [nb + 1] the same for triangles
    void* tmp;
    size_t tmp_bytes;
};
size_t carve_tsdf_touch(void* base, int H, int W, TsdfTouchState& s);
size_t carve_tsdf_extract(void* base, int nb, int R, TsdfExtractState& s);
hipError_t launch_tsdf_touch(int H, int W, const float* depth, const TsdfCamera& cam, float depth_scale,
                             float depth_max, float trunc, float block_size, const TsdfTouchState& s,
                             hipStream_t stream);
hipError_t launch_tsdf_touch_write(const TsdfTouchState& s, int* coords, hipStream_t stream);
hipError_t launch_tsdf_lookup(long long n, const int* coords, int nb, const uint64_t* sorted_keys, int* rank,
                              hipStream_t stream);
hipError_t launch_tsdf_integrate(int n, int R, const int* coords, const int* slots, long long capacity,
                                 float voxel_size, float* tsdf, float* weight, float* color, const float* depth,
                                 const float* image, int H, int W, const TsdfCamera& cam, float depth_scale,
                                 float depth_max, float trunc, hipStream_t stream);
hipError_t launch_mc_mark(const uint64_t* keys, const int* slots, const float* tsdf, const float* weight,
                          float threshold, const TsdfExtractState& s, hipStream_t stream);
hipError_t launch_mc_count(const TsdfExtractState& s, hipStream_t stream);
hipError_t launch_mc_vertices(const uint64_t* keys, const int* slots, const float* tsdf, const float* color,
                              float voxel_size, const TsdfExtractState& s, float* vertices, float* colors,
                              hipStream_t stream);
hipError_t launch_mc_faces(const uint64_t* keys, const TsdfExtractState& s, long long* faces, hipStream_t stream);

// point-cloud evaluation (pointeval.hip): mesh sampling, radius thinning, bounded nearest point; float64
struct PointGrid {      // by value into the kernels
    double mn[3], mx[3];  // bounds of the gridded points
    double cs;            // cell side
    long long nc[3];      // cells per axis
    int bx, by, bz;       // key = cx << (by + bz) | cy << bz | cz
    int hashed;           // more than 64 key bits: key = hash of the cell
};
struct PointSampleState {
    uint64_t* offsets;  // [F + 1] samples per triangle, then their exclusive scan: offsets[F] = S
    uint32_t* bad;      // a face names a vertex outside [0, V), or a non-finite lattice
    void* tmp;
    size_t tmp_bytes;
};
struct PointThinState {
    long long N;
    double* partials;       // bounds reduction
    double* bounds;         // [6] min xyz, max xyz
    uint64_t* keys;         // [N] cell keys in input (shuffled) order
    uint64_t* keys_sorted;  // [N]
    uint32_t* order;        // [N] the rank (input position) of each sorted point
    double *sx, *sy, *sz;   // [N] the sorted points
    uint32_t* state;        // [N] by sorted position: undecided, kept, removed
    uint32_t* undecided;    // a round left a point undecided
    uint32_t* flags;        // [N + 1] (over keys) kept by rank, then their exclusive scan: flags[N] = M
    void* tmp;
    size_t tmp_bytes;
};
struct PointNearestState {
    double* partials;
    double* bounds;
    uint64_t *rkeys, *rkeys_sorted;  // [R] packed cell keys of ref
    uint32_t* rorder;                // [R]
    double *rx, *ry, *rz;            // [R] ref in key order
    uint64_t *qkeys, *qkeys_sorted;  // [Q] Morton codes of the queries' cells
    uint32_t* qorder;                // [Q]
    void* tmp;
    size_t tmp_bytes;
};
size_t carve_point_sample(void* base, long long F, PointSampleState& s);
size_t carve_point_thin(void* base, long long N, PointThinState& s);
size_t carve_point_nearest(void* base, long long Q, long long R, PointNearestState& s);
bool point_thin_grid(const double* bounds, double radius, PointGrid& g);
void point_nearest_grid(const double* bounds, long long R, PointGrid& g);
hipError_t launch_point_bounds(long long n, const double* pts, double* partials, double* bounds, hipStream_t stream);
hipError_t launch_point_sort(long long n, const double* pts, const PointGrid& g, uint64_t* keys, uint64_t* keys_sorted,
                             uint32_t* order, double* sx, double* sy, double* sz, uint32_t* state, void* tmp,
                             size_t tmp_bytes, hipStream_t stream);
hipError_t launch_sample_count(long long F, long long V, const double* vertices, const void* faces, bool is64,
                               double density, const PointSampleState& s, hipStream_t stream);
hipError_t launch_sample_scan(long long F, const PointSampleState& s, hipStream_t stream);
hipError_t launch_sample_emit(long long F, long long V, unsigned long long S, const double* vertices,
                              const void* faces, bool is64, double density, const PointSampleState& s, double* out,
                              hipStream_t stream);
hipError_t launch_thin_round(const PointThinState& s, const PointGrid& g, double radius, hipStream_t stream);
hipError_t launch_thin_plan(const PointThinState& s, hipStream_t stream);
hipError_t launch_thin_write(const PointThinState& s, long long* kept, hipStream_t stream);
hipError_t launch_nearest_fill(long long Q, double* out, hipStream_t stream);
hipError_t launch_nearest_qsort(long long Q, const double* query, const PointGrid& g, const PointNearestState& s,
                                hipStream_t stream);
hipError_t launch_nearest_search(long long Q, const double* query, long long R, const PointGrid& g,
                                 const PointNearestState& s, double max_dist, double* out, hipStream_t stream);

// TnT F-score evaluation (tnteval.hip): polygon-volume crop, voxel-mean grid, a nearest-point index built
// once and queried many times, the ICP correspondence sums, an in-place 4x4; float64
constexpr int kCropMaxVertices = 1024;  // GSR_CROP_MAX_VERTICES: the polygon's (u, v) pairs fill 16 KB of LDS
constexpr int kIcpMaxSums = 10;         // sums of one accumulate pass (8 or 10), then the bad-index count
struct CropParams {    // by value into the kernels
    double T[12];      // rows 0-2 of the 4x4
    int has_T;
    int u, v, w;       // axes of the polygon plane and of the extrusion
    double axis_min, axis_max;
    int M;             // polygon vertices
};
struct CropState {
    double* poly;     // [M,3] the polygon on the device
    uint32_t* flags;  // [N + 1] kept, then their exclusive scan: flags[N] = the number kept
    void* tmp;
    size_t tmp_bytes;
};
struct VoxelGrid {     // by value into the kernels
    double origin[3];  // min_bound - 0.5 voxel
    double voxel;
    int by, bz;        // key = cx << (by + bz) | cy << bz | cz
};
struct VoxelState {
    double* partials;
    double* bounds;         // [6] min xyz, max xyz
    uint64_t* keys;         // [N] in input order
    uint64_t* keys_sorted;  // [N]
    uint32_t* order;        // [N] input position of each sorted point (a cell's points ascending)
    uint32_t* flags;        // [N + 1] (over keys) run heads, then their exclusive scan: flags[N] = cells
    uint32_t* bad;          // a coordinate is not finite
    void* tmp;
    size_t tmp_bytes;
};
struct PointIndexView {  // the caller's index buffer, carved
    uint64_t* keys;      // [R] sorted packed cell keys
    uint32_t* order;     // [R] original position of each sorted point
    double *x, *y, *z;   // [R] ref in key order
};
struct PointIndexBuildState {
    double* partials;
    double* bounds;
    uint64_t* keys;  // [R] unsorted
    void* tmp;
    size_t tmp_bytes;
};
struct IcpState {
    double* partials;  // [kPeReduceBlocks][kIcpMaxSums + 1]
    double* sums;      // [kIcpMaxSums + 1]
};
size_t carve_crop(void* base, long long N, int M, CropState& s);
size_t carve_voxel(void* base, long long N, VoxelState& s);
size_t carve_point_index(void* base, long long R, PointIndexView& v);
size_t carve_point_index_build(void* base, long long R, PointIndexBuildState& s);
size_t carve_point_query(void* base, long long Q, PointNearestState& s);
size_t carve_icp(void* base, IcpState& s);
hipError_t launch_crop_plan(long long N, const double* points, const CropParams& p, const CropState& s,
                            hipStream_t stream);
hipError_t launch_crop_write(long long N, const double* points, const CropParams& p, const CropState& s,
                             long long* kept, double* out, hipStream_t stream);
hipError_t launch_voxel_keys(long long N, const double* points, const VoxelGrid& g, const VoxelState& s,
                             hipStream_t stream);
hipError_t launch_voxel_sort(long long N, unsigned bits, const VoxelState& s, hipStream_t stream);
hipError_t launch_voxel_plan(long long N, const VoxelState& s, hipStream_t stream);
hipError_t launch_voxel_emit(long long N, const double* points, const VoxelGrid& g, const VoxelState& s, double* means,
                             long long* counts, long long* cells, hipStream_t stream);
hipError_t launch_index_search(long long Q, const double* query, long long R, const PointGrid& g,
                               const PointIndexView& v, const PointNearestState& s, double max_dist, double* dist,
                               long long* index, hipStream_t stream);
hipError_t launch_index_fill(long long Q, double* dist, long long* index, hipStream_t stream);
hipError_t launch_icp_accumulate(int pass, long long N, const double* src, long long R, const double* ref,
                                 const long long* index, const double* means6, const IcpState& s, hipStream_t stream);
hipError_t launch_points_transform(long long N, double* points, const double* T12, hipStream_t stream);

// TnT mesh culling (meshraster.hip): triangle depth raster of one pinhole view and the per-vertex view vote.
// Scratch: 4 bytes per pixel, 12 per triangle and the scan's temporary.
constexpr int kRasterLanePixels = 32;      // a screen bound of at most this many centres: one lane
constexpr int kRasterTile = 64;            // beyond: one wave per kRasterTile x kRasterTile tile of the bound
constexpr int kRasterUnitBlocks = 2048;    // the fixed grid of the wave kernel (4 waves per block)
constexpr uint32_t kRasterEmpty = 0xFFFFFFFFu;  // a depth word no triangle has reached
constexpr int kRasterCounters = 4;         // atomics issued, centres tested, lane triangles, wave units
struct RasterCamera {  // by value into the kernels
    float m[12];       // the first three rows of the world -> camera matrix
    float fx, fy, cx, cy, znear, zfar;
    int W, H;
};
struct MeshRasterState {
    uint32_t* depth;              // [H W] depth bit patterns, kRasterEmpty where nothing was drawn
    uint32_t* units;              // [F + 1] wave units per triangle (0: drawn by its lane, or nothing to draw)
    unsigned long long* offsets;  // [F + 1] their exclusive scan: offsets[F] = the number of units
    uint32_t* bad;                // a face names a vertex outside [0, V)
    unsigned long long* counters;  // [kRasterCounters] (measurement only)
    void* tmp;
    size_t tmp_bytes;
};
size_t carve_mesh_raster(void* base, long long F, int H, int W, MeshRasterState& s);
hipError_t launch_raster_reset(const MeshRasterState& s, hipStream_t stream);
hipError_t launch_raster_clear(const RasterCamera& c, const MeshRasterState& s, hipStream_t stream);
hipError_t launch_raster_setup(const RasterCamera& c, long long V, long long F, const float* vertices,
                               const void* faces, bool is64, bool count, const MeshRasterState& s,
                               hipStream_t stream);
hipError_t launch_raster_scan(long long F, const MeshRasterState& s, hipStream_t stream);
hipError_t launch_raster_units(const RasterCamera& c, long long V, long long F, const float* vertices,
                               const void* faces, bool is64, bool count, const MeshRasterState& s,
                               hipStream_t stream);
hipError_t launch_raster_finish(const RasterCamera& c, const MeshRasterState& s, float* depth, hipStream_t stream);
hipError_t launch_view_vote(const RasterCamera& c, float eps, long long V, const float* vertices,
                            const MeshRasterState& s, int* counts, hipStream_t stream);

// The tetrahedral extraction sweep around `integrate` (fieldsweep.hip): per-view update of a chunk's running
// minimum, the chunk's finish, one bisection step.  No scratch, no readback.
constexpr long long kFieldMaxN = 0x7fffffffll * 256;  // one point or edge per lane, 256 lanes per block
struct FieldView {   // by value into the kernel
    float r[9];      // R, row-major: camera = points @ R + t
    float t[3];
    float c[2], s[2];  // grid_sample coordinates c + s * (camera.xy / camera.z)
    int W, H;        // the mask plane
};
hipError_t launch_field_view_update(const FieldView& v, long long N, const float* points, const float* alpha,
                                    const uint8_t* inside, const float* mask, float* weight, uint8_t* seen,
                                    hipStream_t stream);
hipError_t launch_field_finish(long long N, const float* weight, const uint8_t* seen, float* sdf, uint8_t* valid,
                               hipStream_t stream);
hipError_t launch_field_bisect(long long E, void* left, void* right, bool f64, float* left_sdf, float* right_sdf,
                               const float* mid_sdf, void* mid, hipStream_t stream);

// densify.hip: densify / prune plan and gather, radix-select quantile, 3D filter, opacity reset
constexpr int kMaxDensifyParams = 16;
enum : int { kDensifyCopy = 0, kDensifyXyz = 1, kDensifyScaling = 2 };
struct DensifyParam {
    const float* param;       // [P, width]
    const float* exp_avg;     // [P, width] or null (no optimizer state yet)
    const float* exp_avg_sq;
    float* param_out;         // [N, width]
    float* exp_avg_out;
    float* exp_avg_sq_out;
    int width;
    int role;
};
size_t select_workspace_bytes();
hipError_t launch_radix_quantile(long long n, const float* values, const float* q, float* out, void* workspace,
                                 hipStream_t stream);
size_t densify_workspace_bytes(long long P);
hipError_t launch_densify_plan(long long P, const float* accum, const float* accum_abs, const float* denom,
                               const float* scaling, const float* opacity, float max_grad, float min_opacity,
                               float pd_extent, void* workspace, long long* counts_host, float* q_host,
                               hipStream_t stream);
hipError_t launch_densify_apply(long long P, long long N, long long C, long long S, void* workspace, int32_t* map,
                                bool build_map, const float* noise, const float* rotation, const float* scaling, int n,
                                const DensifyParam* params, hipStream_t stream);
hipError_t launch_filter3d(long long P, const float* xyz, int n_cam, const float* cams, float focal, float* out,
                           uint32_t* max_bits, bool* any_seen, hipStream_t stream);
hipError_t launch_reset_opacity(long long P, const float* scaling, const float* opacity, const float* filter3d,
                                float* out, float* m, float* v, hipStream_t stream);

// Launch order of the per-tile raster kernels, heaviest tile first (longest-
// processing-time-first list scheduling: the tail of a launch is then made
// of short tiles).  Cost = the tile's list length (ranges, forward) or its
// max contributor (backward); one 1024-lane workgroup.
hipError_t launch_tile_order(uint32_t num_tiles, const uint2* ranges, const uint32_t* max_contrib, uint32_t* order,
                             hipStream_t stream);
// the tile order (workgroup 0) and the clearing of [zero, zero + zero_bytes)
// (16-B aligned and sized) in one launch
hipError_t launch_bwd_prepare(void* zero, size_t zero_bytes, uint32_t num_tiles, const uint32_t* max_contrib,
                              uint32_t* order, hipStream_t stream);
// the same for sample_depth's point chunks (count *n_dev <= bound, cost = chunk max contributor)
hipError_t launch_chunk_order(uint32_t bound, const uint32_t* n_dev, const uint32_t* chunk_max, uint32_t* order,
                              hipStream_t stream);
uint32_t sample_chunk_bound(int PN, uint32_t tiles);

// imgmetric.hip: 8-bit quantisation, L1 / MSE and the per-image "valid" SSIM of a batch of image pairs
struct ImageMetricsState {  // per (image, channel, tile) partials
    double* p_ssim;
    unsigned long long* p_s1;
    unsigned long long* p_s2;
};
size_t carve_image_metrics(void* base, int N, int C, int H, int W, int with_ssim, ImageMetricsState& st);
hipError_t launch_image_metrics(int N, int C, int H, int W, int quantize, int with_ssim, const float* render,
                                const float* gt, uint8_t* render_bytes, uint8_t* gt_bytes,
                                const ImageMetricsState& st, double* out, hipStream_t stream);
hipError_t launch_image_quantize8(long long N, int C, int H, int W, const float* image, uint8_t* out,
                                  hipStream_t stream);

// viewprep.hip: Pillow's 8-bit bicubic resample (one pass along one axis) and the float planes of a view
int resample_ksize(int in_size, int out_size);
void resample_coeffs(int in_size, int out_size, int32_t* k, int32_t* bounds);  // host: k [out][ksize], bounds [out][2]
// axis 1: along W, axis 0: along H; k tap-major [ksize][out_size] and bounds [out_size][2] on the device
hipError_t launch_image_resample8(long long N, int H, int W, int C, int axis, int out_size, const uint8_t* in,
                                  uint8_t* out, const int32_t* k, const int32_t* bounds, hipStream_t stream);
hipError_t launch_view_planes(long long N, int H, int W, const uint8_t* rgb, const uint8_t* mask, float* original,
                              float* gray, float* gt_mask, hipStream_t stream);

// ---- model files (modelio.hip): the rows of point_cloud.ply <-> the ten stored tensors ----
// tensors: xyz, features_dc, features_rest, opacity, scaling, rotation, sg_axis, sg_sharpness, sg_color, filter_3D
int model_row_floats(int M, int G);               // A = 18 + 3 (M - 1) + 7 G; 0: out of range
int model_block_rows(int A);                      // rows per workgroup of the pack; 0: no row fits the tile
int model_unpack_block_rows(long long stride);    // rows per workgroup of the unpack; 0: no row fits
hipError_t launch_model_pack_rows(long long P, int M, int G, const float* const* tensors, float* rows,
                                  hipStream_t stream);
hipError_t launch_model_unpack_rows(long long P, int M, int G, long long stride, const uint8_t* rows,
                                    const int32_t* col_offset, const int32_t* col_type, float* const* tensors,
                                    hipStream_t stream);

}  // namespace gsr
