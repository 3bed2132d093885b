// gsr_api.hip — the C ABI (include/gsr.h) of the rasteriser: host orchestration
// of the gfx950 kernels, replacing CudaRasterizer::Rasterizer::{forward,
// backward, markVisible} (CR/rasterizer_impl.cu:186-592), with the point
// queries, the options, the last error and the timing and debug hooks.  The
// other subsystems' entry points are in api_train.hip, api_mesh.hip and
// api_eval.hip; what they all share is in gsr_api_common.h.
//
// Everything is enqueued on the caller's stream.  The forward synchronises
// that stream exactly once, to read K (the number of Gaussian/tile instances)
// and size the binning buffer, like the reference's cudaMemcpy at
// rasterizer_impl.cu:384.  No other host<->device traffic, no device
// allocation (all scratch comes from the caller's allocation callbacks).
//
// The render forward (gsr_rasterize_forward_ex2) and the point queries
// (point_query_forward) share the Gaussian side of a forward, which exists
// once: the geometry and binning carves (carve_alloc_scratch of
// gsr_api_common.h on carve_geom / carve_binning), count_instances
// (preprocess, prefiltered check, K) and build_tile_lists.  Each older public
// entry point forwards to its implementation in one call.
#include <stdio.h>

#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "gsr_api_common.h"

using namespace gsr;

namespace gsr {
ReadbackPool g_readback_pool;

static thread_local std::string g_last_error;

int fail(int code, const char* what, hipError_t e) {
    char buf[512];
    if (e != hipSuccess)
        snprintf(buf, sizeof(buf), "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
    else
        snprintf(buf, sizeof(buf), "%s", what);
    g_last_error = buf;
    return code;
}
}  // namespace gsr

namespace {

// getHigherMsb, CR/rasterizer_impl.cu:37-50
uint32_t higher_msb(uint32_t n) {
    uint32_t msb = sizeof(n) * 4;
    uint32_t step = msb;
    while (step > 1) {
        step /= 2;
        if (n >> msb) msb += step;
        else msb -= step;
    }
    if (n >> msb) msb++;
    return msb;
}

// `tmp`: where the forward-only scratch (scan / depth-sort temporaries) goes; NULL keeps it at the end of the buffer itself.  The
// fields the backward reads come first either way, so it re-carves without
// knowing which layout the forward used.
size_t carve_geom(void* base, int P, uint32_t gx, uint32_t gy, GeomState& g, Carver* tmp = nullptr) {
    Carver c(base);
    Carver& t = tmp ? *tmp : c;
    g.splats = c.take<Splat>(P);
    g.depths = c.take<float>(P);
    g.tiles_touched = c.take<uint32_t>(P);
    g.order = c.take<uint32_t>(P);
    g.depth_keys_sorted = c.take<uint32_t>(P);
    g.tiles_live = c.take<uint32_t>(P);
    g.counts = c.take<uint2>(P);
    g.offsets = c.take<uint2>(P);
    g.radii = c.take<int>(P);
    g.clamped = c.take<uint8_t>(P);
    g.ddir = c.take<float>((size_t)9 * P);
    g.offsets_K = c.take<uint32_t>(1);
    g.near_flag = c.take<uint32_t>(1);
    g.scan_tmp_bytes = scan_temp_bytes(P) > reduce_temp_bytes(P) ? scan_temp_bytes(P) : reduce_temp_bytes(P);
    g.scan_tmp = t.take<char>(g.scan_tmp_bytes);
    g.dsort_tmp_bytes = depth_sort_temp_bytes(P);
    g.dsort_tmp = t.take<char>(g.dsort_tmp_bytes);
    g.foot = t.take<uint4>((size_t)2 * P);
    return c.off + 256;
}

// Binning buffer.  The point list comes first, so its offset depends only on
// the base (gsr_debug_binning carves it knowing K alone); the rest depends
// on the binning path, `lists`: the tile lists of tilelists.hip where the
// grid allows (list_binning), else emit + tile-id sort (binning.hip).
// `tmp` as in carve_geom: the list-building (or key-sort) scratch, dead once
// the point list is written, goes there instead of into the saved buffer.
size_t carve_binning(void* base, int K, int P, uint32_t gx, uint32_t gy, bool lists, BinningState& b,
                     Carver* tmp = nullptr) {
    Carver c(base);
    Carver& t = tmp ? *tmp : c;
    b.point_list = c.take<uint32_t>(K);
    const int tiles = (int)(gx * gy);
    const int tile_bits = (int)higher_msb((uint32_t)tiles);
    b.key_bytes = tile_key_bytes(tile_bits);
    if (lists) {
        b.lists = list_layout(P, K, gx, gy);
        b.rows = t.take<uint2>(K);
        b.qrec = t.take<uint4>((size_t)2 * P);
        b.rows_count = t.take<uint32_t>((size_t)gy * b.lists.nseg_rows);
        b.rows_off = t.take<uint32_t>((size_t)gy * b.lists.nseg_rows);
        b.segbase = t.take<uint32_t>(gy + 1);
        b.tiles_count = t.take<uint32_t>((size_t)gx * b.lists.nseg_tiles_max + 1);
        b.tiles_off = t.take<uint32_t>((size_t)gx * b.lists.nseg_tiles_max + 1);
        b.list_tmp = t.take<char>(b.lists.tmp_bytes);
        b.keys_unsorted = b.keys = nullptr;
        b.values_unsorted = nullptr;
        b.sort_tmp = nullptr;
        b.sort_tmp_bytes = 0;
    } else {
        b.keys_unsorted = t.take<char>((size_t)K * b.key_bytes);
        b.keys = t.take<char>((size_t)K * b.key_bytes);
        b.values_unsorted = t.take<uint32_t>(K);
        b.sort_tmp_bytes = sort_temp_bytes(K, tile_bits);
        b.sort_tmp = t.take<char>(b.sort_tmp_bytes);
    }
    return c.off + 256;
}

size_t carve_image(void* base, int HW, ImageState& s) {
    Carver c(base);
    s.n_contrib = c.take<uint32_t>(HW);
    s.dT_dtm = c.take<float>(HW);
    s.md_check = c.take<uint32_t>(HW);
    return c.off + 256;
}

size_t carve_tiles(void* base, int T, TileState& s) {
    Carver c(base);
    s.ranges = c.take<uint2>(T);
    s.max_contrib = c.take<uint32_t>(T);
    s.order = c.take<uint32_t>(T);
    s.blend_mask = c.take<uint32_t>((size_t)T * kBlendWords);
    s.bwd_cost = c.take<uint32_t>(T);
    return c.off + 256;
}

size_t carve_bwd(void* base, int P, BwdState& s, int T = 0) {
    Carver c(base);
    s.acc = c.take<float>((size_t)P * kAccFields);
    s.acc_abs = c.take<float>(P);
    s.tile_order = c.take<uint32_t>(T);
    return c.off;
}

// The backwards' accumulator block from the caller's callback: carve_bwd at `wb`, the aligned base of
// `wbytes` + 256 bytes.
int alloc_bwd(gsr_alloc_fn alloc, void* ctx, int P, int T, BwdState& s, void*& wb, size_t& wbytes) {
    wbytes = carve_bwd(nullptr, P, s, T);
    void* wbuf = alloc(ctx, wbytes + 256);
    if (!wbuf) return fail(GSR_ERR_ALLOC, "backward buffer allocation failed");
    wb = aligned_base(wbuf);
    carve_bwd(wb, P, s, T);
    return GSR_OK;
}

// sample_depth buffers (the reference's pointBuffer, point_binningBuffer,
// tileBuffer<true> and duplicatedTileBuffer, rasterizer_impl.h)
size_t carve_points(void* base, int PN, PointState& s) {
    Carver c(base);
    s.xy = c.take<float2>(PN);
    s.last = c.take<uint32_t>(PN);
    s.mdepth = c.take<float>(PN);
    s.dT = c.take<float>(PN);
    s.cached = c.take<uint8_t>(PN);
    s.t = c.take<float>(PN);
    return c.off + 256;
}

size_t carve_point_binning(void* base, int PN, uint32_t tiles, PointBinState& s) {
    Carver c(base);
    s.keys_unsorted = c.take<uint32_t>(PN);
    s.keys = c.take<uint32_t>(PN);
    s.pt_list = c.take<uint32_t>(PN);
    // (the retired point sort's key output and temporaries: `keys` and the empty `sort_tmp` stay carved, so
    // the buffer's size and offsets are what callers have sized it for)
    s.sort_tmp_bytes = 0;
    s.sort_tmp = c.take<char>(s.sort_tmp_bytes);
    return c.off + 256;
}

size_t carve_sample_tiles(void* base, int T, TileState& ts, SampleTiles& st) {
    Carver c(base);
    ts.ranges = c.take<uint2>(T);
    ts.max_contrib = c.take<uint32_t>(T);
    st.counts = c.take<uint32_t>(T);
    st.pt_ranges = c.take<uint2>(T);
    st.chunk_off = c.take<uint32_t>((size_t)T + 1);
    st.totals = c.take<uint32_t>(4);
    return c.off + 256;
}

size_t carve_chunks(void* base, uint32_t n, ChunkState& s) {
    Carver c(base);
    s.chunk_max = c.take<uint32_t>(n ? n : 1);
    return c.off + 256;
}

FwdParams make_params(int P, int D, int SHM, int SGD, int SGM, const float* background, int W, int H,
                      const float* means3D, const float* colors_precomp, const float* opacities,
                      const float* scales, const float* rotations, const float* cov3D_precomp, const float* shs,
                      const float* sg_axis, const float* sg_sharpness, const float* sg_color, float scale_modifier,
                      const float* view, const float* proj, const float* campos, float tan_fovx, float tan_fovy,
                      float kernel_size, int require_depth) {
    FwdParams p;
    p.P = P;
    p.D = D;
    p.SHM = SHM;
    p.SGD = SGD;
    p.SGM = SGM;
    p.W = W;
    p.H = H;
    p.background = background;
    p.means3D = means3D;
    p.colors_precomp = colors_precomp;
    p.opacities = opacities;
    p.scales = scales;
    p.rotations = rotations;
    p.cov3D_precomp = cov3D_precomp;
    p.shs = shs;
    p.sg_axis = sg_axis;
    p.sg_sharpness = sg_sharpness;
    p.sg_color = sg_color;
    p.scale_modifier = scale_modifier;
    p.view = view;
    p.proj = proj;
    p.campos = campos;
    p.tan_fovx = tan_fovx;
    p.tan_fovy = tan_fovy;
    p.focal_y = H / (2.0f * tan_fovy);
    p.focal_x = W / (2.0f * tan_fovx);
    p.kernel_size = kernel_size;
    p.grid_x = (W + kTile - 1) / kTile;
    p.grid_y = (H + kTile - 1) / kTile;
    p.require_depth = require_depth != 0;
    p.no_color = false;
    p.cull_pad = 0.f;
    return p;
}

const char* check_params(const FwdParams& p) {
    if (p.P < 0 || p.W <= 0 || p.H <= 0) return "invalid P / image size";
    if (p.P == 0) return nullptr;
    if (!p.means3D || !p.opacities || !p.view || !p.proj || !p.background) return "missing required input";
    if ((p.colors_precomp == nullptr) == (p.shs == nullptr))
        return "Please provide excatly one of either SHs or precomputed colors!";
    const bool have_sr = p.scales && p.rotations;
    if (have_sr == (p.cov3D_precomp != nullptr))
        return "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!";
    if (p.shs && (p.D < 0 || p.D > 3 || p.SHM < (p.D + 1) * (p.D + 1))) return "sh_degree / SH size mismatch";
    if (p.shs && !p.campos) return "campos required for SH colours";
    if (p.SGD < 0 || p.SGD > p.SGM) return "sg_degree exceeds SG lobes";
    if (p.SGD > 0 && (!p.sg_axis || !p.sg_sharpness || !p.sg_color)) return "missing SG tensors";
    return nullptr;
}

// ---- per-stage timing (gsr_timing_*) -------------------------------------
struct TimingRec {
    int stage;
    hipEvent_t e0, e1;
};
std::mutex g_tmu;
bool g_timing = false;
unsigned g_stage_mask = ~0u;
std::vector<TimingRec> g_recs;
std::vector<hipEvent_t> g_pool;

hipEvent_t pool_event() {
    if (!g_pool.empty()) {
        hipEvent_t e = g_pool.back();
        g_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

struct StageTimer {
    hipStream_t stream;
    int stage;
    hipEvent_t e0 = nullptr;
    StageTimer(int st, hipStream_t s) : stream(s), stage(st) {
        std::lock_guard<std::mutex> lk(g_tmu);
        if (!g_timing || !((g_stage_mask >> st) & 1u)) return;
        e0 = pool_event();
        if (e0) (void)hipEventRecord(e0, stream);
    }
    ~StageTimer() {
        if (!e0) return;
        std::lock_guard<std::mutex> lk(g_tmu);
        hipEvent_t e1 = pool_event();
        if (!e1) return;
        (void)hipEventRecord(e1, stream);
        g_recs.push_back({stage, e0, e1});
    }
};

#define GSR_STAGE(stage, expr, what)                          \
    do {                                                      \
        StageTimer _t(stage, stream);                         \
        GSR_TRY(expr, what);                                  \
    } while (0)

// ---- the Gaussian side of a forward (render and point queries) ------------
// CR/auxiliary.h:146-148 (the reference traps the kernel)
const char* kPrefilteredMsg = "Point is filtered although prefiltered is set. This shouldn't happen!";

// Words a caller has read back along with K (the point queries' totals; the
// render forward leaves it empty): `words` (at most 4) from the device
// address `src` into the host array `dst`.
struct ReadWords {
    const uint32_t* src = nullptr;
    int words = 0;
    uint32_t* dst = nullptr;
};

// Preprocess, the `prefiltered` near-plane check and the instance counts.
// Ks.x = K, the reference's instance count (rect tiles): returned as
// num_rendered and the capacity of the binning buffer.  Ks.y = K_live, the
// instances that survive tile culling, which only the instance-sort path
// needs and counts.  `queue_more` queues the caller's own launches whose
// results `more` reads back (both behind the preprocess, before the one host
// wait); it returns GSR_OK or the error it has reported.
template <class Queue>
int count_instances(const FwdParams& p, const GeomState& gs, int* radii, int prefiltered, bool lists,
                    Queue&& queue_more, const ReadWords& more, uint2& Ks, int debug, hipStream_t stream) {
    const int P = p.P;
    GSR_STAGE(GSR_STAGE_PREPROCESS, launch_preprocess_fwd(p, gs, radii, stream), "preprocess");
    if (prefiltered) GSR_TRY(launch_near_violation(P, p.means3D, p.view, gs.near_flag, stream), "prefiltered check");
    uint32_t near_flag = 0;
    Ks = make_uint2(0u, 0u);
    if (lists) {
        // K (and what the caller adds) depends on preprocess only: one readback
        Readback rb;
        GSR_TRY(rb.begin(stream), "pinned readback buffer");
        GSR_STAGE(GSR_STAGE_SCAN, launch_count_k_hist(gs, P, true, stream), "count K");
        if (int rc = queue_more()) return rc;
        GSR_TRY(rb.copy(0, gs.offsets_K, sizeof(uint32_t)), "memcpy K");
        if (more.words) GSR_TRY(rb.copy(4, more.src, more.words * sizeof(uint32_t)), "memcpy totals");
        if (prefiltered) GSR_TRY(rb.copy(1, gs.near_flag, sizeof(uint32_t)), "memcpy prefiltered flag");
        GSR_TRY(rb.commit(), "event record");
        // the GPU sorts by depth while the host waits
        GSR_STAGE(GSR_STAGE_DEPTH_ORDER, launch_depth_sort(gs, P, true, stream), "depth order");
        GSR_TRY(rb.wait(), "event sync");
        Ks.x = rb[0];
        if (prefiltered) near_flag = rb[1];
        for (int k = 0; k < more.words; k++) more.dst[k] = rb[4 + k];
    } else {
        GSR_STAGE(GSR_STAGE_DEPTH_ORDER, launch_depth_sort(gs, P, false, stream), "depth order");
        GSR_STAGE(GSR_STAGE_DEPTH_ORDER, launch_live_counts(p, gs, radii, stream), "live counts");
        GSR_STAGE(GSR_STAGE_SCAN, launch_scan(gs, P, stream), "scan");
        if (int rc = queue_more()) return rc;
        GSR_TRY(hipMemcpyAsync(&Ks, gs.offsets + (P - 1), sizeof(uint2), hipMemcpyDeviceToHost, stream), "memcpy K");
        if (more.words)
            GSR_TRY(hipMemcpyAsync(more.dst, more.src, more.words * sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
                    "memcpy totals");
        if (prefiltered)
            GSR_TRY(hipMemcpyAsync(&near_flag, gs.near_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
                    "memcpy prefiltered flag");
        hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return fail(GSR_ERR_HIP, "stream sync", e);
    }
    if (near_flag) return fail(GSR_ERR_ARGS, kPrefilteredMsg);
    return GSR_OK;
}

// The per-tile lists (point list and ts.ranges) into the carved binning buffer.
int build_tile_lists(const FwdParams& p, const GeomState& gs, const int* radii, const BinningState& bs,
                     const TileState& ts, uint2 Ks, bool lists, int debug, hipStream_t stream) {
    if (lists) {
        GSR_STAGE(GSR_STAGE_TILE_LISTS, launch_list_binning(p, gs, radii, bs, ts, (int)Ks.x, stream), "tile lists");
        return GSR_OK;
    }
    const int tiles = (int)(p.grid_x * p.grid_y), K_live = (int)Ks.y;
    const int tile_bits = (int)higher_msb((uint32_t)tiles);
    GSR_STAGE(GSR_STAGE_EMIT_KEYS, launch_emit_keys(p, gs, radii, bs, stream), "emit keys");
    GSR_STAGE(GSR_STAGE_SORT, launch_sort(bs, K_live, tile_bits, stream), "sort");
    GSR_STAGE(GSR_STAGE_TILE_RANGES, launch_tile_ranges(bs, K_live, ts, tiles, stream), "tile ranges");
    return GSR_OK;
}

// A debug getter's tail: the device-to-host copies queued (one with no destination or no bytes is
// skipped), the stream drained, the error reported as `what`.
struct HostCopy {
    void* dst;
    const void* src;
    size_t bytes;
};
int copy_to_host(std::initializer_list<HostCopy> copies, hipStream_t stream, const char* what) {
    hipError_t e = hipSuccess;
    for (const HostCopy& c : copies)
        if (e == hipSuccess && c.dst && c.bytes)
            e = hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, what, e);
}

}  // namespace

namespace gsr {
static int g_options[kNumOptions] = {};
int option(int which) { return (which >= 0 && which < kNumOptions) ? g_options[which] : 0; }
}  // namespace gsr

extern "C" {

int gsr_debug_render_stats(unsigned long long* out20, int reset) {
    hipError_t e = gsr::read_render_stats(out20, reset != 0);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "render stats", e);
}

int gsr_debug_binning(const void* binning_buffer, const void* tile_buffer, int R, int width, int height,
                      uint32_t* point_list_out, uint32_t* ranges_out, void* stream_ptr) {
    if (!binning_buffer || !tile_buffer || R < 0 || width <= 0 || height <= 0)
        return fail(GSR_ERR_ARGS, "invalid arguments");
    const uint32_t gx = (width + kTile - 1) / kTile, gy = (height + kTile - 1) / kTile;
    const int tiles = (int)(gx * gy);
    BinningState bs;
    {
        Carver c(aligned_base(const_cast<void*>(binning_buffer)));
        bs.point_list = c.take<uint32_t>(R);  // first in every layout (carve_binning)
    }
    TileState ts{};
    carve_tiles(aligned_base(const_cast<void*>(tile_buffer)), tiles, ts);
    return copy_to_host({{point_list_out, bs.point_list, sizeof(uint32_t) * R},
                         {ranges_out, ts.ranges, sizeof(uint2) * tiles}},
                        (hipStream_t)stream_ptr, "debug binning");
}

int gsr_debug_sample_points(const void* point_buffer, int PN, float* median_depth_out, uint32_t* last_out,
                            void* stream_ptr) {
    if (!point_buffer || PN < 0) return fail(GSR_ERR_ARGS, "invalid arguments");
    PointState ps;
    carve_points(aligned_base(const_cast<void*>(point_buffer)), PN, ps);
    return copy_to_host({{median_depth_out, ps.mdepth, sizeof(float) * PN}, {last_out, ps.last, sizeof(uint32_t) * PN}},
                        (hipStream_t)stream_ptr, "debug sample points");
}

int gsr_debug_image(const void* image_buffer, int width, int height, uint32_t* n_contrib_out, void* stream_ptr) {
    if (!image_buffer || width <= 0 || height <= 0 || !n_contrib_out) return fail(GSR_ERR_ARGS, "invalid arguments");
    ImageState is;
    carve_image(aligned_base(const_cast<void*>(image_buffer)), width * height, is);
    return copy_to_host({{n_contrib_out, is.n_contrib, sizeof(uint32_t) * (size_t)width * height}},
                        (hipStream_t)stream_ptr, "debug image");
}

int gsr_debug_tile_stats(const void* tile_buffer, int width, int height, uint32_t* max_contrib_out, void* stream_ptr) {
    if (!tile_buffer || width <= 0 || height <= 0 || !max_contrib_out) return fail(GSR_ERR_ARGS, "invalid arguments");
    const int tiles = (int)(((width + kTile - 1) / kTile) * ((height + kTile - 1) / kTile));
    TileState ts{};
    carve_tiles(aligned_base(const_cast<void*>(tile_buffer)), tiles, ts);
    return copy_to_host({{max_contrib_out, ts.max_contrib, sizeof(uint32_t) * (size_t)tiles}},
                        (hipStream_t)stream_ptr, "debug tile stats");
}

int gsr_debug_depth_sort_tile_keys(int P) { return P < 0 ? -1 : gsr::dsort_tile_keys(P); }

// the GeomState fields the depth sort touches that the caller does not pass, carved out of `scratch`
static size_t carve_depth_sort(void* base, int P, GeomState& g) {
    Carver c(base);
    g.tiles_touched = c.take<uint32_t>(P);
    g.offsets_K = c.take<uint32_t>(1);
    g.dsort_tmp_bytes = depth_sort_temp_bytes(P);
    g.dsort_tmp = c.take<char>(g.dsort_tmp_bytes);
    // never fewer bytes for more keys: where the sort switches to its larger tile its look-back state
    // halves (dsort_temp_bytes drops by ~0.7 MB from 2,000,000 to 2,000,001 keys), so the small tile's
    // state (4 passes x 256 words per tile) is reserved on top there
    const int t0 = dsort_tile_keys(0);
    const size_t slack = dsort_tile_keys(P) > t0 ? (size_t)4 * 256 * sizeof(uint32_t) * ((P + t0 - 1) / t0) : 0;
    return c.off + slack + 256;
}

long long gsr_debug_depth_sort_bytes(int P) {
    if (P < 0) return -1;
    GeomState g{};
    return (long long)carve_depth_sort(nullptr, P, g);
}

int gsr_debug_depth_sort(int P, const uint32_t* keys, uint32_t* keys_sorted, uint32_t* order, void* scratch,
                         int prepared, void* stream_ptr) {
    if (P < 0) return fail(GSR_ERR_ARGS, "invalid arguments");
    if (P == 0) return GSR_OK;
    if (!keys || !keys_sorted || !order || !scratch) return fail(GSR_ERR_ARGS, "invalid arguments");
    hipStream_t stream = (hipStream_t)stream_ptr;
    GeomState gs{};
    carve_depth_sort(aligned_base(scratch), P, gs);
    gs.depths = reinterpret_cast<float*>(const_cast<uint32_t*>(keys));  // (read only)
    gs.depth_keys_sorted = keys_sorted;
    gs.order = order;
    hipError_t e = hipSuccess;
    if (prepared) {
        // what the preprocess leaves behind on the render path: the sort's state and K zeroed; then
        // the fused count + histogram kernel
        uint32_t* first = nullptr;
        size_t words = 0;
        dsort_zero_region(gs.dsort_tmp, P, &first, &words);
        e = hipMemsetAsync(first, 0, words * sizeof(uint32_t), stream);
        if (e == hipSuccess) e = hipMemsetAsync(gs.tiles_touched, 0, sizeof(uint32_t) * (size_t)P, stream);
        if (e == hipSuccess) e = hipMemsetAsync(gs.offsets_K, 0, sizeof(uint32_t), stream);
        if (e == hipSuccess) e = launch_count_k_hist(gs, P, true, stream);
    }
    if (e == hipSuccess) e = launch_depth_sort(gs, P, prepared != 0, stream);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "debug depth sort", e);
}

int gsr_debug_list_constants(int* out, int n) {
    if (n < 0 || (n > 0 && !out)) return -1;
    return gsr::list_constants(out, n);
}

// (cap + kScanTile must fit the kernels' 32-bit indices)
static bool scan_cap_ok(long long cap) { return cap >= 0 && cap <= 0x7fffffffLL; }

long long gsr_debug_scan_excl_bytes(long long cap) {
    if (!scan_cap_ok(cap)) return -1;
    return (long long)sizeof(uint32_t) * gsr::scan_sums_count((size_t)cap);
}

int gsr_debug_scan_excl(const uint32_t* in, uint32_t* out, long long cap, uint32_t n_host, const uint32_t* n_dev,
                        uint32_t mul, void* sums, void* stream_ptr) {
    if (!scan_cap_ok(cap) || !out || !sums || (cap > 0 && !in)) return fail(GSR_ERR_ARGS, "invalid arguments");
    if ((uintptr_t)in % 16) return fail(GSR_ERR_ARGS, "scan input must be 16-byte aligned");
    if ((uintptr_t)out % 4 || (uintptr_t)sums % 4) return fail(GSR_ERR_ARGS, "scan output and sums must be 4-byte aligned");
    if (!n_dev && (long long)n_host > cap) return fail(GSR_ERR_ARGS, "scan length above its bound");
    hipError_t e = gsr::launch_scan_excl(in, out, (size_t)cap, n_host, n_dev, mul, reinterpret_cast<uint32_t*>(sums),
                                         (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "debug scan", e);
}

int gsr_set_option(int opt, int value) {
    if (opt < 0 || opt >= gsr::kNumOptions || gsr::option_retired(opt)) return fail(GSR_ERR_ARGS, "unknown option");
    gsr::g_options[opt] = value;
    return GSR_OK;
}


int gsr_abi_version(void) { return 20; }

int gsr_backward_chunk_size(int P, int chunks) {
    if (P < 0 || chunks < 1) return -1;
    const long long per = ((long long)P + chunks - 1) / chunks;
    return (int)((per + 255) / 256 * 256);
}

int gsr_timing_enable(int on) {
    std::lock_guard<std::mutex> lk(g_tmu);
    g_timing = on != 0;
    return GSR_OK;
}

int gsr_timing_stage_mask(unsigned int mask) {
    std::lock_guard<std::mutex> lk(g_tmu);
    g_stage_mask = mask;
    return GSR_OK;
}

int gsr_timing_collect(double* ms, int* launches) {
    std::vector<TimingRec> recs;
    {
        std::lock_guard<std::mutex> lk(g_tmu);
        recs.swap(g_recs);
    }
    int rc = GSR_OK;
    for (const TimingRec& r : recs) {
        float t = 0.f;
        hipError_t e = hipEventSynchronize(r.e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&t, r.e0, r.e1);
        if (e != hipSuccess) rc = fail(GSR_ERR_HIP, "timing", e);
        if (ms) ms[r.stage] += t;
        if (launches) launches[r.stage] += 1;
    }
    std::lock_guard<std::mutex> lk(g_tmu);
    for (const TimingRec& r : recs) {
        g_pool.push_back(r.e0);
        g_pool.push_back(r.e1);
    }
    return rc;
}

const char* gsr_stage_name(int stage) {
    static const char* names[GSR_NUM_STAGES] = {"preprocess", "scan", "emit_keys", "sort", "tile_ranges",
                                                 "render_fwd", "bwd_clear", "render_bwd", "preprocess_bwd",
                                                 "depth_order", "tile_lists", "sample_points", "sample_fwd",
                                                 "sample_bwd"};
    return (stage >= 0 && stage < GSR_NUM_STAGES) ? names[stage] : "?";
}

const char* gsr_last_error(void) { return g_last_error.c_str(); }

int gsr_rasterize_forward_ex2(gsr_alloc_fn geom_alloc, void* geom_ctx, gsr_alloc_fn binning_alloc, void* binning_ctx,
                             gsr_alloc_fn image_alloc, void* image_ctx, gsr_alloc_fn tile_alloc, void* tile_ctx,
                             int P, int sh_degree, int SHM, int sg_degree, int SGM, const float* background, int width,
                             int height, const float* means3D, const float* colors_precomp, const float* opacities,
                             const float* scales, const float* rotations, const float* cov3D_precomp,
                             const float* shs, const float* sg_axis, const float* sg_sharpness, const float* sg_color,
                             float scale_modifier, const float* viewmatrix, const float* projmatrix,
                             const float* cam_pos, float tan_fovx, float tan_fovy, float kernel_size, int prefiltered,
                             float* out_color, float* out_mdepth, float* out_alpha, float* out_normal, int* radii,
                             int require_depth, int debug, void* stream_ptr, int* num_rendered,
                             gsr_alloc_fn scratch_alloc, void* scratch_ctx, const float* shs_rest) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (num_rendered) *num_rendered = 0;
    FwdParams p = make_params(P, sh_degree, SHM, sg_degree, SGM, background, width, height, means3D, colors_precomp,
                              opacities, scales, rotations, cov3D_precomp, shs, sg_axis, sg_sharpness, sg_color,
                              scale_modifier, viewmatrix, projmatrix, cam_pos, tan_fovx, tan_fovy, kernel_size,
                              require_depth);
    p.shs_rest = shs_rest;
    if (shs_rest && (!shs || SHM < 2)) return fail(GSR_ERR_ARGS, "split SH rows need the DC rows and SHM >= 2");
    if (const char* msg = check_params(p)) return fail(GSR_ERR_ARGS, msg);
    if (!out_color || !out_alpha || !out_mdepth || !out_normal) return fail(GSR_ERR_ARGS, "missing output buffer");
    if (!geom_alloc || !binning_alloc || !image_alloc || !tile_alloc) return fail(GSR_ERR_ARGS, "missing allocator");
    const int tiles = (int)(p.grid_x * p.grid_y);

    // forward-only scratch from scratch_alloc when given (two blocks: the
    // per-Gaussian sort/scan temporaries now, the list-building scratch once
    // K is known), else inside the geometry / binning buffers
    GeomState gs;
    if (int rc = carve_alloc_scratch(geom_alloc, geom_ctx, "geometry buffer allocation failed", scratch_alloc,
                                     scratch_ctx, carve_geom, P, p.grid_x, p.grid_y, gs))
        return rc;
    TileState ts{};
    if (int rc = carve_alloc(tile_alloc, tile_ctx, "tile buffer allocation failed", carve_tiles, tiles, ts)) return rc;
    ImageState is;
    if (int rc = carve_alloc(image_alloc, image_ctx, "image buffer allocation failed", carve_image, width * height, is))
        return rc;
    if (radii == nullptr) radii = gs.radii;

    if (P == 0) {
        // empty scene: background image, zero geometry (rasterize_points.cu:95)
        hipError_t e = hipMemsetAsync(ts.ranges, 0, sizeof(uint2) * tiles, stream);
        if (e == hipSuccess) e = hipMemsetAsync(ts.max_contrib, 0, sizeof(uint32_t) * tiles, stream);
        if (e != hipSuccess) return fail(GSR_ERR_HIP, "memset", e);
        BinningState bs;
        if (int rc = carve_alloc(binning_alloc, binning_ctx, "binning buffer allocation failed", carve_binning, 0, 0,
                                 p.grid_x, p.grid_y, true, bs, nullptr))
            return rc;
        GSR_TRY(launch_render_fwd(p, gs, bs, is, ts, out_color, out_alpha, out_normal, out_mdepth, stream), "render");
        return GSR_OK;
    }

    const bool lists = list_binning(p.grid_x, p.grid_y);
    uint2 Ks;
    if (int rc = count_instances(p, gs, radii, prefiltered, lists, [] { return GSR_OK; }, ReadWords{}, Ks, debug,
                                 stream))
        return rc;
    BinningState bs;
    if (int rc = carve_alloc_scratch(binning_alloc, binning_ctx, "binning buffer allocation failed", scratch_alloc,
                                     scratch_ctx, carve_binning, (int)Ks.x, P, p.grid_x, p.grid_y, lists, bs))
        return rc;
    if (int rc = build_tile_lists(p, gs, radii, bs, ts, Ks, lists, debug, stream)) return rc;
    // Heaviest tile first (LPT, cost = list length) when the grid fills the
    // chip only a few times over: then the last round of long tiles sets the
    // launch's length.  At C3 (8160 tiles, ~5 rounds of 6 blocks per CU) the
    // order saved 8 us of render_fwd for a 12 us ordering launch, so larger
    // grids keep the XCD-contiguous order.
#ifndef GSR_FWD_LPT_MAX_TILES
#define GSR_FWD_LPT_MAX_TILES 4096
#endif
    const bool lpt = tiles <= GSR_FWD_LPT_MAX_TILES;
    if (!lpt) ts.order = nullptr;
    // (one stage: the ordering launch is part of the forward raster's time)
    GSR_STAGE(GSR_STAGE_RENDER_FWD, [&]() {
        if (lpt) {
            const hipError_t e = launch_tile_order((uint32_t)tiles, ts.ranges, nullptr, ts.order, stream);
            if (e != hipSuccess) return e;
        }
        return launch_render_fwd(p, gs, bs, is, ts, out_color, out_alpha, out_normal, out_mdepth, stream);
    }(), "render");
    if (num_rendered) *num_rendered = (int)Ks.x;
    return GSR_OK;
}

int gsr_rasterize_forward_ex(gsr_alloc_fn geom_alloc, void* geom_ctx, gsr_alloc_fn binning_alloc, void* binning_ctx,
                             gsr_alloc_fn image_alloc, void* image_ctx, gsr_alloc_fn tile_alloc, void* tile_ctx,
                             int P, int sh_degree, int SHM, int sg_degree, int SGM, const float* background, int width,
                             int height, const float* means3D, const float* colors_precomp, const float* opacities,
                             const float* scales, const float* rotations, const float* cov3D_precomp,
                             const float* shs, const float* sg_axis, const float* sg_sharpness, const float* sg_color,
                             float scale_modifier, const float* viewmatrix, const float* projmatrix,
                             const float* cam_pos, float tan_fovx, float tan_fovy, float kernel_size, int prefiltered,
                             float* out_color, float* out_mdepth, float* out_alpha, float* out_normal, int* radii,
                             int require_depth, int debug, void* stream_ptr, int* num_rendered,
                             gsr_alloc_fn scratch_alloc, void* scratch_ctx) {
    return gsr_rasterize_forward_ex2(geom_alloc, geom_ctx, binning_alloc, binning_ctx, image_alloc, image_ctx,
                                     tile_alloc, tile_ctx, P, sh_degree, SHM, sg_degree, SGM, background, width,
                                     height, means3D, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                     shs, sg_axis, sg_sharpness, sg_color, scale_modifier, viewmatrix, projmatrix,
                                     cam_pos, tan_fovx, tan_fovy, kernel_size, prefiltered, out_color, out_mdepth,
                                     out_alpha, out_normal, radii, require_depth, debug, stream_ptr, num_rendered,
                                     scratch_alloc, scratch_ctx, nullptr);
}

int gsr_rasterize_forward(gsr_alloc_fn geom_alloc, void* geom_ctx, gsr_alloc_fn binning_alloc, void* binning_ctx,
                          gsr_alloc_fn image_alloc, void* image_ctx, gsr_alloc_fn tile_alloc, void* tile_ctx,
                          int P, int sh_degree, int SHM, int sg_degree, int SGM, const float* background, int width,
                          int height, const float* means3D, const float* colors_precomp, const float* opacities,
                          const float* scales, const float* rotations, const float* cov3D_precomp,
                          const float* shs, const float* sg_axis, const float* sg_sharpness, const float* sg_color,
                          float scale_modifier, const float* viewmatrix, const float* projmatrix,
                          const float* cam_pos, float tan_fovx, float tan_fovy, float kernel_size, int prefiltered,
                          float* out_color, float* out_mdepth, float* out_alpha, float* out_normal, int* radii,
                          int require_depth, int debug, void* stream_ptr, int* num_rendered) {
    return gsr_rasterize_forward_ex2(geom_alloc, geom_ctx, binning_alloc, binning_ctx, image_alloc, image_ctx,
                                     tile_alloc, tile_ctx, P, sh_degree, SHM, sg_degree, SGM, background, width,
                                     height, means3D, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                     shs, sg_axis, sg_sharpness, sg_color, scale_modifier, viewmatrix, projmatrix,
                                     cam_pos, tan_fovx, tan_fovy, kernel_size, prefiltered, out_color, out_mdepth,
                                     out_alpha, out_normal, radii, require_depth, debug, stream_ptr, num_rendered,
                                     nullptr, nullptr, nullptr);
}

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
                           int chunks, gsr_chunk_fn on_chunk, void* chunk_ctx, float* dc_rows,
                              void* stream_ptr, const float* shs_rest, float* dL_dsh_rest) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    BwdParams b;
    b.f = make_params(P, sh_degree, SHM, sg_degree, SGM, background, width, height, means3D, colors_precomp,
                      opacities, scales, rotations, cov3D_precomp, shs, sg_axis, sg_sharpness, sg_color,
                      scale_modifier, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, kernel_size, require_depth);
    if (P == 0) return GSR_OK;
    if (const char* msg = check_params(b.f)) return fail(GSR_ERR_ARGS, msg);
    // (a NULL upstream image gradient is zero: gsr.h)
    if (!geom_buffer || !binning_buffer || !image_buffer || !tile_buffer || !radii || !alphas || !dL_dmean3D ||
        !dL_dmean2D || !dL_dcolor || !dL_dopacity)
        return fail(GSR_ERR_ARGS, "missing backward buffer");
    if (b.f.require_depth && (!normalmap || !mdepth))
        return fail(GSR_ERR_ARGS, "missing geometry buffers for require_depth");
    if (scales && (!dL_dscale || !dL_drot)) return fail(GSR_ERR_ARGS, "missing scale/rotation gradients");
    if (cov3D_precomp && !dL_dcov3D) return fail(GSR_ERR_ARGS, "missing cov3D gradient");
    if (shs && !dL_dsh) return fail(GSR_ERR_ARGS, "missing SH gradient");
    if (SGM > 0 && shs && (!dL_dsg_axis || !dL_dsg_sharpness || !dL_dsg_color))
        return fail(GSR_ERR_ARGS, "missing SG gradients");
    if (chunks < 1) return fail(GSR_ERR_ARGS, "chunks must be >= 1");
    if (dc_rows && !shs) return fail(GSR_ERR_ARGS, "dc_rows needs the SH colour path");
    if (shs_rest && (!shs || SHM < 2 || !dL_dsh_rest))
        return fail(GSR_ERR_ARGS, "split SH rows need the DC rows, SHM >= 2 and both gradients");
    b.f.shs_rest = shs_rest;
    b.dL_dsh_rest = dL_dsh_rest;
    b.R = R;
    b.radii = radii;
    b.alphas = alphas;
    b.normalmap = normalmap;
    b.mdepth = mdepth;
    b.dL_dpix = dL_dpix;
    b.dL_dmdepth = dL_dpix_mdepth;
    b.dL_dalpha = dL_dalphas;
    b.dL_dnormal = dL_dpixel_normals;
    b.dL_dmean3D = dL_dmean3D;
    b.dL_dmean2D = dL_dmean2D;
    b.dL_dcolor = dL_dcolor;
    b.dL_dopacity = dL_dopacity;
    b.dL_dscale = dL_dscale;
    b.dL_drot = dL_drot;
    b.dL_dcov3D = dL_dcov3D;
    b.dL_dsh = dL_dsh;
    b.dL_dsg_axis = dL_dsg_axis;
    b.dL_dsg_sharpness = dL_dsg_sharpness;
    b.dL_dsg_color = dL_dsg_color;

    const int tiles = (int)(b.f.grid_x * b.f.grid_y);
    GeomState gs;
    carve_geom(aligned_base(const_cast<void*>(geom_buffer)), P, b.f.grid_x, b.f.grid_y, gs);
    BinningState bs;  // (the backward reads the point list only: first in every layout)
    carve_binning(aligned_base(const_cast<void*>(binning_buffer)), R, P, b.f.grid_x, b.f.grid_y,
                  list_binning(b.f.grid_x, b.f.grid_y), bs);
    ImageState is;
    carve_image(aligned_base(const_cast<void*>(image_buffer)), width * height, is);
    TileState ts{};
    carve_tiles(aligned_base(const_cast<void*>(tile_buffer)), tiles, ts);
    BwdState ws{};
    void* wb = nullptr;
    size_t wbytes = 0;
    if (int rc = alloc_bwd(geom_bwd_alloc, geom_bwd_ctx, P, tiles, ws, wb, wbytes)) return rc;
    if (tiles > 0) {
        // heaviest tiles first (cost: the forward's per-tile max contributor),
        // ordered by one workgroup while the others clear the accumulators
        const size_t zbytes = (size_t)(reinterpret_cast<char*>(ws.tile_order) - static_cast<char*>(wb));
        GSR_STAGE(GSR_STAGE_BWD_CLEAR,
                  launch_bwd_prepare(wb, zbytes, (uint32_t)tiles, ts.bwd_cost, ws.tile_order, stream),
                  "clear accumulators + tile order");
    } else {
        GSR_STAGE(GSR_STAGE_BWD_CLEAR, hipMemsetAsync(wb, 0, wbytes, stream), "memset accumulators");
        ws.tile_order = nullptr;
    }
    GSR_STAGE(GSR_STAGE_RENDER_BWD, launch_render_bwd(b, gs, bs, is, ts, ws, stream), "render backward");
    // the per-Gaussian backward over `chunks` consecutive Gaussian ranges; after each range's launch
    // the host callback may post work on other streams that waits for it (gsr_dist.OverlappedViewGrads:
    // the range's gradient exchange runs while the next range computes)
    // (ranges of whole 256-Gaussian workgroups; gsr_dist.OverlappedViewGrads reads the size from
    // gsr_backward_chunk_size and checks the ranges it is called with against it)
    const int cs = gsr_backward_chunk_size(P, chunks);
    for (int b0 = 0; b0 < P; b0 += cs) {
        const int b1 = min(P, b0 + cs);
        GSR_STAGE(GSR_STAGE_PREPROCESS_BWD, launch_preprocess_bwd(b, gs, ws, stream, b0, b1, dc_rows),
                  "preprocess backward");
        if (on_chunk) on_chunk(chunk_ctx, b0, b1);
    }
    return GSR_OK;
}

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
                           int chunks, gsr_chunk_fn on_chunk, void* chunk_ctx, float* dc_rows,
                              void* stream_ptr) {
    return gsr_rasterize_backward_ex2(geom_bwd_alloc, geom_bwd_ctx, P, sh_degree, SHM, sg_degree, SGM, R, background, width, height, means3D, colors_precomp, opacities, scales, rotations, cov3D_precomp, shs, sg_axis, sg_sharpness, sg_color, scale_modifier, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, kernel_size, radii, alphas, normalmap, mdepth, geom_buffer, binning_buffer, image_buffer, tile_buffer, dL_dpix, dL_dpix_mdepth, dL_dalphas, dL_dpixel_normals, dL_dmean3D, dL_dmean2D, dL_dcolor, dL_dopacity, dL_dscale, dL_drot, dL_dcov3D, dL_dsh, dL_dsg_axis, dL_dsg_sharpness, dL_dsg_color, require_depth, debug, chunks, on_chunk, chunk_ctx, dc_rows, stream_ptr, nullptr, nullptr);
}

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
                           void* stream_ptr) {
    return gsr_rasterize_backward_ex2(geom_bwd_alloc, geom_bwd_ctx, P, sh_degree, SHM, sg_degree, SGM, R, background,
                                      width, height, means3D, colors_precomp, opacities, scales, rotations,
                                      cov3D_precomp, shs, sg_axis, sg_sharpness, sg_color, scale_modifier, viewmatrix,
                                      projmatrix, campos, tan_fovx, tan_fovy, kernel_size, radii, alphas, normalmap,
                                      mdepth, geom_buffer, binning_buffer, image_buffer, tile_buffer, dL_dpix,
                                      dL_dpix_mdepth, dL_dalphas, dL_dpixel_normals, dL_dmean3D, dL_dmean2D,
                                      dL_dcolor, dL_dopacity, dL_dscale, dL_drot, dL_dcov3D, dL_dsh, dL_dsg_axis,
                                      dL_dsg_sharpness, dL_dsg_color, require_depth, debug, 1, nullptr, nullptr,
                                      nullptr, stream_ptr, nullptr, nullptr);
}

// The point-query forwards (sample_depth, integrate, evaluate_sdf) share
// everything but the raster's mode and outputs: Rasterizer::sampleDepth
// (rasterizer_impl.cu:1042-1261), evaluateTransmittance (:594-815) and
// evaluateSDF (:817-1040) run the same preprocess, Gaussian binning, point
// preprocess and point binning.
static int point_query_forward(int query, gsr_alloc_fn geom_alloc, void* geom_ctx, gsr_alloc_fn binning_alloc,
                               void* binning_ctx, gsr_alloc_fn point_alloc, void* point_ctx,
                               gsr_alloc_fn point_binning_alloc, void* point_binning_ctx, gsr_alloc_fn tile_alloc,
                               void* tile_ctx, gsr_alloc_fn dup_tile_alloc, void* dup_tile_ctx, int PN, int P,
                               int width, int height, const float* points3D, const float* means3D,
                               const float* opacities, const float* scales, float scale_modifier,
                               const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                               const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                               float kernel_size, int prefiltered, float* output, float* output2, uint8_t* inside,
                               int debug, void* stream_ptr, int* num_rendered, int* num_points,
                               int* num_duplicated_tiles, gsr_alloc_fn scratch_alloc = nullptr,
                               void* scratch_ctx = nullptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (num_rendered) *num_rendered = 0;
    if (num_points) *num_points = 0;
    if (num_duplicated_tiles) *num_duplicated_tiles = 0;
    if (P < 0 || PN < 0 || width <= 0 || height <= 0) return fail(GSR_ERR_ARGS, "invalid P / PN / image size");
    if (P == 0 || PN == 0) return GSR_OK;  // rasterize_points.cu:517: nothing sampled, zero outputs
    static const float kZeroBg[3] = {0.f, 0.f, 0.f};
    FwdParams p = make_params(P, 0, 0, 0, 0, kZeroBg, width, height, means3D, nullptr, opacities, scales, rotations,
                              cov3D_precomp, nullptr, nullptr, nullptr, nullptr, scale_modifier, viewmatrix,
                              projmatrix, cam_pos, tan_fovx, tan_fovy, kernel_size, 1);
    p.no_color = true;
    p.cull_pad = 0.5f;
    if (!means3D || !opacities || !viewmatrix || !projmatrix || !points3D) return fail(GSR_ERR_ARGS, "missing input");
    if ((scales && rotations) == (cov3D_precomp != nullptr))
        return fail(GSR_ERR_ARGS, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
    if (!output || !inside || (query == kQuerySDF && !output2)) return fail(GSR_ERR_ARGS, "missing output buffer");
    if (!geom_alloc || !binning_alloc || !point_alloc || !point_binning_alloc || !tile_alloc || !dup_tile_alloc)
        return fail(GSR_ERR_ARGS, "missing allocator");
    const uint32_t tiles = p.grid_x * p.grid_y;

    // forward-only scratch as in gsr_rasterize_forward_ex2
    GeomState gs;
    if (int rc = carve_alloc_scratch(geom_alloc, geom_ctx, "geometry buffer allocation failed", scratch_alloc,
                                     scratch_ctx, carve_geom, P, p.grid_x, p.grid_y, gs))
        return rc;
    TileState ts{};
    SampleTiles st;
    if (int rc = carve_alloc(tile_alloc, tile_ctx, "tile buffer allocation failed", carve_sample_tiles, (int)tiles, ts, st))
        return rc;
    PointState ps;
    if (int rc = carve_alloc(point_alloc, point_ctx, "point buffer allocation failed", carve_points, PN, ps)) return rc;
    PointBinState pb;
    if (int rc = carve_alloc(point_binning_alloc, point_binning_ctx, "point binning buffer allocation failed",
                             carve_point_binning, PN, tiles, pb))
        return rc;

    // the Gaussian side as the render forward; the point totals (points kept, duplicated tiles, chunks)
    // depend on the points only and are read back with K
    const bool lists = list_binning(p.grid_x, p.grid_y);
    uint2 Ks;
    uint32_t totals[4] = {0, 0, 0, 0};
    auto queue_points = [&]() -> int {
        GSR_STAGE(GSR_STAGE_SAMPLE_POINTS, launch_sample_points(p, PN, points3D, ps, pb, st, stream), "sample points");
        GSR_STAGE(GSR_STAGE_SAMPLE_POINTS, launch_sample_setup(PN, tiles, pb, st, stream), "sample setup");
        return GSR_OK;
    };
    if (int rc = count_instances(p, gs, gs.radii, prefiltered, lists, queue_points, ReadWords{st.totals, 4, totals}, Ks,
                                 debug, stream))
        return rc;
    const uint32_t n_chunks = totals[2];
    BinningState bs;
    if (int rc = carve_alloc_scratch(binning_alloc, binning_ctx, "binning buffer allocation failed", scratch_alloc,
                                     scratch_ctx, carve_binning, (int)Ks.x, P, p.grid_x, p.grid_y, lists, bs))
        return rc;
    ChunkState cs{};
    if (int rc = carve_alloc(dup_tile_alloc, dup_tile_ctx, "duplicated-tile buffer allocation failed", carve_chunks,
                             n_chunks, cs))
        return rc;
    if (int rc = build_tile_lists(p, gs, gs.radii, bs, ts, Ks, lists, debug, stream)) return rc;
    // (heaviest-first chunk order with the tile's list length as the cost
    // was measured for this forward: no change, 1.52 vs 1.51 ms at 1.27M points)
    GSR_STAGE(GSR_STAGE_SAMPLE_FWD,
              launch_point_fwd(query, p, gs, bs, ts, ps, pb, st, cs, n_chunks, output, output2, inside, stream),
              "point query");
    if (num_rendered) *num_rendered = (int)Ks.x;
    if (num_points) *num_points = (int)totals[0];
    if (num_duplicated_tiles) *num_duplicated_tiles = (int)totals[1];
    return GSR_OK;
}

int gsr_sample_depth_forward(gsr_alloc_fn geom_alloc, void* geom_ctx, gsr_alloc_fn binning_alloc, void* binning_ctx,
                             gsr_alloc_fn point_alloc, void* point_ctx, gsr_alloc_fn point_binning_alloc,
                             void* point_binning_ctx, gsr_alloc_fn tile_alloc, void* tile_ctx,
                             gsr_alloc_fn dup_tile_alloc, void* dup_tile_ctx, int PN, int P, int width, int height,
                             const float* points3D, const float* means3D, const float* opacities,
                             const float* scales, float scale_modifier, const float* rotations,
                             const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                             const float* cam_pos, float tan_fovx, float tan_fovy, float kernel_size,
                             int prefiltered, float* output, uint8_t* inside, int debug, void* stream_ptr,
                             int* num_rendered, int* num_points, int* num_duplicated_tiles) {
    return point_query_forward(kQuerySample, geom_alloc, geom_ctx, binning_alloc, binning_ctx, point_alloc,
                               point_ctx, point_binning_alloc, point_binning_ctx, tile_alloc, tile_ctx,
                               dup_tile_alloc, dup_tile_ctx, PN, P, width, height, points3D, means3D, opacities,
                               scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos,
                               tan_fovx, tan_fovy, kernel_size, prefiltered, output, nullptr, inside, debug,
                               stream_ptr, num_rendered, num_points, num_duplicated_tiles);
}

int gsr_sample_depth_forward_ex(gsr_alloc_fn geom_alloc, void* geom_ctx, gsr_alloc_fn binning_alloc,
                                void* binning_ctx, gsr_alloc_fn point_alloc, void* point_ctx,
                                gsr_alloc_fn point_binning_alloc, void* point_binning_ctx, gsr_alloc_fn tile_alloc,
                                void* tile_ctx, gsr_alloc_fn dup_tile_alloc, void* dup_tile_ctx, int PN, int P,
                                int width, int height, const float* points3D, const float* means3D,
                                const float* opacities, const float* scales, float scale_modifier,
                                const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                                const float* projmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                                float kernel_size, int prefiltered, float* output, uint8_t* inside, int debug,
                                void* stream_ptr, int* num_rendered, int* num_points, int* num_duplicated_tiles,
                                gsr_alloc_fn scratch_alloc, void* scratch_ctx) {
    return point_query_forward(kQuerySample, geom_alloc, geom_ctx, binning_alloc, binning_ctx, point_alloc,
                               point_ctx, point_binning_alloc, point_binning_ctx, tile_alloc, tile_ctx,
                               dup_tile_alloc, dup_tile_ctx, PN, P, width, height, points3D, means3D, opacities,
                               scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos,
                               tan_fovx, tan_fovy, kernel_size, prefiltered, output, nullptr, inside, debug,
                               stream_ptr, num_rendered, num_points, num_duplicated_tiles, scratch_alloc,
                               scratch_ctx);
}

int gsr_integrate_forward(gsr_alloc_fn geom_alloc, void* geom_ctx, gsr_alloc_fn binning_alloc, void* binning_ctx,
                          gsr_alloc_fn point_alloc, void* point_ctx, gsr_alloc_fn point_binning_alloc,
                          void* point_binning_ctx, gsr_alloc_fn tile_alloc, void* tile_ctx,
                          gsr_alloc_fn dup_tile_alloc, void* dup_tile_ctx, int PN, int P, int width, int height,
                          const float* points3D, const float* means3D, const float* opacities, const float* scales,
                          float scale_modifier, const float* rotations, const float* cov3D_precomp,
                          const float* view2gaussian_precomp, const float* viewmatrix, const float* projmatrix,
                          const float* cam_pos, float tan_fovx, float tan_fovy, float kernel_size, int prefiltered,
                          float* out_transmittance, uint8_t* inside, int debug, void* stream_ptr,
                          int* num_rendered) {
    (void)view2gaussian_precomp;  // unused by the reference (rasterizer_impl.cu:610)
    return point_query_forward(kQueryIntegrate, geom_alloc, geom_ctx, binning_alloc, binning_ctx, point_alloc,
                               point_ctx, point_binning_alloc, point_binning_ctx, tile_alloc, tile_ctx,
                               dup_tile_alloc, dup_tile_ctx, PN, P, width, height, points3D, means3D, opacities,
                               scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos,
                               tan_fovx, tan_fovy, kernel_size, prefiltered, out_transmittance, nullptr, inside,
                               debug, stream_ptr, num_rendered, nullptr, nullptr);
}

int gsr_evaluate_sdf_forward(gsr_alloc_fn geom_alloc, void* geom_ctx, gsr_alloc_fn binning_alloc, void* binning_ctx,
                             gsr_alloc_fn point_alloc, void* point_ctx, gsr_alloc_fn point_binning_alloc,
                             void* point_binning_ctx, gsr_alloc_fn tile_alloc, void* tile_ctx,
                             gsr_alloc_fn dup_tile_alloc, void* dup_tile_ctx, int PN, int P, int width, int height,
                             const float* points3D, const float* means3D, const float* opacities,
                             const float* scales, float scale_modifier, const float* rotations,
                             const float* cov3D_precomp, const float* view2gaussian_precomp,
                             const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                             float tan_fovy, float kernel_size, int prefiltered, float* out_depth, float* out_sdf,
                             uint8_t* inside, int debug, void* stream_ptr, int* num_rendered) {
    (void)view2gaussian_precomp;  // unused by the reference (rasterizer_impl.cu:833)
    return point_query_forward(kQuerySDF, geom_alloc, geom_ctx, binning_alloc, binning_ctx, point_alloc, point_ctx,
                               point_binning_alloc, point_binning_ctx, tile_alloc, tile_ctx, dup_tile_alloc,
                               dup_tile_ctx, PN, P, width, height, points3D, means3D, opacities, scales,
                               scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, cam_pos, tan_fovx,
                               tan_fovy, kernel_size, prefiltered, out_depth, out_sdf, inside, debug, stream_ptr,
                               num_rendered, nullptr, nullptr);
}

int gsr_sample_depth_backward(gsr_alloc_fn geom_bwd_alloc, void* geom_bwd_ctx, int PN, int P, int RN, int R, int TN,
                              int width, int height, const float* points3D, const float* means3D,
                              const float* opacities, const float* scales, float scale_modifier,
                              const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                              const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                              float kernel_size, const void* geom_buffer, const void* binning_buffer,
                              const void* point_buffer, const void* point_binning_buffer, const void* tile_buffer,
                              const void* dup_tile_buffer, const uint8_t* inside, const float* dL_doutput,
                              float* dL_dopacity, float* dL_dmean3D, float* dL_dcov3D, float* dL_dscale,
                              float* dL_drot, float* dL_dpoints3D, int debug, void* stream_ptr) {
    (void)RN;
    (void)TN;
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (P == 0 || PN == 0) return GSR_OK;
    if (P < 0 || PN < 0 || width <= 0 || height <= 0) return fail(GSR_ERR_ARGS, "invalid P / PN / image size");
    static const float kZeroBg[3] = {0.f, 0.f, 0.f};
    SampleBwdParams b;
    b.f = make_params(P, 0, 0, 0, 0, kZeroBg, width, height, means3D, nullptr, opacities, scales, rotations,
                      cov3D_precomp, nullptr, nullptr, nullptr, nullptr, scale_modifier, viewmatrix, projmatrix,
                      campos, tan_fovx, tan_fovy, kernel_size, 1);
    b.f.no_color = true;
    b.f.cull_pad = 0.5f;
    b.PN = PN;
    b.points3D = points3D;
    b.inside = inside;
    b.dL_doutput = dL_doutput;
    b.dL_dpoints3D = dL_dpoints3D;
    if (!geom_buffer || !binning_buffer || !point_buffer || !point_binning_buffer || !tile_buffer ||
        !dup_tile_buffer || !inside || !dL_doutput || !dL_dopacity || !dL_dmean3D || !dL_dpoints3D || !points3D)
        return fail(GSR_ERR_ARGS, "missing backward buffer");
    if (scales && (!dL_dscale || !dL_drot)) return fail(GSR_ERR_ARGS, "missing scale/rotation gradients");
    if (cov3D_precomp && !dL_dcov3D) return fail(GSR_ERR_ARGS, "missing cov3D gradient");
    const uint32_t tiles = b.f.grid_x * b.f.grid_y;
    GeomState gs;
    carve_geom(aligned_base(const_cast<void*>(geom_buffer)), P, b.f.grid_x, b.f.grid_y, gs);
    BinningState bs;  // (the backward reads the point list only: first in every layout)
    carve_binning(aligned_base(const_cast<void*>(binning_buffer)), R, P, b.f.grid_x, b.f.grid_y,
                  list_binning(b.f.grid_x, b.f.grid_y), bs);
    PointState ps;
    carve_points(aligned_base(const_cast<void*>(point_buffer)), PN, ps);
    PointBinState pb;
    carve_point_binning(aligned_base(const_cast<void*>(point_binning_buffer)), PN, tiles, pb);
    TileState ts{};
    SampleTiles st;
    carve_sample_tiles(aligned_base(const_cast<void*>(tile_buffer)), (int)tiles, ts, st);
    ChunkState cs;
    {
        Carver c(aligned_base(const_cast<void*>(dup_tile_buffer)));
        cs.chunk_max = c.take<uint32_t>(1);  // first in the buffer (carve_chunks)
    }
    BwdState ws{};
    const uint32_t bound = PN > 0 ? sample_chunk_bound(PN, tiles) : 0u;
    void* wb = nullptr;
    size_t wbytes = 0;
    if (int rc = alloc_bwd(geom_bwd_alloc, geom_bwd_ctx, P, (int)bound, ws, wb, wbytes)) return rc;
    GSR_STAGE(GSR_STAGE_BWD_CLEAR, hipMemsetAsync(wb, 0, wbytes, stream), "memset accumulators");
    if (bound)  // heaviest chunks first (cost: the forward's chunk max contributor)
        GSR_STAGE(GSR_STAGE_BWD_CLEAR, launch_chunk_order(bound, st.totals + 2, cs.chunk_max, ws.tile_order, stream),
                  "chunk order");
    else
        ws.tile_order = nullptr;
    GSR_STAGE(GSR_STAGE_SAMPLE_BWD, launch_sample_bwd(b, gs, bs, ts, ps, pb, st, cs, ws, stream), "sample backward");
    BwdParams pbw{};
    pbw.f = b.f;
    pbw.R = R;
    pbw.radii = gs.radii;
    pbw.dL_dmean3D = dL_dmean3D;
    pbw.dL_dopacity = dL_dopacity;
    pbw.dL_dscale = dL_dscale;
    pbw.dL_drot = dL_drot;
    pbw.dL_dcov3D = dL_dcov3D;
    GSR_STAGE(GSR_STAGE_PREPROCESS_BWD, launch_preprocess_bwd(pbw, gs, ws, stream), "preprocess backward");
    return GSR_OK;
}

int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, void* stream_ptr) {
    (void)projmatrix;
    if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present))) return fail(GSR_ERR_ARGS, "invalid arguments");
    hipError_t e = launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream_ptr);
    if (e != hipSuccess) return fail(GSR_ERR_HIP, "mark_visible", e);
    return GSR_OK;
}

}  // extern "C"
