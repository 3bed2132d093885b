// gsr_api.hip — the C ABI (include/gsr.h): host orchestration of the gfx950
// kernels, replacing CudaRasterizer::Rasterizer::{forward, backward,
// markVisible} (CR/rasterizer_impl.cu:186-592).
//
// Everything is enqueued on the caller's stream.  The forward synchronises
// that stream exactly once, to read K (the number of Gaussian/tile instances)
// and size the binning buffer, like the reference's cudaMemcpy at
// rasterizer_impl.cu:384.  No other host<->device traffic, no device
// allocation (all scratch comes from the caller's allocation callbacks).
#include <float.h>
#include <math.h>
#include <stdio.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/gsr.h"
#include "gsr_kernels.h"

namespace {

thread_local std::string g_last_error;

// The forward's one host synchronisation (K sizes the binning buffer, as
// rasterizer_impl.cu:384) waits on an event recorded right after the counts
// are copied into pinned host memory, not on the whole stream: work queued
// behind the event (the depth sort) keeps the GPU busy while the host reads
// K and allocates.  The pinned words and the event come from a process-wide
// per-device pool: a forward leases a slot for its readback and returns it,
// so slots are created only up to the number of concurrent forwards and are
// reused by every thread (no per-thread slots left behind by short-lived
// threads; no hipHostMalloc / hipHostFree, which synchronise, per call).
struct HostReadback {
    uint32_t* pinned = nullptr;  // 8 words
    hipEvent_t ev = nullptr;
    int dev = 0;
};
constexpr int kMaxReadbackDevices = 64;

class ReadbackPool {
  public:
    hipError_t acquire(HostReadback*& rb) {
        rb = nullptr;
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev < 0 || dev >= kMaxReadbackDevices) return hipErrorInvalidDevice;
        {
            std::lock_guard<std::mutex> lock(m_);
            if (!free_[dev].empty()) {
                rb = free_[dev].back();
                free_[dev].pop_back();
                return hipSuccess;
            }
        }
        auto* slot = new HostReadback();
        slot->dev = dev;
        if ((e = hipHostMalloc(reinterpret_cast<void**>(&slot->pinned), 8 * sizeof(uint32_t),
                               hipHostMallocDefault)) != hipSuccess) {
            delete slot;
            return e;
        }
        if ((e = hipEventCreateWithFlags(&slot->ev, hipEventDisableTiming)) != hipSuccess) {
            (void)hipHostFree(slot->pinned);
            delete slot;
            return e;
        }
        rb = slot;
        return hipSuccess;
    }
    void release(HostReadback* rb) {
        std::lock_guard<std::mutex> lock(m_);
        free_[rb->dev].push_back(rb);
    }

  private:
    std::mutex m_;
    std::vector<HostReadback*> free_[kMaxReadbackDevices];
};
ReadbackPool g_readback_pool;

// a slot leased for one forward's readback, returned on every exit path.  Copies into the
// slot are queued on `stream` (arm() before the first); the slot's event is recorded after
// the last one (recorded()).  An exit between the two has no event covering the copies, so
// the stream is drained instead; a slot whose copies cannot be proven finished is never
// returned to the pool (another forward could otherwise lease it while a late copy lands).
struct ReadbackLease {
    HostReadback* rb = nullptr;
    hipStream_t stream = nullptr;
    bool armed = false, has_event = false;
    ReadbackLease() = default;
    ReadbackLease(const ReadbackLease&) = delete;
    ReadbackLease& operator=(const ReadbackLease&) = delete;
    void arm(hipStream_t s) { stream = s; armed = true; }
    void recorded() { has_event = true; }
    ~ReadbackLease() {
        if (!rb) return;
        hipError_t e = hipSuccess;
        if (has_event) e = hipEventSynchronize(rb->ev);
        else if (armed) e = hipStreamSynchronize(stream);
        if (e == hipSuccess) g_readback_pool.release(rb);  // (else the slot is leaked, not reused)
    }
};

int fail(int code, const char* what, hipError_t e = hipSuccess) {
    char buf[512];
    if (e != hipSuccess)
        snprintf(buf, sizeof(buf), "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
    else
        snprintf(buf, sizeof(buf), "%s", what);
    g_last_error = buf;
    return code;
}

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

using namespace gsr;

// Binning path: the tile lists of tilelists.hip where the grid allows, else
// the instance sort of binning.hip.
int bin_path(uint32_t gx, uint32_t gy) {
    return list_binning(gx, gy) ? kBinLists : kBinInstanceSort;
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
// on the path: tile lists (tilelists.hip) or emit + tile-id sort.
// `tmp` as in carve_geom: the list-building (or key-sort) scratch, dead once
// the point list is written, goes there instead of into the saved buffer.
size_t carve_binning(void* base, int K, int P, uint32_t gx, uint32_t gy, int path, BinningState& b,
                     Carver* tmp = nullptr) {
    Carver c(base);
    Carver& t = tmp ? *tmp : c;
    b.point_list = c.take<uint32_t>(K);
    const int tiles = (int)(gx * gy);
    const int tile_bits = (int)higher_msb((uint32_t)tiles);
    b.path = path;
    b.use_lists = path == kBinLists;
    b.key_bytes = tile_key_bytes(tile_bits);
    if (b.use_lists) {
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

// 256-B alignment of the carve base (callbacks may return any alignment)
void* aligned_base(void* p) {
    return reinterpret_cast<void*>(align_up(reinterpret_cast<uintptr_t>(p), 256));
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

#define GSR_TRY(expr, what)                                   \
    do {                                                      \
        hipError_t _e = (expr);                               \
        if (_e != hipSuccess) return fail(GSR_ERR_HIP, what, _e); \
        if (debug) {                                          \
            _e = hipStreamSynchronize(stream);                \
            if (_e != hipSuccess) return fail(GSR_ERR_HIP, what, _e); \
        }                                                     \
    } while (0)

#define GSR_STAGE(stage, expr, what)                          \
    do {                                                      \
        StageTimer _t(stage, stream);                         \
        GSR_TRY(expr, what);                                  \
    } while (0)

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
    hipStream_t stream = (hipStream_t)stream_ptr;
    hipError_t e = hipSuccess;
    if (point_list_out && R > 0)
        e = hipMemcpyAsync(point_list_out, bs.point_list, sizeof(uint32_t) * R, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && ranges_out)
        e = hipMemcpyAsync(ranges_out, ts.ranges, sizeof(uint2) * tiles, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "debug binning", e);
}

int gsr_debug_sample_points(const void* point_buffer, int PN, float* median_depth_out, uint32_t* last_out,
                            void* stream_ptr) {
    if (!point_buffer || PN < 0) return fail(GSR_ERR_ARGS, "invalid arguments");
    PointState ps;
    carve_points(aligned_base(const_cast<void*>(point_buffer)), PN, ps);
    hipStream_t stream = (hipStream_t)stream_ptr;
    hipError_t e = hipSuccess;
    if (median_depth_out && PN)
        e = hipMemcpyAsync(median_depth_out, ps.mdepth, sizeof(float) * PN, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && last_out && PN)
        e = hipMemcpyAsync(last_out, ps.last, sizeof(uint32_t) * PN, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "debug sample points", e);
}

int gsr_debug_image(const void* image_buffer, int width, int height, uint32_t* n_contrib_out, void* stream_ptr) {
    if (!image_buffer || width <= 0 || height <= 0 || !n_contrib_out) return fail(GSR_ERR_ARGS, "invalid arguments");
    ImageState is;
    carve_image(aligned_base(const_cast<void*>(image_buffer)), width * height, is);
    hipStream_t stream = (hipStream_t)stream_ptr;
    hipError_t e = hipMemcpyAsync(n_contrib_out, is.n_contrib, sizeof(uint32_t) * (size_t)width * height,
                                  hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "debug image", e);
}

int gsr_debug_tile_stats(const void* tile_buffer, int width, int height, uint32_t* max_contrib_out, void* stream_ptr) {
    if (!tile_buffer || width <= 0 || height <= 0 || !max_contrib_out) return fail(GSR_ERR_ARGS, "invalid arguments");
    const int tiles = (int)(((width + kTile - 1) / kTile) * ((height + kTile - 1) / kTile));
    TileState ts{};
    carve_tiles(aligned_base(const_cast<void*>(tile_buffer)), tiles, ts);
    hipStream_t stream = (hipStream_t)stream_ptr;
    hipError_t e = hipMemcpyAsync(max_contrib_out, ts.max_contrib, sizeof(uint32_t) * (size_t)tiles,
                                  hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "debug tile stats", e);
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

// CR/auxiliary.h:146-148 (the reference traps the kernel)
static const char* kPrefilteredMsg = "Point is filtered although prefiltered is set. This shouldn't happen!";

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
    Carver gtmp(nullptr);
    void* gbuf = geom_alloc(geom_ctx, carve_geom(nullptr, P, p.grid_x, p.grid_y, gs, scratch_alloc ? &gtmp : nullptr));
    if (!gbuf) return fail(GSR_ERR_ALLOC, "geometry buffer allocation failed");
    if (scratch_alloc) {
        void* sbuf = scratch_alloc(scratch_ctx, gtmp.off + 256);
        if (!sbuf) return fail(GSR_ERR_ALLOC, "scratch allocation failed");
        gtmp = Carver(aligned_base(sbuf));
    }
    carve_geom(aligned_base(gbuf), P, p.grid_x, p.grid_y, gs, scratch_alloc ? &gtmp : nullptr);
    TileState ts{};
    void* tbuf = tile_alloc(tile_ctx, carve_tiles(nullptr, tiles, ts));
    if (!tbuf) return fail(GSR_ERR_ALLOC, "tile buffer allocation failed");
    carve_tiles(aligned_base(tbuf), tiles, ts);
    ImageState is;
    void* ibuf = image_alloc(image_ctx, carve_image(nullptr, width * height, is));
    if (!ibuf) return fail(GSR_ERR_ALLOC, "image buffer allocation failed");
    carve_image(aligned_base(ibuf), width * height, is);
    if (radii == nullptr) radii = gs.radii;

    if (P == 0) {
        // empty scene: background image, zero geometry (rasterize_points.cu:95)
        hipError_t e = hipMemsetAsync(ts.ranges, 0, sizeof(uint2) * tiles, stream);
        if (e == hipSuccess) e = hipMemsetAsync(ts.max_contrib, 0, sizeof(uint32_t) * tiles, stream);
        if (e != hipSuccess) return fail(GSR_ERR_HIP, "memset", e);
        BinningState bs;
        void* bbuf = binning_alloc(binning_ctx, carve_binning(nullptr, 0, 0, p.grid_x, p.grid_y, kBinLists, bs));
        if (!bbuf) return fail(GSR_ERR_ALLOC, "binning buffer allocation failed");
        carve_binning(aligned_base(bbuf), 0, 0, p.grid_x, p.grid_y, kBinLists, bs);
        GSR_TRY(launch_render_fwd(p, gs, bs, is, ts, out_color, out_alpha, out_normal, out_mdepth, stream), "render");
        return GSR_OK;
    }

    GSR_STAGE(GSR_STAGE_PREPROCESS, launch_preprocess_fwd(p, gs, radii, stream), "preprocess");
    if (prefiltered) GSR_TRY(launch_near_violation(P, means3D, viewmatrix, gs.near_flag, stream), "prefiltered check");
    uint32_t near_flag = 0;
    const int path = bin_path(p.grid_x, p.grid_y);
    // K = the reference's instance count (rect tiles): returned as
    // num_rendered and the capacity of the binning buffer.  The instance-sort
    // path also needs K_live, the instances that survive tile culling.
    uint2 Ks = make_uint2(0u, 0u);
    if (path != kBinInstanceSort) {
        // K depends on preprocess only: one readback
        ReadbackLease lease;
        GSR_TRY(g_readback_pool.acquire(lease.rb), "pinned readback buffer");
        HostReadback* rb = lease.rb;
        GSR_STAGE(GSR_STAGE_SCAN, launch_count_k_hist(gs, P, path == kBinLists, stream), "count K");
        lease.arm(stream);
        GSR_TRY(hipMemcpyAsync(rb->pinned, gs.offsets_K, sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "memcpy K");
        if (prefiltered)
            GSR_TRY(hipMemcpyAsync(rb->pinned + 1, gs.near_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
                    "memcpy prefiltered flag");
        GSR_TRY(hipEventRecord(rb->ev, stream), "event record");
        lease.recorded();
        // the GPU counts the tile lists (or sorts by depth) while the host waits
        if (path == kBinLists) GSR_STAGE(GSR_STAGE_DEPTH_ORDER, launch_depth_sort(gs, P, true, stream), "depth order");
        GSR_TRY(hipEventSynchronize(rb->ev), "event sync");
        Ks.x = rb->pinned[0];
        if (prefiltered) near_flag = rb->pinned[1];
    } else {
        GSR_STAGE(GSR_STAGE_DEPTH_ORDER, launch_depth_sort(gs, P, false, stream), "depth order");
        GSR_STAGE(GSR_STAGE_DEPTH_ORDER, launch_live_counts(p, gs, radii, stream), "live counts");
        GSR_STAGE(GSR_STAGE_SCAN, launch_scan(gs, P, stream), "scan");
        GSR_TRY(hipMemcpyAsync(&Ks, gs.offsets + (P - 1), sizeof(uint2), hipMemcpyDeviceToHost, stream), "memcpy K");
        if (prefiltered)
            GSR_TRY(hipMemcpyAsync(&near_flag, gs.near_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
                    "memcpy prefiltered flag");
        hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return fail(GSR_ERR_HIP, "stream sync", e);
    }
    if (near_flag) return fail(GSR_ERR_ARGS, kPrefilteredMsg);
    const uint32_t K = Ks.x, K_live = Ks.y;
    BinningState bs;
    Carver btmp(nullptr);
    void* bbuf = binning_alloc(binning_ctx, carve_binning(nullptr, (int)K, P, p.grid_x, p.grid_y, path, bs,
                                                          scratch_alloc ? &btmp : nullptr));
    if (!bbuf) return fail(GSR_ERR_ALLOC, "binning buffer allocation failed");
    if (scratch_alloc) {
        void* sbuf = scratch_alloc(scratch_ctx, btmp.off + 256);
        if (!sbuf) return fail(GSR_ERR_ALLOC, "scratch allocation failed");
        btmp = Carver(aligned_base(sbuf));
    }
    carve_binning(aligned_base(bbuf), (int)K, P, p.grid_x, p.grid_y, path, bs, scratch_alloc ? &btmp : nullptr);
    if (path == kBinLists) {
        GSR_STAGE(GSR_STAGE_TILE_LISTS, launch_list_binning(p, gs, radii, bs, ts, (int)K, stream), "tile lists");
    } else {
        const int tile_bits = (int)higher_msb((uint32_t)tiles);
        GSR_STAGE(GSR_STAGE_EMIT_KEYS, launch_emit_keys(p, gs, radii, bs, stream), "emit keys");
        GSR_STAGE(GSR_STAGE_SORT, launch_sort(bs, (int)K_live, tile_bits, stream), "sort");
        GSR_STAGE(GSR_STAGE_TILE_RANGES, launch_tile_ranges(bs, (int)K_live, ts, tiles, stream), "tile ranges");
    }
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
    if (num_rendered) *num_rendered = (int)K;
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
    return gsr_rasterize_forward_ex(geom_alloc, geom_ctx, binning_alloc, binning_ctx, image_alloc, image_ctx,
                                    tile_alloc, tile_ctx, P, sh_degree, SHM, sg_degree, SGM, background, width,
                                    height, means3D, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                    shs, sg_axis, sg_sharpness, sg_color, scale_modifier, viewmatrix, projmatrix,
                                    cam_pos, tan_fovx, tan_fovy, kernel_size, prefiltered, out_color, out_mdepth,
                                    out_alpha, out_normal, radii, require_depth, debug, stream_ptr, num_rendered,
                                    nullptr, nullptr);
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
                  bin_path(b.f.grid_x, b.f.grid_y), bs);
    ImageState is;
    carve_image(aligned_base(const_cast<void*>(image_buffer)), width * height, is);
    TileState ts{};
    carve_tiles(aligned_base(const_cast<void*>(tile_buffer)), tiles, ts);
    BwdState ws{};
    const size_t wbytes = carve_bwd(nullptr, P, ws, tiles);
    void* wbuf = geom_bwd_alloc(geom_bwd_ctx, wbytes + 256);
    if (!wbuf) return fail(GSR_ERR_ALLOC, "backward buffer allocation failed");
    void* wb = aligned_base(wbuf);
    carve_bwd(wb, P, ws, tiles);
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
    return gsr_rasterize_backward_ex(geom_bwd_alloc, geom_bwd_ctx, P, sh_degree, SHM, sg_degree, SGM, R, background,
                                     width, height, means3D, colors_precomp, opacities, scales, rotations,
                                     cov3D_precomp, shs, sg_axis, sg_sharpness, sg_color, scale_modifier, viewmatrix,
                                     projmatrix, campos, tan_fovx, tan_fovy, kernel_size, radii, alphas, normalmap,
                                     mdepth, geom_buffer, binning_buffer, image_buffer, tile_buffer, dL_dpix,
                                     dL_dpix_mdepth, dL_dalphas, dL_dpixel_normals, dL_dmean3D, dL_dmean2D, dL_dcolor,
                                     dL_dopacity, dL_dscale, dL_drot, dL_dcov3D, dL_dsh, dL_dsg_axis,
                                     dL_dsg_sharpness, dL_dsg_color, require_depth, debug, 1, nullptr, nullptr,
                                     nullptr, stream_ptr);
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

    // forward-only scratch as in gsr_rasterize_forward_ex
    GeomState gs;
    Carver gtmp(nullptr);
    void* gbuf = geom_alloc(geom_ctx, carve_geom(nullptr, P, p.grid_x, p.grid_y, gs, scratch_alloc ? &gtmp : nullptr));
    if (!gbuf) return fail(GSR_ERR_ALLOC, "geometry buffer allocation failed");
    if (scratch_alloc) {
        void* sbuf = scratch_alloc(scratch_ctx, gtmp.off + 256);
        if (!sbuf) return fail(GSR_ERR_ALLOC, "scratch allocation failed");
        gtmp = Carver(aligned_base(sbuf));
    }
    carve_geom(aligned_base(gbuf), P, p.grid_x, p.grid_y, gs, scratch_alloc ? &gtmp : nullptr);
    TileState ts{};
    SampleTiles st;
    void* tbuf = tile_alloc(tile_ctx, carve_sample_tiles(nullptr, (int)tiles, ts, st));
    if (!tbuf) return fail(GSR_ERR_ALLOC, "tile buffer allocation failed");
    carve_sample_tiles(aligned_base(tbuf), (int)tiles, ts, st);
    PointState ps;
    void* pbuf = point_alloc(point_ctx, carve_points(nullptr, PN, ps));
    if (!pbuf) return fail(GSR_ERR_ALLOC, "point buffer allocation failed");
    carve_points(aligned_base(pbuf), PN, ps);
    PointBinState pb;
    void* pbbuf = point_binning_alloc(point_binning_ctx, carve_point_binning(nullptr, PN, tiles, pb));
    if (!pbbuf) return fail(GSR_ERR_ALLOC, "point binning buffer allocation failed");
    carve_point_binning(aligned_base(pbbuf), PN, tiles, pb);

    GSR_STAGE(GSR_STAGE_PREPROCESS, launch_preprocess_fwd(p, gs, gs.radii, stream), "preprocess");
    if (prefiltered) GSR_TRY(launch_near_violation(P, means3D, viewmatrix, gs.near_flag, stream), "prefiltered check");
    uint32_t near_flag = 0;
    const int path = bin_path(p.grid_x, p.grid_y);  // as the render forward
    uint2 Ks = make_uint2(0u, 0u);
    uint32_t totals[4] = {0, 0, 0, 0};
    if (path != kBinInstanceSort) {
        // K, the tile list sizes and the point totals depend on preprocess and
        // the points only: one readback (HostReadback)
        ReadbackLease lease;
        GSR_TRY(g_readback_pool.acquire(lease.rb), "pinned readback buffer");
        HostReadback* rb = lease.rb;
        GSR_STAGE(GSR_STAGE_SCAN, launch_count_k_hist(gs, P, path == kBinLists, stream), "count K");
        GSR_STAGE(GSR_STAGE_SAMPLE_POINTS, launch_sample_points(p, PN, points3D, ps, pb, st, stream), "sample points");
        GSR_STAGE(GSR_STAGE_SAMPLE_POINTS, launch_sample_setup(PN, tiles, pb, st, stream), "sample setup");
        lease.arm(stream);
        GSR_TRY(hipMemcpyAsync(rb->pinned, gs.offsets_K, sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "memcpy K");
        GSR_TRY(hipMemcpyAsync(rb->pinned + 4, st.totals, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
                "memcpy totals");
        if (prefiltered)
            GSR_TRY(hipMemcpyAsync(rb->pinned + 1, gs.near_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
                    "memcpy prefiltered flag");
        GSR_TRY(hipEventRecord(rb->ev, stream), "event record");
        lease.recorded();
        // the GPU counts the tile lists (or sorts by depth) while the host waits
        if (path == kBinLists) GSR_STAGE(GSR_STAGE_DEPTH_ORDER, launch_depth_sort(gs, P, true, stream), "depth order");
        GSR_TRY(hipEventSynchronize(rb->ev), "event sync");
        Ks.x = rb->pinned[0];
        if (prefiltered) near_flag = rb->pinned[1];
        for (int k = 0; k < 4; k++) totals[k] = rb->pinned[4 + k];
    } else {
        GSR_STAGE(GSR_STAGE_DEPTH_ORDER, launch_depth_sort(gs, P, false, stream), "depth order");
        GSR_STAGE(GSR_STAGE_DEPTH_ORDER, launch_live_counts(p, gs, gs.radii, stream), "live counts");
        GSR_STAGE(GSR_STAGE_SCAN, launch_scan(gs, P, stream), "scan");
        GSR_STAGE(GSR_STAGE_SAMPLE_POINTS, launch_sample_points(p, PN, points3D, ps, pb, st, stream), "sample points");
        GSR_STAGE(GSR_STAGE_SAMPLE_POINTS, launch_sample_setup(PN, tiles, pb, st, stream), "sample setup");
        GSR_TRY(hipMemcpyAsync(&Ks, gs.offsets + (P - 1), sizeof(uint2), hipMemcpyDeviceToHost, stream), "memcpy K");
        GSR_TRY(hipMemcpyAsync(totals, st.totals, sizeof(totals), hipMemcpyDeviceToHost, stream), "memcpy totals");
        if (prefiltered)
            GSR_TRY(hipMemcpyAsync(&near_flag, gs.near_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
                    "memcpy prefiltered flag");
        hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return fail(GSR_ERR_HIP, "stream sync", e);
    }
    if (near_flag) return fail(GSR_ERR_ARGS, kPrefilteredMsg);
    const uint32_t K = Ks.x, K_live = Ks.y, n_chunks = totals[2];
    BinningState bs;
    Carver btmp(nullptr);
    void* bbuf = binning_alloc(binning_ctx, carve_binning(nullptr, (int)K, P, p.grid_x, p.grid_y, path, bs,
                                                          scratch_alloc ? &btmp : nullptr));
    if (!bbuf) return fail(GSR_ERR_ALLOC, "binning buffer allocation failed");
    if (scratch_alloc) {
        void* sbuf = scratch_alloc(scratch_ctx, btmp.off + 256);
        if (!sbuf) return fail(GSR_ERR_ALLOC, "scratch allocation failed");
        btmp = Carver(aligned_base(sbuf));
    }
    carve_binning(aligned_base(bbuf), (int)K, P, p.grid_x, p.grid_y, path, bs, scratch_alloc ? &btmp : nullptr);
    ChunkState cs{};
    void* cbuf = dup_tile_alloc(dup_tile_ctx, carve_chunks(nullptr, n_chunks, cs));
    if (!cbuf) return fail(GSR_ERR_ALLOC, "duplicated-tile buffer allocation failed");
    carve_chunks(aligned_base(cbuf), n_chunks, cs);
    if (path == kBinLists) {
        GSR_STAGE(GSR_STAGE_TILE_LISTS, launch_list_binning(p, gs, gs.radii, bs, ts, (int)K, stream), "tile lists");
    } else {
        const int tile_bits = (int)higher_msb(tiles);
        GSR_STAGE(GSR_STAGE_EMIT_KEYS, launch_emit_keys(p, gs, gs.radii, bs, stream), "emit keys");
        GSR_STAGE(GSR_STAGE_SORT, launch_sort(bs, (int)K_live, tile_bits, stream), "sort");
        GSR_STAGE(GSR_STAGE_TILE_RANGES, launch_tile_ranges(bs, (int)K_live, ts, (int)tiles, stream), "tile ranges");
    }
    // (heaviest-first chunk order with the tile's list length as the cost
    // was measured for this forward: no change, 1.52 vs 1.51 ms at 1.27M points)
    GSR_STAGE(GSR_STAGE_SAMPLE_FWD,
              launch_point_fwd(query, p, gs, bs, ts, ps, pb, st, cs, n_chunks, output, output2, inside, stream),
              "point query");
    if (num_rendered) *num_rendered = (int)K;
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
                  bin_path(b.f.grid_x, b.f.grid_y), bs);
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
    const size_t wbytes = carve_bwd(nullptr, P, ws, (int)bound);
    void* wbuf = geom_bwd_alloc(geom_bwd_ctx, wbytes + 256);
    if (!wbuf) return fail(GSR_ERR_ALLOC, "backward buffer allocation failed");
    void* wb = aligned_base(wbuf);
    carve_bwd(wb, P, ws, (int)bound);
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
    void* buf = scratch_alloc(scratch_ctx, carve_knn(nullptr, P, ks));
    if (!buf) return fail(GSR_ERR_ALLOC, "distCUDA2: scratch allocation failed");
    carve_knn(aligned_base(buf), P, ks);
    hipError_t e = launch_knn(P, points, ks, mean_dists, (hipStream_t)stream_ptr);
    return e == hipSuccess ? GSR_OK : fail(GSR_ERR_HIP, "distCUDA2", e);
}

namespace {
// optional per-stage GPU times of gsr_marching_tetrahedra (measurement only): a begin and an end
// event around each stage, read after the call's last kernel
struct TetStageTimes {
    static constexpr int kStages = 7;
    hipEvent_t ev[kStages][2] = {};
    bool used[kStages] = {};
    bool on = false;
    hipStream_t stream = nullptr;
    hipError_t begin(int k) {
        if (!on) return hipSuccess;
        hipError_t e = hipEventCreate(&ev[k][0]);
        if (e == hipSuccess) e = hipEventCreate(&ev[k][1]);
        if (e == hipSuccess) e = hipEventRecord(ev[k][0], stream);
        used[k] = e == hipSuccess;
        return e;
    }
    hipError_t end(int k) { return on ? hipEventRecord(ev[k][1], stream) : hipSuccess; }
    hipError_t collect(float* ms) {
        if (!on) return hipSuccess;
        hipError_t e = hipStreamSynchronize(stream);
        for (int k = 0; k < kStages + 1; k++) ms[k] = 0.f;
        for (int k = 0; k < kStages && e == hipSuccess; k++)
            if (used[k]) e = hipEventElapsedTime(&ms[k], ev[k][0], ev[k][1]);
        return e;
    }
    ~TetStageTimes() {
        for (auto& p : ev)
            for (hipEvent_t x : p)
                if (x) (void)hipEventDestroy(x);
    }
};
}  // namespace

int gsr_marching_tetrahedra(gsr_alloc_fn edge_alloc, void* edge_ctx, gsr_alloc_fn face_alloc, void* face_ctx,
                            gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long T, long long V,
                            const void* tets, int tets_int64, const float* sdf, const uint8_t* valid,
                            long long* num_edges, long long* num_faces, float* stage_ms, void* stream_ptr) {
    constexpr int debug = 0;
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (!num_edges || !num_faces) return fail(GSR_ERR_ARGS, "marching_tetrahedra: missing count outputs");
    *num_edges = *num_faces = 0;
    if (stage_ms)
        for (int k = 0; k < 8; k++) stage_ms[k] = 0.f;
    if (T < 0 || V < 0) return fail(GSR_ERR_ARGS, "marching_tetrahedra: negative size");
    if (T == 0) return GSR_OK;
    if (V <= 0) return fail(GSR_ERR_ARGS, "marching_tetrahedra: tets without vertices (V <= 0)");
    if (!tets || !sdf || !valid) return fail(GSR_ERR_ARGS, "marching_tetrahedra: missing input");
    if (!edge_alloc || !face_alloc || !scratch_alloc) return fail(GSR_ERR_ARGS, "marching_tetrahedra: missing allocator");
    if (reinterpret_cast<uintptr_t>(tets) % 16) return fail(GSR_ERR_ARGS, "marching_tetrahedra: tets must be 16-byte aligned");
    if (V > 0x7fffffffll || T > 0xffffffffll)
        return fail(GSR_ERR_ARGS, "marching_tetrahedra: more than 2^31 - 1 vertices or 2^32 - 1 tets");
    const bool is64 = tets_int64 != 0;
    TetStageTimes times;
    times.on = stage_ms != nullptr;
    times.stream = stream;

    TetCountState cs;
    void* buf = scratch_alloc(scratch_ctx, carve_tet_count(nullptr, V, T, cs));
    if (!buf) return fail(GSR_ERR_ALLOC, "marching_tetrahedra: scratch allocation failed");
    carve_tet_count(aligned_base(buf), V, T, cs);
    GSR_TRY(times.begin(0), "event");
    GSR_TRY(launch_tet_flags(V, sdf, valid, cs, stream), "tet vertex flags");
    GSR_TRY(times.end(0), "event");
    GSR_TRY(times.begin(1), "event");
    GSR_TRY(launch_tet_count(T, V, tets, is64, cs, stream), "tet count");
    GSR_TRY(times.end(1), "event");

    // first readback: the totals of one- and two-triangle tets and the bad-id flag
    ReadbackLease lease;
    GSR_TRY(g_readback_pool.acquire(lease.rb), "pinned readback buffer");
    HostReadback* rb = lease.rb;
    lease.arm(stream);
    GSR_TRY(hipMemcpyAsync(rb->pinned, cs.partials + cs.nblocks, sizeof(uint64_t), hipMemcpyDeviceToHost, stream),
            "memcpy tet counts");
    GSR_TRY(hipMemcpyAsync(rb->pinned + 2, cs.bad, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
            "memcpy vertex id flag");
    GSR_TRY(hipEventRecord(rb->ev, stream), "event record");
    lease.recorded();
    GSR_TRY(hipEventSynchronize(rb->ev), "event sync");
    if (rb->pinned[2]) return fail(GSR_ERR_ARGS, "marching_tetrahedra: a tet names a vertex outside [0, V)");
    const uint64_t n1 = rb->pinned[0], n2 = rb->pinned[1];
    const uint64_t S = 3 * n1 + 4 * n2, F = n1 + 2 * n2;
    if (S == 0) {
        GSR_TRY(times.collect(stage_ms), "stage times");
        return GSR_OK;
    }
    if (S > 0xffffffffull) return fail(GSR_ERR_ARGS, "marching_tetrahedra: more than 2^32 - 1 crossing-edge slots");

    TetEdgeState es;
    const int bits = tet_key_bits(V);
    buf = scratch_alloc(scratch_ctx, carve_tet_edges(nullptr, (size_t)S, bits, es));
    if (!buf) return fail(GSR_ERR_ALLOC, "marching_tetrahedra: scratch allocation failed");
    carve_tet_edges(aligned_base(buf), (size_t)S, bits, es);
    GSR_TRY(times.begin(2), "event");
    GSR_TRY(launch_tet_emit(T, V, tets, is64, cs, es, stream), "tet edge keys");
    GSR_TRY(times.end(2), "event");
    GSR_TRY(times.begin(3), "event");
    GSR_TRY(launch_tet_sort(es, stream), "tet edge sort");
    GSR_TRY(times.end(3), "event");
    GSR_TRY(times.begin(4), "event");
    GSR_TRY(launch_tet_ranks(es, stream), "tet edge ranks");
    GSR_TRY(times.end(4), "event");

    // second readback: E, the number of distinct keys
    GSR_TRY(hipMemcpyAsync(rb->pinned + 3, es.heads + (S - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
            "memcpy edge count");
    GSR_TRY(hipEventRecord(rb->ev, stream), "event record");
    GSR_TRY(hipEventSynchronize(rb->ev), "event sync");
    const uint64_t E = rb->pinned[3];
    void* edge_ids = edge_alloc(edge_ctx, (size_t)E * 2 * sizeof(long long));
    if (!edge_ids) return fail(GSR_ERR_ALLOC, "marching_tetrahedra: edge_ids allocation failed");
    void* faces = face_alloc(face_ctx, (size_t)F * 3 * sizeof(long long));
    if (!faces) return fail(GSR_ERR_ALLOC, "marching_tetrahedra: faces allocation failed");
    GSR_TRY(times.begin(5), "event");
    GSR_TRY(launch_tet_edges(es, (long long*)edge_ids, stream), "tet edges");
    GSR_TRY(times.end(5), "event");
    GSR_TRY(times.begin(6), "event");
    GSR_TRY(launch_tet_faces(T, V, tets, is64, cs, es, (long long*)faces, stream), "tet faces");
    GSR_TRY(times.end(6), "event");
    GSR_TRY(times.collect(stage_ms), "stage times");
    *num_edges = (long long)E;
    *num_faces = (long long)F;
    return GSR_OK;
}

int gsr_mesh_clusters(gsr_alloc_fn count_alloc, void* count_ctx, gsr_alloc_fn area_alloc, void* area_ctx,
                      gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long F, long long V, const void* faces,
                      int faces_int64, const float* vertices, long long* triangle_clusters, long long* num_clusters,
                      float* stage_ms, void* stream_ptr) {
    constexpr int debug = 0;
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (!num_clusters) return fail(GSR_ERR_ARGS, "mesh_clusters: missing count output");
    *num_clusters = 0;
    if (stage_ms)
        for (int k = 0; k < 8; k++) stage_ms[k] = 0.f;
    if (F < 0 || V < 0) return fail(GSR_ERR_ARGS, "mesh_clusters: negative size");
    if (F == 0) return GSR_OK;
    if (F >= 0x80000000ll || V > 0x80000000ll)
        return fail(GSR_ERR_ARGS, "mesh_clusters: 2^31 or more triangles, or more than 2^31 vertices");
    if (V == 0) return fail(GSR_ERR_ARGS, "mesh_clusters: faces without vertices (V <= 0)");
    if (!faces || !triangle_clusters) return fail(GSR_ERR_ARGS, "mesh_clusters: missing buffer");
    if (!count_alloc || !scratch_alloc || (vertices && !area_alloc))
        return fail(GSR_ERR_ARGS, "mesh_clusters: missing allocator");
    const bool is64 = faces_int64 != 0, area = vertices != nullptr;
    TetStageTimes times;
    times.on = stage_ms != nullptr;
    times.stream = stream;

    MeshClusterState cs;
    void* buf = scratch_alloc(scratch_ctx, carve_mesh_clusters(nullptr, F, V, area, cs));
    if (!buf) return fail(GSR_ERR_ALLOC, "mesh_clusters: scratch allocation failed");
    carve_mesh_clusters(aligned_base(buf), F, V, area, cs);
    GSR_TRY(times.begin(0), "event");
    GSR_TRY(launch_clean_keys(V, faces, is64, cs, stream), "mesh edge keys");
    GSR_TRY(times.end(0), "event");
    GSR_TRY(times.begin(1), "event");
    GSR_TRY(launch_clean_sort(cs, stream), "mesh edge sort");
    GSR_TRY(times.end(1), "event");
    GSR_TRY(times.begin(2), "event");
    GSR_TRY(launch_clean_union(cs, stream), "mesh union");
    GSR_TRY(times.end(2), "event");
    GSR_TRY(times.begin(3), "event");
    GSR_TRY(launch_clean_flatten(cs, stream), "mesh flatten");
    GSR_TRY(times.end(3), "event");
    GSR_TRY(times.begin(4), "event");
    GSR_TRY(launch_clean_ids(cs, stream), "mesh cluster ids");
    GSR_TRY(times.end(4), "event");

    // the one readback: C and the bad-id flag
    ReadbackLease lease;
    GSR_TRY(g_readback_pool.acquire(lease.rb), "pinned readback buffer");
    HostReadback* rb = lease.rb;
    lease.arm(stream);
    GSR_TRY(hipMemcpyAsync(rb->pinned, cs.cid + F, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
            "memcpy cluster count");
    GSR_TRY(hipMemcpyAsync(rb->pinned + 1, cs.flags + cs.rounds + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
            "memcpy vertex id flag");
    GSR_TRY(hipEventRecord(rb->ev, stream), "event record");
    lease.recorded();
    GSR_TRY(hipEventSynchronize(rb->ev), "event sync");
    if (rb->pinned[1]) return fail(GSR_ERR_ARGS, "mesh_clusters: a face names a vertex outside [0, V)");
    const long long C = rb->pinned[0];
    void* counts = count_alloc(count_ctx, (size_t)C * sizeof(long long));
    if (!counts) return fail(GSR_ERR_ALLOC, "mesh_clusters: cluster_n_triangles allocation failed");
    void* areas = area ? area_alloc(area_ctx, (size_t)C * sizeof(double)) : nullptr;
    if (area && !areas) return fail(GSR_ERR_ALLOC, "mesh_clusters: cluster_area allocation failed");
    GSR_TRY(times.begin(5), "event");
    GSR_TRY(launch_clean_counts(cs, triangle_clusters, (long long*)counts, stream), "mesh cluster counts");
    GSR_TRY(times.end(5), "event");
    if (area) {
        GSR_TRY(times.begin(6), "event");
        GSR_TRY(launch_clean_area(C, faces, is64, vertices, cs, (double*)areas, stream), "mesh cluster areas");
        GSR_TRY(times.end(6), "event");
    }
    GSR_TRY(times.collect(stage_ms), "stage times");
    *num_clusters = C;
    return GSR_OK;
}

int gsr_mesh_filter(gsr_alloc_fn vertex_alloc, void* vertex_ctx, gsr_alloc_fn face_alloc, void* face_ctx,
                    gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long F, long long V, long long C,
                    const float* vertices, const void* faces, int faces_int64, const long long* triangle_clusters,
                    const long long* cluster_n_triangles, const long long* n_min, long long* num_vertices,
                    long long* num_faces, void* stream_ptr) {
    constexpr int debug = 0;
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
    void* buf = scratch_alloc(scratch_ctx, carve_mesh_filter(nullptr, F, V, fs));
    if (!buf) return fail(GSR_ERR_ALLOC, "mesh_filter: scratch allocation failed");
    carve_mesh_filter(aligned_base(buf), F, V, fs);
    GSR_TRY(launch_filter_plan(F, V, C, faces, is64, triangle_clusters, cluster_n_triangles, n_min, fs, stream),
            "mesh filter plan");

    // the one readback: V', F' and the bad-id flag
    ReadbackLease lease;
    GSR_TRY(g_readback_pool.acquire(lease.rb), "pinned readback buffer");
    HostReadback* rb = lease.rb;
    lease.arm(stream);
    GSR_TRY(hipMemcpyAsync(rb->pinned, fs.vmap + V, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
            "memcpy vertex count");
    GSR_TRY(hipMemcpyAsync(rb->pinned + 1, fs.fmap + F, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
            "memcpy face count");
    GSR_TRY(hipMemcpyAsync(rb->pinned + 2, fs.bad, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
            "memcpy id flag");
    GSR_TRY(hipEventRecord(rb->ev, stream), "event record");
    lease.recorded();
    GSR_TRY(hipEventSynchronize(rb->ev), "event sync");
    if (rb->pinned[2])
        return fail(GSR_ERR_ARGS, "mesh_filter: a face names a vertex outside [0, V) or a cluster outside [0, C)");
    const long long Vn = rb->pinned[0], Fn = rb->pinned[1];
    void* vout = Vn ? vertex_alloc(vertex_ctx, (size_t)Vn * 3 * sizeof(float)) : nullptr;
    if (Vn && !vout) return fail(GSR_ERR_ALLOC, "mesh_filter: vertices allocation failed");
    void* fout = Fn ? face_alloc(face_ctx, (size_t)Fn * 3 * sizeof(long long)) : nullptr;
    if (Fn && !fout) return fail(GSR_ERR_ALLOC, "mesh_filter: faces allocation failed");
    GSR_TRY(launch_filter_gather(F, V, vertices, faces, is64, fs, (float*)vout, (long long*)fout, stream),
            "mesh filter gather");
    *num_vertices = Vn;
    *num_faces = Fn;
    return GSR_OK;
}

namespace {
const char* tsdf_camera(const float* intrinsic, const float* extrinsic, TsdfCamera& cam) {
    if (!intrinsic || !extrinsic) return "missing camera";
    cam.fx = intrinsic[0], cam.fy = intrinsic[1], cam.cx = intrinsic[2], cam.cy = intrinsic[3];
    if (!(cam.fx > 0.f) || !(cam.fy > 0.f)) return "focal lengths must be positive";
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) cam.e[r][c] = extrinsic[4 * r + c];
    return nullptr;
}
}  // namespace

int gsr_tsdf_touch(gsr_alloc_fn coord_alloc, void* coord_ctx, gsr_alloc_fn scratch_alloc, void* scratch_ctx,
                   const float* depth, int H, int W, const float* intrinsic, const float* extrinsic,
                   float depth_scale, float depth_max, float sdf_trunc, float block_size, long long* num_blocks,
                   void* stream_ptr) {
    constexpr int debug = 0;
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
    void* buf = scratch_alloc(scratch_ctx, carve_tsdf_touch(nullptr, H, W, ts));
    if (!buf) return fail(GSR_ERR_ALLOC, "tsdf_touch: scratch allocation failed");
    carve_tsdf_touch(aligned_base(buf), H, W, ts);
    GSR_TRY(launch_tsdf_touch(H, W, depth, cam, depth_scale, depth_max, sdf_trunc, block_size, ts, stream),
            "tsdf touch");

    // the one readback: the number of blocks and the out-of-range flag
    ReadbackLease lease;
    GSR_TRY(g_readback_pool.acquire(lease.rb), "pinned readback buffer");
    HostReadback* rb = lease.rb;
    lease.arm(stream);
    GSR_TRY(hipMemcpyAsync(rb->pinned, ts.heads + ts.n, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
            "memcpy block count");
    GSR_TRY(hipMemcpyAsync(rb->pinned + 1, ts.bad, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
            "memcpy range flag");
    GSR_TRY(hipEventRecord(rb->ev, stream), "event record");
    lease.recorded();
    GSR_TRY(hipEventSynchronize(rb->ev), "event sync");
    if (rb->pinned[1]) return fail(GSR_ERR_ARGS, "tsdf_touch: a sample falls in a block beyond +-2^20");
    const long long n = rb->pinned[0];
    if (n == 0) return GSR_OK;
    void* coords = coord_alloc(coord_ctx, (size_t)n * 3 * sizeof(int));
    if (!coords) return fail(GSR_ERR_ALLOC, "tsdf_touch: block coordinate allocation failed");
    GSR_TRY(launch_tsdf_touch_write(ts, (int*)coords, stream), "tsdf touch write");
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
    constexpr int debug = 0;
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (!num_vertices || !num_faces) return fail(GSR_ERR_ARGS, "tsdf_extract: missing count outputs");
    *num_vertices = *num_faces = 0;
    if (stage_ms)
        for (int k = 0; k < 8; k++) stage_ms[k] = 0.f;
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
    TetStageTimes times;
    times.on = stage_ms != nullptr;
    times.stream = stream;

    TsdfExtractState es;
    void* buf = scratch_alloc(scratch_ctx, carve_tsdf_extract(nullptr, (int)num_blocks, block_resolution, es));
    if (!buf) return fail(GSR_ERR_ALLOC, "tsdf_extract: scratch allocation failed");
    carve_tsdf_extract(aligned_base(buf), (int)num_blocks, block_resolution, es);
    GSR_TRY(times.begin(0), "event");
    GSR_TRY(launch_mc_mark(keys, sorted_slots, tsdf, weight, weight_threshold, es, stream), "marching cubes mark");
    GSR_TRY(times.end(0), "event");
    GSR_TRY(times.begin(1), "event");
    GSR_TRY(launch_mc_count(es, stream), "marching cubes count");
    GSR_TRY(times.end(1), "event");

    // the one readback: V and F
    ReadbackLease lease;
    GSR_TRY(g_readback_pool.acquire(lease.rb), "pinned readback buffer");
    HostReadback* rb = lease.rb;
    lease.arm(stream);
    GSR_TRY(hipMemcpyAsync(rb->pinned, es.vbase + num_blocks, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
            "memcpy vertex count");
    GSR_TRY(hipMemcpyAsync(rb->pinned + 1, es.fbase + num_blocks, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
            "memcpy face count");
    GSR_TRY(hipEventRecord(rb->ev, stream), "event record");
    lease.recorded();
    GSR_TRY(hipEventSynchronize(rb->ev), "event sync");
    const long long V = rb->pinned[0], F = rb->pinned[1];
    if (F == 0) {  // a vertex exists only on an emitted cube's crossed edge, and such a cube has a triangle
        GSR_TRY(times.collect(stage_ms), "stage times");
        return GSR_OK;
    }
    void* vout = vertex_alloc(vertex_ctx, (size_t)V * 3 * sizeof(float));
    if (!vout) return fail(GSR_ERR_ALLOC, "tsdf_extract: vertices allocation failed");
    void* cout = color ? color_alloc(color_ctx, (size_t)V * 3 * sizeof(float)) : nullptr;
    if (color && !cout) return fail(GSR_ERR_ALLOC, "tsdf_extract: colours allocation failed");
    void* fout = face_alloc(face_ctx, (size_t)F * 3 * sizeof(long long));
    if (!fout) return fail(GSR_ERR_ALLOC, "tsdf_extract: faces allocation failed");
    GSR_TRY(times.begin(2), "event");
    GSR_TRY(launch_mc_vertices(keys, sorted_slots, tsdf, color, voxel_size, es, (float*)vout, (float*)cout, stream),
            "marching cubes vertices");
    GSR_TRY(times.end(2), "event");
    GSR_TRY(times.begin(3), "event");
    GSR_TRY(launch_mc_faces(keys, es, (long long*)fout, stream), "marching cubes faces");
    GSR_TRY(times.end(3), "event");
    GSR_TRY(times.collect(stage_ms), "stage times");
    *num_vertices = V;
    *num_faces = F;
    return GSR_OK;
}

int gsr_mesh_sample_points(gsr_alloc_fn point_alloc, void* point_ctx, gsr_alloc_fn scratch_alloc, void* scratch_ctx,
                           long long V, long long F, const double* vertices, const void* faces, int faces_int64,
                           double density, long long* num_points, float* stage_ms, void* stream_ptr) {
    constexpr int debug = 0;
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (!num_points) return fail(GSR_ERR_ARGS, "mesh_sample_points: missing count output");
    *num_points = 0;
    if (stage_ms)
        for (int k = 0; k < 8; k++) stage_ms[k] = 0.f;
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
    TetStageTimes times;
    times.on = stage_ms != nullptr;
    times.stream = stream;

    unsigned long long S = 0;
    PointSampleState ss{};
    if (F > 0) {
        void* buf = scratch_alloc(scratch_ctx, carve_point_sample(nullptr, F, ss));
        if (!buf) return fail(GSR_ERR_ALLOC, "mesh_sample_points: scratch allocation failed");
        carve_point_sample(aligned_base(buf), F, ss);
        GSR_TRY(times.begin(0), "event");
        GSR_TRY(launch_sample_count(F, V, vertices, faces, is64, density, ss, stream), "sample count");
        GSR_TRY(times.end(0), "event");
        GSR_TRY(times.begin(1), "event");
        GSR_TRY(launch_sample_scan(F, ss, stream), "sample scan");
        GSR_TRY(times.end(1), "event");
        // the one readback: S (two words) and the bad flag
        ReadbackLease lease;
        GSR_TRY(g_readback_pool.acquire(lease.rb), "pinned readback buffer");
        HostReadback* rb = lease.rb;
        lease.arm(stream);
        GSR_TRY(hipMemcpyAsync(rb->pinned, ss.offsets + F, sizeof(uint64_t), hipMemcpyDeviceToHost, stream),
                "memcpy sample count");
        GSR_TRY(hipMemcpyAsync(rb->pinned + 2, ss.bad, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
                "memcpy face flag");
        GSR_TRY(hipEventRecord(rb->ev, stream), "event record");
        lease.recorded();
        GSR_TRY(hipEventSynchronize(rb->ev), "event sync");
        if (rb->pinned[2])
            return fail(GSR_ERR_ARGS, "mesh_sample_points: a face names a vertex outside [0, V), or a triangle is "
                                      "not finite");
        S = (unsigned long long)rb->pinned[0] | (unsigned long long)rb->pinned[1] << 32;
        if (S >= (1ull << 38)) return fail(GSR_ERR_ARGS, "mesh_sample_points: 2^38 or more sampled points");
    }
    double* out = (double*)point_alloc(point_ctx, ((size_t)V + (size_t)S) * 3 * sizeof(double));
    if (!out) return fail(GSR_ERR_ALLOC, "mesh_sample_points: points allocation failed");
    GSR_TRY(times.begin(2), "event");
    GSR_TRY(hipMemcpyAsync(out, vertices, (size_t)V * 3 * sizeof(double), hipMemcpyDeviceToDevice, stream),
            "copy vertices");
    if (S > 0) GSR_TRY(launch_sample_emit(F, V, S, vertices, faces, is64, density, ss, out, stream), "sample emit");
    GSR_TRY(times.end(2), "event");
    GSR_TRY(times.collect(stage_ms), "stage times");
    *num_points = V + (long long)S;
    return GSR_OK;
}

int gsr_points_downsample(gsr_alloc_fn kept_alloc, void* kept_ctx, gsr_alloc_fn scratch_alloc, void* scratch_ctx,
                          long long N, const double* points, double radius, long long* num_kept,
                          long long* num_rounds, float* stage_ms, void* stream_ptr) {
    constexpr int debug = 0;
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (!num_kept) return fail(GSR_ERR_ARGS, "points_downsample: missing count output");
    *num_kept = 0;
    if (num_rounds) *num_rounds = 0;
    if (stage_ms)
        for (int k = 0; k < 8; k++) stage_ms[k] = 0.f;
    if (N < 0) return fail(GSR_ERR_ARGS, "points_downsample: negative size");
    if (!(radius > 0.0) || !(radius < HUGE_VAL))
        return fail(GSR_ERR_ARGS, "points_downsample: radius must be positive and finite");
    if (N == 0) return GSR_OK;
    if (N >= 0x80000000ll) return fail(GSR_ERR_ARGS, "points_downsample: 2^31 or more points");
    if (!points) return fail(GSR_ERR_ARGS, "points_downsample: missing buffer");
    if (!kept_alloc || !scratch_alloc) return fail(GSR_ERR_ARGS, "points_downsample: missing allocator");
    TetStageTimes times;
    times.on = stage_ms != nullptr;
    times.stream = stream;

    PointThinState ts;
    void* buf = scratch_alloc(scratch_ctx, carve_point_thin(nullptr, N, ts));
    if (!buf) return fail(GSR_ERR_ALLOC, "points_downsample: scratch allocation failed");
    carve_point_thin(aligned_base(buf), N, ts);
    GSR_TRY(times.begin(0), "event");
    GSR_TRY(launch_point_bounds(N, points, ts.partials, ts.bounds, stream), "point bounds");
    GSR_TRY(times.end(0), "event");
    // first readback: the bounds, which size the grid
    double bounds[6];
    GSR_TRY(hipMemcpyAsync(bounds, ts.bounds, sizeof(bounds), hipMemcpyDeviceToHost, stream), "memcpy bounds");
    GSR_TRY(hipStreamSynchronize(stream), "stream sync");
    PointGrid grid;
    if (!point_thin_grid(bounds, radius, grid))
        return fail(GSR_ERR_ARGS, "points_downsample: points are not finite, or span 2^31 or more cells of side radius");
    GSR_TRY(times.begin(1), "event");
    GSR_TRY(launch_point_sort(N, points, grid, ts.keys, ts.keys_sorted, ts.order, ts.sx, ts.sy, ts.sz, ts.state, ts.tmp,
                              ts.tmp_bytes, stream),
            "point cell sort");
    GSR_TRY(times.end(1), "event");

    ReadbackLease lease;
    GSR_TRY(g_readback_pool.acquire(lease.rb), "pinned readback buffer");
    HostReadback* rb = lease.rb;
    lease.arm(stream);
    // a round decides at least the lowest undecided rank, so N rounds are the most there can be
    long long rounds = 0;
    GSR_TRY(times.begin(2), "event");
    for (;;) {
        GSR_TRY(launch_thin_round(ts, grid, radius, stream), "thinning round");
        rounds++;
        GSR_TRY(hipMemcpyAsync(rb->pinned, ts.undecided, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
                "memcpy undecided flag");
        GSR_TRY(hipEventRecord(rb->ev, stream), "event record");
        lease.recorded();
        GSR_TRY(hipEventSynchronize(rb->ev), "event sync");
        if (!rb->pinned[0]) break;
        if (rounds > N) return fail(GSR_ERR_HIP, "points_downsample: the rounds did not end");
    }
    GSR_TRY(times.end(2), "event");
    GSR_TRY(times.begin(3), "event");
    GSR_TRY(launch_thin_plan(ts, stream), "thinning plan");
    GSR_TRY(times.end(3), "event");
    GSR_TRY(hipMemcpyAsync(rb->pinned + 1, ts.flags + N, sizeof(uint32_t), hipMemcpyDeviceToHost, stream),
            "memcpy kept count");
    GSR_TRY(hipEventRecord(rb->ev, stream), "event record");
    GSR_TRY(hipEventSynchronize(rb->ev), "event sync");
    const long long M = rb->pinned[1];
    void* kept = kept_alloc(kept_ctx, (size_t)M * sizeof(long long));
    if (!kept) return fail(GSR_ERR_ALLOC, "points_downsample: kept allocation failed");
    GSR_TRY(times.begin(4), "event");
    GSR_TRY(launch_thin_write(ts, (long long*)kept, stream), "thinning write");
    GSR_TRY(times.end(4), "event");
    GSR_TRY(times.collect(stage_ms), "stage times");
    *num_kept = M;
    if (num_rounds) *num_rounds = rounds;
    return GSR_OK;
}

int gsr_points_nearest(gsr_alloc_fn scratch_alloc, void* scratch_ctx, long long Q, const double* query, long long R,
                       const double* ref, double max_dist, double* dist, float* stage_ms, void* stream_ptr) {
    constexpr int debug = 0;
    hipStream_t stream = (hipStream_t)stream_ptr;
    if (stage_ms)
        for (int k = 0; k < 8; k++) stage_ms[k] = 0.f;
    if (Q < 0 || R < 0) return fail(GSR_ERR_ARGS, "points_nearest: negative size");
    if (!(max_dist > 0.0)) return fail(GSR_ERR_ARGS, "points_nearest: max_dist must be positive");
    if (Q == 0) return GSR_OK;
    if (Q >= 0x80000000ll || R >= 0x80000000ll) return fail(GSR_ERR_ARGS, "points_nearest: 2^31 or more points");
    if (!query || !dist || (R > 0 && !ref)) return fail(GSR_ERR_ARGS, "points_nearest: missing buffer");
    if (R == 0) {
        GSR_TRY(launch_nearest_fill(Q, dist, stream), "nearest fill");
        return GSR_OK;
    }
    if (!scratch_alloc) return fail(GSR_ERR_ARGS, "points_nearest: missing allocator");
    TetStageTimes times;
    times.on = stage_ms != nullptr;
    times.stream = stream;

    PointNearestState ns;
    void* buf = scratch_alloc(scratch_ctx, carve_point_nearest(nullptr, Q, R, ns));
    if (!buf) return fail(GSR_ERR_ALLOC, "points_nearest: scratch allocation failed");
    carve_point_nearest(aligned_base(buf), Q, R, ns);
    GSR_TRY(times.begin(0), "event");
    GSR_TRY(launch_point_bounds(R, ref, ns.partials, ns.bounds, stream), "ref bounds");
    GSR_TRY(times.end(0), "event");
    // the one readback: the bounds of ref, which size the grid
    double bounds[6];
    GSR_TRY(hipMemcpyAsync(bounds, ns.bounds, sizeof(bounds), hipMemcpyDeviceToHost, stream), "memcpy bounds");
    GSR_TRY(hipStreamSynchronize(stream), "stream sync");
    for (double b : bounds)
        if (!(b > -DBL_MAX && b < DBL_MAX)) return fail(GSR_ERR_ARGS, "points_nearest: ref is not finite");
    PointGrid grid;
    point_nearest_grid(bounds, R, grid);
    GSR_TRY(times.begin(1), "event");
    GSR_TRY(launch_point_sort(R, ref, grid, ns.rkeys, ns.rkeys_sorted, ns.rorder, ns.rx, ns.ry, ns.rz, nullptr, ns.tmp,
                              ns.tmp_bytes, stream),
            "ref cell sort");
    GSR_TRY(times.end(1), "event");
    GSR_TRY(times.begin(2), "event");
    GSR_TRY(launch_nearest_qsort(Q, query, grid, ns, stream), "query sort");
    GSR_TRY(times.end(2), "event");
    GSR_TRY(times.begin(3), "event");
    GSR_TRY(launch_nearest_search(Q, query, R, grid, ns, max_dist, dist, stream), "nearest search");
    GSR_TRY(times.end(3), "event");
    GSR_TRY(times.collect(stage_ms), "stage times");
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
