// densify.hip — the consumer of the densification statistics on gfx950:
// GaussianModel.densify_and_prune (scene/gaussian_model.py:613-816), the 3D
// filter (compute_3D_filter, :225-262) and reset_opacity (:521-539).
//
// The reference clones, splits and prunes with boolean-mask indexing and
// torch.cat over 9 parameters, 18 Adam moments and 4 statistics, three times
// per call.  Here the decisions of all three passes are taken per ORIGINAL
// point in one plan, and every output row is written once:
//   plan   1. densify_grads_kernel   grads = accum / denom (NaN -> 0), the
//             per-point tests (grads >= max_grad, max exp(s) > pd * extent,
//             sigmoid(o) < min_opacity) and the count of the first;
//          2. radix select (select_hist_kernel / select_pick_kernel, 4 x 8
//             bits, LDS integer histograms) of the two order statistics of
//             torch.quantile's linear rule -> Q, on the device;
//          3. densify_flags_kernel   the clone / split decisions, with the
//             reference's quirk that the split pass sees the appended clones
//             with gradient 0 (a clone is split again exactly when 0 >= Q);
//          4. rocPRIM exclusive scan of six counters per point; the totals
//             give C, S, pruned, N (one readback).
//   apply  5. densify_map_kernel     every original writes the map entries of
//             its up to five destinations: final layout [surviving originals |
//             surviving clones | surviving children copy 0 | copy 1], each in
//             source order (originals before clones among the children);
//          6. densify_apply_kernel   lanes over the flattened (row, column)
//             range of every tensor: gather the parameter and the moments.
// Offsets come from scans only and the only atomics are integer adds, so two
// runs give the same bits.  Row offsets are 64-bit; point indices and noise
// rows are stored as int32 (P <= 2^31 / 5, checked by the caller).
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "gsr_kernels.h"

namespace gsr {

// ------------------------------------------------------------ radix select
// k-th smallest of n non-negative floats (bit patterns ordered as uint32):
// four passes over 8 bits, most significant first.  Two targets (the ranks
// below and above of the interpolation) are tracked together; while their
// prefixes agree one histogram serves both.
struct SelectState {
    unsigned long long hist[4][2][256];
    unsigned long long k[2];   // rank of each target among the values that share its prefix
    unsigned long long n_hi;   // (plan) points with grads >= max_grad
    uint32_t prefix[2];        // the bits decided so far
    uint32_t same;             // the two prefixes agree
    float weight;              // rank - floor(rank)
    float Q;
};

// rank = q (n - 1) in fp32, below / above = floor / ceil, as ATen's quantile
// (rank and weight are two tensor operations there, each rounded: contracted into one fma, rank - floor
// keeps the product's unrounded tail, up to half an ulp of the rank, and Q moves by that times b - a)
__global__ void select_init_kernel(SelectState* st, long long n, const float* q_in, long long P_ratio) {
#pragma clang fp contract(off)
    float q;
    if (q_in)
        q = *q_in;
    else  // the plan: 1 - mean(grads >= max_grad)
        q = 1.f - (float)st->n_hi / (float)P_ratio;
    q = fminf(fmaxf(q, 0.f), 1.f);
    const float rank = q * (float)(n - 1);
    long long lo = (long long)floorf(rank), hi = (long long)ceilf(rank);
    lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);
    hi = hi < 0 ? 0 : (hi > n - 1 ? n - 1 : hi);
    st->k[0] = (unsigned long long)lo;
    st->k[1] = (unsigned long long)hi;
    st->prefix[0] = st->prefix[1] = 0u;
    st->same = 1u;
    st->weight = rank - (float)lo;
}

__global__ void __launch_bounds__(256) select_hist_kernel(SelectState* st, int pass, long long n,
                                                          const float* __restrict__ values) {
    __shared__ uint32_t s_hist[2][256];
    s_hist[0][threadIdx.x] = 0u;
    s_hist[1][threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t mask = pass == 0 ? 0u : ~0u << (shift + 8);
    const uint32_t p0 = st->prefix[0], p1 = st->prefix[1];
    const bool same = st->same != 0u;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const uint32_t b = __float_as_uint(values[i]);
        const uint32_t d = (b >> shift) & 255u;
        if ((b & mask) == p0) atomicAdd(&s_hist[0][d], 1u);
        if (!same && (b & mask) == p1) atomicAdd(&s_hist[1][d], 1u);
    }
    __syncthreads();
    const uint32_t c0 = s_hist[0][threadIdx.x], c1 = s_hist[1][threadIdx.x];
    if (c0) atomicAdd(&st->hist[pass][0][threadIdx.x], (unsigned long long)c0);
    if (c1) atomicAdd(&st->hist[pass][1][threadIdx.x], (unsigned long long)c1);
}

// one thread: the digit of each target in this pass; after the last pass the interpolation
// (ATen Lerp.h: a + w (b - a) for w < 0.5, else b - (b - a)(1 - w))
__global__ void select_pick_kernel(SelectState* st, int pass, float* q_out) {
    const int shift = 24 - 8 * pass;
    const bool same = st->same != 0u;
    for (int t = 0; t < 2; t++) {
        const unsigned long long* h = st->hist[pass][same ? 0 : t];
        unsigned long long cum = 0, k = st->k[t];
        int d = 0;
        for (; d < 255; d++) {
            if (k < cum + h[d]) break;
            cum += h[d];
        }
        st->k[t] = k - cum;
        st->prefix[t] |= (uint32_t)d << shift;
    }
    st->same = st->prefix[0] == st->prefix[1] ? 1u : 0u;
    if (pass == 3) {
        const float a = __uint_as_float(st->prefix[0]), b = __uint_as_float(st->prefix[1]), w = st->weight;
        const float diff = b - a;
        const float Q = fabsf(w) < 0.5f ? a + w * diff : b - diff * (1.f - w);
        st->Q = Q;
        if (q_out) *q_out = Q;
    }
}

static hipError_t run_select(SelectState* st, long long n, const float* values, const float* q_in, long long P_ratio,
                             float* q_out, hipStream_t stream) {
    hipLaunchKernelGGL(select_init_kernel, dim3(1), dim3(1), 0, stream, st, n, q_in, P_ratio);
    const long long want = (n + 256ll * 8 - 1) / (256ll * 8);
    const unsigned grid = (unsigned)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
    for (int pass = 0; pass < 4; pass++) {
        hipLaunchKernelGGL(select_hist_kernel, dim3(grid), dim3(256), 0, stream, st, pass, n, values);
        hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(1), 0, stream, st, pass, q_out);
    }
    return hipGetLastError();
}

size_t select_workspace_bytes() { return align_up(sizeof(SelectState), 256) + 256; }

hipError_t launch_radix_quantile(long long n, const float* values, const float* q, float* out, void* workspace,
                                 hipStream_t stream) {
    SelectState* st = reinterpret_cast<SelectState*>(align_up(reinterpret_cast<uintptr_t>(workspace), 256));
    hipError_t e = hipMemsetAsync(st, 0, sizeof(SelectState), stream);
    if (e != hipSuccess) return e;
    return run_select(st, n, values, q, 0, out, stream);
}

// ------------------------------------------------------------------- plan
enum : uint32_t {  // densify_grads_kernel's tests
    kPreHi = 1u, kPreBig = 2u, kPreLow = 4u
};
enum : uint32_t {  // per original point, the counters the scan sums (bits 0..5) and what apply needs
    kFClone = 1u,       // cloned (counts C; noise row = its rank)
    kFSplit = 2u,       // the original is selected by the split pass
    kFSurvO = 4u,       // the original stays: not split, not pruned
    kFSurvC = 8u,       // its clone stays: not split again, not pruned
    kFChildO = 16u,     // its two children stay
    kFChildC = 32u,     // its clone's two children stay
};

struct Cnt6 {
    uint32_t v[6];
};
struct Cnt6Plus {
    __host__ __device__ Cnt6 operator()(const Cnt6& a, const Cnt6& b) const {
        Cnt6 r;
#pragma unroll
        for (int k = 0; k < 6; k++) r.v[k] = a.v[k] + b.v[k];
        return r;
    }
};
struct FlagToCnt6 {
    __host__ __device__ Cnt6 operator()(uint8_t f) const {
        Cnt6 r;
#pragma unroll
        for (int k = 0; k < 6; k++) r.v[k] = (f >> k) & 1u;
        return r;
    }
};
using FlagIter = rocprim::transform_iterator<const uint8_t*, FlagToCnt6, Cnt6>;

struct DensifyWorkspace {
    SelectState* st;
    float* gabs;      // [P]
    uint8_t* pre;     // [P]
    uint8_t* flags;   // [P + 1], the last 0: its scan entry holds the totals
    Cnt6* ranks;      // [P + 1] exclusive scan of the flags' counters
    long long* counts;  // [4] C, S, pruned, N
    void* scan_tmp;
    size_t scan_tmp_bytes;
};

static size_t carve_densify(void* base, long long P, DensifyWorkspace& w) {
    Carver c(base);
    w.st = c.take<SelectState>(1);
    w.counts = c.take<long long>(4);
    w.gabs = c.take<float>((size_t)P);
    w.pre = c.take<uint8_t>((size_t)P);
    w.flags = c.take<uint8_t>((size_t)P + 1);
    w.ranks = c.take<Cnt6>((size_t)P + 1);
    w.scan_tmp_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, w.scan_tmp_bytes, FlagIter(nullptr, FlagToCnt6()), (Cnt6*)nullptr, Cnt6{},
                                  (size_t)P + 1, Cnt6Plus());
    w.scan_tmp = c.take<char>(w.scan_tmp_bytes);
    return c.off + 256;
}

size_t densify_workspace_bytes(long long P) {
    DensifyWorkspace w;
    return carve_densify(nullptr, P, w);
}

static void* ws_base(void* p) { return reinterpret_cast<void*>(align_up(reinterpret_cast<uintptr_t>(p), 256)); }

__global__ void __launch_bounds__(256)
    densify_grads_kernel(long long P, const float* __restrict__ accum, const float* __restrict__ accum_abs,
                         const float* __restrict__ denom, const float* __restrict__ scaling,
                         const float* __restrict__ opacity, float max_grad, float min_opacity, float pd_extent,
                         float* __restrict__ gabs, uint8_t* __restrict__ pre, SelectState* st) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool hi = false;
    if (i < P) {
        const float d = denom[i];
        float g = accum[i] / d, ga = accum_abs[i] / d;  // IEEE division
        g = g != g ? 0.f : g;
        ga = ga != ga ? 0.f : ga + 0.f;  // (-0 -> +0: the select orders bit patterns)
        const float ms = fmaxf(fmaxf(expf(scaling[3 * i]), expf(scaling[3 * i + 1])), expf(scaling[3 * i + 2]));
        const float sig = 1.f / (1.f + expf(-opacity[i]));
        hi = g >= max_grad;
        gabs[i] = ga;
        pre[i] = (uint8_t)((hi ? kPreHi : 0u) | (ms > pd_extent ? kPreBig : 0u) | (sig < min_opacity ? kPreLow : 0u));
    }
    const unsigned long long b = __ballot(hi);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&st->n_hi, (unsigned long long)__builtin_popcountll(b));
}

__global__ void __launch_bounds__(256)
    densify_flags_kernel(long long P, const float* __restrict__ gabs, const uint8_t* __restrict__ pre,
                         const SelectState* __restrict__ st, uint8_t* __restrict__ flags) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i > P) return;
    if (i == P) {
        flags[P] = 0;
        return;
    }
    const float Q = st->Q;
    const uint32_t p = pre[i];
    const bool hi = p & kPreHi, big = p & kPreBig, low = p & kPreLow;
    const bool clone = hi && !big;
    const bool split = (hi && big) || gabs[i] >= Q;
    // The split pass sees a clone with gradients 0: selected when 0 >= Q (its other branch,
    // 0 >= max_grad and max exp(s) > pd * extent, cannot hold for a clone, which is not `big`).
    const bool csplit = 0.f >= Q;
    uint32_t f = 0u;
    if (clone) f |= kFClone;
    if (split) f |= kFSplit;
    if (!split && !low) f |= kFSurvO;
    if (clone && !csplit && !low) f |= kFSurvC;
    if (split && !low) f |= kFChildO;
    if (clone && csplit && !low) f |= kFChildC;
    flags[i] = (uint8_t)f;
}

__global__ void densify_counts_kernel(long long P, const Cnt6* __restrict__ ranks, const SelectState* st,
                                      long long* counts) {
    const Cnt6 t = ranks[P];
    const long long C = t.v[0];
    const long long S = (long long)t.v[1] + (0.f >= st->Q ? C : 0);
    const long long N = (long long)t.v[2] + t.v[3] + 2ll * ((long long)t.v[4] + t.v[5]);
    counts[0] = C;
    counts[1] = S;
    counts[2] = P + C + S - N;  // the opacity prune, over survivors and new points alike
    counts[3] = N;
}

hipError_t launch_densify_plan(long long P, const float* accum, const float* accum_abs, const float* denom,
                               const float* scaling, const float* opacity, float max_grad, float min_opacity,
                               float pd_extent, void* workspace, long long* counts_host, float* q_host,
                               hipStream_t stream) {
    DensifyWorkspace w;
    carve_densify(ws_base(workspace), P, w);
    hipError_t e = hipMemsetAsync(w.st, 0, sizeof(SelectState), stream);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)((P + 256) / 256);  // covers P + 1
    hipLaunchKernelGGL(densify_grads_kernel, dim3(grid), dim3(256), 0, stream, P, accum, accum_abs, denom, scaling,
                       opacity, max_grad, min_opacity, pd_extent, w.gabs, w.pre, w.st);
    if ((e = run_select(w.st, P, w.gabs, nullptr, P, nullptr, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(densify_flags_kernel, dim3(grid), dim3(256), 0, stream, P, w.gabs, w.pre, w.st, w.flags);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t bytes = w.scan_tmp_bytes;
    e = rocprim::exclusive_scan(w.scan_tmp, bytes, FlagIter(w.flags, FlagToCnt6()), w.ranks, Cnt6{}, (size_t)P + 1,
                                Cnt6Plus(), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(densify_counts_kernel, dim3(1), dim3(1), 0, stream, P, w.ranks, w.st, w.counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // the one readback
    if ((e = hipMemcpyAsync(counts_host, w.counts, 4 * sizeof(long long), hipMemcpyDeviceToHost, stream)) != hipSuccess)
        return e;
    if (q_host && (e = hipMemcpyAsync(q_host, &w.st->Q, sizeof(float), hipMemcpyDeviceToHost, stream)) != hipSuccess)
        return e;
    return hipStreamSynchronize(stream);
}

// ------------------------------------------------------------------ apply
// map[0][d] = source point, map[1][d] = the row of the noise a new point uses (-1: a surviving
// original; < C: a clone; else a split child), map[2][d] = for a clone's child the clone's own
// noise row (its position is the clone's new position), else -1.
__global__ void __launch_bounds__(256)
    densify_map_kernel(long long P, long long N, long long C, long long S, const uint8_t* __restrict__ flags,
                       const Cnt6* __restrict__ ranks, const long long* __restrict__ counts,
                       int32_t* __restrict__ map) {
    // a plan that is not the one these counts were read from writes nothing
    if (counts[0] != C || counts[1] != S || counts[3] != N) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const uint32_t f = flags[i];
    const Cnt6 r = ranks[i], t = ranks[P];
    int32_t* const src = map;
    int32_t* const nown = map + N;
    int32_t* const npar = map + 2 * N;
    const long long so = t.v[1];  // selected originals: the clones' selection ranks follow them
    if (f & kFSurvO) {
        const long long d = r.v[2];
        src[d] = (int32_t)i, nown[d] = -1, npar[d] = -1;
    }
    if (f & kFSurvC) {
        const long long d = (long long)t.v[2] + r.v[3];
        src[d] = (int32_t)i, nown[d] = (int32_t)r.v[0], npar[d] = -1;
    }
    const long long child0 = (long long)t.v[2] + t.v[3], nchild = (long long)t.v[4] + t.v[5];
    if (f & kFChildO) {
        for (int j = 0; j < 2; j++) {
            const long long d = child0 + j * nchild + r.v[4];
            src[d] = (int32_t)i, nown[d] = (int32_t)(C + j * S + r.v[1]), npar[d] = -1;
        }
    }
    if (f & kFChildC) {
        for (int j = 0; j < 2; j++) {
            const long long d = child0 + j * nchild + t.v[4] + r.v[5];
            src[d] = (int32_t)i, nown[d] = (int32_t)(C + j * S + so + r.v[0]), npar[d] = (int32_t)r.v[0];
        }
    }
}

struct DensifyApplyArgs {
    int n;
    long long N, C;
    const int32_t* map;
    const long long* counts;
    long long S;
    const float* noise;     // [C + 2S, 3]
    const float* rotation;  // source _rotation [P, 4]
    const float* scaling;   // source _scaling [P, 3]
    DensifyParam d[kMaxDensifyParams];
    uint32_t rows_per_block[kMaxDensifyParams];
    uint32_t block_begin[kMaxDensifyParams + 1];
};

// row `row` of R(q / |q|) times (exp(s) * eps): build_rotation (utils/general_utils.py:80-101)
__device__ __forceinline__ float rotated_sample(const float* __restrict__ q4, const float* __restrict__ s3,
                                                const float* __restrict__ eps3, int row) {
    const float q0 = q4[0], q1 = q4[1], q2 = q4[2], q3 = q4[3];
    const float norm = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    const float r = q0 / norm, x = q1 / norm, y = q2 / norm, z = q3 / norm;
    float R0, R1, R2;
    if (row == 0)
        R0 = 1.f - 2.f * (y * y + z * z), R1 = 2.f * (x * y - r * z), R2 = 2.f * (x * z + r * y);
    else if (row == 1)
        R0 = 2.f * (x * y + r * z), R1 = 1.f - 2.f * (x * x + z * z), R2 = 2.f * (y * z - r * x);
    else
        R0 = 2.f * (x * z - r * y), R1 = 2.f * (y * z + r * x), R2 = 1.f - 2.f * (x * x + y * y);
    const float v0 = expf(s3[0]) * eps3[0], v1 = expf(s3[1]) * eps3[1], v2 = expf(s3[2]) * eps3[2];
    return R0 * v0 + R1 * v1 + R2 * v2;
}

__global__ void __launch_bounds__(256) densify_apply_kernel(DensifyApplyArgs a) {
    if (a.counts[0] != a.C || a.counts[1] != a.S || a.counts[3] != a.N) return;  // (as densify_map_kernel)
    int gi = 0;
    while (gi + 1 < a.n && blockIdx.x >= a.block_begin[gi + 1]) gi++;
    const DensifyParam& D = a.d[gi];
    const uint32_t width = (uint32_t)D.width;
    const long long row0 = (long long)(blockIdx.x - a.block_begin[gi]) * a.rows_per_block[gi];
    const long long left = a.N - row0;
    const uint32_t nrows = left < (long long)a.rows_per_block[gi] ? (uint32_t)left : a.rows_per_block[gi];
    const uint32_t total = nrows * width;
    const int32_t* const src = a.map;
    const int32_t* const nown = a.map + a.N;
    const int32_t* const npar = a.map + 2 * a.N;
    for (uint32_t t = threadIdx.x; t < total; t += 256) {
        const uint32_t rl = t / width, col = t - rl * width;
        const long long d = row0 + rl;
        const long long s = src[d];
        const long long own = nown[d];
        const long long in = s * width + col, out = d * width + col;
        float p = D.param[in];
        if (own >= 0) {
            if (D.role == kDensifyXyz) {
                const long long par = npar[d];
                if (par >= 0) p = rotated_sample(a.rotation + 4 * s, a.scaling + 3 * s, a.noise + 3 * par, (int)col) + p;
                p = rotated_sample(a.rotation + 4 * s, a.scaling + 3 * s, a.noise + 3 * own, (int)col) + p;
            } else if (D.role == kDensifyScaling && own >= a.C) {
                p = logf(expf(p) / 1.6f);  // scaling_inverse_activation(get_scaling / (0.8 N)), N = 2
            }
        }
        D.param_out[out] = p;
        if (D.exp_avg) {  // survivors keep their moments, new points start from zero
            D.exp_avg_out[out] = own < 0 ? D.exp_avg[in] : 0.f;
            D.exp_avg_sq_out[out] = own < 0 ? D.exp_avg_sq[in] : 0.f;
        }
    }
}

hipError_t launch_densify_apply(long long P, long long N, long long C, long long S, void* workspace, int32_t* map,
                                bool build_map, const float* noise, const float* rotation, const float* scaling, int n,
                                const DensifyParam* params, hipStream_t stream) {
    DensifyWorkspace w;
    carve_densify(ws_base(workspace), P, w);
    if (N <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    if (build_map) {
        hipLaunchKernelGGL(densify_map_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, P, N, C, S,
                           w.flags, w.ranks, w.counts, map);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    for (int k0 = 0; k0 < n; k0 += kMaxDensifyParams) {
        DensifyApplyArgs a;
        a.n = n - k0 < kMaxDensifyParams ? n - k0 : kMaxDensifyParams;
        a.N = N, a.C = C, a.S = S;
        a.map = map;
        a.counts = w.counts;
        a.noise = noise, a.rotation = rotation, a.scaling = scaling;
        a.block_begin[0] = 0;
        unsigned long long blocks = 0;
        for (int k = 0; k < a.n; k++) {
            a.d[k] = params[k0 + k];
            const uint32_t width = (uint32_t)a.d[k].width;
            a.rows_per_block[k] = width >= 4096u ? 1u : 4096u / width;
            blocks += (unsigned long long)((N + a.rows_per_block[k] - 1) / a.rows_per_block[k]);
            if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
            a.block_begin[k + 1] = (uint32_t)blocks;
        }
        hipLaunchKernelGGL(densify_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

// -------------------------------------------------------------- 3D filter
// compute_3D_filter (gaussian_model.py:225-262): per point the smallest camera-space depth over
// the cameras that see it (z > 0.2, |x / z| and |y / z| within the bounds); points no camera
// sees take the largest such depth; times sqrt(0.2) / max Fx.  One lane per point, the camera
// records (R row-major as the reference stores it: p_cam = p R + T; T; the two bounds) staged
// through LDS 64 at a time.  The three dot products are taken in fp64 (one rounding into the
// fp32 the reference holds them in); the maximum is an integer max over the bit patterns.
constexpr int kCamFloats = 14, kCamChunk = 64;

__global__ void __launch_bounds__(256) filter3d_min_kernel(long long P, const float* __restrict__ xyz, int n_cam,
                                                           const float* __restrict__ cams, float* __restrict__ dist,
                                                           uint32_t* __restrict__ max_bits) {
    __shared__ float s_cam[kCamChunk * kCamFloats];
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) s_max = 0u;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < P;
    const double x = in ? xyz[3 * i] : 0.f, y = in ? xyz[3 * i + 1] : 0.f, z = in ? xyz[3 * i + 2] : 0.f;
    float dmin = INFINITY;
    for (int c0 = 0; c0 < n_cam; c0 += kCamChunk) {
        const int nc = n_cam - c0 < kCamChunk ? n_cam - c0 : kCamChunk;
        __syncthreads();
        for (int t = threadIdx.x; t < nc * kCamFloats; t += 256) s_cam[t] = cams[(long long)c0 * kCamFloats + t];
        __syncthreads();
        for (int c = 0; c < nc; c++) {
            const float* m = s_cam + c * kCamFloats;
            const double zc = x * m[2] + y * m[5] + z * m[8] + m[11];
            const float zf = (float)zc;
            if (!(zf > 0.2f)) continue;
            const double xc = x * m[0] + y * m[3] + z * m[6] + m[9];
            const double yc = x * m[1] + y * m[4] + z * m[7] + m[10];
            const float u = fabsf((float)xc / zf), v = fabsf((float)yc / zf);
            if (u <= m[12] && v <= m[13]) dmin = fminf(dmin, zf);
        }
    }
    const bool seen = in && dmin < INFINITY;
    if (in) dist[i] = dmin;
    if (seen) atomicMax(&s_max, __float_as_uint(dmin));  // positive floats: bit order = value order
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(max_bits, s_max);
}

__global__ void __launch_bounds__(256) filter3d_finish_kernel(long long P, float* __restrict__ dist,
                                                              const uint32_t* __restrict__ max_bits, float focal,
                                                              float factor) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    float d = dist[i];
    if (!(d < INFINITY)) d = __uint_as_float(*max_bits);
    dist[i] = d / focal * factor;
}

hipError_t launch_filter3d(long long P, const float* xyz, int n_cam, const float* cams, float focal, float* out,
                           uint32_t* max_bits, bool* any_seen, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(max_bits, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)((P + 255) / 256);
    hipLaunchKernelGGL(filter3d_min_kernel, dim3(grid), dim3(256), 0, stream, P, xyz, n_cam, cams, out, max_bits);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint32_t bits = 0;
    if ((e = hipMemcpyAsync(&bits, max_bits, sizeof(uint32_t), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    *any_seen = bits != 0u;
    if (!*any_seen) return hipSuccess;
    hipLaunchKernelGGL(filter3d_finish_kernel, dim3(grid), dim3(256), 0, stream, P, out, max_bits, focal,
                       (float)sqrt(0.2));
    return hipGetLastError();
}

// ---------------------------------------------------------- reset_opacity
// reset_opacity (gaussian_model.py:521-539): the filtered opacity capped at 0.01, divided by the
// filter's coefficient again and taken through the inverse sigmoid; both moments start over.
__global__ void __launch_bounds__(256)
    reset_opacity_kernel(long long P, const float* __restrict__ scaling, const float* __restrict__ opacity,
                         const float* __restrict__ filter3d, float* __restrict__ out, float* __restrict__ m,
                         float* __restrict__ v) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const float f2 = filter3d[i] * filter3d[i];
    float det1 = 1.f, det2 = 1.f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float e = expf(scaling[3 * i + k]);
        const float q = e * e;
        det1 = k ? det1 * q : q;
        det2 = k ? det2 * (q + f2) : q + f2;
    }
    const float coef = sqrtf(det1 / det2);
    const float sig = 1.f / (1.f + expf(-opacity[i]));
    const float x = fminf(sig * coef, 0.01f) / coef;
    out[i] = logf(x / (1.f - x));
    if (m) m[i] = 0.f, v[i] = 0.f;
}

hipError_t launch_reset_opacity(long long P, const float* scaling, const float* opacity, const float* filter3d,
                                float* out, float* m, float* v, hipStream_t stream) {
    if (P <= 0) return hipSuccess;
    hipLaunchKernelGGL(reset_opacity_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, P, scaling,
                       opacity, filter3d, out, m, v);
    return hipGetLastError();
}

}  // namespace gsr
