// meshraster.hip — the device half of the Tanks and Temples mesh culling on gfx950 (the reference's
// eval_tnt/cull_mesh.py, which renders with pyrender / OpenGL and votes with torch): a z-buffer
// rasteriser for a triangle mesh seen from one pinhole camera, and the per-vertex view vote that
// reads its depth map.  The contract and its operation order are DESIGN §6j; tests/tntcull_ref.py
// restates them in numpy float32 and the two agree bit for bit, so every expression below keeps
// its parentheses and the file is built with floating-point contraction off.
//
// One view:
//   1. hipMemsetAsync      the depth words to kRasterEmpty (all ones: above every float's pattern);
//   2. raster_setup_kernel one lane per triangle: the three corners sorted by vertex id (both
//                          facings count, so the order is free, and a sorted order makes the result
//                          independent of winding and rotation), camera-space corners, the screen
//                          bound of the part in front of znear.  A bound of at most kRasterLanePixels
//                          pixel centres is rasterised by the lane at once; a larger one leaves its
//                          number of kRasterTile x kRasterTile tiles in units[t];
//   3. rocPRIM exclusive scan of units (64-bit sums): offsets[t], offsets[F] = the number of units;
//   4. raster_unit_kernel  a fixed grid of waves; wave w takes units w, w + waves, ...: a binary
//                          search of offsets names the triangle and the tile, the wave computes the
//                          same set-up again and its lanes take the tile's columns, row by row.  A
//                          bound inside one tile is one wave per triangle, a larger one is split;
//   5. the winner per pixel is atomicMin on the depth's bit pattern (positive floats order as
//      unsigned integers), behind a relaxed atomic read that skips the atomic when the stored depth
//      is already nearer (depths only fall, so a stale read errs to the safe side).
// raster_finish_kernel turns kRasterEmpty into 0 for gsr_mesh_depth; the vote reads the raw words.
#pragma clang fp contract(off)

#include <math.h>

#include <rocprim/device/device_scan.hpp>

#include "gsr_kernels.h"

namespace gsr {

namespace {

struct TriSetup {
    float A[3], B[3], C[3];  // edge k at (u, v): (A u + B v) + C
    float Aw, Bw, Cw, D;     // z = D / ((Aw u + Bw v) + Cw)
    int j0, j1, i0, i1;      // the pixel bound, inclusive
};

__device__ __forceinline__ void cam_point(const RasterCamera& c, const float* __restrict__ v, long long id,
                                          float (&p)[3]) {
    const float x = v[3 * id], y = v[3 * id + 1], z = v[3 * id + 2];
#pragma unroll
    for (int r = 0; r < 3; r++) p[r] = ((c.m[4 * r] * x + c.m[4 * r + 1] * y) + c.m[4 * r + 2] * z) + c.m[4 * r + 3];
}

__device__ __forceinline__ void cross3(const float (&a)[3], const float (&b)[3], float (&n)[3]) {
    n[0] = a[1] * b[2] - a[2] * b[1];
    n[1] = a[2] * b[0] - a[0] * b[2];
    n[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void affine(const RasterCamera& c, const float (&n)[3], float& A, float& B, float& C) {
    A = n[0] / c.fx;
    B = n[1] / c.fy;
    C = n[2] - (A * c.cx + B * c.cy);
}

__device__ __forceinline__ void grow(float u, float v, float (&lo)[2], float (&hi)[2]) {
    lo[0] = fminf(lo[0], u), hi[0] = fmaxf(hi[0], u);
    lo[1] = fminf(lo[1], v), hi[1] = fmaxf(hi[1], v);
}

template <bool is64>
__device__ __forceinline__ long long face_id(const void* __restrict__ faces, long long k) {
    return is64 ? ((const long long*)faces)[k] : (long long)((const int*)faces)[k];
}

// false: the triangle covers nothing (degenerate, not finite, outside the slab or the image); *bad_id
// is set when a corner lies outside [0, V)
template <bool is64>
__device__ __forceinline__ bool tri_setup(const RasterCamera& c, const float* __restrict__ verts, long long V,
                                          const void* __restrict__ faces, long long t, TriSetup& s, bool& bad_id) {
    long long a = face_id<is64>(faces, 3 * t), b = face_id<is64>(faces, 3 * t + 1), d = face_id<is64>(faces, 3 * t + 2);
    bad_id = a < 0 || a >= V || b < 0 || b >= V || d < 0 || d >= V;
    if (bad_id) return false;
    long long x;
    if (a > b) x = a, a = b, b = x;
    if (b > d) x = b, b = d, d = x;
    if (a > b) x = a, a = b, b = x;
    float p[3][3];
    cam_point(c, verts, a, p[0]);
    cam_point(c, verts, b, p[1]);
    cam_point(c, verts, d, p[2]);
    float e1[3], e2[3], N[3];
#pragma unroll
    for (int k = 0; k < 3; k++) e1[k] = p[1][k] - p[0][k], e2[k] = p[2][k] - p[0][k];
    cross3(e1, e2, N);
    s.D = (p[0][0] * N[0] + p[0][1] * N[1]) + p[0][2] * N[2];
    if (!(fabsf(s.D) > 0.f && fabsf(s.D) < INFINITY)) return false;
    const float zmin = fminf(fminf(p[0][2], p[1][2]), p[2][2]), zmax = fmaxf(fmaxf(p[0][2], p[1][2]), p[2][2]);
    if (!(zmax >= c.znear && zmin <= c.zfar)) return false;
    // the bound of the part at z >= znear: its corners and where its edges cross z = znear
    float lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (p[k][2] >= c.znear) grow(c.fx * (p[k][0] / p[k][2]) + c.cx, c.fy * (p[k][1] / p[k][2]) + c.cy, lo, hi);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int k2 = k == 2 ? 0 : k + 1;
        const bool in1 = p[k][2] >= c.znear, in2 = p[k2][2] >= c.znear;
        if (in1 != in2) {
            const float* q0 = in1 ? p[k2] : p[k];  // the corner behind znear
            const float* q1 = in1 ? p[k] : p[k2];
            const float w = (c.znear - q0[2]) / (q1[2] - q0[2]);
            const float xx = q0[0] + w * (q1[0] - q0[0]), yy = q0[1] + w * (q1[1] - q0[1]);
            grow(c.fx * (xx / c.znear) + c.cx, c.fy * (yy / c.znear) + c.cy, lo, hi);
        }
    }
    // centres j + 0.5 within half a pixel of [lo, hi]
    const float fj0 = fmaxf(ceilf(lo[0] - 1.f), 0.f), fj1 = fminf(floorf(hi[0]), (float)(c.W - 1));
    const float fi0 = fmaxf(ceilf(lo[1] - 1.f), 0.f), fi1 = fminf(floorf(hi[1]), (float)(c.H - 1));
    if (!(fj0 <= fj1 && fi0 <= fi1)) return false;
    s.j0 = (int)fj0, s.j1 = (int)fj1, s.i0 = (int)fi0, s.i1 = (int)fi1;
    float n[3];
    cross3(p[1], p[2], n);
    affine(c, n, s.A[0], s.B[0], s.C[0]);
    cross3(p[2], p[0], n);
    affine(c, n, s.A[1], s.B[1], s.C[1]);
    cross3(p[0], p[1], n);
    affine(c, n, s.A[2], s.B[2], s.C[2]);
    affine(c, N, s.Aw, s.Bw, s.Cw);
    return true;
}

// one pixel centre against one triangle; returns 1 when it issued an atomic
__device__ __forceinline__ uint32_t shade(const RasterCamera& c, const TriSetup& s, int i, int j, uint32_t* depth) {
    const float u = (float)j + 0.5f, v = (float)i + 0.5f;
    const float e0 = (s.A[0] * u + s.B[0] * v) + s.C[0];
    const float e1 = (s.A[1] * u + s.B[1] * v) + s.C[1];
    const float e2 = (s.A[2] * u + s.B[2] * v) + s.C[2];
    if (!((e0 >= 0.f && e1 >= 0.f && e2 >= 0.f) || (e0 <= 0.f && e1 <= 0.f && e2 <= 0.f))) return 0u;
    const float z = s.D / ((s.Aw * u + s.Bw * v) + s.Cw);
    if (!(z >= c.znear && z <= c.zfar)) return 0u;
    const uint32_t bits = __float_as_uint(z);
    uint32_t* word = depth + ((size_t)i * (size_t)c.W + (size_t)j);
    // other lanes lower this word during the launch: a relaxed atomic load, not a plain one
    if (bits >= __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return 0u;
    atomicMin(word, bits);
    return 1u;
}

__device__ __forceinline__ void count_add(unsigned long long* counters, int k, unsigned long long n) {
    if (n) atomicAdd(counters + k, n);
}

template <bool is64, bool kCount>
__global__ void __launch_bounds__(256) raster_setup_kernel(RasterCamera c, long long V, long long F,
                                                           const float* __restrict__ verts,
                                                           const void* __restrict__ faces,
                                                           uint32_t* __restrict__ depth, uint32_t* __restrict__ units,
                                                           uint32_t* __restrict__ bad,
                                                           unsigned long long* __restrict__ counters) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t > F) return;
    if (t == F) {
        units[F] = 0u;
        return;
    }
    TriSetup s;
    bool bad_id;
    uint32_t n_units = 0u;
    if (tri_setup<is64>(c, verts, V, faces, t, s, bad_id)) {
        const int w = s.j1 - s.j0 + 1, h = s.i1 - s.i0 + 1;
        if ((long long)w * h <= kRasterLanePixels) {
            uint32_t atomics = 0u;
            for (int i = s.i0; i <= s.i1; i++)
                for (int j = s.j0; j <= s.j1; j++) atomics += shade(c, s, i, j, depth);
            if (kCount) {
                count_add(counters, 0, atomics);
                count_add(counters, 1, (unsigned long long)w * h);
                count_add(counters, 2, 1);
            }
        } else {
            n_units = (uint32_t)((w + kRasterTile - 1) / kRasterTile) * (uint32_t)((h + kRasterTile - 1) / kRasterTile);
        }
    } else if (bad_id) {
        *bad = 1u;
    }
    units[t] = n_units;
}

template <bool is64, bool kCount>
__global__ void __launch_bounds__(256) raster_unit_kernel(RasterCamera c, long long V, long long F,
                                                          const float* __restrict__ verts,
                                                          const void* __restrict__ faces,
                                                          const unsigned long long* __restrict__ offsets,
                                                          uint32_t* __restrict__ depth,
                                                          unsigned long long* __restrict__ counters) {
    const unsigned long long U = offsets[F];
    const unsigned long long waves = (unsigned long long)gridDim.x * 4;
    const unsigned long long first =
        (unsigned long long)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + threadIdx.x / 64));
    const int lane = threadIdx.x & 63;
    for (unsigned long long item = first; item < U; item += waves) {
        // the last t with offsets[t] <= item: the triangle whose units hold `item`
        long long lo = 0, hi = F;  // offsets[lo] <= item < offsets[hi]
        while (hi - lo > 1) {
            const long long mid = lo + (hi - lo) / 2;
            if (offsets[mid] <= item) lo = mid;
            else hi = mid;
        }
        const long long t = lo;
        TriSetup s;
        bool bad_id;
        if (!tri_setup<is64>(c, verts, V, faces, t, s, bad_id)) continue;  // (never: the set-up is the same)
        const int w = s.j1 - s.j0 + 1;
        const uint32_t k = (uint32_t)(item - offsets[t]), tiles_x = (uint32_t)((w + kRasterTile - 1) / kRasterTile);
        const int jb = s.j0 + (int)(k % tiles_x) * kRasterTile, ib = s.i0 + (int)(k / tiles_x) * kRasterTile;
        const int je = min(jb + kRasterTile - 1, s.j1), ie = min(ib + kRasterTile - 1, s.i1);
        const int j = jb + lane;
        uint32_t atomics = 0u;
        if (j <= je)
            for (int i = ib; i <= ie; i++) atomics += shade(c, s, i, j, depth);
        if (kCount) {
            count_add(counters, 0, atomics);
            if (lane == 0) {
                count_add(counters, 1, (unsigned long long)(je - jb + 1) * (ie - ib + 1));
                count_add(counters, 3, 1);
            }
        }
    }
}

__global__ void __launch_bounds__(256) raster_finish_kernel(long long n, const uint32_t* __restrict__ raw,
                                                            float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t b = raw[i];
    out[i] = b == kRasterEmpty ? 0.f : __uint_as_float(b);
}

__device__ __forceinline__ float depth_at(const uint32_t* __restrict__ raw, int W, int i, int j) {
    const uint32_t b = raw[(size_t)i * (size_t)W + (size_t)j];
    return b == kRasterEmpty ? 0.f : __uint_as_float(b);
}

// cull_mesh.py:96-183 per vertex, one view: counts[v] += in_frustum and front
__global__ void __launch_bounds__(256) view_vote_kernel(RasterCamera c, float eps, long long V,
                                                        const float* __restrict__ verts,
                                                        const uint32_t* __restrict__ raw, int* __restrict__ counts) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= V) return;
    float p[3];
    cam_point(c, verts, id, p);
    const float z = p[2] + 1e-8f;
    const float u = (c.fx * p[0] + c.cx * p[2]) / z, v = (c.fy * p[1] + c.cy * p[2]) / z;
    const float wm = (float)(c.W - 1), hm = (float)(c.H - 1);
    if (!(u >= 0.f && u <= wm && v >= 0.f && v <= hm && z > 0.f)) return;
    // bilinear, integer coordinates are pixel indices, the border repeated (grid_sample, align_corners)
    const float fx0 = floorf(u), fy0 = floorf(v);
    const int x0 = (int)fx0, y0 = (int)fy0, x1 = min(x0 + 1, c.W - 1), y1 = min(y0 + 1, c.H - 1);
    const float tx = u - fx0, ty = v - fy0, sx = (fx0 + 1.f) - u, sy = (fy0 + 1.f) - v;
    const float d = ((depth_at(raw, c.W, y0, x0) * (sx * sy) + depth_at(raw, c.W, y0, x1) * (tx * sy)) +
                     depth_at(raw, c.W, y1, x0) * (sx * ty)) +
                    depth_at(raw, c.W, y1, x1) * (tx * ty);
    const bool front = d > 0.f ? z < d + eps : true;
    if (front) counts[id] += 1;
}

}  // namespace

size_t carve_mesh_raster(void* base, long long F, int H, int W, MeshRasterState& s) {
    Carver c(base);
    s.depth = c.take<uint32_t>((size_t)H * (size_t)W);
    s.units = c.take<uint32_t>((size_t)F + 1);
    s.offsets = c.take<unsigned long long>((size_t)F + 1);
    s.bad = c.take<uint32_t>(1);
    s.counters = c.take<unsigned long long>(kRasterCounters);
    s.tmp_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, s.tmp_bytes, (uint32_t*)nullptr, (unsigned long long*)nullptr, 0ull,
                                  (size_t)F + 1, rocprim::plus<unsigned long long>());
    s.tmp = c.take<char>(s.tmp_bytes);
    return c.off + 256;
}

hipError_t launch_raster_reset(const MeshRasterState& s, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(s.bad, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    return hipMemsetAsync(s.counters, 0, kRasterCounters * sizeof(unsigned long long), stream);
}

hipError_t launch_raster_clear(const RasterCamera& c, const MeshRasterState& s, hipStream_t stream) {
    return hipMemsetAsync(s.depth, 0xFF, (size_t)c.H * (size_t)c.W * sizeof(uint32_t), stream);
}

hipError_t launch_raster_setup(const RasterCamera& c, long long V, long long F, const float* vertices,
                               const void* faces, bool is64, bool count, const MeshRasterState& s,
                               hipStream_t stream) {
    const dim3 grid((unsigned)((F + 256) / 256)), block(256);
#define GSR_RASTER_SETUP(A, B)                                                                                  \
    hipLaunchKernelGGL((raster_setup_kernel<A, B>), grid, block, 0, stream, c, V, F, vertices, faces, s.depth, \
                       s.units, s.bad, s.counters)
    if (is64) {
        if (count) GSR_RASTER_SETUP(true, true);
        else GSR_RASTER_SETUP(true, false);
    } else {
        if (count) GSR_RASTER_SETUP(false, true);
        else GSR_RASTER_SETUP(false, false);
    }
#undef GSR_RASTER_SETUP
    return hipGetLastError();
}

hipError_t launch_raster_scan(long long F, const MeshRasterState& s, hipStream_t stream) {
    size_t bytes = s.tmp_bytes;
    return rocprim::exclusive_scan(s.tmp, bytes, s.units, s.offsets, 0ull, (size_t)F + 1,
                                   rocprim::plus<unsigned long long>(), stream);
}

hipError_t launch_raster_units(const RasterCamera& c, long long V, long long F, const float* vertices,
                               const void* faces, bool is64, bool count, const MeshRasterState& s,
                               hipStream_t stream) {
    const dim3 grid(kRasterUnitBlocks), block(256);
#define GSR_RASTER_UNITS(A, B)                                                                                   \
    hipLaunchKernelGGL((raster_unit_kernel<A, B>), grid, block, 0, stream, c, V, F, vertices, faces, s.offsets, \
                       s.depth, s.counters)
    if (is64) {
        if (count) GSR_RASTER_UNITS(true, true);
        else GSR_RASTER_UNITS(true, false);
    } else {
        if (count) GSR_RASTER_UNITS(false, true);
        else GSR_RASTER_UNITS(false, false);
    }
#undef GSR_RASTER_UNITS
    return hipGetLastError();
}

hipError_t launch_raster_finish(const RasterCamera& c, const MeshRasterState& s, float* depth, hipStream_t stream) {
    const long long n = (long long)c.H * c.W;
    hipLaunchKernelGGL(raster_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, s.depth,
                       depth);
    return hipGetLastError();
}

hipError_t launch_view_vote(const RasterCamera& c, float eps, long long V, const float* vertices,
                            const MeshRasterState& s, int* counts, hipStream_t stream) {
    hipLaunchKernelGGL(view_vote_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, stream, c, eps, V, vertices,
                       s.depth, counts);
    return hipGetLastError();
}

}  // namespace gsr
