// tsdf.hip — TSDF fusion and marching cubes on gfx950 (the open3d VoxelBlockGrid of the
// reference's mesh_extract.py:63-85: compute_unique_block_coordinates, integrate,
// extract_triangle_mesh).  The contract is DESIGN §6h; open3d itself was not available to
// compare against, so nothing here claims bit-parity with it.
//
// Blocks are R^3 voxels (R = 8 or 16), a voxel is linear in (z R + y) R + x inside its block, and
// a block's packed key is (x + 2^20) << 42 | (y + 2^20) << 21 | (z + 2^20).  The grid itself
// (slots in insertion order, a sorted key -> slot index) lives with the caller.
//
// gsr_tsdf_touch:
//   1. tsdf_touch_keys_kernel   one thread per stride-4 pixel: four samples along its ray between
//                               d - trunc and d + trunc, one key each (all ones: no sample);
//   2. rocPRIM radix sort of the keys;
//   3. tsdf_touch_heads_kernel  head flags of the runs of equal keys, rocPRIM scan;
//   4. tsdf_touch_write_kernel  the unique block coordinates, ascending by key.
// gsr_tsdf_lookup: binary search of a coordinate's key in the sorted keys -> its rank, or -1.
// gsr_tsdf_integrate: one workgroup per listed block, one thread per voxel (x fastest): project,
//   round to the nearest pixel, running mean of the truncated signed distance and the colour.
// gsr_tsdf_extract, one workgroup per block, blocks in ascending key order:
//   1. mc_mark_kernel      the (R + 1)^3 samples of the block and of its up to 7 upper neighbours in
//                          LDS; a cube is emitted when its 8 corners are usable (block present,
//                          weight > threshold); its case goes to cases[], and every crossed edge
//                          sets its bit in the mask of the voxel that owns it (atomic OR, so the
//                          result does not depend on the order), which may lie in a neighbour;
//   2. mc_count_kernel     vertices (mask bits) and triangles per block; rocPRIM scans over the
//                          blocks give every block's first vertex and first triangle;
//   3. mc_vertices_kernel  a scan over the block's voxels numbers the vertices (block base +
//                          voxels before + lower axes) and keeps the per-voxel offset for step 4;
//                          position and colour by linear interpolation along the edge;
//   4. mc_faces_kernel     a scan over the block's triangle counts, then the table's triangles
//                          with the vertex ids of their edges' owners.
// Every vertex is shared by the cubes around its edge: the mesh is indexed and connected.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "gsr_kernels.h"
#define GSR_MC_TABLE_ATTR __constant__ const
#include "mc_table.h"

namespace gsr {

namespace {

constexpr uint64_t kNoKey = ~0ull;
constexpr int kKeyBias = 1 << 20;

__host__ __device__ __forceinline__ uint64_t tsdf_pack(int x, int y, int z) {
    return (uint64_t)(uint32_t)(x + kKeyBias) << 42 | (uint64_t)(uint32_t)(y + kKeyBias) << 21 |
           (uint64_t)(uint32_t)(z + kKeyBias);
}
__device__ __forceinline__ bool tsdf_in_range(int x, int y, int z) {
    return x >= -kKeyBias && x < kKeyBias && y >= -kKeyBias && y < kKeyBias && z >= -kKeyBias && z < kKeyBias;
}

// the rank of `key` in sorted[0, n), or -1
__device__ __forceinline__ int tsdf_find(const uint64_t* __restrict__ sorted, int n, uint64_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sorted[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && sorted[lo] == key) ? lo : -1;
}

// ---- touch -------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) tsdf_touch_keys_kernel(int H, int W, int gw, int gh,
                                                              const float* __restrict__ depth, TsdfCamera cam,
                                                              float depth_scale, float depth_max, float trunc,
                                                              float block_size, uint64_t* __restrict__ keys,
                                                              uint32_t* __restrict__ bad_flag) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < (long long)gw * gh) {
        const int x = (int)(i % gw) * 4, y = (int)(i / gw) * 4;
        const float d = depth[(size_t)y * W + x] / depth_scale;
        uint64_t k[4] = {kNoKey, kNoKey, kNoKey, kNoKey};
        if (d > 0.f && d < depth_max) {  // NaN fails
            const float px = ((float)x - cam.cx) / cam.fx, py = ((float)y - cam.cy) / cam.fy;
            // o = -R^T t, dir = R^T (px, py, 1)
            float o[3], dir[3];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                o[a] = -(cam.e[0][a] * cam.e[0][3] + cam.e[1][a] * cam.e[1][3] + cam.e[2][a] * cam.e[2][3]);
                dir[a] = cam.e[0][a] * px + cam.e[1][a] * py + cam.e[2][a];
            }
            const float t_min = fmaxf(d - trunc, 0.f), t_max = fminf(d + trunc, depth_max);
            const float step = (t_max - t_min) / 3.f;
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const float t = t_min + (float)s * step;
                float c[3];
                bool in = true;
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    c[a] = floorf((o[a] + t * dir[a]) / block_size);
                    in &= c[a] >= -(float)kKeyBias && c[a] < (float)kKeyBias;  // NaN fails
                }
                if (in) k[s] = tsdf_pack((int)c[0], (int)c[1], (int)c[2]);
                else bad = true;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; s++) keys[4 * i + s] = k[s];
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad_flag, 1u);
}

// heads[i] = 1 where sorted key i starts a run of a real key; heads[n] = 0 (the exclusive scan ends with the count)
__global__ void __launch_bounds__(256) tsdf_touch_heads_kernel(long long n, const uint64_t* __restrict__ ks,
                                                               uint32_t* __restrict__ heads) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    heads[i] = (i < n && ks[i] != kNoKey && (i == 0 || ks[i] != ks[i - 1])) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) tsdf_touch_write_kernel(long long n, const uint64_t* __restrict__ ks,
                                                               const uint32_t* __restrict__ rank,
                                                               int* __restrict__ coords) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = rank[i];
    if (rank[i + 1] == o) return;
    const uint64_t k = ks[i];
    coords[3 * (size_t)o + 0] = (int)(k >> 42 & 0x1fffffu) - kKeyBias;
    coords[3 * (size_t)o + 1] = (int)(k >> 21 & 0x1fffffu) - kKeyBias;
    coords[3 * (size_t)o + 2] = (int)(k & 0x1fffffu) - kKeyBias;
}

// ---- lookup ------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) tsdf_lookup_kernel(long long n, const int* __restrict__ coords, int nb,
                                                          const uint64_t* __restrict__ sorted,
                                                          int* __restrict__ rank) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = coords[3 * i], y = coords[3 * i + 1], z = coords[3 * i + 2];
    rank[i] = tsdf_in_range(x, y, z) ? tsdf_find(sorted, nb, tsdf_pack(x, y, z)) : -1;
}

// ---- integrate ---------------------------------------------------------------------------------

template <int R>
__global__ void __launch_bounds__(256) tsdf_integrate_kernel(const int* __restrict__ coords,
                                                             const int* __restrict__ slots, long long capacity,
                                                             float voxel_size, float* __restrict__ tsdf,
                                                             float* __restrict__ weight, float* __restrict__ color,
                                                             const float* __restrict__ depth,
                                                             const float* __restrict__ image, int H, int W,
                                                             TsdfCamera cam, float depth_scale, float depth_max,
                                                             float trunc) {
    constexpr int N = R * R * R;
    const int b = blockIdx.x;
    const int slot = slots[b];
    if (slot < 0 || slot >= capacity) return;  // not a block of the grid
    const int bx = coords[3 * b] * R, by = coords[3 * b + 1] * R, bz = coords[3 * b + 2] * R;
    const size_t base = (size_t)slot * N;
    for (int i = threadIdx.x; i < N; i += 256) {
        const int x = i % R, y = i / R % R, z = i / (R * R);
        const float wx = (float)(bx + x) * voxel_size, wy = (float)(by + y) * voxel_size,
                    wz = (float)(bz + z) * voxel_size;
        const float xc = cam.e[0][0] * wx + cam.e[0][1] * wy + cam.e[0][2] * wz + cam.e[0][3];
        const float yc = cam.e[1][0] * wx + cam.e[1][1] * wy + cam.e[1][2] * wz + cam.e[1][3];
        const float zc = cam.e[2][0] * wx + cam.e[2][1] * wy + cam.e[2][2] * wz + cam.e[2][3];
        if (!(zc > 0.f)) continue;
        const float uf = rintf(cam.fx * xc / zc + cam.cx), vf = rintf(cam.fy * yc / zc + cam.cy);
        if (!(uf >= 0.f && uf < (float)W && vf >= 0.f && vf < (float)H)) continue;
        const size_t pix = (size_t)(int)vf * W + (int)uf;
        const float d = depth[pix] / depth_scale;
        if (!(d > 0.f) || d > depth_max) continue;
        const float sdf = d - zc;
        if (sdf < -trunc) continue;
        const float s = fminf(sdf, trunc) / trunc;
        const float w = weight[base + i], w1 = w + 1.f;
        tsdf[base + i] = (w * tsdf[base + i] + s) / w1;
        if (color) {
            float* c = color + 3 * (base + i);
#pragma unroll
            for (int k = 0; k < 3; k++) c[k] = (w * c[k] + image[3 * pix + k]) / w1;
        }
        weight[base + i] = w1;
    }
}

// ---- extract -----------------------------------------------------------------------------------

// the ranks of the block's 8 neighbours (dx + 2 dy + 4 dz, itself at 0) into LDS, by 8 threads
__device__ __forceinline__ void mc_neighbours(const uint64_t* __restrict__ keys, int nb, int b, int* s_rank) {
    if (threadIdx.x < 8) {
        const uint64_t k = keys[b];
        const int x = (int)(k >> 42 & 0x1fffffu) + (threadIdx.x & 1), y = (int)(k >> 21 & 0x1fffffu) + (threadIdx.x >> 1 & 1),
                  z = (int)(k & 0x1fffffu) + (threadIdx.x >> 2 & 1);
        int r = -1;
        if (x < 2 * kKeyBias && y < 2 * kKeyBias && z < 2 * kKeyBias)
            r = tsdf_find(keys, nb, (uint64_t)x << 42 | (uint64_t)y << 21 | (uint64_t)z);
        s_rank[threadIdx.x] = r;
    }
}

// where voxel (x, y, z), each coordinate in [0, R], of block `b` lives: neighbour n = which
// coordinates reached R, the linear index there
template <int R>
__device__ __forceinline__ void mc_locate(int x, int y, int z, int* n, int* lin) {
    *n = (x == R) | (y == R) << 1 | (z == R) << 2;
    *lin = ((z % R) * R + (y % R)) * R + (x % R);
}

// edge e of the cube at p: its owner voxel is p + the edge's first corner, its bit the axis
__device__ __forceinline__ void mc_edge_owner(int e, int* dx, int* dy, int* dz, int* axis) {
    const int a = e >> 2, j = e & 3;
    const int lo = j & 1, hi = j >> 1;
    *axis = a;
    *dx = a == 0 ? 0 : lo;
    *dy = a == 0 ? lo : (a == 1 ? 0 : hi);
    *dz = a == 2 ? 0 : hi;
}

template <int R>
__global__ void __launch_bounds__(256) mc_mark_kernel(int nb, const uint64_t* __restrict__ keys,
                                                      const int* __restrict__ slots,
                                                      const float* __restrict__ tsdf,
                                                      const float* __restrict__ weight, float threshold,
                                                      uint8_t* __restrict__ cases, uint32_t* __restrict__ masks) {
    constexpr int N = R * R * R, S = R + 1, NS = S * S * S;
    __shared__ float s_tsdf[NS];
    __shared__ uint8_t s_ok[NS];
    __shared__ int s_rank[8];
    const int b = blockIdx.x;
    mc_neighbours(keys, nb, b, s_rank);
    __syncthreads();
    for (int i = threadIdx.x; i < NS; i += 256) {
        const int x = i % S, y = i / S % S, z = i / (S * S);
        int n, lin;
        mc_locate<R>(x, y, z, &n, &lin);
        const int r = s_rank[n];
        float v = 0.f;
        bool ok = false;
        if (r >= 0) {
            const size_t at = (size_t)slots[r] * N + lin;
            ok = weight[at] > threshold;
            v = tsdf[at];
        }
        s_tsdf[i] = v;
        s_ok[i] = ok;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < N; i += 256) {
        const int x = i % R, y = i / R % R, z = i / (R * R);
        int c = 0;
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int at = ((z + (k >> 2)) * S + y + (k >> 1 & 1)) * S + x + (k & 1);
            ok &= s_ok[at] != 0;
            c |= (s_tsdf[at] < 0.f ? 1 : 0) << k;
        }
        if (!ok) c = 0;
        cases[(size_t)b * N + i] = (uint8_t)c;
        uint32_t em = kMcEdgeMask[c];
        while (em) {
            const int e = __builtin_ctz(em);
            em &= em - 1;
            int dx, dy, dz, axis, n, lin;
            mc_edge_owner(e, &dx, &dy, &dz, &axis);
            mc_locate<R>(x + dx, y + dy, z + dz, &n, &lin);
            if (s_rank[n] < 0) continue;  // (an emitted cube's corners are usable, so the owner's block exists)
            const size_t at = (size_t)s_rank[n] * N + lin;
            atomicOr(masks + (at >> 3), 1u << ((at & 7) * 4 + axis));
        }
    }
}

// nvert[b], ntri[b]: the vertices and triangles of block b; 0 at b = nb
template <int R>
__global__ void __launch_bounds__(256) mc_count_kernel(int nb, const uint8_t* __restrict__ cases,
                                                       const uint32_t* __restrict__ masks,
                                                       uint32_t* __restrict__ nvert, uint32_t* __restrict__ ntri) {
    constexpr int N = R * R * R;
    __shared__ uint32_t s_v[256], s_t[256];
    const int b = blockIdx.x;
    uint32_t v = 0, t = 0;
    if (b < nb) {
        for (int i = threadIdx.x; i < N / 8; i += 256) v += __popc(masks[(size_t)b * (N / 8) + i] & 0x77777777u);
        for (int i = threadIdx.x; i < N; i += 256) t += kMcNumTris[cases[(size_t)b * N + i]];
    }
    s_v[threadIdx.x] = v;
    s_t[threadIdx.x] = t;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            s_v[threadIdx.x] += s_v[threadIdx.x + d];
            s_t[threadIdx.x] += s_t[threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        nvert[b] = s_v[0];
        ntri[b] = s_t[0];
    }
}

__device__ __forceinline__ uint32_t mc_mask_of(const uint32_t* __restrict__ masks, size_t at) {
    return masks[at >> 3] >> ((at & 7) * 4) & 7u;
}

template <int R>
__global__ void __launch_bounds__(256) mc_vertices_kernel(int nb, const uint64_t* __restrict__ keys,
                                                          const int* __restrict__ slots,
                                                          const float* __restrict__ tsdf,
                                                          const float* __restrict__ color, float voxel_size,
                                                          const uint32_t* __restrict__ masks,
                                                          const uint32_t* __restrict__ vbase,
                                                          uint16_t* __restrict__ voffset,
                                                          float* __restrict__ vertices,
                                                          float* __restrict__ colors) {
    constexpr int N = R * R * R, PER = N / 256;
    __shared__ uint32_t s_scan[4];
    __shared__ int s_rank[8];
    const int b = blockIdx.x;
    mc_neighbours(keys, nb, b, s_rank);
    // thread t owns the PER consecutive voxels from t * PER
    uint32_t m[PER], mine = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        m[k] = mc_mask_of(masks, (size_t)b * N + threadIdx.x * PER + k);
        mine += __popc(m[k]);
    }
    uint32_t total;
    uint32_t off = block_excl_scan<4>(mine, s_scan, &total);  // (its barrier covers s_rank)
    const uint64_t key = keys[b];
    const int bx = ((int)(key >> 42 & 0x1fffffu) - kKeyBias) * R, by = ((int)(key >> 21 & 0x1fffffu) - kKeyBias) * R,
              bz = ((int)(key & 0x1fffffu) - kKeyBias) * R;
    const size_t self = (size_t)slots[b] * N;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int i = threadIdx.x * PER + k;
        voffset[(size_t)b * N + i] = (uint16_t)off;
        if (m[k]) {
            const int x = i % R, y = i / R % R, z = i / (R * R);
            const float ta = tsdf[self + i];
            for (int axis = 0; axis < 3; axis++) {
                if (!(m[k] >> axis & 1)) continue;
                int n, lin;
                mc_locate<R>(x + (axis == 0), y + (axis == 1), z + (axis == 2), &n, &lin);
                if (s_rank[n] < 0) continue;  // (a marked edge belongs to an emitted cube: both ends exist)
                const size_t other = (size_t)slots[s_rank[n]] * N + lin;
                const float tb = tsdf[other];
                const float t = ta / (ta - tb);
                const size_t v = (size_t)vbase[b] + off;
                vertices[3 * v + 0] = ((float)(bx + x) + (axis == 0 ? t : 0.f)) * voxel_size;
                vertices[3 * v + 1] = ((float)(by + y) + (axis == 1 ? t : 0.f)) * voxel_size;
                vertices[3 * v + 2] = ((float)(bz + z) + (axis == 2 ? t : 0.f)) * voxel_size;
                if (colors) {
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) {
                        const float ca = color[3 * (self + i) + ch], cb = color[3 * other + ch];
                        colors[3 * v + ch] = ca + t * (cb - ca);
                    }
                }
                off++;
            }
        }
    }
}

template <int R>
__global__ void __launch_bounds__(256) mc_faces_kernel(int nb, const uint64_t* __restrict__ keys,
                                                       const uint8_t* __restrict__ cases,
                                                       const uint32_t* __restrict__ masks,
                                                       const uint32_t* __restrict__ vbase,
                                                       const uint16_t* __restrict__ voffset,
                                                       const uint32_t* __restrict__ fbase,
                                                       long long* __restrict__ faces) {
    constexpr int N = R * R * R, PER = N / 256;
    __shared__ uint32_t s_scan[4];
    __shared__ int s_rank[8];
    const int b = blockIdx.x;
    mc_neighbours(keys, nb, b, s_rank);
    uint32_t c[PER], mine = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        c[k] = cases[(size_t)b * N + threadIdx.x * PER + k];
        mine += kMcNumTris[c[k]];
    }
    uint32_t total;
    size_t f = (size_t)fbase[b] + block_excl_scan<4>(mine, s_scan, &total);
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int nt = kMcNumTris[c[k]];
        if (nt == 0) continue;
        const int i = threadIdx.x * PER + k;
        const int x = i % R, y = i / R % R, z = i / (R * R);
        for (int j = 0; j < 3 * nt; j++) {
            const int e = kMcTris[c[k]][j];
            int dx, dy, dz, axis, n, lin;
            mc_edge_owner(e, &dx, &dy, &dz, &axis);
            mc_locate<R>(x + dx, y + dy, z + dz, &n, &lin);
            const int r = s_rank[n] < 0 ? b : s_rank[n];  // (never negative for an emitted cube)
            const size_t at = (size_t)r * N + lin;
            const uint32_t m = mc_mask_of(masks, at);
            faces[3 * f + j] = (long long)vbase[r] + voffset[at] + __popc(m & ((1u << axis) - 1u));
        }
        f += nt;
    }
}

}  // namespace

size_t carve_tsdf_touch(void* base, int H, int W, TsdfTouchState& s) {
    Carver c(base);
    s.gw = (W + 3) / 4;
    s.gh = (H + 3) / 4;
    s.n = 4ll * s.gw * s.gh;
    s.keys = c.take<uint64_t>((size_t)s.n);
    s.keys_sorted = c.take<uint64_t>((size_t)s.n);
    s.heads = c.take<uint32_t>((size_t)s.n + 1);
    s.bad = c.take<uint32_t>(1);
    size_t a = 0, b = 0;
    (void)rocprim::radix_sort_keys(nullptr, a, (const uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)s.n, 0u, 64u);
    (void)rocprim::exclusive_scan(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)s.n + 1,
                                  rocprim::plus<uint32_t>());
    s.tmp_bytes = a > b ? a : b;
    s.tmp = c.take<char>(s.tmp_bytes);
    return c.off + 256;
}

// after this heads[n] is the number of distinct blocks
hipError_t launch_tsdf_touch(int H, int W, const float* depth, const TsdfCamera& cam, float depth_scale,
                             float depth_max, float trunc, float block_size, const TsdfTouchState& s,
                             hipStream_t stream) {
    hipError_t e = hipMemsetAsync(s.bad, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const long long px = (long long)s.gw * s.gh;
    hipLaunchKernelGGL(tsdf_touch_keys_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, stream, H, W, s.gw,
                       s.gh, depth, cam, depth_scale, depth_max, trunc, block_size, s.keys, s.bad);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t bytes = s.tmp_bytes;
    e = rocprim::radix_sort_keys(s.tmp, bytes, s.keys, s.keys_sorted, (size_t)s.n, 0u, 64u, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tsdf_touch_heads_kernel, dim3((unsigned)((s.n + 256) / 256)), dim3(256), 0, stream, s.n,
                       s.keys_sorted, s.heads);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    bytes = s.tmp_bytes;
    return rocprim::exclusive_scan(s.tmp, bytes, s.heads, s.heads, 0u, (size_t)s.n + 1, rocprim::plus<uint32_t>(),
                                   stream);
}

hipError_t launch_tsdf_touch_write(const TsdfTouchState& s, int* coords, hipStream_t stream) {
    hipLaunchKernelGGL(tsdf_touch_write_kernel, dim3((unsigned)((s.n + 255) / 256)), dim3(256), 0, stream, s.n,
                       s.keys_sorted, s.heads, coords);
    return hipGetLastError();
}

hipError_t launch_tsdf_lookup(long long n, const int* coords, int nb, const uint64_t* sorted_keys, int* rank,
                              hipStream_t stream) {
    hipLaunchKernelGGL(tsdf_lookup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, coords, nb,
                       sorted_keys, rank);
    return hipGetLastError();
}

hipError_t launch_tsdf_integrate(int n, int R, const int* coords, const int* slots, long long capacity,
                                 float voxel_size, float* tsdf, float* weight, float* color, const float* depth,
                                 const float* image, int H, int W, const TsdfCamera& cam, float depth_scale,
                                 float depth_max, float trunc, hipStream_t stream) {
    if (R == 16)
        hipLaunchKernelGGL(tsdf_integrate_kernel<16>, dim3((unsigned)n), dim3(256), 0, stream, coords, slots, capacity,
                           voxel_size, tsdf, weight, color, depth, image, H, W, cam, depth_scale, depth_max, trunc);
    else
        hipLaunchKernelGGL(tsdf_integrate_kernel<8>, dim3((unsigned)n), dim3(256), 0, stream, coords, slots, capacity,
                           voxel_size, tsdf, weight, color, depth, image, H, W, cam, depth_scale, depth_max, trunc);
    return hipGetLastError();
}

size_t carve_tsdf_extract(void* base, int nb, int R, TsdfExtractState& s) {
    Carver c(base);
    const size_t N = (size_t)R * R * R, n = (size_t)nb;
    s.nb = nb;
    s.R = R;
    s.cases = c.take<uint8_t>(n * N);
    s.masks = c.take<uint32_t>(n * N / 8);
    s.voffset = c.take<uint16_t>(n * N);
    s.vbase = c.take<uint32_t>(n + 1);
    s.fbase = c.take<uint32_t>(n + 1);
    s.tmp_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, s.tmp_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n + 1,
                                  rocprim::plus<uint32_t>());
    s.tmp = c.take<char>(s.tmp_bytes);
    return c.off + 256;
}

hipError_t launch_mc_mark(const uint64_t* keys, const int* slots, const float* tsdf, const float* weight,
                          float threshold, const TsdfExtractState& s, hipStream_t stream) {
    const size_t N = (size_t)s.R * s.R * s.R;
    hipError_t e;
    if ((e = hipMemsetAsync(s.masks, 0, (size_t)s.nb * N / 8 * sizeof(uint32_t), stream)) != hipSuccess) return e;
    if (s.R == 16)
        hipLaunchKernelGGL(mc_mark_kernel<16>, dim3((unsigned)s.nb), dim3(256), 0, stream, s.nb, keys, slots, tsdf,
                           weight, threshold, s.cases, s.masks);
    else
        hipLaunchKernelGGL(mc_mark_kernel<8>, dim3((unsigned)s.nb), dim3(256), 0, stream, s.nb, keys, slots, tsdf,
                           weight, threshold, s.cases, s.masks);
    return hipGetLastError();
}

// after this vbase[nb] and fbase[nb] are the numbers of vertices and triangles
hipError_t launch_mc_count(const TsdfExtractState& s, hipStream_t stream) {
    if (s.R == 16)
        hipLaunchKernelGGL(mc_count_kernel<16>, dim3((unsigned)s.nb + 1), dim3(256), 0, stream, s.nb, s.cases, s.masks,
                           s.vbase, s.fbase);
    else
        hipLaunchKernelGGL(mc_count_kernel<8>, dim3((unsigned)s.nb + 1), dim3(256), 0, stream, s.nb, s.cases, s.masks,
                           s.vbase, s.fbase);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = s.tmp_bytes;
    e = rocprim::exclusive_scan(s.tmp, bytes, s.vbase, s.vbase, 0u, (size_t)s.nb + 1, rocprim::plus<uint32_t>(),
                                stream);
    if (e != hipSuccess) return e;
    bytes = s.tmp_bytes;
    return rocprim::exclusive_scan(s.tmp, bytes, s.fbase, s.fbase, 0u, (size_t)s.nb + 1, rocprim::plus<uint32_t>(),
                                   stream);
}

hipError_t launch_mc_vertices(const uint64_t* keys, const int* slots, const float* tsdf, const float* color,
                              float voxel_size, const TsdfExtractState& s, float* vertices, float* colors,
                              hipStream_t stream) {
    if (s.R == 16)
        hipLaunchKernelGGL(mc_vertices_kernel<16>, dim3((unsigned)s.nb), dim3(256), 0, stream, s.nb, keys, slots, tsdf,
                           color, voxel_size, s.masks, s.vbase, s.voffset, vertices, colors);
    else
        hipLaunchKernelGGL(mc_vertices_kernel<8>, dim3((unsigned)s.nb), dim3(256), 0, stream, s.nb, keys, slots, tsdf,
                           color, voxel_size, s.masks, s.vbase, s.voffset, vertices, colors);
    return hipGetLastError();
}

hipError_t launch_mc_faces(const uint64_t* keys, const TsdfExtractState& s, long long* faces, hipStream_t stream) {
    if (s.R == 16)
        hipLaunchKernelGGL(mc_faces_kernel<16>, dim3((unsigned)s.nb), dim3(256), 0, stream, s.nb, keys, s.cases,
                           s.masks, s.vbase, s.voffset, s.fbase, faces);
    else
        hipLaunchKernelGGL(mc_faces_kernel<8>, dim3((unsigned)s.nb), dim3(256), 0, stream, s.nb, keys, s.cases,
                           s.masks, s.vbase, s.voffset, s.fbase, faces);
    return hipGetLastError();
}

}  // namespace gsr
