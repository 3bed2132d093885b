// tnteval.hip — the device half of the Tanks and Temples F-score evaluation on gfx950 (the
// reference's eval_tnt/run.py, which is open3d on the CPU from end to end): polygon-volume crop,
// voxel-mean grid, a nearest-point index built once and queried many times, the correspondence
// sums of point-to-point ICP, and a 4x4 applied in place.  All geometry is float64 with contraction
// off; there is no float atomic anywhere, so every result is the same bits on every run.
//
// gsr_points_crop_polygon (open3d SelectionPolygonVolume::CropInPolygon):
//   1. crop_flag_kernel   the polygon's (u, v) pairs in LDS; per point the optional transform
//                         p' = ((r0 x + r1 y) + r2 z) + t, the axis range (both ends kept), and the
//                         parity of the edge nodes strictly below p'[u] — the reference sorts the
//                         nodes and takes lower_bound, which is that count;
//   2. rocPRIM exclusive scan of the flags, one readback (the number kept);
//   3. crop_write_kernel  the kept positions, ascending, and the kept transformed points (the
//                         transform is computed again: the same operations, the same bits).
//
// gsr_points_voxel_mean (open3d PointCloud::VoxelDownSample): bounds -> origin = min - voxel / 2 ->
// keys of floor((p - origin) / voxel) packed x | y | z -> the stable radix sort of (key, position)
// -> run heads -> scan -> voxel_emit_kernel: one lane per occupied cell walks its run, which the
// stable sort left in ascending input position, so the sum is the sequential loop's.  A cell of
// very many points costs its lane that many additions; there is no second path for long runs.
//
// gsr_points_index_build / _query: gsr_points_nearest (pointeval.hip) split at the ref sort.  The
// sorted keys, the positions and the gathered coordinates go into the caller's buffer; the query
// is nearest_search_block<true> of pointgrid.h, which also carries the original position of the
// best point (lowest position among equally near ones).
//
// gsr_icp_accumulate: icp_partial_kernel<pass> — a fixed grid (a function of N alone), every lane
// adds its strided pairs in ascending order, then a xor-shuffle tree over the wave, the four waves
// through LDS as (w0 + w1) + (w2 + w3); icp_final_kernel reduces the per-block rows with the same
// tree.  The shape of the sum depends on N only.
#pragma clang fp contract(off)

#include "pointgrid.h"

namespace gsr {

// ---- gsr_points_crop_polygon -------------------------------------------------------------------------------------

size_t carve_crop(void* base, long long N, int M, CropState& s) {
    Carver c(base);
    s.poly = c.take<double>((size_t)M * 3);
    s.flags = c.take<uint32_t>((size_t)N + 1);
    s.tmp_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, s.tmp_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)N + 1,
                                  rocprim::plus<uint32_t>());
    s.tmp = c.take<char>(s.tmp_bytes);
    return c.off + 256;
}

__device__ __forceinline__ double pick3(const double (&q)[3], int k) { return k == 0 ? q[0] : (k == 1 ? q[1] : q[2]); }

__device__ __forceinline__ void transform_point(const double* __restrict__ T, double x, double y, double z,
                                                double (&q)[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) q[r] = ((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3];
}

__device__ __forceinline__ void crop_point(const CropParams& p, const double* __restrict__ pts, long long i,
                                           double (&q)[3]) {
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (p.has_T) transform_point(p.T, x, y, z, q);
    else q[0] = x, q[1] = y, q[2] = z;
}

__global__ void __launch_bounds__(256) crop_flag_kernel(long long N, const double* __restrict__ pts, CropParams p,
                                                        const double* __restrict__ poly,
                                                        uint32_t* __restrict__ flags) {
    __shared__ double s_u[kCropMaxVertices], s_v[kCropMaxVertices];
    for (int k = threadIdx.x; k < p.M; k += 256) s_u[k] = poly[3 * k + p.u], s_v[k] = poly[3 * k + p.v];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i > N) return;
    if (i == N) {
        flags[N] = 0u;
        return;
    }
    double q[3];
    crop_point(p, pts, i, q);
    const double pu = pick3(q, p.u), pv = pick3(q, p.v), pw = pick3(q, p.w);
    uint32_t keep = 0u;
    if (!(pw < p.axis_min || pw > p.axis_max)) {
        uint32_t below = 0u;
        for (int a = 0; a < p.M; a++) {
            const int b = a + 1 == p.M ? 0 : a + 1;
            const double au = s_u[a], av = s_v[a], bu = s_u[b], bv = s_v[b];
            if ((av < pv && bv >= pv) || (bv < pv && av >= pv)) {
                const double node = au + (pv - av) / (bv - av) * (bu - au);
                below += node < pu ? 1u : 0u;
            }
        }
        keep = below & 1u;
    }
    flags[i] = keep;
}

__global__ void __launch_bounds__(256) crop_write_kernel(long long N, const double* __restrict__ pts, CropParams p,
                                                         const uint32_t* __restrict__ flags,
                                                         long long* __restrict__ kept, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint32_t o = flags[i];
    if (flags[i + 1] == o) return;
    double q[3];
    crop_point(p, pts, i, q);
    kept[o] = i;
    out[3 * (size_t)o] = q[0], out[3 * (size_t)o + 1] = q[1], out[3 * (size_t)o + 2] = q[2];
}

// after this flags[N] is the number of kept points
hipError_t launch_crop_plan(long long N, const double* points, const CropParams& p, const CropState& s,
                            hipStream_t stream) {
    hipLaunchKernelGGL(crop_flag_kernel, dim3((unsigned)((N + 256) / 256)), dim3(256), 0, stream, N, points, p,
                       s.poly, s.flags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = s.tmp_bytes;
    return rocprim::exclusive_scan(s.tmp, bytes, s.flags, s.flags, 0u, (size_t)N + 1, rocprim::plus<uint32_t>(),
                                   stream);
}

hipError_t launch_crop_write(long long N, const double* points, const CropParams& p, const CropState& s,
                             long long* kept, double* out, hipStream_t stream) {
    hipLaunchKernelGGL(crop_write_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, N, points, p,
                       s.flags, kept, out);
    return hipGetLastError();
}

// ---- gsr_points_voxel_mean ---------------------------------------------------------------------------------------

size_t carve_voxel(void* base, long long N, VoxelState& s) {
    Carver c(base);
    const size_t n = (size_t)N;
    s.partials = c.take<double>((size_t)kPeReduceBlocks * 6);
    s.bounds = c.take<double>(8);
    s.keys = c.take<uint64_t>(n);
    s.keys_sorted = c.take<uint64_t>(n);
    s.order = c.take<uint32_t>(n);
    s.bad = c.take<uint32_t>(1);
    s.flags = reinterpret_cast<uint32_t*>(s.keys);  // [N + 1] the unsorted keys are dead after the sort
    size_t scan = 0;
    (void)rocprim::exclusive_scan(nullptr, scan, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n + 1,
                                  rocprim::plus<uint32_t>());
    s.tmp_bytes = pe_sort_bytes(n);
    if (scan > s.tmp_bytes) s.tmp_bytes = scan;
    s.tmp = c.take<char>(s.tmp_bytes);
    return c.off + 256;
}

__global__ void __launch_bounds__(256) voxel_keys_kernel(long long N, const double* __restrict__ pts, VoxelGrid g,
                                                         uint64_t* __restrict__ keys, uint32_t* __restrict__ bad_flag) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < N) {
        uint64_t c[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double x = pts[3 * i + k];
            const double u = floor((x - g.origin[k]) / g.voxel);
            const bool ok = x > -DBL_MAX && x < DBL_MAX && u >= 0.0;  // (u >= 0 for every finite x >= min)
            bad |= !ok;
            c[k] = ok ? (uint64_t)u : 0ull;
        }
        const int sh = g.by + g.bz;
        keys[i] = (sh < 64 ? c[0] << sh : 0ull) | c[1] << g.bz | c[2];
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad_flag, 1u);
}

// flags[i] = sorted position i starts a run, flags[N] = 0: their exclusive scan ends with the number of cells
__global__ void __launch_bounds__(256) voxel_heads_kernel(long long N, const uint64_t* __restrict__ keys,
                                                          uint32_t* __restrict__ flags) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i > N) return;
    flags[i] = i < N && (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) voxel_emit_kernel(long long N, const double* __restrict__ pts, VoxelGrid g,
                                                         const uint64_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ order,
                                                         const uint32_t* __restrict__ flags, double* __restrict__ means,
                                                         long long* __restrict__ counts, long long* __restrict__ cells) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const size_t o = flags[i];
    if (flags[i + 1] == o) return;  // not the head of a run
    const uint64_t key = keys[i];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    long long j = i;
    for (; j < N && keys[j] == key; j++) {  // ascending input position: the sequential loop's sum
        const size_t r = order[j];
        sx += pts[3 * r], sy += pts[3 * r + 1], sz += pts[3 * r + 2];
    }
    const double n = (double)(j - i);
    means[3 * o] = sx / n, means[3 * o + 1] = sy / n, means[3 * o + 2] = sz / n;
    counts[o] = j - i;
    const int sh = g.by + g.bz;
    cells[3 * o] = sh < 64 ? (long long)(key >> sh) : 0ll;
    cells[3 * o + 1] = (long long)((key >> g.bz) & ((1ull << g.by) - 1ull));
    cells[3 * o + 2] = (long long)(key & ((1ull << g.bz) - 1ull));
}

hipError_t launch_voxel_keys(long long N, const double* points, const VoxelGrid& g, const VoxelState& s,
                             hipStream_t stream) {
    hipError_t e = hipMemsetAsync(s.bad, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(voxel_keys_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, N, points, g,
                       s.keys, s.bad);
    return hipGetLastError();
}

hipError_t launch_voxel_sort(long long N, unsigned bits, const VoxelState& s, hipStream_t stream) {
    size_t bytes = s.tmp_bytes;
    // stable: a cell's points stay in ascending input order
    return rocprim::radix_sort_pairs<PeSortConfig>(s.tmp, bytes, s.keys, s.keys_sorted,
                                                   rocprim::counting_iterator<uint32_t>(0), s.order, (size_t)N, 0u,
                                                   bits, stream);
}

// after this flags[N] is the number of occupied cells
hipError_t launch_voxel_plan(long long N, const VoxelState& s, hipStream_t stream) {
    hipLaunchKernelGGL(voxel_heads_kernel, dim3((unsigned)((N + 256) / 256)), dim3(256), 0, stream, N, s.keys_sorted,
                       s.flags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = s.tmp_bytes;
    return rocprim::exclusive_scan(s.tmp, bytes, s.flags, s.flags, 0u, (size_t)N + 1, rocprim::plus<uint32_t>(),
                                   stream);
}

hipError_t launch_voxel_emit(long long N, const double* points, const VoxelGrid& g, const VoxelState& s, double* means,
                             long long* counts, long long* cells, hipStream_t stream) {
    hipLaunchKernelGGL(voxel_emit_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, N, points, g,
                       s.keys_sorted, s.order, s.flags, means, counts, cells);
    return hipGetLastError();
}

// ---- gsr_points_index_build / gsr_points_index_query -------------------------------------------------------------

size_t carve_point_index(void* base, long long R, PointIndexView& v) {
    Carver c(base);
    const size_t r = (size_t)R;
    v.keys = c.take<uint64_t>(r);
    v.order = c.take<uint32_t>(r);
    v.x = c.take<double>(r);
    v.y = c.take<double>(r);
    v.z = c.take<double>(r);
    return c.off + 256;
}

size_t carve_point_index_build(void* base, long long R, PointIndexBuildState& s) {
    Carver c(base);
    s.partials = c.take<double>((size_t)kPeReduceBlocks * 6);
    s.bounds = c.take<double>(8);
    s.keys = c.take<uint64_t>((size_t)R);
    s.tmp_bytes = pe_sort_bytes((size_t)R);
    s.tmp = c.take<char>(s.tmp_bytes);
    return c.off + 256;
}

// the query half of carve_point_nearest (the ref half stays NULL: it lives in the index)
size_t carve_point_query(void* base, long long Q, PointNearestState& s) {
    Carver c(base);
    const size_t q = (size_t)Q;
    s = PointNearestState{};
    s.qkeys = c.take<uint64_t>(q);
    s.qkeys_sorted = c.take<uint64_t>(q);
    s.qorder = c.take<uint32_t>(q);
    s.tmp_bytes = pe_sort_bytes(q);
    s.tmp = c.take<char>(s.tmp_bytes);
    return c.off + 256;
}

__global__ void __launch_bounds__(256) nearest_index_kernel(long long Q, const double* __restrict__ query,
                                                            const uint32_t* __restrict__ qorder, long long R,
                                                            const uint64_t* __restrict__ rkeys,
                                                            const uint32_t* __restrict__ rorder,
                                                            const double* __restrict__ rx, const double* __restrict__ ry,
                                                            const double* __restrict__ rz, PointGrid g, double max_dist,
                                                            double* __restrict__ out, long long* __restrict__ out_idx) {
    nearest_search_block<true>(Q, query, qorder, R, rkeys, rorder, rx, ry, rz, g, max_dist, out, out_idx);
}

__global__ void __launch_bounds__(256) index_fill_kernel(long long Q, double* __restrict__ dist,
                                                         long long* __restrict__ index) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < Q) dist[i] = HUGE_VAL, index[i] = -1ll;
}

hipError_t launch_index_search(long long Q, const double* query, long long R, const PointGrid& g,
                               const PointIndexView& v, const PointNearestState& s, double max_dist, double* dist,
                               long long* index, hipStream_t stream) {
    hipLaunchKernelGGL(nearest_index_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, stream, Q, query,
                       s.qorder, R, v.keys, v.order, v.x, v.y, v.z, g, max_dist, dist, index);
    return hipGetLastError();
}

hipError_t launch_index_fill(long long Q, double* dist, long long* index, hipStream_t stream) {
    hipLaunchKernelGGL(index_fill_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, stream, Q, dist, index);
    return hipGetLastError();
}

// ---- gsr_icp_accumulate ------------------------------------------------------------------------------------------

size_t carve_icp(void* base, IcpState& s) {
    Carver c(base);
    s.partials = c.take<double>((size_t)kPeReduceBlocks * (kIcpMaxSums + 1));
    s.sums = c.take<double>(kIcpMaxSums + 1);
    return c.off + 256;
}

struct IcpMeans {
    double s[3], t[3];
};

// the block's sum of v[0 .. kN) in lane 0: a xor tree over each wave, then (w0 + w1) + (w2 + w3)
template <int kN>
__device__ __forceinline__ void icp_block_sum(double (&v)[kN], double (*s)[kIcpMaxSums + 1]) {
#pragma unroll
    for (int k = 0; k < kN; k++) v[k] = wave_sum(v[k]);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kN; k++) s[wave][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kN; k++) v[k] = (s[0][k] + s[1][k]) + (s[2][k] + s[3][k]);
}

// pass 1: n, sum d^2, sum s, sum t (8); pass 2: sum (s - ms)(t - mt)^T row-major, sum |s - ms|^2 (10); then
// the number of indices outside [-1, R), whose pairs are left out
template <int kPass>
__global__ void __launch_bounds__(256) icp_partial_kernel(long long N, const double* __restrict__ src, long long R,
                                                          const double* __restrict__ ref,
                                                          const long long* __restrict__ index, IcpMeans m,
                                                          double* __restrict__ partials) {
    constexpr int K = kPass == 1 ? 8 : 10;
    __shared__ double s_w[4][kIcpMaxSums + 1];
    double acc[K + 1];
#pragma unroll
    for (int k = 0; k <= K; k++) acc[k] = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
        const long long j = index[i];
        if (j < 0) {
            if (j != -1) acc[K] += 1.0;
            continue;
        }
        if (j >= R) {
            acc[K] += 1.0;
            continue;
        }
        const double s[3] = {src[3 * i], src[3 * i + 1], src[3 * i + 2]};
        const double t[3] = {ref[3 * j], ref[3 * j + 1], ref[3 * j + 2]};
        if (kPass == 1) {
            const double dx = s[0] - t[0], dy = s[1] - t[1], dz = s[2] - t[2];
            acc[0] += 1.0;
            acc[1] += (dx * dx + dy * dy) + dz * dz;
#pragma unroll
            for (int k = 0; k < 3; k++) acc[2 + k] += s[k], acc[5 + k] += t[k];
        } else {
            const double a[3] = {s[0] - m.s[0], s[1] - m.s[1], s[2] - m.s[2]};
            const double b[3] = {t[0] - m.t[0], t[1] - m.t[1], t[2] - m.t[2]};
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = 0; c < 3; c++) acc[3 * r + c] += a[r] * b[c];
            }
            acc[9] += (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
        }
    }
    icp_block_sum<K + 1>(acc, s_w);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k <= K; k++) partials[(size_t)blockIdx.x * (kIcpMaxSums + 1) + k] = acc[k];
    }
}

__global__ void __launch_bounds__(256) icp_final_kernel(int rows, const double* __restrict__ partials,
                                                        double* __restrict__ sums) {
    __shared__ double s_w[4][kIcpMaxSums + 1];
    double acc[kIcpMaxSums + 1];
#pragma unroll
    for (int k = 0; k <= kIcpMaxSums; k++) acc[k] = 0.0;
    for (int r = threadIdx.x; r < rows; r += 256) {
#pragma unroll
        for (int k = 0; k <= kIcpMaxSums; k++) acc[k] += partials[(size_t)r * (kIcpMaxSums + 1) + k];
    }
    icp_block_sum<kIcpMaxSums + 1>(acc, s_w);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k <= kIcpMaxSums; k++) sums[k] = acc[k];
    }
}

// after this sums[0 .. K) are the pass's sums and sums[K] the bad-index count (K = 8 or 10)
hipError_t launch_icp_accumulate(int pass, long long N, const double* src, long long R, const double* ref,
                                 const long long* index, const double* means6, const IcpState& s, hipStream_t stream) {
    const int nb = (int)((N + 255) / 256 < kPeReduceBlocks ? (N + 255) / 256 : kPeReduceBlocks);
    // a pass-1 row leaves its last two slots unwritten: clear them for the final sum
    hipError_t e = hipMemsetAsync(s.partials, 0, (size_t)nb * (kIcpMaxSums + 1) * sizeof(double), stream);
    if (e != hipSuccess) return e;
    IcpMeans m{};
    if (pass == 2)
        for (int k = 0; k < 3; k++) m.s[k] = means6[k], m.t[k] = means6[3 + k];
    if (pass == 1)
        hipLaunchKernelGGL(icp_partial_kernel<1>, dim3(nb), dim3(256), 0, stream, N, src, R, ref, index, m,
                           s.partials);
    else
        hipLaunchKernelGGL(icp_partial_kernel<2>, dim3(nb), dim3(256), 0, stream, N, src, R, ref, index, m,
                           s.partials);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(icp_final_kernel, dim3(1), dim3(256), 0, stream, nb, s.partials, s.sums);
    return hipGetLastError();
}

// ---- gsr_points_transform ----------------------------------------------------------------------------------------

struct Rows3x4 {
    double T[12];
};

__global__ void __launch_bounds__(256) transform_kernel(long long N, double* __restrict__ pts, Rows3x4 t) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    double q[3];
    transform_point(t.T, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], q);
    pts[3 * i] = q[0], pts[3 * i + 1] = q[1], pts[3 * i + 2] = q[2];
}

hipError_t launch_points_transform(long long N, double* points, const double* T12, hipStream_t stream) {
    Rows3x4 t;
    for (int k = 0; k < 12; k++) t.T[k] = T12[k];
    hipLaunchKernelGGL(transform_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, N, points, t);
    return hipGetLastError();
}

}  // namespace gsr
