// meshclean.hip — mesh clean-up on gfx950: the clusters of triangles connected
// through shared edges and the removal of the small ones (the reference's
// post_process_mesh, mesh_extract_tetrahedra.py:18-40, which calls open3d's
// cluster_connected_triangles, remove_triangles_by_mask,
// remove_unreferenced_vertices and remove_degenerate_triangles on the CPU).
//
// Two triangles are adjacent when they share an undirected edge (min, max) of
// vertex ids; a vertex alone does not connect them, an edge of three or more
// triangles connects them all, and all three edges of every triangle count,
// those of index-degenerate triangles included.  Clusters are numbered in
// ascending order of their lowest triangle index (the order open3d's BFS
// seeds them).
//
// gsr_mesh_clusters:
//   1. clean_keys_kernel    3 keys per triangle, a << bits | b with a <= b and
//                           bits = ceil(log2 V), in slot 3 t + edge; parent[t] = t;
//   2. rocPRIM radix sort of (key, slot) over the 2 * bits live key bits;
//   3. clean_union_kernel   every sorted slot whose key equals its predecessor's
//                           unites the two triangles: chaining inside a run gives
//                           the connectivity of all pairs;
//   4. clean_jump_kernel    ceil(log2 F) rounds of parent[x] = parent[parent[x]],
//                           a round returning at once when the one before it
//                           changed nothing;
//   5. roots flagged, rocPRIM scan -> cluster ids, triangle_clusters;
//   6. counts: integer atomics per root, one per distinct root of a wave, then
//      written in cluster order;
//   7. areas (only with vertices): 0.5 |cross| per triangle in float64, a stable
//      radix sort by cluster id, one rocPRIM segmented reduction per cluster.
//
// The union-find.  parent[] is a forest over the triangles and
//     parent[x] <= x   holds at all times
// because a hook only ever stores the smaller of two roots into the larger
// (one atomicCAS on the larger root, expected value: itself) and the walks only
// replace a parent by one of its ancestors.  Every find therefore walks strictly
// downward and ends after at most x steps; a failed CAS means another thread
// hooked that root under a smaller one, and the retry starts from that strictly
// smaller value, so the larger of the two candidates decreases with every retry
// and the loop ends.  A stale read is an earlier value of parent[x], still a
// member of x's component and still <= x, so it costs steps and never
// correctness.  The pointer jumping halves the depth of every tree per round
// (depth < F), so after ceil(log2 F) rounds every triangle points at its root.
// The root of a component is its smallest triangle index whatever the
// schedule: labels, counts and areas (fixed summation order: ascending
// triangle index into a fixed reduction tree) are the same bits on every run.
//
// gsr_mesh_filter: keep the triangles of clusters with n_min or more
// triangles; mark the vertices they use; drop the kept triangles with two
// equal ids (after the marking: a vertex orphaned only by this step stays, as
// in open3d's call order); two rocPRIM scans give the new vertex and triangle
// indices, one gather writes each output.  Order and winding are kept.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_reduce.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "gsr_kernels.h"

namespace gsr {

using CleanSortConfig = rocprim::default_config;

static int clean_rounds(long long F) {
    int r = 1;
    while (r < 32 && (1ll << r) < F) r++;
    return r;
}

size_t carve_mesh_clusters(void* base, long long F, long long V, bool area, MeshClusterState& s) {
    Carver c(base);
    const size_t S = 3 * (size_t)F, n = (size_t)F;
    s.F = F;
    s.bits = tet_key_bits(V);
    s.rounds = clean_rounds(F);
    s.keys = c.take<uint64_t>(S);
    s.keys_sorted = c.take<uint64_t>(S);
    s.slots_sorted = c.take<uint32_t>(S);
    s.parent = c.take<uint32_t>(n);
    s.flags = c.take<uint32_t>((size_t)s.rounds + 2);
    // the unsorted keys are dead after the sort, the sorted ones after the union: 24 bytes per
    // triangle each for the cluster ids and counts per root and the area stage's arrays
    s.cid = reinterpret_cast<uint32_t*>(s.keys);
    s.root_count = s.cid + n + 1;
    s.label32 = reinterpret_cast<uint32_t*>(s.keys_sorted);
    s.label_sorted = s.label32 + n;
    s.seg = s.label_sorted + n;
    s.tri_area = reinterpret_cast<double*>(s.slots_sorted);  // 12 bytes per triangle: 8 needed
    s.area_sorted = c.take<double>(area ? n : 0);
    size_t sort_bytes = 0, scan_bytes = 0, asort_bytes = 0, seg_bytes = 0;
    (void)rocprim::radix_sort_pairs<CleanSortConfig>(nullptr, sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                     rocprim::counting_iterator<uint32_t>(0), (uint32_t*)nullptr, S,
                                                     0u, (unsigned)(2 * s.bits));
    (void)rocprim::exclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n + 1,
                                  rocprim::plus<uint32_t>());
    if (area) {
        (void)rocprim::radix_sort_pairs<CleanSortConfig>(nullptr, asort_bytes, (const uint32_t*)nullptr,
                                                         (uint32_t*)nullptr, (const double*)nullptr, (double*)nullptr,
                                                         n, 0u, 32u);
        (void)rocprim::segmented_reduce(nullptr, seg_bytes, (const double*)nullptr, (double*)nullptr, (unsigned)n,
                                        (const uint32_t*)nullptr, (const uint32_t*)nullptr, rocprim::plus<double>(),
                                        0.0);
    }
    s.tmp_bytes = sort_bytes;
    if (scan_bytes > s.tmp_bytes) s.tmp_bytes = scan_bytes;
    if (asort_bytes > s.tmp_bytes) s.tmp_bytes = asort_bytes;
    if (seg_bytes > s.tmp_bytes) s.tmp_bytes = seg_bytes;
    s.tmp = c.take<char>(s.tmp_bytes);
    return c.off + 256;
}

size_t carve_mesh_filter(void* base, long long F, long long V, MeshFilterState& s) {
    Carver c(base);
    s.vmap = c.take<uint32_t>((size_t)V + 1);
    s.fmap = c.take<uint32_t>((size_t)F + 1);
    s.bad = c.take<uint32_t>(1);
    size_t a = 0, b = 0;
    (void)rocprim::exclusive_scan(nullptr, a, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)V + 1,
                                  rocprim::plus<uint32_t>());
    (void)rocprim::exclusive_scan(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)F + 1,
                                  rocprim::plus<uint32_t>());
    s.tmp_bytes = a > b ? a : b;
    s.tmp = c.take<char>(s.tmp_bytes);
    return c.off + 256;
}

template <class I>
__device__ __forceinline__ void load_face(const I* __restrict__ faces, long long t, long long (&v)[3]) {
    v[0] = (long long)faces[3 * t], v[1] = (long long)faces[3 * t + 1], v[2] = (long long)faces[3 * t + 2];
}

__device__ __forceinline__ uint32_t uf_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void uf_store(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above x, halving the path on the way: every node passed is re-pointed at its
// grandparent.  parent[y] <= y: each step goes strictly down, at most x of them.
__device__ __forceinline__ uint32_t uf_find(uint32_t* __restrict__ parent, uint32_t x) {
    uint32_t p = uf_load(parent + x);
    while (p != x) {
        const uint32_t g = uf_load(parent + p);
        if (g != p) uf_store(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

// hooks the larger of the two roots under the smaller; the larger candidate decreases with every
// retry (see the file header)
__device__ __forceinline__ void uf_unite(uint32_t* __restrict__ parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old;  // < hi: another thread hooked hi in the meantime
        b = lo;
    }
}

// slot 3 t + e holds the key of edge e = (v0 v1, v1 v2, v2 v0) of triangle t.  A vertex id outside
// [0, V) sets `bad`; its triangle's keys are 0 (the call fails before anything reads vertices).
template <class I>
__global__ void __launch_bounds__(256) clean_keys_kernel(long long F, long long V, const I* __restrict__ faces,
                                                         int bits, uint64_t* __restrict__ keys,
                                                         uint32_t* __restrict__ parent,
                                                         uint32_t* __restrict__ bad_flag) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (t < F) {
        long long v[3];
        load_face<I>(faces, t, v);
#pragma unroll
        for (int i = 0; i < 3; i++) bad |= (unsigned long long)v[i] >= (unsigned long long)V;
#pragma unroll
        for (int e = 0; e < 3; e++) {
            const uint64_t x = (uint64_t)v[e], y = (uint64_t)v[(e + 1) % 3];
            const uint64_t a = x < y ? x : y, b = x < y ? y : x;
            keys[3 * t + e] = bad ? 0ull : (a << bits | b);
        }
        parent[t] = (uint32_t)t;
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad_flag, 1u);
}

__global__ void __launch_bounds__(256) clean_union_kernel(size_t S, const uint64_t* __restrict__ ks,
                                                          const uint32_t* __restrict__ slots,
                                                          uint32_t* __restrict__ parent) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0 || i >= S || ks[i] != ks[i - 1]) return;
    uf_unite(parent, slots[i] / 3u, slots[i - 1] / 3u);
}

// one round of pointer jumping; changed[round] is set when a parent moved, and a round whose
// predecessor moved nothing has nothing to do
__global__ void __launch_bounds__(256) clean_jump_kernel(long long F, uint32_t* __restrict__ parent,
                                                         uint32_t* __restrict__ changed, int round) {
    if (round > 0 && changed[round - 1] == 0u) return;
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    bool moved = false;
    if (x < F) {
        const uint32_t p = uf_load(parent + x);
        const uint32_t g = uf_load(parent + p);
        if (g != p) {
            uf_store(parent + x, g);
            moved = true;
        }
    }
    if (__ballot(moved) != 0ull && (threadIdx.x & 63) == 0) changed[round] = 1u;
}

// is_root[x] (F + 1 entries, the last one 0: the exclusive scan then ends with the number of roots)
__global__ void __launch_bounds__(256) clean_roots_kernel(long long F, const uint32_t* __restrict__ parent,
                                                          uint32_t* __restrict__ is_root,
                                                          uint32_t* __restrict__ root_count) {
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x > F) return;
    is_root[x] = (x < F && parent[x] == (uint32_t)x) ? 1u : 0u;
    if (x < F) root_count[x] = 0u;
}

// triangle_clusters[x] = cid[root]; the root's count by integer atomics, one per distinct root of a
// wave (one atomic per triangle on the root of a cluster of millions costs 9 ns each)
__global__ void __launch_bounds__(256) clean_labels_kernel(long long F, const uint32_t* __restrict__ parent,
                                                           const uint32_t* __restrict__ cid,
                                                           long long* __restrict__ triangle_clusters,
                                                           uint32_t* __restrict__ label32,
                                                           uint32_t* __restrict__ root_count) {
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool in = x < F;
    uint32_t r = 0u;
    if (in) {
        r = parent[x];
        const uint32_t c = cid[r];
        triangle_clusters[x] = (long long)c;
        label32[x] = c;
    }
    // at most 64 turns: every turn retires the lanes that share the first live lane's root
    unsigned long long live = __ballot(in);
    while (live != 0ull) {
        const int first = __builtin_ctzll(live);
        const uint32_t r0 = (uint32_t)__shfl((int)r, first, 64);
        const unsigned long long same = __ballot(in && r == r0) & live;
        if ((int)(threadIdx.x & 63) == first) atomicAdd(root_count + r0, (uint32_t)__builtin_popcountll(same));
        live &= ~same;
    }
}

__global__ void __launch_bounds__(256) clean_counts_kernel(long long F, const uint32_t* __restrict__ parent,
                                                           const uint32_t* __restrict__ cid,
                                                           const uint32_t* __restrict__ root_count,
                                                           long long* __restrict__ cluster_n) {
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x < F && parent[x] == (uint32_t)x) cluster_n[cid[x]] = (long long)root_count[x];
}

template <class I>
__global__ void __launch_bounds__(256) clean_area_kernel(long long F, const I* __restrict__ faces,
                                                         const float* __restrict__ vertices,
                                                         double* __restrict__ tri_area) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= F) return;
    long long v[3];
    load_face<I>(faces, t, v);
    double p[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) p[i][k] = (double)vertices[3 * v[i] + k];
    const double ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
    const double bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    tri_area[t] = 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
}

// seg[c] = the first sorted position of cluster c, seg[C] = F (every cluster has a triangle)
__global__ void __launch_bounds__(256) clean_segments_kernel(long long F, const uint32_t* __restrict__ ls,
                                                             uint32_t* __restrict__ seg) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= F) return;
    const uint32_t c = ls[i];
    if (i == 0 || c != ls[i - 1]) seg[c] = (uint32_t)i;
    if (i == F - 1) seg[c + 1] = (uint32_t)F;
}

hipError_t launch_clean_keys(long long V, const void* faces, bool is64, const MeshClusterState& s,
                             hipStream_t stream) {
    hipError_t e = hipMemsetAsync(s.flags, 0, ((size_t)s.rounds + 2) * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((s.F + 255) / 256));
    uint32_t* bad = s.flags + s.rounds + 1;
    if (is64)
        hipLaunchKernelGGL(clean_keys_kernel<int64_t>, grid, dim3(256), 0, stream, s.F, V, (const int64_t*)faces,
                           s.bits, s.keys, s.parent, bad);
    else
        hipLaunchKernelGGL(clean_keys_kernel<int32_t>, grid, dim3(256), 0, stream, s.F, V, (const int32_t*)faces,
                           s.bits, s.keys, s.parent, bad);
    return hipGetLastError();
}

hipError_t launch_clean_sort(const MeshClusterState& s, hipStream_t stream) {
    size_t bytes = s.tmp_bytes;
    return rocprim::radix_sort_pairs<CleanSortConfig>(s.tmp, bytes, s.keys, s.keys_sorted,
                                                      rocprim::counting_iterator<uint32_t>(0), s.slots_sorted,
                                                      3 * (size_t)s.F, 0u, (unsigned)(2 * s.bits), stream);
}

hipError_t launch_clean_union(const MeshClusterState& s, hipStream_t stream) {
    const size_t S = 3 * (size_t)s.F;
    hipLaunchKernelGGL(clean_union_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, stream, S, s.keys_sorted,
                       s.slots_sorted, s.parent);
    return hipGetLastError();
}

hipError_t launch_clean_flatten(const MeshClusterState& s, hipStream_t stream) {
    const dim3 grid((unsigned)((s.F + 255) / 256));
    for (int r = 0; r < s.rounds; r++) {
        hipLaunchKernelGGL(clean_jump_kernel, grid, dim3(256), 0, stream, s.F, s.parent, s.flags, r);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// after this cid[F] is the number of clusters
hipError_t launch_clean_ids(const MeshClusterState& s, hipStream_t stream) {
    hipLaunchKernelGGL(clean_roots_kernel, dim3((unsigned)((s.F + 256) / 256)), dim3(256), 0, stream, s.F, s.parent,
                       s.cid, s.root_count);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = s.tmp_bytes;
    return rocprim::exclusive_scan(s.tmp, bytes, s.cid, s.cid, 0u, (size_t)s.F + 1, rocprim::plus<uint32_t>(), stream);
}

hipError_t launch_clean_counts(const MeshClusterState& s, long long* triangle_clusters, long long* cluster_n,
                               hipStream_t stream) {
    const dim3 grid((unsigned)((s.F + 255) / 256));
    hipLaunchKernelGGL(clean_labels_kernel, grid, dim3(256), 0, stream, s.F, s.parent, s.cid, triangle_clusters,
                       s.label32, s.root_count);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(clean_counts_kernel, grid, dim3(256), 0, stream, s.F, s.parent, s.cid, s.root_count, cluster_n);
    return hipGetLastError();
}

hipError_t launch_clean_area(long long C, const void* faces, bool is64, const float* vertices,
                             const MeshClusterState& s, double* cluster_area, hipStream_t stream) {
    const dim3 grid((unsigned)((s.F + 255) / 256));
    if (is64)
        hipLaunchKernelGGL(clean_area_kernel<int64_t>, grid, dim3(256), 0, stream, s.F, (const int64_t*)faces,
                           vertices, s.tri_area);
    else
        hipLaunchKernelGGL(clean_area_kernel<int32_t>, grid, dim3(256), 0, stream, s.F, (const int32_t*)faces,
                           vertices, s.tri_area);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // the temporary was sized for 32 key bits and F segments before C was known
    size_t need = 0, bytes = s.tmp_bytes;
    (void)rocprim::radix_sort_pairs<CleanSortConfig>(nullptr, need, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                     (const double*)nullptr, (double*)nullptr, (size_t)s.F, 0u,
                                                     (unsigned)tet_key_bits(C));
    if (need > s.tmp_bytes) return hipErrorInvalidValue;
    (void)rocprim::segmented_reduce(nullptr, need, (const double*)nullptr, (double*)nullptr, (unsigned)C,
                                    (const uint32_t*)nullptr, (const uint32_t*)nullptr, rocprim::plus<double>(), 0.0);
    if (need > s.tmp_bytes) return hipErrorInvalidValue;
    // stable: a cluster's areas stay in ascending triangle order
    e = rocprim::radix_sort_pairs<CleanSortConfig>(s.tmp, bytes, s.label32, s.label_sorted, s.tri_area, s.area_sorted,
                                                   (size_t)s.F, 0u, (unsigned)tet_key_bits(C), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(clean_segments_kernel, grid, dim3(256), 0, stream, s.F, s.label_sorted, s.seg);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    bytes = s.tmp_bytes;
    return rocprim::segmented_reduce(s.tmp, bytes, s.area_sorted, cluster_area, (unsigned)C, s.seg, s.seg + 1,
                                     rocprim::plus<double>(), 0.0, stream);
}

// ---- gsr_mesh_filter -------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) filter_clear_kernel(long long n, uint32_t* __restrict__ flags) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i <= n) flags[i] = 0u;
}

// keep[t] = 1 for a triangle of a large enough cluster without two equal ids; used[v] = 1 for the vertices of
// the triangles of large enough clusters, degenerate ones included.  An id outside its range sets `bad`.
template <class I>
__global__ void __launch_bounds__(256) filter_mark_kernel(long long F, long long V, long long C,
                                                          const I* __restrict__ faces,
                                                          const long long* __restrict__ clusters,
                                                          const long long* __restrict__ cluster_n,
                                                          const long long* __restrict__ n_min,
                                                          uint32_t* __restrict__ used, uint32_t* __restrict__ keep,
                                                          uint32_t* __restrict__ bad_flag) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (t <= F) {
        uint32_t k = 0u;
        if (t < F) {
            long long v[3];
            load_face<I>(faces, t, v);
            const long long c = clusters[t];
#pragma unroll
            for (int i = 0; i < 3; i++) bad |= (unsigned long long)v[i] >= (unsigned long long)V;
            bad |= (unsigned long long)c >= (unsigned long long)C;
            if (!bad && cluster_n[c] >= *n_min) {
#pragma unroll
                for (int i = 0; i < 3; i++) used[v[i]] = 1u;
                k = (v[0] != v[1] && v[1] != v[2] && v[0] != v[2]) ? 1u : 0u;
            }
        }
        keep[t] = k;
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad_flag, 1u);
}

// flags before the scan cannot be told from offsets after it, so the gathers re-derive them:
// entry i was set iff map[i + 1] != map[i]
__global__ void __launch_bounds__(256) filter_vertices_kernel(long long V, const float* __restrict__ vertices,
                                                              const uint32_t* __restrict__ vmap,
                                                              float* __restrict__ out) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const uint32_t o = vmap[v];
    if (vmap[v + 1] == o) return;
#pragma unroll
    for (int k = 0; k < 3; k++) out[3 * (size_t)o + k] = vertices[3 * v + k];
}

template <class I>
__global__ void __launch_bounds__(256) filter_faces_kernel(long long F, const I* __restrict__ faces,
                                                           const uint32_t* __restrict__ vmap,
                                                           const uint32_t* __restrict__ fmap,
                                                           long long* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= F) return;
    const uint32_t o = fmap[t];
    if (fmap[t + 1] == o) return;
    long long v[3];
    load_face<I>(faces, t, v);
#pragma unroll
    for (int k = 0; k < 3; k++) out[3 * (size_t)o + k] = (long long)vmap[v[k]];
}

// after this vmap[V] and fmap[F] are the numbers of vertices and triangles that stay
hipError_t launch_filter_plan(long long F, long long V, long long C, const void* faces, bool is64,
                              const long long* clusters, const long long* cluster_n, const long long* n_min,
                              const MeshFilterState& s, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(s.bad, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(filter_clear_kernel, dim3((unsigned)((V + 256) / 256)), dim3(256), 0, stream, V, s.vmap);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const dim3 grid((unsigned)((F + 256) / 256));
    if (is64)
        hipLaunchKernelGGL(filter_mark_kernel<int64_t>, grid, dim3(256), 0, stream, F, V, C, (const int64_t*)faces,
                           clusters, cluster_n, n_min, s.vmap, s.fmap, s.bad);
    else
        hipLaunchKernelGGL(filter_mark_kernel<int32_t>, grid, dim3(256), 0, stream, F, V, C, (const int32_t*)faces,
                           clusters, cluster_n, n_min, s.vmap, s.fmap, s.bad);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t bytes = s.tmp_bytes;
    e = rocprim::exclusive_scan(s.tmp, bytes, s.vmap, s.vmap, 0u, (size_t)V + 1, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    bytes = s.tmp_bytes;
    return rocprim::exclusive_scan(s.tmp, bytes, s.fmap, s.fmap, 0u, (size_t)F + 1, rocprim::plus<uint32_t>(), stream);
}

hipError_t launch_filter_gather(long long F, long long V, const float* vertices, const void* faces, bool is64,
                                const MeshFilterState& s, float* vertices_out, long long* faces_out,
                                hipStream_t stream) {
    if (vertices_out) {
        hipLaunchKernelGGL(filter_vertices_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, stream, V, vertices,
                           s.vmap, vertices_out);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (!faces_out) return hipSuccess;
    const dim3 grid((unsigned)((F + 255) / 256));
    if (is64)
        hipLaunchKernelGGL(filter_faces_kernel<int64_t>, grid, dim3(256), 0, stream, F, (const int64_t*)faces, s.vmap,
                           s.fmap, faces_out);
    else
        hipLaunchKernelGGL(filter_faces_kernel<int32_t>, grid, dim3(256), 0, stream, F, (const int32_t*)faces, s.vmap,
                           s.fmap, faces_out);
    return hipGetLastError();
}

}  // namespace gsr
