// tetmesh.hip — marching tetrahedra on gfx950: the triangle mesh of the zero
// level set of a per-vertex sdf over a tetrahedral grid (step 4 of the
// offline mesh extraction, mesh_extract_tetrahedra.py:128-132; semantics of
// utils/tetmesh.py:51-190).
//
// A vertex is positive when sdf > 0.  A tet takes part when 1-3 of its four
// vertices are positive and all four are valid; its case index is
// sum(positive[i] << i).  The mesh vertices are the undirected edges (a, b),
// a < b, with exactly one positive end that belong to a participating tet,
// each once, in ascending (a, b) order; a tet gives one triangle (one or
// three positive vertices) or two (two positive vertices).
//
// The reference materialises all six edges of every surviving tet as int64
// pairs and runs torch.unique over them in chunks.  Here only the crossing
// edges (3 or 4 per participating tet) ever exist, as packed 64-bit keys:
//   1. tet_flags_kernel    2 bits per vertex (positive, valid), V / 4 bytes:
//                          the four gathers of a tet hit a table that stays
//                          in L2 instead of sdf and valid separately;
//   2. tet_count_kernel    one tet per lane (16-B loads), wave ballots ->
//                          per 1024-tet block the number of one- and
//                          two-triangle tets; rocPRIM scan over the blocks;
//   3. tet_walk_kernel<0>  the same walk with the block prefix: every
//                          participating tet writes its crossing edges' keys
//                          (a << bits | b, bits = ceil(log2 V)) into its own
//                          consecutive slots;
//   4. rocPRIM radix sort of (key, slot) over the 2 * bits live key bits;
//   5. tet_heads_kernel + scan: the rank of each distinct key;
//   6. tet_edges_kernel    rank -> slot scatter and edge_ids;
//   7. tet_walk_kernel<1>  the walk again: triangles read their three ranks
//                          from the tet's slots, written in tet order.
// Every offset comes from a scan and the order of equal keys does not reach
// the outputs, so the result is the same bits on every run (the one atomic
// is the OR into the bad-vertex-id flag).
//
// Triangle table: edges are numbered 01, 02, 03, 12, 13, 23.  Cases 1..7 are
// listed below; case c >= 8 is case 15 - c (the complementary signs) with the
// winding reversed.  tests/golden/tetmesh.npz (all 16 cases x 24 vertex
// orders) pins winding and the two-triangle cases' diagonal.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "gsr_kernels.h"

namespace gsr {

constexpr int kTetIters = 4;                      // tets per lane of a walk
constexpr int kTetsPerBlock = 256 * kTetIters;    // one scan partial per 1024 tets

constexpr uint32_t tri_pack(int a, int b, int c, int d = 0, int e = 0, int f = 0) {
    return (uint32_t)(a | b << 3 | c << 6 | d << 9 | e << 12 | f << 15);
}
// cases 1..7 (index 0 unused): up to two triangles of edge numbers
__constant__ uint32_t kTetTriangles[8] = {
    0u,
    tri_pack(0, 2, 1),              // 1: vertex 0 positive
    tri_pack(0, 3, 4),              // 2: vertex 1
    tri_pack(1, 3, 4, 1, 4, 2),     // 3: vertices 0, 1 (diagonal 02-13)
    tri_pack(1, 5, 3),              // 4: vertex 2
    tri_pack(0, 2, 3, 2, 5, 3),     // 5: vertices 0, 2 (diagonal 03-12)
    tri_pack(0, 1, 4, 1, 5, 4),     // 6: vertices 1, 2 (diagonal 02-13)
    tri_pack(2, 5, 4),              // 7: vertices 0, 1, 2
};

using TetSortConfig = rocprim::default_config;

int tet_key_bits(long long V) {
    int bits = 1;
    while (bits < 32 && (1ll << bits) < V) bits++;
    return bits;
}

size_t carve_tet_count(void* base, long long V, long long T, TetCountState& s) {
    Carver c(base);
    s.nblocks = (T + kTetsPerBlock - 1) / kTetsPerBlock;
    s.flags = c.take<uint32_t>((size_t)((V + 15) / 16));
    s.partials = c.take<uint64_t>((size_t)s.nblocks + 1);
    s.bad = c.take<uint32_t>(1);
    s.scan_tmp_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, s.scan_tmp_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0,
                                  (size_t)s.nblocks + 1, rocprim::plus<uint64_t>());
    s.scan_tmp = c.take<char>(s.scan_tmp_bytes);
    return c.off + 256;
}

size_t carve_tet_edges(void* base, size_t S, int bits, TetEdgeState& s) {
    Carver c(base);
    s.S = S;
    s.bits = bits;
    s.keys = c.take<uint64_t>(S);
    // the unsorted keys are dead after the sort: their 8 bytes per slot then hold the head
    // flags / unique ranks in sorted order and the rank of every slot
    s.heads = reinterpret_cast<uint32_t*>(s.keys);
    s.rank = s.heads + S;
    s.keys_sorted = c.take<uint64_t>(S);
    s.slots_sorted = c.take<uint32_t>(S);
    size_t sort_bytes = 0, scan_bytes = 0;
    (void)rocprim::radix_sort_pairs<TetSortConfig>(nullptr, sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                   rocprim::counting_iterator<uint32_t>(0), (uint32_t*)nullptr, S,
                                                   0u, (unsigned)(2 * bits));
    (void)rocprim::inclusive_scan(nullptr, scan_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, S,
                                  rocprim::plus<uint32_t>());
    s.tmp_bytes = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
    s.tmp = c.take<char>(s.tmp_bytes);
    return c.off + 256;
}

// bits 0..15 of x to the even bit positions
__device__ inline uint32_t spread16(uint32_t x) {
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}

// flags[v >> 4] bits 2 (v & 15), 2 (v & 15) + 1 = (sdf[v] > 0, valid[v]); one wave writes four words
__global__ void __launch_bounds__(256) tet_flags_kernel(long long V, const float* __restrict__ sdf,
                                                        const uint8_t* __restrict__ valid,
                                                        uint32_t* __restrict__ flags) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool in = v < V;
    const bool pos = in && sdf[v] > 0.f;
    const bool ok = in && valid[v] != 0;
    const unsigned long long pb = __ballot(pos), vb = __ballot(ok);
    const int lane = threadIdx.x & 63;
    const long long first = v - lane + 16 * lane;  // first vertex of this lane's word
    if (lane < 4 && first < V)
        flags[first >> 4] = spread16((uint32_t)(pb >> (16 * lane)) & 0xFFFFu) |
                            spread16((uint32_t)(vb >> (16 * lane)) & 0xFFFFu) << 1;
}

template <class I>
__device__ __forceinline__ void load_tet(const I* __restrict__ tets, long long t, long long (&v)[4]);
template <>
__device__ __forceinline__ void load_tet<int32_t>(const int32_t* __restrict__ tets, long long t, long long (&v)[4]) {
    const int4 q = reinterpret_cast<const int4*>(tets)[t];
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
}
template <>
__device__ __forceinline__ void load_tet<int64_t>(const int64_t* __restrict__ tets, long long t, long long (&v)[4]) {
    const longlong2 a = reinterpret_cast<const longlong2*>(tets)[2 * t];
    const longlong2 b = reinterpret_cast<const longlong2*>(tets)[2 * t + 1];
    v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
}

// the case index of a participating tet (1..14), else 0; a vertex id outside [0, V) sets
// `bad` and reads nothing
__device__ __forceinline__ uint32_t tet_case(const long long (&v)[4], long long V, const uint32_t* __restrict__ flags,
                                             bool& bad) {
    bad = false;
#pragma unroll
    for (int i = 0; i < 4; i++) bad |= (unsigned long long)v[i] >= (unsigned long long)V;
    if (bad) return 0u;
    uint32_t pos = 0u, ok = 1u;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t f = (flags[v[i] >> 4] >> (2 * ((uint32_t)v[i] & 15u))) & 3u;
        pos |= (f & 1u) << i;
        ok &= f >> 1;
    }
    return (ok && pos != 15u) ? pos : 0u;
}

__device__ __forceinline__ bool two_triangles(uint32_t code) { return __builtin_popcount(code) == 2; }

// partials[b] = (one-triangle tets) | (two-triangle tets) << 32 of block b's 1024 tets
template <class I>
__global__ void __launch_bounds__(256) tet_count_kernel(long long T, long long V, const I* __restrict__ tets,
                                                        const uint32_t* __restrict__ flags,
                                                        uint64_t* __restrict__ partials,
                                                        uint32_t* __restrict__ bad_flag) {
    __shared__ uint32_t s_n[4][2];
    const long long base = (long long)blockIdx.x * kTetsPerBlock;
    uint32_t n1 = 0, n2 = 0;
    bool any_bad = false;
#pragma unroll
    for (int j = 0; j < kTetIters; j++) {
        const long long t = base + j * 256 + threadIdx.x;
        uint32_t code = 0u;
        if (t < T) {
            long long v[4];
            bool bad;
            load_tet<I>(tets, t, v);
            code = tet_case(v, V, flags, bad);
            any_bad |= bad;
        }
        const bool two = code != 0u && two_triangles(code);
        n1 += (uint32_t)__builtin_popcountll(__ballot(code != 0u && !two));
        n2 += (uint32_t)__builtin_popcountll(__ballot(two));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (__ballot(any_bad) != 0ull && lane == 0) atomicOr(bad_flag, 1u);
    if (lane == 0) s_n[wave][0] = n1, s_n[wave][1] = n2;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint64_t a = (uint64_t)s_n[0][0] + s_n[1][0] + s_n[2][0] + s_n[3][0];
        const uint64_t b = (uint64_t)s_n[0][1] + s_n[1][1] + s_n[2][1] + s_n[3][1];
        partials[blockIdx.x] = a | b << 32;
        if (blockIdx.x == 0) partials[gridDim.x] = 0ull;  // the scan's last element: the totals
    }
}

// The second and third walk over the tets.  A participating tet preceded by n1 one-triangle and
// n2 two-triangle tets owns the key slots [3 n1 + 4 n2, +3 or +4), its crossing edges in edge-number
// order, and the triangles [n1 + 2 n2, +1 or +2).  FACES = false writes the keys, true the triangles.
template <class I, bool FACES>
__global__ void __launch_bounds__(256) tet_walk_kernel(long long T, long long V, const I* __restrict__ tets,
                                                       const uint32_t* __restrict__ flags,
                                                       const uint64_t* __restrict__ prefix, int bits,
                                                       uint64_t* __restrict__ keys, const uint32_t* __restrict__ rank,
                                                       long long* __restrict__ faces) {
    __shared__ uint32_t s_n[kTetIters][4][2];
    const long long base = (long long)blockIdx.x * kTetsPerBlock;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t code[kTetIters], p1[kTetIters], p2[kTetIters], vid[kTetIters][4];
#pragma unroll
    for (int j = 0; j < kTetIters; j++) {
        const long long t = base + j * 256 + threadIdx.x;
        code[j] = 0u;
        if (t < T) {
            long long v[4];
            bool bad;
            load_tet<I>(tets, t, v);
            code[j] = tet_case(v, V, flags, bad);
#pragma unroll
            for (int i = 0; i < 4; i++) vid[j][i] = (uint32_t)v[i];  // < V <= 2^31 when code != 0
        }
        const bool two = code[j] != 0u && two_triangles(code[j]);
        const unsigned long long b1 = __ballot(code[j] != 0u && !two), b2 = __ballot(two);
        p1[j] = (uint32_t)__builtin_popcountll(b1 & below);
        p2[j] = (uint32_t)__builtin_popcountll(b2 & below);
        if (lane == 0) s_n[j][wave][0] = (uint32_t)__builtin_popcountll(b1), s_n[j][wave][1] = (uint32_t)__builtin_popcountll(b2);
    }
    __syncthreads();
    const uint64_t pre = prefix[blockIdx.x];
    uint32_t run1 = (uint32_t)pre, run2 = (uint32_t)(pre >> 32);
#pragma unroll
    for (int j = 0; j < kTetIters; j++) {
        uint32_t n1 = run1, n2 = run2;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            if (w < wave) n1 += s_n[j][w][0], n2 += s_n[j][w][1];
            run1 += s_n[j][w][0], run2 += s_n[j][w][1];
        }
        const uint32_t c = code[j];
        if (c == 0u) continue;
        n1 += p1[j], n2 += p2[j];
        const uint64_t slot = 3ull * n1 + 4ull * n2;
        // crossing mask over the edges 01, 02, 03, 12, 13, 23
        constexpr int ea[6] = {0, 0, 0, 1, 1, 2}, eb[6] = {1, 2, 3, 2, 3, 3};
        uint32_t cross = 0u;
#pragma unroll
        for (int e = 0; e < 6; e++) cross |= (((c >> ea[e]) ^ (c >> eb[e])) & 1u) << e;
        if (!FACES) {
            uint32_t k = 0;
#pragma unroll
            for (int e = 0; e < 6; e++) {
                if (cross >> e & 1u) {
                    const uint32_t x = vid[j][ea[e]], y = vid[j][eb[e]];
                    const uint64_t a = x < y ? x : y, b = x < y ? y : x;
                    keys[slot + k++] = a << bits | b;
                }
            }
        } else {
            const bool flip = c >= 8u;
            const uint32_t tri = kTetTriangles[flip ? 15u - c : c];
            const int ntri = two_triangles(c) ? 2 : 1;
            long long* out = faces + 3 * ((uint64_t)n1 + 2ull * n2);
            for (int q = 0; q < ntri; q++) {
                uint32_t r[3];
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const uint32_t e = (tri >> (9 * q + 3 * i)) & 7u;
                    r[i] = rank[slot + __builtin_popcount(cross & ((1u << e) - 1u))];
                }
                out[3 * q] = r[0];
                out[3 * q + 1] = flip ? r[2] : r[1];
                out[3 * q + 2] = flip ? r[1] : r[2];
            }
        }
    }
}

// heads[i] = 1 where sorted key i starts a run of equal keys
__global__ void __launch_bounds__(256) tet_heads_kernel(size_t S, const uint64_t* __restrict__ ks,
                                                        uint32_t* __restrict__ heads) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < S) heads[i] = (i == 0 || ks[i] != ks[i - 1]) ? 1u : 0u;
}

// urank = inclusive scan of heads: key i is mesh vertex urank[i] - 1.  Every slot learns its
// vertex; each run's first key writes the vertex's edge.
__global__ void __launch_bounds__(256) tet_edges_kernel(size_t S, int bits, const uint64_t* __restrict__ ks,
                                                        const uint32_t* __restrict__ slots,
                                                        const uint32_t* __restrict__ urank,
                                                        uint32_t* __restrict__ rank, long long* __restrict__ edge_ids) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    const uint64_t k = ks[i];
    const uint32_t r = urank[i] - 1u;
    rank[slots[i]] = r;
    if (i == 0 || k != ks[i - 1]) {
        edge_ids[2 * (size_t)r] = (long long)(k >> bits);
        edge_ids[2 * (size_t)r + 1] = (long long)(k & ((1ull << bits) - 1ull));
    }
}

hipError_t launch_tet_flags(long long V, const float* sdf, const uint8_t* valid, const TetCountState& s,
                            hipStream_t stream) {
    hipLaunchKernelGGL(tet_flags_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, stream, V, sdf, valid,
                       s.flags);
    return hipGetLastError();
}

hipError_t launch_tet_count(long long T, long long V, const void* tets, bool is64, const TetCountState& s,
                            hipStream_t stream) {
    hipError_t e = hipMemsetAsync(s.bad, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)s.nblocks);
    if (is64)
        hipLaunchKernelGGL(tet_count_kernel<int64_t>, grid, dim3(256), 0, stream, T, V, (const int64_t*)tets, s.flags,
                           s.partials, s.bad);
    else
        hipLaunchKernelGGL(tet_count_kernel<int32_t>, grid, dim3(256), 0, stream, T, V, (const int32_t*)tets, s.flags,
                           s.partials, s.bad);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t bytes = s.scan_tmp_bytes;
    return rocprim::exclusive_scan(s.scan_tmp, bytes, s.partials, s.partials, (uint64_t)0, (size_t)s.nblocks + 1,
                                   rocprim::plus<uint64_t>(), stream);
}

template <bool FACES>
static hipError_t launch_walk(long long T, long long V, const void* tets, bool is64, const TetCountState& s,
                              const TetEdgeState& es, long long* faces, hipStream_t stream) {
    const dim3 grid((unsigned)s.nblocks);
    if (is64)
        hipLaunchKernelGGL((tet_walk_kernel<int64_t, FACES>), grid, dim3(256), 0, stream, T, V, (const int64_t*)tets,
                           s.flags, s.partials, es.bits, es.keys, es.rank, faces);
    else
        hipLaunchKernelGGL((tet_walk_kernel<int32_t, FACES>), grid, dim3(256), 0, stream, T, V, (const int32_t*)tets,
                           s.flags, s.partials, es.bits, es.keys, es.rank, faces);
    return hipGetLastError();
}

hipError_t launch_tet_emit(long long T, long long V, const void* tets, bool is64, const TetCountState& s,
                           const TetEdgeState& es, hipStream_t stream) {
    return launch_walk<false>(T, V, tets, is64, s, es, nullptr, stream);
}

hipError_t launch_tet_sort(const TetEdgeState& es, hipStream_t stream) {
    size_t bytes = es.tmp_bytes;
    return rocprim::radix_sort_pairs<TetSortConfig>(es.tmp, bytes, es.keys, es.keys_sorted,
                                                    rocprim::counting_iterator<uint32_t>(0), es.slots_sorted, es.S, 0u,
                                                    (unsigned)(2 * es.bits), stream);
}

// after this heads[S - 1] is the number of mesh vertices
hipError_t launch_tet_ranks(const TetEdgeState& es, hipStream_t stream) {
    hipLaunchKernelGGL(tet_heads_kernel, dim3((unsigned)((es.S + 255) / 256)), dim3(256), 0, stream, es.S,
                       es.keys_sorted, es.heads);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = es.tmp_bytes;
    return rocprim::inclusive_scan(es.tmp, bytes, es.heads, es.heads, es.S, rocprim::plus<uint32_t>(), stream);
}

hipError_t launch_tet_edges(const TetEdgeState& es, long long* edge_ids, hipStream_t stream) {
    hipLaunchKernelGGL(tet_edges_kernel, dim3((unsigned)((es.S + 255) / 256)), dim3(256), 0, stream, es.S, es.bits,
                       es.keys_sorted, es.slots_sorted, es.heads, es.rank, edge_ids);
    return hipGetLastError();
}

hipError_t launch_tet_faces(long long T, long long V, const void* tets, bool is64, const TetCountState& s,
                            const TetEdgeState& es, long long* faces, hipStream_t stream) {
    return launch_walk<true>(T, V, tets, is64, s, es, faces, stream);
}

}  // namespace gsr
