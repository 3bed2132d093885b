// pointeval.hip — the point-cloud half of the DTU Chamfer evaluation on gfx950
// (the reference's dtu_eval/eval.py --mode mesh, which runs numpy, a
// multiprocessing pool and sklearn KD-trees on the CPU): mesh -> sampled
// cloud, greedy radius thinning, bounded nearest-point distance.  All geometry
// is float64 with contraction off, so products and sums round as numpy's do.
//
// gsr_mesh_sample_points (eval.py:48-71):
//   1. sample_count_kernel  per triangle with area2 > 0 the number of lattice
//                           points (i + .5) / max(n1, 1e-7) + (j + .5) / max(n2, 1e-7) < 1,
//                           0 <= i <= n1, 0 <= j <= n2; a row's count is an estimate
//                           fixed up with the float64 predicate itself (it is
//                           monotone in j), so the count is the reference's;
//   2. rocPRIM exclusive scan of the counts (uint64);
//   3. sample_emit_kernel   one lane per output point: the triangle by binary
//                           search in the offsets, the row by walking the row
//                           counts, then the reference's v1 k0 + v2 k1 + p0.  A
//                           triangle's points are spread over as many lanes as it
//                           has points; their order is i outer, j inner.
//
// gsr_points_downsample (eval.py:80-94, the points already in shuffled order):
// the survivors of "walking the order, a point stays iff no earlier survivor
// lies within radius" are the lexicographically first maximal independent set
// of the radius graph.  Rounds: an undecided point is kept once every earlier
// neighbour is removed, removed once one earlier neighbour is kept; states only
// ever go undecided -> final, the final states are the sequential loop's, and a
// round may read states written in the same round (they are final).  The lowest
// undecided rank is decided every round, so the loop ends; it runs until a round
// leaves nothing undecided.  Neighbours: cells of side radius (1 + 2^-20) (the
// margin absorbs the rounding of the cell coordinate, so two points within
// radius are never two cells apart), keys cx | cy | cz packed in the fewest
// bits, a stable rocPRIM radix sort of (key, rank), 9 runs of 3 cells each found
// by binary search.  Grids of more than 64 key bits hash the cell instead and
// look 27 cells up; a collision only adds candidates, every one is distance-
// tested.  The test is sklearn's: dx^2 + dy^2 + dz^2 <= radius^2.
//
// gsr_points_nearest: ref is sorted by the packed cell of a grid whose cell side
// comes from the density of ref (the largest of cbrt(volume / R), sqrt(largest
// face / R), longest edge / R, so flat and thin sets get cells too), queries by
// the Morton code of their cell.  A 256-lane workgroup owns 256 consecutive
// sorted queries and the box W of their cells.  Shell s is W grown by s cells
// minus W grown by s - 1: every lane finds the run of one (x, y, z-range) piece
// by binary search, the runs of 256 pieces are laid end to end by a block scan
// and staged 512 points at a time into LDS, and every unfinished lane scans them
// with broadcast reads — a cell leaves HBM once per workgroup.  A lane is
// finished when no unvisited cell can hold a point nearer than its best or than
// max_dist (distance to the faces of the grown box that still have cells behind
// them, less 2^-20 cell for the rounding of cell coordinates); the workgroup
// stops when all are.  The result is exact within max_dist.  (The grid helpers and the
// search itself live in pointgrid.h, shared with tnteval.hip's indexed query.)
#pragma clang fp contract(off)

#include "pointgrid.h"

namespace gsr {

// ---- bounds ------------------------------------------------------------------------------------------------------

// partials [gridDim.x][6]; `final` reduces partials themselves (n rows of 6: min xyz, max xyz)
__global__ void __launch_bounds__(256) pe_bounds_kernel(long long n, const double* __restrict__ pts, int final,
                                                        double* __restrict__ out) {
    __shared__ double s[4][6];
    double v[6] = {DBL_MAX, DBL_MAX, DBL_MAX, -DBL_MAX, -DBL_MAX, -DBL_MAX};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            v[c] = fmin(v[c], final ? pts[6 * i + c] : pts[3 * i + c]);
            v[3 + c] = fmax(v[3 + c], final ? pts[6 * i + 3 + c] : pts[3 * i + c]);
        }
    }
    block_minmax6(v, s);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 6; k++) out[6 * blockIdx.x + k] = v[k];
    }
}

hipError_t launch_point_bounds(long long n, const double* pts, double* partials, double* bounds, hipStream_t stream) {
    const int nred = (int)((n + 255) / 256 < kPeReduceBlocks ? (n + 255) / 256 : kPeReduceBlocks);
    hipLaunchKernelGGL(pe_bounds_kernel, dim3(nred), dim3(256), 0, stream, n, pts, 0, partials);
    hipLaunchKernelGGL(pe_bounds_kernel, dim3(1), dim3(256), 0, stream, (long long)nred, partials, 1, bounds);
    return hipGetLastError();
}

// ---- the grid ----------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) pe_keys_kernel(long long n, const double* __restrict__ pts, PointGrid g,
                                                      uint64_t* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    keys[i] = pe_key(g, pe_cell(pts[3 * i], g.mn[0], g.cs, g.nc[0]), pe_cell(pts[3 * i + 1], g.mn[1], g.cs, g.nc[1]),
                     pe_cell(pts[3 * i + 2], g.mn[2], g.cs, g.nc[2]));
}

__global__ void __launch_bounds__(256) pe_gather_kernel(long long n, const double* __restrict__ pts,
                                                        const uint32_t* __restrict__ order, double* __restrict__ sx,
                                                        double* __restrict__ sy, double* __restrict__ sz,
                                                        uint32_t* __restrict__ state) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t o = order[i];
    sx[i] = pts[3 * o], sy[i] = pts[3 * o + 1], sz[i] = pts[3 * o + 2];
    if (state) state[i] = 0u;
}

hipError_t launch_point_sort(long long n, const double* pts, const PointGrid& g, uint64_t* keys, uint64_t* keys_sorted,
                             uint32_t* order, double* sx, double* sy, double* sz, uint32_t* state, void* tmp,
                             size_t tmp_bytes, hipStream_t stream) {
    const dim3 grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(pe_keys_kernel, grid, dim3(256), 0, stream, n, pts, g, keys);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned bits = g.hashed ? 64u : (unsigned)(g.bx + g.by + g.bz > 0 ? g.bx + g.by + g.bz : 1);
    size_t need = 0, bytes = tmp_bytes;
    (void)rocprim::radix_sort_pairs<PeSortConfig>(nullptr, need, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                  rocprim::counting_iterator<uint32_t>(0), (uint32_t*)nullptr,
                                                  (size_t)n, 0u, bits);
    if (need > tmp_bytes) return hipErrorInvalidValue;
    // stable: a cell's points stay in ascending input order
    e = rocprim::radix_sort_pairs<PeSortConfig>(tmp, bytes, keys, keys_sorted, rocprim::counting_iterator<uint32_t>(0),
                                                order, (size_t)n, 0u, bits, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pe_gather_kernel, grid, dim3(256), 0, stream, n, pts, order, sx, sy, sz, state);
    return hipGetLastError();
}

// ---- gsr_mesh_sample_points --------------------------------------------------------------------------------------

size_t carve_point_sample(void* base, long long F, PointSampleState& s) {
    Carver c(base);
    s.offsets = c.take<uint64_t>((size_t)F + 1);
    s.bad = c.take<uint32_t>(1);
    s.tmp_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, s.tmp_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, 0ull, (size_t)F + 1,
                                  rocprim::plus<uint64_t>());
    s.tmp = c.take<char>(s.tmp_bytes);
    return c.off + 256;
}

struct SampleTri {
    double p0[3], v1[3], v2[3];
    double n1, n2, d1, d2;  // d = max(n, 1e-7)
};

// eval.py:50-65 for one triangle; false when area2 > 0 fails.  `bad`: a vertex id outside [0, V), or a
// lattice of 2^31 or more rows or columns (non-finite input).
template <class I>
__device__ __forceinline__ bool sample_tri(const double* __restrict__ vtx, const I* __restrict__ faces, long long t,
                                           long long V, double density, SampleTri& s, bool& bad) {
    const long long a = (long long)faces[3 * t], b = (long long)faces[3 * t + 1], c = (long long)faces[3 * t + 2];
    if ((unsigned long long)a >= (unsigned long long)V || (unsigned long long)b >= (unsigned long long)V ||
        (unsigned long long)c >= (unsigned long long)V) {
        bad = true;
        return false;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        s.p0[k] = vtx[3 * a + k];
        s.v1[k] = vtx[3 * b + k] - s.p0[k];
        s.v2[k] = vtx[3 * c + k] - s.p0[k];
    }
    const double l1 = sqrt(s.v1[0] * s.v1[0] + s.v1[1] * s.v1[1] + s.v1[2] * s.v1[2]);
    const double l2 = sqrt(s.v2[0] * s.v2[0] + s.v2[1] * s.v2[1] + s.v2[2] * s.v2[2]);
    const double cx = s.v1[1] * s.v2[2] - s.v1[2] * s.v2[1];
    const double cy = s.v1[2] * s.v2[0] - s.v1[0] * s.v2[2];
    const double cz = s.v1[0] * s.v2[1] - s.v1[1] * s.v2[0];
    const double area2 = sqrt(cx * cx + cy * cy + cz * cz);
    if (!(area2 > 0.0)) return false;
    const double thr = density * sqrt(l1 * l2 / area2);
    s.n1 = floor(l1 / thr);
    s.n2 = floor(l2 / thr);
    if (!(s.n1 >= 0.0 && s.n1 < 2147483648.0 && s.n2 >= 0.0 && s.n2 < 2147483648.0)) {
        bad = true;
        return false;
    }
    s.d1 = fmax(s.n1, 1e-7);
    s.d2 = fmax(s.n2, 1e-7);
    return true;
}

// the number of j in [0, n2] with c0 + (j + .5) / d2 < 1.  The sum is monotone in j, so the last j that
// passes is an estimate corrected by the predicate itself.
__device__ __forceinline__ long long sample_row_count(double c0, double n2, double d2) {
    const long long hi = (long long)n2;
    const double e = floor((1.0 - c0) * n2 - 0.5);
    long long j = !(e >= -1.0) ? -1ll : (e > n2 ? hi : (long long)e);
    while (j < hi && c0 + ((double)(j + 1) + 0.5) / d2 < 1.0) j++;
    while (j >= 0 && !(c0 + ((double)j + 0.5) / d2 < 1.0)) j--;
    return j + 1;
}

template <class I>
__global__ void __launch_bounds__(256) sample_count_kernel(long long F, long long V, const double* __restrict__ vtx,
                                                           const I* __restrict__ faces, double density,
                                                           uint64_t* __restrict__ counts,
                                                           uint32_t* __restrict__ bad_flag) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (t <= F) {
        uint64_t n = 0;
        SampleTri s;
        if (t < F && sample_tri<I>(vtx, faces, t, V, density, s, bad)) {
            const long long rows = (long long)s.n1;
            for (long long i = 0; i <= rows; i++) {
                const long long c = sample_row_count(((double)i + 0.5) / s.d1, s.n2, s.d2);
                if (c == 0) break;  // the rows only get shorter
                n += (uint64_t)c;
            }
        }
        counts[t] = n;
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad_flag, 1u);
}

template <class I>
__global__ void __launch_bounds__(256) sample_emit_kernel(long long F, long long V, unsigned long long S,
                                                          const double* __restrict__ vtx, const I* __restrict__ faces,
                                                          double density, const uint64_t* __restrict__ offsets,
                                                          double* __restrict__ out) {
    const unsigned long long gidx = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (gidx >= S) return;
    // the triangle: the last t with offsets[t] <= gidx (offsets[F] = S > gidx)
    long long lo = 0, hi = F;
    while (lo < hi) {
        const long long mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] <= gidx) lo = mid;
        else hi = mid - 1;
    }
    SampleTri s;
    bool bad = false;
    if (!sample_tri<I>(vtx, faces, lo, V, density, s, bad)) return;  // not reached: its count was > 0
    long long k = (long long)(gidx - offsets[lo]), i = 0;
    for (;; i++) {
        const long long c = sample_row_count(((double)i + 0.5) / s.d1, s.n2, s.d2);
        if (k < c || c == 0) break;
        k -= c;
    }
    const double k0 = ((double)i + 0.5) / s.d1, k1 = ((double)k + 0.5) / s.d2;
#pragma unroll
    for (int c = 0; c < 3; c++) out[3 * ((size_t)V + gidx) + c] = s.v1[c] * k0 + s.v2[c] * k1 + s.p0[c];
}

// after this offsets[F] is the number of sampled points
hipError_t launch_sample_count(long long F, long long V, const double* vertices, const void* faces, bool is64,
                               double density, const PointSampleState& s, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(s.bad, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((F + 256) / 256));
    if (is64)
        hipLaunchKernelGGL(sample_count_kernel<int64_t>, grid, dim3(256), 0, stream, F, V, vertices,
                           (const int64_t*)faces, density, s.offsets, s.bad);
    else
        hipLaunchKernelGGL(sample_count_kernel<int32_t>, grid, dim3(256), 0, stream, F, V, vertices,
                           (const int32_t*)faces, density, s.offsets, s.bad);
    return hipGetLastError();
}

hipError_t launch_sample_scan(long long F, const PointSampleState& s, hipStream_t stream) {
    size_t bytes = s.tmp_bytes;
    return rocprim::exclusive_scan(s.tmp, bytes, s.offsets, s.offsets, 0ull, (size_t)F + 1, rocprim::plus<uint64_t>(),
                                   stream);
}

hipError_t launch_sample_emit(long long F, long long V, unsigned long long S, const double* vertices,
                              const void* faces, bool is64, double density, const PointSampleState& s, double* out,
                              hipStream_t stream) {
    const dim3 grid((unsigned)((S + 255) / 256));
    if (is64)
        hipLaunchKernelGGL(sample_emit_kernel<int64_t>, grid, dim3(256), 0, stream, F, V, S, vertices,
                           (const int64_t*)faces, density, s.offsets, out);
    else
        hipLaunchKernelGGL(sample_emit_kernel<int32_t>, grid, dim3(256), 0, stream, F, V, S, vertices,
                           (const int32_t*)faces, density, s.offsets, out);
    return hipGetLastError();
}

// ---- gsr_points_downsample ---------------------------------------------------------------------------------------

size_t carve_point_thin(void* base, long long N, PointThinState& s) {
    Carver c(base);
    const size_t n = (size_t)N;
    s.N = N;
    s.partials = c.take<double>((size_t)kPeReduceBlocks * 6);
    s.bounds = c.take<double>(8);
    s.keys = c.take<uint64_t>(n);
    s.keys_sorted = c.take<uint64_t>(n);
    s.order = c.take<uint32_t>(n);
    s.sx = c.take<double>(n);
    s.sy = c.take<double>(n);
    s.sz = c.take<double>(n);
    s.state = c.take<uint32_t>(n);
    s.undecided = c.take<uint32_t>(1);
    s.flags = reinterpret_cast<uint32_t*>(s.keys);  // [N + 1] the unsorted keys are dead after the sort
    size_t scan = 0;
    (void)rocprim::exclusive_scan(nullptr, scan, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n + 1,
                                  rocprim::plus<uint32_t>());
    s.tmp_bytes = pe_sort_bytes(n);
    if (scan > s.tmp_bytes) s.tmp_bytes = scan;
    s.tmp = c.take<char>(s.tmp_bytes);
    return c.off + 256;
}

// the grid of gsr_points_downsample from the bounds [min xyz, max xyz]; false when an axis has 2^31 or more cells
bool point_thin_grid(const double* bounds, double radius, PointGrid& g) {
    g.cs = radius * (1.0 + 1.0 / 1048576.0);
    for (int k = 0; k < 3; k++) {
        g.mn[k] = bounds[k];
        g.mx[k] = bounds[3 + k];
        const double cells = floor((bounds[3 + k] - bounds[k]) / g.cs) + 1.0;
        if (!(cells >= 1.0 && cells < 2147483648.0)) return false;
        g.nc[k] = (long long)cells;
    }
    g.bx = pe_bits(g.nc[0]), g.by = pe_bits(g.nc[1]), g.bz = pe_bits(g.nc[2]);
    g.hashed = g.bx + g.by + g.bz > 64 ? 1 : 0;
    return true;
}

enum : uint32_t { kThinUndecided = 0u, kThinKept = 1u, kThinRemoved = 2u };

__device__ __forceinline__ uint32_t thin_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one round over the sorted points; *undecided is set when a point is still undecided after it
__global__ void __launch_bounds__(256) thin_round_kernel(long long N, PointGrid g, double r2,
                                                         const uint64_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ order,
                                                         const double* __restrict__ sx, const double* __restrict__ sy,
                                                         const double* __restrict__ sz, uint32_t* __restrict__ state,
                                                         uint32_t* __restrict__ undecided) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool open = false;
    if (i < N && thin_load(state + i) == kThinUndecided) {
        const uint32_t rank = order[i];
        const double x = sx[i], y = sy[i], z = sz[i];
        const long long c[3] = {pe_cell(x, g.mn[0], g.cs, g.nc[0]), pe_cell(y, g.mn[1], g.cs, g.nc[1]),
                                pe_cell(z, g.mn[2], g.cs, g.nc[2])};
        bool kept_near = false;
        // packed keys: the three z cells of one (x, y) are one run; hashed keys: one run per cell
        const int nz = g.hashed ? 3 : 1;
        for (int q = 0; q < 9 * nz && !kept_near; q++) {
            const long long cx = c[0] + (q / nz) / 3 - 1, cy = c[1] + (q / nz) % 3 - 1;
            if (cx < 0 || cx >= g.nc[0] || cy < 0 || cy >= g.nc[1]) continue;
            long long z0 = c[2] - 1, z1 = c[2] + 1;
            if (g.hashed) z0 = z1 = c[2] + q % 3 - 1;
            z0 = z0 < 0 ? 0 : z0;
            z1 = z1 >= g.nc[2] ? g.nc[2] - 1 : z1;
            if (z0 > z1) continue;
            const uint32_t a = pe_lower(keys, 0u, (uint32_t)N, pe_key(g, cx, cy, z0));
            const uint32_t b = pe_upper(keys, a, (uint32_t)N, pe_key(g, cx, cy, z1));
            for (uint32_t j = a; j < b; j++) {
                if (order[j] >= rank) continue;  // only earlier points decide (the point itself: equal)
                const double dx = x - sx[j], dy = y - sy[j], dz = z - sz[j];
                if (!(dx * dx + dy * dy + dz * dz <= r2)) continue;
                const uint32_t st = thin_load(state + j);
                if (st == kThinKept) {
                    kept_near = true;
                    break;
                }
                open |= st == kThinUndecided;
            }
        }
        if (kept_near) open = false;
        if (kept_near || !open)
            __hip_atomic_store(state + i, kept_near ? kThinRemoved : kThinKept, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    if (__ballot(open) != 0ull && (threadIdx.x & 63) == 0)
        __hip_atomic_store(undecided, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// flags[rank] = kept, flags[N] = 0: their exclusive scan ends with the number of survivors
__global__ void __launch_bounds__(256) thin_flags_kernel(long long N, const uint32_t* __restrict__ order,
                                                         const uint32_t* __restrict__ state,
                                                         uint32_t* __restrict__ flags) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i > N) return;
    if (i == N) flags[N] = 0u;
    else flags[order[i]] = state[i] == kThinKept ? 1u : 0u;
}

__global__ void __launch_bounds__(256) thin_write_kernel(long long N, const uint32_t* __restrict__ flags,
                                                         long long* __restrict__ out) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const uint32_t o = flags[r];
    if (flags[r + 1] != o) out[o] = r;
}

hipError_t launch_thin_round(const PointThinState& s, const PointGrid& g, double radius, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(s.undecided, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(thin_round_kernel, dim3((unsigned)((s.N + 255) / 256)), dim3(256), 0, stream, s.N, g,
                       radius * radius, s.keys_sorted, s.order, s.sx, s.sy, s.sz, s.state, s.undecided);
    return hipGetLastError();
}

// after this flags[N] is the number of survivors
hipError_t launch_thin_plan(const PointThinState& s, hipStream_t stream) {
    hipLaunchKernelGGL(thin_flags_kernel, dim3((unsigned)((s.N + 256) / 256)), dim3(256), 0, stream, s.N, s.order,
                       s.state, s.flags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = s.tmp_bytes;
    return rocprim::exclusive_scan(s.tmp, bytes, s.flags, s.flags, 0u, (size_t)s.N + 1, rocprim::plus<uint32_t>(),
                                   stream);
}

hipError_t launch_thin_write(const PointThinState& s, long long* kept, hipStream_t stream) {
    hipLaunchKernelGGL(thin_write_kernel, dim3((unsigned)((s.N + 255) / 256)), dim3(256), 0, stream, s.N, s.flags,
                       kept);
    return hipGetLastError();
}

// ---- gsr_points_nearest ------------------------------------------------------------------------------------------

size_t carve_point_nearest(void* base, long long Q, long long R, PointNearestState& s) {
    Carver c(base);
    const size_t q = (size_t)Q, r = (size_t)R;
    s.partials = c.take<double>((size_t)kPeReduceBlocks * 6);
    s.bounds = c.take<double>(8);
    s.rkeys = c.take<uint64_t>(r);
    s.rkeys_sorted = c.take<uint64_t>(r);
    s.rorder = c.take<uint32_t>(r);
    s.rx = c.take<double>(r);
    s.ry = c.take<double>(r);
    s.rz = c.take<double>(r);
    s.qkeys = c.take<uint64_t>(q);
    s.qkeys_sorted = c.take<uint64_t>(q);
    s.qorder = c.take<uint32_t>(q);
    s.tmp_bytes = pe_sort_bytes(q > r ? q : r);
    s.tmp = c.take<char>(s.tmp_bytes);
    return c.off + 256;
}

// the grid of gsr_points_nearest: the cell side from the density of ref, at most 2^20 cells an axis
void point_nearest_grid(const double* bounds, long long R, PointGrid& g) {
    double e[3], longest = 0.0;
    for (int k = 0; k < 3; k++) {
        g.mn[k] = bounds[k];
        g.mx[k] = bounds[3 + k];
        e[k] = bounds[3 + k] - bounds[k];
        if (e[k] > longest) longest = e[k];
    }
    const double face = fmax(e[0] * e[1], fmax(e[1] * e[2], e[0] * e[2]));
    double cs = cbrt(e[0] * e[1] * e[2] / (double)R);
    cs = fmax(cs, sqrt(face / (double)R));
    cs = fmax(cs, longest / (double)R);
    cs = fmax(cs, longest / 1048576.0);
    if (!(cs > 0.0) || !(cs < DBL_MAX)) cs = 1.0;  // one point, or all the same
    g.cs = cs;
    for (int k = 0; k < 3; k++) {
        double cells = floor(e[k] / cs) + 1.0;
        if (!(cells >= 1.0)) cells = 1.0;
        if (cells > 2097152.0) cells = 2097152.0;
        g.nc[k] = (long long)cells;
    }
    g.bx = pe_bits(g.nc[0]), g.by = pe_bits(g.nc[1]), g.bz = pe_bits(g.nc[2]);
    g.hashed = 0;
}

__device__ __forceinline__ uint64_t pe_spread3(uint64_t x) {  // 21 bits -> every third bit
    x &= 0x1fffffull;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__global__ void __launch_bounds__(256) nearest_qkeys_kernel(long long Q, const double* __restrict__ query, PointGrid g,
                                                            uint64_t* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Q) return;
    keys[i] = pe_spread3((uint64_t)pe_cell(query[3 * i], g.mn[0], g.cs, g.nc[0])) << 2 |
              pe_spread3((uint64_t)pe_cell(query[3 * i + 1], g.mn[1], g.cs, g.nc[1])) << 1 |
              pe_spread3((uint64_t)pe_cell(query[3 * i + 2], g.mn[2], g.cs, g.nc[2]));
}

__global__ void __launch_bounds__(256) nearest_fill_kernel(long long Q, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < Q) out[i] = HUGE_VAL;
}

__global__ void __launch_bounds__(256) nearest_kernel(long long Q, const double* __restrict__ query,
                                                      const uint32_t* __restrict__ qorder, long long R,
                                                      const uint64_t* __restrict__ rkeys, const double* __restrict__ rx,
                                                      const double* __restrict__ ry, const double* __restrict__ rz,
                                                      PointGrid g, double max_dist, double* __restrict__ out) {
    nearest_search_block<false>(Q, query, qorder, R, rkeys, nullptr, rx, ry, rz, g, max_dist, out, nullptr);
}

hipError_t launch_nearest_fill(long long Q, double* out, hipStream_t stream) {
    hipLaunchKernelGGL(nearest_fill_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, stream, Q, out);
    return hipGetLastError();
}

hipError_t launch_nearest_qsort(long long Q, const double* query, const PointGrid& g, const PointNearestState& s,
                                hipStream_t stream) {
    hipLaunchKernelGGL(nearest_qkeys_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, stream, Q, query, g,
                       s.qkeys);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t bytes = s.tmp_bytes;
    return rocprim::radix_sort_pairs<PeSortConfig>(s.tmp, bytes, s.qkeys, s.qkeys_sorted,
                                                   rocprim::counting_iterator<uint32_t>(0), s.qorder, (size_t)Q, 0u,
                                                   63u, stream);
}

hipError_t launch_nearest_search(long long Q, const double* query, long long R, const PointGrid& g,
                                 const PointNearestState& s, double max_dist, double* out, hipStream_t stream) {
    hipLaunchKernelGGL(nearest_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, stream, Q, query, s.qorder, R,
                       s.rkeys_sorted, s.rx, s.ry, s.rz, g, max_dist, out);
    return hipGetLastError();
}

}  // namespace gsr
