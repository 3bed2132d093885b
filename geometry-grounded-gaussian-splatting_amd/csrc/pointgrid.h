// pointgrid.h — what pointeval.hip (DTU Chamfer) and tnteval.hip (TnT F-score) share: the cell grid
// of a float64 cloud (cell coordinate, packed / hashed key, binary searches in the sorted keys), the
// stable radix sort's configuration, and the exact bounded nearest-point search staged through LDS.
// Device and host helpers of those two translation units only; both compile with contraction off.
#pragma once

#include <float.h>
#include <math.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "gsr_kernels.h"
#include "gsr_wave.h"

namespace gsr {

constexpr int kPeReduceBlocks = 512;
constexpr int kPeStage = 512;  // points staged in LDS at a time (12 KB)

using PeSortConfig = rocprim::default_config;

static inline size_t pe_sort_bytes(size_t n) {
    size_t b = 0;
    (void)rocprim::radix_sort_pairs<PeSortConfig>(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                  rocprim::counting_iterator<uint32_t>(0), (uint32_t*)nullptr, n, 0u,
                                                  64u);
    return b;
}

static inline int pe_bits(long long n) {  // bits that hold 0 .. n - 1
    int b = 0;
    while (b < 63 && (1ll << b) < n) b++;
    return b;
}

__device__ __forceinline__ long long pe_cell(double x, double mn, double cs, long long nc) {
    double u = floor((x - mn) / cs);
    u = fmin(fmax(u, 0.0), (double)(nc - 1));  // a NaN coordinate lands in cell 0
    return u == u ? (long long)u : 0ll;
}

__device__ __forceinline__ uint64_t pe_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

__device__ __forceinline__ uint64_t pe_key(const PointGrid& g, long long cx, long long cy, long long cz) {
    if (g.hashed) return pe_mix(pe_mix(pe_mix((uint64_t)cx) ^ (uint64_t)cy) ^ (uint64_t)cz);
    return ((uint64_t)cx << (g.by + g.bz)) | ((uint64_t)cy << g.bz) | (uint64_t)cz;
}

__device__ __forceinline__ uint32_t pe_lower(const uint64_t* __restrict__ keys, uint32_t lo, uint32_t hi, uint64_t k) {
    while (lo < hi) {  // first position in [lo, hi) whose key is >= k
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint32_t pe_upper(const uint64_t* __restrict__ keys, uint32_t lo, uint32_t hi, uint64_t k) {
    while (lo < hi) {  // first position in [lo, hi) whose key is > k
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] <= k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// exclusive scan of one value per lane over the 256-lane block; total = the sum
__device__ __forceinline__ uint32_t pe_block_scan(uint32_t v, uint32_t* s_wave, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t inc = wave_incl_scan(v);
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    for (int k = 0; k < wave; k++) before += s_wave[k];
    total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
    return before + inc - v;
}

// the staged positions of the indexed search; nothing (and no LDS) without an index
template <bool kIndex>
struct NearestStagePos {
    uint32_t v[kPeStage];
};
template <>
struct NearestStagePos<false> {};

// The search of one 256-lane workgroup (the file comment of pointeval.hip): out[src] = the distance
// to the nearest ref point where that is < max_dist, else +inf.  kIndex: out_idx[src] = the
// position of that point in the caller's ref (rorder: sorted position -> original), -1 beyond;
// among equally near points the lowest original position wins, whatever the order of the scan.
// Without kIndex the arithmetic and its order are those of gsr_points_nearest.
template <bool kIndex>
__device__ __forceinline__ void nearest_search_block(long long Q, const double* __restrict__ query,
                                                     const uint32_t* __restrict__ qorder, long long R,
                                                     const uint64_t* __restrict__ rkeys,
                                                     const uint32_t* __restrict__ rorder,
                                                     const double* __restrict__ rx, const double* __restrict__ ry,
                                                     const double* __restrict__ rz, const PointGrid& g,
                                                     double max_dist, double* __restrict__ out,
                                                     long long* __restrict__ out_idx) {
    __shared__ double s_x[kPeStage], s_y[kPeStage], s_z[kPeStage];
    __shared__ NearestStagePos<kIndex> s_p;
    __shared__ uint32_t s_a[256], s_off[256], s_wave[4];
    __shared__ int s_box[6];
    const int tid = threadIdx.x;
    const long long idx = (long long)blockIdx.x * 256 + tid;
    const bool valid = idx < Q;
    const size_t src = valid ? qorder[idx] : 0;
    double q[3] = {0.0, 0.0, 0.0};
    int c[3] = {0, 0, 0};
    bool done = !valid;
    if (valid) {
        double bd2 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            q[k] = query[3 * src + k];
            c[k] = (int)pe_cell(q[k], g.mn[k], g.cs, g.nc[k]);
            const double d = fmax(fmax(g.mn[k] - q[k], q[k] - g.mx[k]), 0.0);
            bd2 += d * d;
        }
        // farther than max_dist from the box of ref (with room for the rounding of the three squares)
        done = bd2 > max_dist * max_dist * (1.0 + 1e-9);
    }
    if (tid < 6) s_box[tid] = tid < 3 ? 0x7fffffff : -1;
    __syncthreads();
    if (!done) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            atomicMin(&s_box[k], c[k]);
            atomicMax(&s_box[3 + k], c[k]);
        }
    }
    __syncthreads();
    int w_lo[3], w_hi[3];
#pragma unroll
    for (int k = 0; k < 3; k++) w_lo[k] = s_box[k], w_hi[k] = s_box[3 + k];
    double best = HUGE_VAL;
    uint32_t best_pos = 0xffffffffu;
    if (w_hi[0] >= 0) {  // some lane has a search to do
        int p_lo[3] = {0, 0, 0}, p_hi[3] = {-1, -1, -1};
        for (int s = 0;; s++) {
            int e_lo[3], e_hi[3];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                e_lo[k] = w_lo[k] - s < 0 ? 0 : w_lo[k] - s;
                e_hi[k] = w_hi[k] + s > (int)g.nc[k] - 1 ? (int)g.nc[k] - 1 : w_hi[k] + s;
            }
            const long long ey = e_hi[1] - e_lo[1] + 1;
            const long long npieces = 2ll * (e_hi[0] - e_lo[0] + 1) * ey;
            for (long long base = 0; base < npieces; base += 256) {
                const long long p = base + tid;
                uint32_t a = 0, b = 0;
                if (p < npieces) {
                    const long long row = p >> 1;
                    const int upper = (int)(p & 1);
                    const int x = e_lo[0] + (int)(row / ey), y = e_lo[1] + (int)(row % ey);
                    const bool inside = s > 0 && x >= p_lo[0] && x <= p_hi[0] && y >= p_lo[1] && y <= p_hi[1];
                    int z0 = 0, z1 = -1;
                    if (!inside) {
                        if (!upper) z0 = e_lo[2], z1 = e_hi[2];
                    } else if (!upper) {
                        z0 = e_lo[2], z1 = p_lo[2] - 1;
                    } else {
                        z0 = p_hi[2] + 1, z1 = e_hi[2];
                    }
                    if (z0 <= z1) {
                        a = pe_lower(rkeys, 0u, (uint32_t)R, pe_key(g, x, y, z0));
                        b = pe_upper(rkeys, a, (uint32_t)R, pe_key(g, x, y, z1));
                    }
                }
                uint32_t total;
                const uint32_t off = pe_block_scan(b - a, s_wave, total);
                s_a[tid] = a;
                s_off[tid] = off;
                __syncthreads();
                for (uint32_t ws = 0; ws < total; ws += kPeStage) {
#pragma unroll
                    for (int h = 0; h < kPeStage / 256; h++) {
                        const uint32_t k = (uint32_t)(h * 256 + tid), gi = ws + k;
                        if (gi < total) {
                            int lo = 0, hi = 255;  // the last piece with s_off <= gi: the one that holds it
                            while (lo < hi) {
                                const int mid = (lo + hi + 1) >> 1;
                                if (s_off[mid] <= gi) lo = mid;
                                else hi = mid - 1;
                            }
                            const size_t j = (size_t)s_a[lo] + (gi - s_off[lo]);
                            s_x[k] = rx[j], s_y[k] = ry[j], s_z[k] = rz[j];
                            if constexpr (kIndex) s_p.v[k] = rorder[j];
                        }
                    }
                    __syncthreads();
                    if (!done) {
                        const int n = (int)(total - ws < (uint32_t)kPeStage ? total - ws : (uint32_t)kPeStage);
                        for (int j = 0; j < n; j++) {
                            const double dx = q[0] - s_x[j], dy = q[1] - s_y[j], dz = q[2] - s_z[j];
                            const double d2 = dx * dx + dy * dy + dz * dz;
                            if constexpr (kIndex) {
                                if (d2 <= best) {  // rare after the first few candidates: the position is read here only
                                    const uint32_t pos = s_p.v[j];
                                    if (d2 < best || pos < best_pos) best = d2, best_pos = pos;
                                }
                            } else {
                                if (d2 < best) best = d2;
                            }
                        }
                    }
                    __syncthreads();
                }
            }
            // what is left lies behind a face of the grown box that still has cells behind it
            double lb = HUGE_VAL;
            bool covered = true;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                if (e_lo[k] > 0) {
                    covered = false;
                    lb = fmin(lb, q[k] - (g.mn[k] + (double)e_lo[k] * g.cs));
                }
                if (e_hi[k] < (int)g.nc[k] - 1) {
                    covered = false;
                    lb = fmin(lb, (g.mn[k] + (double)(e_hi[k] + 1) * g.cs) - q[k]);
                }
            }
            if (covered) break;  // the same for every lane
            // (a point behind such a face is strictly farther than lb, so a tie with best is never left behind)
            lb -= g.cs / 1048576.0;
            if (lb > 0.0 && (lb * lb >= best || lb > max_dist)) done = true;
            if (!__syncthreads_or(!done)) break;
#pragma unroll
            for (int k = 0; k < 3; k++) p_lo[k] = e_lo[k], p_hi[k] = e_hi[k];
        }
    }
    if (valid) {
        const double d = sqrt(best);
        out[src] = d < max_dist ? d : HUGE_VAL;
        if constexpr (kIndex) out_idx[src] = d < max_dist ? (long long)best_pos : -1ll;
    }
}

}  // namespace gsr
