// gsr_wave.h — the wave64 and workgroup primitives of the HIP kernels: butterfly reductions, the
// inclusive wave scan, the block scan and bounding-box reduction built on them, and the DPP
// forms.  Depends on the HIP runtime only.
//
// Contracts of the block primitives (restated on the host in tests/test_wave_ref.py):
//   - every lane of the workgroup calls them (each holds one barrier);
//   - a scan is exclusive, in thread order, modulo 2^32; its total includes every lane;
//   - the scratch is read after that one barrier and there is none behind it: a caller that
//     writes the scratch again (a second call, a loop) places its own __syncthreads() first.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace gsr {

// --------------------------------------------------------------------------
// wave64 helpers
// --------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ T lane_min(T a, T b) {
    if constexpr (std::is_floating_point<T>::value) return fmin(a, b);
    else return a < b ? a : b;
}
template <class T>
__device__ __forceinline__ T lane_max(T a, T b) {
    if constexpr (std::is_floating_point<T>::value) return fmax(a, b);
    else return a > b ? a : b;
}

// Butterfly reductions over the 64 lanes of a wave, result in every lane.  The partners are
// l ^ 32, l ^ 16, ..., l ^ 1 in that order: the association of a floating-point sum is part of
// the callers' contracts.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = lane_max(v, __shfl_xor(v, o, 64));
    return v;
}
template <class T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = lane_min(v, __shfl_xor(v, o, 64));
    return v;
}

// inclusive prefix sum over the lanes of a wave (lane 63 holds the wave's total)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

// --------------------------------------------------------------------------
// workgroup helpers (the contracts at the top of the file)
// --------------------------------------------------------------------------
// Exclusive scan of one value per lane over the first WAVES waves of the block (the block has at
// least that many; a lane of a later wave writes nothing and gets the total); *total, where asked
// for, = the sum over those waves.  s_w: WAVES words.
template <int WAVES>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_w, uint32_t* total = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t x = wave_incl_scan(v);
    if (lane == 63 && wave < WAVES) s_w[wave] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        const uint32_t t = s_w[w];
        before += w < wave ? t : 0u;
        all += t;
    }
    if (total) *total = all;
    return before + x - v;
}

// min of v[0..2] and max of v[3..5] over a 256-lane block, in every lane (min and max are exact,
// so the order of the reduction does not matter)
template <class T>
__device__ __forceinline__ void block_minmax6(T (&v)[6], T (*s)[6]) {
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = k < 3 ? wave_min(v[k]) : wave_max(v[k]);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; k++) s[wave][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const T a = s[0][k], b = s[1][k], c = s[2][k], d = s[3][k];
        v[k] = k < 3 ? lane_min(lane_min(a, b), lane_min(c, d)) : lane_max(lane_max(a, b), lane_max(c, d));
    }
}

// DPP lane moves (VOP_DPP, folded into the consuming v_add by the compiler):
// quad_perm xor 1 / xor 2 within quads, row_half_mirror (l ^ 7 within 8
// lanes) and row_mirror (l ^ 15 within a 16-lane row).  No LDS traffic,
// unlike __shfl_xor (ds_bpermute_b32).
enum : int { kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppRowMirror = 0x140, kDppRowHalfMirror = 0x141 };
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// a_l + a_{l ^ 16} and a_l + a_{l ^ 32} through gfx950's permlane swaps
__device__ __forceinline__ float add_lane_xor16(float a) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(a), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float add_lane_xor32(float a) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(a), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// OR over the 64 lanes of a wave, result in every lane; VALU only (as wave_sum_dpp)
__device__ __forceinline__ uint32_t wave_or_dpp(uint32_t v) {
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kDppRowMirror, 0xF, 0xF, false);
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kDppRowHalfMirror, 0xF, 0xF, false);
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kDppXor2, 0xF, 0xF, false);
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kDppXor1, 0xF, 0xF, false);
    auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    v = r[0] | r[1];
    r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return r[0] | r[1];
}

// Sum over the 64 lanes of a wave, result in every lane; VALU only.  Within
// a 16-lane row the partners are l^15, l^7 (mirrors: each stage pairs the two
// halves of a group bijectively, so each lane is counted once), then l^2, l^1.
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v += dpp_mov<kDppRowMirror>(v);
    v += dpp_mov<kDppRowHalfMirror>(v);
    v += dpp_mov<kDppXor2>(v);
    v += dpp_mov<kDppXor1>(v);
    return add_lane_xor32(add_lane_xor16(v));
}

// Transposed butterfly reduction of 16 per-lane values over the 64 lanes of
// a wave.  Stage 1/2 use gfx950's v_permlane32_swap / v_permlane16_swap (one
// swap moves half of a pair across the 32- or 16-lane boundary, so each stage
// halves the number of live values); stages 3/4 pair the halves of 16- and
// 8-lane groups with DPP mirrors (keep/send select: field bit 1 <- lane bit 3,
// field bit 0 <- lane bit 2); the last two stages are DPP quad adds.  On
// return lane l (all four lanes of each quad) holds the full wave sum of field
// (l >> 2); every cross-lane move is a VALU op.
__device__ inline float wave_transpose_reduce16(const float (&v)[16]) {
    const int lane = threadIdx.x & 63;
    float a[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[i]), __float_as_uint(v[i + 8]), false, false);
        a[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    // lanes 0..31 hold fields 0..7, lanes 32..63 fields 8..15 (sums over l, l^32)
    float b[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a[i]), __float_as_uint(a[i + 4]), false, false);
        b[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    // field bit 1 <- lane bit 3 (partner l ^ 15: opposite bit 3, same row)
    const bool hi8 = (lane & 8) != 0;
    float c[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const float keep = hi8 ? b[i + 2] : b[i];
        const float send = hi8 ? b[i] : b[i + 2];
        c[i] = keep + dpp_mov<kDppRowMirror>(send);
    }
    // field bit 0 <- lane bit 2 (partner l ^ 7: opposite bit 2, same 8 lanes)
    const bool hi4 = (lane & 4) != 0;
    const float keep = hi4 ? c[1] : c[0];
    const float send = hi4 ? c[0] : c[1];
    float d = keep + dpp_mov<kDppRowHalfMirror>(send);
    d += dpp_mov<kDppXor2>(d);
    d += dpp_mov<kDppXor1>(d);
    return d;
}

// The tile of a 256-point chunk: the last t in [0, n) with off[t] <= chunk
// (off non-decreasing, off[0] = 0), searched 64-wide — each lane tests one of
// 64 evenly spaced candidates and the ballot narrows the span 64-fold — so
// 8160 tiles take 3 dependent loads, against 13 for a binary search (the
// chain sat in front of every SAMPLE workgroup's first batch).  Call with
// every lane of the wave active; the result is wave-uniform.
__device__ inline uint32_t wave_find_chunk_tile(const uint32_t* __restrict__ off, uint32_t n, uint32_t chunk) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t lo = 0, span = n;
    while (span > 1) {
        const uint32_t step = (span + 63u) >> 6;
        const uint32_t t = lo + lane * step;
        const bool ok = lane == 0u || (t < lo + span && off[t] <= chunk);
        const unsigned long long b = __ballot(ok);
        const uint32_t L = 63u - (uint32_t)__builtin_clzll(b);
        const uint32_t end = lo + span;
        lo += L * step;
        span = min(step, end - lo);
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

}  // namespace gsr
