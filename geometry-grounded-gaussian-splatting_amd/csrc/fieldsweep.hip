// fieldsweep.hip — what the tetrahedral extraction sweep does around `integrate` (the reference's
// mesh_extract_tetrahedra.py:44-87 and :155-163), as three bandwidth-bound kernels on gfx950:
//
//   field_view_update_kernel  one view's `integrate` outputs folded into the running state of a chunk of
//                             points: ok = inside and, where the view has a mask, the bilinear sample of
//                             the mask at the point's projection > 0.5; seen |= ok; weight = ok ?
//                             min(alpha, weight) : weight.  One point per lane, no atomics.  A point with
//                             `inside` clear costs its one byte of `inside`: nothing else of it is read,
//                             so a point at or behind the near plane never reaches the division.
//   field_finish_kernel       sdf = 0.5 - (seen ? weight : 0), valid = seen, at the end of a chunk.
//   field_bisect_kernel       one bisection step over the crossing edges, in place: the midpoint replaces
//                             the left end when its sdf has the left end's sign, the right end otherwise
//                             (so a midpoint whose sdf is exactly 0 replaces the right end), and the next
//                             midpoint is written.  One edge per lane: the three lanes of a
//                             lane-per-component layout would race on the edge's left_sdf.
//
// The contract and the operation order are DESIGN §6k; tests/fieldsweep_ref.py restates them in numpy
// float32 and the two agree bit for bit, so every expression below keeps its parentheses and the file is
// built with floating-point contraction off (as meshraster.hip, §6j).
#pragma clang fp contract(off)

#include <math.h>

#include "gsr_kernels.h"

// A/B: 1 stages a block's 3 KB of points through LDS with whole-row loads instead of
// three dword loads per lane at a 12-byte stride.
#ifndef GSR_FIELD_STAGE_POINTS
#define GSR_FIELD_STAGE_POINTS 0
#endif

namespace gsr {

namespace {

// one bilinear tap of grid_sample's zeros padding: a texel outside the plane adds nothing
__device__ __forceinline__ float tap(const float* __restrict__ mask, const FieldView& v, float fx, float fy,
                                     float w, float acc) {
    if (!(fx >= 0.f && fx <= (float)(v.W - 1) && fy >= 0.f && fy <= (float)(v.H - 1))) return acc;
    return acc + mask[(size_t)(int)fy * (size_t)v.W + (size_t)(int)fx] * w;
}

// mesh_extract_tetrahedra.py:48-61 for one point: the mask's bilinear sample at the projection > 0.5
__device__ __forceinline__ bool on_mask(const FieldView& v, const float* __restrict__ mask, float x, float y,
                                        float z) {
    const float cx = ((x * v.r[0] + y * v.r[3]) + z * v.r[6]) + v.t[0];
    const float cy = ((x * v.r[1] + y * v.r[4]) + z * v.r[7]) + v.t[1];
    const float cz = ((x * v.r[2] + y * v.r[5]) + z * v.r[8]) + v.t[2];
    const float gx = v.c[0] + v.s[0] * (cx / cz), gy = v.c[1] + v.s[1] * (cy / cz);
    // align_corners: -1 and +1 are the centres of the first and last texel
    const float ix = ((gx + 1.f) * 0.5f) * (float)(v.W - 1), iy = ((gy + 1.f) * 0.5f) * (float)(v.H - 1);
    const float x0 = floorf(ix), y0 = floorf(iy), x1 = x0 + 1.f, y1 = y0 + 1.f;
    const float tx = ix - x0, ty = iy - y0, sx = x1 - ix, sy = y1 - iy;
    float acc = 0.f;
    acc = tap(mask, v, x0, y0, sx * sy, acc);
    acc = tap(mask, v, x1, y0, tx * sy, acc);
    acc = tap(mask, v, x0, y1, sx * ty, acc);
    acc = tap(mask, v, x1, y1, tx * ty, acc);
    return acc > 0.5f;
}

template <bool kMask>
__global__ void __launch_bounds__(256) field_view_update_kernel(FieldView v, long long N,
                                                                const float* __restrict__ points,
                                                                const float* __restrict__ alpha,
                                                                const uint8_t* __restrict__ inside,
                                                                const float* __restrict__ mask,
                                                                float* __restrict__ weight,
                                                                uint8_t* __restrict__ seen) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool ok = i < N && inside[i] != 0;
    if (kMask) {
#if GSR_FIELD_STAGE_POINTS
        __shared__ float stage[768];
        if (__syncthreads_or(ok)) {  // (block-uniform)
            const long long base = (long long)blockIdx.x * 768;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int w = threadIdx.x + 256 * k;
                if (base + w < 3 * N) stage[w] = points[base + w];
            }
            __syncthreads();
            const float* p = stage + 3 * threadIdx.x;
            if (ok) ok = on_mask(v, mask, p[0], p[1], p[2]);
        }
#else
        if (ok) ok = on_mask(v, mask, points[3 * i], points[3 * i + 1], points[3 * i + 2]);
#endif
    }
    if (!ok) return;
    seen[i] = 1;
    // torch.where(ok, torch.min(alpha, weight), weight): only a smaller (or NaN) alpha changes the word
    const float a = alpha[i];
    if (a < weight[i] || a != a) weight[i] = a;
}

// `valid` may be `seen` and `sdf` may be `weight`: a lane reads its own elements before it writes them
__global__ void __launch_bounds__(256) field_finish_kernel(long long N, const float* weight, const uint8_t* seen,
                                                           float* sdf, uint8_t* valid) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const bool s = seen[i] != 0;
    const float w = s ? weight[i] : 0.f;
    sdf[i] = 0.5f - w;
    valid[i] = s ? 1 : 0;
}

// mesh_extract_tetrahedra.py:155-163 for one edge
template <class T>
__global__ void __launch_bounds__(256) field_bisect_kernel(long long E, T* __restrict__ left, T* __restrict__ right,
                                                           float* __restrict__ left_sdf,
                                                           float* __restrict__ right_sdf,
                                                           const float* __restrict__ mid_sdf,
                                                           T* __restrict__ mid) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const float m = mid_sdf[e], l = left_sdf[e];
    const bool low = (m < 0.f && l < 0.f) || (m > 0.f && l > 0.f);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        T a = left[3 * e + k], b = right[3 * e + k];
        const T p = (a + b) * (T)0.5;  // the point mid_sdf was queried at
        if (low) left[3 * e + k] = a = p;
        else right[3 * e + k] = b = p;
        mid[3 * e + k] = (a + b) * (T)0.5;
    }
    if (low) left_sdf[e] = m;
    else right_sdf[e] = m;
}

inline dim3 field_grid(long long n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

hipError_t launch_field_view_update(const FieldView& v, long long N, const float* points, const float* alpha,
                                    const uint8_t* inside, const float* mask, float* weight, uint8_t* seen,
                                    hipStream_t stream) {
    if (mask)
        hipLaunchKernelGGL(field_view_update_kernel<true>, field_grid(N), dim3(256), 0, stream, v, N, points, alpha,
                           inside, mask, weight, seen);
    else
        hipLaunchKernelGGL(field_view_update_kernel<false>, field_grid(N), dim3(256), 0, stream, v, N, points, alpha,
                           inside, mask, weight, seen);
    return hipGetLastError();
}

hipError_t launch_field_finish(long long N, const float* weight, const uint8_t* seen, float* sdf, uint8_t* valid,
                               hipStream_t stream) {
    hipLaunchKernelGGL(field_finish_kernel, field_grid(N), dim3(256), 0, stream, N, weight, seen, sdf, valid);
    return hipGetLastError();
}

hipError_t launch_field_bisect(long long E, void* left, void* right, bool f64, float* left_sdf, float* right_sdf,
                               const float* mid_sdf, void* mid, hipStream_t stream) {
    if (f64)
        hipLaunchKernelGGL(field_bisect_kernel<double>, field_grid(E), dim3(256), 0, stream, E, (double*)left,
                           (double*)right, left_sdf, right_sdf, mid_sdf, (double*)mid);
    else
        hipLaunchKernelGGL(field_bisect_kernel<float>, field_grid(E), dim3(256), 0, stream, E, (float*)left,
                           (float*)right, left_sdf, right_sdf, mid_sdf, (float*)mid);
    return hipGetLastError();
}

}  // namespace gsr
