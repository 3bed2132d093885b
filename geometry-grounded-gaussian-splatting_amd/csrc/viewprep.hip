// viewprep.hip — from a decoded image to what a training view keeps, on gfx950 (the reference's loadCam ->
// PILtoTorch -> Camera.__init__, utils/camera_utils.py:22-66, scene/cameras.py:44-62): Pillow's 8-bit bicubic
// resize and the float planes of the resized bytes.
//
// The contract is the byte.  Training does not see "a bicubic downscale" but Pillow's resample:
// per axis a table of windows whose float64 bicubic weights (a = -0.5, support 2 x max(scale, 1)) are
// normalised to sum 1 and rounded to 22 fractional bits, each output byte
//   clip8((2^21 + sum pixel * k) >> 22)      in int32 (255 * sum |k| < 2^31 for this filter),
// the horizontal pass first, its result rounded to bytes, then the vertical pass.  Integer sums are exact in
// any order, so the kernels below may split a window as they like; the table itself is float64 on the host
// and this file is compiled with -ffp-contract=off (Makefile): no a * b + c of resample_coeffs or of the
// gray plane is contracted.
//
// Tables on the device are tap-major, k[t * out_size + xx]: lanes of the horizontal pass hold consecutive xx.
//
// resample_rows_kernel (horizontal): rows are independent, so the batch is N * H rows.  One workgroup = 4 rows
// (one per wave) x 64 output pixels.  The input pixels under the tile's windows are staged in LDS in chunks
// of 1008 + 16 bytes per row, 16 bytes per lane from 16-byte aligned addresses (a row of 5187 RGB pixels
// starts anywhere), and every lane adds the taps of its window that begin in the chunk: the window width
// grows with the scale factor (83 taps at 20.5x) and no size of it is assumed — a tile whose windows span
// more than a chunk loops.  At 5187 -> 1600 the span of a tile is 0.7 KB: one chunk.
// resample_cols_kernel (vertical): a column of bytes is independent of its neighbours whatever C is, so a
// row is W * C bytes and a lane owns four consecutive bytes of one output row; the taps are whole rows
// apart, each a coalesced dword per lane (rows that are no multiple of four bytes: byte loads), and the
// weights of the output row are wave-uniform.
// view_planes_kernel: [N,H,W,3] bytes (and [N,H,W] mask bytes) -> original_image [N,3,H,W] = byte / 255 (an
// IEEE divide), gray_image [N,1,H,W] = (0.299f r + 0.587f g) + 0.114f b with every product and sum rounded,
// gt_mask [N,1,H,W] = mask byte / 255, one launch.
// No atomics, no reduction: an image's bytes do not depend on its batch.
#include <math.h>

#include <vector>

#include "gsr_kernels.h"

namespace gsr {

constexpr int kResampleBits = 32 - 8 - 2;  // Pillow's PRECISION_BITS
constexpr int kRowsTX = 64, kRowsTY = 4;   // the horizontal tile: output pixels x rows (one wave per row)
constexpr int kRowsStride = 1008;          // chunk stride in bytes; 16 more are staged so a pixel never straddles

// ---- the coefficient table (host, float64) -----------------------------------------------------------------------

static double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

int resample_ksize(int in_size, int out_size) {
    double filterscale = (double)in_size / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(2.0 * filterscale) * 2 + 1;
}

// k [out_size][ksize] (zero past a window's count), bounds [out_size][2] = (xmin, count): Pillow's
// precompute_coeffs and normalize_coeffs_8bpc for the bicubic filter, statement by statement.
void resample_coeffs(int in_size, int out_size, int32_t* k, int32_t* bounds) {
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    const double ss = 1.0 / filterscale;
    std::vector<double> w(ksize);
    for (int xx = 0; xx < out_size; xx++) {
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < xmax; x++) {
            w[x] = bicubic_filter((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int32_t* kk = k + (size_t)xx * ksize;
        for (int x = 0; x < ksize; x++) {
            if (x >= xmax) {
                kk[x] = 0;
                continue;
            }
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            kk[x] = v < 0 ? (int32_t)(-0.5 + v * (1 << kResampleBits)) : (int32_t)(0.5 + v * (1 << kResampleBits));
        }
        bounds[2 * xx + 0] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

// ---- kernels ------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint8_t clip8(int acc) {
    const int v = acc >> kResampleBits;  // arithmetic shift, as Pillow's table lookup of in >> PRECISION_BITS
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// in [rows][in_w][C] -> out [rows][out_w][C].  [lo, hi): the bytes of `in` (a lane never reads outside them).
template <int C>
__global__ void __launch_bounds__(kRowsTX* kRowsTY)
    resample_rows_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, long long rows, int in_w,
                         int out_w, const int32_t* __restrict__ k, const int32_t* __restrict__ bounds) {
    __shared__ __attribute__((aligned(16))) uint8_t s_px[kRowsTY][kRowsStride + 16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * kRowsTY + wave;
    const int x0 = blockIdx.y * kRowsTX;
    const int x1 = min(x0 + kRowsTX, out_w) - 1;  // the tile's last output pixel
    // the windows of a tile: xmin and xmin + count do not decrease with xx
    const int xstart = bounds[2 * x0], xend = bounds[2 * x1] + bounds[2 * x1 + 1];
    const bool live_row = row < rows;
    const uintptr_t lo = (uintptr_t)in, hi = lo + (size_t)rows * in_w * C;
    const uintptr_t g0 = lo + ((size_t)(live_row ? row : 0) * in_w + xstart) * C;  // first byte under the tile
    const uintptr_t a0 = g0 & ~(uintptr_t)15;
    const int sh = (int)(g0 - a0);
    const int chunks = ((xend - xstart) * C + 15 + kRowsStride - 1) / kRowsStride;  // (the same for all four rows)

    const int xx = x0 + lane;
    const bool live = live_row && xx <= x1;
    const int xmin = live ? bounds[2 * xx] : xstart, count = live ? bounds[2 * xx + 1] : 0;
    const int first = (xmin - xstart) * C + sh;  // offset of the window's first byte from a0
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 1 << (kResampleBits - 1);

    for (int ch = 0; ch < chunks; ch++) {
        if (ch) __syncthreads();  // every lane is done with the chunk before
        if (live_row) {
            // this lane's 16 bytes of the chunk [a0 + ch * stride, + stride + 16)
            const uintptr_t a = a0 + (size_t)ch * kRowsStride + 16 * lane;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (a >= lo && a + 16 <= hi) {
                v = *reinterpret_cast<const uint4*>(a);
            } else if (a + 16 > lo && a < hi) {  // the ends of the tensor: byte by byte, inside it only
                uint32_t d[4] = {0, 0, 0, 0};
#pragma unroll
                for (int j = 0; j < 16; j++)
                    if (a + j >= lo && a + j < hi)
                        d[j >> 2] |= (uint32_t)*reinterpret_cast<const uint8_t*>(a + j) << (8 * (j & 3));
                v = make_uint4(d[0], d[1], d[2], d[3]);
            }
            *reinterpret_cast<uint4*>(&s_px[wave][16 * lane]) = v;
        }
        __syncthreads();
        // the taps whose first byte lies in [ch * stride, (ch + 1) * stride) of the row's staged bytes
        const int b0 = ch * kRowsStride - first, b1 = b0 + kRowsStride;  // in bytes from the window's start
        const int t0 = b0 <= 0 ? 0 : (b0 + C - 1) / C;
        const int t1 = b1 <= 0 ? 0 : min(count, (b1 + C - 1) / C);
        for (int t = t0; t < t1; t++) {
            const int w = k[(size_t)t * out_w + xx];
            const uint8_t* p = &s_px[wave][first + t * C - ch * kRowsStride];
#pragma unroll
            for (int c = 0; c < C; c++) acc[c] += (int)p[c] * w;
        }
    }
    if (live) {
        uint8_t* o = out + ((size_t)row * out_w + xx) * C;
#pragma unroll
        for (int c = 0; c < C; c++) o[c] = clip8(acc[c]);
    }
}

// in [N][in_h][row_bytes] -> out [N][out_h][row_bytes]; blockIdx.x = n * out_h + yy, a lane owns bytes
// [4 j, 4 j + 4) of the row.  ALIGNED: every row of `in` and `out` starts on a dword.
template <bool ALIGNED>
__global__ void __launch_bounds__(256)
    resample_cols_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int in_h, int out_h,
                         long long row_bytes, const int32_t* __restrict__ k,
                         const int32_t* __restrict__ bounds) {
    const long long n = blockIdx.x / out_h;
    const int yy = (int)(blockIdx.x - n * out_h);
    const long long col = 4 * ((long long)blockIdx.y * 256 + threadIdx.x);
    if (col >= row_bytes) return;
    const int ymin = bounds[2 * yy], count = bounds[2 * yy + 1];
    const int live = row_bytes - col < 4 ? (int)(row_bytes - col) : 4;  // (4 when ALIGNED)
    const uint8_t* src = in + ((size_t)n * in_h + ymin) * row_bytes + col;
    int acc[4];
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = 1 << (kResampleBits - 1);
    for (int t = 0; t < count; t++, src += row_bytes) {
        const int w = k[(size_t)t * out_h + yy];
        uint32_t v = 0;
        if (ALIGNED) {
            v = *reinterpret_cast<const uint32_t*>(src);
        } else {
            for (int j = 0; j < live; j++) v |= (uint32_t)src[j] << (8 * j);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j] += (int)((v >> (8 * j)) & 255u) * w;
    }
    uint8_t* dst = out + ((size_t)n * out_h + yy) * row_bytes + col;
    if (ALIGNED) {
        *reinterpret_cast<uint32_t*>(dst) = (uint32_t)clip8(acc[0]) | (uint32_t)clip8(acc[1]) << 8 |
                                            (uint32_t)clip8(acc[2]) << 16 | (uint32_t)clip8(acc[3]) << 24;
    } else {
        for (int j = 0; j < live; j++) dst[j] = clip8(acc[j]);
    }
}

// one lane per pixel of the batch
__global__ void __launch_bounds__(256)
    view_planes_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ mask, size_t HW, size_t total,
                       float* __restrict__ original, float* __restrict__ gray, float* __restrict__ gt_mask) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const size_t n = g / HW, p = g - n * HW;
    // PILtoTorch: byte / 255.0 in float32, correctly rounded (a divide, not a reciprocal multiply)
    const float r = (float)rgb[3 * g + 0] / 255.0f;
    const float gr = (float)rgb[3 * g + 1] / 255.0f;
    const float b = (float)rgb[3 * g + 2] / 255.0f;
    float* o = original + 3 * n * HW + p;
    o[0] = r;
    o[HW] = gr;
    o[2 * HW] = b;
    // cameras.py:45, left to right; the products and sums are separate statements (no fma: see the head)
    const float t0 = 0.299f * r;
    const float t1 = 0.587f * gr;
    const float t2 = 0.114f * b;
    const float s = t0 + t1;
    gray[g] = s + t2;
    if (mask) gt_mask[g] = (float)mask[g] / 255.0f;
}

// ---- host ---------------------------------------------------------------------------------------------------------

hipError_t launch_image_resample8(long long N, int H, int W, int C, int axis, int out_size, const uint8_t* in,
                                  uint8_t* out, const int32_t* k, const int32_t* bounds, hipStream_t stream) {
    if (axis == 1) {  // along W
        const long long rows = N * H;
        const dim3 grid((unsigned)((rows + kRowsTY - 1) / kRowsTY), (unsigned)((out_size + kRowsTX - 1) / kRowsTX));
        const dim3 block(kRowsTX * kRowsTY);
        switch (C) {
            case 1: hipLaunchKernelGGL(resample_rows_kernel<1>, grid, block, 0, stream, in, out, rows, W, out_size, k, bounds); break;
            case 2: hipLaunchKernelGGL(resample_rows_kernel<2>, grid, block, 0, stream, in, out, rows, W, out_size, k, bounds); break;
            case 3: hipLaunchKernelGGL(resample_rows_kernel<3>, grid, block, 0, stream, in, out, rows, W, out_size, k, bounds); break;
            default: hipLaunchKernelGGL(resample_rows_kernel<4>, grid, block, 0, stream, in, out, rows, W, out_size, k, bounds); break;
        }
        return hipGetLastError();
    }
    const long long row_bytes = (long long)W * C;
    const dim3 grid((unsigned)(N * out_size), (unsigned)((row_bytes + 1023) / 1024));
    const bool aligned = row_bytes % 4 == 0 && ((uintptr_t)in & 3) == 0 && ((uintptr_t)out & 3) == 0;
    if (aligned)
        hipLaunchKernelGGL(resample_cols_kernel<true>, grid, dim3(256), 0, stream, in, out, H, out_size, row_bytes, k,
                           bounds);
    else
        hipLaunchKernelGGL(resample_cols_kernel<false>, grid, dim3(256), 0, stream, in, out, H, out_size, row_bytes,
                           k, bounds);
    return hipGetLastError();
}

hipError_t launch_view_planes(long long N, int H, int W, const uint8_t* rgb, const uint8_t* mask, float* original,
                              float* gray, float* gt_mask, hipStream_t stream) {
    const size_t HW = (size_t)H * W, total = (size_t)N * HW;
    hipLaunchKernelGGL(view_planes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, rgb, mask, HW,
                       total, original, gray, gt_mask);
    return hipGetLastError();
}

}  // namespace gsr
