// imgmetric.hip — the image-quality tail on gfx950 (the reference's render.py -> metric.py, and the
// in-training report of train.py:332-365): 8-bit quantisation, L1, MSE (PSNR on the host) and the per-image
// "valid" SSIM of a batch of image pairs, in one pass over the floats.
//
// The contract.  metric.py does not score the float render: it scores what survives
// torchvision's save_image -> PNG -> to_tensor,
//   byte = trunc(clamp(fl(fl(x * 255) + 0.5), 0, 255)),   value = fl(byte / 255),
// the multiply and the add rounded separately in fp32 (torch's mul(255).add_(0.5).clamp_(0, 255).to(uint8);
// NaN -> 0, +inf -> 255, -inf -> 0).  A fused multiply-add lands on another byte for a few values in a
// million, so this file is compiled with -ffp-contract=off (Makefile): no a * b + c below is contracted.
//
// image_metrics_kernel: one 256-lane workgroup per 32 x 16 tile of SSIM window positions of one image, the
// channels in a loop.  Per channel the (32+10) x (16+10) pixels under the tile's windows are read from both
// images, converted (quantised to byte / 255, or clamped to [0, 1]) and staged in LDS as fp32; the horizontal
// and vertical 11-tap passes have the shape of ssim.hip's (restated, as photoloss.hip does; the window is
// ssim.hip's) but run in float64: a reported metric is held to the float64 value of the reference's expression,
// and the fp32 moments of a lone 11 x 11 window (E[x^2] - mu^2 cancels) miss it by a few 1e-7.
// The tiles partition the image: a tile owns the 32 x 16 pixels at the top left of what it stages, and the
// last tile of a row or column owns the up to 10 left over, so every pixel is summed (and its byte written)
// by exactly one workgroup while it is staged.  Quantised sums are exact integers: 32-bit per workgroup and
// channel (at most 42 * 26 * 255^2 < 2^27), 64-bit from there on.  Float sums are float64, per wave by
// xor-shuffle, the four waves in a fixed order.  The byte images leave through LDS as dword stores.
// Without SSIM the same body runs with no halo (32 x 16 staged).
// image_metrics_finish_kernel: one 1024-lane workgroup per image sums that image's partials in a fixed order
// and writes {l1, mse, ssim} as float64: an image's numbers do not depend on the rest of the batch.
// image_quantize8_kernel: [N,C,H,W] fp32 -> [N,H,W,C] bytes, one dword of four interleaved bytes per lane.
#include "gsr_kernels.h"

namespace gsr {

// the window and tile of ssim.hip (which stays as it is: the same definitions, restated)
constexpr int kImR = 5;
constexpr int kImTW = 32, kImTH = 16;
constexpr double kImC1 = 0.01 * 0.01, kImC2 = 0.03 * 0.03;
constexpr int kImMaxByteC = 4;  // channels of a byte image written by image_metrics (a PNG has at most 4)

struct SsimWindow {
    float w[2 * kImR + 1];
};
SsimWindow ssim_window();  // ssim.hip

// save_image's byte: the two roundings are separate statements and the file is built without contraction
__device__ __forceinline__ unsigned quantize8(float x) {
    float t = x * 255.0f;
    t = t + 0.5f;
    if (!(t > 0.f)) return 0u;  // negatives, -inf and NaN (torch's uint8 cast of NaN gives 0)
    if (t >= 255.f) return 255u;
    return (unsigned)t;  // truncation toward zero
}

// torch.clamp(x, 0, 1): NaN stays NaN
__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

struct ImageMetricsParams {
    int C, H, W;
    const float* render;  // [N, C, H, W]
    const float* gt;
    uint8_t* render_bytes;  // [N, H, W, C] or NULL (BYTES instances only)
    uint8_t* gt_bytes;
    double* p_ssim;             // per (image, channel, tile): the SSIM sum of the tile's windows
    unsigned long long* p_s1;   // sum |a - b|: an integer (QUANT) or the bits of a double
    unsigned long long* p_s2;   // sum (a - b)^2
};

// the interleaved bytes of the rows this workgroup owns, from LDS: per row the segment [s, e) of the byte
// image is cut at dword boundaries; whole dwords go out as dword stores, the ragged ends as byte stores
template <int IH, int IW>
__device__ __forceinline__ void store_bytes(uint8_t* __restrict__ out, const uint8_t (*sq)[IH][IW], int C, int W,
                                            size_t image_base, int y0, int x0, int own_h, int own_w, int tid) {
    const int seg = own_w * C;       // bytes of one owned row
    const int slots = seg / 4 + 2;   // dwords a segment can touch
    for (int k = tid; k < own_h * slots; k += 256) {
        const int r = k / slots, slot = k - r * slots;
        const size_t s = image_base + ((size_t)(y0 + r) * W + x0) * C, e = s + seg;
        const size_t d = (s & ~(size_t)3) + 4 * (size_t)slot;  // this lane's dword, by byte address
        if (d >= e) continue;
        uint32_t word = 0;
        bool whole = true;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const size_t a = d + j;
            if (a < s || a >= e) {
                whole = false;
                continue;
            }
            const int off = (int)(a - s), x = off / C, c = off - x * C;
            word |= (uint32_t)sq[c][r][x] << (8 * j);
        }
        if (whole) {
            *reinterpret_cast<uint32_t*>(out + d) = word;  // (out is 4-byte aligned: checked by the caller)
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (d + j >= s && d + j < e) out[d + j] = (uint8_t)(word >> (8 * j));
        }
    }
}

template <bool SSIM, bool QUANT, bool BYTES>
__global__ void __launch_bounds__(256) image_metrics_kernel(ImageMetricsParams q, SsimWindow win) {
    constexpr int R = SSIM ? kImR : 0;
    constexpr int IW = kImTW + 2 * R, IH = kImTH + 2 * R;
    constexpr int HR = SSIM ? IH : 1, HC = SSIM ? kImTW : 1;
    constexpr int BC = BYTES ? kImMaxByteC : 1, BH = BYTES ? IH : 1, BW = BYTES ? IW : 1;
    __shared__ float s_x[IH][IW], s_y[IH][IW];
    __shared__ double s_h[5][HR][HC];
    __shared__ uint8_t s_qa[BC][BH][BW], s_qb[BC][BH][BW];
    __shared__ double s_red[4], s_d1[4], s_d2[4];
    __shared__ unsigned s_u1[4], s_u2[4];
    const int tid = threadIdx.x;
    const int H = q.H, W = q.W, C = q.C;
    // the tile's staged pixels start at (y0, x0): its windows are centred R further in
    const int x0 = blockIdx.x * kImTW, y0 = blockIdx.y * kImTH;
    const int own_w = blockIdx.x == gridDim.x - 1 ? W - x0 : kImTW;  // (<= IW: the grid covers W - 2R)
    const int own_h = blockIdx.y == gridDim.y - 1 ? H - y0 : kImTH;
    const size_t tiles = (size_t)gridDim.x * gridDim.y;
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;

    for (int ch = 0; ch < C; ch++) {
        const size_t plane = ((size_t)blockIdx.z * C + ch) * H * W;
        const float* X = q.render + plane;
        const float* Y = q.gt + plane;
        unsigned u1 = 0, u2 = 0;
        double d1 = 0.0, d2 = 0.0;
        for (int k = tid; k < IH * IW; k += 256) {
            const int r = k / IW, c = k - r * IW;
            const int y = y0 + r, x = x0 + c;
            float a = 0.f, b = 0.f;
            if (y < H && x < W) {
                const float xa = X[(size_t)y * W + x], xb = Y[(size_t)y * W + x];
                const bool own = r < own_h && c < own_w;
                if (QUANT) {
                    const unsigned qa = quantize8(xa), qb = quantize8(xb);
                    a = (float)qa / 255.0f;
                    b = (float)qb / 255.0f;
                    if (own) {
                        const unsigned d = qa > qb ? qa - qb : qb - qa;
                        u1 += d;
                        u2 += d * d;
                        if (BYTES) {
                            s_qa[ch][r][c] = (uint8_t)qa;
                            s_qb[ch][r][c] = (uint8_t)qb;
                        }
                    }
                } else {
                    a = clamp01(xa);
                    b = clamp01(xb);
                    if (own) {
                        const float d = a - b;
                        d1 += (double)fabsf(d);
                        d2 += (double)d * (double)d;
                    }
                }
            }
            if (SSIM) {
                s_x[r][c] = a;
                s_y[r][c] = b;
            }
        }
        double sum = 0.0;
        if (SSIM) {
            __syncthreads();
            // horizontal pass: 26 staged rows x 32 window columns, five moments
            for (int k = tid; k < IH * kImTW; k += 256) {
                const int r = k / kImTW, c = k - r * kImTW;
                double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int t = 0; t < 2 * kImR + 1; t++) {
                    const double a = s_x[r][c + t], b = s_y[r][c + t], w = win.w[t];
                    m[0] += w * a;
                    m[1] += w * b;
                    m[2] += w * (a * a);
                    m[3] += w * (b * b);
                    m[4] += w * (a * b);
                }
#pragma unroll
                for (int p = 0; p < 5; p++) s_h[p][r][c] = m[p];
            }
            __syncthreads();
            // vertical pass: lane -> column (tid % 32), rows tid / 32 and + 8
            const int c = tid & (kImTW - 1);
#pragma unroll
            for (int rr = 0; rr < 2; rr++) {
                const int r = (tid >> 5) + 8 * rr;
                double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int t = 0; t < 2 * kImR + 1; t++) {
                    const double w = win.w[t];
#pragma unroll
                    for (int p = 0; p < 5; p++) m[p] += w * s_h[p][r + t][c];
                }
                // the window centred at (y0 + r + R, x0 + c + R) lies inside the image
                if (y0 + r + 2 * kImR >= H || x0 + c + 2 * kImR >= W) continue;
                const double mu1 = m[0], mu2 = m[1];
                const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
                const double s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu12;
                const double num1 = 2.0 * mu12 + kImC1, num2 = 2.0 * s12 + kImC2;
                const double den1 = mu1_sq + mu2_sq + kImC1, den2 = s1 + s2 + kImC2;
                sum += (num1 * num2) / (den1 * den2);
            }
            sum = wave_sum(sum);
        }
        if (QUANT) {
            u1 = wave_sum(u1);
            u2 = wave_sum(u2);
        } else {
            d1 = wave_sum(d1);
            d2 = wave_sum(d2);
        }
        if ((tid & 63) == 0) {
            s_red[tid >> 6] = sum;
            s_u1[tid >> 6] = u1;
            s_u2[tid >> 6] = u2;
            s_d1[tid >> 6] = d1;
            s_d2[tid >> 6] = d2;
        }
        __syncthreads();  // (also: every lane is done with s_x, s_y, s_h before the next channel stages)
        if (tid == 0) {
            const size_t o = ((size_t)blockIdx.z * C + ch) * tiles + tile;
            if (SSIM) q.p_ssim[o] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
            if (QUANT) {
                q.p_s1[o] = (s_u1[0] + s_u1[1]) + (s_u1[2] + s_u1[3]);
                q.p_s2[o] = (s_u2[0] + s_u2[1]) + (s_u2[2] + s_u2[3]);
            } else {
                q.p_s1[o] = (unsigned long long)__double_as_longlong((s_d1[0] + s_d1[1]) + (s_d1[2] + s_d1[3]));
                q.p_s2[o] = (unsigned long long)__double_as_longlong((s_d2[0] + s_d2[1]) + (s_d2[2] + s_d2[3]));
            }
        }
        __syncthreads();  // the four-wave slots are free again
    }
    if (BYTES) {
        const size_t image_base = (size_t)blockIdx.z * H * W * C;
        if (q.render_bytes) store_bytes<BH, BW>(q.render_bytes, s_qa, C, W, image_base, y0, x0, own_h, own_w, tid);
        if (q.gt_bytes) store_bytes<BH, BW>(q.gt_bytes, s_qb, C, W, image_base, y0, x0, own_h, own_w, tid);
    }
}

// One workgroup per image: its partials (channels x tiles, contiguous) in a fixed order.  den1, den2: the
// divisors of the two sums (n and n, or 255 n and 65025 n); count: the windows of one image.
template <bool QUANT>
__global__ void __launch_bounds__(1024)
    image_metrics_finish_kernel(const double* __restrict__ p_ssim, const unsigned long long* __restrict__ p_s1,
                                const unsigned long long* __restrict__ p_s2, int per_image, int with_ssim,
                                double den1, double den2, double count, double* __restrict__ out) {
    __shared__ double s_s[16], s_1[16], s_2[16];
    __shared__ unsigned long long s_i1[16], s_i2[16];
    const size_t base = (size_t)blockIdx.x * per_image;
    double ss = 0.0, a1 = 0.0, a2 = 0.0;
    unsigned long long i1 = 0, i2 = 0;
    for (int k = threadIdx.x; k < per_image; k += 1024) {
        if (with_ssim) ss += p_ssim[base + k];
        if (QUANT) {
            i1 += p_s1[base + k];
            i2 += p_s2[base + k];
        } else {
            a1 += __longlong_as_double((long long)p_s1[base + k]);
            a2 += __longlong_as_double((long long)p_s2[base + k]);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ss = wave_sum(ss), a1 = wave_sum(a1), a2 = wave_sum(a2), i1 = wave_sum(i1), i2 = wave_sum(i2);
    if (lane == 0) {
        s_s[wave] = ss;
        s_1[wave] = a1;
        s_2[wave] = a2;
        s_i1[wave] = i1;
        s_i2[wave] = i2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double ts = 0.0, t1 = 0.0, t2 = 0.0;
        unsigned long long j1 = 0, j2 = 0;
        for (int w = 0; w < 16; w++) {
            ts += s_s[w];
            t1 += s_1[w];
            t2 += s_2[w];
            j1 += s_i1[w];
            j2 += s_i2[w];
        }
        double* o = out + 3 * (size_t)blockIdx.x;
        o[0] = (QUANT ? (double)j1 : t1) / den1;
        o[1] = (QUANT ? (double)j2 : t2) / den2;
        o[2] = with_ssim ? ts / count : 0.0;
    }
}

// [N, C, H, W] fp32 -> [N, H, W, C] bytes over the whole batch as one byte array: lane -> dword
__global__ void __launch_bounds__(256)
    image_quantize8_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, int C, size_t HW, size_t total) {
    const size_t g = 4 * ((size_t)blockIdx.x * 256 + threadIdx.x);  // first byte of this lane's dword
    if (g >= total) return;
    size_t pix = g / C;  // pixel over the batch
    int c = (int)(g - pix * C);
    size_t n = pix / HW, p = pix - n * HW;
    uint32_t word = 0;
    const int live = total - g < 4 ? (int)(total - g) : 4;
    for (int j = 0; j < live; j++) {
        word |= quantize8(in[(n * C + c) * HW + p]) << (8 * j);
        if (++c == C) {
            c = 0;
            if (++p == HW) {
                p = 0;
                n++;
            }
        }
    }
    if (live == 4) {
        *reinterpret_cast<uint32_t*>(out + g) = word;  // (out is 4-byte aligned: checked by the caller)
    } else {
        for (int j = 0; j < live; j++) out[g + j] = (uint8_t)(word >> (8 * j));
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------

static dim3 image_metrics_grid(int N, int H, int W, bool ssim) {
    const int R = ssim ? kImR : 0;
    return dim3((W - 2 * R + kImTW - 1) / kImTW, (H - 2 * R + kImTH - 1) / kImTH, N);
}

static size_t image_metrics_partials(int N, int C, int H, int W, int with_ssim) {
    const dim3 g = image_metrics_grid(N, H, W, with_ssim != 0);
    return (size_t)N * C * g.x * g.y;
}

size_t carve_image_metrics(void* base, int N, int C, int H, int W, int with_ssim, ImageMetricsState& st) {
    const size_t n = image_metrics_partials(N, C, H, W, with_ssim);
    char* p = (char*)base;
    size_t off = 0;
    st.p_s1 = (unsigned long long*)(p + off);
    off = align_up(off + n * sizeof(unsigned long long), 256);
    st.p_s2 = (unsigned long long*)(p + off);
    off = align_up(off + n * sizeof(unsigned long long), 256);
    st.p_ssim = (double*)(p + off);
    off = align_up(off + n * sizeof(double), 256);
    return off + 256;  // (room to align the base)
}

template <bool SSIM, bool QUANT>
static void launch_metrics_instance(dim3 grid, const ImageMetricsParams& q, hipStream_t stream) {
    if (QUANT && (q.render_bytes || q.gt_bytes))
        hipLaunchKernelGGL((image_metrics_kernel<SSIM, QUANT, QUANT>), grid, dim3(256), 0, stream, q, ssim_window());
    else
        hipLaunchKernelGGL((image_metrics_kernel<SSIM, QUANT, false>), grid, dim3(256), 0, stream, q, ssim_window());
}

hipError_t launch_image_metrics(int N, int C, int H, int W, int quantize, int with_ssim, const float* render,
                                const float* gt, uint8_t* render_bytes, uint8_t* gt_bytes,
                                const ImageMetricsState& st, double* out, hipStream_t stream) {
    const dim3 grid = image_metrics_grid(N, H, W, with_ssim != 0);
    const ImageMetricsParams q{C, H, W, render, gt, quantize ? render_bytes : nullptr, quantize ? gt_bytes : nullptr,
                               st.p_ssim, st.p_s1, st.p_s2};
    if (with_ssim && quantize) launch_metrics_instance<true, true>(grid, q, stream);
    else if (with_ssim) launch_metrics_instance<true, false>(grid, q, stream);
    else if (quantize) launch_metrics_instance<false, true>(grid, q, stream);
    else launch_metrics_instance<false, false>(grid, q, stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const double n = (double)C * H * W;
    const double count = with_ssim ? (double)C * (H - 2 * kImR) * (W - 2 * kImR) : 1.0;
    const int per_image = (int)((size_t)C * grid.x * grid.y);
    if (quantize)
        hipLaunchKernelGGL(image_metrics_finish_kernel<true>, dim3(N), dim3(1024), 0, stream, st.p_ssim, st.p_s1,
                           st.p_s2, per_image, with_ssim, 255.0 * n, 65025.0 * n, count, out);
    else
        hipLaunchKernelGGL(image_metrics_finish_kernel<false>, dim3(N), dim3(1024), 0, stream, st.p_ssim, st.p_s1,
                           st.p_s2, per_image, with_ssim, n, n, count, out);
    return hipGetLastError();
}

hipError_t launch_image_quantize8(long long N, int C, int H, int W, const float* image, uint8_t* out,
                                  hipStream_t stream) {
    const size_t HW = (size_t)H * W, total = (size_t)N * C * HW;
    const size_t blocks = (total + 1023) / 1024;  // 256 lanes x 4 bytes
    hipLaunchKernelGGL(image_quantize8_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, image, out, C, HW,
                       total);
    return hipGetLastError();
}

}  // namespace gsr
