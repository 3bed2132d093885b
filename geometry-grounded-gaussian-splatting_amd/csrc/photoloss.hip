// photoloss.hip — the photometric term of the training loss on gfx950, fused: the ground-truth
// composite over the background outside the segmentation mask (train.py:159-166), the L1 of the
// rendered image after the per-view appearance transform (utils/loss_utils.py:90-123) and the D-SSIM of
// the raw rendered image against the composite (train.py:189), with their gradients.
//
//   g_c  = mask > 0.5 ? gt_c : bg_c            (strict: 0.5 is outside; no mask: gt_c)
//   t_c  = x_c                                 NO
//          E[c,3] + sum_k E[c,k] x_k           GS    (E [3,4])
//          e[1] + exp(e[0]) x_c                PGSR  (e [2])
//          gain_c[p] x_c inside the crop       GAIN  (the kernel half of GOF; the L1 over the crop only)
//   l1   = mean |t - g|,  ssim = the "valid" mean SSIM of x against g (ssim.hip's arithmetic),
//   out  = {(1 - lambda) l1 + lambda (1 - ssim), l1, ssim}
//
// Forward: the tiling of ssim_fwd_kernel (one 256-lane workgroup per 32 x 16 tile of one channel, both
// images staged in LDS with the composite applied while staging), every pixel also adding |t - g| and,
// when training, its terms of the embedding gradient; one partial row per workgroup, summed by a
// one-workgroup kernel in a fixed order in double (deterministic, no float atomics).
// Backward: one launch.  Nothing is kept for the L1 half: sign(t - g) (0 at equality) is recomputed from
// x, gt, mask and the embedding; the embedding gradient is the forward's sums times a scalar.
// The L1-only instances (SSIM = false) skip the stencil and keep the tiling, so their l1 is the full
// call's bit for bit.
#include "gsr_kernels.h"

namespace gsr {

// the window and tile of ssim.hip (which stays as it is: the same definitions, restated)
constexpr int kPhR = 5;
constexpr int kPhTW = 32, kPhTH = 16;
constexpr int kPhIW = kPhTW + 2 * kPhR, kPhIH = kPhTH + 2 * kPhR;
constexpr float kPhC1 = 0.01f * 0.01f, kPhC2 = 0.03f * 0.03f;
constexpr int kPhRow = 6;  // per-workgroup partials: ssim, l1, four embedding sums

struct SsimWindow {
    float w[2 * kPhR + 1];
};
SsimWindow ssim_window();  // ssim.hip

__device__ __forceinline__ float photo_x(const float* plane, int H, int W, int y, int x) {
    return (y >= 0 && y < H && x >= 0 && x < W) ? plane[(size_t)y * W + x] : 0.f;
}

// the composited ground truth of one channel, zero outside the image
__device__ __forceinline__ float photo_g(const float* gt, const float* mask, float bg, int H, int W, int y, int x) {
    if (!(y >= 0 && y < H && x >= 0 && x < W)) return 0.f;
    const size_t o = (size_t)y * W + x;
    if (mask && !(mask[o] > 0.5f)) return bg;
    return gt[o];
}

__device__ __forceinline__ float photo_sign(float d) { return (float)(d > 0.f) - (float)(d < 0.f); }

__device__ __forceinline__ bool photo_in_crop(const PhotoLossParams& q, int y, int x) {
    return y >= q.top && y < q.top + q.Hc && x >= q.left && x < q.left + q.Wc;
}

template <bool SSIM>
__global__ void __launch_bounds__(256)
    photo_fwd_kernel(PhotoLossParams q, SsimWindow win, float* __restrict__ out_gt, float* __restrict__ fA,
                     float* __restrict__ fB, float* __restrict__ fC, int want_emb, float* __restrict__ partial) {
    __shared__ float s_x[SSIM ? kPhIH : 1][SSIM ? kPhIW : 1], s_y[SSIM ? kPhIH : 1][SSIM ? kPhIW : 1];
    __shared__ float s_h[SSIM ? 5 : 1][SSIM ? kPhIH : 1][SSIM ? kPhTW : 1];
    __shared__ float s_red[kPhRow][4];
    const int tid = threadIdx.x;
    const int H = q.H, W = q.W;
    const int x0 = blockIdx.x * kPhTW, y0 = blockIdx.y * kPhTH;
    const int ch = blockIdx.z;
    const size_t HW = (size_t)H * W;
    const size_t plane = (size_t)ch * HW;
    const float* X = q.img + plane;
    const float* Y = q.gt + plane;
    const float bg = q.bg ? q.bg[ch] : 0.f;
    if (SSIM) {
        for (int k = tid; k < kPhIH * kPhIW; k += 256) {
            const int r = k / kPhIW, c = k - r * kPhIW;
            s_x[r][c] = photo_x(X, H, W, y0 + r - kPhR, x0 + c - kPhR);
            s_y[r][c] = photo_g(Y, q.mask, bg, H, W, y0 + r - kPhR, x0 + c - kPhR);
        }
        __syncthreads();
        // horizontal pass: 26 staged rows x 32 output columns, five moments
        for (int k = tid; k < kPhIH * kPhTW; k += 256) {
            const int r = k / kPhTW, c = k - r * kPhTW;
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 2 * kPhR + 1; t++) {
                const float a = s_x[r][c + t], b = s_y[r][c + t], w = win.w[t];
                m[0] += w * a;
                m[1] += w * b;
                m[2] += w * (a * a);
                m[3] += w * (b * b);
                m[4] += w * (a * b);
            }
#pragma unroll
            for (int j = 0; j < 5; j++) s_h[j][r][c] = m[j];
        }
        __syncthreads();
    }
    float E[4] = {0.f, 0.f, 0.f, 0.f};  // GS: row ch of the exposure; PGSR: {exp(e0), e1}
    if (q.mode == kAppGS) {
#pragma unroll
        for (int k = 0; k < 4; k++) E[k] = q.emb[ch * 4 + k];
    } else if (q.mode == kAppPGSR) {
        E[0] = expf(q.emb[0]);
        E[1] = q.emb[1];
    }
    // vertical pass: lane -> column (tid % 32), rows tid / 32 and + 8
    float sum = 0.f, l1 = 0.f, es[4] = {0.f, 0.f, 0.f, 0.f};
    const int c = tid & (kPhTW - 1);
#pragma unroll
    for (int rr = 0; rr < 2; rr++) {
        const int r = (tid >> 5) + 8 * rr;
        const int y = y0 + r, x = x0 + c;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (SSIM) {
#pragma unroll
            for (int t = 0; t < 2 * kPhR + 1; t++) {
                const float w = win.w[t];
#pragma unroll
                for (int j = 0; j < 5; j++) m[j] += w * s_h[j][r + t][c];
            }
        }
        if (y >= H || x >= W) continue;
        const size_t pix = (size_t)y * W + x;
        const size_t o = plane + pix;
        if (SSIM) {
            const float mu1 = m[0], mu2 = m[1];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu12;
            const float num1 = 2.f * mu12 + kPhC1, num2 = 2.f * s12 + kPhC2;
            const float den1 = mu1_sq + mu2_sq + kPhC1, den2 = s1 + s2 + kPhC2;
            const float S = (num1 * num2) / (den1 * den2);
            const bool counted = y >= kPhR && y < H - kPhR && x >= kPhR && x < W - kPhR;
            if (counted) sum += S;
            if (fA) {
                const float inv = 1.f / (den1 * den2);
                const float dS_dmu1 = (2.f * mu2 * num2) * inv - S * (2.f * mu1) / den1;
                const float dS_ds1 = -S / den2;
                const float dS_ds12 = 2.f * num1 * inv;
                fA[o] = counted ? dS_dmu1 - 2.f * mu1 * dS_ds1 - mu2 * dS_ds12 : 0.f;
                fB[o] = counted ? dS_ds1 : 0.f;
                fC[o] = counted ? dS_ds12 : 0.f;
            }
        }
        const float xv = SSIM ? s_x[r + kPhR][c + kPhR] : X[pix];
        const float gv = SSIM ? s_y[r + kPhR][c + kPhR] : photo_g(Y, q.mask, bg, H, W, y, x);
        if (out_gt) out_gt[o] = gv;
        float t = xv, sg;
        if (q.mode == kAppGS) {
            const float a0 = q.img[pix], a1 = q.img[HW + pix], a2 = q.img[2 * HW + pix];
            t = E[3] + (E[0] * a0 + E[1] * a1 + E[2] * a2);
            const float d = t - gv;
            l1 += fabsf(d);
            sg = photo_sign(d);
            es[0] += sg * a0;
            es[1] += sg * a1;
            es[2] += sg * a2;
            es[3] += sg;
        } else if (q.mode == kAppPGSR) {
            const float ax = E[0] * xv;
            const float d = (E[1] + ax) - gv;
            l1 += fabsf(d);
            sg = photo_sign(d);
            es[0] += sg * ax;
            es[1] += sg;
        } else if (q.mode == kAppGain) {
            if (photo_in_crop(q, y, x)) {
                const float gn = q.gain[((size_t)ch * q.Hc + (y - q.top)) * q.Wc + (x - q.left)];
                l1 += fabsf(gn * xv - gv);
            }
        } else {
            l1 += fabsf(t - gv);
        }
    }
    const int nq = 2 + (want_emb ? (q.mode == kAppGS ? 4 : q.mode == kAppPGSR ? 2 : 0) : 0);
    sum = wave_sum(sum);
    l1 = wave_sum(l1);
    if ((tid & 63) == 0) {
        s_red[0][tid >> 6] = sum;
        s_red[1][tid >> 6] = l1;
    }
    if (nq > 2) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float v = wave_sum(es[k]);
            if ((tid & 63) == 0) s_red[2 + k][tid >> 6] = v;
        }
    }
    __syncthreads();
    if (tid < nq) {
        const size_t nblk = (size_t)gridDim.x * gridDim.y * gridDim.z;
        const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[(size_t)tid * nblk + b] = (s_red[tid][0] + s_red[tid][1]) + (s_red[tid][2] + s_red[tid][3]);
    }
}

// fixed-order sum of n floats by the 1024-lane workgroup (ssim_reduce_kernel's order); the total on thread 0
__device__ __forceinline__ double photo_block_sum(const float* __restrict__ p, int n, double* s) {
    double acc = 0.0;
    for (int k = threadIdx.x; k < n; k += 1024) acc += (double)p[k];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    acc = wave_sum(acc);
    __syncthreads();  // (the previous total has been read)
    if (lane == 0) s[wave] = acc;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < 16; w++) t += s[w];
    return t;
}

// out = {rgb_loss, l1, ssim}; emb_sums: GS 12 (row c from the workgroups of channel c), PGSR 2
__global__ void __launch_bounds__(1024)
    photo_reduce_kernel(const float* __restrict__ partial, int nblk, int mode, int with_ssim, int want_emb,
                        double count_ssim, double count_l1, float lambda, float one_minus_lambda,
                        float* __restrict__ out, float* __restrict__ emb_sums) {
    __shared__ double s[16];
    const double ts = with_ssim ? photo_block_sum(partial, nblk, s) : 0.0;
    const double tl = photo_block_sum(partial + nblk, nblk, s);
    if (threadIdx.x == 0) {
        const float ssim = with_ssim ? (float)(ts / count_ssim) : 0.f;
        const float l1 = (float)(tl / count_l1);
        out[0] = with_ssim ? one_minus_lambda * l1 + lambda * (1.f - ssim) : l1;
        out[1] = l1;
        out[2] = ssim;
    }
    if (!want_emb) return;
    if (mode == kAppGS) {
        const int per = nblk / 3;
        for (int cc = 0; cc < 3; cc++)
            for (int k = 0; k < 4; k++) {
                const double t = photo_block_sum(partial + (size_t)(2 + k) * nblk + (size_t)cc * per, per, s);
                if (threadIdx.x == 0) emb_sums[cc * 4 + k] = (float)t;
            }
    } else if (mode == kAppPGSR) {
        for (int k = 0; k < 2; k++) {
            const double t = photo_block_sum(partial + (size_t)(2 + k) * nblk, nblk, s);
            if (threadIdx.x == 0) emb_sums[k] = (float)t;
        }
    }
}

template <bool SSIM>
__global__ void __launch_bounds__(256)
    photo_bwd_kernel(PhotoLossParams q, SsimWindow win, const float* __restrict__ fA, const float* __restrict__ fB,
                     const float* __restrict__ fC, const float* __restrict__ dL_dloss, double inv_count_ssim,
                     double inv_count_l1, float lambda, float one_minus_lambda, const float* __restrict__ emb_sums,
                     float* __restrict__ dL_dimg, float* __restrict__ dL_demb, float* __restrict__ dL_dgain) {
    __shared__ float s_f[SSIM ? 3 : 1][SSIM ? kPhIH : 1][SSIM ? kPhIW : 1];
    __shared__ float s_h[SSIM ? 3 : 1][SSIM ? kPhIH : 1][SSIM ? kPhTW : 1];
    const int tid = threadIdx.x;
    const int H = q.H, W = q.W;
    const int x0 = blockIdx.x * kPhTW, y0 = blockIdx.y * kPhTH;
    const int ch = blockIdx.z;
    const size_t HW = (size_t)H * W;
    const size_t plane = (size_t)ch * HW;
    if (SSIM) {
        for (int k = tid; k < kPhIH * kPhIW; k += 256) {
            const int r = k / kPhIW, c = k - r * kPhIW;
            const int y = y0 + r - kPhR, x = x0 + c - kPhR;
            s_f[0][r][c] = photo_x(fA + plane, H, W, y, x);
            s_f[1][r][c] = photo_x(fB + plane, H, W, y, x);
            s_f[2][r][c] = photo_x(fC + plane, H, W, y, x);
        }
        __syncthreads();
        for (int k = tid; k < kPhIH * kPhTW; k += 256) {
            const int r = k / kPhTW, c = k - r * kPhTW;
            float m[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 2 * kPhR + 1; t++) {
                const float w = win.w[t];
#pragma unroll
                for (int j = 0; j < 3; j++) m[j] = fmaf(w, s_f[j][r][c + t], m[j]);
            }
#pragma unroll
            for (int j = 0; j < 3; j++) s_h[j][r][c] = m[j];
        }
        __syncthreads();
    }
    const float up = dL_dloss[0];
    const float s = SSIM ? (float)((double)(-lambda * up) * inv_count_ssim) : 0.f;
    const float l1k = (float)((double)((SSIM ? one_minus_lambda : 1.f) * up) * inv_count_l1);
    // dL/d embedding: the forward's sums times the scalar
    if (dL_demb && blockIdx.x == 0 && blockIdx.y == 0 && ch == 0) {
        const int n = q.mode == kAppGS ? 12 : q.mode == kAppPGSR ? 2 : 0;
        if (tid < n) dL_demb[tid] = l1k * emb_sums[tid];
    }
    const float pa = q.mode == kAppPGSR ? expf(q.emb[0]) : 1.f;
    const float pb = q.mode == kAppPGSR ? q.emb[1] : 0.f;
    const int c = tid & (kPhTW - 1);
#pragma unroll
    for (int rr = 0; rr < 2; rr++) {
        const int r = (tid >> 5) + 8 * rr;
        const int y = y0 + r, x = x0 + c;
        float m[3] = {0.f, 0.f, 0.f};
        if (SSIM) {
#pragma unroll
            // The roundings of ssim_bwd_kernel as it is compiled, spelt out, so that the SSIM half of this gradient
            // is that kernel's bit for bit: its column sums of A and C are fused multiply-add chains, that of B
            // (packed by the vectoriser) adds rounded products in tap order; then (2x) B + A, + g C, times s.
            for (int t = 0; t < 2 * kPhR + 1; t++) {
                const float w = win.w[t];
                m[0] = fmaf(w, s_h[0][r + t][c], m[0]);
                m[2] = fmaf(w, s_h[2][r + t][c], m[2]);
                {
#pragma clang fp contract(off)
                    const float p = w * s_h[1][r + t][c];
                    m[1] = m[1] + p;
                }
            }
        }
        if (y >= H || x >= W) continue;
        const size_t pix = (size_t)y * W + x;
        const size_t o = plane + pix;
        const float xv = q.img[o];
        const float gv = photo_g(q.gt + plane, q.mask, q.bg ? q.bg[ch] : 0.f, H, W, y, x);
        float sp = 0.f;
        if (SSIM) sp = s * fmaf(m[2], gv, fmaf(m[1], xv + xv, m[0]));
        float v;  // sum_c' sign_c' dt_c'/dx_ch
        if (q.mode == kAppGS) {
            const float a0 = q.img[pix], a1 = q.img[HW + pix], a2 = q.img[2 * HW + pix];
            v = 0.f;
#pragma unroll
            for (int cc = 0; cc < 3; cc++) {
                const float* Er = q.emb + cc * 4;
                const float t = Er[3] + (Er[0] * a0 + Er[1] * a1 + Er[2] * a2);
                const float gc = photo_g(q.gt + (size_t)cc * HW, q.mask, q.bg ? q.bg[cc] : 0.f, H, W, y, x);
                v += photo_sign(t - gc) * Er[ch];
            }
        } else if (q.mode == kAppPGSR) {
            v = photo_sign((pb + pa * xv) - gv) * pa;
        } else if (q.mode == kAppGain) {
            v = 0.f;
            if (photo_in_crop(q, y, x)) {
                const size_t go = ((size_t)ch * q.Hc + (y - q.top)) * q.Wc + (x - q.left);
                const float gn = q.gain[go];
                const float sg = photo_sign(gn * xv - gv);
                v = sg * gn;
                if (dL_dgain) dL_dgain[go] = l1k * (sg * xv);
            }
        } else {
            v = photo_sign(xv - gv);
        }
        dL_dimg[o] = sp + l1k * v;
    }
}

size_t photo_loss_partials(int H, int W) {
    return (size_t)kPhRow * 3 * ((H + kPhTH - 1) / kPhTH) * ((W + kPhTW - 1) / kPhTW);
}

static double photo_count_l1(const PhotoLossParams& q) {
    return q.mode == kAppGain ? 3.0 * q.Hc * q.Wc : 3.0 * q.H * q.W;
}

hipError_t launch_photo_loss_fwd(const PhotoLossParams& q, float* out_gt, float* fA, float* fB, float* fC,
                                 float* partial, float* out3, float* emb_sums, hipStream_t stream) {
    const dim3 grid((q.W + kPhTW - 1) / kPhTW, (q.H + kPhTH - 1) / kPhTH, 3);
    const int want_emb = emb_sums != nullptr;
    if (q.ssim)
        hipLaunchKernelGGL(photo_fwd_kernel<true>, grid, dim3(256), 0, stream, q, ssim_window(), out_gt, fA, fB, fC,
                           want_emb, partial);
    else
        hipLaunchKernelGGL(photo_fwd_kernel<false>, grid, dim3(256), 0, stream, q, ssim_window(), out_gt, nullptr,
                           nullptr, nullptr, want_emb, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const double count = q.ssim ? 3.0 * (q.H - 2 * kPhR) * (q.W - 2 * kPhR) : 1.0;
    hipLaunchKernelGGL(photo_reduce_kernel, dim3(1), dim3(1024), 0, stream, partial,
                       (int)(grid.x * grid.y * grid.z), q.mode, q.ssim, want_emb, count, photo_count_l1(q), q.lambda,
                       (float)(1.0 - (double)q.lambda), out3, emb_sums);
    return hipGetLastError();
}

hipError_t launch_photo_loss_bwd(const PhotoLossParams& q, const float* fA, const float* fB, const float* fC,
                                 const float* emb_sums, const float* dL_dloss, float* dL_dimg, float* dL_demb,
                                 float* dL_dgain, hipStream_t stream) {
    const dim3 grid((q.W + kPhTW - 1) / kPhTW, (q.H + kPhTH - 1) / kPhTH, 3);
    const double count = q.ssim ? 3.0 * (q.H - 2 * kPhR) * (q.W - 2 * kPhR) : 1.0;
    const float oml = (float)(1.0 - (double)q.lambda);
    if (q.ssim)
        hipLaunchKernelGGL(photo_bwd_kernel<true>, grid, dim3(256), 0, stream, q, ssim_window(), fA, fB, fC, dL_dloss,
                           1.0 / count, 1.0 / photo_count_l1(q), q.lambda, oml, emb_sums, dL_dimg, dL_demb, dL_dgain);
    else
        hipLaunchKernelGGL(photo_bwd_kernel<false>, grid, dim3(256), 0, stream, q, ssim_window(), nullptr, nullptr,
                           nullptr, dL_dloss, 1.0, 1.0 / photo_count_l1(q), q.lambda, oml, emb_sums, dL_dimg, dL_demb,
                           dL_dgain);
    return hipGetLastError();
}

}  // namespace gsr
